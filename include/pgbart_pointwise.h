/*
 * pgbart_pointwise.h -- scoring a fit: the pointwise log-likelihood of posterior draws at given rows, and its
 * reduction over the draws (log pointwise predictive density, the WAIC terms), fused into the tree walk.
 *
 * Kept apart from pgbart.h like pgbart_compiled.h: pgbart.h is the ABI every backend (the CPU oracle included)
 * exports in full; the entry point below exists in the HIP library only (both particle builds).  The numeric
 * contract -- the densities, the clamp, the reduction -- is include/pgbart_logpdf.h.
 */
#ifndef PGBART_POINTWISE_H
#define PGBART_POINTWISE_H

#include <stdint.h>

#include "pgbart.h"

#define PGB_POINTWISE_KERNEL "k_pointwise_compiled"

typedef struct {
  int32_t family;             /* a built-in family of pgbart_spec.h, or PGB_FAMILY_COMPILED; the callback family is refused */
  int32_t n_params;           /* params per draw: the family's (pgb_logpdf_nparams), or the compiled body's */
  const double* params_host;  /* [n_forests][n_params], host memory (NULL when n_params = 0) */
  const double* y_dev;        /* [n_rows] observed values, finite */
  const double* offset_dev;   /* [K][n_rows] added to the predictors, |.| <= PGB_MAX_OFFSET, or NULL */
  const double* aux_dev;      /* [n_rows] the compiled body's aux column, finite, or NULL (aux = 0.0) */
  const void* code_object;    /* family compiled: a code object built with pointwise=True (pymc_bart_amd.compiled) ... */
  int64_t code_bytes;         /* ... and its size; NULL / 0 otherwise */
} pgb_pointwise_lik;

#ifdef __cplusplus
extern "C" {
#endif
/* loglik[d][i] = clamp(log p(y[i] | mu_d(X[i,:]) + offset[.][i], params[d])) for the forests d (rows of
 * forest_tree_idx, as pgb_predict takes them; no excluded variables) and the rows of X (device memory, row-major,
 * leading dimension ldx).  mu_d is exactly what pgb_predict computes for the same arguments.
 *   loglik_dev_out     [n_forests][n_rows], or NULL
 *   row_stats_dev_out  [3][n_rows] = (lppd_i, mean_i, var_i) over the forests (pgbart_logpdf.h: the reduction), or
 *                      NULL; with loglik_dev_out = NULL nothing of size n_forests x n_rows is written
 *   n_clamped_out      the number of (forest, row) pairs whose value met the clamp (host memory, may be NULL)
 * At least one of the two outputs must be given.  Everything is validated before a launch: PGB_E_INVALID for a
 * malformed history, an unknown or callback family, a wrong n_params, params outside the family's domain, a K the
 * family does not take, non-finite y / aux, an offset beyond PGB_MAX_OFFSET, or a code object that does not match
 * (not built with pointwise=True, other headers, another n_params or K).  The call returns when the outputs are
 * written.  PGB_PW_WGS (environment, read per call) overrides the number of workgroups aimed at, like PGB_PRED_WGS;
 * results do not depend on it. */
int pgb_pointwise_loglik(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                         const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx, const pgb_pointwise_lik* lik,
                         double* loglik_dev_out, double* row_stats_dev_out, int64_t* n_clamped_out, void* stream);

/* PSIS-LOO of the rows of such a matrix (the numeric contract is include/pgbart_psis.h: Pareto-smoothed importance
 * sampling of each row's values over the draws).  ll_dev is [D][ld] device memory as pgb_pointwise_loglik writes it
 * (finite values within [-2047, 2047]; the first n_rows of every ld are read), tail_len the number of largest
 * importance ratios that are smoothed, M = ceil(min(D / 5, 3 sqrt(D / r_eff))), computed by the caller.
 *   out_dev  [2][n_rows] = (elpd_loo_i, k_i); k_i = +inf where no generalised-Pareto fit was possible
 * Everything is validated before the launch: PGB_E_INVALID unless 2 <= D <= PGB_PSIS_MAX_DRAWS (16384),
 * 1 <= tail_len < D, tail_len <= PGB_PSIS_MAX_TAIL (448) and ld >= n_rows >= 1.  The call returns when the output is
 * written.  HIP library only (both particle builds). */
int pgb_psis_rows(const double* ll_dev, int32_t D, int64_t n_rows, int64_t ld, int32_t tail_len, double* out_dev,
                  void* stream);

/* PSIS-weighted expectations over the same weights (pgbart_psis.h: pgb_psis_row_expect): per row the self-normalised
 * sum of a functional of a second matrix g_dev [D][ldg] -- the draws' predictors or replicated observations of the
 * same rows (the first n_rows of every ldg are read) -- under the row's Pareto-smoothed weights, which never leave the
 * kernel.  ll_dev, D, n_rows, ld, tail_len: as pgb_psis_rows takes them.  ldg is separate from ld, so that output k of
 * pgb_predict's [D][K][nb] can be passed as g_dev + k * nb with ldg = K * nb.
 *   kind     PGB_PSIS_G_VALUE (0): E[g] and E[g^2] (n_e = 2);  PGB_PSIS_G_PIT (1): the mid-p LOO-PIT of y_dev
 *            [n_rows], E[(g < y) + 0.5 (g == y)] (n_e = 1).  y_dev is not read for kind 0 (may be NULL)
 *   out_dev  [2 + n_e][n_rows] = (elpd_loo_i, k_i, E_0[, E_1]); the first two are pgb_psis_rows' bits
 * g is held within +-1e150 (a NaN becomes -1e150).  Everything is validated before the launch: PGB_E_INVALID for what
 * pgb_psis_rows refuses, a NULL g_dev, ldg < n_rows, a kind other than 0 / 1, a NULL y_dev with kind 1.  The call
 * returns when the output is written.  HIP library only (both particle builds). */
int pgb_psis_expect(const double* ll_dev, int32_t D, int64_t n_rows, int64_t ld, int32_t tail_len, const double* g_dev,
                    int64_t ldg, const double* y_dev, int32_t kind, double* out_dev /* [2 + n_e][n_rows] */, void* stream);

/* a[d][k][i] = a[d][k][i] + offset[k][i] in place: pgb_predict's [D][K][n_rows] made the linear predictor that
 * pgb_pointwise_loglik and pgb_ppc_draw see (one rounding per element, so the host's mu + offset bit for bit).
 * PGB_E_INVALID for a NULL pointer or D, K, n_rows < 1.  HIP library only (both particle builds). */
int pgb_add_offset(double* a_dev, int32_t D, int32_t K, int64_t n_rows, const double* offset_dev, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_POINTWISE_H */
