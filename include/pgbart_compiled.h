/*
 * pgbart_compiled.h -- the "compiled" likelihood family: a per-row log-density written by the user as a
 * short C function body, compiled at run time into a k_loglik instance for gfx950 (a code object the HIP
 * library loads) and, for the CPU backends, into a host function with the pgb_loglik_fn signature.
 * A body may also take K = 2 .. PGB_MAX_OUTPUTS linear predictors (a sampler with n_outputs = K): the code
 * object is then the library's K-vector pass, k_loglik<K> (K <= 4) or k_loglik<0> (run-time K), with the body
 * at its evaluation sites.  A code object holds ONE pass kernel, for constant leaves or for linear leaves
 * (response linear / mix: k_loglik<1, ., true>, or the run-time-K linear path with K fixed at compile time);
 * its layout record says which, and the library takes the one that matches the sampler's response.  No CPU
 * backend runs a K-vector body or linear leaves (the callback family has one output and constant leaves): the
 * host build of such a body serves as a reference evaluator only.
 *
 * Kept apart from pgbart.h on purpose: pgbart.h is the ABI every backend (the CPU oracle included) exports in
 * full; the entry points below exist in the HIP library only.  A CPU backend runs the same body as family
 * PGB_FAMILY_CALLBACK with the host build installed as its callback (pymc_bart_amd/compiled.py).
 *
 * The body is the inside of
 *     double f(double y, double mu, double aux, const double <param 0>, ..., const double <param n-1>)
 * (at most PGB_COMPILED_MAX_PARAMS params).  Its vocabulary -- the only functions it may call -- is defined
 * ONCE here for both compiles (section "vocabulary"): the table functions of pgbart_spec.h (bit-identical on
 * the host and the device) and explicit comparisons, no libm.  Both compiles run with -ffp-contract=off.
 * The result goes through the contract's clamp ([-2047, 2047], NaN -> -2047) and the fixed-point sums of the
 * callback family: on a given backend the compiled family and the callback family are the same sampler.
 *
 * A likelihood may carry a second body, its SAMPLER BODY: the inside of
 *     double r(double mu, double aux, const double <param 0>, ..., const double <param n-1>)
 * (mu[0 .. K-1] for K outputs; no y), which returns one replicated observation.  It is compiled into a code object of
 * its own (mark 2: the kernel k_ppc_compiled of csrc/k_ppc_compiled.hip, launched by pgb_ppc_draw_compiled) and into a
 * host evaluator.  It calls the vocabulary above plus the RANDOM vocabulary (section "vocabulary" below), whose
 * numeric contract -- the samplers, the addressing of every call, the caps -- is include/pgbart_ppc.h.
 */
#ifndef PGBART_COMPILED_H
#define PGBART_COMPILED_H

#include <stdint.h>

#define PGB_FAMILY_COMPILED 11    /* y ~ a per-row log-density compiled at run time (this header) */
#define PGB_COMPILED_MAX_PARAMS 8
#define PGB_COMPILED_MAGIC 0x43424750 /* "PGBC" */
#define PGB_COMPILED_KERNEL "k_loglik_compiled"
#define PGB_COMPILED_PROBE "k_loglik_compiled_probe"
#define PGB_COMPILED_LAYOUT "pgb_compiled_layout_record"

/* The layout record every compiled code object carries (a __device__ global named PGB_COMPILED_LAYOUT): the
 * library compares it with its own values before the first launch and refuses a code object built for the
 * other particle build, from other kernel headers, for another number of outputs or for the other kind of leaves. */
typedef struct {
  int32_t magic;          /* PGB_COMPILED_MAGIC */
  int32_t max_particles;  /* PGB_MAX_PARTICLES */
  int32_t n_params;       /* params the body was compiled for */
  int32_t n_outputs;      /* the K of the body's mu (1: a scalar mu) */
  int64_t sizeof_dev, sizeof_job, sizeof_cmd, sizeof_ctrl, sizeof_acc;
  uint64_t headers_hash;  /* PGB_HEADERS_HASH: a hash of the kernel headers (pymc_bart_amd/compiled.py) */
  int32_t linear_leaves;  /* 0: the constant-leaf pass, 1: the linear-leaf pass (response linear / mix) */
  int32_t pointwise;      /* the object's MARK.  0: a sampler's pass kernel; 1: k_pointwise_compiled
                             (pgbart_pointwise.h), no pass kernel; 2: k_ppc_compiled, the SAMPLER BODY of the likelihood
                             (pgbart_ppc.h), no pass kernel, n_outputs is the K of the sampler body's mu */
} pgb_compiled_layout;
#define PGB_COMPILED_MARK_PASS 0
#define PGB_COMPILED_MARK_POINTWISE 1
#define PGB_COMPILED_MARK_SAMPLER 2
#define PGB_PPC_COMPILED_KERNEL "k_ppc_compiled"

/* The params of one launch, by value (they arrive in SGPRs with the kernel arguments). */
typedef struct {
  double v[PGB_COMPILED_MAX_PARAMS];
} pgb_compiled_params;

#if !defined(PGB_COMPILED_NO_ENTRY_POINTS)
#include "pgbart.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Load a compiled code object (hipModuleLoadData) for a sampler created with family PGB_FAMILY_COMPILED and
 * check its layout record.  PGB_E_INVALID for another family, bytes that are not a gfx950 code object, a code
 * object without the kernel or the record, or a record that does not match this library or the sampler
 * (outputs; constant against linear / mix leaves); the handle stays usable
 * (a refused image is never launched).  A new code object replaces the old one; pgb_destroy unloads it.
 * n_params: the params the body declares (pgb_set_likelihood then takes exactly that many). */
int pgb_set_loglik_code(pgb_handle* h, const void* code_object, int64_t bytes, int32_t n_params);
/* Optional per-row column `aux` (n doubles, device memory) the body reads as `aux`; NULL clears it (aux = 0.0).
 * Non-finite values are refused (PGB_E_INVALID) and the column is cleared. */
int pgb_set_loglik_aux(pgb_handle* h, const double* aux_dev);
/* Evaluate the loaded body, clamped like the sampler takes it ([-2047, 2047], NaN -> -2047), on n arbitrary rows:
 * out[i] = f(y[i], mu[0 .. K-1][i], aux ? aux[i] : 0.0, the params of pgb_set_likelihood).  All pointers are device
 * memory, mu is [K][n]; the call returns when out is written.  Runs the code object's kernel PGB_COMPILED_PROBE: the
 * device's values of a body, to hold against its host build. */
int pgb_compiled_probe(pgb_handle* h, const double* y, const double* mu, const double* aux, int64_t n, double* out);
#ifdef __cplusplus
}
#endif
#endif

/* ---- the functions behind the vocabulary (section "vocabulary" below); pgbart_logpdf.h uses pgb_cl_lgamma too */
#include "pgbart_spec.h"
/* fabs(-0.0) = +0.0, a NaN stays a NaN; fmin / fmax return the SECOND argument when the comparison fails (a NaN
 * in either) */
PGB_HD double pgb_cl_fabs(double x) { return x < 0.0 ? -x : x + 0.0; }
PGB_HD double pgb_cl_fmin(double a, double b) { return a < b ? a : b; }
PGB_HD double pgb_cl_fmax(double a, double b) { return a > b ? a : b; }
/* pgb_softplus_t on the two tables (the same operations) */
PGB_HD double pgb_cl_softplus(double t, const double* expt, const double* logt) {
  if (t > 36.0) return t;
  return pgb_log_t(1.0 + pgb_exp_t(t, expt), logt);
}
/* log Gamma(x): x < 10 moves up by the recurrence (log Gamma(x) = log Gamma(x + j) - log(x (x + 1) .. (x + j - 1)),
 * one logarithm of the product), then Stirling's series to the z^-11 term (truncation < 7e-16 at z >= 10).
 * |error| < 1e-13 max(1, |log Gamma(x)|) on [1e-6, 1e12].  x <= 0 or NaN -> NaN (the row takes the lower bound),
 * +inf -> +inf. */
PGB_HD double pgb_cl_lgamma(double x, const double* logt) {
  if (!(x > 0.0)) return pgb_u2d(0x7FF8000000000000ull);
  if (x > 1.7976931348623157e308) return x;
  double z = x, p = 1.0;
  while (z < 10.0) {
    p = p * z;
    z = z + 1.0;
  }
  const double r = 1.0 / z, r2 = r * r;
  double s = -1.9175269175269176e-03 * r2 + 8.4175084175084175e-04;  /* -691/360360, 1/1188 */
  s = s * r2 - 5.9523809523809524e-04;                                  /* -1/1680 */
  s = s * r2 + 7.9365079365079365e-04;                                  /*  1/1260 */
  s = s * r2 - 2.7777777777777778e-03;                                  /* -1/360  */
  s = s * r2 + 8.3333333333333333e-02;                                  /*  1/12   */
  const double lz = pgb_log_t(z, logt);
  double v = ((z - 0.5) * lz - z) + (9.1893853320467274e-01 + s * r);    /* + log sqrt(2 pi) */
  if (p != 1.0) v = v - pgb_log_t(p, logt);
  return v;
}

#endif /* PGBART_COMPILED_H */

/* ------------------------------------------------------------------ vocabulary
 * (outside the include guard: a unit that compiles a body includes this header again around it)
 * The prelude of every such unit, pgbart_compiled_body.h, defines right in front of the body:
 *   PGB_COMPILED_VOCABULARY                    then includes this header: the vocabulary is on
 *   PGB_CL_EXPT / PGB_CL_LOGT / PGB_CL_LPHI   the tables (those of the function's first argument)
 * and behind it PGB_COMPILED_VOCABULARY_END (and includes this header again): the names are released.
 * The functions are macros so that the same text serves C (host) and HIP (device):
 *   exp, log         pgb_exp_t, pgb_log_t             (pgbart_spec.h: table-driven, the same bits on both sides)
 *   log_ndtr         pgb_lphi_t                       (log Phi, the probit family's function)
 *   softplus         pgb_softplus_t                   (log(1 + e^x))
 *   fabs, fmin, fmax explicit comparisons             (no builtin: the same NaN / signed-zero behaviour)
 *   lgamma           pgb_cl_lgamma                    (log Gamma(x), x > 0: + - * / and pgb_log_t only)
 * A unit that compiles a SAMPLER BODY also defines PGB_COMPILED_SAMPLER_VOCABULARY, after it has included
 * pgbart_ppc.h, and has a `pgb_ppc_ctx* pgb_cl_rng` in scope around the body: the random vocabulary is on as well --
 *   uniform()        pgb_ppc_ctx_uniform       [0, 1)     uniform_open()   pgb_ppc_ctx_uniform_open   (0, 1)
 *   normal()         pgb_ppc_ctx_normal                   gamma(a)         pgb_ppc_ctx_gamma
 *   poisson(lam)     pgb_ppc_ctx_poisson
 *   sqrt(x)          pgb_psis_sqrt                        floor(x)         pgb_ppc_floor
 * -- with the addressing of repeated calls, the call cap and the flags as include/pgbart_ppc.h states them.  A
 * density body never sees these names: a param of a density-only likelihood may be called gamma. */
#if defined(PGB_COMPILED_VOCABULARY) && !defined(PGB_COMPILED_VOCABULARY_ON)
#define PGB_COMPILED_VOCABULARY_ON
#define exp(x) pgb_exp_t((double)(x), PGB_CL_EXPT)
#define log(x) pgb_log_t((double)(x), PGB_CL_LOGT)
#define log_ndtr(x) pgb_lphi_t((double)(x), PGB_CL_LPHI)
#define softplus(x) pgb_cl_softplus((double)(x), PGB_CL_EXPT, PGB_CL_LOGT)
#define fabs(x) pgb_cl_fabs((double)(x))
#define fmin(a, b) pgb_cl_fmin((double)(a), (double)(b))
#define fmax(a, b) pgb_cl_fmax((double)(a), (double)(b))
#define lgamma(x) pgb_cl_lgamma((double)(x), PGB_CL_LOGT)
#ifdef PGB_COMPILED_SAMPLER_VOCABULARY
#define uniform() pgb_ppc_ctx_uniform(pgb_cl_rng)
#define uniform_open() pgb_ppc_ctx_uniform_open(pgb_cl_rng)
#define normal() pgb_ppc_ctx_normal(pgb_cl_rng)
#define gamma(a) pgb_ppc_ctx_gamma(pgb_cl_rng, (double)(a))
#define poisson(lam) pgb_ppc_ctx_poisson(pgb_cl_rng, (double)(lam))
#define sqrt(x) pgb_psis_sqrt((double)(x), pgb_cl_rng->tb)
#define floor(x) pgb_ppc_floor((double)(x))
#endif
#endif
#if defined(PGB_COMPILED_VOCABULARY_END) && defined(PGB_COMPILED_VOCABULARY_ON)
#undef PGB_COMPILED_VOCABULARY_ON
#undef PGB_COMPILED_VOCABULARY
#undef PGB_COMPILED_VOCABULARY_END
#undef exp
#undef log
#undef log_ndtr
#undef softplus
#undef fabs
#undef fmin
#undef fmax
#undef lgamma
#ifdef PGB_COMPILED_SAMPLER_VOCABULARY
#undef PGB_COMPILED_SAMPLER_VOCABULARY
#undef uniform
#undef uniform_open
#undef normal
#undef gamma
#undef poisson
#undef sqrt
#undef floor
#endif
#endif
