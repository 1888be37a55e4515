/*
 * pgbart_surv.h -- the numeric contract of DISCRETE-TIME SURVIVAL CURVES of stored posterior draws (Sparapani et al.
 * 2016): a Bernoulli forest fitted on person-period rows with time as a covariate predicts the hazard p_l of the l-th
 * grid time, and the survival curve of a row is S(t_j | x) = prod_{l <= j} (1 - p_l).  pgb_predict_arms
 * (pgbart_arms.h) writes the predictions of a grid of times on the time column -- a grid IS a set of arms on that
 * column -- and the step below turns them, in place, into survival probabilities, with the restricted mean survival
 * time and the times at which the curve reaches given levels, per (draw, row) (pgb_surv_curves;
 * pymc_bart_amd/survival.py).
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /, comparisons,
 * integer operations, pgb_exp_t and pgb_lphi_t only, and the ORDER OF EVERY OPERATION is part of the definition, so that
 * a host evaluation (pgb_surv_block) checks the device kernel bit for bit and a result depends neither on the launch
 * geometry, nor on how the rows are cut into blocks, nor on how the grid is cut into chunks.
 *
 * The state of one (draw d, row i):  (S, R, T[0 .. Q)),  0 <= Q <= PGB_SURV_MAX_LEVELS.  It starts (init != 0) at
 * S = 1.0, R = 0.0, T[l] = beyond.
 *
 * One call handles A consecutive grid times, 1 <= A <= PGB_ARMS_MAX: t[a], the widths dt[a] (finite, > 0), the levels
 * u[l] in (0, 1] and beyond, a finite double > t[A - 1].  Element (a, d, i) of the predictions is f[a lda + d ldd + i],
 * as in pgb_arm_decide.  For a = 0 .. A - 1, in this order (pgb_surv_step):
 *   R = R + S * dt[a]     the product is rounded, then the sum.  S is the one BEFORE this time's update: the curve is a
 *                         step function that equals S_{j-1} on [t_{j-1}, t_j).
 *   q = pgb_rowsum_value(-f, has_off, -off_i, transform, tb)
 *                         the link at the negated predictor -- Phi(-s) or 1 / (1 + e^s) with s = f + off_i: 1 - p
 *                         without the cancellation of 1 - Phi(s).  (-f) + (-off) is -(f + off) exactly.  transform is
 *                         PGB_ROWSUM_LOGISTIC or PGB_ROWSUM_PROBIT.  What pgb_rowsum_value does with a predictor that is
 *                         no finite number is its own, and kept: under the logistic link a NaN or an infinity gives a
 *                         NaN q; under the probit link the infinities give their limits 0.0 and 1.0, and the
 *                         predictor must not be a NaN -- pgb_lphi_t reads the clamp row of the NaN's sign bit, which
 *                         compilers do not agree on: q is 0.0 or 1.0 and nothing is counted.  A sum of finite leaves
 *                         and a finite offset is finite.
 *   S = S * q             one rounding; S replaces f at (a, d, i).
 *   T[l]                  for every l < Q: if T[l] == beyond and S <= u[l] then T[l] = t[a].  A NaN S compares false:
 *                         it reaches no level.
 *   n_nonfinite           a q with all exponent bits set (pgb_rowred_nonfinite) adds one to the 64-bit counter; the
 *                         step is executed all the same.  The counter is the caller's: no call clears it.
 * With init == 0 the state continues from the stored one, so a grid of J times may be cut into calls anywhere: the
 * operations and their order are those of one call.  R after the last time is the restricted mean survival time up to
 * t_{J-1}; T[l] == beyond says that level l is not reached on the grid.
 *
 *   state     doubles [2 + Q][D][nb]: the slabs S, R, T[0], .., T[Q - 1]; each is a [D][nb] matrix that pgb_row_summary
 *             and pgb_row_reduce take as it is (pgb_surv_state_at).
 */
#ifndef PGBART_SURV_H
#define PGBART_SURV_H

#include <stdint.h>

#include "pgbart_arms.h"

#define PGB_SURV_MAX_LEVELS 4
#define PGB_SURV_S 0
#define PGB_SURV_R 1
#define PGB_SURV_T(l) (2 + (l))

typedef struct {
  double S, R;
  double T[PGB_SURV_MAX_LEVELS]; /* (indexed by the unrolled loops below only: registers on the device) */
} pgb_surv_state;

typedef struct {
  double u[PGB_SURV_MAX_LEVELS];
} pgb_surv_levels;

/* where slab `slab` of the state keeps (d, i) */
PGB_HD int64_t pgb_surv_state_at(int D, int64_t nb, int slab, int d, int64_t i) {
  return ((int64_t)slab * D + d) * nb + i;
}

/* 1 - p of one prediction */
PGB_HD double pgb_surv_q(double f, int has_off, double off, int transform, const pgb_lltabs* tb) {
  return pgb_rowsum_value(-f, has_off, -off, transform, tb);
}

PGB_HD void pgb_surv_start(pgb_surv_state* st, double beyond) {
  st->S = 1.0;
  st->R = 0.0;
  for (int l = 0; l < PGB_SURV_MAX_LEVELS; ++l) st->T[l] = beyond;
}

/* One grid time of one (d, i): returns the new S (what replaces f) and whether q was an infinity or a NaN.  Slots
 * l >= Q of T and of lv are never read. */
PGB_HD double pgb_surv_step(pgb_surv_state* st, double f, int has_off, double off, int transform, const pgb_lltabs* tb,
                            double t, double dt, const pgb_surv_levels* lv, int Q, double beyond, int* nonfinite) {
  const double area = st->S * dt;
  st->R = st->R + area;
  const double q = pgb_surv_q(f, has_off, off, transform, tb);
  *nonfinite = pgb_rowred_nonfinite(q);
  const double S = st->S * q;
  st->S = S;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int l = 0; l < PGB_SURV_MAX_LEVELS; ++l)
    if (l < Q && st->T[l] == beyond && S <= lv->u[l]) st->T[l] = t;
  return S;
}

/* One call on a block of nb rows, evaluated sequentially -- what the device kernel computes.  f is overwritten in place;
 * off: [nb] or NULL; t, dt: [A]; u: [Q] (NULL with Q == 0); state: [2 + Q][D][nb]. */
PGB_HD void pgb_surv_block(double* f, int64_t lda, int64_t ldd, int D, int A, int64_t nb, const double* off, int transform,
                           const double* t, const double* dt, const double* u, int Q, double beyond, int init,
                           const pgb_lltabs* tb, double* state, uint64_t* n_nonfinite) {
  pgb_surv_levels lv;
  for (int l = 0; l < PGB_SURV_MAX_LEVELS; ++l) lv.u[l] = l < Q ? u[l] : 1.0;
  for (int d = 0; d < D; ++d)
    for (int64_t i = 0; i < nb; ++i) {
      pgb_surv_state st;
      pgb_surv_start(&st, beyond);
      if (!init) {
        st.S = state[pgb_surv_state_at(D, nb, PGB_SURV_S, d, i)];
        st.R = state[pgb_surv_state_at(D, nb, PGB_SURV_R, d, i)];
        for (int l = 0; l < Q; ++l) st.T[l] = state[pgb_surv_state_at(D, nb, PGB_SURV_T(l), d, i)];
      }
      double* fd = f + (int64_t)d * ldd + i;
      for (int a = 0; a < A; ++a) {
        int nonfinite;
        fd[(int64_t)a * lda] = pgb_surv_step(&st, fd[(int64_t)a * lda], off != 0, off ? off[i] : 0.0, transform, tb, t[a],
                                             dt[a], &lv, Q, beyond, &nonfinite);
        if (nonfinite) *n_nonfinite += 1;
      }
      state[pgb_surv_state_at(D, nb, PGB_SURV_S, d, i)] = st.S;
      state[pgb_surv_state_at(D, nb, PGB_SURV_R, d, i)] = st.R;
      for (int l = 0; l < Q; ++l) state[pgb_surv_state_at(D, nb, PGB_SURV_T(l), d, i)] = st.T[l];
    }
}

#ifdef __cplusplus
extern "C" {
#endif
/* (HIP library only, both particle builds; not part of pgbart.h.  Everything is validated before the launch; a refused
 * call writes nothing and PGB_E_INVALID names the argument.)
 *
 * pgb_surv_curves: A consecutive grid times of one block of nb rows.  f_dev: element (a, d, i) at [a lda + d ldd + i],
 * so that one output k of pgb_predict_arms' result is handed over without a copy (f_dev = out_dev + k nb, lda =
 * n_picks K nb, ldd = K nb); only those cells are overwritten, with S.  off_dev: [nb] on the device or NULL.  t_host,
 * dt_host: [A]; u_host: [Q] (NULL is legal with Q == 0): host memory.  init != 0 starts the state, otherwise the call
 * continues from state_dev [2 + Q][D][nb] (the same D, nb, Q, u and beyond).  n_nonfinite_dev: one 64-bit counter on the
 * device, added to and never cleared.  Refused: a null pointer; D, A or nb below 1; A > PGB_ARMS_MAX; Q outside
 * [0, PGB_SURV_MAX_LEVELS]; ldd < nb, lda < (D - 1) ldd + nb or strides that overflow the index arithmetic; a transform
 * other than PGB_ROWSUM_LOGISTIC and PGB_ROWSUM_PROBIT; a t or dt that is not finite, a dt <= 0, a t that is not
 * strictly increasing; a level outside (0, 1]; beyond not finite or <= t[A - 1].  Returns when f_dev and state_dev are
 * written.
 *
 * pgb_surv_kernel_ms: with PGB_WALK_TIMING=1 in the environment (read per call) pgb_surv_curves puts its kernel between
 * HIP events; this reports the last such measurement of the calling thread in milliseconds (-1.0: none yet).  For
 * tools/timing_survival.py. */
int pgb_surv_curves(double* f_dev, int64_t lda, int64_t ldd, int32_t D, int32_t A, int64_t nb, const double* off_dev,
                    int32_t transform, const double* t_host, const double* dt_host, const double* u_host, int32_t Q,
                    double beyond, int32_t init, double* state_dev, uint64_t* n_nonfinite_dev, void* stream);
int pgb_surv_kernel_ms(double* ms_out);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_SURV_H */
