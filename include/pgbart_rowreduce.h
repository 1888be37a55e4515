/*
 * pgbart_rowreduce.h -- the numeric contract of the per-draw averages over rows: weighted group means of (a transform
 * of) the posterior predictions, contrasts of two prediction matrices, and the per-draw goodness of fit against
 * observations -- one value per (draw, output, group) of a [D][K][n] matrix of predictions (pgb_row_reduce and
 * pgb_row_reduce_finish, below; pymc_bart_amd/average.py).  pgbart_rowsummary.h reduces over the draws, per row; this
 * header goes the other way.
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /,
 * comparisons, integer operations, pgb_exp_t and pgb_lphi_t only, and the ORDER OF EVERY SUM is part of the
 * definition, so that a host evaluation (pgb_rowred_block, pgb_rowred_finish, pgb_rowred_call) checks the device
 * kernels bit for bit and a result depends neither on the launch geometry nor on how the rows are cut into blocks.
 *
 * One call: predictions a[d][k][i] (and, for a contrast, b[d][k][i]), d < D draws, k < K outputs, i < n rows; per row a
 * weight w_i >= 0 and a group g_i in [0, G); optional y_i (K == 1 only), offsets off_a[k][i], off_b[k][i] and centres
 * c[k][g] (without them: 0.0).
 *
 *   value      v = T(a + off_a), and with b:  v = T(a + off_a) - T(b + off_b)  (one more rounding).  T and the
 *              addition of an offset are pgb_rowsum_value's with the PGB_ROWSUM_* transform codes
 *              (pgbart_rowsummary.h): without an offset nothing is added.
 *   terms      u = v - c[k][g_i] (one rounding; c = 0.0 subtracts 0.0) and, with y, r = y_i - v (one rounding):
 *                S1 term  w * u          E1 term  w * r           (two roundings each: u | r, the product)
 *                S2 term  w * (u * u)    E2 term  w * (r * r)     (three roundings each: u | r, the square, the product)
 *                W  term  w                                        (none; per group only, not per draw and output)
 *   sums       LANE SUMS (the convention of pgbart_rowsummary.h and pgbart_psis.h, carried over to the rows): every
 *              sum of a (d, k, g) has PGB_ROWRED_LANES = 64 partials; partial l adds, starting from 0.0 and in
 *              ascending row order, the terms of the rows of group g whose index i in the whole of X has
 *              i mod 64 == l; the partials are then added in the order l = 0 .. 63 onto 0.0 (pgb_rowsum_lanes).
 *              A block of rows starts at a multiple of 64, so carrying the partials from block to block (the
 *              workspace below) gives the same bits for every blocking, by construction.
 *   non-finite a term whose v is an infinity or a NaN (exp overflow, inf - inf) is counted in the integer
 *              n_nonfinite -- one count per (d, k, i), order-independent -- and is STILL ADDED.  (A row of weight 0
 *              and infinite v adds 0 * inf = NaN.)
 *   bad group  a row whose g_i is outside [0, G) adds nothing to any sum or to n_nonfinite; it is counted once in
 *              n_bad_group, and pgb_row_reduce_finish refuses a workspace whose count is not 0.
 *   finish     per (d, k, g), with W the group's weight:  m1 = S1 / W;  mean = c + m1;
 *              var_fit = S2 / W - m1 * m1, and 0.0 where that is < 0.0;  with y:  bias = E1 / W;  mse = E2 / W;
 *              var_res = mse - bias * bias, and 0.0 where that is < 0.0;  r2 = var_fit / (var_fit + var_res).
 *              A NaN is not < 0.0 and stays; r2 of 0 / 0 (a constant fit that equals y) stays NaN; a group of weight
 *              0 gives NaN or an infinity everywhere (the Python layer refuses such a group).  No square root here
 *              (rmse = sqrt(mse) is the caller's).  Multiplying every weight by a power of two scales every term and
 *              every sum exactly, so no bit of mean, var_fit, bias, mse, var_res or r2 changes.
 *   workspace  doubles: part[D][K][G][ns][64] (ns = 2: S1, S2; with y 4: S1, S2, E1, E2), then wpart[G][64], then two
 *              64-bit integer counters (n_nonfinite, n_bad_group): pgb_rowred_ws_doubles words of 8 bytes.
 *   output     out[PGB_ROWRED_NOUT][D][K][G]: mean, var_fit [, bias, mse, var_res, r2];  w_out[G].
 */
#ifndef PGBART_ROWREDUCE_H
#define PGBART_ROWREDUCE_H

#include "pgbart_rowsummary.h"

#define PGB_ROWRED_LANES 64
#define PGB_ROWRED_MAX_GROUPS 4096 /* G above it is refused: the workspace grows with D K G */
#define PGB_ROWRED_NSUMS(has_y) ((has_y) ? 4 : 2)
#define PGB_ROWRED_NOUT(has_y) ((has_y) ? 6 : 2)

/* v of one (d, k, i) */
PGB_HD double pgb_rowred_value(double a, int has_oa, double oa, int has_b, double b, int has_ob, double ob, int transform,
                               const pgb_lltabs* tb) {
  const double va = pgb_rowsum_value(a, has_oa, oa, transform, tb);
  if (!has_b) return va;
  return va - pgb_rowsum_value(b, has_ob, ob, transform, tb);
}
/* an infinity or a NaN: all exponent bits set */
PGB_HD int pgb_rowred_nonfinite(double v) { return ((pgb_d2u(v) >> 52) & 0x7FFull) == 0x7FFull; }
/* the terms of S1 | E1 and of S2 | E2 from the weight and u | r */
PGB_HD double pgb_rowred_term1(double w, double u) { return w * u; }
PGB_HD double pgb_rowred_term2(double w, double u) { return w * (u * u); }

/* the workspace: its size in 8-byte words, and where its parts begin */
PGB_HD int64_t pgb_rowred_part(int K, int G, int ns, int d, int k, int g) {
  return ((((int64_t)d * K + k) * G + g) * ns) * PGB_ROWRED_LANES;
}
PGB_HD int64_t pgb_rowred_wpart(int D, int K, int G, int ns) { return pgb_rowred_part(K, G, ns, D, 0, 0); }
PGB_HD int64_t pgb_rowred_counters(int D, int K, int G, int ns) {
  return pgb_rowred_wpart(D, K, G, ns) + (int64_t)G * PGB_ROWRED_LANES;
}
PGB_HD int64_t pgb_rowred_ws_doubles(int D, int K, int G, int has_y) {
  return pgb_rowred_counters(D, K, G, PGB_ROWRED_NSUMS(has_y)) + 2;
}

/* One block of nb rows whose first row has the index first_row (a multiple of 64) in the whole of X, evaluated
 * sequentially -- what the device kernel computes.  a, b (NULL: no contrast), v_out (NULL, or where v is written; it may
 * be a itself): element (d, k, i) at [(d K + k) ld + i].  off_a, off_b: [K][nb] or NULL; y: [nb] or NULL; centre:
 * [K][G] or NULL.  init != 0 starts every partial and both counters from 0; otherwise they continue from ws. */
PGB_HD void pgb_rowred_block(const double* a, const double* b, int D, int K, int64_t nb, int64_t ld, const double* w,
                             const int32_t* g, const double* y, const double* off_a, const double* off_b,
                             const double* centre, int G, int transform, int64_t first_row, int init, const pgb_lltabs* tb,
                             double* ws, double* v_out) {
  const int ns = PGB_ROWRED_NSUMS(y != 0);
  const int64_t n_words = pgb_rowred_ws_doubles(D, K, G, y != 0);
  uint64_t* cnt = (uint64_t*)(ws + pgb_rowred_counters(D, K, G, ns));
  if (init) {
    for (int64_t j = 0; j < n_words - 2; ++j) ws[j] = 0.0;
    cnt[0] = 0;
    cnt[1] = 0;
  }
  double* wpart = ws + pgb_rowred_wpart(D, K, G, ns);
  for (int64_t i = 0; i < nb; ++i) {
    const int l = (int)((first_row + i) % PGB_ROWRED_LANES);
    if (g[i] < 0 || g[i] >= G) {
      cnt[1] += 1;
      continue;
    }
    wpart[(int64_t)g[i] * PGB_ROWRED_LANES + l] = wpart[(int64_t)g[i] * PGB_ROWRED_LANES + l] + w[i];
  }
  for (int d = 0; d < D; ++d)
    for (int k = 0; k < K; ++k) {
      const int64_t row = ((int64_t)d * K + k) * ld;
      for (int64_t i = 0; i < nb; ++i) {
        const int l = (int)((first_row + i) % PGB_ROWRED_LANES);
        const double v = pgb_rowred_value(a[row + i], off_a != 0, off_a ? off_a[(int64_t)k * nb + i] : 0.0, b != 0,
                                          b ? b[row + i] : 0.0, off_b != 0, off_b ? off_b[(int64_t)k * nb + i] : 0.0,
                                          transform, tb);
        if (v_out) v_out[row + i] = v;
        if (g[i] < 0 || g[i] >= G) continue;
        if (pgb_rowred_nonfinite(v)) cnt[0] += 1;
        double* p = ws + pgb_rowred_part(K, G, ns, d, k, g[i]) + l;
        const double u = v - (centre ? centre[(int64_t)k * G + g[i]] : 0.0);
        p[0] = p[0] + pgb_rowred_term1(w[i], u);
        p[PGB_ROWRED_LANES] = p[PGB_ROWRED_LANES] + pgb_rowred_term2(w[i], u);
        if (y) {
          const double r = y[i] - v;
          p[2 * PGB_ROWRED_LANES] = p[2 * PGB_ROWRED_LANES] + pgb_rowred_term1(w[i], r);
          p[3 * PGB_ROWRED_LANES] = p[3 * PGB_ROWRED_LANES] + pgb_rowred_term2(w[i], r);
        }
      }
    }
}

/* The finish of one (d, k, g) from its ns finished sums s[ns] (S1, S2 [, E1, E2]), the group's weight W and its centre:
 * o[PGB_ROWRED_NOUT] = mean, var_fit [, bias, mse, var_res, r2] */
PGB_HD void pgb_rowred_finish_one(const double* s, int has_y, double W, double c, double* o) {
  const double m1 = s[0] / W;
  double var_fit = s[1] / W - m1 * m1;
  if (var_fit < 0.0) var_fit = 0.0;
  o[0] = c + m1;
  o[1] = var_fit;
  if (!has_y) return;
  const double bias = s[2] / W, mse = s[3] / W;
  double var_res = mse - bias * bias;
  if (var_res < 0.0) var_res = 0.0;
  o[2] = bias;
  o[3] = mse;
  o[4] = var_res;
  o[5] = var_fit / (var_fit + var_res);
}

/* The whole finish, sequentially: out[PGB_ROWRED_NOUT(has_y)][D][K][G], w_out[G], counts[2] = n_nonfinite, n_bad_group */
PGB_HD void pgb_rowred_finish(const double* ws, int D, int K, int G, int has_y, const double* centre, double* out,
                              double* w_out, int64_t* counts) {
  const int ns = PGB_ROWRED_NSUMS(has_y), n_out = PGB_ROWRED_NOUT(has_y);
  const int64_t n_items = (int64_t)D * K * G;
  const uint64_t* cnt = (const uint64_t*)(ws + pgb_rowred_counters(D, K, G, ns));
  counts[0] = (int64_t)cnt[0];
  counts[1] = (int64_t)cnt[1];
  for (int g = 0; g < G; ++g) w_out[g] = pgb_rowsum_lanes(ws + pgb_rowred_wpart(D, K, G, ns) + (int64_t)g * PGB_ROWRED_LANES);
  for (int d = 0; d < D; ++d)
    for (int k = 0; k < K; ++k)
      for (int g = 0; g < G; ++g) {
        double s[4], o[6];
        const double* p = ws + pgb_rowred_part(K, G, ns, d, k, g);
        for (int j = 0; j < ns; ++j) s[j] = pgb_rowsum_lanes(p + (int64_t)j * PGB_ROWRED_LANES);
        pgb_rowred_finish_one(s, has_y, w_out[g], centre ? centre[(int64_t)k * G + g] : 0.0, o);
        const int64_t item = ((int64_t)d * K + k) * G + g;
        for (int j = 0; j < n_out; ++j) out[(int64_t)j * n_items + item] = o[j];
      }
}

/* One whole call on n rows in one block (first row 0): the reference of pgb_row_reduce + pgb_row_reduce_finish.  The
 * caller provides ws[pgb_rowred_ws_doubles(D, K, G, y != NULL)]. */
PGB_HD void pgb_rowred_call(const double* a, const double* b, int D, int K, int64_t n, int64_t ld, const double* w,
                            const int32_t* g, const double* y, const double* off_a, const double* off_b,
                            const double* centre, int G, int transform, const pgb_lltabs* tb, double* ws, double* v_out,
                            double* out, double* w_out, int64_t* counts) {
  pgb_rowred_block(a, b, D, K, n, ld, w, g, y, off_a, off_b, centre, G, transform, 0, 1, tb, ws, v_out);
  pgb_rowred_finish(ws, D, K, G, y != 0, centre, out, w_out, counts);
}

#ifdef __cplusplus
extern "C" {
#endif
/* (HIP library only; not part of pgbart.h.)
 *
 * pgb_row_reduce_workspace_bytes: the bytes of the workspace of a call, 8 pgb_rowred_ws_doubles; 0 when D < 1, K < 1 or
 * G is outside [1, PGB_ROWRED_MAX_GROUPS].
 *
 * pgb_row_reduce: accumulates one block of nb rows of the device matrices a_dev and b_dev (NULL: no contrast), each
 * [D][K][nb] with the leading dimension ld >= nb between consecutive (d, k), into the device workspace ws_dev.  w_dev
 * [nb], g_dev [nb] (int32), y_dev [nb] or NULL, off_a_dev and off_b_dev [K][nb] or NULL, centre_dev [K][G] or NULL: all
 * on the device.  first_row: the index of the block's first row in the whole of X, a multiple of 64.  init != 0 starts
 * the partials from 0.0; otherwise the call continues from the stored ones (the same D, K, G, y or not, as the call that
 * started them).  v_out_dev: NULL, or where v is written with the same ld -- it may be a_dev itself -- for a following
 * pgb_row_summary.  Everything is validated before anything is launched (PGB_E_INVALID with a message: D < 1, K < 1,
 * nb < 1, ld < nb, first_row negative or not a multiple of 64, G outside [1, PGB_ROWRED_MAX_GROUPS], an unknown
 * transform, y with K > 1, off_b without b).  Returns when ws_dev (and v_out_dev) is written.
 *
 * pgb_row_reduce_finish: out_dev [PGB_ROWRED_NOUT(has_y)][D][K][G] and w_out_dev [G] on the device from the workspace;
 * counts_out (host memory): n_nonfinite and n_bad_group.  PGB_E_INVALID after writing them when n_bad_group != 0. */
int64_t pgb_row_reduce_workspace_bytes(int32_t D, int32_t K, int32_t G, int32_t has_y);
int pgb_row_reduce(const double* a_dev, const double* b_dev, int32_t D, int32_t K, int64_t nb, int64_t ld, const double* w_dev,
                   const int32_t* g_dev, const double* y_dev, const double* off_a_dev, const double* off_b_dev,
                   const double* centre_dev, int32_t G, int32_t transform, int64_t first_row, int32_t init, void* ws_dev,
                   double* v_out_dev, void* stream);
int pgb_row_reduce_finish(const void* ws_dev, int32_t D, int32_t K, int32_t G, int32_t has_y, const double* centre_dev,
                          double* out_dev, double* w_out_dev, int64_t* counts_out, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_ROWREDUCE_H */
