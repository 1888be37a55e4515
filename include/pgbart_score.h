/*
 * pgbart_score.h -- the numeric contract of the scoring rules of the posterior predictive: what the CRPS, the
 * quantile (pinball) loss, the interval score, the coverage and the Dawid-Sebastiani score of one row are made of,
 * computed from one column of a [D][ld] matrix of replicated observations y_rep over its D draws and the row's
 * observed y (pgb_row_score, below; pymc_bart_amd/scores.py).
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /,
 * comparisons and integer operations only -- no libm, no table --, and the ORDER OF EVERY SUM is part of the
 * definition, so that a host evaluation (pgb_score_column) checks the device kernel bit for bit and a result never
 * depends on the launch geometry.  The order, the lane sums and the quantile are those of pgbart_rowsummary.h.
 *
 * One column: a[0 ld], a[1 ld], ..., a[(D-1) ld], 2 <= D <= PGB_ROWSUM_MAX_DRAWS, finite by precondition, and one
 * finite y.  No offset and no transform: y_rep is on the scale of the observations already.
 *
 *   order      t_0 .. t_(D-1): the values sorted ascending by pgb_rowsum_key (pgbart_rowsummary.h: -0.0 before +0.0,
 *              ties bit-identical).  Everything below is computed from t BY POSITION, so permuting the draws of a
 *              column changes no bit of any output.
 *   mean, var  pgb_rowsum_part_sum, pgb_rowsum_part_sq and pgb_rowsum_lanes themselves: the bits of pgb_row_summary
 *              with the identity transform and no offset.
 *   abs_err    E|Y - y|: the LANE SUM over j = 0 .. D-1 of |t_j - y|, divided by (double)D.  d = t_j - y, then
 *              d < 0 ? -d : d.  Term j belongs to lane j mod 64.
 *   pair_sum   sum over i < j of (t_j - t_i), in its GAP FORM: the LANE SUM over g = 0 .. D-2 of
 *              c_g (t_(g+1) - t_g), c_g = (double)((int64_t)(g + 1) (D - 1 - g)) -- the number of pairs that straddle
 *              gap g, an exact integer below 2^27.  The difference first, then the product.  Term g belongs to lane
 *              g mod 64.  Every term is non-negative, so nothing cancels (the reason this form is taken and not
 *              sum (2j - D + 1) t_j).  With it  E|Y - Y'| / 2 = pair_sum / D^2, and the caller forms
 *              crps = abs_err - pair_sum / D^2  (the fair form divides by D (D - 1)).
 *   n_below,   the number of t_j < y and of t_j == y: comparisons of doubles as pgb_ppc_compare makes them
 *   n_equal    (pgbart_ppc.h; -0.0 == +0.0).  Integers, stored as doubles; any order of adding them gives the same.
 *   q_k        pgb_rowsum_quantile(t, D, level_k), at most PGB_ROWSUM_MAX_Q levels per call.
 *   pinball_k  u = y - q_k;  u >= 0 ? level_k u : (level_k - 1.0) u.
 *   output     [mean, var, abs_err, pair_sum, n_below, n_equal, q_0 .., pinball_0 ..]: PGB_SCORE_NOUT(n_q) doubles
 *              per column.
 */
#ifndef PGBART_SCORE_H
#define PGBART_SCORE_H

#include "pgbart_rowsummary.h"

#define PGB_SCORE_NFIXED 6
#define PGB_SCORE_NOUT(n_q) (PGB_SCORE_NFIXED + 2 * (n_q))
#define PGB_SCORE_MEAN 0
#define PGB_SCORE_VAR 1
#define PGB_SCORE_ABS_ERR 2
#define PGB_SCORE_PAIR_SUM 3
#define PGB_SCORE_N_BELOW 4
#define PGB_SCORE_N_EQUAL 5

/* partial l of the LANE SUM of |t_j - y| over t[0 .. D) */
PGB_HD double pgb_score_part_abs(const double* t, int D, int l, double y) {
  double s = 0.0;
  for (int j = l; j < D; j += PGB_ROWSUM_LANES) {
    const double d = t[j] - y;
    s = s + (d < 0.0 ? -d : d);
  }
  return s;
}
/* partial l of the LANE SUM of the gap form of pair_sum over the gaps g = 0 .. D-2 */
PGB_HD double pgb_score_part_pair(const double* t, int D, int l) {
  double s = 0.0;
  for (int g = l; g < D - 1; g += PGB_ROWSUM_LANES) {
    const double c = (double)((int64_t)(g + 1) * (int64_t)(D - 1 - g));
    const double w = t[g + 1] - t[g];
    s = s + c * w;
  }
  return s;
}
/* lane l's share of the two counts (integers: the lanes' shares are added in any order) */
PGB_HD void pgb_score_part_counts(const double* t, int D, int l, double y, int32_t* below, int32_t* equal) {
  int32_t b = 0, e = 0;
  for (int j = l; j < D; j += PGB_ROWSUM_LANES) {
    b += t[j] < y ? 1 : 0;
    e += t[j] == y ? 1 : 0;
  }
  *below = b;
  *equal = e;
}
PGB_HD double pgb_score_pinball(double y, double q, double level) {
  const double u = y - q;
  return u >= 0.0 ? level * u : (level - 1.0) * u;
}

/* The whole of one column, a[d * stride], d < D, against y: out[PGB_SCORE_NOUT(n_q)] -- what the device kernel
 * computes.  The caller has checked D, n_q and the levels (above) and provides the workspace: D keys and D doubles.
 * (The sort here is the heap sort of pgb_rowsum_column: any correct sort gives the same array.) */
PGB_HD void pgb_score_column(const double* a, int64_t stride, int D, double y, const double* q, int n_q, uint64_t* key,
                             double* wk, double* out) {
  for (int d = 0; d < D; ++d) key[d] = pgb_rowsum_key(a[(int64_t)d * stride]);
  for (int start = D / 2 - 1; start >= 0; --start) pgb_rowsum_sift(key, start, D);
  for (int end = D - 1; end > 0; --end) {
    const uint64_t v = key[0];
    key[0] = key[end];
    key[end] = v;
    pgb_rowsum_sift(key, 0, end);
  }
  double* t = wk;
  for (int d = 0; d < D; ++d) t[d] = pgb_rowsum_unkey(key[d]);
  double part[PGB_ROWSUM_LANES];
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_rowsum_part_sum(t, D, l);
  const double mean = pgb_rowsum_lanes(part) / (double)D;
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_rowsum_part_sq(t, D, l, mean);
  out[PGB_SCORE_MEAN] = mean;
  out[PGB_SCORE_VAR] = pgb_rowsum_lanes(part) / (double)(D - 1);
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_score_part_abs(t, D, l, y);
  out[PGB_SCORE_ABS_ERR] = pgb_rowsum_lanes(part) / (double)D;
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_score_part_pair(t, D, l);
  out[PGB_SCORE_PAIR_SUM] = pgb_rowsum_lanes(part);
  int64_t below = 0, equal = 0;
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) {
    int32_t b, e;
    pgb_score_part_counts(t, D, l, y, &b, &e);
    below += b;
    equal += e;
  }
  out[PGB_SCORE_N_BELOW] = (double)below;
  out[PGB_SCORE_N_EQUAL] = (double)equal;
  for (int j = 0; j < n_q; ++j) {
    const double qv = pgb_rowsum_quantile(t, D, q[j]);
    out[PGB_SCORE_NFIXED + j] = qv;
    out[PGB_SCORE_NFIXED + n_q + j] = pgb_score_pinball(y, qv, q[j]);
  }
}

#ifdef __cplusplus
extern "C" {
#endif
/* The scores of the first n_cols columns of the device matrix a_dev [D][ld] against y_dev [n_cols] (HIP library only;
 * not part of pgbart.h): out_dev [PGB_SCORE_NOUT(n_q)][n_cols].  q_host: n_q levels in [0, 1] (host memory).
 * Everything is validated before the launch (PGB_E_INVALID with a message: a null pointer, D outside
 * [2, PGB_ROWSUM_MAX_DRAWS], n_cols < 1, ld < n_cols, n_q outside [0, PGB_ROWSUM_MAX_Q], a level outside [0, 1] or
 * NaN).  Returns when out_dev is written. */
int pgb_row_score(const double* a_dev, int32_t D, int64_t n_cols, int64_t ld, const double* y_dev, const double* q_host,
                  int32_t n_q, double* out_dev, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_SCORE_H */
