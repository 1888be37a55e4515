/*
 * pgbart_rowsummary.h -- the numeric contract of the per-row posterior summaries: mean, variance, quantiles and the
 * highest-density interval of one column of a [D][ld] matrix of posterior predictions over its D draws
 * (pgb_row_summary, below; pymc_bart_amd/summary.py).
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /,
 * comparisons, integer operations, pgb_exp_t and pgb_lphi_t only, and the ORDER OF EVERY SUM is part of the
 * definition, so that a host evaluation (pgb_rowsum_column) checks the device kernel bit for bit and a result never
 * depends on the launch geometry.
 *
 * One column: a[0 ld], a[1 ld], ..., a[(D-1) ld], 2 <= D <= PGB_ROWSUM_MAX_DRAWS, finite by precondition.
 *
 *   order      the values sorted ascending by the TOTAL ORDER of their bit patterns: pgb_rowsum_key flips every bit
 *              of a negative double and the sign bit of the others, and the unsigned keys are compared.  -0.0 comes
 *              before +0.0; ties are bit-identical, so every correct sort gives the same array a_(0) .. a_(D-1).  (A
 *              NaN sorts by its bits too -- deterministic, and nothing below loops on a value.)
 *   offset     optional, one double per column: s_j = a_(j) + off, added before everything else (a constant shift
 *              keeps the order).  Without an offset nothing is added (-0.0 stays -0.0).
 *   transform  t_j = f(s_j) AFTER the sort: identity | exp: pgb_exp_t(x) | logistic: 1 / (1 + pgb_exp_t(-x)) |
 *              probit: pgb_exp_t(pgb_lphi_t(x)).  Everything below is computed from t BY POSITION, so a table
 *              function that is not monotone in its last ulp cannot change which draw is "the j-th".  (The table exp
 *              is exact in its saturation only for |x| < 4.6e7, pgbart_spec.h: beyond it the bits are still the same
 *              on both sides, but they are not exp(x).)
 *   mean, var  LANE SUMS (the convention of pgbart_psis.h): PGB_ROWSUM_LANES partial sums, partial l adds
 *              t_l, t_(l+64), ... in ascending index order starting from 0.0, and the partials are added in the
 *              order l = 0 .. 63 onto 0.0.  mean = sum / D;  var = (the same shape of sum over (t_j - mean)^2) /
 *              (D - 1).  No square root here (sd = sqrt(var) is the caller's).  The sums run over the SORTED array,
 *              so permuting the draws of a column changes no bit of any output.
 *   quantile   q in [0, 1]: pos = q (D - 1) in double, lo = min((int)pos, D - 1), frac = pos - lo; the result is
 *              t_lo when frac == 0 and t_lo + (t_(lo+1) - t_lo) * frac otherwise (two roundings, no contraction).
 *              At most PGB_ROWSUM_MAX_Q per call.
 *   HDI        hdi_k = max(floor(prob D), 1) is the caller's integer (0: no interval, both slots are 0.0).
 *              hdi_k >= D: (t_0, t_(D-1)).  Otherwise i* = the first index minimising w_i = t_(i+hdi_k) - t_i over
 *              0 <= i < D - hdi_k, the interval (t_i*, t_(i*+hdi_k)) -- the narrowest interval holding hdi_k + 1 of
 *              the sorted draws (importance.hdi; ArviZ's unimodal HDI).  So that a NaN width (inf - inf after exp)
 *              cannot make the answer depend on the geometry either, the minimisation has a fixed shape: lane l
 *              scans i = l, l + 64, ... and keeps the first strictly smaller width; the lanes are combined in the
 *              order l = 0 .. 63 by pgb_rowsum_hdi_better (smaller width, or equal width and lower index).
 *   output     [mean, var, q_0 .. q_(n_q-1), hdi_lo, hdi_hi]: PGB_ROWSUM_NOUT(n_q) doubles per column.
 */
#ifndef PGBART_ROWSUMMARY_H
#define PGBART_ROWSUMMARY_H

#include "pgbart_spec.h"

#define PGB_ROWSUM_MAX_DRAWS 16384 /* D above it is refused (PGB_PSIS_MAX_DRAWS: one column's keys fit the LDS of a CU) */
#define PGB_ROWSUM_MAX_Q 16
#define PGB_ROWSUM_LANES 64
#define PGB_ROWSUM_NOUT(n_q) (2 + (n_q) + 2)

#define PGB_ROWSUM_IDENTITY 0
#define PGB_ROWSUM_EXP 1
#define PGB_ROWSUM_LOGISTIC 2
#define PGB_ROWSUM_PROBIT 3
#define PGB_ROWSUM_N_TRANSFORMS 4

/* the order: a before b iff key(a) < key(b) */
PGB_HD uint64_t pgb_rowsum_key(double x) {
  const uint64_t u = pgb_d2u(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
PGB_HD double pgb_rowsum_unkey(uint64_t k) {
  return pgb_u2d((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}
#define PGB_ROWSUM_PAD_KEY 0xFFFFFFFFFFFFFFFFull /* no key is larger: what a sorting network pads with */

/* t = f(a + off) of one sorted value; has_off == 0: nothing is added */
PGB_HD double pgb_rowsum_value(double a, int has_off, double off, int transform, const pgb_lltabs* tb) {
  const double s = has_off ? a + off : a;
  if (transform == PGB_ROWSUM_EXP) return pgb_exp_t(s, tb->expt);
  if (transform == PGB_ROWSUM_LOGISTIC) return 1.0 / (1.0 + pgb_exp_t(-s, tb->expt));
  if (transform == PGB_ROWSUM_PROBIT) return pgb_exp_t(pgb_lphi_t(s, tb->lphi), tb->expt);
  return s;
}

/* partial l of the two LANE SUMS over t[0 .. D) */
PGB_HD double pgb_rowsum_part_sum(const double* t, int D, int l) {
  double s = 0.0;
  for (int j = l; j < D; j += PGB_ROWSUM_LANES) s = s + t[j];
  return s;
}
PGB_HD double pgb_rowsum_part_sq(const double* t, int D, int l, double mean) {
  double s = 0.0;
  for (int j = l; j < D; j += PGB_ROWSUM_LANES) {
    const double d = t[j] - mean;
    s = s + d * d;
  }
  return s;
}
/* the end of a LANE SUM */
PGB_HD double pgb_rowsum_lanes(const double* part) {
  double s = 0.0;
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) s = s + part[l];
  return s;
}

PGB_HD double pgb_rowsum_quantile(const double* t, int D, double q) {
  const double pos = q * (double)(D - 1);
  int lo = (int)pos;
  if (lo > D - 1) lo = D - 1;
  const double frac = pos - (double)lo;
  if (frac == 0.0) return t[lo];
  const int hi = lo + 1 < D ? lo + 1 : D - 1;
  return t[lo] + (t[hi] - t[lo]) * frac;
}

/* candidate (w, i) before the best so far (bw, bi) */
PGB_HD int pgb_rowsum_hdi_better(double w, int i, double bw, int bi) { return w < bw || (w == bw && i < bi); }
/* lane l's candidate over 0 <= i < D - k (1 <= k < D): its index, or -1 when the lane has none; *w its width */
PGB_HD int pgb_rowsum_hdi_part(const double* t, int D, int k, int l, double* w) {
  const int n = D - k;
  if (l >= n) {
    *w = 0.0;
    return -1;
  }
  int bi = l;
  double bw = t[l + k] - t[l];
  for (int i = l + PGB_ROWSUM_LANES; i < n; i += PGB_ROWSUM_LANES) {
    const double wi = t[i + k] - t[i];
    if (wi < bw) {
      bw = wi;
      bi = i;
    }
  }
  *w = bw;
  return bi;
}
/* i* of the lanes' candidates (lane 0 always has one) */
PGB_HD int pgb_rowsum_hdi_combine(const double* w, const int32_t* idx) {
  int bi = idx[0];
  double bw = w[0];
  for (int l = 1; l < PGB_ROWSUM_LANES; ++l) {
    if (idx[l] < 0) continue;
    if (pgb_rowsum_hdi_better(w[l], idx[l], bw, bi)) {
      bw = w[l];
      bi = idx[l];
    }
  }
  return bi;
}

/* heap sort's sift-down of key[root] within key[0 .. end) (a max-heap) */
PGB_HD void pgb_rowsum_sift(uint64_t* key, int root, int end) {
  const uint64_t v = key[root];
  for (;;) {
    int child = 2 * root + 1;
    if (child >= end) break;
    if (child + 1 < end && key[child + 1] > key[child]) ++child;
    if (!(key[child] > v)) break;
    key[root] = key[child];
    root = child;
  }
  key[root] = v;
}

/* The whole of one column, a[d * stride], d < D: out[PGB_ROWSUM_NOUT(n_q)] -- what the device kernel computes.  The
 * caller has checked D, n_q, the q's and hdi_k (above) and provides the workspace: D keys and D doubles.  off: NULL or the
 * column's offset.  (The sort here is a heap sort of the keys: any correct sort gives the same array.) */
PGB_HD void pgb_rowsum_column(const double* a, int64_t stride, int D, const double* off, int transform, const double* q,
                              int n_q, int hdi_k, const pgb_lltabs* tb, uint64_t* key, double* wk, double* out) {
  for (int d = 0; d < D; ++d) key[d] = pgb_rowsum_key(a[(int64_t)d * stride]);
  for (int start = D / 2 - 1; start >= 0; --start) pgb_rowsum_sift(key, start, D);
  for (int end = D - 1; end > 0; --end) {
    const uint64_t v = key[0];
    key[0] = key[end];
    key[end] = v;
    pgb_rowsum_sift(key, 0, end);
  }
  double* t = wk;
  for (int d = 0; d < D; ++d) t[d] = pgb_rowsum_value(pgb_rowsum_unkey(key[d]), off != 0, off ? *off : 0.0, transform, tb);
  double part[PGB_ROWSUM_LANES];
  int32_t idx[PGB_ROWSUM_LANES];
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_rowsum_part_sum(t, D, l);
  const double mean = pgb_rowsum_lanes(part) / (double)D;
  for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_rowsum_part_sq(t, D, l, mean);
  out[0] = mean;
  out[1] = pgb_rowsum_lanes(part) / (double)(D - 1);
  for (int j = 0; j < n_q; ++j) out[2 + j] = pgb_rowsum_quantile(t, D, q[j]);
  double lo = 0.0, hi = 0.0;
  if (hdi_k >= D) {
    lo = t[0];
    hi = t[D - 1];
  } else if (hdi_k > 0) {
    for (int l = 0; l < PGB_ROWSUM_LANES; ++l) idx[l] = pgb_rowsum_hdi_part(t, D, hdi_k, l, &part[l]);
    const int is = pgb_rowsum_hdi_combine(part, idx);
    lo = t[is];
    hi = t[is + hdi_k];
  }
  out[2 + n_q] = lo;
  out[3 + n_q] = hi;
}

#ifdef __cplusplus
extern "C" {
#endif
/* The summaries of the first n_cols columns of the device matrix a_dev [D][ld] (HIP library only; not part of
 * pgbart.h): out_dev [PGB_ROWSUM_NOUT(n_q)][n_cols].  offset_dev: [n_cols] or NULL; transform: PGB_ROWSUM_*;
 * q_host: n_q quantile levels in [0, 1] (host memory).  Everything is validated before the launch (PGB_E_INVALID
 * with a message: D outside [2, PGB_ROWSUM_MAX_DRAWS], n_cols < 1, ld < n_cols, n_q outside [0, PGB_ROWSUM_MAX_Q], a
 * q outside [0, 1] or not finite, hdi_k < 0, an unknown transform).  Returns when out_dev is written. */
int pgb_row_summary(const double* a_dev, int32_t D, int64_t n_cols, int64_t ld, const double* offset_dev, int32_t transform,
                    const double* q_host, int32_t n_q, int32_t hdi_k, double* out_dev, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_ROWSUMMARY_H */
