/*
 * pgbart_rank.h -- the contract of the discrimination measures of a one-output (Bernoulli) fit, per posterior draw and
 * by group: the ROC AUC, the two-sample Kolmogorov-Smirnov distance and the true / false positive counts at given
 * thresholds (pgb_rank_keys, pgb_rank_metrics, below; pymc_bart_amd/discrimination.py).  pgbart_rowsummary.h takes order
 * statistics over the draws, per row; this header is its transpose: order statistics over the ROWS, per draw.
 *
 * EVERY RESULT IS AN INTEGER -- a count of pairs or of rows -- and a function of the multiset of the keys of two
 * segments only.  So host and device agree exactly, and no bit depends on blocking, chunking, the launch geometry or
 * the order in which a sort or an atomic meets the elements.  Host and device compile the functions below from this
 * one text (PGB_HD, -ffp-contract=off).
 *
 *   value    v = pgb_rowsum_value(a, has_off, off, transform, tb): the value pgb_row_reduce and pgb_row_summary use,
 *            with the PGB_ROWSUM_* transform codes.  Fits with one output only (K == 1).
 *   key      pgb_rank_key(v): a uint64_t whose unsigned order is the order of the doubles.  -0.0 is made +0.0 first,
 *            so the two zeros share a key; -inf and +inf are ordinary values; a NaN (any sign, any payload) gets
 *            PGB_RANK_NAN_KEY = UINT64_MAX, above every other key, and is counted in n_nan (an AUC over NaN scores
 *            is undefined: the Python layer turns n_nan > 0 into an error).
 *   layout   the n rows of a call form 2 G segments, s = 2 g + c, c = 1 for y == 1 and c = 0 for y == 0.  The host
 *            computes seg_off[2 G + 1] (seg_off[0] = 0, seg_off[2 G] = n) and dest[i], the position of row i: the rows
 *            of a segment in ascending row order, the segments in ascending s (pgb_rank_layout).  X is neither copied
 *            nor permuted: the key of row i of draw d is written to keys[d n + dest[i]].
 *   results  per (draw d, group g), n1 and n0 the group's class sizes, all int64:
 *              U2  = sum over the positives i of (2 #{j neg : v_j < v_i} + #{j neg : v_j == v_i});
 *                    the AUC is U2 / (2 n1 n0);
 *              KSN = max over every element e of either class of |tp(e) n0 - fp(e) n1|, tp(e) = #{pos : v >= v_e},
 *                    fp(e) = #{neg : v >= v_e}; the KS distance is KSN / (n1 n0);
 *              tp[t] = #{pos : v >= thr[t]}, fp[t] = #{neg : v >= thr[t]}, t < T <= PGB_RANK_MAX_THRESHOLDS: the
 *                    thresholds are given on the scale of v and compared as doubles through their keys -- positive
 *                    iff score >= threshold, the rule of sklearn's roc_curve.  A NaN threshold is refused; the
 *                    infinities are allowed.
 *            out[(d G + g) (2 + 2 T) + .] = U2, KSN, tp[0 .. T), fp[0 .. T).
 *   bounds   refused (pgb_rank_fault names the argument): G outside [1, PGB_RANK_MAX_GROUPS]; an empty segment;
 *            n1 n0 >= 2^52 in a group (so that the divisions of the Python layer are of exactly representable
 *            integers; every product and sum above then fits an int64); D < 1; n < 2; T outside
 *            [0, PGB_RANK_MAX_THRESHOLDS]; a NaN threshold; D n >= 2^31 (the sort counts its items in an int).
 */
#ifndef PGBART_RANK_H
#define PGBART_RANK_H

#include "pgbart_rowsummary.h"

#define PGB_RANK_MAX_GROUPS 256
#define PGB_RANK_MAX_THRESHOLDS 64
#define PGB_RANK_NAN_KEY 0xFFFFFFFFFFFFFFFFull
#define PGB_RANK_NOUT(T) (2 + 2 * (T))
#define PGB_RANK_N_COUNTERS 2 /* n_nan, n_bad_dest */

PGB_HD int pgb_rank_is_nan(double v) { return (pgb_d2u(v) & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }
PGB_HD uint64_t pgb_rank_key(double v) {
  uint64_t u = pgb_d2u(v);
  if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return PGB_RANK_NAN_KEY;
  if (u == 0x8000000000000000ull) u = 0; /* -0.0 == +0.0 */
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

/* the first position in the sorted k[0 .. len) whose key is >= key (lower) | > key (upper) */
PGB_HD int64_t pgb_rank_lower(const uint64_t* k, int64_t len, uint64_t key) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (k[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
PGB_HD int64_t pgb_rank_upper(const uint64_t* k, int64_t len, uint64_t key) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (k[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
/* what one element proposes for KSN */
PGB_HD int64_t pgb_rank_ks_term(int64_t tp, int64_t fp, int64_t n1, int64_t n0) {
  const int64_t t = tp * n0 - fp * n1;
  return t < 0 ? -t : t;
}

/* The bounds of one call, in the order they are reported: 0 when all hold, otherwise the number of the sentence of
 * pgb_rank_fault_text.  *where: the segment, group or threshold the sentence is about. */
PGB_HD int pgb_rank_fault(int64_t D, int64_t n, const int64_t* seg_off, int64_t G, const double* thr, int64_t T, int64_t* where) {
  *where = 0;
  if (D < 1) return 1;
  if (n < 2) return 2;
  if (G < 1 || G > PGB_RANK_MAX_GROUPS) return 3;
  if (T < 0 || T > PGB_RANK_MAX_THRESHOLDS) return 4;
  if (!seg_off) return 5;
  if (T > 0 && !thr) return 6;
  if (n >= ((int64_t)1 << 31) || D >= ((int64_t)1 << 31) || D * n >= ((int64_t)1 << 31)) return 7;
  if (seg_off[0] != 0 || seg_off[2 * G] != n) return 8;
  for (int64_t s = 0; s < 2 * G; ++s)
    if (seg_off[s + 1] <= seg_off[s] || seg_off[s + 1] > n) {
      *where = s;
      return 9;
    }
  for (int64_t g = 0; g < G; ++g) {
    const int64_t n0 = seg_off[2 * g + 1] - seg_off[2 * g], n1 = seg_off[2 * g + 2] - seg_off[2 * g + 1];
    if (n1 >= ((int64_t)1 << 52) / n0 + (((int64_t)1 << 52) % n0 != 0)) { /* n1 n0 >= 2^52 */
      *where = g;
      return 10;
    }
  }
  for (int64_t t = 0; t < T; ++t)
    if (pgb_rank_is_nan(thr[t])) {
      *where = t;
      return 11;
    }
  return 0;
}
#define PGB_RANK_FAULT_TEXTS                                                                                            \
  {"", "D must be >= 1", "n must be >= 2", "G must be in [1, PGB_RANK_MAX_GROUPS = 256]",                               \
   "T must be in [0, PGB_RANK_MAX_THRESHOLDS = 64]", "seg_off_host is null", "thr_host is null",                        \
   "D x n must be < 2^31", "seg_off_host must start at 0 and end at n", "seg_off_host: segment %lld is empty or out of order", \
   "seg_off_host: n1 x n0 of group %lld must be < 2^52", "thr_host[%lld] is a NaN"}

/* seg_off[2 G + 1] and dest[n] from the class c[i] in {0, 1} and the group g[i] in [0, G) of every row; returns 0, or
 * 1 + the first row whose class or group is outside its range */
PGB_HD int64_t pgb_rank_layout(const int32_t* c, const int32_t* g, int64_t n, int G, int64_t* seg_off, int64_t* dest) {
  for (int s = 0; s <= 2 * G; ++s) seg_off[s] = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (c[i] < 0 || c[i] > 1 || g[i] < 0 || g[i] >= G) return 1 + i;
    seg_off[2 * g[i] + c[i] + 1] += 1;
  }
  for (int s = 0; s < 2 * G; ++s) seg_off[s + 1] += seg_off[s];
  for (int64_t i = 0; i < n; ++i) dest[i] = seg_off[2 * g[i] + c[i]]++; /* (seg_off[s] is now the END of segment s) */
  for (int s = 2 * G; s > 0; --s) seg_off[s] = seg_off[s - 1];
  seg_off[0] = 0;
  return 0;
}

/* One block of nb rows of D draws, sequentially -- what k_rank_keys computes.  a: element (d, i) at [d ld + i]; off:
 * [nb] or NULL; dest: [nb], the positions of the block's rows among the n of the call; keys: [D][n];
 * counters[PGB_RANK_N_COUNTERS] are added to: n_nan, and n_bad_dest, the (d, i) whose dest is outside [0, n) -- they
 * write nothing. */
PGB_HD void pgb_rank_keys_block(const double* a, int64_t D, int64_t nb, int64_t ld, const double* off, int transform,
                                const int64_t* dest, int64_t n, const pgb_lltabs* tb, uint64_t* keys, uint64_t* counters) {
  for (int64_t d = 0; d < D; ++d)
    for (int64_t i = 0; i < nb; ++i) {
      if (dest[i] < 0 || dest[i] >= n) {
        counters[1] += 1;
        continue;
      }
      const double v = pgb_rowsum_value(a[d * ld + i], off != 0, off ? off[i] : 0.0, transform, tb);
      if (pgb_rank_is_nan(v)) counters[0] += 1;
      keys[d * n + dest[i]] = pgb_rank_key(v);
    }
}

/* The results of a call by plain pair counting, O(n1 n0) per (draw, group) for U2 and O((n1 + n0)^2) for KSN, with no
 * sort: keys [D][n] in the layout above (in any order inside a segment), out[D][G][PGB_RANK_NOUT(T)].  The caller has
 * checked the bounds (pgb_rank_fault). */
PGB_HD void pgb_rank_reference(const uint64_t* keys, int64_t D, int64_t n, const int64_t* seg_off, int G, const double* thr,
                               int T, int64_t* out) {
  for (int64_t d = 0; d < D; ++d)
    for (int g = 0; g < G; ++g) {
      const uint64_t* neg = keys + d * n + seg_off[2 * g];
      const uint64_t* pos = keys + d * n + seg_off[2 * g + 1];
      const int64_t n0 = seg_off[2 * g + 1] - seg_off[2 * g], n1 = seg_off[2 * g + 2] - seg_off[2 * g + 1];
      int64_t* o = out + (d * G + g) * PGB_RANK_NOUT(T);
      int64_t u2 = 0, ksn = 0;
      for (int64_t i = 0; i < n1; ++i)
        for (int64_t j = 0; j < n0; ++j) u2 += neg[j] < pos[i] ? 2 : (neg[j] == pos[i] ? 1 : 0);
      for (int64_t e = 0; e < n1 + n0; ++e) {
        const uint64_t k = e < n0 ? neg[e] : pos[e - n0];
        int64_t tp = 0, fp = 0;
        for (int64_t i = 0; i < n1; ++i) tp += pos[i] >= k ? 1 : 0;
        for (int64_t j = 0; j < n0; ++j) fp += neg[j] >= k ? 1 : 0;
        const int64_t term = pgb_rank_ks_term(tp, fp, n1, n0);
        if (term > ksn) ksn = term;
      }
      o[0] = u2;
      o[1] = ksn;
      for (int t = 0; t < T; ++t) {
        const uint64_t k = pgb_rank_key(thr[t]);
        int64_t tp = 0, fp = 0;
        for (int64_t i = 0; i < n1; ++i) tp += pos[i] >= k ? 1 : 0;
        for (int64_t j = 0; j < n0; ++j) fp += neg[j] >= k ? 1 : 0;
        o[2 + t] = tp;
        o[2 + T + t] = fp;
      }
    }
}

#ifdef __cplusplus
extern "C" {
#endif
/* (HIP library only; not part of pgbart.h.)
 *
 * pgb_rank_keys: the keys of one block of nb rows of D draws.  a_dev: the device matrix [D][nb] with the leading
 * dimension ld >= nb between consecutive draws (the output of pgb_predict for a fit with one output); off_dev [nb] or
 * NULL; dest_dev [nb] (int64): the positions of the block's rows among the n rows of the call; keys_dev [D][n];
 * counters_dev: PGB_RANK_N_COUNTERS 64-bit integers on the device, ADDED to (the caller clears them before the first
 * block): n_nan and n_bad_dest.  A dest outside [0, n) writes no key and is counted; pgb_rank_metrics refuses such a
 * call.  Everything else is validated before anything is launched (PGB_E_INVALID with a message naming the argument:
 * null pointers, D < 1, nb < 1, n < 2, nb > n, ld < nb, an unknown transform, D x n >= 2^31).  Returns when keys_dev
 * is written.
 *
 * pgb_rank_workspace_bytes: the bytes ws_dev of pgb_rank_metrics must have -- the second half of the keys' double
 * buffer and the temporary storage of the segmented sort; 0 when an argument is out of bounds; negative: the
 * query failed.
 *
 * pgb_rank_metrics: sorts each of the 2 G D segments of keys_dev (hipcub::DeviceSegmentedRadixSort::SortKeys on the
 * 64-bit keys, keys only, through a double buffer of keys_dev and ws_dev: keys_dev does not keep its contents) and
 * counts.  seg_off_host [2 G + 1], thr_host [T] or NULL with T == 0, out_host [D][G][PGB_RANK_NOUT(T)] (int64) and
 * counts_host [PGB_RANK_N_COUNTERS] are host memory; counters_dev is what pgb_rank_keys added to.  Everything is
 * validated before anything is launched (pgb_rank_fault); a refused call writes nothing.  PGB_E_INVALID after writing
 * counts_host alone when n_bad_dest != 0.
 *
 * pgb_rank_kernel_ms: with PGB_WALK_TIMING=1 in the environment (read per call) the last k_rank_keys, segmented sort
 * and k_rank_count (with the threshold counts) of the calling thread in milliseconds; -1.0: none yet. */
int pgb_rank_keys(const double* a_dev, int32_t D, int64_t nb, int64_t ld, const double* off_dev, int32_t transform,
                  const int64_t* dest_dev, int64_t n, uint64_t* keys_dev, uint64_t* counters_dev, void* stream);
int64_t pgb_rank_workspace_bytes(int32_t D, int64_t n, int32_t G);
int pgb_rank_metrics(uint64_t* keys_dev, void* ws_dev, int32_t D, int64_t n, const int64_t* seg_off_host, int32_t G,
                     const double* thr_host, int32_t T, const uint64_t* counters_dev, int64_t* out_host, int64_t* counts_host,
                     void* stream);
int pgb_rank_kernel_ms(double* keys_ms, double* sort_ms, double* count_ms);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_RANK_H */
