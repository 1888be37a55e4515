/*
 * pgbart_diag.h -- the numeric contract of the per-column convergence diagnostics of a [D][ld] matrix of posterior
 * draws that came from several chains: rank-normalised split R-hat^2, bulk / tail / mean effective sample sizes
 * (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; what ArviZ's rhat / ess compute) and the relative efficiency
 * r_eff that PSIS-LOO takes (pgb_chain_diag, below; pymc_bart_amd/diagnostics.py).
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /,
 * comparisons, integer operations and pgb_exp_t only -- no FFT, no square root, no logarithm and no inverse normal
 * CDF -- and the ORDER OF EVERY SUM is part of the definition, so that a host evaluation (pgb_diag_column) checks the
 * device kernel bit for bit and a result never depends on the launch geometry.
 *
 * One column: a[0 ld], a[1 ld], ..., a[(D-1) ld], D = n_chains n_per_chain, draw c n_per_chain + i is draw i of chain
 * c, finite by precondition.
 *
 *   split      h = n_per_chain / 2.  Split chain 2c is draws 0 .. h-1 of chain c, split chain 2c+1 its last h draws;
 *              with an odd n_per_chain the middle draw is dropped from everything below, ranks and quantiles too.
 *              J = 2 n_chains split chains of h draws, S = J h KEPT draws; kept position p = j h + i is draw i of split
 *              chain j (pgb_diag_row).  1 <= n_chains <= PGB_DIAG_MAX_CHAINS, n_per_chain >= 4, S <=
 *              PGB_DIAG_MAX_DRAWS (PGB_DIAG_MAX_DRAWS_MEAN for PGB_DIAG_MEAN_ONLY).
 *   transform  x_p = a_p (PGB_DIAG_IDENTITY) | pgb_exp_t(a_p - amax) (PGB_DIAG_EXP_SHIFT), amax the largest kept value
 *              of the column by the key order below: what r_eff needs, the ESS of exp(ll), which does not change
 *              under the shift and cannot overflow.  A -0.0 becomes +0.0 here (and in |x - median|), so that values
 *              that compare equal have equal keys and TIES BY VALUE ARE TIES BY KEY: the ranks are those of
 *              rankdata(method="average").  Everything below is a function of the x_p alone, so EXP_SHIFT equals
 *              IDENTITY on the matrix of the x_p.
 *   order      the x_p sorted ascending by pgb_rowsum_key (include/pgbart_rowsummary.h: the total order of the bit
 *              patterns, -0.0 before +0.0): t_0 .. t_(S-1).
 *   ranks      the keys equal to a value's key occupy the sorted positions [i, j) (pgb_diag_lower, pgb_diag_upper);
 *              its average rank is (i + j + 1) / 2 (1-based) and its z-score is z[i + j - 1], z a TABLE of 2 S - 1
 *              doubles the caller fills with ndtri((r - 3/8) / (S + 1/4)) for r = 1, 1.5, .., S.  The table is an
 *              input: the device needs no inverse CDF and parity does not depend on one.
 *   LANE SUM   the convention of pgbart_rowsummary.h: 64 partials, partial l adds the terms i = l, l + 64, .. in
 *              ascending order onto 0.0, and the partials are added in the order l = 0 .. 63 onto 0.0.
 *   ORDERED SUM  of one value per split chain (pgb_diag_osum): the J values are sorted ascending by pgb_rowsum_key and
 *              added in that order onto 0.0.  Every sum over j below is one, so that PERMUTING WHOLE CHAINS CHANGES NO
 *              BIT of any output (a sum "in j order" would not have that property).
 *
 * For a sequence w_p (one value per kept position), per split chain j:
 *   mean_j     = LANESUM_i(w_ji) / h;  d_ji = w_ji - mean_j;
 *   acov_j[t]  = LANESUM_{i < h - t}(d_ji d_j(i+t)) / h   (biased);   var_j = acov_j[0] h / (h - 1);
 * across the chains (pgb_diag_head):
 *   mbar = OSUM_j(mean_j) / J;  vm = OSUM_j((mean_j - mbar)^2) / (J - 1)   (the variance of the chain means, ddof 1);
 *   s0 = OSUM_j(acov_j[0]);     W = OSUM_j(var_j) / J;   B = h vm;
 *   mean_var = (s0 / J) h / (h - 1);   var_plus = mean_var (h - 1) / h + vm;
 *   rhat2    = (B / W + h - 1) / h   (the square root is the host's);
 *   ESS (Geyer's initial sequences, as ArviZ's _ess writes them), pgb_diag_tau, stated ONCE for both sides:
 *     rho[t] = 1 - (mean_var - OSUM_j(acov_j[t]) / J) / var_plus, rho[0] = 1.  The lags are consumed in PAIRS (0, 1),
 *     (2, 3), ...: after pair k the next pair is asked for while t = 2 k + 1 < h - 3 and the sum of pair k is > 0;
 *     every pair that is followed by another one is INCLUDED.  Initial monotone sequence: an included pair whose sum
 *     exceeds the sum of the included pair before it (as adjusted) is replaced by two halves of that sum.  With
 *     (e, o) the last pair consumed (never included):  extra = e if e > 0 or e + o >= 0, else 0;
 *     tau = -1 + 2 acc + extra, acc the included values added one by one in lag order onto 0.0;  tau below
 *     tau_floor (the host passes 1 / log10(S)) or not a number is tau_floor;  ess = S / tau.
 *     Lags beyond the stopping pair are never computed: the cost of a sequence is O(S x lags kept) -- a few pairs for
 *     a column that mixes, up to h - 3 lags for one that never does.
 *   constant   a sequence whose values all compare equal (a constant column, an indicator that is all 0 or all 1)
 *              is seen BEFORE anything is summed -- the rounded mean of S copies of 0.1 is not 0.1, so its var_plus
 *              is not 0 -- and one whose var_plus is exactly 0.0 after the sums is treated alike: ess = S, rhat2 =
 *              1.0, var = 0.  A zero W with B > 0 gives rhat2 = +inf by the formula, on both sides alike.  Nothing
 *              loops on a value: the only data-dependent loop is the one over the pairs, bounded by h - 3 in its own
 *              condition.
 *
 * Output, PGB_DIAG_NOUT = 10 doubles per column:
 *   0 rhat2_bulk    w = the z-scores of x
 *   1 rhat2_folded  w = the z-scores of |x - median|, median = (t_(S/2-1) + t_(S/2)) / 2 (S is even); the |x - median|
 *                   are sorted and ranked again
 *   2 ess_bulk      of the z-scores of x
 *   3 ess_tail_lo   of the indicator x <= q05          q05, q95 = pgb_rowsum_quantile(t, S, 0.05 | 0.95)
 *   4 ess_tail_hi   of the indicator x >= q95
 *   5 ess_mean      of x itself
 *   6 mean          of x over the kept draws = mbar of w = x
 *   7 var           of x over the kept draws, ddof 1 = h (s0 + (J - 1) vm) / (S - 1) of w = x (the sum of squares
 *                   about mbar, split into its within- and between-chain parts)
 *   8 constant      1.0 when w = x is constant (above), else 0.0
 *   9 reserved      0.0
 * PGB_DIAG_MEAN_ONLY writes rows 5 to 8 and 0.0 elsewhere; it needs no sort, only the maximum (EXP_SHIFT).
 */
#ifndef PGBART_DIAG_H
#define PGBART_DIAG_H

#include "pgbart_rowsummary.h"

#define PGB_DIAG_MAX_DRAWS 8192       /* S above it is refused: keys and sequence of one column fill the LDS of a CU */
#define PGB_DIAG_MAX_DRAWS_MEAN 16384 /* ... PGB_DIAG_MEAN_ONLY keeps the sequence alone */
#define PGB_DIAG_MAX_CHAINS 64        /* J = 2 n_chains values per ordered sum: at most 128 */
#define PGB_DIAG_NOUT 10

#define PGB_DIAG_IDENTITY 0
#define PGB_DIAG_EXP_SHIFT 1
#define PGB_DIAG_N_TRANSFORMS 2

#define PGB_DIAG_ALL 0
#define PGB_DIAG_MEAN_ONLY 1
#define PGB_DIAG_N_STATS 2

/* the row of a_dev that holds kept position p */
PGB_HD int64_t pgb_diag_row(int p, int n_per_chain, int h) {
  const int j = p / h, i = p - j * h;
  return (int64_t)(j >> 1) * (int64_t)n_per_chain + (int64_t)((j & 1) ? n_per_chain - h + i : i);
}

PGB_HD double pgb_diag_x(double a, int transform, double amax, const double* expt) {
  const double x = transform == PGB_DIAG_EXP_SHIFT ? pgb_exp_t(a - amax, expt) : a;
  return x == 0.0 ? 0.0 : x; /* -0.0 becomes +0.0 */
}

/* [i, j) = [lower, upper): the positions of the sorted values t[0 .. S) whose key equals k */
PGB_HD int pgb_diag_lower(const double* t, int S, uint64_t k) {
  int lo = 0, hi = S;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pgb_rowsum_key(t[mid]) < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
PGB_HD int pgb_diag_upper(const double* t, int S, uint64_t k) {
  int lo = 0, hi = S;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pgb_rowsum_key(t[mid]) <= k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
/* the z-score of x among the sorted values t */
PGB_HD double pgb_diag_z(const double* t, int S, double x, const double* z) {
  const uint64_t k = pgb_rowsum_key(x);
  return z[pgb_diag_lower(t, S, k) + pgb_diag_upper(t, S, k) - 1];
}
PGB_HD double pgb_diag_median(const double* t, int S) { return (t[S / 2 - 1] + t[S / 2]) / 2.0; }
PGB_HD double pgb_diag_fold(double x, double med) {
  const double d = x - med;
  return d < 0.0 ? -d : (d == 0.0 ? 0.0 : d);
}

/* partial l of the LANE SUM of acov[t] h over the centred values d[0 .. h) of one split chain */
PGB_HD double pgb_diag_part_acov(const double* d, int h, int t, int l) {
  double s = 0.0;
  for (int i = l; i < h - t; i += PGB_ROWSUM_LANES) s = s + d[i] * d[i + t];
  return s;
}

/* ORDERED SUM: v[0 .. J) is sorted in place (insertion sort: any correct sort gives the same array) */
PGB_HD double pgb_diag_osum(double* v, int J) {
  for (int i = 1; i < J; ++i) {
    const double x = v[i];
    const uint64_t k = pgb_rowsum_key(x);
    int j = i;
    while (j > 0 && pgb_rowsum_key(v[j - 1]) > k) {
      v[j] = v[j - 1];
      --j;
    }
    v[j] = x;
  }
  double s = 0.0;
  for (int j = 0; j < J; ++j) s = s + v[j];
  return s;
}

typedef struct {
  double mbar, vm, s0, wsum;
} pgb_diag_head_t;
/* across the chains, from the chain means mj[J] and the lag-0 autocovariances a0[J] (both are overwritten) */
PGB_HD void pgb_diag_head(double* mj, double* a0, int h, int J, pgb_diag_head_t* o) {
  o->mbar = pgb_diag_osum(mj, J) / (double)J;
  for (int j = 0; j < J; ++j) {
    const double d = mj[j] - o->mbar;
    mj[j] = d * d;
  }
  o->vm = pgb_diag_osum(mj, J) / (double)(J - 1);
  o->s0 = pgb_diag_osum(a0, J);
  for (int j = 0; j < J; ++j) a0[j] = a0[j] * (double)h / (double)(h - 1);
  o->wsum = pgb_diag_osum(a0, J);
}

typedef struct {
  int t;            /* -1 before the pair (0, 1); then the next pair is the lags (t + 1, t + 2) */
  int h, J, n_inc, constant;
  double vm, mean_var, var_plus;
  double even, odd; /* rho of the last pair consumed */
  double pa, pb;    /* the last included pair, as adjusted */
  double acc, tau;
} pgb_diag_geyer;

PGB_HD void pgb_diag_geyer_init(pgb_diag_geyer* g, int h, int J, double vm) {
  g->t = -1;
  g->h = h;
  g->J = J;
  g->n_inc = 0;
  g->constant = 0;
  g->vm = vm;
  g->mean_var = g->var_plus = 0.0;
  g->even = g->odd = g->pa = g->pb = 0.0;
  g->acc = 0.0;
  g->tau = 1.0;
}

/* Geyer's loop, the only statement of it.  Consumes s_even = OSUM_j(acov_j[t + 1]) and s_odd = OSUM_j(acov_j[t + 2])
 * (the first call: lags 0 and 1) and returns 1 when the next pair of lags (g->t + 1, g->t + 2) is needed, 0 when done
 * (g->tau, g->constant are set).  It asks for a pair only while g->t < h - 3. */
PGB_HD int pgb_diag_tau(pgb_diag_geyer* g, double s_even, double s_odd, double tau_floor) {
  const double h = (double)g->h, J = (double)g->J;
  if (g->t < 0) {
    g->mean_var = s_even / J * h / (h - 1.0);
    g->var_plus = g->mean_var * (h - 1.0) / h + g->vm;
    g->t = 1;
    if (g->var_plus == 0.0) {
      g->constant = 1;
      g->tau = 1.0;
      return 0;
    }
    g->even = 1.0;
    g->odd = 1.0 - (g->mean_var - s_odd / J) / g->var_plus;
  } else {
    /* the pair before is followed by this one: it is included */
    double a = g->even, b = g->odd;
    if (g->n_inc > 0 && a + b > g->pa + g->pb) {
      a = (g->pa + g->pb) / 2.0;
      b = a;
    }
    g->acc = g->acc + a;
    g->acc = g->acc + b;
    g->pa = a;
    g->pb = b;
    g->n_inc += 1;
    g->even = 1.0 - (g->mean_var - s_even / J) / g->var_plus;
    g->odd = 1.0 - (g->mean_var - s_odd / J) / g->var_plus;
    g->t += 2;
  }
  if (g->t < g->h - 3 && g->even + g->odd > 0.0) return 1;
  const double extra = (g->even > 0.0 || g->even + g->odd >= 0.0) ? g->even : 0.0;
  double tau = -1.0 + 2.0 * g->acc + extra;
  if (!(tau > tau_floor)) tau = tau_floor;
  g->tau = tau;
  return 0;
}

typedef struct {
  double rhat2, ess, mean, var, constant;
} pgb_diag_seq;
/* the results of one sequence from its head and its finished Geyer state (ess is meaningful only if the loop ran) */
PGB_HD void pgb_diag_result(const pgb_diag_head_t* hd, const pgb_diag_geyer* g, pgb_diag_seq* o) {
  const double h = (double)g->h, J = (double)g->J, S = J * h;
  o->mean = hd->mbar;
  o->var = h * (hd->s0 + (J - 1.0) * hd->vm) / (S - 1.0);
  o->constant = g->constant ? 1.0 : 0.0;
  if (g->constant) {
    o->rhat2 = 1.0;
    o->ess = S;
  } else {
    const double W = hd->wsum / J, B = h * hd->vm;
    o->rhat2 = (B / W + h - 1.0) / h;
    o->ess = S / g->tau;
  }
}

/* the results of a sequence whose S values all compare equal to w0: nothing is summed */
PGB_HD void pgb_diag_all_equal(double w0, int S, pgb_diag_seq* o) {
  o->rhat2 = 1.0;
  o->ess = (double)S;
  o->mean = w0;
  o->var = 0.0;
  o->constant = 1.0;
}

/* One sequence w[0 .. S) (centred in place): what the device does with it.  Workspace: mj, a0, a1 of J doubles each.
 * want_ess == 0: the pairs beyond (0, 1) are not computed and o->ess is not to be read. */
PGB_HD void pgb_diag_sequence(double* w, int h, int J, int want_ess, double tau_floor, double* mj, double* a0, double* a1,
                              pgb_diag_seq* o) {
  double part[PGB_ROWSUM_LANES];
  int same = 1;
  for (int p = 1; p < J * h; ++p) same = same && w[p] == w[0];
  if (same) {
    pgb_diag_all_equal(w[0], J * h, o);
    return;
  }
  for (int j = 0; j < J; ++j) {
    for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_rowsum_part_sum(w + (size_t)j * h, h, l);
    mj[j] = pgb_rowsum_lanes(part) / (double)h;
  }
  for (int j = 0; j < J; ++j)
    for (int i = 0; i < h; ++i) w[(size_t)j * h + i] = w[(size_t)j * h + i] - mj[j];
  pgb_diag_head_t hd;
  pgb_diag_geyer g;
  int need = 1;
  for (int t = -1; need && (t < 0 || (want_ess && t < h - 3)); t += 2) {
    for (int j = 0; j < J; ++j) {
      for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_diag_part_acov(w + (size_t)j * h, h, t + 1, l);
      a0[j] = pgb_rowsum_lanes(part) / (double)h;
      for (int l = 0; l < PGB_ROWSUM_LANES; ++l) part[l] = pgb_diag_part_acov(w + (size_t)j * h, h, t + 2, l);
      a1[j] = pgb_rowsum_lanes(part) / (double)h;
    }
    double s_even;
    if (t < 0) {
      pgb_diag_head(mj, a0, h, J, &hd);
      pgb_diag_geyer_init(&g, h, J, hd.vm);
      s_even = hd.s0;
    } else {
      s_even = pgb_diag_osum(a0, J);
    }
    need = pgb_diag_tau(&g, s_even, pgb_diag_osum(a1, J), tau_floor);
  }
  pgb_diag_result(&hd, &g, o);
}

/* heap sort of the values t[0 .. S) by their keys (any correct sort gives the same array) */
PGB_HD void pgb_diag_sort(double* t, int S, uint64_t* key) {
  for (int p = 0; p < S; ++p) key[p] = pgb_rowsum_key(t[p]);
  for (int start = S / 2 - 1; start >= 0; --start) pgb_rowsum_sift(key, start, S);
  for (int end = S - 1; end > 0; --end) {
    const uint64_t v = key[0];
    key[0] = key[end];
    key[end] = v;
    pgb_rowsum_sift(key, 0, end);
  }
  for (int p = 0; p < S; ++p) t[p] = pgb_rowsum_unkey(key[p]);
}

/* The whole of one column, a[d * stride]: out[PGB_DIAG_NOUT] -- what the device kernel computes.  The caller has
 * checked the arguments (above) and provides the workspace: key[S], x[S], t[S], w[S] and wk[3 J].  z: the table of
 * 2 S - 1 z-scores (not read by PGB_DIAG_MEAN_ONLY). */
PGB_HD void pgb_diag_column(const double* a, int64_t stride, int n_chains, int n_per_chain, int transform, int stats,
                            const double* z, double tau_floor, const double* expt, uint64_t* key, double* x, double* t,
                            double* w, double* wk, double* out) {
  const int h = n_per_chain / 2, J = 2 * n_chains, S = J * h;
  double *mj = wk, *a0 = wk + J, *a1 = wk + 2 * J;
  pgb_diag_seq o;
  for (int r = 0; r < PGB_DIAG_NOUT; ++r) out[r] = 0.0;
  double amax = 0.0;
  if (transform == PGB_DIAG_EXP_SHIFT) {
    uint64_t km = 0;
    for (int p = 0; p < S; ++p) {
      const uint64_t k = pgb_rowsum_key(a[pgb_diag_row(p, n_per_chain, h) * stride]);
      if (k > km) km = k;
    }
    amax = pgb_rowsum_unkey(km);
  }
  for (int p = 0; p < S; ++p) x[p] = pgb_diag_x(a[pgb_diag_row(p, n_per_chain, h) * stride], transform, amax, expt);
  if (stats != PGB_DIAG_MEAN_ONLY) {
    for (int p = 0; p < S; ++p) t[p] = x[p];
    pgb_diag_sort(t, S, key);
    const double med = pgb_diag_median(t, S);
    const double q05 = pgb_rowsum_quantile(t, S, 0.05), q95 = pgb_rowsum_quantile(t, S, 0.95);
    for (int p = 0; p < S; ++p) w[p] = pgb_diag_z(t, S, x[p], z);
    pgb_diag_sequence(w, h, J, 1, tau_floor, mj, a0, a1, &o);
    out[0] = o.rhat2;
    out[2] = o.ess;
    for (int p = 0; p < S; ++p) w[p] = x[p] <= q05 ? 1.0 : 0.0;
    pgb_diag_sequence(w, h, J, 1, tau_floor, mj, a0, a1, &o);
    out[3] = o.ess;
    for (int p = 0; p < S; ++p) w[p] = x[p] >= q95 ? 1.0 : 0.0;
    pgb_diag_sequence(w, h, J, 1, tau_floor, mj, a0, a1, &o);
    out[4] = o.ess;
    for (int p = 0; p < S; ++p) t[p] = pgb_diag_fold(x[p], med);
    pgb_diag_sort(t, S, key);
    for (int p = 0; p < S; ++p) w[p] = pgb_diag_z(t, S, pgb_diag_fold(x[p], med), z);
    pgb_diag_sequence(w, h, J, 0, tau_floor, mj, a0, a1, &o);
    out[1] = o.rhat2;
  }
  for (int p = 0; p < S; ++p) w[p] = x[p];
  pgb_diag_sequence(w, h, J, 1, tau_floor, mj, a0, a1, &o);
  out[5] = o.ess;
  out[6] = o.mean;
  out[7] = o.var;
  out[8] = o.constant;
}

#ifdef __cplusplus
extern "C" {
#endif
/* The diagnostics of the first n_cols columns of the device matrix a_dev [n_chains n_per_chain][ld] (HIP library only;
 * not part of pgbart.h): out_dev [PGB_DIAG_NOUT][n_cols].  transform: PGB_DIAG_IDENTITY | PGB_DIAG_EXP_SHIFT; stats:
 * PGB_DIAG_ALL | PGB_DIAG_MEAN_ONLY; z_host: the 2 S - 1 z-scores (host memory; may be NULL for PGB_DIAG_MEAN_ONLY);
 * tau_floor: 1 / log10(S).  Everything is validated before the launch (PGB_E_INVALID with a message that names the
 * value: n_chains outside [1, PGB_DIAG_MAX_CHAINS], n_per_chain < 4, S above its cap, n_cols < 1, ld < n_cols, an
 * unknown transform or stats, a missing table, a tau_floor that is not finite and positive).  Returns when out_dev is
 * written. */
int pgb_chain_diag(const double* a_dev, int32_t n_chains, int32_t n_per_chain, int64_t n_cols, int64_t ld, int32_t transform,
                   int32_t stats, const double* z_host, double tau_floor, double* out_dev, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_DIAG_H */
