/*
 * pgbart_psis.h -- the numeric contract of PSIS-LOO: Pareto-smoothed importance sampling of one row's pointwise
 * log-likelihoods over the posterior draws (Vehtari, Simpson, Gelman, Yao, Gabry; the generalised-Pareto fit of
 * Zhang and Stephens), giving the row's elpd_loo and its Pareto k (pgb_psis_rows, include/pgbart_pointwise.h;
 * pymc_bart_amd/loo.py).
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /,
 * comparisons, PGB_FMA, pgb_exp_t and pgb_log_t only -- no libm, no hardware sqrt -- and the ORDER OF EVERY SUM is
 * part of the definition, so that a host evaluation (pgb_psis_row) checks the device kernel bit for bit and a result
 * never depends on the launch geometry.
 *
 * One row: the clamped values ll[0 .. D-1] as pgb_pointwise_loglik writes them (finite, within [-2047, 2047]) and a
 * tail length M = ceil(min(D / 5, 3 sqrt(D / r_eff))) computed by the caller, 1 <= M < D, M <= PGB_PSIS_MAX_TAIL.
 *
 *   shift     mx = max_d(-ll_d) = -(min_d ll_d);  x_d = (-ll_d) - mx   (<= 0)
 *   cutoff    the (M+1)-th largest x, floored at log(DBL_MIN)
 *   tail      the draws with x_d > cutoff, T of them (ties can make T < M), ascending by (x_d, d)
 *   fit       T <= 4: none, k = +inf.  Otherwise a_t = exp(x_(t)) - exp(cutoff), m_est = 30 + floor(sqrt(T)),
 *             b_j = (1 - sqrt(m_est / (j - 0.5))) / (3 a_[floor(T/4 + 0.5) - 1]) + 1 / a_[T-1],  j = 1 .. m_est
 *             k_j = (sum_t log(1 - b_j a_t)) / T   (t ascending),  L_j = T ((log(-b_j / k_j) - k_j) - 1)
 *             w_j = 1 / sum_i exp(L_i - L_j)       (i ascending, the difference held within +-1000)
 *             every w_j < 10 DBL_EPSILON dropped, the rest divided by their sum (j ascending);  b = sum_j w_j b_j
 *             k' = (sum_t log(1 - b a_t)) / T      (a LANE SUM, below),  sigma = -k' / b,  k = (T k' + 5) / (T + 10)
 *             a k or sigma that is not finite (a degenerate tail: equal a_t, b = 0) counts as no fit: k = +inf
 *   smooth    with a fit, the t-th smallest tail value (t = 1 .. T, p = (t - 0.5) / T) becomes
 *             log(sigma expm1(-k log1p(-p)) / k + exp(cutoff))   (k = 0: -sigma log1p(-p) in place of the quotient),
 *             a non-positive argument gives log(DBL_MIN), and the result is held within [log(DBL_MIN), 0]
 *   result    elpd_loo = logsumexp_d(w_d + ll_d) - logsumexp_d(w_d), w_d the smoothed x_d.  Each logsumexp is
 *             (shift + log(N e + S)): N the LANE SUM over the draws outside the tail of exp(x_d - cutoff)
 *             (of exp((x_d + ll_d) + mx) for the numerator), e = exp(cutoff - wmax) (exp((-mx) - vmax)), S the LANE
 *             SUM over the tail in ascending order of exp(w_t - wmax) (exp(v_t - vmax), v_t = w_t + ll_(t)), and
 *             wmax = max(cutoff, max_t w_t), vmax = max(-mx, max_t v_t).
 *
 * A LANE SUM of terms numbered 0, 1, 2, ... is PGB_PSIS_LANES partial sums -- partial l adds the terms whose number
 * is l mod PGB_PSIS_LANES, in ascending order, starting from 0.0 -- added in the order l = 0 .. PGB_PSIS_LANES-1
 * onto 0.0.  (The draws outside the tail keep their draw index as their number.)
 *
 * sqrt: pgb_psis_sqrt is exp(log(x) / 2) polished by two Newton steps -- built from the operations above, hence the
 * same bits on both sides (its arguments are ratios of integers below 2 PGB_PSIS_MAX_TAIL; within 1 ulp of sqrt).
 * log1p / expm1: pgb_psis_log1p corrects log(1 + x) by x / ((1 + x) - 1); pgb_psis_expm1 is a Taylor polynomial for
 * |y| < 1/4 (where exp(y) - 1 cancels) and exp(y) - 1 beyond.
 *
 * PSIS-weighted expectations (pgb_psis_row_expect; pgb_psis_expect, include/pgbart_pointwise.h): a second row
 * g[0 .. D-1] of the same draws (a predictor, a replicated observation) and the self-normalised sum
 * sum_d exp(w_d) g_c(d) / sum_d exp(w_d) over the row's smoothed weights, which never leave the row.  With mx, cutoff, T,
 * the final tail weights w_t (ascending), wmax, Dn (the N of the denominator above) and St (its S) exactly as above:
 *
 *   clamp     v_d = pgb_psis_gclamp(g_d): held within +-PGB_PSIS_G_MAX = 1e150, so that squares and sums of
 *             PGB_PSIS_MAX_DRAWS terms stay finite; a NaN becomes -PGB_PSIS_G_MAX
 *   kind      PGB_PSIS_G_VALUE (0): g_0 = v, g_1 = v v -- two outputs, E[g] and E[g^2]
 *             PGB_PSIS_G_PIT   (1): g_0 = (v < y) + 0.5 (v == y), y the row's observed value (pgb_ppc_compare's sense:
 *             the mid-p LOO-PIT) -- one output; y is not read for kind 0
 *   result    E_c = (Gn_c e + Gt_c) / (Dn e + St), e = exp(cutoff - wmax): Gn_c the LANE SUM over the draws outside the
 *             tail (numbered by draw index) of pgb_psis_den_term(x_d, cutoff) g_c(d), Gt_c the LANE SUM over the tail
 *             in ascending order of exp(w_t - wmax) g_c(idx_t).  In both the product is formed first, then added (no
 *             FMA), so that g = 1 gives exactly 1.
 */
#ifndef PGBART_PSIS_H
#define PGBART_PSIS_H

#include "pgbart_spec.h"

#define PGB_PSIS_MAX_DRAWS 16384 /* D above it is refused (4 chains x 4096 draws; tail indices are 16-bit on the device) */
#define PGB_PSIS_MAX_TAIL 448    /* M above it is refused: 3 sqrt(D) <= 384 at PGB_PSIS_MAX_DRAWS; m_est <= 51 lanes */
#define PGB_PSIS_LANES 64
#define PGB_PSIS_LOG_DBL_MIN (-708.3964185322641) /* log(2.2250738585072014e-308) */
#define PGB_PSIS_W_MIN 2.220446049250313e-15     /* 10 DBL_EPSILON */

PGB_HD int pgb_psis_finite(double x) { return x - x == 0.0; }
PGB_HD double pgb_psis_inf(void) { return pgb_u2d(0x7FF0000000000000ull); }

/* x positive, finite, normal */
PGB_HD double pgb_psis_sqrt(double x, const pgb_lltabs* tb) {
  double s = pgb_exp_t(0.5 * pgb_log_t(x, tb->logt), tb->expt);
  s = 0.5 * (s + x / s);
  s = 0.5 * (s + x / s);
  return s;
}
PGB_HD int pgb_psis_isqrt(int n) {
  int r = 0;
  while ((r + 1) * (r + 1) <= n) ++r;
  return r;
}
/* log(1 + x), -1 < x */
PGB_HD double pgb_psis_log1p(double x, const pgb_lltabs* tb) {
  const double u = 1.0 + x;
  if (u == 1.0) return x;
  return pgb_log_t(u, tb->logt) * (x / (u - 1.0));
}
/* e^y - 1, y held within +-1000 (beyond it the result is -1 / inf either way) */
PGB_HD double pgb_psis_expm1(double y, const pgb_lltabs* tb) {
  if (y > 1000.0) y = 1000.0;
  if (y < -1000.0) y = -1000.0;
  if (y < 0.25 && y > -0.25) {
    double q = 1.1470745597729725e-11;           /* 1/14! */
    q = PGB_FMA(q, y, 1.6059043836821613e-10);   /* 1/13! */
    q = PGB_FMA(q, y, 2.08767569878681e-09);     /* 1/12! */
    q = PGB_FMA(q, y, 2.505210838544172e-08);    /* 1/11! */
    q = PGB_FMA(q, y, 2.755731922398589e-07);    /* 1/10! */
    q = PGB_FMA(q, y, 2.7557319223985893e-06);   /* 1/9!  */
    q = PGB_FMA(q, y, 2.48015873015873e-05);     /* 1/8!  */
    q = PGB_FMA(q, y, 1.984126984126984e-04);    /* 1/7!  */
    q = PGB_FMA(q, y, 1.3888888888888889e-03);   /* 1/6!  */
    q = PGB_FMA(q, y, 8.3333333333333332e-03);   /* 1/5!  */
    q = PGB_FMA(q, y, 4.1666666666666664e-02);   /* 1/4!  */
    q = PGB_FMA(q, y, 1.6666666666666666e-01);   /* 1/3!  */
    q = PGB_FMA(q, y, 0.5);
    q = PGB_FMA(q, y, 1.0);
    return q * y;
  }
  return pgb_exp_t(y, tb->expt) - 1.0;
}

/* the order of the tail and of the candidates: a before b */
PGB_HD int pgb_psis_before(double xa, int da, double xb, int db) { return xa > xb || (xa == xb && da > db); }

PGB_HD double pgb_psis_x(double ll, double mx) { return (-ll) - mx; }
PGB_HD double pgb_psis_cutoff(double x_m1) { return x_m1 > PGB_PSIS_LOG_DBL_MIN ? x_m1 : PGB_PSIS_LOG_DBL_MIN; }
PGB_HD int pgb_psis_m_est(int T) { return 30 + pgb_psis_isqrt(T); }
/* the terms of the two sums over the draws outside the tail */
PGB_HD double pgb_psis_den_term(double x, double cutoff, const pgb_lltabs* tb) { return pgb_exp_t(x - cutoff, tb->expt); }
PGB_HD double pgb_psis_num_term(double x, double ll, double mx, const pgb_lltabs* tb) {
  return pgb_exp_t((x + ll) + mx, tb->expt);
}

/* b_j, j = 1 .. m_est; q1 = a[(T + 2) / 4 - 1], aN = a[T - 1] */
PGB_HD double pgb_psis_bj(int j, int m_est, double q1, double aN, const pgb_lltabs* tb) {
  return (1.0 - pgb_psis_sqrt((double)m_est / ((double)j - 0.5), tb)) / (3.0 * q1) + 1.0 / aN;
}
PGB_HD double pgb_psis_grid_term(double b, double a, const pgb_lltabs* tb) { return pgb_log_t(1.0 - b * a, tb->logt); }
/* L_j from the plain sum s = sum_t pgb_psis_grid_term(b_j, a_t) */
PGB_HD double pgb_psis_Lj(double b, double s, int T, const pgb_lltabs* tb) {
  const double kj = s / (double)T;
  return (double)T * ((pgb_log_t(-b / kj, tb->logt) - kj) - 1.0);
}
/* w_j of the m_est values L[] */
PGB_HD double pgb_psis_wj(const double* L, int j, int m_est, const pgb_lltabs* tb) {
  double s = 0.0;
  for (int i = 0; i < m_est; ++i) {
    double d = L[i] - L[j];
    if (d > 1000.0) d = 1000.0;
    if (d < -1000.0) d = -1000.0;
    s = s + pgb_exp_t(d, tb->expt);
  }
  return 1.0 / s;
}
/* b = sum_j w_j b_j over the weights kept, renormalised */
PGB_HD double pgb_psis_b(const double* w, const double* bj, int m_est) {
  double ws = 0.0;
  for (int j = 0; j < m_est; ++j) {
    if (w[j] < PGB_PSIS_W_MIN) continue;
    ws = ws + w[j];
  }
  double b = 0.0;
  for (int j = 0; j < m_est; ++j) {
    if (w[j] < PGB_PSIS_W_MIN) continue;
    b = b + (w[j] / ws) * bj[j];
  }
  return b;
}
/* the end of a LANE SUM */
PGB_HD double pgb_psis_lanes(const double* part) {
  double s = 0.0;
  for (int l = 0; l < PGB_PSIS_LANES; ++l) s = s + part[l];
  return s;
}
/* (k, sigma) from b and the lane sum ks = sum_t pgb_psis_grid_term(b, a_t); 1 when there is a fit */
PGB_HD int pgb_psis_k_sigma(double b, double ks, int T, double* k, double* sigma) {
  const double kp = ks / (double)T;
  *sigma = -kp / b;
  *k = ((double)T * kp + 5.0) / ((double)T + 10.0);
  return pgb_psis_finite(*k) && pgb_psis_finite(*sigma);
}
/* the smoothed value of the tail's t-th smallest (t = 0 .. T-1) */
PGB_HD double pgb_psis_smooth(int t, int T, double k, double sigma, double ecut, const pgb_lltabs* tb) {
  const double p = ((double)(t + 1) - 0.5) / (double)T;
  const double l1 = pgb_psis_log1p(-p, tb);
  const double z = k == 0.0 ? -sigma * l1 : sigma * pgb_psis_expm1(-k * l1, tb) / k;
  const double arg = z + ecut;
  double w = arg > 0.0 ? pgb_log_t(arg, tb->logt) : PGB_PSIS_LOG_DBL_MIN;
  if (!(w >= PGB_PSIS_LOG_DBL_MIN)) w = PGB_PSIS_LOG_DBL_MIN;
  if (w > 0.0) w = 0.0;
  return w;
}
/* elpd_loo of the row from the four sums */
PGB_HD double pgb_psis_elpd(double Nn, double Dn, double Vt, double St, double mx, double cutoff, double vmax, double wmax,
                            const pgb_lltabs* tb) {
  const double den = Dn * pgb_exp_t(cutoff - wmax, tb->expt) + St;
  const double num = Nn * pgb_exp_t((-mx) - vmax, tb->expt) + Vt;
  return (vmax + pgb_log_t(num, tb->logt)) - (wmax + pgb_log_t(den, tb->logt));
}

/* the functionals of the PSIS-weighted expectations */
#define PGB_PSIS_G_VALUE 0
#define PGB_PSIS_G_PIT 1
#define PGB_PSIS_G_NONE (-1) /* (pgb_psis_row: no second row) */
#define PGB_PSIS_G_MAX 1e150
PGB_HD double pgb_psis_gclamp(double g) { return g > PGB_PSIS_G_MAX ? PGB_PSIS_G_MAX : (g >= -PGB_PSIS_G_MAX ? g : -PGB_PSIS_G_MAX); }
PGB_HD int pgb_psis_n_expect(int kind) { return kind == PGB_PSIS_G_VALUE ? 2 : 1; }
/* g_0 of the clamped value v */
PGB_HD double pgb_psis_g0(double v, double y, int kind) {
  return kind == PGB_PSIS_G_PIT ? (v < y ? 1.0 : 0.0) + 0.5 * (v == y ? 1.0 : 0.0) : v;
}
/* E_c from its two lane sums and the denominator's */
PGB_HD double pgb_psis_ratio(double Gn, double Gt, double Dn, double St, double cutoff, double wmax, const pgb_lltabs* tb) {
  const double e = pgb_exp_t(cutoff - wmax, tb->expt);
  return (Gn * e + Gt) / (Dn * e + St);
}

/* doubles / int32s of workspace pgb_psis_row needs */
#define PGB_PSIS_WORK_DOUBLES(M) (2 * ((M) + 1) + 3 * PGB_PSIS_LANES)
#define PGB_PSIS_WORK_INTS(M) ((M) + 1)

/* The whole of one row, ll[d * stride], d < D, with the second row g[d * gstride] when kind is not PGB_PSIS_G_NONE:
 * out = (elpd_loo_i, k_i[, E_0[, E_1]]) -- what the device kernels compute.  The caller has checked D, M (above) and
 * provides the workspace. */
PGB_HD void pgb_psis_row_any(const double* ll, int64_t stride, const double* g, int64_t gstride, double y, int kind, int D,
                             int M, const pgb_lltabs* tb, double* wk, int32_t* idx, double* out2) {
  double* key = wk;            /* the M + 1 largest x, descending by pgb_psis_before */
  double* a = wk + (M + 1);    /* the tail's a_t, then its final weights w_t, ascending */
  double* bj = a + (M + 1);
  double* Lj = bj + PGB_PSIS_LANES;
  double* wj = Lj + PGB_PSIS_LANES;
  double p1[PGB_PSIS_LANES], p2[PGB_PSIS_LANES], e1[PGB_PSIS_LANES], e2[PGB_PSIS_LANES];
  double mn = ll[0];
  for (int d = 1; d < D; ++d)
    if (ll[(int64_t)d * stride] < mn) mn = ll[(int64_t)d * stride];
  const double mx = -mn;
  int cnt = 0;
  for (int d = 0; d < D; ++d) {
    const double x = pgb_psis_x(ll[(int64_t)d * stride], mx);
    if (cnt == M + 1 && !pgb_psis_before(x, d, key[M], idx[M])) continue;
    int pos = cnt < M + 1 ? cnt : M;
    while (pos > 0 && pgb_psis_before(x, d, key[pos - 1], idx[pos - 1])) {
      key[pos] = key[pos - 1];
      idx[pos] = idx[pos - 1];
      --pos;
    }
    key[pos] = x;
    idx[pos] = d;
    if (cnt < M + 1) ++cnt;
  }
  const double cutoff = pgb_psis_cutoff(key[M]);
  int T = 0;
  while (T < M && key[T] > cutoff) ++T;
  /* the draws outside the tail */
  for (int l = 0; l < PGB_PSIS_LANES; ++l) p1[l] = p2[l] = e1[l] = e2[l] = 0.0;
  for (int d = 0; d < D; ++d) {
    const double v = ll[(int64_t)d * stride];
    const double x = pgb_psis_x(v, mx);
    if (x > cutoff) continue;
    const double dt = pgb_psis_den_term(x, cutoff, tb);
    p1[d % PGB_PSIS_LANES] = p1[d % PGB_PSIS_LANES] + dt;
    p2[d % PGB_PSIS_LANES] = p2[d % PGB_PSIS_LANES] + pgb_psis_num_term(x, v, mx, tb);
    if (kind != PGB_PSIS_G_NONE) {
      const double gv = pgb_psis_gclamp(g[(int64_t)d * gstride]);
      e1[d % PGB_PSIS_LANES] = e1[d % PGB_PSIS_LANES] + dt * pgb_psis_g0(gv, y, kind);
      if (kind == PGB_PSIS_G_VALUE) e2[d % PGB_PSIS_LANES] = e2[d % PGB_PSIS_LANES] + dt * (gv * gv);
    }
  }
  const double Dn = pgb_psis_lanes(p1), Nn = pgb_psis_lanes(p2);
  const double Gn0 = pgb_psis_lanes(e1), Gn1 = pgb_psis_lanes(e2);
  /* the fit */
  const double ecut = pgb_exp_t(cutoff, tb->expt);
  double khat = pgb_psis_inf();
  int fit = 0;
  if (T > 4) {
    for (int t = 0; t < T; ++t) a[t] = pgb_exp_t(key[T - 1 - t], tb->expt) - ecut;
    const int m_est = pgb_psis_m_est(T);
    const double q1 = a[(T + 2) / 4 - 1], aN = a[T - 1];
    for (int j = 1; j <= m_est; ++j) {
      const double b = pgb_psis_bj(j, m_est, q1, aN, tb);
      double s = 0.0;
      for (int t = 0; t < T; ++t) s = s + pgb_psis_grid_term(b, a[t], tb);
      bj[j - 1] = b;
      Lj[j - 1] = pgb_psis_Lj(b, s, T, tb);
    }
    for (int j = 0; j < m_est; ++j) wj[j] = pgb_psis_wj(Lj, j, m_est, tb);
    const double b = pgb_psis_b(wj, bj, m_est);
    for (int l = 0; l < PGB_PSIS_LANES; ++l) p1[l] = 0.0;
    for (int t = 0; t < T; ++t) p1[t % PGB_PSIS_LANES] = p1[t % PGB_PSIS_LANES] + pgb_psis_grid_term(b, a[t], tb);
    double k, sigma;
    fit = pgb_psis_k_sigma(b, pgb_psis_lanes(p1), T, &k, &sigma);
    if (fit) {
      khat = k;
      for (int t = 0; t < T; ++t) a[t] = pgb_psis_smooth(t, T, k, sigma, ecut, tb);
    }
  }
  if (!fit)
    for (int t = 0; t < T; ++t) a[t] = key[T - 1 - t];
  /* the tail's terms */
  double wmax = cutoff, vmax = -mx;
  for (int t = 0; t < T; ++t) {
    const double v = a[t] + ll[(int64_t)idx[T - 1 - t] * stride];
    if (a[t] > wmax) wmax = a[t];
    if (v > vmax) vmax = v;
  }
  for (int l = 0; l < PGB_PSIS_LANES; ++l) p1[l] = p2[l] = e1[l] = e2[l] = 0.0;
  for (int t = 0; t < T; ++t) {
    const double v = a[t] + ll[(int64_t)idx[T - 1 - t] * stride];
    const double et = pgb_exp_t(a[t] - wmax, tb->expt);
    p1[t % PGB_PSIS_LANES] = p1[t % PGB_PSIS_LANES] + et;
    p2[t % PGB_PSIS_LANES] = p2[t % PGB_PSIS_LANES] + pgb_exp_t(v - vmax, tb->expt);
    if (kind != PGB_PSIS_G_NONE) {
      const double gv = pgb_psis_gclamp(g[(int64_t)idx[T - 1 - t] * gstride]);
      e1[t % PGB_PSIS_LANES] = e1[t % PGB_PSIS_LANES] + et * pgb_psis_g0(gv, y, kind);
      if (kind == PGB_PSIS_G_VALUE) e2[t % PGB_PSIS_LANES] = e2[t % PGB_PSIS_LANES] + et * (gv * gv);
    }
  }
  const double St = pgb_psis_lanes(p1);
  out2[0] = pgb_psis_elpd(Nn, Dn, pgb_psis_lanes(p2), St, mx, cutoff, vmax, wmax, tb);
  out2[1] = khat;
  if (kind != PGB_PSIS_G_NONE) {
    out2[2] = pgb_psis_ratio(Gn0, pgb_psis_lanes(e1), Dn, St, cutoff, wmax, tb);
    if (kind == PGB_PSIS_G_VALUE) out2[3] = pgb_psis_ratio(Gn1, pgb_psis_lanes(e2), Dn, St, cutoff, wmax, tb);
  }
}

/* PSIS-LOO of one row: out2 = (elpd_loo_i, k_i) */
PGB_HD void pgb_psis_row(const double* ll, int64_t stride, int D, int M, const pgb_lltabs* tb, double* wk, int32_t* idx,
                         double* out2) {
  pgb_psis_row_any(ll, stride, (const double*)0, 0, 0.0, PGB_PSIS_G_NONE, D, M, tb, wk, idx, out2);
}
/* ... and its PSIS-weighted expectations of the row g: out = (elpd_loo_i, k_i, E_0[, E_1]), kind PGB_PSIS_G_VALUE
 * (E[g], E[g^2]) or PGB_PSIS_G_PIT (the mid-p LOO-PIT of y); the first two are pgb_psis_row's bits */
PGB_HD void pgb_psis_row_expect(const double* ll, int64_t stride, const double* g, int64_t gstride, double y, int kind, int D,
                                int M, const pgb_lltabs* tb, double* wk, int32_t* idx, double* out) {
  pgb_psis_row_any(ll, stride, g, gstride, y, kind, D, M, tb, wk, idx, out);
}

#endif /* PGBART_PSIS_H */
