/*
 * pgbart_logpdf.h -- the numeric contract of scoring a fit: the FULL, normalised log density (or log mass) of one
 * observation under each built-in family, and the reduction of one row's values over the posterior draws
 * (pgb_pointwise_loglik, include/pgbart_pointwise.h; pymc_bart_amd/pointwise.py).
 *
 * The sampler's own per-row values (pgb_loglik1q and friends, pgbart_spec.h) are written relative to a saturated
 * model with their mu-free terms dropped: right for particle weights, wrong for comparing two models or two
 * values of sigma.  The functions below keep every term.  Host and device compile them from this one text
 * (PGB_HD, -ffp-contract=off), with + - * /, comparisons, pgb_exp_t, pgb_log_t, pgb_lphi_t, pgb_softplus_t and
 * pgb_cl_lgamma only -- no libm -- so that a host evaluation checks the device bit for bit.
 *
 *   family               params          log density at y, linear predictor(s) mu
 *   NORMAL               sigma           -log sigma - log sqrt(2 pi) - ((y - mu) / sigma)^2 / 2
 *   BERNOULLI_PROBIT                     log Phi(+-mu)
 *   BERNOULLI_LOGIT                      -log(1 + e^(-+mu))
 *   CATEGORICAL          (K <= 16)       mu[y] - logsumexp(mu)
 *   NORMAL_MEANSCALE     (K = 2)         NORMAL with mean mu[0], sigma = |mu[1]| (floored at 1e-8 like the sampler)
 *   POISSON_LOG                          y mu - e^mu - lgamma(y + 1)
 *   NEGBIN_LOG           alpha           lgamma(y + alpha) - lgamma(y + 1) - lgamma(alpha) + alpha log alpha + y mu
 *                                        - (alpha + y) log(alpha + e^mu)
 *   ASYMLAPLACE          b, q            log(q (1 - q) / b) - rho_q((y - mu) / b)        (Yu-Moyeed)
 *   STUDENT_T            sigma, nu       lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2 - log sigma
 *                                        - (nu + 1) / 2 log(1 + ((y - mu) / sigma)^2 / nu)
 *   GAMMA_LOG            alpha           alpha log alpha - lgamma(alpha) + (alpha - 1) log y - alpha (y e^-mu + mu)
 *
 * The terms of a draw's parameters alone are computed ONCE per draw (pgb_logpdf_prepare, on the host) into a row
 * of PGB_PW_NPAR values q[]; pgb_logpdf_raw reads that row.  The value then passes through pgb_clamp_loglik
 * ([-2047, 2047], NaN -> -2047: what the sampler itself can represent); pgb_pw_is_clamped says whether it did, and
 * every caller counts those (draw, row) pairs -- a clamp is reported, never silent.
 */
#ifndef PGBART_LOGPDF_H
#define PGBART_LOGPDF_H

#include "pgbart_spec.h"
#include "pgbart_compiled.h" /* pgb_cl_lgamma: the vocabulary's log Gamma */

#define PGB_PW_CHUNK 32 /* draws per chunk of the reduction over draws: part of the result's definition */
#define PGB_PW_NPAR 4   /* prepared values per draw of a built-in family */

/* the params a built-in family takes (pgb_set_likelihood's), -1: no density here (callback, compiled, unknown) */
PGB_HD int pgb_logpdf_nparams(int family) {
  switch (family) {
    case PGB_FAMILY_NORMAL: case PGB_FAMILY_NEGBIN_LOG: case PGB_FAMILY_GAMMA_LOG: return 1;
    case PGB_FAMILY_ASYMLAPLACE: case PGB_FAMILY_STUDENT_T: return 2;
    case PGB_FAMILY_BERNOULLI_PROBIT: case PGB_FAMILY_BERNOULLI_LOGIT: case PGB_FAMILY_CATEGORICAL:
    case PGB_FAMILY_NORMAL_MEANSCALE: case PGB_FAMILY_POISSON_LOG: return 0;
    default: return -1;
  }
}
/* the outputs a family takes: 1 when K must be 1, 2 for mean/scale, 0: any K in [2, PGB_MAX_OUTPUTS] */
PGB_HD int pgb_logpdf_outputs(int family) {
  if (family == PGB_FAMILY_CATEGORICAL) return 0;
  return family == PGB_FAMILY_NORMAL_MEANSCALE ? 2 : 1;
}

/* q[0 .. PGB_PW_NPAR-1] of one draw from its params; 0, or 1 when a param is outside the family's domain (sigma, nu,
 * alpha, b > 0, 0 < q < 1, all finite) */
PGB_HD int pgb_logpdf_prepare(int family, const double* params, double* q, const pgb_lltabs* tb) {
  const int np = pgb_logpdf_nparams(family);
  for (int i = 0; i < PGB_PW_NPAR; ++i) q[i] = 0.0;
  if (np < 0) return 1;
  for (int i = 0; i < np; ++i) {
    if (!(params[i] - params[i] == 0.0) || !(params[i] > 0.0)) return 1;
    q[i] = params[i];
  }
  if (family == PGB_FAMILY_NORMAL) {
    q[1] = -pgb_log_t(q[0], tb->logt) - 9.1893853320467274e-01; /* log sqrt(2 pi) */
  } else if (family == PGB_FAMILY_NEGBIN_LOG || family == PGB_FAMILY_GAMMA_LOG) {
    q[1] = q[0] * pgb_log_t(q[0], tb->logt) - pgb_cl_lgamma(q[0], tb->logt);
  } else if (family == PGB_FAMILY_ASYMLAPLACE) {
    if (!(q[1] < 1.0)) return 1;
    q[2] = pgb_log_t((q[1] * (1.0 - q[1])) / q[0], tb->logt);
  } else if (family == PGB_FAMILY_STUDENT_T) {
    const double nu = q[1];
    q[2] = ((pgb_cl_lgamma(0.5 * (nu + 1.0), tb->logt) - pgb_cl_lgamma(0.5 * nu, tb->logt)) -
            0.5 * pgb_log_t(nu * 3.14159265358979323846, tb->logt)) - pgb_log_t(q[0], tb->logt);
    q[3] = -0.5 * (nu + 1.0);
  }
  return 0;
}

/* the log density before the clamp; mu holds K predictors (the offset included), q the draw's prepared row */
PGB_HD double pgb_logpdf_raw(int family, int K, double y, const double* mu, const double* q, const pgb_lltabs* tb) {
  if (family == PGB_FAMILY_NORMAL) {
    const double z = (y - mu[0]) / q[0];
    return q[1] - 0.5 * (z * z);
  }
  if (family == PGB_FAMILY_BERNOULLI_PROBIT) return pgb_lphi_t(y > 0.5 ? mu[0] : -mu[0], tb->lphi);
  if (family == PGB_FAMILY_BERNOULLI_LOGIT) return -pgb_softplus_t(y > 0.5 ? -mu[0] : mu[0], tb);
  if (family == PGB_FAMILY_CATEGORICAL) { /* pgb_loglik_cat_t's operations; the class is matched by compares */
    double mx = mu[0];
    for (int k = 1; k < K; ++k)
      if (mu[k] > mx) mx = mu[k];
    const int c = pgb_cat_class(K, y);
    double sum = 0.0, muc = mu[0];
    for (int k = 0; k < K; ++k) {
      sum += pgb_exp_t(mu[k] - mx, tb->expt);
      if (k == c) muc = mu[k];
    }
    if (!(sum >= 1.0)) return -2047.0;
    return (muc - mx) - pgb_log_pos_t(sum, tb->logt);
  }
  if (family == PGB_FAMILY_NORMAL_MEANSCALE) {
    double sd = mu[1] < 0.0 ? -mu[1] : mu[1];
    if (!(sd >= 1e-8)) sd = 1e-8;
    if (sd > 1.0e300) sd = 1.0e300;
    const double z = (y - mu[0]) / sd;
    return (-pgb_log_pos_t(sd, tb->logt) - 9.1893853320467274e-01) - 0.5 * (z * z);
  }
  if (family == PGB_FAMILY_POISSON_LOG || family == PGB_FAMILY_NEGBIN_LOG) {
    const double yy = y > 0.0 ? y : 0.0;
    const double em = pgb_exp_t(mu[0], tb->expt);
    const double lf = pgb_cl_lgamma(yy + 1.0, tb->logt);
    if (family == PGB_FAMILY_POISSON_LOG) return (yy * mu[0] - em) - lf;
    const double ay = q[0] + yy;
    return ((pgb_cl_lgamma(ay, tb->logt) - lf) + q[1]) + (yy * mu[0] - ay * pgb_log_t(q[0] + em, tb->logt));
  }
  if (family == PGB_FAMILY_GAMMA_LOG) {
    return (q[1] + (q[0] - 1.0) * pgb_log_t(y, tb->logt)) - q[0] * (y * pgb_exp_t(-mu[0], tb->expt) + mu[0]);
  }
  if (family == PGB_FAMILY_ASYMLAPLACE) {
    const double u = (y - mu[0]) / q[0];
    return q[2] - u * (u < 0.0 ? q[1] - 1.0 : q[1]);
  }
  if (family == PGB_FAMILY_STUDENT_T) {
    const double u = (y - mu[0]) / q[0];
    return q[2] + q[3] * pgb_log_t(1.0 + (u * u) / q[1], tb->logt);
  }
  return pgb_u2d(0x7FF8000000000000ull); /* no density: the lower bound, counted */
}
/* a value AT a bound counts: the probit table's clamp row returns exactly -2047 */
PGB_HD int pgb_pw_is_clamped(double raw) { return !(raw > -2047.0 && raw < 2047.0); }
PGB_HD double pgb_logpdf(int family, int K, double y, const double* mu, const double* q, const pgb_lltabs* tb) {
  return pgb_clamp_loglik(pgb_logpdf_raw(family, K, y, mu, q, tb));
}

/* ------------------------------------------------------------------ the reduction over draws of one row
 * Draws are taken in chunks of PGB_PW_CHUNK.  Inside a chunk, in draw order: a running (max, sum of exp(v - max))
 * on pgb_exp_t and Welford's (mean, M2).  Chunks are merged in chunk order by the one formula of pgb_pw_merge.  At the
 * end lppd = max + log(sum) - log(D) and var = M2 / (D - 1) (0 for D = 1).  A result is a function of the values and
 * PGB_PW_CHUNK alone, never of the launch geometry. */
typedef struct {
  double mx, s, mean, m2;
} pgb_pw_acc;
PGB_HD void pgb_pw_first(pgb_pw_acc* a, double v) {
  a->mx = v;
  a->s = 1.0;
  a->mean = v;
  a->m2 = 0.0;
}
/* the n-th value of the chunk (n >= 2) */
PGB_HD void pgb_pw_push(pgb_pw_acc* a, double v, int n, const double* expt) {
  if (v > a->mx) {
    a->s = a->s * pgb_exp_t(a->mx - v, expt) + 1.0;
    a->mx = v;
  } else {
    a->s = a->s + pgb_exp_t(v - a->mx, expt);
  }
  const double delta = v - a->mean;
  a->mean = a->mean + delta / (double)n;
  a->m2 = a->m2 + delta * (v - a->mean);
}
/* a (na values) followed by b (nb values) -> a */
PGB_HD void pgb_pw_merge(pgb_pw_acc* a, int na, const pgb_pw_acc* b, int nb, const double* expt) {
  if (b->mx > a->mx) {
    a->s = a->s * pgb_exp_t(a->mx - b->mx, expt) + b->s;
    a->mx = b->mx;
  } else {
    a->s = a->s + b->s * pgb_exp_t(b->mx - a->mx, expt);
  }
  const double n = (double)(na + nb);
  const double delta = b->mean - a->mean;
  a->mean = a->mean + delta * ((double)nb / n);
  a->m2 = (a->m2 + b->m2) + (delta * delta) * (((double)na * (double)nb) / n);
}
/* out3 = (lppd_i, mean_i, var_i) of D values */
PGB_HD void pgb_pw_finish(const pgb_pw_acc* a, int D, const pgb_lltabs* tb, double* out3) {
  out3[0] = (a->mx + pgb_log_t(a->s, tb->logt)) - pgb_log_t((double)D, tb->logt);
  out3[1] = a->mean;
  out3[2] = D > 1 ? a->m2 / (double)(D - 1) : 0.0;
}
/* the whole reduction of ll[d * stride], d < D: what the device's two kernels compute for a row */
PGB_HD void pgb_pw_reduce(const double* ll, int64_t stride, int D, const pgb_lltabs* tb, double* out3) {
  pgb_pw_acc tot;
  tot.mx = tot.s = tot.mean = tot.m2 = 0.0;
  int done = 0;
  for (int d0 = 0; d0 < D; d0 += PGB_PW_CHUNK) {
    const int d1 = d0 + PGB_PW_CHUNK < D ? d0 + PGB_PW_CHUNK : D;
    pgb_pw_acc c;
    pgb_pw_first(&c, ll[(int64_t)d0 * stride]);
    for (int d = d0 + 1; d < d1; ++d) pgb_pw_push(&c, ll[(int64_t)d * stride], d - d0 + 1, tb->expt);
    if (d0 == 0) tot = c;
    else pgb_pw_merge(&tot, done, &c, d1 - d0, tb->expt);
    done = d1;
  }
  pgb_pw_finish(&tot, D, tb, out3);
}

#endif /* PGBART_LOGPDF_H */
