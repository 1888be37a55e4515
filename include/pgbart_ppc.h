/*
 * pgbart_ppc.h -- the numeric contract of a REPLICATED OBSERVATION: one value y_rep drawn from a built-in family at
 * the linear predictor(s) of one (draw, row) pair (pgb_ppc_draw, below; pymc_bart_amd/predictive.py).
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /,
 * comparisons, integer operations, pgb_philox4x32_10, pgb_normal2, pgb_exp_t, pgb_log_t, pgb_lphi_t, pgb_softplus_t,
 * pgb_cl_lgamma and pgb_psis_sqrt (exp(log(x) / 2) and two Newton steps: the same vocabulary) -- no libm -- so that a
 * host evaluation checks the device kernel bit for bit.
 *
 * ADDRESSING.  A value is a function of (seed, d, i) and of its inputs, where d is the POSITION of the draw in the
 * call's draw list and i the GLOBAL row index -- never of blocking, launch geometry or the order of evaluation.  Every
 * random pair is one Philox block: key = seed; counter words (i low, i high, d, (purpose << 16) | attempt) -- the
 * fourth word as pgb_draw2 builds it.  The purposes (PGB_PPC_RNG_*, from 16 on) are disjoint from the sampler's
 * PGB_RNG_* (1 .. 6).  A block gives two uniforms: pgb_u01's [0, 1) where a comparison or Box-Muller takes them, and
 * the OPEN form (x + 0.5) 2^-53 of the same 53 bits (the largest, which rounds to 1, steps down to 1 - 2^-53) where a
 * logarithm does.
 *
 * FAMILIES (the prepared parameter row q[] is pgb_logpdf_prepare's, whose domain checks the callers reuse):
 *   NORMAL             mu + sigma z
 *   NORMAL_MEANSCALE   mu[0] + sd z, sd = |mu[1]| floored at 1e-8 and capped at 1e300 like pgb_logpdf_raw
 *   BERNOULLI_PROBIT   u < exp_t(lphi_t(mu))                  -> 1.0 / 0.0
 *   BERNOULLI_LOGIT    u < exp_t(-softplus_t(-mu))
 *   CATEGORICAL        inverse CDF over exp_t(mu_k - max) in class order: the first k with u S < e_0 + .. + e_k, the
 *                      last class is the fall-through           -> the class as a double
 *   ASYMLAPLACE        inverse CDF (Yu-Moyeed): u < q: mu + b / (1 - q) log(u / q), else mu - b / q log((1 - u) / (1 - q))
 *   GAMMA_LOG          exp(mu) G(alpha) / alpha
 *   STUDENT_T          mu + sigma z / sqrt(G(nu / 2) / (nu / 2))
 *   POISSON_LOG        Poisson(exp(mu))
 *   NEGBIN_LOG         Poisson(exp(mu) G(alpha) / alpha)
 * z: the first normal of pgb_normal2 of one pair.
 *
 * G(a): Marsaglia-Tsang.  a' = a (a >= 1) or a + 1; d = a' - 1/3, c = 1 / sqrt(9 d); attempt t takes z from one pair
 * and an open uniform U from another: v = (1 + c z)^3, accepted when v > 0 and log U < z^2 / 2 + d - d v + d log v;
 * the value is d v.  (The density of d v under acceptance is Gamma(a') for ANY c: the last ulp of the square root
 * costs acceptance rate, not exactness.)  a < 1: times U'^(1/a) = exp(log U' / a), U' open, of a pair of its own.  At
 * most PGB_PPC_MAX_TRIES attempts, every one with fresh counters; exhausted: d (the proposal's centre, v = 1), and
 * PGB_PPC_EXHAUSTED is set.
 *
 * Poisson(lam): lam > 2^30 is capped there (PGB_PPC_CAPPED).  Below PGB_PPC_POISSON_SWITCH: sequential-search
 * inversion of ONE uniform (p_0 = exp(-lam), p_k = p_(k-1) lam / k, the first k with u < p_0 + .. + p_k), at most
 * PGB_PPC_POISSON_STEPS steps (beyond: floor(lam), EXHAUSTED -- the sum's rounding leaves ~1e-15 of u uncovered).
 * At or above it: Hoermann's PTRS transformed rejection (1993) with its log-density test
 * log V + log(1 / alpha) - log(a / us^2 + b) <= -lam + k log lam - lgamma(k + 1), the same try cap, floor(lam) on
 * exhaustion.  (pgb_cl_lgamma is within 1e-13 relative: the acceptance probability of the ~10 % of attempts that reach
 * the test is off by at most 1e-13 lgamma(k + 1), 1e-6 at lam = 1e6.)
 *
 * A result that is not finite (GAMMA_LOG overflowing, a Student-t denominator that underflowed to 0) becomes
 * +-1.7976931348623157e308 (a NaN: 0.0) and sets PGB_PPC_CAPPED.  Flags are counted by every caller -- reported,
 * never silent, like n_clamped.
 *
 * SAMPLER BODIES (pgb_ppc_draw_compiled, below; the vocabulary is include/pgbart_compiled.h's).  A compiled
 * likelihood may carry a second C body, the inside of
 *     double r(double mu (or mu[0 .. K-1], K readable), double aux, const double <param>...)
 * which returns ONE replicated observation -- there is no y.  It calls the density vocabulary and, in sampler bodies
 * only, the random vocabulary:
 *   uniform()       pgb_u01 of a pair's first half, in [0, 1)
 *   uniform_open()  the open form of the same bits, in (0, 1)
 *   normal()        the first normal of pgb_normal2 of one pair
 *   gamma(a)        pgb_ppc_gamma       poisson(lam)    pgb_ppc_poisson
 *   sqrt(x)         pgb_psis_sqrt       floor(x)        pgb_ppc_floor       (the helpers the built-in samplers use)
 * The addressing rule above stands.  A body may call a random function more than once: the c-th call (c = 0, 1, ..
 * in execution order) of one KIND within one evaluation uses that kind's purpose(s) plus PGB_PPC_CALL_STRIDE c in the
 * purpose half of counter word 3.  The kinds: normal (purpose 16), uniform (17; uniform and uniform_open share the
 * counter), gamma (18 .. 20), poisson (21, 22).  The purposes 16 .. 22 stay distinct mod 32 and never meet the
 * sampler's 1 .. 6.  The offset is the `salt` of pgb_ppc_addr, added inside pgb_ppc_block; it is 0 for every built-in
 * family and for c = 0, so that a body which restates a built-in family's formula reproduces pgb_ppc_value of that
 * family bit for bit.  At most PGB_PPC_MAX_CALLS calls per kind per evaluation: beyond, a call draws nothing, returns
 * a fixed value -- normal 0.0, uniform and uniform_open 0.5, gamma(a) a, poisson(lam) floor(lam) -- and sets
 * PGB_PPC_EXHAUSTED.  ("Execution order" is C's: two calls of one kind inside ONE expression, normal() - normal(),
 * are unsequenced, and two compilers may number them differently -- the values are as good, but a body that must give
 * the same bits on the host and on the device puts such calls into statements of their own.)  A result that is not finite is capped and counted as PGB_PPC_CAPPED exactly as above.  The body
 * owns its domain: its params are finite, nothing else is checked.  Host and device compile the body from the one text
 * with -ffp-contract=off and no libm; the call counters and the flags live in a pgb_ppc_ctx the vocabulary macros
 * reach as pgb_cl_rng.
 *
 * A compiled likelihood without a sampler body, and the callback family, have a log density only, no sampler: they are
 * refused by name.
 */
#ifndef PGBART_PPC_H
#define PGBART_PPC_H

#include "pgbart_logpdf.h"
#include "pgbart_psis.h"

#ifndef PGB_PPC_MAX_TRIES
#define PGB_PPC_MAX_TRIES 32 /* attempts of a rejection sampler (a test build lowers it) */
#endif
#define PGB_PPC_POISSON_SWITCH 10.0  /* rates from here on: PTRS (its squeeze is proven for lam >= 10) */
#define PGB_PPC_POISSON_STEPS 256    /* inversion below the switch: P(k > 256 | lam < 10) < 1e-250 */
#define PGB_PPC_MAX_RATE 1073741824.0 /* 2^30 */
#define PGB_PPC_DBL_MAX 1.7976931348623157e308

#define PGB_PPC_CAPPED 1u
#define PGB_PPC_EXHAUSTED 2u

/* RNG purposes (high half of counter word 3): none of the sampler's PGB_RNG_* */
#define PGB_PPC_RNG_NORMAL 16u      /* z of the location-scale families                          */
#define PGB_PPC_RNG_UNIFORM 17u     /* u of the Bernoulli / categorical / Laplace inverse CDFs    */
#define PGB_PPC_RNG_GAMMA_Z 18u     /* Marsaglia-Tsang, attempt t: the normal                     */
#define PGB_PPC_RNG_GAMMA_U 19u     /* ... and the uniform of its test                            */
#define PGB_PPC_RNG_GAMMA_BOOST 20u /* a < 1: U'                                                  */
#define PGB_PPC_RNG_POISSON_INV 21u /* u of the inversion                                         */
#define PGB_PPC_RNG_POISSON_PTRS 22u /* PTRS, attempt t: (U, V)                                   */
#define PGB_PPC_RNG_FIRST 16u
#define PGB_PPC_RNG_LAST 22u
#define PGB_PPC_CALL_STRIDE 32u /* sampler bodies: the c-th call of a kind adds 32 c to its purposes */
#define PGB_PPC_MAX_CALLS 1024u /* ... and a kind has at most this many calls per evaluation (22 + 32 * 1023 < 2^16) */

typedef struct {
  uint32_t k0, k1; /* seed */
  uint32_t c0, c1; /* global row */
  uint32_t c2;     /* position of the draw */
  uint32_t salt;   /* added to every purpose: 0 but for the repeated calls of a sampler body */
} pgb_ppc_addr;

PGB_HD pgb_ppc_addr pgb_ppc_address(uint64_t seed, uint32_t draw_pos, uint64_t global_row) {
  pgb_ppc_addr a;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.c0 = (uint32_t)global_row;
  a.c1 = (uint32_t)(global_row >> 32);
  a.c2 = draw_pos;
  a.salt = 0u;
  return a;
}
PGB_HD pgb_u32x4 pgb_ppc_block(const pgb_ppc_addr* a, uint32_t purpose, uint32_t attempt) {
  return pgb_philox4x32_10(a->k0, a->k1, a->c0, a->c1, a->c2, ((purpose + a->salt) << 16) | (attempt & 0xFFFFu));
}
/* the pair in [0, 1) */
PGB_HD pgb_u2 pgb_ppc_pair(const pgb_ppc_addr* a, uint32_t purpose, uint32_t attempt) {
  const pgb_u32x4 x = pgb_ppc_block(a, purpose, attempt);
  pgb_u2 r;
  r.u0 = pgb_u01(x.v[0], x.v[1]);
  r.u1 = pgb_u01(x.v[2], x.v[3]);
  return r;
}
/* (x + 0.5) 2^-53 in (0, 1) */
PGB_HD double pgb_ppc_open(uint32_t hi, uint32_t lo) {
  const uint64_t x = (((uint64_t)hi << 32) | lo) >> 11;
  const double u = ((double)x + 0.5) * 1.1102230246251565404e-16;
  return u < 1.0 ? u : 0.99999999999999988898;
}
PGB_HD pgb_u2 pgb_ppc_pair_open(const pgb_ppc_addr* a, uint32_t purpose, uint32_t attempt) {
  const pgb_u32x4 x = pgb_ppc_block(a, purpose, attempt);
  pgb_u2 r;
  r.u0 = pgb_ppc_open(x.v[0], x.v[1]);
  r.u1 = pgb_ppc_open(x.v[2], x.v[3]);
  return r;
}
PGB_HD double pgb_ppc_normal(const pgb_ppc_addr* a, uint32_t purpose, uint32_t attempt) {
  const pgb_u2 u = pgb_ppc_pair(a, purpose, attempt);
  double z0, z1;
  pgb_normal2(u.u0, u.u1, &z0, &z1);
  return z0;
}

/* exp for any argument: the table exp is exact in its saturation only for |x| < 4.6e7 */
PGB_HD double pgb_ppc_exp(double x, const pgb_lltabs* tb) {
  if (x < -800.0) return 0.0;
  if (x > 800.0) return pgb_psis_inf();
  return pgb_exp_t(x, tb->expt);
}
/* floor of a finite x, as a double */
PGB_HD double pgb_ppc_floor(double x) {
  if (x >= 4503599627370496.0 || x <= -4503599627370496.0) return x;
  const double k = (double)(int64_t)x;
  return k > x ? k - 1.0 : k;
}

/* G(a), a > 0 finite */
PGB_HD double pgb_ppc_gamma(double a, const pgb_ppc_addr* ad, const pgb_lltabs* tb, uint32_t* flags) {
  const double a1 = a < 1.0 ? a + 1.0 : a;
  const double d = a1 - 0.33333333333333331;
  const double c = 1.0 / pgb_psis_sqrt(9.0 * d, tb);
  double g = d;
  int done = 0;
  for (int t = 0; t < PGB_PPC_MAX_TRIES && !done; ++t) {
    const double z = pgb_ppc_normal(ad, PGB_PPC_RNG_GAMMA_Z, (uint32_t)t);
    const double w = 1.0 + c * z;
    if (!(w > 0.0)) continue;
    const double v = (w * w) * w;
    const double U = pgb_ppc_pair_open(ad, PGB_PPC_RNG_GAMMA_U, (uint32_t)t).u0;
    if (pgb_log_t(U, tb->logt) < ((0.5 * (z * z) + d) - d * v) + d * pgb_log_t(v, tb->logt)) {
      g = d * v;
      done = 1;
    }
  }
  if (!done) *flags |= PGB_PPC_EXHAUSTED;
  if (a < 1.0) {
    const double U = pgb_ppc_pair_open(ad, PGB_PPC_RNG_GAMMA_BOOST, 0u).u0;
    g = g * pgb_ppc_exp(pgb_log_t(U, tb->logt) / a, tb);
  }
  return g;
}

/* Poisson(lam), lam >= 0 or NaN (-> the cap) */
PGB_HD double pgb_ppc_poisson(double lam, const pgb_ppc_addr* ad, const pgb_lltabs* tb, uint32_t* flags) {
  if (!(lam <= PGB_PPC_MAX_RATE)) {
    lam = PGB_PPC_MAX_RATE;
    *flags |= PGB_PPC_CAPPED;
  }
  if (lam < PGB_PPC_POISSON_SWITCH) {
    const double u = pgb_ppc_pair(ad, PGB_PPC_RNG_POISSON_INV, 0u).u0;
    double p = pgb_ppc_exp(-lam, tb), s = p, k = 0.0;
    for (int j = 1; j <= PGB_PPC_POISSON_STEPS; ++j) {
      if (u < s) return k;
      k = (double)j;
      p = p * (lam / k);
      s = s + p;
    }
    *flags |= PGB_PPC_EXHAUSTED;
    return pgb_ppc_floor(lam);
  }
  const double slam = pgb_psis_sqrt(lam, tb), loglam = pgb_log_t(lam, tb->logt);
  const double b = 0.931 + 2.53 * slam;
  const double a = -0.059 + 0.02483 * b;
  const double linva = pgb_log_t(1.1239 + 1.1328 / (b - 3.4), tb->logt);
  const double vr = 0.9277 - 3.6224 / (b - 2.0);
  for (int t = 0; t < PGB_PPC_MAX_TRIES; ++t) {
    const pgb_u2 uv = pgb_ppc_pair_open(ad, PGB_PPC_RNG_POISSON_PTRS, (uint32_t)t);
    const double U = uv.u0 - 0.5, V = uv.u1;
    const double us = 0.5 - (U < 0.0 ? -U : U);
    const double k = pgb_ppc_floor(((2.0 * a) / us + b) * U + (lam + 0.43));
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if ((pgb_log_t(V, tb->logt) + linva) - pgb_log_t(a / (us * us) + b, tb->logt) <=
        (k * loglam - lam) - pgb_cl_lgamma(k + 1.0, tb->logt))
      return k;
  }
  *flags |= PGB_PPC_EXHAUSTED;
  return pgb_ppc_floor(lam);
}

/* a value that is not finite: +-DBL_MAX (a NaN: 0.0), counted */
PGB_HD double pgb_ppc_cap(double v, uint32_t* flags) {
  if (!(v - v == 0.0)) {
    *flags |= PGB_PPC_CAPPED;
    v = v > 0.0 ? PGB_PPC_DBL_MAX : (v < 0.0 ? -PGB_PPC_DBL_MAX : 0.0);
  }
  return v;
}

/* One replicated observation.  mu: the K predictors (the offset included), finite; q: the draw's prepared row
 * (pgb_logpdf_prepare returned 0); flags: PGB_PPC_CAPPED / PGB_PPC_EXHAUSTED are OR-ed in.  A family without a sampler
 * gives 0.0 (the callers refuse it before). */
PGB_HD double pgb_ppc_value(int family, int K, const double* mu, const double* q, uint64_t seed, uint32_t draw_pos,
                            uint64_t global_row, const pgb_lltabs* tb, uint32_t* flags) {
  const pgb_ppc_addr ad = pgb_ppc_address(seed, draw_pos, global_row);
  double v = 0.0;
  if (family == PGB_FAMILY_NORMAL) {
    v = mu[0] + q[0] * pgb_ppc_normal(&ad, PGB_PPC_RNG_NORMAL, 0u);
  } else if (family == PGB_FAMILY_NORMAL_MEANSCALE) {
    double sd = mu[1] < 0.0 ? -mu[1] : mu[1];
    if (!(sd >= 1e-8)) sd = 1e-8;
    if (sd > 1.0e300) sd = 1.0e300;
    v = mu[0] + sd * pgb_ppc_normal(&ad, PGB_PPC_RNG_NORMAL, 0u);
  } else if (family == PGB_FAMILY_BERNOULLI_PROBIT) {
    const double u = pgb_ppc_pair(&ad, PGB_PPC_RNG_UNIFORM, 0u).u0;
    return u < pgb_exp_t(pgb_lphi_t(mu[0], tb->lphi), tb->expt) ? 1.0 : 0.0;
  } else if (family == PGB_FAMILY_BERNOULLI_LOGIT) {
    const double u = pgb_ppc_pair(&ad, PGB_PPC_RNG_UNIFORM, 0u).u0;
    return u < pgb_exp_t(-pgb_softplus_t(-mu[0], tb), tb->expt) ? 1.0 : 0.0;
  } else if (family == PGB_FAMILY_CATEGORICAL) {
    double mx = mu[0];
    for (int k = 1; k < K; ++k)
      if (mu[k] > mx) mx = mu[k];
    double sum = 0.0;
    for (int k = 0; k < K; ++k) sum = sum + pgb_exp_t(mu[k] - mx, tb->expt);
    const double target = pgb_ppc_pair(&ad, PGB_PPC_RNG_UNIFORM, 0u).u0 * sum;
    double cum = 0.0;
    int cls = K - 1;
    for (int k = 0; k < K - 1; ++k) {
      cum = cum + pgb_exp_t(mu[k] - mx, tb->expt);
      if (target < cum) {
        cls = k;
        break;
      }
    }
    return (double)cls;
  } else if (family == PGB_FAMILY_ASYMLAPLACE) {
    const double u = pgb_ppc_pair_open(&ad, PGB_PPC_RNG_UNIFORM, 0u).u0;
    if (u < q[1]) v = mu[0] + (q[0] / (1.0 - q[1])) * pgb_log_t(u / q[1], tb->logt);
    else v = mu[0] - (q[0] / q[1]) * pgb_log_t((1.0 - u) / (1.0 - q[1]), tb->logt);
  } else if (family == PGB_FAMILY_GAMMA_LOG) {
    v = (pgb_ppc_exp(mu[0], tb) * pgb_ppc_gamma(q[0], &ad, tb, flags)) / q[0];
  } else if (family == PGB_FAMILY_STUDENT_T) {
    const double h = 0.5 * q[1];
    const double w = pgb_ppc_gamma(h, &ad, tb, flags) / h;
    const double z = pgb_ppc_normal(&ad, PGB_PPC_RNG_NORMAL, 0u);
    if (w >= 2.2250738585072014e-308 && w <= PGB_PPC_DBL_MAX) v = mu[0] + (q[0] * z) / pgb_psis_sqrt(w, tb);
    else v = z < 0.0 ? -pgb_psis_inf() : pgb_psis_inf();
  } else if (family == PGB_FAMILY_POISSON_LOG) {
    return pgb_ppc_poisson(pgb_ppc_exp(mu[0], tb), &ad, tb, flags);
  } else if (family == PGB_FAMILY_NEGBIN_LOG) {
    return pgb_ppc_poisson((pgb_ppc_exp(mu[0], tb) * pgb_ppc_gamma(q[0], &ad, tb, flags)) / q[0], &ad, tb, flags);
  } else {
    return 0.0;
  }
  return pgb_ppc_cap(v, flags);
}

/* ---- sampler bodies: the state of ONE evaluation (the address, the tables, the flags, the calls so far of each kind)
 * and the random vocabulary on it.  The unit that compiles a body calls pgb_ppc_ctx_begin, the body, pgb_ppc_ctx_end. */
typedef struct {
  pgb_ppc_addr ad;
  const pgb_lltabs* tb;
  uint32_t flags;
  uint32_t n_normal, n_uniform, n_gamma, n_poisson;
} pgb_ppc_ctx;

PGB_HD void pgb_ppc_ctx_begin(pgb_ppc_ctx* c, uint64_t seed, uint32_t draw_pos, uint64_t global_row, const pgb_lltabs* tb) {
  c->ad = pgb_ppc_address(seed, draw_pos, global_row);
  c->tb = tb;
  c->flags = 0u;
  c->n_normal = c->n_uniform = c->n_gamma = c->n_poisson = 0u;
}
/* the body's value, capped; the evaluation's flags are OR-ed into *flags */
PGB_HD double pgb_ppc_ctx_end(pgb_ppc_ctx* c, double v, uint32_t* flags) {
  v = pgb_ppc_cap(v, &c->flags);
  *flags |= c->flags;
  return v;
}
/* the address of the next call of a kind; 0 (and EXHAUSTED) past the cap */
PGB_HD int pgb_ppc_ctx_next(pgb_ppc_ctx* c, uint32_t* calls, pgb_ppc_addr* a) {
  if (*calls >= PGB_PPC_MAX_CALLS) {
    c->flags |= PGB_PPC_EXHAUSTED;
    return 0;
  }
  *a = c->ad;
  a->salt = PGB_PPC_CALL_STRIDE * *calls;
  *calls = *calls + 1u;
  return 1;
}
PGB_HD double pgb_ppc_ctx_normal(pgb_ppc_ctx* c) {
  pgb_ppc_addr a;
  if (!pgb_ppc_ctx_next(c, &c->n_normal, &a)) return 0.0;
  return pgb_ppc_normal(&a, PGB_PPC_RNG_NORMAL, 0u);
}
PGB_HD double pgb_ppc_ctx_uniform(pgb_ppc_ctx* c) {
  pgb_ppc_addr a;
  if (!pgb_ppc_ctx_next(c, &c->n_uniform, &a)) return 0.5;
  return pgb_ppc_pair(&a, PGB_PPC_RNG_UNIFORM, 0u).u0;
}
PGB_HD double pgb_ppc_ctx_uniform_open(pgb_ppc_ctx* c) {
  pgb_ppc_addr a;
  if (!pgb_ppc_ctx_next(c, &c->n_uniform, &a)) return 0.5;
  return pgb_ppc_pair_open(&a, PGB_PPC_RNG_UNIFORM, 0u).u0;
}
PGB_HD double pgb_ppc_ctx_gamma(pgb_ppc_ctx* c, double shape) {
  pgb_ppc_addr a;
  if (!pgb_ppc_ctx_next(c, &c->n_gamma, &a)) return shape;
  return pgb_ppc_gamma(shape, &a, c->tb, &c->flags);
}
PGB_HD double pgb_ppc_ctx_poisson(pgb_ppc_ctx* c, double lam) {
  pgb_ppc_addr a;
  if (!pgb_ppc_ctx_next(c, &c->n_poisson, &a)) return pgb_ppc_floor(lam);
  return pgb_ppc_poisson(lam, &a, c->tb, &c->flags);
}

/* the mid-p comparison of the PIT counts: pit = (#below + 0.5 #equal) / D */
PGB_HD void pgb_ppc_compare(double yrep, double y, int* below, int* equal) {
  *below = yrep < y ? 1 : 0;
  *equal = yrep == y ? 1 : 0;
}

typedef struct {
  int32_t family;            /* a built-in family of pgbart_spec.h; the callback and compiled families are refused */
  int32_t n_params;          /* params per draw: the family's (pgb_logpdf_nparams) */
  const double* params_host; /* [D][n_params], host memory (NULL when n_params = 0) */
  const double* offset_dev;  /* [K][ld] added to the predictors, or NULL */
} pgb_ppc_lik;

/* A compiled likelihood's sampler body for pgb_ppc_draw_compiled. */
typedef struct {
  const void* code_object;   /* a gfx950 code object built as a sampler object: k_ppc_compiled, layout mark 2 */
  int64_t code_bytes;
  int32_t n_params;          /* params per draw: what the body declares */
  const double* params_host; /* [D][n_params], host memory, finite (NULL when n_params = 0) */
  const double* offset_dev;  /* [K][ld] added to the predictors, or NULL */
  const double* aux_dev;     /* [n_rows] the body's aux column, or NULL (aux = 0.0) */
} pgb_ppc_code;

#ifdef __cplusplus
extern "C" {
#endif
/* Replicated observations of the device matrix mu_dev [D][K][ld] as pgb_predict writes it (HIP library only, both
 * particle builds; not part of pgbart.h): element (d, i), i < n_rows, is pgb_ppc_value at draw position d and global
 * row row0 + i, of the predictors mu[d][.][i] + offset[.][i] and the parameter row of draw d.
 *   out_dev         [D][ld_out] the values, or NULL.  out_dev == mu_dev is allowed exactly when K == 1 and
 *                   ld_out == ld (every element is read before it is written, by the same thread); any other overlap
 *                   of the two ranges is refused.
 *   y_dev           [n_rows] observed values and pit_counts_dev [2][n_rows] (int32, ZEROED by the caller): the number
 *                   of draws with y_rep < y and with y_rep == y are ADDED; both or neither.
 *   flags_host      [2]: the number of (draw, row) pairs that set PGB_PPC_CAPPED and PGB_PPC_EXHAUSTED.
 * Everything is validated before a launch (PGB_E_INVALID with a message naming the argument: a null pointer, D < 1,
 * n_rows < 1, ld < n_rows, ld_out < n_rows, a family without a sampler, a wrong n_params, a K the family does not
 * take, the params of a draw outside the family's domain, overlapping ranges, no output).  mu (and the offset) must be
 * finite with |mu + offset| < 4.6e7, which pgb_predict's output and an offset within PGB_MAX_OFFSET are.  The call
 * returns when the outputs are written. */
int pgb_ppc_draw(const double* mu_dev, int32_t D, int32_t K, int64_t n_rows, int64_t ld, int64_t row0,
                 const pgb_ppc_lik* lik, uint64_t seed, double* out_dev, int64_t ld_out, const double* y_dev,
                 int32_t* pit_counts_dev, int64_t* flags_host, void* stream);
/* The same call with the sampler body of a compiled likelihood at the evaluation site (HIP library only, both particle
 * builds; not part of pgbart.h): every argument rule of pgb_ppc_draw, and element (d, i) is the body's value at the
 * predictors mu[d][.][i] + offset[.][i], aux[i] and the params of draw d, under the addressing of SAMPLER BODIES above.
 * The code object is loaded per call and checked before any launch, each message naming both sides: the ELF header,
 * the kernel, the layout record's magic, its mark (2: a pass-kernel or pointwise object is refused), the headers hash,
 * n_params, the body's outputs against K, finite params.  pgb_ppc_draw keeps refusing the compiled family;
 * pgb_pointwise_loglik and pgb_set_loglik_code refuse a sampler object. */
int pgb_ppc_draw_compiled(const double* mu_dev, int32_t D, int32_t K, int64_t n_rows, int64_t ld, int64_t row0,
                          const pgb_ppc_code* code, uint64_t seed, double* out_dev, int64_t ld_out, const double* y_dev,
                          int32_t* pit_counts_dev, int64_t* flags_host, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_PPC_H */
