/*
 * pgbart_shap.h -- the numeric contract of the exact Shapley attributions of stored posterior draws: for a forest d
 * (a row of forest_tree_idx), an output k and a row x, how much of pgb_predict's answer each of the p columns
 * accounts for (pgb_predict_shap, below; pymc_bart_amd/shap.py).
 *
 * Players and value.  The players are the p columns.  v(S; x) is what pgb_predict returns for the row with every
 * column OUTSIDE S excluded: a split on an excluded column -- or on a value that is NaN -- takes both subtrees,
 * weighted by the training counts of the two children ("path-dependent" TreeSHAP's conditional expectation).
 *
 *   phi_j    = sum over S in P \ {j} of |S|! (p - |S| - 1)! / p! * (v(S + {j}) - v(S))
 *   phi_base = v({})                    (it does not depend on the row)
 *   phi_base + sum_j phi_j = v(P)       (efficiency: the plain prediction of the row)
 *
 * Leaf-wise form -- what is computed.  A leaf is reached by a path of splits.  The path's splits are grouped by
 * column, the groups in order of first appearance on the path, path order inside a group.  For a group g on column j:
 *   z_g   the product, in path order, of the members' child fractions c_child / (c_left + c_right) -- the counts as
 *         doubles, the sum, one division; 0.0 when c_left + c_right == 0 (the walk adds nothing there).  The first
 *         member's fraction starts the product.
 *   o_g   1.0 when the row takes the path's side at EVERY member of the group, else 0.0; the test is the walk's own
 *         (`x <= v` under the continuous rule, pgb_go_left otherwise), so -0.0, infinities and subset codes behave as
 *         in pgb_predict.
 * A group whose column reads NaN in the row is marginalised in every coalition: the column is a null player (its
 * phi stays exactly 0.0), z_g is folded into the leaf's weight w (w = 1.0, then w = w * z_g in group order) and the
 * group leaves the set.  U: the groups that remain, u their number.  A leaf gives ONE TERM (coef_k = value_k) and,
 * when it regresses on a column s whose value is not NaN, a SECOND one (coef_k = slope_k * (x_s - xbar)) over the same
 * groups with s added as a member with o = 1, z = 0 behind the path's groups -- or, when s already has a group, with
 * that group's z set to 0.  For a term and a group j of its U:
 *   c        the coefficients of prod over e in U \ {j}, in group order, of (z_e + o_e t): c = [1, 0, ...]; per e, for
 *            k from the top down to 1: c_k = c_k * z_e + c_(k-1) * o_e, then c_0 = c_0 * z_e.  (Recomputed per j: no
 *            factor is ever divided out, z may be 0.)
 *   W(u, k)  = k! (u - k - 1)! / u! by pgb_shap_weights: W(u, 0) = 1 / u, W(u, k) = (W(u, k - 1) * k) / (u - k).
 *   s        = 0.0, then s = s + W(u, k) * c_k for k = 0 .. u - 1
 *   g        = (o_j - z_j) * s
 *   phi[k][j] = phi[k][j] + (coef_k * w) * g      for k = 0 .. K - 1
 * phi starts at 0.0; trees go in forest order, the leaves of a tree depth-first, left first, a leaf's first term
 * before its second, the groups of a term in order.  No product is contracted with a sum (-ffp-contract=off).  One
 * evaluation owns one (row, forest) from start to finish, so a result depends on the arguments only: never on the
 * launch geometry, on how a caller blocks rows, nor on where the accumulators live.
 *   base[k]  = 0.0, then base[k] = base[k] + value_k * (z_0 * z_1 * ... in group order; 1.0 without groups) per leaf
 *              in the same order.
 * Paths of up to PGB_MAX_DEPTH distinct columns work (u <= PGB_SHAP_MAX_U with a regressor added); an evaluation
 * whose slots number at most PGB_SHAP_FAST_U runs the same statements with every loop unrolled to that length.
 *
 * Host and device compile pgb_shap_row from this one text (PGB_HD); the packer is plain C on the host.
 */
#ifndef PGBART_SHAP_H
#define PGBART_SHAP_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "pgbart.h"
#include "pgbart_spec.h"

#define PGB_SHAP_MAX_U (PGB_MAX_DEPTH + 1) /* the slots of a term: the path's groups and the regressor */
#define PGB_SHAP_FAST_U 8                  /* at most this many slots: the unrolled evaluation */
#define PGB_SHAP_WSTRIDE PGB_SHAP_MAX_U    /* wtab[u * PGB_SHAP_WSTRIDE + k], u = 0 .. PGB_SHAP_MAX_U */
#define PGB_SHAP_WTAB ((PGB_SHAP_MAX_U + 1) * PGB_SHAP_WSTRIDE)

#define PGB_SHAP_HEAD 1 /* member flags: the first / the last member of its group */
#define PGB_SHAP_TAIL 2

/* one split of a leaf's path; the members of a leaf are stored group by group */
typedef struct {
  int32_t var;   /* the split column */
  int32_t rule;  /* PGB_RULE_* of the split node */
  int32_t side;  /* 0: the path goes left here, 1: right */
  int32_t flags; /* PGB_SHAP_HEAD | PGB_SHAP_TAIL */
  double split;
  double frac;   /* c_child / (c_left + c_right) of the child the path takes, 0.0 when the sum is 0 */
} pgb_shap_member;

typedef struct {
  int32_t node;      /* pool-wide index of the leaf (its K values, K slopes) */
  int32_t first;     /* its first member */
  int32_t n_members; /* = the leaf's depth */
  int32_t n_groups;
  int32_t svar;      /* the regressor's column, -1: a constant leaf (or a column X does not have) */
  int32_t sgroup;    /* the group of the path on svar, -1: none */
  double xbar;
} pgb_shap_leaf;

/* what an evaluation reads (host or device pointers) */
typedef struct {
  const int32_t* tree_leaf_off; /* [n_trees + 1]: tree t owns the leaf records [off[t], off[t + 1]) */
  const pgb_shap_leaf* leaf;
  const pgb_shap_member* member;
  const double* wtab;           /* [PGB_SHAP_WTAB] */
  const double* value;          /* [total_nodes][K] */
  const double* slope;          /* [total_nodes][K], NULL: no linear leaves */
  int32_t K;
} pgb_shap_view;

/* w[0 .. u) = W(u, .) */
PGB_HD void pgb_shap_weights(int u, double* w) {
  if (u < 1) return;
  double v = 1.0 / (double)u;
  w[0] = v;
  for (int k = 1; k < u; ++k) {
    v = (v * (double)k) / (double)(u - k);
    w[k] = v;
  }
}

#if defined(__clang__)
#define PGB_SHAP_UNROLL_ _Pragma("unroll")
#else
#define PGB_SHAP_UNROLL_
#endif
#define PGB_SHAP_NOUNROLL_

/* One term of a leaf over the slots 0 .. ns - 1 (live[e] == 0: the slot is not in U), u of them live.  `top`: the
 * length every loop runs to (ns, or PGB_SHAP_FAST_U with the loops unrolled).  coef_k = lin ? slope[k] * d : value[k]. */
#define PGB_SHAP_TERM_(top, UNR)                                                                                      \
  do {                                                                                                                \
    UNR for (int k = 0; k < (top); ++k) wk[k] = k < u ? wtab[u * PGB_SHAP_WSTRIDE + k] : 0.0;                         \
    UNR for (int j = 0; j < (top); ++j) {                                                                             \
      if (j < ns && live[j]) {                                                                                        \
        UNR for (int k = 0; k < (top); ++k) c[k] = 0.0;                                                               \
        c[0] = 1.0;                                                                                                   \
        UNR for (int e = 0; e < (top); ++e) {                                                                         \
          if (e < ns && e != j && live[e]) {                                                                          \
            UNR for (int k = (top) - 1; k >= 1; --k) c[k] = c[k] * z[e] + c[k - 1] * o[e];                            \
            c[0] = c[0] * z[e];                                                                                       \
          }                                                                                                           \
        }                                                                                                             \
        double s = 0.0;                                                                                               \
        UNR for (int k = 0; k < (top); ++k) {                                                                         \
          if (k < u) s = s + wk[k] * c[k];                                                                            \
        }                                                                                                             \
        const double g = (o[j] - z[j]) * s;                                                                           \
        double* pj = phi + (int64_t)gv[j] * ps;                                                                       \
        for (int k = 0; k < K; ++k) {                                                                                 \
          const double cw = (lin ? slope[k] * d : value[k]) * w;                                                      \
          pj[(int64_t)k * p * ps] = pj[(int64_t)k * p * ps] + cw * g;                                                 \
        }                                                                                                             \
      }                                                                                                               \
    }                                                                                                                 \
  } while (0)

/* The slots of the path's groups: z, o, the column and whether the row holds a value there; w and u. */
#define PGB_SHAP_GROUPS_(top, UNR)                                                                                    \
  do {                                                                                                                \
    UNR for (int g = 0; g < (top); ++g) {                                                                             \
      if (g < ng) {                                                                                                   \
        const int var = mem[i].var;                                                                                   \
        const double xv = x[(int64_t)var * xs];                                                                       \
        const int nan = xv != xv;                                                                                     \
        double zz = mem[i].frac;                                                                                      \
        int on = 1;                                                                                                   \
        for (;;) {                                                                                                    \
          const pgb_shap_member mb = mem[i];                                                                          \
          if (!(mb.flags & PGB_SHAP_HEAD)) zz = zz * mb.frac;                                                         \
          if (!nan) {                                                                                                 \
            const int left = cont ? xv <= mb.split : pgb_go_left(mb.rule, xv, mb.split);                              \
            on = on && ((left != 0) == (mb.side == 0));                                                               \
          }                                                                                                           \
          ++i;                                                                                                        \
          if (mb.flags & PGB_SHAP_TAIL) break;                                                                        \
        }                                                                                                             \
        z[g] = zz;                                                                                                    \
        o[g] = on ? 1.0 : 0.0;                                                                                        \
        gv[g] = var;                                                                                                  \
        live[g] = !nan;                                                                                               \
        if (nan) w = w * zz;                                                                                          \
        else ++u;                                                                                                     \
      }                                                                                                               \
    }                                                                                                                 \
  } while (0)

/* the regressor's slot: the z of slot `at` becomes 0; a fresh slot behind the groups has o = 1 */
#define PGB_SHAP_REGRESSOR_(top, UNR)                                                                                 \
  do {                                                                                                                \
    UNR for (int e = 0; e < (top); ++e) {                                                                             \
      if (e == at) {                                                                                                  \
        z[e] = 0.0;                                                                                                   \
        if (fresh) {                                                                                                  \
          o[e] = 1.0;                                                                                                 \
          gv[e] = lf->svar;                                                                                           \
          live[e] = 1;                                                                                                \
        }                                                                                                             \
      }                                                                                                               \
    }                                                                                                                 \
  } while (0)

/* The two terms of one leaf added to phi[(k * p + j) * ps].  x[j * xs]: the row; value, slope: the leaf's K values
 * and K slopes (slope NULL: none); cont != 0: every split of the pool follows the continuous rule; fast != 0 (the
 * leaf's slots number at most PGB_SHAP_FAST_U): the unrolled loops -- the same statements, hence the same bits. */
PGB_HD void pgb_shap_leaf_eval(const pgb_shap_leaf* lf, const pgb_shap_member* mem, const double* wtab, const double* value,
                               const double* slope, int K, const double* x, int64_t xs, int p, int cont, int fast,
                               double* phi, int64_t ps) {
  double z[PGB_SHAP_MAX_U], o[PGB_SHAP_MAX_U], c[PGB_SHAP_MAX_U], wk[PGB_SHAP_MAX_U];
  int32_t gv[PGB_SHAP_MAX_U], live[PGB_SHAP_MAX_U];
  const int ng = lf->n_groups;
  double w = 1.0;
  int u = 0, i = 0;
  if (fast) PGB_SHAP_GROUPS_(PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_);
  else PGB_SHAP_GROUPS_(ng, PGB_SHAP_NOUNROLL_);
  int ns = ng, lin = 0;
  double d = 0.0;
  if (fast) PGB_SHAP_TERM_(PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_);
  else PGB_SHAP_TERM_(ns, PGB_SHAP_NOUNROLL_);
  if (slope == 0 || lf->svar < 0) return;
  const double xr = x[(int64_t)lf->svar * xs];
  if (xr != xr) return;
  d = xr - lf->xbar;
  lin = 1;
  const int at = lf->sgroup >= 0 ? lf->sgroup : ng; /* the slot whose z becomes 0; a new one behind the groups */
  const int fresh = lf->sgroup < 0;
  if (fast) PGB_SHAP_REGRESSOR_(PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_);
  else PGB_SHAP_REGRESSOR_(ng + 1, PGB_SHAP_NOUNROLL_);
  if (fresh) {
    ns = ng + 1;
    ++u;
  }
  if (fast) PGB_SHAP_TERM_(PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_);
  else PGB_SHAP_TERM_(ns, PGB_SHAP_NOUNROLL_);
}

/* does the leaf take the unrolled evaluation? */
PGB_HD int pgb_shap_leaf_fast(const pgb_shap_leaf* lf) {
  return lf->n_groups + (lf->svar >= 0 && lf->sgroup < 0 ? 1 : 0) <= PGB_SHAP_FAST_U;
}

/* phi[(k * p + j) * ps], k < K, j < p, of the row x[j * xs] and the forest `forest` (m trees of the pool) */
PGB_HD void pgb_shap_row(const pgb_shap_view* v, const int32_t* forest, int m, const double* x, int64_t xs, int p, int cont,
                         double* phi, int64_t ps) {
  const int K = v->K;
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < p; ++j) phi[((int64_t)k * p + j) * ps] = 0.0;
  for (int t = 0; t < m; ++t) {
    const int tr = forest[t];
    const int l1 = v->tree_leaf_off[tr + 1];
    for (int l = v->tree_leaf_off[tr]; l < l1; ++l) {
      const pgb_shap_leaf lf = v->leaf[l];
      const double* val = v->value + (size_t)lf.node * (size_t)K;
      const double* slo = v->slope ? v->slope + (size_t)lf.node * (size_t)K : 0;
      if (pgb_shap_leaf_fast(&lf)) pgb_shap_leaf_eval(&lf, v->member + lf.first, v->wtab, val, slo, K, x, xs, p, cont, 1, phi, ps);
      else pgb_shap_leaf_eval(&lf, v->member + lf.first, v->wtab, val, slo, K, x, xs, p, cont, 0, phi, ps);
    }
  }
}

/* base[0 .. K) of the forest */
PGB_HD void pgb_shap_base(const pgb_shap_view* v, const int32_t* forest, int m, double* base) {
  const int K = v->K;
  for (int k = 0; k < K; ++k) base[k] = 0.0;
  for (int t = 0; t < m; ++t) {
    const int tr = forest[t];
    for (int l = v->tree_leaf_off[tr]; l < v->tree_leaf_off[tr + 1]; ++l) {
      const pgb_shap_leaf* lf = v->leaf + l;
      const pgb_shap_member* mem = v->member + lf->first;
      double zall = 1.0, zz = 1.0;
      int first = 1;
      for (int i = 0; i < lf->n_members; ++i) {
        zz = (mem[i].flags & PGB_SHAP_HEAD) ? mem[i].frac : zz * mem[i].frac;
        if (mem[i].flags & PGB_SHAP_TAIL) {
          zall = first ? zz : zall * zz;
          first = 0;
        }
      }
      for (int k = 0; k < K; ++k) base[k] = base[k] + v->value[(size_t)lf->node * (size_t)K + k] * zall;
    }
  }
}

/* ------------------------------------------------------------------ the packer (host, plain C) */
/* The leaf records of a VALIDATED pool (every tree walkable and no deeper than PGB_MAX_DEPTH: pred_validate), in ONE
 * buffer [wtab | member | leaf | tree_leaf_off] that is uploaded as it is. */
typedef struct {
  uint8_t* buf;
  size_t bytes, o_member, o_leaf, o_off;
  int64_t n_leaves, n_members;
  int32_t n_trees;
} pgb_shap_pack;

typedef struct {
  const pgb_tree_arrays* t;
  int32_t p, base, depth, lin;
  int32_t pvar[PGB_MAX_DEPTH], prule[PGB_MAX_DEPTH], pside[PGB_MAX_DEPTH];
  double psplit[PGB_MAX_DEPTH], pfrac[PGB_MAX_DEPTH];
  int64_t nl, nm;
  pgb_shap_leaf* leaf; /* NULL: count only */
  pgb_shap_member* member;
  int bad;
} pgb_shap_walk_;

static void pgb_shap_pack_rec_(pgb_shap_walk_* s, int k) {
  const pgb_tree_arrays* t = s->t;
  const int g = s->base + k;
  if (t->var[g] < 0) {
    if (s->leaf) {
      pgb_shap_leaf* lf = s->leaf + s->nl;
      pgb_shap_member* mb = s->member + s->nm;
      int32_t gcol[PGB_MAX_DEPTH];
      int ng = 0, nm = 0;
      for (int d = 0; d < s->depth; ++d) { /* the groups, in order of first appearance */
        int seen = 0;
        for (int e = 0; e < ng; ++e) seen |= gcol[e] == s->pvar[d];
        if (!seen) gcol[ng++] = s->pvar[d];
      }
      int js = s->lin ? t->svar[g] : -1;
      if (js < 0 || js >= s->p) js = -1;
      lf->node = g;
      lf->first = (int32_t)s->nm;
      lf->n_members = s->depth;
      lf->n_groups = ng;
      lf->svar = js;
      lf->sgroup = -1;
      lf->xbar = js >= 0 ? t->xbar[g] : 0.0;
      for (int e = 0; e < ng; ++e) {
        if (gcol[e] == js) lf->sgroup = e;
        int head = 1;
        for (int d = 0; d < s->depth; ++d) {
          if (s->pvar[d] != gcol[e]) continue;
          mb[nm].var = s->pvar[d];
          mb[nm].rule = s->prule[d];
          mb[nm].side = s->pside[d];
          mb[nm].flags = head ? PGB_SHAP_HEAD : 0;
          mb[nm].split = s->psplit[d];
          mb[nm].frac = s->pfrac[d];
          head = 0;
          ++nm;
        }
        mb[nm - 1].flags |= PGB_SHAP_TAIL;
      }
    }
    s->nl += 1;
    s->nm += s->depth;
    return;
  }
  if (s->depth >= PGB_MAX_DEPTH) {
    s->bad = 1;
    return;
  }
  const int l = t->left[g], r = t->right[g];
  const double cl = (double)t->count[s->base + l], cr = (double)t->count[s->base + r];
  const double tot = cl + cr;
  const int d = s->depth;
  s->pvar[d] = t->var[g];
  s->prule[d] = t->rule ? t->rule[g] : PGB_RULE_CONTINUOUS;
  s->psplit[d] = t->split[g];
  s->depth = d + 1;
  s->pside[d] = 0;
  s->pfrac[d] = tot > 0.0 ? cl / tot : 0.0;
  pgb_shap_pack_rec_(s, l);
  s->pside[d] = 1;
  s->pfrac[d] = tot > 0.0 ? cr / tot : 0.0;
  pgb_shap_pack_rec_(s, r);
  s->depth = d;
}

static inline void pgb_shap_pack_free(pgb_shap_pack* pk) {
  free(pk->buf);
  pk->buf = 0;
}

/* 0: packed (release with pgb_shap_pack_free); -1: out of memory; -2: a tree deeper than PGB_MAX_DEPTH, or more than
 * 2^31 - 1 members */
static inline int pgb_shap_pack_build(const pgb_tree_arrays* trees, int32_t p, pgb_shap_pack* pk) {
  pgb_shap_walk_ s;
  memset(&s, 0, sizeof s);
  memset(pk, 0, sizeof *pk);
  s.t = trees;
  s.p = p;
  s.lin = trees->slope && trees->xbar && trees->svar;
  for (int pass = 0; pass < 2; ++pass) {
    int32_t* off = 0;
    if (pass) {
      if (s.nm > 0x7fffffffLL) return -2;
      pk->n_leaves = s.nl;
      pk->n_members = s.nm;
      pk->n_trees = trees->n_trees;
      pk->o_member = sizeof(double) * (size_t)PGB_SHAP_WTAB;
      pk->o_leaf = pk->o_member + sizeof(pgb_shap_member) * (size_t)s.nm;
      pk->o_off = pk->o_leaf + sizeof(pgb_shap_leaf) * (size_t)s.nl;
      pk->bytes = pk->o_off + sizeof(int32_t) * ((size_t)trees->n_trees + 1);
      pk->buf = (uint8_t*)calloc(pk->bytes, 1);
      if (!pk->buf) return -1;
      double* wt = (double*)pk->buf;
      for (int u = 1; u <= PGB_SHAP_MAX_U; ++u) pgb_shap_weights(u, wt + (size_t)u * PGB_SHAP_WSTRIDE);
      s.member = (pgb_shap_member*)(pk->buf + pk->o_member);
      s.leaf = (pgb_shap_leaf*)(pk->buf + pk->o_leaf);
      off = (int32_t*)(pk->buf + pk->o_off);
    }
    s.nl = s.nm = 0;
    for (int t = 0; t < trees->n_trees; ++t) {
      if (off) off[t] = (int32_t)s.nl;
      s.base = trees->node_off[t];
      s.depth = 0;
      pgb_shap_pack_rec_(&s, 0);
      if (s.bad) {
        pgb_shap_pack_free(pk);
        return -2;
      }
    }
    if (off) off[trees->n_trees] = (int32_t)s.nl;
  }
  return 0;
}

/* the view of a pack through the pointer `at` its buffer is read from (pk->buf, or its copy on the device) */
static inline pgb_shap_view pgb_shap_pack_view(const pgb_shap_pack* pk, const uint8_t* at, const double* value,
                                               const double* slope, int32_t K) {
  pgb_shap_view v;
  v.wtab = (const double*)at;
  v.member = (const pgb_shap_member*)(at + pk->o_member);
  v.leaf = (const pgb_shap_leaf*)(at + pk->o_leaf);
  v.tree_leaf_off = (const int32_t*)(at + pk->o_off);
  v.value = value;
  v.slope = slope;
  v.K = K;
  return v;
}

#ifdef __cplusplus
extern "C" {
#endif
/* The attributions of the forests picks_host[0 .. n_picks) (rows of forest_tree_idx; picks may repeat) at the rows of
 * X_dev [n_rows][ldx] (device memory, row-major, p columns read): out_dev [n_picks][K][p][n_rows] (device memory, K =
 * trees->n_outputs) and base_host_out [n_picks][K] (host memory).  HIP library only (both particle builds); not part
 * of pgbart.h.  Everything is validated before a launch: PGB_E_INVALID (the message names the argument) for a null
 * pointer, n_forests / m / p / n_rows / n_picks < 1, ldx < p, a pick outside [0, n_forests), a malformed history
 * (pgb_predict's checks) or an output whose size overflows.  The trees are packed and uploaded once per call; the
 * call returns when out_dev is written. */
int pgb_predict_shap(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                     const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx, const int32_t* picks_host,
                     int32_t n_picks, double* out_dev, double* base_host_out, void* stream);

/* With PGB_WALK_TIMING=1 in the environment (read per call) pgb_predict_shap puts its kernel between HIP events; this
 * reports the last such measurement of the calling thread in milliseconds (-1.0: none yet).  For
 * tools/shap_timing.py. */
int pgb_shap_kernel_ms(double* ms_out);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_SHAP_H */
