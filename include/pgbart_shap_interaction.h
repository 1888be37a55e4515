/*
 * pgbart_shap_interaction.h -- the numeric contract of the exact SHAP interaction values of stored posterior draws:
 * for a forest d, an output k and a row x, how the attribution of pgbart_shap.h splits into main effects and the
 * shares of pairs of columns (pgb_predict_shap_interactions, below; pymc_bart_amd/shap_interaction.py).
 *
 * Definition.  The players are the p columns and v(S; x) is the value function of pgbart_shap.h.  For i != j
 *   Phi_ij = sum over S in P \ {i, j} of |S|! (p - |S| - 2)! / (2 (p - 1)!) * (v(S + ij) - v(S + i) - v(S + j) + v(S))
 *   Phi_ii = phi_i - sum over j != i of Phi_ij                                        (the main effect)
 * so Phi is symmetric, row i of it sums to phi_i and base + sum_ij Phi_ij is the plain prediction of the row.  A column
 * that reads NaN in the row is a null player: its row and its column of Phi are exactly 0.0.
 *
 * Leaf-wise form -- what is computed.  Slots, live, u, w, coef_k, the c recurrence, W and g_j mean exactly what they
 * mean in pgbart_shap.h, and the packer, the members, the leaf records, wtab, the groups, the NaN handling and the
 * regressor's slot are that header's, unchanged.  A term of a leaf (cw_k = coef_k * w) is a product game over its live
 * slots; per term:
 *   1. for every live slot e in slot order: r_e = g_e, by the statements of pgbart_shap.h (c over the live slots but e,
 *      s over row u of wtab, g = (o_e - z_e) * s).
 *   2. for every pair of live slots i < j, i ascending, j ascending inside i:
 *        c    the coefficients of prod over live e not in {i, j}, in slot order, of (z_e + o_e t), by the same top-down
 *             recurrence from c = [1, 0, ...] (recomputed per pair: nothing is ever divided out; the coefficient past
 *             t^(u - 2) is 0 and is not kept)
 *        s2   = 0.0, then s2 = s2 + W(u - 1, k) * c_k for k = 0 .. u - 2          (row u - 1 of wtab:
 *             k! (u - k - 2)! / (u - 1)! = W(u - 1, k))
 *        h    = 0.5 * (((o_i - z_i) * (o_j - z_j)) * s2)                           (bitwise symmetric in (i, j))
 *        r_i  = r_i - h, then r_j = r_j - h
 *        Phi[k][col_i][col_j] = Phi[k][col_i][col_j] + cw_k * h, then the same for Phi[k][col_j][col_i], k = 0 .. K - 1
 *      -- so r_e has lost h_ef for the live f != e in slot order of f, whatever e is.
 *   3. for every live slot e in slot order: Phi[k][col_e][col_e] = Phi[k][col_e][col_e] + cw_k * r_e, k = 0 .. K - 1.
 * A term never holds one column in two slots, so the cells of a term are distinct.  Phi starts at 0.0; the order of
 * trees, leaves and terms is that of pgb_shap_row.  No product is contracted with a sum (-ffp-contract=off).
 *
 * Column subset.  The evaluation takes pos[p]: a column's index among the q chosen ones, or -1.  A cell is added to
 * only when both its columns are chosen; r_e always runs over ALL live slots, chosen or not, so a main effect accounts
 * for every column.  What can reach no chosen cell (g_e of a column that is not chosen, h of a pair neither column of
 * which is) is not computed.  The additions into one cell are the same statements in the same order whatever the
 * subset and its order are: a subset's result is a bitwise slice of the full one.
 *
 * Cost and limit.  A term costs O(u^4): u^2 / 2 pairs, each a product of u factors of u coefficients.  Hence
 * PGB_SHAPX_MAX_U = 32: a history with a leaf whose slots -- its path's groups and a fresh regressor slot -- number
 * more is refused (PGB_E_INVALID) before anything is launched.  A leaf of at most PGB_SHAP_FAST_U slots runs the same
 * statements with every loop unrolled to that length: the same bits.
 *
 * Host and device compile pgb_shapx_row from this one text (PGB_HD).
 */
#ifndef PGBART_SHAP_INTERACTION_H
#define PGBART_SHAP_INTERACTION_H

#include "pgbart_shap.h"

#define PGB_SHAPX_MAX_U 32 /* the slots of a term an evaluation accepts (a term costs O(u^4)) */

/* the slots of a leaf record: its path's groups and the regressor's slot when it is a fresh one */
PGB_HD int pgb_shapx_leaf_slots(const pgb_shap_leaf* lf) {
  return lf->n_groups + (lf->svar >= 0 && lf->sgroup < 0 ? 1 : 0);
}

/* The bodies of a term -- see the head of the file -- for a slot j or a pair of slots i < j; `top`: the length their
 * loops run to (ns, or PGB_SHAP_FAST_U with the loops unrolled).  pp[e]: pos of slot e's column. */
#define PGB_SHAPX_W_(top, UNR)                                                                                        \
  UNR for (int k = 0; k < (top); ++k) {                                                                               \
    wk[k] = k < u ? wtab[u * PGB_SHAP_WSTRIDE + k] : 0.0;                                                             \
    wk2[k] = k < u - 1 ? wtab[(u - 1) * PGB_SHAP_WSTRIDE + k] : 0.0;                                                  \
  }

/* step 1: r_j = g_j */
#define PGB_SHAPX_G_(j, top, UNR)                                                                                     \
  do {                                                                                                                \
    r[j] = 0.0;                                                                                                       \
    if ((j) < ns && live[j] && pp[j] >= 0) {                                                                          \
      UNR for (int k = 0; k < (top); ++k) c[k] = 0.0;                                                                 \
      c[0] = 1.0;                                                                                                     \
      UNR for (int e = 0; e < (top); ++e) {                                                                           \
        if (e < ns && e != (j) && live[e]) {                                                                          \
          UNR for (int k = (top) - 1; k >= 1; --k) c[k] = c[k] * z[e] + c[k - 1] * o[e];                              \
          c[0] = c[0] * z[e];                                                                                         \
        }                                                                                                             \
      }                                                                                                               \
      double s = 0.0;                                                                                                 \
      UNR for (int k = 0; k < (top); ++k) {                                                                           \
        if (k < u) s = s + wk[k] * c[k];                                                                              \
      }                                                                                                               \
      r[j] = (o[j] - z[j]) * s;                                                                                       \
    }                                                                                                                 \
  } while (0)

/* step 2: the pair i < j */
#define PGB_SHAPX_PAIR_(i, j, top, UNR)                                                                               \
  do {                                                                                                                \
    if ((j) < ns && live[i] && live[j] && (pp[i] >= 0 || pp[j] >= 0)) {                                               \
      UNR for (int k = 0; k < (top) - 1; ++k) c[k] = 0.0;                                                             \
      c[0] = 1.0;                                                                                                     \
      UNR for (int e = 0; e < (top); ++e) {                                                                           \
        if (e < ns && e != (i) && e != (j) && live[e]) {                                                              \
          UNR for (int k = (top) - 2; k >= 1; --k) c[k] = c[k] * z[e] + c[k - 1] * o[e];                              \
          c[0] = c[0] * z[e];                                                                                         \
        }                                                                                                             \
      }                                                                                                               \
      double s2 = 0.0;                                                                                                \
      UNR for (int k = 0; k < (top) - 1; ++k) {                                                                       \
        if (k < u - 1) s2 = s2 + wk2[k] * c[k];                                                                       \
      }                                                                                                               \
      const double h = 0.5 * (((o[i] - z[i]) * (o[j] - z[j])) * s2);                                                  \
      r[i] = r[i] - h;                                                                                                \
      r[j] = r[j] - h;                                                                                                \
      if (pp[i] >= 0 && pp[j] >= 0) {                                                                                 \
        double* pij = Phi + ((int64_t)pp[i] * q + pp[j]) * ps;                                                        \
        double* pji = Phi + ((int64_t)pp[j] * q + pp[i]) * ps;                                                        \
        for (int k = 0; k < K; ++k) {                                                                                 \
          const double cw = (lin ? slope[k] * d : value[k]) * w;                                                      \
          pij[(int64_t)k * q * q * ps] = pij[(int64_t)k * q * q * ps] + cw * h;                                       \
          pji[(int64_t)k * q * q * ps] = pji[(int64_t)k * q * q * ps] + cw * h;                                       \
        }                                                                                                             \
      }                                                                                                               \
    }                                                                                                                 \
  } while (0)

/* step 3: the main effect of slot j */
#define PGB_SHAPX_DIAG_(j)                                                                                            \
  do {                                                                                                                \
    if ((j) < ns && live[j] && pp[j] >= 0) {                                                                          \
      double* pjj = Phi + ((int64_t)pp[j] * q + pp[j]) * ps;                                                          \
      for (int k = 0; k < K; ++k) {                                                                                   \
        const double cw = (lin ? slope[k] * d : value[k]) * w;                                                        \
        pjj[(int64_t)k * q * q * ps] = pjj[(int64_t)k * q * q * ps] + cw * r[j];                                      \
      }                                                                                                               \
    }                                                                                                                 \
  } while (0)

/* one term over ns slots, by loops */
#define PGB_SHAPX_TERM_(top)                                                                                          \
  do {                                                                                                                \
    PGB_SHAPX_W_(top, PGB_SHAP_NOUNROLL_)                                                                             \
    for (int j_ = 0; j_ < (top); ++j_) PGB_SHAPX_G_(j_, top, PGB_SHAP_NOUNROLL_);                                     \
    for (int i_ = 0; i_ < (top); ++i_)                                                                                \
      for (int j_ = i_ + 1; j_ < (top); ++j_) PGB_SHAPX_PAIR_(i_, j_, top, PGB_SHAP_NOUNROLL_);                       \
    for (int j_ = 0; j_ < (top); ++j_) PGB_SHAPX_DIAG_(j_);                                                           \
  } while (0)

/* ... and with every slot index a literal, the inner loops unrolled to PGB_SHAP_FAST_U: the same bodies in the same
 * order (the text is written out because an unroll directive gives up on a nest of this size) */
#if PGB_SHAP_FAST_U != 8
#error "PGB_SHAPX_TERM_FAST_ is written out for PGB_SHAP_FAST_U == 8"
#endif
#define PGB_SHAPX_GF_(j) PGB_SHAPX_G_(j, PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_)
#define PGB_SHAPX_PF_(i, j) PGB_SHAPX_PAIR_(i, j, PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_)
#define PGB_SHAPX_TERM_FAST_                                                                                          \
  do {                                                                                                                \
    PGB_SHAPX_W_(PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_)                                                                   \
    PGB_SHAPX_GF_(0); PGB_SHAPX_GF_(1); PGB_SHAPX_GF_(2); PGB_SHAPX_GF_(3);                                           \
    PGB_SHAPX_GF_(4); PGB_SHAPX_GF_(5); PGB_SHAPX_GF_(6); PGB_SHAPX_GF_(7);                                           \
    PGB_SHAPX_PF_(0, 1); PGB_SHAPX_PF_(0, 2); PGB_SHAPX_PF_(0, 3); PGB_SHAPX_PF_(0, 4);                               \
    PGB_SHAPX_PF_(0, 5); PGB_SHAPX_PF_(0, 6); PGB_SHAPX_PF_(0, 7);                                                    \
    PGB_SHAPX_PF_(1, 2); PGB_SHAPX_PF_(1, 3); PGB_SHAPX_PF_(1, 4); PGB_SHAPX_PF_(1, 5);                               \
    PGB_SHAPX_PF_(1, 6); PGB_SHAPX_PF_(1, 7);                                                                         \
    PGB_SHAPX_PF_(2, 3); PGB_SHAPX_PF_(2, 4); PGB_SHAPX_PF_(2, 5); PGB_SHAPX_PF_(2, 6); PGB_SHAPX_PF_(2, 7);          \
    PGB_SHAPX_PF_(3, 4); PGB_SHAPX_PF_(3, 5); PGB_SHAPX_PF_(3, 6); PGB_SHAPX_PF_(3, 7);                               \
    PGB_SHAPX_PF_(4, 5); PGB_SHAPX_PF_(4, 6); PGB_SHAPX_PF_(4, 7);                                                    \
    PGB_SHAPX_PF_(5, 6); PGB_SHAPX_PF_(5, 7);                                                                         \
    PGB_SHAPX_PF_(6, 7);                                                                                              \
    PGB_SHAPX_DIAG_(0); PGB_SHAPX_DIAG_(1); PGB_SHAPX_DIAG_(2); PGB_SHAPX_DIAG_(3);                                   \
    PGB_SHAPX_DIAG_(4); PGB_SHAPX_DIAG_(5); PGB_SHAPX_DIAG_(6); PGB_SHAPX_DIAG_(7);                                   \
  } while (0)

/* pos of every slot's column */
#define PGB_SHAPX_POS_(top, UNR)                                                                                      \
  do {                                                                                                                \
    UNR for (int e = 0; e < (top); ++e) {                                                                             \
      if (e < ns) pp[e] = pos[gv[e]];                                                                                 \
    }                                                                                                                 \
  } while (0)

/* The two terms of one leaf added to Phi[((k * q + a) * q + b) * ps].  The arguments are pgb_shap_leaf_eval's; pos[p]
 * and q: the column subset.  The leaf's slots number at most PGB_SHAPX_MAX_U (the caller has checked the history);
 * fast != 0 (at most PGB_SHAP_FAST_U of them): the unrolled loops -- the same statements, hence the same bits. */
PGB_HD void pgb_shapx_leaf_eval(const pgb_shap_leaf* lf, const pgb_shap_member* mem, const double* wtab, const double* value,
                                const double* slope, int K, const double* x, int64_t xs, int cont, int fast,
                                const int32_t* pos, int q, double* Phi, int64_t ps) {
  double z[PGB_SHAPX_MAX_U], o[PGB_SHAPX_MAX_U], c[PGB_SHAPX_MAX_U], wk[PGB_SHAPX_MAX_U], wk2[PGB_SHAPX_MAX_U];
  double r[PGB_SHAPX_MAX_U];
  int32_t gv[PGB_SHAPX_MAX_U], live[PGB_SHAPX_MAX_U], pp[PGB_SHAPX_MAX_U];
  const int ng = lf->n_groups;
  double w = 1.0;
  int u = 0, i = 0;
  if (fast) PGB_SHAP_GROUPS_(PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_);
  else PGB_SHAP_GROUPS_(ng, PGB_SHAP_NOUNROLL_);
  int ns = ng, lin = 0;
  double d = 0.0;
  for (int term = 0; term < 2; ++term) { /* (a loop, not two copies: the unrolled text is long) */
    if (term) {
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
    }
    if (fast) {
      PGB_SHAPX_POS_(PGB_SHAP_FAST_U, PGB_SHAP_UNROLL_);
      PGB_SHAPX_TERM_FAST_;
    } else {
      PGB_SHAPX_POS_(ns, PGB_SHAP_NOUNROLL_);
      PGB_SHAPX_TERM_(ns);
    }
  }
}

/* Phi[((k * q + a) * q + b) * ps], k < K, a, b < q, of the row x[j * xs] and the forest `forest` (m trees of the pool);
 * force_general != 0: no leaf takes the unrolled evaluation (for tests: the bits do not change) */
PGB_HD void pgb_shapx_row(const pgb_shap_view* v, const int32_t* forest, int m, const double* x, int64_t xs, int cont,
                          const int32_t* pos, int q, int force_general, double* Phi, int64_t ps) {
  const int K = v->K;
  for (int64_t e = 0; e < (int64_t)K * q * q; ++e) Phi[e * ps] = 0.0;
  for (int t = 0; t < m; ++t) {
    const int tr = forest[t];
    const int l1 = v->tree_leaf_off[tr + 1];
    for (int l = v->tree_leaf_off[tr]; l < l1; ++l) {
      const pgb_shap_leaf lf = v->leaf[l];
      const double* val = v->value + (size_t)lf.node * (size_t)K;
      const double* slo = v->slope ? v->slope + (size_t)lf.node * (size_t)K : 0;
      if (!force_general && pgb_shap_leaf_fast(&lf))
        pgb_shapx_leaf_eval(&lf, v->member + lf.first, v->wtab, val, slo, K, x, xs, cont, 1, pos, q, Phi, ps);
      else
        pgb_shapx_leaf_eval(&lf, v->member + lf.first, v->wtab, val, slo, K, x, xs, cont, 0, pos, q, Phi, ps);
    }
  }
}

/* the largest slot count over the leaf records of a pack (0: no leaf has a split on its path) */
static inline int pgb_shapx_pack_slots(const pgb_shap_pack* pk) {
  const pgb_shap_leaf* leaf = (const pgb_shap_leaf*)(pk->buf + pk->o_leaf);
  int top = 0;
  for (int64_t l = 0; l < pk->n_leaves; ++l) {
    const int s = pgb_shapx_leaf_slots(leaf + l);
    if (s > top) top = s;
  }
  return top;
}

#ifdef __cplusplus
extern "C" {
#endif
/* The interaction values of the forests picks_host[0 .. n_picks) at the rows of X_dev [n_rows][ldx], between the
 * columns cols_host[0 .. n_cols) (distinct, in [0, p); any order): out_dev [n_picks][K][n_cols][n_cols][n_rows] (device
 * memory) and base_host_out [n_picks][K] (host memory, pgb_shap_base).  HIP library only (both particle builds); not
 * part of pgbart.h.  Everything is validated before a launch: PGB_E_INVALID (the message names the argument) for what
 * pgb_predict_shap refuses, a null cols_host, n_cols < 1, a column outside [0, p) or named twice, a leaf of more than
 * PGB_SHAPX_MAX_U slots (the message gives the count and the limit) or an output whose size overflows.  The trees are
 * packed and uploaded once per call; the call returns when out_dev is written. */
int pgb_predict_shap_interactions(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                                  const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx, const int32_t* cols_host,
                                  int32_t n_cols, const int32_t* picks_host, int32_t n_picks, double* out_dev,
                                  double* base_host_out, void* stream);

/* With PGB_WALK_TIMING=1 in the environment (read per call) pgb_predict_shap_interactions puts its kernel between HIP
 * events; this reports the last such measurement of the calling thread in milliseconds (-1.0: none yet).  For
 * tools/shap_interaction_timing.py. */
int pgb_shap_interactions_kernel_ms(double* ms_out);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_SHAP_INTERACTION_H */
