/*
 * pgbart_hstat.h -- the numeric contract of Friedman & Popescu's H-statistic of stored posterior draws: per forest and
 * output, the share of the variance of the two-way partial dependence of a pair of columns that the two one-way
 * functions do not explain, and the one-column form "a against everything else" (pgb_hstat_*, below;
 * pymc_bart_amd/hstat.py).  Nothing of size rows x rows, nor draws x rows, is ever formed.
 *
 * Two observations.
 *   Only common trees matter.  PD_S(x) is the partial dependence on the column set S at the values x holds there: the
 *   mean over the background rows r of the prediction of the hybrid row "x on S, x_r elsewhere".  The use lists are
 *   pgb_permimp_pack_build's (pgbart_permimp.h; nothing of them is restated here).  L_a is the list of column a of a
 *   pick; L_ab the trees in both L_a and L_b, in forest order, a tree the forest names twice listed twice.
 *       Write f = sum over the trees t of f_t and I_ab(x) = PD_ab(x) - PD_a(x) - PD_b(x) + PD_0, tree by tree.
 *       A tree that does not use b has PD_ab,t = PD_a,t and PD_b,t = PD_0,t, so its I_ab,t = 0; the same for a.
 *       Hence I_ab is the sum over L_ab alone, and PD_ab = PD_a + PD_b + I_ab - PD_0 over the FULL forest, where
 *       PD_a - PD_0 is the sum over L_a alone: no tree outside the lists is ever walked.
 *   A leaf factorises.  The leaf records are pgb_shap_pack's (pgbart_shap.h): the path's splits grouped by column.
 *   The weight with which a hybrid row reaches a leaf is a product over the groups, each factor depending on x alone
 *   or on x_r alone, so the mean over r is taken once per leaf (the background moments) and not once per x.
 *
 * Per-leaf factors.  For a leaf, a row x and a group g on column j: phi_g(x) = o_g (1.0 or 0.0, the walk's own test at
 * every member, pgbart_shap.h's o) when x holds a value in column j, and z_g (pgbart_shap.h's z, 0.0 where both child
 * counts are 0) when it holds a NaN.  in_S = 1.0, then in_S = in_S * phi_g for the groups on columns in S, in group
 * order; out_S the same over the other groups.  (pgb_hstat_leaf_factors.)
 *
 * Jobs and subsets.  A COLUMN job (pick d, column a, b = -1) runs over L_a with the subsets 0: {}, 1: {a},
 * 2: everything but a.  A PAIR job (pick d, columns a, b) runs over L_ab with 0: {}, 1: {a}, 2: {b}, 3: {a, b}.  The
 * jobs of a call are numbered d * (q + n_pairs) + s for slot s of cols and d * (q + n_pairs) + q + j for pair j; a
 * pair names two SLOTS of cols.  A leaf of a listed tree is one SLOT of the moment workspace; the slots of a job are
 * its trees in list order, the leaves of a tree depth-first, left first (the packer's order).
 *
 * Background moments, per (slot, subset j), over the background rows r with weights v_r >= 0:
 *   M0_j = sum_r v_r * out_j(r)                                             (one rounding per term)
 *   M1_j = sum_r v_r * (out_j(r) * d_r), d_r = x_rs - xbar, 0.0 for a NaN   (only where the leaf regresses on a column
 *          s OUTSIDE subset j; a NaN regressor is the constant leaf, pgb_pred_walk.h's rule)
 *   V    = sum_r v_r
 * all LANE SUMS (pgbart_rowreduce.h's convention, not restated): 64 partials by r mod 64, r the row's index in the
 * whole background matrix, ascending row order, then added in the order l = 0 .. 63 (pgb_rowsum_lanes).
 *   B0_j = M0_j / V;  B1_j = M1_j / V.
 * A leaf with no group outside S adds v_r * 1.0 = v_r where V adds v_r, so its B0 is V / V == 1.0 exactly.
 *
 * Per-row values of a job at the evaluation row i, output k.  pd_j = 0.0; then, trees in list order, leaves in slot
 * order:
 *   e    = pgb_leaf_pred(value_k, slope_k, xbar, x_is) when the leaf regresses on s, s is in subset j and x_is is not
 *          NaN; value_k otherwise
 *   t    = e * B0_j;  and where the leaf regresses on s outside subset j:  t = t + slope_k * B1_j
 *   pd_j = pd_j + in_j(i) * t
 *   g    = the walk's sum over the list at the row itself: the A of pgbart_permimp.h (a column job only).
 *   column:  J_a  = pd_1 - pd_0;            T_a = ((g - pd_1) - pd_2) + pd_0
 *   pair:    I_ab = ((pd_3 - pd_1) - pd_2) + pd_0;   U_ab = (J_a + J_b) + I_ab   (J of the two column jobs)
 * Two facts hold EXACTLY by this order.  (1) A column whose listed trees split and regress on nothing else: every leaf
 * has B0_1 == 1.0, in_1 is the walk's own weight (1.0 * f == f) and the leaves are added in the walk's order, so
 * pd_1 == g and g - pd_1 == +0.0; subset 2 has no group inside and all outside exactly as subset 0 has, so
 * pd_2 == pd_0 bit for bit and (+0.0 - c) + c == +0.0: T_a == +0.0 at every row.  (2) An empty L_ab leaves every pd at
 * 0.0 and I_ab = ((0.0 - 0.0) - 0.0) + 0.0 == +0.0.
 *
 * Row reductions over the evaluation rows with weights w_i >= 0: per (job, k) the lane sums (i mod 64, i the row's
 * index in the whole matrix; blocks start at multiples of 64) of pgb_rowred_term1(w, u) and pgb_rowred_term2(w, u)
 * for u = J_a and u = T_a (column) or u = I_ab and u = U_ab (pair); W = sum_i w_i the same way.
 *
 * Finish, sequentially per (job, k):  var(u) = S2 / W - (S1 / W) * (S1 / W), and 0.0 where that is < 0.0
 * (pgb_rowred_finish_one's clamp).
 *   main_var = var(J_a);  total_inter_var = var(T_a);  h2_total = total_inter_var / var_fit
 *   inter_var = var(I_ab);  h2 = inter_var / var(U_ab)
 * var_fit is pgb_row_reduce's of a pgb_predict block (the caller's).  A numerator that is exactly 0.0 gives 0.0
 * whatever the denominator; otherwise the plain division: an infinity or a NaN stays and is counted in n_nonfinite.
 *
 * Workspace (doubles): rpart[n_jobs][K][4][64] | wpart[64] | vpart[64] | V | mpart[n_slots][8][64] | B[n_slots][8]
 * (the sums of a slot: M0_0 .. M0_3, M1_0 .. M1_3).  pgb_hstat_ws_layout.
 *
 * Limits: a leaf has at most PGB_HSTAT_MAX_U = PGB_SHAP_MAX_U groups (the packer's); a call takes at most
 * PGB_HSTAT_MAX_PAIRS pairs; the slots of a call stay below 2^31 / 8.  Host and device compile every PGB_HD function
 * below from this one text under -ffp-contract=off.
 */
#ifndef PGBART_HSTAT_H
#define PGBART_HSTAT_H

#include "pgbart_permimp.h"
#include "pgbart_rowreduce.h"
#include "pgbart_shap.h"

#define PGB_HSTAT_MAX_U PGB_SHAP_MAX_U
#define PGB_HSTAT_MAX_PAIRS 4096
#define PGB_HSTAT_LANES PGB_ROWRED_LANES
#define PGB_HSTAT_SLOT_SUMS 8 /* M0 of the four subsets, then M1 */
#define PGB_HSTAT_ROW_SUMS 4  /* S1, S2 of the first value, S1, S2 of the second */

typedef struct {
  int64_t o_rpart, o_wpart, o_vpart, o_V, o_mpart, o_B, words;
} pgb_hstat_layout;

PGB_HD pgb_hstat_layout pgb_hstat_ws_layout(int64_t n_jobs, int K, int64_t n_slots) {
  pgb_hstat_layout L;
  L.o_rpart = 0;
  L.o_wpart = n_jobs * K * PGB_HSTAT_ROW_SUMS * PGB_HSTAT_LANES;
  L.o_vpart = L.o_wpart + PGB_HSTAT_LANES;
  L.o_V = L.o_vpart + PGB_HSTAT_LANES;
  L.o_mpart = L.o_V + 1;
  L.o_B = L.o_mpart + n_slots * PGB_HSTAT_SLOT_SUMS * PGB_HSTAT_LANES;
  L.words = L.o_B + n_slots * PGB_HSTAT_SLOT_SUMS;
  return L;
}

/* what an evaluation reads of the jobs (host or device pointers) */
typedef struct {
  const int32_t* tree_off; /* [n_jobs + 1]: job e lists tree[tree_off[e] .. tree_off[e + 1]) */
  const int32_t* slot_off; /* [n_jobs + 1]: its first slot of the moment workspace */
  const int32_t* a;        /* [n_jobs]: the column */
  const int32_t* b;        /* [n_jobs]: the second column of a pair job, -1 for a column job */
  const int32_t* tree;
} pgb_hstat_plan_view;

PGB_HD int pgb_hstat_nsub(int b) { return b >= 0 ? 4 : 3; }
/* does column s (a leaf's regressor) lie in subset j of a job (a, b)? */
PGB_HD int pgb_hstat_inside(int s, int a, int b, int j) {
  if (j == 0) return 0;
  if (j == 1) return s == a;
  if (b >= 0) return j == 2 ? s == b : (s == a || s == b);
  return s != a;
}

/* in[j], out[j], j < 4, of one leaf at the row x[col * xs] for the job (a, b) */
PGB_HD void pgb_hstat_leaf_factors(const pgb_shap_leaf* lf, const pgb_shap_member* mem, const double* x, int64_t xs, int cont,
                                   int a, int b, double* in, double* out) {
  for (int j = 0; j < 4; ++j) in[j] = out[j] = 1.0;
  int i = 0;
  for (int g = 0; g < lf->n_groups; ++g) {
    const int var = mem[i].var;
    const double xv = x[(int64_t)var * xs];
    const int nan = xv != xv;
    double zz = mem[i].frac;
    int on = 1;
    for (;;) {
      const pgb_shap_member mb = mem[i];
      if (!(mb.flags & PGB_SHAP_HEAD)) zz = zz * mb.frac;
      if (!nan) {
        const int left = cont ? xv <= mb.split : pgb_go_left(mb.rule, xv, mb.split);
        on = on && ((left != 0) == (mb.side == 0));
      }
      ++i;
      if (mb.flags & PGB_SHAP_TAIL) break;
    }
    const double f = nan ? zz : (on ? 1.0 : 0.0);
    const int is_a = var == a, is_b = var == b;
    out[0] = out[0] * f;
    if (is_a) in[1] = in[1] * f;
    else out[1] = out[1] * f;
    if (b >= 0) {
      if (is_b) in[2] = in[2] * f;
      else out[2] = out[2] * f;
      if (is_a || is_b) in[3] = in[3] * f;
      else out[3] = out[3] * f;
    } else {
      if (is_a) out[2] = out[2] * f;
      else in[2] = in[2] * f;
    }
  }
}

/* One background row of weight v added to the sums of one slot: part[j * 64] is the row's lane partial of sum j.
 * lin != 0: the pool has linear leaves. */
PGB_HD void pgb_hstat_bg_leaf(const pgb_shap_leaf* lf, const pgb_shap_member* mem, int lin, const double* x, int64_t xs,
                              int cont, int a, int b, double v, double* part) {
  double in[4], out[4];
  pgb_hstat_leaf_factors(lf, mem, x, xs, cont, a, b, in, out);
  const int reg = lin && lf->svar >= 0;
  double d = 0.0;
  if (reg) {
    const double xr = x[(int64_t)lf->svar * xs];
    d = xr != xr ? 0.0 : xr - lf->xbar;
  }
  const int nsub = pgb_hstat_nsub(b);
  for (int j = 0; j < nsub; ++j) {
    part[j * PGB_HSTAT_LANES] = part[j * PGB_HSTAT_LANES] + v * out[j];
    if (reg && !pgb_hstat_inside(lf->svar, a, b, j))
      part[(4 + j) * PGB_HSTAT_LANES] = part[(4 + j) * PGB_HSTAT_LANES] + v * (out[j] * d);
  }
}

/* all background rows of one tile position l (l = row mod 64) for the trees of one job */
PGB_HD void pgb_hstat_bg_job_row(const pgb_shap_view* v, const int32_t* trees, int n_trees, int a, int b, const double* x,
                                 int64_t xs, int cont, double vw, double* part) {
  const int lin = v->slope != 0;
  for (int t = 0; t < n_trees; ++t) {
    const int tr = trees[t];
    const int l1 = v->tree_leaf_off[tr + 1];
    for (int l = v->tree_leaf_off[tr]; l < l1; ++l) {
      const pgb_shap_leaf lf = v->leaf[l];
      pgb_hstat_bg_leaf(&lf, v->member + lf.first, lin, x, xs, cont, a, b, vw, part);
      part += PGB_HSTAT_SLOT_SUMS * PGB_HSTAT_LANES;
    }
  }
}

/* B[8] of one slot from its finished V */
PGB_HD void pgb_hstat_slot_finish(const double* part, double V, double* B) {
  for (int j = 0; j < PGB_HSTAT_SLOT_SUMS; ++j) B[j] = pgb_rowsum_lanes(part + j * PGB_HSTAT_LANES) / V;
}

/* pd[j * K + k], j < 4, of one job at the row x[col * xs]; B: the job's first slot of B[n_slots][8] */
PGB_HD void pgb_hstat_job_row(const pgb_shap_view* v, const int32_t* trees, int n_trees, const double* B, int a, int b,
                              const double* x, int64_t xs, int cont, double* pd) {
  const int K = v->K;
  const int nsub = pgb_hstat_nsub(b);
  for (int j = 0; j < 4 * K; ++j) pd[j] = 0.0;
  for (int t = 0; t < n_trees; ++t) {
    const int tr = trees[t];
    const int l1 = v->tree_leaf_off[tr + 1];
    for (int l = v->tree_leaf_off[tr]; l < l1; ++l) {
      const pgb_shap_leaf lf = v->leaf[l];
      double in[4], out[4];
      pgb_hstat_leaf_factors(&lf, v->member + lf.first, x, xs, cont, a, b, in, out);
      const int reg = v->slope != 0 && lf.svar >= 0;
      double xr = 0.0;
      int have = 0;
      if (reg) {
        xr = x[(int64_t)lf.svar * xs];
        have = !(xr != xr);
      }
      const double* val = v->value + (size_t)lf.node * (size_t)K;
      const double* slo = reg ? v->slope + (size_t)lf.node * (size_t)K : 0;
      for (int j = 0; j < nsub; ++j) {
        const int inside = reg && pgb_hstat_inside(lf.svar, a, b, j);
        for (int k = 0; k < K; ++k) {
          const double e = inside && have ? pgb_leaf_pred(val[k], slo[k], lf.xbar, xr) : val[k];
          double tt = e * B[j];
          if (reg && !inside) tt = tt + slo[k] * B[4 + j];
          pd[j * K + k] = pd[j * K + k] + in[j] * tt;
        }
      }
      B += PGB_HSTAT_SLOT_SUMS;
    }
  }
}

PGB_HD double pgb_hstat_J(const double* pd, int K, int k) { return pd[1 * K + k] - pd[k]; }
PGB_HD double pgb_hstat_T(const double* pd, int K, int k, double g) { return ((g - pd[1 * K + k]) - pd[2 * K + k]) + pd[k]; }
PGB_HD double pgb_hstat_I(const double* pd, int K, int k) { return ((pd[3 * K + k] - pd[1 * K + k]) - pd[2 * K + k]) + pd[k]; }
PGB_HD double pgb_hstat_U(double ja, double jb, double i) { return (ja + jb) + i; }

/* the row of weight w added to the four lane partials rp[0], rp[64], rp[128], rp[192] of a (job, k) */
PGB_HD void pgb_hstat_row_add(double* rp, double w, double u1, double u2) {
  rp[0] = rp[0] + pgb_rowred_term1(w, u1);
  rp[PGB_HSTAT_LANES] = rp[PGB_HSTAT_LANES] + pgb_rowred_term2(w, u1);
  rp[2 * PGB_HSTAT_LANES] = rp[2 * PGB_HSTAT_LANES] + pgb_rowred_term1(w, u2);
  rp[3 * PGB_HSTAT_LANES] = rp[3 * PGB_HSTAT_LANES] + pgb_rowred_term2(w, u2);
}

PGB_HD double pgb_hstat_var(double s1, double s2, double W) {
  const double m1 = s1 / W;
  double var = s2 / W - m1 * m1;
  if (var < 0.0) var = 0.0;
  return var;
}
PGB_HD double pgb_hstat_ratio(double num, double den) { return num == 0.0 ? 0.0 : num / den; }

/* ------------------------------------------------------------------ the whole evaluation, sequentially (the reference) */
/* One block of nb background rows X[nb][ldx] with weights vw[nb]; first_row: a multiple of 64.  init != 0 starts the
 * moments and V from 0.0. */
PGB_HD void pgb_hstat_bg_block(const pgb_shap_view* v, const pgb_hstat_plan_view* pl, int64_t n_jobs, int64_t n_slots,
                               const double* X, int64_t nb, int64_t ldx, const double* vw, int cont, int64_t first_row,
                               int init, double* ws) {
  const pgb_hstat_layout L = pgb_hstat_ws_layout(n_jobs, v->K, n_slots);
  if (init)
    for (int64_t j = L.o_vpart; j < L.o_B; ++j) ws[j] = 0.0;
  for (int64_t i = 0; i < nb; ++i) {
    const int l = (int)((first_row + i) % PGB_HSTAT_LANES);
    ws[L.o_vpart + l] = ws[L.o_vpart + l] + vw[i];
  }
  for (int64_t e = 0; e < n_jobs; ++e)
    for (int64_t i = 0; i < nb; ++i) {
      const int l = (int)((first_row + i) % PGB_HSTAT_LANES);
      pgb_hstat_bg_job_row(v, pl->tree + pl->tree_off[e], pl->tree_off[e + 1] - pl->tree_off[e], pl->a[e], pl->b[e],
                           X + i * ldx, 1, cont, vw[i],
                           ws + L.o_mpart + (int64_t)pl->slot_off[e] * PGB_HSTAT_SLOT_SUMS * PGB_HSTAT_LANES + l);
    }
}

/* V and B from the finished moments */
PGB_HD void pgb_hstat_moments(int64_t n_jobs, int K, int64_t n_slots, double* ws) {
  const pgb_hstat_layout L = pgb_hstat_ws_layout(n_jobs, K, n_slots);
  const double V = pgb_rowsum_lanes(ws + L.o_vpart);
  ws[L.o_V] = V;
  for (int64_t s = 0; s < n_slots; ++s)
    pgb_hstat_slot_finish(ws + L.o_mpart + s * PGB_HSTAT_SLOT_SUMS * PGB_HSTAT_LANES, V, ws + L.o_B + s * PGB_HSTAT_SLOT_SUMS);
}

/* One block of nb evaluation rows with weights w[nb].  g[n_picks][q][K][nb]: the walk's sums of the column jobs (the A
 * of pgbart_permimp.h: pgb_predict with the list as its forest).  jscr[n_picks][q][K][nb] is written; t_rows
 * [n_picks][q][K][nb] and i_rows [n_picks][n_pairs][K][nb] are written where not NULL.  pairs[n_pairs][2]: slots. */
PGB_HD void pgb_hstat_rows_block(const pgb_shap_view* v, const pgb_hstat_plan_view* pl, int n_picks, int q, int n_pairs,
                                 const int32_t* pairs, int64_t n_slots, const double* X, int64_t nb, int64_t ldx,
                                 const double* w, const double* g, int cont, int64_t first_row, int init, double* ws,
                                 double* jscr, double* t_rows, double* i_rows) {
  const int K = v->K;
  const int64_t per = (int64_t)q + n_pairs, n_jobs = (int64_t)n_picks * per;
  const pgb_hstat_layout L = pgb_hstat_ws_layout(n_jobs, K, n_slots);
  double pd[4 * PGB_MAX_OUTPUTS];
  if (init)
    for (int64_t j = 0; j < L.o_vpart; ++j) ws[j] = 0.0;
  for (int64_t i = 0; i < nb; ++i) {
    const int l = (int)((first_row + i) % PGB_HSTAT_LANES);
    ws[L.o_wpart + l] = ws[L.o_wpart + l] + w[i];
  }
  for (int d = 0; d < n_picks; ++d)
    for (int64_t s = 0; s < per; ++s) {
      const int64_t e = d * per + s;
      const int32_t* trees = pl->tree + pl->tree_off[e];
      const int n_trees = pl->tree_off[e + 1] - pl->tree_off[e];
      const double* B = ws + L.o_B + (int64_t)pl->slot_off[e] * PGB_HSTAT_SLOT_SUMS;
      for (int64_t i = 0; i < nb; ++i) {
        const int l = (int)((first_row + i) % PGB_HSTAT_LANES);
        pgb_hstat_job_row(v, trees, n_trees, B, pl->a[e], pl->b[e], X + i * ldx, 1, cont, pd);
        for (int k = 0; k < K; ++k) {
          double u1, u2;
          if (s < q) {
            const int64_t at = (((int64_t)d * q + s) * K + k) * nb + i;
            u1 = pgb_hstat_J(pd, K, k);
            u2 = pgb_hstat_T(pd, K, k, g[at]);
            jscr[at] = u1;
            if (t_rows) t_rows[at] = u2;
          } else {
            const int32_t* pr = pairs + 2 * (s - q);
            u1 = pgb_hstat_I(pd, K, k);
            u2 = pgb_hstat_U(jscr[(((int64_t)d * q + pr[0]) * K + k) * nb + i], jscr[(((int64_t)d * q + pr[1]) * K + k) * nb + i], u1);
            if (i_rows) i_rows[(((int64_t)d * n_pairs + (s - q)) * K + k) * nb + i] = u1;
          }
          pgb_hstat_row_add(ws + L.o_rpart + (e * K + k) * PGB_HSTAT_ROW_SUMS * PGB_HSTAT_LANES + l, w[i], u1, u2);
        }
      }
    }
}

/* The outputs from the row partials rw = ws[0 .. o_vpart) (host memory).  var_fit[n_picks][K].  main_var, total_var,
 * h2_total: [n_picks][q][K]; inter_var, h2: [n_picks][n_pairs][K]; *n_nonfinite: the h2 and h2_total that are an
 * infinity or a NaN. */
PGB_HD void pgb_hstat_finish_host(const double* rw, int n_picks, int q, int n_pairs, int K, const double* var_fit,
                                  double* main_var, double* total_var, double* h2_total, double* inter_var, double* h2,
                                  int64_t* n_nonfinite) {
  const int64_t per = (int64_t)q + n_pairs;
  const pgb_hstat_layout L = pgb_hstat_ws_layout((int64_t)n_picks * per, K, 0);
  const double W = pgb_rowsum_lanes(rw + L.o_wpart);
  int64_t bad = 0;
  for (int d = 0; d < n_picks; ++d)
    for (int64_t s = 0; s < per; ++s)
      for (int k = 0; k < K; ++k) {
        const double* rp = rw + L.o_rpart + ((d * per + s) * K + k) * PGB_HSTAT_ROW_SUMS * PGB_HSTAT_LANES;
        double sum[PGB_HSTAT_ROW_SUMS];
        for (int j = 0; j < PGB_HSTAT_ROW_SUMS; ++j) sum[j] = pgb_rowsum_lanes(rp + j * PGB_HSTAT_LANES);
        const double v1 = pgb_hstat_var(sum[0], sum[1], W), v2 = pgb_hstat_var(sum[2], sum[3], W);
        double h;
        if (s < q) {
          const int64_t at = ((int64_t)d * q + s) * K + k;
          main_var[at] = v1;
          total_var[at] = v2;
          h = h2_total[at] = pgb_hstat_ratio(v2, var_fit[(int64_t)d * K + k]);
        } else {
          const int64_t at = ((int64_t)d * n_pairs + (s - q)) * K + k;
          inter_var[at] = v1;
          h = h2[at] = pgb_hstat_ratio(v1, v2);
        }
        if (pgb_rowred_nonfinite(h)) bad += 1;
      }
  *n_nonfinite = bad;
}

/* ------------------------------------------------------------------ the plan (host, plain C) */
/* The jobs of a call in ONE buffer of int32 [tree_off | slot_off | a | b | tree] that is uploaded as it is. */
typedef struct {
  int32_t* buf;
  int64_t n_jobs, n_tree, n_slots;
} pgb_hstat_plan;

static inline void pgb_hstat_plan_free(pgb_hstat_plan* pl) {
  free(pl->buf);
  pl->buf = 0;
}
static inline pgb_hstat_plan_view pgb_hstat_plan_at(const pgb_hstat_plan* pl, const int32_t* at) {
  pgb_hstat_plan_view v;
  v.tree_off = at;
  v.slot_off = at + pl->n_jobs + 1;
  v.a = v.slot_off + pl->n_jobs + 1;
  v.b = v.a + pl->n_jobs;
  v.tree = v.b + pl->n_jobs;
  return v;
}
static inline int64_t pgb_hstat_plan_words(const pgb_hstat_plan* pl) { return 4 * pl->n_jobs + 2 + pl->n_tree; }

/* 0: built (release with pgb_hstat_plan_free); -1: out of memory; -2: the lists or the slots exceed their range.
 * VALIDATED arguments: cols[q] distinct columns, pairs[n_pairs][2] slots of cols, picks rows of forest_tree_idx;
 * tree_leaf_off: pgb_shap_pack's.  n_common (NULL, or [n_picks][n_pairs]): the length of every L_ab. */
static inline int pgb_hstat_plan_build(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t m, int32_t p,
                                       const int32_t* cols, int32_t q, const int32_t* pairs, int32_t n_pairs,
                                       const int32_t* picks, int32_t n_picks, const int32_t* tree_leaf_off,
                                       int32_t* n_common, pgb_hstat_plan* pl) {
  memset(pl, 0, sizeof *pl);
  pgb_permimp_pack use;
  const int prc = pgb_permimp_pack_build(trees, forest_tree_idx, m, p, cols, q, picks, n_picks, &use);
  if (prc) return prc;
  const int32_t* off = pgb_permimp_pack_off(&use);
  const int32_t* list = pgb_permimp_pack_list(&use);
  const int64_t per = (int64_t)q + n_pairs, n_jobs = (int64_t)n_picks * per;
  int rc = -1;
  for (int pass = 0; pass < 2; ++pass) {
    pgb_hstat_plan_view v;
    int32_t *tree_off = 0, *slot_off = 0, *ja = 0, *jb = 0, *tree = 0;
    if (pass) {
      pl->n_jobs = n_jobs;
      pl->buf = (int32_t*)malloc(sizeof(int32_t) * (size_t)pgb_hstat_plan_words(pl));
      if (!pl->buf) goto done;
      v = pgb_hstat_plan_at(pl, pl->buf);
      tree_off = (int32_t*)v.tree_off;
      slot_off = (int32_t*)v.slot_off;
      ja = (int32_t*)v.a;
      jb = (int32_t*)v.b;
      tree = (int32_t*)v.tree;
    }
    int64_t nt = 0, ns = 0;
    for (int32_t d = 0; d < n_picks; ++d) {
      const int32_t* forest = forest_tree_idx + (size_t)picks[d] * (size_t)m;
      for (int64_t s = 0; s < per; ++s) {
        const int64_t e = d * per + s;
        const int32_t sa = s < q ? (int32_t)s : pairs[2 * (s - q)], sb = s < q ? -1 : pairs[2 * (s - q) + 1];
        if (pass) {
          tree_off[e] = (int32_t)nt;
          slot_off[e] = (int32_t)ns;
          ja[e] = cols[sa];
          jb[e] = sb < 0 ? -1 : cols[sb];
        }
        const int32_t *la = list + off[(int64_t)d * q + sa], *la1 = list + off[(int64_t)d * q + sa + 1];
        int64_t n_here = 0;
        if (sb < 0) {
          for (; la < la1; ++la) {
            if (pass) tree[nt] = *la;
            ++nt;
            ns += tree_leaf_off[*la + 1] - tree_leaf_off[*la];
          }
        } else { /* both lists are subsequences of the forest: one pass over its positions */
          const int32_t *lb = list + off[(int64_t)d * q + sb], *lb1 = list + off[(int64_t)d * q + sb + 1];
          for (int32_t t = 0; t < m && la < la1 && lb < lb1; ++t) {
            const int in_a = *la == forest[t], in_b = *lb == forest[t];
            la += in_a;
            lb += in_b;
            if (!(in_a && in_b)) continue;
            if (pass) tree[nt] = forest[t];
            ++nt;
            ++n_here;
            ns += tree_leaf_off[forest[t] + 1] - tree_leaf_off[forest[t]];
          }
          if (pass && n_common) n_common[(int64_t)d * n_pairs + (s - q)] = (int32_t)n_here;
        }
      }
    }
    if (!pass) {
      if (nt > 0x7fffffffLL || ns > 0x7fffffffLL / PGB_HSTAT_SLOT_SUMS) {
        rc = -2;
        goto done;
      }
      pl->n_tree = nt;
      pl->n_slots = ns;
    } else {
      tree_off[n_jobs] = (int32_t)nt;
      slot_off[n_jobs] = (int32_t)ns;
    }
  }
  rc = 0;
done:
  pgb_permimp_pack_free(&use);
  if (rc) pgb_hstat_plan_free(pl);
  return rc;
}

#ifdef __cplusplus
extern "C" {
#endif
/* (HIP library only, both particle builds; not part of pgbart.h.)  The four calls share the description of the jobs:
 * the history (trees, forest_tree_idx [n_forests][m]), cols_host[q] distinct columns of [0, p), pairs_host[n_pairs][2]
 * SLOTS of cols_host (n_pairs may be 0, pairs_host then NULL; at most PGB_HSTAT_MAX_PAIRS), picks_host[n_picks] rows of
 * forest_tree_idx (picks may repeat).  Everything is validated before a launch: PGB_E_INVALID (the message names the
 * argument) for a null pointer, a size below 1, ldx < p, a column outside [0, p) or named twice, a pair whose slots are
 * outside [0, q), equal, or named twice in either order, a pick outside [0, n_forests), first_row negative or not a
 * multiple of 64, a malformed history (pgb_predict's checks) or a size that overflows.  A refused call writes nothing.
 *
 * pgb_hstat_workspace_bytes: *bytes_out = 8 pgb_hstat_ws_layout(...).words of the call; n_common_out: NULL, or
 * [n_picks][n_pairs] int32 (host), the number of trees of every L_ab.
 *
 * pgb_hstat_background: accumulates the block of nb background rows X_dev [nb][ldx] with the weights v_dev [nb] into the
 * moments of ws_dev; init != 0 starts them from 0.0, otherwise the call continues from the stored ones.
 *
 * pgb_hstat_rows: one block of nb evaluation rows with the weights w_dev [nb].  init != 0 first turns the moments into
 * V, B0 and B1 (so every pgb_hstat_background call comes before the first pgb_hstat_rows call) and starts the row
 * partials from 0.0.  jscr_dev [n_picks][q][K][nb]: device scratch, J of the block.  t_rows_dev [n_picks][q][K][nb] and
 * i_rows_dev [n_picks][n_pairs][K][nb]: NULL, or where the per-row T_a and I_ab are written.
 *
 * pgb_hstat_finish: the outputs (host memory) from the row partials of ws_dev; var_fit_host [n_picks][K]. */
int pgb_hstat_workspace_bytes(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                              int32_t p, const int32_t* cols_host, int32_t q, const int32_t* pairs_host, int32_t n_pairs,
                              const int32_t* picks_host, int32_t n_picks, int64_t* bytes_out, int32_t* n_common_out);
int pgb_hstat_background(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                         const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const double* v_dev, int64_t first_row,
                         int32_t init, const int32_t* cols_host, int32_t q, const int32_t* pairs_host, int32_t n_pairs,
                         const int32_t* picks_host, int32_t n_picks, void* ws_dev, void* stream);
int pgb_hstat_rows(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                   const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const double* w_dev, int64_t first_row,
                   int32_t init, const int32_t* cols_host, int32_t q, const int32_t* pairs_host, int32_t n_pairs,
                   const int32_t* picks_host, int32_t n_picks, void* ws_dev, double* jscr_dev, double* t_rows_dev,
                   double* i_rows_dev, void* stream);
int pgb_hstat_finish(const void* ws_dev, int32_t n_picks, int32_t q, int32_t n_pairs, int32_t K, const double* var_fit_host,
                     double* main_var_out, double* total_var_out, double* h2_total_out, double* inter_var_out,
                     double* h2_out, int64_t* n_nonfinite_out, void* stream);

/* With PGB_WALK_TIMING=1 in the environment (read per call) pgb_hstat_background and pgb_hstat_rows put their kernels
 * between HIP events; this reports the last such measurements of the calling thread in milliseconds (-1.0: none yet):
 * ms_out[0] k_hstat_bg, ms_out[1] k_hstat_rows (both passes).  For tools/timing_hstat.py. */
int pgb_hstat_kernel_ms(double* ms_out);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_HSTAT_H */
