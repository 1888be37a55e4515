/*
 * pgbart_arms.h -- the numeric contract of CHOOSING among candidate interventions with stored posterior draws: the
 * prediction of every draw at every row under each of A arms (pgb_predict_arms), and from those the optimal arm per
 * (draw, row), its posterior probability, the expected utility and regret of every arm per row, and the value of a rule
 * over the rows per draw (pgb_arm_decide, pgb_arm_decide_finish; pymc_bart_amd/decision.py).
 *
 * Host and device compile the functions below from this one text (PGB_HD, -ffp-contract=off) with + - * /, comparisons,
 * integer operations, pgb_exp_t and pgb_lphi_t only, and the ORDER OF EVERY SUM is part of the definition, so that a
 * host evaluation (pgb_arms_block, pgb_arms_finish, pgb_arms_call) checks the device kernels bit for bit and a result
 * depends neither on the launch geometry nor on how the rows are cut into blocks.
 *
 * Arms.  An arm assigns the same s columns cols[0 .. s) in every row: the columns are distinct,
 * 1 <= s <= PGB_ARMS_MAX_COLS, and arms[a][j] (row-major [A][s]) is the value of cols[j] under arm a,
 * 1 <= A <= PGB_ARMS_MAX.  A value may be any double: a NaN is "unknown under this arm" and is marginalised as the walk
 * marginalises any NaN of a row; the infinities are legal; a value on a SubsetSplit column is read exactly as pgb_predict
 * reads that value in a row.
 *
 * The union use list.  For a VALIDATED pool (pred_validate) and a pick d (a row of forest_tree_idx): the pool-wide
 * indices of the trees of that forest that use AT LEAST ONE column of cols, in forest order -- a tree the forest names
 * twice is listed twice.  "Use" is pgbart_permimp.h's: a split at a node reachable from the root, or a reachable leaf
 * that regresses on the column.  One CSR: off[n_picks + 1], then list[] (pgb_arms_pack_build, plain C on the host).
 *
 * The prediction under an arm.  Pick d, output k, row i; x^a is the row with cols replaced by arms[a].
 *   A_self  = the walk's sum over the list at the row, in list order from 0.0: exactly what pgb_predict returns with the
 *             list as its forest;  A_a = the same at x^a.
 *   delta_a = A_a - A_self     (one rounding)
 *   f_a     = f + delta_a      (one rounding), f being pgb_predict's value of (d, k, i).
 * Both statements are ALWAYS executed: an empty list, or an arm equal to the row's own values, gives delta = +0.0 and
 * f_a = f -- except that f = -0.0 gives +0.0.
 *   out[A][n_picks][K][nb], ARM-MAJOR: slab a is a matrix pgb_row_reduce and pgb_row_summary take as it is.
 *
 * Utility and decision (one output; element (a, d, i) of the predictions at f[a lda + d ldd + i]).
 *   u_{a,d,i} = sign * pgb_rowsum_value(f_a, has_off, off_i, transform, tb) - cost[a]: sign is +1.0 (maximise) or -1.0
 *             (minimise), either product is exact; one rounding for the subtraction; without costs 0.0 is subtracted.
 *   better(u_new, u_best) = u_new > u_best || (u_best != u_best && u_new == u_new).  The best arm of a (d, i) starts at
 *             arm 0 and takes arm a = 1 .. A - 1 whenever better holds: ties go to the lowest index, a NaN is never best
 *             unless all arms are NaN, +inf == +inf ties to the lowest index.  umax is that arm's u.
 *   per row, over the draws (ascending d from 0.0, sequentially):
 *             SU[a] = sum_d u_a;  SR[a] = sum_d (umax - u_a), one rounding per term;  NB[a] = the int32 count of the draws
 *             whose best arm is a.  mean_u = SU / D;  regret = SR / D;  bayes_i = the argmax rule applied to SU[.].
 *   per draw, over the rows: LANE SUMS, exactly the convention of pgbart_rowreduce.h -- 64 partials per sum keyed by the
 *             row's index in the whole of X mod 64, in ascending row order, carried from block to block in the
 *             workspace; blocks start at multiples of 64; the partials are finished by pgb_rowsum_lanes.  Per (d, g):
 *               VO += w * umax;  VB += w * u_{bayes_i};  VP += w * u_{pi_i} (only with a policy vector pi);
 *               VA[a] += w * u_a;  SH[best] += w (the other arms add nothing).     Per g:  W += w.
 *   finish    every sum is divided by W: value_optimal, value_bayes, value_policy, value_arm[a], share_best[a];
 *             regret_bayes = value_optimal - value_bayes (one rounding).  Without a policy VP is +0.0 and value_policy
 *             is 0.0 / W.  Multiplying every weight by a power of two scales every term and every sum exactly.
 *   counters  n_nonfinite: one per (d, a, i) whose u has all exponent bits set, of EVERY row of the block (the rows
 *             below included); the term is still added.
 *             n_bad_group: a row with g outside [0, G) adds nothing to the per-draw sums and to W; it still gets its
 *             per-row results; pgb_arm_decide_finish refuses a workspace whose count is not 0.
 *             n_bad_policy: a row with pi outside [0, A), handled as a row with a bad group.  A row with both is counted
 *             in both.
 *   workspace doubles: part[D][G][3 + 2A][64] (VO, VB, VP, VA[0 .. A), SH[0 .. A); the VP slot is always present and
 *             unused without a policy), then wpart[G][64], then three 64-bit integer counters:
 *             pgb_arms_ws_doubles words of 8 bytes.  G <= PGB_ROWRED_MAX_GROUPS.
 *   output    out[PGB_ARMS_NOUT(A)][D][G]: value_optimal, value_bayes, value_policy, regret_bayes, value_arm[0 .. A),
 *             share_best[0 .. A);  w_out[G].
 */
#ifndef PGBART_ARMS_H
#define PGBART_ARMS_H

#include <stdint.h>

#include "pgbart_permimp.h"
#include "pgbart_rowreduce.h"

#define PGB_ARMS_MAX_COLS 16
#define PGB_ARMS_MAX 64
#define PGB_ARMS_NSUMS(A) (3 + 2 * (A))
#define PGB_ARMS_NOUT(A) (4 + 2 * (A))
#define PGB_ARMS_VO 0
#define PGB_ARMS_VB 1
#define PGB_ARMS_VP 2
#define PGB_ARMS_VA(a) (3 + (a))
#define PGB_ARMS_SH(A, a) (3 + (A) + (a))

/* u of one (a, d, i) */
PGB_HD double pgb_arms_utility(double f, int has_off, double off, int transform, const pgb_lltabs* tb, double sign,
                               double cost) {
  const double v = sign * pgb_rowsum_value(f, has_off, off, transform, tb);
  return v - cost;
}
/* the argmax rule */
PGB_HD int pgb_arms_better(double u_new, double u_best) { return u_new > u_best || (u_best != u_best && u_new == u_new); }

/* the workspace: its size in 8-byte words, and where its parts begin */
PGB_HD int64_t pgb_arms_part(int G, int A, int d, int g, int slot) {
  return ((((int64_t)d * G + g) * PGB_ARMS_NSUMS(A)) + slot) * PGB_ROWRED_LANES;
}
PGB_HD int64_t pgb_arms_wpart(int D, int G, int A) { return pgb_arms_part(G, A, D, 0, 0); }
PGB_HD int64_t pgb_arms_counters(int D, int G, int A) { return pgb_arms_wpart(D, G, A) + (int64_t)G * PGB_ROWRED_LANES; }
PGB_HD int64_t pgb_arms_ws_doubles(int D, int G, int A) { return pgb_arms_counters(D, G, A) + 3; }

/* One block of nb rows whose first row has the index first_row (a multiple of 64) in the whole of X, evaluated
 * sequentially -- what the device kernels compute.  f: element (a, d, i) at [a lda + d ldd + i].  w, g: [nb]; policy:
 * [nb] or NULL; off: [nb] or NULL; cost: [A] or NULL.  init != 0 starts every partial and the counters from 0;
 * otherwise they continue from ws.  nbest (int32), mean, regret: [A][nb]; bayes (int32): [nb]. */
PGB_HD void pgb_arms_block(const double* f, int64_t lda, int64_t ldd, int D, int A, int64_t nb, const double* w,
                           const int32_t* g, const int32_t* policy, const double* off, const double* cost, double sign,
                           int transform, int G, int64_t first_row, int init, const pgb_lltabs* tb, double* ws,
                           int32_t* nbest, double* mean, double* regret, int32_t* bayes) {
  const int64_t n_words = pgb_arms_ws_doubles(D, G, A);
  uint64_t* cnt = (uint64_t*)(ws + pgb_arms_counters(D, G, A));
  if (init) {
    for (int64_t j = 0; j < n_words - 3; ++j) ws[j] = 0.0;
    cnt[0] = cnt[1] = cnt[2] = 0;
  }
  double* wpart = ws + pgb_arms_wpart(D, G, A);
  double u[PGB_ARMS_MAX], su[PGB_ARMS_MAX], sr[PGB_ARMS_MAX];
  int32_t nbst[PGB_ARMS_MAX];
  for (int64_t i = 0; i < nb; ++i) {
    const int l = (int)((first_row + i) % PGB_ROWRED_LANES);
    for (int a = 0; a < A; ++a) {
      su[a] = 0.0;
      sr[a] = 0.0;
      nbst[a] = 0;
    }
    for (int pass = 0; pass < 2; ++pass) {
      int by = 0; /* pass 1: bayes_i */
      int ok = 1;
      if (pass) {
        for (int a = 1; a < A; ++a)
          if (pgb_arms_better(su[a], su[by])) by = a;
        bayes[i] = by;
        for (int a = 0; a < A; ++a) {
          nbest[(int64_t)a * nb + i] = nbst[a];
          mean[(int64_t)a * nb + i] = su[a] / (double)D;
          regret[(int64_t)a * nb + i] = sr[a] / (double)D;
        }
        if (g[i] < 0 || g[i] >= G) {
          cnt[1] += 1;
          ok = 0;
        }
        if (policy && (policy[i] < 0 || policy[i] >= A)) {
          cnt[2] += 1;
          ok = 0;
        }
        if (!ok) break;
        wpart[(int64_t)g[i] * PGB_ROWRED_LANES + l] = wpart[(int64_t)g[i] * PGB_ROWRED_LANES + l] + w[i];
      }
      for (int d = 0; d < D; ++d) {
        int best = 0;
        for (int a = 0; a < A; ++a) {
          u[a] = pgb_arms_utility(f[(int64_t)a * lda + (int64_t)d * ldd + i], off != 0, off ? off[i] : 0.0, transform, tb,
                                  sign, cost ? cost[a] : 0.0);
          if (a > 0 && pgb_arms_better(u[a], u[best])) best = a;
        }
        const double umax = u[best];
        if (!pass) {
          for (int a = 0; a < A; ++a) {
            if (pgb_rowred_nonfinite(u[a])) cnt[0] += 1;
            su[a] = su[a] + u[a];
            sr[a] = sr[a] + (umax - u[a]);
          }
          nbst[best] += 1;
          continue;
        }
        double* p = ws + pgb_arms_part(G, A, d, g[i], 0) + l;
        p[PGB_ARMS_VO * PGB_ROWRED_LANES] = p[PGB_ARMS_VO * PGB_ROWRED_LANES] + w[i] * umax;
        p[PGB_ARMS_VB * PGB_ROWRED_LANES] = p[PGB_ARMS_VB * PGB_ROWRED_LANES] + w[i] * u[by];
        if (policy) p[PGB_ARMS_VP * PGB_ROWRED_LANES] = p[PGB_ARMS_VP * PGB_ROWRED_LANES] + w[i] * u[policy[i]];
        for (int a = 0; a < A; ++a)
          p[PGB_ARMS_VA(a) * PGB_ROWRED_LANES] = p[PGB_ARMS_VA(a) * PGB_ROWRED_LANES] + w[i] * u[a];
        p[PGB_ARMS_SH(A, best) * PGB_ROWRED_LANES] = p[PGB_ARMS_SH(A, best) * PGB_ROWRED_LANES] + w[i];
      }
    }
  }
}

/* The finish of one (d, g, slot) from its finished sum s, the group's weight W and (slot PGB_ARMS_VO only) the finished
 * sum of VB: writes the slot's output, and regret_bayes with value_optimal. */
PGB_HD void pgb_arms_finish_one(double s, double s_vb, double W, int slot, int64_t item, int64_t n_items, double* out) {
  const double v = s / W;
  out[(int64_t)(slot < 3 ? slot : slot + 1) * n_items + item] = v;
  if (slot == PGB_ARMS_VO) out[3 * n_items + item] = v - s_vb / W;
}

/* The whole finish, sequentially: out[PGB_ARMS_NOUT(A)][D][G], w_out[G], counts[3] = n_nonfinite, n_bad_group,
 * n_bad_policy */
PGB_HD void pgb_arms_finish(const double* ws, int D, int G, int A, double* out, double* w_out, int64_t* counts) {
  const int64_t n_items = (int64_t)D * G;
  const uint64_t* cnt = (const uint64_t*)(ws + pgb_arms_counters(D, G, A));
  for (int j = 0; j < 3; ++j) counts[j] = (int64_t)cnt[j];
  for (int g = 0; g < G; ++g) w_out[g] = pgb_rowsum_lanes(ws + pgb_arms_wpart(D, G, A) + (int64_t)g * PGB_ROWRED_LANES);
  for (int d = 0; d < D; ++d)
    for (int g = 0; g < G; ++g) {
      const double s_vb = pgb_rowsum_lanes(ws + pgb_arms_part(G, A, d, g, PGB_ARMS_VB));
      for (int slot = 0; slot < PGB_ARMS_NSUMS(A); ++slot)
        pgb_arms_finish_one(pgb_rowsum_lanes(ws + pgb_arms_part(G, A, d, g, slot)), s_vb, w_out[g], slot,
                            (int64_t)d * G + g, n_items, out);
    }
}

/* One whole call on n rows in one block (first row 0): the reference of pgb_arm_decide + pgb_arm_decide_finish.  The
 * caller provides ws[pgb_arms_ws_doubles(D, G, A)]. */
PGB_HD void pgb_arms_call(const double* f, int64_t lda, int64_t ldd, int D, int A, int64_t n, const double* w,
                          const int32_t* g, const int32_t* policy, const double* off, const double* cost, double sign,
                          int transform, int G, const pgb_lltabs* tb, double* ws, int32_t* nbest, double* mean,
                          double* regret, int32_t* bayes, double* out, double* w_out, int64_t* counts) {
  pgb_arms_block(f, lda, ldd, D, A, n, w, g, policy, off, cost, sign, transform, G, 0, 1, tb, ws, nbest, mean, regret, bayes);
  pgb_arms_finish(ws, D, G, A, out, w_out, counts);
}

/* ------------------------------------------------------------------ the packer (host, plain C) */
/* The union use lists of a VALIDATED pool (pred_validate) in ONE buffer [off | list] of int32 that is uploaded as it is. */
typedef struct {
  int32_t* buf;    /* off[n_lists + 1], then list[n_list] */
  int64_t n_lists; /* n_picks */
  int64_t n_list;
} pgb_arms_pack;

static inline void pgb_arms_pack_free(pgb_arms_pack* pk) {
  free(pk->buf);
  pk->buf = 0;
}
static inline const int32_t* pgb_arms_pack_off(const pgb_arms_pack* pk) { return pk->buf; }
static inline const int32_t* pgb_arms_pack_list(const pgb_arms_pack* pk) { return pk->buf + pk->n_lists + 1; }

/* 0: packed (release with pgb_arms_pack_free); -1: out of memory; -2: the lists hold more than 2^31 - 1 entries.
 * cols[s]: distinct columns in [0, p); picks[n_picks]: rows of forest_tree_idx [.][m]. */
static inline int pgb_arms_pack_build(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t m, int32_t p,
                                      const int32_t* cols, int32_t s, const int32_t* picks, int32_t n_picks,
                                      pgb_arms_pack* pk) {
  memset(pk, 0, sizeof *pk);
  const int32_t NT = trees->n_trees;
  const int lin = trees->slope && trees->xbar && trees->svar;
  int32_t max_nodes = 1;
  for (int32_t t = 0; t < NT; ++t) {
    const int32_t nn = trees->node_off[t + 1] - trees->node_off[t];
    if (nn > max_nodes) max_nodes = nn;
  }
  uint8_t* named = (uint8_t*)calloc((size_t)p, 1);                       /* the column is one of cols */
  uint8_t* uses = (uint8_t*)calloc((size_t)(NT > 0 ? NT : 1), 1);        /* the tree uses one of them */
  int32_t* todo = (int32_t*)malloc(sizeof(int32_t) * (size_t)max_nodes);
  int rc = -1;
  if (!named || !uses || !todo) goto done;
  for (int32_t j = 0; j < s; ++j) named[cols[j]] = 1;
  for (int32_t t = 0; t < NT; ++t) {
    const int32_t base = trees->node_off[t];
    int32_t n_todo = 0;
    todo[n_todo++] = 0;
    while (n_todo > 0 && !uses[t]) { /* the nodes reachable from the root */
      const int32_t g = base + todo[--n_todo];
      int32_t c = trees->var[g];
      if (c >= 0) {
        todo[n_todo++] = trees->right[g];
        todo[n_todo++] = trees->left[g];
      } else {
        c = lin ? trees->svar[g] : -1;
      }
      if (c >= 0 && c < p && named[c]) uses[t] = 1;
    }
  }
  {
    int64_t total = 0;
    for (int32_t d = 0; d < n_picks; ++d) {
      const int32_t* forest = forest_tree_idx + (size_t)picks[d] * (size_t)m;
      for (int32_t t = 0; t < m; ++t) total += uses[forest[t]];
    }
    if (total > 0x7fffffffLL) {
      rc = -2;
      goto done;
    }
    pk->buf = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n_picks + 1 + total));
    if (!pk->buf) goto done;
    pk->n_lists = n_picks;
    pk->n_list = total;
    int32_t* off = pk->buf;
    int32_t* list = pk->buf + n_picks + 1;
    int32_t at = 0;
    for (int32_t d = 0; d < n_picks; ++d) {
      const int32_t* forest = forest_tree_idx + (size_t)picks[d] * (size_t)m;
      off[d] = at;
      for (int32_t t = 0; t < m; ++t)
        if (uses[forest[t]]) list[at++] = forest[t];
    }
    off[n_picks] = at;
    rc = 0;
  }
done:
  free(named);
  free(uses);
  free(todo);
  return rc;
}

#ifdef __cplusplus
extern "C" {
#endif
/* (HIP library only, both particle builds; not part of pgbart.h.  Everything is validated before a launch; a refused
 * call writes nothing and PGB_E_INVALID names the argument.)
 *
 * pgb_predict_arms: the predictions under the arms arms_host [A][s] (host memory) of the columns cols_host[0 .. s) for
 * the forests picks_host[0 .. n_picks) (rows of forest_tree_idx; picks may repeat) at the nb rows of X_dev [nb][ldx]
 * (device memory, row-major, p columns read).  f_dev [n_picks][K][nb]: pgb_predict's output for the same picks and rows;
 * out_dev [A][n_picks][K][nb] (device memory, K = trees->n_outputs).  list_len_host: NULL, or [n_picks] (host memory),
 * where the length of every pick's union list is written.  Refused: a null pointer, a size below 1, ldx < p, a column
 * outside [0, p) or named twice, s > PGB_ARMS_MAX_COLS, A > PGB_ARMS_MAX, a pick outside [0, n_forests), a malformed
 * history (pgb_predict's checks) or an output whose size overflows.  The trees, the lists and the arms are packed and
 * uploaded once per call; the call returns when out_dev is written.
 *
 * pgb_arm_decide_workspace_bytes: 8 pgb_arms_ws_doubles; 0 when D < 1, G is outside [1, PGB_ROWRED_MAX_GROUPS] or A is
 * outside [1, PGB_ARMS_MAX].
 *
 * pgb_arm_decide: one block of nb rows into the device workspace ws_dev and the per-row outputs nbest_dev [A][nb]
 * (int32), mean_dev [A][nb], regret_dev [A][nb] and bayes_dev [nb] (int32).  f_dev: element (a, d, i) at
 * [a lda + d ldd + i], so that one output k of pgb_predict_arms' result is handed over without a copy (f_dev = out_dev +
 * k nb, lda = n_picks K nb, ldd = K nb).  w_dev [nb], g_dev [nb] (int32), policy_dev [nb] (int32) or NULL, off_dev [nb]
 * or NULL: on the device; cost_host [A] or NULL: host memory.  first_row: the index of the block's first row in the
 * whole of X; init != 0 starts the partials from 0.0, otherwise the call continues from the stored ones (the same D, G,
 * A, policy or not).  Refused: a null pointer, D, A, nb or G below 1, A > PGB_ARMS_MAX, G > PGB_ROWRED_MAX_GROUPS,
 * ldd < nb, lda < (D - 1) ldd + nb, first_row negative or not a multiple of 64, an unknown transform, a sign other than
 * +1.0 or -1.0, a cost that is not finite.
 *
 * pgb_arm_decide_finish: out_dev [PGB_ARMS_NOUT(A)][D][G] and w_out_dev [G] on the device from the workspace;
 * counts_out[3] (host memory): n_nonfinite, n_bad_group, n_bad_policy.  PGB_E_INVALID after writing them when
 * n_bad_group or n_bad_policy is not 0.
 *
 * pgb_arms_kernel_ms: with PGB_WALK_TIMING=1 in the environment (read per call) pgb_predict_arms puts its walk kernel and
 * pgb_arm_decide its four kernels between HIP events; this reports the last such measurements of the calling thread in
 * milliseconds (-1.0: none yet).  For tools/timing_decision.py. */
int pgb_predict_arms(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                     const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const int32_t* cols_host, int32_t s,
                     const double* arms_host, int32_t A, const int32_t* picks_host, int32_t n_picks, const double* f_dev,
                     double* out_dev, int32_t* list_len_host, void* stream);
int64_t pgb_arm_decide_workspace_bytes(int32_t D, int32_t G, int32_t A);
int pgb_arm_decide(const double* f_dev, int64_t lda, int64_t ldd, int32_t D, int32_t A, int64_t nb, const double* w_dev,
                   const int32_t* g_dev, const int32_t* policy_dev, const double* off_dev, const double* cost_host,
                   double sign, int32_t transform, int32_t G, int64_t first_row, int32_t init, void* ws_dev,
                   int32_t* nbest_dev, double* mean_dev, double* regret_dev, int32_t* bayes_dev, void* stream);
int pgb_arm_decide_finish(const void* ws_dev, int32_t D, int32_t G, int32_t A, int32_t has_policy, double* out_dev,
                          double* w_out_dev, int64_t* counts_out, void* stream);
int pgb_arms_kernel_ms(double* walk_ms, double* decide_ms);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_ARMS_H */
