/*
 * pgbart_proximity.h -- the contract of the posterior proximity of rows: the node where a row stops in every tree of every
 * draw (its "leaf id"), the number of (draw, tree) slots in which two rows stop at different nodes, and the k reference
 * rows nearest to a query row in that count (pgb_predict_leaf_codes, pgb_prox_count and pgb_prox_topk, below;
 * pymc_bart_amd/proximity.py).  Every other consumer of the stored draws reduces the leaf VALUES a row reaches; this
 * header exposes the PARTITION the forest puts on the rows.
 *
 * Every number here is an integer, so host and device agree bit for bit without any floating-point rule; the functions
 * below compile from this one text on both sides (PGB_HD) and the sequential references (pgb_prox_stop,
 * pgb_prox_codes_block, pgb_prox_count_block, pgb_prox_topk_block) are what the device kernels compute.
 *
 *   stop node  s(d, t, i): the tree-local index of the node where row i stops in tree t of draw d.  The walk starts at
 *              node 0.  At a split node on column j the row stops THERE if j is excluded or x_ij is NaN; otherwise it goes
 *              left exactly when pgb_go_left(rule, x_ij, split) says so -- the decision of pgb_predict's walk, all three
 *              split rules, +-inf ordinary values.  A leaf stops the walk.  No marginalisation, no weights, no stack: with
 *              excluded columns this is the proximity in the subspace without them, and a row with a missing value is
 *              close only to rows that stop at the same node.
 *   code       one byte, 0 .. 254: the stop node.  A history with a tree of more than PGB_PROX_MAX_NODES = 255 nodes is
 *              refused (only loaded or hand-built arrays hold one; both samplers stop at PGB_MAX_NODES).
 *   slots      the call's draw list has D entries of m trees: slot s = d_pos * m + t, T = D * m of them (T <= 2^31 - 1).
 *   words      word w holds the slots 4w .. 4w + 3, slot 4w + b in bits 8b .. 8b + 7; W = ceil(T / 4) words; the slots of
 *              the last word beyond T hold PGB_PROX_PAD = 0xFF on both sides -- not a code, so a pad never mismatches.
 *              A code matrix is uint32 [W][ld], row fastest.
 *   distance   dist(i, j) = the number of slots whose codes differ (the Hamming distance of the two code vectors);
 *              matches = T - dist; similarity = matches / T (divided by the caller).  Distances ADD over disjoint sets
 *              of slots: a call may be cut into blocks of reference rows and into chunks of draws, each chunk with its own
 *              tail pad, and no bit depends on the cut (the `init` flag of the count).  Distances, not matches: a pad
 *              adds 0 to a distance and would add 1 to a count of matches, so only distances add without knowing T.
 *   top-k      the key of a pair is (uint64)dist << 32 | j with j the reference row's index in the whole of X_ref
 *              (j < 2^32 - 1); the k smallest keys per query in ascending order: nearest first, ties to the smaller row
 *              index.  1 <= k <= PGB_PROX_MAX_K.  With self_row0 >= 0 the pair whose j equals self_row0 + i is left out.
 *   workspace  per call: keys[q][k] (uint64, started at all-ones: no pair has that key), then sum[q] (uint64, the sum of
 *              dist(i, j) over the pairs taken in): pgb_prox_topk_ws_words words of 8 bytes.
 */
#ifndef PGBART_PROXIMITY_H
#define PGBART_PROXIMITY_H

#include <stdint.h>

#include "pgbart.h"
#include "pgbart_spec.h"

#define PGB_PROX_PAD 0xFFu
#define PGB_PROX_MAX_NODES 255
#define PGB_PROX_MAX_K 128
#define PGB_PROX_MAX_SLOTS 2147483647ll /* T: a distance fits the high half of a key with room to spare */
#define PGB_PROX_KEY_NONE 0xFFFFFFFFFFFFFFFFull

/* the words of T slots */
PGB_HD int64_t pgb_prox_words(int64_t T) { return (T + 3) / 4; }

/* the number of bytes in which two words differ: integer operations only.  Bit 7 of every byte of r says "this byte of
 * a ^ b is not 0": the low seven bits carry into it, the top bit is or-ed in. */
PGB_HD uint32_t pgb_prox_mismatch4(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return (uint32_t)__builtin_popcount((t | x) & 0x80808080u);
}

/* the byte of slot b (0 .. 3) of a word, and a word from its four bytes */
PGB_HD uint32_t pgb_prox_byte(uint32_t word, int b) { return (word >> (8 * b)) & 0xFFu; }
PGB_HD uint32_t pgb_prox_pack4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
  return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

/* the workspace of the top-k: its size in 8-byte words */
PGB_HD int64_t pgb_prox_topk_ws_words(int64_t q, int k) { return q * (int64_t)k + q; }
PGB_HD uint64_t pgb_prox_key(uint32_t dist, int64_t j) { return ((uint64_t)dist << 32) | (uint64_t)j; }

/* s(d, t, i) of one row x[p] in tree t of the arrays; excl: [p] flags (not 0: the column is excluded) or NULL */
PGB_HD int pgb_prox_stop(const pgb_tree_arrays* tr, int t, const double* x, const uint8_t* excl) {
  const int base = tr->node_off[t];
  int k = 0;
  for (;;) {
    const int g = base + k;
    const int j = tr->var[g];
    if (j < 0) return k;
    const double xv = x[j];
    if ((excl && excl[j]) || xv != xv) return k;
    k = pgb_go_left(tr->rule ? tr->rule[g] : PGB_RULE_CONTINUOUS, xv, tr->split[g]) ? tr->left[g] : tr->right[g];
  }
}

/* The code matrix codes[W][ldc] of the nb rows X[nb][ldx] under the D x m forest table fidx (indices into the arrays),
 * evaluated sequentially -- what k_leaf_codes computes.  The columns nb .. ldc - 1 are not written. */
PGB_HD void pgb_prox_codes_block(const pgb_tree_arrays* tr, const int32_t* fidx, int D, int m, const double* X, int64_t nb,
                                 int64_t ldx, const uint8_t* excl, uint32_t* codes, int64_t ldc) {
  const int64_t T = (int64_t)D * m, W = pgb_prox_words(T);
  for (int64_t w = 0; w < W; ++w)
    for (int64_t i = 0; i < nb; ++i) {
      uint32_t c[4];
      for (int b = 0; b < 4; ++b) {
        const int64_t s = 4 * w + b; /* slot s = d_pos * m + t: entry s of the flat forest table */
        c[b] = s < T ? (uint32_t)pgb_prox_stop(tr, fidx[s], X + i * ldx, excl) : PGB_PROX_PAD;
      }
      codes[w * ldc + i] = pgb_prox_pack4(c[0], c[1], c[2], c[3]);
    }
}

/* dist[i][j] (+)= sum over the W words of mismatch4(cq[w][i], cr[w][j]): uint32 [q][ldo].  init != 0 starts every
 * distance from 0; otherwise the call continues from the stored ones (another chunk of draws). */
PGB_HD void pgb_prox_count_block(const uint32_t* cq, int64_t ldq, int64_t q, const uint32_t* cr, int64_t ldr, int64_t nb,
                                 int64_t W, uint32_t* dist, int64_t ldo, int init) {
  for (int64_t i = 0; i < q; ++i)
    for (int64_t j = 0; j < nb; ++j) {
      uint32_t acc = init ? 0u : dist[i * ldo + j];
      for (int64_t w = 0; w < W; ++w) acc += pgb_prox_mismatch4(cq[w * ldq + i], cr[w * ldr + j]);
      dist[i * ldo + j] = acc;
    }
}

/* Merges the distances dist[q][ldo] of one block of nb reference rows, whose first row has the index first_row in the
 * whole of X_ref, into the workspace ws[pgb_prox_topk_ws_words(q, k)].  init != 0 starts the keys at all-ones and the sums
 * at 0.  self_row0 >= 0: query i is row self_row0 + i of X_ref, and that pair is left out of the keys and of the sum. */
PGB_HD void pgb_prox_topk_block(const uint32_t* dist, int64_t ldo, int64_t q, int64_t nb, int64_t first_row,
                                int64_t self_row0, int k, uint64_t* ws, int init) {
  uint64_t* sum = ws + q * (int64_t)k;
  for (int64_t i = 0; i < q; ++i) {
    uint64_t* keys = ws + i * (int64_t)k;
    if (init) {
      for (int r = 0; r < k; ++r) keys[r] = PGB_PROX_KEY_NONE;
      sum[i] = 0;
    }
    for (int64_t j = 0; j < nb; ++j) {
      const int64_t J = first_row + j;
      if (self_row0 >= 0 && J == self_row0 + i) continue;
      const uint32_t d = dist[i * ldo + j];
      sum[i] += d;
      const uint64_t key = pgb_prox_key(d, J);
      if (key >= keys[k - 1]) continue;
      int r = k - 1; /* insertion into the ascending list */
      while (r > 0 && keys[r - 1] > key) {
        keys[r] = keys[r - 1];
        --r;
      }
      keys[r] = key;
    }
  }
}

#ifdef __cplusplus
extern "C" {
#endif
/* (HIP library only; not part of pgbart.h.)
 *
 * pgb_predict_leaf_codes: the code matrix codes_dev [W][ldc] (uint32, W = ceil(n_forests m / 4), ldc >= n_rows) of the
 * n_rows device rows X_dev (row-major, leading dimension ldx >= p) under the forests forest_tree_idx [n_forests][m] of
 * the host arrays `trees`; excluded_host: n_excluded column indices (those outside [0, p) are ignored, as pgb_predict
 * ignores them).  The checks of pgb_predict, and: a tree of more than PGB_PROX_MAX_NODES nodes, ldc < n_rows and
 * n_forests m > PGB_PROX_MAX_SLOTS are refused.  The columns n_rows .. ldc - 1 are not written.
 *
 * pgb_prox_count: dist_dev [q][ldo] (uint32, ldo >= nb) (+)= the distances of the q query rows of cq_dev [W][ldq] to the
 * nb reference rows of cr_dev [W][ldr]; init != 0 starts them from 0.  The columns nb .. ldo - 1 are not written.
 *
 * pgb_prox_topk_workspace_bytes: 8 pgb_prox_topk_ws_words(q, k); 0 when q < 1 or k is outside [1, PGB_PROX_MAX_K].
 * pgb_prox_topk: merges the block's distances into ws_dev (pgb_prox_topk_block); first_row + nb <= 2^32 - 1.
 *
 * All three validate everything before anything is launched (PGB_E_INVALID with a message that carries the entry point's
 * name) and return when their output is written. */
int pgb_predict_leaf_codes(const pgb_tree_arrays* trees_host, const int32_t* forest_tree_idx_host, int32_t n_forests,
                           int32_t m, const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx,
                           const int32_t* excluded_host, int32_t n_excluded, uint32_t* codes_dev, int64_t ldc, void* stream);
int pgb_prox_count(const uint32_t* cq_dev, int64_t ldq, int64_t q, const uint32_t* cr_dev, int64_t ldr, int64_t nb, int64_t W,
                   uint32_t* dist_dev, int64_t ldo, int32_t init, void* stream);
int64_t pgb_prox_topk_workspace_bytes(int64_t q, int32_t k);
int pgb_prox_topk(const uint32_t* dist_dev, int64_t ldo, int64_t q, int64_t nb, int64_t first_row, int64_t self_row0,
                  int32_t k, void* ws_dev, int32_t init, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_PROXIMITY_H */
