/*
 * pgbart_ale.h -- the numeric contract of the accumulated local effects (ALE, Apley & Zhu 2020) of stored posterior
 * draws: per forest, output and row the LOCAL DIFFERENCE of the prediction between the two edges of the bin the row's
 * own value of a column lies in (pgb_predict_ale, below; pymc_bart_amd/ale.py).  Averaging the differences over the
 * rows of a bin (pgb_row_reduce, unchanged) and accumulating the averages along the column is the caller's.
 *
 * The observation is pgbart_permimp.h's: replacing column c of a row can change only the trees that USE c, so per
 * (forest, column) only the trees of the forest's use list are walked -- twice, once per edge.  The use lists are
 * pgb_permimp_pack_build's; nothing of them is restated here.
 *
 * Bins.  A column's edges are e[0] < e[1] < ... < e[B], all finite, 1 <= B <= PGB_ALE_MAX_BINS, so that the
 * G = B + 1 groups of a column (its bins and the missing bin) stay inside PGB_ROWRED_MAX_GROUPS.
 *   pgb_ale_bin(e, B, x): a NaN gives B, the MISSING bin; every other x gives the number of INTERIOR edges
 *   e[1] .. e[B - 1] that are < x, found by binary search.  So bin b is (e[b], e[b + 1]]: a value on an edge belongs to
 *   the bin that ends there; bin 0 also takes everything <= e[0], -inf included, and bin B - 1 everything > e[B],
 *   +inf included.
 *
 * The value.  Pick d, slot s with c = cols[s] and the edges e_s[0 .. B_s], output k, row i of the block,
 * b = pgb_ale_bin(e_s, B_s, X[i][c]).
 *   A_hi  = the walk's sum over the use list of (d, s), in list order, starting from 0.0 (the A of pgbart_permimp.h),
 *           at the row with column c replaced by e_s[b + 1];  A_lo = the same with e_s[b].
 *   delta = A_hi - A_lo     (one rounding), always executed: an empty list gives 0.0 - 0.0 = +0.0.
 *   A row in the missing bin gets delta = +0.0, whatever its walks would give.
 *   out[q][n_picks][K][nb] holds delta, SLOT-MAJOR: slab s is a [n_picks][K][nb] matrix pgb_row_reduce takes as it is.
 *   bins_out[q][nb] (int32): row s is that slab's group vector, G = B_s + 1.
 *
 * Host and device compile pgb_ale_bin from this one text (PGB_HD).
 */
#ifndef PGBART_ALE_H
#define PGBART_ALE_H

#include <stdint.h>

#include "pgbart_permimp.h"

#define PGB_ALE_MAX_BINS 1024

/* the bin of x among the edges e[0 .. B], 1 <= B: [0, B) for a number (the infinities included), B for a NaN */
PGB_HD int32_t pgb_ale_bin(const double* e, int32_t B, double x) {
  if (x != x) return B;
  int32_t lo = 0, hi = B - 1; /* the count of the interior edges e[1 .. B - 1] that are < x lies in [lo, hi] */
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (e[1 + mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

#ifdef __cplusplus
extern "C" {
#endif
/* The local differences of the forests picks_host[0 .. n_picks) (rows of forest_tree_idx; picks may repeat) at the nb
 * rows of X_dev [nb][ldx] (device memory, row-major, p columns read) for the columns cols_host[0 .. q).  The edges of
 * slot s are edges_host[edge_off_host[s] .. edge_off_host[s + 1]) (host memory, edge_off_host[q + 1]).  out_dev
 * [q][n_picks][K][nb] doubles and bins_out_dev [q][nb] int32 (device memory, K = trees->n_outputs).  HIP library only
 * (both particle builds); not part of pgbart.h.  Everything is validated before a launch: PGB_E_INVALID (the message
 * names the argument) for a null pointer, a size below 1, ldx < p, a column outside [0, p) or named twice, a pick
 * outside [0, n_forests), edge_off_host not starting at 0 or not increasing by at least 2, a column with more than
 * PGB_ALE_MAX_BINS + 1 edges, an edge that is not finite or not above its predecessor, a malformed history
 * (pgb_predict's checks) or an output whose size overflows.  A refused call writes nothing.  The trees, the use lists
 * and the edges are packed and uploaded once per call; the call returns when out_dev and bins_out_dev are written. */
int pgb_predict_ale(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                    const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const int32_t* cols_host, int32_t q,
                    const double* edges_host, const int32_t* edge_off_host, const int32_t* picks_host, int32_t n_picks,
                    double* out_dev, int32_t* bins_out_dev, void* stream);

/* With PGB_WALK_TIMING=1 in the environment (read per call) pgb_predict_ale puts its walk kernel between HIP events;
 * this reports the last such measurement of the calling thread in milliseconds (-1.0: none yet).  For
 * tools/timing_ale.py. */
int pgb_ale_kernel_ms(double* ms_out);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_ALE_H */
