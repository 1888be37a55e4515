/*
 * pgbart_pdp.h -- partial dependence of a fit: the predictions of chosen posterior draws along one covariate's values
 * with EVERY OTHER covariate marginalised by the trees' own training counts, for every (column, draw) of a sweep in
 * one call.  The packed trees are uploaded once; a column whose forests test it with `x <= v` splits only is
 * evaluated once per interval between the split values and the rows are looked up (the profile route), any other
 * column walks every row (the direct route).  Both routes write the bits of pgb_predict.
 *
 * Kept apart from pgbart.h like pgbart_ice.h: the entry point below exists in the HIP library only (both particle
 * builds).
 */
#ifndef PGBART_PDP_H
#define PGBART_PDP_H

#include <stdint.h>

#include "pgbart.h"

/* a (column, draw) profile of at most this many breakpoints is staged in LDS by the lookup kernel (its breakpoints
 * and its (B + 2) x K table); longer ones are read from global memory */
#ifndef PGB_PDP_LDS_MAXB
#define PGB_PDP_LDS_MAXB 256
#endif

#define PGB_PDP_ROUTE_AUTO 0
#define PGB_PDP_ROUTE_DIRECT 1
#define PGB_PDP_ROUTE_PROFILE 2 /* the profile route for every eligible column */

#ifdef __cplusplus
extern "C" {
#endif
/* The numeric contract.  out[c][s][k][i] is exactly what pgb_predict writes for forest picks[c][s] (a row of
 * forest_tree_idx), output k, at a row whose column cols[c] holds X[i][cols[c]], with every other column excluded:
 * the same walk, hence the same order of additions.  NaN and infinities in x, the one-hot and subset rules, linear
 * and mix leaves included; a leaf whose regressor is an excluded column gives its mean.  The result is a function of
 * the arguments only: never of `route`, of the launch geometry or of how a caller blocks rows or columns.
 *   X_dev      [n_rows][ldx]  the sweep rows (device memory, row-major); only the columns cols[.] are read
 *   cols_host  [n_cols]       the column of each family of curves (host memory)
 *   picks_host [n_cols][n_picks] rows of forest_tree_idx (host memory); picks may repeat
 *   route      PGB_PDP_ROUTE_*: a column is ELIGIBLE for the profile route when, in every forest picked for it, every
 *              split on it follows the continuous rule and no leaf regresses on it.  AUTO takes the profile route for
 *              an eligible column when its slots (breakpoints + 2) summed over the picks number fewer than
 *              n_rows x n_picks; PROFILE for every eligible column; DIRECT for none.
 *   out_dev    [n_cols][n_picks][K][n_rows], K = trees->n_outputs
 *   route_taken_host [n_cols] or NULL: PGB_PDP_ROUTE_DIRECT or PGB_PDP_ROUTE_PROFILE per column
 * Everything is validated before a launch: PGB_E_INVALID (the message names the argument) for a null pointer, n_cols /
 * n_picks / n_rows / n_forests / m / p < 1, ldx < p, a column outside [0, p), a pick outside [0, n_forests), a route
 * outside 0 .. 2, or a malformed history.  The call returns when out_dev is written. */
int pgb_predict_pdp(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                    const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx,
                    const int32_t* cols_host, int32_t n_cols,
                    const int32_t* picks_host, int32_t n_picks,
                    int32_t route, double* out_dev, int32_t* route_taken_host, void* stream);

/* With PGB_WALK_TIMING=1 in the environment (read per call) pgb_predict_pdp puts its walk launches (k_pdp_walk, both
 * routes) and its lookup launch (k_pdp_lookup) between HIP events; this reports the last such measurement of the
 * calling thread in milliseconds (-1.0: none yet, or that kernel was not launched).  For tools/pdp_timing.py. */
int pgb_pdp_kernel_ms(double* walk_ms_out, double* lookup_ms_out);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_PDP_H */
