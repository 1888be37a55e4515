/*
 * pgbart_ice.h -- individual conditional expectation (ICE) curves of a fit: the mean over chosen posterior draws of
 * the prediction along one covariate's observed values, every other covariate held at an instance row's values,
 * fused into the tree walk of pgb_predict.  No probe matrix exists anywhere and nothing of size draws x rows is
 * written: one call produces every curve of a (columns x instances) sweep.
 *
 * Kept apart from pgbart.h like pgbart_pointwise.h: pgbart.h is the ABI every backend (the CPU oracle included)
 * exports in full; the entry point below exists in the HIP library only (both particle builds).
 */
#ifndef PGBART_ICE_H
#define PGBART_ICE_H

#include <stdint.h>

#include "pgbart.h"

/* instance rows of at most this many columns are staged in LDS (8 bytes each); wider ones are read from global memory */
#ifndef PGB_ICE_LDS_MAXP
#define PGB_ICE_LDS_MAXP 1024
#endif

#ifdef __cplusplus
extern "C" {
#endif
/* The numeric contract.  Let z(c, r, i) be instance row r (inst_dev[r][0 .. p-1]) with its entry cols[c] replaced by
 * X[i][cols[c]], and f_d(z) exactly what pgb_predict returns for forest d (row d of forest_tree_idx) at the row z with
 * no excluded variables: the same walk, hence the same order of additions; NaN entries marginalised by the training
 * counts; one-hot and subset rules; linear and mix leaves.  Then
 *   out[c][r][k][i] = (f_{picks[c][r][0]}(z)_k + f_{picks[c][r][1]}(z)_k + ... ) / (double)n_picks
 * summed in pick order s = 0, 1, ..., starting from f of the first pick, followed by ONE IEEE division.  Picks may
 * repeat.  The result is a function of the arguments only, never of the launch geometry.
 *   X_dev      [n_rows][ldx]  the sweep rows (device memory, row-major); only the columns cols[.] are read
 *   inst_dev   [n_inst][ldi]  the instance rows (device memory, row-major)
 *   cols_host  [n_cols]       the swept column of each curve family (host memory)
 *   picks_host [n_cols][n_inst][n_picks] rows of forest_tree_idx (host memory)
 *   out_dev    [n_cols][n_inst][K][n_rows], K = trees->n_outputs
 * Everything is validated before a launch: PGB_E_INVALID (the message names the argument) for a null pointer,
 * n_inst / n_cols / n_picks / n_rows / n_forests / m / p < 1, ldx < p or ldi < p, a column outside [0, p), a pick outside
 * [0, n_forests), or a malformed history.  The call returns when out_dev is written. */
int pgb_predict_ice(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                    const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx,
                    const double* inst_dev, int32_t n_inst, int64_t ldi,
                    const int32_t* cols_host, int32_t n_cols,
                    const int32_t* picks_host, int32_t n_picks,
                    double* out_dev, void* stream);

/* With PGB_WALK_TIMING=1 in the environment (read per call) pgb_predict and pgb_predict_ice put their walk kernel
 * between two HIP events; this reports the last such measurement of the calling thread in milliseconds (-1.0: none
 * yet).  For tools/ice_timing.py: the kernel alone, without the packing, the uploads and the synchronisation. */
int pgb_walk_kernel_ms(double* ms_out);
#ifdef __cplusplus
}
#endif

#endif /* PGBART_ICE_H */
