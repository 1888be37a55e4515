// k_pointwise_compiled.hip -- the POINTWISE code object of the compiled likelihood family (include/pgbart_compiled.h,
// include/pgbart_pointwise.h).
//
// Not part of libpgbart_hip.so: pymc_bart_amd/compiled.py compiles this unit at run time (compile_loglik(...,
// pointwise=True)) with the library's device flags plus --genco; the body becomes pgb_compiled_user in
// include/pgbart_compiled_body.h, which also describes the two generated files.  The code object holds ONE kernel,
// k_pointwise_compiled: the library's k_pointwise (k_pointwise.h: k_predict's walk, the per (draw, row) epilogue, the
// fold over draws) with the user's body at the evaluation site -- mu a scalar or the register array of the K
// predictors, aux read next to y, the draw's params from the parameter table, the clamp of pgb_compiled_eval -- for
// the four (LDS tile?, continuous rules only?) walks, picked by `mode` (wave-uniform).  The walk applies
// pgb_leaf_pred itself, so one pointwise object serves constant, linear and mix leaves.  No sampler pass kernel:
// pgb_set_loglik_code refuses this object, pgb_pointwise_loglik refuses any other (the layout record's mark).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pgbart.h"
#include "pgbart_spec.h"
#include "pgbart_compiled.h"
#include "pgbart_logpdf.h"

#include "pgb_dims.h"
#include "pgb_compiled_body.inc"

// ---- the body (its tables: global memory, as the probe kernel reads them)
#define PGB_COMPILED_BODY_QUAL __device__ __forceinline__
#include "pgbart_compiled_body.h"

#define PGB_PW_COMPILED 1
#include "pgb_pred_walk.h"
#include "k_pointwise.h"

struct PwCompiled {
  __device__ __forceinline__ double operator()(double y, const double* mu, double aux, const double* prm,
                                               const pgb_lltabs* tb) const {
    const pgb_compiled_params& P = *(const pgb_compiled_params*)prm;  // (a row of the table: PGB_PW_PSTRIDE doubles)
#if PGB_COMPILED_NOUT == 1
    return pgb_compiled_user(tb, y, mu[0], aux PGB_COMPILED_ARGS(P));
#else
    return pgb_compiled_user(tb, y, mu, aux PGB_COMPILED_ARGS(P));
#endif
  }
};

extern "C" __global__ __launch_bounds__(PRED_BT)
void k_pointwise_compiled(PredTrees T, const int32_t* __restrict__ forest_idx, int n_forests, int m, int K, int p,
                          const double* __restrict__ X, long long n_rows, long long ldx, PwArgs A, int mode) {
  if (mode == 3) pw_body<true, true, PGB_COMPILED_NOUT>(T, forest_idx, n_forests, m, K, p, X, n_rows, ldx, A, PwCompiled{});
  else if (mode == 1) pw_body<true, false, PGB_COMPILED_NOUT>(T, forest_idx, n_forests, m, K, p, X, n_rows, ldx, A, PwCompiled{});
  else if (mode == 2) pw_body<false, true, PGB_COMPILED_NOUT>(T, forest_idx, n_forests, m, K, p, X, n_rows, ldx, A, PwCompiled{});
  else pw_body<false, false, PGB_COMPILED_NOUT>(T, forest_idx, n_forests, m, K, p, X, n_rows, ldx, A, PwCompiled{});
}

// (the record of a sampler's pass kernel with the device records' sizes and the particle build left 0: this kernel
// reads none of them)
extern "C" __device__ pgb_compiled_layout pgb_compiled_layout_record = {
    PGB_COMPILED_MAGIC, 0, PGB_COMPILED_NPARAMS, PGB_COMPILED_NOUT, 0, 0, 0, 0, 0, (uint64_t)PGB_HEADERS_HASH, 0, 1};
