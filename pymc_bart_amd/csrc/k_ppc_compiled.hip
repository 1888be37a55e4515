// k_ppc_compiled.hip -- the SAMPLER code object of the compiled likelihood family (include/pgbart_compiled.h,
// include/pgbart_ppc.h).
//
// Not part of libpgbart_hip.so: pymc_bart_amd/compiled.py compiles this unit at run time (compile_sampler) with the
// library's device flags plus --genco; the likelihood's sampler body becomes pgb_compiled_sampler_user in
// include/pgbart_compiled_body.h, which also describes the two generated files.  The code object holds ONE kernel, k_ppc_compiled: the library's k_ppc (k_ppc.h: one thread per row, 256 rows per workgroup,
// chunks of PGB_PW_CHUNK draws on grid y, the PIT fold, the ballot / popcount flag counts, the in-place rule) with the
// user's sampler body at the evaluation site -- mu a scalar or the register array of the K predictors, aux read next to
// the row, the draw's params from the [D][PGB_COMPILED_MAX_PARAMS] table, the random vocabulary on a pgb_ppc_ctx of
// the (seed, draw position, global row), the cap of pgb_ppc_ctx_end.  No pass kernel and no pointwise kernel:
// pgb_ppc_draw_compiled takes this object alone (the layout record's mark 2), pgb_set_loglik_code and
// pgb_pointwise_loglik refuse it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pgbart.h"
#include "pgbart_spec.h"
#include "pgbart_compiled.h"
#include "pgbart_logpdf.h"
#include "pgbart_ppc.h"

#include "pgb_dims.h"
#include "pgb_compiled_body.inc"

// ---- the sampler body, with both vocabularies on (its tables: global memory, as k_ppc reads them)
#define PGB_COMPILED_BODY_QUAL __device__ __forceinline__
#define PGB_COMPILED_BODY_SAMPLER
#include "pgbart_compiled_body.h"

#define PGB_PPC_COMPILED 1
#include "k_ppc.h"

struct PpcCompiled {
  static constexpr bool kAux = true;
  static constexpr int kStride = PGB_COMPILED_MAX_PARAMS;
  __device__ __forceinline__ double operator()(int, const double* mu, double aux, const double* prm, uint64_t seed,
                                               uint32_t d, uint64_t row, const pgb_lltabs* tb, uint32_t* fl) const {
    const pgb_compiled_params& P = *(const pgb_compiled_params*)prm;  // (a row of the table)
    pgb_ppc_ctx ctx;
    pgb_ppc_ctx_begin(&ctx, seed, d, row, tb);
#if PGB_COMPILED_NOUT == 1
    const double v = pgb_compiled_sampler_user(&ctx, mu[0], aux PGB_COMPILED_ARGS(P));
#else
    const double v = pgb_compiled_sampler_user(&ctx, mu, aux PGB_COMPILED_ARGS(P));
#endif
    return pgb_ppc_ctx_end(&ctx, v, fl);
  }
};

extern "C" __global__ __launch_bounds__(PPC_BT) void k_ppc_compiled(PpcArgs A) {
  ppc_body<PGB_COMPILED_NOUT>(A, PpcCompiled{});
}

// (the record of a sampler's pass kernel with the device records' sizes and the particle build left 0: this kernel
// reads none of them)
extern "C" __device__ pgb_compiled_layout pgb_compiled_layout_record = {
    PGB_COMPILED_MAGIC, 0, PGB_COMPILED_NPARAMS, PGB_COMPILED_NOUT, 0, 0, 0, 0, 0, (uint64_t)PGB_HEADERS_HASH, 0,
    PGB_COMPILED_MARK_SAMPLER};
