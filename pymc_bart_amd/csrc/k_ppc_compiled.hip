// k_ppc_compiled.hip -- the SAMPLER code object of the compiled likelihood family (include/pgbart_compiled.h,
// include/pgbart_ppc.h).
//
// Not part of libpgbart_hip.so: pymc_bart_amd/compiled.py compiles this unit at run time (compile_sampler) with the
// library's device flags plus --genco, next to the two generated files k_loglik_compiled.hip documents
// (pgb_compiled_body.inc, pgb_compiled_body_text.inc -- here the text of the likelihood's sampler body).  The code
// object holds ONE kernel, k_ppc_compiled: the library's k_ppc (k_ppc.h: one thread per row, 256 rows per workgroup,
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
#ifndef PGB_COMPILED_NOUT
#define PGB_COMPILED_NOUT 1
#endif
#if PGB_COMPILED_NOUT < 1 || PGB_COMPILED_NOUT > PGB_MAX_OUTPUTS
#error "PGB_COMPILED_NOUT must be in [1, PGB_MAX_OUTPUTS]"
#endif

// ---- the sampler body, with both vocabularies on (the tables: global memory, as k_ppc reads them)
#define PGB_CL_EXPT (pgb_cl_rng->tb->expt)
#define PGB_CL_LOGT (pgb_cl_rng->tb->logt)
#define PGB_CL_LPHI (pgb_cl_rng->tb->lphi)
#define PGB_COMPILED_VOCABULARY
#define PGB_COMPILED_SAMPLER_VOCABULARY
#include "pgbart_compiled.h"
#if PGB_COMPILED_NOUT == 1
typedef double pgb_compiled_mu;
#else
typedef const double* pgb_compiled_mu;  // (the kernel's register array of the K predictors)
#endif
__device__ __forceinline__ double pgb_compiled_sampler_user(pgb_ppc_ctx* __restrict__ pgb_cl_rng, pgb_compiled_mu mu,
                                                            double aux PGB_COMPILED_PARAMS) {
#if PGB_COMPILED_NOUT > 1
  enum { K = PGB_COMPILED_NOUT };
#endif
#include "pgb_compiled_body_text.inc"
}
#define PGB_COMPILED_VOCABULARY_END
#include "pgbart_compiled.h"
#undef PGB_CL_EXPT
#undef PGB_CL_LOGT
#undef PGB_CL_LPHI

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
