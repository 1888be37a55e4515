// k_loglik_compiled.hip -- the code object of the compiled likelihood family (include/pgbart_compiled.h).
//
// Not part of libpgbart_hip.so: pymc_bart_amd/compiled.py compiles this unit at run time with the library's device
// flags plus --genco, once per (body, param names, particle build), next to two generated files in its build
// directory:
//   pgb_compiled_body.inc       PGB_COMPILED_PARAMS (", const double <name>" per param), PGB_COMPILED_ARGS(P)
//                               (", (P).v[i]" per param), PGB_COMPILED_NPARAMS, PGB_COMPILED_EXPLOG, PGB_HEADERS_HASH
//   pgb_compiled_body_text.inc  the user's body, behind a #line directive (compiler messages quote the user's lines)
// The kernel is k_loglik<1, PGB_FAMILY_COMPILED, false> -- the library's one-output, constant-leaf pass, plain
// (not dense) path -- with the generated function at every place where a one-output family is evaluated, and the
// layout record the library checks before the first launch (pgb_set_loglik_code).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "pgbart.h"
#include "pgbart_spec.h"
#include "pgbart_compiled.h"

#include "pgb_dims.h"
#include "pgb_compiled_body.inc"

#define PGB_COMPILED_LOGLIK 1
#include "pgb_dev_types.h"
#include "pgb_dev_helpers.h"
#include "pgb_leaf_values.h"
#include "k_ctrl.h"

// ---- the body, with the vocabulary on (exp / log on the tables the kernel passes: its LDS copies)
#define PGB_CL_EXPT (pgb_cl_tb->expt)
#define PGB_CL_LOGT (pgb_cl_tb->logt)
#define PGB_CL_LPHI (pgb_cl_tb->lphi)
#define PGB_COMPILED_VOCABULARY
#include "pgbart_compiled.h"
__device__ __forceinline__ double pgb_compiled_user(const pgb_lltabs* __restrict__ pgb_cl_tb, double y, double mu,
                                                    double aux PGB_COMPILED_PARAMS) {
#include "pgb_compiled_body_text.inc"
}
#define PGB_COMPILED_VOCABULARY_END
#include "pgbart_compiled.h"
#undef PGB_CL_EXPT
#undef PGB_CL_LOGT
#undef PGB_CL_LPHI

// the per-row value as the callback family takes it: clamped to [-2047, 2047], NaN -> -2047 (pgb_clamp_loglik)
__device__ __forceinline__ double pgb_compiled_eval(double y, double mu, double aux, const pgb_compiled_params& p,
                                                    const pgb_lltabs* tb) {
  return PGB_CLAMP_LL(pgb_compiled_user(tb, y, mu, aux PGB_COMPILED_ARGS(p)), 2047.0);
}

#include "k_loglik.h"

extern "C" __global__ __launch_bounds__(BT, 3)
void k_loglik_compiled(const Dev* __restrict__ Sp, int par, int nwg, const Cmd* __restrict__ cmds,
                       const Ctrl* __restrict__ ctrls, const Job* __restrict__ jobs_all, const Acc* __restrict__ acc_all,
                       const InitAcc* __restrict__ ias, const double* __restrict__ aux, const pgb_compiled_params prm) {
  k_loglik<1, PGB_FAMILY_COMPILED, false>(Sp, par, nwg, cmds, ctrls, jobs_all, acc_all, ias, aux, prm);
}

extern "C" __device__ pgb_compiled_layout pgb_compiled_layout_record = {
    PGB_COMPILED_MAGIC, PGB_MAX_PARTICLES, PGB_COMPILED_NPARAMS, 0,
    (int64_t)sizeof(Dev), (int64_t)sizeof(Job), (int64_t)sizeof(Cmd), (int64_t)sizeof(Ctrl), (int64_t)sizeof(Acc),
    (uint64_t)PGB_HEADERS_HASH};
