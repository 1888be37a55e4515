// k_loglik_compiled.hip -- the PASS code object of the compiled likelihood family (include/pgbart_compiled.h).
//
// Not part of libpgbart_hip.so: pymc_bart_amd/compiled.py compiles this unit at run time with the library's device
// flags plus --genco, once per (body, param names, outputs, particle build, leaves); the body becomes
// pgb_compiled_user in include/pgbart_compiled_body.h, which also describes the two generated files.
// The kernel is the library's constant-leaf pass with that function at every place where the family is evaluated:
// k_loglik<1, PGB_FAMILY_COMPILED, false> (plain, not dense, path) for one output; for K outputs the K-vector pass of
// the same K as the built-in families -- k_loglik<K> for K = 2, 3, 4 (loops unrolled), k_loglik<0> (run-time K) above
// -- at the built-in instance's occupancy.  With PGB_COMPILED_LINEAR the ONE pass kernel of the code object is the
// linear-leaf pass instead (response linear / mix): k_loglik<1, PGB_FAMILY_COMPILED, true> for one output,
// k_loglik<0, PGB_FAMILY_COMPILED, true> -- the run-time-K linear path with the K predictors of a row in an array of
// K doubles -- for K outputs, at the launch bounds of the built-in linear instances.  Next to it: the layout record
// the library checks before the first launch (pgb_set_loglik_code), and a probe kernel that evaluates the body on
// given rows (pgb_compiled_probe).
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
#ifndef PGB_COMPILED_LINEAR
#define PGB_COMPILED_LINEAR 0
#endif
#if PGB_COMPILED_LINEAR != 0 && PGB_COMPILED_LINEAR != 1
#error "PGB_COMPILED_LINEAR must be 0 or 1"
#endif

#define PGB_COMPILED_LOGLIK 1
#include "pgb_dev_types.h"
#include "pgb_dev_helpers.h"
#include "pgb_leaf_values.h"
#include "k_ctrl.h"

// ---- the body (its tables: the ones the kernel passes, its LDS copies)
#define PGB_COMPILED_BODY_QUAL __device__ __forceinline__
#include "pgbart_compiled_body.h"

// the per-row value as the callback family takes it: clamped to [-2047, 2047], NaN -> -2047 (pgb_clamp_loglik)
__device__ __forceinline__ double pgb_compiled_eval(double y, pgb_compiled_mu mu, double aux,
                                                    const pgb_compiled_params& p, const pgb_lltabs* tb) {
  return PGB_CLAMP_LL(pgb_compiled_user(tb, y, mu, aux PGB_COMPILED_ARGS(p)), 2047.0);
}

#include "k_loglik.h"

#if PGB_COMPILED_NOUT == 1
#define PGB_CL_KT 1
#define PGB_CL_WGS 3
#elif PGB_COMPILED_LINEAR  // (K-vector linear leaves: the run-time-K path for any K, as k_loglik<0, -1, true>)
#define PGB_CL_KT 0
#define PGB_CL_WGS 2
#elif PGB_COMPILED_NOUT <= 4
#define PGB_CL_KT PGB_COMPILED_NOUT
#define PGB_CL_WGS PGB_LLK_WGS
#else
#define PGB_CL_KT 0
#define PGB_CL_WGS 2
#endif

extern "C" __global__ __launch_bounds__(BT, PGB_CL_WGS)
void k_loglik_compiled(const Dev* __restrict__ Sp, int par, int nwg, const Cmd* __restrict__ cmds,
                       const Ctrl* __restrict__ ctrls, const Job* __restrict__ jobs_all, const Acc* __restrict__ acc_all,
                       const InitAcc* __restrict__ ias, const double* __restrict__ aux, const pgb_compiled_params prm) {
  k_loglik<PGB_CL_KT, PGB_FAMILY_COMPILED, PGB_COMPILED_LINEAR != 0>(Sp, par, nwg, cmds, ctrls, jobs_all, acc_all, ias, aux, prm);
}

// pgb_compiled_probe: out[i] = the clamped body at (y[i], mu[0..K-1][i], aux[i] or 0.0, prm), i < n; the tables
// are read from global memory (the same values the pass stages in LDS)
extern "C" __global__ __launch_bounds__(BT)
void k_loglik_compiled_probe(const double* __restrict__ y, const double* __restrict__ mu,
                             const double* __restrict__ aux, long long n, const pgb_compiled_params prm,
                             double* __restrict__ out) {
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
  for (long long i = (long long)blockIdx.x * BT + threadIdx.x; i < n; i += (long long)gridDim.x * BT) {
    const double ax = aux ? aux[i] : 0.0;
#if PGB_COMPILED_NOUT == 1
    out[i] = pgb_compiled_eval(y[i], mu[i], ax, prm, &tb);
#else
    double m[PGB_COMPILED_NOUT];
#pragma unroll
    for (int k = 0; k < PGB_COMPILED_NOUT; ++k) m[k] = mu[(size_t)k * n + i];
    out[i] = pgb_compiled_eval(y[i], m, ax, prm, &tb);
#endif
  }
}

extern "C" __device__ pgb_compiled_layout pgb_compiled_layout_record = {
    PGB_COMPILED_MAGIC, PGB_MAX_PARTICLES, PGB_COMPILED_NPARAMS, PGB_COMPILED_NOUT,
    (int64_t)sizeof(Dev), (int64_t)sizeof(Job), (int64_t)sizeof(Cmd), (int64_t)sizeof(Ctrl), (int64_t)sizeof(Acc),
    (uint64_t)PGB_HEADERS_HASH, PGB_COMPILED_LINEAR, 0};
