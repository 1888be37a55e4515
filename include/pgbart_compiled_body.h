/*
 * pgbart_compiled_body.h -- how a body becomes a function: the ONE prelude of every unit that compiles a body of the
 * compiled likelihood family (include/pgbart_compiled.h), host (C) and device (HIP) alike.
 *
 * No include guard: a unit includes it once, after the headers it needs (pgbart_spec.h, pgbart_compiled.h; for a
 * sampler body pgbart_ppc.h) and after "pgb_compiled_body.inc", with
 *   PGB_COMPILED_BODY_QUAL      the function's qualifier: static (host), __device__ __forceinline__ (device)
 *   PGB_COMPILED_BODY_SAMPLER   defined: the body is a SAMPLER body; not defined: a density
 * set in front of it (both are released here).  The two generated files sit in the build directory of
 * pymc_bart_amd/compiled.py, the same pair for the host and the device build of a body:
 *   pgb_compiled_body.inc       PGB_COMPILED_PARAMS (", const double <name>" per param), PGB_COMPILED_ARGV(V)
 *                               (", (V)[i]" per param) and PGB_COMPILED_ARGS(P) (the same of (P).v),
 *                               PGB_COMPILED_NPARAMS, PGB_COMPILED_NOUT (K), PGB_COMPILED_LINEAR (0: constant leaves,
 *                               1: linear leaves), PGB_COMPILED_EXPLOG, PGB_HEADERS_HASH
 *   pgb_compiled_body_text.inc  the user's body, behind a #line directive (compiler messages quote the user's lines)
 * What the unit gets: pgb_compiled_mu (double for K = 1, the array of the K predictors above) and
 *   density   double pgb_compiled_user(const pgb_lltabs* pgb_cl_tb, double y, pgb_compiled_mu mu, double aux, params...)
 *   sampler   double pgb_compiled_sampler_user(pgb_ppc_ctx* pgb_cl_rng, pgb_compiled_mu mu, double aux, params...)
 * with the vocabulary on around the body alone: its tables are the first argument's (pgb_cl_tb, pgb_cl_rng->tb), and
 * a sampler body has the random vocabulary too.
 */
#ifndef PGB_COMPILED_NOUT
#define PGB_COMPILED_NOUT 1
#endif
#if PGB_COMPILED_NOUT < 1 || PGB_COMPILED_NOUT > PGB_MAX_OUTPUTS
#error "PGB_COMPILED_NOUT must be in [1, PGB_MAX_OUTPUTS]"
#endif
#if PGB_COMPILED_NOUT == 1
typedef double pgb_compiled_mu;
#else
typedef const double* pgb_compiled_mu; /* (the caller's array of the K predictors: registers on the device) */
#endif

#ifdef PGB_COMPILED_BODY_SAMPLER
#define PGB_CL_TABS (pgb_cl_rng->tb)
#define PGB_COMPILED_SAMPLER_VOCABULARY
#else
#define PGB_CL_TABS pgb_cl_tb
#endif
#define PGB_CL_EXPT (PGB_CL_TABS->expt)
#define PGB_CL_LOGT (PGB_CL_TABS->logt)
#define PGB_CL_LPHI (PGB_CL_TABS->lphi)
#define PGB_COMPILED_VOCABULARY
#include "pgbart_compiled.h"
#ifdef PGB_COMPILED_BODY_SAMPLER
PGB_COMPILED_BODY_QUAL double pgb_compiled_sampler_user(pgb_ppc_ctx* __restrict__ pgb_cl_rng, pgb_compiled_mu mu,
                                                        double aux PGB_COMPILED_PARAMS) {
#else
PGB_COMPILED_BODY_QUAL double pgb_compiled_user(const pgb_lltabs* __restrict__ pgb_cl_tb, double y, pgb_compiled_mu mu,
                                                double aux PGB_COMPILED_PARAMS) {
#endif
#if PGB_COMPILED_NOUT > 1
  enum { K = PGB_COMPILED_NOUT };
#endif
#include "pgb_compiled_body_text.inc"
}
#define PGB_COMPILED_VOCABULARY_END
#include "pgbart_compiled.h"
#undef PGB_CL_TABS
#undef PGB_CL_EXPT
#undef PGB_CL_LOGT
#undef PGB_CL_LPHI
#undef PGB_COMPILED_BODY_QUAL
#undef PGB_COMPILED_BODY_SAMPLER
