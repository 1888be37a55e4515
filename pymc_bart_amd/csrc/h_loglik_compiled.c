/* h_loglik_compiled.c -- the HOST build of a density body of the compiled likelihood family (include/pgbart_compiled.h).
 *
 * pymc_bart_amd/compiled.py compiles this unit with gcc (the oracle's flags) next to the two generated files the device
 * units read; the body becomes pgb_compiled_user in include/pgbart_compiled_body.h.  One output: the callback a CPU
 * backend runs as family "callback".  K outputs: no CPU backend runs it (the callback family has one output); an
 * evaluator of given rows, the reference the device's probe kernel is held to. */
#include <stddef.h>
#include <stdint.h>
#define PGB_COMPILED_NO_ENTRY_POINTS
#include "pgbart_spec.h"
#include "pgbart_compiled.h"

#include "pgb_compiled_body.inc"
#define PGB_COMPILED_BODY_QUAL static
#include "pgbart_compiled_body.h"

typedef struct { /* (compiled.CompiledContext) */
  const double* aux;
  double params[PGB_COMPILED_MAX_PARAMS];
} pgb_compiled_ctx;

#if PGB_COMPILED_NOUT == 1
/* pgb_loglik_fn: the row index selects aux; the library clamps and quantises the values */
int pgb_compiled_loglik(void* ctx, const int64_t* row, const double* y, const double* mu, int64_t n, double* out) {
  const pgb_compiled_ctx* c = (const pgb_compiled_ctx*)ctx;
  const pgb_lltabs tb = pgb_lltabs_default();
  for (int64_t i = 0; i < n; ++i)
    out[i] = pgb_compiled_user(&tb, y[i], mu[i], c->aux ? c->aux[row[i]] : 0.0 PGB_COMPILED_ARGV(c->params));
  return 0;
}
#else
/* out[i] = the body at (y[i], mu[0 .. K-1][i] ([K][n]), aux[i] or 0.0), clamped like the sampler takes it */
int pgb_compiled_eval_rows(void* ctx, const double* y, const double* mu, int64_t n, double* out) {
  const pgb_compiled_ctx* c = (const pgb_compiled_ctx*)ctx;
  const pgb_lltabs tb = pgb_lltabs_default();
  for (int64_t i = 0; i < n; ++i) {
    double m[PGB_COMPILED_NOUT];
    for (int k = 0; k < PGB_COMPILED_NOUT; ++k) m[k] = mu[(size_t)k * (size_t)n + (size_t)i];
    out[i] = pgb_clamp_loglik(pgb_compiled_user(&tb, y[i], m, c->aux ? c->aux[i] : 0.0 PGB_COMPILED_ARGV(c->params)));
  }
  return 0;
}
#endif
