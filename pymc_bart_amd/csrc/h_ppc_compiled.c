/* h_ppc_compiled.c -- the HOST build of a SAMPLER body of the compiled likelihood family (include/pgbart_compiled.h,
 * include/pgbart_ppc.h).
 *
 * pymc_bart_amd/compiled.py compiles this unit with gcc (the oracle's flags) next to the two generated files
 * k_ppc_compiled.hip reads; the body becomes pgb_compiled_sampler_user in include/pgbart_compiled_body.h.
 * pgb_compiled_draw evaluates it over a [D][K][n] array of predictors the way k_ppc_compiled does on the device: the
 * reference of every device test. */
#include <stddef.h>
#include <stdint.h>
#define PGB_COMPILED_NO_ENTRY_POINTS
#include "pgbart_spec.h"
#include "pgbart_compiled.h"
#include "pgbart_ppc.h"

#include "pgb_compiled_body.inc"
#define PGB_COMPILED_BODY_QUAL static
#define PGB_COMPILED_BODY_SAMPLER
#include "pgbart_compiled_body.h"

/* out[D][n] (or NULL) of mu[D][K][n] at global rows row0 .. row0 + n; params[D][n_params]; aux[n] or NULL (0.0); y[n]
 * and pit[2][n] (added to) or NULL; flags[2] = (capped, exhausted) pairs */
int pgb_compiled_draw(const double* mu, int D, int64_t n, uint64_t row0, const double* params, int n_params,
                      const double* aux, uint64_t seed, double* out, const double* y, int32_t* pit, int64_t* flags) {
  enum { K = PGB_COMPILED_NOUT };
  const pgb_lltabs tb = pgb_lltabs_default();
  flags[0] = flags[1] = 0;
  for (int d = 0; d < D; ++d) {
    const double* prm = params + (size_t)d * (size_t)n_params;
    for (int64_t i = 0; i < n; ++i) {
      double m[K];
      for (int k = 0; k < K; ++k) m[k] = mu[((size_t)d * K + (size_t)k) * (size_t)n + (size_t)i];
      pgb_ppc_ctx ctx;
      uint32_t fl = 0;
      pgb_ppc_ctx_begin(&ctx, seed, (uint32_t)d, row0 + (uint64_t)i, &tb);
#if PGB_COMPILED_NOUT == 1
      const double v = pgb_compiled_sampler_user(&ctx, m[0], aux ? aux[i] : 0.0 PGB_COMPILED_ARGV(prm));
#else
      const double v = pgb_compiled_sampler_user(&ctx, m, aux ? aux[i] : 0.0 PGB_COMPILED_ARGV(prm));
#endif
      const double r = pgb_ppc_ctx_end(&ctx, v, &fl);
      if (fl & PGB_PPC_CAPPED) ++flags[0];
      if (fl & PGB_PPC_EXHAUSTED) ++flags[1];
      if (out) out[(size_t)d * (size_t)n + (size_t)i] = r;
      if (y) {
        int below, equal;
        pgb_ppc_compare(r, y[i], &below, &equal);
        pit[i] += below;
        pit[(size_t)n + (size_t)i] += equal;
      }
    }
  }
  return 0;
}
