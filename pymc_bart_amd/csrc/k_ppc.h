// k_ppc.h -- part of pgbart_hip.hip and of k_ppc_compiled.hip (not a standalone header): replicated observations of the
// predictor matrix pgb_predict has written (pgb_ppc_draw, pgb_ppc_draw_compiled; the numeric contract -- every sampler,
// the addressing of every random pair, the caps -- is include/pgbart_ppc.h, whose pgb_ppc_value a host build evaluates
// to the same bits).  The kernel's body is ppc_body, a device function over a value functor: k_ppc instantiates it with
// pgb_ppc_value of a built-in family, k_ppc_compiled.hip (which defines PGB_PPC_COMPILED and takes nothing below the
// body) with a compiled likelihood's sampler body.
//
// An elementwise epilogue: a workgroup of 256 threads owns 256 adjacent rows, one thread one row; the grid's y
// dimension is dealt whole chunks of PGB_PW_CHUNK draws.  A wave therefore reads 64 consecutive rows of one draw (one
// 512-byte segment per predictor), and the draw's parameter row and the family are wave-uniform.  Per (draw, row): the
// K predictors plus the offset, pgb_ppc_value at (seed, d, row0 + row), the store to out[d][row], and the fold of
// the mid-p comparison with y[row] into two integer counters in registers, added once per chunk to
// pit_counts[2][n_rows] by integer atomics -- integer sums: the result does not depend on the order the chunks arrive
// in.  The flag counts: a ballot / popcount per draw into wave-uniform counters, one integer atomic each per wave at the
// end (as k_pointwise counts clamps).  No thread leaves before its wave's last ballot.
// In place (out == mu, K == 1, ld_out == ld): a thread reads its element before it writes it and touches no other.
#define PPC_BT 256
#define PGB_PPC_PSTRIDE PGB_PW_NPAR /* doubles per draw of the device's parameter table */

struct PpcArgs {
  const double* mu;      // [D][K][ld]
  const double* params;  // [D][PGB_PPC_PSTRIDE]: pgb_logpdf_prepare's rows; [D][PGB_COMPILED_MAX_PARAMS] of a sampler body
  const double* offset;  // [K][ld] or nullptr
  const double* y;       // [n_rows] or nullptr
  const double* aux;     // [n_rows] or nullptr (sampler bodies)
  double* out;           // [D][ld_out] or nullptr (may be mu: K = 1)
  int* pit;              // [2][n_rows] or nullptr
  unsigned long long* flags;  // [2]: capped, exhausted
  long long n_rows, ld, ld_out;
  unsigned long long row0, seed;
  int D, K, family;
};

// VAL: v = val(K, mu, aux, the draw's parameter row, seed, d, global row, tables, &flags) -- the replicated
// observation, capped.  VAL::kAux says whether the unit reads the aux column, VAL::kStride is the doubles per draw of
// the parameter table.  KT: the number of outputs when the unit knows it (1, or a compiled body's K), 0: A.K.
template <int KT, class VAL>
__device__ __forceinline__ void ppc_body(const PpcArgs& A, VAL val) {
  const int K = KT ? KT : A.K;
  const long long row = (long long)blockIdx.x * PPC_BT + threadIdx.x;
  const bool act = row < A.n_rows;
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
  const double yv = act && A.y != nullptr ? A.y[row] : 0.0;
  double ax = 0.0;
  if constexpr (VAL::kAux) ax = act && A.aux != nullptr ? A.aux[row] : 0.0;
  unsigned n_cap = 0, n_exh = 0;  // wave-uniform
  const int n_chunks = (A.D + PGB_PW_CHUNK - 1) / PGB_PW_CHUNK;
  for (int c = blockIdx.y; c < n_chunks; c += gridDim.y) {
    const int d0 = c * PGB_PW_CHUNK;
    const int d1 = d0 + PGB_PW_CHUNK < A.D ? d0 + PGB_PW_CHUNK : A.D;
    int below = 0, equal = 0;
    for (int d = d0; d < d1; ++d) {
      uint32_t fl = 0;
      if (act) {
        double mu[KT ? KT : PGB_MAX_OUTPUTS];
        for (int o = 0; o < K; ++o) {
          mu[o] = A.mu[((size_t)d * (size_t)K + (size_t)o) * (size_t)A.ld + (size_t)row];
          if (A.offset != nullptr) mu[o] = mu[o] + A.offset[(size_t)o * (size_t)A.ld + (size_t)row];
        }
        const double v = val(K, mu, ax, A.params + (size_t)d * VAL::kStride, A.seed, (uint32_t)d,
                             A.row0 + (unsigned long long)row, &tb, &fl);
        if (A.out != nullptr) A.out[(size_t)d * (size_t)A.ld_out + (size_t)row] = v;
        if (A.pit != nullptr) {
          int b, e;
          pgb_ppc_compare(v, yv, &b, &e);
          below += b;
          equal += e;
        }
      }
      n_cap += (unsigned)__popcll(__ballot((fl & PGB_PPC_CAPPED) != 0u));
      n_exh += (unsigned)__popcll(__ballot((fl & PGB_PPC_EXHAUSTED) != 0u));
    }
    if (act && A.pit != nullptr) {
      atomicAdd(A.pit + row, below);
      atomicAdd(A.pit + (size_t)A.n_rows + (size_t)row, equal);
    }
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_cap != 0) atomicAdd(A.flags, (unsigned long long)n_cap);
    if (n_exh != 0) atomicAdd(A.flags + 1, (unsigned long long)n_exh);
  }
}

#ifndef PGB_PPC_COMPILED
struct PpcBuiltin {
  static constexpr bool kAux = false;
  static constexpr int kStride = PGB_PPC_PSTRIDE;
  int family;
  __device__ __forceinline__ double operator()(int K, const double* mu, double, const double* q, uint64_t seed, uint32_t d,
                                               uint64_t row, const pgb_lltabs* tb, uint32_t* fl) const {
    return pgb_ppc_value(family, K, mu, q, seed, d, row, tb, fl);
  }
};
template <bool K1>
__global__ __launch_bounds__(PPC_BT) void k_ppc(PpcArgs A) {
  ppc_body<K1 ? 1 : 0>(A, PpcBuiltin{A.family});
}

// the device buffers of one call, released on every way out
struct PpcScratch {
  double* params = nullptr;
  unsigned long long* flags = nullptr;
  hipModule_t mod = nullptr;  // (a sampler body's code object)
  ~PpcScratch() {
    if (params) (void)hipFree(params);
    if (flags) (void)hipFree(flags);
    if (mod) (void)hipModuleUnload(mod);
  }
};

// ---- the argument rules pgb_ppc_draw and pgb_ppc_draw_compiled share, in the order they are reported
// the pointers and the shape (`lik`: the likelihood argument, whichever struct it is)
static int ppc_check_shape(const double* mu_dev, const void* lik, const int64_t* flags_host, const double* out_dev,
                           const double* y_dev, const int32_t* pit_counts_dev, int32_t D, int64_t n_rows, int64_t ld,
                           int64_t ld_out, int64_t row0) {
  if (!mu_dev) return fail(PGB_E_INVALID, "mu_dev is null");
  if (!lik) return fail(PGB_E_INVALID, "lik is null");
  if (!flags_host) return fail(PGB_E_INVALID, "flags_host is null");
  if (!out_dev && !pit_counts_dev) return fail(PGB_E_INVALID, "no output: give out_dev, pit_counts_dev (with y_dev) or both");
  if ((y_dev == nullptr) != (pit_counts_dev == nullptr))
    return fail(PGB_E_INVALID, "y_dev and pit_counts_dev come together: one of them is null");
  if (D < 1) {
    snprintf(g_err, sizeof g_err, "D must be >= 1, got %d", (int)D);
    return PGB_E_INVALID;
  }
  if (n_rows < 1) return fail(PGB_E_INVALID, "n_rows must be >= 1");
  if (ld < n_rows) return fail(PGB_E_INVALID, "ld must be >= n_rows");
  if (out_dev && ld_out < n_rows) return fail(PGB_E_INVALID, "ld_out must be >= n_rows");
  if (row0 < 0) return fail(PGB_E_INVALID, "row0 must be >= 0");
  return PGB_OK;
}

// the two ranges (the same matrix in place for K = 1, or apart) and the grid: x over the rows, y dealt whole chunks
static int ppc_check_ranges(const double* mu_dev, int32_t D, int32_t K, int64_t n_rows, int64_t ld, const double* out_dev,
                            int64_t ld_out, dim3* grid) {
  if (out_dev) {
    const uintptr_t m0 = (uintptr_t)mu_dev, m1 = m0 + ((size_t)D * (size_t)K * (size_t)ld) * sizeof(double);
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + ((size_t)D * (size_t)ld_out) * sizeof(double);
    const bool in_place = o0 == m0 && K == 1 && ld_out == ld;
    if (!in_place && o0 < m1 && m0 < o1)
      return fail(PGB_E_INVALID, "out_dev overlaps mu_dev: in place only as out_dev == mu_dev with K == 1 and ld_out == ld");
  }
  const long long gx = (n_rows + PPC_BT - 1) / PPC_BT;
  if (gx > 0x7FFFFFFFll) return fail(PGB_E_UNSUPPORTED, "n_rows too large for one call");
  const int n_chunks = (D + PGB_PW_CHUNK - 1) / PGB_PW_CHUNK;
  long long gy = (16384 + gx - 1) / gx;  // (enough workgroups to fill the device; results do not depend on it)
  if (gy > n_chunks) gy = n_chunks;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  *grid = dim3((unsigned)gx, (unsigned)gy);
  return PGB_OK;
}

// uploads the parameter table, fills the kernel's arguments, runs `launch(A)` and returns the flag counts
template <class LAUNCH>
static int ppc_run(PpcScratch& sc, const std::vector<double>& hp, const double* mu_dev, int32_t D, int32_t K,
                   int64_t n_rows, int64_t ld, int64_t row0, const double* offset_dev, const double* aux_dev, int family,
                   uint64_t seed, double* out_dev, int64_t ld_out, const double* y_dev, int32_t* pit_counts_dev,
                   int64_t* flags_host, hipStream_t sm, const char* what, LAUNCH launch) {
  HIPCHK(hipMalloc((void**)&sc.flags, 2 * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(sc.flags, 0, 2 * sizeof(unsigned long long), sm));
  HIPCHK(hipMalloc((void**)&sc.params, hp.size() * sizeof(double)));
  HIPCHK(hipMemcpyAsync(sc.params, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, sm));
  PpcArgs A;
  A.mu = mu_dev;
  A.params = sc.params;
  A.offset = offset_dev;
  A.y = y_dev;
  A.aux = aux_dev;
  A.out = out_dev;
  A.pit = pit_counts_dev;
  A.flags = sc.flags;
  A.n_rows = n_rows;
  A.ld = ld;
  A.ld_out = ld_out;
  A.row0 = (unsigned long long)row0;
  A.seed = seed;
  A.D = D;
  A.K = K;
  A.family = family;
  hipError_t e = launch(A);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, what);
  unsigned long long hw[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hw, sc.flags, sizeof hw, hipMemcpyDeviceToHost, sm));
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, what);
  flags_host[0] = (int64_t)hw[0];
  flags_host[1] = (int64_t)hw[1];
  return PGB_OK;
}

extern "C" int pgb_ppc_draw(const double* mu_dev, int32_t D, int32_t K, int64_t n_rows, int64_t ld, int64_t row0,
                            const pgb_ppc_lik* lik, uint64_t seed, double* out_dev, int64_t ld_out, const double* y_dev,
                            int32_t* pit_counts_dev, int64_t* flags_host, void* stream) {
  int rc = ppc_check_shape(mu_dev, lik, flags_host, out_dev, y_dev, pit_counts_dev, D, n_rows, ld, ld_out, row0);
  if (rc != PGB_OK) return rc;
  if (lik->family == PGB_FAMILY_CALLBACK || lik->family == PGB_FAMILY_COMPILED) {
    snprintf(g_err, sizeof g_err, "the %s family has a log density only, no sampler: pgb_ppc_draw takes the built-in families",
             lik->family == PGB_FAMILY_CALLBACK ? "callback" : "compiled");
    return PGB_E_INVALID;
  }
  const int np = pgb_logpdf_nparams(lik->family);
  if (np < 0) return fail(PGB_E_INVALID, "unknown family");
  if (lik->n_params != np) {
    snprintf(g_err, sizeof g_err, "family %d takes n_params = %d per draw, %d given", (int)lik->family, np, (int)lik->n_params);
    return PGB_E_INVALID;
  }
  const int ko = pgb_logpdf_outputs(lik->family);
  if ((ko > 0 && K != ko) || (ko == 0 && (K < 2 || K > PGB_MAX_OUTPUTS))) {
    snprintf(g_err, sizeof g_err, "family %d does not take K = %d", (int)lik->family, (int)K);
    return PGB_E_INVALID;
  }
  if (np > 0 && !lik->params_host) return fail(PGB_E_INVALID, "params_host is null");
  std::vector<double> hp((size_t)D * PGB_PPC_PSTRIDE, 0.0);
  const pgb_lltabs htb = pgb_lltabs_default();
  for (int d = 0; d < D; ++d) {
    if (pgb_logpdf_prepare(lik->family, lik->params_host + (size_t)d * np, hp.data() + (size_t)d * PGB_PPC_PSTRIDE, &htb) != 0) {
      snprintf(g_err, sizeof g_err, "the params of draw %d are outside family %d's domain (positive and finite; 0 < q < 1)", d,
               (int)lik->family);
      return PGB_E_INVALID;
    }
  }
  dim3 grid;
  rc = ppc_check_ranges(mu_dev, D, K, n_rows, ld, out_dev, ld_out, &grid);
  if (rc != PGB_OK) return rc;
  hipStream_t sm = (hipStream_t)stream;
  PpcScratch sc;
  return ppc_run(sc, hp, mu_dev, D, K, n_rows, ld, row0, lik->offset_dev, nullptr, lik->family, seed, out_dev, ld_out, y_dev,
                 pit_counts_dev, flags_host, sm, "k_ppc", [&](const PpcArgs& A) {
                   if (K == 1) hipLaunchKernelGGL((k_ppc<true>), grid, dim3(PPC_BT), 0, sm, A);
                   else hipLaunchKernelGGL((k_ppc<false>), grid, dim3(PPC_BT), 0, sm, A);
                   return hipSuccess;
                 });
}
#endif  // PGB_PPC_COMPILED
