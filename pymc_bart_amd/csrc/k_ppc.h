// k_ppc.h -- part of pgbart_hip.hip (not a standalone header): replicated observations of the predictor matrix
// pgb_predict has written (pgb_ppc_draw; the numeric contract -- every sampler, the addressing of every random pair,
// the caps -- is include/pgbart_ppc.h, whose pgb_ppc_value a host build evaluates to the same bits).
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
  const double* params;  // [D][PGB_PPC_PSTRIDE]: pgb_logpdf_prepare's rows
  const double* offset;  // [K][ld] or nullptr
  const double* y;       // [n_rows] or nullptr
  double* out;           // [D][ld_out] or nullptr (may be mu: K = 1)
  int* pit;              // [2][n_rows] or nullptr
  unsigned long long* flags;  // [2]: capped, exhausted
  long long n_rows, ld, ld_out;
  unsigned long long row0, seed;
  int D, K, family;
};

template <bool K1>
__global__ __launch_bounds__(PPC_BT) void k_ppc(PpcArgs A) {
  const int K = K1 ? 1 : A.K;
  const long long row = (long long)blockIdx.x * PPC_BT + threadIdx.x;
  const bool act = row < A.n_rows;
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
  const double yv = act && A.y != nullptr ? A.y[row] : 0.0;
  unsigned n_cap = 0, n_exh = 0;  // wave-uniform
  const int n_chunks = (A.D + PGB_PW_CHUNK - 1) / PGB_PW_CHUNK;
  for (int c = blockIdx.y; c < n_chunks; c += gridDim.y) {
    const int d0 = c * PGB_PW_CHUNK;
    const int d1 = d0 + PGB_PW_CHUNK < A.D ? d0 + PGB_PW_CHUNK : A.D;
    int below = 0, equal = 0;
    for (int d = d0; d < d1; ++d) {
      uint32_t fl = 0;
      if (act) {
        double mu[K1 ? 1 : PGB_MAX_OUTPUTS];
        for (int o = 0; o < K; ++o) {
          mu[o] = A.mu[((size_t)d * (size_t)K + (size_t)o) * (size_t)A.ld + (size_t)row];
          if (A.offset != nullptr) mu[o] = mu[o] + A.offset[(size_t)o * (size_t)A.ld + (size_t)row];
        }
        const double v = pgb_ppc_value(A.family, K, mu, A.params + (size_t)d * PGB_PPC_PSTRIDE, A.seed, (uint32_t)d,
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

// the device buffers of one call, released on every way out
struct PpcScratch {
  double* params = nullptr;
  unsigned long long* flags = nullptr;
  ~PpcScratch() {
    if (params) (void)hipFree(params);
    if (flags) (void)hipFree(flags);
  }
};

extern "C" int pgb_ppc_draw(const double* mu_dev, int32_t D, int32_t K, int64_t n_rows, int64_t ld, int64_t row0,
                            const pgb_ppc_lik* lik, uint64_t seed, double* out_dev, int64_t ld_out, const double* y_dev,
                            int32_t* pit_counts_dev, int64_t* flags_host, void* stream) {
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
  if (out_dev) {  // the two ranges: the same matrix in place (K = 1), or apart
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
  hipStream_t sm = (hipStream_t)stream;
  PpcScratch sc;
  HIPCHK(hipMalloc((void**)&sc.flags, 2 * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(sc.flags, 0, 2 * sizeof(unsigned long long), sm));
  HIPCHK(hipMalloc((void**)&sc.params, hp.size() * sizeof(double)));
  HIPCHK(hipMemcpyAsync(sc.params, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, sm));
  PpcArgs A;
  A.mu = mu_dev;
  A.params = sc.params;
  A.offset = lik->offset_dev;
  A.y = y_dev;
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
  A.family = lik->family;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (K == 1) hipLaunchKernelGGL((k_ppc<true>), grid, dim3(PPC_BT), 0, sm, A);
  else hipLaunchKernelGGL((k_ppc<false>), grid, dim3(PPC_BT), 0, sm, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_ppc launch");
  unsigned long long hw[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hw, sc.flags, sizeof hw, hipMemcpyDeviceToHost, sm));
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_ppc");
  flags_host[0] = (int64_t)hw[0];
  flags_host[1] = (int64_t)hw[1];
  return PGB_OK;
}
