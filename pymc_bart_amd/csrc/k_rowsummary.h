// k_rowsummary.h -- part of pgbart_hip.hip (not a standalone header): mean, variance, quantiles and the HDI of every
// column of a [D][ld] device matrix over its D draws (pgb_row_summary; the numeric contract -- the order, every
// formula and the order of every sum -- is include/pgbart_rowsummary.h, whose pgb_rowsum_column a host build
// evaluates to the same bits).
//
// A workgroup of 256 threads owns C = max(1, min(8, 16384 / Dp)) adjacent columns, Dp the next power of two >= D,
// and keeps their C x Dp order keys (64-bit integers, padded with the largest key) in dynamic LDS: at most 128 KiB,
// which one workgroup of a gfx950 CU may take once the kernel has opted in.  The matrix has its columns contiguous,
// so at C = 8 the eight columns of one draw are one 64-byte segment and consecutive lanes read consecutive addresses.
//   1. load: element e of the C x D tile is column e mod C of draw e / C; its key goes to keys[column][draw];
//   2. sort: ONE bitonic network over all C x Dp keys -- the columns are aligned power-of-two segments, so with the
//      direction taken from the index within the column every column is sorted ascending by the same compare-exchange
//      steps, and all 256 threads share every step whatever C is (a column of 16384 draws gets all four waves);
//   3. values: the keys become t = f(a + off) in place (pgb_rowsum_value);
//   4. statistics: one wave per column.  Lane l forms partial l of each lane sum and of the HDI scan, the partials go
//      through LDS and are combined in lane order by the contract's own functions; lane j gathers quantile j.
// No atomics, no floating-point reduction outside the contract's order.  Stages 1 and 2, the launch shape and the LDS
// opt-in are functions of their own: k_rowscore (k_rowscore.h) starts from the same sorted tile.
#define ROWSUM_BT 256
#define ROWSUM_WAVES (ROWSUM_BT / 64)
#define ROWSUM_MAX_KEYS 16384  /* keys of one workgroup: PGB_ROWSUM_MAX_DRAWS x 1 column = 2048 x 8 columns */

extern __shared__ unsigned long long rowsum_keys[];  // [C][Dp] keys, then the same bytes as doubles t

struct rowsum_q {
  double q[PGB_ROWSUM_MAX_Q];
};

// Stages 1 and 2, shared with k_rowscore (k_rowscore.h): the keys of the workgroup's C x D tile of a [D][ld], columns
// c0 .. c0 + C (columns beyond n_cols repeat the last one), padded to [C][Dp]; ends with a barrier
__device__ __forceinline__ void rowsum_load_tile(unsigned long long* keys, const double* __restrict__ a, int D, int lg, int lgC,
                                                 long long c0, long long n_cols, long long ld) {
  const int tid = threadIdx.x;
  const int Dp = 1 << lg, C = 1 << lgC;
  const int total = C << lg;
  const int n_el = D << lgC;
#pragma unroll 4
  for (int e = tid; e < n_el; e += ROWSUM_BT) {
    const int c = e & (C - 1), d = e >> lgC;
    long long gc = c0 + c;
    if (gc >= n_cols) gc = n_cols - 1;
    keys[(c << lg) + d] = pgb_rowsum_key(a[(size_t)d * (size_t)ld + (size_t)gc]);
  }
  if (D < Dp)
    for (int i = tid; i < total; i += ROWSUM_BT)
      if ((i & (Dp - 1)) >= D) keys[i] = PGB_ROWSUM_PAD_KEY;
  __syncthreads();
}

// ... and every column of the tile ascending; ends with a barrier
__device__ __forceinline__ void rowsum_sort_tile(unsigned long long* keys, int lg, int lgC) {
  const int tid = threadIdx.x;
  const int Dp = 1 << lg;
  const int half = (1 << (lg + lgC)) >> 1;
  for (int k = 2; k <= Dp; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < half; p += ROWSUM_BT) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i | j;
        const bool up = (i & k & (Dp - 1)) == 0;  // (k == Dp: the bit above the column's index -- ascending)
        const unsigned long long x = keys[i], y = keys[l];
        if ((x > y) == up) {
          keys[i] = y;
          keys[l] = x;
        }
      }
      __syncthreads();
    }
}

__global__ __launch_bounds__(ROWSUM_BT) void k_rowsum(const double* __restrict__ a, int D, int lg, int lgC, long long n_cols,
                                                      long long ld, const double* __restrict__ off, int transform, rowsum_q qs,
                                                      int n_q, int hdi_k, double* __restrict__ out) {
  __shared__ double s_part[ROWSUM_WAVES][PGB_ROWSUM_LANES];
  __shared__ int32_t s_idx[ROWSUM_WAVES][PGB_ROWSUM_LANES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Dp = 1 << lg, C = 1 << lgC;
  const int total = C << lg;
  const long long c0 = (long long)blockIdx.x << lgC;
  unsigned long long* keys = rowsum_keys;

  rowsum_load_tile(keys, a, D, lg, lgC, c0, n_cols, ld);  // ---- 1. the tile's keys, the padding
  rowsum_sort_tile(keys, lg, lgC);                        // ---- 2. every column ascending

  // ---- 3. t = f(a + off), in place
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
  double* tv = (double*)rowsum_keys;
  for (int i = tid; i < total; i += ROWSUM_BT) {
    if ((i & (Dp - 1)) >= D) continue;
    long long gc = c0 + (i >> lg);
    if (gc >= n_cols) gc = n_cols - 1;
    const double ov = off ? off[gc] : 0.0;
    tv[i] = pgb_rowsum_value(pgb_rowsum_unkey(keys[i]), off != nullptr, ov, transform, &tb);
  }
  __syncthreads();

  // ---- 4. one wave per column (every wave takes every barrier: a wave without a column repeats column 0)
  for (int cb = 0; cb < C; cb += ROWSUM_WAVES) {
    const int c = cb + wave;
    const bool act = c < C && c0 + c < n_cols;
    const double* t = tv + ((size_t)(act ? c : 0) << lg);
    s_part[wave][lane] = pgb_rowsum_part_sum(t, D, lane);
    __syncthreads();
    const double mean = pgb_rowsum_lanes(s_part[wave]) / (double)D;
    __syncthreads();
    s_part[wave][lane] = pgb_rowsum_part_sq(t, D, lane, mean);
    __syncthreads();
    const double var = pgb_rowsum_lanes(s_part[wave]) / (double)(D - 1);
    __syncthreads();
    double lo = 0.0, hi = 0.0;
    if (hdi_k >= D) {
      lo = t[0];
      hi = t[D - 1];
    } else if (hdi_k > 0) {
      double w;
      s_idx[wave][lane] = pgb_rowsum_hdi_part(t, D, hdi_k, lane, &w);
      s_part[wave][lane] = w;
      __syncthreads();
      const int is = pgb_rowsum_hdi_combine(s_part[wave], s_idx[wave]);
      lo = t[is];
      hi = t[is + hdi_k];
      __syncthreads();
    }
    if (act) {
      const size_t col = (size_t)(c0 + c), n = (size_t)n_cols;
      if (lane == 0) {
        out[col] = mean;
        out[n + col] = var;
        out[(size_t)(2 + n_q) * n + col] = lo;
        out[(size_t)(3 + n_q) * n + col] = hi;
      }
      if (lane < n_q) out[(size_t)(2 + lane) * n + col] = pgb_rowsum_quantile(t, D, qs.q[lane]);
    }
  }
}

// The launch shape of both kernels: Dp = 1 << lg, C = 1 << lgC columns per workgroup, gx workgroups, lds bytes of keys
struct rowsum_tiling {
  int lg, lgC;
  long long gx;
  size_t lds;
};

static int rowsum_tile(int32_t D, int64_t n_cols, rowsum_tiling* g) {
  g->lg = 1;
  while ((1 << g->lg) < D) ++g->lg;
  g->lgC = 3;
  while (g->lgC > 0 && ((1 << g->lg) << g->lgC) > ROWSUM_MAX_KEYS) --g->lgC;
  g->gx = (n_cols + (1ll << g->lgC) - 1) >> g->lgC;
  if (g->gx > 0x7FFFFFFFll) return fail(PGB_E_UNSUPPORTED, "n_cols too large for one call");
  g->lds = ((size_t)1 << (g->lg + g->lgC)) * sizeof(unsigned long long);
  return PGB_OK;
}

// more than 64 KiB of dynamic LDS is an opt-in, per kernel and per device (opted: the devices that have it, the caller's)
static int rowsum_lds_opt_in(const void* kernel, std::vector<int>* opted, const char* what) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  bool have = false;
  for (int d : *opted) have = have || d == dev;
  if (!have) {
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(ROWSUM_MAX_KEYS * sizeof(unsigned long long)));
    if (e != hipSuccess) return fail_hip(e, what);
    opted->push_back(dev);
  }
  return PGB_OK;
}

extern "C" int pgb_row_summary(const double* a_dev, int32_t D, int64_t n_cols, int64_t ld, const double* offset_dev,
                               int32_t transform, const double* q_host, int32_t n_q, int32_t hdi_k, double* out_dev,
                               void* stream) {
  if (!a_dev || !out_dev) return fail(PGB_E_INVALID, "null argument");
  if (n_cols < 1 || ld < n_cols) return fail(PGB_E_INVALID, "n_cols must be >= 1 and ld >= n_cols");
  if (D < 2) return fail(PGB_E_INVALID, "a row summary needs at least 2 draws");
  if (D > PGB_ROWSUM_MAX_DRAWS) {
    snprintf(g_err, sizeof g_err, "pgb_row_summary takes at most " PGB_STR(PGB_ROWSUM_MAX_DRAWS) " draws, %d given (thin them: draws=)",
             (int)D);
    return PGB_E_INVALID;
  }
  if (n_q < 0 || n_q > PGB_ROWSUM_MAX_Q) {
    snprintf(g_err, sizeof g_err, "n_q must be in [0, " PGB_STR(PGB_ROWSUM_MAX_Q) "], got %d", (int)n_q);
    return PGB_E_INVALID;
  }
  if (n_q > 0 && !q_host) return fail(PGB_E_INVALID, "null argument");
  rowsum_q qs;
  for (int j = 0; j < PGB_ROWSUM_MAX_Q; ++j) qs.q[j] = 0.0;
  for (int j = 0; j < n_q; ++j) {
    if (!(q_host[j] >= 0.0 && q_host[j] <= 1.0)) {
      snprintf(g_err, sizeof g_err, "quantile %d must be in [0, 1], got %g", j, q_host[j]);
      return PGB_E_INVALID;
    }
    qs.q[j] = q_host[j];
  }
  if (hdi_k < 0) return fail(PGB_E_INVALID, "hdi_k must be >= 0");
  if (transform < 0 || transform >= PGB_ROWSUM_N_TRANSFORMS) {
    snprintf(g_err, sizeof g_err, "unknown transform %d", (int)transform);
    return PGB_E_INVALID;
  }
  rowsum_tiling g;
  int rc = rowsum_tile(D, n_cols, &g);
  if (rc != PGB_OK) return rc;
  static std::vector<int> opted;
  rc = rowsum_lds_opt_in((const void*)k_rowsum, &opted, "k_rowsum: dynamic LDS opt-in");
  if (rc != PGB_OK) return rc;
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rowsum, dim3((unsigned)g.gx), dim3(ROWSUM_BT), g.lds, sm, a_dev, (int)D, g.lg, g.lgC, (long long)n_cols,
                     (long long)ld, offset_dev, (int)transform, qs, (int)n_q, (int)hdi_k, out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_rowsum launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_rowsum");
  return PGB_OK;
}
