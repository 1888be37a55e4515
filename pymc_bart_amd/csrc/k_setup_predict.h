// k_setup_predict.h -- part of pgbart_hip.hip (not a standalone header): set-up kernels and the prediction kernel.
// ------------------------------------------------------------------ setup kernels
// X row-major [n][ldx] -> XT column-major [p][n_pad]; LDS-tiled 32x32 transpose so that both
// the read and the write are coalesced.  Also flags columns that contain NaN.
// 16-bit order keys of the column-major design matrix (see k_rows<..., F32>), one column at a time:
//   k_key_stage   the column's values rounded to float32 (a missing value: the canonical positive NaN, which a
//                 radix sort of the bit patterns puts behind +inf), the number of missing values counted;
//   (hipcub radix sort of the staged values)
//   k_key_bounds  boundary i (1 .. PGB_KEY_BOUNDS) = the value at rank i m / (PGB_KEY_BOUNDS + 1) of the m
//                 non-missing values: equi-depth bins, so that a split value shares its key with m / 65 535 rows;
//   k_key_assign  key(x) = number of boundaries <= float32(x) (binary search; non-decreasing in x), 0xFFFF if missing.
#define PGB_KEY_BOUNDS 65534
__global__ __launch_bounds__(BT) void k_key_stage(const double* __restrict__ col, float* __restrict__ out, long long n,
                                                  unsigned* __restrict__ n_missing) {
  unsigned miss = 0;
  for (long long i = (long long)blockIdx.x * BT + threadIdx.x; i < n; i += (long long)gridDim.x * BT) {
    const double x = col[i];
    const bool m = x != x;
    out[i] = m ? __uint_as_float(0x7FC00000u) : (float)x;
    miss += m ? 1u : 0u;
  }
  if (miss) atomicAdd(n_missing, miss);
}
__global__ __launch_bounds__(BT) void k_key_bounds(const float* __restrict__ sorted, long long n,
                                                   const unsigned* __restrict__ n_missing, float* __restrict__ bnd) {
  const long long m = n - (long long)*n_missing;
  for (int i = blockIdx.x * BT + threadIdx.x; i < PGB_KEY_BOUNDS; i += gridDim.x * BT)
    bnd[i] = m > 0 ? sorted[((long long)(i + 1) * m) / (PGB_KEY_BOUNDS + 1)] : __uint_as_float(0x7F800000u);
}
__global__ __launch_bounds__(BT) void k_key_assign(const double* __restrict__ col, const float* __restrict__ bnd,
                                                   uint16_t* __restrict__ key, long long n_pad) {
  for (long long i = (long long)blockIdx.x * BT + threadIdx.x; i < n_pad; i += (long long)gridDim.x * BT) {
    const double xd = col[i];
    const float x = (float)xd;
    int lo = 0, hi = PGB_KEY_BOUNDS;  // first boundary > x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (bnd[mid] <= x) lo = mid + 1;
      else hi = mid;
    }
    key[i] = xd != xd ? (uint16_t)0xFFFFu : (uint16_t)lo;
  }
}

__global__ __launch_bounds__(BT) void k_transpose(const double* __restrict__ X, long long ldx,
                                                  double* __restrict__ XT, long long n,
                                                  long long n_pad, int p, int32_t* col_nan) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const long long r0 = (long long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  for (int k = ty; k < 32; k += 8) {
    long long r = r0 + k;
    int c = c0 + tx;
    tile[k][tx] = (r < n && c < p) ? X[r * ldx + c] : 0.0;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    int c = c0 + k;
    long long r = r0 + tx;
    if (c < p && r < n_pad) {
      double x = tile[tx][k];
      XT[(size_t)c * n_pad + r] = x;
      if (x != x) col_nan[c] = 1;
    }
  }
}

__global__ void k_init_linp(LinP* p, long long n) {  // constant leaves everywhere
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = LinP{0.0, 0.0, -1};
}
// per-column max |x| (NaN ignored) of the column-major copy: one workgroup per column
__global__ __launch_bounds__(BT) void k_colmax(const double* __restrict__ XT, long long n, long long n_pad,
                                               double* __restrict__ amax) {
  __shared__ double sm[BT];
  const double* c = XT + (size_t)blockIdx.x * n_pad;
  double a = 0.0;
  for (long long i = threadIdx.x; i < n; i += BT) {
    double v = c[i];
    v = v < 0.0 ? -v : v;
    if (v > a) a = v;
  }
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int o = BT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o && sm[threadIdx.x + o] > sm[threadIdx.x]) sm[threadIdx.x] = sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) amax[blockIdx.x] = sm[0];
}
// SubsetSplit columns hold integer category codes 0 .. PGB_SUBSET_BITS - 1 (NaN = missing); anything else would be
// clamped by pgb_subset_code, so pgb_set_data refuses it: one workgroup per column, *bad = 1 + the first such column
__global__ __launch_bounds__(BT) void k_subset_check(const double* __restrict__ XT, long long n, long long n_pad,
                                                     const int32_t* __restrict__ rules, int* __restrict__ bad) {
  if (rules[blockIdx.x] != PGB_RULE_SUBSET) return;
  const double* c = XT + (size_t)blockIdx.x * n_pad;
  bool b = false;
  for (long long i = threadIdx.x; i < n; i += BT) {
    const double v = c[i];
    if (v == v && !(v >= 0.0 && v <= (double)(PGB_SUBSET_BITS - 1) && v == (double)(int)v)) b = true;
  }
  if (b) atomicMax(bad, (int)blockIdx.x + 1);
}
// any non-finite value, or one beyond +-limit, in `rows` rows of n values, `stride` apart?  -> *flag = 1 (the
// host's mapped word).  The linear predictor of a row must be finite and of bounded size: the likelihood tables are
// addressed by its bits (pgb_lphi_t, pgb_exp_t; PGB_MAX_OFFSET).
__global__ __launch_bounds__(BT) void k_nonfinite(const double* __restrict__ a, long long n, long long stride, int rows,
                                                  double limit, unsigned long long* __restrict__ flag) {
  bool b = false;
  for (int r = 0; r < rows; ++r)
    for (long long i = (long long)blockIdx.x * BT + threadIdx.x; i < n; i += (long long)gridDim.x * BT) {
      const double v = a[(size_t)r * stride + i];
      if (!(v - v == 0.0) || !(__builtin_fabs(v) <= limit)) b = true;
    }
  if (__ballot(b) && (threadIdx.x & 63) == 0) *flag = 1ull;
}
__global__ void k_fill_f64(double* a, long long n, double v) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}

__global__ void k_init_tree_lid(uint8_t* a, long long n, long long n_pad, int m) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pad * m) a[i] = (i % n_pad) < n ? 0 : PGB_ORPHAN;
}

__global__ void k_init_trees(DTree* trees, int m, long long n, double init_leaf) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  DTree* T = &trees[t];
  T->n_nodes = 1;
  T->n_leaves = 1;
  DNode z;
  memset(&z, 0, sizeof z);
  z.var = -1;
  z.cc_row = -1;
  z.cnt = (int32_t)n;
  z.value = init_leaf;
  T->nd[0] = z;
}

// integer split weights from the user's prior + their prefix sums (numeric contract:
// pgb_alpha_init / pgb_sample_var)
__global__ void k_init_alpha(const double* prior, double max_prior, long long* alpha, long long* cdfS, int p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    long long cs = 0;
    for (int j = 0; j < p; ++j) {
      const long long a = pgb_alpha_init(prior[j], max_prior);
      alpha[j] = a;
      cs += a;
      cdfS[j] = cs;
    }
  }
}

// ------------------------------------------------------------------ prediction
// (the packed tree records, PRED_* and the walk of one forest: pgb_pred_walk.h)
// CONT: every column follows the ContinuousSplit rule (the usual case): one compare per level.
template <bool LDSX, bool CONT>
__global__ __launch_bounds__(PRED_BT) void k_predict(PredTrees T, const int32_t* __restrict__ forest_idx,
                                                     int n_forests, int m, int K, int p,
                                                     const double* __restrict__ X, long long n_rows,
                                                     long long ldx, double* __restrict__ out) {
  extern __shared__ double s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
  if constexpr (LDSX) pred_stage_rows(s_x, X, row0, n_rows, ldx, p, lane);
  if (row >= n_rows) return;
  const PredRowX<LDSX> xval{s_x, X + row * ldx, lane};
  const bool clean = pred_wave_clean<CONT>(p, xval);
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  for (int d = blockIdx.y; d < n_forests; d += gridDim.y) {
    double acc[PGB_MAX_OUTPUTS];
    pred_walk_forest<CONT>(T, forest_idx + (size_t)d * m, m, K, clean, xval, stk_node, stk_w, acc);
    for (int o = 0; o < K; ++o) out[((size_t)d * K + o) * n_rows + row] = acc[o];
  }
}
