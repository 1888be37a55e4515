// k_ice.h -- part of pgbart_hip.hip (not a standalone header): individual conditional expectation curves, fused into
// the tree walk of k_predict (include/pgbart_ice.h holds the numeric contract), and the host side of pgb_predict_ice.
//
// The probe row of a curve is the instance's row everywhere except the swept column j, so nothing of it is ever
// built: one wave per workgroup, lane = sweep row; the instance row sits in LDS (p doubles; every lane of a walk step
// that tests another column than j reads ONE address there, which the LDS serves as a broadcast) and the lane's own
// X[i][j] in a register: xval(c) = c == j ? xs : inst[c].  The walk is pred_walk_forest (pgb_pred_walk.h), so acc holds
// the bits of pgb_predict; the reduction over the picks is a running sum in registers, in pick order, divided once and
// stored coalesced.  Grid = (row tiles of 64, instances, columns); y and z stride when a sweep exceeds the grid limits.
// The instance rows wider than PGB_ICE_LDS_MAXP are read from global memory (a wave-uniform address per walk step).
extern __shared__ double ice_s_inst[];  // LDSI: [p]

template <bool LDSI, bool CONT, bool K1>
__global__ __launch_bounds__(PRED_BT) void k_ice(PredTrees T, const int32_t* __restrict__ forest_idx, int m, int K_rt, int p,
                                                 const double* __restrict__ X, long long n_rows, long long ldx,
                                                 const double* __restrict__ inst, int n_inst, long long ldi,
                                                 const int32_t* __restrict__ cols, int n_cols,
                                                 const int32_t* __restrict__ picks, int n_picks, double* __restrict__ out) {
  const int K = K1 ? 1 : K_rt;
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * PRED_BT + lane;
  const bool live = row < n_rows;  // (lane 0 always is)
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  const double denom = (double)n_picks;
  for (int c = blockIdx.z; c < n_cols; c += gridDim.z) {
    const int j = cols[c];
    const double xs = live ? X[row * ldx + j] : 0.0;
    for (int r = blockIdx.y; r < n_inst; r += gridDim.y) {
      const double* __restrict__ irow = inst + (size_t)r * ldi;
      if constexpr (LDSI) {
        __syncthreads();  // (the previous curve's walks have read the row they staged)
        for (int i = lane; i < p; i += PRED_BT) ice_s_inst[i] = irow[i];
        __syncthreads();
      }
      auto xval = [&](int v) -> double {
        if constexpr (LDSI) return v == j ? xs : ice_s_inst[v];
        else return v == j ? xs : irow[v];
      };
      // wave-uniform: no missing value in any probe row of this wave (the instance row outside j, the lanes' xs)
      bool clean = CONT;
      if (CONT) {
        bool nan = xs != xs;
        for (int v = lane; v < p; v += PRED_BT) {
          double w;
          if constexpr (LDSI) w = ice_s_inst[v];
          else w = irow[v];
          nan = nan || (v != j && w != w);
        }
        clean = __ballot(nan) == 0ull;
      }
      if (!live) continue;
      const int32_t* __restrict__ pk = picks + ((size_t)c * n_inst + r) * n_picks;
      double sum[K1 ? 1 : PGB_MAX_OUTPUTS];
      for (int s = 0; s < n_picks; ++s) {
        double acc[K1 ? 1 : PGB_MAX_OUTPUTS];
        pred_walk_forest<CONT>(T, forest_idx + (size_t)pk[s] * m, m, K, clean, xval, stk_node, stk_w, acc);
        if (s == 0)
          for (int o = 0; o < K; ++o) sum[o] = acc[o];
        else
          for (int o = 0; o < K; ++o) sum[o] = sum[o] + acc[o];
      }
      double* __restrict__ dst = out + ((size_t)c * n_inst + r) * K * (size_t)n_rows + row;
      for (int o = 0; o < K; ++o) dst[(size_t)o * n_rows] = sum[o] / denom;
    }
  }
}

extern "C" int pgb_predict_ice(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                               const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx, const double* inst_dev,
                               int32_t n_inst, int64_t ldi, const int32_t* cols_host, int32_t n_cols,
                               const int32_t* picks_host, int32_t n_picks, double* out_dev, void* stream) {
  PredCall pc("pgb_predict_ice");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(inst_dev, "inst_dev");
  pc.null(cols_host, "cols_host");
  pc.null(picks_host, "picks_host");
  pc.null(out_dev, "out_dev");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(n_inst, "n_inst");
  pc.at_least_one(n_cols, "n_cols");
  pc.at_least_one(n_picks, "n_picks");
  pc.at_least_one(n_rows, "n_rows");
  pc.ld(ldx, p, "ldx");
  pc.ld(ldi, p, "ldi");
  long long gx = 0;
  pc.tiles(n_rows, &gx);
  const size_t n_pk = (size_t)n_cols * (size_t)n_inst * (size_t)n_picks;
  pc.index_vector(cols_host, (size_t)n_cols, p, "cols_host", "p");
  pc.index_vector(picks_host, n_pk, n_forests, "picks_host", "n_forests");
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;
  const int K = trees->n_outputs;
  hipStream_t sm = (hipStream_t)stream;
  DevBuf sel;  // [n_cols | n_cols n_inst n_picks]: the columns, then the picks
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);  // once per call
  if (rc != PGB_OK) return rc;
  std::vector<int32_t> hs((size_t)n_cols + n_pk);
  memcpy(hs.data(), cols_host, (size_t)n_cols * sizeof(int32_t));
  memcpy(hs.data() + n_cols, picks_host, n_pk * sizeof(int32_t));
  HIPCHK(hipMalloc((void**)&sel.p, hs.size() * sizeof(int32_t)));
  HIPCHK(hipMemcpyAsync(sel.p, hs.data(), hs.size() * sizeof(int32_t), hipMemcpyHostToDevice, sm));
  const int32_t* cols_dev = (const int32_t*)sel.p;
  const int32_t* picks_dev = cols_dev + n_cols;
  // grid = (row tiles, instances, columns); the kernel strides over what y and z cannot hold
  dim3 grid((unsigned)gx, (unsigned)(n_inst < 65535 ? n_inst : 65535), (unsigned)(n_cols < 65535 ? n_cols : 65535));
  const bool ldsi = p <= PGB_ICE_LDS_MAXP;
  const size_t lds = ldsi ? (size_t)p * sizeof(double) : 0;
  const PredTrees T = pk.T;
  WalkTimer wt(sm);
  dispatch_bools(ldsi, pk.cont, K == 1, [&](auto L, auto C, auto K1) {
    hipLaunchKernelGGL((k_ice<L(), C(), K1()>), grid, dim3(PRED_BT), lds, sm, T, pk.fidx, (int)m, K, (int)p, X_dev,
                       (long long)n_rows, (long long)ldx, inst_dev, (int)n_inst, (long long)ldi, cols_dev, (int)n_cols,
                       picks_dev, (int)n_picks, out_dev);
  });
  return finish_walk(hipGetLastError(), sm, wt, nullptr, "k_ice");
}
