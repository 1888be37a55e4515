// k_shap_interaction.h -- part of pgbart_hip.hip (not a standalone header): exact SHAP interaction values of stored
// draws (include/pgbart_shap_interaction.h holds the numeric contract AND the evaluation itself: pgb_shapx_row is
// compiled from that one text by the host and by this kernel), the kernel and the host side of
// pgb_predict_shap_interactions.
//
//   k_shap_interaction  k_shap's shape: one wave per workgroup, lane = row, grid = (row tiles of 64, picks); y strides
//           when the picks exceed the grid limit.  The rows of a tile are staged in LDS (transposed [column][lane], pad
//           of one) when p <= PRED_LDS_MAXP and read from global memory beyond that.  A lane walks the leaf records of
//           its pick's trees -- wave-uniform reads, pos[] included -- and adds each term's cells to ITS column of
//           out[pick][k][a][b][row], which it has zeroed itself: the accumulators live in out, the stores are coalesced
//           over the rows, nobody else touches them, so there are no atomics and the order of the additions is the
//           header's -- whatever the grid, the row blocks and the column subset are.  A leaf of at most PGB_SHAP_FAST_U
//           slots keeps its slots in registers (the header's loops unrolled); a longer path (up to PGB_SHAPX_MAX_U
//           slots: the host refuses more) uses private memory.  K is a run-time value: one instance serves every K.
#include <algorithm>

#include "pgbart_shap_interaction.h"

template <bool LDSX, bool CONT>
__global__ __launch_bounds__(PRED_BT) void k_shap_interaction(pgb_shap_view V, const int32_t* __restrict__ forest_idx, int m,
                                                              int p, const double* __restrict__ X, long long n_rows,
                                                              long long ldx, const int32_t* __restrict__ pos, int q,
                                                              const int32_t* __restrict__ picks, int n_picks,
                                                              double* __restrict__ out) {
  extern __shared__ double shapx_s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
  if constexpr (LDSX) {
    const long long rows_here = n_rows - row0 < PRED_BT ? n_rows - row0 : PRED_BT;
    if (ldx == p) {  // the block of rows is contiguous: fully coalesced copy
      const double* __restrict__ src = X + row0 * ldx;
      const int tot = (int)rows_here * p;
      for (int i = lane; i < tot; i += PRED_BT) shapx_s_x[(i % p) * 65 + i / p] = src[i];
    } else {
      for (int r = 0; r < (int)rows_here; ++r)
        for (int j = lane; j < p; j += PRED_BT) shapx_s_x[j * 65 + r] = X[(row0 + r) * ldx + j];
    }
    __syncthreads();
  }
  if (row >= n_rows) return;
  const pgb_shap_view v = V;
  const size_t per_pick = (size_t)v.K * (size_t)q * (size_t)q * (size_t)n_rows;
  for (int s = blockIdx.y; s < n_picks; s += gridDim.y) {
    const int32_t* __restrict__ forest = forest_idx + (size_t)picks[s] * m;
    double* __restrict__ Phi = out + (size_t)s * per_pick + row;
    if constexpr (LDSX) pgb_shapx_row(&v, forest, m, shapx_s_x + lane, 65, CONT, pos, q, 0, Phi, n_rows);
    else pgb_shapx_row(&v, forest, m, X + row * ldx, 1, CONT, pos, q, 0, Phi, n_rows);
  }
}

static thread_local double g_shapx_ms = -1.0;
extern "C" int pgb_shap_interactions_kernel_ms(double* ms_out) {
  if (!ms_out) return fail(PGB_E_INVALID, "null argument");
  *ms_out = g_shapx_ms;
  return PGB_OK;
}

extern "C" int pgb_predict_shap_interactions(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests,
                                             int32_t m, const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx,
                                             const int32_t* cols_host, int32_t n_cols, const int32_t* picks_host,
                                             int32_t n_picks, double* out_dev, double* base_host_out, void* stream) {
#define SHAPX_ "pgb_predict_shap_interactions: "
  if (!trees) return fail(PGB_E_INVALID, SHAPX_ "trees is null");
  if (!forest_tree_idx) return fail(PGB_E_INVALID, SHAPX_ "forest_tree_idx is null");
  if (!X_dev) return fail(PGB_E_INVALID, SHAPX_ "X_dev is null");
  if (!cols_host) return fail(PGB_E_INVALID, SHAPX_ "cols_host is null");
  if (!picks_host) return fail(PGB_E_INVALID, SHAPX_ "picks_host is null");
  if (!out_dev) return fail(PGB_E_INVALID, SHAPX_ "out_dev is null");
  if (!base_host_out) return fail(PGB_E_INVALID, SHAPX_ "base_host_out is null");
  if (n_forests < 1 || m < 1 || p < 1) return fail(PGB_E_INVALID, SHAPX_ "n_forests, m and p must be >= 1");
  if (n_cols < 1) return fail(PGB_E_INVALID, SHAPX_ "n_cols must be >= 1");
  if (n_picks < 1) return fail(PGB_E_INVALID, SHAPX_ "n_picks must be >= 1");
  if (n_rows < 1) return fail(PGB_E_INVALID, SHAPX_ "n_rows must be >= 1");
  if (ldx < p) return fail(PGB_E_INVALID, SHAPX_ "ldx must be >= p");
  const long long gx = (n_rows + PRED_BT - 1) / PRED_BT;
  if (gx > 0x7fffffffLL) return fail(PGB_E_INVALID, SHAPX_ "n_rows exceeds 2^31 - 1 tiles of 64 rows");
  for (int c = 0; c < n_cols; ++c)
    if (cols_host[c] < 0 || cols_host[c] >= p) {
      snprintf(g_err, sizeof g_err, SHAPX_ "cols_host[%d] = %d is outside [0, p = %d)", c, (int)cols_host[c], (int)p);
      return PGB_E_INVALID;
    }
  {  // a column named twice (sorted pairs: p itself may be far larger than n_cols)
    std::vector<std::pair<int32_t, int32_t>> by(n_cols);
    for (int c = 0; c < n_cols; ++c) by[c] = {cols_host[c], c};
    std::sort(by.begin(), by.end());
    for (int c = 1; c < n_cols; ++c)
      if (by[c].first == by[c - 1].first) {
        snprintf(g_err, sizeof g_err, SHAPX_ "cols_host[%d] = %d repeats cols_host[%d]", (int)by[c].second, (int)by[c].first,
                 (int)by[c - 1].second);
        return PGB_E_INVALID;
      }
  }
  for (int s = 0; s < n_picks; ++s)
    if (picks_host[s] < 0 || picks_host[s] >= n_forests) {
      snprintf(g_err, sizeof g_err, SHAPX_ "picks_host[%d] = %d is outside [0, n_forests = %d)", s, (int)picks_host[s],
               (int)n_forests);
      return PGB_E_INVALID;
    }
  const int K = trees->n_outputs;
  if (K < 1 || K > PGB_MAX_OUTPUTS) return fail(PGB_E_INVALID, "n_outputs");
  // out_dev holds n_picks K n_cols n_cols n_rows doubles: their bytes must fit a 64-bit size (and the index arithmetic)
  {
    const uint64_t lim = (uint64_t)1 << 60;
    uint64_t cells = (uint64_t)n_picks;
    const uint64_t f[4] = {(uint64_t)K, (uint64_t)n_cols, (uint64_t)n_cols, (uint64_t)n_rows};
    for (int i = 0; i < 4; ++i) {
      if (cells > lim / f[i])
        return fail(PGB_E_INVALID, SHAPX_ "out_dev of n_picks x K x n_cols x n_cols x n_rows doubles overflows a 64-bit size");
      cells *= f[i];
    }
  }
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;

  ShapScratch sc;
  const int prc = pgb_shap_pack_build(trees, p, &sc.pack);  // once per call
  if (prc == -1) return fail(PGB_E_NOMEM, SHAPX_ "the leaf records do not fit host memory");
  if (prc != 0) return fail(PGB_E_INVALID, SHAPX_ "the history's leaf paths number more than 2^31 - 1 splits");
  {
    const int slots = pgb_shapx_pack_slots(&sc.pack);
    if (slots > PGB_SHAPX_MAX_U) {
      snprintf(g_err, sizeof g_err,
               SHAPX_ "trees holds a leaf of %d slots (the columns of its path and its regressor), the limit is %d "
                      "(PGB_SHAPX_MAX_U)", slots, (int)PGB_SHAPX_MAX_U);
      return PGB_E_INVALID;
    }
  }
  const bool lin = trees->slope && trees->xbar && trees->svar;
  {
    const pgb_shap_view hv = pgb_shap_pack_view(&sc.pack, sc.pack.buf, trees->value, lin ? trees->slope : nullptr, K);
    for (int s = 0; s < n_picks; ++s)
      pgb_shap_base(&hv, forest_tree_idx + (size_t)picks_host[s] * m, m, base_host_out + (size_t)s * K);
  }
  hipStream_t sm = (hipStream_t)stream;
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);
  if (rc != PGB_OK) return rc;
  sc.db = pk.db;
  // [the header's pack | the picks | pos[p]]
  const size_t o_picks = (sc.pack.bytes + 7) & ~(size_t)7;
  const size_t o_pos = o_picks + (size_t)n_picks * sizeof(int32_t);
  std::vector<uint8_t> hb(o_pos + (size_t)p * sizeof(int32_t));
  memcpy(hb.data(), sc.pack.buf, sc.pack.bytes);
  memcpy(hb.data() + o_picks, picks_host, (size_t)n_picks * sizeof(int32_t));
  {
    int32_t* pos = (int32_t*)(hb.data() + o_pos);
    for (int j = 0; j < p; ++j) pos[j] = -1;
    for (int c = 0; c < n_cols; ++c) pos[cols_host[c]] = c;
  }
  HIPCHK(hipMalloc((void**)&sc.rec, hb.size()));
  HIPCHK(hipMemcpyAsync(sc.rec, hb.data(), hb.size(), hipMemcpyHostToDevice, sm));
  const pgb_shap_view dv = pgb_shap_pack_view(&sc.pack, sc.rec, pk.T.value, pk.T.slope, K);
  const int32_t* picks_dev = (const int32_t*)(sc.rec + o_picks);
  const int32_t* pos_dev = (const int32_t*)(sc.rec + o_pos);
  dim3 grid((unsigned)gx, (unsigned)(n_picks < 65535 ? n_picks : 65535));
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
#define LAUNCH_SHAPX(L_, C_)                                                                                            \
  hipLaunchKernelGGL((k_shap_interaction<L_, C_>), grid, dim3(PRED_BT), lds, sm, dv, pk.fidx, (int)m, (int)p, X_dev,    \
                     (long long)n_rows, (long long)ldx, pos_dev, (int)n_cols, picks_dev, (int)n_picks, out_dev)
  WalkTimer wt(sm);
  if (ldsx) {
    if (pk.cont) LAUNCH_SHAPX(true, true);
    else LAUNCH_SHAPX(true, false);
  } else {
    if (pk.cont) LAUNCH_SHAPX(false, true);
    else LAUNCH_SHAPX(false, false);
  }
#undef LAUNCH_SHAPX
#undef SHAPX_
  hipError_t e = hipGetLastError();
  wt.launched();
  hipError_t e2 = hipStreamSynchronize(sm);
  g_shapx_ms = -1.0;
  if (e == hipSuccess && e2 == hipSuccess && wt.a) {
    wt.synced();
    g_shapx_ms = g_walk_ms;
  }
  if (e != hipSuccess) return fail_hip(e, "k_shap_interaction launch");
  if (e2 != hipSuccess) return fail_hip(e2, "k_shap_interaction");
  return PGB_OK;
}
