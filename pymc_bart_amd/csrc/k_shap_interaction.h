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
  if constexpr (LDSX) pred_stage_rows(shapx_s_x, X, row0, n_rows, ldx, p, lane);
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
  PredCall pc("pgb_predict_shap_interactions");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(cols_host, "cols_host");
  pc.null(picks_host, "picks_host");
  pc.null(out_dev, "out_dev");
  pc.null(base_host_out, "base_host_out");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(n_cols, "n_cols");
  pc.at_least_one(n_picks, "n_picks");
  pc.at_least_one(n_rows, "n_rows");
  pc.ld(ldx, p, "ldx");
  long long gx = 0;
  pc.tiles(n_rows, &gx);
  pc.index_vector(cols_host, (size_t)n_cols, p, "cols_host", "p");
  pc.distinct(cols_host, n_cols);
  pc.index_vector(picks_host, (size_t)n_picks, n_forests, "picks_host", "n_forests");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.n_outputs(trees);
  const int K = trees->n_outputs;
  pc.cells_fit({n_picks, K, n_cols, n_cols, n_rows}, "n_picks x K x n_cols x n_cols x n_rows");
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;

  ShapScratch sc;
  const int prc = pgb_shap_pack_build(trees, p, &sc.pack);  // once per call
  if (prc == -1) return pc.refuse(PGB_E_NOMEM, "the leaf records do not fit host memory");
  if (prc != 0) return pc.refuse(PGB_E_INVALID, "the history's leaf paths number more than 2^31 - 1 splits");
  const int slots = pgb_shapx_pack_slots(&sc.pack);
  if (slots > PGB_SHAPX_MAX_U)
    return pc.refuse(PGB_E_INVALID, "trees holds a leaf of %d slots (the columns of its path and its regressor), the limit is %d "
                                    "(PGB_SHAPX_MAX_U)", slots, (int)PGB_SHAPX_MAX_U);
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
  WalkTimer wt(sm);
  dispatch_bools(ldsx, pk.cont, [&](auto L, auto C) {
    hipLaunchKernelGGL((k_shap_interaction<L(), C()>), grid, dim3(PRED_BT), lds, sm, dv, pk.fidx, (int)m, (int)p, X_dev,
                       (long long)n_rows, (long long)ldx, pos_dev, (int)n_cols, picks_dev, (int)n_picks, out_dev);
  });
  return finish_walk(hipGetLastError(), sm, wt, &g_shapx_ms, "k_shap_interaction");
}
