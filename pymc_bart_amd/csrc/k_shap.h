// k_shap.h -- part of pgbart_hip.hip (not a standalone header): exact Shapley attributions of stored draws
// (include/pgbart_shap.h holds the numeric contract AND the evaluation itself: pgb_shap_row is compiled from that one
// text by the host and by this kernel), the kernel and the host side of pgb_predict_shap.
//
//   k_shap  one wave per workgroup, lane = row, grid = (row tiles of 64, picks); y strides when the picks exceed the
//           grid limit.  The rows of a tile are staged in LDS as k_predict stages them (transposed [column][lane], pad
//           of one) when p <= PRED_LDS_MAXP and read from global memory beyond that.  A lane walks the leaf records of
//           its pick's trees -- wave-uniform reads: every lane of a wave is at the same leaf -- and adds each leaf's
//           terms to ITS column of out[pick][k][j][row]: the stores are coalesced over the rows, nobody else touches
//           them, so there are no atomics and the order of the additions is the header's.  A leaf of at most
//           PGB_SHAP_FAST_U slots keeps its slots in registers (the header's loops unrolled); a longer path uses
//           private memory, as the walk's stack does.
#include "pgbart_shap.h"

template <bool LDSX, bool CONT, bool K1>
__global__ __launch_bounds__(PRED_BT) void k_shap(pgb_shap_view V, const int32_t* __restrict__ forest_idx, int m, int p,
                                                  const double* __restrict__ X, long long n_rows, long long ldx,
                                                  const int32_t* __restrict__ picks, int n_picks, double* __restrict__ out) {
  extern __shared__ double shap_s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
  if constexpr (LDSX) pred_stage_rows(shap_s_x, X, row0, n_rows, ldx, p, lane);
  if (row >= n_rows) return;
  pgb_shap_view v = V;
  if (K1) v.K = 1;
  const size_t per_pick = (size_t)v.K * (size_t)p * (size_t)n_rows;
  for (int s = blockIdx.y; s < n_picks; s += gridDim.y) {
    const int32_t* __restrict__ forest = forest_idx + (size_t)picks[s] * m;
    double* __restrict__ phi = out + (size_t)s * per_pick + row;
    if constexpr (LDSX) pgb_shap_row(&v, forest, m, shap_s_x + lane, 65, p, CONT, phi, n_rows);
    else pgb_shap_row(&v, forest, m, X + row * ldx, 1, p, CONT, phi, n_rows);
  }
}

// every device buffer of one call, released on every way out
struct ShapScratch {
  uint8_t* rec = nullptr;  // [the header's pack | the picks]
  pgb_shap_pack pack;
  ShapScratch() { memset(&pack, 0, sizeof pack); }
  ~ShapScratch() {
    if (rec) (void)hipFree(rec);
    pgb_shap_pack_free(&pack);
  }
};

static thread_local double g_shap_ms = -1.0;
extern "C" int pgb_shap_kernel_ms(double* ms_out) {
  if (!ms_out) return fail(PGB_E_INVALID, "null argument");
  *ms_out = g_shap_ms;
  return PGB_OK;
}

extern "C" int pgb_predict_shap(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                                const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx, const int32_t* picks_host,
                                int32_t n_picks, double* out_dev, double* base_host_out, void* stream) {
  PredCall pc("pgb_predict_shap");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(picks_host, "picks_host");
  pc.null(out_dev, "out_dev");
  pc.null(base_host_out, "base_host_out");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(n_picks, "n_picks");
  pc.at_least_one(n_rows, "n_rows");
  pc.ld(ldx, p, "ldx");
  long long gx = 0;
  pc.tiles(n_rows, &gx);
  pc.index_vector(picks_host, (size_t)n_picks, n_forests, "picks_host", "n_forests");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.n_outputs(trees);
  const int K = trees->n_outputs;
  pc.cells_fit({n_picks, K, p, n_rows}, "n_picks x K x p x n_rows");
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;

  ShapScratch sc;
  const int prc = pgb_shap_pack_build(trees, p, &sc.pack);  // once per call
  if (prc == -1) return pc.refuse(PGB_E_NOMEM, "the leaf records do not fit host memory");
  if (prc != 0) return pc.refuse(PGB_E_INVALID, "the history's leaf paths number more than 2^31 - 1 splits");
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
  const size_t o_picks = (sc.pack.bytes + 7) & ~(size_t)7;
  std::vector<uint8_t> hb(o_picks + (size_t)n_picks * sizeof(int32_t));
  memcpy(hb.data(), sc.pack.buf, sc.pack.bytes);
  memcpy(hb.data() + o_picks, picks_host, (size_t)n_picks * sizeof(int32_t));
  HIPCHK(hipMalloc((void**)&sc.rec, hb.size()));
  HIPCHK(hipMemcpyAsync(sc.rec, hb.data(), hb.size(), hipMemcpyHostToDevice, sm));
  const pgb_shap_view dv = pgb_shap_pack_view(&sc.pack, sc.rec, pk.T.value, pk.T.slope, K);
  const int32_t* picks_dev = (const int32_t*)(sc.rec + o_picks);
  dim3 grid((unsigned)gx, (unsigned)(n_picks < 65535 ? n_picks : 65535));
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  WalkTimer wt(sm);
  dispatch_bools(ldsx, pk.cont, K == 1, [&](auto L, auto C, auto K1) {
    hipLaunchKernelGGL((k_shap<L(), C(), K1()>), grid, dim3(PRED_BT), lds, sm, dv, pk.fidx, (int)m, (int)p, X_dev,
                       (long long)n_rows, (long long)ldx, picks_dev, (int)n_picks, out_dev);
  });
  return finish_walk(hipGetLastError(), sm, wt, &g_shap_ms, "k_shap");
}
