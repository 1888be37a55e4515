// k_ale.h -- part of pgbart_hip.hip (not a standalone header): the local differences of the accumulated local effects
// of stored draws (include/pgbart_ale.h holds the numeric contract and the bin of a value), the two kernels and the host
// side of pgb_predict_ale.
//
//   k_ale_bins  one lane per (slot, row): the slot's edges in LDS (at most 1025 doubles), the row's value of the slot's
//               column once, pgb_ale_bin's binary search; writes bins_out, the group vector of the row reduce.
//   k_ale       launched as k_permimp is: one wave per workgroup, lane = row, the tile staged in LDS as k_predict stages
//               it when p <= PRED_LDS_MAXP.  The (slot, pick) pairs are ordered SLOT-MAJOR and blockIdx.y takes a
//               contiguous share of them, so a workgroup's consecutive pairs share the slot: the row's bin and its two
//               edges are read once per slot, not once per pick.  Per pair two walks of the pair's use list --
//               pred_walk_forest itself, with k_permimp's PermRowX returning an edge for the slot's column -- and K
//               coalesced stores of their difference.  All lanes of a live tile walk (the walk's `clean` is decided per
//               wave); a lane in the missing bin walks with the edges of bin 0 and stores +0.0.  No LDS beyond the
//               tile, no scratch beyond the walk's two stacks, no atomics: nobody else writes a lane's outputs.
#include "pgbart_ale.h"

#define ALE_BINS_BT 256

__global__ __launch_bounds__(ALE_BINS_BT) void k_ale_bins(const double* __restrict__ X, long long nb, long long ldx,
                                                          const int32_t* __restrict__ cols, int q,
                                                          const double* __restrict__ edges,
                                                          const int32_t* __restrict__ edge_off,
                                                          int32_t* __restrict__ bins) {
  __shared__ double s_e[PGB_ALE_MAX_BINS + 1];
  const long long row = (long long)blockIdx.x * ALE_BINS_BT + threadIdx.x;
  for (int slot = blockIdx.y; slot < q; slot += gridDim.y) {  // (block-uniform: every thread meets both barriers)
    const int e0 = edge_off[slot];
    const int n_e = edge_off[slot + 1] - e0;  // (validated: 2 .. PGB_ALE_MAX_BINS + 1)
    for (int j = threadIdx.x; j < n_e; j += ALE_BINS_BT) s_e[j] = edges[e0 + j];
    __syncthreads();
    if (row < nb) bins[(size_t)slot * (size_t)nb + row] = pgb_ale_bin(s_e, n_e - 1, X[row * ldx + cols[slot]]);
    __syncthreads();
  }
}

template <bool LDSX, bool CONT>
__global__ __launch_bounds__(PRED_BT) void k_ale(PredTrees T, int K, int p, const double* __restrict__ X, long long nb,
                                                 long long ldx, const int32_t* __restrict__ cols, int q,
                                                 const double* __restrict__ edges, const int32_t* __restrict__ edge_off,
                                                 const int32_t* __restrict__ use_off, const int32_t* __restrict__ use_list,
                                                 int n_picks, const int32_t* __restrict__ bins, double* __restrict__ out) {
  extern __shared__ double ale_s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
  if constexpr (LDSX) pred_stage_rows(ale_s_x, X, row0, nb, ldx, p, lane);
  if (row >= nb) return;
  const PredRowX<LDSX> xval{ale_s_x, X + row * ldx, lane};
  // an edge is finite: a tile without a NaN stays clean with a column replaced (a NaN of the swept column alone
  // keeps the general walk, which adds the same bits)
  const bool clean = pred_wave_clean<CONT>(p, xval);
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  const long long n_pairs = (long long)q * n_picks;
  const long long share = (n_pairs + gridDim.y - 1) / gridDim.y;
  const long long first = (long long)blockIdx.y * share;
  const long long last = first + share < n_pairs ? first + share : n_pairs;
  int have = -1, c = 0;
  bool missing = false;
  double e_lo = 0.0, e_hi = 0.0;
  for (long long pair = first; pair < last; ++pair) {
    const int slot = (int)(pair / n_picks), pick = (int)(pair % n_picks);
    if (slot != have) {  // (wave-uniform)
      have = slot;
      c = cols[slot];
      const int e0 = edge_off[slot];
      const int B = edge_off[slot + 1] - e0 - 1;
      const int b = bins[(size_t)slot * (size_t)nb + row];
      missing = b >= B;
      const double* __restrict__ e = edges + e0 + (missing ? 0 : b);
      e_lo = e[0];
      e_hi = e[1];
    }
    const long long li = (long long)pick * q + slot;  // (the packer's lists are pick-major)
    const int32_t* __restrict__ list = use_list + use_off[li];
    const int len = use_off[li + 1] - use_off[li];
    double a_hi[PGB_MAX_OUTPUTS], a_lo[PGB_MAX_OUTPUTS];
    const PermRowX<PredRowX<LDSX>> hi_val{xval, c, e_hi};
    pred_walk_forest<CONT>(T, list, len, K, clean, hi_val, stk_node, stk_w, a_hi);
    const PermRowX<PredRowX<LDSX>> lo_val{xval, c, e_lo};
    pred_walk_forest<CONT>(T, list, len, K, clean, lo_val, stk_node, stk_w, a_lo);
    double* __restrict__ o_p = out + ((size_t)pair * K) * (size_t)nb + row;
    for (int o = 0; o < K; ++o) {
      const double delta = a_hi[o] - a_lo[o];
      o_p[(size_t)o * nb] = missing ? 0.0 : delta;
    }
  }
}

// every buffer of one call, released on every way out
struct AleScratch {
  uint8_t* rec = nullptr;  // device: [the edges | the header's pack | the columns | the edge offsets]
  pgb_permimp_pack pack;
  AleScratch() { memset(&pack, 0, sizeof pack); }
  ~AleScratch() {
    if (rec) (void)hipFree(rec);
    pgb_permimp_pack_free(&pack);
  }
};

static thread_local double g_ale_ms = -1.0;
extern "C" int pgb_ale_kernel_ms(double* ms_out) {
  if (!ms_out) return fail(PGB_E_INVALID, "null argument");
  *ms_out = g_ale_ms;
  return PGB_OK;
}

extern "C" int pgb_predict_ale(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                               const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const int32_t* cols_host, int32_t q,
                               const double* edges_host, const int32_t* edge_off_host, const int32_t* picks_host,
                               int32_t n_picks, double* out_dev, int32_t* bins_out_dev, void* stream) {
  PredCall pc("pgb_predict_ale");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(cols_host, "cols_host");
  pc.null(edges_host, "edges_host");
  pc.null(edge_off_host, "edge_off_host");
  pc.null(picks_host, "picks_host");
  pc.null(out_dev, "out_dev");
  pc.null(bins_out_dev, "bins_out_dev");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(nb, "nb");
  pc.at_least_one(q, "q");
  pc.at_least_one(n_picks, "n_picks");
  pc.ld(ldx, p, "ldx");
  long long gx = 0;
  pc.tiles(nb, &gx);
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.index_vector(cols_host, (size_t)q, p, "cols_host", "p");
  pc.distinct(cols_host, q);
  pc.index_vector(picks_host, (size_t)n_picks, n_forests, "picks_host", "n_forests");
  if (pc.rc() != PGB_OK) return pc.rc();
  if (edge_off_host[0] != 0) return pc.refuse(PGB_E_INVALID, "edge_off_host[0] = %d must be 0", (int)edge_off_host[0]);
  for (int s = 0; s < q; ++s) {
    const long long n_e = (long long)edge_off_host[s + 1] - edge_off_host[s];
    if (n_e < 2)
      return pc.refuse(PGB_E_INVALID, "edge_off_host[%d] = %d must be >= edge_off_host[%d] + 2: a column has at least one bin",
                       s + 1, (int)edge_off_host[s + 1], s);
    if (n_e > PGB_ALE_MAX_BINS + 1)
      return pc.refuse(PGB_E_INVALID, "slot %d of edges_host holds %lld edges: at most PGB_ALE_MAX_BINS + 1 = %d", s, n_e,
                       PGB_ALE_MAX_BINS + 1);
  }
  const int32_t n_edges = edge_off_host[q];
  for (int s = 0; s < q; ++s)
    for (int j = edge_off_host[s]; j < edge_off_host[s + 1]; ++j) {
      if (!std::isfinite(edges_host[j])) return pc.refuse(PGB_E_INVALID, "edges_host[%d] (slot %d) is not finite", j, s);
      if (j > edge_off_host[s] && !(edges_host[j] > edges_host[j - 1]))
        return pc.refuse(PGB_E_INVALID, "edges_host[%d] (slot %d) is not above its predecessor", j, s);
    }
  pc.n_outputs(trees);
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;
  const int K = trees->n_outputs;
  pc.cells_fit({q, n_picks, K, nb}, "q x n_picks x K x nb");
  if (pc.rc() != PGB_OK) return pc.rc();

  AleScratch sc;
  const int prc = pgb_permimp_pack_build(trees, forest_tree_idx, m, p, cols_host, q, picks_host, n_picks, &sc.pack);  // once per call
  if (prc == -1) return pc.refuse(PGB_E_NOMEM, "the use lists do not fit host memory");
  if (prc != 0) return pc.refuse(PGB_E_INVALID, "the use lists hold more than 2^31 - 1 trees");
  hipStream_t sm = (hipStream_t)stream;
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);
  if (rc != PGB_OK) return rc;
  const size_t n_pack = (size_t)(sc.pack.n_lists + 1 + sc.pack.n_list);
  const size_t o_pack = (size_t)n_edges * sizeof(double);
  const size_t o_cols = o_pack + n_pack * sizeof(int32_t);
  const size_t o_eoff = o_cols + (size_t)q * sizeof(int32_t);
  std::vector<uint8_t> hb(o_eoff + ((size_t)q + 1) * sizeof(int32_t));
  memcpy(hb.data(), edges_host, o_pack);
  memcpy(hb.data() + o_pack, sc.pack.buf, n_pack * sizeof(int32_t));
  memcpy(hb.data() + o_cols, cols_host, (size_t)q * sizeof(int32_t));
  memcpy(hb.data() + o_eoff, edge_off_host, ((size_t)q + 1) * sizeof(int32_t));
  HIPCHK(hipMalloc((void**)&sc.rec, hb.size()));
  HIPCHK(hipMemcpyAsync(sc.rec, hb.data(), hb.size(), hipMemcpyHostToDevice, sm));
  const double* edges_dev = (const double*)sc.rec;
  const int32_t* off_dev = (const int32_t*)(sc.rec + o_pack);
  const int32_t* list_dev = off_dev + sc.pack.n_lists + 1;
  const int32_t* cols_dev = (const int32_t*)(sc.rec + o_cols);
  const int32_t* eoff_dev = (const int32_t*)(sc.rec + o_eoff);
  {
    const long long bx = (nb + ALE_BINS_BT - 1) / ALE_BINS_BT;
    hipLaunchKernelGGL(k_ale_bins, dim3((unsigned)bx, (unsigned)(q < 65535 ? q : 65535)), dim3(ALE_BINS_BT), 0, sm, X_dev,
                       (long long)nb, (long long)ldx, cols_dev, (int)q, edges_dev, eoff_dev, bins_out_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(sm);
      return fail_hip(e, "k_ale_bins launch");
    }
  }
  // one wave per workgroup; enough workgroups to fill the chip (pgb_predict's figure), each taking a contiguous share
  // of the slot-major (slot, pick) pairs
  const long long n_pairs = (long long)n_picks * q;
  const long long want_wgs = p <= PRED_LDS_MAXP ? 16384 : 4096;
  long long gy = (want_wgs + gx - 1) / gx;
  if (gy > n_pairs) gy = n_pairs;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  dim3 grid((unsigned)gx, (unsigned)gy);
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  WalkTimer wt(sm);
  dispatch_bools(ldsx, pk.cont, [&](auto L, auto C) {
    hipLaunchKernelGGL((k_ale<L(), C()>), grid, dim3(PRED_BT), lds, sm, pk.T, K, (int)p, X_dev, (long long)nb, (long long)ldx,
                       cols_dev, (int)q, edges_dev, eoff_dev, off_dev, list_dev, (int)n_picks, (const int32_t*)bins_out_dev,
                       out_dev);
  });
  return finish_walk(hipGetLastError(), sm, wt, &g_ale_ms, "k_ale");
}
