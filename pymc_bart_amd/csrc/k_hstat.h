// k_hstat.h -- part of pgbart_hip.hip (not a standalone header): Friedman's H-statistic of stored draws
// (include/pgbart_hstat.h holds the numeric contract AND the evaluation of a leaf and of a job at a row: the kernels
// below compile pgb_hstat_bg_job_row, pgb_hstat_slot_finish and pgb_hstat_job_row from that one text), the kernels and
// the host side of pgb_hstat_*.
//
//   k_hstat_bg       one wave per workgroup, lane = row of a tile of 64, so a lane IS a lane partial.  A workgroup owns
//                    the jobs blockIdx.x, blockIdx.x + gridDim.x, ... and walks the tiles of the block in ascending
//                    order, staging each in LDS as k_predict stages it (p <= PRED_LDS_MAXP; global reads beyond): per
//                    (tile, job, leaf) the lane reads its partials of the slot, adds its row's terms and writes them
//                    back -- coalesced, and nobody else touches a job's slots, so there are no atomics and the order
//                    of the additions is the header's.  A workgroup whose jobs list no tree leaves at once.
//   k_hstat_moments  one thread per slot: the 64 partials of its eight sums added in lane order, divided by V.
//   k_hstat_rows     the same geometry over the evaluation rows, once for the column jobs (pd, the walk's sum g by
//                    pred_walk_forest itself, J into the scratch, optionally T for the caller) and once for the pair
//                    jobs (pd, J_a and J_b read back from the scratch, optionally I for the caller); the row's terms
//                    go to the lane partials of the (job, output).  The leaf records and the finished moments of a job
//                    are wave-uniform reads.  LDS: the staged tile alone, at most 126 * 65 * 8 = 65.5 KB, so two
//                    workgroups per CU at the widest staged p and six at p = 50.
#include "pgbart_hstat.h"

#define HSTAT_WGS 2048 /* workgroups of a pass at most: each restages every tile of the block */

template <bool LDSX, bool CONT>
__global__ __launch_bounds__(PRED_BT) void k_hstat_bg(pgb_shap_view V, pgb_hstat_plan_view P, long long n_jobs, int p,
                                                      const double* __restrict__ X, long long nb, long long ldx,
                                                      const double* __restrict__ vw, double* __restrict__ mpart,
                                                      double* __restrict__ vpart) {
  extern __shared__ double hsb_s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  bool any = blockIdx.x == 0;  // (workgroup 0 also owns V)
  for (long long e = blockIdx.x; e < n_jobs && !any; e += gridDim.x) any = P.tree_off[e + 1] > P.tree_off[e];
  if (!any) return;  // (block-uniform)
  for (long long row0 = 0; row0 < nb; row0 += PRED_BT) {
    const long long row = row0 + lane;
    const bool active = row < nb;
    if constexpr (LDSX) pred_stage_rows(hsb_s_x, X, row0, nb, ldx, p, lane);
    if (active) {
      const double* x = LDSX ? hsb_s_x + lane : X + row * ldx;
      const int64_t xs = LDSX ? 65 : 1;
      const double v = vw[row];
      if (blockIdx.x == 0) vpart[lane] = vpart[lane] + v;
      for (long long e = blockIdx.x; e < n_jobs; e += gridDim.x) {
        const int t0 = P.tree_off[e], n_trees = P.tree_off[e + 1] - t0;
        if (n_trees == 0) continue;
        pgb_hstat_bg_job_row(&V, P.tree + t0, n_trees, P.a[e], P.b[e], x, xs, CONT, v,
                             mpart + (size_t)P.slot_off[e] * (PGB_HSTAT_SLOT_SUMS * PGB_HSTAT_LANES) + lane);
      }
    }
    if constexpr (LDSX) __syncthreads();  // (the tile is restaged)
  }
}

__global__ __launch_bounds__(256) void k_hstat_moments(long long n_slots, const double* __restrict__ mpart,
                                                       const double* __restrict__ vpart, double* __restrict__ V_out,
                                                       double* __restrict__ B) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  const double V = pgb_rowsum_lanes(vpart);
  if (s == 0) *V_out = V;
  if (s >= n_slots) return;
  pgb_hstat_slot_finish(mpart + (size_t)s * (PGB_HSTAT_SLOT_SUMS * PGB_HSTAT_LANES), V, B + (size_t)s * PGB_HSTAT_SLOT_SUMS);
}

template <bool LDSX, bool CONT, bool PAIRS>
__global__ __launch_bounds__(PRED_BT) void k_hstat_rows(PredTrees T, pgb_shap_view V, pgb_hstat_plan_view P, int n_picks, int q,
                                                        int n_pairs, const int32_t* __restrict__ pairs, int p,
                                                        const double* __restrict__ X, long long nb, long long ldx,
                                                        const double* __restrict__ w, double* __restrict__ rpart,
                                                        double* __restrict__ wpart, const double* __restrict__ B,
                                                        double* __restrict__ jscr, double* __restrict__ t_rows,
                                                        double* __restrict__ i_rows) {
  extern __shared__ double hsr_s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const int K = V.K;
  const int per = q + n_pairs, width = PAIRS ? n_pairs : q;
  const long long n_mine = (long long)n_picks * width;
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  double pd[4 * PGB_MAX_OUTPUTS], g[PGB_MAX_OUTPUTS];
  for (long long row0 = 0; row0 < nb; row0 += PRED_BT) {
    const long long row = row0 + lane;
    const bool active = row < nb;
    const int src = active ? lane : 0;  // (a lane beyond the block repeats the tile's first row and stores nothing)
    if constexpr (LDSX) pred_stage_rows(hsr_s_x, X, row0, nb, ldx, p, lane);
    const double* x = LDSX ? hsr_s_x + src : X + (row0 + src) * ldx;
    const int64_t xs = LDSX ? 65 : 1;
    const PredRowX<LDSX> xval{hsr_s_x, X + (row0 + src) * ldx, src};
    bool clean = false;
    if constexpr (!PAIRS) clean = pred_wave_clean<CONT>(p, xval);
    const double wi = active ? w[row] : 0.0;
    if (!PAIRS && blockIdx.x == 0 && active) wpart[lane] = wpart[lane] + wi;
    for (long long it = blockIdx.x; it < n_mine; it += gridDim.x) {
      const int d = (int)(it / width), s = (int)(it % width);
      const long long e = (long long)d * per + (PAIRS ? q + s : s);
      const int t0 = P.tree_off[e], n_trees = P.tree_off[e + 1] - t0;
      pgb_hstat_job_row(&V, P.tree + t0, n_trees, B + (size_t)P.slot_off[e] * PGB_HSTAT_SLOT_SUMS, P.a[e], P.b[e], x, xs, CONT, pd);
      if constexpr (!PAIRS) pred_walk_forest<CONT>(T, P.tree + t0, n_trees, K, clean, xval, stk_node, stk_w, g);
      if (!active) continue;
      double* __restrict__ rp = rpart + (size_t)e * K * (PGB_HSTAT_ROW_SUMS * PGB_HSTAT_LANES) + lane;
      for (int k = 0; k < K; ++k) {
        double u1, u2;
        if constexpr (!PAIRS) {
          const size_t at = (((size_t)d * q + s) * K + k) * (size_t)nb + row;
          u1 = pgb_hstat_J(pd, K, k);
          u2 = pgb_hstat_T(pd, K, k, g[k]);
          jscr[at] = u1;
          if (t_rows) t_rows[at] = u2;
        } else {
          const int sa = pairs[2 * s], sb = pairs[2 * s + 1];
          u1 = pgb_hstat_I(pd, K, k);
          u2 = pgb_hstat_U(jscr[(((size_t)d * q + sa) * K + k) * (size_t)nb + row], jscr[(((size_t)d * q + sb) * K + k) * (size_t)nb + row], u1);
          if (i_rows) i_rows[(((size_t)d * n_pairs + s) * K + k) * (size_t)nb + row] = u1;
        }
        pgb_hstat_row_add(rp + (size_t)k * (PGB_HSTAT_ROW_SUMS * PGB_HSTAT_LANES), wi, u1, u2);
      }
    }
    if constexpr (LDSX) __syncthreads();  // (the tile is restaged)
  }
}

// the jobs of one call: validated, packed and -- for the two calls that launch -- uploaded; released on every way out
struct HstatCall {
  pgb_shap_pack spack;
  pgb_hstat_plan plan;
  uint8_t* rec = nullptr;  // device: [the leaf records | the plan | the pairs]
  PredPack pk;
  pgb_shap_view dv;
  pgb_hstat_plan_view dp;
  const int32_t* pairs_dev = nullptr;
  int K = 0;
  long long gx = 0;
  HstatCall() {
    memset(&spack, 0, sizeof spack);
    memset(&plan, 0, sizeof plan);
  }
  ~HstatCall() {
    if (rec) (void)hipFree(rec);
    pgb_shap_pack_free(&spack);
    pgb_hstat_plan_free(&plan);
  }
  pgb_hstat_layout layout() const { return pgb_hstat_ws_layout(plan.n_jobs, K, plan.n_slots); }

  // the checks every call shares, then the packs (host); pc carries the entry point's name
  int prepare(PredCall& pc, const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
              int32_t p, const int32_t* cols_host, int32_t q, const int32_t* pairs_host, int32_t n_pairs,
              const int32_t* picks_host, int32_t n_picks, int32_t* n_common, int64_t nb = 0) {
    pc.null(trees, "trees");
    pc.null(forest_tree_idx, "forest_tree_idx");
    pc.null(cols_host, "cols_host");
    pc.null(picks_host, "picks_host");
    pc.forest_dims(n_forests, m, p);
    pc.at_least_one(q, "q");
    pc.at_least_one(n_picks, "n_picks");
    if (n_pairs < 0) pc.refuse(PGB_E_INVALID, "n_pairs must be >= 0");
    if (n_pairs > PGB_HSTAT_MAX_PAIRS)
      pc.refuse(PGB_E_INVALID, "n_pairs = %d: at most PGB_HSTAT_MAX_PAIRS = %d pairs per call", (int)n_pairs, PGB_HSTAT_MAX_PAIRS);
    if (n_pairs > 0) pc.null(pairs_host, "pairs_host");
    if (pc.rc() != PGB_OK) return pc.rc();
    pc.index_vector(cols_host, (size_t)q, p, "cols_host", "p");
    pc.distinct(cols_host, q);
    pc.index_vector(picks_host, (size_t)n_picks, n_forests, "picks_host", "n_forests");
    if (pc.rc() != PGB_OK) return pc.rc();
    std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t>> by((size_t)n_pairs);
    for (int j = 0; j < n_pairs; ++j) {
      const int32_t a = pairs_host[2 * j], b = pairs_host[2 * j + 1];
      if (a < 0 || a >= q || b < 0 || b >= q)
        return pc.refuse(PGB_E_INVALID, "pairs_host[%d] = (%d, %d) names a slot outside [0, q = %d)", j, (int)a, (int)b, (int)q);
      if (a == b) return pc.refuse(PGB_E_INVALID, "pairs_host[%d] names slot %d twice", j, (int)a);
      by[j] = {{a < b ? a : b, a < b ? b : a}, j};
    }
    std::sort(by.begin(), by.end());
    for (int j = 1; j < n_pairs; ++j)
      if (by[j].first == by[j - 1].first)
        return pc.refuse(PGB_E_INVALID, "pairs_host[%d] repeats pairs_host[%d]", (int)by[j].second, (int)by[j - 1].second);
    pc.n_outputs(trees);
    if (pc.rc() != PGB_OK) return pc.rc();
    const int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
    if (rc != PGB_OK) return rc;
    K = trees->n_outputs;
    pc.cells_fit({n_picks, (int64_t)q + n_pairs, K, PGB_HSTAT_ROW_SUMS * PGB_HSTAT_LANES}, "n_picks x (q + n_pairs) x K x 256");
    if (nb > 0) pc.cells_fit({n_picks, (int64_t)q + n_pairs, K, nb}, "n_picks x (q + n_pairs) x K x nb");  // (the per-row outputs)
    if (pc.rc() != PGB_OK) return pc.rc();
    int prc = pgb_shap_pack_build(trees, p, &spack);
    if (prc == -1) return pc.refuse(PGB_E_NOMEM, "the leaf records do not fit host memory");
    if (prc != 0) return pc.refuse(PGB_E_INVALID, "the history's leaf paths number more than 2^31 - 1 splits");
    prc = pgb_hstat_plan_build(trees, forest_tree_idx, m, p, cols_host, q, pairs_host, n_pairs, picks_host, n_picks,
                               (const int32_t*)(spack.buf + spack.o_off), n_common, &plan);
    if (prc == -1) return pc.refuse(PGB_E_NOMEM, "the jobs do not fit host memory");
    if (prc != 0) return pc.refuse(PGB_E_INVALID, "the jobs list more than 2^31 - 1 trees or 2^28 - 1 leaves: ask for fewer pairs or picks");
    return PGB_OK;
  }

  // the checks of a block of rows; before prepare
  void block(PredCall& pc, const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const double* w_dev, const char* w_name,
             int64_t first_row, const void* ws_dev) {
    pc.null(X_dev, "X_dev");
    pc.null(w_dev, w_name);
    pc.null(ws_dev, "ws_dev");
    pc.at_least_one(nb, "nb");
    pc.ld(ldx, p, "ldx");
    pc.tiles(nb, &gx);
    if (first_row < 0 || first_row % PGB_HSTAT_LANES != 0)
      pc.refuse(PGB_E_INVALID, "first_row = %lld must be a multiple of 64 and >= 0", (long long)first_row);
  }

  int upload(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m, int32_t p,
             const int32_t* pairs_host, int32_t n_pairs, hipStream_t sm) {
    const int rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);
    if (rc != PGB_OK) return rc;
    const size_t o_plan = (spack.bytes + 7) & ~(size_t)7;
    const size_t o_pairs = o_plan + (size_t)pgb_hstat_plan_words(&plan) * sizeof(int32_t);
    std::vector<uint8_t> hb(o_pairs + (size_t)(n_pairs > 0 ? 2 * n_pairs : 1) * sizeof(int32_t));
    memcpy(hb.data(), spack.buf, spack.bytes);
    memcpy(hb.data() + o_plan, plan.buf, (size_t)pgb_hstat_plan_words(&plan) * sizeof(int32_t));
    if (n_pairs > 0) memcpy(hb.data() + o_pairs, pairs_host, (size_t)2 * n_pairs * sizeof(int32_t));
    HIPCHK(hipMalloc((void**)&rec, hb.size()));
    HIPCHK(hipMemcpy(rec, hb.data(), hb.size(), hipMemcpyHostToDevice));
    dv = pgb_shap_pack_view(&spack, rec, pk.T.value, pk.T.slope, K);
    dp = pgb_hstat_plan_at(&plan, (const int32_t*)(rec + o_plan));
    pairs_dev = (const int32_t*)(rec + o_pairs);
    return PGB_OK;
  }
};

static thread_local double g_hstat_ms[2] = {-1.0, -1.0};
extern "C" int pgb_hstat_kernel_ms(double* ms_out) {
  if (!ms_out) return fail(PGB_E_INVALID, "null argument");
  ms_out[0] = g_hstat_ms[0];
  ms_out[1] = g_hstat_ms[1];
  return PGB_OK;
}

extern "C" int pgb_hstat_workspace_bytes(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests,
                                         int32_t m, int32_t p, const int32_t* cols_host, int32_t q, const int32_t* pairs_host,
                                         int32_t n_pairs, const int32_t* picks_host, int32_t n_picks, int64_t* bytes_out,
                                         int32_t* n_common_out) {
  PredCall pc("pgb_hstat_workspace_bytes");
  pc.null(bytes_out, "bytes_out");
  HstatCall hc;
  // (n_common_out is written by the packer's second pass only: a refused call writes nothing)
  const int rc = hc.prepare(pc, trees, forest_tree_idx, n_forests, m, p, cols_host, q, pairs_host, n_pairs, picks_host, n_picks,
                            n_common_out);
  if (rc != PGB_OK) return rc;
  *bytes_out = 8 * hc.layout().words;
  return PGB_OK;
}

extern "C" int pgb_hstat_background(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                                    const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const double* v_dev,
                                    int64_t first_row, int32_t init, const int32_t* cols_host, int32_t q,
                                    const int32_t* pairs_host, int32_t n_pairs, const int32_t* picks_host, int32_t n_picks,
                                    void* ws_dev, void* stream) {
  PredCall pc("pgb_hstat_background");
  HstatCall hc;
  hc.block(pc, X_dev, nb, p, ldx, v_dev, "v_dev", first_row, ws_dev);
  int rc = hc.prepare(pc, trees, forest_tree_idx, n_forests, m, p, cols_host, q, pairs_host, n_pairs, picks_host, n_picks, nullptr);
  if (rc != PGB_OK) return rc;
  hipStream_t sm = (hipStream_t)stream;
  rc = hc.upload(trees, forest_tree_idx, n_forests, m, p, pairs_host, n_pairs, sm);
  if (rc != PGB_OK) return rc;
  const pgb_hstat_layout L = hc.layout();
  double* ws = (double*)ws_dev;
  if (init) {
    const hipError_t e = hipMemsetAsync(ws + L.o_vpart, 0, (size_t)8 * (size_t)(L.o_B - L.o_vpart), sm);  // (all bits 0: 0.0)
    if (e != hipSuccess) return fail_hip(e, "pgb_hstat_background: clearing the moments");
  }
  const long long n_jobs = hc.plan.n_jobs;
  const long long gx = n_jobs < HSTAT_WGS ? n_jobs : HSTAT_WGS;
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  WalkTimer wt(sm);
  dispatch_bools(ldsx, hc.pk.cont, [&](auto Lx, auto C) {
    hipLaunchKernelGGL((k_hstat_bg<Lx(), C()>), dim3((unsigned)gx), dim3(PRED_BT), lds, sm, hc.dv, hc.dp, n_jobs, (int)p, X_dev,
                       (long long)nb, (long long)ldx, v_dev, ws + L.o_mpart, ws + L.o_vpart);
  });
  return finish_walk(hipGetLastError(), sm, wt, &g_hstat_ms[0], "k_hstat_bg");
}

extern "C" int pgb_hstat_rows(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                              const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const double* w_dev, int64_t first_row,
                              int32_t init, const int32_t* cols_host, int32_t q, const int32_t* pairs_host, int32_t n_pairs,
                              const int32_t* picks_host, int32_t n_picks, void* ws_dev, double* jscr_dev, double* t_rows_dev,
                              double* i_rows_dev, void* stream) {
  PredCall pc("pgb_hstat_rows");
  HstatCall hc;
  hc.block(pc, X_dev, nb, p, ldx, w_dev, "w_dev", first_row, ws_dev);
  pc.null(jscr_dev, "jscr_dev");
  int rc = hc.prepare(pc, trees, forest_tree_idx, n_forests, m, p, cols_host, q, pairs_host, n_pairs, picks_host, n_picks, nullptr, nb);
  if (rc != PGB_OK) return rc;
  hipStream_t sm = (hipStream_t)stream;
  rc = hc.upload(trees, forest_tree_idx, n_forests, m, p, pairs_host, n_pairs, sm);
  if (rc != PGB_OK) return rc;
  const pgb_hstat_layout L = hc.layout();
  double* ws = (double*)ws_dev;
  if (init) {
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)8 * (size_t)L.o_vpart, sm);  // (all bits 0: 0.0)
    if (e != hipSuccess) return fail_hip(e, "pgb_hstat_rows: clearing the row partials");
    const long long n_slots = hc.plan.n_slots;
    const long long bx = n_slots > 0 ? (n_slots + 255) / 256 : 1;
    hipLaunchKernelGGL(k_hstat_moments, dim3((unsigned)bx), dim3(256), 0, sm, n_slots, (const double*)(ws + L.o_mpart),
                       (const double*)(ws + L.o_vpart), ws + L.o_V, ws + L.o_B);
    e = hipGetLastError();
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(sm);
      return fail_hip(e, "k_hstat_moments launch");
    }
  }
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  WalkTimer wt(sm);
  hipError_t e = hipSuccess;
  for (int pass = 0; pass < (n_pairs > 0 ? 2 : 1) && e == hipSuccess; ++pass) {
    const long long n_mine = (long long)n_picks * (pass ? n_pairs : q);
    const long long gx = n_mine < HSTAT_WGS ? n_mine : HSTAT_WGS;
    dispatch_bools(ldsx, hc.pk.cont, pass != 0, [&](auto Lx, auto C, auto Pr) {
      hipLaunchKernelGGL((k_hstat_rows<Lx(), C(), Pr()>), dim3((unsigned)gx), dim3(PRED_BT), lds, sm, hc.pk.T, hc.dv, hc.dp,
                         (int)n_picks, (int)q, (int)n_pairs, hc.pairs_dev, (int)p, X_dev, (long long)nb, (long long)ldx, w_dev,
                         ws + L.o_rpart, ws + L.o_wpart, (const double*)(ws + L.o_B), jscr_dev, t_rows_dev, i_rows_dev);
    });
    e = hipGetLastError();
  }
  return finish_walk(e, sm, wt, &g_hstat_ms[1], "k_hstat_rows");
}

extern "C" int pgb_hstat_finish(const void* ws_dev, int32_t n_picks, int32_t q, int32_t n_pairs, int32_t K,
                                const double* var_fit_host, double* main_var_out, double* total_var_out, double* h2_total_out,
                                double* inter_var_out, double* h2_out, int64_t* n_nonfinite_out, void* stream) {
  PredCall pc("pgb_hstat_finish");
  pc.null(ws_dev, "ws_dev");
  pc.null(var_fit_host, "var_fit_host");
  pc.null(main_var_out, "main_var_out");
  pc.null(total_var_out, "total_var_out");
  pc.null(h2_total_out, "h2_total_out");
  pc.null(n_nonfinite_out, "n_nonfinite_out");
  pc.at_least_one(n_picks, "n_picks");
  pc.at_least_one(q, "q");
  if (n_pairs < 0) pc.refuse(PGB_E_INVALID, "n_pairs must be >= 0");
  if (n_pairs > 0) {
    pc.null(inter_var_out, "inter_var_out");
    pc.null(h2_out, "h2_out");
  }
  if (K < 1 || K > PGB_MAX_OUTPUTS) pc.refuse(PGB_E_INVALID, "K must lie in [1, %d]", PGB_MAX_OUTPUTS);
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.cells_fit({n_picks, (int64_t)q + n_pairs, K, PGB_HSTAT_ROW_SUMS * PGB_HSTAT_LANES}, "n_picks x (q + n_pairs) x K x 256");
  if (pc.rc() != PGB_OK) return pc.rc();
  const pgb_hstat_layout L = pgb_hstat_ws_layout((int64_t)n_picks * ((int64_t)q + n_pairs), K, 0);
  std::vector<double> rw((size_t)L.o_vpart);
  hipStream_t sm = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(rw.data(), ws_dev, rw.size() * sizeof(double), hipMemcpyDeviceToHost, sm));
  HIPCHK(hipStreamSynchronize(sm));
  pgb_hstat_finish_host(rw.data(), n_picks, q, n_pairs, K, var_fit_host, main_var_out, total_var_out, h2_total_out, inter_var_out,
                        h2_out, n_nonfinite_out);
  return PGB_OK;
}
