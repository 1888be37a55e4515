// k_pdp.h -- part of pgbart_hip.hip (not a standalone header): partial dependence sweeps (include/pgbart_pdp.h holds
// the numeric contract), the two kernels and the host side of pgb_predict_pdp.
//
// "Every column but j excluded" is the walk in which every other column reads NaN: pred_walk_forest
// (pgb_pred_walk.h) takes `(nd.flags & 1) || xv != xv` into the same branch and gives a leaf whose regressor is
// excluded or missing js = -1.  So the trees are packed ONCE, without exclusions, and xval(v) = v == j ? xs : NaN.
//
//   k_pdp_walk    one wave per workgroup, lane = one value xs of column j, driven by a descriptor per (column, pick):
//                 DIRECT   the lanes are the rows of X, xs = X[i][j], the K sums go to out[c][s][k][i];
//                 PROFILE  the lanes are the B + 2 slots of the (column, forest) profile -- slot k < B is evaluated at
//                          breakpoint b_k and stands for (b_{k-1}, b_k], slot B at +inf for "above all", slot B + 1 at
//                          NaN -- and the K sums go to the table [slot][K].  The breakpoints are the split values the
//                          forest holds on j (sorted, de-duplicated by ==): two values of x that take the same side
//                          of every one of them run the same instructions on the same operands.
//   k_pdp_lookup  one lane per row: x = X[i][j] once, then per pick the first breakpoint >= x (NaN: the NaN slot, none:
//                 the "above" slot) and K table values stored coalesced over i.  Breakpoints and table of a (column,
//                 pick) sit in LDS when B <= PGB_PDP_LDS_MAXB.
#include <algorithm>

#include "pgbart_pdp.h"

struct PdpJob {
  long long src;   // PROFILE: the first of the job's B breakpoints in bp[]
  long long dst;   // the first output: in out[] (DIRECT, [K][n_rows]) or in tab[] (PROFILE, [slot][K])
  int32_t col;     // the swept column j
  int32_t forest;  // row of forest_idx
  int32_t n;       // PROFILE: B + 2 slots; DIRECT: -1 (the lanes are the n_rows rows of X)
  int32_t walk;    // 1: k_pdp_walk fills dst; 0: a repeated (column, forest) -- src / dst / n are the first one's
};

// Grid = (tiles of 64 lanes, picks, columns); y and z stride when a sweep exceeds the grid limits.  `profile`: which of
// the two kinds of descriptor this launch serves (the other kind is skipped: wave-uniform).
template <bool CONT, bool K1>
__global__ __launch_bounds__(PRED_BT) void k_pdp_walk(PredTrees T, const int32_t* __restrict__ forest_idx, int m, int K_rt,
                                                      const PdpJob* __restrict__ jobs, int n_picks, int n_cols, int profile,
                                                      const double* __restrict__ X, long long n_rows, long long ldx,
                                                      const double* __restrict__ bp, double* __restrict__ out) {
  const int K = K1 ? 1 : K_rt;
  const long long idx = (long long)blockIdx.x * PRED_BT + threadIdx.x;
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  for (int c = blockIdx.z; c < n_cols; c += gridDim.z) {
    for (int s = blockIdx.y; s < n_picks; s += gridDim.y) {
      const PdpJob jb = jobs[(size_t)c * n_picks + s];
      if (!jb.walk || (jb.n >= 0) != (profile != 0)) continue;
      const long long cnt = profile ? (long long)jb.n : n_rows;
      if (idx >= cnt) continue;
      const int j = jb.col;
      double xs;
      if (profile) {
        const long long B = (long long)jb.n - 2;
        xs = idx < B ? bp[jb.src + idx] : (idx == B ? __builtin_inf() : __builtin_nan(""));
      } else {
        xs = X[idx * ldx + j];
      }
      auto xval = [&](int v) -> double { return v == j ? xs : __builtin_nan(""); };
      double acc[K1 ? 1 : PGB_MAX_OUTPUTS];
      pred_walk_forest<CONT>(T, forest_idx + (size_t)jb.forest * m, m, K, false, xval, stk_node, stk_w, acc);
      if (profile) {
        double* __restrict__ dst = out + jb.dst + idx * K;
        for (int o = 0; o < K; ++o) dst[o] = acc[o];
      } else {
        double* __restrict__ dst = out + jb.dst + idx;
        for (int o = 0; o < K; ++o) dst[(size_t)o * n_rows] = acc[o];
      }
    }
  }
}

#define PDP_LT 256
extern __shared__ __attribute__((aligned(16))) double pdp_s[];  // [cap breakpoints | (cap + 2) K table values]

// Grid = (tiles of 256 rows, columns); y strides.  Columns of the direct route are skipped (wave-uniform).
template <bool K1>
__global__ __launch_bounds__(PDP_LT) void k_pdp_lookup(const PdpJob* __restrict__ jobs, int n_picks, int n_cols, int K_rt,
                                                       int cap, const double* __restrict__ X, long long n_rows,
                                                       long long ldx, const double* __restrict__ bp,
                                                       const double* __restrict__ tab, double* __restrict__ out) {
  const int K = K1 ? 1 : K_rt;
  const int tid = threadIdx.x;
  const long long row = (long long)blockIdx.x * PDP_LT + tid;
  const bool live = row < n_rows;
  double* s_bp = pdp_s;
  double* s_tab = pdp_s + cap;
  for (int c = blockIdx.y; c < n_cols; c += gridDim.y) {
    const PdpJob* __restrict__ jc = jobs + (size_t)c * n_picks;
    if (jc[0].n < 0) continue;
    const double x = live ? X[row * ldx + jc[0].col] : 0.0;
    const bool missing = x != x;
    for (int s = 0; s < n_picks; ++s) {
      const int B = jc[s].n - 2;
      const double* __restrict__ gb = bp + jc[s].src;
      const double* __restrict__ gt = tab + jc[s].dst;
      double* __restrict__ dst = out + ((size_t)c * n_picks + s) * K * (size_t)n_rows + row;
      auto find = [&](const double* b, const double* t) {
        int lo = 0, hi = B;  // the first breakpoint >= x
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (b[mid] < x) lo = mid + 1;
          else hi = mid;
        }
        const int slot = missing ? B + 1 : lo;
        for (int o = 0; o < K; ++o) dst[(size_t)o * n_rows] = t[(size_t)slot * K + o];
      };
      if (B <= cap) {
        __syncthreads();  // (the previous pick's lookups have read what they staged)
        for (int i = tid; i < B; i += PDP_LT) s_bp[i] = gb[i];
        for (int i = tid; i < (B + 2) * K; i += PDP_LT) s_tab[i] = gt[i];
        __syncthreads();
        if (live) find(s_bp, s_tab);
      } else if (live) {
        find(gb, gt);
      }
    }
  }
}

static thread_local double g_pdp_walk_ms = -1.0, g_pdp_lookup_ms = -1.0;
extern "C" int pgb_pdp_kernel_ms(double* walk_ms_out, double* lookup_ms_out) {
  if (!walk_ms_out || !lookup_ms_out) return fail(PGB_E_INVALID, "null argument");
  *walk_ms_out = g_pdp_walk_ms;
  *lookup_ms_out = g_pdp_lookup_ms;
  return PGB_OK;
}

// The split values forest f holds on column j, sorted and de-duplicated by == (a NaN split value sends every x that
// is not NaN to the right, whatever its slot: it is no breakpoint).  false: the column is not eligible in this forest
// (a split on j under another rule than `x <= v`, or a leaf that regresses on j).
static bool pdp_breakpoints(const pgb_tree_arrays* trees, const int32_t* forest, int m, int j, std::vector<double>* out) {
  const bool lin = trees->slope && trees->xbar && trees->svar;
  out->clear();
  for (int k = 0; k < m; ++k) {
    const int t = forest[k];
    for (int g = trees->node_off[t]; g < trees->node_off[t + 1]; ++g) {
      if (trees->var[g] < 0) {
        if (lin && trees->svar[g] == j) return false;
      } else if (trees->var[g] == j) {
        if (trees->rule && trees->rule[g] != PGB_RULE_CONTINUOUS) return false;
        const double v = trees->split[g];
        if (v == v) out->push_back(v);
      }
    }
  }
  std::sort(out->begin(), out->end());
  out->erase(std::unique(out->begin(), out->end()), out->end());
  return true;
}

extern "C" int pgb_predict_pdp(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                               const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx, const int32_t* cols_host,
                               int32_t n_cols, const int32_t* picks_host, int32_t n_picks, int32_t route, double* out_dev,
                               int32_t* route_taken_host, void* stream) {
  PredCall pc("pgb_predict_pdp");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(cols_host, "cols_host");
  pc.null(picks_host, "picks_host");
  pc.null(out_dev, "out_dev");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(n_cols, "n_cols");
  pc.at_least_one(n_picks, "n_picks");
  pc.at_least_one(n_rows, "n_rows");
  pc.ld(ldx, p, "ldx");
  pc.require(route >= PGB_PDP_ROUTE_AUTO && route <= PGB_PDP_ROUTE_PROFILE, "route must be 0 (auto), 1 (direct) or 2 (profile)");
  long long gx = 0;
  pc.tiles(n_rows, &gx);
  const size_t n_job = (size_t)n_cols * (size_t)n_picks;
  pc.index_vector(cols_host, (size_t)n_cols, p, "cols_host", "p");
  pc.index_vector(picks_host, n_job, n_forests, "picks_host", "n_forests");
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;
  const int K = trees->n_outputs;

  // the descriptors: per column its route, per (column, pick) where its lanes come from and where its sums go
  std::vector<PdpJob> jobs(n_job);
  std::vector<double> bps;               // the breakpoints of every profile, one after the other
  std::vector<double> one;
  std::vector<int32_t> first(n_forests);  // per column: the pick that built forest f's profile (-1: none yet)
  long long n_tab = 0;                    // doubles of all tables
  int max_slots = 0, max_B = 0;
  bool any_profile = false, any_direct = false;
  for (int c = 0; c < n_cols; ++c) {
    const int j = cols_host[c];
    PdpJob* jc = jobs.data() + (size_t)c * n_picks;
    const int32_t* pk = picks_host + (size_t)c * n_picks;
    bool profile = route != PGB_PDP_ROUTE_DIRECT;
    const size_t bps0 = bps.size();
    const long long tab0 = n_tab;
    int col_slots = 0, col_B = 0;
    if (profile) {
      std::fill(first.begin(), first.end(), -1);
      long long slots = 0;  // summed over the picks, repeats included
      for (int s = 0; s < n_picks && profile; ++s) {
        const int f = pk[s];
        if (first[f] >= 0) {
          jc[s] = jc[first[f]];
          jc[s].walk = 0;
        } else {
          if (!pdp_breakpoints(trees, forest_tree_idx + (size_t)f * m, m, j, &one)) {
            profile = false;
            break;
          }
          first[f] = s;
          const int B = (int)one.size();
          jc[s] = PdpJob{(long long)bps.size(), n_tab, j, f, B + 2, 1};
          bps.insert(bps.end(), one.begin(), one.end());
          n_tab += (long long)(B + 2) * K;
          if (B > col_B) col_B = B;
        }
        slots += jc[s].n;
        if (jc[s].n > col_slots) col_slots = jc[s].n;
      }
      // auto: the profile route when it does strictly fewer general walks than one per (row, pick)
      if (profile && route == PGB_PDP_ROUTE_AUTO && slots >= (long long)n_rows * n_picks) profile = false;
      if (!profile) {
        bps.resize(bps0);
        n_tab = tab0;
      }
    }
    if (profile) {
      any_profile = true;
      if (col_slots > max_slots) max_slots = col_slots;
      if (col_B > max_B) max_B = col_B;
    } else {
      any_direct = true;
      for (int s = 0; s < n_picks; ++s)
        jc[s] = PdpJob{0, (long long)(((size_t)c * n_picks + s) * K * (size_t)n_rows), j, pk[s], -1, 1};
    }
    if (route_taken_host) route_taken_host[c] = profile ? PGB_PDP_ROUTE_PROFILE : PGB_PDP_ROUTE_DIRECT;
  }

  hipStream_t sm = (hipStream_t)stream;
  DevBuf job;  // [PdpJob n_cols n_picks | the breakpoints of every profile]
  DevBuf tab;  // the tables of every profile
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);  // once per call
  if (rc != PGB_OK) return rc;
  const size_t job_bytes = n_job * sizeof(PdpJob);
  std::vector<uint8_t> hb(job_bytes + (bps.size() + 1) * sizeof(double));
  memcpy(hb.data(), jobs.data(), job_bytes);
  if (!bps.empty()) memcpy(hb.data() + job_bytes, bps.data(), bps.size() * sizeof(double));
  HIPCHK(hipMalloc((void**)&job.p, hb.size()));
  HIPCHK(hipMemcpyAsync(job.p, hb.data(), hb.size(), hipMemcpyHostToDevice, sm));
  const PdpJob* jobs_dev = (const PdpJob*)job.p;
  const double* bp_dev = (const double*)(job.p + job_bytes);
  if (any_profile) HIPCHK(hipMalloc((void**)&tab.p, (size_t)n_tab * sizeof(double)));
  double* tab_dev = (double*)tab.p;
  const unsigned gy = (unsigned)(n_picks < 65535 ? n_picks : 65535), gz = (unsigned)(n_cols < 65535 ? n_cols : 65535);
  const PredTrees T = pk.T;
  auto launch_walk = [&](dim3 grid, int profile, double* out) {
    dispatch_bools(pk.cont, K == 1, [&](auto C, auto K1) {
      hipLaunchKernelGGL((k_pdp_walk<C(), K1()>), grid, dim3(PRED_BT), 0, sm, T, pk.fidx, (int)m, K, jobs_dev, (int)n_picks,
                         (int)n_cols, profile, X_dev, (long long)n_rows, (long long)ldx, bp_dev, out);
    });
    return hipGetLastError();
  };
  hipError_t e = hipSuccess;
  WalkTimer wt_walk(sm);
  if (any_profile) e = launch_walk(dim3((unsigned)((max_slots + PRED_BT - 1) / PRED_BT), gy, gz), 1, tab_dev);
  if (any_direct && e == hipSuccess) e = launch_walk(dim3((unsigned)gx, gy, gz), 0, out_dev);
  wt_walk.launched();
  WalkTimer wt_look(sm);
  if (any_profile && e == hipSuccess) {
    const int cap = max_B < PGB_PDP_LDS_MAXB ? max_B : PGB_PDP_LDS_MAXB;
    const size_t lds = ((size_t)cap + (size_t)(cap + 2) * K) * sizeof(double);
    const long long lx = (n_rows + PDP_LT - 1) / PDP_LT;
    dim3 grid((unsigned)lx, gz);
    if (K == 1)
      hipLaunchKernelGGL((k_pdp_lookup<true>), grid, dim3(PDP_LT), lds, sm, jobs_dev, (int)n_picks, (int)n_cols, K, cap, X_dev,
                         (long long)n_rows, (long long)ldx, bp_dev, (const double*)tab_dev, out_dev);
    else
      hipLaunchKernelGGL((k_pdp_lookup<false>), grid, dim3(PDP_LT), lds, sm, jobs_dev, (int)n_picks, (int)n_cols, K, cap, X_dev,
                         (long long)n_rows, (long long)ldx, bp_dev, (const double*)tab_dev, out_dev);
    e = hipGetLastError();
  }
  if (!any_profile) wt_look.drop();  // nothing was looked up: no lookup time
  return finish_walk(e, sm, wt_look, &g_pdp_lookup_ms, "k_pdp", &wt_walk, &g_pdp_walk_ms);
}
