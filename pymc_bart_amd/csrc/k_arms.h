// k_arms.h -- part of pgbart_hip.hip (not a standalone header): choosing among candidate interventions with stored
// draws (include/pgbart_arms.h holds the numeric contract, the packer of the union use lists and the sequential
// reference), the kernels and the host side of pgb_predict_arms, pgb_arm_decide and pgb_arm_decide_finish.
//
//   k_arms         launched as k_ale / k_permimp are: one wave per workgroup, lane = row, the tile staged in LDS as
//                  k_predict stages it when p <= PRED_LDS_MAXP; blockIdx.y strides over the picks.  Per pick one walk of
//                  the pick's union list at the row (A_self) and one per arm -- pred_walk_forest itself, with ArmRowX
//                  returning the arm's value for any of the s columns -- and K coalesced stores of f + (A_a - A_self)
//                  per arm.  cols and the arm's values are read with wave-uniform addresses (scalar loads; s <= 16).  A
//                  tile stays on the walk's `clean` path under an arm only if the tile and that arm hold no NaN, decided
//                  per wave and per arm.  No LDS beyond the tile, no scratch beyond the walk's two stacks, no atomics.
//   k_arms_best    one lane per (d, i): u of every arm (coalesced across i, stride lda across the arms), the best arm
//                  and umax of the block into device scratch.
//   k_arms_rows    one lane per (a, i), blockIdx.y = a: runs over d for SU, SR and NB; leaves SU in mean_dev.
//   k_arms_bayes   one lane per i: bayes_i from SU[.], then mean_dev = SU / D.
//   k_arms_reduce  the shape of k_rowreduce: one WAVE owns one (d, j) and streams the block's rows 64 at a time, lane l
//                  forming partial l of its sums for its current group in registers.  j = 0 carries VO, VB, VP (it
//                  gathers u of bayes_i and of pi_i) and -- for d = 0 -- W and the two row counters; j = 1 + a carries
//                  VA[a] and SH[a].  So no lane holds more than three sums, and no two waves share a slot of the
//                  workspace: no floating-point atomics, no LDS, no barrier.
//   k_arms_finish  one lane per (d, g, slot): pgb_rowsum_lanes of its 64 partials and pgb_arms_finish_one.
#include "pgbart_arms.h"

#define ARMS_BT 256
#define ARMS_WAVES (ARMS_BT / 64)

// xval of a row under an arm: the arm's value at any of the s columns, the row's own value elsewhere
template <class XV>
struct ArmRowX {
  XV own;
  const int32_t* __restrict__ cols;  // [s], wave-uniform
  const double* __restrict__ val;    // [s], wave-uniform: the arm's values
  int s;
  __device__ __forceinline__ double operator()(int j) const {
    double v = own(j);
    for (int t = 0; t < s; ++t) v = j == cols[t] ? val[t] : v;
    return v;
  }
};

template <bool LDSX, bool CONT>
__global__ __launch_bounds__(PRED_BT) void k_arms(PredTrees T, int K, int p, const double* __restrict__ X, long long nb,
                                                  long long ldx, const int32_t* __restrict__ cols, int s,
                                                  const double* __restrict__ arms, int A,
                                                  const int32_t* __restrict__ use_off, const int32_t* __restrict__ use_list,
                                                  int n_picks, const double* __restrict__ f, double* __restrict__ out) {
  extern __shared__ double arms_s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
  if constexpr (LDSX) pred_stage_rows(arms_s_x, X, row0, nb, ldx, p, lane);
  if (row >= nb) return;
  const PredRowX<LDSX> xval{arms_s_x, X + row * ldx, lane};
  const bool clean = pred_wave_clean<CONT>(p, xval);
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  const size_t slab = (size_t)n_picks * K * (size_t)nb;
  for (int pick = blockIdx.y; pick < n_picks; pick += gridDim.y) {
    const int32_t* __restrict__ list = use_list + use_off[pick];
    const int len = use_off[pick + 1] - use_off[pick];
    double a_self[PGB_MAX_OUTPUTS], a_arm[PGB_MAX_OUTPUTS];
    pred_walk_forest<CONT>(T, list, len, K, clean, xval, stk_node, stk_w, a_self);
    const size_t at = ((size_t)pick * K) * (size_t)nb + row;
    for (int a = 0; a < A; ++a) {
      const double* __restrict__ val = arms + (size_t)a * s;
      bool aclean = false;
      if (CONT) {
        bool nan = false;  // (wave-uniform: the arm is the same for every lane)
        for (int t = 0; t < s; ++t) nan = nan || val[t] != val[t];
        aclean = clean && !nan;
      }
      const ArmRowX<PredRowX<LDSX>> aval{xval, cols, val, s};
      pred_walk_forest<CONT>(T, list, len, K, aclean, aval, stk_node, stk_w, a_arm);
      double* __restrict__ o_a = out + (size_t)a * slab + at;
      for (int o = 0; o < K; ++o) {
        const double delta = a_arm[o] - a_self[o];
        o_a[(size_t)o * nb] = f[at + (size_t)o * nb] + delta;
      }
    }
  }
}

// ------------------------------------------------------------------ the decide step
struct ArmsU {  // what u of one (a, d, i) needs beyond f
  const double* __restrict__ off;   // [nb] or nullptr
  const double* __restrict__ cost;  // [A] (zeros without costs)
  double sign;
  int transform;
  pgb_lltabs tb;
  __device__ __forceinline__ double operator()(double fv, long long i, int a) const {
    return pgb_arms_utility(fv, off != nullptr, off ? off[i] : 0.0, transform, &tb, sign, cost[a]);
  }
};
__device__ __forceinline__ pgb_lltabs arms_tabs() {
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
  return tb;
}

__global__ __launch_bounds__(ARMS_BT) void k_arms_best(const double* __restrict__ f, long long lda, long long ldd, int D, int A,
                                                       long long nb, const double* __restrict__ off,
                                                       const double* __restrict__ cost, double sign, int transform,
                                                       double* __restrict__ umax_s, int32_t* __restrict__ best_s) {
  const long long i = (long long)blockIdx.x * ARMS_BT + threadIdx.x;
  if (i >= nb) return;
  const ArmsU u_of{off, cost, sign, transform, arms_tabs()};
  for (int d = blockIdx.y; d < D; d += gridDim.y) {
    const double* __restrict__ fd = f + (size_t)d * (size_t)ldd + i;
    int best = 0;
    double umax = u_of(fd[0], i, 0);
    for (int a = 1; a < A; ++a) {
      const double u = u_of(fd[(size_t)a * (size_t)lda], i, a);
      const bool take = pgb_arms_better(u, umax);
      best = take ? a : best;
      umax = take ? u : umax;
    }
    umax_s[(size_t)d * (size_t)nb + i] = umax;
    best_s[(size_t)d * (size_t)nb + i] = best;
  }
}

__global__ __launch_bounds__(ARMS_BT) void k_arms_rows(const double* __restrict__ f, long long lda, long long ldd, int D,
                                                       long long nb, const double* __restrict__ off,
                                                       const double* __restrict__ cost, double sign, int transform,
                                                       const double* __restrict__ umax_s, const int32_t* __restrict__ best_s,
                                                       int32_t* __restrict__ nbest, double* __restrict__ su_out,
                                                       double* __restrict__ regret, unsigned long long* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * ARMS_BT + threadIdx.x;
  if (i >= nb) return;
  const int a = blockIdx.y;
  const ArmsU u_of{off, cost, sign, transform, arms_tabs()};
  const double* __restrict__ fa = f + (size_t)a * (size_t)lda + i;
  double su = 0.0, sr = 0.0;
  int32_t n_best = 0;
  unsigned long long n_nonfinite = 0;
  for (int d = 0; d < D; ++d) {
    const double u = u_of(fa[(size_t)d * (size_t)ldd], i, a);
    n_nonfinite += pgb_rowred_nonfinite(u) ? 1 : 0;
    su = su + u;
    sr = sr + (umax_s[(size_t)d * (size_t)nb + i] - u);
    n_best += best_s[(size_t)d * (size_t)nb + i] == a ? 1 : 0;
  }
  const size_t at = (size_t)a * (size_t)nb + i;
  nbest[at] = n_best;
  su_out[at] = su;
  regret[at] = sr / (double)D;
  if (n_nonfinite) atomicAdd(&cnt[0], n_nonfinite);
}

__global__ __launch_bounds__(ARMS_BT) void k_arms_bayes(int D, int A, long long nb, double* __restrict__ mean,
                                                        int32_t* __restrict__ bayes) {
  const long long i = (long long)blockIdx.x * ARMS_BT + threadIdx.x;
  if (i >= nb) return;
  int by = 0;
  double top = mean[i];  // (SU, left here by k_arms_rows)
  mean[i] = top / (double)D;
  for (int a = 1; a < A; ++a) {
    const double su = mean[(size_t)a * (size_t)nb + i];
    const bool take = pgb_arms_better(su, top);
    by = take ? a : by;
    top = take ? su : top;
    mean[(size_t)a * (size_t)nb + i] = su / (double)D;
  }
  bayes[i] = by;
}

__global__ __launch_bounds__(ARMS_BT) void k_arms_reduce(const double* __restrict__ f, long long lda, long long ldd, int D, int A,
                                                         long long nb, const double* __restrict__ w,
                                                         const int32_t* __restrict__ g, const int32_t* __restrict__ policy,
                                                         const double* __restrict__ off, const double* __restrict__ cost,
                                                         double sign, int transform, int G,
                                                         const double* __restrict__ umax_s, const int32_t* __restrict__ best_s,
                                                         const int32_t* __restrict__ bayes, long long wpart_off,
                                                         double* __restrict__ ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * ARMS_WAVES + wave;  // (d, j), j fastest
  if (item >= (long long)D * (A + 1)) return;
  const int d = (int)(item / (A + 1)), j = (int)(item % (A + 1));
  const bool first = item == 0;  // (the wave that also sums the weights and counts the rows left out)
  const bool has_pi = policy != nullptr;
  const int ns = PGB_ARMS_NSUMS(A);
  const ArmsU u_of{off, cost, sign, transform, arms_tabs()};
  double* part = ws + (size_t)d * (size_t)G * (size_t)ns * PGB_ROWRED_LANES + lane;  // + (g ns + slot) 64
  double* wpart = ws + wpart_off + lane;                                            // + g 64
  unsigned long long* cnt = (unsigned long long*)(ws + wpart_off + (size_t)G * PGB_ROWRED_LANES);
  const double* __restrict__ fd = f + (size_t)d * (size_t)ldd;
  const size_t sd = (size_t)d * (size_t)nb;
  // the slots of this wave: j = 0: VO, VB, VP; j = 1 + a: VA[a], SH[a]
  const int a = j - 1;
  const int slot0 = j == 0 ? PGB_ARMS_VO : PGB_ARMS_VA(a);
  const int slot1 = j == 0 ? PGB_ARMS_VB : PGB_ARMS_SH(A, a);

  int gc = -1;  // the group whose partials are in the registers
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0;
  unsigned long long n_bad_g = 0, n_bad_pi = 0;
  auto put = [&](int gq) {
    double* p = part + (size_t)gq * (size_t)ns * PGB_ROWRED_LANES;
    p[(size_t)slot0 * PGB_ROWRED_LANES] = s0;
    p[(size_t)slot1 * PGB_ROWRED_LANES] = s1;
    if (j == 0 && has_pi) p[(size_t)PGB_ARMS_VP * PGB_ROWRED_LANES] = s2;
    if (first) wpart[(size_t)gq * PGB_ROWRED_LANES] = sw;
  };
  for (long long i = lane; i < nb; i += PGB_ROWRED_LANES) {
    const int gi = g[i];
    const int pi = has_pi ? policy[i] : 0;
    const bool bad_g = gi < 0 || gi >= G, bad_pi = pi < 0 || pi >= A;
    if (bad_g || bad_pi) {
      n_bad_g += first && bad_g ? 1 : 0;
      n_bad_pi += first && bad_pi ? 1 : 0;
      continue;
    }
    const double wi = w[i];
    if (gi != gc) {
      if (gc >= 0) put(gc);
      const double* p = part + (size_t)gi * (size_t)ns * PGB_ROWRED_LANES;
      s0 = p[(size_t)slot0 * PGB_ROWRED_LANES];
      s1 = p[(size_t)slot1 * PGB_ROWRED_LANES];
      if (j == 0 && has_pi) s2 = p[(size_t)PGB_ARMS_VP * PGB_ROWRED_LANES];
      if (first) sw = wpart[(size_t)gi * PGB_ROWRED_LANES];
      gc = gi;
    }
    if (j == 0) {
      const int by = bayes[i];
      s0 = s0 + wi * umax_s[sd + i];
      s1 = s1 + wi * u_of(fd[(size_t)by * (size_t)lda + i], i, by);
      if (has_pi) s2 = s2 + wi * u_of(fd[(size_t)pi * (size_t)lda + i], i, pi);
      if (first) sw = sw + wi;
    } else {
      s0 = s0 + wi * u_of(fd[(size_t)a * (size_t)lda + i], i, a);
      if (best_s[sd + i] == a) s1 = s1 + wi;
    }
  }
  if (gc >= 0) put(gc);
  if (n_bad_g) atomicAdd(&cnt[1], n_bad_g);
  if (n_bad_pi) atomicAdd(&cnt[2], n_bad_pi);
}

__global__ __launch_bounds__(ARMS_BT) void k_arms_finish(const double* __restrict__ ws, int D, int G, int A, long long wpart_off,
                                                         double* __restrict__ out, double* __restrict__ w_out) {
  const int ns = PGB_ARMS_NSUMS(A);
  const long long n_items = (long long)D * G;
  const long long t = (long long)blockIdx.x * ARMS_BT + threadIdx.x;  // (item, slot), slot fastest
  if (t >= n_items * ns) return;
  const long long item = t / ns;
  const int slot = (int)(t % ns), gi = (int)(item % G);
  const double* __restrict__ p = ws + (size_t)item * (size_t)ns * PGB_ROWRED_LANES;
  const double W = pgb_rowsum_lanes(ws + wpart_off + (size_t)gi * PGB_ROWRED_LANES);
  const double s_vb = slot == PGB_ARMS_VO ? pgb_rowsum_lanes(p + (size_t)PGB_ARMS_VB * PGB_ROWRED_LANES) : 0.0;
  pgb_arms_finish_one(pgb_rowsum_lanes(p + (size_t)slot * PGB_ROWRED_LANES), s_vb, W, slot, item, n_items, out);
  if (item < G && slot == 0) w_out[gi] = W;  // d = 0
}

// every buffer of one call, released on every way out
struct ArmsScratch {
  uint8_t* rec = nullptr;  // device
  pgb_arms_pack pack;
  ArmsScratch() { memset(&pack, 0, sizeof pack); }
  ~ArmsScratch() {
    if (rec) (void)hipFree(rec);
    pgb_arms_pack_free(&pack);
  }
};

static thread_local double g_arms_ms[2] = {-1.0, -1.0};
extern "C" int pgb_arms_kernel_ms(double* walk_ms, double* decide_ms) {
  if (!walk_ms || !decide_ms) return fail(PGB_E_INVALID, "null argument");
  *walk_ms = g_arms_ms[0];
  *decide_ms = g_arms_ms[1];
  return PGB_OK;
}

extern "C" int pgb_predict_arms(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                                const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const int32_t* cols_host, int32_t s,
                                const double* arms_host, int32_t A, const int32_t* picks_host, int32_t n_picks,
                                const double* f_dev, double* out_dev, int32_t* list_len_host, void* stream) {
  PredCall pc("pgb_predict_arms");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(cols_host, "cols_host");
  pc.null(arms_host, "arms_host");
  pc.null(picks_host, "picks_host");
  pc.null(f_dev, "f_dev");
  pc.null(out_dev, "out_dev");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(nb, "nb");
  pc.at_least_one(s, "s");
  pc.at_least_one(A, "A");
  pc.at_least_one(n_picks, "n_picks");
  pc.ld(ldx, p, "ldx");
  pc.require(s <= PGB_ARMS_MAX_COLS, "s must be <= PGB_ARMS_MAX_COLS = " PGB_STR(PGB_ARMS_MAX_COLS));
  pc.require(A <= PGB_ARMS_MAX, "A must be <= PGB_ARMS_MAX = " PGB_STR(PGB_ARMS_MAX));
  long long gx = 0;
  pc.tiles(nb, &gx);
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.index_vector(cols_host, (size_t)s, p, "cols_host", "p");
  pc.distinct(cols_host, s);
  pc.index_vector(picks_host, (size_t)n_picks, n_forests, "picks_host", "n_forests");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.n_outputs(trees);
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;
  const int K = trees->n_outputs;
  pc.cells_fit({A, n_picks, K, nb}, "A x n_picks x K x nb");
  if (pc.rc() != PGB_OK) return pc.rc();

  ArmsScratch sc;
  const int prc = pgb_arms_pack_build(trees, forest_tree_idx, m, p, cols_host, s, picks_host, n_picks, &sc.pack);  // once per call
  if (prc == -1) return pc.refuse(PGB_E_NOMEM, "the use lists do not fit host memory");
  if (prc != 0) return pc.refuse(PGB_E_INVALID, "the use lists hold more than 2^31 - 1 trees");
  hipStream_t sm = (hipStream_t)stream;
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);
  if (rc != PGB_OK) return rc;
  // one upload: [the arms | the header's pack | the columns]
  const size_t n_pack = (size_t)(sc.pack.n_lists + 1 + sc.pack.n_list);
  const size_t o_pack = (size_t)A * (size_t)s * sizeof(double);
  const size_t o_cols = o_pack + n_pack * sizeof(int32_t);
  std::vector<uint8_t> hb(o_cols + (size_t)s * sizeof(int32_t));
  memcpy(hb.data(), arms_host, o_pack);
  memcpy(hb.data() + o_pack, sc.pack.buf, n_pack * sizeof(int32_t));
  memcpy(hb.data() + o_cols, cols_host, (size_t)s * sizeof(int32_t));
  HIPCHK(hipMalloc((void**)&sc.rec, hb.size()));
  HIPCHK(hipMemcpyAsync(sc.rec, hb.data(), hb.size(), hipMemcpyHostToDevice, sm));
  const double* arms_dev = (const double*)sc.rec;
  const int32_t* off_dev = (const int32_t*)(sc.rec + o_pack);
  const int32_t* list_dev = off_dev + sc.pack.n_lists + 1;
  const int32_t* cols_dev = (const int32_t*)(sc.rec + o_cols);
  // one wave per workgroup; enough workgroups to fill the chip (pgb_predict's figure), each looping over its share of
  // the picks
  const long long want_wgs = p <= PRED_LDS_MAXP ? 16384 : 4096;
  long long gy = (want_wgs + gx - 1) / gx;
  if (gy > n_picks) gy = n_picks;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  dim3 grid((unsigned)gx, (unsigned)gy);
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  WalkTimer wt(sm);
  dispatch_bools(ldsx, pk.cont, [&](auto L, auto C) {
    hipLaunchKernelGGL((k_arms<L(), C()>), grid, dim3(PRED_BT), lds, sm, pk.T, K, (int)p, X_dev, (long long)nb, (long long)ldx,
                       cols_dev, (int)s, arms_dev, (int)A, off_dev, list_dev, (int)n_picks, f_dev, out_dev);
  });
  rc = finish_walk(hipGetLastError(), sm, wt, &g_arms_ms[0], "k_arms");
  if (rc == PGB_OK && list_len_host) {
    const int32_t* off = pgb_arms_pack_off(&sc.pack);
    for (int d = 0; d < n_picks; ++d) list_len_host[d] = off[d + 1] - off[d];
  }
  return rc;
}

static bool arms_dims_ok(int32_t D, int32_t G, int32_t A) {
  return D >= 1 && G >= 1 && G <= PGB_ROWRED_MAX_GROUPS && A >= 1 && A <= PGB_ARMS_MAX;
}
static void arms_dims(PredCall& pc, int32_t D, int32_t G, int32_t A) {
  pc.at_least_one(D, "D");
  pc.at_least_one(A, "A");
  pc.require(A <= PGB_ARMS_MAX, "A must be <= PGB_ARMS_MAX = " PGB_STR(PGB_ARMS_MAX));
  pc.require(G >= 1 && G <= PGB_ROWRED_MAX_GROUPS, "G must be in [1, PGB_ROWRED_MAX_GROUPS = " PGB_STR(PGB_ROWRED_MAX_GROUPS) "]");
}

extern "C" int64_t pgb_arm_decide_workspace_bytes(int32_t D, int32_t G, int32_t A) {
  if (!arms_dims_ok(D, G, A)) return 0;
  return 8 * pgb_arms_ws_doubles(D, G, A);
}

extern "C" int pgb_arm_decide(const double* f_dev, int64_t lda, int64_t ldd, int32_t D, int32_t A, int64_t nb,
                              const double* w_dev, const int32_t* g_dev, const int32_t* policy_dev, const double* off_dev,
                              const double* cost_host, double sign, int32_t transform, int32_t G, int64_t first_row,
                              int32_t init, void* ws_dev, int32_t* nbest_dev, double* mean_dev, double* regret_dev,
                              int32_t* bayes_dev, void* stream) {
  PredCall pc("pgb_arm_decide");
  pc.null(f_dev, "f_dev");
  pc.null(w_dev, "w_dev");
  pc.null(g_dev, "g_dev");
  pc.null(ws_dev, "ws_dev");
  pc.null(nbest_dev, "nbest_dev");
  pc.null(mean_dev, "mean_dev");
  pc.null(regret_dev, "regret_dev");
  pc.null(bayes_dev, "bayes_dev");
  arms_dims(pc, D, G, A);
  pc.at_least_one(nb, "nb");
  pc.require(nb <= ((int64_t)1 << 40), "nb must be <= 2^40");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.require(ldd >= nb, "ldd must be >= nb");
  pc.require(ldd <= ((int64_t)1 << 45) && lda <= ((int64_t)1 << 50), "lda or ldd overflows the index arithmetic");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.require(lda >= (int64_t)(D - 1) * ldd + nb, "lda must be >= (D - 1) ldd + nb");
  pc.require(first_row >= 0 && first_row % PGB_ROWRED_LANES == 0,
             "first_row must be a multiple of " PGB_STR(PGB_ROWRED_LANES) " and >= 0");
  pc.require(transform >= 0 && transform < PGB_ROWSUM_N_TRANSFORMS, "unknown transform");
  pc.require(sign == 1.0 || sign == -1.0, "sign must be +1.0 or -1.0");
  for (int a = 0; cost_host && pc.rc() == PGB_OK && a < A; ++a)
    if (!std::isfinite(cost_host[a])) pc.refuse(PGB_E_INVALID, "cost_host[%d] is not finite", a);
  pc.cells_fit({D, nb}, "D x nb (the scratch of a block)");
  if (pc.rc() != PGB_OK) return pc.rc();

  hipStream_t sm = (hipStream_t)stream;
  // the scratch of the block: [umax D nb | cost A | best D nb]
  ArmsScratch sc;
  const size_t n_dn = (size_t)D * (size_t)nb;
  const size_t o_cost = n_dn * sizeof(double);
  const size_t o_best = o_cost + (size_t)A * sizeof(double);
  HIPCHK(hipMalloc((void**)&sc.rec, o_best + n_dn * sizeof(int32_t)));
  double cost[PGB_ARMS_MAX];
  for (int a = 0; a < A; ++a) cost[a] = cost_host ? cost_host[a] : 0.0;
  HIPCHK(hipMemcpyAsync(sc.rec + o_cost, cost, (size_t)A * sizeof(double), hipMemcpyHostToDevice, sm));
  double* umax_s = (double*)sc.rec;
  const double* cost_dev = (const double*)(sc.rec + o_cost);
  int32_t* best_s = (int32_t*)(sc.rec + o_best);
  const long long wpart_off = pgb_arms_wpart(D, G, A);
  if (init) {
    const hipError_t e = hipMemsetAsync(ws_dev, 0, (size_t)8 * (size_t)pgb_arms_ws_doubles(D, G, A), sm);  // (all bits 0: 0.0)
    if (e != hipSuccess) return fail_hip(e, "pgb_arm_decide: clearing the workspace");
  }
  unsigned long long* cnt = (unsigned long long*)((double*)ws_dev + pgb_arms_counters(D, G, A));
  const long long bx = (nb + ARMS_BT - 1) / ARMS_BT;
  long long by = (16384 + bx - 1) / bx;  // enough workgroups to fill the chip, each striding over its draws
  if (by > D) by = D;
  WalkTimer wt(sm);
  hipLaunchKernelGGL(k_arms_best, dim3((unsigned)bx, (unsigned)by), dim3(ARMS_BT), 0, sm, f_dev, (long long)lda, (long long)ldd,
                     (int)D, (int)A, (long long)nb, off_dev, cost_dev, sign, (int)transform, umax_s, best_s);
  hipLaunchKernelGGL(k_arms_rows, dim3((unsigned)bx, (unsigned)A), dim3(ARMS_BT), 0, sm, f_dev, (long long)lda, (long long)ldd,
                     (int)D, (long long)nb, off_dev, cost_dev, sign, (int)transform, (const double*)umax_s,
                     (const int32_t*)best_s, nbest_dev, mean_dev, regret_dev, cnt);
  hipLaunchKernelGGL(k_arms_bayes, dim3((unsigned)bx), dim3(ARMS_BT), 0, sm, (int)D, (int)A, (long long)nb, mean_dev, bayes_dev);
  const long long n_waves = (long long)D * (A + 1);
  hipLaunchKernelGGL(k_arms_reduce, dim3((unsigned)((n_waves + ARMS_WAVES - 1) / ARMS_WAVES)), dim3(ARMS_BT), 0, sm, f_dev,
                     (long long)lda, (long long)ldd, (int)D, (int)A, (long long)nb, w_dev, g_dev, policy_dev, off_dev, cost_dev,
                     sign, (int)transform, (int)G, (const double*)umax_s, (const int32_t*)best_s, (const int32_t*)bayes_dev,
                     wpart_off, (double*)ws_dev);
  return finish_walk(hipGetLastError(), sm, wt, &g_arms_ms[1], "k_arms_reduce");
}

extern "C" int pgb_arm_decide_finish(const void* ws_dev, int32_t D, int32_t G, int32_t A, int32_t has_policy, double* out_dev,
                                     double* w_out_dev, int64_t* counts_out, void* stream) {
  PredCall pc("pgb_arm_decide_finish");
  pc.null(ws_dev, "ws_dev");
  pc.null(out_dev, "out_dev");
  pc.null(w_out_dev, "w_out_dev");
  pc.null(counts_out, "counts_out");
  arms_dims(pc, D, G, A);
  pc.require(has_policy == 0 || has_policy == 1, "has_policy must be 0 or 1");
  if (pc.rc() != PGB_OK) return pc.rc();
  const long long n_threads = (long long)D * G * PGB_ARMS_NSUMS(A);
  const long long wpart_off = pgb_arms_wpart(D, G, A);
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_arms_finish, dim3((unsigned)((n_threads + ARMS_BT - 1) / ARMS_BT)), dim3(ARMS_BT), 0, sm,
                     (const double*)ws_dev, (int)D, (int)G, (int)A, wpart_off, out_dev, w_out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_arms_finish launch");
  int64_t counts[3];
  e = hipMemcpyAsync(counts, (const double*)ws_dev + pgb_arms_counters(D, G, A), sizeof counts, hipMemcpyDeviceToHost, sm);
  if (e != hipSuccess) return fail_hip(e, "pgb_arm_decide_finish: reading the counters");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_arms_finish");
  for (int j = 0; j < 3; ++j) counts_out[j] = counts[j];
  if (counts[1] != 0) return pc.refuse(PGB_E_INVALID, "%lld rows have a group outside [0, %d)", (long long)counts[1], (int)G);
  if (counts[2] != 0 && has_policy)
    return pc.refuse(PGB_E_INVALID, "%lld rows have a policy outside [0, %d)", (long long)counts[2], (int)A);
  return PGB_OK;
}
