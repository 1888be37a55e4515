// pgb_pred_host.h -- part of pgbart_hip.hip (not a standalone header): the host front end shared by every entry point
// that walks stored draws (pgb_predict here; pgb_pointwise_loglik, pgb_predict_ice, pgb_predict_pdp, pgb_predict_shap
// and pgb_predict_shap_interactions in the parts after this one): the argument checker that carries the entry point's
// name (PredCall), the history's validation and packing (pred_validate, pred_pack), the bool-to-template dispatch of a
// launch (dispatch_bools) and its epilogue (WalkTimer, finish_walk).
#include <algorithm>
#include <cstdarg>
#include <initializer_list>
#include <utility>

// The argument checks of one entry point, each sentence written once and prefixed with the entry point's name.  The
// first failing check wins: every later one is skipped, so a preamble is a flat list of calls in the order the checks
// fire, read out with rc() before the first use of what they guard.
struct PredCall {
  const char* fn;
  int code = PGB_OK;
  explicit PredCall(const char* fn_) : fn(fn_) {}
  int rc() const { return code; }
  __attribute__((format(printf, 3, 4))) int refuse(int code_, const char* fmt, ...) {
    if (code != PGB_OK) return code;
    int n = snprintf(g_err, sizeof g_err, "%s: ", fn);
    if (n < 0 || n >= (int)sizeof g_err) n = (int)sizeof g_err - 1;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err + n, sizeof g_err - (size_t)n, fmt, ap);
    va_end(ap);
    return code = code_;
  }
  void require(bool holds, const char* otherwise) {
    if (!holds) refuse(PGB_E_INVALID, "%s", otherwise);
  }
  void null(const void* ptr, const char* name) {
    if (!ptr) refuse(PGB_E_INVALID, "%s is null", name);
  }
  void forest_dims(int32_t n_forests, int32_t m, int32_t p) {
    require(n_forests >= 1 && m >= 1 && p >= 1, "n_forests, m and p must be >= 1");
  }
  void at_least_one(int64_t v, const char* name) {
    if (v < 1) refuse(PGB_E_INVALID, "%s must be >= 1", name);
  }
  void ld(int64_t ld_, int32_t p, const char* name) {
    if (ld_ < p) refuse(PGB_E_INVALID, "%s must be >= p", name);
  }
  void tiles(int64_t n_rows, long long* gx) {  // *gx: the row tiles of PRED_BT rows, the x extent of the grid
    if (code != PGB_OK) return;
    *gx = (n_rows + PRED_BT - 1) / PRED_BT;
    if (*gx > 0x7fffffffLL) refuse(PGB_E_INVALID, "n_rows exceeds 2^31 - 1 tiles of 64 rows");
  }
  // every v[i], i < n, lies in [0, hi): "cols_host" against "p", "picks_host" against "n_forests"
  void index_vector(const int32_t* v, size_t n, int32_t hi, const char* name, const char* hi_name) {
    for (size_t i = 0; code == PGB_OK && i < n; ++i)
      if (v[i] < 0 || v[i] >= hi) refuse(PGB_E_INVALID, "%s[%zu] = %d is outside [0, %s = %d)", name, i, (int)v[i], hi_name, (int)hi);
  }
  void distinct(const int32_t* cols, int32_t n_cols) {  // (sorted pairs: p itself may be far larger than n_cols)
    if (code != PGB_OK) return;
    std::vector<std::pair<int32_t, int32_t>> by((size_t)n_cols);
    for (int c = 0; c < n_cols; ++c) by[c] = {cols[c], c};
    std::sort(by.begin(), by.end());
    for (int c = 1; code == PGB_OK && c < n_cols; ++c)
      if (by[c].first == by[c - 1].first)
        refuse(PGB_E_INVALID, "cols_host[%d] = %d repeats cols_host[%d]", (int)by[c].second, (int)by[c].first, (int)by[c - 1].second);
  }
  // out_dev holds the product of `factors` doubles: their bytes must fit a 64-bit size (and the index arithmetic)
  void cells_fit(std::initializer_list<int64_t> factors, const char* shape) {
    const uint64_t lim = (uint64_t)1 << 60;
    uint64_t cells = 1;
    for (const int64_t f : factors) {
      if (code != PGB_OK) return;
      if (cells > lim / (uint64_t)f) refuse(PGB_E_INVALID, "out_dev of %s doubles overflows a 64-bit size", shape);
      cells *= (uint64_t)f;
    }
  }
  void n_outputs(const pgb_tree_arrays* trees) {  // (the sentence is the oracle's: it carries no prefix)
    if (code == PGB_OK && (trees->n_outputs < 1 || trees->n_outputs > PGB_MAX_OUTPUTS)) code = fail(PGB_E_INVALID, "n_outputs");
  }
};

// The history of a prediction (pgb_predict, pgb_pointwise_loglik, pgb_predict_ice), checked: a malformed one
// (truncated file, mismatched m, hand-built arrays) is an error, not an out-of-bounds walk and not a walk that never
// ends.  Beyond the ranges of the indices, every tree must be WALKABLE ("Walkable histories"):
//   * the nodes reachable from node 0 form a tree rooted there: no node is its own child or ancestor, none has two
//     parents, and the root is nobody's child -- the general walk of pgb_pred_walk.h follows left / right until it
//     meets a leaf, so a cycle would keep a wave on the device for ever;
//   * no node lies deeper than PGB_MAX_DEPTH (the root has depth 0) -- a walk that marginalises pushes one entry per
//     level on a private stack of PGB_MAX_DEPTH + 2 entries.  Both samplers stop splitting at that depth
//     (prior_leaf), so only loaded or hand-built arrays can break the rule.
// Nodes that cannot be reached from the root are never walked and are left alone.  The oracle's pgb_validate_forest
// makes the same checks in the same order and pgb_predict reports them with the same messages.
#define PGB_MSG_NOT_A_TREE "a tree's nodes do not form a tree rooted at node 0 (a node is its own ancestor or has two parents)"
#define PGB_MSG_TOO_DEEP "a tree is deeper than PGB_MAX_DEPTH = " PGB_STR(PGB_MAX_DEPTH)
static int pred_validate(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                         int32_t p) {
  if (trees->n_outputs < 1 || trees->n_outputs > PGB_MAX_OUTPUTS) return fail(PGB_E_INVALID, "n_outputs");
  // a malformed history (truncated file, mismatched m) is an error, not an out-of-bounds walk
  if (trees->n_trees < 0 || trees->total_nodes < 0) return fail(PGB_E_INVALID, "tree arrays are inconsistent (node_off / left / right)");
  for (long long i = 0; i < (long long)n_forests * m; ++i)
    if (forest_tree_idx[i] < 0 || forest_tree_idx[i] >= trees->n_trees)
      return fail(PGB_E_INVALID, "forest_tree_idx entry outside [0, n_trees)");
  std::vector<int32_t> dep, todo;  // depth of every node reached from the root (-1: not reached), the nodes to visit
  for (int t = 0; t < trees->n_trees; ++t) {
    const int base = trees->node_off[t], end = trees->node_off[t + 1];
    if (base < 0 || end <= base || end > trees->total_nodes)
      return fail(PGB_E_INVALID, "tree arrays are inconsistent (node_off / left / right)");
    for (int g = base; g < end; ++g) {
      if (trees->var[g] < 0) continue;
      if (trees->var[g] >= p) return fail(PGB_E_INVALID, "a tree splits on a column X does not have");
      if (trees->rule && trees->rule[g] != PGB_RULE_CONTINUOUS && trees->rule[g] != PGB_RULE_ONEHOT &&
          trees->rule[g] != PGB_RULE_SUBSET)
        return fail(PGB_E_INVALID, "a split node carries an unknown split rule");
      if (trees->left[g] < 0 || trees->right[g] < 0 || trees->left[g] >= end - base || trees->right[g] >= end - base)
        return fail(PGB_E_INVALID, "tree arrays are inconsistent (node_off / left / right)");
    }
    // walkable: breadth-first from node 0, left before right; a child met twice (or the root met at all) is a
    // second parent or a cycle
    const int nn = end - base;
    dep.assign((size_t)nn, -1);
    todo.clear();
    dep[0] = 0;
    todo.push_back(0);
    for (size_t q = 0; q < todo.size(); ++q) {
      const int k = todo[q];
      if (trees->var[base + k] < 0) continue;
      const int32_t ch[2] = {trees->left[base + k], trees->right[base + k]};
      for (int s = 0; s < 2; ++s) {
        if (dep[ch[s]] >= 0) return fail(PGB_E_INVALID, PGB_MSG_NOT_A_TREE);
        dep[ch[s]] = dep[k] + 1;
        if (dep[ch[s]] > PGB_MAX_DEPTH) return fail(PGB_E_INVALID, PGB_MSG_TOO_DEEP);
        todo.push_back(ch[s]);
      }
    }
  }
  return PGB_OK;
}

// ... and packed into ONE upload (db: owned, released with the pack) for the walk of pgb_pred_walk.h
struct PredPack {
  uint8_t* db = nullptr;
  PredTrees T;
  const int32_t* fidx = nullptr;  // [n_forests][m], device
  bool cont = true;               // every split of every tree is `x <= v`: the instances without the rule dispatch
  PredPack() = default;
  PredPack(const PredPack&) = delete;
  PredPack& operator=(const PredPack&) = delete;
  ~PredPack() {
    if (db) (void)hipFree(db);
  }
};
static int pred_pack(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m, int32_t p,
                     const int32_t* excluded_host, int32_t n_excluded, hipStream_t sm, PredPack* pk) {
  const int K = trees->n_outputs, N = trees->total_nodes, NT = trees->n_trees;
  std::vector<uint8_t> excl((size_t)p, 0);
  for (int e = 0; e < n_excluded; ++e)
    if (excluded_host[e] >= 0 && excluded_host[e] < p) excl[excluded_host[e]] = 1;
  const bool lin = trees->slope && trees->xbar && trees->svar;
  // one upload buffer: [PNode N | FNode N | value N K | (slope N K | xbar N) | root NT | fidx | (svar N)]
  const size_t o_fn = (size_t)N * sizeof(PNode);
  const size_t o_val = o_fn + (size_t)N * sizeof(FNode);
  const size_t o_slope = o_val + (size_t)N * K * 8;
  const size_t o_xbar = o_slope + (lin ? (size_t)N * K * 8 : 0);
  const size_t o_root = o_xbar + (lin ? (size_t)N * 8 : 0);
  const size_t o_f = o_root + (size_t)NT * sizeof(int2);
  const size_t o_svar = o_f + (size_t)n_forests * m * 4;
  const size_t bytes = o_svar + (lin ? (size_t)N * 4 : 0);
  std::vector<uint8_t> hb(bytes);
  PNode* hn = (PNode*)hb.data();
  FNode* hf = (FNode*)(hb.data() + o_fn);
  int2* hroot = (int2*)(hb.data() + o_root);
  std::vector<int> depth_of;
  bool cont = true;  // every split of every tree is `x <= v`: the instance without the rule dispatch
  int32_t* hsvar = (int32_t*)(hb.data() + o_svar);
  for (int t = 0; t < NT; ++t) {
    const int base = trees->node_off[t], end = trees->node_off[t + 1];
    // depth of the tree and whether it can take the fixed-length walk (<= 255 nodes, children after
    // their parent as both backends build them, no split on an excluded variable)
    const int nn = end - base;
    bool general = nn > 255 || nn < 1;
    int depth = 0;
    depth_of.assign((size_t)(nn > 0 ? nn : 1), 0);
    for (int k = 0; k < nn && !general; ++k) {
      const int g = base + k;
      if (trees->var[g] < 0) continue;
      const int l = trees->left[g], r = trees->right[g];
      if (l <= k || r <= k || l >= nn || r >= nn) { general = true; break; }
      if (trees->var[g] < p && excl[trees->var[g]]) general = true;
      depth_of[l] = depth_of[r] = depth_of[k] + 1;
      if (depth_of[k] + 1 > depth) depth = depth_of[k] + 1;
    }
    if (depth > 255) general = true;
    hroot[t] = make_int2(base, general ? 0x100 : depth);
    for (int g = base; g < end; ++g) {
      PNode z;
      z.var = trees->var[g];
      if (z.var >= p) return fail(PGB_E_INVALID, "a tree splits on a column X does not have");
      z.left = z.var >= 0 ? base + trees->left[g] : -1;
      z.right = z.var >= 0 ? base + trees->right[g] : -1;
      const int rule = z.var >= 0 && trees->rule ? trees->rule[g] : PGB_RULE_CONTINUOUS;  // the node's own
      if (rule != PGB_RULE_CONTINUOUS) cont = false;
      z.flags = z.var >= 0 ? ((rule << 1) | (excl[z.var] ? 1 : 0)) : 0;
      z.split = trees->split[g];
      z.cnt = (double)trees->count[g];
      hn[g] = z;
      FNode f;
      f.pad = 0;
      if (z.var >= 0 && !general) {
        f.split = z.split; f.var = z.var; f.left = (uint8_t)trees->left[g]; f.right = (uint8_t)trees->right[g];
      } else {  // a leaf points at itself: x <= +inf for every value that is not NaN
        f.split = __builtin_inf(); f.var = 0; f.left = f.right = (uint8_t)((g - base) & 255);
      }
      hf[g] = f;
      if (lin) {
        const int js = trees->svar[g];
        hsvar[g] = (js >= 0 && js < p && !excl[js]) ? js : -1;
      }
    }
  }
  memcpy(hb.data() + o_val, trees->value, (size_t)N * K * 8);
  if (lin) {
    memcpy(hb.data() + o_slope, trees->slope, (size_t)N * K * 8);
    memcpy(hb.data() + o_xbar, trees->xbar, (size_t)N * 8);
  }
  memcpy(hb.data() + o_f, forest_tree_idx, (size_t)n_forests * m * 4);
  uint8_t*& db = pk->db;
  HIPCHK(hipMalloc((void**)&db, bytes));
  hipError_t e = hipMemcpyAsync(db, hb.data(), bytes, hipMemcpyHostToDevice, sm);
  if (e != hipSuccess) return fail_hip(e, "hipMemcpyAsync");
  PredTrees& T = pk->T;
  T.node = (const PNode*)db;
  T.value = (const double*)(db + o_val);
  T.slope = lin ? (const double*)(db + o_slope) : nullptr;
  T.xbar = lin ? (const double*)(db + o_xbar) : nullptr;
  T.fnode = (const FNode*)(db + o_fn);
  T.root = (const int2*)(db + o_root);
  T.svar = lin ? (const int32_t*)(db + o_svar) : nullptr;
  pk->fidx = (const int32_t*)(db + o_f);
  pk->cont = cont;
  return PGB_OK;
}

// PGB_WALK_TIMING=1 (environment, read per call): the walk kernel of pgb_predict / pgb_predict_ice alone, between two
// HIP events on the call's stream; pgb_walk_kernel_ms (include/pgbart_ice.h) reports the last one of the calling
// thread (tools/ice_timing.py).  Unset: no event is created.
static thread_local double g_walk_ms = -1.0;
struct WalkTimer {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t sm;
  explicit WalkTimer(hipStream_t s) : sm(s) {
    const char* ev = getenv("PGB_WALK_TIMING");
    if (!ev || atoi(ev) <= 0) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, sm) != hipSuccess) {
      (void)hipGetLastError();
      drop();
    }
  }
  void launched() {
    if (a && hipEventRecord(b, sm) != hipSuccess) drop();
  }
  void synced() {  // (after the stream has been synchronised)
    float ms = 0.f;
    if (a && hipEventElapsedTime(&ms, a, b) == hipSuccess) g_walk_ms = (double)ms;
  }
  void drop() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    a = b = nullptr;
  }
  ~WalkTimer() { drop(); }
};
extern "C" int pgb_walk_kernel_ms(double* ms_out) {
  if (!ms_out) return fail(PGB_E_INVALID, "null argument");
  *ms_out = g_walk_ms;
  return PGB_OK;
}

// The end of every walk call, after its last launch (`e`: hipGetLastError() of the launches): the timer's closing
// event, the synchronisation, the kernel time into *ms_slot (nullptr: none kept; -1.0 when nothing was timed) and the
// two ways a walk can fail, named after `kernel`.  `first` / `first_slot`: a timer that was closed earlier in the call
// (pgb_predict_pdp: the walk before the lookup), read before `wt`.
static int finish_walk(hipError_t e, hipStream_t sm, WalkTimer& wt, double* ms_slot, const char* kernel,
                       WalkTimer* first = nullptr, double* first_slot = nullptr) {
  wt.launched();
  const hipError_t e2 = hipStreamSynchronize(sm);
  const bool ok = e == hipSuccess && e2 == hipSuccess;
  auto read = [ok](WalkTimer& t, double* slot) {
    if (slot) *slot = -1.0;
    if (!ok || !t.a) return;
    t.synced();
    if (slot) *slot = g_walk_ms;
  };
  if (first) read(*first, first_slot);
  read(wt, ms_slot);
  if (e != hipSuccess) {
    char what[64];
    snprintf(what, sizeof what, "%s launch", kernel);
    return fail_hip(e, what);
  }
  if (e2 != hipSuccess) return fail_hip(e2, kernel);
  return PGB_OK;
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{} [, std::bool_constant<b2>{}]): run-time flags as the template
// arguments of a launch, `k<L(), C()>` inside a generic lambda -- every instance from one spelling of its arguments
template <class F>
static void dispatch_bools(bool b0, bool b1, F f) {
  if (b0) {
    if (b1) f(std::true_type{}, std::true_type{});
    else f(std::true_type{}, std::false_type{});
  } else {
    if (b1) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
  }
}
template <class F>
static void dispatch_bools(bool b0, bool b1, bool b2, F f) {
  if (b2) dispatch_bools(b0, b1, [&](auto B0, auto B1) { f(B0, B1, std::true_type{}); });
  else dispatch_bools(b0, b1, [&](auto B0, auto B1) { f(B0, B1, std::false_type{}); });
}

extern "C" int pgb_predict(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests,
                           int32_t m, const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx,
                           const int32_t* excluded_host, int32_t n_excluded,
                           double* out_dev, void* stream) {
  if (!trees || !forest_tree_idx || !X_dev || !out_dev) return fail(PGB_E_INVALID, "null argument");
  if (ldx < p) return fail(PGB_E_INVALID, "pgb_predict: ldx must be >= p");  // (rows that overlap: never a layout)
  if (trees->n_outputs < 1 || trees->n_outputs > PGB_MAX_OUTPUTS) return fail(PGB_E_INVALID, "n_outputs");
  if (n_forests < 1 || n_rows < 1) return PGB_OK;
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;
  hipStream_t sm = (hipStream_t)stream;
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, excluded_host, n_excluded, sm, &pk);
  if (rc != PGB_OK) return rc;
  const int K = trees->n_outputs;
  const PredTrees T = pk.T;
  // one wave per workgroup; enough workgroups to fill the chip, each looping over its share of forests
  const long long gx = (n_rows + PRED_BT - 1) / PRED_BT;
  long long want_wgs = p <= PRED_LDS_MAXP ? 16384 : 4096;  // measured at cfg2 (32 forests x 100k rows): 10.0 vs 11.7 ms
  if (const char* ev = getenv("PGB_PRED_WGS")) want_wgs = atoll(ev) > 0 ? atoll(ev) : want_wgs;
  long long gy = (want_wgs + gx - 1) / gx;
  if (gy > n_forests) gy = n_forests;
  if (gy < 1) gy = 1;
  dim3 grid((unsigned)gx, (unsigned)gy);
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  WalkTimer wt(sm);
  dispatch_bools(ldsx, pk.cont, [&](auto L, auto C) {
    hipLaunchKernelGGL((k_predict<L(), C()>), grid, dim3(PRED_BT), lds, sm, T, pk.fidx, n_forests, m, K, (int)p, X_dev,
                       (long long)n_rows, (long long)ldx, out_dev);
  });
  return finish_walk(hipGetLastError(), sm, wt, nullptr, "k_predict");
}

