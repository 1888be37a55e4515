// pgb_host.h -- part of pgbart_hip.hip (not a standalone header): host side: handles, the C ABI of include/pgbart.h, slot enqueueing.
// ------------------------------------------------------------------ host side
enum { PK_CTRL = 0, PK_ROWS = 1, PK_LL = 2, PK_COUNT = 3 };
static std::atomic<int> g_live_handles{0};  // samplers alive in this process (see feed_until_flag)
static thread_local char g_err[512];
static int fail(int code, const char* msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return code;
}
static int fail_hip(hipError_t e, const char* what) {
  snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
  return PGB_E_DEVICE;
}
#define HIPCHK(expr)                                     \
  do {                                                   \
    hipError_t e_ = (expr);                              \
    if (e_ != hipSuccess) return fail_hip(e_, #expr);    \
  } while (0)

// one device buffer of a call, released on every way out
struct DevBuf {
  uint8_t* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// The kernels of a slot besides the likelihood pass, chosen once per data set (select_slot_kernels): the instance of
// k_ctrl with its workgroup count and the instance of the row pass (k_rows<...> and k_rows_mk<...> take the same
// arguments).  ctrl == nullptr: not chosen yet -- the first enqueue_slots after pgb_create, or after a pgb_set_data
// that changed use_keys or has_subset, fills it in.
typedef void (*ctrl_kernel_t)(const Dev*, int, int, Ctrl*, const InitAcc*, const Job*, const Acc*, const DPart*, const uint16_t*);
typedef void (*rows_kernel_t)(const Dev*, int, const Cmd*, const Job*);
typedef void (*ll_kernel_t)(const Dev*, int, int, const Cmd*, const Ctrl*, const Job*, const Acc*, const InitAcc*);
struct SlotKernels {
  ctrl_kernel_t ctrl = nullptr;
  int ctrl_wgs = 0;  // P - 1, or P: + the workgroup that builds the label tables ahead
  rows_kernel_t rows = nullptr;
  int rows_cap = 0;  // workgroups the row pass keeps resident (enqueue_slots; K-vector instances only, else rows_grid)
};

struct pgb_handle {
  pgb_settings s;
  Dev d;
  Dev* d_dev;                          // device-resident copy passed to every kernel
  volatile unsigned long long* flag;   // pinned host word written by k_ctrl (completed asteps)
  long long steps_target;              // asteps requested so far
  hipStream_t stream;
  hipStream_t stream_out;              // pgb_step_host: the step's results leave on this stream, past the idle slots
  std::vector<void*> allocs;
  std::vector<size_t> alloc_bytes;     // per allocation: payload size ...
  std::vector<char> alloc_owned;       // ... and whether it is a hipMalloc of its own (else a piece of `slab`)
  void* slab;                          // small records share one allocation (see dalloc_bytes)
  size_t slab_used;
  long long slot;  // next slot index (parity = slot & 1)
  int st_cur, alpha_cur;  // mirrors of Ctrl::st_cur / alpha_cur at the last idle point
  int have_data, have_y;
  int has_subset;  // any SubsetSplit column: selects the row-pass instance
  int rows_grid = 1024;  // workgroups of the persistent row-pass grid (dispatch costs ~3.5 ns each)
  int ll_grid;     // ... of the log-likelihood pass
  // 16-bit order keys: decided by pgb_set_data alone, for the data it was last given.  This one flag picks the KEYS
  // instance of k_ctrl and the F32 instance of the row pass TOGETHER (they disagree on the stride of the chunk-count
  // rows otherwise); d.XK16 is xk16_buf while it is set and null while it is not
  int use_keys;
  uint16_t* xk16_buf;  // [p][n_pad], allocated by the first pgb_set_data that wants keys, kept until pgb_destroy
  SlotKernels slot_k;
  ll_kernel_t ll_kernel;  // the instance of k_loglik this sampler launches (family / outputs / response)
  int sigma_dirty = 1;
  double inv_sigma2 = 1.0;
  double lik_param2 = 1.0;
  int lower_host;      // mirror of the batch cursor
  int last_lower, last_n;
  double slots_per_step;  // running estimate of the working slots one astep needs ...
  double slots_var;       // ... and of their variance
  pgb_counters ctr;
  // profiling: events attached to the dispatches of a region, per kernel (PK_*); the row pass is
  // the dominant kernel pgb_profile reports
  int prof;
  std::vector<hipEvent_t> ev[PK_COUNT];
  size_t ev_used[PK_COUNT];
  double prof_ms[PK_COUNT];
  long long prof_launches[PK_COUNT];
  int prof_wgs[PK_COUNT];
  // host-facing results of the last pgb_step_host (mapped pinned block written by k_export_step)
  unsigned char* out_host;   // host address
  unsigned char* out_dev;    // the same block as the device sees it
  StepOutLayout out_layout;
  double* st_dense;          // [K][n] staging of sum_trees in HBM
  int out_valid;             // the block holds the trees of the last step (pgb_export_trees(0) reads it)
  int poisoned;              // a step was abandoned half-way (callback error, stuck state machine): the device
                             // state is undefined until pgb_checkpoint_load restores an idle image
  // pgb_step_async: a worker thread feeds the state machine while the caller goes on
  // callback family: the host evaluates the per-row log-likelihood once per slot
  pgb_loglik_fn cb_fn;
  void* cb_ctx;
  // compiled family (pgb_compiled_host.h): the loaded code object, its kernel (and probe), the params of the next
  // launches (by value) and the aux column ([n_pad], zero unless pgb_set_loglik_aux set it)
  hipModule_t cl_module;
  hipFunction_t cl_fn;
  hipFunction_t cl_probe;
  int cl_nparams = -1;
  pgb_compiled_params cl_prm;
  double* cl_aux;
  std::vector<double> y_host, off_host;
  std::vector<int32_t> rules_host;  // the PGB_RULE_* of the columns: every exported split node carries its own
  int device;
  std::thread worker;
  int job_running, job_rc;
  char job_err[512];
  long long* prof_buf;    // device-clock stamps (allocated on first use)
  long long prof_slot0;   // first slot of the profiled region (device-clock stamps)
  double prof_clock_ms;   // sum over launches of max(end) - min(start), 100 MHz device clock
  long long prof_clock_launches;
};

// A running pgb_step_async job owns the handle: every other entry point waits for it first.
static int join_async(pgb_handle* h) {
  if (h->worker.joinable()) h->worker.join();
  if (h->job_running) {
    h->job_running = 0;
    if (h->job_rc != PGB_OK) {
      const int rc = h->job_rc;
      h->job_rc = PGB_OK;
      return fail(rc, h->job_err);
    }
  }
  return PGB_OK;
}
#define JOIN_ASYNC(h)                          \
  do {                                         \
    int rcj_ = join_async(h);                  \
    if (rcj_ != PGB_OK) return rcj_;           \
  } while (0)
// Entry points that run or read the chain refuse a poisoned handle (see pgb_handle::poisoned).
#define REFUSE_POISONED(h)                                                                                  \
  do {                                                                                                      \
    if ((h)->poisoned)                                                                                      \
      return fail(PGB_E_STATE, "an earlier step of this sampler was abandoned half-way (log-likelihood "    \
                               "callback error or stuck state machine): its state is undefined; restore a " \
                               "checkpoint (pgb_checkpoint_load) or create a new sampler");                 \
  } while (0)

// Device allocations.  The small records every slot touches first (control words, commands, job records,
// split statistics, counters, split weights ...) are carved out of ONE slab: a dozen separate hipMallocs put
// each of them on a page of its own, and the first loads of every (latency-bound) control kernel then paid a
// TLB miss each -- most of the ~1.7 us a fresh kernel waited for its first data.
#define SLAB_BYTES ((size_t)2 << 20)
#define SLAB_ITEM_MAX ((size_t)192 << 10)
static int dalloc_bytes(pgb_handle* h, void** p, size_t bytes) {
  static const bool use_slab = !(getenv("PGB_NO_SLAB") && atoi(getenv("PGB_NO_SLAB")));
  void* q = nullptr;
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (use_slab && need <= SLAB_ITEM_MAX) {
    if (!h->slab) {
      hipError_t e = hipMalloc(&h->slab, SLAB_BYTES);
      if (e != hipSuccess) return fail_hip(e, "hipMalloc");
      h->slab_used = 0;
    }
    if (h->slab_used + need <= SLAB_BYTES) {
      q = (char*)h->slab + h->slab_used;
      h->slab_used += need;
      h->alloc_owned.push_back(0);
    }
  }
  if (!q) {
    hipError_t e = hipMalloc(&q, bytes + 256);
    if (e != hipSuccess) return fail_hip(e, "hipMalloc");
    h->alloc_owned.push_back(1);
  }
  h->allocs.push_back(q);
  h->alloc_bytes.push_back(bytes);
  *p = q;
  return PGB_OK;
}
template <typename T>
static int dalloc(pgb_handle* h, T** p, size_t count) {
  void* q = nullptr;
  const int rc = dalloc_bytes(h, &q, count * sizeof(T));
  if (rc == PGB_OK) *p = (T*)q;
  return rc;
}

// One buffer of the sampler: allocated (in call order: the slab's layout), stored in its member of the handle or of
// Dev -- const-qualified ones included -- and given its initial contents on the sampler's stream, all from ONE count.
enum FillKind { FILL_NONE, FILL_ZERO, FILL_BYTE, FILL_F64, FILL_LINP };
template <typename T>
static int dbuf(pgb_handle* h, T** dst, size_t count, FillKind kind = FILL_NONE, double v = 0.0) {
  typedef typename std::remove_const<T>::type U;
  U* q = nullptr;
  const int rc = dalloc(h, &q, count);
  if (rc != PGB_OK) return rc;
  *dst = q;
  const dim3 grid((unsigned)((count + 255) / 256));
  hipError_t e = hipSuccess;
  if (kind == FILL_ZERO || kind == FILL_BYTE) e = hipMemsetAsync(q, kind == FILL_BYTE ? (int)v : 0, count * sizeof(U), h->stream);
  if constexpr (std::is_same<U, double>::value)
    if (kind == FILL_F64) hipLaunchKernelGGL(k_fill_f64, grid, dim3(256), 0, h->stream, q, (long long)count, v);
  if constexpr (std::is_same<U, LinP>::value)
    if (kind == FILL_LINP) hipLaunchKernelGGL(k_init_linp, grid, dim3(256), 0, h->stream, q, (long long)count);
  return e == hipSuccess ? PGB_OK : fail_hip(e, "hipMemsetAsync");
}

// The likelihood pass is a persistent grid too, and its instances differ a lot in registers (probit 88
// VGPRs, K = 4 softmax 154): the grid is what the chosen instance can keep resident -- 5 workgroups per
// CU for probit, 3 for K = 4 -- so that no workgroup waits for another to finish; the pass aims for at
// least as many work items.  (cfg4: 1024 -> 1280 workgroups, k_loglik 40.3 -> 37.5 us.)
// per_cu: what the occupancy query answered for the instance -- a built-in one (pgb_create) or the loaded module
// kernel (pgb_set_loglik_code; its linear pass is the run-time-K path: what stays resident).
static void size_ll_grid(pgb_handle* h, int per_cu) {
  int cus = 0;
  if (getenv("PGB_LL_GRID") || per_cu <= 0) return;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus <= 0) return;
  // (K = 2, 3, 4 with constant leaves: the instances are compiled for PGB_LLK_WGS workgroups per CU and measured best
  //  there -- cfg5: 768 workgroups 27.2-27.9 us, 1024 28.1-31.2 us, 1280 30.5-31.0 us -- whatever else would fit)
  if (h->d.K >= 2 && h->d.K <= 4 && h->d.response == PGB_RESPONSE_CONSTANT && per_cu > PGB_LLK_WGS) per_cu = PGB_LLK_WGS;
  long long g = (long long)per_cu * cus;
  if (g < 256) g = 256;
  if (g > 2048) g = 2048;
  h->ll_grid = (int)g;
  if (!getenv("PGB_LL_TARGET")) h->d.ll_target = h->ll_grid > 1024 ? h->ll_grid : 1024;
}

extern "C" const char* pgb_last_error(void) { return g_err; }
extern "C" const char* pgb_backend_name(void) { return "hip-gfx950"; }
extern "C" int32_t pgb_max_particles(void) { return PGB_MAX_PARTICLES; }
extern "C" int32_t pgb_abi_version(void) { return PGB_ABI_VERSION; }

// The instance of k_loglik a sampler launches, chosen once: per number of outputs (loops unrolled for
// K = 2, 3, 4), per family for single-output constant leaves (one family's code per instance).
static ll_kernel_t select_ll_kernel(int K, bool lin, int family) {
  if (family == PGB_FAMILY_COMPILED) return nullptr;  // (a module kernel for any K: pgb_set_loglik_code)
  if (K > 1 && lin) return k_loglik<0, -1, true>;
  if (K > 1) {  // constant K-vector leaves: softmax (factorised evaluation, any K) or Normal mean / scale (K = 2)
    if (family != PGB_FAMILY_CATEGORICAL) return k_loglik<2, PGB_FAMILY_NORMAL_MEANSCALE, false>;
    switch (K) {
      case 2: return k_loglik<2, PGB_FAMILY_CATEGORICAL, false>;
      case 3: return k_loglik<3, PGB_FAMILY_CATEGORICAL, false>;
      case 4: return k_loglik<4, PGB_FAMILY_CATEGORICAL, false>;
      default: return k_loglik<0, PGB_FAMILY_CATEGORICAL, false>;
    }
  }
  if (lin) return k_loglik<1, -1, true>;  // linear leaves: one instance, family read at run time
  switch (family) {
    case PGB_FAMILY_BERNOULLI_PROBIT: return k_loglik<1, PGB_FAMILY_BERNOULLI_PROBIT, false>;
    case PGB_FAMILY_BERNOULLI_LOGIT: return k_loglik<1, PGB_FAMILY_BERNOULLI_LOGIT, false>;
    case PGB_FAMILY_POISSON_LOG: return k_loglik<1, PGB_FAMILY_POISSON_LOG, false>;
    case PGB_FAMILY_NEGBIN_LOG: return k_loglik<1, PGB_FAMILY_NEGBIN_LOG, false>;
    case PGB_FAMILY_ASYMLAPLACE: return k_loglik<1, PGB_FAMILY_ASYMLAPLACE, false>;
    case PGB_FAMILY_GAMMA_LOG: return k_loglik<1, PGB_FAMILY_GAMMA_LOG, false>;
    case PGB_FAMILY_CALLBACK: return k_loglik<1, PGB_FAMILY_CALLBACK, false>;
    default: return k_loglik<1, PGB_FAMILY_STUDENT_T, false>;
  }
}

#define PGB_STR2(x) #x
#define PGB_STR(x) PGB_STR2(x)
extern "C" int pgb_create(const pgb_settings* s, void* stream, pgb_handle** out) {
  if (!s || !out) return fail(PGB_E_INVALID, "null argument");
  if (s->n < 1 || s->p < 1 || s->m < 1) return fail(PGB_E_INVALID, "n, p, m must be >= 1");
  if (s->n >= (1ll << 31) - CH) return fail(PGB_E_UNSUPPORTED, "n too large");
  if (s->num_particles < 2 || s->num_particles > PGB_MAX_PARTICLES)
    return fail(PGB_E_INVALID, PGB_MAX_PARTICLES == 64
                                   ? "num_particles must be in [2, 64] (libpgbart_hip_p128.so takes up to 128)"
                                   : "num_particles must be in [2, 128]");
  if (s->family == PGB_FAMILY_CATEGORICAL) {
    if (s->n_outputs < 2 || s->n_outputs > PGB_MAX_OUTPUTS)
      return fail(PGB_E_INVALID, "CATEGORICAL needs 2 <= n_outputs <= " PGB_STR(PGB_MAX_OUTPUTS));
  } else if (s->family == PGB_FAMILY_NORMAL_MEANSCALE) {
    if (s->n_outputs != 2) return fail(PGB_E_INVALID, "NORMAL_MEANSCALE needs n_outputs == 2");
  } else if (s->family == PGB_FAMILY_COMPILED) {  // a body of K = n_outputs predictors (k_loglik_compiled.hip)
    if (s->n_outputs < 1 || s->n_outputs > PGB_MAX_OUTPUTS)
      return fail(PGB_E_INVALID, "COMPILED needs 1 <= n_outputs <= " PGB_STR(PGB_MAX_OUTPUTS));
    // (any response: the code object is the constant or the linear pass, pgb_set_loglik_code checks which)
  } else if (s->family == PGB_FAMILY_NORMAL || s->family == PGB_FAMILY_BERNOULLI_PROBIT ||
             s->family == PGB_FAMILY_BERNOULLI_LOGIT || s->family == PGB_FAMILY_POISSON_LOG ||
             s->family == PGB_FAMILY_NEGBIN_LOG || s->family == PGB_FAMILY_ASYMLAPLACE ||
             s->family == PGB_FAMILY_STUDENT_T || s->family == PGB_FAMILY_GAMMA_LOG ||
             s->family == PGB_FAMILY_CALLBACK) {
    if (s->n_outputs != 1) return fail(PGB_E_INVALID, "this family has a single output");
    if (s->family == PGB_FAMILY_CALLBACK && s->response != PGB_RESPONSE_CONSTANT)
      return fail(PGB_E_UNSUPPORTED, "the callback family has constant leaves");
  } else {
    return fail(PGB_E_UNSUPPORTED, "unknown family");
  }
  if (s->batch_tune < 1 || s->batch_draw < 1) return fail(PGB_E_INVALID, "batch sizes must be >= 1");
  if (s->compat & ~PGB_COMPAT_ALL) return fail(PGB_E_INVALID, "unknown compat bits (pgbart_spec.h: PGB_COMPAT_*)");
  if (s->range_exp < PGB_MIN_RANGE_EXP || s->range_exp > PGB_MAX_RANGE_EXP) {  // (the scales are built from its bits: pgb_pow2)
    char msg[160];
    snprintf(msg, sizeof msg, "range_exp = %d is outside [%d, %d] (PGB_MIN_RANGE_EXP, PGB_MAX_RANGE_EXP: the fixed-point scales must be normal doubles)",
             (int)s->range_exp, PGB_MIN_RANGE_EXP, PGB_MAX_RANGE_EXP);
    return fail(PGB_E_INVALID, msg);
  }
  if (s->response != PGB_RESPONSE_CONSTANT) {
    if (s->response != PGB_RESPONSE_LINEAR && s->response != PGB_RESPONSE_MIX)
      return fail(PGB_E_UNSUPPORTED, "unknown response");
  }
  int ndev = 0;
  hipError_t e0 = hipGetDeviceCount(&ndev);
  if (e0 != hipSuccess || ndev < 1) {
    snprintf(g_err, sizeof g_err, "no HIP device visible (%s, count %d); this backend has no CPU fallback",
             hipGetErrorString(e0), ndev);
    return PGB_E_DEVICE;
  }
  pgb_handle* h = new pgb_handle();  // (value-initialised: zero but for the defaults the struct states)
  g_live_handles.fetch_add(1);
  h->s = *s;
  h->stream = (hipStream_t)stream;
  (void)hipGetDevice(&h->device);
  if (const char* e = getenv("PGB_ROWS_GRID")) h->rows_grid = atoi(e) > 0 ? atoi(e) : h->rows_grid;
  h->ll_grid = h->rows_grid;
  if (const char* e = getenv("PGB_LL_GRID")) h->ll_grid = atoi(e) > 0 ? atoi(e) : h->ll_grid;
  Dev& d = h->d;
  d.n = s->n;
  d.nchunks = (int)((s->n + CH - 1) / CH);
  d.n_pad = (long long)d.nchunks * CH;
  d.cc_stride = (d.nchunks + 7) & ~7;
  // PGB_FOLD_LAST (default 1; 0 = off): a slot whose proposed SMC round is empty and final ends the tree itself instead
  // of leaving that to the next slot (k_ctrl, single-output constant-leaf models).  Results are identical either way;
  // only pgb_counters.slots differs, by one per tree update that folds.  Read here, per handle, so that two samplers
  // of one process can run the two paths side by side.
  d.fold_last = 1;
  if (const char* e = getenv("PGB_FOLD_LAST")) d.fold_last = atoi(e) != 0 ? 1 : 0;
  d.p = s->p;
  d.m = s->m;
  d.P = s->num_particles;
  d.family = s->family;
  d.K = s->n_outputs;
  d.response = s->response;
  d.lin_R = pgb_pow2(s->range_exp - 1);
  d.inv_R = pgb_pow2(1 - s->range_exp);
  d.rows_target = ROWS_TARGET_ITEMS;
  d.rows_target_init = ROWS_TARGET_ITEMS_INIT;
  if (const char* e = getenv("PGB_ROWS_TARGET")) d.rows_target = atoi(e) > 0 ? atoi(e) : d.rows_target;
  d.ll_target = d.rows_target;
  d.compat = s->compat;
  if (const char* e = getenv("PGB_LL_TARGET")) d.ll_target = atoi(e) > 0 ? atoi(e) : d.ll_target;
  h->ll_kernel = select_ll_kernel(d.K, d.response != PGB_RESPONSE_CONSTANT, d.family);
  if (d.family != PGB_FAMILY_NORMAL && h->ll_kernel) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)h->ll_kernel, BT, 0) == hipSuccess) size_ll_grid(h, per_cu);
  }
  if (const char* e = getenv("PGB_ROWS_TARGET_INIT")) d.rows_target_init = atoi(e) > 0 ? atoi(e) : d.rows_target_init;
  // One launch per SMC round where the round is latency-bound: Normal likelihood, one output, constant
  // leaves, and few enough (particle, chunk) pairs that a work item holds <= GMAXF particles.
  d.batch_tune = s->batch_tune;
  d.batch_draw = s->batch_draw;
  d.seed = s->seed;
  d.init_leaf = s->init_leaf;
  d.mdouble = (double)s->m;
  d.sc = pgb_make_scales(s->n, s->range_exp);
  int rc;
  const int K = d.K, KX = d.K - 1;
  const size_t n_pad = (size_t)d.n_pad, PN = (size_t)2 * MAXP * MAXN, MN = (size_t)d.m * MAXN, LV = 2 * 2 * 256;
  // BUF(member, count [, fill [, value]]): one statement per buffer (dbuf); no fill = left as allocated
#define BUF(...) \
  if ((rc = dbuf(h, __VA_ARGS__)) != PGB_OK) { pgb_destroy(h); return rc; }
  BUF(&d.XT, (size_t)d.p * n_pad);
  BUF(&d.y, n_pad, FILL_ZERO);
  BUF(&d.off, K * n_pad, FILL_ZERO);
  BUF(&d.st, 2 * K * n_pad, FILL_F64, s->init_sum);
  BUF(&d.pack, n_pad, FILL_ZERO);
  BUF(&d.rs_mean, K * n_pad, FILL_ZERO);
  BUF(&d.rs_m2, K * n_pad, FILL_ZERO);
  if (KX > 0) {  // K-vector leaves: extension outputs
    BUF(&d.packx, KX * n_pad, FILL_ZERO);
    BUF(&d.pvx, PN * KX, FILL_ZERO);
    BUF(&d.pqx, PN * KX, FILL_ZERO);
    BUF(&d.tvx, MN * KX, FILL_F64, s->init_leaf);  // every accepted tree starts as a stump whose K-vector leaf is init_leaf
    BUF(&d.accx, (size_t)2 * MAXP * AX_PER, FILL_ZERO);
    BUF(&d.iax, (size_t)2 * IA_SLOTS * 2 * KX, FILL_ZERO);
    BUF(&d.lvx, LV * KX, FILL_ZERO);
    BUF(&d.jqx, (size_t)2 * MAXP * KX, FILL_ZERO);
    BUF(&d.jvx, (size_t)2 * MAXP * KX, FILL_ZERO);
    BUF(&d.jzx, (size_t)2 * MAXP * KX * 2, FILL_ZERO);
    BUF(&d.lsdx, (size_t)2 * KXMAX, FILL_F64, s->init_leaf_sd);
    BUF(&d.finx, (size_t)2 * MAXP * KX, FILL_ZERO);
    if (s->family == PGB_FAMILY_CATEGORICAL && s->response == PGB_RESPONSE_CONSTANT) {
      // the row part of the factorised softmax: scratch of one tree update (no checkpoint carries it)
      // (zeroed once here: the passes of a tree's later rounds read the padded rows of the last chunk as well, which
      //  the pass that starts the tree never writes)
      BUF(&d.cat_e, K * n_pad, FILL_ZERO);
      BUF(&d.cat_a, n_pad, FILL_ZERO);
      BUF(&d.cat_c, n_pad, FILL_ZERO);
    }
  }
  BUF(&d.tree_lid, d.m * n_pad);  // (k_init_tree_lid below)
  BUF(&d.lid, (size_t)NGEN * MAXP * n_pad, FILL_BYTE, PGB_ORPHAN);
  BUF(&d.cc, (size_t)CC_ROUNDS * MAXP * 2 * d.cc_stride, FILL_ZERO);
  if (s->family == PGB_FAMILY_CALLBACK) {
    BUF(&d.cb_mu, MAXP * n_pad);
    BUF(&d.cb_side, MAXP * n_pad);
    h->y_host.assign((size_t)d.n, 0.0);
    h->off_host.assign((size_t)d.n, 0.0);
  }
  if (s->family == PGB_FAMILY_COMPILED) BUF(&h->cl_aux, n_pad, FILL_ZERO);
  BUF(&d.trees, d.m);  // (k_init_trees below)
  BUF(&d.parts, 2 * MAXP, FILL_ZERO);
  BUF(&d.jobs, 2 * MAXP, FILL_ZERO);
  BUF(&d.acc, 2 * MAXP * ACC_PER, FILL_ZERO);
  BUF(&d.accl, 2 * MAXP * LL_PER, FILL_ZERO);
  BUF(&d.jobl, 2 * MAXP, FILL_ZERO);
  BUF(&d.initacc, 2 * IA_SLOTS, FILL_ZERO);
  BUF(&d.cmd, 2, FILL_ZERO);
  BUF(&d.ctrl, 2);  // (the idle control word below)
  BUF(&d.counters, 8, FILL_ZERO);
  BUF(&d.vi, d.p, FILL_ZERO);
  BUF(&d.alpha, 2 * d.p);
  BUF(&d.cdfS, 2 * d.p);
  BUF(&d.prior_leaf, PGB_MAX_DEPTH);  // (copied from the settings below)
  BUF(&d.rules, d.p);
  BUF(&d.col_nan, d.p, FILL_ZERO);
  BUF(&d.col_ex, d.p, FILL_ZERO);
  if (d.response != PGB_RESPONSE_CONSTANT) {
    BUF(&d.plin, PN, FILL_LINP);
    BUF(&d.tlin, MN, FILL_LINP);
    BUF(&d.lvl, LV, FILL_LINP);
    BUF(&d.accu, (size_t)2 * MAXP * ACC_PER, FILL_ZERO);
    if (KX > 0) {
      BUF(&d.psx, PN * KX, FILL_ZERO);
      BUF(&d.tsx, MN * KX, FILL_ZERO);
      BUF(&d.lsx, LV * KX, FILL_ZERO);
      BUF(&d.accux, (size_t)2 * MAXP * AX_PER, FILL_ZERO);
    }
  }
  hipStream_t sm = h->stream;
  hipError_t e;
#define HC(expr) \
  if ((e = (expr)) != hipSuccess) { int r_ = fail_hip(e, #expr); pgb_destroy(h); return r_; }
  {
    void* hp = nullptr;
    HC(hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent));
    h->flag = (volatile unsigned long long*)hp;
    h->flag[0] = 0;  // asteps whose last tree has been accepted (its FINAL row pass may still be running)
    h->flag[1] = 0;  // asteps that are complete on the device (published by the first idle slot after them)
    h->flag[2] = 0;  // slots whose control kernel has started (the credit the host enqueues against)
    h->flag[4] = 0;  // set by k_nonfinite (pgb_set_response / pgb_set_offset)
    // (h->stream_out: see pgb_set_output_stream)
    void* dp = nullptr;
    HC(hipHostGetDevicePointer(&dp, hp, 0));
    d.host_flag = (unsigned long long*)dp;
#ifdef PGB_TRACE
    BUF(&d.trace, (size_t)TRACE_SLOTS * TRACE_W, FILL_ZERO);
#endif
    {  // host-facing results of pgb_step_host: mapped pinned block + dense sum_trees staging
      int cap_trees = s->batch_tune > s->batch_draw ? s->batch_tune : s->batch_draw;
      if (cap_trees > s->m) cap_trees = s->m;
      h->out_layout = stepout_layout(d.p, cap_trees, d.K, d.response != PGB_RESPONSE_CONSTANT);
      void* hp2 = nullptr;
      HC(hipHostMalloc(&hp2, (size_t)h->out_layout.bytes, hipHostMallocMapped | hipHostMallocCoherent));
      memset(hp2, 0, (size_t)h->out_layout.bytes);
      h->out_host = (unsigned char*)hp2;
      void* dp2 = nullptr;
      HC(hipHostGetDevicePointer(&dp2, hp2, 0));
      h->out_dev = (unsigned char*)dp2;
      BUF(&h->st_dense, (size_t)d.K * d.n);
    }
    BUF(&h->d_dev, 1);
    HC(hipMemcpyAsync(h->d_dev, &d, sizeof(Dev), hipMemcpyHostToDevice, sm));
  }
#undef BUF
  HC(hipMemcpyAsync((void*)d.prior_leaf, s->prior_leaf, PGB_MAX_DEPTH * sizeof(double), hipMemcpyHostToDevice, sm));
  Ctrl c0;
  memset(&c0, 0, sizeof c0);
  c0.phase = PH_IDLE;
  c0.leaf_sd = s->init_leaf_sd;
  c0.inv_sigma2 = 1.0;
  c0.lik_param2 = 1.0;
  Ctrl cc2[2] = {c0, c0};
  HC(hipMemcpyAsync(d.ctrl, cc2, sizeof cc2, hipMemcpyHostToDevice, sm));
  hipLaunchKernelGGL(k_init_tree_lid, dim3((unsigned)((d.n_pad * d.m + 255) / 256)), dim3(256), 0, sm,
                     d.tree_lid, d.n, d.n_pad, d.m);
  hipLaunchKernelGGL(k_init_trees, dim3((d.m + 63) / 64), dim3(64), 0, sm, d.trees, d.m, d.n,
                     s->init_leaf);
  HC(hipGetLastError());
  HC(hipStreamSynchronize(sm));
#undef HC

  *out = h;
  return PGB_OK;
}

extern "C" int pgb_destroy(pgb_handle* h) {
  if (!h) return PGB_OK;
  if (h->worker.joinable()) h->worker.join();
  // pgb_step_host returns while up to FEED_MIN idle slots are still queued on the sampler's stream (they write
  // the pinned flag words and the control records): nothing below may be freed under them, and torch's
  // streams are non-blocking, so no implicit ordering can be relied on
  (void)hipStreamSynchronize(h->stream);
  if (h->stream_out) (void)hipStreamSynchronize(h->stream_out);
  (void)hipGetLastError();
  for (int k = 0; k < PK_COUNT; ++k)
    for (hipEvent_t e : h->ev[k]) (void)hipEventDestroy(e);
  if (h->flag) (void)hipHostFree((void*)h->flag);
  if (h->out_host) (void)hipHostFree((void*)h->out_host);
  for (size_t i = 0; i < h->allocs.size(); ++i)
    if (h->alloc_owned[i]) (void)hipFree(h->allocs[i]);
  if (h->slab) (void)hipFree(h->slab);
  if (h->cl_module) (void)hipModuleUnload(h->cl_module);
  g_live_handles.fetch_sub(1);
  delete h;
  return PGB_OK;
}

// 16-bit order keys of p columns of a column-major matrix ([p][n_pad] doubles -> [p][n_pad] keys; see k_rows<..., F32>
// and k_key_*): one column at a time -- stage as float32, radix sort, equi-depth boundaries, keys.  Scratch:
// [n] staged | [n] sorted | boundaries | counter | the sort's temporary storage, allocated and freed here.
static hipError_t order_keys_build(const double* XT, long long n, long long n_pad, int p, uint16_t* keys, hipStream_t sm) {
  const size_t nn = (size_t)n;
  size_t tmp_bytes = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (const float*)nullptr, (float*)nullptr, (int)nn, 0, 32, sm);
  if (e != hipSuccess) return e;
  const size_t fl = (2 * nn + PGB_KEY_BOUNDS + 64) * sizeof(float);
  DevBuf scratch;
  e = hipMalloc((void**)&scratch.p, fl + tmp_bytes + 256);
  if (e != hipSuccess) return e;
  float* staged = (float*)scratch.p;
  float* sorted = staged + nn;
  float* bnd = sorted + nn;
  unsigned* miss = (unsigned*)(bnd + PGB_KEY_BOUNDS);
  void* tmp = scratch.p + fl;
  for (int c = 0; c < p && e == hipSuccess; ++c) {
    const double* col = XT + (size_t)c * n_pad;
    e = hipMemsetAsync(miss, 0, sizeof(unsigned), sm);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_key_stage, dim3(1024), dim3(BT), 0, sm, col, staged, n, miss);
    e = hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, (const float*)staged, sorted, (int)nn, 0, 32, sm);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_key_bounds, dim3(256), dim3(BT), 0, sm, (const float*)sorted, n, (const unsigned*)miss, bnd);
    hipLaunchKernelGGL(k_key_assign, dim3(2048), dim3(BT), 0, sm, col, (const float*)bnd, keys + (size_t)c * n_pad, n_pad);
  }
  return e == hipSuccess ? hipStreamSynchronize(sm) : e;
}

extern "C" int pgb_set_data(pgb_handle* h, const double* X_dev, int64_t ldx, const int32_t* rules_host,
                            const double* split_prior_host) {
  if (!h || !X_dev || !rules_host || !split_prior_host) return fail(PGB_E_INVALID, "null argument");
  JOIN_ASYNC(h);
  h->out_valid = 0;
  h->have_data = 0;  // (a call that is refused below has already touched XT, the rules or the keys: no data until one succeeds)
  Dev& d = h->d;
  if (ldx < d.p) return fail(PGB_E_INVALID, "ldx < p");
  double mx = 0.0;
  int has_subset = 0;
  for (int j = 0; j < d.p; ++j) {
    if (rules_host[j] == PGB_RULE_SUBSET) has_subset = 1;
    if (rules_host[j] != PGB_RULE_CONTINUOUS && rules_host[j] != PGB_RULE_ONEHOT &&
        rules_host[j] != PGB_RULE_SUBSET)
      return fail(PGB_E_UNSUPPORTED, "unknown split rule");
    if (!(split_prior_host[j] > 0.0)) return fail(PGB_E_INVALID, "split_prior must be positive");
    if (split_prior_host[j] > mx) mx = split_prior_host[j];
  }
  if (has_subset != h->has_subset) h->slot_k = SlotKernels();  // (another instance of the row pass from here on)
  h->has_subset = has_subset;
  d.max_prior = mx;
  d.alpha_unit = pgb_alpha_unit(mx);
  h->rules_host.assign(rules_host, rules_host + d.p);
  hipStream_t sm = h->stream;
  HIPCHK(hipMemcpyAsync((void*)d.rules, rules_host, d.p * sizeof(int32_t), hipMemcpyHostToDevice, sm));
  // the prior is staged in the (not yet used) running-sd buffer and quantised on the device
  HIPCHK(hipMemcpyAsync(d.rs_mean, split_prior_host, (size_t)(d.p < d.n_pad ? d.p : 0) * sizeof(double),
                        hipMemcpyHostToDevice, sm));
  HIPCHK(hipMemsetAsync((void*)d.col_nan, 0, d.p * sizeof(int32_t), sm));
  dim3 grid((unsigned)(d.n_pad / 32), (unsigned)((d.p + 31) / 32));
  hipLaunchKernelGGL(k_transpose, grid, dim3(BT), 0, sm, X_dev, (long long)ldx, (double*)d.XT, d.n,
                     d.n_pad, d.p, (int32_t*)d.col_nan);
  if (h->has_subset) {  // category codes outside 0 .. 51 are refused, not clamped (include/pgbart.h, Limits)
    DevBuf bad_dev;
    int bad = 0;
    HIPCHK(hipMalloc((void**)&bad_dev.p, sizeof(int)));
    HIPCHK(hipMemsetAsync(bad_dev.p, 0, sizeof(int), sm));
    hipLaunchKernelGGL(k_subset_check, dim3((unsigned)d.p), dim3(BT), 0, sm, d.XT, d.n, d.n_pad, (const int32_t*)d.rules, (int*)bad_dev.p);
    HIPCHK(hipMemcpyAsync(&bad, bad_dev.p, sizeof(int), hipMemcpyDeviceToHost, sm));
    HIPCHK(hipStreamSynchronize(sm));
    if (bad) {
      char msg[160];
      snprintf(msg, sizeof msg, "SubsetSplit column %d: categories must be integer codes in [0, %d) (NaN = missing)", bad - 1,
               PGB_SUBSET_BITS);
      return fail(PGB_E_INVALID, msg);
    }
  }
  // A design matrix that does not fit the 256 MiB Infinity Cache streams from HBM in every row pass: the row pass
  // (single output, K = 2..4) then reads 16-bit order keys of the split column (k_rows<..., F32>: a quarter of the
  // bytes; built here, one column at a time: stage as float32, sort, equi-depth boundaries, keys); smaller matrices
  // stay on the float64 path (cache-resident, latency-bound: keys only add work).
  {
    size_t min_bytes = (size_t)192 << 20;
    if (const char* e = getenv("PGB_X32_MIN_MB")) min_bytes = (size_t)atoll(e) << 20;
    const size_t count = (size_t)d.p * d.n_pad;
    // THE predicate: keys are in use for this data or they are not -- whatever an earlier call decided
    const int use_keys = d.response == PGB_RESPONSE_CONSTANT && !h->has_subset && count * sizeof(double) >= min_bytes;
    if (use_keys != h->use_keys) h->slot_k = SlotKernels();  // (the KEYS / F32 instances, or back, from here on)
    h->use_keys = use_keys;
    d.XK16 = nullptr;  // (the keys of an earlier matrix are ignored; the buffer stays for a later call that wants keys)
    if (use_keys) {
      if (!h->xk16_buf) {
        uint16_t* xk = nullptr;
        int rck = dalloc(h, &xk, count);
        if (rck != PGB_OK) return rck;
        h->xk16_buf = xk;
      }
      hipError_t e = order_keys_build(d.XT, (long long)d.n, (long long)d.n_pad, d.p, h->xk16_buf, sm);
      if (e != hipSuccess) return fail_hip(e, "order keys of the design matrix");
      d.XK16 = h->xk16_buf;
    }
  }
  DevBuf prior_stage;  // (released when the call returns: past the synchronisation below)
  if (d.p >= d.n_pad) {  // more columns than padded rows: stage through a temporary
    HIPCHK(hipMalloc((void**)&prior_stage.p, d.p * sizeof(double)));
    HIPCHK(hipMemcpyAsync(prior_stage.p, split_prior_host, d.p * sizeof(double), hipMemcpyHostToDevice, sm));
  }
  hipLaunchKernelGGL(k_init_alpha, dim3(1), dim3(64), 0, sm, prior_stage.p ? (const double*)prior_stage.p : d.rs_mean, mx,
                     d.alpha, d.cdfS, d.p);
  if (d.response != PGB_RESPONSE_CONSTANT) {  // exponent bound of every column (u = x 2^-ex)
    DevBuf amax_dev;
    HIPCHK(hipMalloc((void**)&amax_dev.p, d.p * sizeof(double)));
    hipLaunchKernelGGL(k_colmax, dim3((unsigned)d.p), dim3(BT), 0, sm, d.XT, d.n, d.n_pad, (double*)amax_dev.p);
    std::vector<double> amax(d.p);
    HIPCHK(hipMemcpyAsync(amax.data(), amax_dev.p, d.p * sizeof(double), hipMemcpyDeviceToHost, sm));
    HIPCHK(hipStreamSynchronize(sm));
    std::vector<int32_t> ex(d.p);
    for (int j = 0; j < d.p; ++j) ex[j] = pgb_col_exponent(amax[j]);
    for (int j = 0; j < d.p; ++j)
      if (ex[j] > PGB_LIN_MAX_EXPONENT) {  // 2^-ex would not be a normal double
        char msg[200];
        snprintf(msg, sizeof msg, "response linear / mix: column %d has max|x| = %g, a regressed column needs max|x| < 2^%d (PGB_LIN_MAX_EXPONENT)",
                 j, amax[j], PGB_LIN_MAX_EXPONENT);
        return fail(PGB_E_INVALID, msg);
      }
    HIPCHK(hipMemcpyAsync((void*)d.col_ex, ex.data(), d.p * sizeof(int32_t), hipMemcpyHostToDevice, sm));
    HIPCHK(hipStreamSynchronize(sm));
  }
  HIPCHK(hipMemsetAsync(d.rs_mean, 0, d.n_pad * sizeof(double), sm));
  HIPCHK(hipMemcpyAsync(h->d_dev, &d, sizeof(Dev), hipMemcpyHostToDevice, sm));  // alpha_unit, max_prior
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(sm));
  h->have_data = 1;
  return PGB_OK;
}

extern "C" int pgb_set_response(pgb_handle* h, const double* y_dev) {
  if (!h || !y_dev) return fail(PGB_E_INVALID, "null argument");
  JOIN_ASYNC(h);
  h->out_valid = 0;
  HIPCHK(hipMemcpyAsync((void*)h->d.y, y_dev, h->d.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (h->s.family == PGB_FAMILY_CALLBACK)
    HIPCHK(hipMemcpyAsync(h->y_host.data(), y_dev, h->d.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  h->flag[4] = 0;
  hipLaunchKernelGGL(k_nonfinite, dim3(256), dim3(BT), 0, h->stream, (const double*)h->d.y, (long long)h->d.n,
                     (long long)h->d.n_pad, 1, __builtin_inf(), h->d.host_flag + 4);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->flag[4]) {
    h->have_y = 0;
    return fail(PGB_E_INVALID, "the response has non-finite values");
  }
  h->have_y = 1;
  return PGB_OK;
}

extern "C" int pgb_set_offset(pgb_handle* h, const double* offset_dev) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  h->out_valid = 0;
  if (h->s.family == PGB_FAMILY_NORMAL)
    return fail(PGB_E_UNSUPPORTED, "offsets are for the per-row families (a Normal model fits observed - offset)");
  if (offset_dev)  // [K][n] -> the padded [K][n_pad] rows
    HIPCHK(hipMemcpy2DAsync((void*)h->d.off, h->d.n_pad * sizeof(double), offset_dev, h->d.n * sizeof(double),
                            h->d.n * sizeof(double), (size_t)h->d.K, hipMemcpyDeviceToDevice, h->stream));
  else
    HIPCHK(hipMemsetAsync((void*)h->d.off, 0, (size_t)h->d.K * h->d.n_pad * sizeof(double), h->stream));
  if (h->s.family == PGB_FAMILY_CALLBACK) {
    if (offset_dev)
      HIPCHK(hipMemcpyAsync(h->off_host.data(), offset_dev, h->d.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    else
      h->off_host.assign((size_t)h->d.n, 0.0);
  }
  if (h->d.has_off != (offset_dev ? 1 : 0)) {
    h->d.has_off = offset_dev ? 1 : 0;
    HIPCHK(hipMemcpyAsync(h->d_dev, &h->d, sizeof(Dev), hipMemcpyHostToDevice, h->stream));
  }
  h->flag[4] = 0;
  if (offset_dev)
    hipLaunchKernelGGL(k_nonfinite, dim3(256), dim3(BT), 0, h->stream, (const double*)h->d.off, (long long)h->d.n,
                       (long long)h->d.n_pad, (int)h->d.K, (double)PGB_MAX_OFFSET, h->d.host_flag + 4);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->flag[4]) {  // (a linear predictor must be finite; the offset is zeroed so that the chain stays usable)
    HIPCHK(hipMemsetAsync((void*)h->d.off, 0, (size_t)h->d.K * h->d.n_pad * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return fail(PGB_E_INVALID, "the offset has non-finite values or values beyond +-1e6 (PGB_MAX_OFFSET)");
  }
  return PGB_OK;
}

static int compiled_set_params(pgb_handle* h, const double* params, int32_t n_params);  // (pgb_compiled_host.h)
extern "C" int pgb_set_likelihood(pgb_handle* h, const double* params, int32_t n_params) {
  if (!h || !params) return fail(PGB_E_INVALID, "null argument");
  JOIN_ASYNC(h);
  if (h->s.family == PGB_FAMILY_NORMAL) {
    if (n_params != 1 || !(params[0] > 0.0)) return fail(PGB_E_INVALID, "NORMAL needs sigma > 0");
    h->inv_sigma2 = 1.0 / (params[0] * params[0]);
    h->sigma_dirty = 1;
  } else if (h->s.family == PGB_FAMILY_NEGBIN_LOG || h->s.family == PGB_FAMILY_GAMMA_LOG) {
    // the slot doubles as "the family's parameter"
    if (n_params != 1 || !(params[0] > 0.0)) return fail(PGB_E_INVALID, "NEGBIN_LOG / GAMMA_LOG need alpha > 0");
    h->inv_sigma2 = params[0];
    h->sigma_dirty = 1;
  } else if (h->s.family == PGB_FAMILY_ASYMLAPLACE) {
    if (n_params != 2 || !(params[0] > 0.0) || !(params[1] > 0.0) || !(params[1] < 1.0))
      return fail(PGB_E_INVALID, "ASYMLAPLACE needs b > 0 and 0 < q < 1");
    h->inv_sigma2 = params[0];
    h->lik_param2 = params[1];
    h->sigma_dirty = 1;
  } else if (h->s.family == PGB_FAMILY_STUDENT_T) {
    if (n_params != 2 || !(params[0] > 0.0) || !(params[1] > 0.0))
      return fail(PGB_E_INVALID, "STUDENT_T needs sigma > 0 and nu > 0");
    h->inv_sigma2 = params[0];
    h->lik_param2 = params[1];
    h->sigma_dirty = 1;
  } else if (h->s.family == PGB_FAMILY_COMPILED) {
    return compiled_set_params(h, params, n_params);
  } else if (n_params != 0) {
    return fail(PGB_E_INVALID, "this family has no parameters");
  }
  return PGB_OK;
}

// Profiling: the events are attached to the dispatch itself (hipExtLaunchKernelGGL), i.e. they carry
// the start / end timestamps of the kernel's own AQL packet -- the interval rocprofv3 reports --
// rather than bracketing the launch with two extra barrier packets.
static int prof_events(pgb_handle* h, int k, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!h->prof) return PGB_OK;
  if (h->ev_used[k] + 2 > h->ev[k].size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)
      return fail(PGB_E_DEVICE, "hipEventCreate");
    h->ev[k].push_back(a);
    h->ev[k].push_back(b);
  }
  *e0 = h->ev[k][h->ev_used[k]];
  *e1 = h->ev[k][h->ev_used[k] + 1];
  h->ev_used[k] += 2;
  return PGB_OK;
}
#define LAUNCH_KT(PK_, KERN, GRID_, THREADS_, ...)                                               \
  do {                                                                                           \
    hipEvent_t e0_, e1_;                                                                         \
    int rc_ = prof_events(h, (PK_), &e0_, &e1_);                                                 \
    if (rc_ != PGB_OK) return rc_;                                                               \
    h->prof_wgs[(PK_)] = (int)(GRID_).x;                                                         \
    if (h->prof) hipExtLaunchKernelGGL((KERN), (GRID_), dim3(THREADS_), 0, h->stream, e0_, e1_, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERN), (GRID_), dim3(THREADS_), 0, h->stream, __VA_ARGS__);          \
  } while (0)
#define LAUNCH_K(PK_, KERN, GRID_, ...) LAUNCH_KT(PK_, KERN, GRID_, BT, __VA_ARGS__)

#include "pgb_compiled_host.h"

// The instances of k_ctrl and of the row pass for a model and its data.  keys (pgb_set_data: constant leaves and no
// SubsetSplit column) picks KEYS of k_ctrl and F32 of the row pass: always chosen together.
static SlotKernels select_slot_kernels(int K, int P, bool lin, bool keys, bool sub, bool nrm) {
  SlotKernels k;
  k.ctrl_wgs = P - 1;
  if (K > 1) {
    // (statements, in this order: the instances are laid out in the code object in the order they are first named,
    //  and k_ctrl is a latency kernel -- moving one to another alignment cost cfg5 0.8 %)
    if (lin) k.ctrl = k_ctrl<true, true>;
    else if (keys) k.ctrl = k_ctrl<true, false, true>;
    else k.ctrl = k_ctrl<true, false>;
    if (lin) k.rows = k_rows_mk<0, true>;  // linear leaves: one instance for any K
    else if (K == 2) k.rows = keys ? k_rows_mk<2, false, true> : k_rows_mk<2, false>;
    else if (K == 3) k.rows = keys ? k_rows_mk<3, false, true> : k_rows_mk<3, false>;
    else if (K == 4) k.rows = keys ? k_rows_mk<4, false, true> : k_rows_mk<4, false>;
    else k.rows = keys ? k_rows_mk<0, false, true> : k_rows_mk<0, false>;
  } else if (lin) {  // (a linear leaf regresses on whatever column its parent split on)
    k.ctrl = k_ctrl<false, true>;
    if (sub) k.rows = nrm ? k_rows<true, true, true> : k_rows<true, false, true>;
    else k.rows = nrm ? k_rows<false, true, true> : k_rows<false, false, true>;
  } else {
    k.ctrl = keys ? k_ctrl<false, false, true> : k_ctrl<false, false>;
    k.ctrl_wgs = P;  // + the workgroup that builds the label tables ahead
    if (sub) k.rows = nrm ? k_rows<true, true, false> : k_rows<true, false, false>;
    else if (keys)  // 16-bit order keys of the split columns (matrix larger than the Infinity Cache)
      k.rows = nrm ? k_rows<false, true, false, true> : k_rows<false, false, false, true>;
    else k.rows = nrm ? k_rows<false, true, false> : k_rows<false, false, false>;
  }
  return k;
}

static int enqueue_slots(pgb_handle* h, int count) {
  Dev& d = h->d;
  SlotKernels& sk = h->slot_k;
  if (!sk.ctrl) {
    sk = select_slot_kernels(d.K, d.P, d.response != PGB_RESPONSE_CONSTANT, h->use_keys != 0, h->has_subset != 0,
                             h->s.family == PGB_FAMILY_NORMAL);
    // the K-vector instances differ in registers (K = 4: 3 workgroups per CU, the run-time-K instance 2-3): a
    // persistent grid larger than what stays resident leaves the surplus workgroups waiting for a first round of
    // items to finish (cfg5, in-kernel stamps: the last quarter of a 1024 grid started 22 us into a 27 us launch)
    int per_cu = 0, cus = 0;
    sk.rows_cap = h->rows_grid;
    if (d.K > 1 && !getenv("PGB_ROWS_GRID") &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)sk.rows, BT, 0) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && per_cu > 0 && cus > 0)
      sk.rows_cap = per_cu * cus < h->rows_grid ? per_cu * cus : h->rows_grid;
  }
  long long want = (long long)d.nchunks * (d.P - 1);
  if (want < d.n_pad / BT) want = d.n_pad / BT;
  if (want > sk.rows_cap) want = sk.rows_cap;
  dim3 gctrl((unsigned)sk.ctrl_wgs), grows((unsigned)want);
  long long wantl = (long long)d.nchunks * (d.P - 1);
  if (wantl > h->ll_grid) wantl = h->ll_grid;
  dim3 gll((unsigned)wantl);
  const Dev* dd = (const Dev*)h->d_dev;
  for (int i = 0; i < count; ++i) {
    int par = (int)(h->slot & 1);
    LAUNCH_K(PK_CTRL, sk.ctrl, gctrl, dd, par, sk.ctrl_wgs, d.ctrl, (const InitAcc*)d.initacc, (const Job*)d.jobs,
             (const Acc*)d.acc, (const DPart*)d.parts, (const uint16_t*)d.XK16);
    LAUNCH_K(PK_ROWS, sk.rows, grows, dd, par, (const Cmd*)d.cmd, (const Job*)d.jobs);
    if (d.family == PGB_FAMILY_COMPILED) {  // (the module kernel of pgb_set_loglik_code)
      const int rc_ = compiled_launch(h, par, (int)gll.x);
      if (rc_ != PGB_OK) return rc_;
    } else if (d.family != PGB_FAMILY_NORMAL)  // per-row log-likelihood of the rows this round re-labelled
      LAUNCH_K(PK_LL, h->ll_kernel, gll, dd, par, (int)gll.x, (const Cmd*)d.cmd, (const Ctrl*)d.ctrl, (const Job*)d.jobs,
               (const Acc*)d.acc, (const InitAcc*)d.initacc);
    h->slot += 1;
  }
  HIPCHK(hipGetLastError());
  return PGB_OK;
}


static int harvest_profile(pgb_handle* h) {
  for (int k = 0; k < PK_COUNT; ++k) {
    for (size_t i = 0; i + 1 < h->ev_used[k]; i += 2) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, h->ev[k][i], h->ev[k][i + 1]));
      h->prof_ms[k] += ms;
      h->prof_launches[k] += 1;
    }
    h->ev_used[k] = 0;
  }
  return PGB_OK;
}

// ---- callback family: the host half of a slot (after {k_ctrl ; k_rows ; k_loglik<callback>} have run)
// k_loglik left, per active particle, every row's side and the linear predictor of the rows of the split
// leaf; the callback evaluates them in ONE call, the values are clamped and quantised like the built-in
// families' and their sums per (particle, side) go where k_loglik would have put them.  A slot that
// starts a tree also needs the log-likelihood of a fresh stump and of the current tree over all rows
// (what the INIT part of k_rows computes for the built-in families).
static int callback_host_phase(pgb_handle* h, int par) {
  Dev& d = h->d;
  const size_t n = (size_t)d.n;
  struct CmdHead { int32_t kind, tree_old, tree_new, sel_gen, sel_slot, tune, dst_gen, st_cur; } ch;
  HIPCHK(hipMemcpy(&ch, &d.cmd[par], sizeof ch, hipMemcpyDeviceToHost));
  if (!(ch.kind & CMD_PARTITION)) return PGB_OK;
  std::vector<Job> jobs(MAXP);
  HIPCHK(hipMemcpy(jobs.data(), d.jobs + (size_t)par * MAXP, sizeof(Job) * MAXP, hipMemcpyDeviceToHost));
  std::vector<double> yy, mm, out;
  std::vector<int64_t> rows;
  std::vector<int> owner;  // (particle << 2) | side of every gathered row
  std::vector<uint8_t> side(n);
  std::vector<double> mu(n);
  for (int p = 1; p < d.P; ++p) {
    if (!jobs[p].active) continue;
    HIPCHK(hipMemcpy(side.data(), d.cb_side + (size_t)p * d.n_pad, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mu.data(), d.cb_mu + (size_t)p * d.n_pad, n * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      if (side[i] < 3) {
        rows.push_back((int64_t)i);
        yy.push_back(h->y_host[i]);
        mm.push_back(mu[i]);
        owner.push_back((p << 2) | side[i]);
      }
  }
  size_t n_part = yy.size();
  const bool init = (ch.kind & CMD_INIT) != 0;
  if (init) {  // stump and current tree over all rows: [n_part, n_part + n) stump, [n_part + n, n_part + 2n) current
    std::vector<double2> pack(n);
    std::vector<double> noi(n);
    HIPCHK(hipMemcpy(pack.data(), d.pack, n * sizeof(double2), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(noi.data(), d.st + (size_t)(ch.st_cur ^ 1) * d.n_pad, n * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      rows.push_back((int64_t)i);
      yy.push_back(h->y_host[i]);
      mm.push_back((noi[i] + h->off_host[i]) + d.init_leaf);
    }
    for (size_t i = 0; i < n; ++i) {
      rows.push_back((int64_t)i);
      yy.push_back(h->y_host[i]);
      mm.push_back(pack[i].x + h->off_host[i]);
    }
  }
  if (yy.empty()) return PGB_OK;
  out.assign(yy.size(), 0.0);
  if (h->cb_fn(h->cb_ctx, rows.data(), yy.data(), mm.data(), (int64_t)yy.size(), out.data()) != 0)
    return fail(PGB_E_STATE, "the log-likelihood callback reported an error");
  unsigned sat = 0;
  std::vector<AccL> sums(MAXP, AccL{0, 0, 0, 0});
  for (size_t i = 0; i < n_part; ++i) {
    const long long q = pgb_quant(pgb_clamp_loglik(out[i]), d.sc.cl, &sat);
    AccL& a = sums[owner[i] >> 2];
    const int sd = owner[i] & 3;
    if (sd == 0) a.llL += q; else if (sd == 1) a.llR += q; else a.llN += q;
  }
  for (int p = 1; p < d.P; ++p)
    if (jobs[p].active)  // copy 0 of the particle's record (k_ctrl zeroed all copies in this slot)
      HIPCHK(hipMemcpy(&d.accl[((size_t)par * MAXP + p) * LL_PER], &sums[p], sizeof(AccL), hipMemcpyHostToDevice));
  if (init) {
    long long C = 0, E0 = 0;
    for (size_t i = 0; i < n; ++i) C += pgb_quant(pgb_clamp_loglik(out[n_part + i]), d.sc.cl, &sat);
    for (size_t i = 0; i < n; ++i) E0 += pgb_quant(pgb_clamp_loglik(out[n_part + n + i]), d.sc.cl, &sat);
    InitAcc ia;
    HIPCHK(hipMemcpy(&ia, &d.initacc[(size_t)par * IA_SLOTS], sizeof ia, hipMemcpyDeviceToHost));
    ia.C += C;
    ia.E0 += E0;
    HIPCHK(hipMemcpy(&d.initacc[(size_t)par * IA_SLOTS], &ia, sizeof ia, hipMemcpyHostToDevice));
  }
  if (sat) {
    unsigned long long cs = 0;
    HIPCHK(hipMemcpy(&cs, &d.counters[4], sizeof cs, hipMemcpyDeviceToHost));
    cs += sat;
    HIPCHK(hipMemcpy(&d.counters[4], &cs, sizeof cs, hipMemcpyHostToDevice));
  }
  return PGB_OK;
}

// ---- feeding the state machine ---------------------------------------------------------------------------
// The device publishes two progress words besides the step count: flag[2] = slots whose control kernel has
// started (Ctrl::slot_no, one posted store per slot) and flag[1] = steps that are complete.  The host
// enqueues against flag[2] like against a credit: up to FEED_AHEAD slots beyond the executed one while the
// step is expected to need them (running mean - 1 sd of the slots such a call took), FEED_MIN beyond it
// after that -- so a finished step leaves at most a few idle slots (~2.6 us each) behind it.  No events, no
// barrier packets: the throttle costs the device nothing and the host one read of pinned memory.
static double watchdog_seconds() {
  static const double v = getenv("PGB_WATCHDOG_S") ? atof(getenv("PGB_WATCHDOG_S")) : 20.0;
  return v > 0.1 ? v : 0.1;
}
// Lost-device watchdog by the WALL clock (a poll count means different times on different hosts, and a false
// trip poisons the chain): PGB_WATCHDOG_S seconds without a single slot starting (flag[2]); the deadline MOVES
// whenever the device publishes progress, so that a pass that takes longer than PGB_WATCHDOG_S on a time-sliced GPU,
// under a profiler or at very large n does not poison a healthy chain (round-4 ADVICE).  A device that stops
// publishing progress (lost GPU, a kernel that faulted) ends the call, not the process: poll() looks at the clock
// every 0x4000 calls and, past the deadline, poisons the handle and fails with the caller's sentence for a stream
// in error (`lost`) or for a healthy but stuck one (`stuck`).
struct ProgressWatch {
  pgb_handle* h;
  const char *lost, *stuck;
  long long polls = 0, seen;
  std::chrono::steady_clock::time_point deadline;
  static std::chrono::steady_clock::time_point after(std::chrono::steady_clock::time_point now) {
    return now + std::chrono::milliseconds((long long)(watchdog_seconds() * 1e3));
  }
  ProgressWatch(pgb_handle* h_, const char* lost_, const char* stuck_)
      : h(h_), lost(lost_), stuck(stuck_), seen((long long)h_->flag[2]), deadline(after(std::chrono::steady_clock::now())) {}
  bool expired(std::chrono::steady_clock::time_point now) {
    if ((long long)h->flag[2] == seen) return now > deadline;
    seen = (long long)h->flag[2];
    deadline = after(now);
    return false;
  }
  int poll() {
    if ((++polls & 0x3FFF) != 0 || !expired(std::chrono::steady_clock::now())) return PGB_OK;
    hipError_t e = hipStreamQuery(h->stream);
    h->poisoned = 1;
    if (e != hipSuccess && e != hipErrorNotReady) return fail_hip(e, lost);
    return fail(PGB_E_STATE, stuck);
  }
};
#define FEED_AHEAD 24
#define FEED_MIN 6
#define FEED_RUN 8
static int feed_until_flag(pgb_handle* h, int n_steps) {
  Dev& d = h->d;
  const long long start = h->slot;
  long long cap = start + (long long)n_steps * (PGB_MAX_NODES + 3) * (d.m + 1) + 64;
  int rc;
  if (h->s.family == PGB_FAMILY_CALLBACK) {  // one slot at a time, the host evaluates between slots
    if (!h->cb_fn) return fail(PGB_E_INVALID, "pgb_set_loglik_callback first");
    while (*h->flag < (unsigned long long)h->steps_target) {
      const int par = (int)(h->slot & 1);
      if ((rc = enqueue_slots(h, 1)) != PGB_OK) return rc;
      HIPCHK(hipStreamSynchronize(h->stream));
      if ((rc = callback_host_phase(h, par)) != PGB_OK) {
        h->poisoned = 1;  // steps_target is ahead of the flag and the device sits in the middle of a round
        return rc;
      }
      if (h->slot > cap) {
        h->poisoned = 1;
        return fail(PGB_E_STATE, "sampler state machine did not finish");
      }
    }
    return PGB_OK;
  }
  static const int feed_ahead = getenv("PGB_FEED_AHEAD") ? atoi(getenv("PGB_FEED_AHEAD")) : FEED_AHEAD;
  static const int feed_min = getenv("PGB_FEED_MIN") ? atoi(getenv("PGB_FEED_MIN")) : FEED_MIN;
  static const double feed_sd = getenv("PGB_FEED_SD") ? atof(getenv("PGB_FEED_SD")) : 1.0;
  // slots this call is expected to need at least: mean - feed_sd * sd of the running per-step estimate
  long long expect_end = 1ll << 60;
  if (h->slots_per_step > 0.0) {
    const double sd = h->slots_var > 0.0 ? __builtin_sqrt(h->slots_var) : 0.15 * h->slots_per_step;
    double e = h->slots_per_step * n_steps - feed_sd * sd * __builtin_sqrt((double)n_steps);
    expect_end = start + (long long)(e > 1.0 ? e : 1.0);
  }
  int refill = 0;
  ProgressWatch watch(h, "device stopped making progress", "device stopped publishing slot progress");
  while (*h->flag < (unsigned long long)h->steps_target) {
    const long long executed = (long long)h->flag[2];
    long long limit = executed + feed_ahead;
    if (limit > expect_end) limit = expect_end;
    if (limit < executed + feed_min) limit = executed + feed_min;
    // far from the expected end the queue is topped up in runs of FEED_RUN slots (several chains share the
    // runtime's launch path: slot-by-slot refills of four chains at once cost them 30 % of their aggregate);
    // near it, slot by slot
    if (refill == 0 && h->slot < limit) {
      const bool far = limit == executed + feed_ahead;
      if (!far || h->slot - executed <= feed_ahead - FEED_RUN) refill = far ? FEED_RUN : 1;
    }
    if (refill > 0 && h->slot < limit) {
      refill -= 1;
      if ((rc = enqueue_slots(h, 1)) != PGB_OK) return rc;
      if (h->slot > cap) {
        h->poisoned = 1;
        return fail(PGB_E_STATE, "sampler state machine did not finish");
      }
      watch.polls = 0;  // (idle polls since the last slot went out)
    } else {
      refill = 0;
      for (int i = 0; i < 16; ++i) __builtin_ia32_pause();
      // several chains feed their own streams from their own threads (chains.sample_chains, bench.py's
      // concurrent chains): a waiting feeder gives its core away instead of spinning against the others
      if (g_live_handles.load(std::memory_order_relaxed) > 1) sched_yield();
      if ((rc = watch.poll()) != PGB_OK) return rc;
    }
  }
  return PGB_OK;
}

static int run_until_idle(pgb_handle* h, int n_steps) {
  Dev& d = h->d;
  int rc;
  if ((rc = feed_until_flag(h, n_steps)) != PGB_OK) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->prof && (rc = harvest_profile(h)) != PGB_OK) return rc;
  Ctrl c;
  HIPCHK(hipMemcpy(&c, &d.ctrl[h->slot & 1], sizeof c, hipMemcpyDeviceToHost));
  if (c.phase != PH_IDLE) return fail(PGB_E_STATE, "device not idle after the progress flag fired");
  h->st_cur = c.st_cur;
  h->alpha_cur = c.alpha_cur;
  return PGB_OK;
}

// what a step needs: data and response, a chain whose state is defined, the compiled family's code
static int check_can_step(pgb_handle* h) {
  if (!h->have_data || !h->have_y) return fail(PGB_E_INVALID, "set_data/set_response first");
  REFUSE_POISONED(h);
  if (h->s.family == PGB_FAMILY_COMPILED && !h->cl_fn) return fail(PGB_E_INVALID, "pgb_set_loglik_code first");
  return PGB_OK;
}

static int begin_steps(pgb_handle* h, int tune, int n_steps) {
  Dev& d = h->d;
  const int rc = check_can_step(h);
  if (rc != PGB_OK) return rc;
  int par = (int)(h->slot & 1);
  h->out_valid = 0;
  hipLaunchKernelGGL(k_begin, dim3(1), dim3(256), 0, h->stream, h->d_dev, par, tune, n_steps,
                     h->inv_sigma2, h->lik_param2, h->sigma_dirty);
  h->steps_target += n_steps;
  h->sigma_dirty = 0;
  // host mirror of the batch cursor ([U] PGBART.astep batching)
  for (int i = 0; i < n_steps; ++i) {
    int bs = tune ? d.batch_tune : d.batch_draw;
    int upper = h->lower_host + bs;
    if (upper > d.m) upper = d.m;
    h->last_lower = h->lower_host;
    h->last_n = upper - h->lower_host;
    h->lower_host = upper < d.m ? upper : 0;
  }
  return PGB_OK;
}

static void counters_from(pgb_handle* h, const unsigned long long* c) {
  h->ctr.particle_steps = (int64_t)c[0];
  h->ctr.tree_updates = (int64_t)c[1];
  h->ctr.rows_touched = (int64_t)c[2];
  h->ctr.rounds = (int64_t)c[3];
  h->ctr.saturations = (int64_t)c[4];
  h->ctr.slots = (int64_t)c[5];
  h->ctr.partitions = (int64_t)c[6];
}

// running estimate of the (working) slots one astep needs, from the device's own count
static void note_step_slots(pgb_handle* h, long long slots_before, int n_steps) {
  const double per = (double)(h->ctr.slots - slots_before) / (double)(n_steps > 0 ? n_steps : 1);
  if (per <= 0.0) return;
  if (h->slots_per_step <= 0.0) {
    h->slots_per_step = per;
    return;
  }
  // exponentially weighted mean / variance (weight 1/8); a batch of n steps averages n of them
  const double dev = per - h->slots_per_step;
  h->slots_per_step += 0.125 * dev;
  h->slots_var = 0.875 * (h->slots_var + 0.125 * dev * dev * (n_steps > 0 ? n_steps : 1));
}

static int fetch_counters(pgb_handle* h, pgb_counters* out) {
  unsigned long long c[8];
  HIPCHK(hipMemcpyAsync(c, h->d.counters, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  counters_from(h, c);
  if (out) *out = h->ctr;
  return PGB_OK;
}

extern "C" int pgb_set_output_stream(pgb_handle* h, void* stream) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  h->stream_out = (hipStream_t)stream;  // owned by the caller
  return PGB_OK;
}

extern "C" int pgb_set_loglik_callback(pgb_handle* h, pgb_loglik_fn fn, void* ctx) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  if (h->s.family != PGB_FAMILY_CALLBACK)
    return fail(PGB_E_INVALID, "the sampler was not created with the callback family");
  h->cb_fn = fn;
  h->cb_ctx = ctx;
  return PGB_OK;
}

extern "C" int pgb_step(pgb_handle* h, int32_t tune, double* sum_trees_dev_out, int32_t* vi_counts_host_out,
                        pgb_counters* counters_out) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  int rc;
  const long long slots0 = h->ctr.slots;
  if ((rc = begin_steps(h, tune, 1)) != PGB_OK) return rc;
  if ((rc = run_until_idle(h, 1)) != PGB_OK) return rc;
  if (sum_trees_dev_out)  // [K][n] out of the padded [K][n_pad] buffer
    HIPCHK(hipMemcpy2DAsync(sum_trees_dev_out, h->d.n * sizeof(double),
                            h->d.st + (size_t)h->st_cur * h->d.K * h->d.n_pad, h->d.n_pad * sizeof(double),
                            h->d.n * sizeof(double), (size_t)h->d.K, hipMemcpyDeviceToDevice, h->stream));
  if (vi_counts_host_out)
    HIPCHK(hipMemcpyAsync(vi_counts_host_out, h->d.vi, h->d.p * sizeof(int32_t), hipMemcpyDeviceToHost,
                          h->stream));
  if ((rc = fetch_counters(h, counters_out)) != PGB_OK) return rc;
  note_step_slots(h, slots0, 1);
  return PGB_OK;
}

// PGBART.astep's return path in one device -> host transaction: the state machine runs to its idle
// point, k_export_step writes the small results (trees of this step, vi, counters, control words)
// into the mapped pinned block and densifies sum_trees, one DMA moves sum_trees to the caller,
// ONE stream synchronisation ends the call.
extern "C" int pgb_step_host(pgb_handle* h, int32_t tune, double* sum_trees_host_out,
                             int32_t* vi_counts_host_out, pgb_counters* counters_out) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  Dev& d = h->d;
  int rc;
  const long long slots0 = h->ctr.slots;
  if ((rc = begin_steps(h, tune, 1)) != PGB_OK) return rc;
  if ((rc = feed_until_flag(h, 1)) != PGB_OK) return rc;
  const int nt = h->last_n;
  if (nt > h->out_layout.cap_trees) return fail(PGB_E_STATE, "step batch exceeds the export block");
  // The progress word fires when the last tree is accepted; its FINAL row pass runs in that same slot, and the
  // first idle slot behind it publishes "step complete" (flag[1]).  From there the results leave on a stream of
  // their own: the idle slots still queued on the sampler's stream (a few, ~2.6 us each) drain
  // while the export, the DMA and the caller's host work go on.
  hipStream_t so = h->stream;
  const bool early = h->s.family != PGB_FAMILY_CALLBACK && !h->prof && h->stream_out != nullptr;
  if (early) {
    int extra = 0;
    ProgressWatch watch(h, "device stopped before the step-complete word", "the step-complete word never fired");
    while (h->flag[1] < (unsigned long long)h->steps_target) {
      // (a device that faults between "last tree accepted" and the first idle slot would otherwise hold this
      //  loop for ever, with the GIL released; a long FINAL pass moves the deadline like any other progress)
      if ((rc = watch.poll()) != PGB_OK) return rc;
      // every enqueued slot has started and none of them was an idle one behind the finishing slot: one more
      if ((long long)h->flag[2] >= h->slot) {
        if (h->flag[1] >= (unsigned long long)h->steps_target) break;
        if (++extra > 16) { h->poisoned = 1; return fail(PGB_E_STATE, "the step-complete word never fired"); }
        if ((rc = enqueue_slots(h, 1)) != PGB_OK) return rc;
      }
      for (int i = 0; i < 16; ++i) __builtin_ia32_pause();
    }
    so = h->stream_out;
  }
  const long long dense_blocks = sum_trees_host_out ? ((long long)d.K * d.n + BT - 1) / BT : 0;
  long long grid = dense_blocks < 512 ? dense_blocks : 512;
  if (grid < nt) grid = nt;
  if (grid < 1) grid = 1;
  // sum_trees goes straight into the caller's buffer when that is device-accessible pinned memory (what
  // PySampler hands in): the export kernel writes it over PCIe itself -- one kernel instead of a densify
  // kernel, a copy kernel and the gap between them.  Pageable memory: densify in HBM, then one DMA.
  double* direct = nullptr;
  if (sum_trees_host_out && !(getenv("PGB_NO_DIRECT_OUT") && atoi(getenv("PGB_NO_DIRECT_OUT")))) {
    // (asked every time: the same address may be pinned in one call and ordinary memory in the next)
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, sum_trees_host_out, 0) == hipSuccess && dp) direct = (double*)dp;
    else (void)hipGetLastError();  // not pinned: the DMA path
  }
  hipLaunchKernelGGL(k_export_step, dim3((unsigned)grid), dim3(BT), 0, so, (const Dev*)h->d_dev,
                     (int)(h->slot & 1), h->last_lower, nt, h->out_dev, h->out_layout,
                     sum_trees_host_out ? (direct ? direct : h->st_dense) : nullptr);
  if (sum_trees_host_out && !direct)
    HIPCHK(hipMemcpyAsync(sum_trees_host_out, h->st_dense, (size_t)d.K * d.n * sizeof(double),
                          hipMemcpyDeviceToHost, so));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so));
  if (h->prof && (rc = harvest_profile(h)) != PGB_OK) return rc;
  const StepOutHdr* H = (const StepOutHdr*)h->out_host;
  if (H->phase != PH_IDLE) return fail(PGB_E_STATE, "device not idle after the progress flag fired");
  h->st_cur = H->st_cur;
  h->alpha_cur = H->alpha_cur;
  counters_from(h, H->counters);
  note_step_slots(h, slots0, 1);
  h->out_valid = 1;
  if (vi_counts_host_out) memcpy(vi_counts_host_out, h->out_host + h->out_layout.vi, (size_t)d.p * sizeof(int32_t));
  if (counters_out) *counters_out = h->ctr;
  return PGB_OK;
}

extern "C" int pgb_step_async(pgb_handle* h, int32_t tune, int32_t n_steps) {
  if (!h || n_steps < 1) return fail(PGB_E_INVALID, "bad argument");
  JOIN_ASYNC(h);
  const int rc0 = check_can_step(h);  // (refused here, synchronously, not in the worker)
  if (rc0 != PGB_OK) return rc0;
  h->job_running = 1;
  h->job_rc = PGB_OK;
  h->job_err[0] = 0;
  h->worker = std::thread([h, tune, n_steps]() {
    int rc = PGB_OK;
    if (hipSetDevice(h->device) != hipSuccess) rc = fail(PGB_E_DEVICE, "hipSetDevice in the step worker");
    if (rc == PGB_OK) rc = begin_steps(h, tune, n_steps);
    if (rc == PGB_OK) rc = run_until_idle(h, n_steps);
    h->job_rc = rc;
    if (rc != PGB_OK) snprintf(h->job_err, sizeof h->job_err, "%s", g_err);  // this thread's message
  });
  return PGB_OK;
}

extern "C" int pgb_sync(pgb_handle* h, pgb_counters* counters_out) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  return fetch_counters(h, counters_out);
}

// the trees describe themselves (include/pgbart.h, pgb_tree_arrays::rule): how each split node sends a row left
static void fill_node_rules(const pgb_handle* h, pgb_tree_arrays* out, int total) {
  if (!out->rule) return;
  const int p = (int)h->rules_host.size();
  for (int g = 0; g < total; ++g) {
    const int j = out->var[g];
    out->rule[g] = j >= 0 && j < p ? h->rules_host[j] : PGB_RULE_CONTINUOUS;
  }
}

// the trees of the last pgb_step_host, already in host memory (k_export_step)
static int export_from_block(pgb_handle* h, pgb_tree_arrays* out) {
  const StepOutHdr* H = (const StepOutHdr*)h->out_host;
  const StepOutLayout& L = h->out_layout;
  const int nt = H->n_trees, total = H->total_nodes, K = H->K;
  if (!out->var) {
    out->n_trees = nt;
    out->n_outputs = K;
    out->total_nodes = total;
    return PGB_OK;
  }
  if (out->n_trees != nt || out->total_nodes != total) return fail(PGB_E_INVALID, "size mismatch");
  const unsigned char* B = h->out_host;
  for (int t = 0; t < nt; ++t) out->tree_id[t] = H->first + t;
  memcpy(out->node_off, B + L.node_off, (size_t)(nt + 1) * 4);
  memcpy(out->var, B + L.var, (size_t)total * 4);
  memcpy(out->left, B + L.left, (size_t)total * 4);
  memcpy(out->right, B + L.right, (size_t)total * 4);
  memcpy(out->split, B + L.split, (size_t)total * 8);
  memcpy(out->count, B + L.count, (size_t)total * 8);
  memcpy(out->value, B + L.value, (size_t)total * 8 * K);
  fill_node_rules(h, out, total);
  if (out->slope && out->xbar && out->svar) {
    if (H->lin) {
      memcpy(out->slope, B + L.slope, (size_t)total * 8 * K);
      memcpy(out->xbar, B + L.xbar, (size_t)total * 8);
      memcpy(out->svar, B + L.svar, (size_t)total * 4);
    } else {
      memset(out->slope, 0, (size_t)total * 8 * K);
      memset(out->xbar, 0, (size_t)total * 8);
      for (int g = 0; g < total; ++g) out->svar[g] = -1;
    }
  }
  return PGB_OK;
}

// Accepted trees [first, first + nt) in host memory: the node tables, and where the model has them the K-vector
// values (tvx), the linear leaves (tlin) and the slopes of outputs 1..K-1 (tsx).  The accessors state once how a
// node's fields follow from them; write_nodes() turns them into the flat node arrays of the chain image and of
// pgb_tree_arrays (host arrays in, host arrays out: no device involved).
struct HostTrees {
  int first = 0, nt = 0, K = 1;
  std::vector<DTree> T;
  std::vector<double> vx, sx;  // [nt][MAXN][K - 1]
  std::vector<LinP> lin;       // [nt][MAXN]; empty: constant leaves, or not fetched
  const DNode& node(int t, int k) const { return T[t].nd[k]; }
  size_t at(int t, int k, int o) const { return ((size_t)t * MAXN + k) * (K - 1) + o - 1; }
  int total_nodes() const {
    int N = 0;
    for (int t = 0; t < nt; ++t) N += T[t].n_nodes;
    return N;
  }
  double value(int t, int k, int o) const { return node(t, k).var >= 0 ? 0.0 : o ? vx[at(t, k, o)] : node(t, k).value; }
  bool is_lin(int t, int k) const { return node(t, k).var < 0 && !lin.empty() && lin[(size_t)t * MAXN + k].svar >= 0; }
  double slope(int t, int k, int o) const { return !is_lin(t, k) ? 0.0 : o ? sx[at(t, k, o)] : lin[(size_t)t * MAXN + k].slope; }
  double xbar(int t, int k) const { return is_lin(t, k) ? lin[(size_t)t * MAXN + k].xbar : 0.0; }
  int32_t svar(int t, int k) const { return is_lin(t, k) ? (int32_t)lin[(size_t)t * MAXN + k].svar : -1; }

  // the node tables: every enqueued slot has run once the stream is idle; blocking copies from there
  int fetch(pgb_handle* h, int first_, int nt_) {
    first = first_, nt = nt_, K = h->d.K;
    T.resize((size_t)nt);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (nt > 0) HIPCHK(hipMemcpy(T.data(), h->d.trees + first, sizeof(DTree) * nt, hipMemcpyDeviceToHost));
    return PGB_OK;
  }
  // ... and the leaf parts next to them (want_lin = false: a caller that takes no slopes)
  int fetch_leaves(pgb_handle* h, bool want_lin) {
    const Dev& d = h->d;
    const size_t nodes = (size_t)nt * MAXN, KX = (size_t)(K - 1);
    if (nt <= 0) return PGB_OK;
    if (KX > 0) {
      vx.resize(nodes * KX);
      HIPCHK(hipMemcpy(vx.data(), d.tvx + (size_t)first * MAXN * KX, vx.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (!want_lin || d.response == PGB_RESPONSE_CONSTANT) return PGB_OK;
    lin.resize(nodes);
    HIPCHK(hipMemcpy(lin.data(), d.tlin + (size_t)first * MAXN, lin.size() * sizeof(LinP), hipMemcpyDeviceToHost));
    if (KX > 0) {
      sx.resize(nodes * KX);
      HIPCHK(hipMemcpy(sx.data(), d.tsx + (size_t)first * MAXN * KX, sx.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    return PGB_OK;
  }
};

// where the flat node arrays go: the fields the image and pgb_tree_arrays share, and the two only the image has
struct NodeSink {
  int32_t *node_off, *var, *left, *right;
  int64_t* count;
  double *split, *value;
  double* slope;  // with xbar and svar, or all three null: no linear part wanted
  double* xbar;
  int32_t* svar;
  int32_t *depth, *label;  // (null: pgb_tree_arrays)
};
static NodeSink node_sink(const pgb_image_view& v) {
  return NodeSink{v.node_off, v.var, v.left, v.right, v.count, v.split, v.value, v.slope, v.xbar, v.svar, v.depth, v.label};
}
static NodeSink node_sink(const pgb_tree_arrays* a) {
  const bool want_lin = a->slope && a->xbar && a->svar;
  return NodeSink{a->node_off, a->var, a->left, a->right, a->count, a->split, a->value, want_lin ? a->slope : nullptr,
                  want_lin ? a->xbar : nullptr, want_lin ? a->svar : nullptr, nullptr, nullptr};
}
static void write_nodes(const HostTrees& ht, const NodeSink& out) {
  const int K = ht.K;
  int32_t g = 0;
  for (int t = 0; t < ht.nt; ++t) {
    out.node_off[t] = g;
    for (int k = 0; k < ht.T[t].n_nodes; ++k, ++g) {
      const DNode& z = ht.node(t, k);
      const bool leaf = z.var < 0;
      out.var[g] = z.var;
      out.split[g] = leaf ? 0.0 : z.split;
      out.left[g] = leaf ? -1 : (int32_t)z.left;
      out.right[g] = leaf ? -1 : (int32_t)z.right;
      out.count[g] = z.cnt;
      for (int o = 0; o < K; ++o) out.value[(size_t)g * K + o] = ht.value(t, k, o);
      if (out.slope) {
        for (int o = 0; o < K; ++o) out.slope[(size_t)g * K + o] = ht.slope(t, k, o);
        out.xbar[g] = ht.xbar(t, k);
        out.svar[g] = ht.svar(t, k);
      }
      if (out.depth) out.depth[g] = z.depth, out.label[g] = z.label;
    }
  }
  out.node_off[ht.nt] = g;
}

extern "C" int pgb_export_trees(pgb_handle* h, int32_t which, pgb_tree_arrays* out) {
  if (!h || !out) return fail(PGB_E_INVALID, "null argument");
  JOIN_ASYNC(h);
  REFUSE_POISONED(h);
  if (which == 0 && h->out_valid) return export_from_block(h, out);
  HostTrees ht;
  int rc = ht.fetch(h, which == 0 ? h->last_lower : 0, which == 0 ? h->last_n : h->d.m);
  if (rc != PGB_OK) return rc;
  const int total = ht.total_nodes();
  if (!out->var) {
    out->n_trees = ht.nt;
    out->n_outputs = ht.K;
    out->total_nodes = total;
    return PGB_OK;
  }
  if (out->n_trees != ht.nt || out->total_nodes != total) return fail(PGB_E_INVALID, "size mismatch");
  const NodeSink sink = node_sink(out);
  if ((rc = ht.fetch_leaves(h, sink.slope != nullptr)) != PGB_OK) return rc;
  for (int t = 0; t < ht.nt; ++t) out->tree_id[t] = ht.first + t;
  write_nodes(ht, sink);
  fill_node_rules(h, out, total);
  return PGB_OK;
}


extern "C" int pgb_export_trees_packed(pgb_handle* h, int32_t which, void* host_buf, int64_t cap_bytes,
                                       int64_t* bytes_out) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  const int rc = pgb_export_trees_packed_via(h, which, host_buf, cap_bytes, bytes_out,
                                             h->s.response != PGB_RESPONSE_CONSTANT);
  if (rc == PGB_E_NOMEM) return fail(rc, "packed tree record does not fit the buffer (*bytes_out has the size)");
  return rc;
}

// (pgb_get_state: pgb_checkpoint.h, next to the image that needs the same idle-state read)

extern "C" int pgb_get_split_weights(pgb_handle* h, double* out) {
  if (!h || !out) return fail(PGB_E_INVALID, "null argument");
  JOIN_ASYNC(h);
  std::vector<long long> a((size_t)h->d.p);
  HIPCHK(hipMemcpyAsync(a.data(), h->d.alpha + (size_t)h->alpha_cur * h->d.p, h->d.p * sizeof(long long),
                        hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // in units of the caller's prior: prior_j + number of tuning counts (up to 2^-24 rounding)
  for (int j = 0; j < h->d.p; ++j) out[j] = (double)a[j] * (h->d.max_prior * pgb_pow2(-PGB_ALPHA_BITS));
  return PGB_OK;
}
