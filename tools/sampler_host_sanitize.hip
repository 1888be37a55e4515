// sampler_host_sanitize.hip -- the sampler's host layer (csrc/pgb_host.h, csrc/pgb_checkpoint.h) under AddressSanitizer
// and UndefinedBehaviorSanitizer: a stand-alone program on the build box, no GPU needed.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ipymc_bart_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fsanitize=address,undefined \
//         tools/sampler_host_sanitize.hip -o build/sampler_host_sanitize && build/sampler_host_sanitize
//
// What the GPU suite cannot pin to a line: every refusal of pgb_create that precedes the device query, with its
// sentence; the kernels select_slot_kernels picks, against a literal table that restates the ladders enqueue_slots
// had; the flat node arrays write_nodes makes of two hand-built forests, through both sinks; and ProgressWatch over a
// host word.  Exit status 0: every expectation held and the sanitizers saw nothing.
#define PGB_HEADERS_HASH 0ull
#include "pgbart_hip.hip"

static int g_bad = 0;
static void check(bool ok, const char* what) {
  if (!ok) ++g_bad;
  if (!ok) printf("BAD  %s\n", what);
}
static void expect(const char* what, int rc, int want_rc, const char* sentence) {
  const char* msg = pgb_last_error();
  const bool ok = rc == want_rc && (!sentence || strstr(msg, sentence));
  printf("%-4s %-48s rc = %d  %s\n", ok ? "ok" : "BAD", what, rc, rc == PGB_OK ? "" : msg);
  if (!ok) ++g_bad;
}

// ---- pgb_create: every refusal ahead of the device query
static void create_refusals() {
  pgb_settings ok;
  memset(&ok, 0, sizeof ok);
  ok.n = 100, ok.p = 3, ok.m = 5, ok.num_particles = 10, ok.n_outputs = 1, ok.family = PGB_FAMILY_NORMAL;
  ok.batch_tune = ok.batch_draw = 1, ok.range_exp = 8, ok.response = PGB_RESPONSE_CONSTANT;
  pgb_handle* h = nullptr;
  const int I = PGB_E_INVALID, U = PGB_E_UNSUPPORTED;
  auto refused = [&](const char* what, pgb_settings s, int rc, const char* sentence) {
    expect(what, pgb_create(&s, nullptr, &h), rc, sentence);
  };
  expect("create: null settings", pgb_create(nullptr, nullptr, &h), I, "null argument");
  expect("create: null out", pgb_create(&ok, nullptr, nullptr), I, "null argument");
  pgb_settings s = ok;
  s.n = 0;
  refused("create: n", s, I, "n, p, m must be >= 1");
  s = ok, s.p = 0;
  refused("create: p", s, I, "n, p, m must be >= 1");
  s = ok, s.m = 0;
  refused("create: m", s, I, "n, p, m must be >= 1");
  s = ok, s.n = (1ll << 31) - CH;
  refused("create: n too large", s, U, "n too large");
  s = ok, s.num_particles = 1;
  refused("create: one particle", s, I, "num_particles must be in [2, 64] (libpgbart_hip_p128.so takes up to 128)");
  s = ok, s.num_particles = PGB_MAX_PARTICLES + 1;
  refused("create: too many particles", s, I, "num_particles must be in [2, 64]");
  s = ok, s.family = PGB_FAMILY_CATEGORICAL;
  refused("create: categorical, one output", s, I, "CATEGORICAL needs 2 <= n_outputs <= " PGB_STR(PGB_MAX_OUTPUTS));
  s.n_outputs = PGB_MAX_OUTPUTS + 1;
  refused("create: categorical, too many outputs", s, I, "CATEGORICAL needs 2 <= n_outputs <= " PGB_STR(PGB_MAX_OUTPUTS));
  s = ok, s.family = PGB_FAMILY_NORMAL_MEANSCALE;
  refused("create: mean / scale, one output", s, I, "NORMAL_MEANSCALE needs n_outputs == 2");
  s = ok, s.family = PGB_FAMILY_COMPILED, s.n_outputs = 0;
  refused("create: compiled, no output", s, I, "COMPILED needs 1 <= n_outputs <= " PGB_STR(PGB_MAX_OUTPUTS));
  s.n_outputs = PGB_MAX_OUTPUTS + 1;
  refused("create: compiled, too many outputs", s, I, "COMPILED needs 1 <= n_outputs <= " PGB_STR(PGB_MAX_OUTPUTS));
  s = ok, s.n_outputs = 2;
  refused("create: normal, two outputs", s, I, "this family has a single output");
  s = ok, s.family = PGB_FAMILY_POISSON_LOG, s.n_outputs = 3;
  refused("create: poisson, three outputs", s, I, "this family has a single output");
  s = ok, s.family = PGB_FAMILY_CALLBACK, s.response = PGB_RESPONSE_LINEAR;
  refused("create: callback, linear leaves", s, U, "the callback family has constant leaves");
  s = ok, s.family = 1000;
  refused("create: unknown family", s, U, "unknown family");
  s = ok, s.batch_tune = 0;
  refused("create: batch_tune", s, I, "batch sizes must be >= 1");
  s = ok, s.batch_draw = 0;
  refused("create: batch_draw", s, I, "batch sizes must be >= 1");
  s = ok, s.compat = PGB_COMPAT_ALL + 1;
  refused("create: compat", s, I, "unknown compat bits (pgbart_spec.h: PGB_COMPAT_*)");
  s = ok, s.response = 1000;
  refused("create: unknown response", s, U, "unknown response");
  check(h == nullptr, "create: a refused call leaves *out alone");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
    (void)hipGetLastError();
    refused("create: no device", ok, PGB_E_DEVICE, "no HIP device visible (");
    expect("create: no device (the sentence's end)", PGB_E_DEVICE, PGB_E_DEVICE, "); this backend has no CPU fallback");
    check(h == nullptr && g_live_handles.load() == 0, "create: no device, no handle");
  }
}

// ---- select_slot_kernels: the ladders of the per-slot loop as they were, one line per legal combination.  Keys imply
// constant leaves and no SubsetSplit column; the Normal family has one output.
struct Choice {
  int K, lin, keys, sub, nrm;
  ctrl_kernel_t ctrl;
  rows_kernel_t rows;
  int extra;  // k_ctrl workgroups beyond P - 1
};
static const Choice g_choices[] = {
    // K = 1: k_rows<SUB, NORMAL, LIN, F32>
    {1, 0, 0, 0, 0, k_ctrl<false, false>, k_rows<false, false, false>, 1},
    {1, 0, 0, 0, 1, k_ctrl<false, false>, k_rows<false, true, false>, 1},
    {1, 0, 0, 1, 0, k_ctrl<false, false>, k_rows<true, false, false>, 1},
    {1, 0, 0, 1, 1, k_ctrl<false, false>, k_rows<true, true, false>, 1},
    {1, 0, 1, 0, 0, k_ctrl<false, false, true>, k_rows<false, false, false, true>, 1},
    {1, 0, 1, 0, 1, k_ctrl<false, false, true>, k_rows<false, true, false, true>, 1},
    {1, 1, 0, 0, 0, k_ctrl<false, true>, k_rows<false, false, true>, 0},
    {1, 1, 0, 0, 1, k_ctrl<false, true>, k_rows<false, true, true>, 0},
    {1, 1, 0, 1, 0, k_ctrl<false, true>, k_rows<true, false, true>, 0},
    {1, 1, 0, 1, 1, k_ctrl<false, true>, k_rows<true, true, true>, 0},
    // K = 2, 3, 4: k_rows_mk<K, false, F32>; linear leaves: k_rows_mk<0, true> for any K
    {2, 0, 0, 0, 0, k_ctrl<true, false>, k_rows_mk<2, false>, 0},
    {2, 0, 0, 1, 0, k_ctrl<true, false>, k_rows_mk<2, false>, 0},
    {2, 0, 1, 0, 0, k_ctrl<true, false, true>, k_rows_mk<2, false, true>, 0},
    {2, 1, 0, 0, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
    {2, 1, 0, 1, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
    {3, 0, 0, 0, 0, k_ctrl<true, false>, k_rows_mk<3, false>, 0},
    {3, 0, 0, 1, 0, k_ctrl<true, false>, k_rows_mk<3, false>, 0},
    {3, 0, 1, 0, 0, k_ctrl<true, false, true>, k_rows_mk<3, false, true>, 0},
    {3, 1, 0, 0, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
    {3, 1, 0, 1, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
    {4, 0, 0, 0, 0, k_ctrl<true, false>, k_rows_mk<4, false>, 0},
    {4, 0, 0, 1, 0, k_ctrl<true, false>, k_rows_mk<4, false>, 0},
    {4, 0, 1, 0, 0, k_ctrl<true, false, true>, k_rows_mk<4, false, true>, 0},
    {4, 1, 0, 0, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
    {4, 1, 0, 1, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
    // K >= 5: the run-time-K instances
    {5, 0, 0, 0, 0, k_ctrl<true, false>, k_rows_mk<0, false>, 0},
    {5, 0, 0, 1, 0, k_ctrl<true, false>, k_rows_mk<0, false>, 0},
    {5, 0, 1, 0, 0, k_ctrl<true, false, true>, k_rows_mk<0, false, true>, 0},
    {5, 1, 0, 0, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
    {5, 1, 0, 1, 0, k_ctrl<true, true>, k_rows_mk<0, true>, 0},
};
static void slot_kernel_choices() {
  int legal = 0;  // the table has a line for every legal combination, and only those
  for (int K = 1; K <= 5; ++K)
    for (int lin = 0; lin < 2; ++lin)
      for (int keys = 0; keys < 2; ++keys)
        for (int sub = 0; sub < 2; ++sub)
          for (int nrm = 0; nrm < 2; ++nrm) legal += !(keys && (lin || sub)) && !(nrm && K > 1);
  check(legal == (int)(sizeof g_choices / sizeof g_choices[0]), "chooser: one line per legal combination");
  int wrong = 0;
  for (const Choice& c : g_choices)
    for (int P : {2, 10, PGB_MAX_PARTICLES}) {
      const SlotKernels k = select_slot_kernels(c.K, P, c.lin != 0, c.keys != 0, c.sub != 0, c.nrm != 0);
      const bool ok = k.ctrl == c.ctrl && k.rows == c.rows && k.ctrl_wgs == P - 1 + c.extra && k.rows_cap == 0;
      if (!ok) {
        printf("BAD  chooser: K = %d lin = %d keys = %d subset = %d normal = %d P = %d\n", c.K, c.lin, c.keys, c.sub, c.nrm, P);
        ++wrong;
      }
    }
  g_bad += wrong;
  printf("%-4s chooser: %d combinations x 3 particle counts\n", wrong ? "BAD" : "ok", legal);
  check(SlotKernels().ctrl == nullptr, "chooser: a fresh record is 'not chosen'");
}

// ---- write_nodes: hand-built forests through both sinks
struct Flat {  // room for both sinks of a forest of up to 8 nodes and 3 outputs
  int32_t node_off[4], var[8], left[8], right[8], depth[8], label[8], svar[8], tree_id[3];
  int64_t count[8];
  double split[8], xbar[8], value[24], slope[24];
  Flat() { memset(this, 0x5a, sizeof *this); }
  pgb_image_view view() {
    pgb_image_view v;
    memset(&v, 0, sizeof v);
    v.node_off = node_off, v.var = var, v.left = left, v.right = right, v.depth = depth, v.label = label, v.svar = svar;
    v.count = count, v.split = split, v.xbar = xbar, v.value = value, v.slope = slope;
    return v;
  }
  pgb_tree_arrays arrays(bool want_lin) {
    pgb_tree_arrays a;
    memset(&a, 0, sizeof a);
    a.tree_id = tree_id, a.node_off = node_off, a.var = var, a.split = split, a.left = left, a.right = right;
    a.count = count, a.value = value;
    if (want_lin) a.slope = slope, a.xbar = xbar, a.svar = svar;
    return a;
  }
};
template <typename T, size_t N>
static bool same(const T* got, const T (&want)[N]) {
  return memcmp(got, want, sizeof want) == 0;
}
static DNode node(int var, double split, double value, int cnt, int left, int right, int depth, int label) {
  DNode z;
  memset(&z, 0, sizeof z);
  z.var = var, z.split = split, z.value = value, z.cnt = cnt, z.cc_row = -1;
  z.left = (uint8_t)left, z.right = (uint8_t)right, z.depth = (uint8_t)depth, z.label = (uint8_t)label;
  return z;
}
static void host_trees() {
  {  // K = 1, constant leaves: a split with two leaves, then a stump
    HostTrees ht;
    ht.first = 3, ht.nt = 2, ht.K = 1;
    ht.T.resize(2);
    memset(ht.T.data(), 0, 2 * sizeof(DTree));
    ht.T[0].n_nodes = 3, ht.T[0].n_leaves = 2;
    ht.T[0].nd[0] = node(1, 0.5, 99.0, 10, 1, 2, 0, 0);  // (a split node's value is not a leaf value)
    ht.T[0].nd[1] = node(-1, 77.0, -1.25, 4, 0, 0, 1, 1);
    ht.T[0].nd[2] = node(-1, 0.0, 2.5, 6, 0, 0, 1, 2);
    ht.T[1].n_nodes = 1, ht.T[1].n_leaves = 1;
    ht.T[1].nd[0] = node(-1, 0.0, 0.125, 10, 0, 0, 0, 0);
    check(ht.total_nodes() == 4, "trees K = 1: total_nodes");
    const int32_t node_off[3] = {0, 3, 4}, var[4] = {1, -1, -1, -1}, left[4] = {1, -1, -1, -1}, right[4] = {2, -1, -1, -1};
    const int32_t depth[4] = {0, 1, 1, 0}, label[4] = {0, 1, 2, 0}, svar[4] = {-1, -1, -1, -1};
    const int64_t count[4] = {10, 4, 6, 10};
    const double split[4] = {0.5, 0.0, 0.0, 0.0}, value[4] = {0.0, -1.25, 2.5, 0.125}, zero[4] = {0.0, 0.0, 0.0, 0.0};
    Flat im, ar, ar0;
    write_nodes(ht, node_sink(im.view()));
    pgb_tree_arrays a = ar.arrays(true), a0 = ar0.arrays(false);
    write_nodes(ht, node_sink(&a));
    write_nodes(ht, node_sink(&a0));
    check(same(im.node_off, node_off) && same(im.var, var) && same(im.left, left) && same(im.right, right) &&
              same(im.depth, depth) && same(im.label, label) && same(im.svar, svar) && same(im.count, count) &&
              same(im.split, split) && same(im.value, value) && same(im.slope, zero) && same(im.xbar, zero),
          "trees K = 1: the image's node arrays");
    check(same(ar.node_off, node_off) && same(ar.var, var) && same(ar.left, left) && same(ar.right, right) &&
              same(ar.svar, svar) && same(ar.count, count) && same(ar.split, split) && same(ar.value, value) &&
              same(ar.slope, zero) && same(ar.xbar, zero),
          "trees K = 1: pgb_tree_arrays");
    check(ar.depth[0] == 0x5a5a5a5a && ar.label[0] == 0x5a5a5a5a, "trees K = 1: pgb_tree_arrays has no depth / label");
    check(same(ar0.node_off, node_off) && same(ar0.var, var) && same(ar0.count, count) && same(ar0.value, value) &&
              ar0.svar[0] == 0x5a5a5a5a && ar0.var[4] == 0x5a5a5a5a,
          "trees K = 1: pgb_tree_arrays without the linear part; nothing written past the last node");
    check(memcmp(im.var, ar.var, sizeof im.var) == 0 && memcmp(im.left, ar.left, sizeof im.left) == 0 &&
              memcmp(im.right, ar.right, sizeof im.right) == 0 && memcmp(im.count, ar.count, sizeof im.count) == 0 &&
              memcmp(im.split, ar.split, sizeof im.split) == 0 && memcmp(im.value, ar.value, sizeof im.value) == 0 &&
              memcmp(im.slope, ar.slope, sizeof im.slope) == 0 && memcmp(im.xbar, ar.xbar, sizeof im.xbar) == 0 &&
              memcmp(im.svar, ar.svar, sizeof im.svar) == 0 && memcmp(im.node_off, ar.node_off, sizeof im.node_off) == 0,
          "trees K = 1: the two sinks agree");
  }
  {  // K = 3, linear response: a split, a linear leaf and a constant leaf
    HostTrees ht;
    ht.first = 0, ht.nt = 1, ht.K = 3;
    ht.T.resize(1);
    memset(ht.T.data(), 0, sizeof(DTree));
    ht.T[0].n_nodes = 3, ht.T[0].n_leaves = 2;
    ht.T[0].nd[0] = node(2, 0.75, 99.0, 9, 1, 2, 0, 0);
    ht.T[0].nd[1] = node(-1, 0.0, -1.0, 4, 0, 0, 1, 1);
    ht.T[0].nd[2] = node(-1, 0.0, 4.0, 5, 0, 0, 1, 2);
    ht.vx.assign((size_t)MAXN * 2, 55.0);  // (what a split node's slots hold must not come through)
    ht.sx.assign((size_t)MAXN * 2, 66.0);  // (nor what a constant leaf's do)
    ht.lin.assign((size_t)MAXN, LinP{88.0, 88.0, -1});
    ht.vx[2] = -2.0, ht.vx[3] = -3.0, ht.vx[4] = 5.0, ht.vx[5] = 6.0;
    ht.sx[2] = 1.5, ht.sx[3] = 2.5;
    ht.lin[0] = LinP{88.0, 88.0, 1};  // (a split node is no linear leaf whatever its slot holds)
    ht.lin[1] = LinP{0.5, 0.25, 1};
    check(!ht.is_lin(0, 0) && ht.is_lin(0, 1) && !ht.is_lin(0, 2), "trees K = 3: is_lin");
    const int32_t node_off[2] = {0, 3}, var[3] = {2, -1, -1}, left[3] = {1, -1, -1}, right[3] = {2, -1, -1};
    const int32_t depth[3] = {0, 1, 1}, label[3] = {0, 1, 2}, svar[3] = {-1, 1, -1};
    const int64_t count[3] = {9, 4, 5};
    const double split[3] = {0.75, 0.0, 0.0}, xbar[3] = {0.0, 0.25, 0.0};
    const double value[9] = {0.0, 0.0, 0.0, -1.0, -2.0, -3.0, 4.0, 5.0, 6.0};
    const double slope[9] = {0.0, 0.0, 0.0, 0.5, 1.5, 2.5, 0.0, 0.0, 0.0};
    Flat im, ar;
    write_nodes(ht, node_sink(im.view()));
    pgb_tree_arrays a = ar.arrays(true);
    write_nodes(ht, node_sink(&a));
    check(same(im.node_off, node_off) && same(im.var, var) && same(im.left, left) && same(im.right, right) &&
              same(im.depth, depth) && same(im.label, label) && same(im.svar, svar) && same(im.count, count) &&
              same(im.split, split) && same(im.xbar, xbar) && same(im.value, value) && same(im.slope, slope),
          "trees K = 3: the image's node arrays");
    check(same(ar.node_off, node_off) && same(ar.var, var) && same(ar.left, left) && same(ar.right, right) &&
              same(ar.svar, svar) && same(ar.count, count) && same(ar.split, split) && same(ar.xbar, xbar) &&
              same(ar.value, value) && same(ar.slope, slope),
          "trees K = 3: pgb_tree_arrays");
    check(memcmp(im.value, ar.value, sizeof im.value) == 0 && memcmp(im.slope, ar.slope, sizeof im.slope) == 0 &&
              memcmp(im.xbar, ar.xbar, sizeof im.xbar) == 0 && memcmp(im.svar, ar.svar, sizeof im.svar) == 0 &&
              memcmp(im.var, ar.var, sizeof im.var) == 0 && memcmp(im.count, ar.count, sizeof im.count) == 0,
          "trees K = 3: the two sinks agree");
    ht.lin.clear();  // a caller that takes no slopes fetches no linear part
    Flat ar0;
    pgb_tree_arrays a0 = ar0.arrays(false);
    write_nodes(ht, node_sink(&a0));
    check(same(ar0.value, value) && ar0.slope[0] != 0.0 && ar0.svar[1] == 0x5a5a5a5a, "trees K = 3: values alone");
  }
  printf("%-4s write_nodes: two forests, both sinks\n", g_bad ? "..." : "ok");
}

// ---- ProgressWatch over a host word (PGB_WATCHDOG_S = 0.1, set in main before its first reading)
static void progress_watch() {
  typedef std::chrono::steady_clock clock;
  const auto seconds_since = [](clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); };
  unsigned long long words[8] = {0};
  pgb_handle* h = new pgb_handle();
  h->flag = words;
  check(watchdog_seconds() == 0.1, "watch: PGB_WATCHDOG_S = 0.1");
  ProgressWatch watch(h, "the caller's sentence for a lost device", "the caller's sentence for a stuck one");
  int rc = PGB_OK;
  const auto t0 = clock::now();
  while (rc == PGB_OK && seconds_since(t0) < 0.45) {  // several deadlines' worth of a word that keeps moving
    for (int i = 0; i < 0x1000 && rc == PGB_OK; ++i) rc = watch.poll();
    words[2] += 1;
  }
  expect("watch: a moving word never expires", rc, PGB_OK, nullptr);
  check(h->poisoned == 0, "watch: ... and leaves the handle alone");
  const auto t1 = clock::now();
  while (rc == PGB_OK && seconds_since(t1) < 5.0) rc = watch.poll();  // the word has stopped
  const double waited = seconds_since(t1);
  // (a stream in error -- no device here -- or a healthy one: either of the caller's two sentences)
  if (rc == PGB_E_DEVICE) expect("watch: expired, stream in error", rc, PGB_E_DEVICE, "the caller's sentence for a lost device: ");
  else expect("watch: expired, stream healthy", rc, PGB_E_STATE, "the caller's sentence for a stuck one");
  check(h->poisoned == 1, "watch: expiry poisons the handle");
  // (the deadline was last moved within one look at the clock -- 0x4000 polls -- before the word stopped)
  check(waited > 0.09 && waited < 2.0, "watch: expiry comes one deadline after the word stopped");
  (void)hipGetLastError();
  delete h;
}

int main() {
  setenv("PGB_WATCHDOG_S", "0.1", 1);
  create_refusals();
  slot_kernel_choices();
  host_trees();
  progress_watch();
  printf("%d unexpected\n", g_bad);
  return g_bad ? 1 : 0;
}
