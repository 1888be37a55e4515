// pred_host_sanitize.hip -- the host front end of the stored-draw entry points (csrc/pgb_pred_host.h and its callers)
// under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program on the build box, no GPU needed.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ipymc_bart_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         tools/pred_host_sanitize.hip -o build/pred_host_sanitize && build/pred_host_sanitize
//
// Every call is refused by a check that precedes the entry point's first HIP call; the last one of each entry point
// passes them all and -- where no device answers -- fails in pred_pack's upload, the way out that releases an empty
// PredPack.  Exit status 0: every refusal carried the sentence expected here and the sanitizers saw nothing.
#define PGB_HEADERS_HASH 0ull
#include "pgbart_hip.hip"

static int g_bad = 0;
static void expect(const char* what, int rc, int want_rc, const char* sentence) {
  const char* msg = pgb_last_error();
  const bool ok = rc == want_rc && (!sentence || strstr(msg, sentence));
  printf("%-4s %-64s rc = %d  %s\n", ok ? "ok" : "BAD", what, rc, rc == PGB_OK ? "" : msg);
  if (!ok) ++g_bad;
}

int main() {
  // one forest of two trees: a stump on column 0 and a lone leaf
  int32_t tree_id[2] = {0, 1}, node_off[3] = {0, 3, 4}, var[4] = {0, -1, -1, -1};
  int32_t left[4] = {1, -1, -1, -1}, right[4] = {2, -1, -1, -1};
  double split[4] = {0.5, 0, 0, 0}, value[4] = {0, -1.0, 1.0, 0.25};
  int64_t count[4] = {10, 4, 6, 10};
  pgb_tree_arrays T;
  memset(&T, 0, sizeof T);
  T.n_trees = 2, T.n_outputs = 1, T.total_nodes = 4;
  T.tree_id = tree_id, T.node_off = node_off, T.var = var, T.split = split, T.left = left, T.right = right;
  T.count = count, T.value = value;
  const int32_t fidx[4] = {0, 1, 1, 0};  // n_forests = 2, m = 2
  static double dev[64];                 // stands in for device memory: never dereferenced on the host
  double base[4];
  int32_t cols[2] = {0, 1}, picks[8] = {0, 1, 0, 1, 0, 1, 0, 1}, taken[2];
  const int32_t cols_twice[2] = {1, 1}, cols_past[2] = {0, 2}, picks_past[8] = {0, 1, 0, 1, 0, 1, 0, 2};
  const int I = PGB_E_INVALID;
  pgb_pointwise_lik lik;
  memset(&lik, 0, sizeof lik);
  lik.family = PGB_FAMILY_CALLBACK, lik.y_dev = dev;

  expect("predict: null", pgb_predict(nullptr, fidx, 2, 2, dev, 8, 2, 2, nullptr, 0, dev, nullptr), I, "null argument");
  expect("predict: ldx", pgb_predict(&T, fidx, 2, 2, dev, 8, 2, 1, nullptr, 0, dev, nullptr), I, "pgb_predict: ldx must be >= p");
  expect("predict: no rows", pgb_predict(&T, fidx, 2, 2, dev, 0, 2, 2, nullptr, 0, dev, nullptr), PGB_OK, nullptr);
  expect("predict: a column X lacks", pgb_predict(&T, fidx, 2, 2, dev, 8, 0, 0, nullptr, 0, dev, nullptr), I, "column X does not have");

  expect("pointwise: null", pgb_pointwise_loglik(&T, fidx, 2, 2, dev, 8, 2, 2, nullptr, dev, nullptr, nullptr, nullptr), I, "null argument");
  expect("pointwise: ldx", pgb_pointwise_loglik(&T, fidx, 2, 2, dev, 8, 2, 1, &lik, dev, nullptr, nullptr, nullptr), I, "ldx >= p");
  expect("pointwise: callback family", pgb_pointwise_loglik(&T, fidx, 2, 2, dev, 8, 2, 2, &lik, dev, nullptr, nullptr, nullptr), I,
         "callback family");

  expect("ice: null", pgb_predict_ice(&T, fidx, 2, 2, dev, 8, 2, 2, nullptr, 2, 2, cols, 2, picks, 2, dev, nullptr), I,
         "pgb_predict_ice: inst_dev is null");
  expect("ice: ldi", pgb_predict_ice(&T, fidx, 2, 2, dev, 8, 2, 2, dev, 2, 1, cols, 2, picks, 2, dev, nullptr), I,
         "pgb_predict_ice: ldi must be >= p");
  expect("ice: cols past the end", pgb_predict_ice(&T, fidx, 2, 2, dev, 8, 2, 2, dev, 2, 2, cols_past, 2, picks, 2, dev, nullptr), I,
         "pgb_predict_ice: cols_host[1] = 2 is outside [0, p = 2)");
  expect("ice: picks past the end", pgb_predict_ice(&T, fidx, 2, 2, dev, 8, 2, 2, dev, 2, 2, cols, 2, picks_past, 2, dev, nullptr), I,
         "pgb_predict_ice: picks_host[7] = 2 is outside [0, n_forests = 2)");
  expect("ice: tiles", pgb_predict_ice(&T, fidx, 2, 2, dev, (int64_t)1 << 38, 2, 2, dev, 2, 2, cols, 2, picks, 2, dev, nullptr), I,
         "n_rows exceeds 2^31 - 1 tiles of 64 rows");

  expect("pdp: route", pgb_predict_pdp(&T, fidx, 2, 2, dev, 8, 2, 2, cols, 2, picks, 2, 3, dev, taken, nullptr), I,
         "pgb_predict_pdp: route must be 0 (auto), 1 (direct) or 2 (profile)");
  expect("pdp: n_picks", pgb_predict_pdp(&T, fidx, 2, 2, dev, 8, 2, 2, cols, 2, picks, 0, 0, dev, taken, nullptr), I,
         "pgb_predict_pdp: n_picks must be >= 1");
  expect("pdp: picks past the end", pgb_predict_pdp(&T, fidx, 2, 2, dev, 8, 2, 2, cols, 2, picks_past + 4, 2, 0, dev, taken, nullptr), I,
         "pgb_predict_pdp: picks_host[3] = 2 is outside [0, n_forests = 2)");

  expect("shap: p", pgb_predict_shap(&T, fidx, 2, 2, dev, 8, 0, 2, picks, 2, dev, base, nullptr), I,
         "pgb_predict_shap: n_forests, m and p must be >= 1");
  expect("shap: picks past the end", pgb_predict_shap(&T, fidx, 2, 2, dev, 8, 2, 2, picks_past + 6, 2, dev, base, nullptr), I,
         "pgb_predict_shap: picks_host[1] = 2 is outside [0, n_forests = 2)");
  expect("shap: cells", pgb_predict_shap(&T, fidx, 2, 2, dev, (int64_t)1 << 36, 1 << 24, 1 << 24, picks, 2, dev, base, nullptr), I,
         "pgb_predict_shap: out_dev of n_picks x K x p x n_rows doubles overflows a 64-bit size");
  T.n_outputs = 0;
  expect("shap: n_outputs", pgb_predict_shap(&T, fidx, 2, 2, dev, 8, 2, 2, picks, 2, dev, base, nullptr), I, "n_outputs");
  T.n_outputs = 1;

  expect("shap interactions: a column twice",
         pgb_predict_shap_interactions(&T, fidx, 2, 2, dev, 8, 2, 2, cols_twice, 2, picks, 2, dev, base, nullptr), I,
         "pgb_predict_shap_interactions: cols_host[1] = 1 repeats cols_host[0]");
  expect("shap interactions: cols past the end",
         pgb_predict_shap_interactions(&T, fidx, 2, 2, dev, 8, 2, 2, cols_past, 2, picks, 2, dev, base, nullptr), I,
         "pgb_predict_shap_interactions: cols_host[1] = 2 is outside [0, p = 2)");
  right[0] = 0;  // the root is its own child
  expect("shap interactions: not a tree",
         pgb_predict_shap_interactions(&T, fidx, 2, 2, dev, 8, 2, 2, cols, 2, picks, 2, dev, base, nullptr), I, "do not form a tree");
  right[0] = 2;

  // every check passed: without a device the upload fails and an empty PredPack is released
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
    (void)hipGetLastError();
    const int D = PGB_E_DEVICE;
    expect("predict: no device", pgb_predict(&T, fidx, 2, 2, dev, 8, 2, 2, nullptr, 0, dev, nullptr), D, "hipMalloc");
    expect("ice: no device", pgb_predict_ice(&T, fidx, 2, 2, dev, 8, 2, 2, dev, 2, 2, cols, 2, picks, 2, dev, nullptr), D, "hipMalloc");
    expect("pdp: no device", pgb_predict_pdp(&T, fidx, 2, 2, dev, 8, 2, 2, cols, 2, picks, 2, 0, dev, taken, nullptr), D, "hipMalloc");
    expect("shap: no device", pgb_predict_shap(&T, fidx, 2, 2, dev, 8, 2, 2, picks, 2, dev, base, nullptr), D, "hipMalloc");
    expect("shap interactions: no device",
           pgb_predict_shap_interactions(&T, fidx, 2, 2, dev, 8, 2, 2, cols, 2, picks, 2, dev, base, nullptr), D, "hipMalloc");
  }
  printf("%d unexpected\n", g_bad);
  return g_bad ? 1 : 0;
}
