// pgb_pointwise_host.h -- part of pgbart_hip.hip (not a standalone header): host side of pgb_pointwise_loglik
// (include/pgbart_pointwise.h).  Handle-free like pgb_predict, whose history validation and node packing it shares
// (pred_validate, pred_pack: pgb_pred_host.h).  Everything is checked before the walk kernel is launched.

// every device buffer of one call next to the packed trees, released on every way out
struct PwScratch {
  double* params = nullptr;     // [n_forests][PGB_PW_PSTRIDE]
  double* partial = nullptr;    // [n_chunks][4][n_rows]
  unsigned long long* words = nullptr;  // [0] clamp count, [1] non-finite y / aux, [2] offset beyond the limit
  hipModule_t mod = nullptr;
  ~PwScratch() {
    if (params) (void)hipFree(params);
    if (partial) (void)hipFree(partial);
    if (words) (void)hipFree(words);
    if (mod) (void)hipModuleUnload(mod);
  }
};

extern "C" int pgb_pointwise_loglik(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests,
                                    int32_t m, const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx,
                                    const pgb_pointwise_lik* lik, double* loglik_dev_out, double* row_stats_dev_out,
                                    int64_t* n_clamped_out, void* stream) {
  if (!trees || !forest_tree_idx || !X_dev || !lik || !lik->y_dev) return fail(PGB_E_INVALID, "null argument");
  if (!loglik_dev_out && !row_stats_dev_out) return fail(PGB_E_INVALID, "no output: give loglik_dev_out, row_stats_dev_out or both");
  if (n_forests < 1 || n_rows < 1 || m < 1 || p < 1 || ldx < p) return fail(PGB_E_INVALID, "n_forests, n_rows, m, p must be >= 1 and ldx >= p");
  const int K = trees->n_outputs;
  if (K < 1 || K > PGB_MAX_OUTPUTS) return fail(PGB_E_INVALID, "n_outputs");
  // ---- the likelihood
  const bool compiled = lik->family == PGB_FAMILY_COMPILED;
  if (lik->family == PGB_FAMILY_CALLBACK)
    return fail(PGB_E_INVALID, "the callback family has no device density: pgb_pointwise_loglik takes the built-in families "
                               "and compiled bodies");
  if (!compiled) {
    const int np = pgb_logpdf_nparams(lik->family);
    if (np < 0) return fail(PGB_E_INVALID, "unknown family");
    if (lik->n_params != np) {
      snprintf(g_err, sizeof g_err, "family %d takes %d params per draw, %d given", (int)lik->family, np, (int)lik->n_params);
      return PGB_E_INVALID;
    }
    const int ko = pgb_logpdf_outputs(lik->family);
    if ((ko > 0 && K != ko) || (ko == 0 && K < 2)) {
      snprintf(g_err, sizeof g_err, "family %d does not take the trees' n_outputs = %d", (int)lik->family, K);
      return PGB_E_INVALID;
    }
  } else if (lik->n_params < 0 || lik->n_params > PGB_COMPILED_MAX_PARAMS) {
    return fail(PGB_E_INVALID, "n_params must be in [0, " PGB_STR(PGB_COMPILED_MAX_PARAMS) "]");
  }
  if (lik->n_params > 0 && !lik->params_host) return fail(PGB_E_INVALID, "params_host is null");
  std::vector<double> hp((size_t)n_forests * PGB_PW_PSTRIDE, 0.0);
  const pgb_lltabs htb = pgb_lltabs_default();
  int bad_d = 0, bad_i = 0;
  if (compiled && !compiled_params_table(lik->params_host, n_forests, lik->n_params, hp.data(), &bad_d, &bad_i))
    return fail(PGB_E_INVALID, "the compiled likelihood's params must be finite");
  for (int d = 0; d < n_forests && !compiled; ++d)
    if (pgb_logpdf_prepare(lik->family, lik->params_host + (size_t)d * lik->n_params,
                           hp.data() + (size_t)d * PGB_PW_PSTRIDE, &htb) != 0) {
      snprintf(g_err, sizeof g_err, "the params of draw %d are outside family %d's domain (positive and finite; 0 < q < 1)",
               d, (int)lik->family);
      return PGB_E_INVALID;
    }
  // ---- the history
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;
  hipStream_t sm = (hipStream_t)stream;
  PwScratch sc;
  hipFunction_t fn = nullptr;
  pgb_compiled_layout rec;
  if (compiled) {
    rc = compiled_load_code(lik->code_object, lik->code_bytes, lik->n_params, K, "the trees have n_outputs",
                            PGB_COMPILED_MARK_POINTWISE, "pgb_pointwise_loglik", &sc.mod, &fn, &rec);
    if (rc != PGB_OK) return rc;
  }
  // ---- the rows' columns: finite y / aux, a bounded offset (the tables are addressed by the predictor's bits)
  HIPCHK(hipMalloc((void**)&sc.words, 3 * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(sc.words, 0, 3 * sizeof(unsigned long long), sm));
  hipLaunchKernelGGL(k_nonfinite, dim3(256), dim3(BT), 0, sm, lik->y_dev, (long long)n_rows, (long long)n_rows, 1,
                     __builtin_inf(), sc.words + 1);
  if (lik->aux_dev)
    hipLaunchKernelGGL(k_nonfinite, dim3(256), dim3(BT), 0, sm, lik->aux_dev, (long long)n_rows, (long long)n_rows, 1,
                       __builtin_inf(), sc.words + 1);
  if (lik->offset_dev)
    hipLaunchKernelGGL(k_nonfinite, dim3(256), dim3(BT), 0, sm, lik->offset_dev, (long long)n_rows, (long long)n_rows, K,
                       (double)PGB_MAX_OFFSET, sc.words + 2);
  unsigned long long hw[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(hw, sc.words, sizeof hw, hipMemcpyDeviceToHost, sm));
  HIPCHK(hipStreamSynchronize(sm));
  if (hw[1]) return fail(PGB_E_INVALID, "y (or aux) has non-finite values");
  if (hw[2]) return fail(PGB_E_INVALID, "the offset has non-finite values or values beyond PGB_MAX_OFFSET");
  // ---- uploads
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);
  if (rc != PGB_OK) return rc;
  HIPCHK(hipMalloc((void**)&sc.params, hp.size() * sizeof(double)));
  HIPCHK(hipMemcpyAsync(sc.params, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, sm));
  const int n_chunks = (n_forests + PGB_PW_CHUNK - 1) / PGB_PW_CHUNK;
  if (row_stats_dev_out) HIPCHK(hipMalloc((void**)&sc.partial, (size_t)n_chunks * 4 * (size_t)n_rows * sizeof(double)));
  PwArgs A;
  A.params = sc.params;
  A.y = lik->y_dev;
  A.offset = lik->offset_dev;
  A.aux = compiled ? lik->aux_dev : nullptr;
  A.out = loglik_dev_out;
  A.partial = sc.partial;
  A.n_clamped = sc.words;
  A.family = lik->family;
  // one wave per workgroup; the y dimension is dealt whole chunks of draws
  const long long gx = (n_rows + PRED_BT - 1) / PRED_BT;
  long long want_wgs = p <= PRED_LDS_MAXP ? 16384 : 4096;  // (k_predict's)
  if (const char* ev = getenv("PGB_PW_WGS")) want_wgs = atoll(ev) > 0 ? atoll(ev) : want_wgs;
  long long gy = (want_wgs + gx - 1) / gx;
  if (gy > n_chunks) gy = n_chunks;
  if (gy < 1) gy = 1;
  dim3 grid((unsigned)gx, (unsigned)gy);
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  const PredTrees T = pk.T;
  if (compiled) {
    const int32_t* fi = pk.fidx;
    int nf = n_forests, mm = m, kk = K, pp = p, mode = (ldsx ? 1 : 0) | (pk.cont ? 2 : 0);
    long long nr = n_rows, ld = ldx;
    PredTrees Tc = T;
    void* args[] = {(void*)&Tc, (void*)&fi, (void*)&nf, (void*)&mm, (void*)&kk, (void*)&pp, (void*)&X_dev,
                    (void*)&nr, (void*)&ld, (void*)&A, (void*)&mode};
    HIPCHK(hipModuleLaunchKernel(fn, grid.x, grid.y, 1, PRED_BT, 1, 1, (unsigned)lds, sm, args, nullptr));
  } else {
    dispatch_bools(ldsx, pk.cont, K == 1, [&](auto L, auto C, auto K1) {
      hipLaunchKernelGGL((k_pointwise<L(), C(), K1()>), grid, dim3(PRED_BT), lds, sm, T, pk.fidx, n_forests, m, K, (int)p,
                         X_dev, (long long)n_rows, (long long)ldx, A);
    });
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_pointwise launch");
  if (row_stats_dev_out) {
    hipLaunchKernelGGL(k_pointwise_merge, dim3((unsigned)((n_rows + BT - 1) / BT)), dim3(BT), 0, sm,
                       (const double*)sc.partial, n_forests, (long long)n_rows, row_stats_dev_out);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "k_pointwise_merge launch");
  }
  HIPCHK(hipMemcpyAsync(hw, sc.words, sizeof(unsigned long long), hipMemcpyDeviceToHost, sm));
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_pointwise");
  if (n_clamped_out) *n_clamped_out = (int64_t)hw[0];
  return PGB_OK;
}
