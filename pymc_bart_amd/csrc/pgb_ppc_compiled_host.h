// pgb_ppc_compiled_host.h -- part of pgbart_hip.hip (not a standalone header): host side of pgb_ppc_draw_compiled
// (include/pgbart_ppc.h), the replicating call with a compiled likelihood's sampler body.  It shares the argument rules,
// the grid and the launch sequence of pgb_ppc_draw (k_ppc.h: ppc_check_shape, ppc_check_ranges, ppc_run) and the
// loader of every compiled code object (pgb_compiled_host.h: compiled_load_code, here with mark 2); the kernel
// is the code object's k_ppc_compiled (k_ppc_compiled.hip).  Everything is checked before the launch.

extern "C" int pgb_ppc_draw_compiled(const double* mu_dev, int32_t D, int32_t K, int64_t n_rows, int64_t ld, int64_t row0,
                                     const pgb_ppc_code* code, uint64_t seed, double* out_dev, int64_t ld_out,
                                     const double* y_dev, int32_t* pit_counts_dev, int64_t* flags_host, void* stream) {
  int rc = ppc_check_shape(mu_dev, code, flags_host, out_dev, y_dev, pit_counts_dev, D, n_rows, ld, ld_out, row0);
  if (rc != PGB_OK) return rc;
  if (K < 1 || K > PGB_MAX_OUTPUTS) {
    snprintf(g_err, sizeof g_err, "K must be in [1, %d], got %d", PGB_MAX_OUTPUTS, (int)K);
    return PGB_E_INVALID;
  }
  if (code->n_params < 0 || code->n_params > PGB_COMPILED_MAX_PARAMS)
    return fail(PGB_E_INVALID, "n_params must be in [0, " PGB_STR(PGB_COMPILED_MAX_PARAMS) "]");
  if (code->n_params > 0 && !code->params_host) return fail(PGB_E_INVALID, "params_host is null");
  dim3 grid;
  rc = ppc_check_ranges(mu_dev, D, K, n_rows, ld, out_dev, ld_out, &grid);
  if (rc != PGB_OK) return rc;
  PpcScratch sc;
  hipFunction_t fn = nullptr;
  pgb_compiled_layout rec;
  rc = compiled_load_code(code->code_object, code->code_bytes, code->n_params, K, "the call has K", PGB_COMPILED_MARK_SAMPLER,
                          "pgb_ppc_draw_compiled", &sc.mod, &fn, &rec);
  if (rc != PGB_OK) return rc;
  std::vector<double> hp((size_t)D * PGB_COMPILED_MAX_PARAMS, 0.0);
  int bad_d = 0, bad_i = 0;
  if (!compiled_params_table(code->params_host, D, code->n_params, hp.data(), &bad_d, &bad_i)) {
    snprintf(g_err, sizeof g_err, "the sampler body's params must be finite: param %d of draw %d is not", bad_i, bad_d);
    return PGB_E_INVALID;
  }
  hipStream_t sm = (hipStream_t)stream;
  return ppc_run(sc, hp, mu_dev, D, K, n_rows, ld, row0, code->offset_dev, code->aux_dev, PGB_FAMILY_COMPILED, seed, out_dev,
                 ld_out, y_dev, pit_counts_dev, flags_host, sm, PGB_PPC_COMPILED_KERNEL, [&](const PpcArgs& A) {
                   PpcArgs Ac = A;
                   void* args[] = {(void*)&Ac};
                   return hipModuleLaunchKernel(fn, grid.x, grid.y, 1, PPC_BT, 1, 1, 0, sm, args, nullptr);
                 });
}
