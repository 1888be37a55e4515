// pgb_compiled_host.h -- part of pgbart_hip.hip (not a standalone header): host side of the compiled likelihood family
// (include/pgbart_compiled.h): loading and checking a code object built from k_loglik_compiled.hip, its params,
// its aux column, its launch.  Included by pgb_host.h after the launch helpers.
#ifndef PGB_HEADERS_HASH
#define PGB_HEADERS_HASH 0ull  // (a build without the hash -- __graft_entry__.build passes it -- refuses every code object)
#endif

// The resident grid of the loaded kernel, as pgb_create sizes it for the built-in instances (size_ll_grid).
static void compiled_size_grid(pgb_handle* h) {
  int per_cu = 0;
  if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->cl_fn, BT, 0) == hipSuccess) size_ll_grid(h, per_cu);
}

extern "C" int pgb_set_loglik_code(pgb_handle* h, const void* code_object, int64_t bytes, int32_t n_params) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  if (h->s.family != PGB_FAMILY_COMPILED)
    return fail(PGB_E_INVALID, "the sampler was not created with the compiled family");
  if (!code_object || bytes < 64) return fail(PGB_E_INVALID, "no code object");
  if (n_params < 0 || n_params > PGB_COMPILED_MAX_PARAMS)
    return fail(PGB_E_INVALID, "n_params must be in [0, " PGB_STR(PGB_COMPILED_MAX_PARAMS) "]");
  // only an ELF object goes to the loader (the runtime parses what it is given; anything else is refused here)
  const unsigned char* b = (const unsigned char*)code_object;
  if (!(b[0] == 0x7f && b[1] == 'E' && b[2] == 'L' && b[3] == 'F'))
    return fail(PGB_E_INVALID, "not a gfx950 code object (no ELF header): compile it with pymc_bart_amd.compiled");
  hipModule_t mod = nullptr;
  hipError_t e = hipModuleLoadData(&mod, code_object);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    snprintf(g_err, sizeof g_err, "the code object does not load: %s", hipGetErrorString(e));
    return PGB_E_INVALID;
  }
  // the layout record: read, never launched
  const char* why = nullptr;
  char why_k[128];
  pgb_compiled_layout rec;
  memset(&rec, 0, sizeof rec);
  hipDeviceptr_t gp = nullptr;
  size_t gbytes = 0;
  if (hipModuleGetGlobal(&gp, &gbytes, mod, PGB_COMPILED_LAYOUT) != hipSuccess || gbytes != sizeof rec)
    why = "the code object has no layout record " PGB_COMPILED_LAYOUT;
  else if (hipMemcpyDtoH(&rec, gp, sizeof rec) != hipSuccess)
    why = "the layout record could not be read";
  else if (rec.magic != PGB_COMPILED_MAGIC)
    why = "the layout record is not one of a compiled likelihood";
  else if (rec.pointwise == PGB_COMPILED_MARK_SAMPLER)
    why = "the code object is one built from a sampler body (" PGB_PPC_COMPILED_KERNEL ", mark 2): pgb_set_loglik_code "
          "takes a sampler's pass kernel";
  else if (rec.max_particles != PGB_MAX_PARTICLES)
    why = PGB_MAX_PARTICLES == 64 ? "the code object was built for another particle build (this library takes 64)"
                                  : "the code object was built for another particle build (this library takes 128)";
  else if (rec.sizeof_dev != (int64_t)sizeof(Dev) || rec.sizeof_job != (int64_t)sizeof(Job) ||
           rec.sizeof_cmd != (int64_t)sizeof(Cmd) || rec.sizeof_ctrl != (int64_t)sizeof(Ctrl) ||
           rec.sizeof_acc != (int64_t)sizeof(Acc))
    why = "the code object's device records differ from this library's";
  else if (PGB_HEADERS_HASH == 0ull || rec.headers_hash != (uint64_t)PGB_HEADERS_HASH)
    why = "the code object was compiled from other kernel headers than this library";
  else if (rec.n_params != n_params)
    why = "n_params differs from the params the code object was compiled for";
  else if (rec.n_outputs != h->s.n_outputs) {
    snprintf(why_k, sizeof why_k, "the code object was compiled for %d outputs, the sampler has n_outputs = %d",
             (int)rec.n_outputs, (int)h->s.n_outputs);
    why = why_k;
  } else if ((rec.linear_leaves != 0) != (h->s.response != PGB_RESPONSE_CONSTANT) ||
             (rec.linear_leaves != 0 && rec.linear_leaves != 1)) {
    const char* resp = h->s.response == PGB_RESPONSE_CONSTANT ? "constant"
                       : h->s.response == PGB_RESPONSE_LINEAR ? "linear" : "mix";
    snprintf(why_k, sizeof why_k, "the code object was compiled for %s leaves, the sampler has response = %s",
             rec.linear_leaves == 0 ? "constant" : rec.linear_leaves == 1 ? "linear" : "unknown", resp);
    why = why_k;
  }
  hipFunction_t fn = nullptr, probe = nullptr;
  if (!why && hipModuleGetFunction(&fn, mod, PGB_COMPILED_KERNEL) != hipSuccess)
    why = "the code object has no kernel " PGB_COMPILED_KERNEL;
  if (!why && hipModuleGetFunction(&probe, mod, PGB_COMPILED_PROBE) != hipSuccess)
    why = "the code object has no kernel " PGB_COMPILED_PROBE;
  if (why) {
    (void)hipGetLastError();
    (void)hipModuleUnload(mod);
    return fail(PGB_E_INVALID, why);
  }
  // replace the old module: nothing queued may still run it
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->cl_module) (void)hipModuleUnload(h->cl_module);
  h->cl_module = mod;
  h->cl_fn = fn;
  h->cl_probe = probe;
  if (h->cl_nparams != n_params) memset(&h->cl_prm, 0, sizeof h->cl_prm);
  h->cl_nparams = n_params;
  compiled_size_grid(h);
  HIPCHK(hipMemcpyAsync(h->d_dev, &h->d, sizeof(Dev), hipMemcpyHostToDevice, h->stream));  // (ll_target)
  HIPCHK(hipStreamSynchronize(h->stream));
  return PGB_OK;
}

extern "C" int pgb_set_loglik_aux(pgb_handle* h, const double* aux_dev) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  if (h->s.family != PGB_FAMILY_COMPILED)
    return fail(PGB_E_INVALID, "the sampler was not created with the compiled family");
  h->out_valid = 0;
  Dev& d = h->d;
  if (!aux_dev) {
    HIPCHK(hipMemsetAsync(h->cl_aux, 0, d.n_pad * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PGB_OK;
  }
  HIPCHK(hipMemcpyAsync(h->cl_aux, aux_dev, d.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  h->flag[4] = 0;
  hipLaunchKernelGGL(k_nonfinite, dim3(256), dim3(BT), 0, h->stream, (const double*)h->cl_aux, (long long)d.n,
                     (long long)d.n_pad, 1, __builtin_inf(), d.host_flag + 4);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->flag[4]) {  // (cleared: the chain stays usable)
    HIPCHK(hipMemsetAsync(h->cl_aux, 0, d.n_pad * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return fail(PGB_E_INVALID, "the aux column has non-finite values");
  }
  return PGB_OK;
}

extern "C" int pgb_compiled_probe(pgb_handle* h, const double* y, const double* mu, const double* aux, int64_t n,
                                  double* out) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  if (h->s.family != PGB_FAMILY_COMPILED)
    return fail(PGB_E_INVALID, "the sampler was not created with the compiled family");
  if (!h->cl_probe) return fail(PGB_E_INVALID, "pgb_set_loglik_code first");
  if (n < 0) return fail(PGB_E_INVALID, "n must be >= 0");
  if (n == 0) return PGB_OK;
  if (!y || !mu || !out) return fail(PGB_E_INVALID, "null argument");
  long long nn = (long long)n;
  pgb_compiled_params prm = h->cl_prm;
  void* args[] = {(void*)&y, (void*)&mu, (void*)&aux, (void*)&nn, (void*)&prm, (void*)&out};
  long long g = (nn + BT - 1) / BT;
  if (g > 4096) g = 4096;  // (a grid-stride loop covers the rest)
  HIPCHK(hipModuleLaunchKernel(h->cl_probe, (unsigned)g, 1, 1, BT, 1, 1, 0, h->stream, args, nullptr));
  HIPCHK(hipStreamSynchronize(h->stream));
  return PGB_OK;
}

// pgb_set_likelihood of the compiled family: exactly the declared params, finite; they travel by value with the
// launches enqueued from here on (the next astep's slots, in stream order)
static int compiled_set_params(pgb_handle* h, const double* params, int32_t n_params) {
  if (h->cl_nparams < 0) return fail(PGB_E_INVALID, "pgb_set_loglik_code first (it declares the params)");
  if (n_params != h->cl_nparams) {
    snprintf(g_err, sizeof g_err, "the compiled likelihood takes %d params, %d given", h->cl_nparams, (int)n_params);
    return PGB_E_INVALID;
  }
  for (int i = 0; i < n_params; ++i)
    if (!(params[i] - params[i] == 0.0)) return fail(PGB_E_INVALID, "the compiled likelihood's params must be finite");
  for (int i = 0; i < n_params; ++i) h->cl_prm.v[i] = params[i];
  return PGB_OK;
}

// the log-likelihood pass of one slot: the module kernel, on the library's grid; hipExtModuleLaunchKernel (global
// size in THREADS) with the profiling events, so that pgb_profile_kernel reports it in the k_loglik slot
static int compiled_launch(pgb_handle* h, int par, int nwg) {
  Dev& d = h->d;
  const Dev* dd = (const Dev*)h->d_dev;
  const Cmd* cmds = (const Cmd*)d.cmd;
  const Ctrl* ctrls = (const Ctrl*)d.ctrl;
  const Job* jobs = (const Job*)d.jobs;
  const Acc* acc = (const Acc*)d.acc;
  const InitAcc* ias = (const InitAcc*)d.initacc;
  const double* aux = h->cl_aux;
  pgb_compiled_params prm = h->cl_prm;
  void* args[] = {(void*)&dd, (void*)&par, (void*)&nwg, (void*)&cmds, (void*)&ctrls, (void*)&jobs,
                  (void*)&acc, (void*)&ias, (void*)&aux, (void*)&prm};
  hipEvent_t e0, e1;
  const int rc = prof_events(h, PK_LL, &e0, &e1);
  if (rc != PGB_OK) return rc;
  h->prof_wgs[PK_LL] = nwg;
  if (h->prof)
    HIPCHK(hipExtModuleLaunchKernel(h->cl_fn, (uint32_t)nwg * BT, 1, 1, BT, 1, 1, 0, h->stream, args, nullptr, e0, e1, 0));
  else
    HIPCHK(hipModuleLaunchKernel(h->cl_fn, (unsigned)nwg, 1, 1, BT, 1, 1, 0, h->stream, args, nullptr));
  return PGB_OK;
}
