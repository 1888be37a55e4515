// pgb_compiled_host.h -- part of pgbart_hip.hip (not a standalone header): host side of the compiled likelihood family
// (include/pgbart_compiled.h): the one loader of a compiled code object of any kind (compiled_load_code; its callers
// pgb_set_loglik_code here, pgb_pointwise_loglik, pgb_ppc_draw_compiled), and a pass object's params, aux column and
// launch.  Included by pgb_host.h after the launch helpers.
#ifndef PGB_HEADERS_HASH
#define PGB_HEADERS_HASH 0ull  // (a build without the hash -- __graft_entry__.build passes it -- refuses every code object)
#endif

// The resident grid of the loaded kernel, as pgb_create sizes it for the built-in instances (size_ll_grid).
static void compiled_size_grid(pgb_handle* h) {
  int per_cu = 0;
  if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->cl_fn, BT, 0) == hipSuccess) size_ll_grid(h, per_cu);
}

// what a layout record's mark says the code object is (the words follow "one")
static const char* compiled_mark_name(int mark) {
  return mark == PGB_COMPILED_MARK_PASS        ? "built without pointwise=True (a sampler's pass kernel, " PGB_COMPILED_KERNEL ")"
         : mark == PGB_COMPILED_MARK_POINTWISE ? "built with pointwise=True (" PGB_POINTWISE_KERNEL ")"
         : mark == PGB_COMPILED_MARK_SAMPLER   ? "built from a sampler body (" PGB_PPC_COMPILED_KERNEL ")"
                                               : "of an unknown kind";
}

// The ONE loader of a compiled body's code object, for `entry` (pgb_set_loglik_code: mark 0, pgb_pointwise_loglik:
// mark 1, pgb_ppc_draw_compiled: mark 2): loaded into *mod (the caller unloads it, on every way out), its layout
// record -- left in *rec -- held against the call's, the mark's kernel looked up; never launched when they differ
// (the message names both sides).  k_side: how the call's K reads in a message.
static int compiled_load_code(const void* code_object, int64_t code_bytes, int n_params, int K, const char* k_side,
                              int want_mark, const char* entry, hipModule_t* mod, hipFunction_t* fn,
                              pgb_compiled_layout* rec) {
  if (!code_object || code_bytes < 64) return fail(PGB_E_INVALID, "the compiled family needs a code object");
  // only an ELF object goes to the loader (the runtime parses what it is given; anything else is refused here)
  const unsigned char* b = (const unsigned char*)code_object;
  if (!(b[0] == 0x7f && b[1] == 'E' && b[2] == 'L' && b[3] == 'F'))
    return fail(PGB_E_INVALID, "not a gfx950 code object (no ELF header): compile it with pymc_bart_amd.compiled");
  hipError_t e = hipModuleLoadData(mod, code_object);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *mod = nullptr;
    snprintf(g_err, sizeof g_err, "the code object does not load: %s", hipGetErrorString(e));
    return PGB_E_INVALID;
  }
  memset(rec, 0, sizeof *rec);
  hipDeviceptr_t gp = nullptr;
  size_t gbytes = 0;
  if (hipModuleGetGlobal(&gp, &gbytes, *mod, PGB_COMPILED_LAYOUT) != hipSuccess || gbytes != sizeof *rec) {
    (void)hipGetLastError();
    return fail(PGB_E_INVALID, "the code object has no layout record " PGB_COMPILED_LAYOUT);
  }
  HIPCHK(hipMemcpyDtoH(rec, gp, sizeof *rec));
  if (rec->magic != PGB_COMPILED_MAGIC) return fail(PGB_E_INVALID, "the layout record is not one of a compiled likelihood");
  if (rec->pointwise != want_mark) {
    snprintf(g_err, sizeof g_err, "the code object is one %s, mark %d: %s takes one %s", compiled_mark_name(rec->pointwise),
             (int)rec->pointwise, entry, compiled_mark_name(want_mark));
    return PGB_E_INVALID;
  }
  if (PGB_HEADERS_HASH == 0ull || rec->headers_hash != (uint64_t)PGB_HEADERS_HASH) {
    snprintf(g_err, sizeof g_err, "the code object was compiled from other kernel headers (hash %016llx) than this library "
             "(%016llx)", (unsigned long long)rec->headers_hash, (unsigned long long)PGB_HEADERS_HASH);
    return PGB_E_INVALID;
  }
  if (rec->n_params != n_params) {
    snprintf(g_err, sizeof g_err, "the code object was compiled for %d params, the call gives n_params = %d",
             (int)rec->n_params, n_params);
    return PGB_E_INVALID;
  }
  if (rec->n_outputs != K) {
    snprintf(g_err, sizeof g_err, "the code object was compiled for %d outputs, %s = %d", (int)rec->n_outputs, k_side, K);
    return PGB_E_INVALID;
  }
  const char* kernel = want_mark == PGB_COMPILED_MARK_SAMPLER     ? PGB_PPC_COMPILED_KERNEL
                       : want_mark == PGB_COMPILED_MARK_POINTWISE ? PGB_POINTWISE_KERNEL
                                                                  : PGB_COMPILED_KERNEL;
  if (hipModuleGetFunction(fn, *mod, kernel) != hipSuccess) {
    (void)hipGetLastError();
    snprintf(g_err, sizeof g_err, "the code object has no kernel %s", kernel);
    return PGB_E_INVALID;
  }
  return PGB_OK;
}

// the draws' params ([D][n_params], host) as the table [D][PGB_COMPILED_MAX_PARAMS] a pointwise or sampler kernel
// reads (dst: zeroed by the caller); false at the first non-finite one, whose place *bad_d, *bad_i give (each caller
// has its own sentence)
static bool compiled_params_table(const double* src, int D, int n_params, double* dst, int* bad_d, int* bad_i) {
  for (int d = 0; d < D; ++d)
    for (int i = 0; i < n_params; ++i) {
      const double v = src[(size_t)d * n_params + i];
      if (!(v - v == 0.0)) {
        *bad_d = d, *bad_i = i;
        return false;
      }
      dst[(size_t)d * PGB_COMPILED_MAX_PARAMS + i] = v;
    }
  return true;
}

// the checks of a PASS object alone, after the shared ones: nullptr, or why the sampler cannot run it (why_k: room for
// a sentence with both sides in it)
static const char* compiled_pass_refusal(const pgb_handle* h, const pgb_compiled_layout& rec, char (&why_k)[128]) {
  if (rec.max_particles != PGB_MAX_PARTICLES)
    return "the code object was built for another particle build (this library takes " PGB_STR(PGB_MAX_PARTICLES) ")";
  if (rec.sizeof_dev != (int64_t)sizeof(Dev) || rec.sizeof_job != (int64_t)sizeof(Job) ||
      rec.sizeof_cmd != (int64_t)sizeof(Cmd) || rec.sizeof_ctrl != (int64_t)sizeof(Ctrl) ||
      rec.sizeof_acc != (int64_t)sizeof(Acc))
    return "the code object's device records differ from this library's";
  if ((rec.linear_leaves != 0) != (h->s.response != PGB_RESPONSE_CONSTANT) ||
      (rec.linear_leaves != 0 && rec.linear_leaves != 1)) {
    const char* resp = h->s.response == PGB_RESPONSE_CONSTANT ? "constant"
                       : h->s.response == PGB_RESPONSE_LINEAR ? "linear" : "mix";
    snprintf(why_k, sizeof why_k, "the code object was compiled for %s leaves, the sampler has response = %s",
             rec.linear_leaves == 0 ? "constant" : rec.linear_leaves == 1 ? "linear" : "unknown", resp);
    return why_k;
  }
  return nullptr;
}

extern "C" int pgb_set_loglik_code(pgb_handle* h, const void* code_object, int64_t bytes, int32_t n_params) {
  if (!h) return fail(PGB_E_INVALID, "null handle");
  JOIN_ASYNC(h);
  if (h->s.family != PGB_FAMILY_COMPILED)
    return fail(PGB_E_INVALID, "the sampler was not created with the compiled family");
  if (n_params < 0 || n_params > PGB_COMPILED_MAX_PARAMS)
    return fail(PGB_E_INVALID, "n_params must be in [0, " PGB_STR(PGB_COMPILED_MAX_PARAMS) "]");
  // a refused object is never launched and never replaces the loaded one: the handle is untouched until every check
  // has passed
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr, probe = nullptr;
  pgb_compiled_layout rec;
  char why_k[128];
  int rc = compiled_load_code(code_object, bytes, n_params, h->s.n_outputs, "the sampler has n_outputs",
                              PGB_COMPILED_MARK_PASS, "pgb_set_loglik_code", &mod, &fn, &rec);
  if (rc == PGB_OK) {
    const char* why = compiled_pass_refusal(h, rec, why_k);
    if (!why && hipModuleGetFunction(&probe, mod, PGB_COMPILED_PROBE) != hipSuccess)
      why = "the code object has no kernel " PGB_COMPILED_PROBE;
    if (why) rc = fail(PGB_E_INVALID, why);
  }
  if (rc != PGB_OK) {
    (void)hipGetLastError();
    if (mod) (void)hipModuleUnload(mod);
    return rc;
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
