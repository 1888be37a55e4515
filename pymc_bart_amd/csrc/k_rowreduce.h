// k_rowreduce.h -- part of pgbart_hip.hip (not a standalone header): the per-draw averages over rows of a [D][K][nb]
// device matrix of predictions -- weighted group sums of v, v^2 and, against y, of the residual and its square
// (pgb_row_reduce, pgb_row_reduce_finish; the numeric contract -- every term, the order of every sum, the workspace -- is
// include/pgbart_rowreduce.h, whose pgb_rowred_block and pgb_rowred_finish a host build evaluates to the same bits).
//
// k_rowreduce: one WAVE owns one (d, k) and streams the block's rows 64 at a time: lane l reads row l of every tile
// (consecutive lanes, consecutive addresses), and because a block starts at a multiple of 64 that is exactly the rows
// of lane class l -- the lane forms partial l of every LANE SUM directly, in ascending row order.  A lane keeps the
// partials of its current group in registers while its group id does not change; when it changes the lane writes them
// to its own slot of the workspace, part[d][k][g][sum][l], and takes up the stored partials of the new group (0.0 after
// init, or what an earlier block or an earlier run of the same group left).  No two lanes share a slot and no two waves
// a (d, k): no floating-point atomics, no LDS, no barrier.  Rows grouped contiguously cost one exchange per group and
// lane; groups interleaved row by row cost one per row and are as correct, only slower.  w, g, y, the offsets and the
// centres are read by every wave and stay in cache; the wave of (0, 0) also forms the partials of the groups' weights.
// The two integer counters are atomic adds of integers (order-independent).  Four waves to a workgroup of 256
// threads, a few dozen VGPRs: the kernel is bound by the D K nb doubles it reads once.
//
// k_rowreduce_finish: one wave per (d, k, g) loads the 64 partials of each sum into LDS (coalesced) and one lane adds
// them in lane order with the contract's own pgb_rowsum_lanes and pgb_rowred_finish_one.
#define ROWRED_BT 256
#define ROWRED_WAVES (ROWRED_BT / 64)

__global__ __launch_bounds__(ROWRED_BT) void k_rowreduce(const double* a, const double* b, long long DK, int K, long long nb,
                                                         long long ld, const double* __restrict__ w,
                                                         const int32_t* __restrict__ g, const double* __restrict__ y,
                                                         const double* __restrict__ off_a, const double* __restrict__ off_b,
                                                         const double* __restrict__ centre, int G, int transform,
                                                         long long wpart_off, double* __restrict__ ws, double* v_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long dk = (long long)blockIdx.x * ROWRED_WAVES + wave;
  if (dk >= DK) return;
  const int k = (int)(dk % K);
  const bool first = dk == 0;  // (the wave that also sums the weights and counts the rows without a group)
  const bool has_y = y != nullptr;
  const int ns = PGB_ROWRED_NSUMS(has_y);
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
  double* part = ws + (size_t)dk * (size_t)G * (size_t)ns * PGB_ROWRED_LANES + lane;  // + g ns 64: this lane's slots
  double* wpart = ws + wpart_off + lane;                                              // + g 64
  unsigned long long* cnt = (unsigned long long*)(ws + wpart_off + (size_t)G * PGB_ROWRED_LANES);
  const size_t row = (size_t)dk * (size_t)ld;
  const double* oa = off_a ? off_a + (size_t)k * (size_t)nb : nullptr;
  const double* ob = off_b ? off_b + (size_t)k * (size_t)nb : nullptr;
  const double* ck = centre ? centre + (size_t)k * (size_t)G : nullptr;

  int gc = -1;  // the group whose partials are in the registers
  double c = 0.0, s1 = 0.0, s2 = 0.0, e1 = 0.0, e2 = 0.0, sw = 0.0;
  unsigned long long n_nonfinite = 0, n_bad = 0;
  for (long long i = lane; i < nb; i += PGB_ROWRED_LANES) {
    const int gi = g[i];
    const double wi = w[i];
    const double v = pgb_rowred_value(a[row + i], oa != nullptr, oa ? oa[i] : 0.0, b != nullptr, b ? b[row + i] : 0.0,
                                      ob != nullptr, ob ? ob[i] : 0.0, transform, &tb);
    if (v_out) v_out[row + i] = v;
    if (gi < 0 || gi >= G) {
      n_bad += first ? 1 : 0;
      continue;
    }
    if (gi != gc) {
      if (gc >= 0) {
        double* p = part + (size_t)gc * (size_t)ns * PGB_ROWRED_LANES;
        p[0] = s1;
        p[PGB_ROWRED_LANES] = s2;
        if (has_y) {
          p[2 * PGB_ROWRED_LANES] = e1;
          p[3 * PGB_ROWRED_LANES] = e2;
        }
        if (first) wpart[(size_t)gc * PGB_ROWRED_LANES] = sw;
      }
      const double* p = part + (size_t)gi * (size_t)ns * PGB_ROWRED_LANES;
      s1 = p[0];
      s2 = p[PGB_ROWRED_LANES];
      if (has_y) {
        e1 = p[2 * PGB_ROWRED_LANES];
        e2 = p[3 * PGB_ROWRED_LANES];
      }
      if (first) sw = wpart[(size_t)gi * PGB_ROWRED_LANES];
      c = ck ? ck[gi] : 0.0;
      gc = gi;
    }
    n_nonfinite += pgb_rowred_nonfinite(v) ? 1 : 0;
    const double u = v - c;
    s1 = s1 + pgb_rowred_term1(wi, u);
    s2 = s2 + pgb_rowred_term2(wi, u);
    if (has_y) {
      const double r = y[i] - v;
      e1 = e1 + pgb_rowred_term1(wi, r);
      e2 = e2 + pgb_rowred_term2(wi, r);
    }
    if (first) sw = sw + wi;
  }
  if (gc >= 0) {
    double* p = part + (size_t)gc * (size_t)ns * PGB_ROWRED_LANES;
    p[0] = s1;
    p[PGB_ROWRED_LANES] = s2;
    if (has_y) {
      p[2 * PGB_ROWRED_LANES] = e1;
      p[3 * PGB_ROWRED_LANES] = e2;
    }
    if (first) wpart[(size_t)gc * PGB_ROWRED_LANES] = sw;
  }
  if (n_nonfinite) atomicAdd(&cnt[0], n_nonfinite);
  if (n_bad) atomicAdd(&cnt[1], n_bad);
}

__global__ __launch_bounds__(ROWRED_BT) void k_rowreduce_finish(const double* __restrict__ ws, long long n_items, int K, int G,
                                                                int has_y, long long wpart_off,
                                                                const double* __restrict__ centre, double* __restrict__ out,
                                                                double* __restrict__ w_out) {
  __shared__ double s_part[ROWRED_WAVES][5][PGB_ROWRED_LANES];  // the partials of S1, S2, E1, E2 and W
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * ROWRED_WAVES + wave;
  const bool act = item < n_items;
  const long long it = act ? item : 0;  // (every wave takes the barrier: a wave without an item repeats item 0)
  const int ns = PGB_ROWRED_NSUMS(has_y);
  const int gi = (int)(it % G), k = (int)((it / G) % K);
  for (int j = 0; j < ns; ++j) s_part[wave][j][lane] = ws[((size_t)it * ns + j) * PGB_ROWRED_LANES + lane];
  s_part[wave][4][lane] = ws[(size_t)wpart_off + (size_t)gi * PGB_ROWRED_LANES + lane];
  __syncthreads();
  if (!act || lane != 0) return;
  double s[4], o[6];
  for (int j = 0; j < ns; ++j) s[j] = pgb_rowsum_lanes(s_part[wave][j]);
  const double W = pgb_rowsum_lanes(s_part[wave][4]);
  pgb_rowred_finish_one(s, has_y, W, centre ? centre[(size_t)k * G + gi] : 0.0, o);
  const int n_out = PGB_ROWRED_NOUT(has_y);
  for (int j = 0; j < n_out; ++j) out[(size_t)j * (size_t)n_items + (size_t)item] = o[j];
  if (item < G) w_out[gi] = W;  // (d, k) = (0, 0)
}

static int rowred_dims(const char* fn, int32_t D, int32_t K, int32_t G) {
  if (D < 1 || K < 1) {
    snprintf(g_err, sizeof g_err, "%s: D and K must be >= 1, got D = %d, K = %d", fn, (int)D, (int)K);
    return PGB_E_INVALID;
  }
  if (G < 1 || G > PGB_ROWRED_MAX_GROUPS) {
    snprintf(g_err, sizeof g_err, "%s: the number of groups must be in [1, " PGB_STR(PGB_ROWRED_MAX_GROUPS) "], got %d", fn, (int)G);
    return PGB_E_INVALID;
  }
  return PGB_OK;
}

extern "C" int64_t pgb_row_reduce_workspace_bytes(int32_t D, int32_t K, int32_t G, int32_t has_y) {
  if (D < 1 || K < 1 || G < 1 || G > PGB_ROWRED_MAX_GROUPS) return 0;
  return 8 * pgb_rowred_ws_doubles(D, K, G, has_y != 0);
}

extern "C" int pgb_row_reduce(const double* a_dev, const double* b_dev, int32_t D, int32_t K, int64_t nb, int64_t ld,
                              const double* w_dev, const int32_t* g_dev, const double* y_dev, const double* off_a_dev,
                              const double* off_b_dev, const double* centre_dev, int32_t G, int32_t transform,
                              int64_t first_row, int32_t init, void* ws_dev, double* v_out_dev, void* stream) {
  if (!a_dev || !w_dev || !g_dev || !ws_dev) return fail(PGB_E_INVALID, "null argument");
  const int rc = rowred_dims("pgb_row_reduce", D, K, G);
  if (rc != PGB_OK) return rc;
  if (nb < 1 || ld < nb) return fail(PGB_E_INVALID, "nb must be >= 1 and ld >= nb");
  if (first_row < 0 || first_row % PGB_ROWRED_LANES != 0) {
    snprintf(g_err, sizeof g_err, "the first row of a block must be a multiple of " PGB_STR(PGB_ROWRED_LANES) ", got %lld",
             (long long)first_row);
    return PGB_E_INVALID;
  }
  if (transform < 0 || transform >= PGB_ROWSUM_N_TRANSFORMS) {
    snprintf(g_err, sizeof g_err, "unknown transform %d", (int)transform);
    return PGB_E_INVALID;
  }
  if (y_dev && K > 1) return fail(PGB_E_INVALID, "y takes one output (K == 1)");
  if (off_b_dev && !b_dev) return fail(PGB_E_INVALID, "an offset of b without b");
  const long long DK = (long long)D * K;
  const long long gx = (DK + ROWRED_WAVES - 1) / ROWRED_WAVES;
  if (gx > 0x7FFFFFFFll) return fail(PGB_E_UNSUPPORTED, "D K too large for one call");
  const int has_y = y_dev != nullptr;
  const long long wpart_off = pgb_rowred_wpart(D, K, G, PGB_ROWRED_NSUMS(has_y));
  hipStream_t sm = (hipStream_t)stream;
  hipError_t e;
  if (init) {
    e = hipMemsetAsync(ws_dev, 0, (size_t)8 * (size_t)pgb_rowred_ws_doubles(D, K, G, has_y), sm);  // (all bits 0: 0.0)
    if (e != hipSuccess) return fail_hip(e, "pgb_row_reduce: clearing the workspace");
  }
  hipLaunchKernelGGL(k_rowreduce, dim3((unsigned)gx), dim3(ROWRED_BT), 0, sm, a_dev, b_dev, DK, (int)K, (long long)nb,
                     (long long)ld, w_dev, g_dev, y_dev, off_a_dev, off_b_dev, centre_dev, (int)G, (int)transform, wpart_off,
                     (double*)ws_dev, v_out_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_rowreduce launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_rowreduce");
  return PGB_OK;
}

extern "C" int pgb_row_reduce_finish(const void* ws_dev, int32_t D, int32_t K, int32_t G, int32_t has_y,
                                     const double* centre_dev, double* out_dev, double* w_out_dev, int64_t* counts_out,
                                     void* stream) {
  if (!ws_dev || !out_dev || !w_out_dev || !counts_out) return fail(PGB_E_INVALID, "null argument");
  const int rc = rowred_dims("pgb_row_reduce_finish", D, K, G);
  if (rc != PGB_OK) return rc;
  if (has_y && K > 1) return fail(PGB_E_INVALID, "y takes one output (K == 1)");
  const long long n_items = (long long)D * K * G;
  const long long gx = (n_items + ROWRED_WAVES - 1) / ROWRED_WAVES;
  if (gx > 0x7FFFFFFFll) return fail(PGB_E_UNSUPPORTED, "D K G too large for one call");
  const int ns = PGB_ROWRED_NSUMS(has_y != 0);
  const long long wpart_off = pgb_rowred_wpart(D, K, G, ns);
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rowreduce_finish, dim3((unsigned)gx), dim3(ROWRED_BT), 0, sm, (const double*)ws_dev, n_items, (int)K,
                     (int)G, (int)(has_y != 0), wpart_off, centre_dev, out_dev, w_out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_rowreduce_finish launch");
  e = hipMemcpyAsync(counts_out, (const double*)ws_dev + pgb_rowred_counters(D, K, G, ns), 2 * sizeof(int64_t),
                     hipMemcpyDeviceToHost, sm);
  if (e != hipSuccess) return fail_hip(e, "pgb_row_reduce_finish: reading the counters");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_rowreduce_finish");
  if (counts_out[1] != 0) {
    snprintf(g_err, sizeof g_err, "%lld rows have a group outside [0, %d)", (long long)counts_out[1], (int)G);
    return PGB_E_INVALID;
  }
  return PGB_OK;
}
