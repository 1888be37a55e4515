// k_diag.h -- part of pgbart_hip.hip (not a standalone header): rank-normalised split R-hat^2 and the bulk, tail and
// mean effective sample sizes of every column of a [n_chains n_per_chain][ld] device matrix (pgb_chain_diag; the
// numeric contract -- the split, the ranks, every formula and the order of every sum -- is include/pgbart_diag.h,
// whose pgb_diag_column a host build evaluates to the same bits).
//
// A workgroup of 256 threads owns C = max(1, min(8, 8192 / Sp)) adjacent columns, Sp the next power of two >= S (the
// kept draws).  Dynamic LDS holds the C x Sp sorted values of the tile (keys while they are sorted) and ONE sequence of
// S doubles, since the columns of a tile are worked through one after the other by all four waves: 128 KiB at S =
// 8192, which one workgroup of a gfx950 CU may take once the kernel has opted in.  PGB_DIAG_MEAN_ONLY keeps the
// sequence alone, hence S <= 16384.
//   1. load: element e of the C x S tile is column e mod C of kept position e / C (the eight columns of one draw are
//      one 64-byte segment); x = T(a) and its key go to keys[column][position];
//   2. sort: one bitonic network over all C x Sp keys (k_rowsum's), the keys become values in place;
//   3. per column, per statistic: the sequence is formed by position -- the raw value is read from a_dev again (L2),
//      its rank is a lower- and an upper-bound search of its key in the sorted values, its z-score a table look-up --
//      and handed to diag_sequence: the chain means, the centring, and then Geyer's loop over PAIRS of lags.  For a
//      pair the waves take (split chain, lag) items, lane l forms partial l of the LANE SUM, the partials meet in LDS
//      (up to 32 items at once) and one thread per item combines them in lane order by the contract's functions, all
//      items side by side; two threads form the ordered sums over the chains
//      and EVERY thread evaluates the contract's stopping rule (pgb_diag_tau) from the same two numbers, so the loop
//      is uniform.  Its condition carries the bound t < h - 3 itself: whatever the data, it ends.
//      The folded R-hat re-keys and re-sorts the column's own segment.
// Cost: O(S x lags kept) per sequence -- a few pairs for a column that mixes, up to h - 3 lags for one that never
// does.  No atomics, no floating-point reduction outside the contract's order.
#define DIAG_BT 256
#define DIAG_WAVES (DIAG_BT / 64)
#define DIAG_MAX_J (2 * PGB_DIAG_MAX_CHAINS)
#define DIAG_ITEMS 32         /* (split chain, lag) items whose lane partials are in LDS at once: 8 chains x 2 lags */
#define DIAG_MAX_KEYS 8192    /* keys of one workgroup: PGB_DIAG_MAX_DRAWS x 1 column = 1024 x 8 columns */
#define DIAG_MAX_COLS 8
#define DIAG_MAX_LDS ((DIAG_MAX_KEYS + PGB_DIAG_MAX_DRAWS) * 8)  /* = PGB_DIAG_MAX_DRAWS_MEAN * 8 */

extern __shared__ unsigned long long diag_lds[];  // [C][Sp] keys, then the same bytes as sorted values; the sequence [S]

struct diag_shared {
  double part[DIAG_ITEMS][PGB_ROWSUM_LANES + 1];
  double acov[2][DIAG_MAX_J];
  double mean[DIAG_MAX_J];
  double sc[2];
  double amax[DIAG_MAX_COLS];
  pgb_diag_head_t hd;
  unsigned long long red[DIAG_BT];
};

// the largest of the threads' keys (an integer maximum: no order to keep)
__device__ unsigned long long diag_block_max(unsigned long long m, diag_shared& sh) {
  const int tid = threadIdx.x;
  sh.red[tid] = m;
  __syncthreads();
  for (int s = DIAG_BT / 2; s > 0; s >>= 1) {
    if (tid < s && sh.red[tid + s] > sh.red[tid]) sh.red[tid] = sh.red[tid + s];
    __syncthreads();
  }
  m = sh.red[0];
  __syncthreads();
  return m;
}

// every aligned segment of Dp keys of keys[0 .. total) ascending (the network of k_rowsum); ends with a barrier
__device__ void diag_sort(unsigned long long* keys, int total, int Dp) {
  const int tid = threadIdx.x, half = total >> 1;
  for (int k = 2; k <= Dp; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < half; p += DIAG_BT) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i | j;
        const bool up = (i & k & (Dp - 1)) == 0;
        const unsigned long long x = keys[i], y = keys[l];
        if ((x > y) == up) {
          keys[i] = y;
          keys[l] = x;
        }
      }
      __syncthreads();
    }
}

// the first S keys of a sorted segment become values in place (the padding stays); ends with a barrier
__device__ void diag_unkey(unsigned long long* keys, int S) {
  double* t = (double*)keys;
  for (int p = threadIdx.x; p < S; p += DIAG_BT) t[p] = pgb_rowsum_unkey(keys[p]);
  __syncthreads();
}

// pgb_diag_sequence of the sequence seq[0 .. S) in LDS (filled and synchronised by the caller; centred in place): the
// same result in every thread.  Every barrier is taken by every thread: a wave without an item repeats item 0.
__device__ void diag_sequence(double* seq, int h, int J, bool want_ess, double tau_floor, diag_shared& sh, pgb_diag_seq* o) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = J * h;
  {  // all values equal: seen before anything is summed (the barrier is the last read of seq)
    const double w0 = seq[0];
    int same = 1;
    for (int p = tid; p < S; p += DIAG_BT) same = same && seq[p] == w0;
    if (__syncthreads_and(same)) {
      pgb_diag_all_equal(w0, S, o);
      return;
    }
  }
  // items are worked off in batches of DIAG_ITEMS: the waves form the lane partials of their items, then one thread
  // per item combines its 64 partials in lane order (the rows are padded to 65 doubles: no two threads on one bank)
  for (int b0 = 0; b0 < J; b0 += DIAG_ITEMS) {
    const int nb = J - b0 < DIAG_ITEMS ? J - b0 : DIAG_ITEMS;
    for (int it = wave; it < nb; it += DIAG_WAVES) sh.part[it][lane] = pgb_rowsum_part_sum(seq + (size_t)(b0 + it) * h, h, lane);
    __syncthreads();
    if (tid < nb) sh.mean[b0 + tid] = pgb_rowsum_lanes(sh.part[tid]) / (double)h;
    __syncthreads();
  }
  for (int p = tid; p < S; p += DIAG_BT) seq[p] = seq[p] - sh.mean[p / h];
  __syncthreads();
  pgb_diag_geyer g;
  int need = 1;
  for (int t = -1; need && (t < 0 || (want_ess && t < h - 3)); t += 2) {  // the lags (t + 1, t + 2)
    for (int b0 = 0; b0 < 2 * J; b0 += DIAG_ITEMS) {  // item g = (split chain g / 2, lag t + 1 + g % 2)
      const int nb = 2 * J - b0 < DIAG_ITEMS ? 2 * J - b0 : DIAG_ITEMS;
      for (int it = wave; it < nb; it += DIAG_WAVES) {
        const int g = b0 + it;
        sh.part[it][lane] = pgb_diag_part_acov(seq + (size_t)(g >> 1) * h, h, t + 1 + (g & 1), lane);
      }
      __syncthreads();
      if (tid < nb) {
        const int g = b0 + tid;
        sh.acov[g & 1][g >> 1] = pgb_rowsum_lanes(sh.part[tid]) / (double)h;
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (t < 0) {
        pgb_diag_head(sh.mean, sh.acov[0], h, J, &sh.hd);
        sh.sc[0] = sh.hd.s0;
      } else {
        sh.sc[0] = pgb_diag_osum(sh.acov[0], J);
      }
    }
    if (tid == 64) sh.sc[1] = pgb_diag_osum(sh.acov[1], J);
    __syncthreads();
    if (t < 0) pgb_diag_geyer_init(&g, h, J, sh.hd.vm);
    need = pgb_diag_tau(&g, sh.sc[0], sh.sc[1], tau_floor);
  }
  pgb_diag_head_t hd = sh.hd;
  pgb_diag_result(&hd, &g, o);
  __syncthreads();
}

__global__ __launch_bounds__(DIAG_BT) void k_chain_diag(const double* __restrict__ a, int n_chains, int n_per_chain, int lg,
                                                        int lgC, long long n_cols, long long ld, int transform, int stats,
                                                        const double* __restrict__ z, double tau_floor,
                                                        double* __restrict__ out) {
  __shared__ diag_shared sh;
  const int tid = threadIdx.x;
  const int h = n_per_chain / 2, J = 2 * n_chains, S = J * h;
  const int Sp = 1 << lg, C = 1 << lgC;
  const bool full = stats != PGB_DIAG_MEAN_ONLY;
  const long long c0 = (long long)blockIdx.x << lgC;
  unsigned long long* keys = diag_lds;
  double* seq = (double*)diag_lds + (full ? (size_t)C << lg : (size_t)0);
  const double* expt = pgb_tab_exp();

  // ---- 0. EXP_SHIFT: every column's largest kept value by the key order
  for (int c = 0; c < C; ++c) {
    long long gc = c0 + c;
    if (gc >= n_cols) gc = n_cols - 1;
    double amax = 0.0;
    if (transform == PGB_DIAG_EXP_SHIFT) {
      unsigned long long m = 0;
      for (int p = tid; p < S; p += DIAG_BT) {
        const unsigned long long k = pgb_rowsum_key(a[(size_t)pgb_diag_row(p, n_per_chain, h) * (size_t)ld + (size_t)gc]);
        if (k > m) m = k;
      }
      amax = pgb_rowsum_unkey(diag_block_max(m, sh));
    }
    if (tid == 0) sh.amax[c] = amax;
  }
  __syncthreads();

  if (full) {
    // ---- 1. the tile's keys (columns beyond n_cols repeat the last one), the padding
    const int n_el = S << lgC;
#pragma unroll 4
    for (int e = tid; e < n_el; e += DIAG_BT) {
      const int c = e & (C - 1), p = e >> lgC;
      long long gc = c0 + c;
      if (gc >= n_cols) gc = n_cols - 1;
      const double v = a[(size_t)pgb_diag_row(p, n_per_chain, h) * (size_t)ld + (size_t)gc];
      keys[(c << lg) + p] = pgb_rowsum_key(pgb_diag_x(v, transform, sh.amax[c], expt));
    }
    if (S < Sp)
      for (int i = tid; i < (C << lg); i += DIAG_BT)
        if ((i & (Sp - 1)) >= S) keys[i] = PGB_ROWSUM_PAD_KEY;
    __syncthreads();
    // ---- 2. every column ascending, as values
    diag_sort(keys, C << lg, Sp);
    for (int c = 0; c < C; ++c) diag_unkey(keys + ((size_t)c << lg), S);
  }

  // ---- 3. one column after the other
  for (int c = 0; c < C; ++c) {
    const long long gc = c0 + c;
    if (gc >= n_cols) break;  // (the same for every thread)
    const double* col = a + (size_t)gc;
    const double amax = sh.amax[c];
    auto X = [&](int p) {
      return pgb_diag_x(col[(size_t)pgb_diag_row(p, n_per_chain, h) * (size_t)ld], transform, amax, expt);
    };
    pgb_diag_seq o;
    double r[PGB_DIAG_NOUT];
    for (int i = 0; i < PGB_DIAG_NOUT; ++i) r[i] = 0.0;
    if (full) {
      unsigned long long* kc = keys + ((size_t)c << lg);
      const double* t = (const double*)kc;
      const double med = pgb_diag_median(t, S);
      const double q05 = pgb_rowsum_quantile(t, S, 0.05), q95 = pgb_rowsum_quantile(t, S, 0.95);
      for (int p = tid; p < S; p += DIAG_BT) seq[p] = pgb_diag_z(t, S, X(p), z);
      __syncthreads();
      diag_sequence(seq, h, J, true, tau_floor, sh, &o);
      r[0] = o.rhat2;
      r[2] = o.ess;
      for (int p = tid; p < S; p += DIAG_BT) seq[p] = X(p) <= q05 ? 1.0 : 0.0;
      __syncthreads();
      diag_sequence(seq, h, J, true, tau_floor, sh, &o);
      r[3] = o.ess;
      for (int p = tid; p < S; p += DIAG_BT) seq[p] = X(p) >= q95 ? 1.0 : 0.0;
      __syncthreads();
      diag_sequence(seq, h, J, true, tau_floor, sh, &o);
      r[4] = o.ess;
      // |x - median|: the column's own segment is keyed and sorted again (its padding is still in place)
      for (int p = tid; p < S; p += DIAG_BT) kc[p] = pgb_rowsum_key(pgb_diag_fold(X(p), med));
      __syncthreads();
      diag_sort(kc, Sp, Sp);
      diag_unkey(kc, S);
      for (int p = tid; p < S; p += DIAG_BT) seq[p] = pgb_diag_z(t, S, pgb_diag_fold(X(p), med), z);
      __syncthreads();
      diag_sequence(seq, h, J, false, tau_floor, sh, &o);
      r[1] = o.rhat2;
    }
    for (int p = tid; p < S; p += DIAG_BT) seq[p] = X(p);
    __syncthreads();
    diag_sequence(seq, h, J, true, tau_floor, sh, &o);
    r[5] = o.ess;
    r[6] = o.mean;
    r[7] = o.var;
    r[8] = o.constant;
    if (tid < PGB_DIAG_NOUT) {
      double v = 0.0;
      for (int i = 0; i < PGB_DIAG_NOUT; ++i)
        if (i == tid) v = r[i];
      out[(size_t)tid * (size_t)n_cols + (size_t)gc] = v;
    }
  }
}

extern "C" int pgb_chain_diag(const double* a_dev, int32_t n_chains, int32_t n_per_chain, int64_t n_cols, int64_t ld,
                              int32_t transform, int32_t stats, const double* z_host, double tau_floor, double* out_dev,
                              void* stream) {
  if (!a_dev || !out_dev) return fail(PGB_E_INVALID, "null argument");
  if (n_chains < 1 || n_chains > PGB_DIAG_MAX_CHAINS) {
    snprintf(g_err, sizeof g_err, "n_chains must be in [1, " PGB_STR(PGB_DIAG_MAX_CHAINS) "], got %d", (int)n_chains);
    return PGB_E_INVALID;
  }
  if (n_per_chain < 4) {
    snprintf(g_err, sizeof g_err, "chain diagnostics need at least 4 draws per chain, got n_per_chain = %d", (int)n_per_chain);
    return PGB_E_INVALID;
  }
  if (stats < 0 || stats >= PGB_DIAG_N_STATS) {
    snprintf(g_err, sizeof g_err, "unknown stats %d", (int)stats);
    return PGB_E_INVALID;
  }
  if (transform < 0 || transform >= PGB_DIAG_N_TRANSFORMS) {
    snprintf(g_err, sizeof g_err, "unknown transform %d", (int)transform);
    return PGB_E_INVALID;
  }
  const bool full = stats != PGB_DIAG_MEAN_ONLY;
  const long long S = 2ll * n_chains * (n_per_chain / 2);
  const long long cap = full ? PGB_DIAG_MAX_DRAWS : PGB_DIAG_MAX_DRAWS_MEAN;
  if (S > cap) {
    snprintf(g_err, sizeof g_err, "pgb_chain_diag takes at most %lld kept draws (%s), %lld given (draws_per_chain=)", cap,
             full ? "all statistics" : "mean only", S);
    return PGB_E_INVALID;
  }
  if (n_cols < 1 || ld < n_cols) {
    snprintf(g_err, sizeof g_err, "n_cols must be >= 1 and ld >= n_cols, got n_cols = %lld, ld = %lld", (long long)n_cols,
             (long long)ld);
    return PGB_E_INVALID;
  }
  if (full && !z_host) return fail(PGB_E_INVALID, "z_host is NULL: the ranks need the table of 2 S - 1 z-scores");
  if (!(tau_floor > 0.0 && tau_floor < 1.0e300)) {
    snprintf(g_err, sizeof g_err, "tau_floor must be finite and positive, got %g", tau_floor);
    return PGB_E_INVALID;
  }
  int lg = 1;
  while ((1ll << lg) < S) ++lg;
  int lgC = 3;
  while (full && lgC > 0 && ((1 << lg) << lgC) > DIAG_MAX_KEYS) --lgC;
  const long long gx = (n_cols + (1ll << lgC) - 1) >> lgC;
  if (gx > 0x7FFFFFFFll) return fail(PGB_E_UNSUPPORTED, "n_cols too large for one call");
  const size_t lds = ((full ? (size_t)1 << (lg + lgC) : (size_t)0) + (size_t)S) * sizeof(double);
  // more than 64 KiB of dynamic LDS is an opt-in, per device
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
  static std::mutex mu;
  static std::vector<int> opted;
  {
    std::lock_guard<std::mutex> lock(mu);
    bool have = false;
    for (int d : opted) have = have || d == dev;
    if (!have) {
      e = hipFuncSetAttribute((const void*)k_chain_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DIAG_MAX_LDS);
      if (e != hipSuccess) return fail_hip(e, "k_chain_diag: dynamic LDS opt-in");
      opted.push_back(dev);
    }
  }
  hipStream_t sm = (hipStream_t)stream;
  double* zd = nullptr;
  if (full) {
    const size_t zb = (size_t)(2 * S - 1) * sizeof(double);
    e = hipMalloc((void**)&zd, zb);
    if (e != hipSuccess) return fail_hip(e, "pgb_chain_diag: the z table");
    e = hipMemcpyAsync(zd, z_host, zb, hipMemcpyHostToDevice, sm);
    if (e != hipSuccess) {
      (void)hipFree(zd);
      return fail_hip(e, "pgb_chain_diag: the z table");
    }
  }
  hipLaunchKernelGGL(k_chain_diag, dim3((unsigned)gx), dim3(DIAG_BT), lds, sm, a_dev, (int)n_chains, (int)n_per_chain, lg, lgC,
                     (long long)n_cols, (long long)ld, (int)transform, (int)stats, (const double*)zd, tau_floor, out_dev);
  e = hipGetLastError();
  hipError_t e2 = hipStreamSynchronize(sm);
  if (zd) (void)hipFree(zd);
  if (e != hipSuccess) return fail_hip(e, "k_chain_diag launch");
  if (e2 != hipSuccess) return fail_hip(e2, "k_chain_diag");
  return PGB_OK;
}
