// k_rank.h -- part of pgbart_hip.hip (not a standalone header): ROC AUC, KS and threshold counts of stored draws, per
// draw and group (include/pgbart_rank.h holds the contract and the pair-counting reference), the kernels and the host
// side of pgb_rank_keys and pgb_rank_metrics.
//
//   k_rank_keys   one lane per (d, i), i fastest: blockIdx.x tiles the rows of the block, blockIdx.y strides over the
//                 draws, so the reads along the rows are coalesced.  Value, key, scatter to keys[d][dest[i]]: the rows
//                 of a segment keep their order, so the stores of a wave fall into as many runs as it has segments.
//                 One 64-bit integer atomic per lane that met a NaN (or a dest out of range), none otherwise.
//   the sort      hipcub::DeviceSegmentedRadixSort::SortKeys over the 2 G D segments, keys only: class and group are
//                 in the layout already.
//   k_rank_count  one lane per sorted element: the lower bound of its key in its own segment, the lower (and, for a
//                 positive, the upper) bound in the opposite segment of its (draw, group).  Neighbouring lanes hold
//                 neighbouring keys, so their searches walk the same cache lines.  The lanes of a wave that share a
//                 (draw, group) are reduced with DPP; one 64-bit atomic add (U2) and one atomic max (KSN) per wave
//                 and target.  Integer atomics: any order gives the same bits.
//   k_rank_thr    one lane per (d, g, t, class): one lower bound, one plain store.
#include "pgbart_rank.h"

#define RANK_BT 256

__global__ __launch_bounds__(RANK_BT) void k_rank_keys(const double* __restrict__ a, int D, long long nb, long long ld,
                                                       const double* __restrict__ off, int transform,
                                                       const int64_t* __restrict__ dest, long long n,
                                                       uint64_t* __restrict__ keys, unsigned long long* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * RANK_BT + threadIdx.x;
  if (i >= nb) return;
  const pgb_lltabs tb = arms_tabs();
  const int has_off = off != nullptr;
  const double off_i = has_off ? off[i] : 0.0;
  const long long di = dest[i];
  const bool bad = di < 0 || di >= n;
  unsigned long long n_nan = 0, n_bad = 0;
  for (int d = blockIdx.y; d < D; d += gridDim.y) {
    if (bad) {
      n_bad += 1;
      continue;
    }
    const double v = pgb_rowsum_value(a[(size_t)d * (size_t)ld + i], has_off, off_i, transform, &tb);
    n_nan += pgb_rank_is_nan(v) ? 1 : 0;
    keys[(size_t)d * (size_t)n + di] = pgb_rank_key(v);
  }
  if (n_nan) atomicAdd(cnt, n_nan);
  if (n_bad) atomicAdd(cnt + 1, n_bad);
}

// 64-bit wave maximum of values >= 0 with the DPP steps of wave_sum_dpp (a lane without a source takes 0, the identity
// here); the result lands in lane 63.
__device__ __forceinline__ long long wave_max_dpp_nonneg(long long v) {
  int lo = (int)v, hi = (int)(v >> 32);
#define PGB_DPP_STEP(ctrl, rm)                                     \
  {                                                                \
    int tl = __builtin_amdgcn_update_dpp(0, lo, ctrl, rm, 0xf, 0); \
    int th = __builtin_amdgcn_update_dpp(0, hi, ctrl, rm, 0xf, 0); \
    long long a = ((long long)hi << 32) | (unsigned)lo;            \
    long long b = ((long long)th << 32) | (unsigned)tl;            \
    a = b > a ? b : a;                                             \
    lo = (int)a;                                                   \
    hi = (int)(a >> 32);                                           \
  }
  PGB_DPP_STEP(0x111, 0xf)  // row_shr:1
  PGB_DPP_STEP(0x112, 0xf)  // row_shr:2
  PGB_DPP_STEP(0x114, 0xf)  // row_shr:4
  PGB_DPP_STEP(0x118, 0xf)  // row_shr:8
  PGB_DPP_STEP(0x142, 0xa)  // row_bcast:15
  PGB_DPP_STEP(0x143, 0xc)  // row_bcast:31
#undef PGB_DPP_STEP
  return ((long long)hi << 32) | (unsigned)lo;
}

__global__ __launch_bounds__(RANK_BT) void k_rank_count(const uint64_t* __restrict__ keys, long long n, long long total,
                                                        const int64_t* __restrict__ seg_off, int G, int n_out,
                                                        unsigned long long* __restrict__ out) {
  const long long e = (long long)blockIdx.x * RANK_BT + threadIdx.x;
  long long target = -1, u2 = 0, ks = 0;  // (no early return: every lane takes part in the DPP steps below)
  if (e < total) {
    const long long d = e / n, j = e - d * n;
    int lo = 0, hi = 2 * G;  // seg_off[lo] <= j < seg_off[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (seg_off[mid] <= j) lo = mid;
      else hi = mid;
    }
    const int g = lo >> 1, c = lo & 1;
    const long long b0 = seg_off[2 * g], b1 = seg_off[2 * g + 1], b2 = seg_off[2 * g + 2];
    const long long n0 = b1 - b0, n1 = b2 - b1;
    const uint64_t* __restrict__ neg = keys + (size_t)d * (size_t)n + b0;
    const uint64_t* __restrict__ pos = keys + (size_t)d * (size_t)n + b1;
    const uint64_t k = keys[e];
    long long tp, fp;
    if (c) {
      const long long lo_opp = pgb_rank_lower(neg, n0, k), hi_opp = pgb_rank_upper(neg, n0, k);
      u2 = 2 * lo_opp + (hi_opp - lo_opp);
      tp = n1 - pgb_rank_lower(pos, n1, k);
      fp = n0 - lo_opp;
    } else {
      tp = n1 - pgb_rank_lower(pos, n1, k);
      fp = n0 - pgb_rank_lower(neg, n0, k);
    }
    ks = pgb_rank_ks_term(tp, fp, n1, n0);
    target = d * G + g;
  }
  unsigned long long todo = __ballot(target >= 0);
  while (todo) {  // (wave-uniform: one turn per (draw, group) the wave holds, usually one)
    const int first = __ffsll((long long)todo) - 1;
    const long long t = uni(__shfl(target, first, 64));
    const bool mine = target == t;
    const long long s = wave_sum_dpp(mine ? u2 : 0), m = wave_max_dpp_nonneg(mine ? ks : 0);
    if (lane_id() == 63) {
      if (s) atomicAdd(out + (size_t)t * n_out, (unsigned long long)s);
      if (m) atomicMax(out + (size_t)t * n_out + 1, (unsigned long long)m);
    }
    todo &= ~__ballot(mine);
  }
}

__global__ __launch_bounds__(RANK_BT) void k_rank_thr(const uint64_t* __restrict__ keys, long long n, int D,
                                                      const int64_t* __restrict__ seg_off, int G, int T,
                                                      const uint64_t* __restrict__ thr_keys,
                                                      unsigned long long* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * RANK_BT + threadIdx.x;
  if (idx >= (long long)D * G * T * 2) return;
  const int c = (int)(idx & 1), t = (int)((idx >> 1) % T);
  const long long dg = (idx >> 1) / T;
  const long long d = dg / G;
  const int g = (int)(dg - d * G);
  const long long b = seg_off[2 * g + c], len = seg_off[2 * g + c + 1] - b;
  const long long lo = pgb_rank_lower(keys + (size_t)d * (size_t)n + b, len, thr_keys[t]);
  out[(size_t)dg * PGB_RANK_NOUT(T) + 2 + (c ? t : T + t)] = (unsigned long long)(len - lo);
}

static thread_local double g_rank_ms[3] = {-1.0, -1.0, -1.0};
extern "C" int pgb_rank_kernel_ms(double* keys_ms, double* sort_ms, double* count_ms) {
  if (!keys_ms || !sort_ms || !count_ms) return fail(PGB_E_INVALID, "null argument");
  *keys_ms = g_rank_ms[0];
  *sort_ms = g_rank_ms[1];
  *count_ms = g_rank_ms[2];
  return PGB_OK;
}

extern "C" int pgb_rank_keys(const double* a_dev, int32_t D, int64_t nb, int64_t ld, const double* off_dev, int32_t transform,
                             const int64_t* dest_dev, int64_t n, uint64_t* keys_dev, uint64_t* counters_dev, void* stream) {
  PredCall pc("pgb_rank_keys");
  pc.null(a_dev, "a_dev");
  pc.null(dest_dev, "dest_dev");
  pc.null(keys_dev, "keys_dev");
  pc.null(counters_dev, "counters_dev");
  pc.at_least_one(D, "D");
  pc.at_least_one(nb, "nb");
  pc.require(n >= 2, "n must be >= 2");
  pc.require(nb <= n, "nb must be <= n");
  pc.require(ld >= nb, "ld must be >= nb");
  pc.require(ld <= ((int64_t)1 << 40), "ld overflows the index arithmetic");
  pc.require(transform >= 0 && transform < PGB_ROWSUM_N_TRANSFORMS, "transform is not one of the PGB_ROWSUM_* codes");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.require(n < ((int64_t)1 << 31) && (int64_t)D * n < ((int64_t)1 << 31), "D x n must be < 2^31");
  if (pc.rc() != PGB_OK) return pc.rc();

  hipStream_t sm = (hipStream_t)stream;
  const long long bx = (nb + RANK_BT - 1) / RANK_BT;
  long long by = (16384 + bx - 1) / bx;  // enough workgroups to fill the chip, each striding over its draws
  if (by > D) by = D;
  if (by > 65535) by = 65535;
  WalkTimer wt(sm);
  hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)bx, (unsigned)by), dim3(RANK_BT), 0, sm, a_dev, (int)D, (long long)nb,
                     (long long)ld, off_dev, (int)transform, dest_dev, (long long)n, keys_dev, (unsigned long long*)counters_dev);
  return finish_walk(hipGetLastError(), sm, wt, &g_rank_ms[0], "k_rank_keys");
}

// the temporary storage of the segmented sort of `total` keys in `n_seg` segments (a query: nothing is launched)
static hipError_t rank_sort_bytes(long long total, long long n_seg, size_t* bytes) {
  hipcub::DoubleBuffer<uint64_t> kb(nullptr, nullptr);
  *bytes = 0;
  return hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, *bytes, kb, (int)total, (int)n_seg, (const int*)nullptr,
                                                    (const int*)nullptr, 0, 64, (hipStream_t) nullptr);
}
static size_t rank_align(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" int64_t pgb_rank_workspace_bytes(int32_t D, int64_t n, int32_t G) {
  if (D < 1 || n < 2 || G < 1 || G > PGB_RANK_MAX_GROUPS || n >= ((int64_t)1 << 31) || (int64_t)D * n >= ((int64_t)1 << 31)) return 0;
  size_t tmp = 0;
  const hipError_t e = rank_sort_bytes((long long)D * n, 2ll * G * D, &tmp);
  if (e != hipSuccess) {
    (void)fail_hip(e, "pgb_rank_workspace_bytes: the sort's storage query");
    return -1;
  }
  return (int64_t)(rank_align((size_t)D * (size_t)n * 8) + rank_align(tmp));
}

extern "C" int pgb_rank_metrics(uint64_t* keys_dev, void* ws_dev, int32_t D, int64_t n, const int64_t* seg_off_host, int32_t G,
                                const double* thr_host, int32_t T, const uint64_t* counters_dev, int64_t* out_host,
                                int64_t* counts_host, void* stream) {
  PredCall pc("pgb_rank_metrics");
  pc.null(keys_dev, "keys_dev");
  pc.null(ws_dev, "ws_dev");
  pc.null(counters_dev, "counters_dev");
  pc.null(out_host, "out_host");
  pc.null(counts_host, "counts_host");
  if (pc.rc() != PGB_OK) return pc.rc();
  {
    static const char* const texts[] = PGB_RANK_FAULT_TEXTS;
    int64_t where = 0;
    const int fault = pgb_rank_fault(D, n, seg_off_host, G, thr_host, T, &where);
    if (fault) return pc.refuse(PGB_E_INVALID, texts[fault], (long long)where);
  }
  hipStream_t sm = (hipStream_t)stream;
  const long long total = (long long)D * n, n_seg = 2ll * G * D;
  const int n_out = PGB_RANK_NOUT(T);
  uint64_t hc[PGB_RANK_N_COUNTERS];
  HIPCHK(hipMemcpyAsync(hc, counters_dev, sizeof hc, hipMemcpyDeviceToHost, sm));
  HIPCHK(hipStreamSynchronize(sm));
  if (hc[1] != 0) {
    for (int j = 0; j < PGB_RANK_N_COUNTERS; ++j) counts_host[j] = (int64_t)hc[j];
    return pc.refuse(PGB_E_INVALID, "%llu keys had a dest outside [0, n)", (unsigned long long)hc[1]);
  }
  size_t tmp_bytes = 0;
  HIPCHK(rank_sort_bytes(total, n_seg, &tmp_bytes));
  // one small upload: [seg_off 2 G + 1 | thr keys T | the segments' begins 2 G D + 1 (int32)], then the results
  const size_t o_thr = (size_t)(2 * G + 1) * 8, o_seg = o_thr + (size_t)T * 8;
  const size_t o_out = rank_align(o_seg + (size_t)(n_seg + 1) * 4), out_bytes = (size_t)D * G * n_out * 8;
  std::vector<uint8_t> hb(o_out);
  memcpy(hb.data(), seg_off_host, o_thr);
  for (int t = 0; t < T; ++t) ((uint64_t*)(hb.data() + o_thr))[t] = pgb_rank_key(thr_host[t]);
  int32_t* hseg = (int32_t*)(hb.data() + o_seg);
  for (long long d = 0; d < D; ++d)
    for (int s = 0; s < 2 * G; ++s) hseg[d * 2 * G + s] = (int32_t)(d * n + seg_off_host[s]);
  hseg[n_seg] = (int32_t)total;
  DevBuf small;
  HIPCHK(hipMalloc((void**)&small.p, o_out + out_bytes));
  HIPCHK(hipMemcpyAsync(small.p, hb.data(), o_out, hipMemcpyHostToDevice, sm));
  HIPCHK(hipMemsetAsync(small.p + o_out, 0, out_bytes, sm));
  const int64_t* seg_dev = (const int64_t*)small.p;
  const uint64_t* thr_dev = (const uint64_t*)(small.p + o_thr);
  const int* begins = (const int*)(small.p + o_seg);
  unsigned long long* out_dev = (unsigned long long*)(small.p + o_out);

  hipcub::DoubleBuffer<uint64_t> kb(keys_dev, (uint64_t*)ws_dev);
  void* tmp = (uint8_t*)ws_dev + rank_align((size_t)total * 8);
  WalkTimer wt_sort(sm);
  hipError_t e = hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, tmp_bytes, kb, (int)total, (int)n_seg, begins, begins + 1, 0, 64, sm);
  wt_sort.launched();
  WalkTimer wt_count(sm);
  if (e == hipSuccess) {
    const uint64_t* sorted = kb.Current();
    hipLaunchKernelGGL(k_rank_count, dim3((unsigned)((total + RANK_BT - 1) / RANK_BT)), dim3(RANK_BT), 0, sm, sorted, (long long)n,
                       total, seg_dev, (int)G, n_out, out_dev);
    if (T > 0) {
      const long long lanes = (long long)D * G * T * 2;
      hipLaunchKernelGGL(k_rank_thr, dim3((unsigned)((lanes + RANK_BT - 1) / RANK_BT)), dim3(RANK_BT), 0, sm, sorted, (long long)n,
                         (int)D, seg_dev, (int)G, (int)T, thr_dev, out_dev);
    }
    e = hipGetLastError();
  }
  const int rc = finish_walk(e, sm, wt_count, &g_rank_ms[2], "k_rank_count", &wt_sort, &g_rank_ms[1]);
  if (rc != PGB_OK) return rc;
  HIPCHK(hipMemcpyAsync(out_host, out_dev, out_bytes, hipMemcpyDeviceToHost, sm));
  HIPCHK(hipStreamSynchronize(sm));
  for (int j = 0; j < PGB_RANK_N_COUNTERS; ++j) counts_host[j] = (int64_t)hc[j];
  return PGB_OK;
}
