// k_proximity.h -- part of pgbart_hip.hip (not a standalone header): the posterior proximity of rows -- the node where a
// row stops in every (draw, tree) slot as one byte, four slots to a word (pgb_predict_leaf_codes), the number of slots in
// which a query row and a reference row stop at different nodes (pgb_prox_count), and the k nearest reference rows of
// every query (pgb_prox_topk).  The contract -- the stop rule, the slots and words, the pad, the keys, the workspace -- is
// include/pgbart_proximity.h, whose sequential references a host build evaluates to the same integers.
//
// k_leaf_codes: the geometry of k_predict (pgb_pred_walk.h): one wave per workgroup, one lane per row, the wave's 64
// rows staged in LDS when p <= PRED_LDS_MAXP.  A lane produces whole WORDS: the four consecutive slots 4w .. 4w + 3 of
// the flat forest table (they may straddle two draws), stored as one dword, coalesced over the rows.  A wave without a
// missing value walks the four trees of a word interleaved on the fixed-length FNode records when none of them is
// "general": that walk ends on its leaf and the tree-local index it holds IS the code.  Everything else -- a NaN in the
// wave, a split rule other than x <= v, a tree that splits on an excluded column or stores children before parents, the
// last, partial word -- takes the PNode loop with the stop rule, one tree at a time.  No stack, no private memory.
//
// k_prox_count: a lane owns one reference row and PROX_QT = 16 query rows in registers.  Per word: ONE coalesced dword
// load of the reference word per lane, the 16 query words of the tile on the scalar path (their address is the same in
// every lane), and per (query, word) xor, and, add, or3 and one accumulating population count -- five VALU instructions
// for four byte comparisons, 80 per load.  The or3 sets the 28 bits of a word that are not a byte's top bit, so the
// count runs 28 high per word and 28 W is taken off once at the end (modulo 2^32, like the sum itself: exact).  Query
// tiles are the fast index of the grid, so the workgroups that stream the same reference rows are dispatched together.
// No LDS, no atomics, no scratch; 16 accumulators keep the kernel at 8 waves per SIMD.
//
// k_prox_topk: one workgroup per query.  The block's keys (dist << 32 | row) and the k carried keys (copied to LDS first)
// are the candidates; round r takes the smallest candidate above the key of round r - 1 by a workgroup min-reduction and
// writes it to place r of the list.  k (nb + k) key comparisons per query: next to the W nb of the count, nothing.
#define PROX_QT 16
#define PROX_BT 256

// the stop node of one row in one tree by the PNode records: pgb_prox_stop
template <bool CONT, class XV>
__device__ __forceinline__ uint32_t prox_stop_general(const PredTrees& T, int root, XV xval) {
  int g = root;
  for (;;) {
    const uint4* __restrict__ np = (const uint4*)(T.node + g);
    uint4 n0 = np[0];
    uint2 n1 = ((const uint2*)np)[2];
    asm volatile("" : "+v"(n0.x), "+v"(n0.y), "+v"(n0.z), "+v"(n0.w), "+v"(n1.x), "+v"(n1.y));  // two whole loads, requested together
    const int var = (int)n0.x;
    if (var < 0) break;
    const double xv = xval(var);
    if ((n0.w & 1u) || xv != xv) break;
    const double split = __hiloint2double((int)n1.y, (int)n1.x);
    const bool gl = CONT ? xv <= split : pgb_go_left((int)n0.w >> 1, xv, split) != 0;
    g = gl ? (int)n0.y : (int)n0.z;
  }
  return (uint32_t)(g - root);
}

// ... and by the fixed-length walk (a wave without a missing value, a tree that is not "general"): rt.y steps
template <class XV>
__device__ __forceinline__ uint32_t prox_stop_fixed(const PredTrees& T, int2 rt, XV xval) {
  const uint4* __restrict__ fn = (const uint4*)(T.fnode + rt.x);
  int gl = 0;
  for (int l = 0; l < rt.y; ++l) {
    uint4 q = fn[gl];
    asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
    const double xv = xval((int)q.z);
    gl = xv <= __hiloint2double((int)q.y, (int)q.x) ? (int)(q.w & 255u) : (int)((q.w >> 8) & 255u);
  }
  return (uint32_t)gl;
}

template <bool LDSX, bool CONT>
__global__ __launch_bounds__(PRED_BT) void k_leaf_codes(PredTrees T, const int32_t* __restrict__ slot_tree, long long n_slots,
                                                        long long W, int p, const double* __restrict__ X, long long n_rows,
                                                        long long ldx, uint32_t* __restrict__ codes, long long ldc) {
  extern __shared__ double s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
  if constexpr (LDSX) pred_stage_rows(s_x, X, row0, n_rows, ldx, p, lane);
  if (row >= n_rows) return;
  const PredRowX<LDSX> xval{s_x, X + row * ldx, lane};
  const bool clean = pred_wave_clean<CONT>(p, xval);
  for (long long w = blockIdx.y; w < W; w += gridDim.y) {
    const long long s0 = 4 * w;
    const int nv = n_slots - s0 < 4 ? (int)(n_slots - s0) : 4;  // the slots of this word that exist (wave-uniform)
    int2 rw[4];
    int any_general = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      rw[b] = T.root[slot_tree[b < nv ? s0 + b : s0]];
      any_general |= rw[b].y & 0x100;
    }
    uint32_t c[4];
    if (clean && nv == 4 && !any_general) {
      int steps = 0, gw[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        steps = rw[b].y > steps ? rw[b].y : steps;  // a finished walk idles on its leaf
        gw[b] = 0;
      }
      for (int l = 0; l < steps; ++l) {
        uint4 q[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) q[b] = ((const uint4*)(T.fnode + rw[b].x))[gw[b]];
#pragma unroll
        for (int b = 0; b < 4; ++b) asm volatile("" : "+v"(q[b].x), "+v"(q[b].y), "+v"(q[b].z), "+v"(q[b].w));
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double xv = xval((int)q[b].z);
          gw[b] = xv <= __hiloint2double((int)q[b].y, (int)q[b].x) ? (int)(q[b].w & 255u) : (int)((q[b].w >> 8) & 255u);
        }
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) c[b] = (uint32_t)gw[b];
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b >= nv) c[b] = PGB_PROX_PAD;
        else if (clean && !(rw[b].y & 0x100)) c[b] = prox_stop_fixed(T, rw[b], xval);
        else c[b] = prox_stop_general<CONT>(T, rw[b].x, xval);
      }
    }
    codes[w * ldc + row] = pgb_prox_pack4(c[0], c[1], c[2], c[3]);
  }
}

// acc[t] += over the W words the 28-high mismatch count of query i0 + t (FULL: all PROX_QT of them exist; otherwise the
// nq that do, the last one repeated) against reference row j
template <bool FULL>
__device__ __forceinline__ void prox_count_tile(const uint32_t* __restrict__ cq, long long ldq, int nq,
                                                const uint32_t* __restrict__ cr, long long ldr, long long W, uint32_t* acc) {
  for (long long w = 0; w < W; ++w) {
    const uint32_t r = cr[w * ldr];
    const uint32_t* __restrict__ qw = cq + w * ldq;
#pragma unroll
    for (int t = 0; t < PROX_QT; ++t) {
      const uint32_t x = qw[FULL ? t : (t < nq ? t : nq - 1)] ^ r;
      const uint32_t u = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
      acc[t] += (uint32_t)__builtin_popcount(u | x | 0x7f7f7f7fu);  // pgb_prox_mismatch4 + 28
    }
  }
}

__global__ __launch_bounds__(PROX_BT) void k_prox_count(const uint32_t* __restrict__ cq, long long ldq, long long q,
                                                        const uint32_t* __restrict__ cr, long long ldr, long long nb,
                                                        long long W, uint32_t* __restrict__ dist, long long ldo, int init,
                                                        long long n_qt) {
  const long long qt = (long long)blockIdx.x % n_qt, rt = (long long)blockIdx.x / n_qt;
  const long long i0 = qt * PROX_QT;
  const long long j = rt * PROX_BT + threadIdx.x;
  const long long jc = j < nb ? j : nb - 1;  // (a lane without a row repeats the last one and stores nothing)
  const int nq = q - i0 < PROX_QT ? (int)(q - i0) : PROX_QT;
  uint32_t acc[PROX_QT];
#pragma unroll
  for (int t = 0; t < PROX_QT; ++t) acc[t] = 0u;
  if (nq == PROX_QT) prox_count_tile<true>(cq + i0, ldq, nq, cr + jc, ldr, W, acc);
  else prox_count_tile<false>(cq + i0, ldq, nq, cr + jc, ldr, W, acc);
  if (j >= nb) return;
  const uint32_t high = (uint32_t)(28ull * (unsigned long long)W);  // modulo 2^32, as the accumulators are
#pragma unroll
  for (int t = 0; t < PROX_QT; ++t) {
    if (t >= nq) break;
    uint32_t* o = dist + (i0 + t) * ldo + j;
    const uint32_t v = acc[t] - high;
    *o = init ? v : *o + v;
  }
}

// the minimum (MIN) or the sum of one value per thread over the workgroup, in every thread; s_red: [PROX_BT / 64]
template <bool MIN>
__device__ __forceinline__ unsigned long long prox_wg_reduce(unsigned long long v, unsigned long long* s_red) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o);
    v = MIN ? (u < v ? u : v) : v + u;
  }
  __syncthreads();  // (the readers of the previous reduction are done with s_red)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = s_red[0];
  for (int i = 1; i < PROX_BT / 64; ++i) v = MIN ? (s_red[i] < v ? s_red[i] : v) : v + s_red[i];
  return v;
}

__global__ __launch_bounds__(PROX_BT) void k_prox_topk(const uint32_t* __restrict__ dist, long long ldo, long long q,
                                                       long long nb, long long first_row, long long self_row0, int k,
                                                       unsigned long long* __restrict__ ws, int init) {
  __shared__ unsigned long long s_old[PGB_PROX_MAX_K];
  __shared__ unsigned long long s_red[PROX_BT / 64];
  const long long i = blockIdx.x;
  const int tid = threadIdx.x;
  unsigned long long* keys = ws + i * k;
  unsigned long long* sum = ws + q * k + i;
  const uint32_t* __restrict__ d = dist + i * ldo;
  for (int r = tid; r < k; r += PROX_BT) s_old[r] = init ? PGB_PROX_KEY_NONE : keys[r];
  const long long skip = self_row0 >= 0 ? self_row0 + i - first_row : -1;  // the block's column of the query itself
  unsigned long long part = 0;
  for (long long j = tid; j < nb; j += PROX_BT)
    if (j != skip) part += d[j];
  const unsigned long long total = prox_wg_reduce<false>(part, s_red);  // (its barriers also publish s_old)
  if (tid == 0) *sum = (init ? 0ull : *sum) + total;
  unsigned long long lo = 0;  // the smallest key not yet taken is >= lo
  for (int r = 0; r < k; ++r) {
    unsigned long long best = PGB_PROX_KEY_NONE;
    for (long long j = tid; j < nb; j += PROX_BT) {
      if (j == skip) continue;
      const unsigned long long key = pgb_prox_key(d[j], first_row + j);
      if (key >= lo && key < best) best = key;
    }
    for (int c = tid; c < k; c += PROX_BT) {
      const unsigned long long key = s_old[c];
      if (key >= lo && key < best) best = key;
    }
    best = prox_wg_reduce<true>(best, s_red);
    if (tid == 0) keys[r] = best;
    lo = best == PGB_PROX_KEY_NONE ? best : best + 1;
  }
}

extern "C" int pgb_predict_leaf_codes(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests,
                                      int32_t m, const double* X_dev, int64_t n_rows, int32_t p, int64_t ldx,
                                      const int32_t* excluded_host, int32_t n_excluded, uint32_t* codes_dev, int64_t ldc,
                                      void* stream) {
  PredCall pc("pgb_predict_leaf_codes");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(codes_dev, "codes_dev");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(n_rows, "n_rows");
  pc.ld(ldx, p, "ldx");
  pc.require(ldc >= n_rows, "ldc must be >= n_rows");
  pc.require(n_excluded >= 0 && (n_excluded == 0 || excluded_host), "excluded_host is null with n_excluded > 0");
  const long long n_slots = (long long)n_forests * m;
  pc.require(n_slots <= PGB_PROX_MAX_SLOTS, "n_forests m exceeds the 2^31 - 1 slots of a distance");
  long long gx = 0;
  pc.tiles(n_rows, &gx);
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;
  for (int t = 0; t < trees->n_trees; ++t) {
    const int nn = trees->node_off[t + 1] - trees->node_off[t];
    if (nn > PGB_PROX_MAX_NODES)
      return pc.refuse(PGB_E_INVALID, "tree %d has %d nodes: a leaf code is one byte, at most " PGB_STR(PGB_PROX_MAX_NODES) " nodes per tree",
                       t, nn);
  }
  hipStream_t sm = (hipStream_t)stream;
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, excluded_host, n_excluded, sm, &pk);
  if (rc != PGB_OK) return rc;
  const long long W = pgb_prox_words(n_slots);
  // one wave per workgroup; enough workgroups to fill the chip, each looping over its share of the words (pgb_predict's rule)
  const long long want_wgs = p <= PRED_LDS_MAXP ? 16384 : 4096;
  long long gy = (want_wgs + gx - 1) / gx;
  if (gy > W) gy = W;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  dim3 grid((unsigned)gx, (unsigned)gy);
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  const PredTrees T = pk.T;
  WalkTimer wt(sm);
  dispatch_bools(ldsx, pk.cont, [&](auto L, auto C) {
    hipLaunchKernelGGL((k_leaf_codes<L(), C()>), grid, dim3(PRED_BT), lds, sm, T, pk.fidx, n_slots, W, (int)p, X_dev,
                       (long long)n_rows, (long long)ldx, codes_dev, (long long)ldc);
  });
  return finish_walk(hipGetLastError(), sm, wt, nullptr, "k_leaf_codes");
}

extern "C" int pgb_prox_count(const uint32_t* cq_dev, int64_t ldq, int64_t q, const uint32_t* cr_dev, int64_t ldr, int64_t nb,
                              int64_t W, uint32_t* dist_dev, int64_t ldo, int32_t init, void* stream) {
  PredCall pc("pgb_prox_count");
  pc.null(cq_dev, "cq_dev");
  pc.null(cr_dev, "cr_dev");
  pc.null(dist_dev, "dist_dev");
  pc.at_least_one(q, "q");
  pc.at_least_one(nb, "nb");
  pc.at_least_one(W, "W");
  pc.require(ldq >= q, "ldq must be >= q");
  pc.require(ldr >= nb, "ldr must be >= nb");
  pc.require(ldo >= nb, "ldo must be >= nb");
  pc.require(W <= pgb_prox_words(PGB_PROX_MAX_SLOTS), "W exceeds the words of 2^31 - 1 slots");
  if (pc.rc() != PGB_OK) return pc.rc();
  const long long n_qt = (q + PROX_QT - 1) / PROX_QT, n_rt = (nb + PROX_BT - 1) / PROX_BT;
  if (n_qt > 0x7fffffffLL / n_rt) return pc.refuse(PGB_E_INVALID, "q nb exceeds 2^31 - 1 tiles of " PGB_STR(PROX_QT) " x " PGB_STR(PROX_BT));
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_prox_count, dim3((unsigned)(n_qt * n_rt)), dim3(PROX_BT), 0, sm, cq_dev, (long long)ldq, (long long)q,
                     cr_dev, (long long)ldr, (long long)nb, (long long)W, dist_dev, (long long)ldo, (int)(init != 0), n_qt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_prox_count launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_prox_count");
  return PGB_OK;
}

extern "C" int64_t pgb_prox_topk_workspace_bytes(int64_t q, int32_t k) {
  if (q < 1 || k < 1 || k > PGB_PROX_MAX_K) return 0;
  return 8 * pgb_prox_topk_ws_words(q, k);
}

extern "C" int pgb_prox_topk(const uint32_t* dist_dev, int64_t ldo, int64_t q, int64_t nb, int64_t first_row,
                             int64_t self_row0, int32_t k, void* ws_dev, int32_t init, void* stream) {
  PredCall pc("pgb_prox_topk");
  pc.null(dist_dev, "dist_dev");
  pc.null(ws_dev, "ws_dev");
  pc.at_least_one(q, "q");
  pc.at_least_one(nb, "nb");
  pc.require(ldo >= nb, "ldo must be >= nb");
  pc.require(k >= 1 && k <= PGB_PROX_MAX_K, "k must be in [1, " PGB_STR(PGB_PROX_MAX_K) "]");
  pc.require(q <= 0x7fffffffLL, "q exceeds 2^31 - 1 queries");
  pc.require(first_row >= 0 && first_row <= 0xffffffffLL - 1 && nb <= 0xffffffffLL - first_row,
             "first_row must be >= 0 and first_row + nb <= 2^32 - 1");
  if (pc.rc() != PGB_OK) return pc.rc();
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_prox_topk, dim3((unsigned)q), dim3(PROX_BT), 0, sm, dist_dev, (long long)ldo, (long long)q,
                     (long long)nb, (long long)first_row, (long long)self_row0, (int)k, (unsigned long long*)ws_dev,
                     (int)(init != 0));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_prox_topk launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_prox_topk");
  return PGB_OK;
}
