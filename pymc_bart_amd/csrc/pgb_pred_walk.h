// pgb_pred_walk.h -- part of pgbart_hip.hip and of k_pointwise_compiled.hip (not a standalone header): the packed
// tree records of a prediction and the walk of one row through the m trees of one forest, shared by k_predict
// (k_setup_predict.h) and k_pointwise (k_pointwise.h) so that both accumulate the same bits.
// ------------------------------------------------------------------ prediction
// out[d][k][row] = sum over the m trees of forest d of the leaf value reached by X[row,:]
// (PosteriorSampler.sample_posterior, utils.py:66-69); excluded / NaN splits average both
// subtrees by their training counts (CHANGELOG.md:410-411).  One thread per (row, forest).
//
// A traversal is a chain of dependent loads, so a node is ONE 32-byte record (packed on the host
// per call: split variable, children as pool-wide indices, split rule and "excluded" folded into
// flags, the split value and the training count) instead of a lookup in five arrays plus the rule
// and exclusion tables: one memory round trip per level for the node and one for the row's value.
struct PNode {
  int32_t var;          // split variable, -1: leaf
  int32_t left, right;  // pool-wide node indices
  int32_t flags;        // bit 0: the split variable is excluded; bits 1..2: split rule
  double split;
  double cnt;           // training rows in the node (exact in a double)
};
// The same tree for the walk that needs no marginalisation (16 bytes, children tree-local): leaves
// point at themselves with split = +inf, so a walk is exactly `depth` steps for every row -- no
// leaf test, no divergence -- and ends on its leaf.
struct FNode {
  double split;
  int32_t var;
  uint8_t left, right;
  uint16_t pad;
};
struct PredTrees {
  const PNode* node;      // [total_nodes]
  const FNode* fnode;     // [total_nodes]
  const int2* root;       // [n_trees] {pool-wide index of the root, depth | 0x100 when the tree needs the general walk}
  const double* value;    // [total_nodes][K]
  // linear leaves (svar == nullptr: none); svar is -1 for constant leaves AND for excluded regressors
  const double* slope;    // [total_nodes][K]
  const double* xbar;     // [total_nodes]
  const int32_t* svar;    // [total_nodes]
};

// The row's values: the threads of a wave own consecutive rows of a row-major matrix, so a read of
// "my row, my split variable" touches 64 different cache lines per instruction -- that, not the node
// chain, bounded the first version (44 G tree-traversals/s at cfg2).  LDSX: the wave first copies its
// 64 rows (coalesced) into LDS, transposed [column][lane] with a pad of one; the traversal reads
// from there.  One wave per workgroup; the workgroup loops over a share of the forests so that the
// staged rows serve several.  (p <= PRED_LDS_MAXP: 64 KB of LDS; wider matrices use global reads.)
#define PRED_BT 64
#ifndef PRED_WALKS
#define PRED_WALKS 4 /* interleaved fixed-length walks per lane */
#endif
#ifndef PRED_LDS_MAXP
#define PRED_LDS_MAXP 126
#endif

// LDSX: the wave's tile of rows row0 .. row0 + 63 (those below n_rows) into s_x[p][65], and the barrier after it.
__device__ __forceinline__ void pred_stage_rows(double* s_x, const double* X, long long row0, long long n_rows, long long ldx,
                                                int p, int lane) {
  const long long rows_here = n_rows - row0 < PRED_BT ? n_rows - row0 : PRED_BT;
  if (ldx == p) {  // the block of rows is contiguous: fully coalesced copy
    const double* __restrict__ src = X + row0 * ldx;
    const int tot = (int)rows_here * p;
    for (int i = lane; i < tot; i += PRED_BT) s_x[(i % p) * 65 + i / p] = src[i];
  } else {
    for (int r = 0; r < (int)rows_here; ++r)
      for (int j = lane; j < p; j += PRED_BT) s_x[j * 65 + r] = X[(row0 + r) * ldx + j];
  }
  __syncthreads();
}

// xval of a lane that walks its own row: column j from the staged tile (LDSX) or from the row itself
template <bool LDSX>
struct PredRowX {
  const double* s_x;              // pred_stage_rows' tile
  const double* __restrict__ x;   // X + row * ldx
  int lane;
  __device__ __forceinline__ double operator()(int j) const {
    if constexpr (LDSX) return s_x[j * 65 + lane];
    else return x[j];
  }
};

// Rows without a missing value take the fixed-length walk through every tree that does not split on an excluded
// variable (decided per wave / per tree, so that the walk stays uniform): pred_walk_forest's `clean`.
template <bool CONT, class XV>
__device__ __forceinline__ bool pred_wave_clean(int p, XV xval) {
  if (!CONT) return false;
  bool nan = false;
  for (int j = 0; j < p; ++j) {
    const double v = xval(j);
    nan = nan || v != v;
  }
  return __ballot(nan) == 0ull;
}

// acc[0 .. K-1] = the sum over the m trees `forest_of_draw` names of the leaf values the row reaches; xval(j) is the
// row's value of column j.  `clean`: wave-uniform, no lane of the wave holds a missing value (CONT only).  The order of
// the additions is the contract: tree 0 first, within a tree that marginalises depth-first, left first.
template <bool CONT, class XV>
__device__ __forceinline__ void pred_walk_forest(const PredTrees& T, const int32_t* __restrict__ forest_of_draw, int m, int K,
                                                 bool clean, XV xval, int* stk_node, double* stk_w, double* acc) {
  for (int o = 0; o < K; ++o) acc[o] = 0.0;
  // Trees are taken PRED_WALKS at a time when all of them qualify for the fixed-length walk: that
  // many independent chains of (node, value) loads per lane; the roots of the next group are
  // requested before the current group is walked.  Otherwise one tree at a time (the explicit
  // stack -- private memory -- is touched only by walks that marginalise).
  const int32_t* __restrict__ fi = forest_of_draw;
  int2 rnx[PRED_WALKS];
  bool have_nx = false;
  for (int t = 0; t < m; ++t) {
    if (clean && t + PRED_WALKS <= m) {
      int2 rw[PRED_WALKS];
      int any_general = 0;
#pragma unroll
      for (int w = 0; w < PRED_WALKS; ++w) {
        rw[w] = have_nx ? rnx[w] : T.root[fi[t + w]];
        any_general |= rw[w].y & 0x100;
      }
      have_nx = false;
      if (!any_general) {
        if (t + 2 * PRED_WALKS <= m) {
#pragma unroll
          for (int w = 0; w < PRED_WALKS; ++w) rnx[w] = T.root[fi[t + PRED_WALKS + w]];
          have_nx = true;
        }
        int steps = 0, gw[PRED_WALKS];
#pragma unroll
        for (int w = 0; w < PRED_WALKS; ++w) {
          steps = rw[w].y > steps ? rw[w].y : steps;  // a finished walk idles on its leaf
          gw[w] = 0;
        }
        for (int l = 0; l < steps; ++l) {
          uint4 q[PRED_WALKS];
#pragma unroll
          for (int w = 0; w < PRED_WALKS; ++w) q[w] = ((const uint4*)(T.fnode + rw[w].x))[gw[w]];
#pragma unroll
          for (int w = 0; w < PRED_WALKS; ++w)
            asm volatile("" : "+v"(q[w].x), "+v"(q[w].y), "+v"(q[w].z), "+v"(q[w].w));  // whole 16-byte loads
#pragma unroll
          for (int w = 0; w < PRED_WALKS; ++w) {
            const double xv = xval((int)q[w].z);
            gw[w] = xv <= __hiloint2double((int)q[w].y, (int)q[w].x) ? (int)(q[w].w & 255u) : (int)((q[w].w >> 8) & 255u);
          }
        }
#pragma unroll
        for (int w = 0; w < PRED_WALKS; ++w) {  // tree t first, then t + 1, ...: the order of the plain loop
          const int hg = rw[w].x + gw[w];
          int js = -1;
          if (T.svar != nullptr) js = T.svar[hg];
          for (int o = 0; o < K; ++o) {
            double vo = T.value[(size_t)hg * K + o];
            if (js >= 0) vo = pgb_leaf_pred(vo, T.slope[(size_t)hg * K + o], T.xbar[hg], xval(js));
            acc[o] += vo;  // (the general walk adds 1.0 * vo: the same bits)
          }
        }
        t += PRED_WALKS - 1;
        continue;
      }
    }
    const int2 rt = T.root[fi[t]];
    if (clean && !(rt.y & 0x100)) {
      const uint4* __restrict__ fn = (const uint4*)(T.fnode + rt.x);
      int gl = 0;
      for (int l = 0; l < rt.y; ++l) {
        uint4 q = fn[gl];
        asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));  // one 16-byte load, not three sunk ones
        const double xv = xval((int)q.z);
        gl = xv <= __hiloint2double((int)q.y, (int)q.x) ? (int)(q.w & 255u) : (int)((q.w >> 8) & 255u);
      }
      const int gg = rt.x + gl;
      int js = -1;
      if (T.svar != nullptr) js = T.svar[gg];
      for (int o = 0; o < K; ++o) {
        double vo = T.value[(size_t)gg * K + o];
        if (js >= 0) vo = pgb_leaf_pred(vo, T.slope[(size_t)gg * K + o], T.xbar[gg], xval(js));
        acc[o] += vo;
      }
      continue;
    }
    int g = rt.x;
    double w = 1.0;
    int sp = 0;
    for (;;) {
      // the record as two 16-byte words, requested together (a struct copy is split into per-field
      // loads that the compiler sinks to their uses: three dependent round trips per level)
      const uint4* __restrict__ np = (const uint4*)(T.node + g);
      uint4 n0 = np[0], n1 = np[1];
      // (an empty asm that "uses" all eight words: without it the loads are narrowed and sunk again)
      asm volatile("" : "+v"(n0.x), "+v"(n0.y), "+v"(n0.z), "+v"(n0.w), "+v"(n1.x), "+v"(n1.y), "+v"(n1.z), "+v"(n1.w));
      PNode nd;
      nd.var = (int32_t)n0.x; nd.left = (int32_t)n0.y; nd.right = (int32_t)n0.z; nd.flags = (int32_t)n0.w;
      nd.split = __hiloint2double((int)n1.y, (int)n1.x);
      bool done = false;  // this branch of the walk has ended
      if (nd.var < 0) {
        int js = -1;  // linear leaf; a missing / excluded regressor: the mean
        double xs = 0.0;
        if (T.svar != nullptr) {
          js = T.svar[g];
          if (js >= 0) {
            xs = xval(js);
            if (xs != xs) js = -1;
          }
        }
        for (int o = 0; o < K; ++o) {
          double vo = T.value[(size_t)g * K + o];
          if (js >= 0) vo = pgb_leaf_pred(vo, T.slope[(size_t)g * K + o], T.xbar[g], xs);
          acc[o] += w * vo;
        }
        done = true;
      } else {
        const double xv = xval(nd.var);
        if ((nd.flags & 1) || xv != xv) {
          const double cl = T.node[nd.left].cnt, cr = T.node[nd.right].cnt;
          const double tot = cl + cr;
          if (!(tot > 0.0)) {
            done = true;
          } else {  // depth-first, left first (same summation order as the oracle's recursion)
            stk_node[sp] = nd.right;
            stk_w[sp] = w * (cr / tot);
            ++sp;
            g = nd.left;
            w = w * (cl / tot);
          }
        } else {
          const bool gl = CONT ? xv <= nd.split : pgb_go_left(nd.flags >> 1, xv, nd.split) != 0;
          g = gl ? nd.left : nd.right;
        }
      }
      if (done) {
        if (sp == 0) break;
        --sp;
        g = stk_node[sp];
        w = stk_w[sp];
      }
    }
  }
}
