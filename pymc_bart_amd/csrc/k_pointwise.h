// k_pointwise.h -- part of pgbart_hip.hip and of k_pointwise_compiled.hip (not a standalone header): the pointwise
// log-likelihood of posterior draws, fused into the tree walk of k_predict (include/pgbart_pointwise.h; the numeric
// contract is include/pgbart_logpdf.h).
//
// k_pointwise has k_predict's structure -- one wave per 64 rows, the rows staged transposed in LDS for
// p <= PRED_LDS_MAXP, the walk of pgb_pred_walk.h, hence the same bits in acc -- and a per (draw, row) epilogue:
// mu_k = acc_k + offset[k][row], the log density at y[row] with the draw's parameter row (global memory, a
// wave-uniform index), the clamp, and then either or both of a store to out[d][row] and the fold into the row's
// chunk accumulator (registers), written as ONE partial record per (chunk, row) when the chunk ends.  The grid's y
// dimension is dealt whole chunks of PGB_PW_CHUNK draws, so that the records -- and k_pointwise_merge's result,
// which merges them in chunk order -- do not depend on the launch geometry.  In summary mode (out == nullptr)
// nothing of size draws x rows is written.
// The likelihood tables are read from global memory (they stay cache resident: 2.3 KB of exp / log tables, the
// probit table by row), as k_loglik_compiled_probe reads them: the LDS of a workgroup belongs to its X tile.
// The clamp count: a ballot / popcount per draw into a wave-uniform counter, one integer atomic per wave at the end.
#define PGB_PW_PSTRIDE PGB_COMPILED_MAX_PARAMS /* doubles per draw of the device's parameter table */

struct PwArgs {
  const double* params;  // [n_forests][PGB_PW_PSTRIDE]: pgb_logpdf_prepare's row, or the compiled body's params
  const double* y;       // [n_rows]
  const double* offset;  // [K][n_rows] or nullptr
  const double* aux;     // [n_rows] or nullptr (compiled bodies)
  double* out;           // [n_forests][n_rows] or nullptr
  double* partial;       // [n_chunks][4][n_rows] or nullptr
  unsigned long long* n_clamped;
  int family;
};

extern __shared__ double pw_s_x[];  // LDSX: [p][65]

// EV: raw = ev(y, mu, aux, the draw's parameter row, tables) -- the value before the clamp.  KT: the number of
// outputs when the unit knows it (compiled bodies), 0: the run-time K.
template <bool LDSX, bool CONT, int KT, class EV>
__device__ __forceinline__ void pw_body(const PredTrees& T, const int32_t* __restrict__ forest_idx, int n_forests, int m,
                                        int K_rt, int p, const double* __restrict__ X, long long n_rows, long long ldx,
                                        const PwArgs& A, EV ev) {
  const int K = KT ? KT : K_rt;
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
#ifdef PGB_PW_LDS_TABLES
  __shared__ __attribute__((aligned(16))) double pw_s_tab[PGB_LPHI_SIZE + PGB_EXPT_SIZE + PGB_LOGT_SIZE];
  for (int i = lane; i < PGB_LPHI_SIZE; i += PRED_BT) pw_s_tab[i] = pgb_tab_lphi()[i];
  for (int i = lane; i < PGB_EXPT_SIZE; i += PRED_BT) pw_s_tab[PGB_LPHI_SIZE + i] = pgb_tab_exp()[i];
  for (int i = lane; i < PGB_LOGT_SIZE; i += PRED_BT) pw_s_tab[PGB_LPHI_SIZE + PGB_EXPT_SIZE + i] = pgb_tab_log()[i];
  if constexpr (!LDSX) __syncthreads();
#endif
  if constexpr (LDSX) pred_stage_rows(pw_s_x, X, row0, n_rows, ldx, p, lane);
  if (row >= n_rows) return;  // (lane 0 always stays: row0 < n_rows)
  const PredRowX<LDSX> xval{pw_s_x, X + row * ldx, lane};
  const bool clean = pred_wave_clean<CONT>(p, xval);
  pgb_lltabs tb;
#ifdef PGB_PW_LDS_TABLES  // (the table-placement A/B of tools/pointwise_timing.py: DESIGN.md section 7; not the product)
  tb.lphi = pw_s_tab;
  tb.expt = pw_s_tab + PGB_LPHI_SIZE;
  tb.logt = pw_s_tab + PGB_LPHI_SIZE + PGB_EXPT_SIZE;
#else
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
#endif
  const double yv = A.y[row];
  const double ax = A.aux ? A.aux[row] : 0.0;
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  unsigned n_cl = 0;  // wave-uniform
  const int n_chunks = (n_forests + PGB_PW_CHUNK - 1) / PGB_PW_CHUNK;
  for (int c = blockIdx.y; c < n_chunks; c += gridDim.y) {
    const int d0 = c * PGB_PW_CHUNK;
    const int d1 = d0 + PGB_PW_CHUNK < n_forests ? d0 + PGB_PW_CHUNK : n_forests;
    pgb_pw_acc ca;
    ca.mx = ca.s = ca.mean = ca.m2 = 0.0;
    for (int d = d0; d < d1; ++d) {
      double acc[KT ? KT : PGB_MAX_OUTPUTS];
      pred_walk_forest<CONT>(T, forest_idx + (size_t)d * m, m, K, clean, xval, stk_node, stk_w, acc);
      if (A.offset != nullptr)
        for (int o = 0; o < K; ++o) acc[o] = acc[o] + A.offset[(size_t)o * n_rows + row];
      const double raw = ev(yv, acc, ax, A.params + (size_t)d * PGB_PW_PSTRIDE, &tb);
      const double v = PGB_CLAMP_LL(raw, 2047.0);  // (pgb_clamp_loglik's values: NaN -> -2047)
      n_cl += (unsigned)__popcll(__ballot(pgb_pw_is_clamped(raw)));
      if (A.out != nullptr) A.out[(size_t)d * n_rows + row] = v;
      if (A.partial != nullptr) {
        if (d == d0) pgb_pw_first(&ca, v);
        else pgb_pw_push(&ca, v, d - d0 + 1, tb.expt);
      }
    }
    if (A.partial != nullptr) {
      double* __restrict__ pr = A.partial + (size_t)c * 4 * n_rows + row;
      pr[0] = ca.mx;
      pr[(size_t)n_rows] = ca.s;
      pr[(size_t)2 * n_rows] = ca.mean;
      pr[(size_t)3 * n_rows] = ca.m2;
    }
  }
  if (n_cl != 0 && lane == 0) atomicAdd(A.n_clamped, (unsigned long long)n_cl);
}

#ifndef PGB_PW_COMPILED
struct PwBuiltin {
  int family, K;
  __device__ __forceinline__ double operator()(double y, const double* mu, double, const double* q,
                                               const pgb_lltabs* tb) const {
    return pgb_logpdf_raw(family, K, y, mu, q, tb);
  }
};
// the four walks with a run-time family, each for one output (K1: acc is a register pair -- 108 VGPRs instead of 153
// with the run-time-K array next to the family switch) and for the run-time K of the K-vector families
template <bool LDSX, bool CONT, bool K1>
__global__ __launch_bounds__(PRED_BT) void k_pointwise(PredTrees T, const int32_t* __restrict__ forest_idx, int n_forests,
                                                       int m, int K, int p, const double* __restrict__ X,
                                                       long long n_rows, long long ldx, PwArgs A) {
  pw_body<LDSX, CONT, K1 ? 1 : 0>(T, forest_idx, n_forests, m, K, p, X, n_rows, ldx, A, PwBuiltin{A.family, K1 ? 1 : K});
}

// row_stats[3][n_rows] = (lppd_i, mean_i, var_i): the row's partial records merged in chunk order
__global__ __launch_bounds__(BT) void k_pointwise_merge(const double* __restrict__ partial, int n_forests, long long n_rows,
                                                        double* __restrict__ row_stats) {
  const long long row = (long long)blockIdx.x * BT + threadIdx.x;
  if (row >= n_rows) return;
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();
  const int n_chunks = (n_forests + PGB_PW_CHUNK - 1) / PGB_PW_CHUNK;
  pgb_pw_acc tot;
  int done = 0;
  for (int c = 0; c < n_chunks; ++c) {
    const double* __restrict__ pr = partial + (size_t)c * 4 * n_rows + row;
    pgb_pw_acc b;
    b.mx = pr[0];
    b.s = pr[(size_t)n_rows];
    b.mean = pr[(size_t)2 * n_rows];
    b.m2 = pr[(size_t)3 * n_rows];
    const int nb = (c + 1) * PGB_PW_CHUNK <= n_forests ? PGB_PW_CHUNK : n_forests - c * PGB_PW_CHUNK;
    if (c == 0) tot = b;
    else pgb_pw_merge(&tot, done, &b, nb, tb.expt);
    done += nb;
  }
  double o3[3];
  pgb_pw_finish(&tot, n_forests, &tb, o3);
  row_stats[row] = o3[0];
  row_stats[(size_t)n_rows + row] = o3[1];
  row_stats[(size_t)2 * n_rows + row] = o3[2];
}
#endif
