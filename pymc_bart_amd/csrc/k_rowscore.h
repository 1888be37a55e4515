// k_rowscore.h -- part of pgbart_hip.hip (not a standalone header; after k_rowsummary.h): what the scoring rules of the
// posterior predictive are made of, for every column of a [D][ld] device matrix of replicated observations against the
// column's observed y (pgb_row_score; the numeric contract -- the order, every formula and the order of every sum --
// is include/pgbart_score.h, whose pgb_score_column a host build evaluates to the same bits).
//
// The geometry is k_rowsum's (k_rowsummary.h): 256 threads own C = max(1, min(8, 16384 / Dp)) adjacent columns, their
// C x Dp order keys live in dynamic LDS (at most 128 KiB, an opt-in), and stages 1 and 2 -- the tile load with its
// padding and the ONE bitonic network over all columns -- are that file's rowsum_load_tile and rowsum_sort_tile.
//   3. values: the keys become the doubles t in place (no offset, no transform);
//   4. statistics: one wave per column.  Lane l forms partial l of the four lane sums (mean, variance, |t - y|, the
//      gap form of the pair sum), the partials go through LDS and are combined in lane order by the contract's own
//      pgb_rowsum_lanes; the two counts are integers and are added across the wave by shuffles; lane j gathers
//      quantile j and its pinball loss.
// No atomics, no floating-point reduction outside the contract's order.

__global__ __launch_bounds__(ROWSUM_BT) void k_rowscore(const double* __restrict__ a, int D, int lg, int lgC, long long n_cols,
                                                        long long ld, const double* __restrict__ y, rowsum_q qs, int n_q,
                                                        double* __restrict__ out) {
  __shared__ double s_part[3][ROWSUM_WAVES][PGB_ROWSUM_LANES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Dp = 1 << lg, C = 1 << lgC;
  const int total = C << lg;
  const long long c0 = (long long)blockIdx.x << lgC;
  unsigned long long* keys = rowsum_keys;

  rowsum_load_tile(keys, a, D, lg, lgC, c0, n_cols, ld);  // ---- 1. the tile's keys, the padding
  rowsum_sort_tile(keys, lg, lgC);                        // ---- 2. every column ascending

  // ---- 3. t, in place
  double* tv = (double*)rowsum_keys;
  for (int i = tid; i < total; i += ROWSUM_BT)
    if ((i & (Dp - 1)) < D) tv[i] = pgb_rowsum_unkey(keys[i]);
  __syncthreads();

  // ---- 4. one wave per column (every wave takes every barrier: a wave without a column repeats column 0)
  for (int cb = 0; cb < C; cb += ROWSUM_WAVES) {
    const int c = cb + wave;
    const bool act = c < C && c0 + c < n_cols;
    const double* t = tv + ((size_t)(act ? c : 0) << lg);
    const double yv = y[c0 + (act ? c : 0)];
    // the three sums that need nothing but t and y: lane k < 3 ends sum k, the others repeat sum 0
    s_part[0][wave][lane] = pgb_rowsum_part_sum(t, D, lane);
    s_part[1][wave][lane] = pgb_score_part_abs(t, D, lane, yv);
    s_part[2][wave][lane] = pgb_score_part_pair(t, D, lane);
    __syncthreads();
    const double s3 = pgb_rowsum_lanes(s_part[lane < 3 ? lane : 0][wave]);
    const double mean = __shfl(s3, 0, 64) / (double)D;
    const double abs_err = __shfl(s3, 1, 64) / (double)D;
    const double pair_sum = __shfl(s3, 2, 64);
    __syncthreads();
    s_part[0][wave][lane] = pgb_rowsum_part_sq(t, D, lane, mean);
    __syncthreads();
    const double var = pgb_rowsum_lanes(s_part[0][wave]) / (double)(D - 1);
    __syncthreads();
    int32_t below, equal;
    pgb_score_part_counts(t, D, lane, yv, &below, &equal);
    for (int m = 32; m > 0; m >>= 1) {
      below += __shfl_xor(below, m, 64);
      equal += __shfl_xor(equal, m, 64);
    }
    if (act) {
      const size_t col = (size_t)(c0 + c), n = (size_t)n_cols;
      if (lane == 0) {
        out[(size_t)PGB_SCORE_MEAN * n + col] = mean;
        out[(size_t)PGB_SCORE_VAR * n + col] = var;
        out[(size_t)PGB_SCORE_ABS_ERR * n + col] = abs_err;
        out[(size_t)PGB_SCORE_PAIR_SUM * n + col] = pair_sum;
        out[(size_t)PGB_SCORE_N_BELOW * n + col] = (double)below;
        out[(size_t)PGB_SCORE_N_EQUAL * n + col] = (double)equal;
      }
      if (lane < n_q) {
        const double qv = pgb_rowsum_quantile(t, D, qs.q[lane]);
        out[(size_t)(PGB_SCORE_NFIXED + lane) * n + col] = qv;
        out[(size_t)(PGB_SCORE_NFIXED + n_q + lane) * n + col] = pgb_score_pinball(yv, qv, qs.q[lane]);
      }
    }
  }
}

extern "C" int pgb_row_score(const double* a_dev, int32_t D, int64_t n_cols, int64_t ld, const double* y_dev,
                             const double* q_host, int32_t n_q, double* out_dev, void* stream) {
  if (!a_dev || !y_dev || !out_dev) return fail(PGB_E_INVALID, "null argument");
  if (n_cols < 1 || ld < n_cols) return fail(PGB_E_INVALID, "n_cols must be >= 1 and ld >= n_cols");
  if (D < 2) return fail(PGB_E_INVALID, "a row score needs at least 2 draws");
  if (D > PGB_ROWSUM_MAX_DRAWS) {
    snprintf(g_err, sizeof g_err, "pgb_row_score takes at most " PGB_STR(PGB_ROWSUM_MAX_DRAWS) " draws, %d given (thin them: draws=)",
             (int)D);
    return PGB_E_INVALID;
  }
  if (n_q < 0 || n_q > PGB_ROWSUM_MAX_Q) {
    snprintf(g_err, sizeof g_err, "n_q must be in [0, " PGB_STR(PGB_ROWSUM_MAX_Q) "], got %d", (int)n_q);
    return PGB_E_INVALID;
  }
  if (n_q > 0 && !q_host) return fail(PGB_E_INVALID, "null argument");
  rowsum_q qs;
  for (int j = 0; j < PGB_ROWSUM_MAX_Q; ++j) qs.q[j] = 0.0;
  for (int j = 0; j < n_q; ++j) {
    if (!(q_host[j] >= 0.0 && q_host[j] <= 1.0)) {
      snprintf(g_err, sizeof g_err, "level %d must be in [0, 1], got %g", j, q_host[j]);
      return PGB_E_INVALID;
    }
    qs.q[j] = q_host[j];
  }
  rowsum_tiling g;
  int rc = rowsum_tile(D, n_cols, &g);
  if (rc != PGB_OK) return rc;
  static std::vector<int> opted;
  rc = rowsum_lds_opt_in((const void*)k_rowscore, &opted, "k_rowscore: dynamic LDS opt-in");
  if (rc != PGB_OK) return rc;
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rowscore, dim3((unsigned)g.gx), dim3(ROWSUM_BT), g.lds, sm, a_dev, (int)D, g.lg, g.lgC, (long long)n_cols,
                     (long long)ld, y_dev, qs, (int)n_q, out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_rowscore launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_rowscore");
  return PGB_OK;
}
