// k_psis.h -- part of pgbart_hip.hip (not a standalone header): PSIS-LOO of the rows of a pointwise log-likelihood
// matrix on the device (pgb_psis_rows, include/pgbart_pointwise.h; the numeric contract -- every formula and the
// order of every sum -- is include/pgbart_psis.h, whose pgb_psis_row a host build evaluates to the same bits).
//
// One wave per workgroup and PSIS_ROWS = 8 adjacent rows per workgroup.  The matrix is [D][ld] with the rows
// contiguous, so the 8 rows of one draw are one 64-byte segment: the wave streams chunks of PSIS_DC draws x 8 rows
// with every lane group of 8 reading one segment, stages them transposed in LDS, and each lane then owns one draw of
// one row at a time (lane l meets the draws l mod 64 -- the contract's lane sums).  Three such passes:
//   1. the rows' minima (the shift);
//   2. the M + 1 largest x of each row: candidates above the row's running threshold are appended (ballot / popcount)
//      to the row's LDS buffer of `cap` slots; a buffer about to overflow is sorted (bitonic, (x, draw) descending) and
//      cut back to its first M + 1, whose last is the new threshold.  About (M + 1) log(D / (M + 1)) candidates pass;
//   3. the two lane sums over the draws outside the tail.
// Then, row by row: the generalised-Pareto fit with lane j on grid point b_j (the m_est x T logs, each lane its own
// plain sum over the tail in LDS), the weights, k and sigma, the smoothed tail and the tail's two lane sums (the
// tail's ll values are gathered by draw index).  No atomics, no floating-point reduction outside the contract's order.
//
// The body is one template, psis_rows<KIND>: k_psis is its instance without a second matrix (PGB_PSIS_G_NONE), and
// k_psis_expect<KIND> (pgb_psis_expect) the instances that also form the PSIS-weighted expectations of a matrix g
// [D][ldg] over the same weights (pgbart_psis.h: pgb_psis_row_expect).  They differ in four places: pass 3 also
// accumulates the lane partials of den_term x g_c; the tail stage gathers g by the draw index next to ll; the final
// stage has the two extra lane sums and the division; rows beyond n_rows repeat the last row for g and y as for ll.
// Pass 3 reads g straight from global memory -- each lane the 8 adjacent row values of its own draw, one 64-byte
// segment with every byte used -- not through a second transposed LDS tile: the tile would cost 8.5 KB per workgroup
// where LDS already bounds the occupancy (35 KB at D = 1000: 4 workgroups per CU, 3 with the tile), and g is read once.
#define PSIS_BT 64
#define PSIS_ROWS 8
#define PSIS_DC 128                 /* draws per staged chunk */
#define PSIS_TS (PSIS_DC + 8)       /* the tile's row stride in doubles (2-way bank conflicts on the transposing store) */
#define PSIS_A PGB_PSIS_MAX_TAIL    /* doubles of the tail's a_t / w_t */

extern __shared__ double psis_s[];  // tile [8][PSIS_TS] | keys [8][cap] | a [PSIS_A] | draw indices [8][cap] (16 bit)

static size_t psis_lds_bytes(int cap) {
  return (size_t)(PSIS_ROWS * PSIS_TS + PSIS_ROWS * cap + PSIS_A) * sizeof(double) + (size_t)PSIS_ROWS * cap * sizeof(uint16_t);
}

// one chunk of draws [d0, d0 + PSIS_DC) x the tile's 8 rows (rows beyond n_rows repeat the last one), coalesced
__device__ __forceinline__ void psis_load(const double* __restrict__ ll, int D, long long n_rows, long long ld, long long i0,
                                          int d0, double* tile, int lane) {
  double v[PSIS_DC * PSIS_ROWS / PSIS_BT];
#pragma unroll
  for (int q = 0; q < PSIS_DC * PSIS_ROWS / PSIS_BT; ++q) {
    const int e = q * PSIS_BT + lane;
    long long gi = i0 + (e & (PSIS_ROWS - 1));
    if (gi >= n_rows) gi = n_rows - 1;
    const int d = d0 + (e >> 3);
    v[q] = d < D ? ll[(size_t)d * (size_t)ld + (size_t)gi] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < PSIS_DC * PSIS_ROWS / PSIS_BT; ++q) {
    const int e = q * PSIS_BT + lane;
    tile[(e & (PSIS_ROWS - 1)) * PSIS_TS + (e >> 3)] = v[q];
  }
}

// cap (a power of two) slots sorted descending by pgb_psis_before; ends on a barrier
__device__ __noinline__ void psis_sort(double* key, uint16_t* idx, int cap, int lane) {
  for (int k = 2; k <= cap; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = lane; p < (cap >> 1); p += PSIS_BT) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i | j;
        const double xi = key[i], xl = key[l];
        const int di = idx[i], dl = idx[l];
        const bool sw = (i & k) == 0 ? pgb_psis_before(xl, dl, xi, di) : pgb_psis_before(xi, di, xl, dl);
        if (sw) {
          key[i] = xl;
          key[l] = xi;
          idx[i] = (uint16_t)dl;
          idx[l] = (uint16_t)di;
        }
      }
      __syncthreads();
    }
}

// the row's buffer cut back to its M + 1 largest (sorted); the threshold follows once there are that many
__device__ __forceinline__ void psis_compact(double* key, uint16_t* idx, int cap, int M, int* cnt, double* tau, int lane) {
  const int c = *cnt;
  for (int p = c + lane; p < cap; p += PSIS_BT) {
    key[p] = -pgb_psis_inf();
    idx[p] = (uint16_t)0xFFFF;
  }
  __syncthreads();
  psis_sort(key, idx, cap, lane);
  if (lane == 0) {
    if (c >= M + 1) {
      *cnt = M + 1;
      *tau = key[M];
    }
  }
  __syncthreads();
}

template <int KIND>
__device__ __forceinline__ void psis_rows(const double* ll, int D, long long n_rows, long long ld, int M, int cap, double* out,
                                          const double* g, long long ldg, const double* y) {  // (the kernels' __restrict__ holds)
  constexpr bool EXPECT = KIND != PGB_PSIS_G_NONE;
  __shared__ double s_r3[PGB_PSIS_LANES], s_r4[PGB_PSIS_LANES], s_G0[PSIS_ROWS], s_G1[PSIS_ROWS];  // (EXPECT only)
  __shared__ double s_bj[PGB_PSIS_LANES], s_Lj[PGB_PSIS_LANES], s_wj[PGB_PSIS_LANES], s_r1[PGB_PSIS_LANES], s_r2[PGB_PSIS_LANES];
  __shared__ double s_mx[PSIS_ROWS], s_cut[PSIS_ROWS], s_tau[PSIS_ROWS], s_Dn[PSIS_ROWS], s_Nn[PSIS_ROWS];
  __shared__ int s_cnt[PSIS_ROWS], s_T[PSIS_ROWS];
  const int lane = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * PSIS_ROWS;
  double* tile = psis_s;
  double* keyb = tile + PSIS_ROWS * PSIS_TS;
  double* a = keyb + (size_t)PSIS_ROWS * cap;
  uint16_t* idxb = (uint16_t*)(a + PSIS_A);
  pgb_lltabs tb;
  tb.lphi = pgb_tab_lphi();
  tb.expt = pgb_tab_exp();
  tb.logt = pgb_tab_log();

  // ---- pass 1: the shift
  {
    double mn[PSIS_ROWS];
#pragma unroll
    for (int r = 0; r < PSIS_ROWS; ++r) mn[r] = pgb_psis_inf();
    for (int d0 = 0; d0 < D; d0 += PSIS_DC) {
      psis_load(ll, D, n_rows, ld, i0, d0, tile, lane);
      __syncthreads();
      for (int sub = 0; sub < PSIS_DC; sub += PSIS_BT) {
        if (d0 + sub + lane < D) {
#pragma unroll
          for (int r = 0; r < PSIS_ROWS; ++r) {
            const double v = tile[r * PSIS_TS + sub + lane];
            mn[r] = v < mn[r] ? v : mn[r];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < PSIS_ROWS; ++r) {
      s_r1[lane] = mn[r];
      __syncthreads();
      if (lane == 0) {
        double m = s_r1[0];
        for (int l = 1; l < PSIS_BT; ++l) m = s_r1[l] < m ? s_r1[l] : m;
        s_mx[r] = -m;
        s_cnt[r] = 0;
        s_tau[r] = -pgb_psis_inf();
      }
      __syncthreads();
    }
  }

  // ---- pass 2: the M + 1 largest x of every row
  for (int d0 = 0; d0 < D; d0 += PSIS_DC) {
    psis_load(ll, D, n_rows, ld, i0, d0, tile, lane);
    __syncthreads();
    for (int sub = 0; sub < PSIS_DC; sub += PSIS_BT) {
      const int d = d0 + sub + lane;
      for (int r = 0; r < PSIS_ROWS; ++r) {
        double* key = keyb + (size_t)r * cap;
        uint16_t* idx = idxb + (size_t)r * cap;
        if (__builtin_amdgcn_readfirstlane(s_cnt[r]) + PSIS_BT > cap)
          psis_compact(key, idx, cap, M, &s_cnt[r], &s_tau[r], lane);
        const int c = s_cnt[r];
        const double x = pgb_psis_x(tile[r * PSIS_TS + sub + lane], s_mx[r]);
        const bool take = d < D && x > s_tau[r];
        const unsigned long long mask = __ballot(take);
        if (take) {
          const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
          key[pos] = x;
          idx[pos] = (uint16_t)d;
        }
        __syncthreads();  // (every lane has read the count)
        if (lane == 0) s_cnt[r] = c + __popcll(mask);
      }
      __syncthreads();
    }
  }
  for (int r = 0; r < PSIS_ROWS; ++r) {
    double* key = keyb + (size_t)r * cap;
    psis_compact(key, idxb + (size_t)r * cap, cap, M, &s_cnt[r], &s_tau[r], lane);
    const double cutoff = pgb_psis_cutoff(key[M]);
    int T = 0;
    for (int j0 = 0; j0 < M; j0 += PSIS_BT) {
      const int j = j0 + lane;
      T += __popcll(__ballot(j < M && key[j] > cutoff));
    }
    if (lane == 0) {
      s_cut[r] = cutoff;
      s_T[r] = T;
    }
  }
  __syncthreads();

  // ---- pass 3: the lane sums over the draws outside the tail
  {
    double s1[PSIS_ROWS], s2[PSIS_ROWS];
#pragma unroll
    for (int r = 0; r < PSIS_ROWS; ++r) s1[r] = s2[r] = 0.0;
    double e1[PSIS_ROWS], e2[PSIS_ROWS], yr[PSIS_ROWS];  // (EXPECT only)
    if constexpr (EXPECT) {
#pragma unroll
      for (int r = 0; r < PSIS_ROWS; ++r) {
        e1[r] = e2[r] = yr[r] = 0.0;
        if constexpr (KIND == PGB_PSIS_G_PIT) yr[r] = y[i0 + r < n_rows ? i0 + r : n_rows - 1];
      }
    }
    for (int d0 = 0; d0 < D; d0 += PSIS_DC) {
      psis_load(ll, D, n_rows, ld, i0, d0, tile, lane);
      __syncthreads();
      for (int sub = 0; sub < PSIS_DC; sub += PSIS_BT) {
        if (d0 + sub + lane < D) {
          double gq[PSIS_ROWS];  // (EXPECT only) this lane's draw of g: the tile's 8 rows, one 64-byte segment
          if constexpr (EXPECT) {
#pragma unroll
            for (int r = 0; r < PSIS_ROWS; ++r) {
              const long long gi = i0 + r < n_rows ? i0 + r : n_rows - 1;
              gq[r] = g[(size_t)(d0 + sub + lane) * (size_t)ldg + (size_t)gi];
            }
          }
#pragma unroll
          for (int r = 0; r < PSIS_ROWS; ++r) {
            const double v = tile[r * PSIS_TS + sub + lane];
            const double mx = s_mx[r], cutoff = s_cut[r];
            const double x = pgb_psis_x(v, mx);
            if (!(x > cutoff)) {
              if constexpr (EXPECT) {
                const double dt = pgb_psis_den_term(x, cutoff, &tb);
                const double gv = pgb_psis_gclamp(gq[r]);
                s1[r] = s1[r] + dt;
                s2[r] = s2[r] + pgb_psis_num_term(x, v, mx, &tb);
                e1[r] = e1[r] + dt * pgb_psis_g0(gv, yr[r], KIND);
                if constexpr (KIND == PGB_PSIS_G_VALUE) e2[r] = e2[r] + dt * (gv * gv);
              } else {
                s1[r] = s1[r] + pgb_psis_den_term(x, cutoff, &tb);
                s2[r] = s2[r] + pgb_psis_num_term(x, v, mx, &tb);
              }
            }
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < PSIS_ROWS; ++r) {
      s_r1[lane] = s1[r];
      s_r2[lane] = s2[r];
      if constexpr (EXPECT) {
        s_r3[lane] = e1[r];
        s_r4[lane] = e2[r];
      }
      __syncthreads();
      if (lane == 0) {
        s_Dn[r] = pgb_psis_lanes(s_r1);
        s_Nn[r] = pgb_psis_lanes(s_r2);
        if constexpr (EXPECT) {
          s_G0[r] = pgb_psis_lanes(s_r3);
          s_G1[r] = pgb_psis_lanes(s_r4);
        }
      }
      __syncthreads();
    }
  }

  // ---- the fit, the smoothed tail and the result, row by row
  for (int r = 0; r < PSIS_ROWS; ++r) {
    const int T = __builtin_amdgcn_readfirstlane(s_T[r]);
    const double cutoff = s_cut[r], mx = s_mx[r];
    const double* key = keyb + (size_t)r * cap;
    const uint16_t* idx = idxb + (size_t)r * cap;
    long long gi = i0 + r;
    if (gi >= n_rows) gi = n_rows - 1;
    const double ecut = pgb_exp_t(cutoff, tb.expt);
    double khat = pgb_psis_inf();
    int fit = 0;
    if (T > 4) {
      for (int t = lane; t < T; t += PSIS_BT) a[t] = pgb_exp_t(key[T - 1 - t], tb.expt) - ecut;
      __syncthreads();
      const int m_est = pgb_psis_m_est(T);
      const double q1 = a[(T + 2) / 4 - 1], aN = a[T - 1];
      if (lane < m_est) {
        const double b = pgb_psis_bj(lane + 1, m_est, q1, aN, &tb);
        double s = 0.0;
        for (int t = 0; t < T; ++t) s = s + pgb_psis_grid_term(b, a[t], &tb);
        s_bj[lane] = b;
        s_Lj[lane] = pgb_psis_Lj(b, s, T, &tb);
      }
      __syncthreads();
      if (lane < m_est) s_wj[lane] = pgb_psis_wj(s_Lj, lane, m_est, &tb);
      __syncthreads();
      const double b = pgb_psis_b(s_wj, s_bj, m_est);
      double s = 0.0;
      for (int t = lane; t < T; t += PSIS_BT) s = s + pgb_psis_grid_term(b, a[t], &tb);
      s_r1[lane] = s;
      __syncthreads();
      double k, sigma;
      fit = pgb_psis_k_sigma(b, pgb_psis_lanes(s_r1), T, &k, &sigma);
      fit = __builtin_amdgcn_readfirstlane(fit);
      __syncthreads();
      if (fit) {
        khat = k;
        for (int t = lane; t < T; t += PSIS_BT) a[t] = pgb_psis_smooth(t, T, k, sigma, ecut, &tb);
      }
    }
    if (!fit)
      for (int t = lane; t < T; t += PSIS_BT) a[t] = key[T - 1 - t];
    __syncthreads();
    double wm = cutoff, vm = -mx;
    for (int t = lane; t < T; t += PSIS_BT) {
      const double w = a[t];
      const double v = w + ll[(size_t)idx[T - 1 - t] * (size_t)ld + (size_t)gi];
      if (w > wm) wm = w;
      if (v > vm) vm = v;
    }
    s_r1[lane] = wm;
    s_r2[lane] = vm;
    __syncthreads();
    double wmax = s_r1[0], vmax = s_r2[0];
    for (int l = 1; l < PSIS_BT; ++l) {
      if (s_r1[l] > wmax) wmax = s_r1[l];
      if (s_r2[l] > vmax) vmax = s_r2[l];
    }
    __syncthreads();
    double ps = 0.0, pv = 0.0;
    if constexpr (EXPECT) {
      double yv = 0.0, pe1 = 0.0, pe2 = 0.0;
      if constexpr (KIND == PGB_PSIS_G_PIT) yv = y[gi];
      for (int t = lane; t < T; t += PSIS_BT) {
        const double w = a[t];
        const size_t dt = (size_t)idx[T - 1 - t];
        const double v = w + ll[dt * (size_t)ld + (size_t)gi];
        const double gv = pgb_psis_gclamp(g[dt * (size_t)ldg + (size_t)gi]);
        const double et = pgb_exp_t(w - wmax, tb.expt);
        ps = ps + et;
        pv = pv + pgb_exp_t(v - vmax, tb.expt);
        pe1 = pe1 + et * pgb_psis_g0(gv, yv, KIND);
        if constexpr (KIND == PGB_PSIS_G_VALUE) pe2 = pe2 + et * (gv * gv);
      }
      s_r3[lane] = pe1;
      s_r4[lane] = pe2;
    } else {
      for (int t = lane; t < T; t += PSIS_BT) {
        const double w = a[t];
        const double v = w + ll[(size_t)idx[T - 1 - t] * (size_t)ld + (size_t)gi];
        ps = ps + pgb_exp_t(w - wmax, tb.expt);
        pv = pv + pgb_exp_t(v - vmax, tb.expt);
      }
    }
    s_r1[lane] = ps;
    s_r2[lane] = pv;
    __syncthreads();
    if (lane == 0 && i0 + r < n_rows) {
      if constexpr (EXPECT) {
        const double St = pgb_psis_lanes(s_r1);
        out[i0 + r] = pgb_psis_elpd(s_Nn[r], s_Dn[r], pgb_psis_lanes(s_r2), St, mx, cutoff, vmax, wmax, &tb);
        out[(size_t)n_rows + (size_t)(i0 + r)] = khat;
        out[2 * (size_t)n_rows + (size_t)(i0 + r)] = pgb_psis_ratio(s_G0[r], pgb_psis_lanes(s_r3), s_Dn[r], St, cutoff, wmax, &tb);
        if constexpr (KIND == PGB_PSIS_G_VALUE)
          out[3 * (size_t)n_rows + (size_t)(i0 + r)] = pgb_psis_ratio(s_G1[r], pgb_psis_lanes(s_r4), s_Dn[r], St, cutoff, wmax, &tb);
      } else {
        out[i0 + r] = pgb_psis_elpd(s_Nn[r], s_Dn[r], pgb_psis_lanes(s_r2), pgb_psis_lanes(s_r1), mx, cutoff, vmax, wmax, &tb);
        out[(size_t)n_rows + (size_t)(i0 + r)] = khat;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PSIS_BT) void k_psis(const double* __restrict__ ll, int D, long long n_rows, long long ld, int M,
                                                  int cap, double* __restrict__ out) {
  psis_rows<PGB_PSIS_G_NONE>(ll, D, n_rows, ld, M, cap, out, nullptr, 0, nullptr);
}

// out [2 + n_e][n_rows]: k_psis's two rows, then E_0[, E_1] of g [D][ldg] (y [n_rows]: the PIT's observed values)
template <int KIND>
__global__ __launch_bounds__(PSIS_BT) void k_psis_expect(const double* __restrict__ ll, int D, long long n_rows, long long ld,
                                                         int M, int cap, double* __restrict__ out,
                                                         const double* __restrict__ g, long long ldg,
                                                         const double* __restrict__ y) {
  psis_rows<KIND>(ll, D, n_rows, ld, M, cap, out, g, ldg, y);
}

// a[d][k][i] = a[d][k][i] + offset[k][i]: the linear predictor of pgb_predict's [D][K][n_rows] (pgb_add_offset)
__global__ __launch_bounds__(BT) void k_add_offset(double* __restrict__ a, int D, long long per_draw,
                                                   const double* __restrict__ offset) {
  const long long step = (long long)gridDim.x * BT;
  for (int d = blockIdx.y; d < D; d += gridDim.y) {
    double* row = a + (size_t)d * (size_t)per_draw;
    for (long long e = (long long)blockIdx.x * BT + threadIdx.x; e < per_draw; e += step) row[e] = row[e] + offset[e];
  }
}

// the checks pgb_psis_rows and pgb_psis_expect share; 0 when the arguments pass
static int psis_check(const char* who, int32_t D, int64_t n_rows, int64_t ld, int32_t tail_len) {
  if (n_rows < 1 || ld < n_rows) return fail(PGB_E_INVALID, "n_rows must be >= 1 and ld >= n_rows");
  if (D < 2) return fail(PGB_E_INVALID, "PSIS needs at least 2 draws");
  if (D > PGB_PSIS_MAX_DRAWS) {
    snprintf(g_err, sizeof g_err, "%s takes at most " PGB_STR(PGB_PSIS_MAX_DRAWS) " draws, %d given (thin them: draws=)", who, (int)D);
    return PGB_E_INVALID;
  }
  if (tail_len < 1 || tail_len >= D) {
    snprintf(g_err, sizeof g_err, "tail_len must be in [1, D - 1] = [1, %d], got %d", (int)D - 1, (int)tail_len);
    return PGB_E_INVALID;
  }
  if (tail_len > PGB_PSIS_MAX_TAIL) {
    snprintf(g_err, sizeof g_err, "tail_len %d is beyond " PGB_STR(PGB_PSIS_MAX_TAIL) " (an r_eff this small with this many draws)",
             (int)tail_len);
    return PGB_E_INVALID;
  }
  if ((n_rows + PSIS_ROWS - 1) / PSIS_ROWS > 0x7FFFFFFFll) return fail(PGB_E_UNSUPPORTED, "n_rows too large for one call");
  return PGB_OK;
}
static int psis_cap(int32_t tail_len) {
  int cap = 128;
  while (cap < tail_len + 1 + PSIS_BT) cap <<= 1;
  return cap;
}

extern "C" int pgb_psis_rows(const double* ll_dev, int32_t D, int64_t n_rows, int64_t ld, int32_t tail_len, double* out_dev,
                             void* stream) {
  if (!ll_dev || !out_dev) return fail(PGB_E_INVALID, "null argument");
  const int rc = psis_check("pgb_psis_rows", D, n_rows, ld, tail_len);
  if (rc != PGB_OK) return rc;
  const long long gx = (n_rows + PSIS_ROWS - 1) / PSIS_ROWS;
  const int cap = psis_cap(tail_len);
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_psis, dim3((unsigned)gx), dim3(PSIS_BT), psis_lds_bytes(cap), sm, ll_dev, (int)D, (long long)n_rows,
                     (long long)ld, (int)tail_len, cap, out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_psis launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_psis");
  return PGB_OK;
}

extern "C" int pgb_psis_expect(const double* ll_dev, int32_t D, int64_t n_rows, int64_t ld, int32_t tail_len,
                               const double* g_dev, int64_t ldg, const double* y_dev, int32_t kind, double* out_dev,
                               void* stream) {
  if (!ll_dev || !out_dev) return fail(PGB_E_INVALID, "null argument");
  if (!g_dev) return fail(PGB_E_INVALID, "g_dev is null");
  const int rc = psis_check("pgb_psis_expect", D, n_rows, ld, tail_len);
  if (rc != PGB_OK) return rc;
  if (ldg < n_rows) return fail(PGB_E_INVALID, "ldg must be >= n_rows");
  if (kind != PGB_PSIS_G_VALUE && kind != PGB_PSIS_G_PIT) {
    snprintf(g_err, sizeof g_err, "kind must be 0 (value: E[g], E[g^2]) or 1 (PIT), got %d", (int)kind);
    return PGB_E_INVALID;
  }
  if (kind == PGB_PSIS_G_PIT && !y_dev) return fail(PGB_E_INVALID, "y_dev is null (the PIT needs the observed values)");
  const long long gx = (n_rows + PSIS_ROWS - 1) / PSIS_ROWS;
  const int cap = psis_cap(tail_len);
  hipStream_t sm = (hipStream_t)stream;
  if (kind == PGB_PSIS_G_VALUE)
    hipLaunchKernelGGL(k_psis_expect<PGB_PSIS_G_VALUE>, dim3((unsigned)gx), dim3(PSIS_BT), psis_lds_bytes(cap), sm, ll_dev, (int)D,
                       (long long)n_rows, (long long)ld, (int)tail_len, cap, out_dev, g_dev, (long long)ldg, y_dev);
  else
    hipLaunchKernelGGL(k_psis_expect<PGB_PSIS_G_PIT>, dim3((unsigned)gx), dim3(PSIS_BT), psis_lds_bytes(cap), sm, ll_dev, (int)D,
                       (long long)n_rows, (long long)ld, (int)tail_len, cap, out_dev, g_dev, (long long)ldg, y_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_psis_expect launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_psis_expect");
  return PGB_OK;
}

extern "C" int pgb_add_offset(double* a_dev, int32_t D, int32_t K, int64_t n_rows, const double* offset_dev, void* stream) {
  if (!a_dev) return fail(PGB_E_INVALID, "a_dev is null");
  if (!offset_dev) return fail(PGB_E_INVALID, "offset_dev is null");
  if (D < 1 || K < 1 || n_rows < 1) return fail(PGB_E_INVALID, "D, K and n_rows must be >= 1");
  const long long per = (long long)K * (long long)n_rows;
  long long gx = (per + BT - 1) / BT;
  if (gx > 4096) gx = 4096;
  hipStream_t sm = (hipStream_t)stream;
  hipLaunchKernelGGL(k_add_offset, dim3((unsigned)gx, (unsigned)(D < 1024 ? D : 1024)), dim3(BT), 0, sm, a_dev, (int)D, per,
                     offset_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "k_add_offset launch");
  e = hipStreamSynchronize(sm);
  if (e != hipSuccess) return fail_hip(e, "k_add_offset");
  return PGB_OK;
}
