// k_surv.h -- part of pgbart_hip.hip (not a standalone header): discrete-time survival curves of stored draws
// (include/pgbart_surv.h holds the numeric contract and the sequential reference), the kernel and the host side of
// pgb_surv_curves.
//
//   k_surv<Q>   one lane per (d, i), i fastest: blockIdx.x tiles the rows, blockIdx.y strides over the draws, so every
//               load and store of a wave is coalesced (8 bytes per lane, 512 contiguous bytes per wave).  A lane runs
//               over the A times of the call in order: the multiply chain S = S * q is sequential, its loads are not --
//               SURV_PF of them are issued before the first is used.  S, R and T[0 .. Q) stay in registers: Q is a
//               template argument and the loop over the levels is fully unrolled, so T is never indexed at run time
//               (no scratch).  The grid and its widths arrive as kernel arguments and are read with wave-uniform
//               indices (scalar loads); the levels are named fields.  One 64-bit atomic per lane that met a non-finite
//               q, none otherwise; no LDS, no barrier.  16 bytes of traffic per element: f in, S out.
#include "pgbart_surv.h"

#define SURV_BT 256
#define SURV_PF 8

struct SurvGrid {  // the times of one call and their widths
  double t[PGB_ARMS_MAX];
  double dt[PGB_ARMS_MAX];
};

template <int Q>
__global__ __launch_bounds__(SURV_BT) void k_surv(double* __restrict__ f, long long lda, long long ldd, int D, int A, long long nb,
                                                  const double* __restrict__ off, int transform, pgb_surv_levels lv,
                                                  double beyond, int init, double* __restrict__ state,
                                                  unsigned long long* __restrict__ cnt, SurvGrid grid) {
  const long long i = (long long)blockIdx.x * SURV_BT + threadIdx.x;
  if (i >= nb) return;
  const pgb_lltabs tb = arms_tabs();
  const int has_off = off != nullptr;
  const double off_i = has_off ? off[i] : 0.0;
  const size_t slab = (size_t)D * (size_t)nb;
  unsigned long long n_nonfinite = 0;
  for (int d = blockIdx.y; d < D; d += gridDim.y) {
    double* __restrict__ fd = f + (size_t)d * (size_t)ldd + i;
    double* __restrict__ sd = state + (size_t)d * (size_t)nb + i;
    pgb_surv_state st;
    pgb_surv_start(&st, beyond);
    if (!init) {
      st.S = sd[PGB_SURV_S * slab];
      st.R = sd[PGB_SURV_R * slab];
#pragma unroll
      for (int l = 0; l < Q; ++l) st.T[l] = sd[PGB_SURV_T(l) * slab];
    }
    for (int a0 = 0; a0 < A; a0 += SURV_PF) {
      double v[SURV_PF];
#pragma unroll
      for (int j = 0; j < SURV_PF; ++j) v[j] = a0 + j < A ? fd[(size_t)(a0 + j) * (size_t)lda] : 0.0;  // (wave-uniform)
#pragma unroll
      for (int j = 0; j < SURV_PF; ++j) {
        if (a0 + j < A) {
          int nonfinite;
          fd[(size_t)(a0 + j) * (size_t)lda] =
              pgb_surv_step(&st, v[j], has_off, off_i, transform, &tb, grid.t[a0 + j], grid.dt[a0 + j], &lv, Q, beyond, &nonfinite);
          n_nonfinite += nonfinite ? 1 : 0;
        }
      }
    }
    sd[PGB_SURV_S * slab] = st.S;
    sd[PGB_SURV_R * slab] = st.R;
#pragma unroll
    for (int l = 0; l < Q; ++l) sd[PGB_SURV_T(l) * slab] = st.T[l];
  }
  if (n_nonfinite) atomicAdd(cnt, n_nonfinite);
}

static thread_local double g_surv_ms = -1.0;
extern "C" int pgb_surv_kernel_ms(double* ms_out) {
  if (!ms_out) return fail(PGB_E_INVALID, "null argument");
  *ms_out = g_surv_ms;
  return PGB_OK;
}

extern "C" int pgb_surv_curves(double* f_dev, int64_t lda, int64_t ldd, int32_t D, int32_t A, int64_t nb, const double* off_dev,
                               int32_t transform, const double* t_host, const double* dt_host, const double* u_host, int32_t Q,
                               double beyond, int32_t init, double* state_dev, uint64_t* n_nonfinite_dev, void* stream) {
  PredCall pc("pgb_surv_curves");
  pc.null(f_dev, "f_dev");
  pc.null(t_host, "t_host");
  pc.null(dt_host, "dt_host");
  pc.null(state_dev, "state_dev");
  pc.null(n_nonfinite_dev, "n_nonfinite_dev");
  pc.at_least_one(D, "D");
  pc.at_least_one(A, "A");
  pc.at_least_one(nb, "nb");
  pc.require(A <= PGB_ARMS_MAX, "A must be <= PGB_ARMS_MAX = " PGB_STR(PGB_ARMS_MAX));
  pc.require(Q >= 0 && Q <= PGB_SURV_MAX_LEVELS, "Q must be in [0, PGB_SURV_MAX_LEVELS = " PGB_STR(PGB_SURV_MAX_LEVELS) "]");
  pc.require(nb <= ((int64_t)1 << 38), "nb must be <= 2^38");  // (the x extent of the grid stays below 2^31)
  if (pc.rc() != PGB_OK) return pc.rc();
  if (Q > 0) pc.null(u_host, "u_host");
  pc.require(ldd >= nb, "ldd must be >= nb");
  pc.require(ldd <= ((int64_t)1 << 45) && lda <= ((int64_t)1 << 50), "lda or ldd overflows the index arithmetic");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.require(lda >= (int64_t)(D - 1) * ldd + nb, "lda must be >= (D - 1) ldd + nb");
  pc.require(transform == PGB_ROWSUM_LOGISTIC || transform == PGB_ROWSUM_PROBIT,
             "transform must be PGB_ROWSUM_LOGISTIC or PGB_ROWSUM_PROBIT");
  for (int a = 0; pc.rc() == PGB_OK && a < A; ++a) {
    if (!std::isfinite(t_host[a])) pc.refuse(PGB_E_INVALID, "t_host[%d] is not finite", a);
    else if (!(std::isfinite(dt_host[a]) && dt_host[a] > 0.0)) pc.refuse(PGB_E_INVALID, "dt_host[%d] must be finite and > 0", a);
    else if (a > 0 && !(t_host[a] > t_host[a - 1])) pc.refuse(PGB_E_INVALID, "t_host[%d] must be > t_host[%d]", a, a - 1);
  }
  for (int l = 0; pc.rc() == PGB_OK && l < Q; ++l)
    if (!(u_host[l] > 0.0 && u_host[l] <= 1.0)) pc.refuse(PGB_E_INVALID, "u_host[%d] must lie in (0, 1]", l);
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.require(std::isfinite(beyond) && beyond > t_host[A - 1], "beyond must be finite and > t_host[A - 1]");
  pc.cells_fit({2 + Q, D, nb}, "(2 + Q) x D x nb (the state)");
  if (pc.rc() != PGB_OK) return pc.rc();

  hipStream_t sm = (hipStream_t)stream;
  SurvGrid grid;
  pgb_surv_levels lv;
  for (int a = 0; a < PGB_ARMS_MAX; ++a) {
    grid.t[a] = a < A ? t_host[a] : 0.0;
    grid.dt[a] = a < A ? dt_host[a] : 0.0;
  }
  for (int l = 0; l < PGB_SURV_MAX_LEVELS; ++l) lv.u[l] = l < Q ? u_host[l] : 1.0;
  const long long bx = (nb + SURV_BT - 1) / SURV_BT;
  long long by = (16384 + bx - 1) / bx;  // enough workgroups to fill the chip, each striding over its draws
  if (by > D) by = D;
  if (by > 65535) by = 65535;
  const dim3 g((unsigned)bx, (unsigned)by), b(SURV_BT);
  unsigned long long* cnt = (unsigned long long*)n_nonfinite_dev;
  WalkTimer wt(sm);
  auto launch = [&](auto q) {
    hipLaunchKernelGGL((k_surv<decltype(q)::value>), g, b, 0, sm, f_dev, (long long)lda, (long long)ldd, (int)D, (int)A,
                       (long long)nb, off_dev, (int)transform, lv, beyond, (int)init, state_dev, cnt, grid);
  };
  switch (Q) {
    case 0: launch(std::integral_constant<int, 0>{}); break;
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    default: launch(std::integral_constant<int, 4>{}); break;
  }
  return finish_walk(hipGetLastError(), sm, wt, &g_surv_ms, "k_surv");
}
