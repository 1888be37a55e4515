// k_permimp.h -- part of pgbart_hip.hip (not a standalone header): permuted predictions of stored draws
// (include/pgbart_permimp.h holds the numeric contract, the permutation and the packer of the use lists), the kernel and
// the host side of pgb_predict_permuted.
//
//   k_permimp  one wave per workgroup, lane = row, grid = (row tiles of 64, a share of the (pick, slot) pairs); y
//              strides over the pairs as k_predict strides over its forests, so that a staged tile serves several.
//              The rows of a tile are staged in LDS as k_predict stages them when p <= PRED_LDS_MAXP and read from
//              global memory beyond that.  The walk is pred_walk_forest itself: its forest is the pair's use list and
//              its xval returns the donor value for the pair's column and the row's own value otherwise.  A (the walk
//              at the row itself) is taken once per pair and serves all repeats; per repeat one gather of the donor
//              value -- a random row of a column-major column: 64 cache lines per wave, once per walk, not per level,
//              requested one repeat ahead -- one walk and K coalesced stores.  Nobody else touches them: no atomics.
#include "pgbart_permimp.h"

// xval of a permuted row: the donor value at column c, the row's own value elsewhere
template <class XV>
struct PermRowX {
  XV own;
  int c;
  double donor;
  __device__ __forceinline__ double operator()(int j) const { return j == c ? donor : own(j); }
};

template <bool LDSX, bool CONT, bool PRED>
__global__ __launch_bounds__(PRED_BT) void k_permimp(PredTrees T, int K, int p, const double* __restrict__ X, long long nb,
                                                     long long ldx, const double* __restrict__ xcols, long long n_total,
                                                     long long first_row, const int32_t* __restrict__ cols, int q, int R,
                                                     unsigned long long seed, const int32_t* __restrict__ use_off,
                                                     const int32_t* __restrict__ use_list, int n_picks,
                                                     const double* __restrict__ f, double* __restrict__ out) {
  extern __shared__ double permimp_s_x[];  // LDSX: [p][65]
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PRED_BT;
  const long long row = row0 + lane;
  if constexpr (LDSX) pred_stage_rows(permimp_s_x, X, row0, nb, ldx, p, lane);
  if (row >= nb) return;
  const PredRowX<LDSX> xval{permimp_s_x, X + row * ldx, lane};
  const bool clean = pred_wave_clean<CONT>(p, xval);
  int stk_node[PGB_MAX_DEPTH + 2];
  double stk_w[PGB_MAX_DEPTH + 2];
  const long long n_pairs = (long long)n_picks * q;
  for (long long pair = blockIdx.y; pair < n_pairs; pair += gridDim.y) {
    const int pick = (int)(pair / q), slot = (int)(pair % q);
    const int c = cols[slot];
    const int32_t* __restrict__ list = use_list + use_off[pair];
    const int len = use_off[pair + 1] - use_off[pair];
    double a[PGB_MAX_OUTPUTS], ap[PGB_MAX_OUTPUTS];
    pred_walk_forest<CONT>(T, list, len, K, clean, xval, stk_node, stk_w, a);
    const double* __restrict__ col = xcols + (size_t)slot * (size_t)n_total;
    auto donor_of = [&](int r) {
      const pgb_perm_key key = pgb_perm_make_key(seed, (uint32_t)c, (uint32_t)r, n_total);  // (wave-uniform)
      return col[pgb_perm_apply(&key, n_total, first_row + row)];
    };
    double next = donor_of(0);
    for (int r = 0; r < R; ++r) {
      const double donor = next;
      if (r + 1 < R) next = donor_of(r + 1);  // the gather of the next repeat is in flight during this walk
      bool pclean = false;
      if (CONT) pclean = clean && __ballot(donor != donor) == 0ull;
      const PermRowX<PredRowX<LDSX>> pval{xval, c, donor};
      pred_walk_forest<CONT>(T, list, len, K, pclean, pval, stk_node, stk_w, ap);
      double* __restrict__ o_r = out + (((size_t)pair * R + r) * K) * (size_t)nb + row;
      for (int o = 0; o < K; ++o) {
        const double delta = ap[o] - a[o];
        if constexpr (PRED) o_r[(size_t)o * nb] = f[((size_t)pick * K + o) * (size_t)nb + row] + delta;
        else o_r[(size_t)o * nb] = delta;
      }
    }
  }
}

// every buffer of one call, released on every way out
struct PermimpScratch {
  int32_t* rec = nullptr;  // device: [the header's pack | the columns]
  pgb_permimp_pack pack;
  PermimpScratch() { memset(&pack, 0, sizeof pack); }
  ~PermimpScratch() {
    if (rec) (void)hipFree(rec);
    pgb_permimp_pack_free(&pack);
  }
};

static thread_local double g_permimp_ms = -1.0;
extern "C" int pgb_permimp_kernel_ms(double* ms_out) {
  if (!ms_out) return fail(PGB_E_INVALID, "null argument");
  *ms_out = g_permimp_ms;
  return PGB_OK;
}

extern "C" int pgb_predict_permuted(const pgb_tree_arrays* trees, const int32_t* forest_tree_idx, int32_t n_forests, int32_t m,
                                    const double* X_dev, int64_t nb, int32_t p, int64_t ldx, const double* xcols_dev,
                                    int64_t n_total, int64_t first_row, const int32_t* cols_host, int32_t q,
                                    int32_t n_repeats, uint64_t seed, const int32_t* picks_host, int32_t n_picks,
                                    const double* f_dev, int32_t mode, double* out_dev, void* stream) {
  PredCall pc("pgb_predict_permuted");
  pc.null(trees, "trees");
  pc.null(forest_tree_idx, "forest_tree_idx");
  pc.null(X_dev, "X_dev");
  pc.null(xcols_dev, "xcols_dev");
  pc.null(cols_host, "cols_host");
  pc.null(picks_host, "picks_host");
  pc.null(out_dev, "out_dev");
  pc.forest_dims(n_forests, m, p);
  pc.at_least_one(nb, "nb");
  pc.at_least_one(n_total, "n_total");
  pc.at_least_one(q, "q");
  pc.at_least_one(n_repeats, "n_repeats");
  pc.at_least_one(n_picks, "n_picks");
  pc.ld(ldx, p, "ldx");
  pc.require(n_total < PGB_PERMIMP_MAX_ROWS, "n_total must be below 2^62");
  pc.require(first_row >= 0 && first_row <= n_total - nb, "first_row must be >= 0 and first_row + nb <= n_total");
  long long gx = 0;
  pc.tiles(nb, &gx);
  pc.require(n_repeats <= PGB_PERMIMP_MAX_REPEATS, "n_repeats must be <= " PGB_STR(PGB_PERMIMP_MAX_REPEATS));
  pc.require(mode == PGB_PERMIMP_PRED || mode == PGB_PERMIMP_DELTA, "mode must be PGB_PERMIMP_PRED or PGB_PERMIMP_DELTA");
  pc.require(mode != PGB_PERMIMP_PRED || f_dev != nullptr, "f_dev is null in mode PGB_PERMIMP_PRED");
  pc.require(mode != PGB_PERMIMP_DELTA || f_dev == nullptr, "f_dev must be null in mode PGB_PERMIMP_DELTA");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.index_vector(cols_host, (size_t)q, p, "cols_host", "p");
  pc.distinct(cols_host, q);
  pc.index_vector(picks_host, (size_t)n_picks, n_forests, "picks_host", "n_forests");
  if (pc.rc() != PGB_OK) return pc.rc();
  pc.n_outputs(trees);
  const int K = trees->n_outputs;
  pc.cells_fit({n_picks, q, n_repeats, K, nb}, "n_picks x q x n_repeats x K x nb");
  if (pc.rc() != PGB_OK) return pc.rc();
  int rc = pred_validate(trees, forest_tree_idx, n_forests, m, p);
  if (rc != PGB_OK) return rc;

  PermimpScratch sc;
  const int prc = pgb_permimp_pack_build(trees, forest_tree_idx, m, p, cols_host, q, picks_host, n_picks, &sc.pack);  // once per call
  if (prc == -1) return pc.refuse(PGB_E_NOMEM, "the use lists do not fit host memory");
  if (prc != 0) return pc.refuse(PGB_E_INVALID, "the use lists hold more than 2^31 - 1 trees");
  hipStream_t sm = (hipStream_t)stream;
  PredPack pk;
  rc = pred_pack(trees, forest_tree_idx, n_forests, m, p, nullptr, 0, sm, &pk);
  if (rc != PGB_OK) return rc;
  const size_t n_pack = (size_t)(sc.pack.n_lists + 1 + sc.pack.n_list);
  std::vector<int32_t> hb(n_pack + (size_t)q);
  memcpy(hb.data(), sc.pack.buf, n_pack * sizeof(int32_t));
  memcpy(hb.data() + n_pack, cols_host, (size_t)q * sizeof(int32_t));
  HIPCHK(hipMalloc((void**)&sc.rec, hb.size() * sizeof(int32_t)));
  HIPCHK(hipMemcpyAsync(sc.rec, hb.data(), hb.size() * sizeof(int32_t), hipMemcpyHostToDevice, sm));
  const int32_t* off_dev = sc.rec;
  const int32_t* list_dev = sc.rec + sc.pack.n_lists + 1;
  const int32_t* cols_dev = sc.rec + n_pack;
  // one wave per workgroup; enough workgroups to fill the chip (pgb_predict's figure), each looping over its share of
  // the (pick, slot) pairs
  const long long n_pairs = (long long)n_picks * q;
  const long long want_wgs = p <= PRED_LDS_MAXP ? 16384 : 4096;
  long long gy = (want_wgs + gx - 1) / gx;
  if (gy > n_pairs) gy = n_pairs;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  dim3 grid((unsigned)gx, (unsigned)gy);
  const bool ldsx = p <= PRED_LDS_MAXP;
  const size_t lds = ldsx ? (size_t)p * 65 * sizeof(double) : 0;
  WalkTimer wt(sm);
  dispatch_bools(ldsx, pk.cont, mode == PGB_PERMIMP_PRED, [&](auto L, auto C, auto P) {
    hipLaunchKernelGGL((k_permimp<L(), C(), P()>), grid, dim3(PRED_BT), lds, sm, pk.T, K, (int)p, X_dev, (long long)nb,
                       (long long)ldx, xcols_dev, (long long)n_total, (long long)first_row, cols_dev, (int)q, (int)n_repeats,
                       (unsigned long long)seed, off_dev, list_dev, (int)n_picks, f_dev, out_dev);
  });
  return finish_walk(hipGetLastError(), sm, wt, &g_permimp_ms, "k_permimp");
}
