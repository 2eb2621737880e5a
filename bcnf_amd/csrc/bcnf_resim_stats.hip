// The two reductions notebooks/resimulation.ipynb makes of the re-simulated positions x (N, M, S, 3) float64 that
// bcnf_resimulate leaves in HBM (psaegert/bcnf), over the draw axis, so that the positions never go to the host:
//
//   bcnf_resim_error_median
//       err[i][s] = np.nanmedian(np.nanmean((x - observed[:, None])**2, axis=3), axis=1)[i][s]
//   bcnf_resim_impacts
//       the (draw, step) pairs of np.where(np.diff((x[i, :, :, 2] > 0).astype(int), axis=1) == -1), the positions
//       there and their np.histogram2d over one edge table per trajectory
//
// Both are exact restatements (the same IEEE operations in the same order, no tolerance): the median is a SORT of the
// per-draw values, not an estimate, and the histogram is integer counting. See include/bcnf_amd.h for the contract.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bcnf_amd.h"
#include "bcnf_device.h"

// numpy rounds the subtract, the square and each add on its own; hipcc contracts a * b + c by default
#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Resimulation error. One workgroup per (trajectory i, tile of TS time steps). The per-draw values
//   v[j][s] = (sum over the non-NaN k of (x[i][j][s][k] - observed[i][s][k])^2, k = 0, 1, 2 in that order) / count
// are >= +0 or NaN, so their bit patterns order like unsigned 64-bit integers; NaN (count = 0) becomes the key
// ~0, above +inf (0x7ff0...). The M keys of each of the tile's columns are staged in LDS, padded with ~0 to
// P = the next power of two, and sorted by a bitonic network (every compare-exchange is exact and its outcome
// does not depend on thread timing: the same bits every run). The c non-NaN keys are then the first c of the column.
// ---------------------------------------------------------------------------------------------------------------
constexpr unsigned long long NAN_KEY = ~0ULL;
constexpr int ERR_TILE_BYTES = 32 * 1024;     // LDS per workgroup while a column fits: 5 workgroups / CU
constexpr int ERR_MAX_TILE = 8;               // time steps per workgroup at most
constexpr int ERR_WG = 256, ERR_WG_BIG = 1024;

template <typename TO>
__global__ __launch_bounds__(ERR_WG_BIG) void k_resim_error(const double* __restrict__ x, const TO* __restrict__ obs,
                                                           long long M, int S, int P, int TS, int ntiles,
                                                           double* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];     // [TS][P]
  const long long i = blockIdx.x / ntiles;
  const int s0 = (int)(blockIdx.x - i * ntiles) * TS;
  const int ts = S - s0 < TS ? S - s0 : TS;
  const double* xi = x + i * M * S * 3;
  const TO* oi = obs + i * (long long)S * 3;
  // stage: consecutive threads take consecutive (j, s) of the tile = consecutive 24-byte runs of x
  for (int e = threadIdx.x; e < P * ts; e += blockDim.x) {
    const int j = e / ts, sl = e - j * ts;
    unsigned long long key = NAN_KEY;
    if (j < M) {
      const double* p = xi + ((long long)j * S + s0 + sl) * 3;
      const TO* o = oi + (s0 + sl) * 3;
      double sum = 0.0;
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double d = __dsub_rn(p[k], (double)o[k]);
        const double sq = __dmul_rn(d, d);
        if (sq == sq) {
          sum = __dadd_rn(sum, sq);
          ++cnt;
        }
      }
      if (cnt) {
        const double v = __ddiv_rn(sum, (double)cnt);
        key = (unsigned long long)__double_as_longlong(v);    // v >= +0 or +inf: never NaN, never negative
      }
    }
    keys[sl * P + j] = key;
  }
  __syncthreads();
  // bitonic sort of each of the ts columns, ascending
  const int half = P >> 1, pairs = half * ts, lh = half ? __builtin_ctz(half) : 0;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = threadIdx.x; q < pairs; q += blockDim.x) {
        const int col = q >> lh, r = q & (half - 1);
        const int lo = ((r & ~(j - 1)) << 1) | (r & (j - 1)), hi = lo | j;
        unsigned long long* c = keys + col * P;
        const unsigned long long a = c[lo], b = c[hi];
        if ((a > b) == ((lo & k) == 0)) {
          c[lo] = b;
          c[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  if ((int)threadIdx.x < ts) {
    const unsigned long long* c = keys + threadIdx.x * P;
    int lo = 0, hi = P;                       // first index holding NAN_KEY = the number of non-NaN draws
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (c[mid] == NAN_KEY) hi = mid; else lo = mid + 1;
    }
    double r = __builtin_nan("");
    if (lo & 1) {
      r = __longlong_as_double((long long)c[lo >> 1]);
    } else if (lo) {
      const double a = __longlong_as_double((long long)c[(lo >> 1) - 1]);
      const double b = __longlong_as_double((long long)c[lo >> 1]);
      r = __ddiv_rn(__dadd_rn(a, b), 2.0);
    }
    err[i * S + s0 + threadIdx.x] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Impacts. One workgroup per trajectory i; a wave takes 64 consecutive draws at a time, and for each of them its
// lanes take 64 consecutive time steps: lane l of chunk c looks at s = 64 c + l and decides
//   above[s] && !above[s + 1]   (s + 1 < S; above = z > 0, false for NaN)
// -- np.diff(...) == -1 at index s. A ballot gives the draw's transitions of the chunk as a 64-bit mask: its lowest
// set bit is the first one, its population count their number. Lanes that hold a transition bin (x, y) there into the
// workgroup's LDS histogram with integer LDS atomics (exact, order-independent). Lane d of the wave keeps the result
// of draw d of the batch, so the per-draw outputs leave as coalesced stores. The workgroup owns hist[i] and writes it
// with plain stores.
// ---------------------------------------------------------------------------------------------------------------
constexpr int IMP_WG = 1024;
constexpr int IMP_U = 4;       // draws whose loads are issued together

// np.searchsorted(edges, v, 'right') - 1 with the last edge included in the last bin; -1 = outside (or NaN)
__device__ __forceinline__ int edge_bin(const double* __restrict__ edges, int E, double v) {
  if (!(v >= edges[0]) || !(v <= edges[E - 1])) return -1;
  int lo = 0, hi = E;            // first index with edges[idx] > v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo == E ? E - 2 : lo - 1;
}

__global__ __launch_bounds__(IMP_WG) void k_resim_impacts(const double* __restrict__ x, long long M, int S,
                                                         const double* __restrict__ edges, int E,
                                                         int32_t* __restrict__ step, double* __restrict__ position,
                                                         int32_t* __restrict__ transitions,
                                                         int32_t* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double* sedge = reinterpret_cast<double*>(lds_raw);                 // [E]
  int* sh = reinterpret_cast<int*>(lds_raw + (size_t)E * 8);          // [(E - 1)^2]
  const int nb = E - 1, nh = nb * nb;
  const long long i = blockIdx.x;
  const double* xi = x + i * M * S * 3;
  const bool do_hist = hist != nullptr;
  if (do_hist) {
    for (int e = threadIdx.x; e < E; e += blockDim.x) sedge[e] = edges[e];
    for (int e = threadIdx.x; e < nh; e += blockDim.x) sh[e] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int nchunks = (S + 63) >> 6;
  for (long long j0 = (long long)wave * 64; j0 < M; j0 += (long long)nwaves * 64) {      // wave-uniform
    const int nd = M - j0 < 64 ? (int)(M - j0) : 64;
    int my_step = -1, my_cnt = 0;
    for (int d0 = 0; d0 < nd; d0 += IMP_U) {
      int st[IMP_U], cn[IMP_U];
#pragma unroll
      for (int u = 0; u < IMP_U; ++u) {
        st[u] = -1;
        cn[u] = 0;
      }
      for (int c = 0; c < nchunks; ++c) {
        const int s = c * 64 + lane;
        double za[IMP_U], zb[IMP_U];
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) {
          const int d = d0 + u < nd ? d0 + u : nd - 1;          // past the batch: a copy, not counted
          const double* p = xi + (j0 + d) * S * 3;
          za[u] = s < S ? p[3 * s + 2] : 0.0;
          zb[u] = s + 1 < S ? p[3 * (s + 1) + 2] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) {
          const bool tr = d0 + u < nd && s + 1 < S && za[u] > 0.0 && !(zb[u] > 0.0);
          const unsigned long long m = __ballot(tr);
          if (m) {
            if (st[u] < 0) st[u] = c * 64 + __ffsll((long long)m) - 1;
            cn[u] += __popcll(m);
            if (tr && do_hist) {
              const double* p = xi + ((j0 + d0 + u) * S + s) * 3;
              const int bx = edge_bin(sedge, E, p[0]), by = edge_bin(sedge, E, p[1]);
              if (bx >= 0 && by >= 0) atomicAdd(sh + bx * nb + by, 1);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < IMP_U; ++u) {
        if (lane == d0 + u) {
          my_step = st[u];
          my_cnt = cn[u];
        }
      }
    }
    if (lane < nd) {
      const long long o = i * M + j0 + lane;
      step[o] = my_step;
      transitions[o] = my_cnt;
      double pos[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
      if (my_step >= 0) {
        const double* p = xi + ((j0 + lane) * S + my_step) * 3;
        pos[0] = p[0];
        pos[1] = p[1];
        pos[2] = p[2];
      }
      position[o * 3 + 0] = pos[0];
      position[o * 3 + 1] = pos[1];
      position[o * 3 + 2] = pos[2];
    }
  }
  if (do_hist) {
    __syncthreads();
    int32_t* h = hist + i * nh;
    for (int e = threadIdx.x; e < nh; e += blockDim.x) h[e] = sh[e];
  }
}

}  // namespace

extern "C" {

int bcnf_resim_error_median(const double* x, const void* observed, int32_t observed_f64, int64_t n_traj,
                            int64_t n_draws, int32_t steps, double* err, void* stream) {
  if (n_traj < 0 || n_draws < 0 || steps < 1) return BCNF_ERR_ARG;
  if (n_draws > BCNF_RESIM_ERROR_MAX_DRAWS) return BCNF_ERR_UNSUPPORTED;
  if (n_traj == 0 || n_draws == 0) return BCNF_OK;
  if (!x || !observed || !err) return BCNF_ERR_ARG;
  int P = 1;
  while (P < n_draws) P <<= 1;
  int TS = ERR_TILE_BYTES / (P * 8);
  TS = TS < 1 ? 1 : TS > ERR_MAX_TILE ? ERR_MAX_TILE : TS;
  if (TS > steps) TS = steps;
  const int ntiles = (steps + TS - 1) / TS;
  const long long nwg = (long long)n_traj * ntiles;
  if (nwg > 0x7fffffffLL) return BCNF_ERR_UNSUPPORTED;
  const size_t lds = (size_t)P * TS * 8;
  const int wg = lds > (size_t)ERR_TILE_BYTES ? ERR_WG_BIG : ERR_WG;
  const bcnf_rt::Lds L(lds, (size_t)BCNF_RESIM_ERROR_MAX_DRAWS * 8);
  return observed_f64
             ? bcnf_rt::launch<k_resim_error<double>>(dim3((unsigned)nwg), dim3(wg), L, (hipStream_t)stream, x,
                                                      (const double*)observed, (long long)n_draws, steps, P, TS,
                                                      ntiles, err)
             : bcnf_rt::launch<k_resim_error<float>>(dim3((unsigned)nwg), dim3(wg), L, (hipStream_t)stream, x,
                                                     (const float*)observed, (long long)n_draws, steps, P, TS, ntiles,
                                                     err);
}

int bcnf_resim_impacts(const double* x, int64_t n_traj, int64_t n_draws, int32_t steps, const double* edges,
                       int32_t n_edges, int32_t* step, double* position, int32_t* transitions, int32_t* hist,
                       void* stream) {
  if (n_traj < 0 || n_draws < 0 || steps < 1) return BCNF_ERR_ARG;
  if ((edges != nullptr) != (hist != nullptr)) return BCNF_ERR_ARG;
  if (edges && n_edges < 2) return BCNF_ERR_ARG;
  if (edges && n_edges > BCNF_RESIM_HIST_MAX_EDGES) return BCNF_ERR_UNSUPPORTED;
  if (n_traj == 0 || n_draws == 0) return BCNF_OK;
  if (!x || !step || !position || !transitions) return BCNF_ERR_ARG;
  if (n_traj > 0x7fffffffLL) return BCNF_ERR_UNSUPPORTED;
  const int E = edges ? n_edges : 0;
  const size_t lds = edges ? (size_t)E * 8 + (size_t)(E - 1) * (E - 1) * 4 : 0;
  const size_t top = (size_t)BCNF_RESIM_HIST_MAX_EDGES * 8 +
                     (size_t)(BCNF_RESIM_HIST_MAX_EDGES - 1) * (BCNF_RESIM_HIST_MAX_EDGES - 1) * 4;
  return bcnf_rt::launch<k_resim_impacts>(dim3((unsigned)n_traj), dim3(IMP_WG), bcnf_rt::Lds(lds, top),
                                          (hipStream_t)stream, x, (long long)n_draws, steps, edges, E, step, position,
                                          transitions, hist);
}

}  // extern "C"
