// Transformer feature networks (feature_network.py: MultiHeadAttention, TransformerBlock): the two pieces that are not
// a Linear layer, for the short sequences the run configs use (S = 30 time steps, 16 rfft bins; head_dim 4 .. 32).
//
//   attention core    out = softmax(q k^T / sqrt(hd)) v per (sample, head), straight on the (B, S, heads * hd) outputs of
//                     the q / k / v Linear layers: head h is columns h hd .. h hd + hd - 1, so neither the head split
//                     nor the head concatenation exists as a copy. Lane i of a (sample, head) slot owns query row i;
//                     keys and values are LDS broadcasts; scores, softmax and the output row stay in the lane's
//                     registers -- no cross-lane traffic. The forward saves the per-row log-sum-exp, the backward
//                     recomputes the probabilities from it.
//   residual + norm   y = LayerNorm(x + r): one wave per row, the row in registers, two-pass mean / biased variance.
//
// fp32 throughout, stream-ordered, no state, no allocation, every sum in a fixed order (same inputs -> same bits).
#include "bcnf_device.h"

namespace {

constexpr int AWAVES = 4;              // waves per workgroup
constexpr int AWG = 64 * AWAVES;

// One slot = one (sample, head): SB lanes (32: two slots per wave, 64: one). LDS per slot: two [SB][HDB] tiles
// (zero-padded columns hd .. HDB - 1, so the dot products run over whole float4) and two [SB] row vectors.
template <int SB, int HDB>
struct AttnLds {
  float a[SB * HDB];
  float b[SB * HDB];
  float r0[SB];
  float r1[SB];
};

// tile[j][c] = src[(row0 + j) * ld + col0 + c] for j < S, c < hd; 0 for hd <= c < HDB. Rows j >= S are never read.
template <int SB, int HDB>
__device__ __forceinline__ void stage_tile(float* __restrict__ tile, const float* __restrict__ src, long long row0,
                                           long long ld, int col0, int S, int hd, int lane) {
  for (int e = lane; e < S * HDB; e += SB) {
    const int j = e / HDB, c = e - j * HDB;
    tile[e] = c < hd ? src[(row0 + j) * ld + col0 + c] : 0.f;
  }
}

template <int HDB>
__device__ __forceinline__ void load_row(float (&dst)[HDB], const float* __restrict__ src, int hd, float scale) {
#pragma unroll
  for (int c = 0; c < HDB; ++c) dst[c] = c < hd ? src[c] * scale : 0.f;
}

template <int HDB>
__device__ __forceinline__ float dot_lds(const float (&x)[HDB], const float* __restrict__ row) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < HDB; c += 4) {
    const floatx4 t = *reinterpret_cast<const floatx4*>(row + c);
    s = fmaf(x[c], t[0], s);
    s = fmaf(x[c + 1], t[1], s);
    s = fmaf(x[c + 2], t[2], s);
    s = fmaf(x[c + 3], t[3], s);
  }
  return s;
}

template <int HDB>
__device__ __forceinline__ void axpy_lds(float (&acc)[HDB], float a, const float* __restrict__ row) {
#pragma unroll
  for (int c = 0; c < HDB; c += 4) {
    const floatx4 t = *reinterpret_cast<const floatx4*>(row + c);
    acc[c] = fmaf(a, t[0], acc[c]);
    acc[c + 1] = fmaf(a, t[1], acc[c + 1]);
    acc[c + 2] = fmaf(a, t[2], acc[c + 2]);
    acc[c + 3] = fmaf(a, t[3], acc[c + 3]);
  }
}

// Forward. grid = ceil(B * heads / slots per workgroup).
template <int SB, int HDB>
__global__ void __launch_bounds__(AWG) k_attn_fwd(const float* __restrict__ q, const float* __restrict__ k,
                                                  const float* __restrict__ v, long long items, int S, int heads,
                                                  int hd, long long ld, float scale, float* __restrict__ out,
                                                  float* __restrict__ lse) {
  constexpr int SPW = 64 / SB, SLOTS = AWAVES * SPW;
  __shared__ __attribute__((aligned(16))) AttnLds<SB, HDB> lds[SLOTS];
  const int slot = threadIdx.x / SB, lane = threadIdx.x % SB;
  const long long item = (long long)blockIdx.x * SLOTS + slot;
  const bool live = item < items;
  const long long b = live ? item / heads : 0;
  const int h = live ? (int)(item - b * heads) : 0;
  const long long row0 = b * S;
  const int col0 = h * hd;
  AttnLds<SB, HDB>& L = lds[slot];
  if (live) {
    stage_tile<SB, HDB>(L.a, k, row0, ld, col0, S, hd, lane);
    stage_tile<SB, HDB>(L.b, v, row0, ld, col0, S, hd, lane);
  }
  __syncthreads();
  if (!live || lane >= S) return;
  float qi[HDB];
  load_row<HDB>(qi, q + (row0 + lane) * ld + col0, hd, scale);
  float s[SB];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < SB; ++j) {
    if (j < S) {
      s[j] = dot_lds<HDB>(qi, L.a + j * HDB);
      m = fmaxf(m, s[j]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < SB; ++j) {
    if (j < S) {
      s[j] = expf(s[j] - m);
      sum += s[j];
    }
  }
  float o[HDB];
#pragma unroll
  for (int c = 0; c < HDB; ++c) o[c] = 0.f;
#pragma unroll
  for (int j = 0; j < SB; ++j) {
    if (j < S) axpy_lds<HDB>(o, s[j], L.b + j * HDB);
  }
  const float inv = 1.f / sum;
  float* orow = out + (row0 + lane) * ld + col0;
#pragma unroll
  for (int c = 0; c < HDB; ++c)
    if (c < hd) orow[c] = o[c] * inv;
  lse[item * S + lane] = m + logf(sum);
}

// Backward: p_ij = exp(s_ij - lse_i), delta_i = dO_i . O_i, ds_ij = p_ij (dO_i . v_j - delta_i);
//   pass 1 (lane i = query row, K / V broadcast):   dq_i = scale sum_j ds_ij k_j
//   pass 2 (lane j = key row, Q / dO broadcast):    dv_j = sum_i p_ij dO_i,  dk_j = scale sum_i ds_ij q_i
// Both passes sum in index order. The two tiles are restaged between the passes; lse and delta go through LDS.
template <int SB, int HDB>
__global__ void __launch_bounds__(AWG) k_attn_bwd(const float* __restrict__ q, const float* __restrict__ k,
                                                  const float* __restrict__ v, const float* __restrict__ out,
                                                  const float* __restrict__ lse, const float* __restrict__ dout,
                                                  long long items, int S, int heads, int hd, long long ld, float scale,
                                                  float* __restrict__ dq, float* __restrict__ dk,
                                                  float* __restrict__ dv) {
  constexpr int SPW = 64 / SB, SLOTS = AWAVES * SPW;
  __shared__ __attribute__((aligned(16))) AttnLds<SB, HDB> lds[SLOTS];
  const int slot = threadIdx.x / SB, lane = threadIdx.x % SB;
  const long long item = (long long)blockIdx.x * SLOTS + slot;
  const bool live = item < items;
  const long long b = live ? item / heads : 0;
  const int h = live ? (int)(item - b * heads) : 0;
  const long long row0 = b * S;
  const int col0 = h * hd;
  const bool mine = live && lane < S;
  const long long off = (row0 + lane) * ld + col0;
  AttnLds<SB, HDB>& L = lds[slot];
  if (live) {
    stage_tile<SB, HDB>(L.a, k, row0, ld, col0, S, hd, lane);
    stage_tile<SB, HDB>(L.b, v, row0, ld, col0, S, hd, lane);
  }
  __syncthreads();
  if (mine) {
    float qi[HDB], doi[HDB], acc[HDB];
    load_row<HDB>(qi, q + off, hd, scale);
    load_row<HDB>(doi, dout + off, hd, 1.f);
    float delta = 0.f;
#pragma unroll
    for (int c = 0; c < HDB; ++c) {
      if (c < hd) delta = fmaf(doi[c], out[off + c], delta);
      acc[c] = 0.f;
    }
    const float li = lse[item * S + lane];
    for (int j = 0; j < S; ++j) {
      const float p = expf(dot_lds<HDB>(qi, L.a + j * HDB) - li);
      const float ds = p * (dot_lds<HDB>(doi, L.b + j * HDB) - delta);
      axpy_lds<HDB>(acc, ds, L.a + j * HDB);
    }
#pragma unroll
    for (int c = 0; c < HDB; ++c)
      if (c < hd) dq[off + c] = acc[c] * scale;
    L.r0[lane] = li;
    L.r1[lane] = delta;
  }
  __syncthreads();                       // every lane is done with the K / V tiles
  if (live) {
    stage_tile<SB, HDB>(L.a, q, row0, ld, col0, S, hd, lane);
    stage_tile<SB, HDB>(L.b, dout, row0, ld, col0, S, hd, lane);
  }
  __syncthreads();
  if (mine) {
    float kj[HDB], vj[HDB], gk[HDB], gv[HDB];
    load_row<HDB>(kj, k + off, hd, scale);
    load_row<HDB>(vj, v + off, hd, 1.f);
#pragma unroll
    for (int c = 0; c < HDB; ++c) gk[c] = gv[c] = 0.f;
    for (int i = 0; i < S; ++i) {
      const float p = expf(dot_lds<HDB>(kj, L.a + i * HDB) - L.r0[i]);
      const float ds = p * (dot_lds<HDB>(vj, L.b + i * HDB) - L.r1[i]);
      axpy_lds<HDB>(gv, p, L.b + i * HDB);
      axpy_lds<HDB>(gk, ds, L.a + i * HDB);
    }
#pragma unroll
    for (int c = 0; c < HDB; ++c) {
      if (c < hd) {
        dk[off + c] = gk[c] * scale;
        dv[off + c] = gv[c];
      }
    }
  }
}

// ---- residual + LayerNorm -------------------------------------------------------------------------------------------
constexpr int LN_MAX_D = 1024;
constexpr int LN_MAX_WG = 1024;        // workgroups (= gamma / beta partials) of the backward
constexpr int LN_MIN_RPW = 8;          // ... each owning at least two rows per wave

// Sum over the wave in a fixed butterfly order; every lane gets the total.
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// z = x + r of one row into the lane's registers (element lane + 64 t, T = ceil(d / 64) rounded up to a power of
// two); returns the row's mean and 1 / std.
template <int T>
__device__ __forceinline__ void ln_row_stats(const float* __restrict__ x, const float* __restrict__ r, int d, int lane,
                                             float eps, float (&z)[T], float* mean, float* rstd) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int e = lane + 64 * t;
    z[t] = e < d ? x[e] + r[e] : 0.f;
    s += z[t];
  }
  const float mu = wave_sum(s) / (float)d;
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float c = lane + 64 * t < d ? z[t] - mu : 0.f;
    ss = fmaf(c, c, ss);
  }
  *mean = mu;
  *rstd = 1.f / sqrtf(wave_sum(ss) / (float)d + eps);
}

template <int T>
__global__ void __launch_bounds__(AWG) k_add_ln_fwd(const float* __restrict__ x, const float* __restrict__ r,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    long long rows, int d, float eps, float* __restrict__ y,
                                                    float* __restrict__ mean, float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * AWAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  float z[T], mu, rs;
  ln_row_stats<T>(x + row * d, r + row * d, d, lane, eps, z, &mu, &rs);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int e = lane + 64 * t;
    if (e < d) y[row * d + e] = fmaf((z[t] - mu) * rs, gamma[e], beta ? beta[e] : 0.f);
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// Backward of y = LN(x + r): g = dy gamma, xh = (x + r - mean) rstd,
//   dx = dr = rstd (g - mean_e(g) - xh mean_e(g xh));   dgamma = sum_rows dy xh;   dbeta = sum_rows dy.
// Workgroup w owns rows [w rpw, (w + 1) rpw), its four waves take them round-robin; the waves' column sums are added in
// wave order into part[w] = [dgamma (d) | dbeta (d)], which k_add_ln_reduce sums over w in a fixed order.
template <int T>
__global__ void __launch_bounds__(AWG) k_add_ln_bwd(const float* __restrict__ x, const float* __restrict__ r,
                                                    const float* __restrict__ gamma, const float* __restrict__ mean,
                                                    const float* __restrict__ rstd, const float* __restrict__ dy,
                                                    long long rows, int d, long long rpw, float* __restrict__ dx,
                                                    float* __restrict__ part) {
  __shared__ float red[AWAVES][2][64 * T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long lo = (long long)blockIdx.x * rpw, hi = lo + rpw < rows ? lo + rpw : rows;
  float gam[T], gg[T], gb[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    gam[t] = lane + 64 * t < d ? gamma[lane + 64 * t] : 0.f;
    gg[t] = gb[t] = 0.f;
  }
  for (long long row = lo + wave; row < hi; row += AWAVES) {
    const float mu = mean[row], rs = rstd[row];
    float dyv[T], xh[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int e = lane + 64 * t;
      const bool in = e < d;
      dyv[t] = in ? dy[row * d + e] : 0.f;
      xh[t] = in ? (x[row * d + e] + r[row * d + e] - mu) * rs : 0.f;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float g = dyv[t] * gam[t];
      gg[t] = fmaf(dyv[t], xh[t], gg[t]);
      gb[t] += dyv[t];
      s1 += g;
      s2 = fmaf(g, xh[t], s2);
    }
    const float m1 = wave_sum(s1) / (float)d, m2 = wave_sum(s2) / (float)d;
    if (dx) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int e = lane + 64 * t;
        if (e < d) dx[row * d + e] = rs * (dyv[t] * gam[t] - m1 - xh[t] * m2);
      }
    }
  }
  if (!part) return;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    red[wave][0][lane + 64 * t] = gg[t];
    red[wave][1][lane + 64 * t] = gb[t];
  }
  __syncthreads();
  float* dst = part + (long long)blockIdx.x * 2 * d;
  for (int e = threadIdx.x; e < 2 * d; e += AWG) {
    const int which = e >= d ? 1 : 0, col = e - which * d;
    float s = red[0][which][col];
#pragma unroll
    for (int w = 1; w < AWAVES; ++w) s += red[w][which][col];
    dst[e] = s;
  }
}

// dgamma | dbeta [e] = sum over the nwg partials: a workgroup takes LN_RC columns; lane group q of its LN_RG sums
// partials q, q + LN_RG, ... in index order, then the group sums are added in group order.
constexpr int LN_RC = 16, LN_RG = AWG / LN_RC;
__global__ void __launch_bounds__(AWG) k_add_ln_reduce(const float* __restrict__ part, int nwg, int d,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float red[LN_RG][LN_RC];
  const int c = threadIdx.x % LN_RC, q = threadIdx.x / LN_RC;
  const int e = blockIdx.x * LN_RC + c;
  float s = 0.f;
  if (e < 2 * d) {
#pragma unroll 4
    for (int w = q; w < nwg; w += LN_RG) s += part[(long long)w * 2 * d + e];
  }
  red[q][c] = s;
  __syncthreads();
  if (q != 0 || e >= 2 * d) return;
  s = red[0][c];
#pragma unroll
  for (int w = 1; w < LN_RG; ++w) s += red[w][c];
  if (e < d) {
    if (dgamma) dgamma[e] = s;
  } else if (dbeta) {
    dbeta[e - d] = s;
  }
}

struct LnPlan {
  long long rpw;
  int nwg;
};

inline bool ln_plan(long long rows, int d, LnPlan* P) {
  if (rows < 1 || d < 1 || d > LN_MAX_D || rows > 0x7fffffffLL) return false;
  long long nwg = (rows + LN_MIN_RPW - 1) / LN_MIN_RPW;
  if (nwg > LN_MAX_WG) nwg = LN_MAX_WG;
  P->rpw = (rows + nwg - 1) / nwg;
  P->nwg = (int)((rows + P->rpw - 1) / P->rpw);
  return true;
}

inline bool attn_args(long long B, int S, int heads, int hd, long long ld) {
  return B >= 1 && S >= 1 && S <= 64 && heads >= 1 && hd >= 1 && hd <= 64 && ld >= (long long)heads * hd &&
         B * heads <= 0x7fffffffLL;
}

template <int SB, int HDB>
int attn_fwd_launch(const float* q, const float* k, const float* v, long long B, int S, int heads, int hd, long long ld,
                    float* out, float* lse, hipStream_t st) {
  constexpr int SLOTS = AWAVES * (64 / SB);
  const long long items = B * heads;
  return bcnf_rt::launch<k_attn_fwd<SB, HDB>>(dim3((unsigned)((items + SLOTS - 1) / SLOTS)), dim3(AWG), 0, st, q, k, v,
                                              items, S, heads, hd, ld, 1.f / sqrtf((float)hd), out, lse);
}

template <int SB, int HDB>
int attn_bwd_launch(const float* q, const float* k, const float* v, const float* out, const float* lse,
                    const float* dout, long long B, int S, int heads, int hd, long long ld, float* dq, float* dk,
                    float* dv, hipStream_t st) {
  constexpr int SLOTS = AWAVES * (64 / SB);
  const long long items = B * heads;
  return bcnf_rt::launch<k_attn_bwd<SB, HDB>>(dim3((unsigned)((items + SLOTS - 1) / SLOTS)), dim3(AWG), 0, st, q, k, v,
                                              out, lse, dout, items, S, heads, hd, ld, 1.f / sqrtf((float)hd), dq, dk,
                                              dv);
}

// (S <= 32 | S <= 64) x head_dim bucket (8, 16, 32, 64): the register arrays of a lane have these compile-time sizes
#define ATTN_DISPATCH(FN, ...)                                       \
  do {                                                               \
    if (S <= 32) {                                                   \
      if (hd <= 8) return FN<32, 8>(__VA_ARGS__);                    \
      if (hd <= 16) return FN<32, 16>(__VA_ARGS__);                  \
      if (hd <= 32) return FN<32, 32>(__VA_ARGS__);                  \
      return FN<32, 64>(__VA_ARGS__);                                \
    }                                                                \
    if (hd <= 8) return FN<64, 8>(__VA_ARGS__);                      \
    if (hd <= 16) return FN<64, 16>(__VA_ARGS__);                    \
    if (hd <= 32) return FN<64, 32>(__VA_ARGS__);                    \
    return FN<64, 64>(__VA_ARGS__);                                  \
  } while (0)

// elements per lane of a LayerNorm row: ceil(d / 64) rounded up to a power of two; the value is the launch's status
#define LN_DISPATCH(K, GRID, ST, ...)                                            \
  (d <= 64    ? bcnf_rt::launch<K<1>>(GRID, dim3(AWG), 0, ST, __VA_ARGS__)       \
   : d <= 128 ? bcnf_rt::launch<K<2>>(GRID, dim3(AWG), 0, ST, __VA_ARGS__)       \
   : d <= 256 ? bcnf_rt::launch<K<4>>(GRID, dim3(AWG), 0, ST, __VA_ARGS__)       \
   : d <= 512 ? bcnf_rt::launch<K<8>>(GRID, dim3(AWG), 0, ST, __VA_ARGS__)       \
              : bcnf_rt::launch<K<16>>(GRID, dim3(AWG), 0, ST, __VA_ARGS__))

}  // namespace

extern "C" {

int bcnf_attn_forward(const float* q, const float* k, const float* v, int64_t B, int32_t S, int32_t heads, int32_t hd,
                      int64_t ld, float* out, float* lse, void* stream) {
  if (!q || !k || !v || !out || !lse || !attn_args(B, S, heads, hd, ld)) return BCNF_ERR_ARG;
  ATTN_DISPATCH(attn_fwd_launch, q, k, v, (long long)B, S, heads, hd, (long long)ld, out, lse, (hipStream_t)stream);
}

int bcnf_attn_backward(const float* q, const float* k, const float* v, const float* out, const float* lse,
                       const float* dout, int64_t B, int32_t S, int32_t heads, int32_t hd, int64_t ld, float* dq,
                       float* dk, float* dv, void* stream) {
  if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !attn_args(B, S, heads, hd, ld))
    return BCNF_ERR_ARG;
  ATTN_DISPATCH(attn_bwd_launch, q, k, v, out, lse, dout, (long long)B, S, heads, hd, (long long)ld, dq, dk, dv,
                (hipStream_t)stream);
}

int bcnf_add_layernorm_forward(const float* x, const float* r, const float* gamma, const float* beta, int64_t rows,
                               int32_t d, float eps, float* y, float* mean, float* rstd, void* stream) {
  LnPlan P;
  if (!x || !r || !gamma || !y || !mean || !rstd || !(eps >= 0.f) || !ln_plan(rows, d, &P)) return BCNF_ERR_ARG;
  const dim3 grid((unsigned)((rows + AWAVES - 1) / AWAVES));
  return LN_DISPATCH(k_add_ln_fwd, grid, (hipStream_t)stream, x, r, gamma, beta, (long long)rows, d, eps, y, mean, rstd);
}

int bcnf_add_layernorm_work_bytes(int64_t rows, int32_t d, int64_t* bytes) {
  LnPlan P;
  if (!bytes || !ln_plan(rows, d, &P)) return BCNF_ERR_ARG;
  *bytes = (int64_t)P.nwg * 2 * d * 4;
  return BCNF_OK;
}

int bcnf_add_layernorm_backward(const float* x, const float* r, const float* gamma, const float* mean,
                                const float* rstd, const float* dy, int64_t rows, int32_t d, float* dx, float* dgamma,
                                float* dbeta, void* work, void* stream) {
  LnPlan P;
  if (!x || !r || !gamma || !mean || !rstd || !dy || !ln_plan(rows, d, &P)) return BCNF_ERR_ARG;
  const bool params = dgamma || dbeta;
  if (params && !work) return BCNF_ERR_ARG;
  if (!dx && !params) return BCNF_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rc = LN_DISPATCH(k_add_ln_bwd, dim3((unsigned)P.nwg), st, x, r, gamma, mean, rstd, dy, (long long)rows, d,
                             P.rpw, dx, params ? static_cast<float*>(work) : nullptr);
  if (rc || !params) return rc;
  return bcnf_rt::launch<k_add_ln_reduce>(dim3((unsigned)((2 * d + LN_RC - 1) / LN_RC)), dim3(AWG), 0, st,
                                          static_cast<const float*>(work), P.nwg, d, dgamma, dbeta);
}

}  // extern "C"
