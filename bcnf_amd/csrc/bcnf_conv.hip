// CNN feature network (models/cnn.py): one Conv2d -> ReLU -> Dropout -> MaxPool2d(2, 2) layer per launch and
// direction (include/bcnf_amd.h, "CNN layer"). fp32, NCHW contiguous, stride 1, zero padding; stream-ordered,
// stateless, no atomics, every sum in a fixed order.
//
// Form: a register-tiled direct convolution on the VALU. The layers of the video configs have c_in * c_out between
// 8 and 512 and K between 3 and 8: an implicit GEMM on v_mfma_f32_16x16x4_f32 would run the first layer (c_in = 1,
// c_out = 8) with half of every tile empty and would gather its B operand from LDS one dword per lane and MFMA,
// while the fp32 VALU rate equals the fp32 MFMA rate; the direct form reads K + 1 LDS values per 4 K OCB FMAs and
// takes its weights as scalar operands.
//
//  * k_conv_tile<K, false> (forward): a workgroup owns one image, OCB output channels and a TH x TW tile of POOLED
//    pixels; a thread owns one pooled pixel = a 2 x 2 window of conv outputs for OCB channels (4 OCB accumulators).
//    The zero-padded input tile of `cib` input channels is staged in LDS per round; per input channel a thread reads
//    the K + 1 rows of its (K + 1) x (K + 1) patch as 8-byte pairs. Epilogue: bias, ReLU, the dropout draw, the
//    first-wins maximum; only y and one code byte per pooled pixel are written.
//  * k_conv_tile<K, true> (input gradient): the same tile loop with the roles of the channels swapped, the taps
//    flipped and padding K - 1 - pad, reading g -- the zeroed tile with dy / (1 - p) put at each window's winner, one
//    code byte and one dy load per window -- and writing each thread's 2 x 2 patch of dx.
//  * k_conv_wgrad<K> (weight / bias gradient): workgroup w walks images w, w + nwg, ...; a thread owns the K taps
//    (kx) of one (4 output channels, input channel, ky) task for one slice of the rows and slides a 2 K register
//    window of the input row along x: 4 K FMAs per 5 LDS reads. Every (workgroup, slice) writes one partial of
//    [dweight | dbias] into `work`; k_conv_wreduce sums the partials in index order.
#include "bcnf_device.h"

namespace {

constexpr int CWG = 256;                         // largest workgroup
constexpr int OCB = 8;                           // output channels per thread of the tile kernels
constexpr int WCB = 4;                           // output channels per task of the weight-gradient kernel
constexpr uint32_t BCNF_CONV_KEY = 0x40000000u;  // feature layers: 0x80000000 (bcnf_train.hip)
constexpr int CONV_MAX_K = 8, CONV_MAX_C = 32;
constexpr int TILE_LDS_BYTES = 32 * 1024;        // staged input channels per round fill at most this
constexpr int WGRAD_LDS_BYTES = 64 * 1024;
constexpr int WGRAD_MAX_WG = 512;

struct ConvDims {
  long long N;
  int CI, H, W, CO, K, PH, PW;
  int HC, WC, HP, WP;          // conv output, pooled output
};

struct ConvDrop {
  const uint64_t* rng;         // NULL: no dropout
  uint32_t salt, thresh;
  float scale;                 // 1 / (1 - p)
};

// u32 of element e of the layer's (n_images, c_out, Hc, Wc) conv output: word e & 3 of the Philox4x32-10 draw with
// counter (e >> 2 low, e >> 2 high, offset low, offset high) and key (seed low ^ salt 0x9E3779B9, seed high ^
// BCNF_CONV_KEY). A thread needs e and e + 1 (its window's two columns): one draw unless e & 3 == 3.
__device__ __forceinline__ uint32_t word_of(const uint4& r, uint32_t w) {
  return w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w;
}
__device__ __forceinline__ void conv_u32_pair(unsigned long long e, uint64_t seed, uint64_t off, uint32_t salt,
                                              uint32_t& u0, uint32_t& u1) {
  const uint2 key = make_uint2((uint32_t)seed ^ salt, (uint32_t)(seed >> 32) ^ BCNF_CONV_KEY);
  const unsigned long long q = e >> 2;
  const uint32_t w = (uint32_t)(e & 3ull);
  const uint4 r = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)), key);
  u0 = word_of(r, w);
  if (w < 3) {
    u1 = word_of(r, w + 1);
  } else {
    const unsigned long long q1 = q + 1;
    u1 = philox4x32_10(make_uint4((uint32_t)q1, (uint32_t)(q1 >> 32), (uint32_t)off, (uint32_t)(off >> 32)), key).x;
  }
}

struct TileArgs {
  int tw_log2, TH;             // threads: TH rows of TW = 1 << tw_log2
  int tiles_x, tiles_y, ocblocks;
  int IH, IWP, cib;            // LDS tile rows, padded row length (even), input channels per round
};

// The tile loop of the forward (BWD = false) and of the input gradient (BWD = true).
//   forward: in = x (N, CI, H, W), out = y (N, CO, HP, WP), code_out (nullable)
//   BWD:     in = dy (N, CO, HP, WP) with code_in, out = dx (N, CI, H, W)
template <int K, bool BWD>
__global__ void __launch_bounds__(CWG) k_conv_tile(const float* __restrict__ in, const uint8_t* __restrict__ code_in,
                                                   const float* __restrict__ wgt, const float* __restrict__ bias,
                                                   float* __restrict__ out, uint8_t* __restrict__ code_out,
                                                   ConvDims D, TileArgs T, ConvDrop dr) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int KK = K * K;
  constexpr int NV = (K + 2) & ~1;                 // K + 1 patch columns, read as pairs
  const int TW = 1 << T.tw_log2;
  const int nthreads = T.TH * TW;
  const int tid = threadIdx.x;
  const int tx = tid & (TW - 1), ty = tid >> T.tw_log2;
  const int IC = BWD ? D.CO : D.CI, OC = BWD ? D.CI : D.CO;
  const int pad_y = BWD ? K - 1 - D.PH : D.PH, pad_x = BWD ? K - 1 - D.PW : D.PW;
  const int ocs = BWD ? KK : D.CI * KK, ics = BWD ? D.CI * KK : KK;     // weight strides of the out / in channel

  long long b = blockIdx.x;
  const int ntiles = T.tiles_x * T.tiles_y;
  const int tl = (int)(b % ntiles);
  b /= ntiles;
  const int oc0 = (int)(b % T.ocblocks) * OCB;
  const long long n = b / T.ocblocks;
  const int py0 = (tl / T.tiles_x) * T.TH, px0 = (tl % T.tiles_x) * TW;
  const int iy0 = 2 * py0 - pad_y, ix0 = 2 * px0 - pad_x;

  float acc[OCB][2][2];
#pragma unroll
  for (int c = 0; c < OCB; ++c) acc[c][0][0] = acc[c][0][1] = acc[c][1][0] = acc[c][1][1] = 0.f;

  const int plane = T.IH * T.IWP;
  for (int ic0 = 0; ic0 < IC; ic0 += T.cib) {
    const int nc = IC - ic0 < T.cib ? IC - ic0 : T.cib;
    __syncthreads();                                // the previous round's reads are done
    if (!BWD) {
      for (int e = tid; e < nc * plane; e += nthreads) {
        const int c = e / plane, rem = e - c * plane;
        const int r = rem / T.IWP, col = rem - r * T.IWP;
        const int iy = iy0 + r, ix = ix0 + col;
        float v = 0.f;
        if (iy >= 0 && iy < D.H && ix >= 0 && ix < D.W) v = in[((n * D.CI + (ic0 + c)) * D.H + iy) * D.W + ix];
        tile[e] = v;
      }
    } else {
      // g is one value per window: zero the tile, then every pooled element whose window touches the tile puts
      // dy / (1 - p) at its winner (one owner per tile element: no write conflicts)
      for (int e = tid; e < nc * plane; e += nthreads) tile[e] = 0.f;
      __syncthreads();
      const int pr0 = iy0 >> 1, pc0 = ix0 >> 1;                   // floor: iy0, ix0 may be negative
      const int PR = (T.IH >> 1) + 1, PC = (T.IWP >> 1) + 1;
      for (int e = tid; e < nc * PR * PC; e += nthreads) {
        const int c = e / (PR * PC), rem = e - c * (PR * PC);
        const int r = rem / PC;
        const int wy = pr0 + r, wx = pc0 + (rem - r * PC);
        if (wy < 0 || wy >= D.HP || wx < 0 || wx >= D.WP) continue;
        const long long ci = ((n * D.CO + (ic0 + c)) * D.HP + wy) * D.WP + wx;
        const uint32_t cd = code_in[ci];
        if (!(cd & 4u)) continue;
        const int ry = 2 * wy + (int)((cd >> 1) & 1u) - iy0, rx = 2 * wx + (int)(cd & 1u) - ix0;
        if (ry >= 0 && ry < T.IH && rx >= 0 && rx < T.IWP) tile[c * plane + ry * T.IWP + rx] = in[ci] * dr.scale;
      }
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      const float* tp = tile + c * plane + (2 * ty) * T.IWP + 2 * tx;
      const float* wp = wgt + (long long)(ic0 + c) * ics;
#pragma unroll
      for (int r = 0; r <= K; ++r) {
        float v[NV];
        const float2* row = reinterpret_cast<const float2*>(tp + r * T.IWP);
#pragma unroll
        for (int m = 0; m < NV / 2; ++m) {
          const float2 t2 = row[m];
          v[2 * m] = t2.x;
          v[2 * m + 1] = t2.y;
        }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
          const int ky = r - dy;
          if (ky < 0 || ky >= K) continue;
#pragma unroll
          for (int oc = 0; oc < OCB; ++oc) {
            const int occ = oc0 + oc < OC ? oc0 + oc : OC - 1;     // clamped: computed, never stored
            const float* wr = wp + (long long)occ * ocs;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
              const float wv = wr[BWD ? KK - 1 - (ky * K + kx) : ky * K + kx];
              acc[oc][dy][0] = fmaf(v[kx], wv, acc[oc][dy][0]);
              acc[oc][dy][1] = fmaf(v[kx + 1], wv, acc[oc][dy][1]);
            }
          }
        }
      }
    }
  }

  const int py = py0 + ty, px = px0 + tx;
  if (BWD) {
#pragma unroll
    for (int oc = 0; oc < OCB; ++oc) {
      if (oc0 + oc >= OC) continue;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int oy = 2 * py + dy, ox = 2 * px + dx;
          if (oy < D.H && ox < D.W) out[((n * D.CI + (oc0 + oc)) * D.H + oy) * D.W + ox] = acc[oc][dy][dx];
        }
    }
    return;
  }
  if (py >= D.HP || px >= D.WP) return;
  uint64_t seed = 0, off = 0;
  if (dr.rng) {
    seed = dr.rng[0];
    off = dr.rng[1];
  }
#pragma unroll
  for (int oc = 0; oc < OCB; ++oc) {
    const int o = oc0 + oc;
    if (o >= D.CO) continue;
    const float bb = bias ? bias[o] : 0.f;
    float a[4];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      float m0 = 1.f, m1 = 1.f;
      if (dr.rng) {
        const unsigned long long e =
            (unsigned long long)(((n * D.CO + o) * D.HC + (2 * py + dy)) * D.WC + 2 * px);
        uint32_t u0, u1;
        conv_u32_pair(e, seed, off, dr.salt, u0, u1);
        m0 = u0 >= dr.thresh ? dr.scale : 0.f;
        m1 = u1 >= dr.thresh ? dr.scale : 0.f;
      }
      a[2 * dy] = fmaxf(acc[oc][dy][0] + bb, 0.f) * m0;
      a[2 * dy + 1] = fmaxf(acc[oc][dy][1] + bb, 0.f) * m1;
    }
    float best = a[0];
    uint32_t win = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (a[i] > best) {           // strictly greater: the first of equal values wins
        best = a[i];
        win = i;
      }
    const long long yi = ((n * D.CO + o) * D.HP + py) * D.WP + px;
    out[yi] = best;
    if (code_out) code_out[yi] = (uint8_t)(win | (best > 0.f ? 4u : 0u));
  }
}

struct WgradArgs {
  int nwg, YS, tpp, ntasks, passes;     // workgroups, row slices, tasks per pass, tasks, passes
  int COP;                              // c_out rounded up to WCB
  int BR, GWC, GW;                      // band rows, chunk columns (multiple of K), padded conv width
  long long P;                          // floats per partial: COP * CI * K * K + COP
  float scale;
};

// Partials of dweight / dbias: part[(w * YS + s) * P + ...] for workgroup w, row slice s.
template <int K>
__global__ void __launch_bounds__(CWG) k_conv_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                    const uint8_t* __restrict__ code, ConvDims D, WgradArgs A,
                                                    float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int XW = A.GWC + K, XR = A.BR + K - 1;
  float* gt = lds;                                    // [COP][BR][GWC]
  float* xt = lds + A.COP * A.BR * A.GWC;             // [CI][XR][XW]
  const int ng = A.COP * A.BR * A.GWC, nx = D.CI * XR * XW;
  const int slice = tid / A.tpp, tlocal = tid - slice * A.tpp;
  const bool lane_on = slice < A.YS;
  for (int pass = 0; pass < A.passes; ++pass) {
    const int task = pass * A.tpp + tlocal;
    const bool on = lane_on && task < A.ntasks;
    const int ky = task % K, ci = (task / K) % D.CI, cb = task / (K * D.CI);
    float acc[WCB][K], gs[WCB];
#pragma unroll
    for (int c = 0; c < WCB; ++c) {
      gs[c] = 0.f;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) acc[c][kx] = 0.f;
    }
    for (long long n = blockIdx.x; n < D.N; n += A.nwg) {
      for (int y0 = 0; y0 < 2 * D.HP; y0 += A.BR) {
        for (int x0 = 0; x0 < A.GW; x0 += A.GWC) {
          __syncthreads();
          for (int e = tid; e < ng; e += CWG) gt[e] = 0.f;
          for (int e = tid; e < nx; e += CWG) {
            const int c = e / (XR * XW), rem = e - c * (XR * XW);
            const int r = rem / XW, col = rem - r * XW;
            const int iy = y0 + r - D.PH, ix = x0 + col - D.PW;
            float v = 0.f;
            if (iy >= 0 && iy < D.H && ix >= 0 && ix < D.W) v = x[((n * D.CI + c) * D.H + iy) * D.W + ix];
            xt[e] = v;
          }
          __syncthreads();
          {
            // g is one value per window: every pooled element whose window touches the band puts dy / (1 - p) at
            // its winner in the zeroed band (one owner per band element)
            const int pr0 = y0 >> 1, pc0 = x0 >> 1;
            const int PR = (A.BR >> 1) + 1, PC = (A.GWC >> 1) + 1;
            for (int e = tid; e < D.CO * PR * PC; e += CWG) {
              const int co = e / (PR * PC), rem = e - co * (PR * PC);
              const int r = rem / PC;
              const int wy = pr0 + r, wx = pc0 + (rem - r * PC);
              if (wy >= D.HP || wx >= D.WP) continue;
              const long long pi = ((n * D.CO + co) * D.HP + wy) * D.WP + wx;
              const uint32_t cd = code[pi];
              if (!(cd & 4u)) continue;
              const int ry = 2 * wy + (int)((cd >> 1) & 1u) - y0, rx = 2 * wx + (int)(cd & 1u) - x0;
              if (ry >= 0 && ry < A.BR && rx >= 0 && rx < A.GWC) gt[(co * A.BR + ry) * A.GWC + rx] = dy[pi] * A.scale;
            }
          }
          __syncthreads();
          if (!on) continue;
          for (int r = slice; r < A.BR; r += A.YS) {
            const float* xrow = xt + (ci * XR + r + ky) * XW;
            const float* grow = gt + (cb * WCB * A.BR + r) * A.GWC;
            float xs[2 * K];
#pragma unroll
            for (int kx = 0; kx < K; ++kx) xs[kx] = xrow[kx];
            for (int xx = 0; xx < A.GWC; xx += K) {
#pragma unroll
              for (int j = 0; j < K; ++j) xs[K + j] = xrow[xx + K + j];
#pragma unroll
              for (int j = 0; j < K; ++j) {
#pragma unroll
                for (int c = 0; c < WCB; ++c) {
                  const float gv = grow[c * A.BR * A.GWC + xx + j];
                  gs[c] += gv;
#pragma unroll
                  for (int kx = 0; kx < K; ++kx) acc[c][kx] = fmaf(gv, xs[j + kx], acc[c][kx]);
                }
              }
#pragma unroll
              for (int kx = 0; kx < K; ++kx) xs[kx] = xs[K + kx];
            }
          }
        }
      }
    }
    if (on) {
      float* dst = part + ((long long)blockIdx.x * A.YS + slice) * A.P;
#pragma unroll
      for (int c = 0; c < WCB; ++c) {
        const int co = cb * WCB + c;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) dst[((long long)(co * D.CI + ci) * K + ky) * K + kx] = acc[c][kx];
        if (ci == 0 && ky == 0) dst[(long long)A.COP * D.CI * K * K + co] = gs[c];
      }
    }
  }
}

// dweight | dbias [e] = sum over the np partials: a workgroup takes WR_C outputs; lane group q of its WR_G sums
// partials q, q + WR_G, ... in index order, then the group sums are added in group order (k_add_ln_reduce's scheme).
constexpr int WR_C = 16, WR_G = CWG / WR_C;
__global__ void __launch_bounds__(CWG) k_conv_wreduce(const float* __restrict__ part, long long np, long long P,
                                                      int nweight, int nbias, long long bias_off,
                                                      float* __restrict__ dweight, float* __restrict__ dbias) {
  __shared__ float red[WR_G][WR_C];
  const int c = threadIdx.x % WR_C, q = threadIdx.x / WR_C;
  const int e = blockIdx.x * WR_C + c;
  const bool in = e < nweight + nbias;
  const long long src = e < nweight ? e : bias_off + (e - nweight);
  float s = 0.f;
  if (in) {
#pragma unroll 4
    for (long long w = q; w < np; w += WR_G) s += part[w * P + src];
  }
  red[q][c] = s;
  __syncthreads();
  if (q != 0 || !in) return;
  s = red[0][c];
#pragma unroll
  for (int w = 1; w < WR_G; ++w) s += red[w][c];
  if (e < nweight) {
    if (dweight) dweight[e] = s;
  } else if (dbias) {
    dbias[e - nweight] = s;
  }
}

bool conv_dims(long long N, int CI, int H, int W, int CO, int K, int PH, int PW, float p, ConvDims* D) {
  if (N < 1 || K < 1 || K > CONV_MAX_K || CI < 1 || CI > CONV_MAX_C || CO < 1 || CO > CONV_MAX_C) return false;
  if (PH < 0 || PH > K - 1 || PW < 0 || PW > K - 1 || H < 1 || W < 1 || !(p >= 0.f && p < 1.f)) return false;
  const long long HC = (long long)H + 2 * PH - K + 1, WC = (long long)W + 2 * PW - K + 1;
  if (HC < 2 || WC < 2 || HC > 0x3fffffffLL || WC > 0x3fffffffLL) return false;
  // every flat index below 2^62: the kernels' 64-bit arithmetic never wraps
  const double big = (double)N * 32.0 * (double)(HC + 2 * K) * (double)(WC + 2 * K);
  if (big > 4.0e18) return false;
  *D = ConvDims{N, CI, H, W, CO, K, PH, PW, (int)HC, (int)WC, (int)(HC / 2), (int)(WC / 2)};
  return true;
}

// Tile of np_y x np_x thread patches: the (TH, TW) with the smallest padded area, the larger workgroup on a tie.
bool tile_plan(const ConvDims& D, int np_y, int np_x, int IC, int OC, TileArgs* T, unsigned* grid, int* threads,
               size_t* lds) {
  long long best = -1;
  int bth = 0, btl = 0;
  for (int tl = 3; tl <= 5; ++tl)
    for (int th = 2; th <= 32; th *= 2) {
      const int tw = 1 << tl, nt = th * tw;
      if (nt < 64 || nt > CWG) continue;
      const long long area = (long long)((np_y + th - 1) / th) * th * ((np_x + tw - 1) / tw) * tw;
      if (best < 0 || area < best || (area == best && nt > bth * (1 << btl))) {
        best = area;
        bth = th;
        btl = tl;
      }
    }
  const int TW = 1 << btl;
  T->tw_log2 = btl;
  T->TH = bth;
  T->tiles_x = (np_x + TW - 1) / TW;
  T->tiles_y = (np_y + bth - 1) / bth;
  T->ocblocks = (OC + OCB - 1) / OCB;
  T->IH = 2 * bth + D.K - 1;
  T->IWP = 2 * TW + D.K - (D.K & 1);
  const int plane_bytes = T->IH * T->IWP * 4;
  int cib = TILE_LDS_BYTES / plane_bytes;
  T->cib = cib < 1 ? 1 : cib > IC ? IC : cib;
  const long long blocks = D.N * T->ocblocks * T->tiles_x * T->tiles_y;
  if (blocks > 0x7fffffffLL) return false;
  *grid = (unsigned)blocks;
  *threads = bth * TW;
  *lds = (size_t)T->cib * plane_bytes;
  return true;
}

void wgrad_plan(const ConvDims& D, WgradArgs* A, size_t* lds) {
  const int K = D.K;
  A->COP = (D.CO + WCB - 1) / WCB * WCB;
  A->GW = (2 * D.WP + K - 1) / K * K;
  A->GWC = A->GW;
  A->ntasks = (A->COP / WCB) * D.CI * K;
  A->tpp = A->ntasks < CWG ? A->ntasks : CWG;
  const int ys_want = CWG / A->tpp;                 // row slices that fill the workgroup: keep that many band rows
  int br = 2 * D.HP < 16 ? 2 * D.HP : 16;
  auto bytes = [&](int b, int g) { return ((long long)A->COP * b * g + (long long)D.CI * (b + K - 1) * (g + K)) * 4; };
  while (bytes(br, A->GWC) > WGRAD_LDS_BYTES) {
    if (br > (ys_want > 4 ? ys_want : 4))
      br = (br + 1) / 2;
    else if (A->GWC > 4 * K)
      A->GWC = ((A->GWC / K + 1) / 2) * K;
    else if (br > 4)
      br = (br + 1) / 2;
    else if (A->GWC > K)
      A->GWC = ((A->GWC / K + 1) / 2) * K;
    else if (br > 1)
      br = (br + 1) / 2;
    else
      break;                         // 1 row x K columns: 32 * K + 32 * K * 2 K floats at most, always fits
  }
  A->BR = br;
  A->YS = ys_want > br ? br : ys_want;
  A->passes = (A->ntasks + A->tpp - 1) / A->tpp;
  A->nwg = D.N < WGRAD_MAX_WG ? (int)D.N : WGRAD_MAX_WG;
  A->P = (long long)A->COP * D.CI * K * K + A->COP;
  *lds = (size_t)bytes(br, A->GWC);
}

#define CONV_K_DISPATCH(CALL)   \
  switch (D.K) {                \
    case 1: return CALL(1);     \
    case 2: return CALL(2);     \
    case 3: return CALL(3);     \
    case 4: return CALL(4);     \
    case 5: return CALL(5);     \
    case 6: return CALL(6);     \
    case 7: return CALL(7);     \
    default: return CALL(8);    \
  }

int tile_launch(bool bwd, const ConvDims& D, const TileArgs& T, unsigned grid, int threads, size_t lds,
                hipStream_t st, const float* in, const uint8_t* code_in, const float* w, const float* bias, float* out,
                uint8_t* code_out, const ConvDrop& dr) {
  const bcnf_rt::Lds L(lds, (size_t)TILE_LDS_BYTES + 8192);
#define CONV_TILE_CALL(KV)                                                                                          \
  (bwd ? bcnf_rt::launch<k_conv_tile<KV, true>>(dim3(grid), dim3(threads), L, st, in, code_in, w, bias, out,        \
                                                code_out, D, T, dr)                                                 \
       : bcnf_rt::launch<k_conv_tile<KV, false>>(dim3(grid), dim3(threads), L, st, in, code_in, w, bias, out,       \
                                                 code_out, D, T, dr))
  CONV_K_DISPATCH(CONV_TILE_CALL)
#undef CONV_TILE_CALL
}

int wgrad_launch(const ConvDims& D, const WgradArgs& A, size_t lds, hipStream_t st, const float* x, const float* dy,
                 const uint8_t* code, float* part) {
  const bcnf_rt::Lds L(lds, (size_t)WGRAD_LDS_BYTES);
#define CONV_WGRAD_CALL(KV) bcnf_rt::launch<k_conv_wgrad<KV>>(dim3(A.nwg), dim3(CWG), L, st, x, dy, code, D, A, part)
  CONV_K_DISPATCH(CONV_WGRAD_CALL)
#undef CONV_WGRAD_CALL
}

}  // namespace

extern "C" {

int bcnf_conv_block_forward(const float* x, const float* weight, const float* bias, int64_t n_images, int32_t c_in,
                            int32_t height, int32_t width, int32_t c_out, int32_t ksize, int32_t pad_h, int32_t pad_w,
                            float p, const uint64_t* rng_state, int32_t salt, float* y, uint8_t* code, void* stream) {
  ConvDims D;
  if (!x || !weight || !y || !conv_dims(n_images, c_in, height, width, c_out, ksize, pad_h, pad_w, p, &D))
    return BCNF_ERR_ARG;
  TileArgs T;
  unsigned grid;
  int threads;
  size_t lds;
  if (!tile_plan(D, D.HP, D.WP, D.CI, D.CO, &T, &grid, &threads, &lds)) return BCNF_ERR_ARG;
  ConvDrop dr{nullptr, (uint32_t)salt * 0x9E3779B9u, 0u, 1.f};
  if (p > 0.f && rng_state) {
    dr.rng = rng_state;
    dr.thresh = (uint32_t)fmin(4294967295.0, floor((double)p * 4294967296.0 + 0.5));   // keep iff u >= thresh
    dr.scale = 1.f / (1.f - p);
  }
  return tile_launch(false, D, T, grid, threads, lds, (hipStream_t)stream, x, nullptr, weight, bias, y, code, dr);
}

int bcnf_conv_block_work_bytes(int64_t n_images, int32_t c_in, int32_t height, int32_t width, int32_t c_out,
                               int32_t ksize, int32_t pad_h, int32_t pad_w, float p, int64_t* bytes) {
  ConvDims D;
  if (!bytes || !conv_dims(n_images, c_in, height, width, c_out, ksize, pad_h, pad_w, p, &D)) return BCNF_ERR_ARG;
  WgradArgs A;
  size_t lds;
  wgrad_plan(D, &A, &lds);
  *bytes = (int64_t)A.nwg * A.YS * A.P * 4;
  return BCNF_OK;
}

int bcnf_conv_block_backward(const float* x, const float* weight, const float* dy, const uint8_t* code,
                             int64_t n_images, int32_t c_in, int32_t height, int32_t width, int32_t c_out,
                             int32_t ksize, int32_t pad_h, int32_t pad_w, float p, float* dx, float* dweight,
                             float* dbias, void* work, void* stream) {
  ConvDims D;
  if (!x || !weight || !dy || !code || !conv_dims(n_images, c_in, height, width, c_out, ksize, pad_h, pad_w, p, &D))
    return BCNF_ERR_ARG;
  const bool params = dweight || dbias;
  if (params && !work) return BCNF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const float scale = 1.f / (1.f - p);
  if (dx) {
    TileArgs T;
    unsigned grid;
    int threads;
    size_t lds;
    if (!tile_plan(D, (D.H + 1) / 2, (D.W + 1) / 2, D.CO, D.CI, &T, &grid, &threads, &lds)) return BCNF_ERR_ARG;
    const ConvDrop dr{nullptr, 0u, 0u, scale};
    const int rc = tile_launch(true, D, T, grid, threads, lds, st, dy, code, weight, nullptr, dx, nullptr, dr);
    if (rc) return rc;
  }
  if (!params) return BCNF_OK;
  WgradArgs A;
  size_t lds;
  wgrad_plan(D, &A, &lds);
  A.scale = scale;
  float* part = static_cast<float*>(work);
  const int rc = wgrad_launch(D, A, lds, st, x, dy, code, part);
  if (rc) return rc;
  const int nweight = D.CO * D.CI * D.K * D.K;
  return bcnf_rt::launch<k_conv_wreduce>(dim3((unsigned)((nweight + D.CO + WR_C - 1) / WR_C)), dim3(CWG), 0, st,
                                         (const float*)part, (long long)A.nwg * A.YS, A.P, nweight, D.CO,
                                         (long long)A.COP * D.CI * D.K * D.K, dweight, dbias);
}

}  // extern "C"
