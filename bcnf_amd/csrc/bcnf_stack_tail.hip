// bcnf_amd small stack family: the backward's tails, which turn k_backward's D1 rows and gradient slabs into
// canonical gradients -- unfolded (k_bwd_tail + k_dw1h_reduce, k_dh) and folded onto the feature Linear
// (k_fold_tail, k_fold_gx, k_fold_finish, with the fused Adam). The family's files: bcnf_stack_internal.h.
#include "bcnf_stack_internal.h"
#include "bcnf_stack_rec.h"

namespace {
using namespace bcnf_small;
using bcnf_rt::launch;

// ------------------------------------------------------------------------------------------------
// Condition projection, hoisted out of the stack kernels (one fp32 MFMA GEMM per direction):
//   HP[k][r][j] = sum_c h[r][c] W1_k[j][Da + c] + b1_k[j]     (the y-independent part of Linear 1)
//   dh[b][c]   = sum_k sum_j D1[k][b][j] W1_k[j][Da + c]      (dL/dh, all blocks)
//   dW1_k[j][Da + c] = sum_b D1[k][b][j] h[b][c]               (split-K, then fixed-order reduce)
// W1h^T comes from the packed buffer ([k][Cp][17], zero-padded); D1 = dL/d pre-activation of Linear 1.
// MFMA lane roles: A[l&15][l>>4], B[l>>4][l&15], D[4(l>>4)+i][l&15].
// ------------------------------------------------------------------------------------------------
// The three projection GEMMs (FC_small: 4096 x 512 x 80, 4096 x 80 x 512, 512 x 80 x 4096). They are
// bound by load issue / round trips rather than MFMA, so: operands come from contiguous packed copies
// (W1hC, W1hR) with float4 loads, a workgroup stages a K-chunk of up to 128 of both operands in LDS per
// round trip (next chunk in flight), and the K loops issue all LDS reads of 4-8 steps before their MFMAs.
// VEC: float4 row loads (vec_rows: the row stride ld and the base are 16-byte aligned).

// load_rows64 in two steps, for a caller that wants every load of a round in flight before the first value is
// used: load_rows64's ones-column select sits behind a branch per float4, which reads the loaded value before the
// next load goes out (one round trip per float4). Same values as load_rows64.
template <bool VEC>
__device__ __forceinline__ void rows64_issue(const float* __restrict__ M, long long nrows, int ncols, long long ld,
                                             long long r0, int c0, floatx4* reg) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int i4 = threadIdx.x + 256 * e, row = i4 >> 5, col = c0 + (i4 & 31) * 4;
    const long long r = r0 + row < nrows ? r0 + row : nrows - 1;
    if (VEC) {
      reg[e] = *reinterpret_cast<const floatx4*>(M + r * ld + (col < ncols ? col : 0));
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) reg[e][q] = M[r * ld + (col + q < ncols ? col + q : ncols - 1)];
    }
  }
}
__device__ __forceinline__ void rows64_mask(long long nrows, int ncols, long long r0, int c0, floatx4* reg, int ones) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int i4 = threadIdx.x + 256 * e, row = i4 >> 5, col = c0 + (i4 & 31) * 4;
    const bool in = r0 + row < nrows;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v = (in && col + q < ncols) ? reg[e][q] : 0.f;
      reg[e][q] = (in && col + q == ones) ? 1.f : v;
    }
  }
}

// dh tile: 64 rows x 16 columns; K = nb * 16 (kj) in chunks of 128 (8 blocks). grid = (ceil(B/64), Cp/16)
__device__ __forceinline__ void dh_body(const BcnfLayout& L, const float* __restrict__ pk, const float* __restrict__ d1,
                                        long long B, float* __restrict__ dh, int bx, int by, float* __restrict__ smem) {
  float* As = smem;                    // [64][KCP] (row b, kj)
  float* Bs = smem + 64 * KCP;         // [KC][16]  (kj, c)
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const long long b0 = (long long)bx * 64;
  const int n = by;
  const int K = L.nb * 16, Cp = L.Cp;
  const float* w1r = pk + L.w1r_off + 16 * n;
  floatx4 ra[8], rb[2];
  const int arow = tid >> 2, aj4 = (tid & 3) * 4;
  const long long ab = b0 + arow < B ? b0 + arow : B - 1;
  auto load = [&](int kj0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {                    // A: block (kj0 / 16 + e), rows [b0, b0 + 64) x 16
      const int k = (kj0 >> 4) + e;
      const floatx4 v = *reinterpret_cast<const floatx4*>(d1 + ((long long)(k < L.nb ? k : L.nb - 1) * B + ab) * 16 + aj4);
      ra[e] = v * (k < L.nb ? 1.f : 0.f);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {                    // B: [128 kj][16 c]: row = i4 / 4, col4
      const int i4 = tid + 256 * e, kj = kj0 + (i4 >> 2);
      const floatx4 v = *reinterpret_cast<const floatx4*>(w1r + (long long)(kj < K ? kj : K - 1) * Cp + (i4 & 3) * 4);
      rb[e] = v * (kj < K ? 1.f : 0.f);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int e = 0; e < 8; ++e) *reinterpret_cast<floatx4*>(As + arow * KCP + 16 * e + aj4) = ra[e];
#pragma unroll
    for (int e = 0; e < 2; ++e) *reinterpret_cast<floatx4*>(Bs + (tid + 256 * e) * 4) = rb[e];
  };
  floatx4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int kj0 = 0; kj0 < K; kj0 += KC) {
    store();
    __syncthreads();
    if (kj0 + KC < K) load(kj0 + KC);
    const int ks = (K - kj0 < KC ? K - kj0 : KC) >> 2;   // multiple of 4
    for (int t0 = 0; t0 < ks; t0 += 4) {
      float a[4], bv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[t] = As[(16 * wave + lr) * KCP + 4 * (t0 + t) + lq];
        bv[t] = Bs[(4 * (t0 + t) + lq) * 16 + lr];
      }
      acc = mfma4(a[0], bv[0], acc);
      acc1 = mfma4(a[1], bv[1], acc1);
      acc = mfma4(a[2], bv[2], acc);
      acc1 = mfma4(a[3], bv[3], acc1);
    }
    __syncthreads();
  }
  acc += acc1;
  const int col = 16 * n + lr;
  if (col < L.C) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long r = b0 + 16 * wave + 4 * lq + i;
      if (r < B) dh[r * L.C + col] = acc[i];
    }
  }
}

__global__ __launch_bounds__(BCNF_WG) void k_dh(BcnfLayout L, const float* __restrict__ pk,
                                                const float* __restrict__ d1, long long B, float* __restrict__ dh) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  dh_body(L, pk, d1, B, dh, blockIdx.x, blockIdx.y, smem);
}

// dW1h split-K partials: 64 kj (4 blocks, one per wave) x all columns over one split of KC rows.
// grid = (ceil(nb/4), splits); work[s][k][16][Cp]
template <bool VEC>
__device__ __forceinline__ void dw1h_body(const BcnfLayout& L, const float* __restrict__ d1, const float* __restrict__ h,
                                          long long B, int rows_per_split, float* __restrict__ work, int bx, int by,
                                          float* __restrict__ smem) {
  const int hs = bstride16(L.Cp);
  float* As = smem;                    // [64][KCP] (kj, b)
  float* Bs = smem + 64 * KCP;         // [KC][hs]  (b, c)
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const int k0 = bx * 4, s = by;
  const long long m0 = (long long)s * rows_per_split;
  long long m1 = m0 + rows_per_split;
  if (m1 > B) m1 = B;
  const int NC16 = L.Cp >> 4;
  {
    // every global load of the tile goes out before the first LDS store (one round trip, not three): A = the 4
    // blocks' D1 rows [KC][16] (transposed into [kj][b]), B = the split's h rows [KC][Cp] in 64-row halves (a
    // second K-chunk of columns only when Cp > KC)
    const int row = tid >> 1, j8 = (tid & 1) * 8;
    const long long b = m0 + row;
    const bool ok = b < m1;
    const long long bb = ok ? b : m1 - 1;
    floatx4 va[8];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = k0 + kk < L.nb ? k0 + kk : L.nb - 1;
      const floatx4* src = reinterpret_cast<const floatx4*>(d1 + ((long long)k * B + bb) * 16 + j8);
      va[2 * kk] = src[0];
      va[2 * kk + 1] = src[1];
    }
    floatx4 rv[2][8];
#pragma unroll
    for (int half = 0; half < 2; ++half) load_rows64<VEC>(h, m1, L.C, L.ldh, m0 + 64 * half, 0, rv[half]);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const float m = (ok && k0 + kk < L.nb) ? 1.f : 0.f;
      const floatx4 v0 = va[2 * kk] * m, v1 = va[2 * kk + 1] * m;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        As[(kk * 16 + j8 + q) * KCP + row] = v0[q];
        As[(kk * 16 + j8 + 4 + q) * KCP + row] = v1[q];
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i4 = tid + 256 * e, r = 64 * half + (i4 >> 5), col = (i4 & 31) * 4;
        if (col < L.Cp) *reinterpret_cast<floatx4*>(Bs + r * hs + col) = rv[half][e];
      }
    }
    for (int c0 = KC; c0 < L.Cp; c0 += KC) {           // Cp > 128 only
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        load_rows64<VEC>(h, m1, L.C, L.ldh, m0 + 64 * half, c0, rv[half]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int i4 = tid + 256 * e, r = 64 * half + (i4 >> 5), col = c0 + (i4 & 31) * 4;
          if (col < L.Cp) *reinterpret_cast<floatx4*>(Bs + r * hs + col) = rv[half][e];
        }
      }
    }
  }
  __syncthreads();
  const int k = k0 + wave;
  float* o = work + (((long long)s * L.nb + (k < L.nb ? k : 0)) * 16) * L.Cp;
  for (int n = 0; n < NC16; ++n) {
    floatx4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < KC / 4; t0 += 8) {            // LDS reads of 8 steps, then 8 MFMAs (2 chains)
      float a[8], bv[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        a[t] = As[(16 * wave + lr) * KCP + 4 * (t0 + t) + lq];
        bv[t] = Bs[(4 * (t0 + t) + lq) * hs + 16 * n + lr];
      }
#pragma unroll
      for (int t = 0; t < 8; t += 2) {
        acc = mfma4(a[t], bv[t], acc);
        acc1 = mfma4(a[t + 1], bv[t + 1], acc1);
      }
    }
    acc += acc1;
    if (k < L.nb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[(long long)(4 * lq + i) * L.Cp + 16 * n + lr] = acc[i];
    }
  }
}


// Folded path's split-K D1^T [x | 1]: the same partials as dw1h_body (work[s][k][16][Cp], one split of KC rows
// each), shaped to share a launch with the slab reduce (k_fold_tail), whose workgroups all get this role's LDS:
//   * two blocks per workgroup, two waves per block with half the column tiles each (twice the workgroups);
//   * the split's KC rows staged as two KH-row halves, so a workgroup holds 4 (32 KHP + KH hs) B of LDS (37 KB at
//     Xp = 96, four workgroups per CU; dw1h_body's whole-split staging of two blocks took 74 KB, two per CU);
//   * each wave keeps acc / acc1 of its NT column tiles across the halves: per tile, t still runs 0 .. KC/4 - 1
//     in order, alternating acc / acc1, then acc += acc1 -- dw1h_body's sums, bit for bit.
// Every global load of a half is issued before its first LDS store: one memory round trip per half (both halves'
// 80 staging registers held at once, or the second half's held under the first half's products, put the launch
// below four waves per SIMD); the column chunks beyond KC of Cp > KC take a round trip of their own.
template <bool VEC, int NT>
__device__ __forceinline__ void dw1h_half_body(const BcnfLayout& L, const float* __restrict__ d1,
                                               const float* __restrict__ h, long long B, int rows_per_split,
                                               float* __restrict__ work, int bx, int by, float* __restrict__ smem,
                                               int ones) {
  const int hs = bstride16(L.Cp);
  float* As = smem;                    // [32][KHP] (kj, b)
  float* Bs = smem + 32 * KHP;         // [KH][hs]  (b, c)
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const int k0 = bx * 2, s = by;
  const long long m0 = (long long)s * rows_per_split;
  long long m1 = m0 + rows_per_split;
  if (m1 > B) m1 = B;
  const int NC16 = L.Cp >> 4;
  // A: the 2 blocks' D1 rows [KH][16] of the half, one float4 per (thread, block); B: the half's rows of h
  const int row = tid >> 2, j4 = (tid & 3) * 4;
  floatx4 va[2], rv[8];
  float am[2];
  auto load_half = [&](int half) {
    rows64_issue<VEC>(h, m1, L.C, L.ldh, m0 + KH * half, 0, rv);
    const long long b = m0 + KH * half + row;
    const bool ok = b < m1;
    const long long bb = ok ? b : m1 - 1;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int k = k0 + kk < L.nb ? k0 + kk : L.nb - 1;
      va[kk] = *reinterpret_cast<const floatx4*>(d1 + ((long long)k * B + bb) * 16 + j4);
      am[kk] = (ok && k0 + kk < L.nb) ? 1.f : 0.f;
    }
  };
  const int kw = wave >> 1, k = k0 + kw;
  const int nh = (NC16 + 1) >> 1, n_lo = (wave & 1) * nh, n_hi = min(NC16, n_lo + nh);   // nh <= NT
  floatx4 acc[NT], acc1[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = acc1[j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    load_half(half);
    if (half) __syncthreads();                          // every wave is done with the first half's tiles
    rows64_mask(m1, L.C, m0 + KH * half, 0, rv, ones);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i4 = tid + 256 * e, r = i4 >> 5, col = (i4 & 31) * 4;
      if (col < L.Cp) *reinterpret_cast<floatx4*>(Bs + r * hs + col) = rv[e];
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const floatx4 v = va[kk] * am[kk];
#pragma unroll
      for (int q = 0; q < 4; ++q) As[(kk * 16 + j4 + q) * KHP + row] = v[q];
    }
    for (int c0 = KC; c0 < L.Cp; c0 += KC) {           // Cp > 128 only
      rows64_issue<VEC>(h, m1, L.C, L.ldh, m0 + KH * half, c0, rv);
      rows64_mask(m1, L.C, m0 + KH * half, c0, rv, ones);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i4 = tid + 256 * e, r = i4 >> 5, col = c0 + (i4 & 31) * 4;
        if (col < L.Cp) *reinterpret_cast<floatx4*>(Bs + r * hs + col) = rv[e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n_lo + j;
      if (n >= n_hi) continue;
#pragma unroll
      for (int t0 = 0; t0 < KH / 4; t0 += 8) {          // LDS reads of 8 steps, then 8 MFMAs (2 chains)
        float a[8], bv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          a[t] = As[(16 * kw + lr) * KHP + 4 * (t0 + t) + lq];
          bv[t] = Bs[(4 * (t0 + t) + lq) * hs + 16 * n + lr];
        }
#pragma unroll
        for (int t = 0; t < 8; t += 2) {
          acc[j] = mfma4(a[t], bv[t], acc[j]);
          acc1[j] = mfma4(a[t + 1], bv[t + 1], acc1[j]);
        }
      }
    }
  }
  if (k >= L.nb) return;
  float* o = work + (((long long)s * L.nb + k) * 16) * L.Cp;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n_lo + j;
    if (n >= n_hi) continue;
    const floatx4 r = acc[j] + acc1[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[(long long)(4 * lq + i) * L.Cp + 16 * n + lr] = r[i];
  }
}

__global__ __launch_bounds__(BCNF_WG) void k_dw1h_reduce(BcnfLayout L, const float* __restrict__ work, int splits,
                                                         float* __restrict__ dparams) {
  const long long per = 16LL * L.Cp, total = (long long)L.nb * per;
  const long long i = (long long)blockIdx.x * BCNF_WG + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i / per);
  const int rem = (int)(i - (long long)k * per);
  const int j = rem / L.Cp, c = rem - j * L.Cp;
  if (j >= L.H[1] || c >= L.C) return;
  float acc = 0.f;
  int s = 0;
  for (; s + 8 <= splits; s += 8) {
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = work[(long long)(s + t) * total + i];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc += v[t];
  }
  for (; s < splits; ++s) acc += work[(long long)s * total + i];
  dparams[coupling_base(L, k) + L.lin_w[1] + j * L.lin_in[1] + L.Da + c] = acc;
}

// Folded path: Gx[kj][xc] = sum of the split-K partials work[s][kj][xc] (fixed order), dense [nb*16][Xp].
__device__ __forceinline__ void gx_reduce_body(long long total, const float* __restrict__ work, int splits,
                                               float* __restrict__ gx, long long i) {
  if (i >= total) return;
  float acc = 0.f;
  int s = 0;
  for (; s + 16 <= splits; s += 16) {               // 16 loads in flight per lane (32 splits at B = 4096)
    float v[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = work[(long long)(s + t) * total + i];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc += v[t];
  }
  for (; s < splits; ++s) acc += work[(long long)s * total + i];
  gx[i] = acc;
}

// Folded path, second launch of the backward tail: the Gx sum alone (6 MB of partials at B = 4096).
__global__ __launch_bounds__(BCNF_WG) void k_fold_gx(long long total, const float* __restrict__ work, int splits,
                                                     float* __restrict__ gx) {
  gx_reduce_body(total, work, splits, gx, (long long)blockIdx.x * BCNF_WG + threadIdx.x);
}

// The slab reduce of the folded tail (reduce_body, below) is cut into contiguous ranges of its workgroups, one per
// launch that takes a share (fold_tail_plan: k_fold_tail and k_fold_finish): the launch's own workgroups come first
// in its grid, block indices past them (`own`) run reduce workgroups first, first + 1, ... k_fold_finish is
// latency-bound and leaves the memory system nearly idle; the slab stream is the tail's only bandwidth-bound work.
// No hand-off: nothing a reduce workgroup reads is written by its launch, and what it writes (dparams and the Adam
// state outside the W1 condition columns) no other role touches.
struct RedShare {
  const float* slab;
  long long stride;     // slab_stride_of
  int nwg;              // slabs (backward workgroups)
  int own, first;       // the launch's own workgroups; the first reduce workgroup of its share
  float* dparams;
};
// Where a reduce workgroup's Adam scalars come from (compile-time): no Adam; derived from the step count inside the
// workgroup (k_fold_tail only: nothing of that launch writes the count); or the two floats k_fold_tail's publisher
// workgroup stored (adam_scalars_publish, the same double arithmetic, so the update is bit-identical), loaded with the
// other operands as k_fold_finish's own roles load them -- k_fold_finish's share, which must not read the step count:
// the keeper thread of that launch advances it at its end.
enum RedAdam { RED_NO_ADAM, RED_ADAM_DERIVED, RED_ADAM_PUBLISHED };

// Deterministic sum of the per-workgroup gradient slabs (fixed order over workgroups). Slab block m (slab_blk_floats
// floats at m * L.sblk) is what the backward's helper waves wrote (BwdJobs): NH + 2 MFMA tiles in lane order, then
// NH + 6 column sums; this maps each element back to its canonical position, or -1 for tile padding (rows / columns
// past a Linear's shape, ActNorm sums of the last block). W1's condition columns come from the split-K GEMM.
// a[i] for a per-lane i through constant indices (scalar argument loads and selects): indexed directly, every such
// read was a per-lane load of the kernel arguments in front of the reduce's first dependent load
template <int N>
__device__ __forceinline__ int lpick(const int (&a)[N], int i) {
  int r = a[0];
#pragma unroll
  for (int t = 1; t < N; ++t) r = (i == t) ? a[t] : r;
  return r;
}

__device__ __forceinline__ long long slab_to_canonical(const BcnfLayout& L, int m, int o) {
  const int NH = L.NH, NW = NH + 2;
  const int cb = m * L.blk_stride + ((m < L.nb - 1) ? L.an_size : 0);      // coupling base
  if (o < NW * 256) {
    const int c = o >> 8, e = o & 255, lane = e >> 2;
    const int row = 4 * (lane >> 4) + (e & 3), col = lane & 15;
    const int l = c < NH ? c + 1 : NH + 1;
    const int nrows = c < NH ? lpick(L.H, l) : L.Db, ncols = (l == 1) ? L.Da : lpick(L.H, l - 1);
    if (row >= nrows || col >= ncols) return -1;
    const int row0 = (c == NH + 1) ? L.Db : 0;
    return (long long)cb + lpick(L.lin_w, l) + (row0 + row) * lpick(L.lin_in, l) + col;
  }
  const int o2 = o - NW * 256, c = o2 >> 4, r = o2 & 15;
  if (c < NH) return r < lpick(L.H, c + 1) ? (long long)cb + lpick(L.lin_b, c + 1) + r : -1;
  if (c < NH + 2) return r < L.Db ? (long long)cb + lpick(L.lin_b, NH + 1) + ((c == NH + 1) ? L.Db : 0) + r : -1;
  const int a = c - NH - 2;
  if (a >= 4 || !L.act_norm || m >= L.nb - 1 || r >= ((a < 2) ? L.Da : L.Db)) return -1;
  return (long long)m * L.blk_stride + ((a & 1) ? L.D : 0) + ((a < 2) ? 0 : L.Da) + r;
}

// RED_O4 output float4 per workgroup x RED_G slab groups (group g sums workgroups g, g+RED_G, ...; RED_T loads
// in flight per lane), combined in a fixed order through LDS. The slab stream is latency-bound on bytes in
// flight: 32 lanes x 16 B x 16 loads per group keeps ~35 MB in flight over the ~580-workgroup grid at B=4096.
constexpr int RED_G = 8, RED_O4 = 32, RED_T = 16;

// With `A` (folded training step inside a multi-step graph, FoldAdamArgs): the reduced gradient of each output also
// takes its Adam update here; the parameters / moments are fetched before the slab stream. The step's two scalars
// are derived in the workgroup (adam_scalars' arithmetic on threads 0 and 64: no earlier launch to publish them to
// this one) once the first round of slab loads is out, and reach the updating threads through LDS and the barrier
// the reduction has anyway: no round trip and no barrier of their own (r06: 5.9 us with the two pows in front of the
// first load).
constexpr int RED_SMEM = RED_G * RED_O4 * 4 + 4;      // floats: the partial sums, then the two scalars

// AM (RedAdam): where the Adam scalars come from.
template <RedAdam AM>
__device__ __forceinline__ void reduce_body(const BcnfLayout& L, const float* __restrict__ slab, long long stride,
                                            int nwg, float* __restrict__ out, int bx, float* __restrict__ smem,
                                            const FoldAdamArgs* A = nullptr) {
  floatx4 (*part)[RED_O4] = reinterpret_cast<floatx4 (*)[RED_O4]>(smem);   // [RED_G][RED_O4]
  float* sc = smem + RED_G * RED_O4 * 4;
  const int g = threadIdx.x / RED_O4, o4 = threadIdx.x % RED_O4;
  const long long i = ((long long)bx * RED_O4 + o4) * 4;
  const bool live = i < stride;
  const long long ic = live ? i : 0;
  const int m = (int)(ic / L.sblk), o = (int)(ic - (long long)m * L.sblk);
  long long ci[4];
  float ap[4], am[4], av[4];
  const float step0 = AM == RED_ADAM_DERIVED ? A->step[0] : 0.f;
  float pub[2] = {0.f, 0.f};
  if (AM == RED_ADAM_PUBLISHED && g == 0) {
    pub[0] = A->asc[0];
    pub[1] = A->asc[1];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ci[e] = slab_to_canonical(L, m, o + e);
    if (AM != RED_NO_ADAM && g == 0) {
      const long long c = ci[e] >= 0 ? ci[e] : 0;
      ap[e] = A->p[0][c];
      am[e] = A->m[0][c];
      av[e] = A->v[0][c];
    }
  }
  bool scalars_due = AM == RED_ADAM_DERIVED;
  auto scalars = [&]() {
    const double t = (double)(step0 + 1.0f);
    if (threadIdx.x == 0) sc[0] = (float)(A->lr / (1.0 - pow(A->b1, t)));
    if (threadIdx.x == 64) sc[1] = (float)sqrt(1.0 - pow(A->b2, t));
    scalars_due = false;
  };
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  int w = g;
  for (; w + RED_G * (RED_T - 1) < nwg; w += RED_G * RED_T) {
    floatx4 v[RED_T];
#pragma unroll
    for (int t = 0; t < RED_T; ++t)
      v[t] = *reinterpret_cast<const floatx4*>(slab + (long long)(w + RED_G * t) * stride + ic);
    if (scalars_due) scalars();                        // under the loads just issued
#pragma unroll
    for (int t = 0; t < RED_T; ++t) acc += v[t];
  }
  for (; w < nwg; w += RED_G) acc += *reinterpret_cast<const floatx4*>(slab + (long long)w * stride + ic);
  if (scalars_due) scalars();                          // fewer than RED_G RED_T slabs: no full round above
  part[g][o4] = acc;
  __syncthreads();
  if (g != 0 || !live) return;
  floatx4 tot = part[0][o4];
#pragma unroll
  for (int q = 1; q < RED_G; ++q) tot += part[q][o4];
  AdamScalars as{};
  if (AM == RED_ADAM_DERIVED) as = adam_scalars_of(*A, sc[0], sc[1]);
  if (AM == RED_ADAM_PUBLISHED) as = adam_scalars_of(*A, pub[0], pub[1]);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (ci[e] < 0) continue;
    out[ci[e]] = tot[e];
    if (AM != RED_NO_ADAM) {
      adam_elem(ap[e], tot[e], am[e], av[e], as);
      A->p[0][ci[e]] = ap[e];
      A->m[0][ci[e]] = am[e];
      A->v[0][ci[e]] = av[e];
    }
  }
}

// A reduce workgroup of k_fold_tail or k_fold_finish (block indices past the launch's own workgroups; a
// workgroup-uniform branch of the caller). Per output element the same reduce_body whichever launch runs it.
template <RedAdam AM>
__device__ __forceinline__ void reduce_share(const BcnfLayout& L, const RedShare& R, const FoldAdamArgs& A,
                                             float* __restrict__ smem) {
  const int bx = R.first + ((int)blockIdx.x - R.own);
  if (A.on && !(A.guard && A.guard[BCNF_GUARD_HALTED])) {      // (a halted step updates nothing)
    reduce_body<AM>(L, R.slab, R.stride, R.nwg, R.dparams, bx, smem, &A);
    return;
  }
  reduce_body<RED_NO_ADAM>(L, R.slab, R.stride, R.nwg, R.dparams, bx, smem);
}

// Folded path, last launch of the backward: two small GEMMs as 16 x 16 output tiles, each operand K-chunk staged
// in LDS as [k][16] in one memory round trip (every load of a chunk issued together: the operands were written by
// other XCDs, so each access is an L2 miss and a streaming K loop of dependent round trips is what costs).
//   role a, workgroups [0, nb * nct): dW1h_k[j][c] = sum_{xc<=X} Gx[k*16+j][xc] Wf1[c][xc]   (Wf1 = [Wf | bf])
//   role b, the rest:               [dWf | dbf][c][xc] = sum_kj W1hR[kj][c] Gx[kj][xc], K = nb*16
// Tile product: thread (ks = lane & 15, rb = lane >> 4, cb = wave) accumulates the 4 x 4 block rows 4rb.., cols
// 4cb.. over k = ks + 16 i (conflict-free ds_read_b128: 16 consecutive rows x 4 float4 per wave), then the 16
// k-slices are summed in a fixed order through LDS.
// wf / bf are k_fold_tail's copy of the feature Linear in the tail's scratch, not the parameters: role b's fused
// Adam updates those in place in this launch, and nothing orders role a's reads before it.
// Behind the two roles' workgroups the grid carries this launch's share of the slab reduce (RedShare): every
// workgroup of the launch has the 64 KB of LDS, two per CU, so 512 slots for the 190 finish workgroups of FC_small
// plus the share.
__device__ __forceinline__ int c0_of_finish(int bx, int nct) { return (bx % nct) * 16; }

constexpr int FIN_KC = 512;                           // K chunk: role a (Xp <= 256) and role b at nb <= 32
                                                      // (K = 16 nb) each load their operands in ONE round trip
constexpr int FIN_SMEM = 2 * FIN_KC * 16;             // As + Bs; the 16 x 256 reduction aliases them

__device__ __forceinline__ void tile16_accum(const float* __restrict__ As, const float* __restrict__ Bs, int kn,
                                             floatx4 (&acc)[4]) {
  const int lane = threadIdx.x & 63, ks = lane & 15, rb = lane >> 4, cb = threadIdx.x >> 6;
#pragma unroll 4
  for (int k = ks; k < kn; k += 16) {
    const floatx4 a = *reinterpret_cast<const floatx4*>(As + k * 16 + 4 * rb);
    const floatx4 b = *reinterpret_cast<const floatx4*>(Bs + k * 16 + 4 * cb);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
  }
}

// Fixed-order sum of the 16 k-slices; returns element (row = tid / 16, col = tid % 16) of the tile.
__device__ __forceinline__ float tile16_reduce(float* __restrict__ red, const floatx4 (&acc)[4]) {
  const int lane = threadIdx.x & 63, ks = lane & 15, rb = lane >> 4, cb = threadIdx.x >> 6;
  __syncthreads();                                    // the staging buffers are reused
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) red[ks * 256 + (4 * rb + r) * 16 + 4 * cb + c] = acc[r][c];
  __syncthreads();
  float v = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) v += red[q * 256 + threadIdx.x];
  return v;
}

__global__ __launch_bounds__(BCNF_WG) void k_fold_finish(BcnfLayout L, const float* __restrict__ pk,
                                                         const float* __restrict__ gx, const float* __restrict__ wf,
                                                         const float* __restrict__ bf, int X,
                                                         float* __restrict__ dparams, float* __restrict__ dwf,
                                                         float* __restrict__ dbf, FoldAdamArgs A, RedShare R) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // FIN_SMEM floats (64 KB: dynamic)
  if ((int)blockIdx.x >= R.own) {                      // this launch's share of the slab reduce (RedShare)
    reduce_share<RED_ADAM_PUBLISHED>(L, R, A, smem);
    return;
  }
  float* As = smem;
  float* Bs = smem + FIN_KC * 16;
  const int Xp = fold_xp(X), tid = threadIdx.x, nct = L.Cp >> 4;
  floatx4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = floatx4{0.f, 0.f, 0.f, 0.f};
  // fused Adam (FoldAdamArgs): this thread's output is one parameter whose gradient it computes; its parameter and
  // moments are fetched now, the update follows the tile product. The launch's last workgroup does the step's
  // bookkeeping (bcnf_adam_step_bookkeep semantics), workgroup 0 stores the logged values.
  // The scalars come from k_fold_tail (adam_scalars_publish); workgroup 0's log row index is loaded now and its
  // system-scope stores issued once the operands are staged, their fence at the end (no round trip up front).
  const bool adam = A.on && !(A.guard && A.guard[BCNF_GUARD_HALTED]);
  AdamScalars as{};
  // Workgroup 0's thread 0 keeps the step's books (bcnf_adam_step_bookkeep semantics): it alone reads the step count
  // and the cursor in this launch (the scalars came from k_fold_tail), so it advances both itself at its end --
  // no arrival counter, no last-workgroup round trip.
  const bool keeper = adam && blockIdx.x == 0 && tid == 0;
  const bool logger = keeper && A.log_values && A.log_history;
  long long log_row = 0;
  float step0 = 0.f, log_v[3];
  if (adam) {
    as = adam_scalars_of(A, A.asc[0], A.asc[1]);
    if (keeper) {
      log_row = A.cursor ? A.cursor[0] : 0LL;
      step0 = A.step[0];
    }
    if (logger) {
#pragma unroll
      for (int i = 0; i < 3; ++i) log_v[i] = A.log_values[i];
    }
  }
  int slot = -1;                                       // which parameter tensor / element this thread updates
  long long idx = 0;
  float ap = 0.f, am = 0.f, av = 0.f;
  if ((int)blockIdx.x < L.nb * nct) {
    const int j = tid >> 4, c = c0_of_finish(blockIdx.x, nct) + (tid & 15), k = blockIdx.x / nct;
    if (j < L.H[1] && c < L.C) {
      slot = 0;
      idx = coupling_base(L, k) + L.lin_w[1] + j * L.lin_in[1] + L.Da + c;
    }
  } else {
    const int tile = blockIdx.x - L.nb * nct, c = (tile % nct) * 16 + (tid >> 4), x = (tile / nct) * 16 + (tid & 15);
    if (c < L.C) {
      if (x < X) {
        slot = 1;
        idx = (long long)c * X + x;
      } else if (x == X && dbf) {
        slot = 2;
        idx = c;
      }
    }
  }
  // the slot's tensors picked with constant indices (scalar argument loads + a per-lane select): indexed by the
  // per-lane slot they were per-lane loads of the kernel arguments, a round trip in front of the p / m / v loads
  float *sp = nullptr, *sm = nullptr, *sv = nullptr;
  if (adam) {
    if (slot == 0) {
      sp = A.p[0]; sm = A.m[0]; sv = A.v[0];
    } else if (slot == 1) {
      sp = A.p[1]; sm = A.m[1]; sv = A.v[1];
    } else if (slot == 2) {
      sp = A.p[2]; sm = A.m[2]; sv = A.v[2];
    }
  }
  if (sp) {
    ap = sp[idx];
    am = sm[idx];
    av = sv[idx];
  }
  auto finish_elem = [&](float gval) {
    if (!sp) return;
    adam_elem(ap, gval, am, av, as);
    sp[idx] = ap;
    sm[idx] = am;
    sv[idx] = av;
  };
  auto arrive = [&]() {
    if (!keeper) return;
    if (logger) __threadfence_system();                // the log row's stores (system scope)
    A.step[0] = step0 + 1.0f;                          // advance_counters on the values read at the start
    if (A.cursor) {
      const long long c = log_row + 1;
      A.cursor[0] = c < A.n_batches ? c : 0;
    }
  };
  if ((int)blockIdx.x < L.nb * nct) {
    const int k = blockIdx.x / nct, c0 = (blockIdx.x % nct) * 16;
    const float* g = gx + (long long)k * 16 * Xp;     // [16][Xp], contiguous
    float va[16], vb[16];                             // every load issued before the first LDS store
#pragma unroll
    for (int e = 0; e < 16; ++e) {                    // 16 Xp <= 16 * 256: at most 16 elements per thread
      const int i = tid + BCNF_WG * e;
      const int j = i / Xp, xc = i - j * Xp, c = c0 + j;   // (row, xc) of Gx_k and of Wf1[c0 + row]
      const bool in = i < 16 * Xp;
      va[e] = in ? g[i] : 0.f;
      float v = 0.f;
      if (in && c < L.C) v = xc < X ? wf[(long long)c * X + xc] : ((xc == X && bf) ? bf[c] : 0.f);
      vb[e] = v;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = tid + BCNF_WG * e;
      if (i < 16 * Xp) {
        const int j = i / Xp, xc = i - j * Xp;
        As[xc * 16 + j] = va[e];
        Bs[xc * 16 + j] = vb[e];
      }
    }
    __syncthreads();
    if (logger) {                                     // the step's logged values -> history row of this batch
#pragma unroll
      for (int i = 0; i < 3; ++i)
        __hip_atomic_store(A.log_history + 3 * log_row + i, log_v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    tile16_accum(As, Bs, Xp, acc);
    const float v = tile16_reduce(smem, acc);
    const int j = tid >> 4, c = c0 + (tid & 15);
    if (j < L.H[1] && c < L.C) dparams[coupling_base(L, k) + L.lin_w[1] + j * L.lin_in[1] + L.Da + c] = v;
    finish_elem(v);
    __syncthreads();
    arrive();
    return;
  }
  const int tile = blockIdx.x - L.nb * nct, c0 = (tile % nct) * 16, x0 = (tile / nct) * 16;
  const int K = L.nb * 16;
  const float* w1r = pk + L.w1r_off + c0;             // W1hR [NKp][Cp], zero beyond C
  for (int k0 = 0; k0 < K; k0 += FIN_KC) {
    const int kn = min(FIN_KC, K - k0);
    if (k0) __syncthreads();
    floatx4 va[FIN_KC * 4 / BCNF_WG], vb[FIN_KC * 4 / BCNF_WG];
#pragma unroll
    for (int e = 0; e < FIN_KC * 4 / BCNF_WG; ++e) {   // row = i4 / 4, float4 q = i4 % 4
      const int i4 = tid + BCNF_WG * e, r = i4 >> 2, q = i4 & 3, kj = k0 + (r < kn ? r : 0);
      va[e] = *reinterpret_cast<const floatx4*>(w1r + (long long)kj * L.Cp + 4 * q);
      vb[e] = *reinterpret_cast<const floatx4*>(gx + (long long)kj * Xp + x0 + 4 * q);
    }
#pragma unroll
    for (int e = 0; e < FIN_KC * 4 / BCNF_WG; ++e) {
      const int i4 = tid + BCNF_WG * e;
      reinterpret_cast<floatx4*>(As)[i4] = va[e];
      reinterpret_cast<floatx4*>(Bs)[i4] = vb[e];
    }
    __syncthreads();
    tile16_accum(As, Bs, kn, acc);
  }
  const float v = tile16_reduce(smem, acc);
  const int c = c0 + (tid >> 4), x = x0 + (tid & 15);
  if (c < L.C) {
    if (x < X) {
      if (dwf) dwf[(long long)c * X + x] = v;
    } else if (x == X && dbf) {
      dbf[c] = v;
    }
  }
  finish_elem(v);
  __syncthreads();
  arrive();
}

// The backward's tail in ONE launch: dL/dh tiles, the slab reduction and the W1 condition-part split-K
// partials are independent, so their workgroups share a grid (role by block index) and run
// concurrently instead of paying three launch floors back to back.
struct TailGrid {
  int n_dh, gx_dh;      // dh tiles: (gx_dh x Cp/16), 0 if dh is not requested
  int n_red;            // slab-reduce workgroups
  int gx_dw;            // dW1h: (gx_dw x splits)
};

template <bool VEC>
__global__ __launch_bounds__(BCNF_WG) void k_bwd_tail(BcnfLayout L, TailGrid G, const float* __restrict__ pk,
                                                      const float* __restrict__ d1, const float* __restrict__ h,
                                                      long long B, float* __restrict__ dh,
                                                      const float* __restrict__ slab, long long stride, int nwg,
                                                      float* __restrict__ dparams, int rows_per_split,
                                                      float* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int i = blockIdx.x;
  if (i < G.n_dh) {
    dh_body(L, pk, d1, B, dh, i % G.gx_dh, i / G.gx_dh, smem);
    return;
  }
  i -= G.n_dh;
  if (i < G.n_red) {
    reduce_body<RED_NO_ADAM>(L, slab, stride, nwg, dparams, i, smem);
    return;
  }
  i -= G.n_red;
  dw1h_body<VEC>(L, d1, h, B, rows_per_split, work, i % G.gx_dw, i / G.gx_dw, smem);
}

// Folded path, first launch of the backward tail: the split-K D1^T [x | 1] (latency-bound: 27 MB and 0.4 GFLOP at
// B = 4096, waiting on D1 rows k_backward wrote from other XCDs) and the slab reduce (HBM-bound, 90 MB) depend on
// k_backward alone and share this launch. Block-index ranges, in dispatch order:
//   [0, n_sk)   split-K workgroups (dw1h_half_body), first, so their round trip starts at once and the stream of the
//               reduce fills the machine behind them;
//   n_sk        one workgroup: copies [Wf | bf] into the tail's scratch for k_fold_finish (which Adam-updates the
//               tensors themselves) and publishes the step's Adam scalars for it;
//   the rest    slab reduce (reduce_body) of this launch's share of the reduce workgroups (fold_tail_plan: the other
//               share runs behind k_fold_finish's own workgroups), with the fused Adam's scalars derived in each
//               workgroup.
// The order is for speed only: no role reads what another role of this launch writes.
// An earlier one-launch tail (r01j) measured 28 us against 13 + 10 for two launches, for two reasons that were not
// the overlap itself: its grid put the split-K last, so the latency-bound role ran alone at the end, and every
// workgroup carried the split-K's 74 KB of LDS, so the ~625 reduce workgroups (2.4 per CU, which must all be
// resident to keep their loads in flight) ran two per CU in two rounds. Here the split-K leads and stages 37 KB.
template <bool VEC, int NT>
__global__ __launch_bounds__(BCNF_WG, VEC && NT <= 3 ? 4 : 2) void k_fold_tail(BcnfLayout L, BcnfLayout F, const float* __restrict__ d1,
                                                       const float* __restrict__ x, long long B, int rows_per_split,
                                                       float* __restrict__ work, int gx_dw, int n_sk, int ones,
                                                       RedShare R, const float* __restrict__ wf,
                                                       const float* __restrict__ bf, float* __restrict__ wf1,
                                                       FoldAdamArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int bx = blockIdx.x;
  if (bx < n_sk) {
    dw1h_half_body<VEC, NT>(F, d1, x, B, rows_per_split, work, bx % gx_dw, bx / gx_dw, smem, ones);
    return;
  }
  if (bx == n_sk) {
    const int nw = L.C * F.C, n1 = nw + (bf ? L.C : 0);   // wf1 = Wf [C][X], then bf [C]
    for (int i0 = 0; i0 < n1; i0 += 16 * BCNF_WG) {
      float v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = min(i0 + e * BCNF_WG + (int)threadIdx.x, n1 - 1);
        v[e] = i < nw ? wf[i] : bf[i - nw];
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = i0 + e * BCNF_WG + (int)threadIdx.x;
        if (i < n1) wf1[i] = v[e];
      }
    }
    if (A.on && threadIdx.x == 0) adam_scalars_publish(A);
    return;
  }
  reduce_share<RED_ADAM_DERIVED>(L, R, A, smem);
}

constexpr int FOLD_RED_FIN_8THS = 2;   // k_fold_finish's share of the slab reduce (fold_tail_plan)

}  // namespace

namespace bcnf_small {

int launch_tail(const BcnfLayout& L, const float* pk, const float* slab, const float* h, const float* ws,
                long long batch, float* dh, float* dparams, hipStream_t st) {
  const long long S = slab_stride_of(L);
  const int nwg = (int)((batch + 15) / 16);
  const float* d1 = ws + ws_d1_off(L, batch);
  float* work = const_cast<float*>(slab) + (long long)nwg * S;
  const int rps = W1H_ROWS_PER_SPLIT;
  const long long splits = w1h_splits(batch);
  TailGrid G;
  G.gx_dh = (int)((batch + 63) / 64);
  G.n_dh = dh ? G.gx_dh * (L.Cp >> 4) : 0;
  G.n_red = (int)((S / 4 + RED_O4 - 1) / RED_O4);
  G.gx_dw = (L.nb + 3) / 4;
  const long long n_dw = (long long)G.gx_dw * splits;
  size_t lds = dw1h_lds_bytes(L);
  if (dh_lds_bytes() > lds) lds = dh_lds_bytes();
  const dim3 grid((unsigned)(G.n_dh + G.n_red + n_dw));
  const int rc = vec_rows(L, h) ? launch<k_bwd_tail<true>>(grid, dim3(BCNF_WG), lds, st, L, G, pk, d1, h, batch, dh, slab,
                                                           S, nwg, dparams, rps, work)
                                : launch<k_bwd_tail<false>>(grid, dim3(BCNF_WG), lds, st, L, G, pk, d1, h, batch, dh, slab,
                                                            S, nwg, dparams, rps, work);
  if (rc) return rc;
  const long long outs = (long long)L.nb * 16 * L.Cp;
  return launch<k_dw1h_reduce>(dim3((unsigned)((outs + BCNF_WG - 1) / BCNF_WG)), dim3(BCNF_WG), 0, st, L,
                               (const float*)work, (int)splits, dparams);
}

int launch_dh(const BcnfLayout& L, const float* pk, const float* ws, long long batch, float* dh, hipStream_t st) {
  const float* d1 = ws + ws_d1_off(L, batch);
  return launch<k_dh>(dim3((unsigned)((batch + 63) / 64), (unsigned)(L.Cp >> 4)), dim3(BCNF_WG), dh_lds_bytes(), st, L,
                      pk, d1, batch, dh);
}

FoldTailPlan fold_tail_plan(const BcnfLayout& L, const BcnfLayout& F, int64_t batch) {
  FoldTailPlan P;
  P.S = slab_stride_of(L);
  P.splits = w1h_splits(batch);
  P.n_red = (int)((P.S / 4 + RED_O4 - 1) / RED_O4);
  P.gx_dw = (L.nb + 1) / 2;
  P.own[0] = (int)(P.gx_dw * P.splits) + 1;
  P.own[1] = (int)(((long long)L.nb * 16 * F.Cp + BCNF_WG - 1) / BCNF_WG);
  P.own[2] = (L.nb + (F.Cp >> 4)) * (L.Cp >> 4);
  P.count[1] = 0;
  P.count[2] = (int)((long long)P.n_red * FOLD_RED_FIN_8THS / 8);
  P.count[0] = P.n_red - P.count[2];
  P.first[0] = 0;
  P.first[1] = P.first[2] = P.count[0];
  return P;
}

int launch_fold_tail(const BcnfLayout& L, const BcnfLayout& F, const float* pk, float* slab, const float* x,
                     const float* feat_weight, const float* feat_bias, const float* ws, long long batch,
                     float* dparams, float* dfeat_weight, float* dfeat_bias, FoldAdamArgs A, hipStream_t st) {
  const int in_features = F.C;
  const FoldTailPlan P = fold_tail_plan(L, F, batch);
  const long long S = P.S;
  const int nwg = (int)((batch + 15) / 16);
  const float* d1 = ws + ws_d1_off(L, batch);
  float* work = slab + (long long)nwg * S;
  float* gx = work + w1h_work_floats(F, batch);
  A.asc = gx + (long long)L.nb * 16 * F.Cp;
  const int rps = W1H_ROWS_PER_SPLIT;
  float* wf1 = A.asc + 4;                              // [Wf | bf] as k_fold_finish's role a reads them
  const float* bf1 = feat_bias ? wf1 + (long long)L.C * in_features : nullptr;
  RedShare R[3];
  unsigned grid[3];
  for (int t = 0; t < 3; ++t) {
    R[t] = RedShare{(const float*)slab, S, nwg, P.own[t], P.first[t], dparams};
    grid[t] = (unsigned)(P.own[t] + P.count[t]);
  }
  const int n_sk = P.own[0] - 1;
  size_t lds = dw1h_half_lds_bytes(F);
  if (lds < sizeof(float) * RED_SMEM) lds = sizeof(float) * RED_SMEM;
  const bool vec = vec_rows(F, x);
  const bool nt3 = (F.Cp >> 4) <= 6;                   // column tiles per wave: 3 (Xp <= 96: FC_small) or 8
#define FOLD_TAIL(V, NT)                                                                                          \
  launch<k_fold_tail<V, NT>>(dim3(grid[0]), dim3(BCNF_WG), lds, st, L, F, d1, x, batch, rps, work, P.gx_dw, n_sk,      \
                             in_features, R[0], feat_weight, feat_bias, wf1, A)
  int rc = vec ? (nt3 ? FOLD_TAIL(true, 3) : FOLD_TAIL(true, 8)) : (nt3 ? FOLD_TAIL(false, 3) : FOLD_TAIL(false, 8));
#undef FOLD_TAIL
  if (rc) return rc;
  const long long total = (long long)L.nb * 16 * F.Cp;
  rc = launch<k_fold_gx>(dim3(grid[1]), dim3(BCNF_WG), 0, st, total, (const float*)work, (int)P.splits, gx);
  if (rc) return rc;
  return launch<k_fold_finish>(dim3(grid[2]), dim3(BCNF_WG), sizeof(float) * FIN_SMEM, st, L, pk, (const float*)gx,
                               (const float*)wf1, bf1, in_features, dparams, dfeat_weight, dfeat_bias, A, R[2]);
}

}  // namespace bcnf_small
