// bcnf_amd small stack family: the whole-stack inverse -- the condition projection GEMM in front of it (k_hp), the
// row-layout inverse that draws dropout masks (k_inverse, training mode) and the matrix-core inverse of eval
// (k_inverse_mfma, optionally with log|det J| and log_prob). The family's files: bcnf_stack_internal.h.
#include "bcnf_stack_internal.h"
#include "bcnf_stack_rec.h"

namespace {
using namespace bcnf_small;
using bcnf_rt::launch;

// HP[k][r][j] = sum_c h[r][c] W1_k[j][Da + c] + b1_k[j], the y-independent part of Linear 1, as one fp32 MFMA GEMM
// (operand staging and LDS strides: the projection GEMMs of bcnf_stack_tail.hip).
// HP tile: 64 rows x 64 columns kj. grid = (ceil(R/64), NKp/64)
template <bool VEC>
__global__ __launch_bounds__(BCNF_WG) void k_hp(BcnfLayout L, const float* __restrict__ pk,
                                                const float* __restrict__ h, long long R, float* __restrict__ hp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                    // [64][KCP]  (row, c)
  float* Bs = smem + 64 * KCP;         // [KC][BNS]  (c, kj)
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const long long b0 = (long long)blockIdx.x * 64;
  const int n0 = blockIdx.y * 64;
  const int Cp = L.Cp, NKp = L.NKp;
  const float* w1c = pk + L.w1c_off;
  floatx4 ra[8], rb[8];
  auto load = [&](int c0) {
    load_rows64<VEC>(h, R, L.C, L.ldh, b0, c0, ra);
#pragma unroll
    for (int e = 0; e < 8; ++e) {                    // B: [KC rows c][64 cols]: row = i4 / 16, col4
      const int i4 = tid + 256 * e, row = c0 + (i4 >> 4), col = n0 + (i4 & 15) * 4;
      const floatx4 v = *reinterpret_cast<const floatx4*>(w1c + (long long)(row < Cp ? row : Cp - 1) * NKp + col);
      rb[e] = v * (row < Cp ? 1.f : 0.f);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i4 = tid + 256 * e;
      *reinterpret_cast<floatx4*>(As + (i4 >> 5) * KCP + (i4 & 31) * 4) = ra[e];
      *reinterpret_cast<floatx4*>(Bs + (i4 >> 4) * BNS + (i4 & 15) * 4) = rb[e];
    }
  };
  floatx4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = floatx4{0.f, 0.f, 0.f, 0.f};
  load(0);
  float b1v[4];                                        // the epilogue's biases, fetched with the first chunk
#pragma unroll
  for (int u = 0; u < 4; ++u) b1v[u] = pk[L.b1c_off + n0 + 16 * u + lr];
  for (int c0 = 0; c0 < Cp; c0 += KC) {
    store();
    __syncthreads();
    if (c0 + KC < Cp) load(c0 + KC);
    const int ks = (Cp - c0 < KC ? Cp - c0 : KC) >> 2;   // multiple of 4
    for (int t0 = 0; t0 < ks; t0 += 4) {
      float a[4], bv[4][4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[t] = As[(16 * wave + lr) * KCP + 4 * (t0 + t) + lq];
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[t][u] = Bs[(4 * (t0 + t) + lq) * BNS + 16 * u + lr];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = mfma4(a[t], bv[t][u], acc[u]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int kj = n0 + 16 * u + lr, k = kj >> 4;
    if (k < L.nb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long r = b0 + 16 * wave + 4 * lq + i;
        if (r < R) hp[((long long)k * R + r) * 16 + lr] = acc[u][i] + b1v[u];
      }
    }
  }
}

// Whole-stack inverse on the row layout, one launch: the training-mode inverse, which draws the forward's dropout
// masks under tag 0x40000000 (eval takes k_inverse_mfma, below).
template <int NH>
__global__ __launch_bounds__(BCNF_WG) void k_inverse(BcnfLayout L, const float* __restrict__ pk,
                                                     const float* __restrict__ zin, const float* __restrict__ hp,
                                                     long long R, const int64_t* __restrict__ cond_index, long long N,
                                                     float* __restrict__ yout, const uint64_t* __restrict__ rng) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int RFL = 16 * L.RF;
  float* rec = smem;
  const int tid = threadIdx.x, j = tid & 15, s = tid >> 4;
  const long long b = (long long)blockIdx.x * 16 + s;
  const long long bc = b < N ? b : N - 1;
  const int D = L.D, Da = L.Da, Db = L.Db, nb = L.nb;
  const float* pi = pk + L.pi_off;
  const long long hr = cond_index ? (long long)cond_index[bc] : bc;   // projection row of this sample
  const float* hpl = hp + hr * 16 + j;                                // HP[k][hr][j] = hpl[k * R * 16]
  const long long hps = R * 16;

  float ya = (j < Da) ? zin[bc * D + j] : 0.f;
  float yb = (j < Db) ? zin[bc * D + Da + j] : 0.f;
  const uint64_t seed = rng[0], off = rng[1];
  const int kl = nb - 1;
  float hp_n = hpl[kl * hps];
  {
    Stage<STAGE_REC> sr;
    sr.load(pi + (long long)kl * RFL, RFL);
    sr.store(rec + (kl & 1) * RING);
  }
  __syncthreads();

  for (int k = kl; k >= 0; --k) {
    const int cur = k & 1;
    const int k1 = k >= 1 ? k - 1 : 0;                // clamped: no branches
    Stage<STAGE_REC> sr;
    sr.load(pi + (long long)k1 * RFL, RFL);
    const float hpk = hp_n;
    hp_n = hpl[k1 * hps];
    __builtin_amdgcn_sched_barrier(0);
    float rr[RecF<NH>::USED];
    ld_rec<0, RecF<NH>::USED>(rr, rec + cur * RING + j * L.RF);
    float za, zb;
    if (QBC_DEV(L, QBC_MIX)) mix_bc(rr + RecF<NH>::Q, ya, yb, za, zb);   // z @ Q^T (cnf.py:339); identity for the last block
    else mix(rr + RecF<NH>::Q, ya, yb, za, zb);
    const uint32_t bits = dropout_bits<NH>(L, seed, off, bc, k, j, 0x40000000u);
    float T, Sp;
    mlp_forward<NH>(L, rr, za, hpk, bits, T, Sp);
    const float S = tanh_bf(Sp);
    const float ybn = (zb - T) * exp_fast(-S);         // cnf.py:205
    ya = (j < Da) ? (za - rr[1]) * rr[0] : 0.f;        // ActNorm inverse (cnf.py:353-354), rr[0] = 1 / scale;
    yb = (j < Db) ? (ybn - rr[3]) * rr[2] : 0.f;       // identity where none
    sr.store(rec + (cur ^ 1) * RING);
    __syncthreads();
  }
  if (b < N) {
    if (j < Da) yout[b * D + j] = ya;
    if (j < Db) yout[b * D + Da + j] = yb;
  }
}

// Whole-stack inverse on the matrix cores (eval / no dropout: sampling, cnf.py:499-506 via _sample), 16 samples
// per wave. A feature vector of the wave's samples is 4 registers per lane: lane (q = l >> 4, s = l & 15) holds
// features 4q .. 4q+3 of sample s -- exactly the v_mfma_f32_16x16x4f32 output layout D[4q + r][s] of out = W x
// (rows = out features, columns = samples). Contracting the 16 inputs in 4 MFMA steps with input feature 4q + t
// in K-slot q of step t makes the B operand of step t the lane's own register t, so a dense 16 x 16 layer is 4
// MFMAs with no data movement; the A operand (W[s][4q + t]) is one LDS read per step from the same pre-rotated
// inverse record k_inverse uses (entry (o - c) & 15 of out-row o). Mix, Linear 1 (condition part + bias from k_hp
// as the accumulator), hidden layers and the T / S heads run on the matrix pipe; the VALU keeps GELU, tanh, exp
// and the coupling / ActNorm inverse (row-layout k_inverse: ~380 VALU instructions per block per 4 samples, 95% of
// VALU issue in profiles/r02y_k_inverse_pmc_insts.csv). Same sums as k_inverse in a different association order.
// G independent 16-sample groups per wave interleaving their MFMA chains and GELUs (G = 2 measured neutral, DESIGN 3e;
// again with the r04 GELU: 1.304 against 1.295 ms per 512k draws, profiles/r04zc_ab_sample.txt).
constexpr int INV_M_G = 1;
constexpr int INV_M_SPW = 16 * INV_M_G;              // samples per wave
constexpr int INV_M_WG = 512;                       // 8 waves share one record ring (2 x 16 KB): 4 workgroups per CU
constexpr int INV_M_SPB = INV_M_SPW * (INV_M_WG / 64);

typedef float f32x2 __attribute__((ext_vector_type(2)));   // a pair for packed fp32 arithmetic (v_pk_fma_f32)
// max(x, 0) as ONE v_max_f32 (fmaxf under IEEE mode adds a canonicalising max per operand). hipcc pads no hazard
// inside an asm string, and x is usually an MFMA result (its D needs 12 wait states before any VALU read,
// cdna_hip_programming.md, inline-asm rule 2): `after` is a value hipcc computed from x with the pad in front of it,
// so the dependency places this read behind that pad.
__device__ __forceinline__ float relu_f(float x, float after) {
  float r;
  asm("v_max_f32_e32 %0, 0, %1" : "=v"(r) : "v"(x), "v"(after));
  return r;
}
// GELU for the forward-only kernels (sampling): x Phi(x) = max(x, 0) - |x| h(|x|) with log2 h fitted as ONE degree-6
// polynomial in a = min(|x|, 6.5) (the -x^2/2 of erfc's decay is quadratic in a, so it is inside the fit): one exp2
// and no reciprocal per element, 14 instructions per pair (the rational erfc fit of gelu_f took 20, four of them
// transcendental). The pair form of bcnf_device.h gelu_h / gelu_f (same coefficients): fp32 error <= 1 ulp of the result
// above 0, <= 1e-7 below (tools/fit_erf.py: fit_log2h); past |x| = 6.5, |x| h < 3e-10.
__device__ __forceinline__ f32x2 gelu_p2(f32x2 x) {
  // med3(|x|, 0, 6.5): ONE v_med3_f32 with the |x| source modifier (fminf under IEEE mode adds a canonicalising
  // v_max first)
  const f32x2 a = {__builtin_amdgcn_fmed3f(fabsf(x.x), 0.f, 6.5f), __builtin_amdgcn_fmed3f(fabsf(x.y), 0.f, 6.5f)};
  f32x2 p = {3.3094816899392754e-05f, 3.3094816899392754e-05f};
  p = __builtin_elementwise_fma(p, a, f32x2{-7.692371727898717e-04f, -7.692371727898717e-04f});
  p = __builtin_elementwise_fma(p, a, f32x2{8.080773986876011e-03f, 8.080773986876011e-03f});
  p = __builtin_elementwise_fma(p, a, f32x2{-5.3412191569805145e-02f, -5.3412191569805145e-02f});
  p = __builtin_elementwise_fma(p, a, f32x2{-4.5877090096473694e-01f, -4.5877090096473694e-01f});
  p = __builtin_elementwise_fma(p, a, f32x2{-1.1512017250061035e+00f, -1.1512017250061035e+00f});
  p = __builtin_elementwise_fma(p, a, f32x2{-9.99993085861206e-01f, -9.99993085861206e-01f});
  const f32x2 h = {__builtin_amdgcn_exp2f(p.x), __builtin_amdgcn_exp2f(p.y)};
  return f32x2{fmaf(-fabsf(x.x), h.x, relu_f(x.x, a.x)), fmaf(-fabsf(x.y), h.y, relu_f(x.y, a.y))};
}
__device__ __forceinline__ void gelu4(floatx4& a) {
  const f32x2 lo = gelu_p2(f32x2{a[0], a[1]}), hi = gelu_p2(f32x2{a[2], a[3]});
  a[0] = lo.x;
  a[1] = lo.y;
  a[2] = hi.x;
  a[3] = hi.y;
}

constexpr int INV_M_OCC = 6;   // min waves per SIMD (80 VGPRs, no spills; 5 and 8 measured slower)

// One dense layer on the matrix cores: the lane's A operands of the KS K-steps are ONE float4 of the operand-ordered
// record (rec_pm: matrix mat, lane l), conflict-free ds_read_b128.
template <int G, int KS>
__device__ __forceinline__ void inv_mv_mo(floatx4 (&acc)[G], const float* __restrict__ mat, int l,
                                          const floatx4 (&x)[G]) {
  const floatx4 w = *reinterpret_cast<const floatx4*>(mat + 4 * l);
#pragma unroll
  for (int t = 0; t < KS; ++t) {
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = mfma4(w[t], x[g][t], acc[g]);
  }
}

// PERM (D_a, D_b <= 12): the y / z half-vectors hold feature 3q + r in register r < 3 of lane (q, s) (register 3
// stays 0), so every product with a half-vector input contracts in 3 MFMA steps instead of 4 (mix 16 -> 12 and
// Linear 1 4 -> 3 MFMAs per block) and the coupling / ActNorm inverse runs on 3 registers. Rows of a permuted
// output with no feature read entry 0 of lane record 15, which is zero in the mix, T and S rows when D_a, D_b < 15.
// LDJ: also the forward's log|det J| at the returned y (and log_prob of it). A one-way coupling's inverse passes the
// identity half through, so the S = tanh(s') it forms at block k IS the forward's S at y: each lane keeps the running
// sum of S over its valid features (registers in order, blocks nb - 1 .. 0), the four 16-lane rows are added once
// after the loop (sum_rows4), then the packed ActNorm constant; |z|^2 comes from the prologue's z loads the same way.
template <int NH, bool PERM, bool LDJ = false>
__global__ __launch_bounds__(INV_M_WG, PERM ? INV_M_OCC - 1 : INV_M_OCC) void k_inverse_mfma(BcnfLayout L, const float* __restrict__ pk,
                                                          const float* __restrict__ zin, const float* __restrict__ hp,
                                                          long long R, const int64_t* __restrict__ cond_index,
                                                          long long N, float* __restrict__ yout,
                                                          float* __restrict__ ldj_out = nullptr,
                                                          float* __restrict__ logp_out = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using F = RecF<NH>;
  constexpr int G = INV_M_G;
  constexpr int KA = PERM ? 3 : 4;                  // MFMA steps over a half-vector input
  constexpr int NM = NH + 6;                         // matrices of the operand-ordered record (rec_pm)
  constexpr int PMB = NM * 256 + (NH - 1) * 16 + 32 + 64;   // == L.PMB (layout_matches)
  constexpr int BIAS = NM * 256, TSB = BIAS + (NH - 1) * 16, ANB = TSB + 32;
  static_assert(PMB <= RING, "operand-ordered record fits a ring slot");
  float* rec = smem;
  const int l = threadIdx.x & 63, q = l >> 4, s = l & 15;
  const int D = L.D, Da = L.Da, Db = L.Db, nb = L.nb;
  const float* pm = pk + L.pm_off;
  long long b[G];
  const floatx4* hpl[G];
  const long long hps4 = R * 4;
  // half-vector feature of register r (15: none -- a zero row of the mix / T / S records)
  auto feat = [&](int r) { return PERM ? (r < 3 ? 3 * q + r : 15) : 4 * q + r; };
  floatx4 ya[G], yb[G];
  float ls[G];                                      // LDJ: the lane's sum of S over its valid features
#pragma unroll
  for (int g = 0; g < G; ++g) {
    b[g] = (long long)blockIdx.x * INV_M_SPB + (threadIdx.x >> 6) * INV_M_SPW + 16 * g + s;
    const long long bc = b[g] < N ? b[g] : N - 1;
    const long long hr = cond_index ? (long long)cond_index[bc] : bc;
    hpl[g] = reinterpret_cast<const floatx4*>(hp + hr * 16 + 4 * q);   // HP[k][hr][4q..4q+3]
    ls[g] = 0.f;
    float zz = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = feat(r);
      ya[g][r] = (f < Da) ? zin[bc * D + f] : 0.f;
      yb[g][r] = (f < Db) ? zin[bc * D + Da + f] : 0.f;
      if (LDJ) zz += ya[g][r] * ya[g][r] + yb[g][r] * yb[g][r];
    }
    if (LDJ && logp_out) {
      // log_prob's latent term now, while z is in registers; the epilogue adds ldj to it (the same lane stores and
      // reloads it, so no register stays live across the coupling loop for it)
      const float q2 = sum_rows4(zz);
      if (q == 0 && b[g] < N) logp_out[b[g]] = -0.5f * q2 - 0.5f * (float)D * 1.8378770664093454836f;
    }
  }

  const int kl = nb - 1;
  floatx4 hp_n[G];
#pragma unroll
  for (int g = 0; g < G; ++g) hp_n[g] = hpl[g][kl * hps4];
  // record staging by LDS-DMA (global_load_lds_dwordx4, no staging registers): wave w copies 1 KB chunks
  // w, w + 8 of block k's record into a ring slot; chunks past the record re-read its start (slot slack)
  const int wv = threadIdx.x >> 6;
  static_assert(RING % (INV_M_WG * 4) == 0, "ring chunks per wave");
  auto stage = [&](int k, float* dst) {
#pragma unroll
    for (int c = 0; c < RING / (INV_M_WG * 4); ++c) {
      const int ch = wv + (INV_M_WG / 64) * c, e = ch * 256 + 4 * l;
      const float* src = pm + (long long)k * PMB + (e < PMB ? e : 0);
      __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(dst + ch * 256), 16,
                                       0, 0);
    }
  };
  stage(kl, rec + (kl & 1) * RING);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int k = kl; k >= 0; --k) {
    const int cur = k & 1;
    const int k1 = k >= 1 ? k - 1 : 0;
    stage(k1, rec + (cur ^ 1) * RING);               // slot cur ^ 1 was last read before the previous barrier
    floatx4 a[G], za[G], zb[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      a[g] = hp_n[g];                                // Linear 1 accumulator: condition projection + b1 (k_hp)
      hp_n[g] = hpl[g][k1 * hps4];
      za[g] = floatx4{0.f, 0.f, 0.f, 0.f};
      zb[g] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    const float* slot = rec + cur * RING;
    // z @ Q^T (cnf.py:339): quadrants [a->a | b->a | a->b | b->b]; identity for the last block
    inv_mv_mo<G, KA>(za, slot, l, ya);                // quadrant 0: a -> a
    inv_mv_mo<G, KA>(zb, slot + 2 * 256, l, ya);      // quadrant 2: a -> b
    inv_mv_mo<G, KA>(za, slot + 1 * 256, l, yb);      // quadrant 1: b -> a
    inv_mv_mo<G, KA>(zb, slot + 3 * 256, l, yb);      // quadrant 3: b -> b
    // nested MLP (cnf.py:98-107): Linear 1 on za, then the hidden layers
    inv_mv_mo<G, KA>(a, slot + 4 * 256, l, za);
#pragma unroll
    for (int g = 0; g < G; ++g) gelu4(a[g]);
#pragma unroll
    for (int h = 2; h <= NH; ++h) {
      const floatx4 bias = *reinterpret_cast<const floatx4*>(slot + BIAS + 16 * (h - 2) + 4 * q);
      floatx4 x[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        x[g] = a[g];
        a[g] = bias;
      }
      inv_mv_mo<G, 4>(a, slot + (5 + h - 2) * 256, l, x);
#pragma unroll
      for (int g = 0; g < G; ++g) gelu4(a[g]);
    }
    floatx4 T[G], Sp[G];
    const floatx4 tb = *reinterpret_cast<const floatx4*>(slot + TSB + 4 * q);
    const floatx4 sb = *reinterpret_cast<const floatx4*>(slot + TSB + 16 + 4 * q);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      T[g] = tb;
      Sp[g] = sb;
    }
    inv_mv_mo<G, 4>(T, slot + (NH + 4) * 256, l, a);
    inv_mv_mo<G, 4>(Sp, slot + (NH + 5) * 256, l, a);
#pragma unroll
    for (int r = 0; r < (PERM ? 3 : 4); ++r) {
      const int f = feat(r);
      const floatx4 an = *reinterpret_cast<const floatx4*>(slot + ANB + 16 * q + 4 * r);   // [1/sa ba 1/sb bb]
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float S = tanh_bf(Sp[g][r]);
        const float ybn = (zb[g][r] - T[g][r]) * exp_fast(-S);                    // cnf.py:205
        if (LDJ) ls[g] += (f < Db) ? S : 0.f;                                      // cnf.py:190 at the returned y
        ya[g][r] = (f < Da) ? (za[g][r] - an[1]) * an[0] : 0.f;                    // ActNorm inverse (cnf.py:353-354)
        yb[g][r] = (f < Db) ? (ybn - an[3]) * an[2] : 0.f;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next record has landed in LDS
    __syncthreads();
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (b[g] < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = feat(r);
        if (f < Da) yout[b[g] * D + f] = ya[g][r];
        if (f < Db) yout[b[g] * D + Da + f] = yb[g][r];
      }
    }
  }
  if (LDJ) {
    const float ldc = pk[L.ldc_off];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float ltot = sum_rows4(ls[g]) + ldc;
      if (q == 0 && b[g] < N) {
        ldj_out[b[g]] = ltot;
        if (logp_out) logp_out[b[g]] += ltot;
      }
    }
  }
}

}  // namespace

namespace bcnf_small {

int launch_hp(const BcnfLayout& L, const float* pk, const float* h, long long R, float* hp, hipStream_t st) {
  const size_t lds = hp_lds_bytes();
  const dim3 grid((unsigned)((R + 63) / 64), (unsigned)(L.NKp / 64));
  return vec_rows(L, h) ? launch<k_hp<true>>(grid, dim3(BCNF_WG), lds, st, L, pk, h, R, hp)
                        : launch<k_hp<false>>(grid, dim3(BCNF_WG), lds, st, L, pk, h, R, hp);
}

// Eval: the matrix cores (every layout that passes layout_matches has their record); training: the drawing inverse.
int launch_inverse(const BcnfLayout& L, const float* pk, const float* z, const float* hp, long long R,
                   const int64_t* ci, long long N, float* y, bool drop, const uint64_t* rng, hipStream_t st) {
  return dispatch_nh(L.NH, [&](auto nh) -> int {
    constexpr int NH = decltype(nh)::value;
    if (!layout_matches<NH>(L)) return BCNF_ERR_ARG;
    if (drop)
      return launch<k_inverse<NH>>(dim3((unsigned)((N + 15) / 16)), dim3(BCNF_WG), INV_LDS_BYTES, st, L, pk, z, hp, R,
                                   ci, N, y, rng);
    const dim3 grid_m((unsigned)((N + INV_M_SPB - 1) / INV_M_SPB));
    float* const none = nullptr;   // no ldj / log_prob outputs
    return L.Da <= 12 && L.Db <= 12
               ? launch<k_inverse_mfma<NH, true>>(grid_m, dim3(INV_M_WG), INV_LDS_BYTES, st, L, pk, z, hp, R, ci, N, y, none, none)
               : launch<k_inverse_mfma<NH, false>>(grid_m, dim3(INV_M_WG), INV_LDS_BYTES, st, L, pk, z, hp, R, ci, N, y, none, none);
  });
}

// The eval inverse that also returns the forward's log|det J| at y (and log_prob).
int launch_inverse_logdet(const BcnfLayout& L, const float* pk, const float* z, const float* hp, long long R,
                          const int64_t* ci, long long N, float* y, float* ldj, float* logp, hipStream_t st) {
  return dispatch_nh(L.NH, [&](auto nh) -> int {
    constexpr int NH = decltype(nh)::value;
    if (!layout_matches<NH>(L)) return BCNF_ERR_ARG;
    const dim3 grid_m((unsigned)((N + INV_M_SPB - 1) / INV_M_SPB));
    return L.Da <= 12 && L.Db <= 12
               ? launch<k_inverse_mfma<NH, true, true>>(grid_m, dim3(INV_M_WG), INV_LDS_BYTES, st, L, pk, z, hp, R, ci, N, y, ldj, logp)
               : launch<k_inverse_mfma<NH, false, true>>(grid_m, dim3(INV_M_WG), INV_LDS_BYTES, st, L, pk, z, hp, R, ci, N, y, ldj, logp);
  });
}

}  // namespace bcnf_small
