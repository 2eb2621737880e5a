// Small stack family (bcnf_stack*.hip): the device vocabulary the stack kernels share -- the compile-time mirrors of
// the record layouts (RecF / RecB / ActRec) with the host's check of them, record staging and reads, the nested MLP
// on the row layout, the mix, the NLL finalize, sum_rows4 and the row loader of the projection GEMMs (load_rows64).
#pragma once
#include "bcnf_stack_layout.h"

// Phase stamps (s_memtime per phase of workgroup 0's first compute and helper waves) exist only in a diagnostic
// build with -DBCNF_PHASE_STAMPS (tools/exp_variants.sh); the shipped library has no stamp code, no debug globals
// and no debug exports.
#ifdef BCNF_PHASE_STAMPS
#define BCNF_STAMPS 1
#else
#define BCNF_STAMPS 0
#endif
#define QBC_DEV(L, bit) (((L).qbc & (bit)) != 0)   // the kernels' test of a section's form (QBC_*)

#pragma GCC visibility push(hidden)
namespace bcnf_small {

// Cooperative copy of n floats (multiple of 4) global -> registers (phase 1) -> LDS (phase 2), so the
// global latency of the NEXT block's data hides under the current block's compute.
template <int N>
struct Stage {
  floatx4 r[N];
  __device__ __forceinline__ void load(const float* __restrict__ g, int n) { load_t(g, n, (int)threadIdx.x); }
  // all N float4 per thread, no bounds branch: the destination is a RING-sized slot
  __device__ __forceinline__ void store(float* __restrict__ s) const { store_t(s, (int)threadIdx.x); }
  // the same for thread t of a 256-thread role inside a larger workgroup
  __device__ __forceinline__ void load_t(const float* __restrict__ g, int n, int t) {
    const floatx4* g4 = reinterpret_cast<const floatx4*>(g);
    const int n4 = n >> 2;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int idx = t + i * BCNF_WG;
      r[i] = g4[idx < n4 ? idx : 0];   // unconditional (clamped) so r[] stays in VGPRs
    }
  }
  __device__ __forceinline__ void store_t(float* __restrict__ s, int t) const {
    floatx4* s4 = reinterpret_cast<floatx4*>(s);
#pragma unroll
    for (int i = 0; i < N; ++i) s4[t + i * BCNF_WG] = r[i];
  }
  // mapped form: float4 ix[i] of the source to float4 ix[i] of the slot (a record staged without its dead quads)
  __device__ __forceinline__ void load_ix(const float* __restrict__ g, const int* ix) {
    const floatx4* g4 = reinterpret_cast<const floatx4*>(g);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = g4[ix[i]];
  }
  __device__ __forceinline__ void store_ix(float* __restrict__ s, const int* ix) const {
    floatx4* s4 = reinterpret_cast<floatx4*>(s);
#pragma unroll
    for (int i = 0; i < N; ++i) s4[ix[i]] = r[i];
  }
};

// Stage rows [r0, r0 + 64) x cols [c0, c0 + KC) of a row-major (nrows x ncols, ld) matrix into regs
// (8 float4 per thread: row = i4 / 32, col = 4 (i4 % 32)), zero outside; column `ones` (>= ncols, or -1 for
// none) of every valid row reads 1.0 (the bias column of the folded feature Linear).
template <bool VEC>
__device__ __forceinline__ void load_rows64(const float* __restrict__ M, long long nrows, int ncols, long long ld,
                                            long long r0, int c0, floatx4* reg, int ones = -1) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int i4 = threadIdx.x + 256 * e, row = i4 >> 5, col = c0 + (i4 & 31) * 4;
    const long long r = r0 + row < nrows ? r0 + row : nrows - 1;
    if (VEC) {
      const floatx4 v = *reinterpret_cast<const floatx4*>(M + r * ld + (col < ncols ? col : 0));
#pragma unroll
      for (int q = 0; q < 4; ++q) reg[e][q] = (r0 + row < nrows && col + q < ncols) ? v[q] : 0.f;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cq = col + q;
        const float v = M[r * ld + (cq < ncols ? cq : ncols - 1)];
        reg[e][q] = (r0 + row < nrows && cq < ncols) ? v : 0.f;
      }
    }
    if (ones >= 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (col + q == ones && r0 + row < nrows) reg[e][q] = 1.f;
    }
  }
}

// Compile-time mirror of the forward / backward record layouts of make_layout (checked on the host).
// A broadcast-form section (QBC_*: bc10, mix_bc, bc9x2) keeps its rotation-form size and offset -- the record sizes
// of the D = 19 stacks are pinned (tests/test_small_arms_cpu.py) -- and its live words are the section's first ones:
// 10 of W1's 16, 38 of Q's 64, 9 of each head transpose's 16. The words past them are dead: k_forward and k_backward
// (BC = all three bits, the only non-zero value make_layout gives) read none of them, k_backward stages none.
// A section's last live words are read with a ds_read_b64 / _b32, not as part of a quad: a quad whose upper words
// nobody uses gets registers the allocator hands to the next read at once, and that read then waits for it.
constexpr int BC_W1 = 10, BC_Q = 38, BC_HEAD = 9;    // live floats of a broadcast section
__host__ __device__ constexpr int quads(int n) { return (n + 3) / 4; }
template <int NH>
struct RecF {
  static constexpr int B1 = 4, W1 = 8, HID = 24, T = 24 + 17 * (NH - 1), S = T + 17;
  static constexpr int Q = (S + 17 + 3) & ~3, MLP_END = (S + 17 + 3) & ~3, USED = Q + 64;
  __host__ __device__ static constexpr int head_end(bool bc) { return bc ? W1 + BC_W1 : HID; }   // of [0, HID)
  __host__ __device__ static constexpr int live_end(bool bc) { return bc ? Q + BC_Q : USED; }
};
template <int NH>
struct RecB {   // consumption order (make_layout): ActNorm, Q^T, T / S heads, hidden l = NH .. 2, W1^T
  static constexpr int AN = 0, QT = 4, TT = 68, ST = 84, HID = 100, W1T = 100 + 16 * (NH - 1);
  static constexpr int USED = W1T + 16;
  __host__ __device__ static constexpr int qt_end(bool bc) { return bc ? QT + BC_Q : TT; }
  __host__ __device__ static constexpr int head_len(bool bc) { return bc ? BC_HEAD : 16; }
  // the quads of a lane's record that hold a live word, in order: live_quad(c), c < live_quads(bc)
  __host__ __device__ static constexpr int live_quads(bool bc) {
    return bc ? quads(qt_end(true)) + 2 * quads(BC_HEAD) + (USED - HID) / 4 : USED / 4;
  }
  __host__ __device__ static constexpr int live_quad(bool bc, int c) {
    if (!bc) return c;
    const int nq = quads(qt_end(true)), nh = quads(BC_HEAD);
    return c < nq ? c : c < nq + nh ? TT / 4 + (c - nq) : c < nq + 2 * nh ? ST / 4 + (c - nq - nh)
                                                                        : HID / 4 + (c - nq - 2 * nh);
  }
  __host__ __device__ static constexpr int dead_quad() { return quads(qt_end(true)); }   // all of it dead under BC
};
// Activation record a training forward saves per (block, sample, lane) for the backward, so the backward never
// recomputes the MLP: masked activations, masked GELU derivatives, tanh(s) and the block input, 2 NH + 3 floats
// stored as AR4 float4 [k][workgroup][AR4][256 threads] plus AR1 floats [k][workgroup][AR1][256] (no padding).
// Order (r05): (activation, derivative) of hidden layer 1, 2, ..., then y_a, y_b, tanh(s) -- a float4 is complete
// every two layers and the forward stores it there (ready_layer), spread over the block. Measured: the
// record writes cost k_forward ~7 us (an ablation without them: 57 -> 50 us), the same whether the stores go out in
// one burst after the coupling, spread like this, or from the helper waves through LDS -- the cost is the 132 MB of
// writes in the memory system, not the issuing wave.
template <int NH>
struct ActRec {
  static constexpr int YA = 2 * NH, YB = 2 * NH + 1, S = 2 * NH + 2;
  static constexpr int AR = 2 * NH + 3, AR4 = AR / 4, AR1 = AR - 4 * AR4;
  __host__ __device__ static constexpr int act(int l) { return 2 * l; }   // hidden layer l + 1
  __host__ __device__ static constexpr int gd(int l) { return 2 * l + 1; }
  // the hidden layer (1-based) after which float4 q is complete; NH + 1: only after tanh(s)
  __host__ __device__ static constexpr int ready_layer(int q) {
    int r = 0;
    for (int i = 4 * q; i < 4 * q + 4; ++i) {
      const int li = i < 2 * NH ? i / 2 + 1 : (i == S ? NH + 1 : 0);
      r = li > r ? li : r;
    }
    return r;
  }
};

// Burst-load floats [lo, hi) of this lane's LDS record into registers (compile-time indices, so the
// array lives in VGPRs): one LDS wait per block instead of one per layer.
// The n < 4 floats at e (a multiple of 4) that end a slice: one 8-byte and / or one 4-byte read.
template <int N>
__device__ __forceinline__ void ld_rec_tail(float* __restrict__ rr, const float* __restrict__ R, int e) {
  static_assert(N >= 0 && N < 4, "less than a quad");
  if (N >= 2) {
    const floatx2 v = *reinterpret_cast<const floatx2*>(R + e);
    rr[e] = v.x;
    rr[e + 1] = v.y;
  }
  if (N & 1) rr[e + (N & 2)] = R[e + (N & 2)];
}
template <int LO, int HI>
__device__ __forceinline__ void ld_rec(float* __restrict__ rr, const float* __restrict__ R) {
  static_assert(LO % 4 == 0 && HI >= LO, "record slices start 16-B aligned");
  const floatx4* R4 = reinterpret_cast<const floatx4*>(R + LO);
#pragma unroll
  for (int i = 0; i < (HI - LO) / 4; ++i) {
    const floatx4 v = R4[i];
    rr[LO + 4 * i + 0] = v.x;
    rr[LO + 4 * i + 1] = v.y;
    rr[LO + 4 * i + 2] = v.z;
    rr[LO + 4 * i + 3] = v.w;
  }
  ld_rec_tail<(HI - LO) % 4>(rr, R, LO + (HI - LO) / 4 * 4);
}

// Nested MLP forward on the row layout (cnf.py:98-107) from a register-resident forward record.
// Input x (layer-1 y-part operand) and hp (its condition part + bias, from k_hp); returns t and s'
// (pre-tanh). Dropout bit l - 1 of `bits` keeps hidden layer l (k_inverse, the only caller, always draws).
template <int NH>
__device__ __forceinline__ void mlp_forward(const BcnfLayout& L, const float* __restrict__ rr, float x, float hp,
                                            uint32_t bits, float& T, float& Sp) {
  using F = RecF<NH>;
  float a = x;
#pragma unroll
  for (int l = 1; l <= NH; ++l) {
    const float* w = (l == 1) ? rr + F::W1 : rr + F::HID + 17 * (l - 2);
    const float bias = (l == 1) ? hp : w[16];            // hp = h W1h^T + b1 (k_hp)
    const float pre = (l == 1 && QBC_DEV(L, QBC_W1)) ? bc10(a, w, bias) : rot16(a, w, bias);   // (uniform)
    const float m = ((bits >> (l - 1)) & 1u) ? L.keep_scale : 0.f;
    a = gelu_f(pre) * m;
  }
  T = rr[F::T + 16];
  Sp = rr[F::S + 16];
  rot16x2(a, rr + F::T, T, a, rr + F::S, Sp);
}

// Streamed form for k_forward's compute waves (r05), with the dropout multipliers as floats (msk[l - 1] = keep_scale
// or 0 for hidden layer l, drawn by k_forward's helper waves: no bit extraction on the compute wave's chain).
// The record is read in consumption order: before stage l (hidden
// layer l = 1..NH, then NH + 1 = the T / S heads, NH + 2 = the mix) the wave issues the quads stage l + FWD_AHEAD
// ends in, behind a scheduling barrier, so each lgkmcnt wait covers reads issued two layers earlier. (r04's
// burst form ld_rec<FWD_HEAD, USED> let hipcc issue 17 reads after layer 1 and wait for all of them at once, then
// 4 and 8 more each with a wait one GELU later: five exposed LDS round trips per block under four waves' load.)
constexpr int FWD_AHEAD = 2;
template <int NH, bool BC>
__host__ __device__ constexpr int rf_stage_end(int l) {   // exclusive end (floats) of what stage l reads
  return l <= NH ? 24 + 17 * (l - 1) : (l == NH + 1 ? RecF<NH>::S + 17 : RecF<NH>::live_end(BC));
}
template <int NH, bool BC>
__host__ __device__ constexpr int rf_stage_q(int l) {     // quads issued once stage l's reads are out
  // at most 8 new quads per stage (lgkmcnt tracks 15 outstanding: a 16-read burst at the last layer made hipcc wait
  // for its oldest reads at once); whatever the cap defers goes out with the next stage, all of it by the mix
  int q = 6;
  for (int i = 1; i <= l; ++i) {
    const int want = (rf_stage_end<NH, BC>(i + FWD_AHEAD < NH + 2 ? i + FWD_AHEAD : NH + 2) + 3) / 4;
    q = i >= NH + 2 ? want : (want < q + 8 ? want : q + 8);
  }
  return q;
}
template <int NH, bool BC>
__device__ __forceinline__ void rf_issue(float* __restrict__ rr, const float* __restrict__ R, int l) {
  const floatx4* R4 = reinterpret_cast<const floatx4*>(R);
#pragma unroll
  for (int q = rf_stage_q<NH, BC>(l - 1); q < rf_stage_q<NH, BC>(l); ++q) {
    if (4 * q + 4 > RecF<NH>::live_end(BC)) {           // (BC: the mix section's last two live words)
      ld_rec_tail<RecF<NH>::live_end(BC) % 4>(rr, R, 4 * q);
      continue;
    }
    const floatx4 v = R4[q];
    rr[4 * q] = v.x;
    rr[4 * q + 1] = v.y;
    rr[4 * q + 2] = v.z;
    rr[4 * q + 3] = v.w;
  }
  __builtin_amdgcn_sched_barrier(0);
}
// KEEP: the activation record goes to ar (ActRec order), and emit(q) is called right after float4 q is complete.
// BC: the broadcast form (Linear 1 here), whose dead words no stage reads (rf_stage_end, RecF::head_end).
template <int NH, bool KEEP, bool DROP, bool BC, typename Emit>
__device__ __forceinline__ void mlp_forward_s(float* __restrict__ rr, const float* __restrict__ R, float x, float hp,
                                              const float* __restrict__ msk, float& T, float& Sp, float* ar,
                                              Emit&& emit) {
  static_assert(RecF<NH>::HID == 24, "stage 1 reads only the prefetched head (FWD_HEAD = 24)");
  using F = RecF<NH>;
  using AR = ActRec<NH>;
  float a = x;
#pragma unroll
  for (int l = 1; l <= NH; ++l) {
    rf_issue<NH, BC>(rr, R, l);
    const float* w = (l == 1) ? rr + F::W1 : rr + F::HID + 17 * (l - 2);
    const float pre = (l == 1 && BC) ? bc10(a, w, hp) : rot16(a, w, (l == 1) ? hp : w[16]);
    if (KEEP) {
      float g, dg;
      gelu_fg(pre, g, dg);
      a = DROP ? g * msk[l - 1] : g;
      ar[AR::act(l - 1)] = a;
      ar[AR::gd(l - 1)] = DROP ? dg * msk[l - 1] : dg;
#pragma unroll
      for (int q = 0; q < AR::AR4; ++q)
        if (AR::ready_layer(q) == l) emit(q);
    } else if (DROP) {
      // training forward that saves nothing (under no_grad): the saving forward's GELU form, not the forward-only
      // polynomial, so at one (seed, offset) z and log|det J| are the same bits whether or not autograd records
      float g, dg;
      gelu_fg(pre, g, dg);
      a = g * msk[l - 1];
    } else {
      a = gelu_f(pre);
    }
  }
  rf_issue<NH, BC>(rr, R, NH + 1);
  T = rr[F::T + 16];
  Sp = rr[F::S + 16];
  rot16x2(a, rr + F::T, T, a, rr + F::S, Sp);
  rf_issue<NH, BC>(rr, R, NH + 2);   // (empty: the mix's quads went out with stage NH)
}

// Row-layout orthonormal mix: (na, nb) = (a, b) @ M with the four pre-rotated quadrants at rq
// (register-resident): [a->a | b->a | a->b | b->b].
__device__ __forceinline__ void mix(const float* __restrict__ rq, float a, float b, float& na, float& nbv) {
  na = 0.f;
  nbv = 0.f;
  rot16x2(a, rq, na, a, rq + 32, nbv);
  rot16x2(b, rq + 16, na, b, rq + 48, nbv);
}

// Mean of the forward's per-workgroup NLL partials -> loss_out = [loss, nll, mse = 0] (trainer.py:260-266)
// and the dropout RNG offset advance, by ONE workgroup that runs strictly after the forward (a separate
// launch, or workgroup 0 of the backward): no cross-workgroup synchronisation inside any kernel.
// Divergence guard (int32[4], BCNF_GUARD_*): a step whose loss exceeds 1e5 or is NaN while checking is
// enabled raises `diverged` (trainer.py:168 raises after that step's update); the NEXT step's finalize
// then raises `halted`, which turns that step's RNG advance, Adam update, clip and counter advances into
// no-ops -- so an epoch replayed without host syncs stops with the state the reference raises in.
// (static: not __forceinline__, so each translation unit keeps an internal copy that its inliner may fold away)
template <int NTH = BCNF_WG>
static __device__ void nll_finalize(const float* __restrict__ part, int nparts, long long B, float* __restrict__ loss_out,
                             uint64_t* rng_w, int32_t* guard, float* __restrict__ red) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += NTH) acc += part[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = NTH / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float nll = red[0] / (float)B;
    loss_out[0] = nll;                                 // (nll + mse * 0) / (1 + 0)   (trainer.py:264)
    loss_out[1] = nll;
    loss_out[2] = 0.f;
    bool halt = false;
    if (guard) {
      if (guard[BCNF_GUARD_DIVERGED]) {
        guard[BCNF_GUARD_HALTED] = 1;
        halt = true;
      } else if (guard[BCNF_GUARD_CHECK] && (nll > 1e5f || isnan(nll))) {
        guard[BCNF_GUARD_DIVERGED] = 1;
      }
    }
    if (rng_w && !halt) rng_w[1] += 1;                 // the forward has read the offset
  }
}

// Sum of v over the 4 rows (16-lane groups) of the wave, returned in every lane (gfx950 permlane swaps:
// the two results of each swap are the row pairs, so adding them is the pairwise sum whatever the order).
__device__ __forceinline__ float sum_rows4(float v) {
  const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(p[0]) + __uint_as_float(p[1]);
  const auto p2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(p2[0]) + __uint_as_float(p2[1]);
}

// Does the host layout agree with the kernels' compile-time offsets? Every dispatch asks first (BCNF_ERR_ARG if
// not). RF and PMB are what make_layout derives from these offsets: k_inverse_mfma addresses its records with them.
template <int NH>
constexpr int inv_m_rf() { return round_rec(RecF<NH>::USED); }
template <int NH>
bool layout_matches(const BcnfLayout& L) {
  return L.rf_b1 == RecF<NH>::B1 && L.rf_w1 == RecF<NH>::W1 && L.rf_hid == RecF<NH>::HID && L.rf_t == RecF<NH>::T &&
         L.rf_s == RecF<NH>::S && L.rf_q == RecF<NH>::Q && L.RF == inv_m_rf<NH>() &&
         L.PMB == (NH + 6) * 256 + (NH - 1) * 16 + 96 && L.rb_w1t == RecB<NH>::W1T &&
         L.rb_hid == RecB<NH>::HID && L.rb_tt == RecB<NH>::TT && L.rb_st == RecB<NH>::ST && L.rb_qt == RecB<NH>::QT &&
         L.rb_an == RecB<NH>::AN && L.RB >= RecB<NH>::USED && (L.qbc == 0 || L.qbc == (QBC_W1 | QBC_MIX | QBC_HEAD));
}
// The record form k_forward and k_backward are instantiated for (BC): every section in broadcast form, or none.
inline bool layout_bc(const BcnfLayout& L) { return L.qbc == (QBC_W1 | QBC_MIX | QBC_HEAD); }

}  // namespace bcnf_small
#pragma GCC visibility pop
