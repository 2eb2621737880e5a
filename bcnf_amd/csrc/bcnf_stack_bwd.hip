// bcnf_amd small stack family: the whole-stack backward (k_backward): per-block back-propagation on the row layout,
// dW on fp32 MFMA into per-workgroup gradient slabs, which bcnf_stack_tail.hip reduces. The family's files:
// bcnf_stack_internal.h.
#include "bcnf_stack_internal.h"
#include "bcnf_stack_rec.h"

namespace {
using namespace bcnf_small;
using bcnf_rt::launch;

#if BCNF_STAMPS
__device__ unsigned long long g_phase[32];   // phase stamps (bcnf_debug_phases), diagnostic build only
#endif

// Backward LDS tiles ([16 samples][17] each): the compute waves' delta tiles of a block, [D_1 .. D_NH, D_T, D_S, PA,
// GA, PB, GB] (2 slots), and the helper waves' activation tiles A_0 .. A_NH (A_0 = ActNorm output of the y-part,
// A_l = masked GELU output of hidden layer l; 3 slots, since they are built one block ahead of the compute waves).
template <int NH>
struct BwdJobs {
  static constexpr int ND = NH + 6, NA = NH + 1;
  static constexpr int NW = NH + 2, NS = NH + 6;
  static constexpr int SUM_OFF = NW * 256;                 // slab block: [NW][64 lanes][4] then [NS][16]
  static constexpr int BLK = NW * 256 + NS * 16;
  // W job c = dW of Linear c + 1 (c = NH, NH + 1: the last Linear's t / s row halves): delta tile c x act tile wb(c)
  __device__ static constexpr int wb(int c) { return c < NH ? c : NH; }
  // sum job c = column sum of delta tile c (biases of Linear 1 .. NH, t / s halves, then ActNorm PA, GA, PB, GB)
};

// Helper-wave gradient jobs of block m, from its delta tiles Td and activation tiles Ta, straight to slab block m
// (no LDS gradient block):
//   W job c: 16 x 16 fp32-MFMA tile over the workgroup's 16 samples, out[i][j] = sum_s delta[s][i] act[s][j]; lane l
//            holds D[4(l>>4) + r][l & 15], r = 0..3, stored as ONE float4 at [c][l] (1 KB per wave, coalesced)
//            (Linear 1: only its y-part columns; the condition part is the split-K GEMM of the tail)
//   sum job c: 16 column sums at SUM_OFF + 16 c (lanes 0..15)
// The slab layout is decoded by slab_to_canonical. The MFMA tiles are written through (sc1), like the forward's
// records: k_fold_tail reads them from memory anyway.
template <int NH>
__device__ __forceinline__ void bwd_grad_jobs(const float* __restrict__ Td, const float* __restrict__ Ta,
                                              float* __restrict__ out, int hw) {
  using J = BwdJobs<NH>;
  const int l64 = threadIdx.x & 63, q = l64 >> 4, r = l64 & 15;
  constexpr int UW = (J::NW + 3) / 4, US = (J::NS + 3) / 4;
  floatx4 a[UW], bv[UW], v[US];                            // lane (q, r): samples 4 t + q of column r, t = 0..3
  const int o = 4 * tile_slot(r, q);
#pragma unroll
  for (int u = 0; u < UW; ++u) {                           // all operand reads first
    const int c = hw + 4 * u < J::NW ? hw + 4 * u : J::NW - 1;
    a[u] = *reinterpret_cast<const floatx4*>(Td + c * TILE + o);
    bv[u] = *reinterpret_cast<const floatx4*>(Ta + J::wb(c) * TILE + o);
  }
#pragma unroll
  for (int u = 0; u < US; ++u) {
    const int c = hw + 4 * u < J::NS ? hw + 4 * u : J::NS - 1;
    v[u] = *reinterpret_cast<const floatx4*>(Td + c * TILE + o);
  }
  floatx4 acc[UW];
#pragma unroll
  for (int u = 0; u < UW; ++u) acc[u] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t)                              // independent chains interleaved
#pragma unroll
    for (int u = 0; u < UW; ++u) acc[u] = mfma4(a[u][t], bv[u][t], acc[u]);
#pragma unroll
  for (int u = 0; u < US; ++u) {
    const float tot = sum_rows4((v[u][0] + v[u][1]) + (v[u][2] + v[u][3]));
    if (hw + 4 * u < J::NS && q == 0) out[J::SUM_OFF + 16 * (hw + 4 * u) + r] = tot;
  }
#pragma unroll
  for (int u = 0; u < UW; ++u)
    if (hw + 4 * u < J::NW) st4_wt_mfma(reinterpret_cast<floatx4*>(out + 256 * (hw + 4 * u)) + l64, acc[u]);
}

// Whole-stack backward, one launch, 512 threads = two roles per SIMD (waves w and w + 4 share a SIMD):
//  * compute waves 0..3 (4 samples each, row layout): back-propagate block k (VALU, DPP rotations) from its
//    backward record and its masked GELU derivatives (LDS), writing block k's delta tiles;
//  * helper waves 4..7, in the same interval: the MFMA / column-sum gradient jobs of block k+1 (tiles of the
//    previous interval) straight to the slab, and block k-1's inputs -- its activation record (loaded one interval
//    earlier) split into activation tiles and the compute waves' derivative slot, its backward record staged into
//    the LDS ring.
// One barrier per block; the compute waves issue no global loads.
constexpr int BWD_WG = 2 * BCNF_WG;
constexpr int BWD_G4 = 3;                // float4 per thread of the derivative slot: gd[NH], S, ya, yb (NH <= 9)

// BC: a D = 19 stack, whose Q^T and T / S head sections are in broadcast form (L.qbc): the compute waves read only
// the live words of those sections (47 LDS reads per block instead of 56), and the helpers stage only the record's live
// quads (RecB::live_quad: 3 float4 per thread at NH = 7, where the whole record takes STAGE_REC = 4); the dead words
// of the LDS ring keep whatever they held.
template <int NH, bool BC>
__global__ __launch_bounds__(BWD_WG) void k_backward(BcnfLayout L, const float* __restrict__ pk,
                                                     const float* __restrict__ dz, const float* __restrict__ dldj,
                                                     const float* __restrict__ dloss, int nll, long long B,
                                                     const float* __restrict__ arec,
                                                     float* __restrict__ dy, float* __restrict__ d1,
                                                     float* __restrict__ slab_all, long long slab_stride,
                                                     const float* __restrict__ nll_part, float* __restrict__ loss_out,
                                                     uint64_t* rng_w, int32_t* guard) {
  static_assert(NH + 3 <= 4 * BWD_G4, "derivative slot");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using AR = ActRec<NH>;
  using RBk = RecB<NH>;
  using J = BwdJobs<NH>;
  const int RBL = 16 * L.RB;
  float* recB = smem;                                   // [2][16*RB]
  float* dT = recB + 2 * RING;                          // [2][ND][TILE]
  float* aT = dT + 2 * J::ND * TILE;                    // [3][NA][TILE]
  floatx4* gsl = reinterpret_cast<floatx4*>(aT + 3 * J::NA * TILE);   // [2][BWD_G4][256]
  const int nb = L.nb;
  const float* pbk = pk + L.pb_off;
  const bool helper = threadIdx.x >= BCNF_WG;
  const int t8 = (int)threadIdx.x & (BCNF_WG - 1);
  const int j = t8 & 15, s = sample_of(t8);
  const int tix = tile_ix(s, j);
  // diagnostic build: per-phase cycles of workgroup 0's wave 0 (compute) and wave 4 (helper) -> g_phase
  unsigned long long ph_t = BCNF_STAMPS ? __builtin_amdgcn_s_memtime() : 0ULL, ph_acc[4] = {0, 0, 0, 0};
#define PHS(i)                                                                                   \
  if (BCNF_STAMPS) {                                                                             \
    const unsigned long long _t = __builtin_amdgcn_s_memtime();                                  \
    ph_acc[i] += _t - ph_t;                                                                      \
    ph_t = _t;                                                                                   \
  }

  if (helper) {
    const int hw = __builtin_amdgcn_readfirstlane(t8 >> 6);
    float* slab = slab_all + (long long)blockIdx.x * slab_stride;
    // activation records [k][workgroup][AR/4][256 threads] float4 (k_forward)
    const floatx4* arl = reinterpret_cast<const floatx4*>(arec) + (long long)blockIdx.x * AR::AR4 * BCNF_WG + t8;
    const long long ars = (long long)gridDim.x * AR::AR4 * BCNF_WG;
    // float4 of the record this thread stages: n-th live quad (n = t8 + 256 i) = live quad n % LQ of lane n / LQ; a
    // slot past the last one copies a dead quad of lane 0 onto itself. (NH = 8: the live quads take 4 float4 per
    // thread as well, so the record is staged whole.)
    constexpr int LQ = RBk::live_quads(BC), LSTAGE = (16 * LQ + BCNF_WG - 1) / BCNF_WG;
    constexpr bool MAPPED = BC && LSTAGE < STAGE_REC;
    constexpr int BSTAGE = MAPPED ? LSTAGE : STAGE_REC;
    int six[BSTAGE];
    if constexpr (MAPPED) {
      const int rb4 = L.RB >> 2;
#pragma unroll
      for (int i = 0; i < BSTAGE; ++i) {
        const int n = t8 + i * BCNF_WG, lane = n / LQ, c = n - lane * LQ;
        six[i] = n < 16 * LQ ? lane * rb4 + RBk::live_quad(true, c) : RBk::dead_quad();
      }
    }
    struct Prep {
      Stage<BSTAGE> sr;
      floatx4 rec[AR::AR4];
      float rec1[AR::AR1 > 0 ? AR::AR1 : 1];
      float sa, ba;
    };
    const float* ar1l = arec + ar1_off(nb, gridDim.x, AR::AR4) + (long long)blockIdx.x * AR::AR1 * BCNF_WG + t8;
    const long long ar1s = (long long)gridDim.x * AR::AR1 * BCNF_WG;
    auto prep_load = [&](Prep& P, int k) {                  // block k's inputs: HBM / L2 -> registers
      if constexpr (MAPPED) P.sr.load_ix(pbk + (long long)k * RBL, six);
      else P.sr.load_t(pbk + (long long)k * RBL, RBL, t8);
#pragma unroll
      for (int i = 0; i < AR::AR4; ++i) P.rec[i] = arl[(long long)k * ars + i * BCNF_WG];
#pragma unroll
      for (int i = 0; i < AR::AR1; ++i) P.rec1[i] = ar1l[(long long)k * ar1s + i * BCNF_WG];
      const float* an = pbk + (long long)k * RBL + j * L.RB + RBk::AN;
      P.sa = an[0];
      P.ba = an[1];
    };
    auto prep_store = [&](Prep& P, int k) {                 // registers -> LDS slots of block k
      // every loaded register stays live until here: a register the compiler reallocated while its load is in
      // flight would cost a wait for that load
#pragma unroll
      for (int i = 0; i < AR::AR4; ++i) asm volatile("" : "+v"(P.rec[i]));
#pragma unroll
      for (int i = 0; i < AR::AR1; ++i) asm volatile("" : "+v"(P.rec1[i]));
      asm volatile("" : "+v"(P.sa), "+v"(P.ba));
      float ar[4 * AR::AR4 + AR::AR1];
#pragma unroll
      for (int i = 0; i < AR::AR4; ++i) {
        ar[4 * i] = P.rec[i][0];
        ar[4 * i + 1] = P.rec[i][1];
        ar[4 * i + 2] = P.rec[i][2];
        ar[4 * i + 3] = P.rec[i][3];
      }
#pragma unroll
      for (int i = 0; i < AR::AR1; ++i) ar[4 * AR::AR4 + i] = P.rec1[i];
      float* ta = aT + (k % 3) * J::NA * TILE + tix;
#pragma unroll
      for (int l = 1; l <= NH; ++l) ta[l * TILE] = ar[AR::act(l - 1)];
      ta[0] = fmaf(P.sa, ar[AR::YA], P.ba);                // A_0: ActNorm output of the y-part (cnf.py:349)
      float gs[4 * BWD_G4];
#pragma unroll
      for (int l = 0; l < NH; ++l) gs[l] = ar[AR::gd(l)];
      gs[NH] = ar[AR::S];
      gs[NH + 1] = ar[AR::YA];
      gs[NH + 2] = ar[AR::YB];
#pragma unroll
      for (int i = NH + 3; i < 4 * BWD_G4; ++i) gs[i] = 0.f;
      floatx4* gd = gsl + (k & 1) * BWD_G4 * BCNF_WG + t8;
#pragma unroll
      for (int i = 0; i < BWD_G4; ++i) gd[i * BCNF_WG] = floatx4{gs[4 * i], gs[4 * i + 1], gs[4 * i + 2], gs[4 * i + 3]};
      if constexpr (MAPPED) P.sr.store_ix(recB + (k & 1) * RING, six);
      else P.sr.store_t(recB + (k & 1) * RING, t8);
    };
    // two-deep pipeline: block k-1 is rebuilt from registers loaded one interval earlier, while block k-2's
    // loads are in flight (an HBM round trip under load is longer than one interval)
    // (the two register sets alternate by hand-unrolling: a copy of in-flight loads would wait for them)
    Prep Pa, Pb;
    prep_load(Pa, nb - 1);
    prep_load(Pb, nb >= 2 ? nb - 2 : 0);
    prep_store(Pa, nb - 1);
    __syncthreads();
    auto step = [&](int k, Prep& Pc, Prep& Pnext) {  // interval k: Pc holds block k-1's loads
      PHS(0)
      prep_load(Pnext, k >= 2 ? k - 2 : 0);             // unconditional (clamped): no branch around loads in flight
      PHS(1)
      if (k + 1 < nb)
        bwd_grad_jobs<NH>(dT + ((k + 1) & 1) * J::ND * TILE, aT + ((k + 1) % 3) * J::NA * TILE,
                          slab + (long long)(k + 1) * J::BLK, hw);
      PHS(2)
      if (k >= 1) prep_store(Pc, k - 1);
      PHS(3)
      __syncthreads();
    };
    for (int k = nb - 1; k >= 0; k -= 2) {
      step(k, Pb, Pa);
      if (k == 0) break;
      step(k - 1, Pa, Pb);
    }
    bwd_grad_jobs<NH>(dT, aT, slab, hw);                     // block 0 (tiles of the last interval)
  } else {
    const int tid = t8;
    const long long b = (long long)blockIdx.x * 16 + s;
    const bool valid = b < B;
    const long long bc = valid ? b : B - 1;
    const int D = L.D, Da = L.Da, Db = L.Db;
    float* d1l = d1 + bc * 16 + j;                    // D1[k][b][j]  = d1l[k * B * 16]
    float* d1_dummy = d1 + (long long)nb * B * 16 + j; // rows past the batch (workspace slack)
    const long long hps = B * 16;

    float gya = 0.f, gyb = 0.f, dl = 0.f;
    if (valid) {                                      // padded rows carry zero gradient
      if (nll) {    // d/dz, d/dldj of mean_b(0.5 |z_b|^2 - ldj_b); dz holds z here
        const float sc = (dloss ? dloss[0] + dloss[1] : 1.f) / (float)B;   // d loss/d nll = d nll/d nll = 1
        gya = (j < Da) ? dz[b * D + j] * sc : 0.f;
        gyb = (j < Db) ? dz[b * D + Da + j] * sc : 0.f;
        dl = -sc;
      } else {
        if (dz) {
          gya = (j < Da) ? dz[b * D + j] : 0.f;
          gyb = (j < Db) ? dz[b * D + Da + j] : 0.f;
        }
        if (dldj) dl = dldj[b];
      }
    }
    __syncthreads();
    PHS(0)
    for (int k = nb - 1; k >= 0; --k) {
      const int cur = k & 1;
      float gs[4 * BWD_G4];
      {
        const floatx4* gd4 = gsl + cur * BWD_G4 * BCNF_WG + tid;
#pragma unroll
        for (int i = 0; i < BWD_G4; ++i) {
          const floatx4 v = gd4[i * BCNF_WG];
          gs[4 * i] = v[0];
          gs[4 * i + 1] = v[1];
          gs[4 * i + 2] = v[2];
          gs[4 * i + 3] = v[3];
        }
      }
      float* Tt = dT + cur * J::ND * TILE + tix;
      // the record streams in consumption order (RecB): ActNorm + Q^T, then the heads, then each stage issues the
      // reads of a later one behind a scheduling barrier, so every wait covers a few reads, not the whole record
      // (lgkmcnt counts at most 15 outstanding: a block-wide burst of 53 reads made the mix wait for ~40 of them).
      // BC: ActNorm + Q^T are 11 reads behind the slot's 3, so the mix waits on a counted lgkmcnt with the head
      // reads still in flight (the rotation form's 3 + 17 + 8 reads overflow the counter: its mix waits for all).
      const float* R = recB + cur * RING + j * L.RB;
      float rb[RBk::USED];
      ld_rec<0, RBk::qt_end(BC)>(rb, R);                 // ActNorm, Q^T
      __builtin_amdgcn_sched_barrier(0);
      ld_rec<RBk::TT, RBk::TT + RBk::head_len(BC)>(rb, R);   // T / S heads
      ld_rec<RBk::ST, RBk::ST + RBk::head_len(BC)>(rb, R);
      __builtin_amdgcn_sched_barrier(0);
      const float* gd = gs;
      const float S = gs[NH], ya = gs[NH + 1], yb = gs[NH + 2];
      const float an_sa = rb[RBk::AN], an_sb = rb[RBk::AN + 2], an_bb = rb[RBk::AN + 3];
      const float xb = fmaf(an_sb, yb, an_bb);
      const float e = exp_fast(S);
      float gza, gzb;
      if constexpr (BC) mix_bc(rb + RBk::QT, gya, gyb, gza, gzb);   // g @ Q^T (identity for the last block)
      else mix(rb + RBk::QT, gya, gyb, gza, gzb);
      ld16(rb + RBk::HID, R + RBk::HID);                 // hidden layer NH
      __builtin_amdgcn_sched_barrier(0);
      const float dT_ = gzb;                             // z_b = exp(s) y_b + t
      const float dS = (j < Db) ? fmaf(gzb * e, xb, dl) : 0.f;
      const float dSp = dS * (1.f - S * S);
      const float dxb = gzb * e;
      Tt[NH * TILE] = dT_;
      Tt[(NH + 1) * TILE] = dSp;
      float da = 0.f, da2 = 0.f;
      if constexpr (BC) bc9x2(dT_, rb + RBk::TT, da, dSp, rb + RBk::ST, da2);
      else rot16x2(dT_, rb + RBk::TT, da, dSp, rb + RBk::ST, da2);
      da += da2;
#pragma unroll
      for (int l = NH; l >= 2; --l) {
        ld16(rb + RBk::HID + 16 * (NH - l + 1), R + RBk::HID + 16 * (NH - l + 1));   // next layer (last: W1^T)
        __builtin_amdgcn_sched_barrier(0);
        const float dpre = da * gd[l - 1];
        Tt[(l - 1) * TILE] = dpre;
        da = rot16(dpre, rb + RBk::HID + 16 * (NH - l), 0.f);
      }
      const float dpre1 = da * gd[0];
      Tt[0] = dpre1;
      *(valid ? d1l + k * hps : d1_dummy) = dpre1;      // dL/d pre-activation of Linear 1 (split-K, dh)
      const float dxa = rot16(dpre1, rb + RBk::W1T, gza);
      {   // ActNorm tiles (consumed only for blocks that have an ActNorm)
        const float inv_a = (j < Da) ? __builtin_amdgcn_rcpf(an_sa) : 0.f;
        const float inv_b = (j < Db) ? __builtin_amdgcn_rcpf(an_sb) : 0.f;
        Tt[(NH + 2) * TILE] = fmaf(dxa, ya, dl * inv_a);
        Tt[(NH + 3) * TILE] = dxa;
        Tt[(NH + 4) * TILE] = fmaf(dxb, yb, dl * inv_b);
        Tt[(NH + 5) * TILE] = dxb;
      }
      gya = an_sa * dxa;
      gyb = an_sb * dxb;
      PHS(1)
      __syncthreads();
      PHS(2)
    }
    if (dy && valid) {
      if (j < Da) dy[b * D + j] = gya;
      if (j < Db) dy[b * D + Da + j] = gyb;
    }
  }
#if BCNF_STAMPS
  if (blockIdx.x == 0 && (threadIdx.x == 0 || threadIdx.x == BCNF_WG))
    for (int i = 0; i < 4; ++i) g_phase[(helper ? 4 : 0) + i] = ph_acc[i];
#endif
#undef PHS
  if (loss_out && blockIdx.x == 0) {                 // deferred NLL reduction of the forward
    __syncthreads();                                  // (the helpers' last jobs have read the tiles)
    nll_finalize<BWD_WG>(nll_part, (int)gridDim.x, B, loss_out, rng_w, guard, dT);
  }
}

}  // namespace

namespace bcnf_small {

int launch_backward(const BcnfLayout& L, const float* pk, const float* dz, const float* dldj, const float* dloss,
                    int nll, long long B, const float* arec, float* dy, float* d1, float* slab, const float* part,
                    float* loss_out, uint64_t* rng_w, int32_t* guard, hipStream_t st) {
  return dispatch_nh(L.NH, [&](auto nh) -> int {
    constexpr int NH = decltype(nh)::value;
    if (!layout_matches<NH>(L)) return BCNF_ERR_ARG;
    const dim3 grid((unsigned)((B + 15) / 16));
#define BWD(BC) \
  launch<k_backward<NH, BC>>(grid, dim3(BWD_WG), bwd_lds_bytes(L), st, L, pk, dz, dldj, dloss, nll, B, arec, dy, d1, \
                             slab, slab_stride_of(L), part, loss_out, rng_w, guard)
    return layout_bc(L) ? BWD(true) : BWD(false);
#undef BWD
  });
}

#if BCNF_STAMPS
int bwd_debug_phases(unsigned long long* out) {
  return bcnf_rt::hip_status(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(g_phase)));
}
#endif

}  // namespace bcnf_small
