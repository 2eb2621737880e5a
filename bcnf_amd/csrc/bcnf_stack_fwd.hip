// bcnf_amd small stack family: the whole-stack forward (k_forward, packed and pack-free) and the NLL finalize launch.
// The family's files: bcnf_stack_internal.h.
#include "bcnf_stack_internal.h"
#include "bcnf_stack_rec.h"

namespace {
using namespace bcnf_small;
using bcnf_rt::launch;

#if BCNF_STAMPS
__device__ unsigned long long g_phase[32];   // phase stamps (bcnf_debug_phases), diagnostic build only
#endif

// Condition projection operands of the forward (the y-independent part of Linear 1, cnf.py:98-107 with the
// condition columns): HP[b][16k + j] = sum_c h[b][c] W1hC[c][16k + j] + b1c[16k + j]; on the folded path h = x and
// W1hC / b1c are the folded Wc / bc (fold_layout).
struct ProjArgs {
  const float* h;
  const float* w1c;      // [Cp][NKp], rows >= C zero
  const float* b1c;      // [NKp]
  long long ldh;
  int C, Cp, NKp;
};
// RAW (bcnf_fold_train_forward): the pack-free folded training forward, so the folded training step needs no pack
// launch. Differences from the packed forward, all in the prologue and the helper waves:
//  * records: each helper thread owns RAW_NS words of a ring slot (build_raw_table) and gathers block k's record
//    straight from the parameters -- RAW_NP loads at k * blk_stride + src, RAW_NQ at k * D * D + src, zero words
//    written once; the last block (no ActNorm, identity mix) through rec_f on the same words;
//  * projection: helper wave hw computes h^T = Wf x^T + bf for its 16-column tiles ct = hw, hw + 4, .. of the
//    workgroup's 16 samples on fp32 MFMA (once), and that output layout IS the projection's A operand with the K
//    order (ct, r) -> column 16 ct + 4 lq + r, so no LDS round trip: per block the B operand is W1_k[j][Da + that
//    column] read from the parameters. The sums are the unfolded ones (h first), not the folded Wc;
//  * batch rows: with idx the rows come from the pools (the captured step's batch gather), and the forward writes
//    the gathered y and x rows for the backward;
//  * side outputs for the backward kernels, spread over the grid in the helpers' first interval: the backward
//    records PB and W1hR into `pk`; the compute waves sum the ActNorm log-det constant themselves.
struct RawArgs : RawForward {};         // the fields: bcnf_stack_internal.h
constexpr int RAW_WQ = 8;              // Wf quads per thread in flight while staging (C * ceil(X / 4) <= 2048 in one go)
constexpr int RAW_SIDE_Q = 4;          // side units per workgroup done in the idle interval
__host__ __device__ constexpr int raw_hs_pitch(int C) { return 16 * ((C + 15) / 16) + 4; }
__device__ __forceinline__ long long raw_row(const RawArgs& R, long long B, long long b) {
  return R.idx ? (long long)R.idx[(R.cursor ? R.cursor[0] * B : 0) + b] : b;
}

constexpr int HP_SMAX = 16;            // K-steps of 4 per helper wave: Cp / 16 <= 16 (Cp <= 256)
constexpr int FWD_SLOTS = 3;           // ring depth: the helpers prepare block k + 2 while block k runs
constexpr int FWD_HP = FWD_SLOTS * 4 * 256;   // LDS: [slot][4 helper waves][16 samples][16] partial HP tiles
constexpr int FWD_HEAD = 24;           // record floats the compute waves prefetch one block ahead (ActNorm, b1, W1y)

// Whole-stack forward, one launch, 512 threads = two roles per SIMD (waves w and w + 4 share a SIMD):
//  * compute waves 0..3 (4 samples each, row layout): ActNorm -> nested MLP (GELU, dropout) -> affine coupling ->
//    log-det -> orthonormal mix of block k, reading its record, condition projection and dropout multipliers from
//    LDS;
//  * helper waves 4..7 prepare block k + 2 in the same interval (a 3-slot ring): stage its forward record into LDS,
//    compute its condition projection for the workgroup's 16 samples on fp32 MFMA (one K-quarter per helper wave;
//    the compute lanes add the four partials in a fixed order), and draw its dropout multipliers (Philox -> floats).
// With the ring one block deeper, the compute waves read block k + 1's record head, projection partials and
// multipliers at the end of block k (its slot is complete since the previous barrier), so a block starts without
// an LDS round trip: a lone wave per SIMD is issue-bound on its own stream (tools/probe_issue.py, recalibrated in
// r05: ~5 cycles per plain VALU, 6-8 per DPP FMA), and the old block start waited for 27 record reads of
// all four compute waves. The rest of the record streams in two stages ahead (mlp_forward_s).
// The projection needs no separate GEMM launch and no HBM round trip, and the compute waves' loop issues no global
// loads (the record stores of SAVE are its only VMEM traffic).
// BC: a D = 19 stack, whose Linear 1 y-part and mix sections are in broadcast form (L.qbc): the compute waves read
// only those sections' live words -- 52 LDS reads per block instead of 59 (bcnf_stack_rec.h, RecF).
template <int NH, bool DROP, bool SAVE, bool RAW, bool BC>
__global__ __launch_bounds__(2 * BCNF_WG) void k_forward(BcnfLayout L, const float* __restrict__ pk,
                                                    const float* __restrict__ y, ProjArgs P,
                                                    long long B, float* __restrict__ z, float* __restrict__ ldj_out,
                                                    float* __restrict__ logp, const uint64_t* rng,
                                                    float* __restrict__ arec, float* __restrict__ nll_part,
                                                    RawArgs R) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int RFL = 16 * L.RF;
  float* rec = smem;                          // [3][16*RF]
  float* hpb = rec + FWD_SLOTS * RING;        // [3][4][16][16]
  floatx4* mkb = reinterpret_cast<floatx4*>(hpb + FWD_HP);   // [3][2][256] dropout multipliers of layers 1..8
  float* lps = hpb + FWD_HP + FWD_SLOTS * 8 * 256;            // RAW: the helpers' log-det constant partials [4]
  float* hs = lps + 4;                                        // RAW: h of the 16 rows [16][raw_hs_pitch(C)]
  using AR = ActRec<NH>;
  static_assert(NH <= 8, "two float4 of dropout multipliers");
  const int nb = L.nb;
  const float* pf = pk + L.pf_off;
  const bool helper = threadIdx.x >= BCNF_WG;
  const int t8 = (int)threadIdx.x & (BCNF_WG - 1);              // thread index within the role
  const int j = t8 & 15, s = sample_of(t8);                     // (sample, lane) of a compute / Philox thread
  const long long b = (long long)blockIdx.x * 16 + s;
  const long long bc = b < B ? b : B - 1;                       // rows past the batch replay the last sample
  uint64_t seed = 0, off = 0;
  if (DROP) { seed = rng[0]; off = rng[1]; }
  // diagnostic build: per-phase cycles of workgroup 0's wave 0 (compute) and wave 4 (helper) -> g_phase[8..]
  unsigned long long ph_t = BCNF_STAMPS ? __builtin_amdgcn_s_memtime() : 0ULL, ph_acc[3] = {0, 0, 0};
  const unsigned long long ph_t0 = ph_t;
  const unsigned long long ph_r0 = BCNF_STAMPS ? __builtin_amdgcn_s_memrealtime() : 0ULL;   // 100 MHz
  unsigned long long ph_b[2] = {0, 0};   // RAW prologue: cycles from the start to barrier #0 / #1 arrival
#define PHB(i)                                                 \
  if (BCNF_STAMPS) ph_b[i] = __builtin_amdgcn_s_memtime() - ph_t0;
  unsigned long long ph_p[4] = {0, 0, 0, 0};   // RAW prologue points (each after an explicit wait: stamped build only)
#define PHP(i)                                                                           \
  if (BCNF_STAMPS) {                                                                     \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                          \
    ph_p[i] = __builtin_amdgcn_s_memtime() - ph_t0;                                      \
  }
#define PHF(i)                                                                                   \
  if (BCNF_STAMPS) {                                                                             \
    const unsigned long long _t = __builtin_amdgcn_s_memtime();                                  \
    ph_acc[i] += _t - ph_t;                                                                      \
    ph_t = _t;                                                                                   \
  }

  if (helper) {
    const int hw = __builtin_amdgcn_readfirstlane(t8 >> 6);
    const int l64 = t8 & 63, lr = l64 & 15, lq = l64 >> 4;
    if constexpr (RAW) {
      const int Da = L.Da, C = L.C, X = R.X, H1 = L.H[1], D = L.D, an = L.an_size;
      const int nt = (C + 15) >> 4;                               // 16-column tiles of h (<= 4 RAW_TPW)
      const long long row = (long long)blockIdx.x * 16 + lr;
      const float* xrow = R.xpool + raw_row(R, B, row < B ? row : B - 1) * R.ldx;
      // ---- prologue loads, all issued before any of them is consumed ----
      // this thread's table slots: RAW_NSP / 4 16-byte loads, all issued before any is used (decoded one at a time,
      // the compiler waited for each load before issuing the next)
      uint32_t tw[RAW_NSP];
#pragma unroll
      for (int i = 0; i < RAW_NSP / 4; ++i) {
        const uint4 v = reinterpret_cast<const uint4*>(R.table + t8 * RAW_NSP)[i];
        tw[4 * i] = v.x;
        tw[4 * i + 1] = v.y;
        tw[4 * i + 2] = v.z;
        tw[4 * i + 3] = v.w;
      }
      // side units of this workgroup (RawSide): backward-record chunks u < nb * ch, then W1hR rows
      const int rb16 = 16 * L.RB, ch = (rb16 + BCNF_WG - 1) / BCNF_WG, n_units = nb * ch + L.NKp;
      const uint32_t* tpb = R.table + RAW_NSP * BCNF_WG;
      uint32_t pbe[RAW_SIDE_Q];                                   // (the unit checks happen at the use)
#pragma unroll
      for (int q = 0; q < RAW_SIDE_Q; ++q) {
        const int u = blockIdx.x + q * gridDim.x, n = (u % ch) * BCNF_WG + t8;
        pbe[q] = tpb[n < rb16 ? n : 0];
      }
      asm volatile("" ::: "memory");                              // the table loads above are all in flight
      uint32_t srcb[RAW_NP + RAW_NQ], dstb[RAW_NP + RAW_NQ];      // byte offsets: source, word of the ring slot
#pragma unroll
      for (int i = 0; i < RAW_NP + RAW_NQ; ++i) {
        srcb[i] = (tw[i] >> 12) * 4u;
        dstb[i] = (tw[i] & 4095u) * 4u;
      }
      uint32_t zw[RAW_NZ];
#pragma unroll
      for (int i = 0; i < RAW_NZ; ++i) zw[i] = tw[RAW_NP + RAW_NQ + i] & 4095u;
      PHP(0)
      // projection B operand of block k: W1_k[lr][Da + 16 ct + 4 lq + r], r = 0..3 one (dword-aligned) 16-byte load
      // per tile (at most 3 floats past the row end: still inside the block's parameters), zero past C or H[1]
      int wo[RAW_TPW];
      uint32_t wok = 0;
#pragma unroll
      for (int i = 0; i < RAW_TPW; ++i) {
        const int c0 = 16 * (hw + 4 * i) + 4 * lq;
        wo[i] = (c0 < C && lr < H1) ? L.lin_w[1] + lr * L.lin_in[1] + Da + c0 : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) wok |= (c0 + r < C && lr < H1) ? 1u << (4 * i + r) : 0u;
      }
      const bool bias_lane = hw == 0 && lr < H1;
      struct Pre {                                                // one block's loaded operands
        float v[RAW_NP + RAW_NQ];
        floatx4 w4[RAW_TPW];
        float bias;
      };
      // buffer loads: the block base goes in the scalar offset, the table's byte offset in the vector offset (no
      // per-lane 64-bit address arithmetic, which otherwise stays live across the loop)
      const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(R.P), (short)0,
                                                                         (int)(L.n_trainable * 4), 0x00020000);
      const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(R.Q), (short)0,
                                                                         (nb - 1) * D * D * 4, 0x00020000);
      // The last block (rec_f with k = nb - 1) goes through the same branch-free loads: its coupling sits an_size
      // floats earlier in its block (no ActNorm), so the P base shifts by -an_size and only the ActNorm words --
      // the an_size smallest sources, slot 0 of threads < an_size -- take constants (scale 1, bias 0); its Q base
      // lies past the end of qmats, where the buffer range check returns 0, and the diagonal words take 1
      // (identity mix). Those fix-ups happen at the use (finish_rec), so no load is waited for early.
      const bool an_word = (int)(srcb[0] >> 2) < an;
      const float an_val = (int)(srcb[0] >> 2) < D ? 1.f : 0.f;
      bool q_diag[RAW_NQ];
#pragma unroll
      for (int i = 0; i < RAW_NQ; ++i) q_diag[i] = ((srcb[RAW_NP + i] >> 2) % (uint32_t)(D + 1)) == 0;
      auto load = [&](int k, Pre& g) {
        const int cb = coupling_base(L, k);
        const int sp = (k < nb - 1 ? k * L.blk_stride : k * L.blk_stride - an) * 4, sq = k * D * D * 4;
#pragma unroll
        for (int i = 0; i < RAW_NP; ++i)
          g.v[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rP, srcb[i], sp, 0));
#pragma unroll
        for (int i = RAW_NP; i < RAW_NP + RAW_NQ; ++i)
          g.v[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rQ, srcb[i], sq, 0));
#pragma unroll
        for (int i = 0; i < RAW_TPW; ++i) {   // unconditional (wo = 0 for an absent tile, whose MFMAs are skipped)
          const auto w = __builtin_amdgcn_raw_buffer_load_b128(rP, wo[i] * 4, cb * 4, 0);
          g.w4[i] = floatx4{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3])};
        }
        // raw: the select waits for the load, so it happens at the use (finish_proj), not here
        g.bias = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rP, (L.lin_b[1] + lr) * 4, cb * 4, 0));
      };
      float xa[RAW_TPW][4];                                       // h[row lr][16 (hw + 4 i) + 4 lq + r]
      // block k -> slot sl (a constant after unrolling): dropout multipliers and record (no h needed), then the
      // projection partial
      auto finish_rec = [&](int k, int sl, const Pre& g) {
        if (DROP) {
          const uint32_t bits = dropout_bits<NH>(L, seed, off, bc, k, j, 0u);
          float m[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) m[i] = ((bits >> i) & 1u) ? L.keep_scale : 0.f;
          mkb[(2 * sl) * BCNF_WG + t8] = floatx4{m[0], m[1], m[2], m[3]};
          mkb[(2 * sl + 1) * BCNF_WG + t8] = floatx4{m[4], m[5], m[6], m[7]};
        }
        char* slot = reinterpret_cast<char*>(rec + sl * RING);
        float v0 = g.v[0], vq[RAW_NQ];
#pragma unroll
        for (int i = 0; i < RAW_NQ; ++i) vq[i] = g.v[RAW_NP + i];
        if (k == nb - 1) {                                        // uniform
          v0 = an_word ? an_val : v0;
#pragma unroll
          for (int i = 0; i < RAW_NQ; ++i) vq[i] = q_diag[i] ? 1.f : vq[i];
        }
        *reinterpret_cast<float*>(slot + dstb[0]) = v0;
#pragma unroll
        for (int i = 1; i < RAW_NP; ++i) *reinterpret_cast<float*>(slot + dstb[i]) = g.v[i];
#pragma unroll
        for (int i = 0; i < RAW_NQ; ++i) *reinterpret_cast<float*>(slot + dstb[RAW_NP + i]) = vq[i];
      };
      auto finish_proj = [&](int sl, const Pre& g) {
        const float bias = bias_lane ? g.bias : 0.f;
        floatx4 acc = {bias, bias, bias, bias};
#pragma unroll
        for (int i = 0; i < RAW_TPW; ++i)
          if (hw + 4 * i < nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc = mfma4(xa[i][r], ((wok >> (4 * i + r)) & 1u) ? g.w4[i][r] : 0.f, acc);
        float* hd = hpb + sl * 1024 + hw * 256 + 64 * lq + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) hd[16 * r] = acc[r];
      };
      auto finish = [&](int k, int sl, const Pre& g) {
        finish_rec(k, sl, g);
        finish_proj(sl, g);
      };
      Pre gb[FWD_SLOTS];                                          // block b's operands in gb[b % 3] (interval())
      load(0, gb[0]);
      load(1, gb[1]);                                             // nb >= 2 (build_raw_table)
      load(nb > 2 ? 2 : 1, gb[2]);
      asm volatile("" ::: "memory");                              // all three blocks' loads issued here, not sunk
      PHP(1)
#pragma unroll
      for (int i = 0; i < RAW_NZ; ++i)                            // this thread's zero words, in all three slots
#pragma unroll
        for (int sl = 0; sl < FWD_SLOTS; ++sl) rec[sl * RING + zw[i]] = 0.f;
      finish_rec(0, 0, gb[0]);
      finish_rec(1, 1, gb[1]);
      PHP(2)
      __syncthreads();                                            // barrier A (the compute waves' operand staging)
      PHB(0)
      __syncthreads();                                            // barrier B: the compute waves' h tile is in hs
#pragma unroll
      for (int i = 0; i < RAW_TPW; ++i) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(hs + lr * raw_hs_pitch(C) + 16 * (hw + 4 * i) + 4 * lq);
#pragma unroll
        for (int r = 0; r < 4; ++r) xa[i][r] = v[r];
      }
      finish_proj(0, gb[0]);
      finish_proj(1, gb[1]);
      // ---- side work: the backward kernels' inputs, one unit per workgroup and q (coalesced rows) ----
      auto side_unit = [&](int u, uint32_t e) {
        if (u < nb * ch) {
          const int k = u / ch, n = (u - k * ch) * BCNF_WG + t8;
          if (n >= rb16) return;
          const uint32_t kind = e & 3u, src = e >> 2;
          float v = 0.f;
          if (k < nb - 1) {
            if (kind == 0) v = R.P[(long long)k * L.blk_stride + src];
            else if (kind == 1) v = R.Q[(long long)k * D * D + src];
          } else if (kind == 0) {
            v = (int)src < an ? ((int)src < D ? 1.f : 0.f) : R.P[(long long)k * L.blk_stride - an + src];
          } else if (kind == 1) {
            v = (src % (uint32_t)(D + 1)) == 0 ? 1.f : 0.f;
          }
          R.pk[L.pb_off + (long long)k * rb16 + n] = v;
        } else if (u < n_units) {
          const int kj = u - nb * ch, k = kj >> 4, jj = kj & 15;
          const bool live = k < nb && jj < H1;
          const float* w = live ? R.P + coupling_base(L, k) + L.lin_w[1] + jj * L.lin_in[1] + Da : R.P;
          for (int c = t8; c < L.Cp; c += BCNF_WG) R.pk[L.w1r_off + (long long)kj * L.Cp + c] = (live && c < C) ? w[c] : 0.f;
        }
      };
      // intervals k < nb - 2 prepare block k + 2 into slot (k + 2) % 3 (unrolled by 3: constant LDS offsets); the
      // last two intervals have no block to prepare and take the side work: this workgroup's units (k = nb - 2) and
      // the log-det constant into lps for the compute epilogue (k = nb - 1)
      // software-pipelined: block k + 3's operands are loaded in interval k and consumed in interval k + 1, so an
      // interval never waits for its own loads; with the loop unrolled by 3 every buffer index is a constant
      PHB(1)
      auto interval = [&](int k, int sl) {
        // unconditional (block nb - 1 again past the end, unused): a load on one path only would make the wait
        // counts conservative -- the consumers would wait for this interval's loads too
        load(k + 3 < nb ? k + 3 : nb - 1, gb[sl == FWD_SLOTS - 1 ? 0 : sl + 1]);
        asm volatile("" ::: "memory");                            // issued here, consumed next interval
        finish(k + 2, sl, gb[sl]);
        PHF(1)
        // LDS writes complete, then a bare barrier: __syncthreads' release fence would also wait for the loads of
        // block k + 3 still in flight (vmcnt counts them too)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        PHF(2)
      };
      __syncthreads();
      PHF(0)
      for (int k = 0; k < nb - 2; k += FWD_SLOTS) {
        interval(k, 2);
        if (k + 1 < nb - 2) interval(k + 1, 0);
        if (k + 2 < nb - 2) interval(k + 2, 1);
      }
#pragma unroll
      for (int q = 0; q < RAW_SIDE_Q; ++q) side_unit(blockIdx.x + q * gridDim.x, pbe[q]);
      {  // the ActNorm log-det constant  sum_k sum_i log|scale_k,i|  (cnf.py:350): strided partials (loads issued
         // together), a fixed-order butterfly per wave, lps[hw] for the compute epilogue after the last barrier
        constexpr int LU = 4;
        float acc = 0.f;
        const int n = (nb - 1) * D;
        for (int i0 = t8; i0 < n; i0 += LU * BCNF_WG) {
          float v[LU];
#pragma unroll
          for (int u = 0; u < LU; ++u) {
            const int i = i0 + u * BCNF_WG, ii = i < n ? i : 0, kb = ii / D;
            v[u] = R.P[(long long)kb * L.blk_stride + (ii - kb * D)];
          }
#pragma unroll
          for (int u = 0; u < LU; ++u)
            if (i0 + u * BCNF_WG < n) acc += logf(fabsf(v[u]));
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
        if (l64 == 0) lps[hw] = acc;
      }
      __syncthreads();                                            // interval nb - 2
      __syncthreads();                                            // interval nb - 1
      for (int u = blockIdx.x + RAW_SIDE_Q * gridDim.x; u < n_units; u += gridDim.x)   // small grids only
        side_unit(u, u < nb * ch ? tpb[(u % ch) * BCNF_WG + t8 < rb16 ? (u % ch) * BCNF_WG + t8 : 0] : 0u);
    } else {
    const int S = P.Cp >> 4;                                     // K-steps per helper wave
    const long long row = (long long)blockIdx.x * 16 + lr;
    const float* hrow = P.h + (row < B ? row : B - 1) * P.ldh;
    float xa[HP_SMAX];                                           // A operand: this wave's K-quarter of h / x
#pragma unroll
    for (int t = 0; t < HP_SMAX; ++t) {
      const int kk = 4 * (hw * S + t) + lq;
      xa[t] = (t < S && kk < P.C) ? hrow[kk < P.C ? kk : 0] : 0.f;
    }
    const float* wcol = P.w1c + (long long)(4 * hw * S + lq) * P.NKp + lr;   // + 4 t NKp + 16 k
    // block k's projection partial, dropout multipliers and record -> slot sl
    auto prepare = [&](int k, int sl) {
      Stage<STAGE_REC> sr;
      sr.load_t(pf + (long long)k * RFL, RFL, t8);
      float wb[HP_SMAX];
#pragma unroll
      for (int t = 0; t < HP_SMAX; ++t) wb[t] = (t < S) ? wcol[(long long)4 * t * P.NKp + 16 * k] : 0.f;
      if (DROP) {
        const uint32_t bits = dropout_bits<NH>(L, seed, off, bc, k, j, 0u);
        float m[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = ((bits >> i) & 1u) ? L.keep_scale : 0.f;
        mkb[(2 * sl) * BCNF_WG + t8] = floatx4{m[0], m[1], m[2], m[3]};
        mkb[(2 * sl + 1) * BCNF_WG + t8] = floatx4{m[4], m[5], m[6], m[7]};
      }
      const float bias = (hw == 0) ? P.b1c[16 * k + lr] : 0.f;
      floatx4 acc = {bias, bias, bias, bias};
#pragma unroll
      for (int t = 0; t < HP_SMAX; ++t)
        if (t < S) acc = mfma4(xa[t], wb[t], acc);
      float* hd = hpb + sl * 1024 + hw * 256 + 64 * lq + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) hd[16 * r] = acc[r];
      sr.store_t(rec + sl * RING, t8);
    };
    prepare(0, 0);
    if (nb > 1) prepare(1, 1);
    __syncthreads();
    PHF(0)
    int sl = 2;
    for (int k = 0; k < nb; ++k) {
      if (k + 2 < nb) prepare(k + 2, sl);
      sl = sl == FWD_SLOTS - 1 ? 0 : sl + 1;
      PHF(1)
      __syncthreads();
      PHF(2)
    }
    }
  } else {
    const int tid = t8;
    // the compute waves issue ahead of the helper wave on their SIMD whenever both are ready (r06: k_forward
    // -1.1 us same box, profiles/r06b_rawab.txt; the helpers have slack at every block's barrier)
    __builtin_amdgcn_s_setprio(3);
    const int D = L.D, Da = L.Da, Db = L.Db;
    float ya, yb, ldc = 0.f;
    if constexpr (RAW) {
      // h^T = Wf x^T + bf of the workgroup's 16 rows on the matrix cores. Wf (C x X) and the 16 x rows are staged
      // into LDS by coalesced 16-byte loads of all four compute waves (per-lane strided operand loads made ~1.2M
      // cache-line requests per launch and queued everyone's first loads behind them), then compute wave
      // cw takes the column tiles ct = cw + 4 i. K order: MFMA step (u, r) of lane (lr, lq) is column
      // 16 u + 4 lq + r, so each operand quad is one conflict-free ds_read_b128 (row pitch RAW_KP = 4 mod 32), and
      // the output layout (h[row lr][16 ct + 4 lq + r] at lane (lr, lq)) is helper wave cw's projection A operand.
      // ldc: the helpers' wave sums of the ActNorm log-det constant (lps), read after the last barrier.
      const long long src = raw_row(R, B, bc);
      ya = (j < Da) ? R.ypool[src * D + j] : 0.f;
      yb = (j < Db) ? R.ypool[src * D + Da + j] : 0.f;
      // float4 quads per row (<= RAW_KP / 4 - 1): XQ hold columns; the h GEMM's K steps run to XQP, so Wf's quads
      // XQ .. XQP - 1 are stored as zeros -- LDS holds whatever the previous kernel left there, and a 0 x NaN residue
      // made the loss NaN
      const int C = L.C, X = R.X, XQ = (X + 3) >> 2, XQP = ((X + 15) >> 4) * 4;
      float* ws = hs + 16 * raw_hs_pitch(C);                      // Wf [C][RAW_KP]
      float* xs = ws + C * RAW_KP;                                // x rows [16][RAW_KP]
      const int cw = __builtin_amdgcn_readfirstlane(tid >> 6), l64 = tid & 63, lr = l64 & 15, lq = l64 >> 4;
      const float* bfp = R.bf ? R.bf : R.wf;
      float hb[RAW_TPW][4];                                       // bf of the columns this lane ends with
#pragma unroll
      for (int i = 0; i < RAW_TPW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cc = 16 * (cw + 4 * i) + 4 * lq + r;
          hb[i][r] = bfp[cc < C ? cc : 0];
        }
      {
        // every staging load in flight at once (one round trip): Wf quad (c, q) = columns 4q .. 4q + 3 of row c,
        // read past the row end into the next row (zeroed below) and past the tensor's end through a range-checked
        // buffer load (0); the x quads of the 16 rows (gathered through idx when given), the row's last partial
        // quad element by element
        const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(R.wf), (short)0,
                                                                           C * X * 4, 0x00020000);
        // the K padding quads first: their stores need no load and go out before the staging round trip
        for (int i = tid; i < C * (XQP - XQ); i += BCNF_WG) {
          const int c = i / (XQP - XQ), q = XQ + (i - c * (XQP - XQ));
          *reinterpret_cast<floatx4*>(ws + c * RAW_KP + 4 * q) = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        const int nq = C * XQ;
        uint32_t v[RAW_WQ][4];
#pragma unroll
        for (int u = 0; u < RAW_WQ; ++u) {
          const int i = tid + u * BCNF_WG, ii = i < nq ? i : 0, c = ii / XQ, q = ii - c * XQ;
          const auto w = __builtin_amdgcn_raw_buffer_load_b128(rW, (c * X + 4 * q) * 4, 0, 0);
          v[u][0] = w[0]; v[u][1] = w[1]; v[u][2] = w[2]; v[u][3] = w[3];
        }
        constexpr int NXQ = (16 * (RAW_KP / 4) + BCNF_WG - 1) / BCNF_WG;
        floatx4 xo[NXQ];
#pragma unroll
        for (int u = 0; u < NXQ; ++u) {
          const int i = tid + u * BCNF_WG, ii = i < 16 * (RAW_KP / 4) ? i : 0;
          const int rr = ii / (RAW_KP / 4), q = ii - rr * (RAW_KP / 4);
          const long long bb = (long long)blockIdx.x * 16 + rr;
          const float* xr = R.xpool + raw_row(R, B, bb < B ? bb : B - 1) * R.ldx + 4 * q;
          xo[u] = floatx4{0.f, 0.f, 0.f, 0.f};
          if (4 * q + 3 < X) {
            __builtin_memcpy(&xo[u], xr, sizeof(floatx4));
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (4 * q + r < X) xo[u][r] = xr[r];
          }
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = 0; u < RAW_WQ; ++u) {
          const int i = tid + u * BCNF_WG, c = i / XQ, q = i - c * XQ;
          if (i < nq) {
            floatx4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = 4 * q + r < X ? __uint_as_float(v[u][r]) : 0.f;
            *reinterpret_cast<floatx4*>(ws + c * RAW_KP + 4 * q) = o;
          }
        }
        for (int i = nq > RAW_WQ * BCNF_WG ? tid + RAW_WQ * BCNF_WG : nq; i < nq; i += BCNF_WG) {   // C X > 7680
          const int c = i / XQ, q = i - c * XQ;
          const auto w = __builtin_amdgcn_raw_buffer_load_b128(rW, (c * X + 4 * q) * 4, 0, 0);
          floatx4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = 4 * q + r < X ? __uint_as_float(w[r]) : 0.f;
          *reinterpret_cast<floatx4*>(ws + c * RAW_KP + 4 * q) = o;
        }
#pragma unroll
        for (int u = 0; u < NXQ; ++u) {
          const int i = tid + u * BCNF_WG;
          if (i < 16 * (RAW_KP / 4)) {
            const int rr = i / (RAW_KP / 4), q = i - rr * (RAW_KP / 4);
            *reinterpret_cast<floatx4*>(xs + rr * RAW_KP + 4 * q) = xo[u];
            const long long bb = (long long)blockIdx.x * 16 + rr;
            if (R.xdst && bb < B && 4 * q < X) {                  // the backward tail's x rows
              float* xd = R.xdst + bb * R.ldx + 4 * q;
              if (4 * q + 3 < X) {
                __builtin_memcpy(xd, &xo[u], sizeof(floatx4));
              } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (4 * q + r < X) xd[r] = xo[u][r];
              }
            }
          }
        }
      }
      PHP(0)
      __syncthreads();                                            // ws / xs complete (barrier A)
      // independent accumulation chains (tile i, parity of r), summed in a fixed order
      floatx4 acc[RAW_TPW][2];
#pragma unroll
      for (int i = 0; i < RAW_TPW; ++i) acc[i][0] = acc[i][1] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < RAW_KP / 16; ++u) {
        if (16 * u >= X) break;                                   // uniform
        const floatx4 xv = *reinterpret_cast<const floatx4*>(xs + lr * RAW_KP + 16 * u + 4 * lq);
#pragma unroll
        for (int i = 0; i < RAW_TPW; ++i) {
          const int ct = cw + 4 * i;
          if (16 * ct < C) {
            const int c = 16 * ct + lr;
            const floatx4 wv = *reinterpret_cast<const floatx4*>(ws + (c < C ? c : 0) * RAW_KP + 16 * u + 4 * lq);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r & 1] = mfma4(wv[r], xv[r], acc[i][r & 1]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < RAW_TPW; ++i) {
        const int ct = cw + 4 * i;
        if (16 * ct < C) {                                        // uniform
          floatx4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int cc = 16 * ct + 4 * lq + r;
            o[r] = cc < C ? (acc[i][0][r] + acc[i][1][r]) + (R.bf ? hb[i][r] : 0.f) : 0.f;
          }
          *reinterpret_cast<floatx4*>(hs + lr * raw_hs_pitch(C) + 16 * ct + 4 * lq) = o;
        }
      }
      PHB(0)
      __syncthreads();                                            // hs complete (barrier B)
      PHB(1)
      if (R.ydst && b < B) {                                      // the gathered y rows for the backward
        if (j < Da) R.ydst[b * D + j] = ya;
        if (j < Db) R.ydst[b * D + Da + j] = yb;
      }
    } else {
      ya = (j < Da) ? y[bc * D + j] : 0.f;
      yb = (j < Db) ? y[bc * D + Da + j] : 0.f;
      ldc = pk[L.ldc_off];
    }
    __syncthreads();
    // block k + 1's head: record floats [0, FWD_HEAD), the four projection partials, the dropout multipliers
    constexpr int HEAD_END = RecF<NH>::head_end(BC);            // (BC: W1's last quad is dead)
    float hd[FWD_HEAD], hq4[4];
    floatx4 mk0 = {1.f, 1.f, 1.f, 1.f}, mk1 = {1.f, 1.f, 1.f, 1.f};
    auto fetch_head = [&](int sl) {
      ld_rec<0, HEAD_END>(hd, rec + sl * RING + j * L.RF);
      const float* hq = hpb + sl * 1024 + 16 * s + j;            // [sample][neuron] partial tiles
#pragma unroll
      for (int i = 0; i < 4; ++i) hq4[i] = hq[256 * i];
      if (DROP) {
        mk0 = mkb[(2 * sl) * BCNF_WG + tid];
        mk1 = mkb[(2 * sl + 1) * BCNF_WG + tid];
      }
    };
    fetch_head(0);
    float ldj = 0.f;
    int cur = 0;
    // activation-record destinations, advanced per block: nothing in the loop reads the grid size (hipcc reloaded
    // it from the kernarg segment after every barrier's memory clobber, and that scalar load in flight turned the
    // next LDS wait into lgkmcnt(0))
    int gdim = gridDim.x;
    asm volatile("" : "+s"(gdim));
    floatx4* d4 = reinterpret_cast<floatx4*>(arec) + (long long)blockIdx.x * AR::AR4 * BCNF_WG + tid;
    float* d1p = arec + ar1_off(nb, gdim, AR::AR4) + (long long)blockIdx.x * AR::AR1 * BCNF_WG + tid;
    const long long d4s = (long long)gdim * AR::AR4 * BCNF_WG, d1s = (long long)gdim * AR::AR1 * BCNF_WG;
    for (int k = 0; k < nb; ++k) {
      const int nxt = cur == FWD_SLOTS - 1 ? 0 : cur + 1;
      float rr[RecF<NH>::USED];
#pragma unroll
      for (int i = 0; i < HEAD_END; ++i) rr[i] = hd[i];
      const float hpk = ((hq4[0] + hq4[1]) + hq4[2]) + hq4[3];
      const float msk[8] = {mk0[0], mk0[1], mk0[2], mk0[3], mk1[0], mk1[1], mk1[2], mk1[3]};
      const float xa = fmaf(rr[0], ya, rr[1]);          // ActNorm (cnf.py:349)
      const float xb = fmaf(rr[2], yb, rr[3]);
      float T, Sp;
      float ar[AR::AR];                                   // activation record of this block (SAVE)
      ar[AR::YA] = ya;
      ar[AR::YB] = yb;
      // each float4 of the record is stored as soon as it is complete (coalesced across the wave), written through
      // (sc1): the 132 MB of records never sit dirty in the L2s, whose write-back the kernel's end would otherwise
      // wait for (r05: k_forward 55.3 -> 51.5 us, step -1.7 %, profiles/r05zl_ab_write_through_records.txt)
      auto emit = [&](int q) {
        if (SAVE) st4_wt(d4 + q * BCNF_WG, floatx4{ar[4 * q], ar[4 * q + 1], ar[4 * q + 2], ar[4 * q + 3]});
      };
      mlp_forward_s<NH, SAVE, DROP, BC>(rr, rec + cur * RING + j * L.RF, xa, hpk, msk, T, Sp, ar, emit);
      const float Sv = tanh_bf(Sp);                      // cnf.py:107
      const float zb = fmaf(exp_fast(Sv), xb, T);        // cnf.py:179
      ldj += Sv;                                         // cnf.py:190
      if (SAVE) {
        ar[AR::S] = Sv;
#pragma unroll
        for (int q = 0; q < AR::AR4; ++q)
          if (AR::ready_layer(q) == NH + 1) emit(q);
#pragma unroll
        for (int i = 0; i < AR::AR1; ++i) st1_wt(d1p + i * BCNF_WG, ar[4 * AR::AR4 + i]);
        d4 += d4s;
        d1p += d1s;
      }
      fetch_head(nxt);     // slot nxt is complete since the previous barrier (after the last block: unused, no
                           // branch); the reads land while the mix runs
      if constexpr (BC) mix_bc(rr + RecF<NH>::Q, xa, zb, ya, yb);   // y @ Q (cnf.py:335); identity after the last block
      else mix(rr + RecF<NH>::Q, xa, zb, ya, yb);
      cur = nxt;
      PHF(1)
      // a bare barrier: the head reads stay in flight across it (nobody writes slot nxt in the next interval; the
      // helpers write slot k % 3, whose reads this block's compute has consumed), so the wait for them lands on
      // their first use in block k + 1, not here
      asm volatile("s_barrier" ::: "memory");
      PHF(2)
    }
    if constexpr (RAW) ldc = ((lps[0] + lps[1]) + lps[2]) + lps[3];
    const float ltot = row_sum16(ldj) + ldc;
    const float q2 = row_sum16(ya * ya + yb * yb);
    if (j < Da) z[bc * D + j] = ya;
    if (j < Db) z[bc * D + Da + j] = yb;
    if (j == 0 && ldj_out) ldj_out[bc] = ltot;
    if (logp && j == 0) logp[bc] = -(0.5f * q2 - ltot) - 0.5f * (float)D * 1.8378770664093454836f;
    if (nll_part && j == 0) rec[s] = (b < B) ? 0.5f * q2 - ltot : 0.f;   // rec: free after the last barrier
  }
#if BCNF_STAMPS
  if (SAVE && blockIdx.x == 0 && (threadIdx.x == 0 || threadIdx.x == BCNF_WG))
  {
    for (int i = 0; i < 3; ++i) g_phase[8 + (helper ? 4 : 0) + i] = ph_acc[i];
    g_phase[helper ? 15 : 11] = (ph_b[1] << 32) | (ph_b[0] & 0xffffffffULL);   // slots 3 / 7 belong to the backward
    for (int i = 0; i < 4; ++i) g_phase[16 + (helper ? 4 : 0) + i] = ph_p[i];
    // the wave's whole life in shader cycles and in 100 MHz ticks: the clock it ran at (MI355X_MICROARCH note 6)
    g_phase[24 + (helper ? 2 : 0)] = __builtin_amdgcn_s_memtime() - ph_t0;
    g_phase[25 + (helper ? 2 : 0)] = __builtin_amdgcn_s_memrealtime() - ph_r0;
  }
#endif
#undef PHF
#undef PHB
#undef PHP
  if (nll_part) {   // per-workgroup partial of inn_nll_loss (utils.py:40-46); reduced by nll_finalize
    __syncthreads();
    if (threadIdx.x == 0) {
      float acc = 0.f;
      for (int i = 0; i < 16; ++i) acc += rec[i];
      nll_part[blockIdx.x] = acc;
    }
  }
}

__global__ __launch_bounds__(BCNF_WG) void k_nll_finalize(const float* __restrict__ part, int nparts, long long B,
                                                          float* __restrict__ loss_out, uint64_t* rng_w,
                                                          int32_t* guard) {
  __shared__ float red[BCNF_WG];
  nll_finalize(part, nparts, B, loss_out, rng_w, guard, red);
}

}  // namespace

namespace bcnf_small {

int launch_forward(const BcnfLayout& L, const float* pk, const float* y, const float* h, const float* fold, int X,
                   int ldx, long long B, float* z, float* ldj, float* logp, bool drop, const uint64_t* rng,
                   float* arec, float* part, const RawForward* raw, hipStream_t st) {
  const BcnfLayout Lp = fold ? fold_layout(L, X, ldx) : L;
  const float* pbase = fold ? fold : pk;
  const ProjArgs P{h, pbase + Lp.w1c_off, pbase + Lp.b1c_off, (long long)Lp.ldh, Lp.C, Lp.Cp, Lp.NKp};
  const dim3 grid((unsigned)((B + 15) / 16));
  const size_t lds = fwd2_lds_bytes(L, raw != nullptr);
  const bool save = arec != nullptr;
  const RawArgs R = raw ? RawArgs{*raw} : RawArgs{};
  return dispatch_nh(L.NH, [&](auto nh) -> int {
    constexpr int NH = decltype(nh)::value;
    if (!layout_matches<NH>(L)) return BCNF_ERR_ARG;
    if (P.Cp % 16 != 0 || P.Cp / 16 > HP_SMAX || P.C > P.Cp) return BCNF_ERR_UNSUPPORTED;
    // the six instantiations that exist per record form: the pack-free forward always saves (k_forward<NH, *, false,
    // true, *> is none)
#define FWD1(DR, SV, RW, BC) \
  launch<k_forward<NH, DR, SV, RW, BC>>(grid, dim3(2 * BCNF_WG), lds, st, L, pk, y, P, B, z, ldj, logp, rng, arec, part, R)
#define FWD(DR, SV, RW) (layout_bc(L) ? FWD1(DR, SV, RW, true) : FWD1(DR, SV, RW, false))
    if (raw) return !save ? BCNF_ERR_ARG : drop ? FWD(true, true, true) : FWD(false, true, true);
    if (save) return drop ? FWD(true, true, false) : FWD(false, true, false);
    return drop ? FWD(true, false, false) : FWD(false, false, false);
#undef FWD
#undef FWD1
  });
}

int launch_nll_finalize(const float* part, int nparts, long long B, float* loss_out, uint64_t* rng_w, int32_t* guard,
                        hipStream_t st) {
  return launch<k_nll_finalize>(dim3(1), dim3(BCNF_WG), 0, st, part, nparts, B, loss_out, rng_w, guard);
}

#if BCNF_STAMPS
int fwd_debug_phases(unsigned long long* out) {
  return bcnf_rt::hip_status(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(g_phase)));
}
#endif

}  // namespace bcnf_small
