// bcnf_amd: fused CondRealNVP_v2 coupling stack for MI355X (gfx950 / CDNA4).
//
// The small stack family (widths <= 16, all fp32), one file per kernel family:
//   bcnf_stack.hip         this file: the family's C ABI (argument checks, then one launcher per family), and the
//                          pack side -- k_pack / k_pack_fold (canonical nn.Module parameters -> per-lane LDS records,
//                          the ActNorm log|det| constant, the folded feature Linear), the pack-free forward's table
//   bcnf_stack_fwd.hip     k_forward: ActNorm -> nested MLP (GELU, dropout) -> affine coupling -> log-det ->
//                          orthonormal mix, all n_blocks in one launch (cnf.py:476-488); k_nll_finalize
//   bcnf_stack_inv.hip     k_hp, k_inverse (training mode), k_inverse_mfma (eval)              (cnf.py:499-506)
//   bcnf_stack_bwd.hip     k_backward: from the forward's activation records, dW via fp32 MFMA into per-workgroup slabs
//   bcnf_stack_tail.hip    deterministic slab sum and the projection GEMMs -> canonical flat gradient, unfolded and
//                          folded (with the fused Adam)
//   bcnf_stack_layout.h    shared constants and the host layout; bcnf_stack_rec.h the kernels' shared device pieces;
//   bcnf_stack_internal.h  the launchers the ABI calls
//
// Reference: psaegert/bcnf src/bcnf/models/cnf.py. See DESIGN.md for layouts and rooflines.
#include "bcnf_stack_internal.h"
#include "bcnf_stack_rec.h"

#include <utility>
#include <vector>

namespace {
using namespace bcnf_small;
using bcnf_rt::launch;

// ------------------------------------------------------------------------------------------------
// Packing
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cW(const BcnfLayout& L, const float* P, int k, int l, int row, int col) {
  return P[coupling_base(L, k) + L.lin_w[l] + row * L.lin_in[l] + col];
}
__device__ __forceinline__ float cB(const BcnfLayout& L, const float* P, int k, int l, int row) {
  return P[coupling_base(L, k) + L.lin_b[l] + row];
}

// Input index of record entry r of lane j in a matvec section: rotation form (r-th rotation: input (j - r) & 15) or,
// with L.qbc's bit for the section (QBC_*), broadcast form (entry r = input r; bc10 / bc9x2 / mix_bc).
__host__ __device__ inline int rec_src(const BcnfLayout& L, int j, int r, int bit) {
  return (L.qbc & bit) ? r : ((j - r) & 15);
}

// Entry c (0..63) of lane j of a mix section -> (quadrant qi: 0 a->a, 1 b->a, 2 a->b, 3 b->b, input src of the
// quadrant's input half); false: a padding entry. Rotation form: 16 entries per quadrant; broadcast form (mix_bc):
// entries [0, D) feed output half a, [D, 2D) half b, each over the D inputs (a's Da first, then b's Db).
__host__ __device__ inline bool q_entry(const BcnfLayout& L, int j, int c, int* qi, int* src) {
  if (!(L.qbc & QBC_MIX)) {
    *qi = c / 16;
    *src = (j - c % 16) & 15;
    return true;
  }
  const int D = L.D;
  if (c >= 2 * D) return false;
  const int oh = c / D, gi = c % D;
  *qi = 2 * oh + (gi < L.Da ? 0 : 1);
  *src = gi < L.Da ? gi : gi - L.Da;
  return true;
}

// The mix weight of quadrant qi from input src (of its input half) to output lane j (of its output half) in block k:
// y_new = y @ Q (cnf.py:335) or, inverse, z_prev = y @ Q^T (cnf.py:339); the identity after the last block (no mix),
// so the kernels need no branch.
__device__ float q_quad(const BcnfLayout& L, const float* Q, int k, int j, int qi, int src, bool inverse) {
  const int Da = L.Da, Db = L.Db, D = L.D;
  const int no = (qi < 2) ? Da : Db, ni = (qi & 1) ? Db : Da;   // output / input half widths
  if (j >= no || src >= ni) return 0.f;
  if (k >= L.nb - 1) return ((qi == 0 || qi == 3) && src == j) ? 1.f : 0.f;
  const float* q = Q + (long long)k * D * D;
  const int gi = (qi & 1) ? Da + src : src, go = (qi < 2) ? j : Da + j;   // global input / output index
  return inverse ? q[go * D + gi] : q[gi * D + go];
}

// PF (inverse=false) / PI (inverse=true) record entry e of lane j in block k.
__device__ float rec_f(const BcnfLayout& L, const float* P, const float* Q, int k, int j, int e, bool inverse) {
  const int Da = L.Da, Db = L.Db, D = L.D, NH = L.NH;
  const bool has_an = L.act_norm && k < L.nb - 1;
  const int anb = k * L.blk_stride;
  if (e < 4) {   // ActNorm scale / bias; the inverse record holds 1 / scale (the inverse multiplies, no fp32 divide)
    switch (e) {
      case 0: return (j < Da) ? (has_an ? (inverse ? 1.f / P[anb + j] : P[anb + j]) : 1.f) : 0.f;
      case 1: return (j < Da && has_an) ? P[anb + D + j] : 0.f;
      case 2: return (j < Db) ? (has_an ? (inverse ? 1.f / P[anb + Da + j] : P[anb + Da + j]) : 1.f) : 0.f;
      default: return (j < Db && has_an) ? P[anb + D + Da + j] : 0.f;
    }
  }
  if (e == L.rf_b1) return (j < L.H[1]) ? cB(L, P, k, 1, j) : 0.f;
  if (e >= L.rf_w1 && e < L.rf_w1 + 16) {
    const int src = rec_src(L, j, e - L.rf_w1, QBC_W1);
    return (j < L.H[1] && src < Da) ? cW(L, P, k, 1, j, src) : 0.f;
  }
  if (e >= L.rf_hid && e < L.rf_t) {
    const int l = 2 + (e - L.rf_hid) / 17, r = (e - L.rf_hid) % 17;
    if (r == 16) return (j < L.H[l]) ? cB(L, P, k, l, j) : 0.f;
    const int src = (j - r) & 15;
    return (j < L.H[l] && src < L.H[l - 1]) ? cW(L, P, k, l, j, src) : 0.f;
  }
  if (e >= L.rf_t && e < L.rf_t + 34) {
    const int half = (e - L.rf_t) / 17, r = (e - L.rf_t) % 17;   // half 0: t rows, 1: s rows
    if (r == 16) return (j < Db) ? cB(L, P, k, NH + 1, half * Db + j) : 0.f;
    const int src = (j - r) & 15;
    return (j < Db && src < L.H[NH]) ? cW(L, P, k, NH + 1, half * Db + j, src) : 0.f;
  }
  if (e >= L.rf_q && e < L.rf_q + 64) {
    int qi, src;
    if (!q_entry(L, j, e - L.rf_q, &qi, &src)) return 0.f;
    return q_quad(L, Q, k, j, qi, src, inverse);
  }
  return 0.f;
}

// PB record entry (transposed weight rows for the backward).
__device__ float rec_b(const BcnfLayout& L, const float* P, const float* Q, int k, int j, int e) {
  const int NH = L.NH, Db = L.Db;
  if (e >= L.rb_w1t && e < L.rb_w1t + 16) {
    const int src = (j - (e - L.rb_w1t)) & 15;
    return (j < L.Da && src < L.H[1]) ? cW(L, P, k, 1, src, j) : 0.f;
  }
  if (e >= L.rb_hid && e < L.rb_w1t) {
    const int l = NH - (e - L.rb_hid) / 16, r = (e - L.rb_hid) % 16, src = (j - r) & 15;
    return (j < L.H[l - 1] && src < L.H[l]) ? cW(L, P, k, l, src, j) : 0.f;
  }
  if (e >= L.rb_tt && e < L.rb_tt + 32) {
    const int half = (e - L.rb_tt) / 16, src = rec_src(L, j, (e - L.rb_tt) % 16, QBC_HEAD);
    return (j < L.H[NH] && src < Db) ? cW(L, P, k, NH + 1, half * Db + src, j) : 0.f;
  }
  if (e >= L.rb_qt && e < L.rb_qt + 64) return rec_f(L, P, Q, k, j, L.rf_q + (e - L.rb_qt), true);
  if (e >= L.rb_an && e < L.rb_an + 4) return rec_f(L, P, Q, k, j, e - L.rb_an, false);
  return 0.f;
}

// Matrix-core inverse record of block k in MFMA A-operand order, entry e (k_inverse_mfma): matrix m's lane l = (q, s)
// reads ONE float4 at m * 256 + 4 l -- its A operands of the layer's 4 K-steps t -- instead of 4 scalar reads of the
// row-layout inverse record at lane-dependent offsets (bank conflicts: DESIGN 3e). Values are PI-record entries
// (rec_f, inverse = true): m = 0..3 the mix quadrants qi (half -> half), 4 Linear 1 (half -> hidden), 5 .. NH + 3
// the hidden layers, NH + 4 / NH + 5 the T / S heads (hidden -> half). PERM (D_a, D_b <= 12): half-vector feature
// 3q + r in register r < 3; rows with no feature read lane 15's zero entry.
__device__ float rec_pm(const BcnfLayout& L, const float* P, const float* Q, int k, int e) {
  const int NH = L.NH, nm = NH + 6;
  const bool perm = L.Da <= 12 && L.Db <= 12;
  auto feat = [&](int q, int r) { return perm ? (r < 3 ? 3 * q + r : 15) : 4 * q + r; };
  if (e < nm * 256) {
    const int m = e >> 8, l = (e >> 2) & 63, t = e & 3, q = l >> 4, s = l & 15;
    const bool none = perm && (s & 3) == 3;
    const int fo = perm ? 3 * (s >> 2) + (s & 3) : s;
    const int ch = perm ? 3 * q + t : 4 * q + t, cu = 4 * q + t;
    if (m < 4) {                                                           // mix quadrant qi = m
      if (perm && t == 3) return 0.f;
      return none ? 0.f : q_quad(L, Q, k, fo, m, ch, true);
    }
    if (m == 4) {                                                          // Linear 1, y-part
      if (perm && t == 3) return 0.f;
      return (s < L.H[1] && ch < L.Da) ? cW(L, P, k, 1, s, ch) : 0.f;
    }
    if (m < NH + 4) return rec_f(L, P, Q, k, s, L.rf_hid + 17 * (m - 5) + ((s - cu) & 15), true);
    const int off = (m == NH + 4) ? L.rf_t : L.rf_s;
    return none ? rec_f(L, P, Q, k, 15, off, true) : rec_f(L, P, Q, k, fo, off + ((fo - cu) & 15), true);
  }
  e -= nm * 256;
  if (e < (NH - 1) * 16) {                                                 // hidden biases, row 4q + r
    const int h = e >> 4, q = (e >> 2) & 3, r = e & 3;
    return rec_f(L, P, Q, k, 4 * q + r, L.rf_hid + 17 * h + 16, true);
  }
  e -= (NH - 1) * 16;
  if (e < 32) {                                                            // T / S biases, row feat(q, r)
    const int half = e >> 4, q = (e >> 2) & 3, r = e & 3;
    return rec_f(L, P, Q, k, feat(q, r), (half ? L.rf_s : L.rf_t) + 16, true);
  }
  e -= 32;                                                                 // ActNorm inverse [1/sa ba 1/sb bb]
  const int q = e >> 4, r = (e >> 2) & 3, i = e & 3;
  return rec_f(L, P, Q, k, feat(q, r), i, true);
}

// ------------------------------------------------------------------------------------------------
// Pack-free training forward (bcnf_fold_train_forward, round 4): the forward's helper waves build each block's
// forward record straight from the canonical parameters instead of reading a packed copy, so the folded training
// step needs no pack launch. The record entries of a block k < nb - 1 that are not structurally zero are each one
// parameter at a block-independent offset from k * blk_stride (ActNorm, coupling Linears) or from k * D * D
// (the orthonormal mix); RawTable lists them once per layout, split into P-sourced and Q-sourced slots of RAW_NP /
// RAW_NQ entries per helper thread (padding entries copy parameter 0 into an unused word of the ring slot), so a
// helper thread gathers its entries with block-uniform base pointers and never branches. The zero entries stay zero
// in the LDS ring (zeroed once); the last block (no ActNorm, identity mix) goes through rec_f itself.
// ------------------------------------------------------------------------------------------------

// Source of mix-section entry c of lane j (q_entry / q_quad): kind 2 (qmats at k * D * D + off) or 0 (zero).
int q_quad_source(const BcnfLayout& L, int j, int c, bool inverse, int* off) {
  int qi, src;
  if (!q_entry(L, j, c, &qi, &src)) return 0;
  const int Da = L.Da, Db = L.Db, D = L.D;
  const int no = (qi < 2) ? Da : Db, ni = (qi & 1) ? Db : Da;
  if (j >= no || src >= ni) return 0;
  const int gi = (qi & 1) ? Da + src : src, go = (qi < 2) ? j : Da + j;
  *off = inverse ? go * D + gi : gi * D + go;
  return 2;
}

// Source of forward-record entry e of lane j for a block k < nb - 1: kind 0 = structurally zero, 1 = params at
// k * blk_stride + off, 2 = qmats at k * D * D + off; -1 = a constant the table cannot express (no ActNorm: 1.0).
// Mirrors rec_f (inverse = false) entry by entry.
int rec_f_source(const BcnfLayout& L, int j, int e, int* off) {
  const int Da = L.Da, Db = L.Db, D = L.D, NH = L.NH, an = L.an_size;
  auto lin_w = [&](int l, int row, int col) { return an + L.lin_w[l] + row * L.lin_in[l] + col; };
  *off = 0;
  if (e < 4) {
    if (!L.act_norm) return ((e == 0 && j < Da) || (e == 2 && j < Db)) ? -1 : 0;
    switch (e) {
      case 0: return j < Da ? (*off = j, 1) : 0;
      case 1: return j < Da ? (*off = D + j, 1) : 0;
      case 2: return j < Db ? (*off = Da + j, 1) : 0;
      default: return j < Db ? (*off = D + Da + j, 1) : 0;
    }
  }
  if (e == L.rf_b1) return j < L.H[1] ? (*off = an + L.lin_b[1] + j, 1) : 0;
  if (e >= L.rf_w1 && e < L.rf_w1 + 16) {
    const int src = rec_src(L, j, e - L.rf_w1, QBC_W1);
    return (j < L.H[1] && src < Da) ? (*off = lin_w(1, j, src), 1) : 0;
  }
  if (e >= L.rf_hid && e < L.rf_t) {
    const int l = 2 + (e - L.rf_hid) / 17, r = (e - L.rf_hid) % 17;
    if (r == 16) return j < L.H[l] ? (*off = an + L.lin_b[l] + j, 1) : 0;
    const int src = (j - r) & 15;
    return (j < L.H[l] && src < L.H[l - 1]) ? (*off = lin_w(l, j, src), 1) : 0;
  }
  if (e >= L.rf_t && e < L.rf_t + 34) {
    const int half = (e - L.rf_t) / 17, r = (e - L.rf_t) % 17;
    if (r == 16) return j < Db ? (*off = an + L.lin_b[NH + 1] + half * Db + j, 1) : 0;
    const int src = (j - r) & 15;
    return (j < Db && src < L.H[NH]) ? (*off = lin_w(NH + 1, half * Db + j, src), 1) : 0;
  }
  if (e >= L.rf_q && e < L.rf_q + 64) return q_quad_source(L, j, e - L.rf_q, false, off);
  return 0;
}

// Source of backward-record entry e of lane j for a block k < nb - 1 (mirrors rec_b): kinds as rec_f_source.
int rec_b_source(const BcnfLayout& L, int j, int e, int* off) {
  const int NH = L.NH, Da = L.Da, Db = L.Db, D = L.D, an = L.an_size;
  auto lin_w = [&](int l, int row, int col) { return an + L.lin_w[l] + row * L.lin_in[l] + col; };
  *off = 0;
  if (e >= L.rb_w1t && e < L.rb_w1t + 16) {
    const int src = (j - (e - L.rb_w1t)) & 15;
    return (j < Da && src < L.H[1]) ? (*off = lin_w(1, src, j), 1) : 0;
  }
  if (e >= L.rb_hid && e < L.rb_w1t) {
    const int l = NH - (e - L.rb_hid) / 16, r = (e - L.rb_hid) % 16, src = (j - r) & 15;
    return (j < L.H[l - 1] && src < L.H[l]) ? (*off = lin_w(l, src, j), 1) : 0;
  }
  if (e >= L.rb_tt && e < L.rb_tt + 32) {
    const int half = (e - L.rb_tt) / 16, src = rec_src(L, j, (e - L.rb_tt) % 16, QBC_HEAD);
    return (j < L.H[NH] && src < Db) ? (*off = lin_w(NH + 1, half * Db + src, j), 1) : 0;
  }
  if (e >= L.rb_qt && e < L.rb_qt + 64) return q_quad_source(L, j, e - L.rb_qt, true, off);   // Q^T
  if (e >= L.rb_an && e < L.rb_an + 4) return rec_f_source(L, j, e - L.rb_an, off);
  return 0;
}

// Words of the pack-free forward's table: the forward slots [256 threads][RAW_NSP] (a thread's slots contiguous, so
// it loads them with RAW_NSP / 4 16-byte loads), then one block's backward record [16 RB] as (source << 2 | kind)
// with kind 0 params, 1 qmats, 2 zero.
long long raw_table_words(const BcnfLayout& L) { return (long long)RAW_NSP * BCNF_WG + 16LL * L.RB; }

// The table [RAW_NS][BCNF_WG] (P slots, then Q slots, then zero slots) for layout L: every float of a ring slot's
// 16 RF record floats belongs to exactly one (thread, slot), so a helper thread writes its own words and no two
// threads race. Within a kind the entries go in SOURCE order, entry n to slot n / 256, thread n % 256: a wave's
// gather then reads 64 consecutive parameters (the P entries are exactly a block's parameters minus the W1
// condition columns, the Q entries all of Q_k) -- a few cache lines per load instead of one per lane -- and the
// scattered side is the LDS write. Padding entries name RAW_DUMMY. False if the raw path does not apply (no
// ActNorm: constant entries; or more entries of a kind than slots).
bool build_raw_table(const BcnfLayout& L, uint32_t* out) {
  if (L.nb < 2 || 16 * L.RF > RAW_DUMMY || L.blk_stride >= RAW_SRC_MAX) return false;
  std::vector<std::pair<int, int>> ent[3];                  // (src, dst) per kind: P, Q, zero
  for (int j = 0; j < 16; ++j)
    for (int e = 0; e < L.RF; ++e) {
      int off;
      const int kind = rec_f_source(L, j, e, &off);
      if (kind < 0) return false;
      ent[kind == 1 ? 0 : kind == 2 ? 1 : 2].emplace_back(off, j * L.RF + e);
    }
  const int cap[3] = {RAW_NP, RAW_NQ, RAW_NZ}, first[3] = {0, RAW_NP, RAW_NP + RAW_NQ};
  for (int i = 0; i < RAW_NSP * BCNF_WG; ++i) out[i] = raw_entry(RAW_DUMMY, 0);
  if (L.an_size > BCNF_WG) return false;                     // the ActNorm words (smallest sources) in P slot 0
  for (int g = 0; g < 3; ++g) {
    if ((int)ent[g].size() > cap[g] * BCNF_WG) return false;
    std::sort(ent[g].begin(), ent[g].end());
    for (int n = 0; n < (int)ent[g].size(); ++n)
      out[(n % BCNF_WG) * RAW_NSP + first[g] + n / BCNF_WG] = raw_entry(ent[g][n].second, ent[g][n].first);
  }
  uint32_t* pb = out + (long long)RAW_NSP * BCNF_WG;
  for (int j = 0; j < 16; ++j)
    for (int e = 0; e < L.RB; ++e) {
      int off;
      const int kind = rec_b_source(L, j, e, &off);
      if (kind < 0 || off >= (1 << 29)) return false;
      pb[j * L.RB + e] = ((uint32_t)off << 2) | (uint32_t)(kind == 1 ? 0 : kind == 2 ? 1 : 2);
    }
  return true;
}

// Grid: 1 workgroup that computes the ActNorm log|det| constant  sum_k sum_i log|scale_k,i|  (cnf.py:350) in a
// fixed order, then npw record workgroups (grid-stride over every packed float; pack_wgs gives every thread about
// one element, so the launch is one load round trip, not a chain of them).
constexpr int PACK_WG_MAX = 4096;

// train_only (the folded training step, bcnf_pack_params_fold): only what its forward, backward and tail read --
// PF, PB, W1hR and the log-det constant -- not the inverse records PI / PM (the costliest entries: rec_pm calls
// rec_f per element) nor the unfolded projection's W1hC / b1c: about half the elements of a full pack.
__device__ __forceinline__ void pack_body(const BcnfLayout& L, const float* __restrict__ P,
                                          const float* __restrict__ Q, float* __restrict__ out, int bx, int npw,
                                          float* __restrict__ part, bool train_only = false) {
  if (bx == 0) {
    float acc = 0.f;
    if (L.act_norm) {
      const int n = (L.nb - 1) * L.D;
      for (int i = threadIdx.x; i < n; i += BCNF_WG) {
        const int k = i / L.D, d = i - k * L.D;
        acc += logf(fabsf(P[k * L.blk_stride + d]));
      }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = BCNF_WG / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[L.ldc_off] = part[0];
    return;
  }
  // every packed section is < 2^31 floats (layout_supported bounds the shapes), so 32-bit index math
  const int n_pf = L.nb * 16 * L.RF;
  const int n_pb = L.nb * 16 * L.RB;
  const int n_w = L.Cp * L.NKp;                       // each of W1hC, W1hR
  const int n_pm = L.nb * L.PMB;
  const int total = train_only ? n_pf + n_pb + n_w : 2 * n_pf + n_pb + 2 * n_w + L.NKp + n_pm;
  for (int ii0 = (bx - 1) * BCNF_WG + threadIdx.x; ii0 < total; ii0 += npw * BCNF_WG) {
    float v;
    long long o;
    // train_only: [PF | PB | W1hR] mapped onto the full pack's index space (PI and W1hC skipped)
    const int i = (train_only && ii0 >= n_pf + n_pb) ? ii0 + n_pf + n_w : ii0;
    if (i < n_pf) {                                   // PF
      const int kj = i / L.RF, e = i - kj * L.RF;
      v = rec_f(L, P, Q, kj >> 4, kj & 15, e, false);
      o = L.pf_off + i;
    } else if (i < n_pf + n_pb) {                     // PB
      const int ii = i - n_pf;
      const int kj = ii / L.RB, e = ii - kj * L.RB;
      v = rec_b(L, P, Q, kj >> 4, kj & 15, e);
      o = L.pb_off + ii;
    } else if (i < 2 * n_pf + n_pb) {                 // PI
      const int ii = i - n_pf - n_pb;
      const int kj = ii / L.RF, e = ii - kj * L.RF;
      v = rec_f(L, P, Q, kj >> 4, kj & 15, e, true);
      o = L.pi_off + ii;
    } else if (i < 2 * n_pf + n_pb + n_w) {           // W1hC [c][kj]
      const int ii = i - 2 * n_pf - n_pb;
      const int c = ii / L.NKp, kj = ii - c * L.NKp, k = kj >> 4, j = kj & 15;
      v = (k < L.nb && j < L.H[1] && c < L.C) ? cW(L, P, k, 1, j, L.Da + c) : 0.f;
      o = L.w1c_off + ii;
    } else if (i < 2 * n_pf + n_pb + 2 * n_w) {       // W1hR [kj][c]
      const int ii = i - 2 * n_pf - n_pb - n_w;
      const int kj = ii / L.Cp, c = ii - kj * L.Cp, k = kj >> 4, j = kj & 15;
      v = (k < L.nb && j < L.H[1] && c < L.C) ? cW(L, P, k, 1, j, L.Da + c) : 0.f;
      o = L.w1r_off + ii;
    } else if (i < 2 * n_pf + n_pb + 2 * n_w + L.NKp) {   // b1c [kj]
      const int kj = i - 2 * n_pf - n_pb - 2 * n_w, k = kj >> 4, j = kj & 15;
      v = (k < L.nb && j < L.H[1]) ? cB(L, P, k, 1, j) : 0.f;
      o = L.b1c_off + kj;
    } else {                                          // PM (matrix-core inverse, operand order)
      const int ii = i - 2 * n_pf - n_pb - 2 * n_w - L.NKp;
      const int k = ii / L.PMB, e = ii - k * L.PMB;
      v = rec_pm(L, P, Q, k, e);
      o = L.pm_off + ii;
    }
    out[o] = v;
  }
}

__global__ __launch_bounds__(BCNF_WG) void k_pack(BcnfLayout L, const float* __restrict__ P,
                                                  const float* __restrict__ Q, float* __restrict__ out, int npw) {
  __shared__ float part[BCNF_WG];
  pack_body(L, P, Q, out, blockIdx.x, npw, part);
}

// Record workgroups of a pack launch (the log-det workgroup not included).
int pack_wgs(const BcnfLayout& L, bool train_only = false) {
  const long long total = train_only ? (long long)L.nb * 16 * (L.RF + L.RB) + (long long)L.Cp * L.NKp
                                     : 2LL * L.nb * 16 * L.RF + (long long)L.nb * 16 * L.RB + 2LL * L.Cp * L.NKp +
                                           L.NKp + (long long)L.nb * L.PMB;
  const long long w = (total + BCNF_WG - 1) / BCNF_WG;
  return (int)(w < PACK_WG_MAX ? (w > 0 ? w : 1) : PACK_WG_MAX);
}

// ------------------------------------------------------------------------------------------------
// Folded linear feature network (training fast path when the feature stack is ONE nn.Linear,
// feature_network.py:114-145 with sizes [X, C] — trajectory_FC_small). h = x Wf^T + bf reaches the stack
// only through the condition projection, so with kj = k*16 + j and W1h_k[j][c] = W1_k[j][Da + c]:
//   HP[k][r][j] = sum_xc x[r][xc] Wc[xc][kj] + bc[kj],  Wc[xc][kj] = sum_c W1h_k[j][c] Wf[c][xc],
//                                                       bc[kj]     = b1_k[j] + sum_c W1h_k[j][c] bf[c]
// and with Gx[kj][xc] = sum_b D1[k][b][j] x1[b][xc]  (x1 = [x | 1], D1 = dL/d pre-activation of Linear 1):
//   dW1h_k[j][c] = sum_{xc<X} Gx[kj][xc] Wf[c][xc] + Gx[kj][X] bf[c]
//   dWf[c][xc]   = sum_kj W1h_k[j][c] Gx[kj][xc],       dbf[c] = sum_kj W1h_k[j][c] Gx[kj][X]
// h and dL/dh are never formed: the feature Linear's forward GEMM, the dL/dh GEMM and the feature dW split-K
// disappear from the step (same sums, reassociated: fp32 rounding differs from the unfolded path at ~1e-6).
// The fold buffer: Wc [Xp][NKp] then bc [NKp], Xp = 16-multiple > X (row X, the ones column, is zero).
// ------------------------------------------------------------------------------------------------

// Fold workgroup f: block k = f / 4, rows j0 = 4 (f % 4) .. j0 + 3; thread xc < Xp computes column xc of
// W1h_k[j0:j0+4] [Wf | bf | 0]: Wc[xc][kj] for xc < X, the bias dot for xc == X, zero rows X..Xp-1. One staging
// round trip (the 4 W1h rows, [c][4] in LDS, read as broadcast float4), then C independent L2-resident loads of Wf
// per thread, coalesced across the lanes.
constexpr int FOLD_SPLIT = 4;

__device__ __forceinline__ void fold_body(const BcnfLayout& L, const float* __restrict__ P,
                                          const float* __restrict__ wf, const float* __restrict__ bf, int X,
                                          float* __restrict__ fold, int f, float* __restrict__ w1s) {
  const int Xp = fold_xp(X), k = f / FOLD_SPLIT, j0 = (f % FOLD_SPLIT) * 4, tid = threadIdx.x;
  const bool kval = k < L.nb;
  for (int i = tid; i < 4 * L.C; i += BCNF_WG) {
    const int c = i >> 2, jj = i & 3, j = j0 + jj;
    w1s[i] = (kval && j < L.H[1]) ? cW(L, P, k, 1, j, L.Da + c) : 0.f;
  }
  __syncthreads();
  if (tid >= Xp) return;
  const int xc = tid;
  const bool isw = xc < X, live = isw || (xc == X && bf != nullptr);
  const float* src = isw ? wf + xc : bf;
  const int stride = isw ? X : 1;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int c = 0; c < L.C; ++c) {
    const float v = live ? src[(long long)c * stride] : 0.f;
    const floatx4 w = *reinterpret_cast<const floatx4*>(w1s + 4 * c);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) acc[jj] = fmaf(w[jj], v, acc[jj]);
  }
  const int kj = k * 16 + j0;
  if (xc == X) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = j0 + jj;
      fold[(long long)Xp * L.NKp + kj + jj] = (kval && j < L.H[1]) ? cB(L, P, k, 1, j) + acc[jj] : 0.f;
    }
    acc = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  *reinterpret_cast<floatx4*>(fold + (long long)xc * L.NKp + kj) = acc;
}

// NKp / 4 fold workgroups first (they start before the record workgroups), then the optional batch gather's
// workgroups (the step's batch feed: independent of the pack), then k_pack's grid. The fold reads the canonical
// parameters, not k_pack's output.
__global__ __launch_bounds__(BCNF_WG) void k_pack_fold(BcnfLayout L, const float* __restrict__ P,
                                                       const float* __restrict__ Q, float* __restrict__ out,
                                                       const float* __restrict__ wf, const float* __restrict__ bf,
                                                       int X, float* __restrict__ fold, BcnfGatherArgs ga, int npw) {
  __shared__ __attribute__((aligned(16))) float smem[4 * 16 * NC16_MAX];
  const int n_fold = L.NKp / 16 * FOLD_SPLIT;
  int bx = blockIdx.x;
  if (bx < n_fold) {
    fold_body(L, P, wf, bf, X, fold, bx, smem);
    return;
  }
  bx -= n_fold;
  if (bx < ga.nwg) {
    gather2_rows(ga.idx, ga.n, ga.rpw, ga.s0, ga.c0, ga.d0, ga.s1, ga.c1, ga.d1, ga.cursor, bx);
    return;
  }
  pack_body(L, P, Q, out, bx - ga.nwg, npw, smem, true);
}

// Test hook: the whole dynamic LDS of the workgroup set to `value` (bcnf_lds_fill).
__global__ __launch_bounds__(BCNF_WG) void k_fill_lds(float value) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  for (int i = threadIdx.x; i < (int)(LDS_MAX / 16); i += BCNF_WG)
    reinterpret_cast<floatx4*>(smem)[i] = floatx4{value, value, value, value};
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// The entries' common bodies
// ------------------------------------------------------------------------------------------------
int forward_impl(const BcnfStackDesc* desc, const void* packed, const float* y, const float* h, int64_t batch,
                 float* z, float* ldj, float* log_prob, int32_t training, const uint64_t* rng_state, void* workspace,
                 bool save, bool nll, bool finalize, float* loss_out, int32_t* guard, void* stream,
                 const float* fold = nullptr, int X = 0, int ldx = 0, const RawForward* raw = nullptr) {
  BcnfLayout L;
  int rc = stack_setup(desc, &L);
  if (rc) return rc;
  if (batch < 0) return BCNF_ERR_ARG;
  if (batch == 0) return nll ? BCNF_ERR_ARG : BCNF_OK;      // the mean over an empty batch is undefined
  if (!packed || !y || !h || !z || !workspace) return BCNF_ERR_ARG;
  if (nll && finalize && !loss_out) return BCNF_ERR_ARG;
  const bool drop = training && L.p > 0.f;
  if (drop && !rng_state) return BCNF_ERR_ARG;
  float* ws = (float*)workspace;
  float* arec = (save || nll) ? ws : nullptr;
  float* part = nll ? ws + ws_part_off(L, batch) : nullptr;
  const float* pk = (const float*)packed;
  hipStream_t st = (hipStream_t)stream;
  rc = launch_forward(L, pk, y, h, fold, X, ldx, batch, z, ldj, log_prob, drop, rng_state, arec, part, raw, st);
  if (rc || !nll || !finalize) return rc;
  return launch_nll_finalize(part, (int)((batch + 15) / 16), batch, loss_out,
                             drop ? const_cast<uint64_t*>(rng_state) : nullptr, guard, st);
}

int backward_impl(const BcnfStackDesc* desc, const void* packed, const float* h, const float* dz, const float* dldj,
                  const float* dloss, int nll, int64_t batch, int32_t training, void* workspace, float* dy,
                  float* dh, float* dparams, void* slab, float* loss_out, uint64_t* rng_state, int32_t* guard,
                  void* stream) {
  BcnfLayout L;
  int rc = stack_setup(desc, &L);
  if (rc) return rc;
  if (batch < 0 || !packed || !h || !workspace || !slab) return BCNF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0) {
    if (dparams) return bcnf_rt::hip_status(hipMemsetAsync(dparams, 0, sizeof(float) * (size_t)L.n_trainable, st));
    return BCNF_OK;
  }
  // `training` must match the forward call that filled the workspace: it says whether dropout masks
  // were saved behind the block inputs.
  const bool drop = training && L.p > 0.f;
  float* ws = (float*)workspace;
  const float* arec = ws;
  float* d1 = ws + ws_d1_off(L, batch);
  const float* pk = (const float*)packed;
  const float* part = ws + ws_part_off(L, batch);
  uint64_t* rng_w = (loss_out && drop) ? rng_state : nullptr;
  rc = launch_backward(L, pk, dz, dldj, dloss, nll, batch, arec, dy, d1, (float*)slab, part, loss_out, rng_w, guard, st);
  if (rc) return rc;
  if (dparams) return launch_tail(L, pk, (const float*)slab, h, ws, batch, dh, dparams, st);
  if (dh) return launch_dh(L, pk, ws, batch, dh, st);
  return BCNF_OK;   // caller finishes with bcnf_backward_tail / bcnf_grad_reduce
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int bcnf_stack_supported(const BcnfStackDesc* desc) {
  BcnfLayout L;
  return stack_setup(desc, &L) == BCNF_OK ? 1 : 0;
}

int bcnf_param_count(const BcnfStackDesc* desc, int64_t* n_trainable, int64_t* n_frozen) {
  BcnfLayout L;
  const int rc = make_layout(desc, &L);
  if (rc) return rc;
  if (n_trainable) *n_trainable = L.n_trainable;
  if (n_frozen) *n_frozen = (int64_t)(L.nb - 1) * L.D * L.D;
  return BCNF_OK;
}

int bcnf_packed_bytes(const BcnfStackDesc* desc, int64_t* bytes) {
  BcnfLayout L;
  const int rc = make_layout(desc, &L);
  if (rc) return rc;
  if (!bytes) return BCNF_ERR_ARG;
  *bytes = (int64_t)L.total * (int64_t)sizeof(float);
  return BCNF_OK;
}

int bcnf_workspace_bytes(const BcnfStackDesc* desc, int64_t batch, int32_t training, int64_t* bytes) {
  BcnfLayout L;
  const int rc = make_layout(desc, &L);
  if (rc) return rc;
  if (!bytes || batch < 0) return BCNF_ERR_ARG;
  *bytes = ws_floats(L, batch) * 4;
  return BCNF_OK;
}

int bcnf_slab_bytes(const BcnfStackDesc* desc, int64_t batch, int64_t* bytes) {
  BcnfLayout L;
  const int rc = make_layout(desc, &L);
  if (rc) return rc;
  if (!bytes || batch < 0) return BCNF_ERR_ARG;
  *bytes = ((int64_t)((batch + 15) / 16) * slab_stride_of(L) + w1h_work_floats(L, batch)) * 4;
  return BCNF_OK;
}

int bcnf_inverse_scratch_bytes(const BcnfStackDesc* desc, int64_t h_rows, int64_t* bytes) {
  BcnfLayout L;
  const int rc = make_layout(desc, &L);
  if (rc) return rc;
  if (!bytes || h_rows < 0) return BCNF_ERR_ARG;
  *bytes = (int64_t)L.nb * h_rows * 16 * 4;
  return BCNF_OK;
}

int bcnf_pack_params(const BcnfStackDesc* desc, const float* params, const float* qmats, void* packed, void* stream) {
  BcnfLayout L;
  const int rc = stack_setup(desc, &L);
  if (rc) return rc;
  if (!params || !packed || (L.nb > 1 && !qmats)) return BCNF_ERR_ARG;
  const int npw = pack_wgs(L);
  return launch<k_pack>(dim3(npw + 1), dim3(BCNF_WG), 0, (hipStream_t)stream, L, params, qmats, (float*)packed, npw);
}

int bcnf_stack_forward(const BcnfStackDesc* desc, const void* packed, const float* y, const float* h, int64_t batch,
                       float* z, float* ldj, float* log_prob, int32_t training, const uint64_t* rng_state,
                       void* workspace, int32_t save, void* stream) {
  return forward_impl(desc, packed, y, h, batch, z, ldj, log_prob, training, rng_state, workspace, save != 0, false,
                      false, nullptr, nullptr, stream);
}

int bcnf_stack_backward(const BcnfStackDesc* desc, const void* packed, const float* h, const float* dz,
                        const float* dldj, int64_t batch, int32_t training, void* workspace, float* dy,
                        float* dh, float* dparams, void* slab, void* stream) {
  return backward_impl(desc, packed, h, dz, dldj, nullptr, 0, batch, training, workspace, dy, dh, dparams, slab,
                       nullptr, nullptr, nullptr, stream);
}

int bcnf_stack_dh(const BcnfStackDesc* desc, const void* packed, const void* workspace, int64_t batch, int32_t training,
                  float* dh, void* stream) {
  BcnfLayout L;
  const int rc = stack_setup(desc, &L);
  if (rc) return rc;
  if (batch < 0 || !packed || !workspace || !dh) return BCNF_ERR_ARG;
  if (batch == 0) return BCNF_OK;
  return launch_dh(L, (const float*)packed, (const float*)workspace, batch, dh, (hipStream_t)stream);
}

int bcnf_backward_tail(const BcnfStackDesc* desc, const void* packed, const void* slab, const float* h,
                       const void* workspace, int64_t batch, int32_t training, float* dh, float* dparams,
                       void* stream) {
  BcnfLayout L;
  const int rc = stack_setup(desc, &L);
  if (rc) return rc;
  if (!packed || !slab || !h || !workspace || !dparams || batch < 1) return BCNF_ERR_ARG;
  return launch_tail(L, (const float*)packed, (const float*)slab, h, (const float*)workspace, batch, dh, dparams,
                     (hipStream_t)stream);
}

// ---- folded linear feature network (see fold_body) ----
int bcnf_fold_bytes(const BcnfStackDesc* desc, int32_t in_features, int64_t* bytes) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!bytes) return BCNF_ERR_ARG;
  *bytes = fold_floats(L, in_features) * 4;
  return BCNF_OK;
}

int bcnf_fold_slab_bytes(const BcnfStackDesc* desc, int32_t in_features, int64_t batch, int64_t* bytes) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!bytes || batch < 0) return BCNF_ERR_ARG;
  const BcnfLayout F = fold_layout(L, in_features, in_features);
  *bytes = ((int64_t)((batch + 15) / 16) * slab_stride_of(L) + w1h_work_floats(F, batch) +
            (int64_t)L.nb * 16 * F.Cp + 4 +                    // + the fused Adam's two scalars (FoldAdamArgs::asc)
            (int64_t)L.C * (in_features + 1)) * 4;             // + k_fold_tail's copy of [Wf | bf]
  return BCNF_OK;
}

int bcnf_pack_params_fold(const BcnfStackDesc* desc, const float* params, const float* qmats,
                          const float* feat_weight, const float* feat_bias, int32_t in_features, void* packed,
                          float* fold, const BcnfGather2* gather, void* stream) {
  BcnfLayout L;
  int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!params || !packed || !fold || !feat_weight || (L.nb > 1 && !qmats)) return BCNF_ERR_ARG;
  BcnfGatherArgs ga = {};
  if (gather) {
    const BcnfGather2& g = *gather;
    if (g.n < 1 || g.cols0 < 1 || g.cols1 < 1 || !g.idx || !g.src0 || !g.dst0 || !g.src1 || !g.dst1)
      return BCNF_ERR_ARG;
    if (g.n * (int64_t)(g.cols0 + g.cols1) >= (1LL << 31)) return BCNF_ERR_UNSUPPORTED;
    ga = BcnfGatherArgs{g.idx, (const long long*)g.cursor, g.src0, g.dst0, g.src1, g.dst1, (int)g.n, 0, g.cols0,
                        g.cols1, 0};
    gather2_plan(g.n, &ga.rpw, &ga.nwg);
  }
  const int npw = pack_wgs(L, true);
  const unsigned grid = (unsigned)(L.NKp / 16 * FOLD_SPLIT + ga.nwg + npw + 1);
  return launch<k_pack_fold>(dim3(grid), dim3(BCNF_WG), 0, (hipStream_t)stream, L, params, qmats, (float*)packed,
                             feat_weight, feat_bias, (int)in_features, fold, ga, npw);
}

int bcnf_fold_nll_forward(const BcnfStackDesc* desc, const void* packed, const float* fold, int32_t in_features,
                          const float* y, const float* x, int32_t ldx, int64_t batch, float* z, float* ldj, int32_t training,
                          uint64_t* rng_state, void* workspace, int32_t finalize, float* loss_out, int32_t* guard,
                          void* stream) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!fold || ldx < in_features) return BCNF_ERR_ARG;
  return forward_impl(desc, packed, y, x, batch, z, ldj, nullptr, training, rng_state, workspace, true, true,
                      finalize != 0, loss_out, guard, stream, fold, in_features, ldx);
}

int bcnf_fold_raw_table_bytes(const BcnfStackDesc* desc, int32_t in_features, int64_t* bytes) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!bytes) return BCNF_ERR_ARG;
  if (!raw_applicable(L, in_features)) return BCNF_ERR_UNSUPPORTED;
  std::vector<uint32_t> t((size_t)raw_table_words(L));
  if (!build_raw_table(L, t.data())) return BCNF_ERR_UNSUPPORTED;
  *bytes = (int64_t)t.size() * (int64_t)sizeof(uint32_t);
  return BCNF_OK;
}

int bcnf_fold_raw_table(const BcnfStackDesc* desc, int32_t in_features, void* host_table) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!host_table) return BCNF_ERR_ARG;
  if (!raw_applicable(L, in_features)) return BCNF_ERR_UNSUPPORTED;
  return build_raw_table(L, (uint32_t*)host_table) ? BCNF_OK : BCNF_ERR_UNSUPPORTED;
}

int bcnf_fold_train_forward(const BcnfStackDesc* desc, const float* params, const float* qmats, const void* table,
                            const float* feat_weight, const float* feat_bias, int32_t in_features,
                            const BcnfGather2* gather, const float* y, const float* x, int32_t ldx, int64_t batch,
                            void* packed, float* z, float* ldj, int32_t training, uint64_t* rng_state,
                            void* workspace, int32_t finalize, float* loss_out, int32_t* guard, void* stream) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!raw_applicable(L, in_features)) return BCNF_ERR_UNSUPPORTED;
  if (!params || !qmats || !table || !feat_weight || !packed || batch < 1) return BCNF_ERR_ARG;
  RawForward R = {};
  R.P = params;
  R.Q = qmats;
  R.table = (const uint32_t*)table;
  R.wf = feat_weight;
  R.bf = feat_bias;
  R.pk = (float*)packed;
  R.X = in_features;
  if (gather) {
    const BcnfGather2& g = *gather;
    if (g.n != batch || g.cols0 != L.D || g.cols1 < in_features || !g.idx || !g.src0 || !g.src1 || !g.dst0 ||
        !g.dst1)
      return BCNF_ERR_ARG;
    R.idx = g.idx;
    R.cursor = (const long long*)g.cursor;
    R.ypool = g.src0;
    R.ydst = g.dst0;
    R.xpool = g.src1;
    R.xdst = g.dst1;
    R.ldx = g.cols1;
  } else {
    if (!y || !x || ldx < in_features) return BCNF_ERR_ARG;
    R.ypool = y;
    R.xpool = x;
    R.ldx = ldx;
  }
  return forward_impl(desc, packed, R.ypool, R.xpool, batch, z, ldj, nullptr, training, rng_state, workspace, true,
                      true, finalize != 0, loss_out, guard, stream, nullptr, 0, 0, &R);
}

int bcnf_fold_backward_tail(const BcnfStackDesc* desc, const void* packed, const void* slab, const float* x,
                            int32_t ldx, int32_t in_features, const float* feat_weight, const float* feat_bias,
                            const void* workspace, int64_t batch, int32_t training, float* dparams,
                            float* dfeat_weight, float* dfeat_bias, const BcnfFoldAdam* adam, void* stream) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!packed || !slab || !x || !feat_weight || !workspace || !dparams || batch < 1 || ldx < in_features)
    return BCNF_ERR_ARG;
  FoldAdamArgs A = {};
  if (adam) {
    const BcnfFoldAdam& a = *adam;
    if (!a.params[0] || !a.exp_avg[0] || !a.exp_avg_sq[0] || !a.params[1] || !a.exp_avg[1] || !a.exp_avg_sq[1] ||
        !a.step || !a.done_counter || (feat_bias && (!a.params[2] || !a.exp_avg[2] || !a.exp_avg_sq[2])) ||
        (a.advance_cursor && a.cursor_modulo < 1))
      return BCNF_ERR_ARG;
    for (int t = 0; t < 3; ++t) {
      A.p[t] = a.params[t];
      A.m[t] = a.exp_avg[t];
      A.v[t] = a.exp_avg_sq[t];
    }
    if (!feat_bias) A.p[2] = A.m[2] = A.v[2] = nullptr;
    A.step = a.step;
    A.lr = a.lr;
    A.b1 = a.beta1;
    A.b2 = a.beta2;
    A.eps = a.eps;
    A.wd = a.weight_decay;
    A.cursor = (long long*)a.advance_cursor;
    A.n_batches = (long long)a.cursor_modulo;
    A.log_values = a.log_values;
    A.log_history = a.log_history;
    A.done = (int*)a.done_counter;
    A.guard = (const int*)a.guard;
    A.on = 1;
  }
  return launch_fold_tail(L, fold_layout(L, in_features, ldx), (const float*)packed, (float*)slab, x, feat_weight,
                          feat_bias, (const float*)workspace, batch, dparams, dfeat_weight, dfeat_bias, A,
                          (hipStream_t)stream);
}

int bcnf_fold_tail_plan(const BcnfStackDesc* desc, int32_t in_features, int64_t batch, int64_t* out) {
  BcnfLayout L;
  const int rc = fold_setup(desc, in_features, &L);
  if (rc) return rc;
  if (!out || batch < 1) return BCNF_ERR_ARG;
  const FoldTailPlan P = fold_tail_plan(L, fold_layout(L, in_features, in_features), batch);
  out[0] = P.n_red;
  out[1] = P.S;
  for (int t = 0; t < 3; ++t) {
    out[2 + 2 * t] = P.first[t];
    out[3 + 2 * t] = P.count[t];
    out[8 + t] = P.own[t] + P.count[t];
    out[11 + t] = P.own[t];
  }
  return BCNF_OK;
}

int bcnf_grad_reduce(const BcnfStackDesc* desc, const void* slab, const float* h, const void* workspace,
                     int64_t batch, int32_t training, float* dparams, void* stream) {
  // (packed is only read by the dh role, which is off here)
  return bcnf_backward_tail(desc, slab, slab, h, workspace, batch, training, nullptr, dparams, stream);
}

int bcnf_stack_inverse(const BcnfStackDesc* desc, const void* packed, const float* z, const float* h, int64_t h_rows,
                       const int64_t* cond_index, int64_t n_rows, float* y, int32_t training,
                       const uint64_t* rng_state, void* scratch, void* stream) {
  BcnfLayout L;
  int rc = stack_setup(desc, &L);
  if (rc) return rc;
  if (n_rows == 0) return BCNF_OK;
  if (n_rows < 0 || h_rows < 1 || !packed || !z || !h || !y || !scratch) return BCNF_ERR_ARG;
  if (!cond_index && h_rows != n_rows) return BCNF_ERR_ARG;
  const bool drop = training && L.p > 0.f;
  if (drop && !rng_state) return BCNF_ERR_ARG;
  const float* pk = (const float*)packed;
  hipStream_t st = (hipStream_t)stream;
  float* hp = (float*)scratch;
  if ((rc = launch_hp(L, pk, h, h_rows, hp, st))) return rc;
  return launch_inverse(L, pk, z, hp, h_rows, cond_index, n_rows, y, drop, rng_state, st);
}

int bcnf_stack_inverse_logdet(const BcnfStackDesc* desc, const void* packed, const float* z, const float* h,
                              int64_t h_rows, const int64_t* cond_index, int64_t n_rows, float* y, float* ldj,
                              float* log_prob, void* scratch, void* stream) {
  if (!desc) return BCNF_ERR_ARG;
  if (desc->two_way) return BCNF_ERR_UNSUPPORTED;   // the reference's two_way inverse is not its forward's inverse
  if (!y || !ldj) return BCNF_ERR_ARG;
  BcnfLayout L;
  int rc = stack_setup(desc, &L);
  if (rc) return rc;
  if (n_rows == 0) return BCNF_OK;
  if (n_rows < 0 || h_rows < 1 || !packed || !z || !h || !scratch) return BCNF_ERR_ARG;
  if (!cond_index && h_rows != n_rows) return BCNF_ERR_ARG;
  const float* pk = (const float*)packed;
  hipStream_t st = (hipStream_t)stream;
  float* hp = (float*)scratch;
  if ((rc = launch_hp(L, pk, h, h_rows, hp, st))) return rc;
  return launch_inverse_logdet(L, pk, z, hp, h_rows, cond_index, n_rows, y, ldj, log_prob, st);
}

int bcnf_nll_forward(const BcnfStackDesc* desc, const void* packed, const float* y, const float* h, int64_t batch,
                     float* z, float* ldj, int32_t training, uint64_t* rng_state, void* workspace, int32_t finalize,
                     float* loss_out, int32_t* guard, void* stream) {
  return forward_impl(desc, packed, y, h, batch, z, ldj, nullptr, training, rng_state, workspace, true, true,
                      finalize != 0, loss_out, guard, stream);
}

int bcnf_nll_backward(const BcnfStackDesc* desc, const void* packed, const float* h, const float* z,
                      const float* dloss, int64_t batch, int32_t training, void* workspace, float* dy,
                      float* dh, float* dparams, void* slab, float* loss_out, uint64_t* rng_state, int32_t* guard,
                      void* stream) {
  if (!z && batch > 0) return BCNF_ERR_ARG;
  return backward_impl(desc, packed, h, z, nullptr, dloss, 1, batch, training, workspace, dy, dh, dparams, slab,
                       loss_out, rng_state, guard, stream);
}

const char* bcnf_status_string(int status) {
  switch (status) {
    case BCNF_OK: return "ok";
    case BCNF_ERR_ARG: return "invalid argument";
    case BCNF_ERR_UNSUPPORTED: return "unsupported stack shape for the fused kernel family";
    default: return status >= BCNF_ERR_HIP_BASE ? hipGetErrorString((hipError_t)(status - BCNF_ERR_HIP_BASE))
                                                 : "unknown status";
  }
}

int bcnf_lds_fill(float value, void* stream) {
  return launch<k_fill_lds>(dim3(4 * 256), dim3(BCNF_WG), LDS_MAX, (hipStream_t)stream, value);
}

#if BCNF_STAMPS
// diagnostic build only (not in include/bcnf_amd.h): slots 0-7 from the backward's file, 8-31 from the forward's
int bcnf_debug_phases(unsigned long long* out) {
  unsigned long long bwd[32];
  int rc = fwd_debug_phases(out);
  if (!rc) rc = bwd_debug_phases(bwd);
  for (int i = 0; i < 8 && !rc; ++i) out[i] = bwd[i];
  return rc;
}
#endif

}  // extern "C"
