// Small stack family (bcnf_stack*.hip): the constants every file shares, the host-side layout of a stack, and the
// LDS sizes and workspace offsets derived from it. Host functions are inline in bcnf_small: one definition for all
// translation units of the family, none of them exported.
#pragma once
#include "bcnf_device.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#pragma GCC visibility push(hidden)
namespace bcnf_small {

using bcnf_rt::LDS_MAX;

constexpr int NC16_MAX = 16;           // C <= 256: register-resident column tiles of k_hp / k_dh / dw1h_body
// Backward LDS tile of [16 samples s][16 columns r], unpadded: the four samples 4 t + q (t = 0..3) of column r sit in
// the 16-B slot tile_slot(r, q) = 4 r + ((q + (r >> 1)) & 3), so the MFMA operand of lane (q, r) for the four K-steps t
// is ONE 16-B read at 4 tile_slot(r, q), and each ds_read_b128 lane group covers all 16 slot banks (conflict-free). The
// rotation by r >> 1 also spreads the element stores: a compute / helper wave holds samples w + 4 i (sample_of) --
// one q per wave, t = i -- so a 32-lane half stores to 16 distinct banks (2-way, which costs a ds_write_b32 nothing;
// the padded pitch-24 rows were 4-way: 4.13M conflict cycles per k_backward launch).
constexpr int TILE = 256;
__host__ __device__ constexpr int tile_slot(int r, int q) { return 4 * r + ((q + (r >> 1)) & 3); }
__host__ __device__ constexpr int tile_ix(int s, int r) { return 4 * tile_slot(r, s & 3) + (s >> 2); }
// Sample (0..15) a forward / backward thread t8 (role-relative, 256 per role) works on: wave w = t8 >> 6 holds the
// samples w + 4 i of its four 16-lane rows i (the activation records and the derivative slots are per t8, so both
// kernels use the same map).
__host__ __device__ constexpr int sample_of(int t8) { return (t8 >> 6) + 4 * ((t8 >> 4) & 3); }
constexpr int STAGE_REC = 4;   // 16 * RF (RB) floats  <= 4 float4 per thread (RF, RB <= 256)
constexpr int RING = STAGE_REC * BCNF_WG * 4;    // floats per record-ring slot: a Stage stores all of it
constexpr int RAW_KP = 100;   // pack-free forward: LDS row pitch of the staged Wf / x rows (X <= 96), = 4 mod 32
// floats per lane of a block's activation record (ActRec); the AR1 single floats follow all the float4 parts
__host__ __device__ constexpr int act_rec_floats(int NH) { return 2 * NH + 3; }
__host__ __device__ constexpr long long ar1_off(int nb, long long nwg, int ar4) { return (long long)nb * nwg * ar4 * 4 * 256; }
// floats per block of a backward workgroup's gradient slab: NH + 2 MFMA tiles + NH + 6 column sums (BwdJobs)
__host__ __device__ constexpr int slab_blk_floats(int NH) { return (NH + 2) * 256 + (NH + 6) * 16; }

// Broadcast-form sections (row_newbcast DPP, D_a = 10 / D_b = 9 stacks only): QBC_W1 Linear 1 (forward), QBC_MIX
// the mix Q / Q^T (forward, inverse, backward), QBC_HEAD the T / S heads' transposes (backward).
constexpr int QBC_W1 = 1, QBC_MIX = 2, QBC_HEAD = 4;

// ------------------------------------------------------------------------------------------------
// Host-side layout
// ------------------------------------------------------------------------------------------------
constexpr int round_rec(int n) {            // multiple of 4 floats with odd quotient (conflict-free ds_read_b128)
  n = (n + 3) & ~3;
  if (((n / 4) & 1) == 0) n += 4;
  return n;
}

inline int make_layout(const BcnfStackDesc* d, BcnfLayout* L) {
  if (!d || !L) return BCNF_ERR_ARG;
  memset(L, 0, sizeof(*L));
  if (d->size < 2 || d->n_blocks < 1 || d->n_hidden < 0 || d->n_hidden > BCNF_MAX_HIDDEN || d->n_conditions < 0)
    return BCNF_ERR_ARG;
  for (int i = 0; i < d->n_hidden; ++i)
    if (d->hidden[i] < 1) return BCNF_ERR_ARG;
  if (!(d->dropout >= 0.f && d->dropout < 1.f)) return BCNF_ERR_ARG;
  L->D = d->size;
  L->Da = (d->size + 1) / 2;
  L->Db = d->size / 2;
  L->C = d->n_conditions;
  L->ldh = d->n_conditions;
  L->Cp = ((d->n_conditions + 15) / 16) * 16;
  if (L->Cp == 0) L->Cp = 16;
  L->NH = d->n_hidden;
  L->nb = d->n_blocks;
  L->act_norm = d->act_norm ? 1 : 0;
  L->H[0] = L->Da;
  for (int i = 0; i < L->NH; ++i) L->H[i + 1] = d->hidden[i];
  L->H[L->NH + 1] = 2 * L->Db;
  int off = 0;
  for (int l = 1; l <= L->NH + 1; ++l) {
    L->lin_in[l] = (l == 1) ? (L->Da + L->C) : L->H[l - 1];
    L->lin_out[l] = L->H[l];
    L->lin_w[l] = off;
    off += L->lin_in[l] * L->lin_out[l];
    L->lin_b[l] = off;
    off += L->lin_out[l];
  }
  L->an_size = L->act_norm ? 2 * L->D : 0;
  L->blk_stride = L->an_size + off;
  L->n_trainable = (L->nb - 1) * L->blk_stride + off;
  L->cblk = L->blk_stride - L->H[1] * L->C;
  L->blk_pad = (L->cblk + 3) & ~3;
  L->sblk = slab_blk_floats(L->NH);
  L->qbc = (L->Da == 10 && L->Db == 9) ? (QBC_W1 | QBC_MIX | QBC_HEAD) : 0;
  L->p = d->dropout;
  L->keep_scale = (d->dropout > 0.f) ? (1.0f / (1.0f - d->dropout)) : 1.0f;
  const double t32 = std::min(4294967295.0, floor((double)d->dropout * 4294967296.0 + 0.5));   // dropout_bits
  L->thr_hi = (uint32_t)t32 >> 16;
  L->thr_lo = (uint32_t)t32 & 0xffffu;
  // forward/inverse record: [sa ba sb bb][b1 pad pad pad][W1y:16][hidden l: 16+1 ...][T:16+1][S:16+1][Q:64]
  L->rf_b1 = 4;
  L->rf_w1 = 8;
  L->rf_hid = 24;
  L->rf_t = L->rf_hid + 17 * (L->NH > 0 ? L->NH - 1 : 0);
  L->rf_s = L->rf_t + 17;
  L->rf_q = (L->rf_s + 17 + 3) & ~3;
  L->RF = round_rec(L->rf_q + 64);
  // backward record, in the order the backward consumes it (so its LDS reads are waited for piecewise, not all at
  // once): [ActNorm sa ba sb bb][Q^T:64][Tout^T:16][Sout^T:16][hidden^T l = NH .. 2: 16 each][W1T:16]
  L->rb_an = 0;
  L->rb_qt = 4;
  L->rb_tt = 68;
  L->rb_st = 84;
  L->rb_hid = 100;                             // hidden layer l at rb_hid + 16 (NH - l)
  L->rb_w1t = 100 + 16 * (L->NH > 0 ? L->NH - 1 : 0);
  L->RB = round_rec(L->rb_w1t + 16);
  long long nbl = L->nb;
  L->pf_off = 0;
  L->pb_off = L->pf_off + nbl * 16 * L->RF;
  L->pi_off = L->pb_off + nbl * 16 * L->RB;
  L->NKp = ((L->nb * 16 + 63) / 64) * 64;
  L->w1c_off = L->pi_off + nbl * 16 * L->RF;
  L->w1r_off = L->w1c_off + (long long)L->Cp * L->NKp;
  L->b1c_off = L->w1r_off + (long long)L->NKp * L->Cp;
  L->ldc_off = L->b1c_off + L->NKp;
  // matrix-core inverse record in MFMA A-operand order (k_inverse_mfma, inv_mo_*): NH + 6 matrices x 64 lanes x 4
  // steps, hidden / T / S biases as [4 q][4 r], ActNorm inverse [4 q][4 r][4]
  L->PMB = (L->NH + 6) * 256 + (L->NH - 1) * 16 + 32 + 64;
  L->pm_off = L->ldc_off + 4;
  L->total = L->pm_off + nbl * L->PMB;
  return BCNF_OK;
}

constexpr size_t INV_LDS_BYTES = sizeof(float) * (size_t)(2 * RING);   // inverse record ring (2 blocks)
inline size_t fwd2_lds_bytes(const BcnfLayout& L, bool raw = false) {  // k_forward: record ring, projection partials,
  return sizeof(float) * (size_t)(3 * RING + 3 * 4 * 256 + 3 * 8 * 256 +   // dropout masks (3 slots)
                                  (raw ? 4 + 16 * (128 + 4) + (L.C + 16) * RAW_KP : 0));   // RAW: log-det
                                                                           // partials, h tile, staged Wf / x
}
inline size_t bwd_lds_bytes(const BcnfLayout& L) {   // backward record ring, delta tiles (2), activation tiles (3), derivative slots (2)
  return sizeof(float) * (size_t)(2 * RING + 2 * (L.NH + 6) * TILE + 3 * (L.NH + 1) * TILE + 2 * 3 * 4 * 256);
}

inline bool layout_supported(const BcnfLayout& L, const BcnfStackDesc* d) {
  if (d->two_way) return false;
  if (L.NH < 1 || L.NH > BCNF_MAX_HIDDEN) return false;
  if (L.Da > 16 || L.Db > 16) return false;
  for (int l = 1; l <= L.NH; ++l)
    if (L.H[l] > 16) return false;
  if (L.C < 1 || L.Cp > 16 * NC16_MAX) return false;
  if (sizeof(float) * (size_t)(64 * 132 + 128 * (L.Cp + 32)) > LDS_MAX) return false;   // dw1h_body staging
  if (16 * L.RF > 4 * 4 * BCNF_WG || 16 * L.RB > 4 * 4 * BCNF_WG) return false;
  if (INV_LDS_BYTES > LDS_MAX || bwd_lds_bytes(L) > LDS_MAX) return false;
  return true;
}

// The pack-free forward's table (build_raw_table, bcnf_stack.hip; read by k_forward's helper waves).
constexpr int RAW_NP = 10, RAW_NQ = 2, RAW_NZ = 6;   // slots per helper thread (FC_small: 2152 P-sourced, 361
                                                     // Q-sourced and 1071 zero entries)
constexpr int RAW_NS = RAW_NP + RAW_NQ + RAW_NZ;
constexpr int RAW_NSP = (RAW_NS + 3) & ~3;   // a thread's entries, contiguous: RAW_NSP / 4 16-byte loads
constexpr int RAW_DUMMY = RING - 1;       // an unused float of a ring slot (16 RF <= RING - 1)
constexpr int RAW_SRC_MAX = 1 << 20;
constexpr int RAW_TPW = 2;             // h column tiles per helper wave: C <= 128

// A table entry: destination float of the ring slot (j * RF + e, < 4096) | source offset << 12.
__host__ __device__ constexpr uint32_t raw_entry(int dst, int src) { return (uint32_t)dst | ((uint32_t)src << 12); }

// The folded feature Linear (fold_body, bcnf_stack.hip): Xp = 16-multiple > X.
__host__ __device__ inline int fold_xp(int X) { return ((X + 1 + 15) / 16) * 16; }

// Layout seen by the projection kernels (k_hp, the split-K dW1h body) when they run on x instead of h.
inline BcnfLayout fold_layout(const BcnfLayout& L, int X, int ldx) {
  BcnfLayout F = L;
  F.C = X;
  F.ldh = ldx;
  F.Cp = fold_xp(X);
  F.w1c_off = 0;
  F.b1c_off = (long long)F.Cp * L.NKp;
  return F;
}

// The projection GEMMs (k_hp, bcnf_stack_inv.hip; the tail's bodies, bcnf_stack_tail.hip)
constexpr int KC = 128;                // K-chunk
// LDS strides for the MFMA operand reads: [row = lane&15][k = 4t + lane>>4] wants stride = 4 (mod 32),
// [k = 4t + lane>>4][col = lane&15] wants stride = 16 (mod 32): 64 lanes then hit every bank exactly twice.
constexpr int KCP = KC + 4;            // A tiles [64][KC]
constexpr int BNS = 80;                // k_hp B tile [KC][64]
__host__ __device__ constexpr int bstride16(int n) { return n + ((16 - (n & 31)) & 31); }   // >= n, = 16 mod 32
inline size_t hp_lds_bytes() { return sizeof(float) * (size_t)(64 * KCP + KC * BNS); }
inline size_t dh_lds_bytes() { return sizeof(float) * (size_t)(64 * KCP + KC * 16); }
inline size_t dw1h_lds_bytes(const BcnfLayout& L) { return sizeof(float) * (size_t)(64 * KCP + KC * bstride16(L.Cp)); }
constexpr int KH = KC / 2, KHP = KH + 4;   // dw1h_half_body stages a split as two KH-row halves
inline size_t dw1h_half_lds_bytes(const BcnfLayout& L) {
  return sizeof(float) * (size_t)(32 * KHP + KH * bstride16(L.Cp));
}

// float4 row loads: the row stride and the base are 16-byte aligned (columns >= C of a loaded float4 are
// discarded by select, so a padded row's tail may hold anything).
inline bool vec_rows(const BcnfLayout& L, const float* h) { return L.ldh % 4 == 0 && ((uintptr_t)h & 15) == 0; }

inline long long slab_stride_of(const BcnfLayout& L) { return (long long)L.nb * L.sblk; }
// split-K geometry of the W1 condition-part gradient
constexpr int W1H_ROWS_PER_SPLIT = KC;   // one LDS chunk of rows per split
inline long long w1h_splits(long long B) { return (B + W1H_ROWS_PER_SPLIT - 1) / W1H_ROWS_PER_SPLIT; }
inline long long w1h_work_floats(const BcnfLayout& L, long long B) { return w1h_splits(B) * L.nb * 16LL * L.Cp; }

// Workspace (floats): [activation records nb*B*16*AR][loss partials][HP nb*B*16][D1 nb*B*16]
// (the same with and without dropout: the records hold the masked activations)
inline long long ws_part_off(const BcnfLayout& L, long long B) {
  return (long long)L.nb * ((B + 15) / 16) * BCNF_WG * act_rec_floats(L.NH);   // padded rows own slots
}
inline long long ws_hp_off(const BcnfLayout& L, long long B) { return ws_part_off(L, B) + (((B + 15) / 16 + 3) & ~3LL); }
inline long long ws_d1_off(const BcnfLayout& L, long long B) { return ws_hp_off(L, B) + (long long)L.nb * B * 16; }
inline long long ws_floats(const BcnfLayout& L, long long B) {
  return ws_d1_off(L, B) + (long long)L.nb * B * 16 + 16;   // + D1 dummy row
}

// The prologue of an entry that runs a stack: its layout, or the status of a malformed / unsupported description.
inline int stack_setup(const BcnfStackDesc* desc, BcnfLayout* L) {
  const int rc = make_layout(desc, L);
  if (rc) return rc;
  return layout_supported(*L, desc) ? BCNF_OK : BCNF_ERR_UNSUPPORTED;
}
// ... and of an entry of the folded path (feature network = one Linear of X inputs).
inline int fold_setup(const BcnfStackDesc* desc, int32_t X, BcnfLayout* L) {
  const int rc = stack_setup(desc, L);
  if (rc) return rc;
  if (X < 1 || fold_xp(X) > 16 * NC16_MAX) return BCNF_ERR_UNSUPPORTED;
  if (dw1h_lds_bytes(fold_layout(*L, X, X)) > LDS_MAX) return BCNF_ERR_UNSUPPORTED;
  return BCNF_OK;
}
inline long long fold_floats(const BcnfLayout& L, int X) { return (long long)(fold_xp(X) + 1) * L.NKp; }
// The pack-free forward's shape limits (its table must also build: build_raw_table).
inline bool raw_applicable(const BcnfLayout& L, int X) {
  return X <= RAW_KP - 4 && L.C <= 64 * RAW_TPW && L.nb >= 2 && L.act_norm;
}

// The kernels are templates over the number of hidden layers: f(std::integral_constant<int, NH>) for NH = 1 .. 8.
template <typename F>
int dispatch_nh(int NH, F&& f) {
  switch (NH) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return BCNF_ERR_UNSUPPORTED;
  }
}

}  // namespace bcnf_small
#pragma GCC visibility pop
