// Prediction head of a hybrid CondRealNVP_v2 (cnf.py: prediction_head = nn.Linear(C, D)) fused with its MSE loss
// (trainer.py:261-269, hybrid_weight > 0): r = x W^T + bias - y, mse = mean(r^2), and the backward through
// w / (1 + w) * mse into dW, dbias and the stack's dL/dh buffer. A skinny GEMM (N = D <= 32: one or two 16-column
// tiles of v_mfma_f32_16x16x4_f32) bound by reading x once; every reduction runs in a fixed order (no float
// atomics, no hand-off between workgroups), so a launch gives the same bits wherever its workgroups land.
#include "bcnf_device.h"

namespace {

using bcnf_rt::launch;

constexpr int HWG = 256;          // forward / dx / finalize workgroup (4 waves)
constexpr int HEAD_SPLITS = 64;   // most batch splits of the dW / dbias partials
constexpr int HEAD_KW = 64;       // x columns per dW wave

inline long long r4(long long n) { return (n + 3) / 4 * 4; }

// Workspace carve-up (floats): residual r [B][D], one squared-error partial per 16-row forward workgroup, the batch
// splits' dW partials [S][D][Kp] (Kp = K rounded up to 4: whole float4 stores) and dbias partials [S][32]. The
// reserved split count bounds the launched one and does not decrease in B.
struct HeadPlan {
  long long r_off, mse_off, dw_off, db_off, total;
  int n_mse, splits, rps, Kp, kgroups, cap;
};

bool head_plan(long long B, long long K, int D, HeadPlan* P) {
  if (B < 1 || K < 1 || D < 2 || D > 32 || K > (1LL << 24) || B > 0x7fffffffLL - 16) return false;
  P->Kp = (int)r4(K);
  P->kgroups = (int)((K + HEAD_KW - 1) / HEAD_KW);
  int target = 512 / P->kgroups;
  target = target < 1 ? 1 : (target > HEAD_SPLITS ? HEAD_SPLITS : target);
  long long rps = r4((B + target - 1) / target);       // rows per split: a multiple of the MFMA's 4, at least 8
  if (rps < 8) rps = 8;
  P->rps = (int)rps;
  P->splits = (int)((B + rps - 1) / rps);
  const long long by8 = (B + 7) / 8;
  P->cap = (int)(by8 < target ? by8 : target);
  P->n_mse = (int)((B + 15) / 16);
  P->r_off = 0;
  P->mse_off = r4(B * D);
  P->dw_off = P->mse_off + r4(P->n_mse);
  P->db_off = P->dw_off + (long long)P->cap * D * P->Kp;
  P->total = P->db_off + (long long)P->cap * 32;
  return P->splits <= P->cap;
}

// Four consecutive floats p[k .. k + 3] of a row of K valid columns: one 16-byte load where the row is aligned and
// whole, else element by element; columns >= K (padding the caller may have left uninitialised) and rows that do
// not exist read as 0.
__device__ __forceinline__ floatx4 ld4(const float* __restrict__ p, int k, int K, bool vec, bool ok) {
  floatx4 v{0.f, 0.f, 0.f, 0.f};
  if (!ok) return v;
  if (vec && k + 3 < K) return *reinterpret_cast<const floatx4*>(p + k);
  if (k < K) v.x = p[k];
  if (k + 1 < K) v.y = p[k + 1];
  if (k + 2 < K) v.z = p[k + 2];
  if (k + 3 < K) v.w = p[k + 3];
  return v;
}

// d(logged values) -> the scale of e = scale * r: 2 g / (B D), g = dloss[0] w / (1 + w) + dloss[2].
__device__ __forceinline__ float head_scale(const float* __restrict__ dloss, float wfrac, long long B, int D) {
  const float g = dloss ? fmaf(dloss[0], wfrac, dloss[2]) : wfrac;
  return 2.0f * g / (float)(B * D);
}

// ---- forward: 16 rows per workgroup, its 4 waves each a quarter of K, summed in wave order ---------------------
// Lane (i = l & 15, g = l >> 4) loads x[row i][16 c + 4 g .. + 3] and W[col i (+ 16)][same k] as float4; MFMA t of
// the chunk multiplies element t of both, i.e. k = 16 c + 4 g + t: the same k on the A and the B side.
template <int NT>
__global__ __launch_bounds__(HWG) void k_head_fwd(const float* __restrict__ x, long long ldx, int K,
                                                  const float* __restrict__ W, const float* __restrict__ bias,
                                                  const float* __restrict__ y, long long B, int D,
                                                  float* __restrict__ r, float* __restrict__ part, int vecx,
                                                  int vecw) {
  __shared__ floatx4 red[4][NT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const long long row0 = (long long)blockIdx.x * 16;
  const bool rowok = row0 + i < B;
  const float* xr = x + (rowok ? row0 + i : 0) * ldx;
  const int nchunk = (K + 15) / 16, cpw = (nchunk + 3) / 4;
  const int c0 = wave * cpw, c1 = c0 + cpw < nchunk ? c0 + cpw : nchunk;
  floatx4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int c = c0; c < c1; ++c) {
    const int k = 16 * c + 4 * g;
    const floatx4 a = ld4(xr, k, K, vecx != 0, rowok);
    floatx4 b[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = i + 16 * nt;
      b[nt] = ld4(W + (long long)(j < D ? j : 0) * K, k, K, vecw != 0, j < D);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      acc[nt] = mfma4(a.x, b[nt].x, acc[nt]);
      acc[nt] = mfma4(a.y, b[nt].y, acc[nt]);
      acc[nt] = mfma4(a.z, b[nt].z, acc[nt]);
      acc[nt] = mfma4(a.w, b[nt].w, acc[nt]);
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) red[wave][nt][lane] = acc[nt];
  __syncthreads();
  if (wave != 0) return;
  float sq = 0.f;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const floatx4 s = ((red[0][nt][lane] + red[1][nt][lane]) + red[2][nt][lane]) + red[3][nt][lane];
    const int col = i + 16 * nt;                      // accumulator element rr: row 4 g + rr, column l & 15
    if (col < D) {
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long row = row0 + 4 * g + rr;
        if (row < B) {
          const float v = (s[rr] + bv) - y[row * D + col];
          r[row * D + col] = v;
          sq = fmaf(v, v, sq);
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off);
  if (lane == 0) part[blockIdx.x] = sq;
}

// ---- backward, dx = e W (B x K), optionally added into dx: transposed tiles out[k][b] = sum_j W[j][k] e[b][j], so
// a lane ends with four consecutive k of one row: one 16-byte read-modify-write, each element touched once. --------
template <int NT>
__global__ __launch_bounds__(HWG) void k_head_dx(const float* __restrict__ W, int K, const float* __restrict__ r,
                                                 const float* __restrict__ dloss, float wfrac, long long B, int D,
                                                 float* __restrict__ dx, long long ldd, int accumulate, int vecd) {
  constexpr int NJ = 4 * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const long long row = (long long)blockIdx.x * 16 + i;
  const bool rowok = row < B;
  const float sc = head_scale(dloss, wfrac, B, D);
  float e[NJ];
#pragma unroll
  for (int js = 0; js < NJ; ++js) {
    const int j = 4 * js + g;
    e[js] = (rowok && j < D) ? sc * r[row * D + j] : 0.f;
  }
  const int nct = (K + 15) / 16;
  float* drow = dx + (rowok ? row : 0) * ldd;
  for (int ct = blockIdx.y * 4 + wave; ct < nct; ct += gridDim.y * 4) {
    const int kc = 16 * ct;
    floatx4 acc{0.f, 0.f, 0.f, 0.f};
    float a[NJ];
#pragma unroll
    for (int js = 0; js < NJ; ++js) {
      const int j = 4 * js + g;
      a[js] = (j < D && kc + i < K) ? W[(long long)j * K + kc + i] : 0.f;
    }
#pragma unroll
    for (int js = 0; js < NJ; ++js) acc = mfma4(a[js], e[js], acc);
    if (!rowok) continue;
    const int k = kc + 4 * g;
    if (vecd && k + 3 < K) {
      floatx4* p = reinterpret_cast<floatx4*>(drow + k);
      *p = accumulate ? *p + acc : acc;
    } else {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        if (k + rr < K) drow[k + rr] = accumulate ? drow[k + rr] + acc[rr] : acc[rr];
    }
  }
}

// ---- backward, dW = e^T x and dbias = sum_b e: one wave per (64 columns of x, batch split); the split's partial
// goes to the workspace, k_head_wreduce adds the splits in order. Lane (c, g) loads x[row b0 + g][kc + 4 c .. + 3];
// MFMA t takes element t, so its output column c is k = kc + 4 c + t, and the four t of a lane form one float4. ----
template <int NT>
__global__ __launch_bounds__(64) void k_head_dw(const float* __restrict__ x, long long ldx, int K,
                                                const float* __restrict__ r, const float* __restrict__ dloss,
                                                float wfrac, long long B, int D, int rps, int Kp,
                                                float* __restrict__ wpart, float* __restrict__ bpart, int vecx) {
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int kc = blockIdx.x * HEAD_KW, s = blockIdx.y;
  const long long b_lo = (long long)s * rps, b_hi = b_lo + rps < B ? b_lo + rps : B;
  const float sc = head_scale(dloss, wfrac, B, D);
  const bool first = blockIdx.x == 0;
  floatx4 acc[NT][4], accb[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    accb[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[nt][t] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  // 16 rows per round: the four row groups' loads are all issued before the first MFMA (rows past the split read as 0)
  constexpr int UN = 4;
  for (long long b0 = b_lo; b0 < b_hi; b0 += 4 * UN) {
    floatx4 xv[UN];
    float a[UN][NT];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const long long b = b0 + 4 * u + g;
      const bool ok = b < b_hi;
      xv[u] = ld4(x + (ok ? b : 0) * ldx, kc + 4 * c, K, vecx != 0, ok);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int j = c + 16 * nt;
        a[u][nt] = (ok && j < D) ? sc * r[b * D + j] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[nt][0] = mfma4(a[u][nt], xv[u].x, acc[nt][0]);
        acc[nt][1] = mfma4(a[u][nt], xv[u].y, acc[nt][1]);
        acc[nt][2] = mfma4(a[u][nt], xv[u].z, acc[nt][2]);
        acc[nt][3] = mfma4(a[u][nt], xv[u].w, acc[nt][3]);
        if (first) accb[nt] = mfma4(a[u][nt], 1.0f, accb[nt]);
      }
    }
  }
  const int k = kc + 4 * c;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int j = 16 * nt + 4 * g + rr;               // accumulator element rr: row 4 g + rr
      if (j >= D) continue;
      if (k < Kp)
        *reinterpret_cast<floatx4*>(wpart + ((long long)s * D + j) * Kp + k) =
            floatx4{acc[nt][0][rr], acc[nt][1][rr], acc[nt][2][rr], acc[nt][3][rr]};
      if (first && c == 0) bpart[s * 32 + j] = accb[nt][rr];
    }
  }
}

__global__ __launch_bounds__(HWG) void k_head_wreduce(const float* __restrict__ wpart, const float* __restrict__ bpart,
                                                      int splits, int D, int K, int Kp, float* __restrict__ dW,
                                                      float* __restrict__ dbias) {
  const long long idx = (long long)blockIdx.x * HWG + threadIdx.x;
  const long long n = (long long)D * K;
  if (idx < n) {
    if (!dW) return;
    const int j = (int)(idx / K), k = (int)(idx - (long long)j * K);
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += wpart[((long long)s * D + j) * Kp + k];
    dW[idx] = v;
  } else if (idx < n + D && dbias) {
    const int j = (int)(idx - n);
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += bpart[s * 32 + j];
    dbias[j] = v;
  }
}

// ---- after the stack's NLL finalize wrote [nll, nll, 0]: mse from the forward's partials in a fixed order, the
// Trainer's combined loss, and the divergence rule of k_guard_global on it. A halted step keeps its books closed. --
__global__ __launch_bounds__(HWG) void k_hybrid_finalize(float* __restrict__ vals, const float* __restrict__ part,
                                                         int nparts, long long B, int D, float weight,
                                                         int32_t* __restrict__ guard) {
  __shared__ float red[HWG];
  if (guard && guard[BCNF_GUARD_HALTED]) return;
  float acc = 0.f;
  for (int p = threadIdx.x; p < nparts; p += HWG) acc += part[p];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = HWG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float mse = red[0] / (float)(B * D);
  const float loss = (vals[1] + mse * weight) / (1.0f + weight);      // trainer.py:264
  vals[2] = mse;
  vals[0] = loss;
  if (guard && guard[BCNF_GUARD_CHECK_GLOBAL] && (loss > 1e5f || isnan(loss))) guard[BCNF_GUARD_DIVERGED] = 1;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int bcnf_head_work_bytes(int64_t batch, int32_t in_features, int32_t out_features, int64_t* bytes) {
  HeadPlan P;
  if (!bytes || !head_plan(batch, in_features, out_features, &P)) return BCNF_ERR_ARG;
  *bytes = P.total * 4;
  return BCNF_OK;
}

int bcnf_head_mse_forward(const float* x, int64_t ldx, int32_t K, const float* W, const float* bias, const float* y,
                          int64_t B, int32_t D, void* work, void* stream) {
  HeadPlan P;
  if (!x || !W || !y || !work || ldx < K || !aligned16(work) || !head_plan(B, K, D, &P)) return BCNF_ERR_ARG;
  float* ws = static_cast<float*>(work);
  const int vecx = (ldx % 4 == 0 && aligned16(x)) ? 1 : 0, vecw = (K % 4 == 0 && aligned16(W)) ? 1 : 0;
  const dim3 grid((unsigned)P.n_mse);
  return D <= 16 ? launch<k_head_fwd<1>>(grid, dim3(HWG), 0, (hipStream_t)stream, x, (long long)ldx, K, W, bias, y,
                                         (long long)B, D, ws + P.r_off, ws + P.mse_off, vecx, vecw)
                 : launch<k_head_fwd<2>>(grid, dim3(HWG), 0, (hipStream_t)stream, x, (long long)ldx, K, W, bias, y,
                                         (long long)B, D, ws + P.r_off, ws + P.mse_off, vecx, vecw);
}

int bcnf_head_mse_backward(const float* x, int64_t ldx, int32_t K, const float* W, void* work, const float* dloss,
                           float weight, int64_t B, int32_t D, float* dW, float* dbias, float* dx, int64_t ldd,
                           int32_t accumulate_dx, void* stream) {
  HeadPlan P;
  if (!x || !W || !work || ldx < K || !aligned16(work) || !(weight >= 0.f) || !head_plan(B, K, D, &P))
    return BCNF_ERR_ARG;
  if (dx && ldd < K) return BCNF_ERR_ARG;
  float* ws = static_cast<float*>(work);
  const float wfrac = (float)((double)weight / (1.0 + (double)weight));
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    const int nct = (K + 15) / 16, tiles4 = (nct + 3) / 4;
    long long gy = (512 + P.n_mse - 1) / P.n_mse;
    gy = gy < 1 ? 1 : (gy > tiles4 ? tiles4 : gy);
    if (gy > 65535) gy = 65535;
    const dim3 grid((unsigned)P.n_mse, (unsigned)gy);
    const int vecd = (ldd % 4 == 0 && aligned16(dx)) ? 1 : 0;
    const int rc = D <= 16 ? launch<k_head_dx<1>>(grid, dim3(HWG), 0, st, W, K, ws + P.r_off, dloss, wfrac, (long long)B,
                                                  D, dx, (long long)ldd, accumulate_dx, vecd)
                           : launch<k_head_dx<2>>(grid, dim3(HWG), 0, st, W, K, ws + P.r_off, dloss, wfrac, (long long)B,
                                                  D, dx, (long long)ldd, accumulate_dx, vecd);
    if (rc) return rc;
  }
  if (dW || dbias) {
    const int vecx = (ldx % 4 == 0 && aligned16(x)) ? 1 : 0;
    const dim3 grid((unsigned)P.kgroups, (unsigned)P.splits);
    const int rc = D <= 16 ? launch<k_head_dw<1>>(grid, dim3(64), 0, st, x, (long long)ldx, K, ws + P.r_off, dloss, wfrac,
                                                  (long long)B, D, P.rps, P.Kp, ws + P.dw_off, ws + P.db_off, vecx)
                           : launch<k_head_dw<2>>(grid, dim3(64), 0, st, x, (long long)ldx, K, ws + P.r_off, dloss, wfrac,
                                                  (long long)B, D, P.rps, P.Kp, ws + P.dw_off, ws + P.db_off, vecx);
    if (rc) return rc;
    const long long n = (long long)D * K + D;
    return launch<k_head_wreduce>(dim3((unsigned)((n + HWG - 1) / HWG)), dim3(HWG), 0, st, ws + P.dw_off, ws + P.db_off,
                                  P.splits, D, K, P.Kp, dW, dbias);
  }
  return BCNF_OK;
}

int bcnf_hybrid_finalize(float* loss_vals, const void* work, int64_t B, int32_t D, float weight, int32_t* guard,
                         void* stream) {
  HeadPlan P;
  if (!loss_vals || !work || !(weight >= 0.f) || !head_plan(B, 1, D, &P)) return BCNF_ERR_ARG;
  const float* ws = static_cast<const float*>(work);
  return launch<k_hybrid_finalize>(dim3(1), dim3(HWG), 0, (hipStream_t)stream, loss_vals, ws + P.mse_off, P.n_mse,
                                   (long long)B, D, weight, guard);
}

}  // extern "C"
