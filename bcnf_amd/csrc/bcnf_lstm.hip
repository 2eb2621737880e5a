// One LSTM layer (reference feature_network.py:310-398, VerboseLSTM's single-layer nn.LSTM modules), both directions
// in one launch. The input projection P = x W_ih^T + b_ih is NOT here (bcnf_linear_forward, one call per direction),
// nor are the weight gradients (bcnf_linear_backward on dP): these kernels are the serial part only,
//
//   gates_t = P_t + h_{t-1} W_hh^T + b_hh,  c_t = s(f) c_{t-1} + s(i) tanh(g),  h_t = s(o) tanh(c_t)   (i, f, g, o)
//
// A workgroup owns 16 batch rows of one direction for all S steps (samples never interact: no grid barrier). Wave w
// owns hidden units 16 w .. 16 w + 15 and the i, f, g, o columns of those SAME units, so its four 16x16 gate tiles
// share one MFMA accumulator layout (lane (q, j): rows 4 q .. 4 q + 3 of unit 16 w + j) and the cell update is
// lane-local: c never leaves registers. W_hh stays on chip for the whole sequence as the wave's MFMA B operands,
// H VGPRs per lane each way (forward: 4 gates x H / 4 k-steps; backward: 4 H / 4 k-steps of one 16-column tile), for
// every H, so there is one scheme and no LDS copy of the weights. h_t (forward) / dP_t (backward) goes to the other
// waves through a double-buffered LDS tile, one barrier per step. Lane (q, j) of an MFMA takes k = q (K / 4) + kk at
// k-step kk (A and B agree on it, the sum over k does not care), so an A operand is four consecutive floats of one
// LDS row: one 16-byte read per four MFMAs. Every sum runs in a fixed order: same inputs, same bits.
#include "bcnf_device.h"

namespace {

constexpr int LROWS = 16;      // batch rows of a workgroup = the M of the 16x16x4 MFMA

__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + exp_fast(-x)); }

// Forward. p / whh / bhh: direction 0 | 1. p rows (b S + t), ldp floats apart, 4 H floats each. out (B S) rows, ldo
// apart, direction d at columns d H ... gates (dirs, B S, 4 H) and cells (dirs, B S, H): the activated gates and c_t,
// written when gates != nullptr.
template <int H>
__global__ void __launch_bounds__(H * 4) k_lstm_fwd(const float* __restrict__ p0, const float* __restrict__ p1,
                                                    long long ldp, const float* __restrict__ w0,
                                                    const float* __restrict__ w1, const float* __restrict__ b0,
                                                    const float* __restrict__ b1, long long B, int S,
                                                    float* __restrict__ out, long long ldo,
                                                    float* __restrict__ gates, float* __restrict__ cells) {
  constexpr int NK = H / 4;          // k-steps of h W_hh^T (K = H)
  constexpr int LDH = H + 4;         // LDS row stride: 16-byte rows, row r starts 4 (H / 4 + 1) banks on (odd multiple)
  __shared__ __attribute__((aligned(16))) float hs[2][LROWS][LDH];

  const int d = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * LROWS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const int u = wave * 16 + j;       // this lane's hidden unit (the N index of all four gate tiles)
  const float* __restrict__ P = d ? p1 : p0;
  const float* __restrict__ W = d ? w1 : w0;
  const float* __restrict__ bh = d ? b1 : b0;

  // B operands: W_hh[g H + u][q NK + kk], contiguous in kk
  float w[4][NK];
  float bias[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float* wr = W + (long long)(g * H + u) * H + q * NK;
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) w[g][kk] = wr[kk];
    bias[g] = bh ? bh[g * H + u] : 0.0f;
  }
  for (int i = threadIdx.x; i < 2 * LROWS * LDH; i += H * 4) (&hs[0][0][0])[i] = 0.0f;     // h_0 = 0 (and the pads)

  bool valid[4];
  long long rbase[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long row = row0 + 4 * q + r;
    valid[r] = row < B;
    rbase[r] = (valid[r] ? row : 0) * S;
  }
  const long long save_dir = (long long)d * B * S;

  float c[4] = {0.f, 0.f, 0.f, 0.f};
  float p[4][4], pn[4][4];
  {
    const int t = d ? S - 1 : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int g = 0; g < 4; ++g) p[g][r] = valid[r] ? P[(rbase[r] + t) * ldp + g * H + u] : 0.0f;
  }
  __syncthreads();

  for (int s = 0; s < S; ++s) {
    const int t = d ? S - 1 - s : s;
    const int cur = s & 1;
    if (s + 1 < S) {                 // the next step's projection rows, in flight behind this step's MFMAs
      const int tn = d ? t - 1 : t + 1;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int g = 0; g < 4; ++g) pn[g][r] = valid[r] ? P[(rbase[r] + tn) * ldp + g * H + u] : 0.0f;
    }
    floatx4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = floatx4{p[g][0] + bias[g], p[g][1] + bias[g], p[g][2] + bias[g],
                                                p[g][3] + bias[g]};
    const float* hrow = &hs[cur][j][q * NK];
#pragma unroll
    for (int k4 = 0; k4 < NK / 4; ++k4) {
      const floatx4 a = *reinterpret_cast<const floatx4*>(hrow + 4 * k4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = mfma4(a[e], w[g][4 * k4 + e], acc[g]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = sigmoid_f(acc[0][r]), gf = sigmoid_f(acc[1][r]), gg = tanh_bf(acc[2][r]),
                  go = sigmoid_f(acc[3][r]);
      c[r] = fmaf(gf, c[r], gi * gg);
      const float h = go * tanh_bf(c[r]);
      hs[cur ^ 1][4 * q + r][u] = h;
      if (valid[r]) {
        const long long row = rbase[r] + t;
        out[row * ldo + d * H + u] = h;
        if (gates) {
          float* gr = gates + (save_dir + row) * (4 * H) + u;
          gr[0] = gi;
          gr[H] = gf;
          gr[2 * H] = gg;
          gr[3 * H] = go;
          cells[(save_dir + row) * H + u] = c[r];
        }
      }
    }
    __syncthreads();                 // h_t is complete; buffer `cur` is free again after the NEXT barrier
    if (s + 1 < S) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) p[g][r] = pn[g][r];
    }
  }
}

// What one backward step reads for a lane's four (row, unit) pairs.
struct BwdIn {
  float g[4][4];      // activated i, f, g, o
  float cp[4];        // c of the forward's previous step (0 at its first)
  float dy[4];
};

// Backward, against the forward's order. dout rows ldo apart, direction d at columns d H ...; dp0 / dp1 (B S) rows of
// 4 H floats, ldp apart: the gradient of the PRE-activation gates, which is dP, d(h_prev W_hh^T) and db_hh at once.
template <int H>
__global__ void __launch_bounds__(H * 4) k_lstm_bwd(const float* __restrict__ dout, long long ldo,
                                                    const float* __restrict__ gates, const float* __restrict__ cells,
                                                    const float* __restrict__ w0, const float* __restrict__ w1,
                                                    long long B, int S, float* __restrict__ dp0,
                                                    float* __restrict__ dp1, long long ldp) {
  constexpr int LDG = 4 * H + 4;     // LDS row stride of the dP tile
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  float* ds = lds_dyn;               // [2][LROWS][LDG]

  const int d = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * LROWS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const int u = wave * 16 + j;
  const float* __restrict__ W = d ? w1 : w0;
  float* __restrict__ dP = d ? dp1 : dp0;

  // B operands of dh_rec = dP_t W_hh (K = 4 H, N = H): W_hh[q H + kk][u]
  float w[H];
#pragma unroll
  for (int kk = 0; kk < H; ++kk) w[kk] = W[(long long)(q * H + kk) * H + u];

  bool valid[4];
  long long rbase[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long row = row0 + 4 * q + r;
    valid[r] = row < B;
    rbase[r] = (valid[r] ? row : 0) * S;
  }
  const long long save_dir = (long long)d * B * S;

  auto load = [&](BwdIn& in, int t, bool has_prev) {
    const int tp = d ? t + 1 : t - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long row = rbase[r] + t;
#pragma unroll
      for (int g = 0; g < 4; ++g) in.g[g][r] = valid[r] ? gates[(save_dir + row) * (4 * H) + g * H + u] : 0.0f;
      in.cp[r] = (valid[r] && has_prev) ? cells[(save_dir + rbase[r] + tp) * H + u] : 0.0f;
      in.dy[r] = valid[r] ? dout[row * ldo + d * H + u] : 0.0f;
    }
  };

  BwdIn in, nx;
  float ct[4];
  float dcn[4] = {0.f, 0.f, 0.f, 0.f};
  floatx4 dhrec = {0.f, 0.f, 0.f, 0.f};
  {
    const int t = d ? 0 : S - 1;
    load(in, t, S > 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) ct[r] = valid[r] ? cells[(save_dir + rbase[r] + t) * H + u] : 0.0f;
  }

  for (int s = 0; s < S; ++s) {
    const int t = d ? s : S - 1 - s;
    float* tile = ds + (s & 1) * (LROWS * LDG);
    if (s + 1 < S) load(nx, d ? t + 1 : t - 1, s + 2 < S);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = in.g[0][r], gf = in.g[1][r], gg = in.g[2][r], go = in.g[3][r];
      const float dh = in.dy[r] + dhrec[r];
      const float tc = tanh_bf(ct[r]);
      const float dc = fmaf(dh * go, fmaf(-tc, tc, 1.0f), dcn[r]);
      const float di = dc * gg * gi * (1.0f - gi);
      const float df = dc * in.cp[r] * gf * (1.0f - gf);
      const float dg = dc * gi * fmaf(-gg, gg, 1.0f);
      const float dO = dh * tc * go * (1.0f - go);
      dcn[r] = dc * gf;
      float* tr = tile + (4 * q + r) * LDG + u;
      tr[0] = di;
      tr[H] = df;
      tr[2 * H] = dg;
      tr[3 * H] = dO;
      if (valid[r]) {
        float* gr = dP + (rbase[r] + t) * ldp + u;
        gr[0] = di;
        gr[H] = df;
        gr[2 * H] = dg;
        gr[3 * H] = dO;
      }
      ct[r] = in.cp[r];              // the next step processed is the forward's previous one
    }
    __syncthreads();                 // dP_t is complete; this tile is free again after the NEXT barrier
    if (s + 1 < S) {
      // four independent accumulator chains (k-step 4 k4 + e on chain e), summed in a fixed order
      floatx4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const float* arow = tile + j * LDG + q * H;
#pragma unroll
      for (int k4 = 0; k4 < H / 4; ++k4) {
        const floatx4 a = *reinterpret_cast<const floatx4*>(arow + 4 * k4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = mfma4(a[e], w[4 * k4 + e], acc[e]);
      }
      dhrec = (acc[0] + acc[1]) + (acc[2] + acc[3]);
      in = nx;
    }
  }
}

inline bool lstm_args(long long B, int S, int H, int dirs) {
  return H >= 16 && H <= 128 && H % 16 == 0 && S >= 1 && B >= 1 && (dirs == 1 || dirs == 2) &&
         (B + LROWS - 1) / LROWS <= 0x7fffffffLL && B <= 0x7fffffffffffLL / S / (4 * H) / 2;
}

template <int H>
int lstm_fwd_launch(const float* p0, const float* p1, long long ldp, const float* w0, const float* w1, const float* b0,
                    const float* b1, long long B, int S, int dirs, float* out, long long ldo, float* gates,
                    float* cells, hipStream_t st) {
  const dim3 grid((unsigned)((B + LROWS - 1) / LROWS), (unsigned)dirs);
  return bcnf_rt::launch<k_lstm_fwd<H>>(grid, dim3(H * 4), 0, st, p0, p1, ldp, w0, w1, b0, b1, B, S, out, ldo, gates,
                                        cells);
}

template <int H>
int lstm_bwd_launch(const float* dout, long long ldo, const float* gates, const float* cells, const float* w0,
                    const float* w1, long long B, int S, int dirs, float* dp0, float* dp1, long long ldp,
                    hipStream_t st) {
  const dim3 grid((unsigned)((B + LROWS - 1) / LROWS), (unsigned)dirs);
  const size_t lds = (size_t)2 * LROWS * (4 * H + 4) * sizeof(float);
  return bcnf_rt::launch<k_lstm_bwd<H>>(grid, dim3(H * 4), bcnf_rt::Lds(lds), st, dout, ldo, gates, cells, w0, w1, B, S,
                                        dp0, dp1, ldp);
}

// the weight registers of a lane have the compile-time size H
#define LSTM_DISPATCH(FN, ...)                 \
  switch (H) {                                 \
    case 16: return FN<16>(__VA_ARGS__);       \
    case 32: return FN<32>(__VA_ARGS__);       \
    case 48: return FN<48>(__VA_ARGS__);       \
    case 64: return FN<64>(__VA_ARGS__);       \
    case 80: return FN<80>(__VA_ARGS__);       \
    case 96: return FN<96>(__VA_ARGS__);       \
    case 112: return FN<112>(__VA_ARGS__);     \
    case 128: return FN<128>(__VA_ARGS__);     \
    default: return BCNF_ERR_ARG;              \
  }

}  // namespace

extern "C" {

int bcnf_lstm_forward(const float* p_fwd, const float* p_rev, int64_t ldp, const float* w_hh_fwd,
                      const float* w_hh_rev, const float* b_hh_fwd, const float* b_hh_rev, int64_t batch,
                      int32_t seq_len, int32_t hidden, int32_t dirs, float* out, int64_t ldo, float* gates,
                      float* cells, void* stream) {
  const int H = hidden;
  if (!lstm_args(batch, seq_len, H, dirs) || !p_fwd || !w_hh_fwd || !out || (dirs == 2 && (!p_rev || !w_hh_rev)) ||
      ldp < 4LL * H || ldo < (long long)dirs * H || (gates == nullptr) != (cells == nullptr))
    return BCNF_ERR_ARG;
  LSTM_DISPATCH(lstm_fwd_launch, p_fwd, p_rev, (long long)ldp, w_hh_fwd, w_hh_rev, b_hh_fwd, b_hh_rev, (long long)batch,
                seq_len, dirs, out, (long long)ldo, gates, cells, (hipStream_t)stream);
}

int bcnf_lstm_backward(const float* dout, int64_t ldo, const float* gates, const float* cells, const float* w_hh_fwd,
                       const float* w_hh_rev, int64_t batch, int32_t seq_len, int32_t hidden, int32_t dirs,
                       float* dp_fwd, float* dp_rev, int64_t ldp, void* stream) {
  const int H = hidden;
  if (!lstm_args(batch, seq_len, H, dirs) || !dout || !gates || !cells || !w_hh_fwd || !dp_fwd ||
      (dirs == 2 && (!w_hh_rev || !dp_rev)) || ldp < 4LL * H || ldo < (long long)dirs * H)
    return BCNF_ERR_ARG;
  LSTM_DISPATCH(lstm_bwd_launch, dout, (long long)ldo, gates, cells, w_hh_fwd, w_hh_rev, (long long)batch, seq_len,
                dirs, dp_fwd, dp_rev, (long long)ldp, (hipStream_t)stream);
}

}  // extern "C"
