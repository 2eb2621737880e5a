// Validation statistics of one batch (Trainer._validate_batch, trainer.py:279-303, and the values _train logs from
// its last batch, trainer.py:213-217): from z (B x D), log|det J| (B) and optionally the prediction head's output and
// its target (B x D each), ONE launch writes the row
//   [loss, nll, mse, mean(ldj), z.mean(0)[D], z.std(0)[D]]
// and adds (loss, nll, mse) as doubles into an epoch sum.
//
// One workgroup of 1024 threads. A validation batch is a few thousand floats (B = 256, D = 19: 19 KB), so the launch
// is latency, not bandwidth: a second workgroup could only add a hand-off between workgroups -- a ticket, a fence and
// a cold re-read of the partials -- to a kernel whose whole input one CU streams from L2 in a few microseconds. Within
// the workgroup thread t owns column t & 31 of the rows t >> 5, t >> 5 + 32, ...: a wave reads two whole rows per
// step, and every sum is fp64 in an order fixed by (B, D) alone -- lane pairs by xor-shuffle, the 16 waves in index
// order by one thread per column -- so the same inputs give the same bits on every run. No atomics of any kind.
// The deviations are a second pass over z (L2-resident by then) around the fp64 mean, never sum(z^2) / B - mean^2.
#include "bcnf_device.h"

namespace {

using bcnf_rt::launch;

constexpr int VWG = 1024;            // 16 waves
constexpr int VWAVES = VWG / 64;
constexpr int VCOLS = 32;            // D <= 32: the stack's own limit
constexpr int VGROUPS = VWG / VCOLS; // row groups

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(VWG) void k_validation_stats(const float* __restrict__ z, const float* __restrict__ ldj,
                                                          const float* __restrict__ pred, const float* __restrict__ y,
                                                          long long B, int D, float weight, float* __restrict__ row,
                                                          double* __restrict__ epoch_sum, long long* cursor,
                                                          long long n_batches) {
  __shared__ double col[VWAVES][VCOLS];   // per-wave column partials (pass 1: sum z, pass 2: sum (z - mean)^2)
  __shared__ double sc[VWAVES][3];        // per-wave partials of sum z^2, sum ldj, sum (pred - y)^2
  __shared__ double mean[VCOLS];
  __shared__ double tot[3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = t & (VCOLS - 1), g = t >> 5;
  const bool live = c < D;

  double s1 = 0.0, s2 = 0.0;
  if (live)
    for (long long b = g; b < B; b += VGROUPS) {
      const double v = (double)z[b * D + c];
      s1 += v;
      s2 += v * v;
    }
  double sl = 0.0;
  for (long long b = t; b < B; b += VWG) sl += (double)ldj[b];
  double se = 0.0;
  if (pred) {
    const long long n = B * D;
    for (long long e = t; e < n; e += VWG) {
      const double d = (double)pred[e] - (double)y[e];
      se += d * d;
    }
  }
  s1 += __shfl_xor(s1, 32, 64);           // the wave's two row groups
  s2 = wave_sum(s2);
  sl = wave_sum(sl);
  se = wave_sum(se);
  if (lane < VCOLS) col[wave][lane] = s1;
  if (lane == 0) {
    sc[wave][0] = s2;
    sc[wave][1] = sl;
    sc[wave][2] = se;
  }
  __syncthreads();
  if (t < VCOLS) {
    double a = 0.0;
    for (int w = 0; w < VWAVES; ++w) a += col[w][t];
    mean[t] = a / (double)B;
  } else if (t < VCOLS + 3) {
    double a = 0.0;
    for (int w = 0; w < VWAVES; ++w) a += sc[w][t - VCOLS];
    tot[t - VCOLS] = a;
  }
  __syncthreads();

  double q = 0.0;
  if (live) {
    const double m = mean[c];
    for (long long b = g; b < B; b += VGROUPS) {
      const double d = (double)z[b * D + c] - m;
      q += d * d;
    }
  }
  q += __shfl_xor(q, 32, 64);
  __syncthreads();                         // every reader of pass 1's col is done
  if (lane < VCOLS) col[wave][lane] = q;
  __syncthreads();

  // an epoch cursor selects the row (one captured launch serves every batch of the epoch); thread 0 advances it last
  float* out = row + (cursor ? cursor[0] * (long long)(4 + 2 * D) : 0LL);
  if (t < D) {
    double a = 0.0;
    for (int w = 0; w < VWAVES; ++w) a += col[w][t];
    out[4 + t] = (float)mean[t];
    out[4 + D + t] = (float)sqrt(a / (double)(B - 1));      // torch.std's unbiased estimate; NaN at B = 1 (0 / 0)
  }
  __syncthreads();
  if (t != 0) return;
  {
#pragma clang fp contract(off)
    const float nll = (float)((0.5 * tot[0] - tot[1]) / (double)B);
    const float mse = pred ? (float)(tot[2] / ((double)B * (double)D)) : 0.0f;
    const float loss = (nll + mse * weight) / (1.0f + weight);      // trainer.py:301, an fp32 tensor expression
    out[0] = loss;
    out[1] = nll;
    out[2] = mse;
    out[3] = (float)(tot[1] / (double)B);
    if (epoch_sum) {      // after the row, in batch order (launches of one stream): the Trainer's `val_loss += loss`
      epoch_sum[0] += (double)loss;
      epoch_sum[1] += (double)nll;
      epoch_sum[2] += (double)mse;
    }
  }
  advance_counters(nullptr, cursor, n_batches);
}

}  // namespace

extern "C" {

int bcnf_validation_stats(const float* z, const float* ldj, const float* pred, const float* y, int64_t B, int32_t D,
                          float weight, float* row, double* epoch_sum, int64_t* cursor, int64_t n_batches,
                          void* stream) {
  if (!z || !ldj || !row || B < 1 || D < 1 || (pred == nullptr) != (y == nullptr) || !(weight >= 0.f) ||
      !(weight < 3.0e38f) || (cursor && n_batches < 1))
    return BCNF_ERR_ARG;
  if (D > VCOLS || B > (1LL << 40)) return BCNF_ERR_UNSUPPORTED;
  return launch<k_validation_stats>(dim3(1), dim3(VWG), 0, (hipStream_t)stream, z, ldj, pred, y, (long long)B, D,
                                    weight, row, epoch_sum, reinterpret_cast<long long*>(cursor),
                                    (long long)n_batches);
}

}  // extern "C"
