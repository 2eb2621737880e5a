// The candidates of generate_data (psaegert/bcnf src/bcnf/simulation/sampling.py:287-410): the prior draws of
// sample_ballistic_parameters (sampling.py:156-284), the runaway and underground tests, calculate_point_of_impact
// (physics.py:246-276) and accept_traveled_distance (sampling.py:145-153) for a range of candidates in ONE launch. The
// reference runs one Python iteration per candidate with up to 1200 odeint calls in it.
//
// Draws: the counter-based rule stated at bcnf_sample_candidates in include/bcnf_amd.h and restated in numpy by
// bcnf_amd/generate.py:sample_candidates_host -- Philox4x32-10 of (candidate, slot, attempt) keyed by the seed, so a
// candidate's row depends on (seed, candidate) and the prior tables only, never on the launch it ran in.
//
// A workgroup is one wave and owns GTILE consecutive candidates, in two phases:
//   A  sampling, one thread per candidate, GTILE / 64 rounds. The slot loop is wave-uniform (a slot's distribution and
//      transformation are kernel arguments); only the Marsaglia-Tsang rejection loop diverges (about 1 attempt in 20).
//      The slot values of a round sit in LDS ([slot][lane], 64-bit words: conflict-free), so the loop needs no register
//      array indexed by a loop variable. The row, the reject code (runaway / underground) and NaN for the point of
//      impact go to global memory.
//   B  the march, for the candidates still pending. Flight times differ by two orders of magnitude (a ball that drops
//      from 0.1 m takes 2 intervals of 0.1 s, one whose buoyancy exceeds its weight takes all 1200), so a fixed
//      thread-to-candidate mapping would leave most lanes of every wave idle behind its longest flight. Instead a lane
//      that finishes its candidate takes the tile's next one from an LDS counter, and the loop body is ONE
//      Dormand-Prince attempt, the only expensive piece, which every busy lane executes together. A wave therefore runs
//      for about max(longest flight, tile's total attempts / 64) instead of GTILE / 64 longest flights.
// The march is the reference's: x <- x + v dt with the velocity at the START of the interval, v integrated over
// [t, t + dt] (dt = 0.1, t accumulated as the reference accumulates it) by the pair k_resim uses (bcnf_ode.h), impact
// x + v (-x.z / v.z) at the first z < 0, (999, 999, 999) after 120 s or once the velocity is not finite (a NaN position
// never satisfies z < 0, so the reference's loop runs out).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bcnf_amd.h"
#include "bcnf_device.h"

namespace {

#include "bcnf_ode.h"     // Phys, rhs, the Dormand-Prince tableau, finite3, dp_attempt

constexpr int GWG = 64;                       // one wave per workgroup
constexpr int GTILE = 512;                    // candidates per workgroup: 8 sampling rounds, then one shared march queue
constexpr int NSLOT = BCNF_GEN_NSLOT, NCOL = BCNF_GEN_NCOL;
constexpr int GAMMA_MAX_ATTEMPTS = 1000;      // the rule's bound (a shape >= 1/3 accepts 19 attempts in 20)

struct CandArgs {
  int32_t kind[NSLOT];       // BCNF_GEN_UNIFORM / GAUSSIAN / GAMMA
  int32_t xf[NSLOT];         // BCNF_GEN_XF_*
  double p0[NSLOT], p1[NSLOT];     // min, max | mean, std | shape, scale
  uint32_t key0, key1;
  long long first, count;
  int do_filter, max_attempts;
  double rtol, atol, cam1_radian;
  double* params;            // [count][NCOL]
  double* poi;               // [count][3]
  double* dist;              // [count]
  int32_t* code;             // [count]
};

__device__ __forceinline__ double unit_open(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

__device__ __forceinline__ double box_muller(uint32_t w0, uint32_t w1) {
  return sqrt(-2.0 * log(unit_open(w0))) * cos(6.283185307179586 * unit_open(w1));
}

// One slot of one candidate: the raw draw of its distribution, then the slot's transformation.
__device__ __forceinline__ double draw_slot(const CandArgs& a, int s, uint32_t c_lo, uint32_t c_hi) {
  const uint2 key = make_uint2(a.key0, a.key1);
  const int kind = a.kind[s];
  const double p0 = a.p0[s], p1 = a.p1[s];
  double raw;
  if (kind == BCNF_GEN_GAMMA) {
    // Marsaglia-Tsang (2000) without the squeeze: d = k - 1/3 (k = shape, or shape + 1 below 1), c = 1 / sqrt(9 d)
    const double k = p0 < 1.0 ? p0 + 1.0 : p0;
    const double d = k - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    raw = __builtin_nan("");
    for (int att = 0; att < GAMMA_MAX_ATTEMPTS; ++att) {
      const uint4 w = philox4x32_10(make_uint4(c_lo, c_hi, (uint32_t)s, (uint32_t)att), key);
      const double x = box_muller(w.x, w.y);
      const double t = 1.0 + c * x, v = t * t * t;
      if (v > 0.0 && log(unit_open(w.z)) < 0.5 * x * x + d - d * v + d * log(v)) {
        raw = d * v;
        if (p0 < 1.0) raw *= pow(unit_open(w.w), 1.0 / p0);
        raw *= p1;
        break;
      }
    }
  } else {
    const uint4 w = philox4x32_10(make_uint4(c_lo, c_hi, (uint32_t)s, 0u), key);
    raw = kind == BCNF_GEN_GAUSSIAN ? box_muller(w.x, w.y) : p0 + (p1 - p0) * unit_open(w.x);
  }
  switch (a.xf[s]) {       // wave-uniform
    case BCNF_GEN_XF_SQRT_ABS: return sqrt(fabs(raw)) * p1 + p0;
    case BCNF_GEN_XF_AFFINE: return raw * p1 + p0;
    case BCNF_GEN_XF_CBRT_ABS: return cbrt(fabs(raw)) * p1 + p0;
    case BCNF_GEN_XF_SQRT: return sqrt(raw);
    default: return raw;
  }
}

__global__ __launch_bounds__(GWG) void k_candidates(const CandArgs a) {
  __shared__ double sv[NSLOT * GWG];
  __shared__ int s_next;
  const int lane = threadIdx.x;
  const long long base = (long long)blockIdx.x * GTILE;
  const int ntile = a.count - base < GTILE ? (int)(a.count - base) : GTILE;
  if (lane == 0) s_next = 0;
  const double qnan = __builtin_nan("");

  // ---- phase A: the rows --------------------------------------------------------------------------------------------
  for (int r0 = 0; r0 < ntile; r0 += GWG) {
    const int j = r0 + lane;
    const bool live = j < ntile;
    const unsigned long long cand = (unsigned long long)(a.first + base + (live ? j : 0));
    const uint32_t c_lo = (uint32_t)cand, c_hi = (uint32_t)(cand >> 32);
    for (int s = 0; s < NSLOT; ++s) sv[s * GWG + lane] = draw_slot(a, s, c_lo, c_hi);
    // a lane reads back its own column only: no barrier
#define SV(s) sv[(s) * GWG + lane]
    if (live) {
      double* row = a.params + (base + j) * NCOL;
      double sn, cs;
      sincos(SV(1), &sn, &cs);
      const double x0z = SV(2);
      row[0] = SV(0) * cs;
      row[1] = SV(0) * sn;
      row[2] = x0z;
      sincos(SV(4), &sn, &cs);
      row[3] = SV(3) * cs;
      row[4] = SV(3) * sn;
      row[5] = SV(5);
      sincos(SV(7), &sn, &cs);
      row[9] = SV(6) * cs;
      row[10] = SV(6) * sn;
      row[11] = SV(8);
      double st, ct;
      sincos(SV(10), &sn, &cs);
      sincos(SV(11), &st, &ct);
      const double ra = SV(9), az = ra * ct;
      row[14] = ra * st * cs;
      row[15] = ra * st * sn;
      row[16] = az;
      const double gz = -SV(12), rho = SV(13), r = SV(14), A = M_PI * (r * r), Cd = SV(15);
      row[6] = 0.0;
      row[7] = 0.0;
      row[8] = gz;
      row[12] = rho * A * Cd;
      row[13] = SV(16);
      row[17] = a.cam1_radian;
      row[18] = SV(17);
      row[19] = r;
      row[20] = A;
      row[21] = Cd;
      row[22] = rho;
#pragma unroll
      for (int q = 0; q < 7; ++q) row[23 + q] = SV(18 + q);      // cam_radius, cam_angles, cam_heights, the two uniforms
      int code = BCNF_GEN_PENDING;
      if (a.do_filter) code = gz + az > 0.0 ? BCNF_GEN_RUNAWAY : (x0z < 0.0 ? BCNF_GEN_UNDERGROUND : BCNF_GEN_PENDING);
      a.code[base + j] = code;
      a.dist[base + j] = qnan;
#pragma unroll
      for (int c = 0; c < 3; ++c) a.poi[(base + j) * 3 + c] = qnan;
    }
#undef SV
  }
  if (!a.do_filter) return;        // every candidate stays pending, nothing marches
  __syncthreads();                 // the rows and codes of this tile, written by this workgroup, are visible to it

  // ---- phase B: the march, lanes refilled from the tile's queue ----------------------------------------------------
  constexpr double DT = 0.1;       // calculate_point_of_impact's default; generate_data passes none
  bool have = false;
  long long idx = 0;
  Phys P;
  double x[3], vs[3], v[3], k1[3];     // position, velocity at the start of the interval, running velocity, f(v)
  double t = 0.0, tau = 0.0, len = 0.0, h = 0.0, udist = 0.0, x00 = 0.0, x01 = 0.0, x02 = 0.0;
  int tries = 0;
  for (;;) {
    if (!have) {
      const int j = atomicAdd(&s_next, 1);
      if (j >= ntile) break;
      idx = base + j;
      if (a.code[idx] != BCNF_GEN_PENDING) continue;
      const double* row = a.params + idx * NCOL;
      const double b = row[12], m = row[13], rho = row[22], r = row[19];
      const double w[3] = {row[9], row[10], row[11]};
      const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double g = row[6 + c];
        P.gb[c] = g - g * rho * (4.0 / 3.0) * (M_PI * (r * r * r)) / m;
        P.wt[c] = w[c] * w[c] * w[c] / nw;
        P.a[c] = row[14 + c];
        x[c] = row[c];
        vs[c] = v[c] = row[3 + c];
      }
      P.kd = 0.5 * b / m;
      udist = row[28];
      x00 = x[0], x01 = x[1], x02 = x[2];
      rhs(P, v, k1);
      t = 0.0;
      tau = 0.0;
      len = (t + DT) - t;
      h = 0.25 * DT;
      tries = 0;
      have = true;
    }
    // one attempt inside the interval [t, t + len); `bad` ends the interval with a velocity that is not finite
    bool done = false, bad = !finite3(k1) || !finite3(v);
    if (!bad) {
      bool last = false;
      double hh = h;
      if (hh >= len - tau) { hh = len - tau; last = true; }
      double vn[3], k7[3];
      const float en2 = dp_attempt(P, v, k1, hh, a.rtol, a.atol, vn, k7);
      const float fac0 = 0.9f * __builtin_amdgcn_exp2f(-0.1f * __builtin_amdgcn_logf(en2));
      if (!(en2 <= 1.f) || !finite3(vn)) {
        h = hh * (double)(en2 < INFINITY ? fmaxf(0.2f, fac0) : 0.2f);
        if (++tries > a.max_attempts || !(h > 1e-13 * len)) bad = true;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c] = vn[c];
          k1[c] = k7[c];
        }
        tau = last ? len : tau + hh;
        done = last;
        const double fac = en2 > 0.f ? (double)fminf(5.f, fmaxf(0.2f, fac0)) : 5.0;
        if (!last || fac < 1.0) h = hh * fac;
        if (++tries > a.max_attempts && !done) bad = true;
      }
    }
    if (done || bad) {             // physics.py:259-273: the position moves with the interval's starting velocity
      double xn[3], out[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) xn[c] = x[c] + vs[c] * DT;
      bool finished = false;
      if (xn[2] < 0.0) {
        const double ti = -x[2] / vs[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = x[c] + vs[c] * ti;
        finished = true;
      } else {
        t += DT;
        if (bad || !(t < 120.0)) {
          out[0] = out[1] = out[2] = 999.0;
          finished = true;
        }
      }
      if (finished) {
        const double d0 = out[0] - x00, d1 = out[1] - x01, d2 = out[2] - x02;
        const double dist = sqrt(d0 * d0 + d1 * d1 + d2 * d2), ratio = dist / 50.0;
        const bool accept = ratio > 0.75 || sqrt(ratio) > udist;      // sampling.py:145-153, NaN rejects
#pragma unroll
        for (int c = 0; c < 3; ++c) a.poi[idx * 3 + c] = out[c];
        a.dist[idx] = dist;
        if (!accept) a.code[idx] = BCNF_GEN_DISTANCE;
        have = false;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          x[c] = xn[c];
          vs[c] = v[c];
        }
        tau = 0.0;
        len = (t + DT) - t;
      }
    }
  }
}

}  // namespace

extern "C" {

int bcnf_sample_candidates(const int32_t* kind, const int32_t* transform, const double* p0, const double* p1,
                           uint64_t seed, int64_t first_candidate, int64_t n_candidates, double cam1_radian,
                           int32_t do_filter, double rtol, double atol, int32_t max_attempts, double* params,
                           double* poi, double* distance, int32_t* code, void* stream) {
  if (n_candidates < 0 || first_candidate < 0 || !kind || !transform || !p0 || !p1 || !(rtol > 0.0) || !(atol > 0.0) ||
      max_attempts < 1)
    return BCNF_ERR_ARG;
  if (n_candidates == 0) return BCNF_OK;
  if (!params || !poi || !distance || !code) return BCNF_ERR_ARG;
  CandArgs a;
  for (int s = 0; s < NSLOT; ++s) {
    if (kind[s] < BCNF_GEN_UNIFORM || kind[s] > BCNF_GEN_GAMMA || transform[s] < BCNF_GEN_XF_NONE ||
        transform[s] > BCNF_GEN_XF_SQRT)
      return BCNF_ERR_ARG;
    if (kind[s] == BCNF_GEN_GAMMA && !(p0[s] > 0.0)) return BCNF_ERR_ARG;
    a.kind[s] = kind[s];
    a.xf[s] = transform[s];
    a.p0[s] = p0[s];
    a.p1[s] = p1[s];
  }
  const long long nwg = (n_candidates + GTILE - 1) / GTILE;
  if (nwg > 0x7fffffffLL || first_candidate > INT64_MAX - n_candidates) return BCNF_ERR_UNSUPPORTED;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32) ^ BCNF_GEN_KEY_TAG;
  a.first = first_candidate;
  a.count = n_candidates;
  a.do_filter = do_filter ? 1 : 0;
  a.max_attempts = max_attempts;
  a.rtol = rtol;
  a.atol = atol;
  a.cam1_radian = cam1_radian;
  a.params = params;
  a.poi = poi;
  a.dist = distance;
  a.code = code;
  return bcnf_rt::launch<k_candidates>(dim3((unsigned)nwg), dim3(GWG), 0, (hipStream_t)stream, a);
}

}  // extern "C"
