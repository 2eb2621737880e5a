// The ballistic velocity ODE (psaegert/bcnf src/bcnf/simulation/physics.py:42, ballistic_ODE) and one attempt of the
// adaptive Dormand-Prince 5(4) pair that integrates it: shared by k_resim (bcnf_resim.hip, physics_ODE_simulation) and
// k_candidates (bcnf_generate.hip, calculate_point_of_impact). Include inside the translation unit's anonymous
// namespace; fp64 throughout, no memory traffic.
#ifndef BCNF_ODE_H
#define BCNF_ODE_H

struct Phys {
  double gb[3], a[3], wt[3], kd;
};

// ballistic_ODE (physics.py:42): (g - buoyancy) - kd (v^2 v / |v| - w^2 w / |w|) + a
__device__ __forceinline__ void rhs(const Phys& P, const double v[3], double d[3]) {
  const double inv = rsqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);     // 1 / |v| (no fp64 division)
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = P.gb[c] - P.kd * (v[c] * v[c] * v[c] * inv - P.wt[c]) + P.a[c];
}

// Dormand-Prince 5(4) tableau
constexpr double A21 = 1.0 / 5;
constexpr double A31 = 3.0 / 40, A32 = 9.0 / 40;
constexpr double A41 = 44.0 / 45, A42 = -56.0 / 15, A43 = 32.0 / 9;
constexpr double A51 = 19372.0 / 6561, A52 = -25360.0 / 2187, A53 = 64448.0 / 6561, A54 = -212.0 / 729;
constexpr double A61 = 9017.0 / 3168, A62 = -355.0 / 33, A63 = 46732.0 / 5247, A64 = 49.0 / 176,
                 A65 = -5103.0 / 18656;
constexpr double B1 = 35.0 / 384, B3 = 500.0 / 1113, B4 = 125.0 / 192, B5 = -2187.0 / 6784, B6 = 11.0 / 84;
constexpr double E1 = 71.0 / 57600, E3 = -71.0 / 16695, E4 = 71.0 / 1920, E5 = -17253.0 / 339200, E6 = 22.0 / 525,
                 E7 = -1.0 / 40;

__device__ __forceinline__ bool finite3(const double v[3]) {
  return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
}

// One Dormand-Prince attempt over [t, t + hh] from v (k1 = f(v), FSAL). Returns the squared RMS error norm and
// writes vn and k7 = f(vn).
__device__ __forceinline__ float dp_attempt(const Phys& P, const double v[3], const double k1[3], double hh,
                                            double rtol, double atol, double vn[3], double k7[3]) {
  double y[3], k2[3], k3[3], k4[3], k5[3], k6[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = v[c] + hh * (A21 * k1[c]);
  rhs(P, y, k2);
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = v[c] + hh * (A31 * k1[c] + A32 * k2[c]);
  rhs(P, y, k3);
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = v[c] + hh * (A41 * k1[c] + A42 * k2[c] + A43 * k3[c]);
  rhs(P, y, k4);
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = v[c] + hh * (A51 * k1[c] + A52 * k2[c] + A53 * k3[c] + A54 * k4[c]);
  rhs(P, y, k5);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    y[c] = v[c] + hh * (A61 * k1[c] + A62 * k2[c] + A63 * k3[c] + A64 * k4[c] + A65 * k5[c]);
  rhs(P, y, k6);
#pragma unroll
  for (int c = 0; c < 3; ++c) vn[c] = v[c] + hh * (B1 * k1[c] + B3 * k3[c] + B4 * k4[c] + B5 * k5[c] + B6 * k6[c]);
  rhs(P, vn, k7);
  // squared RMS error norm in fp32: it only steers the step size (accept / shrink), so its rounding never reaches the
  // solution beyond the tolerance it enforces; no fp64 division, square root or pow
  float en2 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double e = hh * (E1 * k1[c] + E3 * k3[c] + E4 * k4[c] + E5 * k5[c] + E6 * k6[c] + E7 * k7[c]);
    const double sc = atol + rtol * fmax(fabs(v[c]), fabs(vn[c]));
    const float q = (float)e * __builtin_amdgcn_rcpf((float)sc);
    en2 += q * q;
  }
  return en2 * (1.f / 3.f);
}

#endif  // BCNF_ODE_H
