// The camera of the videos_* configs (psaegert/bcnf src/bcnf/simulation/camera.py:74-150, looped over the frames by
// record_trajectory, camera.py:30-71, and over two cameras per sample by generate_data, sampling.py:366-368): every
// frame of a batch in ONE launch.
//
// camera() per frame: 5000 points N(ball_pos, (radius / 1.644854)^2 I), v = normalise(point - cam_pos),
//   ph = arctan2(v . cam_orthogonal, v . cam_dir), th = arctan2(v . cam_orthogonal_z, v . cam_dir),
//   np.histogram2d(ph, th, bins = [160, 90], range = [[-phi, phi], [-theta, theta]]), normalised by its sum (all zeros
//   when empty), returned as np.flipud(vals.T): pixel (row 89 - th_bin, column ph_bin).
//
// One workgroup per frame, fp64 geometry:
//   * the 90 x 160 histogram is 14,400 32-bit counters in LDS (57.6 KB) filled with LDS atomics -- no global atomics;
//     the two edge tables (np.linspace, built by the caller) sit beside it (2 KB), so two workgroups share a CU;
//   * a sample's draws are Philox4x32-10 of (sample index, first_frame + frame, offset) keyed by the seed (the rule is
//     stated at bcnf_render_frames in include/bcnf_amd.h and restated in numpy by bcnf_amd/render.py:standard_normals);
//     they do not depend on the launch's size or on which slice of a batch the launch renders;
//   * the bin is a multiply-and-floor guess corrected against the edge table, so the sample lands where
//     np.searchsorted(edges, x, 'right') - 1 puts it (half-open bins, the last edge included, outside dropped);
//   * the image is written once, 16 bytes per lane, already flipped and transposed: count / n_in divided in fp64 and
//     rounded once to the output type. A frame with n_in == 0 (the ball is out of view) never reads its histogram back:
//     it only writes zeros.
// 512 threads (8 waves) per workgroup at no more than 128 VGPRs: with the LDS's two workgroups per CU that is 4 waves
// per SIMD, which the fp64 log / sincos / atan2 dependency chains need more than the ~10 samples a thread draws.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bcnf_amd.h"
#include "bcnf_device.h"

namespace {

constexpr int NPH = BCNF_RENDER_WIDTH, NTH = BCNF_RENDER_HEIGHT, NPIX = NPH * NTH;
constexpr int RENDER_WG = 512;
static_assert(NPH % 4 == 0, "a 16-byte store stays inside one image row");

struct RenderArgs {
  const double* ball;        // [F][3]
  const int32_t* cam_index;  // [F]
  const double* sigma;       // [F]
  const double* cam_pos;     // [C][3]
  const double* basis;       // [C][3][3]: cam_dir, cam_orthogonal (ph axis), cam_orthogonal_z (th axis)
  const double* ph_edges;    // [NPH + 1]
  const double* th_edges;    // [NTH + 1]
  int n_cams, n_samples;
  uint32_t key0, key1, off_lo, off_hi, first_frame;
  const uint32_t* frame_index;     // [F] draw-rule frame indices, or NULL: first_frame + f
  void* images;              // [F][NTH][NPH] float or double
  int32_t* counts;           // [F][NTH][NPH], optional
  int32_t* n_in;             // [F], optional
};

// A uniform strictly inside (0, 1) from one 32-bit word, exact in fp64: (w + 1/2) 2^-32.
__device__ __forceinline__ double unit_open(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

// np.searchsorted(edges, x, 'right') - 1 for x inside [edges[0], edges[n]], the last edge counted into bin n - 1:
// the guess floor((x - edges[0]) * inv_width) is at most a bin off; the loops settle it against the table itself.
__device__ __forceinline__ int bin_of(const double* edges, int n, double inv_width, double x) {
  int b = (int)((x - edges[0]) * inv_width);
  b = b < 0 ? 0 : (b > n - 1 ? n - 1 : b);
  while (b > 0 && x < edges[b]) --b;
  while (b < n - 1 && x >= edges[b + 1]) ++b;
  return b;
}

template <typename TO>
struct Vec16;
template <>
struct Vec16<float> {
  typedef float type __attribute__((ext_vector_type(4)));
  static constexpr int N = 4;
};
template <>
struct Vec16<double> {
  typedef double type __attribute__((ext_vector_type(2)));
  static constexpr int N = 2;
};

// IMAGES = false is the lit-frame pass (bcnf_render_lit): the same draws, geometry and range test, n_in only -- no
// histogram, so no bins, no 57.6 KB of LDS and no image traffic.
template <typename TO, bool IMAGES>
__global__ __launch_bounds__(RENDER_WG, 4) void k_render(const RenderArgs a) {
  __shared__ uint32_t hist[IMAGES ? NPIX : 4];     // [th_bin][ph_bin]
  __shared__ double s_ph[NPH + 1], s_th[NTH + 1];
  __shared__ uint32_t s_n;
  const int f = blockIdx.x, tid = threadIdx.x;
  if constexpr (IMAGES) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4* h4 = reinterpret_cast<u32x4*>(hist);
    for (int e = tid; e < NPIX / 4; e += RENDER_WG) h4[e] = u32x4{0u, 0u, 0u, 0u};
  }
  for (int e = tid; e <= NPH; e += RENDER_WG) s_ph[e] = a.ph_edges[e];
  for (int e = tid; e <= NTH; e += RENDER_WG) s_th[e] = a.th_edges[e];
  if (tid == 0) s_n = 0;
  const int cam = a.cam_index[f];
  const bool cam_ok = cam >= 0 && cam < a.n_cams;     // wave-uniform; a frame with a bad index is empty, n_in = -1
  const int cc = cam_ok ? cam : 0;
  double cp[3], bs[9], bp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cp[c] = a.cam_pos[3 * cc + c];
    bp[c] = a.ball[3 * (long long)f + c];
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) bs[c] = a.basis[9 * cc + c];
  const double sigma = a.sigma[f];
  __syncthreads();
  const double ph_lo = s_ph[0], ph_hi = s_ph[NPH], th_lo = s_th[0], th_hi = s_th[NTH];
  const double ph_iw = (double)NPH / (ph_hi - ph_lo), th_iw = (double)NTH / (th_hi - th_lo);
  const uint32_t frame = a.frame_index ? a.frame_index[f] : a.first_frame + (uint32_t)f;
  uint32_t mine = 0;
  if (cam_ok) {
    for (int s = tid; s < a.n_samples; s += RENDER_WG) {
      const uint4 w = philox4x32_10(make_uint4((uint32_t)s, frame, a.off_lo, a.off_hi), make_uint2(a.key0, a.key1));
      // Box-Muller: (z0, z1) from words 0, 1 and z2 from words 2, 3
      const double r0 = sqrt(-2.0 * log(unit_open(w.x))), r1 = sqrt(-2.0 * log(unit_open(w.z)));
      const double t0 = 6.283185307179586 * unit_open(w.y), t1 = 6.283185307179586 * unit_open(w.w);
      double sn, cs;
      sincos(t0, &sn, &cs);
      const double z[3] = {r0 * cs, r0 * sn, r1 * cos(t1)};
      double v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (bp[c] + sigma * z[c]) - cp[c];
      const double inv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] *= inv;
      const double d_dir = v[0] * bs[0] + v[1] * bs[1] + v[2] * bs[2];
      const double d_ph = v[0] * bs[3] + v[1] * bs[4] + v[2] * bs[5];
      const double d_th = v[0] * bs[6] + v[1] * bs[7] + v[2] * bs[8];
      const double ph = atan2(d_ph, d_dir), th = atan2(d_th, d_dir);
      if (ph >= ph_lo && ph <= ph_hi && th >= th_lo && th <= th_hi) {      // false for a NaN, as numpy drops it
        if constexpr (IMAGES) {
          const int bph = bin_of(s_ph, NPH, ph_iw, ph), bth = bin_of(s_th, NTH, th_iw, th);
          atomicAdd(&hist[bth * NPH + bph], 1u);
        }
        ++mine;
      }
    }
  }
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  const uint32_t n = s_n;
  if (tid == 0 && a.n_in) a.n_in[f] = cam_ok ? (int32_t)n : -1;
  if constexpr (!IMAGES) return;
  typedef typename Vec16<TO>::type vec_t;
  constexpr int VN = Vec16<TO>::N;
  vec_t* img = reinterpret_cast<vec_t*>(static_cast<TO*>(a.images) + (long long)f * NPIX);
  typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
  i32x4* cnt = a.counts ? reinterpret_cast<i32x4*>(a.counts + (long long)f * NPIX) : nullptr;
  if (n == 0) {                                     // uniform: nothing of the histogram is read back
    vec_t zero;
#pragma unroll
    for (int j = 0; j < VN; ++j) zero[j] = (TO)0;
    for (int e = tid; e < NPIX / VN; e += RENDER_WG) img[e] = zero;
    if (cnt)
      for (int e = tid; e < NPIX / 4; e += RENDER_WG) cnt[e] = i32x4{0, 0, 0, 0};
    return;
  }
  const double dn = (double)n;
  for (int e = tid; e < NPIX / VN; e += RENDER_WG) {
    const int p = e * VN, row = p / NPH, col = p - row * NPH;       // output pixel; its bin is (NTH - 1 - row, col)
    const uint32_t* src = hist + (NTH - 1 - row) * NPH + col;
    vec_t o;
#pragma unroll
    for (int j = 0; j < VN; ++j) o[j] = src[j] ? (TO)((double)src[j] / dn) : (TO)0;
    img[e] = o;
  }
  if (cnt)
    for (int e = tid; e < NPIX / 4; e += RENDER_WG) {
      const int p = e * 4, row = p / NPH, col = p - row * NPH;
      const uint32_t* src = hist + (NTH - 1 - row) * NPH + col;
      cnt[e] = i32x4{(int32_t)src[0], (int32_t)src[1], (int32_t)src[2], (int32_t)src[3]};
    }
}

}  // namespace

extern "C" {

static int render_launch(const double* ball_pos, const int32_t* cam_index, const double* sigma, int64_t n_frames,
                         const double* cam_pos, const double* basis, int32_t n_cams, const double* ph_edges,
                         const double* th_edges, int32_t n_samples, uint64_t seed, uint64_t offset, int64_t first_frame,
                         const uint32_t* frame_index, void* images, int32_t images_f64, int32_t* counts, int32_t* n_in,
                         bool lit_only, void* stream) {
  if (n_frames < 0 || n_cams < 0 || n_samples < 0 || first_frame < 0) return BCNF_ERR_ARG;
  if (n_frames == 0) return BCNF_OK;
  if ((!frame_index && first_frame + n_frames > 0x100000000LL) || n_frames > 0x7fffffffLL) return BCNF_ERR_UNSUPPORTED;
  if (!ball_pos || !cam_index || !sigma || !cam_pos || !basis || !ph_edges || !th_edges || n_cams < 1)
    return BCNF_ERR_ARG;
  if (lit_only ? !n_in : !images) return BCNF_ERR_ARG;
  if (((uintptr_t)images | (uintptr_t)counts) & 15) return BCNF_ERR_ARG;
  RenderArgs a;
  a.ball = ball_pos;
  a.cam_index = cam_index;
  a.sigma = sigma;
  a.cam_pos = cam_pos;
  a.basis = basis;
  a.ph_edges = ph_edges;
  a.th_edges = th_edges;
  a.n_cams = n_cams;
  a.n_samples = n_samples;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32) ^ 0xC0000000u;
  a.off_lo = (uint32_t)offset;
  a.off_hi = (uint32_t)(offset >> 32);
  a.first_frame = (uint32_t)first_frame;
  a.frame_index = frame_index;
  a.images = images;
  a.counts = counts;
  a.n_in = n_in;
  const dim3 grid((unsigned)n_frames), block(RENDER_WG);
  if (lit_only) return bcnf_rt::launch<k_render<float, false>>(grid, block, 0, (hipStream_t)stream, a);
  return images_f64 ? bcnf_rt::launch<k_render<double, true>>(grid, block, 0, (hipStream_t)stream, a)
                    : bcnf_rt::launch<k_render<float, true>>(grid, block, 0, (hipStream_t)stream, a);
}

int bcnf_render_frames(const double* ball_pos, const int32_t* cam_index, const double* sigma, int64_t n_frames,
                       const double* cam_pos, const double* basis, int32_t n_cams, const double* ph_edges,
                       const double* th_edges, int32_t n_samples, uint64_t seed, uint64_t offset, int64_t first_frame,
                       void* images, int32_t images_f64, int32_t* counts, int32_t* n_in, void* stream) {
  return render_launch(ball_pos, cam_index, sigma, n_frames, cam_pos, basis, n_cams, ph_edges, th_edges, n_samples, seed,
                       offset, first_frame, nullptr, images, images_f64, counts, n_in, false, stream);
}

int bcnf_render_frames_at(const double* ball_pos, const int32_t* cam_index, const double* sigma, int64_t n_frames,
                          const double* cam_pos, const double* basis, int32_t n_cams, const double* ph_edges,
                          const double* th_edges, int32_t n_samples, uint64_t seed, uint64_t offset,
                          const uint32_t* frame_index, void* images, int32_t images_f64, int32_t* counts, int32_t* n_in,
                          void* stream) {
  if (!frame_index && n_frames > 0) return BCNF_ERR_ARG;
  return render_launch(ball_pos, cam_index, sigma, n_frames, cam_pos, basis, n_cams, ph_edges, th_edges, n_samples, seed,
                       offset, 0, frame_index, images, images_f64, counts, n_in, false, stream);
}

int bcnf_render_lit(const double* ball_pos, const int32_t* cam_index, const double* sigma, int64_t n_frames,
                    const double* cam_pos, const double* basis, int32_t n_cams, const double* ph_edges,
                    const double* th_edges, int32_t n_samples, uint64_t seed, uint64_t offset, int64_t first_frame,
                    const uint32_t* frame_index, int32_t* n_in, void* stream) {
  return render_launch(ball_pos, cam_index, sigma, n_frames, cam_pos, basis, n_cams, ph_edges, th_edges, n_samples, seed,
                       offset, first_frame, frame_index, nullptr, 0, nullptr, n_in, true, stream);
}

}  // extern "C"
