// Ray depth of a set of views (gfx950): per pixel, the depth of the point on the pixel's ray at which the density of the
// pixel's median Gaussian is largest -- the ray-Gaussian intersection depth of RaDe-GS and GOF -- where median.hip reports
// the depth of that Gaussian's centre.  A forward-only pass of its own, not differentiable; no tile kernel is involved.
//
// One lane per pixel, grid over C x H x W.  A lane reads the pixel's median id and median depth (median.hip's two maps),
// gathers the 40 B of that row (mean, quaternion, activated scales), evaluates ray_math.h in float64 and stores one
// float.  Neighbouring pixels share rows, so the gather is served by L2: the pass moves 12 B per pixel plus the touched
// rows.  A workgroup lies within one camera, so the camera record (16 doubles of a caller-made table) is read through
// wave-uniform addresses.  No LDS, no atomics, no cross-lane traffic, no scratch.
//
// An id outside [0, N) (median.hip's -1 where nothing is accumulated) gives 0.0 and reads no row.  Every pixel is written
// exactly once.
#include "common.h"
#include "ray_math.h"

namespace clmgs {

constexpr int RAY_BLOCK = 256;

__global__ void __launch_bounds__(RAY_BLOCK)
ray_depth_kernel(int N, int HW, int W, int blocks_per_cam, const float* __restrict__ means, const float* __restrict__ quats,
                 const float* __restrict__ scales, const double* __restrict__ cams, const int32_t* __restrict__ median_id,
                 const float* __restrict__ median_depth, double near, int ortho, float* __restrict__ ray_depth_out) {
  const int cam = blockIdx.x / blocks_per_cam;  // wave-uniform
  const int in_cam = (blockIdx.x - cam * blocks_per_cam) * RAY_BLOCK + threadIdx.x;
  if (in_cam >= HW) return;
  const size_t pix = (size_t)cam * HW + in_cam;
  const int id = median_id[pix];
  if ((unsigned)id >= (unsigned)N) {
    ray_depth_out[pix] = 0.f;
    return;
  }
  const float centre = median_depth[pix];
  const int py = in_cam / W, px = in_cam - py * W;
  const float* m = means + 3 * (size_t)id;
  const float* qr = quats + 4 * (size_t)id;
  const float* s = scales + 3 * (size_t)id;
  const double mu[3] = {(double)m[0], (double)m[1], (double)m[2]};
  const double q[4] = {(double)qr[0], (double)qr[1], (double)qr[2], (double)qr[3]};
  const double sc[3] = {(double)s[0], (double)s[1], (double)s[2]};
  ray_depth_out[pix] = ray_depth(mu, q, sc, cams + RAY_CAM_DOUBLES * (size_t)cam, (double)px, (double)py, ortho, near, centre);
}

__global__ void __launch_bounds__(RAY_BLOCK)
ray_depth_fill_kernel(int64_t n, float* __restrict__ ray_depth_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    ray_depth_out[i] = 0.f;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_ray_depth(void* stream, int C, int N, int height, int width, const float* means, const float* quats,
                               const float* scales, const double* cams, const int32_t* median_id,
                               const float* median_depth, double near_plane, int camera_model, float* ray_depth_out) {
  CLMGS_CHECK_ARG(C >= 0 && N >= 0 && width >= 0 && height >= 0);
  CLMGS_CHECK_ARG(camera_model == 0 || camera_model == 1);
  const int64_t HW = (int64_t)height * width;
  const int64_t blocks_per_cam = (HW + RAY_BLOCK - 1) / RAY_BLOCK;
  CLMGS_CHECK_ARG(HW <= INT32_MAX && (int64_t)C * HW <= INT32_MAX && (int64_t)C * blocks_per_cam <= INT32_MAX);
  const int64_t n_pix = (int64_t)C * HW;
  CLMGS_CHECK_ARG(n_pix == 0 || (ray_depth_out && median_id && median_depth && cams));
  CLMGS_CHECK_ARG(n_pix == 0 || N == 0 || (means && quats && scales));
  CLMGS_CHECK_ARG(((uintptr_t)cams & 7) == 0);
  if (n_pix == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {  // no rows: every id lies outside [0, N)
    const dim3 fgrid(min(ceil_div(n_pix, RAY_BLOCK), 256 * 8));
    hipLaunchKernelGGL(ray_depth_fill_kernel, fgrid, dim3(RAY_BLOCK), 0, s, n_pix, ray_depth_out);
    CLMGS_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(ray_depth_kernel, dim3((unsigned)(C * blocks_per_cam)), dim3(RAY_BLOCK), 0, s, N, (int)HW, width,
                     (int)blocks_per_cam, means, quats, scales, cams, median_id, median_depth, near_plane, camera_model,
                     ray_depth_out);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
