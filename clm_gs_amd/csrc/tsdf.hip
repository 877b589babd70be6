// Mesh export ("Mesh export"): TSDF fusion of rendered depth maps into a dense voxel grid and the
// extraction of a triangle mesh from it by naive Surface Nets.  The arithmetic is csrc/tsdf_math.h.
//
// The volume is one float32 tensor [6, nz, ny, nx] (x fastest): planes tsum, wsum, cr, cg, cb, cw.  The kernels know
// nothing of the world frame: a camera record is the 3x4 matrix that takes the grid point (i + 0.5, j + 0.5, k + 0.5, 1)
// to camera space, followed by fx, fy, cx, cy, all float64 and composed by the host.
//
// Fusion.  A workgroup of 256 lanes owns a brick of 64 x 4 x 8 voxels: a lane owns the voxels (i, j, k0 .. k0 + 7), one at
// a time, and keeps a voxel's six sums in registers over the whole batch of cameras, so the grid is read and written
// once per launch, not once per camera -- and only where it changes: the sums of a voxel are loaded at the first camera
// that observes it and stored only then.  A wave is 64 neighbouring x, which project to neighbouring pixels.  The cameras
// travel as a kernel argument (scalar loads).  Every sum is sequential in camera order and a voxel has one owner, so there
// are no atomics and splitting the cameras into launches differently cannot change a bit.
//
// Brick cull.  Before the voxels, lane 8 b + c projects corner c of the brick's box of voxel centres into camera b and
// tests it against five half spaces: behind the near plane, and (with near >= 0) left, right, above and below the image
// by more than a pixel, each as a LINEAR function of the grid point (for z > 0, u < -1 <=> fx x + (cx + 1) z < 0) with a
// margin of 2^-40 of the magnitude of its terms.  A linear function on a box is extreme at its corners, so a camera
// whose eight corners all fail the same test observes no voxel of the brick, and the workgroup skips it (a uniform
// branch).  The margin is 4000 times the rounding of the float64 projection, so the cull never decides a voxel: the
// result is the same with and without it, bit for bit (tests/test_gpu_tsdf.py).
//
// Extraction.  The four Surface Nets passes of csrc/tsdf_extract.h, shared with the brick-allocated volume, over the
// voxels, one lane per voxel.  The output order is fixed by the ranks: vertices by cell index, faces by (owner voxel
// index, axis).
#include "common.h"
#include "tsdf_extract.h"
#include "tsdf_fuse.h"
#include "tsdf_math.h"

namespace clmgs {

constexpr int TS_BX = 64, TS_BY = 4, TS_BZ = 8;
constexpr int TS_THREADS = TS_BX * TS_BY;

// The cull and the per-voxel camera loop are csrc/tsdf_fuse.h, shared with the brick-allocated volume.
__global__ void __launch_bounds__(TS_THREADS)
tsdf_integrate_kernel(float* __restrict__ grid, int nx, int ny, int nz, int nbx, int nby, const TsdfCams cams, int B, int H,
                      int W, const float* __restrict__ depth, const float* __restrict__ alpha,
                      const float* __restrict__ rgb, float near_f, float depth_max, float alpha_min, float trunc,
                      float inv_trunc, int cull) {
#pragma clang fp contract(off)
  __shared__ unsigned char seen_lds[TSDF_MAX_B];
  const unsigned blk = blockIdx.x;
  const int bi = blk % nbx, bj = (blk / nbx) % nby, bk = blk / nbx / nby;
  const int i0 = bi * TS_BX, j0 = bj * TS_BY, k0 = bk * TS_BZ;
  const double near = (double)near_f;
  unsigned seen = (1u << B) - 1u;  // B <= 16
  if (cull)  // (uniform)
    seen = ts_cull_seen(cams, B, H, W, near, (double)i0 + 0.5, (double)min(i0 + TS_BX - 1, nx - 1) + 0.5, (double)j0 + 0.5,
                        (double)min(j0 + TS_BY - 1, ny - 1) + 0.5, (double)k0 + 0.5, (double)min(k0 + TS_BZ - 1, nz - 1) + 0.5,
                        seen_lds);
  seen = __builtin_amdgcn_readfirstlane(seen);
  if (seen == 0u) return;
  const int i = i0 + (threadIdx.x & (TS_BX - 1)), j = j0 + (threadIdx.x >> 6);
  if (i >= nx || j >= ny) return;
  const int64_t n = (int64_t)nx * ny * nz, hw = (int64_t)H * W;
  const double px = (double)i + 0.5, py = (double)j + 0.5;
  const int kend = min(k0 + TS_BZ, nz);
  for (int k = k0; k < kend; ++k) {
    const double pz = (double)k + 0.5;
    ts_fuse_voxel(grid + ((int64_t)k * ny + j) * nx + i, n, cams, B, seen, px, py, pz, near, H, W, hw, depth, alpha, rgb,
                  depth_max, alpha_min, trunc, inv_trunc);
  }
}

// ---------------------------------------------------------------------------------------------- extraction
// The accessor of csrc/tsdf_extract.h: a lane index is the linear voxel index, a neighbour a stride away, nothing missing.
struct DenseVol {
  static constexpr bool KEYS = false;
  const float* grid;
  int nx, ny, nz;
  int64_t n;

  __host__ __device__ __forceinline__ int64_t lanes() const { return n; }
  __device__ __forceinline__ bool decode(int v, int (&p)[3]) const {
    p[0] = v % nx;
    const int t = v / nx;
    p[1] = t % ny;
    p[2] = t / ny;
    return true;
  }
  __device__ __forceinline__ int neighbour(int v, const int (&)[3], int dx, int dy, int dz) const {
    return v + dx + dy * nx + dz * nx * ny;
  }
  __device__ __forceinline__ bool stored(int) const { return true; }
  __device__ __forceinline__ float plane(int v, int pl) const { return grid[pl * n + v]; }
};

static bool ts_vol(int nx, int ny, int nz, const float* grid, DenseVol& D) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  const int64_t n = (int64_t)nx * ny;  // < 2^62
  if (n >= ((int64_t)1 << 31) || n * nz >= ((int64_t)1 << 31)) return false;
  D.grid = grid; D.nx = nx; D.ny = ny; D.nz = nz; D.n = n * nz;
  return true;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_tsdf_integrate(void* stream, int nx, int ny, int nz, float* grid, int B, int H, int W,
                                    const float* depth, const float* alpha, const float* rgb, const double* cams, float near,
                                    float depth_max, float alpha_min, float trunc, float inv_trunc, int cull) {
  DenseVol D;
  CLMGS_CHECK_ARG(ts_vol(nx, ny, nz, grid, D));
  CLMGS_CHECK_ARG(ts_image(H, W));
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(depth, 4) && ts_aligned(alpha, 4) && ts_aligned(rgb, 4));
  CLMGS_CHECK_ARG(cull == 0 || cull == 1);
  CLMGS_CHECK_ARG(isfinite(trunc) && trunc > 0.0f && isfinite(inv_trunc) && inv_trunc > 0.0f);
  CLMGS_CHECK_ARG(isfinite(near) && !isnan(depth_max) && !isnan(alpha_min));
  TsdfCams C;
  CLMGS_CHECK_ARG(ts_load_cams(cams, B, INFINITY, C));
  const uint64_t gbytes = (uint64_t)D.n * TSDF_PLANES * 4, ibytes = (uint64_t)B * H * W * 4;
  CLMGS_CHECK_ARG(ts_apart(grid, gbytes, depth, ibytes) && ts_apart(grid, gbytes, alpha, ibytes) &&
                  ts_apart(grid, gbytes, rgb, 3 * ibytes));
  const int nbx = ceil_div(nx, TS_BX), nby = ceil_div(ny, TS_BY), nbz = ceil_div(nz, TS_BZ);
  const int64_t blocks = (int64_t)nbx * nby * nbz;  // <= n / 2 + ... < 2^31: every side >= 2
  CLMGS_CHECK_ARG(blocks < ((int64_t)1 << 31));
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)blocks), dim3(TS_THREADS), 0, (hipStream_t)stream, grid, nx, ny,
                     nz, nbx, nby, C, B, H, W, depth, alpha, rgb, near, depth_max, alpha_min, trunc, inv_trunc, cull);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_cells(void* stream, int nx, int ny, int nz, const float* grid, float min_weight,
                                int32_t* cell_count) {
  DenseVol D;
  CLMGS_CHECK_ARG(ts_vol(nx, ny, nz, grid, D));
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_count, 4) && ts_weight(min_weight));
  CLMGS_CHECK_ARG(ts_apart(grid, (uint64_t)D.n * TSDF_PLANES * 4, cell_count, (uint64_t)D.n * 4));
  hipLaunchKernelGGL(tsdf_cells_kernel<DenseVol>, ts_ex_grid(D.lanes()), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, D, min_weight,
                     cell_count);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_vertices(void* stream, int nx, int ny, int nz, const float* grid, const int32_t* cell_scan, int V,
                                   const double* grid_to_world, float* verts, uint8_t* colours) {
  DenseVol D;
  CLMGS_CHECK_ARG(ts_vol(nx, ny, nz, grid, D));
  CLMGS_CHECK_ARG(V >= 1 && V <= D.n);
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_scan, 4) && ts_aligned(verts, 4) && colours != nullptr);
  TsdfCams G;
  CLMGS_CHECK_ARG(ts_load_g2w(grid_to_world, G));
  const uint64_t gbytes = (uint64_t)D.n * TSDF_PLANES * 4, sbytes = (uint64_t)D.n * 4, vbytes = (uint64_t)V * 12,
                 cbytes = (uint64_t)V * 3;
  CLMGS_CHECK_ARG(ts_apart(verts, vbytes, grid, gbytes) && ts_apart(verts, vbytes, cell_scan, sbytes) &&
                  ts_apart(colours, cbytes, grid, gbytes) && ts_apart(colours, cbytes, cell_scan, sbytes) &&
                  ts_apart(verts, vbytes, colours, cbytes));
  hipLaunchKernelGGL(tsdf_vertices_kernel<DenseVol>, ts_ex_grid(D.lanes()), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, D, cell_scan,
                     V, G, verts, colours);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_quad_count(void* stream, int nx, int ny, int nz, const float* grid, float min_weight,
                                     const int32_t* cell_scan, int32_t* quad_count) {
  DenseVol D;
  CLMGS_CHECK_ARG(ts_vol(nx, ny, nz, grid, D));
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_scan, 4) && ts_aligned(quad_count, 4) && ts_weight(min_weight));
  const uint64_t gbytes = (uint64_t)D.n * TSDF_PLANES * 4, sbytes = (uint64_t)D.n * 4;
  CLMGS_CHECK_ARG(ts_apart(quad_count, sbytes, grid, gbytes) && ts_apart(quad_count, sbytes, cell_scan, sbytes));
  hipLaunchKernelGGL((tsdf_quads_kernel<DenseVol, false>), ts_ex_grid(D.lanes()), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, D,
                     min_weight, cell_scan, quad_count, (const int32_t*)nullptr, 0, 0, (int32_t*)nullptr);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_quads(void* stream, int nx, int ny, int nz, const float* grid, float min_weight,
                                const int32_t* cell_scan, const int32_t* quad_scan, int V, int Q, int32_t* faces) {
  DenseVol D;
  CLMGS_CHECK_ARG(ts_vol(nx, ny, nz, grid, D));
  CLMGS_CHECK_ARG(V >= 1 && V <= D.n && Q >= 1 && Q < (1 << 30));
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_scan, 4) && ts_aligned(quad_scan, 4) && ts_aligned(faces, 4) &&
                  ts_weight(min_weight));
  const uint64_t gbytes = (uint64_t)D.n * TSDF_PLANES * 4, sbytes = (uint64_t)D.n * 4, fbytes = (uint64_t)Q * 24;
  CLMGS_CHECK_ARG(ts_apart(faces, fbytes, grid, gbytes) && ts_apart(faces, fbytes, cell_scan, sbytes) &&
                  ts_apart(faces, fbytes, quad_scan, sbytes));
  hipLaunchKernelGGL((tsdf_quads_kernel<DenseVol, true>), ts_ex_grid(D.lanes()), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, D,
                     min_weight, cell_scan, (int32_t*)nullptr, quad_scan, V, Q, faces);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
