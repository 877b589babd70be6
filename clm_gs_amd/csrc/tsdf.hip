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
// Extraction.  Four passes over the voxels, one lane per voxel, between which the host takes two inclusive int32
// prefix sums: cells (0 / 1 per active cell), vertices (one per active cell, at the cell's rank), quad_count (0..3 per
// voxel: its +x, +y, +z edges) and quads (two triangles per quad at the voxel's rank).  The output order is fixed by the
// ranks: vertices by cell index, faces by (owner voxel index, axis).
#include "common.h"
#include "tsdf_fuse.h"
#include "tsdf_math.h"

namespace clmgs {

constexpr int TS_BX = 64, TS_BY = 4, TS_BZ = 8;
constexpr int TS_THREADS = TS_BX * TS_BY;
constexpr int TS_MAX_SIDE = 32768;      // of an image
constexpr int TS_EX_THREADS = 256;
constexpr int TS_EX_MAX_BLOCKS = 8192;  // the extraction passes stride over the voxels

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
struct TsdfDims {
  int nx, ny, nz;
  int64_t n;
};

__device__ __forceinline__ void ts_decode(const TsdfDims& D, int v, int& i, int& j, int& k) {
  i = v % D.nx;
  const int t = v / D.nx;
  j = t % D.ny;
  k = t / D.ny;
}

__device__ __forceinline__ int ts_corner(const TsdfDims& D, int v, int c) {
  return v + (c & 1) + ((c >> 1) & 1) * D.nx + (c >> 2) * D.nx * D.ny;
}

// (i, j, k) is the origin of a cell iff it has a +1 neighbour along every axis.
__device__ __forceinline__ bool ts_is_cell(const TsdfDims& D, int i, int j, int k) {
  return i + 1 < D.nx && j + 1 < D.ny && k + 1 < D.nz;
}

__device__ __forceinline__ bool ts_ranked(const int32_t* __restrict__ scan, int v) {
  return scan[v] != (v > 0 ? scan[v - 1] : 0);
}

__global__ void __launch_bounds__(TS_EX_THREADS)
tsdf_cells_kernel(const float* __restrict__ grid, TsdfDims D, float min_weight, int32_t* __restrict__ cell_count) {
  for (int64_t v64 = (int64_t)blockIdx.x * TS_EX_THREADS + threadIdx.x; v64 < D.n; v64 += (int64_t)gridDim.x * TS_EX_THREADS) {
    const int v = (int)v64;
    int i, j, k;
    ts_decode(D, v, i, j, k);
    int active = 0;
    if (ts_is_cell(D, i, j, k)) {
      float t8[8], w8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int vc = ts_corner(D, v, c);
        t8[c] = grid[vc];
        w8[c] = grid[D.n + vc];
      }
      active = tsdf_cell_active(t8, w8, min_weight) ? 1 : 0;
    }
    cell_count[v] = active;
  }
}

__global__ void __launch_bounds__(TS_EX_THREADS)
tsdf_vertices_kernel(const float* __restrict__ grid, TsdfDims D, const int32_t* __restrict__ cell_scan, int V,
                     const TsdfCams g2w, float* __restrict__ verts, uint8_t* __restrict__ colours) {
  for (int64_t v64 = (int64_t)blockIdx.x * TS_EX_THREADS + threadIdx.x; v64 < D.n; v64 += (int64_t)gridDim.x * TS_EX_THREADS) {
    const int v = (int)v64;
    if (!ts_ranked(cell_scan, v)) continue;
    const int id = cell_scan[v] - 1;
    int i, j, k;
    ts_decode(D, v, i, j, k);
    if (id < 0 || id >= V || !ts_is_cell(D, i, j, k)) continue;  // (a scan that does not belong to this grid writes nothing outside)
    float vox[TSDF_PLANES][8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int vc = ts_corner(D, v, c);
#pragma unroll
      for (int p = 0; p < TSDF_PLANES; ++p) vox[p][c] = grid[p * D.n + vc];
    }
    float xyz[3];
    uint8_t q[3];
    tsdf_cell_vertex(vox, i, j, k, g2w.c[0], xyz, q);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      verts[(int64_t)id * 3 + d] = xyz[d];
      colours[(int64_t)id * 3 + d] = q[d];
    }
  }
}

// The quad of the grid edge that voxel v = (p[0], p[1], p[2]) owns along `axis`: it exists iff the edge's two voxels are
// valid with different inside flags and the four cells around the edge are active (ranked in cell_scan).  q[0..3]: the
// origins of those cells, right-handed about the axis: with a1, a2 the two axes after `axis` in cyclic order (axis =
// a1 x a2), the cells at (p[a1] - 1, p[a2] - 1), (p[a1], p[a2] - 1), (p[a1], p[a2]), (p[a1] - 1, p[a2]).
__device__ __forceinline__ bool ts_quad(const float* __restrict__ grid, const TsdfDims& D, const int32_t* __restrict__ cell_scan,
                                        float min_weight, int v, const int (&p)[3], int axis, int (&q)[4], bool& inside) {
  const int dim[3] = {D.nx, D.ny, D.nz};
  const int stride[3] = {1, D.nx, D.nx * D.ny};
  const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
  if (p[axis] + 1 >= dim[axis]) return false;
  if (p[a1] < 1 || p[a1] + 1 >= dim[a1] || p[a2] < 1 || p[a2] + 1 >= dim[a2]) return false;
  const int v2 = v + stride[axis];
  if (!tsdf_valid(grid[D.n + v], min_weight) || !tsdf_valid(grid[D.n + v2], min_weight)) return false;
  inside = tsdf_inside(grid[v]);
  if (inside == tsdf_inside(grid[v2])) return false;
  q[0] = v - stride[a1] - stride[a2];
  q[1] = v - stride[a2];
  q[2] = v;
  q[3] = v - stride[a1];
  return ts_ranked(cell_scan, q[0]) && ts_ranked(cell_scan, q[1]) && ts_ranked(cell_scan, q[2]) &&
         ts_ranked(cell_scan, q[3]);
}

// EMIT false: quad_out[v] = the number of quads voxel v owns; true: their triangles at rank quad_scan[v] - that number.
template <bool EMIT>
__global__ void __launch_bounds__(TS_EX_THREADS)
tsdf_quads_kernel(const float* __restrict__ grid, TsdfDims D, float min_weight, const int32_t* __restrict__ cell_scan,
                  int32_t* __restrict__ quad_count, const int32_t* __restrict__ quad_scan, int V, int Q,
                  int32_t* __restrict__ faces) {
  for (int64_t v64 = (int64_t)blockIdx.x * TS_EX_THREADS + threadIdx.x; v64 < D.n; v64 += (int64_t)gridDim.x * TS_EX_THREADS) {
    const int v = (int)v64;
    int p[3];
    ts_decode(D, v, p[0], p[1], p[2]);
    if (EMIT && !ts_ranked(quad_scan, v)) continue;
    int count = 0, rank = EMIT ? (v > 0 ? quad_scan[v - 1] : 0) : 0;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      int q[4];
      bool inside = false;
      if (!ts_quad(grid, D, cell_scan, min_weight, v, p, axis, q, inside)) continue;
      ++count;
      if (EMIT) {
        int id[4];
        bool ok = rank >= 0 && rank < Q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          id[e] = cell_scan[q[e]] - 1;
          ok = ok && id[e] >= 0 && id[e] < V;
        }
        if (ok) {  // two triangles along the diagonal q0 - q2; the owner inside: right-handed about the axis
          int32_t* f = faces + (int64_t)rank * 6;
          f[0] = id[0];
          f[1] = inside ? id[1] : id[2];
          f[2] = inside ? id[2] : id[1];
          f[3] = id[0];
          f[4] = inside ? id[2] : id[3];
          f[5] = inside ? id[3] : id[2];
        }
        ++rank;
      }
    }
    if (!EMIT) quad_count[v] = count;
  }
}

static bool ts_dims(int nx, int ny, int nz, TsdfDims& D) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  const int64_t n = (int64_t)nx * ny;  // < 2^62
  if (n >= ((int64_t)1 << 31) || n * nz >= ((int64_t)1 << 31)) return false;
  D.nx = nx; D.ny = ny; D.nz = nz; D.n = n * nz;
  return true;
}

static dim3 ts_ex_grid(const TsdfDims& D) {
  return dim3((unsigned)min((int64_t)TS_EX_MAX_BLOCKS, (D.n + TS_EX_THREADS - 1) / TS_EX_THREADS));
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_tsdf_integrate(void* stream, int nx, int ny, int nz, float* grid, int B, int H, int W,
                                    const float* depth, const float* alpha, const float* rgb, const double* cams, float near,
                                    float depth_max, float alpha_min, float trunc, float inv_trunc, int cull) {
  TsdfDims D;
  CLMGS_CHECK_ARG(ts_dims(nx, ny, nz, D));
  CLMGS_CHECK_ARG(B >= 1 && B <= TSDF_MAX_B);
  CLMGS_CHECK_ARG(H >= 1 && W >= 1 && H <= TS_MAX_SIDE && W <= TS_MAX_SIDE);
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(depth, 4) && ts_aligned(alpha, 4) && ts_aligned(rgb, 4));
  CLMGS_CHECK_ARG(cams != nullptr && (cull == 0 || cull == 1));
  CLMGS_CHECK_ARG(isfinite(trunc) && trunc > 0.0f && isfinite(inv_trunc) && inv_trunc > 0.0f);
  CLMGS_CHECK_ARG(isfinite(near) && !isnan(depth_max) && !isnan(alpha_min));
  TsdfCams C;
  for (int b = 0; b < TSDF_MAX_B; ++b)
    for (int e = 0; e < TSDF_CAM_DOUBLES; ++e) {
      C.c[b][e] = b < B ? cams[b * TSDF_CAM_DOUBLES + e] : 0.0;
      CLMGS_CHECK_ARG(isfinite(C.c[b][e]));
    }
  for (int b = 0; b < B; ++b) CLMGS_CHECK_ARG(C.c[b][12] > 0.0 && C.c[b][13] > 0.0);
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
  TsdfDims D;
  CLMGS_CHECK_ARG(ts_dims(nx, ny, nz, D));
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_count, 4) && ts_weight(min_weight));
  CLMGS_CHECK_ARG(ts_apart(grid, (uint64_t)D.n * TSDF_PLANES * 4, cell_count, (uint64_t)D.n * 4));
  hipLaunchKernelGGL(tsdf_cells_kernel, ts_ex_grid(D), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, grid, D, min_weight,
                     cell_count);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_vertices(void* stream, int nx, int ny, int nz, const float* grid, const int32_t* cell_scan, int V,
                                   const double* grid_to_world, float* verts, uint8_t* colours) {
  TsdfDims D;
  CLMGS_CHECK_ARG(ts_dims(nx, ny, nz, D));
  CLMGS_CHECK_ARG(V >= 1 && V <= D.n && grid_to_world != nullptr);
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_scan, 4) && ts_aligned(verts, 4) && colours != nullptr);
  TsdfCams G;
  for (int e = 0; e < TSDF_MAX_B * TSDF_CAM_DOUBLES; ++e) {
    G.c[0][e] = e < 12 ? grid_to_world[e] : 0.0;
    CLMGS_CHECK_ARG(isfinite(G.c[0][e]));
  }
  const uint64_t gbytes = (uint64_t)D.n * TSDF_PLANES * 4, sbytes = (uint64_t)D.n * 4, vbytes = (uint64_t)V * 12,
                 cbytes = (uint64_t)V * 3;
  CLMGS_CHECK_ARG(ts_apart(verts, vbytes, grid, gbytes) && ts_apart(verts, vbytes, cell_scan, sbytes) &&
                  ts_apart(colours, cbytes, grid, gbytes) && ts_apart(colours, cbytes, cell_scan, sbytes) &&
                  ts_apart(verts, vbytes, colours, cbytes));
  hipLaunchKernelGGL(tsdf_vertices_kernel, ts_ex_grid(D), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, grid, D, cell_scan, V,
                     G, verts, colours);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_quad_count(void* stream, int nx, int ny, int nz, const float* grid, float min_weight,
                                     const int32_t* cell_scan, int32_t* quad_count) {
  TsdfDims D;
  CLMGS_CHECK_ARG(ts_dims(nx, ny, nz, D));
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_scan, 4) && ts_aligned(quad_count, 4) && ts_weight(min_weight));
  const uint64_t gbytes = (uint64_t)D.n * TSDF_PLANES * 4, sbytes = (uint64_t)D.n * 4;
  CLMGS_CHECK_ARG(ts_apart(quad_count, sbytes, grid, gbytes) && ts_apart(quad_count, sbytes, cell_scan, sbytes));
  hipLaunchKernelGGL(tsdf_quads_kernel<false>, ts_ex_grid(D), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, grid, D,
                     min_weight, cell_scan, quad_count, (const int32_t*)nullptr, 0, 0, (int32_t*)nullptr);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_quads(void* stream, int nx, int ny, int nz, const float* grid, float min_weight,
                                const int32_t* cell_scan, const int32_t* quad_scan, int V, int Q, int32_t* faces) {
  TsdfDims D;
  CLMGS_CHECK_ARG(ts_dims(nx, ny, nz, D));
  CLMGS_CHECK_ARG(V >= 1 && V <= D.n && Q >= 1 && Q < (1 << 30));
  CLMGS_CHECK_ARG(ts_aligned(grid, 4) && ts_aligned(cell_scan, 4) && ts_aligned(quad_scan, 4) && ts_aligned(faces, 4) &&
                  ts_weight(min_weight));
  const uint64_t gbytes = (uint64_t)D.n * TSDF_PLANES * 4, sbytes = (uint64_t)D.n * 4, fbytes = (uint64_t)Q * 24;
  CLMGS_CHECK_ARG(ts_apart(faces, fbytes, grid, gbytes) && ts_apart(faces, fbytes, cell_scan, sbytes) &&
                  ts_apart(faces, fbytes, quad_scan, sbytes));
  hipLaunchKernelGGL(tsdf_quads_kernel<true>, ts_ex_grid(D), dim3(TS_EX_THREADS), 0, (hipStream_t)stream, grid, D, min_weight,
                     cell_scan, (int32_t*)nullptr, quad_scan, V, Q, faces);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
