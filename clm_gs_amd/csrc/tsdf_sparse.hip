// Mesh export, sparse volume ("Sparse volume"): a brick-allocated TSDF volume that stores, fuses and
// extracts only where a surface can be, and gives the mesh of the dense volume (csrc/tsdf.hip) bit for bit.  The arithmetic
// is csrc/tsdf_math.h; the cull and the per-voxel camera loop are csrc/tsdf_fuse.h, the very code of the dense kernel.
//
// Layout.  Bricks of 8 x 8 x 8 voxels aligned to the grid origin; the brick grid is nbx x nby x nbz = ceil(n / 8) per axis.
// marks uint8 [nbz, nby, nbx]; table int32 [nbz, nby, nbx]: the slot of a brick, or -1; bricks int32 [S]: the linear brick
// index of every slot, ascending; pool float32 [S, 6, 8, 8, 8]: per slot the six planes tsum, wsum, cr, cg, cb, cw, each z, y, x
// with x fastest.  A "slot voxel" is the int sv = slot * 512 + (z * 64 + y * 8 + x) < 2^31.
//
// Why the meshes are equal.  A voxel is inside iff tsum < 0, which needs a negative term: some camera saw it with
// -trunc <= sdf < 0, through a pixel that passed the gates, at camera depth z in (d, d + trunc] up to the float32 rounding
// of z.  N is the set of such voxels over all cameras.  An active cell has an inside corner and all its corners within 1
// voxel of it; a quad has an inside voxel on its edge and the four cells around the edge have all their corners within 1
// voxel of it.  So when every voxel within 1 voxel of N is stored and every stored voxel carries the dense sums, every
// active cell, vertex and quad is the dense one; a cell that touches a voxel that is not stored is inactive in both.
//
// 1. tsdf_mark_kernel: one lane per pixel.  A pixel (col, row) of camera b that passes a >= alpha_min, 0 < d <= depth_max
// (and d finite: an infinite depth gives only free-space votes) can put into N only voxels whose centre, in camera space,
// lies in the frustum piece of the pixel square [col, col + 1] x [row, row + 1] between the depths
//     z0 = max(d, near) (1 - 2^-20)   and   z1 = (d + trunc) (1 + 2^-20).
// Margins.  tsdf_sdf compares d - (float) z, a float32 difference of magnitude <= trunc: (float) z is within 2^-24 of z
// and the difference within 2^-24 of itself, so z lies in (d (1 - 2^-23), (d + trunc) (1 + 2^-23)); the relative margin
// TS_MARK_ZREL = 2^-20 covers that eight times, and the rounding of the slab boundaries below (2^-52) with it.  The
// range is cut into ceil((z1 - z0) / (4 voxel)) sub-slabs, none longer than 4 voxels, so that a long oblique ray marks a
// chain of small boxes and not its bounding box; slab s is [z(s), z(s + 1)] with z(s) = z0 + (z1 - z0) (s / n), the same
// expression for the boundary two slabs share.  The eight corners ((u - cx) / fx z, (v - cy) / fy z, z) of a sub-slab map
// through the camera record -- the inverse affine map camera space -> grid coordinates (composed by the host in float64)
// -- in float64 without contraction, in the order written.  Coverage: a frustum piece is convex and an affine map keeps
// it so, so the piece lies inside the bounding box of its eight mapped corners: pixel footprint and obliquity need no
// assumption.  The box is widened by 1 + TS_MARK_GEPS voxels per side: 1 for the expansion dilate(N, 1) the equality
// needs, and TS_MARK_GEPS = 2^-16 voxel for rounding -- of the corner arithmetic (16 operations on numbers below 2^15
// voxels: 2^-33), of the host's inverse (its condition number times 2^-52 times 2^15), and of the dense kernel's own
// floor(u), floor(v) (2^-50 of a pixel).  Every voxel index whose centre i + 0.5 the widened box contains, clipped to the
// grid, has its brick marked with a plain byte store of 1.  Every lane stores the same value, so the result is a set: a
// pure function of the set of (camera, depth map) pairs, whatever their order and their split into launches.  No float
// atomics, no waiting between workgroups.
//
// 2. tsdf_sparse_integrate_kernel: one workgroup of 256 lanes per allocated brick; the brick index comes from bricks[] and
// is wave-uniform.  Wave w owns the z layers 2 w and 2 w + 1, lane l the voxel (x = l & 7, y = l >> 3): a wave reads and
// writes 256 contiguous bytes per plane and layer.  The cull tests the brick's eight corner centres, clipped to the grid
// as in the dense kernel; voxels of a border brick beyond nx, ny, nz are never touched.  A voxel has one owner: no atomics,
// and the result does not depend on how the cameras are split into launches.
//
// 3. Extraction: the four Surface Nets passes of csrc/tsdf_extract.h, the very code of the dense kernel, over the S * 512
// slot voxels (cells -> prefix sum -> vertices; quad_count -> prefix sum -> quads).  A neighbour in the lane's own brick
// is an offset; any other is read through the table, and a missing brick counts as wsum = 0 and unranked.  The vertices
// pass also writes the dense linear cell index (k ny + j) nx + i as an int64 key per vertex, the quads pass 3 * (owner's
// linear index) + axis per quad: sorted by them (the host, torch.sort) the output is in the dense order.
#include "common.h"
#include "tsdf_extract.h"
#include "tsdf_fuse.h"
#include "tsdf_math.h"

namespace clmgs {

constexpr int SP_SIDE = 8, SP_VOX = 512, SP_BRICK_FLOATS = TSDF_PLANES * SP_VOX;
constexpr int SP_THREADS = 256;
constexpr int64_t SP_MAX_BRICK_GRID = (int64_t)1 << 30;
constexpr double TS_MARK_ZREL = 1.0 / 1048576.0;  // 2^-20
constexpr double TS_MARK_GEPS = 1.0 / 65536.0;    // 2^-16 voxel
constexpr int TS_MARK_MAX_SLABS = 4096;
constexpr double TS_MARK_MAX_ENTRY = 1e30;  // of a record: no product below can overflow

struct SpDims {
  int nx, ny, nz, nbx, nby, nbz, S;
  int64_t nb;  // nbx nby nbz
};

// ---------------------------------------------------------------------------------------------- 1. marking
__global__ void __launch_bounds__(SP_THREADS)
tsdf_mark_kernel(uint8_t* __restrict__ marks, SpDims D, const TsdfCams cams, int B, int H, int W,
                 const float* __restrict__ depth, const float* __restrict__ alpha, float near_f, float depth_max,
                 float alpha_min, float trunc, double voxel_cam) {
#pragma clang fp contract(off)
  const int64_t hw = (int64_t)H * W, t = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (t >= (int64_t)B * hw) return;
  const int b = (int)(t / hw);
  const int64_t r = t - (int64_t)b * hw;
  const int row = (int)(r / W), col = (int)(r - (int64_t)row * W);
  const float d = depth[t], a = alpha[t];
  if (!(a >= alpha_min && d > 0.0f && d <= depth_max) || !isfinite(d)) return;
  const double* m = cams.c[b];
  const double z0 = fmax((double)d, (double)near_f) * (1.0 - TS_MARK_ZREL);
  const double z1 = ((double)d + (double)trunc) * (1.0 + TS_MARK_ZREL);
  if (!(z1 > z0)) return;  // the near plane lies behind the band
  const double fn = ceil((z1 - z0) / (4.0 * voxel_cam));
  const int nslab = fn >= 1.0 ? (fn <= (double)TS_MARK_MAX_SLABS ? (int)fn : TS_MARK_MAX_SLABS) : 1;
  const double fx = m[12], fy = m[13], cx = m[14], cy = m[15];
  const double xf[2] = {((double)col - cx) / fx, ((double)(col + 1) - cx) / fx};
  const double yf[2] = {((double)row - cy) / fy, ((double)(row + 1) - cy) / fy};
  const int dim[3] = {D.nx, D.ny, D.nz};
  for (int s = 0; s < nslab; ++s) {
    const double zz[2] = {z0 + (z1 - z0) * ((double)s / (double)nslab), z0 + (z1 - z0) * ((double)(s + 1) / (double)nslab)};
    double lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double z = zz[c >> 2], x = xf[c & 1] * z, y = yf[(c >> 1) & 1] * z;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const double g = tsdf_row(m + 4 * e, x, y, z);
        lo[e] = c == 0 ? g : fmin(lo[e], g);
        hi[e] = c == 0 ? g : fmax(hi[e], g);
      }
    }
    int b0[3], b1[3];
    bool any = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {  // the voxel indices whose centre i + 0.5 lies in [lo - (1 + eps), hi + (1 + eps)]
      const double first = fmax(ceil((lo[e] - (1.0 + TS_MARK_GEPS)) - 0.5), 0.0);
      const double last = fmin(floor((hi[e] + (1.0 + TS_MARK_GEPS)) - 0.5), (double)(dim[e] - 1));
      any = any && first <= last;  // (a NaN fails)
      b0[e] = any ? (int)first >> 3 : 0;
      b1[e] = any ? (int)last >> 3 : -1;
    }
    if (!any) continue;
    for (int bz = b0[2]; bz <= b1[2]; ++bz)
      for (int by = b0[1]; by <= b1[1]; ++by)
        for (int bx = b0[0]; bx <= b1[0]; ++bx) {
          uint8_t* p = marks + ((int64_t)bz * D.nby + by) * D.nbx + bx;  // inside [0, nb): the ranges are clipped to the grid
          if (*p == 0) *p = 1;  // (a same-value byte store; the read only spares the write)
        }
  }
}

// ---------------------------------------------------------------------------------------------- 2. fusion
__global__ void __launch_bounds__(SP_THREADS)
tsdf_sparse_integrate_kernel(float* __restrict__ pool, const int32_t* __restrict__ bricks, SpDims D, const TsdfCams cams, int B,
                             int H, int W, const float* __restrict__ depth, const float* __restrict__ alpha,
                             const float* __restrict__ rgb, float near_f, float depth_max, float alpha_min, float trunc,
                             float inv_trunc, int cull) {
#pragma clang fp contract(off)
  __shared__ unsigned char seen_lds[TSDF_MAX_B];
  const int slot = blockIdx.x;  // < S
  const int bidx = __builtin_amdgcn_readfirstlane(bricks[slot]);
  if (bidx < 0 || (int64_t)bidx >= D.nb) return;  // (uniform: a list that does not belong to this grid writes nothing)
  const int bi = bidx % D.nbx, bj = (bidx / D.nbx) % D.nby, bk = bidx / D.nbx / D.nby;
  const int i0 = bi * SP_SIDE, j0 = bj * SP_SIDE, k0 = bk * SP_SIDE;
  const double near = (double)near_f;
  unsigned seen = (1u << B) - 1u;  // B <= 16
  if (cull)  // (uniform)
    seen = ts_cull_seen(cams, B, H, W, near, (double)i0 + 0.5, (double)min(i0 + SP_SIDE - 1, D.nx - 1) + 0.5, (double)j0 + 0.5,
                        (double)min(j0 + SP_SIDE - 1, D.ny - 1) + 0.5, (double)k0 + 0.5,
                        (double)min(k0 + SP_SIDE - 1, D.nz - 1) + 0.5, seen_lds);
  seen = __builtin_amdgcn_readfirstlane(seen);
  if (seen == 0u) return;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int i = i0 + (l & 7), j = j0 + (l >> 3);
  if (i >= D.nx || j >= D.ny) return;
  const int64_t hw = (int64_t)H * W;
  const double px = (double)i + 0.5, py = (double)j + 0.5;
  float* brick = pool + (int64_t)slot * SP_BRICK_FLOATS;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int z = 2 * w + s, k = k0 + z;
    if (k >= D.nz) break;
    ts_fuse_voxel(brick + z * 64 + l, SP_VOX, cams, B, seen, px, py, (double)k + 0.5, near, H, W, hw, depth, alpha, rgb,
                  depth_max, alpha_min, trunc, inv_trunc);
  }
}

// ---------------------------------------------------------------------------------------------- 3. extraction
// The accessor of csrc/tsdf_extract.h: a lane index is a slot voxel, and the passes write sort keys.
struct BrickVol : SpDims {
  static constexpr bool KEYS = true;
  const float* pool;
  const int32_t *bricks, *table;
  int64_t* keys;  // of the pass that writes them, else null

  __host__ __device__ __forceinline__ int64_t lanes() const { return (int64_t)S * SP_VOX; }
  // false for a voxel of a border brick beyond the grid (or a brick list that does not belong to this grid)
  __device__ __forceinline__ bool decode(int sv, int (&p)[3]) const {
    const int bidx = bricks[sv >> 9];
    if (bidx < 0 || (int64_t)bidx >= nb) return false;
    const int l = sv & 511;
    p[0] = (bidx % nbx) * SP_SIDE + (l & 7);
    p[1] = ((bidx / nbx) % nby) * SP_SIDE + ((l >> 3) & 7);
    p[2] = (bidx / nbx / nby) * SP_SIDE + (l >> 6);
    return p[0] < nx && p[1] < ny && p[2] < nz;
  }
  // an offset inside the lane's own brick, else through the table; -1 where no brick is stored
  __device__ __forceinline__ int neighbour(int sv, const int (&p)[3], int dx, int dy, int dz) const {
    const int x = (p[0] & 7) + dx, y = (p[1] & 7) + dy, z = (p[2] & 7) + dz;
    if (((x | y | z) & ~7) == 0) return sv + dx + 8 * dy + 64 * dz;  // the fast path
    const int i = p[0] + dx, j = p[1] + dy, k = p[2] + dz;
    const int slot = table[((int64_t)(k >> 3) * nby + (j >> 3)) * nbx + (i >> 3)];
    if (slot < 0 || slot >= S) return -1;
    return slot * SP_VOX + (k & 7) * 64 + (j & 7) * 8 + (i & 7);
  }
  __device__ __forceinline__ bool stored(int sv) const { return sv >= 0; }
  __device__ __forceinline__ float plane(int sv, int pl) const {
    return sv < 0 ? 0.0f : pool[(int64_t)(sv >> 9) * SP_BRICK_FLOATS + pl * SP_VOX + (sv & 511)];
  }
  __device__ __forceinline__ int64_t linear(const int (&p)[3]) const { return ((int64_t)p[2] * ny + p[1]) * nx + p[0]; }
};

// ---------------------------------------------------------------------------------------------- host
static bool sp_dims(int nx, int ny, int nz, int S, SpDims& D) {
  if (nx < 2 || ny < 2 || nz < 2 || S < 1 || (int64_t)S * SP_VOX >= ((int64_t)1 << 31)) return false;
  D.nx = nx; D.ny = ny; D.nz = nz; D.S = S;
  D.nbx = ceil_div(nx, SP_SIDE); D.nby = ceil_div(ny, SP_SIDE); D.nbz = ceil_div(nz, SP_SIDE);
  const int64_t nb2 = (int64_t)D.nbx * D.nby;  // < 2^56
  if (nb2 > SP_MAX_BRICK_GRID || nb2 * D.nbz > SP_MAX_BRICK_GRID) return false;
  D.nb = nb2 * D.nbz;
  return (int64_t)S <= D.nb;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_tsdf_mark(void* stream, int nx, int ny, int nz, uint8_t* marks, int B, int H, int W, const float* depth,
                               const float* alpha, const double* cams, float near, float depth_max, float alpha_min,
                               float trunc, double voxel_cam) {
  SpDims D;
  CLMGS_CHECK_ARG(sp_dims(nx, ny, nz, 1, D));
  CLMGS_CHECK_ARG(ts_image(H, W));
  CLMGS_CHECK_ARG(marks != nullptr && ts_aligned(depth, 4) && ts_aligned(alpha, 4));
  CLMGS_CHECK_ARG(isfinite(trunc) && trunc > 0.0f && isfinite(voxel_cam) && voxel_cam > 0.0);
  CLMGS_CHECK_ARG((double)trunc / voxel_cam <= (double)TS_MARK_MAX_SLABS);
  CLMGS_CHECK_ARG(isfinite(near) && !isnan(depth_max) && !isnan(alpha_min));
  TsdfCams C;
  CLMGS_CHECK_ARG(ts_load_cams(cams, B, TS_MARK_MAX_ENTRY, C));
  const uint64_t ibytes = (uint64_t)B * H * W * 4;
  CLMGS_CHECK_ARG(ts_apart(marks, (uint64_t)D.nb, depth, ibytes) && ts_apart(marks, (uint64_t)D.nb, alpha, ibytes));
  const int64_t blocks = ((int64_t)B * H * W + SP_THREADS - 1) / SP_THREADS;  // <= 2^26
  hipLaunchKernelGGL(tsdf_mark_kernel, dim3((unsigned)blocks), dim3(SP_THREADS), 0, (hipStream_t)stream, marks, D, C, B, H, W,
                     depth, alpha, near, depth_max, alpha_min, trunc, voxel_cam);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_sparse_integrate(void* stream, int nx, int ny, int nz, int S, const int32_t* bricks, float* pool,
                                           int B, int H, int W, const float* depth, const float* alpha, const float* rgb,
                                           const double* cams, float near, float depth_max, float alpha_min, float trunc,
                                           float inv_trunc, int cull) {
  SpDims D;
  CLMGS_CHECK_ARG(sp_dims(nx, ny, nz, S, D));
  CLMGS_CHECK_ARG(ts_image(H, W));
  CLMGS_CHECK_ARG(ts_aligned(bricks, 4) && ts_aligned(pool, 4) && ts_aligned(depth, 4) && ts_aligned(alpha, 4) &&
                  ts_aligned(rgb, 4));
  CLMGS_CHECK_ARG(cull == 0 || cull == 1);
  CLMGS_CHECK_ARG(isfinite(trunc) && trunc > 0.0f && isfinite(inv_trunc) && inv_trunc > 0.0f);
  CLMGS_CHECK_ARG(isfinite(near) && !isnan(depth_max) && !isnan(alpha_min));
  TsdfCams C;
  CLMGS_CHECK_ARG(ts_load_cams(cams, B, INFINITY, C));
  const uint64_t pbytes = (uint64_t)S * SP_BRICK_FLOATS * 4, ibytes = (uint64_t)B * H * W * 4, bbytes = (uint64_t)S * 4;
  CLMGS_CHECK_ARG(ts_apart(pool, pbytes, depth, ibytes) && ts_apart(pool, pbytes, alpha, ibytes) &&
                  ts_apart(pool, pbytes, rgb, 3 * ibytes) && ts_apart(pool, pbytes, bricks, bbytes));
  hipLaunchKernelGGL(tsdf_sparse_integrate_kernel, dim3((unsigned)S), dim3(SP_THREADS), 0, (hipStream_t)stream, pool, bricks, D,
                     C, B, H, W, depth, alpha, rgb, near, depth_max, alpha_min, trunc, inv_trunc, cull);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_tsdf_sparse_extract(void* stream, int pass, int nx, int ny, int nz, int S, const int32_t* bricks,
                                         const int32_t* table, const float* pool, float min_weight, int32_t* count,
                                         const int32_t* cell_scan, const int32_t* quad_scan, int V, int Q,
                                         const double* grid_to_world, float* verts, uint8_t* colours, int64_t* vert_keys,
                                         int32_t* faces, int64_t* quad_keys) {
  BrickVol D;
  CLMGS_CHECK_ARG(sp_dims(nx, ny, nz, S, D));
  CLMGS_CHECK_ARG(pass >= 0 && pass <= 3);
  CLMGS_CHECK_ARG(ts_aligned(bricks, 4) && ts_aligned(table, 4) && ts_aligned(pool, 4));
  D.pool = pool; D.bricks = bricks; D.table = table;
  D.keys = pass == 1 ? vert_keys : pass == 3 ? quad_keys : nullptr;
  const uint64_t pbytes = (uint64_t)S * SP_BRICK_FLOATS * 4, sbytes = (uint64_t)S * SP_VOX * 4, bbytes = (uint64_t)S * 4,
                 tbytes = (uint64_t)D.nb * 4;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid = ts_ex_grid(D.lanes()), block(TS_EX_THREADS);
  // an output overlaps no input
  auto clear = [&](const void* out, uint64_t obytes) {
    return ts_apart(out, obytes, pool, pbytes) && ts_apart(out, obytes, bricks, bbytes) && ts_apart(out, obytes, table, tbytes) &&
           (cell_scan == nullptr || ts_apart(out, obytes, cell_scan, sbytes)) &&
           (quad_scan == nullptr || ts_apart(out, obytes, quad_scan, sbytes));
  };
  if (pass == 0 || pass == 2) {
    CLMGS_CHECK_ARG(ts_aligned(count, 4) && ts_weight(min_weight) && clear(count, sbytes));
    if (pass == 0) {
      hipLaunchKernelGGL(tsdf_cells_kernel<BrickVol>, grid, block, 0, st, D, min_weight, count);
    } else {
      CLMGS_CHECK_ARG(ts_aligned(cell_scan, 4));
      hipLaunchKernelGGL((tsdf_quads_kernel<BrickVol, false>), grid, block, 0, st, D, min_weight, cell_scan, count,
                         (const int32_t*)nullptr, 0, 0, (int32_t*)nullptr);
    }
  } else if (pass == 1) {
    CLMGS_CHECK_ARG(V >= 1 && (int64_t)V <= (int64_t)S * SP_VOX);
    CLMGS_CHECK_ARG(ts_aligned(cell_scan, 4) && ts_aligned(verts, 4) && colours != nullptr && ts_aligned(vert_keys, 8));
    TsdfCams G;
    CLMGS_CHECK_ARG(ts_load_g2w(grid_to_world, G));
    const uint64_t vbytes = (uint64_t)V * 12, cbytes = (uint64_t)V * 3, kbytes = (uint64_t)V * 8;
    CLMGS_CHECK_ARG(clear(verts, vbytes) && clear(colours, cbytes) && clear(vert_keys, kbytes) &&
                    ts_apart(verts, vbytes, colours, cbytes) && ts_apart(verts, vbytes, vert_keys, kbytes) &&
                    ts_apart(colours, cbytes, vert_keys, kbytes));
    hipLaunchKernelGGL(tsdf_vertices_kernel<BrickVol>, grid, block, 0, st, D, cell_scan, V, G, verts, colours);
  } else {
    CLMGS_CHECK_ARG(V >= 1 && (int64_t)V <= (int64_t)S * SP_VOX && Q >= 1 && Q < (1 << 30) && ts_weight(min_weight));
    CLMGS_CHECK_ARG(ts_aligned(cell_scan, 4) && ts_aligned(quad_scan, 4) && ts_aligned(faces, 4) && ts_aligned(quad_keys, 8));
    const uint64_t fbytes = (uint64_t)Q * 24, kbytes = (uint64_t)Q * 8;
    CLMGS_CHECK_ARG(clear(faces, fbytes) && clear(quad_keys, kbytes) && ts_apart(faces, fbytes, quad_keys, kbytes));
    hipLaunchKernelGGL((tsdf_quads_kernel<BrickVol, true>), grid, block, 0, st, D, min_weight, cell_scan, (int32_t*)nullptr,
                       quad_scan, V, Q, faces);
  }
  CLMGS_LAUNCH_CHECK();
  return 0;
}
