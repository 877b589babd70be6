// Mesh export ("Mesh export" and "Sparse volume"): the two pieces of the TSDF fusion that the dense
// kernel (csrc/tsdf.hip) and the brick-allocated one (csrc/tsdf_sparse.hip) share, as raster_tile.h does for the tile
// kernels: the frustum cull of a box of voxel centres and the sequential camera loop of one voxel.  Both volumes run this
// code, so a voxel stored in both carries the same six sums, bit for bit.  The arithmetic is csrc/tsdf_math.h.
#pragma once
#include "common.h"
#include "tsdf_math.h"

namespace clmgs {

constexpr double TS_CULL_EPS = 1.0 / 1099511627776.0;  // 2^-40

struct TsdfCams {
  double c[TSDF_MAX_B][TSDF_CAM_DOUBLES];
};

// |r0| X + |r1| Y + |r2| Z + |r3|: a bound of the magnitude of every term of tsdf_row over the box [0,X] x [0,Y] x [0,Z]
__device__ __forceinline__ double row_mag(const double* r, double X, double Y, double Z) {
  return fabs(r[0]) * X + fabs(r[1]) * Y + fabs(r[2]) * Z + fabs(r[3]);
}

// The cull of a workgroup (>= 128 lanes, all of them call): lane 8 b + c projects corner c of the box of voxel centres
// [xl, xh] x [yl, yh] x [zl, zh] into camera b and tests it against five half spaces: behind the near plane, and (with
// near >= 0) left, right, above and below the image by more than a pixel, each as a LINEAR function of the grid point
// with a margin of 2^-40 of the magnitude of its terms.  -> the mask of the cameras that may observe a voxel of the box.
__device__ __forceinline__ unsigned ts_cull_seen(const TsdfCams& cams, int B, int H, int W, double near, double xl, double xh,
                                                 double yl, double yh, double zl, double zh, unsigned char* seen_lds) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t < 8 * TSDF_MAX_B) {  // waves 0 and 1, whole: lanes 8 b .. 8 b + 7 are the corners of camera b
    const int b = t >> 3, c = t & 7;
    bool out[5] = {false, false, false, false, false};
    if (b < B) {
      const double* m = cams.c[b];
      const double px = (c & 1) ? xh : xl, py = (c & 2) ? yh : yl, pz = (c & 4) ? zh : zl;
      const double x = tsdf_row(m, px, py, pz), y = tsdf_row(m + 4, px, py, pz), z = tsdf_row(m + 8, px, py, pz);
      const double sx = row_mag(m, xh, yh, zh), sy = row_mag(m + 4, xh, yh, zh), sz = row_mag(m + 8, xh, yh, zh);
      const double fx = m[12], fy = m[13], cx = m[14], cy = m[15];
      out[0] = z + TS_CULL_EPS * (sz + fabs(near)) < near;
      if (near >= 0.0) {
        const double l = cx + 1.0, r = cx - (double)W - 1.0, u = cy + 1.0, d = cy - (double)H - 1.0;
        out[1] = fx * x + l * z + TS_CULL_EPS * (fx * sx + fabs(l) * sz) < 0.0;
        out[2] = fx * x + r * z - TS_CULL_EPS * (fx * sx + fabs(r) * sz) > 0.0;
        out[3] = fy * y + u * z + TS_CULL_EPS * (fy * sy + fabs(u) * sz) < 0.0;
        out[4] = fy * y + d * z - TS_CULL_EPS * (fy * sy + fabs(d) * sz) > 0.0;
      }
    }
    bool culled = false;
#pragma unroll
    for (int p = 0; p < 5; ++p) {  // the eight corners of a camera are eight neighbouring lanes of one wave
      const unsigned long long all = __ballot(out[p]);
      culled = culled || ((all >> (t & 56)) & 0xffull) == 0xffull;
    }
    if (c == 0) seen_lds[b] = (b < B && !culled) ? 1 : 0;
  }
  __syncthreads();
  unsigned seen = 0u;
#pragma unroll
  for (int b = 0; b < TSDF_MAX_B; ++b) seen |= seen_lds[b] ? (1u << b) : 0u;
  return seen;
}

// The cameras of `seen`, in order, on the voxel at the grid point (px, py, pz) whose six sums sit at g[0], g[n], ..,
// g[5 n]: loaded at the first camera that observes it and stored only then.
__device__ __forceinline__ void ts_fuse_voxel(float* g, int64_t n, const TsdfCams& cams, int B, unsigned seen, double px,
                                              double py, double pz, double near, int H, int W, int64_t hw,
                                              const float* __restrict__ depth, const float* __restrict__ alpha,
                                              const float* __restrict__ rgb, float depth_max, float alpha_min, float trunc,
                                              float inv_trunc) {
#pragma clang fp contract(off)
  float tsum = 0.f, wsum = 0.f, cr = 0.f, cg = 0.f, cb = 0.f, cw = 0.f;
  bool touched = false, coloured = false;
  for (int b = 0; b < B; ++b) {
    if (!((seen >> b) & 1u)) continue;
    int col, row;
    double z;
    if (!tsdf_pixel(cams.c[b], px, py, pz, near, H, W, col, row, z)) continue;
    const int64_t pix = (int64_t)b * hw + (int64_t)row * W + col;
    float sdf;
    if (!tsdf_sdf(depth[pix], alpha[pix], z, depth_max, alpha_min, trunc, sdf)) continue;
    if (!touched) {
      tsum = g[0];
      wsum = g[n];
      touched = true;
    }
    tsum = tsum + tsdf_term(sdf, inv_trunc);
    wsum = wsum + 1.0f;
    if (sdf <= trunc) {
      if (!coloured) {
        cr = g[2 * n];
        cg = g[3 * n];
        cb = g[4 * n];
        cw = g[5 * n];
        coloured = true;
      }
      const float* c3 = rgb + ((int64_t)b * 3) * hw + (int64_t)row * W + col;
      cr = cr + tsdf_clamp01(c3[0]);
      cg = cg + tsdf_clamp01(c3[hw]);
      cb = cb + tsdf_clamp01(c3[2 * hw]);
      cw = cw + 1.0f;
    }
  }
  if (touched) {  // a voxel no camera of the batch observed is not stored back
    g[0] = tsum;
    g[n] = wsum;
  }
  if (coloured) {
    g[2 * n] = cr;
    g[3 * n] = cg;
    g[4 * n] = cb;
    g[5 * n] = cw;
  }
}

// Argument checks shared by the entries of both volumes.
static inline bool ts_aligned(const void* p, size_t a) { return p != nullptr && ((uintptr_t)p % a) == 0; }

// [a, a + na) and [b, b + nb) do not overlap
static inline bool ts_apart(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + na <= b0 || b0 + nb <= a0;
}

static inline bool ts_weight(float w) { return isfinite(w) && w > 0.0f; }

constexpr int TS_MAX_SIDE = 32768;  // of an image

static inline bool ts_image(int H, int W) { return H >= 1 && W >= 1 && H <= TS_MAX_SIDE && W <= TS_MAX_SIDE; }

// B records of TSDF_CAM_DOUBLES doubles as the kernel argument, the rest zero; false: null, B outside 1 .. TSDF_MAX_B, an
// entry that is not finite or above max_entry in magnitude (the marking's bound; INFINITY: none), a focal length <= 0.
static inline bool ts_load_cams(const double* cams, int B, double max_entry, TsdfCams& C) {
  if (cams == nullptr || B < 1 || B > TSDF_MAX_B) return false;
  for (int b = 0; b < TSDF_MAX_B; ++b)
    for (int e = 0; e < TSDF_CAM_DOUBLES; ++e) {
      C.c[b][e] = b < B ? cams[b * TSDF_CAM_DOUBLES + e] : 0.0;
      if (!isfinite(C.c[b][e]) || fabs(C.c[b][e]) > max_entry) return false;
    }
  for (int b = 0; b < B; ++b)
    if (!(C.c[b][12] > 0.0 && C.c[b][13] > 0.0)) return false;
  return true;
}

}  // namespace clmgs
