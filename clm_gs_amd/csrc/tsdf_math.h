// Mesh export ("Mesh export"): the arithmetic of csrc/tsdf.hip, host and device -- the projection of
// a voxel into a camera and the TSDF update of the fusion, and the vertex of an active cell of the naive Surface Nets
// extraction.
//
// No contraction: every product, quotient and sum below is rounded on its own, in the order written, so that a
// restatement in another language computes the same numbers (tests/tsdf_reference.py compares the fused grid bit for
// bit).  The projection is float64 (as lens_math.h and mcmc.hip): a voxel is decided by floor(u), floor(v) and three
// comparisons, and a float32 projection would decide thousands of voxels per camera differently from any reference.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TSDF_HD __host__ __device__ __forceinline__
#else
#define TSDF_HD inline
#endif

namespace clmgs {

constexpr int TSDF_MAX_B = 16;        // cameras of one launch
constexpr int TSDF_CAM_DOUBLES = 16;  // a camera record: the 12 entries of M (3x4, row-major), fx, fy, cx, cy
constexpr int TSDF_PLANES = 6;        // tsum, wsum, cr, cg, cb, cw

// One row of a 3x4 matrix applied to (px, py, pz, 1).
TSDF_HD double tsdf_row(const double* r, double px, double py, double pz) {
#pragma clang fp contract(off)
  return ((r[0] * px + r[1] * py) + r[2] * pz) + r[3];
}

// Grid point (px, py, pz) = (i + 0.5, j + 0.5, k + 0.5) through the camera record c -> the pixel (col, row) that
// contains its projection (pixel j covers [j, j + 1)) and its camera depth z.  False: z <= near (or NaN), or the
// projection lies outside the H x W image (a NaN fails every comparison).
TSDF_HD bool tsdf_pixel(const double* c, double px, double py, double pz, double near, int H, int W, int& col, int& row,
                        double& z) {
#pragma clang fp contract(off)
  z = tsdf_row(c + 8, px, py, pz);
  if (!(z > near)) return false;
  const double x = tsdf_row(c, px, py, pz), y = tsdf_row(c + 4, px, py, pz);
  const double u = c[12] * x / z + c[14];
  const double v = c[13] * y / z + c[15];
  const double fu = floor(u), fv = floor(v);
  if (!(fu >= 0.0 && fu < (double)W && fv >= 0.0 && fv < (double)H)) return false;
  col = (int)fu;
  row = (int)fv;
  return true;
}

// The observation of a voxel at camera depth z by a pixel of expected depth d and opacity a: false when the pixel is
// gated (alpha, depth range; a NaN depth fails) or the voxel lies more than trunc behind the surface.
TSDF_HD bool tsdf_sdf(float d, float a, double z, float depth_max, float alpha_min, float trunc, float& sdf) {
#pragma clang fp contract(off)
  if (!(a >= alpha_min && d > 0.0f && d <= depth_max)) return false;
  sdf = d - (float)z;
  return !(sdf < -trunc);
}

TSDF_HD float tsdf_term(float sdf, float inv_trunc) {
#pragma clang fp contract(off)
  return fminf(sdf * inv_trunc, 1.0f);
}

TSDF_HD float tsdf_clamp01(float c) { return fminf(fmaxf(c, 0.0f), 1.0f); }

// ---------------------------------------------------------------------------------------------- extraction
TSDF_HD bool tsdf_valid(float wsum, float min_weight) { return wsum >= min_weight; }
TSDF_HD bool tsdf_inside(float tsum) { return tsum < 0.0f; }

// Corner c of a cell is the voxel (i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)).  A cell is active iff all eight
// voxels are valid and their inside flags differ.
TSDF_HD bool tsdf_cell_active(const float* tsum8, const float* wsum8, float min_weight) {
  int in = 0;
  bool ok = true;
  for (int c = 0; c < 8; ++c) {
    ok = ok && tsdf_valid(wsum8[c], min_weight);
    in += tsdf_inside(tsum8[c]) ? 1 : 0;
  }
  return ok && in != 0 && in != 8;
}

// Edge e = 4 * axis + r of a cell joins corners a and a + (1 << axis): axis x (0,1) (2,3) (4,5) (6,7), axis y (0,2) (1,3)
// (4,6) (5,7), axis z (0,4) (1,5) (2,6) (3,7).
TSDF_HD int tsdf_edge_corner(int axis, int r) {
  const int s = 1 << axis;
  return (r & (s - 1)) | ((r >> axis) << (axis + 1));
}

// The vertex of the ACTIVE cell (i, j, k): the mean, in float64, of the zero crossings of its sign-changing edges,
// interpolated linearly on tsum / wsum, in grid coordinates (voxel (i, j, k) sits at (i + 0.5, j + 0.5, k + 0.5)), mapped
// through g2w (3x4, row-major) and rounded to float32; its colour the same mean of the interpolated corner colours
// c / cw (0.5 where cw == 0), quantised with floor(255 c + 0.5).  vox[p][c]: plane p of corner c.
TSDF_HD void tsdf_cell_vertex(const float (*vox)[8], int i, int j, int k, const double* g2w, float* xyz, uint8_t* rgb) {
#pragma clang fp contract(off)
  double val[8], col[3][8];
  for (int c = 0; c < 8; ++c) {
    val[c] = (double)vox[0][c] / (double)vox[1][c];
    for (int ch = 0; ch < 3; ++ch) col[ch][c] = vox[5][c] > 0.0f ? (double)vox[2 + ch][c] / (double)vox[5][c] : 0.5;
  }
  double sp[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
  int n = 0;
  for (int axis = 0; axis < 3; ++axis)
    for (int r = 0; r < 4; ++r) {
      const int a = tsdf_edge_corner(axis, r), b = a + (1 << axis);
      if (tsdf_inside(vox[0][a]) == tsdf_inside(vox[0][b])) continue;
      const double t = val[a] / (val[a] - val[b]);
      for (int d = 0; d < 3; ++d) sp[d] = sp[d] + (d == axis ? t : (double)((a >> d) & 1));
      for (int ch = 0; ch < 3; ++ch) sc[ch] = sc[ch] + (col[ch][a] + t * (col[ch][b] - col[ch][a]));
      ++n;
    }
  const double dn = (double)n;
  const double gx = ((double)i + 0.5) + sp[0] / dn, gy = ((double)j + 0.5) + sp[1] / dn, gz = ((double)k + 0.5) + sp[2] / dn;
  for (int d = 0; d < 3; ++d) xyz[d] = (float)tsdf_row(g2w + 4 * d, gx, gy, gz);
  for (int ch = 0; ch < 3; ++ch) {
    double q = floor(255.0 * (sc[ch] / dn) + 0.5);
    q = q >= 0.0 ? q : 0.0;
    rgb[ch] = (uint8_t)(q <= 255.0 ? q : 255.0);
  }
}

}  // namespace clmgs
