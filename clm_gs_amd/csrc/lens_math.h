// Lens distortion ("Lens distortion"): the inverse map of csrc/undistort.hip in float64, host and
// device.  One record describes every accepted COLMAP model (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV,
// OPENCV_FISHEYE): intrinsics in pixels of the decoded source image, COLMAP's convention (the centre of the top-left
// pixel is at (0.5, 0.5)), and the coefficients a model does not have are 0.
//
// No contraction: every product and sum below is rounded on its own, in the order written, so that a float64 restatement
// in another language computes the same doubles (the tests compare pixel for pixel, not within a tolerance).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LENS_HD __host__ __device__ __forceinline__
#else
#define LENS_HD inline
#endif

namespace clmgs {

struct LensRec {
  double fx, fy, cx, cy, k1, k2, k3, k4, p1, p2;
  int fisheye;
};

constexpr double LENS_TAU = 1.0 / 1048576.0;  // 2^-20 px: the slack of the bounds test (an identity lens lands ON the rim)

// Output pixel (i, j) of the Ho x Wo centred pinhole with focal lengths fxo, fyo -> the sample position (u, v) in pixel
// indices of the source image and `mono`, the derivative of the distorted radius (<= 0: the radial profile has folded
// back and the position is a second image of a ray that is not there).
LENS_HD void lens_map(const LensRec& L, double fxo, double fyo, int Ho, int Wo, int i, int j, double& u, double& v,
                      double& mono) {
#pragma clang fp contract(off)
  const double x = ((double)j + 0.5 - (double)Wo / 2.0) / fxo;
  const double y = ((double)i + 0.5 - (double)Ho / 2.0) / fyo;
  const double r2 = x * x + y * y;
  double xd, yd;
  if (L.fisheye) {
    const double r = sqrt(r2), th = atan(r), t2 = th * th;
    const double rad = 1.0 + t2 * (L.k1 + t2 * (L.k2 + t2 * (L.k3 + t2 * L.k4)));
    mono = 1.0 + t2 * (3.0 * L.k1 + t2 * (5.0 * L.k2 + t2 * (7.0 * L.k3 + t2 * 9.0 * L.k4)));
    const double s = r < 1e-12 ? 1.0 : th * rad / r;
    xd = x * s;
    yd = y * s;
  } else {
    const double rad = 1.0 + r2 * (L.k1 + r2 * L.k2);
    mono = 1.0 + r2 * (3.0 * L.k1 + r2 * 5.0 * L.k2);
    xd = x * rad + 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * x * x);
    yd = y * rad + L.p1 * (r2 + 2.0 * y * y) + 2.0 * L.p2 * x * y;
  }
  u = L.fx * xd + L.cx - 0.5;
  v = L.fy * yd + L.cy - 0.5;
}

// mono > 0 and (u, v) inside the source's pixel centres, with the slack.  A NaN fails every comparison: invalid.
LENS_HD bool lens_valid(double u, double v, double mono, int Hs, int Ws) {
  return mono > 0.0 && u >= -LENS_TAU && u <= (double)(Ws - 1) + LENS_TAU && v >= -LENS_TAU &&
         v <= (double)(Hs - 1) + LENS_TAU;
}

// One axis of the bilinear footprint: t clamped into [0, n-1] (a NaN becomes 0) -> the two taps and the weight of the
// second.  i0 <= i1 <= n - 1 always: the taps of ANY pixel, valid or not, lie inside the source.
LENS_HD void lens_taps(double t, int n, int& i0, int& i1, double& w) {
#pragma clang fp contract(off)
  t = t >= 0.0 ? t : 0.0;
  t = t <= (double)(n - 1) ? t : (double)(n - 1);
  const int top = n >= 2 ? n - 2 : 0;
  const int f = (int)floor(t);
  i0 = f < top ? f : top;
  i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
  w = t - (double)i0;
}

// The blend of the four taps, rounded half up (val >= 0, so floor(val + 0.5) is the rounding).
LENS_HD double lens_blend(double a, double b, double p00, double p01, double p10, double p11) {
#pragma clang fp contract(off)
  const double val = (1.0 - b) * ((1.0 - a) * p00 + a * p01) + b * ((1.0 - a) * p10 + a * p11);
  return floor(val + 0.5);
}

}  // namespace clmgs
