// Ray depth ("Ray depth"): the arithmetic of csrc/ray_depth.hip, host and device -- the depth of the
// point on a pixel's ray at which one Gaussian's 3-D density is largest (the ray-Gaussian intersection depth of RaDe-GS and
// GOF), where the blended and the median depth report the depth of the Gaussian's centre.
//
// The density along the ray o + t d is exp(-0.5 (o + t d - m)^T S^-1 (o + t d - m)) with S = B diag(s^2) B^T in camera
// axes; its maximum lies at  t* = d^T S^-1 (m - o) / d^T S^-1 d.  S^-1 is never formed: with g = diag(1/s) B^T d and
// p = diag(1/s) B^T (m - o) the two forms are g.p and g.g -- two rotations into the Gaussian's own axes and six divisions.
// A flat Gaussian (one scale thousands of times smaller than the others) makes S^-1 ill conditioned, not g and p; and a
// common factor on the three scales multiplies g.p and g.g alike (a power of two changes no bit).
//
// float64 throughout, no contraction: every product, quotient and sum below is rounded on its own, in the order written,
// so that a restatement in another language computes the same numbers (tests/ray_depth_reference.py compares bit for
// bit).  The inputs are the float32 values the projection reads, widened.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RAY_HD __host__ __device__ __forceinline__
#else
#define RAY_HD inline
#endif

namespace clmgs {

constexpr int RAY_CAM_DOUBLES = 16;  // a camera record: the view matrix's top 3x4 (row-major: Rv | t), fx, fy, cx, cy

// quat_to_rotmat of gs_math.h in double: q = (w, x, y, z), normalised here.
RAY_HD void ray_quat_to_rotmat(const double q[4], double R[9]) {
#pragma clang fp contract(off)
  const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  const double inv = 1.0 / sqrt(n2);
  const double w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

RAY_HD double ray_dot3(double a, double b, double c, double d, double e, double f) {
#pragma clang fp contract(off)
  return (a * b + c * d) + e * f;
}

// The ray parameter t* of pixel (px, py) of camera record `cam` for the Gaussian (mu, q, s): s the ACTIVATED scales.
// ortho == 0: pinhole, origin 0, direction (u, v, 1); ortho != 0: K in pixels per world unit (ortho_math.h), origin
// (u, v, 0), direction (0, 0, 1).  In both the origin has z = 0 and the direction z = 1, so t* is a camera z-depth.
// May be NaN or infinite (a zero scale, g.g == 0, non-finite inputs): ray_depth decides.
RAY_HD double ray_tstar(const double mu[3], const double q[4], const double s[3], const double* cam, double px, double py,
                        int ortho) {
#pragma clang fp contract(off)
  double R[9], B[9], m[3];
  ray_quat_to_rotmat(q, R);
  for (int i = 0; i < 3; ++i) {
    const double* rv = cam + 4 * i;
    for (int j = 0; j < 3; ++j) B[3 * i + j] = ray_dot3(rv[0], R[j], rv[1], R[3 + j], rv[2], R[6 + j]);  // B = Rv R
    m[i] = ray_dot3(rv[0], mu[0], rv[1], mu[1], rv[2], mu[2]) + rv[3];
  }
  const double u = ((px + 0.5) - cam[14]) / cam[12];
  const double v = ((py + 0.5) - cam[15]) / cam[13];
  const double o[3] = {ortho ? u : 0.0, ortho ? v : 0.0, 0.0};
  const double d[3] = {ortho ? 0.0 : u, ortho ? 0.0 : v, 1.0};
  const double r[3] = {m[0] - o[0], m[1] - o[1], m[2] - o[2]};
  double g[3], p[3];
  for (int j = 0; j < 3; ++j) {
    g[j] = ray_dot3(B[j], d[0], B[3 + j], d[1], B[6 + j], d[2]) / s[j];
    p[j] = ray_dot3(B[j], r[0], B[3 + j], r[1], B[6 + j], r[2]) / s[j];
  }
  const double num = ray_dot3(g[0], p[0], g[1], p[1], g[2], p[2]);
  const double den = ray_dot3(g[0], g[0], g[1], g[1], g[2], g[2]);
  return num / den;
}

// The depth reported: (float) t* where t* is finite and in front of the near plane, else the centre depth handed in
// (the median pass's value, returned as it is).
RAY_HD float ray_depth(const double mu[3], const double q[4], const double s[3], const double* cam, double px, double py,
                       int ortho, double near, float centre_depth) {
  const double t = ray_tstar(mu, q, s, cam, px, py, ortho);
  return (isfinite(t) && t > near) ? (float)t : centre_depth;
}

}  // namespace clmgs
