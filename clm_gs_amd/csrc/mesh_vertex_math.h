// Mesh smoothing and vertex normals ("Mesh smoothing and normals"): the arithmetic of
// csrc/mesh_smooth.hip, host and device -- the neighbour sum of one incidence, the umbrella step of a vertex, the
// area-weighted normal of a face and the normalisation of a vertex's sum.
//
// No contraction: every product, quotient and sum below is float64 and rounded on its own, in the order written, which is
// the order of tests/mesh_smooth_reference.py; positions and normals are compared with that restatement bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MV_HD __host__ __device__ __forceinline__
#else
#define MV_HD inline
#endif

namespace clmgs {

// One incidence of a vertex: the two other corners of the face, in the face's rotation, added to s one after the other.
MV_HD void mv_add_neighbours(const double* pa, const double* pb, double* s) {
#pragma clang fp contract(off)
  s[0] = s[0] + pa[0];
  s[1] = s[1] + pa[1];
  s[2] = s[2] + pa[2];
  s[0] = s[0] + pb[0];
  s[1] = s[1] + pb[1];
  s[2] = s[2] + pb[2];
}

// The umbrella step of a vertex p with the sum s of n neighbour terms: float32(p + c (s / n - p)); p itself for n == 0.
MV_HD void mv_step(const float* p, const double* s, int64_t n, double c, float* out) {
#pragma clang fp contract(off)
  if (n <= 0) {
    out[0] = p[0];
    out[1] = p[1];
    out[2] = p[2];
    return;
  }
  const double dn = (double)n;
  for (int d = 0; d < 3; ++d) {
    const double pd = (double)p[d];
    const double m = s[d] / dn;
    out[d] = (float)(pd + c * (m - pd));
  }
}

// a += (p1 - p0) x (p2 - p0): the face's normal times twice its area, from the corners in STORED order, so that every
// vertex of the face adds the same bits.
MV_HD void mv_add_face_normal(const double* p0, const double* p1, const double* p2, double* a) {
#pragma clang fp contract(off)
  const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const double n0 = e1[1] * e2[2] - e1[2] * e2[1];
  const double n1 = e1[2] * e2[0] - e1[0] * e2[2];
  const double n2 = e1[0] * e2[1] - e1[1] * e2[0];
  a[0] = a[0] + n0;
  a[1] = a[1] + n1;
  a[2] = a[2] + n2;
}

// float32(a / |a|), or (0, 0, 0) where |a|^2 is zero, NaN or infinite.
MV_HD void mv_normalise(const double* a, float* out) {
#pragma clang fp contract(off)
  const double q = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
  if (!(q > 0.0) || !isfinite(q)) {
    out[0] = out[1] = out[2] = 0.0f;
    return;
  }
  const double inv = 1.0 / sqrt(q);
  out[0] = (float)(a[0] * inv);
  out[1] = (float)(a[1] * inv);
  out[2] = (float)(a[2] * inv);
}

}  // namespace clmgs
