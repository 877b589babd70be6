// Mesh evaluation ("Mesh evaluation"): the arithmetic of csrc/mesh_distance.hip, host and device --
// the squared distance from a point to a triangle and to a point, the area of a face, the number and the positions of
// its samples, and the cell of a coordinate in the primitive grid.
//
// No contraction: every product, quotient, sum and difference below is float64 and rounded on its own, in the order
// written, which is the order of tests/mesh_eval_reference.py; distances and samples are compared with that restatement
// bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MD_HD __host__ __device__ __forceinline__
#else
#define MD_HD inline
#endif

namespace clmgs {

constexpr double MD_R2_U = 0.7548776662466927;  // 1 / g and 1 / g^2 of the plastic number g: the R2 sequence
constexpr double MD_R2_V = 0.5698402909980532;
constexpr int64_t MD_MAX_FACE_SAMPLES = (int64_t)1 << 31;  // n_f is capped here, so that a sum over F < 2^31 faces fits int64

MD_HD double md_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// |p - a|^2, summed x, y, z.
MD_HD double md_point_d2(const double* p, const double* a) {
#pragma clang fp contract(off)
  const double d[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  return md_dot(d, d);
}

// The squared distance from p to the triangle abc: the closest point q of Ericson, Real-Time Collision Detection 5.1.5,
// with the region tests in the book's order (vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior), then
// |p - q|^2.  NaN for a triangle without area whose interior branch is reached: such faces are not primitives.
MD_HD double md_closest_d2(const double* p, const double* a, const double* b, const double* c) {
#pragma clang fp contract(off)
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const double d1 = md_dot(ab, ap), d2 = md_dot(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) return md_point_d2(p, a);
  const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
  const double d3 = md_dot(ab, bp), d4 = md_dot(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) return md_point_d2(p, b);
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double v = d1 / (d1 - d3);
    const double q[3] = {a[0] + v * ab[0], a[1] + v * ab[1], a[2] + v * ab[2]};
    return md_point_d2(p, q);
  }
  const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const double d5 = md_dot(ab, cp), d6 = md_dot(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) return md_point_d2(p, c);
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    const double q[3] = {a[0] + w * ac[0], a[1] + w * ac[1], a[2] + w * ac[2]};
    return md_point_d2(p, q);
  }
  const double va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
    const double w = e43 / (e43 + e56);
    const double q[3] = {b[0] + w * (c[0] - b[0]), b[1] + w * (c[1] - b[1]), b[2] + w * (c[2] - b[2])};
    return md_point_d2(p, q);
  }
  const double denom = 1.0 / ((va + vb) + vc);
  const double v = vb * denom, w = vc * denom;
  const double q[3] = {(a[0] + ab[0] * v) + ac[0] * w, (a[1] + ab[1] * v) + ac[1] * w, (a[2] + ab[2] * v) + ac[2] * w};
  return md_point_d2(p, q);
}

// 0.5 sqrt(|(b - a) x (c - a)|^2).
MD_HD double md_face_area(const double* a, const double* b, const double* c) {
#pragma clang fp contract(off)
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
  return 0.5 * sqrt(md_dot(n, n));
}

// A face is a primitive (sampled, binned, measured against) iff its area is positive and finite.
MD_HD bool md_area_ok(double area) { return area > 0.0 && isfinite(area); }

// ceil(area / spacing^2), at most MD_MAX_FACE_SAMPLES; 0 for a face that is no primitive.
MD_HD int64_t md_sample_count(double area, double spacing) {
#pragma clang fp contract(off)
  if (!md_area_ok(area)) return 0;
  const double n = ceil(area / (spacing * spacing));
  if (!(n < (double)MD_MAX_FACE_SAMPLES)) return MD_MAX_FACE_SAMPLES;
  return n < 1.0 ? 1 : (int64_t)n;
}

// Sample k of a face: the R2 sequence folded into the triangle.  -> (u, v) with u, v >= 0 and u + v <= 1.
MD_HD void md_sample_uv(int64_t k, double* u, double* v) {
#pragma clang fp contract(off)
  const double i = (double)(k + 1);
  const double tu = 0.5 + i * MD_R2_U, tv = 0.5 + i * MD_R2_V;
  double uu = tu - floor(tu), vv = tv - floor(tv);
  if (uu + vv > 1.0) {
    uu = 1.0 - uu;
    vv = 1.0 - vv;
  }
  *u = uu;
  *v = vv;
}

// float32((a + u (b - a)) + v (c - a)) per coordinate.
MD_HD void md_sample_position(int64_t k, const double* a, const double* b, const double* c, float* out) {
#pragma clang fp contract(off)
  double u, v;
  md_sample_uv(k, &u, &v);
  for (int d = 0; d < 3; ++d) out[d] = (float)((a[d] + u * (b[d] - a[d])) + v * (c[d] - a[d]));
}

// The cell of a coordinate along one axis of the grid: clamp(floor((x - o) / h), 0, g - 1).  Monotone in x.  A NaN goes
// to cell 0 (no caller passes one).
MD_HD int md_cell(double x, double o, double h, int g) {
#pragma clang fp contract(off)
  const double t = floor((x - o) / h);
  if (!(t >= 0.0)) return 0;
  return t > (double)(g - 1) ? g - 1 : (int)t;
}

}  // namespace clmgs
