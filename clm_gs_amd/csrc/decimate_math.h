// Mesh decimation ("Mesh decimation"): the arithmetic of csrc/mesh_decimate.hip, host and device --
// the cell of a vertex, the quadric of a face about a cell centre and the placement of a cluster's vertex.
//
// No contraction: every product, quotient and sum below is float64 and rounded on its own, in the order written, which is
// the order of tests/mesh_decimate_reference.py; the output vertex is compared with that restatement bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DEC_HD __host__ __device__ __forceinline__
#else
#define DEC_HD inline
#endif

namespace clmgs {

constexpr int64_t DEC_BIAS = (int64_t)1 << 20;  // cell indices lie in [-2^20, 2^20)
constexpr int DEC_NONFINITE = 1, DEC_RANGE = 2;  // the bits of the key pass's flag
constexpr int DEC_QUADRIC = 0, DEC_MEAN_DEGENERATE = 1, DEC_MEAN_OUTSIDE = 2;  // placement codes

// The key of the cell of (x, y, z): ((i + 2^20) << 42) | ((j + 2^20) << 21) | (k + 2^20) with i = floor(double(x) / cell).
// Returns 0, or the flag bit of what refuses the vertex (then key is -1).
DEC_HD int dec_key(float x, float y, float z, double cell, int64_t& key) {
#pragma clang fp contract(off)
  const double q[3] = {floor((double)x / cell), floor((double)y / cell), floor((double)z / cell)};
  key = -1;
  if (!(isfinite((double)x) && isfinite((double)y) && isfinite((double)z))) return DEC_NONFINITE;
  for (int e = 0; e < 3; ++e)
    if (!(q[e] >= -(double)DEC_BIAS && q[e] < (double)DEC_BIAS)) return DEC_RANGE;
  key = (((int64_t)q[0] + DEC_BIAS) << 42) | (((int64_t)q[1] + DEC_BIAS) << 21) | ((int64_t)q[2] + DEC_BIAS);
  return 0;
}

// The centre of the cell of a key: c = (double(i) + 0.5) * cell per axis.
DEC_HD void dec_centre(int64_t key, double cell, double* c) {
#pragma clang fp contract(off)
  const int64_t m = 2 * DEC_BIAS - 1;
  c[0] = ((double)((key >> 42) - DEC_BIAS) + 0.5) * cell;
  c[1] = ((double)(((key >> 21) & m) - DEC_BIAS) + 0.5) * cell;
  c[2] = ((double)((key & m) - DEC_BIAS) + 0.5) * cell;
}

// One face (p0, p1, p2) added to the sums of a cluster centred at c: A (00 01 02 11 12 22) += nrm nrm^T and r += -d nrm
// with nrm = (p1 - p0) x (p2 - p0), not normalised, and d = -(nrm . (p0 - c)).
DEC_HD void dec_add_face(const double* p0, const double* p1, const double* p2, const double* c, double* A, double* r) {
#pragma clang fp contract(off)
  const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const double n0 = e1[1] * e2[2] - e1[2] * e2[1];
  const double n1 = e1[2] * e2[0] - e1[0] * e2[2];
  const double n2 = e1[0] * e2[1] - e1[1] * e2[0];
  const double a0 = p0[0] - c[0], a1 = p0[1] - c[1], a2 = p0[2] - c[2];
  const double d = -((n0 * a0 + n1 * a1) + n2 * a2);
  A[0] = A[0] + n0 * n0;
  A[1] = A[1] + n0 * n1;
  A[2] = A[2] + n0 * n2;
  A[3] = A[3] + n1 * n1;
  A[4] = A[4] + n1 * n2;
  A[5] = A[5] + n2 * n2;
  r[0] = r[0] + (-d) * n0;
  r[1] = r[1] + (-d) * n1;
  r[2] = r[2] + (-d) * n2;
}

// The offset x of a cluster's vertex from its cell centre: the minimiser of sum (nrm . x + d)^2 + mu |x - m|^2, that is
// (A + mu I) x = r + mu m with mu = (tr 2^-10) / 3, solved by the adjugate; the mean m where that fails.  -> the
// placement code.
DEC_HD int dec_place(const double* A, const double* r, const double* m, double cell, double* x) {
#pragma clang fp contract(off)
  x[0] = m[0];
  x[1] = m[1];
  x[2] = m[2];
  const double tr = (A[0] + A[3]) + A[5];
  if (!(tr > 0.0)) return DEC_MEAN_DEGENERATE;
  const double mu = (tr * 0.0009765625) / 3.0;
  const double a00 = A[0] + mu, a01 = A[1], a02 = A[2], a11 = A[3] + mu, a12 = A[4], a22 = A[5] + mu;
  const double b0 = r[0] + mu * m[0], b1 = r[1] + mu * m[1], b2 = r[2] + mu * m[2];
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  const double y0 = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
  const double y1 = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
  const double y2 = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
  if (!(det > 0.0) || !(isfinite(y0) && isfinite(y1) && isfinite(y2))) return DEC_MEAN_DEGENERATE;
  if (fabs(y0) > cell || fabs(y1) > cell || fabs(y2) > cell) return DEC_MEAN_OUTSIDE;
  x[0] = y0;
  x[1] = y1;
  x[2] = y2;
  return DEC_QUADRIC;
}

}  // namespace clmgs
