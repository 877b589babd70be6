// Per-element arithmetic of the orthographic projection (gsplat's camera_model="ortho"), beside gs_math.h and with the
// same two builds: inlined into the gfx950 kernels of ortho.hip, and compiled with plain g++ by tests/.
//
// An orthographic camera has K = [[sx,0,cx],[0,sy,cy],[0,0,1]] with sx, sy in pixels per world unit (Cam::fx / fy).
// The projection of p = R m + t is (sx p.x + cx, sy p.y + cy), its Jacobian J = [[sx,0,0],[0,sy,0]] is the same for
// every point: no perspective divide, no frustum clamp, no vJ terms in the VJP.  The depth stays p.z.
#pragma once
#include "gs_math.h"

namespace clmgs {

// Intermediate values shared by forward and backward (ProjMid without the Jacobian).
struct OrthoMid {
  float p[3];                // camera-space mean
  float M[9];                // R(q) * diag(s)
  float Sc[6];               // camera-space covariance, upper triangle xx xy xz yy yz zz
  float c00, c01, c11, det;  // blurred 2D covariance
  float det_orig;            // determinant of J Sc J^T before eps2d is added
};

CLMGS_HD bool ortho_mid(const Cam& cam, const float m[3], const float q[4], const float s[3], float eps2d,
                        float near_plane, float far_plane, OrthoMid& o) {
  const float* Rv = cam.R;
  o.p[0] = Rv[0] * m[0] + Rv[1] * m[1] + Rv[2] * m[2] + cam.t[0];
  o.p[1] = Rv[3] * m[0] + Rv[4] * m[1] + Rv[5] * m[2] + cam.t[1];
  o.p[2] = Rv[6] * m[0] + Rv[7] * m[1] + Rv[8] * m[2] + cam.t[2];
  if (o.p[2] < near_plane || o.p[2] > far_plane) return false;
  float R[9];
  quat_to_rotmat(q, R);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o.M[i * 3 + j] = R[i * 3 + j] * s[j];
  // A = Rv * M  (3x3);  Sc = A A^T
  float A[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      A[i * 3 + j] = Rv[i * 3 + 0] * o.M[0 * 3 + j] + Rv[i * 3 + 1] * o.M[1 * 3 + j] + Rv[i * 3 + 2] * o.M[2 * 3 + j];
  o.Sc[0] = A[0] * A[0] + A[1] * A[1] + A[2] * A[2];
  o.Sc[1] = A[0] * A[3] + A[1] * A[4] + A[2] * A[5];
  o.Sc[2] = A[0] * A[6] + A[1] * A[7] + A[2] * A[8];
  o.Sc[3] = A[3] * A[3] + A[4] * A[4] + A[5] * A[5];
  o.Sc[4] = A[3] * A[6] + A[4] * A[7] + A[5] * A[8];
  o.Sc[5] = A[6] * A[6] + A[7] * A[7] + A[8] * A[8];
  // cov2d = J Sc J^T, J = [[sx,0,0],[0,sy,0]]
  const float sx = cam.fx, sy = cam.fy;
  float c00 = sx * sx * o.Sc[0];
  float c01 = sx * sy * o.Sc[1];
  float c11 = sy * sy * o.Sc[3];
  o.c00 = c00 + eps2d;
  o.c11 = c11 + eps2d;
  o.c01 = c01;
  o.det = o.c00 * o.c11 - o.c01 * o.c01;
  o.det_orig = c00 * c11 - c01 * c01;  // from the un-blurred entries, as project_mid
  return o.det > 0.f;
}

// Forward of one (camera, Gaussian).  *compensation (optional) receives the Mip-Splatting opacity factor, 0 for a culled
// pair.  Radius, radius_clip, the off-screen tests and the conic are project_fwd's.
CLMGS_HD Proj project_fwd_ortho(const Cam& cam, const float m[3], const float q[4], const float s[3],
                                float W, float H, float eps2d, float near_plane, float far_plane,
                                float radius_clip, float* compensation = nullptr) {
  Proj r;
  r.radius = 0; r.mx = r.my = r.depth = r.ca = r.cb = r.cc = 0.f;
  if (compensation) *compensation = 0.f;
  OrthoMid o;
  if (!ortho_mid(cam, m, q, s, eps2d, near_plane, far_plane, o)) return r;
  float mx = cam.fx * o.p[0] + cam.cx;
  float my = cam.fy * o.p[1] + cam.cy;
  float b = 0.5f * (o.c00 + o.c11);
  float v1 = b + sqrtf(fmaxf(0.01f, b * b - o.det));
  float radius = ceilf(3.f * sqrtf(v1));
  if (radius <= radius_clip) return r;
  if (mx + radius <= 0.f || mx - radius >= W || my + radius <= 0.f || my - radius >= H) return r;
  float idet = 1.f / o.det;
  r.radius = (int)radius;
  r.mx = mx; r.my = my; r.depth = o.p[2];
  r.ca = o.c11 * idet; r.cb = -o.c01 * idet; r.cc = o.c00 * idet;
  if (compensation) *compensation = sqrtf(fmaxf(0.f, o.det_orig / o.det));
  return r;
}

// VJP of project_fwd_ortho for one (camera, Gaussian); caller guarantees radius > 0.
// v_m / v_q / v_s are OVERWRITTEN with this camera's contribution.  v_compensation enters in gsplat's guarded form
// (the square root's derivative is 0.5 / (compensation + 1e-6)), as project_bwd<true>; 0 adds exact zeros.
CLMGS_HD void project_bwd_ortho(const Cam& cam, const float m[3], const float q[4], const float s[3], float eps2d,
                                const float v_mean2d[2], float v_depth, const float v_conic[3], float v_compensation,
                                float v_m[3], float v_q[4], float v_s[3]) {
  OrthoMid o;
  ortho_mid(cam, m, q, s, eps2d, -1e30f, 1e30f, o);
  float idet = 1.f / o.det;
  float a = o.c11 * idet, b = -o.c01 * idet, c = o.c00 * idet;  // conic
  // v_cov2d = -inv * V * inv, V = [[va, vb/2],[vb/2, vc]]
  float va = v_conic[0], vb = 0.5f * v_conic[1], vc = v_conic[2];
  float t00 = va * a + vb * b, t01 = va * b + vb * c;
  float t10 = vb * a + vc * b, t11 = vb * b + vc * c;
  float g00 = -(a * t00 + b * t10);
  float g01 = -(a * t01 + b * t11);
  float g10 = -(b * t00 + c * t10);
  float g11 = -(b * t01 + c * t11);
  float G00 = g00, G11 = g11, G01 = 0.5f * (g01 + g10);
  {  // d comp^2 / d cov2d = (1 - comp^2) conic - eps2d / det * I
    const float comp = sqrtf(fmaxf(0.f, o.det_orig / o.det));
    const float k = v_compensation * 0.5f / (comp + 1e-6f), w = 1.f - comp * comp;
    G00 += k * (w * a - eps2d * idet);
    G11 += k * (w * c - eps2d * idet);
    G01 += k * w * b;
  }
  const float sx = cam.fx, sy = cam.fy;
  // v_Sc = J^T G J: four non-zero entries
  float vS[9] = {sx * sx * G00, sx * sy * G01, 0.f, sx * sy * G01, sy * sy * G11, 0.f, 0.f, 0.f, 0.f};
  float vp[3] = {sx * v_mean2d[0], sy * v_mean2d[1], v_depth};
  const float* Rv = cam.R;
  // v_m = Rv^T vp
  v_m[0] = Rv[0] * vp[0] + Rv[3] * vp[1] + Rv[6] * vp[2];
  v_m[1] = Rv[1] * vp[0] + Rv[4] * vp[1] + Rv[7] * vp[2];
  v_m[2] = Rv[2] * vp[0] + Rv[5] * vp[1] + Rv[8] * vp[2];
  // v_Sigma(world) = Rv^T vS Rv
  float tmp[9], vW[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      tmp[i * 3 + j] = vS[i * 3 + 0] * Rv[0 * 3 + j] + vS[i * 3 + 1] * Rv[1 * 3 + j] + vS[i * 3 + 2] * Rv[2 * 3 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      vW[i * 3 + j] = Rv[0 * 3 + i] * tmp[0 * 3 + j] + Rv[1 * 3 + i] * tmp[1 * 3 + j] + Rv[2 * 3 + i] * tmp[2 * 3 + j];
  // Sigma = M M^T -> v_M = 2 vW M (vW symmetric)
  float vM[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      vM[i * 3 + j] = 2.f * (vW[i * 3 + 0] * o.M[0 * 3 + j] + vW[i * 3 + 1] * o.M[1 * 3 + j] + vW[i * 3 + 2] * o.M[2 * 3 + j]);
  // M = R diag(s)
  float R[9];
  quat_to_rotmat(q, R);
  float vR[9];
  for (int j = 0; j < 3; ++j) {
    v_s[j] = R[0 * 3 + j] * vM[0 * 3 + j] + R[1 * 3 + j] * vM[1 * 3 + j] + R[2 * 3 + j] * vM[2 * 3 + j];
    for (int i = 0; i < 3; ++i) vR[i * 3 + j] = vM[i * 3 + j] * s[j];
  }
  quat_to_rotmat_vjp(q, vR, v_q);
}

}  // namespace clmgs
