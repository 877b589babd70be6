// Camera-pose VJP of the EWA projection for one (camera, Gaussian): the cotangents of the world-to-camera
// matrix [Rv | t] that gsplat's fully_fused_projection returns as v_viewmats[:3, :4] (viewmats_requires_grad).
//
// With  p = Rv m + t,  Sc = Rv Sigma Rv^T,  Sigma = M M^T,  M = R(q) diag(s):
//   v_t = vp                                   vp: camera-space mean cotangent
//   v_R = vp m^T + 2 vS Rv Sigma               vS: symmetric camera-space covariance cotangent J^T G J
// vp and vS are the values project_bwd (gs_math.h) forms before it multiplies by Rv^T.  They are restated here on top
// of project_mid instead of being taken from project_bwd: that function is inlined into the front-end kernels, which
// sit at their register limit, and any edit or wrapper changes their instructions (see the note in gs_math.h).
// Compiles with plain g++ (CLMGS_HD empty): tests/pose_math_host.cpp checks it against central differences.
#pragma once
#include "gs_math.h"

namespace clmgs {

// Caller guarantees radius > 0 (the pair passed the forward's culls).  v_t[3] and v_R[9] (row major) are OVERWRITTEN.
// AA: v_compensation is one more cotangent, in gsplat's guarded form (see project_bwd).
template <bool AA = false>
CLMGS_HD void project_pose_vjp(const Cam& cam, const float m[3], const float q[4], const float s[3],
                               float W, float H, float eps2d,
                               const float v_mean2d[2], float v_depth, const float v_conic[3],
                               float v_compensation, float v_t[3], float v_R[9]) {
  ProjMid o;
  project_mid(cam, m, q, s, W, H, eps2d, -1e30f, 1e30f, o);
  const float idet = 1.f / o.det;
  const float a = o.c11 * idet, b = -o.c01 * idet, c = o.c00 * idet;  // conic
  // v_cov2d = -conic V conic, V = [[va, vb/2], [vb/2, vc]], symmetrised
  const float va = v_conic[0], vb = 0.5f * v_conic[1], vc = v_conic[2];
  const float t00 = va * a + vb * b, t01 = va * b + vb * c;
  const float t10 = vb * a + vc * b, t11 = vb * b + vc * c;
  float G00 = -(a * t00 + b * t10);
  float G11 = -(b * t01 + c * t11);
  float G01 = -0.5f * ((a * t01 + b * t11) + (b * t00 + c * t10));
  if (AA) {  // d comp^2 / d cov2d = (1 - comp^2) conic - eps2d / det * I
    const float comp = compensation_of(o);
    const float k = v_compensation * 0.5f / (comp + 1e-6f), w = 1.f - comp * comp;
    G00 += k * (w * a - eps2d * idet);
    G11 += k * (w * c - eps2d * idet);
    G01 += k * w * b;
  }
  const float sxx = o.Sc[0], sxy = o.Sc[1], sxz = o.Sc[2], syy = o.Sc[3], syz = o.Sc[4], szz = o.Sc[5];
  const float J00 = o.J00, J02 = o.J02, J11 = o.J11, J12 = o.J12;
  // vS = J^T G J, J = [[J00, 0, J02], [0, J11, J12]]
  const float gj0 = G00 * J02 + G01 * J12, gj1 = G01 * J02 + G11 * J12;
  float vS[9];
  vS[0] = J00 * G00 * J00;
  vS[1] = J00 * G01 * J11;
  vS[2] = J00 * gj0;
  vS[4] = J11 * G11 * J11;
  vS[5] = J11 * gj1;
  vS[8] = J02 * gj0 + J12 * gj1;
  vS[3] = vS[1]; vS[6] = vS[2]; vS[7] = vS[5];
  // v_J = 2 G J Sc
  const float js00 = J00 * sxx + J02 * sxz, js01 = J00 * sxy + J02 * syz, js02 = J00 * sxz + J02 * szz;
  const float js10 = J11 * sxy + J12 * sxz, js11 = J11 * syy + J12 * syz, js12 = J11 * syz + J12 * szz;
  const float vJ00 = 2.f * (G00 * js00 + G01 * js10);
  const float vJ02 = 2.f * (G00 * js02 + G01 * js12);
  const float vJ11 = 2.f * (G01 * js01 + G11 * js11);
  const float vJ12 = 2.f * (G01 * js02 + G11 * js12);

  const float x = o.p[0], y = o.p[1], z = o.p[2];
  const float rz = 1.f / z, rz2 = rz * rz, rz3 = rz2 * rz;
  float vp0 = cam.fx * rz * v_mean2d[0];
  float vp1 = cam.fy * rz * v_mean2d[1];
  float vp2 = -(cam.fx * x * v_mean2d[0] + cam.fy * y * v_mean2d[1]) * rz2 + v_depth;
  vp2 += -cam.fx * rz2 * vJ00 - cam.fy * rz2 * vJ11;  // J00 = fx / z, J11 = fy / z
  // J02 = -fx tx / z^2;  tx = x (free) or z * lim (clamped)
  if (!o.clamp_x) {
    vp0 += -cam.fx * rz2 * vJ02;
    vp2 += 2.f * cam.fx * o.tx * rz3 * vJ02;
  } else {
    vp2 += cam.fx * o.tx * rz3 * vJ02;
  }
  if (!o.clamp_y) {
    vp1 += -cam.fy * rz2 * vJ12;
    vp2 += 2.f * cam.fy * o.ty * rz3 * vJ12;
  } else {
    vp2 += cam.fy * o.ty * rz3 * vJ12;
  }
  v_t[0] = vp0; v_t[1] = vp1; v_t[2] = vp2;
  // Rv Sigma = (Rv M) M^T
  const float* Rv = cam.R;
  float A[9], RS[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      A[i * 3 + j] = Rv[i * 3 + 0] * o.M[0 * 3 + j] + Rv[i * 3 + 1] * o.M[1 * 3 + j] + Rv[i * 3 + 2] * o.M[2 * 3 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      RS[i * 3 + j] = A[i * 3 + 0] * o.M[j * 3 + 0] + A[i * 3 + 1] * o.M[j * 3 + 1] + A[i * 3 + 2] * o.M[j * 3 + 2];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      v_R[i * 3 + j] = v_t[i] * m[j] +
                       2.f * (vS[i * 3 + 0] * RS[0 * 3 + j] + vS[i * 3 + 1] * RS[1 * 3 + j] + vS[i * 3 + 2] * RS[2 * 3 + j]);
}

}  // namespace clmgs
