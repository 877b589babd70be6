// g++ -O1 -g -I clm_gs_amd/csrc tests/host_shim/pose_math_host.cpp -o pose_math_host [-fsanitize=address,undefined]
// Stand-alone host check of clm_gs_amd/csrc/pose_math.h: project_pose_vjp (float, the product's code) against central
// differences of a double restatement of the projection, for the twelve entries of [Rv | t].  The scalar is
//   f = <v_mean2d, mean2d> + v_depth * depth + <v_conic, conic> [+ v_compensation * compensation].
// Prints the largest error relative to the gradient's largest entry per case; exit status 1 above 2e-3 (float
// evaluation of the VJP; the differences are exact to ~1e-9).
#include <stdio.h>
#include <stdlib.h>

#include "pose_math.h"

using namespace clmgs;

struct Case { float m[3], q[4], s[3], vm2[2], vd, vc[3], vk; bool aa; };

static double forward(const double Rv[9], const double t[3], const double K[4], const Case& c, double W, double H,
                      double eps2d) {
  double n = 0;
  for (int i = 0; i < 4; ++i) n += (double)c.q[i] * c.q[i];
  n = sqrt(n);
  const double w = c.q[0] / n, x = c.q[1] / n, y = c.q[2] / n, z = c.q[3] / n;
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  double A[9], Sc[9], p[3];
  for (int i = 0; i < 3; ++i) {
    p[i] = t[i];
    for (int j = 0; j < 3; ++j) p[i] += Rv[3 * i + j] * c.m[j];
    for (int j = 0; j < 3; ++j) {
      A[3 * i + j] = 0;
      for (int k = 0; k < 3; ++k) A[3 * i + j] += Rv[3 * i + k] * R[3 * k + j] * c.s[j];
    }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      Sc[3 * i + j] = 0;
      for (int k = 0; k < 3; ++k) Sc[3 * i + j] += A[3 * i + k] * A[3 * j + k];
    }
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const double lxp = (W - cx) / fx + 0.15 * W / fx, lxn = cx / fx + 0.15 * W / fx;
  const double lyp = (H - cy) / fy + 0.15 * H / fy, lyn = cy / fy + 0.15 * H / fy;
  const double rz = 1 / p[2];
  const double tx = p[2] * fmin(lxp, fmax(-lxn, p[0] * rz)), ty = p[2] * fmin(lyp, fmax(-lyn, p[1] * rz));
  const double J[6] = {fx * rz, 0, -fx * tx * rz * rz, 0, fy * rz, -fy * ty * rz * rz};
  double JS[6], c2[4];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 3; ++j) {
      JS[3 * i + j] = 0;
      for (int k = 0; k < 3; ++k) JS[3 * i + j] += J[3 * i + k] * Sc[3 * k + j];
    }
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      c2[2 * i + j] = 0;
      for (int k = 0; k < 3; ++k) c2[2 * i + j] += JS[3 * i + k] * J[3 * j + k];
    }
  const double det0 = c2[0] * c2[3] - c2[1] * c2[1];
  const double c00 = c2[0] + eps2d, c11 = c2[3] + eps2d, c01 = c2[1];
  const double det = c00 * c11 - c01 * c01;
  double f = c.vm2[0] * (fx * p[0] * rz + cx) + c.vm2[1] * (fy * p[1] * rz + cy) + c.vd * p[2];
  f += (c.vc[0] * c11 - c.vc[1] * c01 + c.vc[2] * c00) / det;
  if (c.aa) f += c.vk * sqrt(fmax(0.0, det0 / det));
  return f;
}

static float frand() { return (float)rand() / (float)RAND_MAX * 2.f - 1.f; }

int main() {
  srand(7);
  const float W = 64.f, H = 48.f, eps2d = 0.3f;
  const float Kf[9] = {57.6f, 0.f, 32.f, 0.f, 57.6f, 24.f, 0.f, 0.f, 1.f};
  const double Kd[4] = {57.6f, 57.6f, 32.f, 24.f};
  const float ang = 0.2f;
  const float vmf[16] = {cosf(ang), 0.f, sinf(ang), 0.1f, 0.f, 1.f, 0.f, -0.05f, -sinf(ang), 0.f, cosf(ang), 0.3f,
                         0.f, 0.f, 0.f, 1.f};
  const Cam cam = load_cam(vmf, Kf);
  double worst = 0;
  int n_clamped = 0;
  for (int it = 0; it < 400; ++it) {
    Case c;
    // every eighth case far off axis: tx (or ty) is clamped
    const bool far = (it % 8) == 7;
    c.m[0] = far ? (it % 16 == 7 ? 9.f : -9.f) : 1.5f * frand();
    c.m[1] = (far && it % 32 == 31) ? 8.f : 1.5f * frand();
    c.m[2] = 6.f + 1.5f * frand();
    for (int i = 0; i < 4; ++i) c.q[i] = frand();
    for (int i = 0; i < 3; ++i) c.s[i] = expf(-1.5f + 0.4f * frand());
    c.vm2[0] = frand(); c.vm2[1] = frand(); c.vd = frand();
    for (int i = 0; i < 3; ++i) c.vc[i] = frand();
    c.vk = frand();
    c.aa = (it & 1) != 0;
    ProjMid mid;
    project_mid(cam, c.m, c.q, c.s, W, H, eps2d, 0.01f, 1e10f, mid);
    n_clamped += (mid.clamp_x || mid.clamp_y) ? 1 : 0;
    float vt[3], vR[9];
    if (c.aa) project_pose_vjp<true>(cam, c.m, c.q, c.s, W, H, eps2d, c.vm2, c.vd, c.vc, c.vk, vt, vR);
    else project_pose_vjp<false>(cam, c.m, c.q, c.s, W, H, eps2d, c.vm2, c.vd, c.vc, 0.f, vt, vR);
    double Rv[9], t[3], num[12], scale = 0;
    for (int i = 0; i < 9; ++i) Rv[i] = cam.R[i];
    for (int i = 0; i < 3; ++i) t[i] = cam.t[i];
    for (int k = 0; k < 12; ++k) {
      double* x = k < 9 ? &Rv[k] : &t[k - 9];
      const double x0 = *x, h = 1e-6;
      *x = x0 + h; const double fp = forward(Rv, t, Kd, c, W, H, eps2d);
      *x = x0 - h; const double fm = forward(Rv, t, Kd, c, W, H, eps2d);
      *x = x0;
      num[k] = (fp - fm) / (2 * h);
      scale = fmax(scale, fabs(num[k]));
    }
    double err = 0;
    for (int k = 0; k < 12; ++k) err = fmax(err, fabs((k < 9 ? vR[k] : vt[k - 9]) - num[k]));
    worst = fmax(worst, err / (scale + 1e-30));
  }
  printf("project_pose_vjp vs central differences: worst relative error %.3e over 400 cases (%d clamped)\n", worst,
         n_clamped);
  if (n_clamped < 10) { printf("too few clamped cases\n"); return 1; }
  return worst < 2e-3 ? 0 : 1;
}
