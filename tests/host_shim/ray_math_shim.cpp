// Host build of clm_gs_amd/csrc/ray_math.h for tests/test_ray_depth_cpu.py (plain g++, no HIP).
#include "ray_math.h"

using namespace clmgs;

// n independent evaluations: mu [n,3], q [n,4], s [n,3], cam [n,16], px / py [n], centre [n] -> tstar [n], depth [n]
extern "C" void shim_ray_depth(int n, const double* mu, const double* q, const double* s, const double* cam, const double* px,
                               const double* py, int ortho, double near, const float* centre, double* tstar, float* depth) {
  for (int i = 0; i < n; ++i) {
    tstar[i] = ray_tstar(mu + 3 * i, q + 4 * i, s + 3 * i, cam + RAY_CAM_DOUBLES * i, px[i], py[i], ortho);
    depth[i] = ray_depth(mu + 3 * i, q + 4 * i, s + 3 * i, cam + RAY_CAM_DOUBLES * i, px[i], py[i], ortho, near, centre[i]);
  }
}
