// Host build of clm_gs_amd/csrc/mesh_distance_math.h for tests/test_mesh_eval_cpu.py (plain g++, no HIP).
#include "mesh_distance_math.h"

using namespace clmgs;

// n independent evaluations; p, a, b, c are [n,3]
extern "C" void shim_closest_d2(int n, const double* p, const double* a, const double* b, const double* c, double* out) {
  for (int i = 0; i < n; ++i) out[i] = md_closest_d2(p + 3 * i, a + 3 * i, b + 3 * i, c + 3 * i);
}

extern "C" void shim_point_d2(int n, const double* p, const double* a, double* out) {
  for (int i = 0; i < n; ++i) out[i] = md_point_d2(p + 3 * i, a + 3 * i);
}

extern "C" void shim_face_area(int n, const double* a, const double* b, const double* c, double spacing, double* area,
                               unsigned char* ok, int64_t* count) {
  for (int i = 0; i < n; ++i) {
    area[i] = md_face_area(a + 3 * i, b + 3 * i, c + 3 * i);
    ok[i] = md_area_ok(area[i]) ? 1 : 0;
    count[i] = md_sample_count(area[i], spacing);
  }
}

// sample k[i] of triangle i -> uv [n,2], out [n,3]
extern "C" void shim_sample_position(int n, const int64_t* k, const double* a, const double* b, const double* c, double* uv,
                                     float* out) {
  for (int i = 0; i < n; ++i) {
    md_sample_uv(k[i], uv + 2 * i, uv + 2 * i + 1);
    md_sample_position(k[i], a + 3 * i, b + 3 * i, c + 3 * i, out + 3 * i);
  }
}

extern "C" void shim_cell(int n, const double* x, double o, double h, int g, int* out) {
  for (int i = 0; i < n; ++i) out[i] = md_cell(x[i], o, h, g);
}
