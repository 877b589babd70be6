// g++ -O2 -shared -fPIC -I clm_gs_amd/csrc tests/host_shim/ortho_math_shim.cpp -o shim.so
// Exposes the product's per-element orthographic projection (ortho_math.h) to the CPU tests.
#include "ortho_math.h"
using namespace clmgs;

extern "C" {
void shim_project_ortho_fwd(int N, const float* means, const float* quats, const float* scales,
                            const float* viewmat, const float* K, float W, float H, float eps2d, float near_plane,
                            float far_plane, float radius_clip, int* radii, float* means2d, float* depths,
                            float* conics, float* compensations) {
  Cam cam = load_cam(viewmat, K);
  for (int i = 0; i < N; ++i) {
    float comp;
    Proj p = project_fwd_ortho(cam, means + 3 * i, quats + 4 * i, scales + 3 * i, W, H, eps2d,
                               near_plane, far_plane, radius_clip, &comp);
    radii[i] = p.radius;
    means2d[2 * i] = p.mx; means2d[2 * i + 1] = p.my;
    depths[i] = p.depth;
    conics[3 * i] = p.ca; conics[3 * i + 1] = p.cb; conics[3 * i + 2] = p.cc;
    compensations[i] = comp;
  }
}

void shim_project_ortho_bwd(int N, const float* means, const float* quats, const float* scales,
                            const float* viewmat, const float* K, float eps2d, const int* radii,
                            const float* v_means2d, const float* v_depths, const float* v_conics,
                            const float* v_compensations, float* v_means, float* v_quats, float* v_scales) {
  Cam cam = load_cam(viewmat, K);
  for (int i = 0; i < N; ++i) {
    if (radii[i] <= 0) continue;
    project_bwd_ortho(cam, means + 3 * i, quats + 4 * i, scales + 3 * i, eps2d, v_means2d + 2 * i, v_depths[i],
                      v_conics + 3 * i, v_compensations[i], v_means + 3 * i, v_quats + 4 * i, v_scales + 3 * i);
  }
}
}
