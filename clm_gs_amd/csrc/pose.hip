// Camera-pose gradient of the fused front end (gfx950): for the rows of one visibility filter and the cotangent
// lines the rasterize backward left, the 15 sums
//   v_R[9] = sum_i (vp_i m_i^T + 2 vS_i Rv Sigma_i),  v_t[3] = sum_i vp_i,  v_campos[3] = -sum_i vd_i
// over the rows with radius > 0 (pose_math.h; vd_i is the direction cotangent of the SH VJP, clamp mask applied).
// v_R | v_t are gsplat's v_viewmats[:3, :4] of fully_fused_projection(viewmats_requires_grad=True); v_campos is what
// gsplat gets by autograd through dirs = means - camtoworlds[:3, 3].
//
// A kernel of its own, launched only for a camera that asks for it: preprocess_bwd_kernel (preprocess.hip) sits at its
// register limit and is not touched.  It has that kernel's shape -- a wavefront owns 64-row chunks, unconditional
// gathers with dead rows redirected, camera constants laundered into SGPRs, SH rows staged through wave-private LDS --
// reads what that kernel reads (minus every read-modify-write target) and writes 16 floats per workgroup: each lane
// keeps its 15 sums in registers across its chunks, the wave adds them once at the end.  No atomics, no scratch;
// clmgs_pose_grad_finish adds the workgroups' rows in ascending order, once: the same inputs give the same bits.
#include <stdlib.h>

#include "common.h"
#include "pose_math.h"
#include "rowsum.h"

namespace clmgs {

constexpr int POSE_ROWS = 64;        // rows per chunk = lanes per wavefront = threads per workgroup
constexpr int POSE_PITCH = 52;       // floats per LDS row (see sh.hip)
constexpr int POSE_GRID_CAP = 3072;  // the front end's 256 * 12: above 196 608 rows a wave runs a second chunk
constexpr int VM_THREADS = 256;      // operator form: one thread per Gaussian, four waves per workgroup
constexpr int VM_GRID_CAP = 1024;

struct PoseArgs {
  const int64_t* filter;     // [V] row ids, or NULL (identity)
  const float* xyz;          // [N,3], or the [N,12] packed table
  const float* opacity_raw;  // [N]
  const float* scaling_raw;  // [N,3]
  const float* rotation_raw; // [N,4]
  const float* sh_rows;      // [N,48] by row id, or [V,48] by position (sh_by_filter = 0); not read at degree 0
  int sh_by_filter;
  const int32_t* sh_index;   // != NULL: SH row of position i is sh_rows[sh_index[i]]
  float viewmat[16];
  float K[9];
  float campos[3];
  int width, height;
  float eps2d;
  const float4* packed_grad;  // [V,16] cotangent lines, or
  const float4* partials;     // one line per (row, tile) intersection with
  const int64_t* row_cum;     // row i owning lines [row_cum[i-1], row_cum[i])
};

#define POSE_FOR12(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11)
#define POSE_DECL_ST(j) float4 st##j = make_float4(0.f, 0.f, 0.f, 0.f);
// (row, piece) of staging element j of this lane, from a laundered lane id (see preprocess.hip: keeps the index math
// of the 12 elements out of long-lived registers)
#define POSE_ELEM(j) const int e = tl + POSE_ROWS * j, r = e / NF4, k = e - r * NF4;
#define POSE_LAUNDER_LANE int tl = t; asm volatile("" : "+v"(tl));

struct PoseSmallRow { float m[3]; float4 q4; float s[3]; float oraw; };

template <bool PK>
__device__ __forceinline__ PoseSmallRow pose_load_small(const PoseArgs& a, int64_t g) {
  PoseSmallRow r;
  if (PK) {
    const float4* row = reinterpret_cast<const float4*>(a.xyz) + 3 * g;
    const float4 r0 = row[0], r1 = row[1], r2 = row[2];
    r.m[0] = r0.x; r.m[1] = r0.y; r.m[2] = r0.z; r.oraw = r0.w;
    r.s[0] = r1.x; r.s[1] = r1.y; r.s[2] = r1.z;
    r.q4 = make_float4(r1.w, r2.x, r2.y, r2.z);
  } else {
    r.m[0] = a.xyz[3 * g]; r.m[1] = a.xyz[3 * g + 1]; r.m[2] = a.xyz[3 * g + 2];
    r.q4 = *reinterpret_cast<const float4*>(a.rotation_raw + 4 * g);
    r.s[0] = a.scaling_raw[3 * g]; r.s[1] = a.scaling_raw[3 * g + 1]; r.s[2] = a.scaling_raw[3 * g + 2];
    r.oraw = a.opacity_raw[g];
  }
  return r;
}

// Camera constants live in SGPRs; laundering the copies inside the chunk loop keeps the camera-derived subexpressions
// of the projection loop-variant instead of hoisted into long-lived VGPRs (preprocess.hip, launder_cam).
__device__ __forceinline__ Cam pose_launder_cam(const Cam& c) {
  Cam r = c;
#pragma unroll
  for (int i = 0; i < 9; ++i) asm volatile("" : "+s"(r.R[i]));
#pragma unroll
  for (int i = 0; i < 3; ++i) asm volatile("" : "+s"(r.t[i]));
  asm volatile("" : "+s"(r.fx)); asm volatile("" : "+s"(r.fy));
  asm volatile("" : "+s"(r.cx)); asm volatile("" : "+s"(r.cy));
  return r;
}

// LDS hand-over between the lanes of one wavefront (no s_waitcnt, gathers stay in flight)
__device__ __forceinline__ void pose_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float pose_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }

// out[gridDim.x][16]: v_R 0..8 | v_t 9..11 | v_campos 12..14 | 0.  Every workgroup stores its row.
template <int DEG, bool PK, bool AA>
__global__ void __launch_bounds__(POSE_ROWS, 2)
pose_grad_kernel(int V, PoseArgs a, const int32_t* __restrict__ radii, float* __restrict__ out) {
  constexpr int NB = (DEG + 1) * (DEG + 1);
  constexpr int NF4 = (NB * 3 + 3) / 4;
  __shared__ __attribute__((aligned(16))) float lds[DEG > 0 ? POSE_ROWS * POSE_PITCH : 4];
  const Cam cam = load_cam(a.viewmat, a.K);
  const int n_chunks = (V + POSE_ROWS - 1) / POSE_ROWS;
  const int t = threadIdx.x;
  int chunk = blockIdx.x;
  int my_row = -1, my_radius = 0, my_sh = 0;
  int64_t my_s0 = 0;
  int my_cnt = 0;
  if (chunk < n_chunks && chunk * POSE_ROWS + t < V) {
    const int i = chunk * POSE_ROWS + t;
    my_row = a.filter ? (int)a.filter[i] : i;
    my_sh = a.sh_index ? a.sh_index[i] : my_row;
    my_radius = radii[i];
    if (a.partials) { my_s0 = i ? a.row_cum[i - 1] : 0; my_cnt = (int)(a.row_cum[i] - my_s0); }
  }
  float acc[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) acc[k] = 0.f;
  for (; chunk < n_chunks; chunk += gridDim.x) {
    const int base = chunk * POSE_ROWS;
    const int radius = my_radius;
    const int64_t s0 = my_s0;
    const int cnt = my_cnt;
    const bool mine = my_row >= 0;
    const bool vis = mine && radius > 0;
    const unsigned long long live = __ballot(vis);
    const int first = live ? (int)__builtin_ctzll(live) : 0;
    // dead lanes redirect every gather to the chunk's first live row: no branches, cache hits
    const int64_t g = mine ? my_row : 0;
    const int sh_id = mine ? my_sh : 0;
    const int64_t gl = vis ? g : (int64_t)__shfl((int)g, first);
    const int i = mine ? base + t : base;
    // ---- everything this lane needs from HBM, requested at once
    float4 ga, gb;  // line: x y ca cb | cc r g b | o
    float go;
    float4 pa[4], pb[4];
    float po[4];
    if (a.partials) {  // kernel-uniform: the row's first four partial lines now, longer ranges below
      ga = make_float4(0.f, 0.f, 0.f, 0.f); gb = ga; go = 0.f;
      const float4* src = a.partials + PART_F4 * (size_t)s0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pa[u] = ga; pb[u] = ga; po[u] = 0.f;
        if (mine && u < cnt) { pa[u] = src[PART_F4 * u]; pb[u] = src[PART_F4 * u + 1]; po[u] = src[PART_F4 * u + 2].x; }
      }
    } else {
      ga = a.packed_grad[4 * (size_t)i];
      gb = a.packed_grad[4 * (size_t)i + 1];
      go = a.packed_grad[4 * (size_t)i + 2].x;
    }
    const PoseSmallRow sr = pose_load_small<PK>(a, gl);
    const float m[3] = {sr.m[0], sr.m[1], sr.m[2]};
    {  // row id, radius and line range of this wave's next chunk
      const int ni = (chunk + (int)gridDim.x) * POSE_ROWS + t;
      my_row = -1; my_radius = 0; my_s0 = 0; my_cnt = 0;
      if (ni < V) {
        my_row = a.filter ? (int)a.filter[ni] : ni; my_radius = radii[ni];
        my_sh = a.sh_index ? a.sh_index[ni] : my_row;
        if (a.partials) { my_s0 = ni ? a.row_cum[ni - 1] : 0; my_cnt = (int)(a.row_cum[ni] - my_s0); }
      }
    }
    if (a.partials) {  // ascending slot order, exactly as preprocess_bwd_kernel sums the lines
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // lines beyond cnt were loaded as zeros
        ga.x += pa[u].x; ga.y += pa[u].y; ga.z += pa[u].z; ga.w += pa[u].w;
        gb.x += pb[u].x; gb.y += pb[u].y; gb.z += pb[u].z; gb.w += pb[u].w;
        go += po[u];
      }
      if (mine) {
        const float4* src = a.partials + PART_F4 * (size_t)s0;
        for (int tt = 4; tt < cnt; tt += 4) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int l = min(tt + u, cnt - 1);
            pa[u] = src[PART_F4 * l]; pb[u] = src[PART_F4 * l + 1]; po[u] = src[PART_F4 * l + 2].x;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (tt + u < cnt) {
              ga.x += pa[u].x; ga.y += pa[u].y; ga.z += pa[u].z; ga.w += pa[u].w;
              gb.x += pb[u].x; gb.y += pb[u].y; gb.z += pb[u].z; gb.w += pb[u].w;
              go += po[u];
            }
          }
        }
      }
    }
    if (!live) continue;  // wave-uniform: nothing of this chunk reached the screen
    // ---- projection VJP (while, at degree > 0, nothing else is in flight: the SH rows are requested after it, as
    // in preprocess_bwd_kernel, so that their 12 staging registers are not live across the projection)
    if (vis) {
      const float q[4] = {sr.q4.x, sr.q4.y, sr.q4.z, sr.q4.w};
      const float se[3] = {__expf(sr.s[0]), __expf(sr.s[1]), __expf(sr.s[2])};
      const float v_m2[2] = {ga.x, ga.y};
      const float v_con[3] = {ga.z, ga.w, gb.x};
      const Cam camL = pose_launder_cam(cam);
      float vt[3], vR[9];
      const float vk = AA ? go * pose_sigmoid(sr.oraw) : 0.f;  // v_compensation = go * op
      project_pose_vjp<AA>(camL, m, q, se, (float)a.width, (float)a.height, a.eps2d, v_m2, 0.f, v_con, vk, vt, vR);
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[k] += vR[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[9 + k] += vt[k];
    }
    if constexpr (DEG > 0) {
      // ---- SH rows -> wave-private LDS; every lane then reads its own row
      POSE_FOR12(POSE_DECL_ST)
#define POSE_LOAD_SH(j)                                                                             \
  if constexpr (j < NF4) {                                                                          \
    POSE_ELEM(j)                                                                                    \
    const int rr = ((live >> r) & 1ull) ? r : first;                                                \
    const int64_t src = a.sh_by_filter ? (int64_t)__shfl(sh_id, rr) : (int64_t)(base + rr);         \
    st##j = *reinterpret_cast<const float4*>(a.sh_rows + src * 48 + 4 * k);                         \
  }
      { POSE_LAUNDER_LANE POSE_FOR12(POSE_LOAD_SH) }
#undef POSE_LOAD_SH
      pose_wave_lds_sync();  // the previous chunk's LDS rows are consumed
#define POSE_X(j)                                                                                   \
  if constexpr (j < NF4) {                                                                          \
    POSE_ELEM(j)                                                                                    \
    *reinterpret_cast<float4*>(lds + r * POSE_PITCH + 4 * k) = st##j;                               \
  }
      { POSE_LAUNDER_LANE POSE_FOR12(POSE_X) }
#undef POSE_X
      pose_wave_lds_sync();
      if (vis) {
        const float* row = lds + t * POSE_PITCH;
        const float dx = m[0] - a.campos[0], dy = m[1] - a.campos[1], dz = m[2] - a.campos[2];
        const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
        const float x = dx * inv, y = dy * inv, z = dz * inv;
        float B[16], Bx[16], By[16], Bz[16];
        sh_basis(DEG, x, y, z, B);
        sh_basis_grad(DEG, x, y, z, Bx, By, Bz);
        // one pass over the row: colour P_c (for the clamp mask) and the un-clamped direction cotangent U_c
        float P[3] = {0.f, 0.f, 0.f};
        float U[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const float rk[3] = {row[3 * k], row[3 * k + 1], row[3 * k + 2]};
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            P[c] += B[k] * rk[c];
            if (k > 0) { U[c][0] += rk[c] * Bx[k]; U[c][1] += rk[c] * By[k]; U[c][2] += rk[c] * Bz[k]; }
          }
        }
        const float vc[3] = {(P[0] + 0.5f > 0.f) ? gb.y : 0.f, (P[1] + 0.5f > 0.f) ? gb.z : 0.f,
                             (P[2] + 0.5f > 0.f) ? gb.w : 0.f};
        const float ux = vc[0] * U[0][0] + vc[1] * U[1][0] + vc[2] * U[2][0];
        const float uy = vc[0] * U[0][1] + vc[1] * U[1][1] + vc[2] * U[2][1];
        const float uz = vc[0] * U[0][2] + vc[1] * U[1][2] + vc[2] * U[2][2];
        const float dot = ux * x + uy * y + uz * z;
        acc[12] -= (ux - dot * x) * inv;
        acc[13] -= (uy - dot * y) * inv;
        acc[14] -= (uz - dot * z) * inv;
      }
    }
  }
  // ---- the wave's 15 sums, once; lane k stores sum k (lane 15: the pad word)
  float mine_out = 0.f;
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    const float s = wave_sum(acc[k]);
    if (t == k) mine_out = s;
  }
  if (t < 16) out[(size_t)blockIdx.x * 16 + t] = mine_out;
}

// Operator form: v_viewmats of fully_fused_projection.  Thread n walks the Gaussians n, n + stride, ... of camera
// blockIdx.y and keeps its 12 sums in registers; the four waves of the workgroup are joined through LDS in wave order
// and the workgroup stores one row: partials[(c * gridDim.x + blockIdx.x)][16], rows 0..2 of the 4x4 (v_R[i] | v_t[i]) | 0.
template <bool AA>
__global__ void __launch_bounds__(VM_THREADS)
projection_viewmat_bwd_kernel(int N, const float* __restrict__ means, const float* __restrict__ quats,
                              const float* __restrict__ scales, const float* __restrict__ viewmats,
                              const float* __restrict__ Ks, float W, float H, float eps2d,
                              const int32_t* __restrict__ radii, const float* __restrict__ v_means2d,
                              const float* __restrict__ v_depths, const float* __restrict__ v_conics,
                              const float* __restrict__ v_compensations, float* __restrict__ partials) {
  __shared__ float red[VM_THREADS / 64][12];
  const int c = blockIdx.y;
  const Cam cam = load_cam(viewmats + 16 * c, Ks + 9 * c);
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  for (int n = blockIdx.x * VM_THREADS + threadIdx.x; n < N; n += gridDim.x * VM_THREADS) {
    const size_t o = (size_t)c * N + n;
    if (radii[o] <= 0) continue;
    const float m[3] = {means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2]};
    const float4 q4 = *reinterpret_cast<const float4*>(quats + 4 * (size_t)n);
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    const float s[3] = {scales[3 * (size_t)n], scales[3 * (size_t)n + 1], scales[3 * (size_t)n + 2]};
    const float vm2[2] = {v_means2d[2 * o], v_means2d[2 * o + 1]};
    const float vc[3] = {v_conics[3 * o], v_conics[3 * o + 1], v_conics[3 * o + 2]};
    const float vd = v_depths ? v_depths[o] : 0.f;
    const float vk = (AA && v_compensations) ? v_compensations[o] : 0.f;
    float vt[3], vR[9];
    project_pose_vjp<AA>(cam, m, q, s, W, H, eps2d, vm2, vd, vc, vk, vt, vR);
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // the layout of the 4x4: row i = v_R[i][0..2] | v_t[i]
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[4 * i + j] += vR[3 * i + j];
      acc[4 * i + 3] += vt[i];
    }
  }
  const float s = workgroup_row<VM_THREADS / 64, 12>(acc, red);  // rowsum.h; threads 12..15 hold 0.f: the pad words
  if (threadIdx.x < 16) partials[((size_t)c * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = s;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_pose_grad_partials_rows(int V) {
  if (V < 1) return 0;
  return min(ceil_div(V, POSE_ROWS), POSE_GRID_CAP);
}

extern "C" int clmgs_pose_grad(void* stream, int V, const int64_t* filter, const float* xyz, const float* opacity_raw,
                               const float* scaling_raw, const float* rotation_raw, const float* sh_rows,
                               int sh_by_filter, const float* viewmat_host, const float* K_host,
                               const float* campos_host, int width, int height, int degree, float eps2d,
                               const int32_t* radii, const void* packed_grad, const void* partials,
                               const int64_t* row_cum, const int32_t* sh_index, int antialiased,
                               float* partials_out) {
  CLMGS_CHECK_ARG(V >= 0 && degree >= 0 && degree <= 3 && width > 0 && height > 0);  // row ids are int32 in flight
  if (V == 0) return 0;
  CLMGS_CHECK_ARG(xyz && (sh_rows || degree == 0) && viewmat_host && K_host && campos_host && radii && partials_out);
  // exactly one source of the per-row raster gradient: the [V,16] table, or the partial lines + ranges
  CLMGS_CHECK_ARG((packed_grad != nullptr) != (partials != nullptr));
  CLMGS_CHECK_ARG(!partials || (row_cum && (((uintptr_t)partials & 15) == 0)));
  CLMGS_CHECK_ARG(!packed_grad || (((uintptr_t)packed_grad & 15) == 0));
  CLMGS_CHECK_ARG((opacity_raw && scaling_raw && rotation_raw) ||
                  (!opacity_raw && !scaling_raw && !rotation_raw && (((uintptr_t)xyz & 15) == 0)));
  CLMGS_CHECK_ARG(!sh_index || sh_by_filter);
  CLMGS_CHECK_ARG(((uintptr_t)sh_rows & 15) == 0);
  const bool pk = !opacity_raw && !scaling_raw && !rotation_raw;
  PoseArgs a;
  a.filter = filter; a.xyz = xyz; a.opacity_raw = opacity_raw; a.scaling_raw = scaling_raw;
  a.rotation_raw = rotation_raw; a.sh_rows = sh_rows; a.sh_by_filter = sh_by_filter; a.sh_index = sh_index;
  for (int i = 0; i < 16; ++i) a.viewmat[i] = viewmat_host[i];
  for (int i = 0; i < 9; ++i) a.K[i] = K_host[i];
  for (int i = 0; i < 3; ++i) a.campos[i] = campos_host[i];
  a.width = width; a.height = height; a.eps2d = eps2d;
  a.packed_grad = (const float4*)packed_grad; a.partials = (const float4*)partials; a.row_cum = row_cum;
  const int grid = clmgs_pose_grad_partials_rows(V);
#define CLMGS_POSE_K(D, PKD, A)                                                                    \
  hipLaunchKernelGGL((pose_grad_kernel<D, PKD, A>), dim3(grid), dim3(POSE_ROWS), 0, (hipStream_t)stream, V, a, radii, \
                     partials_out)
#define CLMGS_POSE(D)                                                                              \
  do {                                                                                             \
    if (antialiased) { if (pk) CLMGS_POSE_K(D, true, true); else CLMGS_POSE_K(D, false, true); }   \
    else if (pk) CLMGS_POSE_K(D, true, false);                                                     \
    else CLMGS_POSE_K(D, false, false);                                                            \
  } while (0)
  switch (degree) {
    case 0: CLMGS_POSE(0); break;
    case 1: CLMGS_POSE(1); break;
    case 2: CLMGS_POSE(2); break;
    default: CLMGS_POSE(3); break;
  }
#undef CLMGS_POSE
#undef CLMGS_POSE_K
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_pose_grad_finish(void* stream, int rows, const float* partials, float* grad15) {
  CLMGS_CHECK_ARG(rows >= 0 && (partials || rows == 0) && grad15);
  if (rows == 0) return 0;
  hipLaunchKernelGGL((rows_finish_kernel<16, 16, true>), dim3(1), dim3(64), 0, (hipStream_t)stream, rows, partials, grad15, 15);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_projection_viewmat_partials_rows(int N) {
  if (N < 1) return 0;
  return min(ceil_div(N, VM_THREADS), VM_GRID_CAP);
}

extern "C" int clmgs_projection_viewmat_bwd(void* stream, int C, int N, const float* means, const float* quats,
                                            const float* scales, const float* viewmats, const float* Ks, int width,
                                            int height, float eps2d, const int32_t* radii, const float* v_means2d,
                                            const float* v_depths, const float* v_conics,
                                            const float* v_compensations, float* partials, float* v_viewmats) {
  CLMGS_CHECK_ARG(C >= 1 && N >= 0 && width > 0 && height > 0 && v_viewmats);
  const int rows = clmgs_projection_viewmat_partials_rows(N);
  if (N > 0) {
    CLMGS_CHECK_ARG(means && quats && scales && viewmats && Ks && radii && v_means2d && v_conics && partials);
    const dim3 grid(rows, C);
    if (v_compensations)
      hipLaunchKernelGGL(projection_viewmat_bwd_kernel<true>, grid, dim3(VM_THREADS), 0, (hipStream_t)stream, N, means,
                         quats, scales, viewmats, Ks, (float)width, (float)height, eps2d, radii, v_means2d, v_depths,
                         v_conics, v_compensations, partials);
    else
      hipLaunchKernelGGL(projection_viewmat_bwd_kernel<false>, grid, dim3(VM_THREADS), 0, (hipStream_t)stream, N, means,
                         quats, scales, viewmats, Ks, (float)width, (float)height, eps2d, radii, v_means2d, v_depths,
                         v_conics, v_compensations, partials);
    CLMGS_LAUNCH_CHECK();
  }
  // rows == 0: nothing is read, every camera's 16 words are stored as zeros
  hipLaunchKernelGGL((rows_finish_kernel<16, 16, false>), dim3(C), dim3(64), 0, (hipStream_t)stream, rows, partials, v_viewmats, 12);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
