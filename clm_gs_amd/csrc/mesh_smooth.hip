// Mesh smoothing and vertex normals ("Mesh smoothing and normals"): one umbrella step of Taubin's
// lambda | mu smoothing, and area-weighted vertex normals, over the vertex -> face incidence lists of a mesh.  The
// arithmetic is csrc/mesh_vertex_math.h; the lists (a stable sort of the 3F corner slots by vertex and a searchsorted) are
// torch (clm_kernels.mesh_incidence).
//
//   order   int64 [3F]: the corner slots e = 3 f + k sorted by the vertex they name, ascending e within a vertex
//   start   int64 [V+1]: the segment of vertex v is order[start[v] .. start[v+1])
//
//   step     ONE LANE PER VERTEX.  It walks its segment and adds, per entry, the two other corners of the face in the
//            face's rotation (float64, left to right), then writes float32(p + c (s / n - p)) to a SECOND buffer: every
//            lane reads the step's input only (Jacobi).  A vertex without entries keeps its bits.
//   normals  ONE LANE PER VERTEX.  Per entry the cross product of the face's edges from its corners in stored order, added
//            to three float64 sums, then normalised; (0, 0, 0) where the sum has no direction.
//
// Why one lane per vertex.  The contract fixes each vertex's sums as a serial left-to-right float64 chain in list order,
// and a vertex of a Surface Nets mesh has about six entries: there is nothing for a part-wave to share.  A lane walks its
// own segment and nothing crosses lanes, so any launch shape gives the same bits.  The vertices of an extracted mesh lie
// in the memory order of the grid and the lists are not re-ordered: neighbouring lanes walk neighbouring segments of
// `order` and gather face rows and vertices a few rows apart, which share cache lines.  The walk is bound by scattered
// requests (per entry 8 B of order, a 12 B face row and two or three 12 B vertices), not by arithmetic; 256 lanes per
// workgroup and a register count far below the 64-per-lane mark keep eight waves per SIMD in flight to hide their latency.
//
// No atomics, no kernel waits for another workgroup.  Every index read from memory is compared (unsigned) with its bound
// before it is used: a slot outside [0, 3F), a face index outside [0, V) or a segment outside the list is skipped, never
// followed.
#include "common.h"
#include "mesh_vertex_math.h"

namespace clmgs {

constexpr int MS_THREADS = 256;
constexpr int MS_MAX_BLOCKS = 16384;  // the kernels stride over the vertices

__device__ __forceinline__ bool ms_in(int x, int n) { return (unsigned)x < (unsigned)n; }

__device__ __forceinline__ void ms_load(const float* __restrict__ verts, int v, double* p) {
  p[0] = (double)verts[(int64_t)v * 3];
  p[1] = (double)verts[(int64_t)v * 3 + 1];
  p[2] = (double)verts[(int64_t)v * 3 + 2];
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_smooth_step_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int F,
                        const int64_t* __restrict__ order, const int64_t* __restrict__ start, double factor, float* out) {
#pragma clang fp contract(off)
  const int64_t E = 3 * (int64_t)F;
  for (int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MS_THREADS) {
    int64_t b = start[v], e = start[v + 1];
    b = b < 0 ? 0 : b;
    e = e > E ? E : e;
    double s[3] = {0.0, 0.0, 0.0};
    int64_t n = 0;
    for (int64_t j = b; j < e; ++j) {
      const int64_t slot = order[j];
      if ((uint64_t)slot >= (uint64_t)E) continue;
      const int64_t f = slot / 3;
      const int k = (int)(slot - 3 * f);
      const int va = faces[f * 3 + (k == 2 ? 0 : k + 1)];
      const int vb = faces[f * 3 + (k == 0 ? 2 : k - 1)];
      if (!(ms_in(va, V) && ms_in(vb, V))) continue;
      double pa[3], pb[3];
      ms_load(verts, va, pa);
      ms_load(verts, vb, pb);
      mv_add_neighbours(pa, pb, s);
      n += 2;
    }
    const float p[3] = {verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]};
    float o[3];
    mv_step(p, s, n, factor, o);
    out[v * 3] = o[0];
    out[v * 3 + 1] = o[1];
    out[v * 3 + 2] = o[2];
  }
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_vertex_normals_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int F,
                           const int64_t* __restrict__ order, const int64_t* __restrict__ start, float* normals) {
#pragma clang fp contract(off)
  const int64_t E = 3 * (int64_t)F;
  for (int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MS_THREADS) {
    int64_t b = start[v], e = start[v + 1];
    b = b < 0 ? 0 : b;
    e = e > E ? E : e;
    double a[3] = {0.0, 0.0, 0.0};
    for (int64_t j = b; j < e; ++j) {
      const int64_t slot = order[j];
      if ((uint64_t)slot >= (uint64_t)E) continue;
      const int64_t f = slot / 3;
      const int v0 = faces[f * 3], v1 = faces[f * 3 + 1], v2 = faces[f * 3 + 2];
      if (!(ms_in(v0, V) && ms_in(v1, V) && ms_in(v2, V))) continue;
      double p0[3], p1[3], p2[3];
      ms_load(verts, v0, p0);
      ms_load(verts, v1, p1);
      ms_load(verts, v2, p2);
      mv_add_face_normal(p0, p1, p2, a);
    }
    float o[3];
    mv_normalise(a, o);
    normals[v * 3] = o[0];
    normals[v * 3 + 1] = o[1];
    normals[v * 3 + 2] = o[2];
  }
}

static bool ms_aligned(const void* p, uintptr_t a) { return p != nullptr && ((uintptr_t)p % a) == 0; }

static bool ms_apart(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + na <= b0 || b0 + nb <= a0;
}

static dim3 ms_grid(int64_t n) { return dim3((unsigned)min((int64_t)MS_MAX_BLOCKS, (n + MS_THREADS - 1) / MS_THREADS)); }

// The checks the two entries share: sizes, pointers, and an output that overlaps no input.
static bool ms_args_ok(int V, int F, const float* verts, const int32_t* faces, const int64_t* order, const int64_t* start,
                       const float* out) {
  if (!(V >= 1 && F >= 1 && (int64_t)F <= (int64_t)0x7fffffff)) return false;
  if (!(ms_aligned(verts, 4) && ms_aligned(faces, 4) && ms_aligned(order, 8) && ms_aligned(start, 8) && ms_aligned(out, 4)))
    return false;
  const uint64_t vb = (uint64_t)V * 12, fb = (uint64_t)F * 12, ob = (uint64_t)F * 24, sb = ((uint64_t)V + 1) * 8;
  return ms_apart(out, vb, verts, vb) && ms_apart(out, vb, faces, fb) && ms_apart(out, vb, order, ob) &&
         ms_apart(out, vb, start, sb);
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_mesh_smooth_step(void* stream, int V, int F, const float* verts_in, const int32_t* faces,
                                      const int64_t* order, const int64_t* start, double factor, float* verts_out) {
  CLMGS_CHECK_ARG(ms_args_ok(V, F, verts_in, faces, order, start, verts_out));
  CLMGS_CHECK_ARG(isfinite(factor));
  hipLaunchKernelGGL(mesh_smooth_step_kernel, ms_grid(V), dim3(MS_THREADS), 0, (hipStream_t)stream, verts_in, faces, V, F,
                     order, start, factor, verts_out);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_vertex_normals(void* stream, int V, int F, const float* verts, const int32_t* faces,
                                         const int64_t* order, const int64_t* start, float* normals) {
  CLMGS_CHECK_ARG(ms_args_ok(V, F, verts, faces, order, start, normals));
  hipLaunchKernelGGL(mesh_vertex_normals_kernel, ms_grid(V), dim3(MS_THREADS), 0, (hipStream_t)stream, verts, faces, V, F,
                     order, start, normals);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
