// Mesh evaluation ("Mesh evaluation"): area-weighted surface samples of a mesh, a uniform grid of
// primitives (triangles or points), and the exact distance from every query point to its nearest primitive.  The
// arithmetic is csrc/mesh_distance_math.h; the prefix sums, the sort of the (cell, primitive) pairs by cell and the
// searchsorted that gives the cell segments are torch (clm_kernels.mesh_sample / mesh_distance_grid / mesh_distance).
//
//   sample_count  ONE LANE PER FACE: its area (float64) and its number of samples n_f = ceil(area / spacing^2).
//   sample_emit   ONE LANE PER SAMPLE, so that one huge triangle does not serialise a wave: the face of a sample is the
//                 caller's (repeat_interleave of the counts), its number within the face s - offsets[f].
//   bin_count     ONE LANE PER PRIMITIVE: the number of cells in the index range of its bounding box (0 for a face
//                 without area and for a point with a non-finite coordinate: they are not primitives).
//   bin_emit      ONE LANE PER PRIMITIVE: the (cell, primitive) pairs of that range, at the lane's offset.
//   distance      ONE LANE PER QUERY, two instantiations of one body (triangles | points).  The lane walks the Chebyshev
//                 shells R = 0, 1, ... of cells around the clamped cell of its query, evaluates every listed primitive and
//                 keeps the minimum, ties to the smaller primitive index (a rule that does not depend on the order or on
//                 how often a primitive is met).  It stops after shell R once best_d2 < (R h SLACK)^2, once R h SLACK
//                 exceeds max_distance, or when the grid is exhausted.
//
// Why stopping is exact.  A primitive is listed in every cell of the index range of its bounding box and md_cell is
// monotone, so every point x of a primitive that has not been visited after shell R lies in a cell that differs from
// the query's clamped cell c by at least R + 1 along some axis: floor(fl(fl(x - o) / h)) >= c + R + 1 while
// floor(fl(fl(q - o) / h)) <= c (or q was clamped from outside, which only moves it farther).  Two roundings of relative
// size 2^-53 each move either quotient by less than 2^-52 (c + R + 2) < 2^-31 cells for a grid of at most 2^20 cells per
// axis, so |x - q| > h (R - 2^-30) along that axis.  The closest point the arithmetic of md_closest_d2 finds lies within
// about 2^-49 of the triangle's extent, at most 2^-28 h, of the true one.  SLACK = 1 - 2^-16 covers both with a margin of
// four thousand, and the comparison is strict: what is unvisited is strictly farther than the best found, so it can
// neither beat it nor tie with it.  A query outside the box is clamped to the nearest cell, which moves every bound in
// the safe direction.
//
// The queries arrive sorted by cell (the caller's sort), so the lanes of a wave walk the same lists: the gathers of a
// wave fall on the same cache lines and the wave diverges only at the shell where its lanes stop.  The body is float64
// arithmetic on gathered rows (a 4 B pair, a 12 B face row, three 12 B vertices per evaluation): supposed bound by the
// float64 rate and the gather latency, not by memory bandwidth.
//
// No atomics, no kernel waits for another workgroup, every loop is bounded by the grid's dimensions or a list's length.
// Every index read from memory is compared (unsigned) with its bound before it is used; a query with a non-finite
// coordinate is answered (+inf, -1) before any index arithmetic.
#include "common.h"
#include "mesh_distance_math.h"

namespace clmgs {

constexpr int MD_THREADS = 256;
constexpr int MD_MAX_BLOCKS = 16384;         // the kernels stride over their items
constexpr int MD_MAX_AXIS = 1 << 20;         // cells per axis
constexpr int64_t MD_MAX_CELLS = (int64_t)1 << 27;
constexpr double MD_SLACK = 1.0 - 1.0 / 65536.0;

struct MdGrid {
  double ox, oy, oz, h;
  int gx, gy, gz;
};

__device__ __forceinline__ bool md_in(int x, int n) { return (unsigned)x < (unsigned)n; }

__device__ __forceinline__ void md_load(const float* __restrict__ verts, int v, double* p) {
  p[0] = (double)verts[(int64_t)v * 3];
  p[1] = (double)verts[(int64_t)v * 3 + 1];
  p[2] = (double)verts[(int64_t)v * 3 + 2];
}

// The corners of face f, or false when an index lies outside [0, V).
__device__ __forceinline__ bool md_corners(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V,
                                           int64_t f, double* a, double* b, double* c) {
  const int va = faces[f * 3], vb = faces[f * 3 + 1], vc = faces[f * 3 + 2];
  if (!(md_in(va, V) && md_in(vb, V) && md_in(vc, V))) return false;
  md_load(verts, va, a);
  md_load(verts, vb, b);
  md_load(verts, vc, c);
  return true;
}

__global__ void __launch_bounds__(MD_THREADS)
mesh_sample_count_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int F, double spacing,
                         double* __restrict__ area, int64_t* __restrict__ count) {
  for (int64_t f = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * MD_THREADS) {
    double a[3], b[3], c[3];
    double ar = 0.0;
    if (md_corners(verts, faces, V, f, a, b, c)) ar = md_face_area(a, b, c);
    area[f] = ar;
    count[f] = md_sample_count(ar, spacing);
  }
}

__global__ void __launch_bounds__(MD_THREADS)
mesh_sample_emit_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int F,
                        const double* __restrict__ area, const int64_t* __restrict__ offsets,
                        const int32_t* __restrict__ sample_face, int64_t S, float* __restrict__ points,
                        double* __restrict__ weight) {
#pragma clang fp contract(off)
  for (int64_t s = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; s < S; s += (int64_t)gridDim.x * MD_THREADS) {
    float o[3] = {0.0f, 0.0f, 0.0f};
    double w = 0.0;
    const int f = sample_face[s];
    if (md_in(f, F)) {
      const int64_t k = s - offsets[f], n = offsets[f + 1] - offsets[f];
      double a[3], b[3], c[3];
      if (k >= 0 && k < n && md_corners(verts, faces, V, f, a, b, c)) {
        md_sample_position(k, a, b, c, o);
        w = area[f] / (double)n;
      }
    }
    points[s * 3] = o[0];
    points[s * 3 + 1] = o[1];
    points[s * 3 + 2] = o[2];
    weight[s] = w;
  }
}

// The cell range [lo, hi] per axis of primitive i, or false when it is no primitive.
template <bool TRI>
__device__ __forceinline__ bool md_range(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int64_t i,
                                         const MdGrid& g, int* lo, int* hi) {
  double mn[3], mx[3];
  if (TRI) {
    double a[3], b[3], c[3];
    if (!md_corners(verts, faces, V, i, a, b, c)) return false;
    if (!md_area_ok(md_face_area(a, b, c))) return false;
    for (int d = 0; d < 3; ++d) {
      mn[d] = fmin(a[d], fmin(b[d], c[d]));
      mx[d] = fmax(a[d], fmax(b[d], c[d]));
    }
  } else {
    md_load(verts, (int)i, mn);
    if (!(isfinite(mn[0]) && isfinite(mn[1]) && isfinite(mn[2]))) return false;
    mx[0] = mn[0];
    mx[1] = mn[1];
    mx[2] = mn[2];
  }
  lo[0] = md_cell(mn[0], g.ox, g.h, g.gx);
  hi[0] = md_cell(mx[0], g.ox, g.h, g.gx);
  lo[1] = md_cell(mn[1], g.oy, g.h, g.gy);
  hi[1] = md_cell(mx[1], g.oy, g.h, g.gy);
  lo[2] = md_cell(mn[2], g.oz, g.h, g.gz);
  hi[2] = md_cell(mx[2], g.oz, g.h, g.gz);
  return true;
}

template <bool TRI>
__global__ void __launch_bounds__(MD_THREADS)
mesh_bin_count_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int N, MdGrid g,
                      int64_t* __restrict__ count) {
  for (int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * MD_THREADS) {
    int lo[3], hi[3];
    int64_t n = 0;
    if (md_range<TRI>(verts, faces, V, i, g, lo, hi))
      n = (int64_t)(hi[0] - lo[0] + 1) * (int64_t)(hi[1] - lo[1] + 1) * (int64_t)(hi[2] - lo[2] + 1);
    count[i] = n;
  }
}

template <bool TRI>
__global__ void __launch_bounds__(MD_THREADS)
mesh_bin_emit_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int N, MdGrid g,
                     const int64_t* __restrict__ offsets, int64_t pairs, int64_t* __restrict__ cell,
                     int32_t* __restrict__ prim) {
  for (int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * MD_THREADS) {
    int lo[3], hi[3];
    if (!md_range<TRI>(verts, faces, V, i, g, lo, hi)) continue;
    int64_t j = offsets[i];
    const int64_t end = min(offsets[i + 1], pairs);
    if (j < 0) continue;
    for (int z = lo[2]; z <= hi[2]; ++z)
      for (int y = lo[1]; y <= hi[1]; ++y)
        for (int x = lo[0]; x <= hi[0]; ++x) {
          if (j >= end) break;
          cell[j] = ((int64_t)z * g.gy + y) * g.gx + x;
          prim[j] = (int32_t)i;
          ++j;
        }
  }
}

struct MdBest {
  double d2;
  int prim;
  int evaluated;
};

// Every primitive listed in cell (x, y, z), which lies inside the grid.
template <bool TRI>
__device__ __forceinline__ void md_visit(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int N,
                                         const MdGrid& g, const int64_t* __restrict__ cell_start,
                                         const int32_t* __restrict__ pair_prim, int64_t pairs, const double* q, int x, int y,
                                         int z, MdBest& best) {
  const int64_t cell = ((int64_t)z * g.gy + y) * g.gx + x;
  int64_t j = cell_start[cell];
  const int64_t end = min(cell_start[cell + 1], pairs);
  if (j < 0) return;
  for (; j < end; ++j) {
    const int i = pair_prim[j];
    if (!md_in(i, N)) continue;
    double d2;
    if (TRI) {
      double a[3], b[3], c[3];
      if (!md_corners(verts, faces, V, i, a, b, c)) continue;
      d2 = md_closest_d2(q, a, b, c);
    } else {
      double a[3];
      md_load(verts, i, a);
      d2 = md_point_d2(q, a);
    }
    ++best.evaluated;
    if (d2 < best.d2 || (d2 == best.d2 && i < best.prim)) {  // (a NaN compares false: never taken)
      best.d2 = d2;
      best.prim = i;
    }
  }
}

template <bool TRI>
__global__ void __launch_bounds__(MD_THREADS)
mesh_distance_kernel(int64_t P, const float* __restrict__ queries, const float* __restrict__ verts,
                     const int32_t* __restrict__ faces, int V, int N, MdGrid g, const int64_t* __restrict__ cell_start,
                     const int32_t* __restrict__ pair_prim, int64_t pairs, double max_distance, float* __restrict__ dist,
                     int32_t* __restrict__ prim, int32_t* __restrict__ evaluated) {
#pragma clang fp contract(off)
  for (int64_t p = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; p < P; p += (int64_t)gridDim.x * MD_THREADS) {
    const float qf[3] = {queries[p * 3], queries[p * 3 + 1], queries[p * 3 + 2]};
    MdBest best = {(double)INFINITY, -1, 0};
    if (isfinite(qf[0]) && isfinite(qf[1]) && isfinite(qf[2])) {
      const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
      const int cx = md_cell(q[0], g.ox, g.h, g.gx), cy = md_cell(q[1], g.oy, g.h, g.gy), cz = md_cell(q[2], g.oz, g.h, g.gz);
      // the last shell that holds a cell of the grid
      const int last = max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
      for (int R = 0; R <= last; ++R) {
        const int z0 = max(cz - R, 0), z1 = min(cz + R, g.gz - 1);
        const int y0 = max(cy - R, 0), y1 = min(cy + R, g.gy - 1);
        for (int z = z0; z <= z1; ++z) {
          const bool zface = (z == cz - R) || (z == cz + R);
          for (int y = y0; y <= y1; ++y) {
            if (zface || y == cy - R || y == cy + R) {  // a full row of the shell
              const int x0 = max(cx - R, 0), x1 = min(cx + R, g.gx - 1);
              for (int x = x0; x <= x1; ++x)
                md_visit<TRI>(verts, faces, V, N, g, cell_start, pair_prim, pairs, q, x, y, z, best);
            } else {  // an interior row: only its two ends belong to the shell (R >= 1 here)
              if (cx - R >= 0) md_visit<TRI>(verts, faces, V, N, g, cell_start, pair_prim, pairs, q, cx - R, y, z, best);
              if (cx + R <= g.gx - 1)
                md_visit<TRI>(verts, faces, V, N, g, cell_start, pair_prim, pairs, q, cx + R, y, z, best);
            }
          }
        }
        const double reach = ((double)R * g.h) * MD_SLACK;  // everything unvisited is strictly farther than this
        if (best.d2 < reach * reach || reach > max_distance) break;
      }
    }
    float d = INFINITY;
    int32_t who = -1;
    if (best.prim >= 0) {
      const double dd = sqrt(best.d2);
      if (!(dd > max_distance)) {
        d = (float)dd;
        who = best.prim;
      }
    }
    dist[p] = d;
    prim[p] = who;
    if (evaluated) evaluated[p] = best.evaluated;
  }
}

static bool md_aligned(const void* p, uintptr_t a) { return p != nullptr && ((uintptr_t)p % a) == 0; }

static dim3 md_blocks(int64_t n) { return dim3((unsigned)min((int64_t)MD_MAX_BLOCKS, (n + MD_THREADS - 1) / MD_THREADS)); }

static bool md_grid_ok(double ox, double oy, double oz, double h, int gx, int gy, int gz) {
  if (!(isfinite(ox) && isfinite(oy) && isfinite(oz) && h > 0.0 && isfinite(h))) return false;
  if (!(gx >= 1 && gy >= 1 && gz >= 1 && gx <= MD_MAX_AXIS && gy <= MD_MAX_AXIS && gz <= MD_MAX_AXIS)) return false;
  return (int64_t)gx * gy * gz <= MD_MAX_CELLS;
}

// verts [V,3]; faces [N,3] for triangles, null for points (then N == V)
static bool md_prims_ok(int V, int N, const float* verts, const int32_t* faces) {
  if (!(V >= 1 && N >= 1 && md_aligned(verts, 4))) return false;
  return faces ? md_aligned(faces, 4) : N == V;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_mesh_sample_count(void* stream, int V, int F, const float* verts, const int32_t* faces, double spacing,
                                       double* area, int64_t* count) {
  CLMGS_CHECK_ARG(V >= 1 && F >= 1);
  CLMGS_CHECK_ARG(spacing > 0.0 && isfinite(spacing));
  CLMGS_CHECK_ARG(md_aligned(verts, 4) && md_aligned(faces, 4) && md_aligned(area, 8) && md_aligned(count, 8));
  hipLaunchKernelGGL(mesh_sample_count_kernel, md_blocks(F), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, faces, V, F,
                     spacing, area, count);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_sample_emit(void* stream, int V, int F, const float* verts, const int32_t* faces,
                                      const double* area, const int64_t* offsets, const int32_t* sample_face, int64_t S,
                                      float* points, double* weight) {
  CLMGS_CHECK_ARG(V >= 1 && F >= 1 && S >= 1 && S < ((int64_t)1 << 31));
  CLMGS_CHECK_ARG(md_aligned(verts, 4) && md_aligned(faces, 4) && md_aligned(area, 8) && md_aligned(offsets, 8) &&
                  md_aligned(sample_face, 4) && md_aligned(points, 4) && md_aligned(weight, 8));
  hipLaunchKernelGGL(mesh_sample_emit_kernel, md_blocks(S), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, faces, V, F,
                     area, offsets, sample_face, S, points, weight);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_bin_count(void* stream, int V, int N, const float* verts, const int32_t* faces, double ox, double oy,
                                    double oz, double h, int gx, int gy, int gz, int64_t* count) {
  CLMGS_CHECK_ARG(md_prims_ok(V, N, verts, faces));
  CLMGS_CHECK_ARG(md_grid_ok(ox, oy, oz, h, gx, gy, gz));
  CLMGS_CHECK_ARG(md_aligned(count, 8));
  const MdGrid g{ox, oy, oz, h, gx, gy, gz};
  if (faces)
    hipLaunchKernelGGL(mesh_bin_count_kernel<true>, md_blocks(N), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, faces, V, N,
                       g, count);
  else
    hipLaunchKernelGGL(mesh_bin_count_kernel<false>, md_blocks(N), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, faces, V, N,
                       g, count);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_bin_emit(void* stream, int V, int N, const float* verts, const int32_t* faces, double ox, double oy,
                                   double oz, double h, int gx, int gy, int gz, const int64_t* offsets, int64_t pairs,
                                   int64_t* cell, int32_t* prim) {
  CLMGS_CHECK_ARG(md_prims_ok(V, N, verts, faces));
  CLMGS_CHECK_ARG(md_grid_ok(ox, oy, oz, h, gx, gy, gz));
  CLMGS_CHECK_ARG(pairs >= 1 && md_aligned(offsets, 8) && md_aligned(cell, 8) && md_aligned(prim, 4));
  const MdGrid g{ox, oy, oz, h, gx, gy, gz};
  if (faces)
    hipLaunchKernelGGL(mesh_bin_emit_kernel<true>, md_blocks(N), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, faces, V, N,
                       g, offsets, pairs, cell, prim);
  else
    hipLaunchKernelGGL(mesh_bin_emit_kernel<false>, md_blocks(N), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, faces, V, N,
                       g, offsets, pairs, cell, prim);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_distance(void* stream, int64_t P, const float* queries, int V, int N, const float* verts,
                                   const int32_t* faces, double ox, double oy, double oz, double h, int gx, int gy, int gz,
                                   const int64_t* cell_start, const int32_t* pair_prim, int64_t pairs, double max_distance,
                                   float* dist, int32_t* prim, int32_t* evaluated) {
  CLMGS_CHECK_ARG(P >= 1 && md_aligned(queries, 4));
  CLMGS_CHECK_ARG(md_prims_ok(V, N, verts, faces));
  CLMGS_CHECK_ARG(md_grid_ok(ox, oy, oz, h, gx, gy, gz));
  CLMGS_CHECK_ARG(pairs >= 1 && md_aligned(cell_start, 8) && md_aligned(pair_prim, 4));
  CLMGS_CHECK_ARG(max_distance > 0.0);  // (+inf allowed, NaN not)
  CLMGS_CHECK_ARG(md_aligned(dist, 4) && md_aligned(prim, 4) && (evaluated == nullptr || md_aligned(evaluated, 4)));
  CLMGS_CHECK_ARG((const void*)dist != (const void*)queries && (const void*)prim != (const void*)queries);
  const MdGrid g{ox, oy, oz, h, gx, gy, gz};
  if (faces)
    hipLaunchKernelGGL(mesh_distance_kernel<true>, md_blocks(P), dim3(MD_THREADS), 0, (hipStream_t)stream, P, queries, verts,
                       faces, V, N, g, cell_start, pair_prim, pairs, max_distance, dist, prim, evaluated);
  else
    hipLaunchKernelGGL(mesh_distance_kernel<false>, md_blocks(P), dim3(MD_THREADS), 0, (hipStream_t)stream, P, queries, verts,
                       faces, V, N, g, cell_start, pair_prim, pairs, max_distance, dist, prim, evaluated);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
