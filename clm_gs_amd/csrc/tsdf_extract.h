// Mesh export ("Mesh export" and "Sparse volume"): the extraction half of what the dense volume
// (csrc/tsdf.hip) and the brick-allocated one (csrc/tsdf_sparse.hip) share, as csrc/tsdf_fuse.h is the fusion half: naive
// Surface Nets in four passes.  Both volumes run this code, so where they store the same sums they give the same cells,
// vertices and quads, bit for bit.  The arithmetic is csrc/tsdf_math.h.
//
// The passes: one lane per lane index, between which the host takes two inclusive int32 prefix sums: cells (0 / 1 per
// active cell), vertices (one per active cell, at the cell's rank), quad_count (0..3 per voxel: its +x, +y, +z edges) and
// quads (two triangles per quad at the voxel's rank).  The ranks fix the output order: vertices by cell, faces by (owner
// voxel, axis), both in lane-index order.
//
// A pass sees its volume through an accessor Vol, a small struct passed by value (DenseVol, BrickVol):
//   nx, ny, nz                      the grid
//   lanes()                         the number of lane indices; a lane index v < 2^31 names a voxel the volume stores
//   decode(v, p)                    v -> its voxel (p[0], p[1], p[2]); false: v names no voxel of the grid
//   neighbour(v, p, dx, dy, dz)     the lane index of the voxel p + (dx, dy, dz), which lies in the grid, seen from v = p;
//                                   < 0: not stored
//   stored(v)                       v >= 0, or true at compile time for a volume that stores every voxel
//   plane(v, pl)                    plane pl of v; 0 where not stored
//   KEYS                            compile time: whether the order above is not the output order wanted, so that the
//                                   vertices and quad passes also write a sort key; then keys (int64*) and linear(p), the
//                                   dense linear index (p[2] ny + p[1]) nx + p[0].  Vertex key: linear(cell); quad key:
//                                   3 linear(owner) + axis.
#pragma once
#include "common.h"
#include "tsdf_fuse.h"
#include "tsdf_math.h"

namespace clmgs {

constexpr int TS_EX_THREADS = 256;
constexpr int TS_EX_MAX_BLOCKS = 8192;  // the passes stride over the lane indices

// p is the origin of a cell iff it has a +1 neighbour along every axis.
template <class Vol>
__device__ __forceinline__ bool ts_is_cell(const Vol& vol, const int (&p)[3]) {
  return p[0] + 1 < vol.nx && p[1] + 1 < vol.ny && p[2] + 1 < vol.nz;
}

template <class Vol>
__device__ __forceinline__ bool ts_ranked(const Vol& vol, const int32_t* __restrict__ scan, int v) {
  return vol.stored(v) && scan[v] != (v > 0 ? scan[v - 1] : 0);
}

template <class Vol>
__global__ void __launch_bounds__(TS_EX_THREADS)
tsdf_cells_kernel(const Vol vol, float min_weight, int32_t* __restrict__ cell_count) {
  const int64_t n = vol.lanes();
  for (int64_t v64 = (int64_t)blockIdx.x * TS_EX_THREADS + threadIdx.x; v64 < n; v64 += (int64_t)gridDim.x * TS_EX_THREADS) {
    const int v = (int)v64;
    int p[3], active = 0;
    if (vol.decode(v, p) && ts_is_cell(vol, p)) {
      float t8[8], w8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int vc = vol.neighbour(v, p, c & 1, (c >> 1) & 1, c >> 2);
        t8[c] = vol.plane(vc, 0);
        w8[c] = vol.plane(vc, 1);
      }
      active = tsdf_cell_active(t8, w8, min_weight) ? 1 : 0;
    }
    cell_count[v] = active;
  }
}

template <class Vol>
__global__ void __launch_bounds__(TS_EX_THREADS)
tsdf_vertices_kernel(const Vol vol, const int32_t* __restrict__ cell_scan, int V, const TsdfCams g2w,
                     float* __restrict__ verts, uint8_t* __restrict__ colours) {
  const int64_t n = vol.lanes();
  for (int64_t v64 = (int64_t)blockIdx.x * TS_EX_THREADS + threadIdx.x; v64 < n; v64 += (int64_t)gridDim.x * TS_EX_THREADS) {
    const int v = (int)v64;
    if (!ts_ranked(vol, cell_scan, v)) continue;
    const int id = cell_scan[v] - 1;
    int p[3];
    if (id < 0 || id >= V || !vol.decode(v, p) || !ts_is_cell(vol, p)) continue;  // (a scan that does not belong to this volume writes nothing outside)
    float vox[TSDF_PLANES][8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int vc = vol.neighbour(v, p, c & 1, (c >> 1) & 1, c >> 2);
#pragma unroll
      for (int pl = 0; pl < TSDF_PLANES; ++pl) vox[pl][c] = vol.plane(vc, pl);
    }
    float xyz[3];
    uint8_t q[3];
    tsdf_cell_vertex(vox, p[0], p[1], p[2], g2w.c[0], xyz, q);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      verts[(int64_t)id * 3 + d] = xyz[d];
      colours[(int64_t)id * 3 + d] = q[d];
    }
    if constexpr (Vol::KEYS) vol.keys[id] = vol.linear(p);
  }
}

// The quad of the grid edge that lane index v = voxel (p[0], p[1], p[2]) owns along `axis`: it exists iff the edge's two
// voxels are valid with different inside flags and the four cells around the edge are active (ranked in cell_scan).
// q[0..3]: the lane indices of the origins of those cells, right-handed about the axis: with a1, a2 the two axes after
// `axis` in cyclic order (axis = a1 x a2), the cells at (p[a1] - 1, p[a2] - 1), (p[a1], p[a2] - 1), (p[a1], p[a2]),
// (p[a1] - 1, p[a2]).
template <class Vol>
__device__ __forceinline__ bool ts_quad(const Vol& vol, const int32_t* __restrict__ cell_scan, float min_weight, int v,
                                        const int (&p)[3], int axis, int (&q)[4], bool& inside) {
  const int dim[3] = {vol.nx, vol.ny, vol.nz};
  const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
  if (p[axis] + 1 >= dim[axis]) return false;
  if (p[a1] < 1 || p[a1] + 1 >= dim[a1] || p[a2] < 1 || p[a2] + 1 >= dim[a2]) return false;
  int e[3] = {0, 0, 0}, e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
  e[axis] = 1;
  e1[a1] = -1;
  e2[a2] = -1;
  const int v2 = vol.neighbour(v, p, e[0], e[1], e[2]);
  if (!tsdf_valid(vol.plane(v, 1), min_weight) || !tsdf_valid(vol.plane(v2, 1), min_weight)) return false;
  inside = tsdf_inside(vol.plane(v, 0));
  if (inside == tsdf_inside(vol.plane(v2, 0))) return false;
  q[0] = vol.neighbour(v, p, e1[0] + e2[0], e1[1] + e2[1], e1[2] + e2[2]);
  q[1] = vol.neighbour(v, p, e2[0], e2[1], e2[2]);
  q[2] = v;
  q[3] = vol.neighbour(v, p, e1[0], e1[1], e1[2]);
  return ts_ranked(vol, cell_scan, q[0]) && ts_ranked(vol, cell_scan, q[1]) && ts_ranked(vol, cell_scan, q[2]) &&
         ts_ranked(vol, cell_scan, q[3]);
}

// EMIT false: quad_count[v] = the number of quads v owns; true: their triangles (and keys) at rank quad_scan[v] - that number.
template <class Vol, bool EMIT>
__global__ void __launch_bounds__(TS_EX_THREADS)
tsdf_quads_kernel(const Vol vol, float min_weight, const int32_t* __restrict__ cell_scan, int32_t* __restrict__ quad_count,
                  const int32_t* __restrict__ quad_scan, int V, int Q, int32_t* __restrict__ faces) {
  const int64_t n = vol.lanes();
  for (int64_t v64 = (int64_t)blockIdx.x * TS_EX_THREADS + threadIdx.x; v64 < n; v64 += (int64_t)gridDim.x * TS_EX_THREADS) {
    const int v = (int)v64;
    if (EMIT && !ts_ranked(vol, quad_scan, v)) continue;
    int p[3];
    const bool in_grid = vol.decode(v, p);
    int count = 0, rank = EMIT ? (v > 0 ? quad_scan[v - 1] : 0) : 0;
    if (in_grid) {
#pragma unroll
      for (int axis = 0; axis < 3; ++axis) {
        int q[4];
        bool inside = false;
        if (!ts_quad(vol, cell_scan, min_weight, v, p, axis, q, inside)) continue;
        ++count;
        if (EMIT) {
          int id[4];
          bool ok = rank >= 0 && rank < Q;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            id[e] = cell_scan[q[e]] - 1;
            ok = ok && id[e] >= 0 && id[e] < V;
          }
          if (ok) {  // two triangles along the diagonal q0 - q2; the owner inside: right-handed about the axis
            int32_t* f = faces + (int64_t)rank * 6;
            f[0] = id[0];
            f[1] = inside ? id[1] : id[2];
            f[2] = inside ? id[2] : id[1];
            f[3] = id[0];
            f[4] = inside ? id[2] : id[3];
            f[5] = inside ? id[3] : id[2];
            if constexpr (Vol::KEYS) vol.keys[rank] = 3 * vol.linear(p) + axis;
          }
          ++rank;
        }
      }
    }
    if (!EMIT) quad_count[v] = count;
  }
}

// ---------------------------------------------------------------------------------------------- host
// The launch grid of a pass over `lanes` lane indices.
static inline dim3 ts_ex_grid(int64_t lanes) {
  return dim3((unsigned)min((int64_t)TS_EX_MAX_BLOCKS, (lanes + TS_EX_THREADS - 1) / TS_EX_THREADS));
}

// grid_to_world (12 doubles, 3x4) as record 0 of the kernel argument; false: null or not finite.
static inline bool ts_load_g2w(const double* grid_to_world, TsdfCams& G) {
  if (grid_to_world == nullptr) return false;
  G = TsdfCams{};
  for (int e = 0; e < 12; ++e) {
    G.c[0][e] = grid_to_world[e];
    if (!isfinite(G.c[0][e])) return false;
  }
  return true;
}

}  // namespace clmgs
