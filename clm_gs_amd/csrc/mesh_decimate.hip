// Mesh decimation ("Mesh decimation"): vertex clustering on a world-aligned grid with quadric-error
// representatives (Lindstrom 2000; quadrics after Garland & Heckbert 1997).  The arithmetic is csrc/decimate_math.h; the
// sorts, prefix sums and compactions between the kernels are torch (clm_kernels.mesh_decimate_*, mesh_decimate.py).
//
//   mark    one lane per face: mark[v] = 1 for its three corners.  Plain byte stores of one value: the marks form a set,
//           whatever the order.
//   keys    one lane per vertex: the int64 key of the cell of a marked vertex, -1 for an unmarked one; a marked vertex
//           with a non-finite coordinate or a cell index outside [-2^20, 2^20) raises its bit of *flag (an integer atomic
//           OR, once per lane that saw one).  The caller reads that ONE flag before anything else is launched.
//   faces   one lane per face: the corners' clusters, rotated so that the smallest comes first (orientation kept), a
//           collapsed flag when two are equal, and the face's incidences: one int64 (cluster << 32 | face) per DISTINCT
//           cluster among the corners, INT64_MAX in the unused slots of its three.  Sorted ascending, the incidences are
//           ordered by cluster, then face, the unused slots last.
//   place   ONE LANE PER CLUSTER.  It walks the cluster's vertices (ascending index) for the mean and the colour sums, then
//           its incidences (ascending face) for the nine sums of the quadric, solves and writes the float32 vertex, the
//           colour and the placement code.
//
// Why one lane per cluster and not a part-wave.  The contract fixes each cluster's sums as left-to-right float64 sums in
// ascending face order, so the additions of one cluster are a serial chain whoever performs them: a part-wave could only
// spread the gathers and the per-face products over its lanes and would still hand the terms to one lane, through
// shuffles, to add.  On a Surface Nets mesh with a cell of k voxels a cluster has a few times k^2 faces (tens), far
// below 64, so most lanes of a part-wave would idle; and the clusters are many (V / k^2), so one lane per cluster fills
// the machine.  The cost is divergence when segment lengths differ inside a wave, and a single huge cluster (a cell
// larger than the mesh) is walked by one lane: correct, and slow only where decimation is pointless.
//
// Which cluster a lane takes is the caller's choice (lane_order, a permutation; the output does not depend on it).  In
// key order neighbouring clusters are neighbours along z, while an extracted mesh stores its vertices and faces along x
// first: the 64 lanes of a wave then gather from 64 places a slab apart and fetch a cache line per vertex.  The caller
// orders the lanes by each cluster's first member vertex instead, so that neighbouring lanes gather from neighbouring
// rows: 16.2 -> 10.9 ms on the 90.7 M faces of DESIGN.md's table.  Two further forms were measured and dropped for no
// gain: reading the incidence, the face row and the corners one step ahead of each other (16.2 ms unchanged: the walk is
// bound by the number of scattered requests, not by the latency of one chain), and ordering the incidence list itself by
// lane (10.4 ms in the kernel, 0.6 ms more in the face pass).
//
// No float atomics, no kernel waits for another workgroup.  Every index read from memory is compared (unsigned) with its
// bound before it is used: a face index outside [0, V), a vertex or face index of a list outside its array, or a segment
// outside its list is skipped, never followed.
#include "common.h"
#include "decimate_math.h"

namespace clmgs {

constexpr int MD_THREADS = 256;
constexpr int MD_MAX_BLOCKS = 8192;  // the kernels stride over faces / vertices / clusters

__device__ __forceinline__ bool md_in(int x, int n) { return (unsigned)x < (unsigned)n; }

__global__ void __launch_bounds__(MD_THREADS)
decimate_mark_kernel(const int32_t* __restrict__ faces, int F, int V, uint8_t* mark) {
  for (int64_t f = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * MD_THREADS) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int v = faces[f * 3 + e];
      if (md_in(v, V)) mark[v] = 1;
    }
  }
}

__global__ void __launch_bounds__(MD_THREADS)
decimate_keys_kernel(const float* __restrict__ verts, const uint8_t* __restrict__ mark, int V, double cell, int64_t* keys,
                     int32_t* flag) {
  int raised = 0;
  for (int64_t v = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MD_THREADS) {
    int64_t key = -1;
    if (mark[v]) raised |= dec_key(verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2], cell, key);
    keys[v] = key;
  }
  if (raised) atomicOr(flag, raised);
}

__global__ void __launch_bounds__(MD_THREADS)
decimate_faces_kernel(const int32_t* __restrict__ faces, int F, int V, const int32_t* __restrict__ cluster, int C,
                      int32_t* out_faces, uint8_t* collapsed, int64_t* inc) {
  for (int64_t f = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * MD_THREADS) {
    int c[3];
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int v = faces[f * 3 + e];
      c[e] = md_in(v, V) ? cluster[v] : -1;
      ok = ok && md_in(c[e], C);
    }
    const int64_t none = INT64_MAX;
    if (!ok) {  // (refused by the caller before the launch; never followed here)
      out_faces[f * 3] = out_faces[f * 3 + 1] = out_faces[f * 3 + 2] = 0;
      collapsed[f] = 1;
      inc[f * 3] = inc[f * 3 + 1] = inc[f * 3 + 2] = none;
      continue;
    }
    collapsed[f] = (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) ? 1 : 0;
    const int s = (c[1] < c[0] && c[1] <= c[2]) ? 1 : ((c[2] < c[0] && c[2] < c[1]) ? 2 : 0);  // the first smallest
    out_faces[f * 3] = c[s];
    out_faces[f * 3 + 1] = c[(s + 1) % 3];
    out_faces[f * 3 + 2] = c[(s + 2) % 3];
    inc[f * 3] = ((int64_t)c[0] << 32) | f;
    inc[f * 3 + 1] = c[1] != c[0] ? (((int64_t)c[1] << 32) | f) : none;
    inc[f * 3 + 2] = (c[2] != c[0] && c[2] != c[1]) ? (((int64_t)c[2] << 32) | f) : none;
  }
}

__global__ void __launch_bounds__(MD_THREADS)
decimate_place_kernel(const float* __restrict__ verts, const uint8_t* __restrict__ colours, const int32_t* __restrict__ faces,
                      int V, int F, int C, const int64_t* __restrict__ ckeys, const int32_t* __restrict__ vorder,
                      const int64_t* __restrict__ vstart, int64_t n_members, const int64_t* __restrict__ inc,
                      const int64_t* __restrict__ istart, int64_t n_inc, const int32_t* __restrict__ lane_order,
                      double cell, float* out_verts, uint8_t* out_colours, uint8_t* code) {
#pragma clang fp contract(off)
  for (int64_t t = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; t < C; t += (int64_t)gridDim.x * MD_THREADS) {
    const int64_t k = lane_order[t];  // neighbouring lanes take clusters whose vertices are neighbours in memory
    if (!md_in((int)k, C)) continue;
    double c[3];
    dec_centre(ckeys[k], cell, c);
    // ---- the mean and the colour sums over the members, ascending vertex index
    double ms[3] = {0.0, 0.0, 0.0};
    int64_t cs[3] = {0, 0, 0}, n = 0;
    int64_t b = vstart[k], e = vstart[k + 1];
    b = b < 0 ? 0 : b;
    e = e > n_members ? n_members : e;
    for (int64_t j = b; j < e; ++j) {
      const int v = vorder[j];
      if (!md_in(v, V)) continue;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        ms[d] = ms[d] + ((double)verts[(int64_t)v * 3 + d] - c[d]);
        cs[d] += colours[(int64_t)v * 3 + d];
      }
      ++n;
    }
    double m[3] = {0.0, 0.0, 0.0};
    uint8_t rgb[3] = {0, 0, 0};
    if (n > 0) {
      const double dn = (double)n;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        m[d] = ms[d] / dn;
        rgb[d] = (uint8_t)((2 * cs[d] + n) / (2 * n));
      }
    }
    // ---- the nine sums of the quadric over the incidences, ascending face index
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
    b = istart[k];
    e = istart[k + 1];
    b = b < 0 ? 0 : b;
    e = e > n_inc ? n_inc : e;
    for (int64_t j = b; j < e; ++j) {
      const int64_t f = inc[j] & 0xffffffffll;
      if (f >= F) continue;
      const int v0 = faces[f * 3], v1 = faces[f * 3 + 1], v2 = faces[f * 3 + 2];
      if (!(md_in(v0, V) && md_in(v1, V) && md_in(v2, V))) continue;
      double p[3][3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        p[0][d] = (double)verts[(int64_t)v0 * 3 + d];
        p[1][d] = (double)verts[(int64_t)v1 * 3 + d];
        p[2][d] = (double)verts[(int64_t)v2 * 3 + d];
      }
      dec_add_face(p[0], p[1], p[2], c, A, r);
    }
    double x[3];
    code[k] = (uint8_t)dec_place(A, r, m, cell, x);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      out_verts[k * 3 + d] = (float)(c[d] + x[d]);
      out_colours[k * 3 + d] = rgb[d];
    }
  }
}

static bool md_aligned(const void* p, uintptr_t a) { return p != nullptr && ((uintptr_t)p % a) == 0; }

static bool md_apart(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + na <= b0 || b0 + nb <= a0;
}

static dim3 md_grid(int64_t n) { return dim3((unsigned)min((int64_t)MD_MAX_BLOCKS, (n + MD_THREADS - 1) / MD_THREADS)); }

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_mesh_decimate_mark(void* stream, int V, int F, const int32_t* faces, uint8_t* mark) {
  CLMGS_CHECK_ARG(V >= 1 && F >= 1);
  CLMGS_CHECK_ARG(md_aligned(faces, 4) && mark != nullptr);
  CLMGS_CHECK_ARG(md_apart(mark, (uint64_t)V, faces, (uint64_t)F * 12));
  hipLaunchKernelGGL(decimate_mark_kernel, md_grid(F), dim3(MD_THREADS), 0, (hipStream_t)stream, faces, F, V, mark);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_decimate_keys(void* stream, int V, const float* verts, const uint8_t* mark, double cell,
                                        int64_t* keys, int32_t* flag) {
  CLMGS_CHECK_ARG(V >= 1);
  CLMGS_CHECK_ARG(cell > 0.0 && isfinite(cell));
  CLMGS_CHECK_ARG(md_aligned(verts, 4) && mark != nullptr && md_aligned(keys, 8) && md_aligned(flag, 4));
  const uint64_t vb = (uint64_t)V * 12, kb = (uint64_t)V * 8;
  CLMGS_CHECK_ARG(md_apart(keys, kb, verts, vb) && md_apart(keys, kb, mark, (uint64_t)V) && md_apart(flag, 4, keys, kb) &&
                  md_apart(flag, 4, verts, vb) && md_apart(flag, 4, mark, (uint64_t)V));
  hipLaunchKernelGGL(decimate_keys_kernel, md_grid(V), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, mark, V, cell, keys,
                     flag);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_decimate_faces(void* stream, int V, int F, int C, const int32_t* faces, const int32_t* cluster,
                                         int32_t* out_faces, uint8_t* collapsed, int64_t* inc) {
  CLMGS_CHECK_ARG(V >= 1 && F >= 1 && C >= 1 && C <= V);
  CLMGS_CHECK_ARG(md_aligned(faces, 4) && md_aligned(cluster, 4) && md_aligned(out_faces, 4) && collapsed != nullptr &&
                  md_aligned(inc, 8));
  const uint64_t fb = (uint64_t)F * 12, ib = (uint64_t)F * 24, cb = (uint64_t)V * 4;
  CLMGS_CHECK_ARG(md_apart(out_faces, fb, faces, fb) && md_apart(out_faces, fb, cluster, cb) &&
                  md_apart(collapsed, (uint64_t)F, faces, fb) && md_apart(collapsed, (uint64_t)F, cluster, cb) &&
                  md_apart(inc, ib, faces, fb) && md_apart(inc, ib, cluster, cb) && md_apart(out_faces, fb, inc, ib) &&
                  md_apart(out_faces, fb, collapsed, (uint64_t)F) && md_apart(inc, ib, collapsed, (uint64_t)F));
  hipLaunchKernelGGL(decimate_faces_kernel, md_grid(F), dim3(MD_THREADS), 0, (hipStream_t)stream, faces, F, V, cluster, C,
                     out_faces, collapsed, inc);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_decimate_place(void* stream, int V, int F, int C, const float* verts, const uint8_t* colours,
                                         const int32_t* faces, const int64_t* cluster_keys, const int32_t* vert_order,
                                         const int64_t* vert_start, int64_t n_members, const int64_t* inc,
                                         const int64_t* inc_start, int64_t n_inc, const int32_t* lane_order, double cell,
                                         float* out_verts, uint8_t* out_colours, uint8_t* code) {
  CLMGS_CHECK_ARG(V >= 1 && F >= 1 && C >= 1 && C <= V);
  CLMGS_CHECK_ARG(n_members >= C && n_members <= (int64_t)V && n_inc >= 0 && n_inc <= 3 * (int64_t)F);
  CLMGS_CHECK_ARG(cell > 0.0 && isfinite(cell));
  CLMGS_CHECK_ARG(md_aligned(verts, 4) && colours != nullptr && md_aligned(faces, 4) && md_aligned(cluster_keys, 8) &&
                  md_aligned(vert_order, 4) && md_aligned(vert_start, 8) && md_aligned(inc, 8) && md_aligned(inc_start, 8) &&
                  md_aligned(lane_order, 4) && md_aligned(out_verts, 4) && out_colours != nullptr && code != nullptr);
  const struct { const void* p; uint64_t n; } in[] = {
      {verts, (uint64_t)V * 12}, {colours, (uint64_t)V * 3}, {faces, (uint64_t)F * 12}, {cluster_keys, (uint64_t)C * 8},
      {vert_order, (uint64_t)n_members * 4}, {vert_start, ((uint64_t)C + 1) * 8}, {inc, (uint64_t)n_inc * 8},
      {inc_start, ((uint64_t)C + 1) * 8}, {lane_order, (uint64_t)C * 4}};
  const struct { const void* p; uint64_t n; } out[] = {
      {out_verts, (uint64_t)C * 12}, {out_colours, (uint64_t)C * 3}, {code, (uint64_t)C}};
  for (const auto& o : out) {
    for (const auto& i : in) CLMGS_CHECK_ARG(md_apart(o.p, o.n, i.p, i.n));
    for (const auto& o2 : out) CLMGS_CHECK_ARG(o.p == o2.p || md_apart(o.p, o.n, o2.p, o2.n));
  }
  hipLaunchKernelGGL(decimate_place_kernel, md_grid(C), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, colours, faces, V, F,
                     C, cluster_keys, vert_order, vert_start, n_members, inc, inc_start, n_inc, lane_order, cell, out_verts,
                     out_colours, code);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
