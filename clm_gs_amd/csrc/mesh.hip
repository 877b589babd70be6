// Mesh cleanup ("Mesh cleanup"): the connected components of a triangle list and their face counts.
//
// Input: faces int32 [F,3], any triangle list over V vertices; two vertices are connected when a face names both (a
// degenerate face connects what it names).  Contract: label[v] = the smallest vertex index of v's component, label[v] = v
// for a vertex no face names.  The contract fixes every bit, whatever the order of faces, waves or launches.
//
// Labelling is hook and shortcut (FastSV style) over parent int32 [V], which the caller starts as arange(V).  The caller
// alternates the two kernels below and reads ONE changed flag per round; no kernel waits on, polls or spins for another
// workgroup, and neither kernel has a loop other than its stride over faces / vertices.
//   hook      one lane per face (a, b, c): reads p_x = parent[x] and g_x = parent[p_x] for its three vertices, takes m =
//             min(g_a, g_b, g_c) (g_x <= p_x <= x) and lowers parent[x], parent[p_x] and parent[g_x] to m by integer
//             atomicMin at device scope wherever the value it holds for them is larger than m.  It raises the flag
//             whenever an atomicMin returned something larger than what it wrote.
//   shortcut  one lane per vertex: parent[v] = parent[parent[v]], raising the flag on change.
// The caller stops after a round in which the flag stayed down.
//
// Why this is correct.
//   (1) parent[x] <= x always holds and parent[x] is always in x's component: true of arange; hook writes m, one of the
//       values parent held for a vertex of the face's component, below what it replaces (atomicMin); shortcut writes
//       parent[parent[v]] <= parent[v], in the component by induction.
//   (2) Values only decrease: atomicMin, and (1) for the plain store of shortcut, whose lane is the only writer of parent[v]
//       in its launch.
//   (3) A stale read inside a launch (the per-XCD L2s are not coherent with each other, and a CU's L1 is not refreshed by
//       another CU's stores) therefore only yields an OLDER value of parent[x]: still <= x, still in the component, so
//       still a valid ancestor.  It can cost a round, never correctness.
//   (4) A launch boundary makes every write of a round visible to the next launch.
//   (5) A round in which neither kernel wrote read the true state everywhere (no write in flight to be stale against), so
//       it proves a fixed point: shortcut changed nothing, so parent[parent[v]] = parent[v] for every v (every tree is a
//       star); hook changed nothing, so for every face g_x = p_x and p_a = p_b = p_c (a larger one would have been
//       lowered).  All vertices of a component then share one root r with parent[r] = r; r is in the component and
//       r = parent[v] <= v for every v of it (1): r is the component's minimum.  A vertex no face names is never written.
// Every face index is compared (unsigned) against V and a face with an index outside [0, V) is skipped; values read from
// parent are checked the same way before they are used as an index, so a parent array that is not what the caller was
// asked for is not followed outside [0, V).
//
// Sizes.  One lane per face adds to count[label[faces[f,0]]] (int32 [V], zero except at labels), an integer sum and so
// independent of order.  One component usually owns nearly all faces, and every adder on one address is the slow shape
// of an atomic, so the adds are aggregated in the wave first: a lane whose label differs from its lower neighbour's
// heads a run, a ballot of the heads gives every head the length of its run (the distance to the next head bit), and
// only heads add, that length.  A wave owns a contiguous range of faces and walks it 64 at a time; the run still open
// at the end of a step is carried into the next one and added only when it ends, so a wave whose faces all belong to
// one component adds once.  Surface Nets emits a component's faces close together: the runs are long.
#include "common.h"

namespace clmgs {

constexpr int MS_THREADS = 256;
constexpr int MS_MAX_BLOCKS = 8192;  // the kernels stride over faces / vertices

__device__ __forceinline__ bool ms_in(int x, int V) { return (unsigned)x < (unsigned)V; }

__device__ __forceinline__ int ms_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parent[x] = min(parent[x], m); true iff that lowered it
__device__ __forceinline__ bool ms_lower(int32_t* parent, int x, int m) {
  return __hip_atomic_fetch_min(parent + x, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > m;
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_hook_kernel(const int32_t* __restrict__ faces, int F, int V, int32_t* parent, int32_t* flag) {
  bool changed = false;
  for (int64_t f = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * MS_THREADS) {
    int x[3], p[3], g[3];
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      x[e] = faces[f * 3 + e];
      ok = ok && ms_in(x[e], V);
    }
    if (!ok) continue;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      p[e] = ms_load(parent + x[e]);
      ok = ok && ms_in(p[e], V);
    }
    if (!ok) continue;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      g[e] = ms_load(parent + p[e]);
      ok = ok && ms_in(g[e], V);
    }
    if (!ok) continue;
    const int m = min(g[0], min(g[1], g[2]));
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      if (p[e] > m) changed = ms_lower(parent, x[e], m) || changed;
      if (g[e] > m) {
        changed = ms_lower(parent, p[e], m) || changed;
        changed = ms_lower(parent, g[e], m) || changed;
      }
    }
  }
  if (changed) *flag = 1;
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_shortcut_kernel(int V, int32_t* parent, int32_t* flag) {
  bool changed = false;
  for (int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MS_THREADS) {
    const int p = ms_load(parent + v);
    if (!ms_in(p, V)) continue;
    const int g = ms_load(parent + p);
    if (g < p && g >= 0) {
      parent[v] = g;
      changed = true;
    }
  }
  if (changed) *flag = 1;
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_component_faces_kernel(const int32_t* __restrict__ faces, int F, int V, const int32_t* __restrict__ labels,
                            int32_t* count) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (MS_THREADS / 64);
  const int64_t chunk = (((int64_t)F + waves - 1) / waves + 63) & ~(int64_t)63;  // faces per wave, whole steps of 64
  const int64_t begin = ((int64_t)blockIdx.x * (MS_THREADS / 64) + (threadIdx.x >> 6)) * chunk;
  const int64_t end = min(begin + chunk, (int64_t)F);
  int open_l = -1, open_n = 0;  // the run still open at the end of the last step (the same in every lane)
  // (begin and end are the same for every lane of a wave: whole waves reach the ballot)
  for (int64_t base = begin; base < end; base += 64) {
    const int64_t f = base + lane;
    int l = -1;  // no label: a lane past the end, a face outside [0, V)
    if (f < end) {
      const int a = faces[f * 3];
      if (ms_in(a, V)) {
        l = labels[a];
        if (!ms_in(l, V)) l = -1;
      }
    }
    const int below = __shfl_up(l, 1, 64);
    const bool head = lane == 0 || l != below;
    const unsigned long long heads = __ballot(head);           // (bit 0 is always set)
    const unsigned long long above = (heads >> lane) >> 1;     // the head bits of the lanes above this one
    const int run = above ? __ffsll(above) : 64 - lane;        // of a head: to the next head, or to the end of the wave
    const int top = 63 - __clzll(heads);                       // the head of the step's last run
    const int first_l = __shfl(l, 0, 64), first_n = __shfl(run, 0, 64), last_l = __shfl(l, 63, 64);
    if (first_l == open_l) {
      open_n += first_n;
    } else {
      if (lane == 0 && open_l >= 0) atomicAdd(count + open_l, open_n);
      open_l = first_l;
      open_n = first_n;
    }
    if (top != 0) {  // the step's first run has ended: it is added, the runs between it and the last add themselves
      if (lane == 0 && open_l >= 0) atomicAdd(count + open_l, open_n);
      if (head && lane != 0 && lane != top && l >= 0) atomicAdd(count + l, run);
      open_l = last_l;
      open_n = 64 - top;
    }
  }
  if (lane == 0 && open_l >= 0) atomicAdd(count + open_l, open_n);
}

static bool ms_aligned(const void* p) { return p != nullptr && ((uintptr_t)p % 4) == 0; }

static bool ms_apart(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + na <= b0 || b0 + nb <= a0;
}

static dim3 ms_grid(int64_t n) { return dim3((unsigned)min((int64_t)MS_MAX_BLOCKS, (n + MS_THREADS - 1) / MS_THREADS)); }

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_mesh_hook(void* stream, int V, int F, const int32_t* faces, int32_t* parent, int32_t* flag) {
  CLMGS_CHECK_ARG(V >= 1 && F >= 1);
  CLMGS_CHECK_ARG(ms_aligned(faces) && ms_aligned(parent) && ms_aligned(flag));
  const uint64_t fbytes = (uint64_t)F * 12, pbytes = (uint64_t)V * 4;
  CLMGS_CHECK_ARG(ms_apart(parent, pbytes, faces, fbytes) && ms_apart(flag, 4, faces, fbytes) &&
                  ms_apart(flag, 4, parent, pbytes));
  hipLaunchKernelGGL(mesh_hook_kernel, ms_grid(F), dim3(MS_THREADS), 0, (hipStream_t)stream, faces, F, V, parent, flag);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_shortcut(void* stream, int V, int32_t* parent, int32_t* flag) {
  CLMGS_CHECK_ARG(V >= 1);
  CLMGS_CHECK_ARG(ms_aligned(parent) && ms_aligned(flag) && ms_apart(flag, 4, parent, (uint64_t)V * 4));
  hipLaunchKernelGGL(mesh_shortcut_kernel, ms_grid(V), dim3(MS_THREADS), 0, (hipStream_t)stream, V, parent, flag);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mesh_component_faces(void* stream, int V, int F, const int32_t* faces, const int32_t* labels,
                                          int32_t* count) {
  CLMGS_CHECK_ARG(V >= 1 && F >= 1);
  CLMGS_CHECK_ARG(ms_aligned(faces) && ms_aligned(labels) && ms_aligned(count));
  const uint64_t fbytes = (uint64_t)F * 12, vbytes = (uint64_t)V * 4;
  CLMGS_CHECK_ARG(ms_apart(count, vbytes, faces, fbytes) && ms_apart(count, vbytes, labels, vbytes));
  hipLaunchKernelGGL(mesh_component_faces_kernel, ms_grid(F), dim3(MS_THREADS), 0, (hipStream_t)stream, faces, F, V, labels,
                     count);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
