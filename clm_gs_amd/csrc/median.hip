// Median depth of a set of views (gfx950): per pixel, the camera-space depth and the row of the Gaussian at which the
// transmittance falls through one half -- the surface depth 2DGS, RaDe-GS and GOF extract meshes from.  A forward-only
// pass of its own, not differentiable; the two shipped tile kernels of rasterize.hip are not involved.
//
// One 64-lane wave per 16x16 tile walks the tile's depth-ordered list front to back with the rules of
// rasterize_fwd_kernel -- the same scaled_sigma, sigma >= 0 test, 0.999 clamp, alpha >= 1/255 cut, quadrant culling,
// per-quadrant termination and two-deep staging (raster_tile.h) -- but carries no colours: per pixel it holds T and the
// depth and id of the current median candidate.  The MEDIAN ENTRY of a pixel is the last accumulated entry whose
// transmittance before blending it is > 0.5: the entry at which T crosses one half, or the pixel's last contributor
// where T stays above it.  Per (entry, quadrant) the scalar mask  sigma >= 0 & alpha >= 1/255 & T > 0.5  selects the
// entry's depth and id into the candidate and T (1 - alpha) into T; a pixel that has fallen to T <= 0.5 is never
// touched again.  No wave-wide reductions, no atomics, no scratch.
//
// Why the forward's "stop before T <= 1e-4" rule does not appear: while T > 0.5 before an entry, alpha <= 0.999 leaves
// T >= 0.5 * 0.001 = 5e-4 > 1e-4 after it, so that rule can never fire at or before the median entry.  The pass
// therefore needs neither that test nor the exec-narrowing sign trick of the forward and of contrib.hip: "this pixel is
// still open" is simply T > 0.5 (an out-of-image pixel starts at a negative T), a quadrant is finished when no lane of
// it is open, and the wave when no quadrant is -- after a PREFIX of the list (the forward goes on to T <= 1e-4).
//
// Outputs: median_depth[C,H,W] (the depth of that entry, copied, not computed) and median_id[C,H,W] (its row within its
// camera, flatten_id - cam * N); 0.0 and -1 where nothing is accumulated.  Every in-image pixel of every tile is
// written exactly once at the end, empty tiles included.
//
// Records: 32 B {x, y, opacity, conic.a | conic.b, conic.c, depth, -} packed into caller scratch by a pass of this file:
// the staging lane's gather is one aligned half of a 64 B line, and no colour array has to exist.
#include "common.h"
#include "gs_math.h"
#include "raster_tile.h"

namespace clmgs {

constexpr int MREC_F4 = 2;  // float4 per median record
constexpr float T_HALF = 0.5f;

__global__ void __launch_bounds__(256)
median_pack_kernel(int64_t n, const float* __restrict__ means2d, const float* __restrict__ conics,
                   const float* __restrict__ opacities, const float* __restrict__ depths, float4* __restrict__ packed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float2 m = *reinterpret_cast<const float2*>(means2d + 2 * i);
    const float* cn = conics + 3 * i;
    float4* rec = packed + MREC_F4 * i;
    rec[0] = make_float4(m.x, m.y, opacities[i], cn[0]);
    rec[1] = make_float4(cn[1], cn[2], depths[i], 0.f);
  }
}

// nothing listed: every pixel holds "no entry"
__global__ void __launch_bounds__(256)
median_fill_kernel(int64_t n, float* __restrict__ median_depth, int32_t* __restrict__ median_id) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    median_depth[i] = 0.f;
    median_id[i] = -1;
  }
}

// List entry idx of a tile of the camera whose rows are [cam_base, cam_base + N): its id, or -1 past the end of the list
// (and for an id that is not a row of that camera: such an entry reads and writes nothing).
__device__ __forceinline__ int median_list_id(const int32_t* __restrict__ flatten_ids, int idx, int re, int cam_base, int N) {
  if (idx >= re) return -1;
  const int id = flatten_ids[idx];
  return ((unsigned)(id - cam_base) < (unsigned)N) ? id : -1;
}

// Gather of record g (g < 0: no record, `r` keeps its value); the depth rides in B.z
__device__ __forceinline__ void median_gather(Rec& r, const float4* __restrict__ packed, int g) {
  if (g >= 0) {
    const float4* rec = packed + MREC_F4 * (size_t)g;
    r.A = rec[0]; r.B = rec[1];
  }
}

struct MedianLds {
  float4 a[64];   // x, y, opacity, conic.a (pre-scaled)
  float4 b[64];   // conic.b, conic.c (pre-scaled), depth, bits of the row within the camera
  int meta[64];   // (offset in staging round << 4) | quadrant mask
};

// 8 waves per SIMD: three values per pixel fit their 64 VGPRs with no spill (the forward: 80 at 6)
__global__ void __launch_bounds__(64, 8)
rasterize_median_kernel(int C, int N, int64_t n_isects, const float4* __restrict__ packed, int W, int H, int tile_w,
                        int tile_h, const int32_t* __restrict__ offsets, const int32_t* __restrict__ flatten_ids,
                        float* __restrict__ median_depth, int32_t* __restrict__ median_id) {
  __shared__ MedianLds sm;
  const TileGeom g(C, tile_w, tile_h);
  const int lane = g.lane;
  const int cam_base = g.cam * N;
  const float px0 = g.px0, py0 = g.py0;

  // per pixel: T (negative outside the image: never open), the candidate's depth and row
  float T[PPL], md[PPL];
  int mi[PPL];
  unsigned long long open_m[PPL];  // scalar: the lanes whose pixel of quadrant k still has T > 0.5
  int alive = 0;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    size_t pix;
    T[k] = g.pixel_of(k, W, H, pix) ? 1.f : -1.f;
    md[k] = 0.f;
    mi[k] = -1;
    open_m[k] = __builtin_amdgcn_ballot_w64(T[k] > T_HALF);
    alive |= (open_m[k] != 0ull) ? (1 << k) : 0;
  }

  int rs, re;
  tile_range(offsets, g.tile, g.n_tiles_total, n_isects, rs, re);

  // two-deep staging (see the forward): ids two rounds ahead of the blend loop, records one
  Rec nxt = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};
  int cur_g = median_list_id(flatten_ids, rs + lane, re, cam_base, N);
  int nxt_g = median_list_id(flatten_ids, rs + 64 + lane, re, cam_base, N);
  median_gather(nxt, packed, cur_g);
  for (int bs = rs; bs < re; bs += 64) {
    if (!alive) break;
    const Rec cur = nxt;
    const int cur_row = cur_g - cam_base;
    // The tile corner is re-made from its scalar integers every round: left to itself the compiler hoists the eight
    // corner offsets of quadrant_mask out of the loop into VGPRs that live through the blend loop, and spills five.
    int cx = g.tx * TILE, cy = g.ty * TILE;
    asm volatile("" : "+s"(cx), "+s"(cy));
    const int mask = (cur_g >= 0) ? (quadrant_mask(cur, (float)cx, (float)cy) & alive) : 0;
    cur_g = nxt_g;
    median_gather(nxt, packed, cur_g);
    nxt_g = median_list_id(flatten_ids, bs + 128 + lane, re, cam_base, N);
    int bn;
    const int pos = wave_compact(mask != 0, lane, bn);
    __syncthreads();
    if (mask) {
      sm.a[pos] = make_float4(cur.A.x, cur.A.y, cur.A.z, cur.A.w * CONIC_DIAG);
      sm.b[pos] = make_float4(cur.B.x * LOG2E, cur.B.y * CONIC_DIAG, cur.B.z, __int_as_float(cur_row));
      sm.meta[pos] = (lane << 4) | mask;
    }
    __syncthreads();
    for (int t = 0; t < bn; ++t) {
      const float4 RA = sm.a[t];
      const float4 RB = sm.b[t];
      const int meta = __builtin_amdgcn_readfirstlane(sm.meta[t]);
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (meta & alive & (1 << k)) {  // wave-uniform: this quadrant can be touched and has an open pixel
          const float dx = RA.x - (px0 + (float)(8 * (k & 1)));
          const float dy = RA.y - (py0 + (float)(8 * (k >> 1)));
          const float sigma = scaled_sigma(RA.w, RB.x, RB.y, dx, dy);  // log2(e) * sigma
          const float alpha = fminf(0.999f, RA.z * __builtin_amdgcn_exp2f(-sigma));
          const float next_T = T[k] * (1.f - alpha);
          // accumulated here and T > 0.5 before it: the new median candidate of those pixels
          const unsigned long long acc_m = __builtin_amdgcn_ballot_w64(sigma >= 0.f) &
                                           __builtin_amdgcn_ballot_w64(alpha >= ALPHA_MIN) & open_m[k];
          asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(md[k]) : "v"(RB.z), "s"(acc_m));
          asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(mi[k]) : "v"(__float_as_int(RB.w)), "s"(acc_m));
          asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(T[k]) : "v"(next_T), "s"(acc_m));
          open_m[k] = __builtin_amdgcn_ballot_w64(T[k] > T_HALF);
          if (open_m[k] == 0ull) alive &= ~(1 << k);
        }
      }
      if (!alive) break;
    }
  }

#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    size_t pix;
    if (g.pixel_of(k, W, H, pix)) {
      median_depth[pix] = md[k];
      median_id[pix] = mi[k];
    }
  }
}

}  // namespace clmgs

using namespace clmgs;

extern "C" size_t clmgs_rasterize_median_pack_bytes(int C, int N) {
  const size_t n = (size_t)(C > 0 ? C : 0) * (size_t)(N > 0 ? N : 0);
  return (n ? n : 1) * MREC_F4 * sizeof(float4);
}

extern "C" int clmgs_rasterize_median(void* stream, int C, int N, int64_t n_isects, const float* means2d,
                                      const float* conics, const float* opacities, const float* depths, int width,
                                      int height, int tile_size, int tile_width, int tile_height,
                                      const int32_t* offsets, const int32_t* flatten_ids, void* packed,
                                      float* median_depth, int32_t* median_id) {
  CLMGS_CHECK_ARG(tile_size == TILE);
  CLMGS_CHECK_ARG(C >= 1 && N >= 0 && width > 0 && height > 0 && tile_width * TILE >= width &&
                  tile_height * TILE >= height);
  CLMGS_CHECK_ARG(n_isects >= 0 && n_isects <= INT32_MAX && (int64_t)C * N <= INT32_MAX);
  CLMGS_CHECK_ARG((int64_t)C * tile_width * tile_height <= INT32_MAX);
  CLMGS_CHECK_ARG(offsets && median_depth && median_id);
  CLMGS_CHECK_ARG(n_isects == 0 || (flatten_ids && packed && means2d && conics && opacities && depths));
  CLMGS_CHECK_ARG(((uintptr_t)packed & 31) == 0);
  const int64_t CN = (int64_t)C * N;
  hipStream_t s = (hipStream_t)stream;
  if (n_isects == 0 || CN == 0) {  // nothing listed: no pixel has an entry
    const int64_t n_pix = (int64_t)C * height * width;
    const dim3 fgrid(min(ceil_div(n_pix, 256), 256 * 8));
    hipLaunchKernelGGL(median_fill_kernel, fgrid, dim3(256), 0, s, n_pix, median_depth, median_id);
    CLMGS_LAUNCH_CHECK();
    return 0;
  }
  const dim3 pgrid(min(ceil_div(CN, 256), 256 * 8));
  hipLaunchKernelGGL(median_pack_kernel, pgrid, dim3(256), 0, s, CN, means2d, conics, opacities, depths, (float4*)packed);
  CLMGS_LAUNCH_CHECK();
  const int n_blocks = C * tile_width * tile_height;
  hipLaunchKernelGGL(rasterize_median_kernel, dim3(n_blocks), dim3(64), 0, s, C, N, n_isects, (const float4*)packed,
                     width, height, tile_width, tile_height, offsets, flatten_ids, median_depth, median_id);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
