// Per-Gaussian blend weights of a set of views (gfx950): what each Gaussian contributes to the images, for contribution
// pruning (Mini-Splatting / LightGaussian: sum of w = alpha * T; RadSplat: max of w).  A forward-only pass of its own,
// off the training step; the two shipped tile kernels of rasterize.hip are not involved.
//
// One 64-lane wave per 16x16 tile walks the tile's depth-ordered list front to back with the rules of
// rasterize_fwd_kernel -- the same scaled_sigma, sigma >= 0 test, 0.999 clamp, alpha >= 1/255 cut, stop before
// T <= 1e-4, quadrant culling, per-quadrant termination and two-deep staging (raster_tile.h) -- but carries no colours:
// per pixel it holds T only.  For every entry it forms, over the in-image pixels at which the forward accumulates that
// entry (its mask acc_m):
//   S = sum of alpha * T     (per lane over its <= 4 pixels in quadrant order, then one DPP chain: a fixed order)
//   M = max of alpha * T     (a second DPP chain)
//   P = number of such pixels (popcount of the scalar masks: no vector work)
// and 64 entries at a time, by 64 lanes, adds them into three caller-owned arrays with INTEGER atomics only, so the
// arrays are bit-reproducible whatever the order of the tiles, launches and cameras:
//   wsum_q    uint64  += round_to_nearest(S * 2^28)   (S <= 256: below 2^36, the scaling is exact; unit 3.7e-9)
//   wmax_bits uint32  max= bits(M)                    (M >= 0: the order of the bit patterns is the order of the floats)
//   pixels    uint64  += P
// Entries that are culled, never reached or valid at no pixel touch nothing.
//
// Records: 32 B {x, y, opacity, conic.a | conic.b, conic.c, -, -} packed into caller scratch by a pass of this file.  The
// staging lane needs 6 floats: a 32 B record is one aligned half of a 64 B line, so the gather moves half the bytes of the
// rasterizer's 64 B line, and no colour array has to exist (the scoring pass never evaluates SH).
#include "common.h"
#include "gs_math.h"
#include "raster_tile.h"

namespace clmgs {

constexpr int CREC_F4 = 2;            // float4 per contribution record
constexpr float WSUM_SCALE = 268435456.f;  // 2^28

__global__ void __launch_bounds__(256)
contrib_pack_kernel(int64_t n, const float* __restrict__ means2d, const float* __restrict__ conics,
                    const float* __restrict__ opacities, float4* __restrict__ packed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float2 m = *reinterpret_cast<const float2*>(means2d + 2 * i);
    const float* cn = conics + 3 * i;
    float4* rec = packed + CREC_F4 * i;
    rec[0] = make_float4(m.x, m.y, opacities[i], cn[0]);
    rec[1] = make_float4(cn[1], cn[2], 0.f, 0.f);
  }
}

// List entry idx of a tile of the camera whose rows are [cam_base, cam_base + N): its id, or -1 past the end of the list
// (and for an id that is not a row of that camera: such an entry reads and writes nothing).
__device__ __forceinline__ int contrib_id(const int32_t* __restrict__ flatten_ids, int idx, int re, int cam_base, int N) {
  if (idx >= re) return -1;
  const int id = flatten_ids[idx];
  return ((unsigned)(id - cam_base) < (unsigned)N) ? id : -1;
}

// Gather of record g and of its destination row (g < 0: neither, both keep their values).  g = cam * N + row of the camera.
__device__ __forceinline__ void contrib_gather(Rec& r, long long& dst, const float4* __restrict__ packed,
                                               const int64_t* __restrict__ rows, int g, int cam_base) {
  if (g >= 0) {
    const float4* rec = packed + CREC_F4 * (size_t)g;
    r.A = rec[0]; r.B = rec[1];
    dst = rows ? (long long)rows[g - cam_base] : (long long)g;
  }
}

struct ContribLds {
  float4 a[64];     // x, y, opacity, conic.a (pre-scaled)
  float2 b[64];     // conic.b, conic.c (pre-scaled)
  int meta[64];     // (offset in staging round << 4) | quadrant mask
  long long dst[64];  // destination row of the compacted slot
  float s[64], m[64];  // the wave-wide sum and maximum of the entry
  int p[64];           // its pixel count
};

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_max(float v) {  // v >= 0: a masked-off or out-of-row source reads 0
  const int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true);
  return fmaxf(v, __int_as_float(r));
}
// lane 63 holds the maximum of the wave (values >= 0); the lane order of wave_sum_to_lane63
__device__ __forceinline__ float wave_max_to_lane63(float v) {
  v = dpp_max<0x111>(v);
  v = dpp_max<0x112>(v);
  v = dpp_max<0x114>(v);
  v = dpp_max<0x118>(v);
  v = dpp_max<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
  v = dpp_max<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}

// 8 waves per SIMD: without colour accumulators the kernel fits their 64 VGPRs with no spill (the forward: 80 at 6)
__global__ void __launch_bounds__(64, 8)
rasterize_contrib_kernel(int C, int N, int64_t n_isects, const float4* __restrict__ packed,
                         int W, int H, int tile_w, int tile_h, const int32_t* __restrict__ offsets,
                         const int32_t* __restrict__ flatten_ids, const int64_t* __restrict__ rows, int64_t n_out,
                         unsigned long long* __restrict__ wsum_q, unsigned int* __restrict__ wmax_bits,
                         unsigned long long* __restrict__ pixels) {
  __shared__ ContribLds sm;
  const TileGeom g(C, tile_w, tile_h);
  const int lane = g.lane;
  const int cam_base = g.cam * N;
  const float px0 = g.px0, py0 = g.py0;

  // "this pixel still accumulates" is the SIGN of T, as in the forward: a terminated or out-of-image pixel holds -T
  float T[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    size_t pix;
    T[k] = g.pixel_of(k, W, H, pix) ? 1.f : -1.f;
  }

  int rs, re;
  tile_range(offsets, g.tile, g.n_tiles_total, n_isects, rs, re);

  // two-deep staging (see the forward): ids two rounds ahead of the blend loop, records and destination rows one
  Rec nxt = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};
  long long nxt_dst = 0;
  int cur_g = contrib_id(flatten_ids, rs + lane, re, cam_base, N);
  int nxt_g = contrib_id(flatten_ids, rs + 64 + lane, re, cam_base, N);
  contrib_gather(nxt, nxt_dst, packed, rows, cur_g, cam_base);
  int alive = 0;
#pragma unroll
  for (int k = 0; k < PPL; ++k) alive |= wave_any(T[k] > 0.f) ? (1 << k) : 0;
  for (int bs = rs; bs < re; bs += 64) {
    if (!alive) break;
    const Rec cur = nxt;
    const long long cur_dst = nxt_dst;
    const int mask = (cur_g >= 0) ? (quadrant_mask(cur, g.x0, g.y0) & alive) : 0;
    cur_g = nxt_g;
    contrib_gather(nxt, nxt_dst, packed, rows, cur_g, cam_base);
    nxt_g = contrib_id(flatten_ids, bs + 128 + lane, re, cam_base, N);
    int bn;
    const int pos = wave_compact(mask != 0, lane, bn);
    __syncthreads();
    if (mask) {
      sm.a[pos] = make_float4(cur.A.x, cur.A.y, cur.A.z, cur.A.w * CONIC_DIAG);
      sm.b[pos] = make_float2(cur.B.x * LOG2E, cur.B.y * CONIC_DIAG);
      sm.meta[pos] = (lane << 4) | mask;
      sm.dst[pos] = cur_dst;
    }
    __syncthreads();
    unsigned long long touched = 0ull;
    for (int t = 0; t < bn; ++t) {
      const float4 RA = sm.a[t];
      const float2 RB = sm.b[t];
      const int meta = __builtin_amdgcn_readfirstlane(sm.meta[t]);
      float s_l = 0.f, m_l = 0.f;
      int np = 0;  // wave-uniform
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (meta & alive & (1 << k)) {  // wave-uniform: this quadrant can be touched and still accumulates
          const float dx = RA.x - (px0 + (float)(8 * (k & 1)));
          const float dy = RA.y - (py0 + (float)(8 * (k >> 1)));
          const float sigma = scaled_sigma(RA.w, RB.x, RB.y, dx, dy);  // log2(e) * sigma
          const float alpha = fminf(0.999f, RA.z * __builtin_amdgcn_exp2f(-sigma));
          const float next_T = T[k] * (1.f - alpha);
          const unsigned long long hit_m = __builtin_amdgcn_ballot_w64(sigma >= 0.f) & __builtin_amdgcn_ballot_w64(alpha >= ALPHA_MIN);
          const unsigned long long go_m = __builtin_amdgcn_ballot_w64(next_T > T_EPS);
          const unsigned long long acc_m = hit_m & go_m, stop_m = hit_m & ~go_m;
          float vis = alpha * T[k];
          asm("v_cndmask_b32_e64 %0, 0, %0, %1" : "+v"(vis) : "s"(acc_m));
          s_l += vis;
          m_l = fmaxf(m_l, vis);
          np += __popcll(acc_m);
          asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(T[k]) : "v"(next_T), "s"(acc_m));
          if (stop_m != 0ull) {  // rare: the sign of T set under a narrowed exec mask (see the forward)
            unsigned long long exec_keep;
            asm volatile("s_mov_b64 %1, exec\n\ts_and_b64 exec, exec, %2\n\t"
                         "v_or_b32_e32 %0, 0x80000000, %0\n\ts_mov_b64 exec, %1"
                         : "+v"(T[k]), "=&s"(exec_keep) : "s"(stop_m) : "scc");
            if (__builtin_amdgcn_ballot_w64(T[k] > 0.f) == 0ull) alive &= ~(1 << k);
          }
        }
      }
      if (np != 0) {  // wave-uniform
        const float s_w = wave_sum_to_lane63(s_l);
        const float m_w = wave_max_to_lane63(m_l);
        if (lane == 63) { sm.s[t] = s_w; sm.m[t] = m_w; sm.p[t] = np; }
        touched |= (1ull << t);
      }
      if (!alive) break;
    }
    __syncthreads();
    if ((touched >> lane) & 1ull) {  // lane e flushes entry e of the round: three integer atomics
      const long long d = sm.dst[lane];
      if ((unsigned long long)d < (unsigned long long)n_out) {  // a row outside the caller's arrays is dropped
        atomicAdd(wsum_q + d, (unsigned long long)__float2ll_rn(sm.s[lane] * WSUM_SCALE));
        atomicMax(wmax_bits + d, __float_as_uint(sm.m[lane]));
        atomicAdd(pixels + d, (unsigned long long)sm.p[lane]);
      }
    }
  }
}

}  // namespace clmgs

using namespace clmgs;

extern "C" size_t clmgs_rasterize_contrib_pack_bytes(int C, int N) {
  const size_t n = (size_t)(C > 0 ? C : 0) * (size_t)(N > 0 ? N : 0);
  return (n ? n : 1) * CREC_F4 * sizeof(float4);
}

extern "C" int clmgs_rasterize_contrib(void* stream, int C, int N, int64_t n_isects, const float* means2d,
                                       const float* conics, const float* opacities, int width, int height,
                                       int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                                       const int32_t* flatten_ids, const int64_t* rows, int64_t n_out, void* packed,
                                       uint64_t* wsum_q, uint32_t* wmax_bits, uint64_t* pixels) {
  CLMGS_CHECK_ARG(tile_size == TILE);
  CLMGS_CHECK_ARG(C >= 1 && N >= 0 && width > 0 && height > 0 && tile_width * TILE >= width &&
                  tile_height * TILE >= height);
  CLMGS_CHECK_ARG(n_isects >= 0 && n_isects <= INT32_MAX && (int64_t)C * N <= INT32_MAX);
  CLMGS_CHECK_ARG(offsets && wsum_q && wmax_bits && pixels);
  CLMGS_CHECK_ARG(n_out >= 1 && (rows || n_out >= (int64_t)C * N));
  CLMGS_CHECK_ARG(n_isects == 0 || (flatten_ids && packed && means2d && conics && opacities));
  CLMGS_CHECK_ARG(((uintptr_t)packed & 31) == 0);
  const int64_t CN = (int64_t)C * N;
  if (n_isects == 0 || CN == 0) return 0;  // nothing listed: nothing is written
  hipStream_t s = (hipStream_t)stream;
  const dim3 pgrid(min(ceil_div(CN, 256), 256 * 8));
  hipLaunchKernelGGL(contrib_pack_kernel, pgrid, dim3(256), 0, s, CN, means2d, conics, opacities, (float4*)packed);
  CLMGS_LAUNCH_CHECK();
  const int n_blocks = C * tile_width * tile_height;
  hipLaunchKernelGGL(rasterize_contrib_kernel, dim3(n_blocks), dim3(64), 0, s, C, N, n_isects, (const float4*)packed,
                     width, height, tile_width, tile_height, offsets, flatten_ids, rows, n_out,
                     (unsigned long long*)wsum_q, (unsigned int*)wmax_bits, (unsigned long long*)pixels);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
