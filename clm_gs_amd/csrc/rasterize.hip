// Per-tile front-to-back alpha blending and its VJP (gfx950).
// Replaces gsplat.rasterize_to_pixels forward + autograd backward
// (strategies/base_engine.py:192-203, strategies/no_offload/engine.py:86-97,
// strategies/clm_offload/engine.py:106-117; arithmetic: SURVEY.md A5/A6).
//
// CDNA4 mapping -- NOT the 16x16-threads-per-tile CUDA shape:
//   * one 64-lane wavefront owns one 16x16 tile; every lane carries 4 pixels, one in each 8x8
//     quadrant (lane = 8x8 position).  A tile's Gaussian record is read from LDS once per wave
//     and reused for up to 4 pixels per lane: LDS traffic per pixel-Gaussian pair is 1/4 of a
//     thread-per-pixel kernel, there is no multi-wave barrier, and the independent pixels give
//     the exp/fma chain ILP;
//   * exact sub-tile culling: the staging lane computes, from the conic and opacity, the exact
//     minimum of sigma over each 8x8 quadrant and a 4-bit mask of the quadrants where
//     alpha >= 1/255 is reachable.  Records whose box
//     misses the tile are compacted away with a ballot/popcount prefix (depth order kept),
//     quadrants it misses are skipped with wave-uniform branches.  Only pairs the reference
//     itself skips (alpha < 1/255) are dropped, so results are unchanged;
//   * backward: each lane first sums its pixels' contributions; the nine wave-wide sums of an entry then go
//     through LDS (eight of them, transposed: four ds_write2st64 + two ds_read_b128 + 7 adds + 3 DPP adds per
//     lane) and one DPP chain (the ninth), and ONE 64 B partial line per (Gaussian, tile) leaves the wave
//     (engine path: plain stores at the intersection's slot; gsplat-compatible op: float atomics), 64
//     Gaussians at a time by 64 lanes;
//   * both tile kernels are templates on the number of blended channels: 3, or 4 for gsplat's depth modes
//     (rasterize_to_pixels with colors[..., 4]: clmgs_rasterize4_fwd / _bwd).  The fourth channel rides in the record's
//     spare word, takes one more accumulator per pixel in the forward and a tenth wave-wide sum (a second DPP chain) and
//     a tenth atomic (atomic route) or word 9 of the stored line (slot route) in the backward; the 3-channel
//     instantiations are, instruction for instruction, the kernels they were without the parameter (DESIGN.md section 3,
//     "Depth");
//   * the backward is also a template on ABS, gsplat's absgrad (clmgs_rasterize_abs_bwd / _abs_bwd_dev): two more per-lane
//     accumulators of the per-pixel |dL_p/dmean2d|, two more DPP chains per entry, words 10 and 11 of the 64 B line; the
//     plain instantiations are, instruction for instruction, the kernels they were ("Absgrad");
//   * blockIdx -> tile mapping is XCD-aware: each XCD's L2 sees a contiguous stripe of tiles,
//     so neighbouring tiles' shared Gaussians hit in L2.
#include "common.h"
#include "gs_math.h"
#include "raster_tile.h"

namespace clmgs {

// NCH (3 or 4) = blended channels.  Everything the fourth channel adds is under `if constexpr (NCH == 4)`; the
// 3-channel instantiations compile to the code they were before the parameter existed.
template <int NCH>
__global__ void __launch_bounds__(256)
raster_pack_kernel(int64_t n, const float* __restrict__ means2d, const float* __restrict__ conics,
                   const float* __restrict__ colors, const float* __restrict__ opacities,
                   float4* __restrict__ packed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float2 m = *reinterpret_cast<const float2*>(means2d + 2 * i);
    const float* cn = conics + 3 * i;
    const float* cl = colors + NCH * i;
    float4* rec = packed + REC_F4 * i;
    rec[0] = make_float4(m.x, m.y, opacities[i], cn[0]);
    rec[1] = make_float4(cn[1], cn[2], cl[0], cl[1]);
    rec[2] = make_float4(cl[2], NCH == 4 ? cl[NCH - 1] : 0.f, 0.f, 0.f);
  }
}

// packed_grad line: x y ca cb | cc r g b | o d ax ay | -   (d: NCH = 4 only; ax ay: ABS only, the absgrad pair)
template <int NCH>
__global__ void __launch_bounds__(256)
raster_unpack_grad_kernel(int64_t n, const float4* __restrict__ packed_grad,
                          float* __restrict__ v_means2d, float* __restrict__ v_conics,
                          float* __restrict__ v_colors, float* __restrict__ v_opacities) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = packed_grad[REC_F4 * i], b = packed_grad[REC_F4 * i + 1];
    const float4 c = packed_grad[REC_F4 * i + 2];
    *reinterpret_cast<float2*>(v_means2d + 2 * i) = make_float2(a.x, a.y);
    v_conics[3 * i] = a.z; v_conics[3 * i + 1] = a.w; v_conics[3 * i + 2] = b.x;
    v_colors[NCH * i] = b.y; v_colors[NCH * i + 1] = b.z; v_colors[NCH * i + 2] = b.w;
    if constexpr (NCH == 4) v_colors[NCH * i + 3] = c.y;
    v_opacities[i] = c.x;
  }
}
// ... and the absgrad pair of the same lines to v_means2d_abs [n,2].  Its own kernel: one more argument, or a shared
// body, moved the plain kernel's instructions.
__global__ void __launch_bounds__(256)
raster_unpack_abs_kernel(int64_t n, const float4* __restrict__ packed_grad, float* __restrict__ v_means2d_abs) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 c = packed_grad[REC_F4 * i + 2];
    *reinterpret_cast<float2*>(v_means2d_abs + 2 * i) = make_float2(c.z, c.w);
  }
}

// waves/SIMD the forward is compiled for: 6 (80 VGPRs, six spilled dwords) measured 0.940 vs 0.970 ms at 5
// (87 VGPRs); 7 / 8 (more spills) 0.934 / 0.925 -- the issue rate of one-wave workgroups grows with the
// resident waves (profiles/ilp_probe.hip), the spills eat most of it
#ifndef CLMGS_FWD_WAVES
#define CLMGS_FWD_WAVES 6
#endif
// ... and the 4-channel forward: its four extra accumulators do not fit the 80 VGPRs of 6 waves without spills
#ifndef CLMGS_FWD4_WAVES
#define CLMGS_FWD4_WAVES 5
#endif
template <int NCH>
__global__ void __launch_bounds__(64, NCH == 4 ? CLMGS_FWD4_WAVES : CLMGS_FWD_WAVES)
rasterize_fwd_kernel(int C, int N, int64_t n_isects, const float4* __restrict__ packed,
                     const float* __restrict__ backgrounds,
                     int W, int H, int tile_w, int tile_h, const int32_t* __restrict__ offsets,
                     const int32_t* __restrict__ flatten_ids, float* __restrict__ render_colors,
                     float* __restrict__ render_alphas, int32_t* __restrict__ last_ids,
                     const int64_t* __restrict__ n_dev) {
  static_assert(NCH == 3 || NCH == 4, "3 or 4 blended channels");
  __shared__ TileLds<NCH> sm;
  if (n_dev) n_isects = min(n_isects, *n_dev);  // device-side count (the launch was prepared for a capacity)
  const TileGeom g(C, tile_w, tile_h);
  const int lane = g.lane, cam = g.cam;
  const float px0 = g.px0, py0 = g.py0;

  // Per-pixel state kept lean (the VGPR budget decides the waves per SIMD, and the issue rate of one-wave
  // workgroups grows with them): pixel centres are recomputed from the lane, and "this pixel still
  // accumulates" is the SIGN of T (T > 1e-4 while alive; a terminated or out-of-image pixel holds -T).
  float T[PPL], cr[PPL], cg[PPL], cb[PPL], cd[PPL];
  int last[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    size_t pix;
    cr[k] = cg[k] = cb[k] = cd[k] = 0.f; last[k] = 0;
    T[k] = g.pixel_of(k, W, H, pix) ? 1.f : -1.f;
  }

  int rs, re;
  tile_range(offsets, g.tile, g.n_tiles_total, n_isects, rs, re);

  // Software-pipelined staging: the id -> record gather of round r+1 is issued before round r's
  // blend loop and consumed after it, so its two dependent HBM/L2 latencies hide under compute.
  // Two-deep: ids run two rounds ahead of the blend loop, records one round ahead, so neither of
  // the two dependent gathers (id -> record) is ever waited for right after it is issued.
  Rec nxt = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};
  int cur_g = (rs + lane < re) ? flatten_ids[rs + lane] : -1;        // ids of round 0
  int nxt_g = (rs + 64 + lane < re) ? flatten_ids[rs + 64 + lane] : -1;  // ids of round 1
  gather_record<NCH>(nxt, packed, cur_g);
  // Per-quadrant termination (gsplat's per-pixel `done`, at the granularity this kernel branches on): bit k of
  // `alive` = some pixel of quadrant k still accumulates.  A quadrant whose 64 pixels have all terminated (or lie
  // outside the image) takes no further pass -- a pass over it changes nothing (`valid` needs T > 0) -- and an entry
  // that only reaches dead quadrants is not even staged.  Wave-uniform (SGPR), refreshed by the passes themselves.
  int alive = 0;
#pragma unroll
  for (int k = 0; k < PPL; ++k) alive |= __any(T[k] > 0.f) ? (1 << k) : 0;
  for (int bs = rs; bs < re; bs += 64) {
    if (!alive) break;
    const Rec cur = nxt;
    const int mask = (cur_g >= 0) ? (quadrant_mask(cur, g.x0, g.y0) & alive) : 0;
    cur_g = nxt_g;
    gather_record<NCH>(nxt, packed, cur_g);  // records of the next round (their ids arrived a round ago)
    {
      const int nidx = bs + 128 + lane;  // ids of the round after next
      nxt_g = (nidx < re) ? flatten_ids[nidx] : -1;
    }
    int bn;
    const int pos = wave_compact(mask != 0, lane, bn);
    __syncthreads();
    if (mask) sm.stage(pos, cur, (lane << 4) | mask);
    __syncthreads();
    for (int t = 0; t < bn; ++t) {
      const float4 RA = sm.a[t];
      const float4 RB = sm.b[t];
      const int meta = __builtin_amdgcn_readfirstlane(sm.meta[t]);
      const float rblue = sm.c[0][t];
      float rdep = 0.f;
      if constexpr (NCH == 4) rdep = sm.c[1][t];
      const int gi = bs + (meta >> 4);
      int gi_v;  // the wave-uniform index in a VGPR, once per entry (v_cndmask cannot take it as a scalar
      asm("v_mov_b32 %0, %1" : "=v"(gi_v) : "s"(gi));  // next to its mask; the compiler re-moved it per pass)
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        if (meta & alive & (1 << k)) {  // wave-uniform: this quadrant can be touched and still accumulates
          const float dx = RA.x - (px0 + (float)(8 * (k & 1)));
          const float dy = RA.y - (py0 + (float)(8 * (k >> 1)));
          const float sigma = scaled_sigma(RA.w, RB.x, RB.y, dx, dy);  // log2(e) * sigma
          const float alpha = fminf(0.999f, RA.z * __builtin_amdgcn_exp2f(-sigma));
          // Three compares and three selects per pass, and no scalar work beyond the mask arithmetic (compares, selects and
          // v_min issue at half the FMA rate: profiles/r06_valu_calib.jsonl).  A finished / out-of-image pixel holds a
          // NEGATIVE T, so its next_T < 0 fails `next_T > eps` by itself (no `T > 0` compare); the two outcomes of a hit are
          // mask arithmetic on the compares' scalar results (s_and / s_andn2; written with bools the compiler issued
          // v_cmp_nlt AND v_cmp_lt for `goes_on` / `!goes_on`); the selects are v_cndmask on those scalar masks.
          const float next_T = T[k] * (1.f - alpha);
          const unsigned long long hit_m = __builtin_amdgcn_ballot_w64(sigma >= 0.f) & __builtin_amdgcn_ballot_w64(alpha >= ALPHA_MIN);
          const unsigned long long go_m = __builtin_amdgcn_ballot_w64(next_T > T_EPS);
          const unsigned long long acc_m = hit_m & go_m, stop_m = hit_m & ~go_m;
          float vis = alpha * T[k];
          asm("v_cndmask_b32_e64 %0, 0, %0, %1" : "+v"(vis) : "s"(acc_m));
          cr[k] += RB.z * vis; cg[k] += RB.w * vis; cb[k] += rblue * vis;
          if constexpr (NCH == 4) cd[k] += rdep * vis;
          asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(last[k]) : "v"(gi_v), "s"(acc_m));
          asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(T[k]) : "v"(next_T), "s"(acc_m));
          if (stop_m != 0ull) {
            // rare (a pixel stops once; finished pixels of a part-finished quadrant come by again): the sign of T is set
            // under a narrowed exec mask -- one full-rate v_or here instead of a fourth select in every pass.  The live mask
            // is saved, narrowed and restored, so the block holds wherever the compiler places it.
            unsigned long long exec_keep;
            asm volatile("s_mov_b64 %1, exec\n\ts_and_b64 exec, exec, %2\n\t"
                         "v_or_b32_e32 %0, 0x80000000, %0\n\ts_mov_b64 exec, %1"
                         : "+v"(T[k]), "=&s"(exec_keep) : "s"(stop_m) : "scc");
            if (__builtin_amdgcn_ballot_w64(T[k] > 0.f) == 0ull) alive &= ~(1 << k);
          }
        }
      }
      if (!alive) break;
    }
  }

  float bgr = 0.f, bgg = 0.f, bgb = 0.f, bgd = 0.f;
  if (backgrounds) {
    bgr = backgrounds[NCH * cam]; bgg = backgrounds[NCH * cam + 1]; bgb = backgrounds[NCH * cam + 2];
    if constexpr (NCH == 4) bgd = backgrounds[NCH * cam + 3];
  }
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    size_t pix;
    if (g.pixel_of(k, W, H, pix)) {
      const float Tf = fabsf(T[k]);
      render_colors[NCH * pix] = cr[k] + Tf * bgr;
      render_colors[NCH * pix + 1] = cg[k] + Tf * bgg;
      render_colors[NCH * pix + 2] = cb[k] + Tf * bgb;
      if constexpr (NCH == 4) render_colors[NCH * pix + 3] = cd[k] + Tf * bgd;
      render_alphas[pix] = 1.f - Tf;
      last_ids[pix] = last[k];
    }
  }
}

template <int NCH>
struct TileLdsBwd : TileLds<NCH> {
  int id[64];        // Gaussian id (cam*N + g) of the compacted slot, or its emit slot (PART)
  __attribute__((aligned(16))) float acc[64][12];  // reduced per-Gaussian sums of this tile (6 + NCH used)
  __attribute__((aligned(16))) float red[8][64];   // transposed scratch of the wave-wide sums: [value][lane]
  // Moments -> gradients, both flush routes: words 0..3 of entry e's gradient line (x y ca cb) and word 4 (cc) from
  // acc[e] = {Sx Sy Sxx Sxy | Syy ..}, with the conic of the entry taken back from its pre-scaled form.
  __device__ __forceinline__ float4 grad_xy_conic(int e, float& g_cc) const {
    const float ca = this->a[e].w * CONIC_DIAG_INV, cb = this->b[e].x * CONIC_OFF_INV,
                cc = this->b[e].y * CONIC_DIAG_INV;
    const float* m = acc[e];
    g_cc = 0.5f * m[4];
    return make_float4(ca * m[0] + cb * m[1], cb * m[0] + cc * m[1], 0.5f * m[2], m[3]);
  }
};

#ifndef CLMGS_BWD_WAVES
#define CLMGS_BWD_WAVES 4  // 5 spills (96 VGPRs): scratch reloads force vmcnt(0) and kill the prefetch
#endif
// PART: atomic-free accumulation.  Every sorted intersection owns the line partials[slot] (PART_F4 float4 = 64 B)
// (slot = its emit index, see isect2_emit_kernel); the tile's wave STORES the reduced sums there
// (zeros for culled / unreached entries, so every line is written exactly once per launch) and
// raster_partials_sum_kernel adds each row's contiguous range.
// NCH = 4, both routes: a tenth sum g_d = sum fac * vd, at word 9 of the line: a tenth atomic, or the slot route's stored
// line  x y ca cb | cc r g b | o d - -  (zero lines stay zero).
// ABS (NCH = 3, both routes): gsplat's absgrad.  The kernel reduces MOMENTS of w = v_sigma and forms g_x = ca Sx + cb Sy
// once per entry, so the per-pixel |dL_p/dmean2d| = |w (ca dx + cb dy)|, |w (cb dx + cc dy)| is new arithmetic in the pass:
// two FMA pairs whose results enter their accumulators through the |.| input modifier, on the pre-scaled conic
// (a log2(e)/2, b log2(e)/2, c log2(e)/2: the positive factor 2/log2(e) is applied once, after the wave-wide sum).  The
// pair takes two more DPP chains next to g_o's and lands in words 10 and 11 of the line: x y ca cb | cc r g b | o - ax ay.
template <bool PART, int NCH, bool ABS = false>
__global__ void __launch_bounds__(64, CLMGS_BWD_WAVES)
rasterize_bwd_kernel(int C, int N, int64_t n_isects, const float4* __restrict__ packed,
                     const float* __restrict__ backgrounds,
                     int W, int H, int tile_w, int tile_h, const int32_t* __restrict__ offsets,
                     const int32_t* __restrict__ flatten_ids,
                     const float* __restrict__ render_alphas, const int32_t* __restrict__ last_ids,
                     const float* __restrict__ v_render_colors,
                     const float* __restrict__ v_render_alphas, float* __restrict__ packed_grad,
                     const int32_t* __restrict__ emit_slot, float4* __restrict__ partials,
                     const int64_t* __restrict__ n_dev) {
  static_assert(NCH == 3 || NCH == 4, "3 or 4 blended channels");
  static_assert(!ABS || NCH == 3, "absgrad: three channels only (word 9 stays the fourth channel's)");
  __shared__ TileLdsBwd<NCH> sm;
  if (n_dev) n_isects = min(n_isects, *n_dev);
  const TileGeom g(C, tile_w, tile_h);
  const int lane = g.lane, cam = g.cam;
  const float px0 = g.px0, py0 = g.py0;

  int rs, re;
  tile_range(offsets, g.tile, g.n_tiles_total, n_isects, rs, re);
  if (re <= rs) return;

  // per-pixel state kept lean (VGPR budget decides waves/SIMD): pixel centres are recomputed from
  // the lane, "inside" is bin < 0, and T_final * v_alpha' is pre-multiplied.
  // Bk = (colour accumulated behind the current Gaussian) . v_rgb  -  T_final * v_alpha': the
  // behind-colour only ever appears dotted with the pixel's colour cotangent, so ONE running
  // scalar replaces three buffers and the alpha-cotangent term (fewer VGPRs, 7 fewer VALU/pair).
  float T[PPL], Bk[PPL], vr[PPL], vg[PPL], vb[PPL];
  int bin[PPL];
  int max_bin = -1;
  int qmax[PPL];  // per quadrant: the deepest contributor of its 64 pixels (wave-uniform)
  float bgr = 0.f, bgg = 0.f, bgb = 0.f;
  if (backgrounds) { bgr = backgrounds[NCH * cam]; bgg = backgrounds[NCH * cam + 1]; bgb = backgrounds[NCH * cam + 2]; }
  float vd[PPL], bgd = 0.f;  // the fourth channel's cotangents and background (NCH = 4)
  if constexpr (NCH == 4) { if (backgrounds) bgd = backgrounds[NCH * cam + 3]; }
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    size_t pix;
    if (g.pixel_of(k, W, H, pix)) {
      const float Tf = 1.f - render_alphas[pix];
      bin[k] = last_ids[pix];
      vr[k] = v_render_colors[NCH * pix]; vg[k] = v_render_colors[NCH * pix + 1]; vb[k] = v_render_colors[NCH * pix + 2];
      vd[k] = 0.f;
      if constexpr (NCH == 4) vd[k] = v_render_colors[NCH * pix + 3];
      float va = v_render_alphas ? v_render_alphas[pix] : 0.f;
      // d(out)/d(T_final) through the background term folds into the alpha cotangent
      va -= (bgr * vr[k] + bgg * vg[k] + bgb * vb[k]);
      if constexpr (NCH == 4) va -= bgd * vd[k];
      Bk[k] = -Tf * va;
      T[k] = Tf;
      max_bin = max(max_bin, bin[k]);
    } else {
      T[k] = 1.f; bin[k] = -1; vr[k] = vg[k] = vb[k] = vd[k] = Bk[k] = 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < PPL; ++k) qmax[k] = __builtin_amdgcn_readfirstlane(wave_max_i32(bin[k]));
  max_bin = max(max(qmax[0], qmax[1]), max(qmax[2], qmax[3]));
  const int hi = min(re - 1, max_bin);  // nothing behind the deepest contributor matters

  // two-deep software-pipelined staging (see the forward kernel): ids two rounds ahead,
  // records one round ahead; nothing is waited for right after issue, and the waits never
  // include the previous round's atomics
  Rec nxt = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};
  int cur_g = (hi - lane >= rs) ? flatten_ids[hi - lane] : -1;
  int nxt_g = (hi - 64 - lane >= rs) ? flatten_ids[hi - 64 - lane] : -1;
  int cur_p = 0, nxt_p = 0;
  if (PART) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int idx = max(hi + 1, rs) + lane; idx < re; idx += 64) {  // behind the deepest contributor: zeros
      float4* dst = partials + PART_F4 * (size_t)emit_slot[idx];
#pragma unroll
      for (int q = 0; q < PART_F4; ++q) dst[q] = z4;
    }
    cur_p = (hi - lane >= rs) ? emit_slot[hi - lane] : 0;
    nxt_p = (hi - 64 - lane >= rs) ? emit_slot[hi - 64 - lane] : 0;
  }
  gather_record<NCH>(nxt, packed, cur_g);
  for (int bh = hi; bh >= rs; bh -= 64) {
    const Rec cur = nxt;
    const int gid = cur_g;
    const int pid = cur_p;
    // Per-quadrant termination: entry gi matters to quadrant k only while gi <= qmax[k] (`valid` needs
    // gi <= bin of the pixel); the staging lane drops the other quadrants from its mask, and an entry left
    // without a quadrant is not staged at all (its partial line is the zero line below).  Results unchanged.
    const int gidx = bh - lane;
    const int reach = (gidx <= qmax[0] ? 1 : 0) | (gidx <= qmax[1] ? 2 : 0) | (gidx <= qmax[2] ? 4 : 0) |
                      (gidx <= qmax[3] ? 8 : 0);
    const int mask = (gid >= 0) ? (quadrant_mask(cur, g.x0, g.y0) & reach) : 0;
    cur_g = nxt_g;
    cur_p = nxt_p;
    gather_record<NCH>(nxt, packed, cur_g);
    {
      const int nidx = bh - 128 - lane;
      nxt_g = (nidx >= rs) ? flatten_ids[nidx] : -1;
      if (PART) nxt_p = (nidx >= rs) ? emit_slot[nidx] : 0;
    }
    if (PART && gid >= 0 && mask == 0) {  // culled for this tile: its line is all zeros
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      float4* dst = partials + PART_F4 * (size_t)pid;
#pragma unroll
      for (int q = 0; q < PART_F4; ++q) dst[q] = z4;
    }
    int bn;
    const int pos = wave_compact(mask != 0, lane, bn);
    __syncthreads();
    if (mask) {
      sm.stage(pos, cur, (lane << META_SHIFT) | special_entry(cur.A.z, cur.A.w, cur.B.x, cur.B.y) | mask);
      sm.id[pos] = PART ? pid : gid;
    }
    __syncthreads();
    unsigned long long touched = 0ull;
    for (int t = 0; t < bn; ++t) {
      const float4 RA = sm.a[t];
      const float4 RB = sm.b[t];
      const int meta = __builtin_amdgcn_readfirstlane(sm.meta[t]);
      const float rblue = sm.c[0][t];
      float rdep = 0.f;
      if constexpr (NCH == 4) rdep = sm.c[1][t];
      const int gi = bh - (meta >> META_SHIFT);
      const bool special = (meta & META_SPECIAL) != 0;  // wave-uniform
      // moments of w = v_sigma over the tile: the five screen-space gradients are linear in them
      // (g_x = a Sx + b Sy, g_y = b Sx + c Sy, g_conic = Sxx/2, Sxy, Syy/2), applied at the flush
      float g_d = 0.f;  // NCH = 4: sum fac * vd
      float ax = 0.f, ay = 0.f, cbh = 0.f;  // ABS: sum |v_xy| on the pre-scaled conic, and its off-diagonal word halved
      if constexpr (ABS) cbh = 0.5f * RB.x;
      float g_r = 0.f, g_g = 0.f, g_b = 0.f, Sx = 0.f, Sy = 0.f, Sxx = 0.f, Sxy = 0.f, Syy = 0.f,
            g_o = 0.f;
      // OR of the passes' valid masks, kept as scalar mask arithmetic on the compares' results (a per-lane flag costs a
      // v_mov per pass and a v_cmp at the end; measured -0.8 % slab / -1.2 % heavy, profiles/r06_raster_ab8.txt)
      unsigned long long any_valid = 0ull;
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
          if (meta & (1 << k)) {  // wave-uniform
            const float dx = RA.x - (px0 + (float)(8 * (k & 1)));
            const float dy = RA.y - (py0 + (float)(8 * (k >> 1)));
            const float sigma = scaled_sigma(RA.w, RB.x, RB.y, dx, dy);  // log2(e) * sigma
            const float gex = __builtin_amdgcn_exp2f(-sigma);
            const float oa = RA.z * gex;
            // (scalar branches on `special`; the empty asm keeps them branches -- if-converted they are selects again)
            float alpha = oa;
            bool ok = true;
            unsigned long long ok_m = ~0ull;
            if (__builtin_expect(special, 0)) {
              asm volatile("");
              alpha = fminf(0.999f, oa); ok = sigma >= 0.f; ok_m = __builtin_amdgcn_ballot_w64(sigma >= 0.f);
            }
            const bool valid = ok & (gi <= bin[k]) & (alpha >= ALPHA_MIN);
            any_valid |= ok_m & __builtin_amdgcn_ballot_w64(gi <= bin[k]) & __builtin_amdgcn_ballot_w64(alpha >= ALPHA_MIN);
            if (valid) {
              const float ra = __builtin_amdgcn_rcpf(1.f - alpha);  // v_rcp_f32 (1 ulp), not the 10-op IEEE divide
              T[k] *= ra;
              const float fac = alpha * T[k];
              g_r += fac * vr[k]; g_g += fac * vg[k]; g_b += fac * vb[k];
              float cv = RB.z * vr[k] + RB.w * vg[k] + rblue * vb[k];
              if constexpr (NCH == 4) { g_d += fac * vd[k]; cv += rdep * vd[k]; }
              // a saturated alpha (o * G > 0.999, clamped; special entries only) passes no gradient to sigma / opacity
              float v_alpha = T[k] * cv - ra * Bk[k];
              if (__builtin_expect(special, 0)) { asm volatile(""); v_alpha = (oa <= 0.999f) ? v_alpha : 0.f; }
              const float w = -oa * v_alpha;  // v_sigma
              const float wdx = w * dx, wdy = w * dy;
              Sx += wdx; Sy += wdy;
              Sxx += wdx * dx; Sxy += wdx * dy; Syy += wdy * dy;
              if constexpr (ABS) { ax += fabsf(fmaf(RA.w, wdx, cbh * wdy)); ay += fabsf(fmaf(cbh, wdx, RB.y * wdy)); }
              g_o += gex * v_alpha;
              Bk[k] += fac * cv;
            }
          }
        }
      if (any_valid == 0ull) continue;
      // Eight of the nine wave-wide sums through LDS, transposed: lane L stores value q at red[q][L] (four
      // ds_write2st64_b32: the two values of a pair lie 64 dwords apart); lane j = 8 q + c then loads eight
      // floats of red[q][.] (two ds_read_b128, conflict-free: see below), adds them (7 VALU) and three
      // row_shr DPP adds finish value q in lane 8 q + 7.  ~12 issue slots for eight sums (the cross-lane
      // butterflies before it took ~37); the LDS instructions issue beside other waves' VALU.  The ninth sum (opacity)
      // keeps its DPP chain.  One wave per workgroup: LDS operations of a wave execute in order, the fences only
      // keep the compiler from moving the loads above the stores.
      sm.red[0][lane] = Sx; sm.red[1][lane] = Sy; sm.red[2][lane] = Sxx; sm.red[3][lane] = Sxy;
      sm.red[4][lane] = Syy; sm.red[5][lane] = g_r; sm.red[6][lane] = g_g; sm.red[7][lane] = g_b;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
      // (lane 8q + c takes floats [4c, 4c+4) and [32 + 4c, 32 + 4c + 4) of value q: consecutive lanes read consecutive
      //  16 B pieces -- the [8c, 8c+8) assignment had a stride of 32 B between lanes and a 2-way bank conflict on both loads)
      const float4* rp = reinterpret_cast<const float4*>(&sm.red[lane >> 3][4 * (lane & 7)]);
      const float4 r0 = rp[0], r1 = rp[8];
      g_o = wave_sum_to_lane63(g_o);
      if constexpr (NCH == 4) g_d = wave_sum_to_lane63(g_d);  // the transpose carries eight values: a second chain
      if constexpr (ABS) { ax = wave_sum_to_lane63(ax); ay = wave_sum_to_lane63(ay); }  // ... and a third and fourth
      float u = ((r0.x + r0.y) + (r0.z + r0.w)) + ((r1.x + r1.y) + (r1.z + r1.w));
      u = dpp_add<0x111>(u);
      u = dpp_add<0x112>(u);
      u = dpp_add<0x114>(u);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();  // (the next entry's stores stay below this entry's loads)
      if ((lane & 7) == 7) sm.acc[t][lane >> 3] = u;   // Sx Sy Sxx Sxy | Syy r g b | o
      if (lane == 63) sm.acc[t][8] = g_o;
      if constexpr (NCH == 4) { if (lane == 63) sm.acc[t][9] = g_d; }
      if constexpr (ABS) { if (lane == 63) { sm.acc[t][10] = ax * CONIC_DIAG_INV; sm.acc[t][11] = ay * CONIC_DIAG_INV; } }
      touched |= (1ull << t);
    }
    __syncthreads();
    if (PART) {
      if (lane < bn) {  // one full line (PART_F4 float4) per entry of the round, zeros if no pixel was valid
        const bool hit = (touched >> lane) & 1ull;
        const float4* a = reinterpret_cast<const float4*>(sm.acc[lane]);
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 r0 = z4, r1 = z4, r2 = z4;
        if (hit) {  // moments -> gradients here (the conic is at hand): x y ca cb | cc r g b | o
          const float4 m1 = a[1];
          float g_cc;
          r0 = sm.grad_xy_conic(lane, g_cc);
          r1 = make_float4(g_cc, m1.y, m1.z, m1.w);
          r2 = make_float4(a[2].x, 0.f, 0.f, 0.f);
          if constexpr (NCH == 4) r2.y = a[2].y;                 // x y ca cb | cc r g b | o d
          if constexpr (ABS) { r2.z = a[2].z; r2.w = a[2].w; }  // x y ca cb | cc r g b | o - ax ay
        }
        float4* dst = partials + PART_F4 * (size_t)sm.id[lane];
        dst[0] = r0; dst[1] = r1; dst[2] = r2;
        if (PART_F4 > 3) dst[3] = z4;
      }
    } else if ((touched >> lane) & 1ull) {
      // all nine (ten: NCH = 4) atomics of a Gaussian land in its one 64 B gradient line
      float* dst = packed_grad + 4 * REC_F4 * (size_t)sm.id[lane];
      const float* a = sm.acc[lane];
      float g_cc;
      const float4 g0 = sm.grad_xy_conic(lane, g_cc);
      atomicAdd(dst + 0, g0.x);  // x
      atomicAdd(dst + 1, g0.y);  // y
      atomicAdd(dst + 2, g0.z);  // conic a
      atomicAdd(dst + 3, g0.w);  // conic b
      atomicAdd(dst + 4, g_cc);  // conic c
#pragma unroll
      for (int c = 5; c < 6 + NCH; ++c) atomicAdd(dst + c, a[c]);
      if constexpr (ABS) { atomicAdd(dst + 10, a[10]); atomicAdd(dst + 11, a[11]); }
    }
  }
}

// Per-row sum of the tile partials (API surface: the engine path folds this sum into
// clmgs_preprocess_bwd).  Row i owns the contiguous slot range [row_cum[i-1], row_cum[i]); ranges and
// gradient lines are both walked sequentially; fixed order (ascending slot).
// partials line = gradient line: x y ca cb | cc r g b | o - - - | -   (ABS: o - ax ay, D4: o d, summed in the same order)
template <bool ABS = false, bool D4 = false>
__global__ void __launch_bounds__(256)
raster_partials_sum_kernel(int64_t n_rows, const int64_t* __restrict__ row_cum,
                           const float4* __restrict__ partials, float4* __restrict__ packed_grad) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n_rows;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s0 = r ? row_cum[r - 1] : 0;
    const int cnt = (int)(row_cum[r] - s0);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    float o = 0.f;
    const float4* src = partials + PART_F4 * (size_t)s0;
    for (int t = 0; t < cnt; t += 4) {  // four lines in flight per step (clamped; extra ones masked)
      float4 pa[4], pb[4];
      float po[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tt = min(t + u, cnt - 1);
        pa[u] = src[PART_F4 * tt]; pb[u] = src[PART_F4 * tt + 1]; po[u] = src[PART_F4 * tt + 2].x;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (t + u < cnt) {
          a.x += pa[u].x; a.y += pa[u].y; a.z += pa[u].z; a.w += pa[u].w;
          b.x += pb[u].x; b.y += pb[u].y; b.z += pb[u].z; b.w += pb[u].w;
          o += po[u];
        }
      }
    }
    float4* dst = packed_grad + REC_F4 * r;
    dst[0] = a; dst[1] = b; dst[2] = make_float4(o, 0.f, 0.f, 0.f);
    if constexpr (ABS) {  // the absgrad pair, same ascending order, in a pass of its own over lines the loop above just
      // read (API surface, cache hits): folded into that loop it permuted the plain kernel's registers
      float ax = 0.f, ay = 0.f;
      for (int t = 0; t < cnt; ++t) { const float4 c = src[PART_F4 * t + 2]; ax += c.z; ay += c.w; }
      *reinterpret_cast<float2*>(reinterpret_cast<float*>(dst) + 10) = make_float2(ax, ay);
    }
    if constexpr (D4) {  // the fourth channel's word, likewise in a pass of its own
      float d = 0.f;
      for (int t = 0; t < cnt; ++t) d += src[PART_F4 * t + 2].y;
      reinterpret_cast<float*>(dst)[9] = d;
    }
  }
}

}  // namespace clmgs

using namespace clmgs;

extern "C" size_t clmgs_rasterize_partials_bytes(int64_t n_isects) {
  return (size_t)(n_isects > 0 ? n_isects : 1) * (PART_F4 * 16);
}

extern "C" size_t clmgs_rasterize_pack_bytes(int C, int N) {
  return (size_t)C * (size_t)N * REC_F4 * sizeof(float4);
}

// nch: blended channels (3, or 4 = clmgs_rasterize4_*): colors / backgrounds / render_colors rows of nch floats
static int rasterize_fwd_impl(int nch, void* stream, int C, int N, int64_t n_isects,
                              const float* means2d, const float* conics, const float* colors,
                              const float* opacities, const float* backgrounds, int width,
                              int height, int tile_size, int tile_width, int tile_height,
                              const int32_t* offsets, const int32_t* flatten_ids, void* packed,
                              float* render_colors, float* render_alphas, int32_t* last_ids,
                              const int64_t* n_dev) {
  CLMGS_CHECK_ARG(tile_size == TILE);
  CLMGS_CHECK_ARG(C >= 1 && width > 0 && height > 0 && tile_width * TILE >= width &&
                  tile_height * TILE >= height);
  CLMGS_CHECK_ARG(offsets && render_colors && render_alphas && last_ids);
  CLMGS_CHECK_ARG(n_isects == 0 || (flatten_ids && packed));
  CLMGS_CHECK_ARG(!means2d || (conics && colors && opacities));
  CLMGS_CHECK_ARG(((uintptr_t)packed & 63) == 0);
  hipStream_t s = (hipStream_t)stream;
  const int64_t CN = (int64_t)C * N;
  if (means2d && n_isects > 0 && CN > 0) {  // means2d == NULL: `packed` was filled by the caller
    const dim3 grid(min(ceil_div(CN, 256), 256 * 8));
    hipLaunchKernelGGL(nch == 4 ? raster_pack_kernel<4> : raster_pack_kernel<3>, grid, dim3(256), 0, s, CN, means2d,
                       conics, colors, opacities, (float4*)packed);
    CLMGS_LAUNCH_CHECK();
  }
  const int n_blocks = C * tile_width * tile_height;
  hipLaunchKernelGGL(nch == 4 ? rasterize_fwd_kernel<4> : rasterize_fwd_kernel<3>, dim3(n_blocks), dim3(64), 0, s, C, N,
                     n_isects, (const float4*)packed, backgrounds, width, height, tile_width, tile_height, offsets,
                     flatten_ids, render_colors, render_alphas, last_ids, n_dev);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_rasterize_fwd(void* stream, int C, int N, int64_t n_isects,
                                   const float* means2d, const float* conics, const float* colors,
                                   const float* opacities, const float* backgrounds, int width,
                                   int height, int tile_size, int tile_width, int tile_height,
                                   const int32_t* offsets, const int32_t* flatten_ids, void* packed,
                                   float* render_colors, float* render_alphas, int32_t* last_ids) {
  return rasterize_fwd_impl(3, stream, C, N, n_isects, means2d, conics, colors, opacities, backgrounds, width, height,
                            tile_size, tile_width, tile_height, offsets, flatten_ids, packed, render_colors,
                            render_alphas, last_ids, nullptr);
}

// Four blended channels (gsplat's rasterize_to_pixels with colors[..., 4], render_mode="RGB+D"): same contract, rows of 4.
extern "C" int clmgs_rasterize4_fwd(void* stream, int C, int N, int64_t n_isects,
                                    const float* means2d, const float* conics, const float* colors,
                                    const float* opacities, const float* backgrounds, int width,
                                    int height, int tile_size, int tile_width, int tile_height,
                                    const int32_t* offsets, const int32_t* flatten_ids, void* packed,
                                    float* render_colors, float* render_alphas, int32_t* last_ids) {
  return rasterize_fwd_impl(4, stream, C, N, n_isects, means2d, conics, colors, opacities, backgrounds, width, height,
                            tile_size, tile_width, tile_height, offsets, flatten_ids, packed, render_colors,
                            render_alphas, last_ids, nullptr);
}

// Device-count form (see clmgs_isect2_emit_sort_dev): `capacity` bounds the list, the true count is read on the
// device; the records are the caller's packed [N,16] lines.
extern "C" int clmgs_rasterize_fwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                                       const float* backgrounds, int width, int height, int tile_size,
                                       int tile_width, int tile_height, const int32_t* offsets,
                                       const int32_t* flatten_ids, void* packed, float* render_colors,
                                       float* render_alphas, int32_t* last_ids) {
  CLMGS_CHECK_ARG(n_isects_dev && capacity > 0);
  return rasterize_fwd_impl(3, stream, C, N, capacity, nullptr, nullptr, nullptr, nullptr, backgrounds, width, height,
                            tile_size, tile_width, tile_height, offsets, flatten_ids, packed, render_colors,
                            render_alphas, last_ids, n_isects_dev);
}

// Four channels, device-count form: the records are the caller's packed [N,16] lines with the fourth colour in word 9
// (clmgs_invdepth_pack writes it into the lines clmgs_preprocess_fwd left); render_colors rows of 4.
extern "C" int clmgs_rasterize4_fwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                                        const float* backgrounds, int width, int height, int tile_size,
                                        int tile_width, int tile_height, const int32_t* offsets,
                                        const int32_t* flatten_ids, void* packed, float* render_colors,
                                        float* render_alphas, int32_t* last_ids) {
  CLMGS_CHECK_ARG(n_isects_dev && capacity > 0);
  return rasterize_fwd_impl(4, stream, C, N, capacity, nullptr, nullptr, nullptr, nullptr, backgrounds, width, height,
                            tile_size, tile_width, tile_height, offsets, flatten_ids, packed, render_colors,
                            render_alphas, last_ids, n_isects_dev);
}

static int rasterize_bwd_impl(int nch, void* stream, int C, int N, int64_t n_isects, const void* packed,
                              const float* backgrounds, int width, int height, int tile_size,
                              int tile_width, int tile_height, const int32_t* offsets,
                              const int32_t* flatten_ids, const float* render_alphas,
                              const int32_t* last_ids, const float* v_render_colors,
                              const float* v_render_alphas, void* packed_grad,
                              float* v_means2d, float* v_conics, float* v_colors,
                              float* v_opacities, const int32_t* emit_slot,
                              const int64_t* row_cum, void* partials, const int64_t* n_dev,
                              bool abs = false, float* v_means2d_abs = nullptr, bool slot4 = false) {
  if (abs && nch != 3) {  // before anything is written
    clmgs::set_error("clmgs_rasterize_abs_bwd: absgrad blends three channels only (word 9 of the gradient line is the "
                     "fourth channel's, words 10 and 11 the absgrad pair's)");
    return CLMGS_EINVAL;
  }
  if (nch == 4 && !slot4 && (partials || emit_slot)) {  // before anything is written
    clmgs::set_error("clmgs_rasterize4_bwd: the slot route (emit_slot / partials) of four channels is "
                     "clmgs_rasterize4_slot_bwd / clmgs_rasterize4_bwd_dev; pass emit_slot = partials = NULL for the "
                     "atomic route");
    return CLMGS_EINVAL;
  }
  CLMGS_CHECK_ARG(tile_size == TILE);
  CLMGS_CHECK_ARG(C >= 1 && width > 0 && height > 0 && tile_width * TILE >= width &&
                  tile_height * TILE >= height);
  CLMGS_CHECK_ARG(!v_means2d || (v_conics && v_colors && v_opacities));
  CLMGS_CHECK_ARG(!v_means2d_abs || (abs && v_means2d));  // the abs pair leaves with the unpack
  hipStream_t s = (hipStream_t)stream;
  const int64_t CN = (int64_t)C * N;
  if (CN == 0) return 0;  // nothing to differentiate: no argument below is required to exist
  // slot mode is selected by the partial-line table: a camera without a single intersection hands over
  // an EMPTY emit_slot (NULL data pointer) and must still be accepted (its gradients are all zero)
  const bool part = partials != nullptr;
  CLMGS_CHECK_ARG(!part || (C == 1 && (emit_slot || n_isects == 0) && (((uintptr_t)partials & 63) == 0)));
  // packed_grad == NULL (slot mode only): the caller sums the partial lines itself (clmgs_preprocess_bwd)
  CLMGS_CHECK_ARG(packed_grad ? ((((uintptr_t)packed_grad & 63) == 0) && (!part || row_cum)) : (part && !v_means2d));
  if (packed_grad && (!part || n_isects == 0))
    CLMGS_HIP(hipMemsetAsync(packed_grad, 0, clmgs_rasterize_pack_bytes(C, N), s));
  if (n_isects > 0) {
    CLMGS_CHECK_ARG(packed && offsets && flatten_ids && render_alphas && last_ids && v_render_colors);
    const int n_blocks = C * tile_width * tile_height;
    const auto kernel = abs ? (part ? rasterize_bwd_kernel<true, 3, true> : rasterize_bwd_kernel<false, 3, true>)
                        : part ? (nch == 4 ? rasterize_bwd_kernel<true, 4> : rasterize_bwd_kernel<true, 3>)
                               : nch == 4 ? rasterize_bwd_kernel<false, 4> : rasterize_bwd_kernel<false, 3>;
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(64), 0, s, C, N, n_isects, (const float4*)packed, backgrounds, width,
                       height, tile_width, tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                       v_render_alphas, (float*)packed_grad, emit_slot, (float4*)partials, n_dev);
    CLMGS_LAUNCH_CHECK();
    if (part && packed_grad) {
      const auto sum_kernel = abs ? raster_partials_sum_kernel<true>
                              : nch == 4 ? raster_partials_sum_kernel<false, true> : raster_partials_sum_kernel<false>;
      hipLaunchKernelGGL(sum_kernel, dim3(min(ceil_div(CN, 256), 256 * 16)), dim3(256),
                         0, s, CN, row_cum, (const float4*)partials, (float4*)packed_grad);
      CLMGS_LAUNCH_CHECK();
    }
  }
  if (v_means2d) {  // NULL: the caller consumes the packed gradient lines directly
    const dim3 grid(min(ceil_div(CN, 256), 256 * 8));
    hipLaunchKernelGGL(nch == 4 ? raster_unpack_grad_kernel<4> : raster_unpack_grad_kernel<3>, grid, dim3(256), 0, s, CN,
                       (const float4*)packed_grad, v_means2d, v_conics, v_colors, v_opacities);
    CLMGS_LAUNCH_CHECK();
    if (v_means2d_abs)
      hipLaunchKernelGGL(raster_unpack_abs_kernel, grid, dim3(256), 0, s, CN, (const float4*)packed_grad, v_means2d_abs);
    CLMGS_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int clmgs_rasterize_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                                   const float* backgrounds, int width, int height, int tile_size,
                                   int tile_width, int tile_height, const int32_t* offsets,
                                   const int32_t* flatten_ids, const float* render_alphas,
                                   const int32_t* last_ids, const float* v_render_colors,
                                   const float* v_render_alphas, void* packed_grad,
                                   float* v_means2d, float* v_conics, float* v_colors,
                                   float* v_opacities, const int32_t* emit_slot,
                                   const int64_t* row_cum, void* partials) {
  return rasterize_bwd_impl(3, stream, C, N, n_isects, packed, backgrounds, width, height, tile_size, tile_width,
                            tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                            v_render_alphas, packed_grad, v_means2d, v_conics, v_colors, v_opacities, emit_slot,
                            row_cum, partials, nullptr);
}

// Four blended channels, atomic route only: emit_slot / partials != NULL is refused before anything is written (the slot
// route of four channels is clmgs_rasterize4_slot_bwd below).
extern "C" int clmgs_rasterize4_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                                    const float* backgrounds, int width, int height, int tile_size,
                                    int tile_width, int tile_height, const int32_t* offsets,
                                    const int32_t* flatten_ids, const float* render_alphas,
                                    const int32_t* last_ids, const float* v_render_colors,
                                    const float* v_render_alphas, void* packed_grad,
                                    float* v_means2d, float* v_conics, float* v_colors,
                                    float* v_opacities, const int32_t* emit_slot,
                                    const int64_t* row_cum, void* partials) {
  return rasterize_bwd_impl(4, stream, C, N, n_isects, packed, backgrounds, width, height, tile_size, tile_width,
                            tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                            v_render_alphas, packed_grad, v_means2d, v_conics, v_colors, v_opacities, emit_slot,
                            row_cum, partials, nullptr);
}

// Four blended channels, slot route: clmgs_rasterize_bwd's contract with emit_slot / partials (partials is required).
// The stored line is  x y ca cb | cc r g b | o d - -;  with packed_grad + row_cum the per-row sum carries word 9 too, and
// the unpack writes v_colors rows of 4.
extern "C" int clmgs_rasterize4_slot_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                                         const float* backgrounds, int width, int height, int tile_size,
                                         int tile_width, int tile_height, const int32_t* offsets,
                                         const int32_t* flatten_ids, const float* render_alphas,
                                         const int32_t* last_ids, const float* v_render_colors,
                                         const float* v_render_alphas, void* packed_grad,
                                         float* v_means2d, float* v_conics, float* v_colors,
                                         float* v_opacities, const int32_t* emit_slot,
                                         const int64_t* row_cum, void* partials) {
  CLMGS_CHECK_ARG(partials);
  return rasterize_bwd_impl(4, stream, C, N, n_isects, packed, backgrounds, width, height, tile_size, tile_width,
                            tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                            v_render_alphas, packed_grad, v_means2d, v_conics, v_colors, v_opacities, emit_slot,
                            row_cum, partials, nullptr, false, nullptr, true);
}

// ... and its device-count form (clmgs_rasterize_bwd_dev's contract; word 9 of every line is the fourth channel's).
extern "C" int clmgs_rasterize4_bwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                                        const void* packed, const float* backgrounds, int width, int height,
                                        int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                                        const int32_t* flatten_ids, const float* render_alphas,
                                        const int32_t* last_ids, const float* v_render_colors,
                                        const float* v_render_alphas, const int32_t* emit_slot,
                                        const int64_t* row_cum, void* partials) {
  CLMGS_CHECK_ARG(n_isects_dev && capacity > 0 && emit_slot && partials);
  return rasterize_bwd_impl(4, stream, C, N, capacity, packed, backgrounds, width, height, tile_size, tile_width,
                            tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                            v_render_alphas, nullptr, nullptr, nullptr, nullptr, nullptr, emit_slot, row_cum,
                            partials, n_isects_dev, false, nullptr, true);
}

// Device-count form of the slot mode (one 64 B partial line per intersection, summed by the caller):
// `capacity` sizes `partials`, the true count is read on the device (see clmgs_isect2_emit_sort_dev).
extern "C" int clmgs_rasterize_bwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                                       const void* packed, const float* backgrounds, int width, int height,
                                       int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                                       const int32_t* flatten_ids, const float* render_alphas,
                                       const int32_t* last_ids, const float* v_render_colors,
                                       const float* v_render_alphas, const int32_t* emit_slot,
                                       const int64_t* row_cum, void* partials) {
  CLMGS_CHECK_ARG(n_isects_dev && capacity > 0 && emit_slot && partials);
  return rasterize_bwd_impl(3, stream, C, N, capacity, packed, backgrounds, width, height, tile_size, tile_width,
                            tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                            v_render_alphas, nullptr, nullptr, nullptr, nullptr, nullptr, emit_slot, row_cum,
                            partials, n_isects_dev);
}

// gsplat's absgrad (rasterize_to_pixels(absgrad=True) -> means2d.absgrad; AbsGS): clmgs_rasterize_bwd with
// sum_p |dL_p/dmean2d| next to the signed sums.  Three channels, both routes.  The gradient line and the slot route's
// partial line become  x y ca cb | cc r g b | o - ax ay  (words 10 and 11; word 9 stays the fourth channel's); every other
// word is the plain entry's.  v_means2d_abs [C*N,2] (optional) is written with the unpack.
extern "C" int clmgs_rasterize_abs_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                                       const float* backgrounds, int width, int height, int tile_size,
                                       int tile_width, int tile_height, const int32_t* offsets,
                                       const int32_t* flatten_ids, const float* render_alphas,
                                       const int32_t* last_ids, const float* v_render_colors,
                                       const float* v_render_alphas, void* packed_grad,
                                       float* v_means2d, float* v_conics, float* v_colors,
                                       float* v_opacities, const int32_t* emit_slot,
                                       const int64_t* row_cum, void* partials, float* v_means2d_abs) {
  return rasterize_bwd_impl(3, stream, C, N, n_isects, packed, backgrounds, width, height, tile_size, tile_width,
                            tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                            v_render_alphas, packed_grad, v_means2d, v_conics, v_colors, v_opacities, emit_slot,
                            row_cum, partials, nullptr, true, v_means2d_abs);
}

// Device-count form of the slot mode with the absgrad pair in words 10 and 11 of every partial line
// (clmgs_preprocess_abs_bwd sums them with the row).
extern "C" int clmgs_rasterize_abs_bwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                                           const void* packed, const float* backgrounds, int width, int height,
                                           int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                                           const int32_t* flatten_ids, const float* render_alphas,
                                           const int32_t* last_ids, const float* v_render_colors,
                                           const float* v_render_alphas, const int32_t* emit_slot,
                                           const int64_t* row_cum, void* partials) {
  CLMGS_CHECK_ARG(n_isects_dev && capacity > 0 && emit_slot && partials);
  return rasterize_bwd_impl(3, stream, C, N, capacity, packed, backgrounds, width, height, tile_size, tile_width,
                            tile_height, offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                            v_render_alphas, nullptr, nullptr, nullptr, nullptr, nullptr, emit_slot, row_cum,
                            partials, n_isects_dev, true, nullptr);
}
