// What the tile kernels share (rasterize.hip: forward and backward; contrib.hip: the contribution pass): the blend
// constants, the 64 B raster record and its staging through LDS, exact quadrant culling, the block -> tile mapping.
// Everything here is `__device__ __forceinline__` or constexpr: a kernel that includes it compiles to the code it was
// with the helpers written in its own file.
#pragma once
#include "common.h"
#include "gs_math.h"

namespace clmgs {

// Wave-uniform "some lane" / "no lane" tests straight from the compare's scalar mask.  (HIP's __any() goes through an
// int: the i1 is materialised with v_cndmask 0/1 and compared again -- two half-rate VALU per use in the blend loops.)
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
__device__ __forceinline__ bool wave_none(bool p) { return __builtin_amdgcn_ballot_w64(p) == 0ull; }

constexpr int TILE = 16;
constexpr int PPL = 4;        // pixels per lane (one per 8x8 quadrant)
constexpr float ALPHA_MIN = 1.f / 255.f;
constexpr float T_EPS = 1e-4f;
// The staging lane stores the conic pre-multiplied by log2(e) (and the 1/2 of the quadratic form), so
// the blend loops evaluate  s = log2(e) * sigma  with three FMA-class operations and feed v_exp_f32
// (a base-2 exponential) directly: two VALU fewer per (entry, quadrant) in both tile kernels.
constexpr float LOG2E = 1.4426950408889634f;
constexpr float CONIC_DIAG = 0.5f * LOG2E, CONIC_DIAG_INV = 2.f / LOG2E, CONIC_OFF_INV = 1.f / LOG2E;

// s = log2(e) * (0.5 (a dx^2 + c dy^2) + b dx dy) from the pre-scaled conic; identical code in the
// forward and the backward kernel, so both see the same alpha for every (entry, pixel)
__device__ __forceinline__ float scaled_sigma(float as, float bs, float cs, float dx, float dy) {
  return fmaf(cs * dy, dy, fmaf(as * dx, dx, (bs * dx) * dy));
}

// Per-Gaussian raster record, one 64 B line: {x, y, opacity, conic.a | conic.b, conic.c, r, g |
// b, d, -, - | -}.  The tile kernels gather ONE line per (Gaussian, tile) instead of touching
// four arrays (measured: 4.6 GB fetched per backward launch vs 1.3 GB algorithmic before).
// d: the fourth blended channel of the NCH = 4 kernels (gsplat's render_mode="RGB+D": the camera-space depth rides as a
// fourth colour); 0 in a 3-channel record.  It sits in the word next to blue, so the staging lane's gather of rec[2]
// brings it along: no second gather per (Gaussian, tile).
constexpr int REC_F4 = 4;

// The words of one record that the tile kernels use, in registers: the prefetch slot of the staging pipeline.
struct Rec {
  float4 A, B;      // rec[0], rec[1]
  float blue, dep;  // rec[2].x, rec[2].y (NCH = 4)
};
// Gather of record g (g < 0: no record, `r` keeps its value)
template <int NCH>
__device__ __forceinline__ void gather_record(Rec& r, const float4* __restrict__ packed, int g) {
  if (g >= 0) {
    const float4* rec = packed + REC_F4 * (size_t)g;
    r.A = rec[0]; r.B = rec[1]; r.blue = rec[2].x;
    if constexpr (NCH == 4) r.dep = rec[2].y;
  }
}

template <int NCH>
struct TileLds {
  float4 a[64];   // x, y, opacity, conic.a
  float4 b[64];   // conic.b, conic.c, r, g
  float c[NCH - 2][64];  // b (, d)
  int meta[64];   // (offset in staging round << 4) | quadrant mask  (backward: << META_SHIFT, | META_SPECIAL)
  // The staging lane's store of its record at compacted slot `pos`; the conic is pre-scaled here (LOG2E above).
  __device__ __forceinline__ void stage(int pos, const Rec& r, int meta_word) {
    a[pos] = make_float4(r.A.x, r.A.y, r.A.z, r.A.w * CONIC_DIAG);
    b[pos] = make_float4(r.B.x * LOG2E, r.B.y * CONIC_DIAG, r.B.z, r.B.w);
    c[0][pos] = r.blue; meta[pos] = meta_word;
    if constexpr (NCH == 4) c[1][pos] = r.dep;
  }
};

// Depth-ordered compaction of the lanes that keep their record: this lane's slot; n = records kept by the wave.
__device__ __forceinline__ int wave_compact(bool keep, int lane, int& n) {
  const unsigned long long bal = __ballot(keep);
  n = __popcll(bal);
  return __popcll(bal & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ void tile_range(const int32_t* __restrict__ offsets, int tile,
                                           int n_tiles_total, int64_t n_isects, int& s, int& e) {
  s = offsets[tile];
  e = (tile == n_tiles_total - 1) ? (int)n_isects : offsets[tile + 1];
}

// Block -> tile (XCD-aware) and lane -> 8x8 position, shared by both tile kernels.
struct TileGeom {
  int n_tiles_total, tile, cam, tx, ty, lane, qx, qy;
  float x0, y0;    // the tile's corner
  float px0, py0;  // this lane's pixel centre in quadrant 0; quadrant k lies 8 (k & 1), 8 (k >> 1) further
  __device__ __forceinline__ TileGeom(int C, int tile_w, int tile_h) {
    const int n_tiles = tile_w * tile_h;
    n_tiles_total = C * n_tiles;
    tile = (int)xcd_remap(blockIdx.x, (unsigned)n_tiles_total);
    cam = tile / n_tiles;
    const int t_in = tile - cam * n_tiles;
    ty = t_in / tile_w; tx = t_in - ty * tile_w;
    lane = threadIdx.x;
    qx = lane & 7; qy = lane >> 3;
    x0 = (float)(tx * TILE); y0 = (float)(ty * TILE);
    px0 = x0 + (float)qx + 0.5f; py0 = y0 + (float)qy + 0.5f;
  }
  // this lane's pixel of quadrant k: inside the image?  pix = its index
  __device__ __forceinline__ bool pixel_of(int k, int W, int H, size_t& pix) const {
    const int j = tx * TILE + 8 * (k & 1) + qx;
    const int i = ty * TILE + 8 * (k >> 1) + qy;
    pix = ((size_t)cam * H + i) * W + j;
    return (i < H) && (j < W);
  }
};

// Quadrant mask of the pixels (centres) where alpha can reach 1/255, i.e. sigma <= L = ln(255 o).
// Exact: the minimum of sigma over each quadrant's rectangle of pixel centres is compared with L
// (a small margin absorbs rounding), so a quadrant is skipped only if EVERY pixel in it fails the
// reference's own alpha >= 1/255 test -- results are unchanged.  The test costs ~150 VALU but
// runs once per entry on the staging lane (64 entries per instruction): ~2.5 VALU per entry to
// save whole 64-lane blend passes.
__device__ __forceinline__ int quadrant_mask(const Rec& r, float tile_x0, float tile_y0) {
  const float mx = r.A.x, my = r.A.y, opac = r.A.z, ca = r.A.w, cb = r.B.x, cc = r.B.y;
  if (!(opac >= ALPHA_MIN)) return 0;
  const float L = __logf(255.f * opac);
  const float det = ca * cc - cb * cb;
  if (!(det > 0.f) || !(ca > 0.f) || !(cc > 0.f)) return 15;  // degenerate conic: never cull
  const float Lm = L * 1.0001f + 1e-4f;
  if (!(Lm == Lm)) return 15;
  const float rca = __builtin_amdgcn_rcpf(ca), rcc = __builtin_amdgcn_rcpf(cc);
  // quadrant q covers pixel centres [q0 + 0.5, q0 + 7.5]; offsets are pixel - centre
  const float xa0 = tile_x0 + 0.5f - mx, xa1 = tile_x0 + 7.5f - mx;
  const float xb0 = tile_x0 + 8.5f - mx, xb1 = tile_x0 + 15.5f - mx;
  const float ya0 = tile_y0 + 0.5f - my, ya1 = tile_y0 + 7.5f - my;
  const float yb0 = tile_y0 + 8.5f - my, yb1 = tile_y0 + 15.5f - my;
  int m = 0;
  if (rect_min_sigma(ca, cb, cc, rca, rcc, xa0, xa1, ya0, ya1) <= Lm) m |= 1;
  if (rect_min_sigma(ca, cb, cc, rca, rcc, xb0, xb1, ya0, ya1) <= Lm) m |= 2;
  if (rect_min_sigma(ca, cb, cc, rca, rcc, xa0, xa1, yb0, yb1) <= Lm) m |= 4;
  if (rect_min_sigma(ca, cb, cc, rca, rcc, xb0, xb1, yb0, yb1) <= Lm) m |= 8;
  return m;
}

// SPECIAL entries (a wave-uniform flag in the entry's meta word, computed once per entry by the staging lane): opacity
// above 0.998, or a conic that is not positive definite with a condition number far from fp32's reach.  For every
// OTHER entry
//   * sigma cannot round below zero (sigma >= 0.5 lambda_min |d|^2, the rounding error of the three products is
//     <= 3 ulp x max(a, c) |d|^2, and det > 1e-5 (a + c)^2 puts lambda_min / max(a, c) fourteen times above that),
//     so gsplat's `sigma < 0` skip never fires, and
//   * o x G <= o <= 0.998 < 0.999, so the alpha clamp never fires and the saturated-alpha select is the identity,
// and the blend loops jump over those instructions with scalar branches on the flag: two compares, a v_min and a
// v_cndmask -- all half-rate VALU on this chip -- fewer per (entry, quadrant) in the backward, a compare and a v_min in
// the forward; same results bit for bit, one copy of the loop body.
#ifndef CLMGS_SPECIAL_ENTRIES
#define CLMGS_SPECIAL_ENTRIES 1
#endif
constexpr int META_SPECIAL = 16, META_SHIFT = 5;
__device__ __forceinline__ int special_entry(float opac, float ca, float cb, float cc) {
  const float tr = ca + cc;
  const bool plain = opac <= 0.998f && ca > 0.f && cc > 0.f && (ca * cc - cb * cb) > 1e-5f * tr * tr;
  return (CLMGS_SPECIAL_ENTRIES && plain) ? 0 : META_SPECIAL;
}

}  // namespace clmgs
