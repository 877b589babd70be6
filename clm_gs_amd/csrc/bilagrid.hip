// Bilateral-grid colour correction ("Bilateral grid"): gsplat's `use_bilateral_grid` operator
// ("Bilateral Guided Radiance Field Processing") between the rasterizer and the loss.  A camera's grid is float32
// G[L][Hg][Wg][12], a lattice of 3x4 affine colour transforms (coefficient 4c + k = A[c][k]), sliced per pixel by its
// position and by its own luminance:
//   u  = (px + 0.5) / W        v  = (py + 0.5) / H        s = 0.299 x[0] + 0.587 x[1] + 0.114 x[2]
//   fx = u (Wg - 1)            fy = v (Hg - 1)            fz = clamp(s, 0, 1) (L - 1)
//   x0 = min(floor(fx), Wg - 2), tx = fx - x0             (likewise y0, ty and z0, tz)
//   A  = lerp_z(lerp_y(lerp_x ..)) of the 8 surrounding nodes, every lerp(a, b, t) = fmaf(t, b - a, a)
//   y[c] = A[c][0] x[0] + A[c][1] x[1] + A[c][2] x[2] + A[c][3]
//   dL/dG[node ijk][4c + k] += w_ijk g[c] x[k]   (x[3] := 1, g = dL/dy, w_ijk the trilinear weight)
//   dL/dx[k] = sum_c A[c][k] g[c] + lum[k] (L - 1) [0 < s < 1] sum_{c,k'} (A_hi - A_lo)[c][k'] g[c] x[k']
//
// Decomposition: a workgroup belongs to one xy CELL of the lattice (the pixels whose float32 fx, fy above floor to this
// x0, y0: a rectangle, found on the device by bisection over the SAME float32 expression the pixels use) and takes a
// chunk of the cell's pixels.  Its four xy corners are therefore uniform: the 4 x L nodes are staged in LDS once
// (1.5 KB at L = 8) and a pixel reads its 384 B of coefficients from there, not from L2.
// dL/dG uses no float atomics: a lane keeps BG_P pixels in registers, loops over the levels OUTERMOST accumulating the 48
// values of a level (4 corners x 12) with a z-weight that is zero unless the level is z0 or z0 + 1, the 48 sums go
// through wave_sum and, wave by wave in a fixed order, through LDS; the workgroup STORES its L x 48 block as one row of
// a slab.  clmgs_bilagrid_grad_finish sums, per node, the rows of its at most four cells in a fixed order and ADDS the
// sum into the camera's gradient grid.  The same inputs give the same bits on every run.
#include <algorithm>

#include "common.h"
#include "rowsum.h"

// Every fused multiply-add in this file is written as fmaf; nothing else may be fused.  Left to itself the compiler
// contracts tx = fx - x0 into one fma in some places and not in others, and the forward, the backward and the cell
// search would no longer evaluate the same float32 expression.
#pragma clang fp contract(off)

namespace clmgs {

constexpr int BG_THREADS = 256;
constexpr int BG_WAVES = BG_THREADS / 64;
constexpr int BG_P = 4;                        // pixels a lane holds at a time
constexpr int BG_CHUNK = BG_THREADS * BG_P;    // pixels per workgroup step = per slab row (when the host's bound holds)
constexpr int BG_MAX_L = 32, BG_MAX_XY = 64;
constexpr int BG_LEVEL = 52;                   // LDS floats per level: 4 corners x 12 + 4 of padding (level z starts at bank
                                               // 20 z mod 32: lanes on different levels read different banks)
constexpr int BG_ROW = 48;                     // slab floats per level and workgroup

// THE float32 lattice coordinate of pixel p on an axis of n pixels and m nodes; used by the cell search and by every pixel
__device__ __forceinline__ float bg_coord(int p, int n, int m) { return ((float)p + 0.5f) / (float)n * (float)(m - 1); }

// smallest p in [0, n] with floor(bg_coord(p)) >= c (bg_coord is monotone in p: correctly rounded operations)
__device__ __forceinline__ int bg_lower(int c, int n, int m) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)floorf(bg_coord(mid, n, m)) >= c) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ float bg_lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// the xy-interpolated matrix of one staged level: lerp_x on both rows, then lerp_y
__device__ __forceinline__ void bg_level_matrix(const float* lv, float tx, float ty, float A[12]) {
  const float4* l4 = reinterpret_cast<const float4*>(lv);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float4 c00 = l4[q], c01 = l4[3 + q], c10 = l4[6 + q], c11 = l4[9 + q];
    A[4 * q + 0] = bg_lerp(bg_lerp(c00.x, c01.x, tx), bg_lerp(c10.x, c11.x, tx), ty);
    A[4 * q + 1] = bg_lerp(bg_lerp(c00.y, c01.y, tx), bg_lerp(c10.y, c11.y, tx), ty);
    A[4 * q + 2] = bg_lerp(bg_lerp(c00.z, c01.z, tx), bg_lerp(c10.z, c11.z, tx), ty);
    A[4 * q + 3] = bg_lerp(bg_lerp(c00.w, c01.w, tx), bg_lerp(c10.w, c11.w, tx), ty);
  }
}

// s in the written order: one product, two fused multiply-adds
__device__ __forceinline__ float bg_luma(const float x[3]) {
  float s = 0.299f * x[0];
  s = fmaf(0.587f, x[1], s);
  return fmaf(0.114f, x[2], s);
}

__device__ __forceinline__ void bg_guide(float s, int L, int& z0, float& tz) {
  const float fz = fminf(fmaxf(s, 0.f), 1.f) * (float)(L - 1);
  z0 = min((int)floorf(fz), L - 2);
  tz = fz - (float)z0;
}

struct BgCell {
  int xa, ya, cw, npx;  // first column, first row, width, pixel count of the cell
  int x0, y0;
};

__device__ __forceinline__ BgCell bg_cell(int cell, int H, int W, int Hg, int Wg) {
  BgCell c;
  c.y0 = cell / (Wg - 1);
  c.x0 = cell - c.y0 * (Wg - 1);
  c.xa = c.x0 == 0 ? 0 : bg_lower(c.x0, W, Wg);
  const int xb = c.x0 == Wg - 2 ? W : bg_lower(c.x0 + 1, W, Wg);
  c.ya = c.y0 == 0 ? 0 : bg_lower(c.y0, H, Hg);
  const int yb = c.y0 == Hg - 2 ? H : bg_lower(c.y0 + 1, H, Hg);
  c.cw = max(xb - c.xa, 0);
  c.npx = c.cw * max(yb - c.ya, 0);  // < 2^31: H W is
  return c;
}

// the cell's 4 corners x L levels -> nodes[z][corner = 2 dy + dx][12]
__device__ __forceinline__ void bg_stage(float* nodes, const float* __restrict__ G, const BgCell& c, int L, int Hg, int Wg) {
  for (int t = threadIdx.x; t < L * 48; t += BG_THREADS) {
    const int z = t / 48, r = t - z * 48, corner = r / 12, j = r - corner * 12;
    const int y = c.y0 + (corner >> 1), x = c.x0 + (corner & 1);
    nodes[z * BG_LEVEL + r] = G[(((int64_t)z * Hg + y) * Wg + x) * 12 + j];
  }
}

__global__ void __launch_bounds__(BG_THREADS)
bilagrid_fwd_kernel(int H, int W, ImgView xv, const float* __restrict__ G, int L, int Hg, int Wg, ImgView yv) {
  __shared__ __attribute__((aligned(16))) float nodes[BG_MAX_L * BG_LEVEL];
  const BgCell c = bg_cell(blockIdx.y, H, W, Hg, Wg);
  if ((int64_t)blockIdx.x * BG_CHUNK >= c.npx) return;  // block-uniform
  bg_stage(nodes, G, c, L, Hg, Wg);
  __syncthreads();
  for (int64_t q0 = (int64_t)blockIdx.x * BG_CHUNK; q0 < c.npx; q0 += (int64_t)gridDim.x * BG_CHUNK) {
#pragma unroll
    for (int i = 0; i < BG_P; ++i) {
      const uint32_t q = (uint32_t)q0 + i * BG_THREADS + threadIdx.x;  // 32-bit division; q < 2^31 + BG_CHUNK
      if (q >= (uint32_t)c.npx) break;
      const int row = (int)(q / (uint32_t)c.cw), px = c.xa + (int)(q - (uint32_t)row * (uint32_t)c.cw), py = c.ya + row;
      const int64_t xo = (int64_t)py * xv.sy + (int64_t)px * xv.sx, yo = py * yv.sy + px * yv.sx;
      float x[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] = xv.p[xo + k * xv.sc];
      const float tx = bg_coord(px, W, Wg) - (float)c.x0, ty = bg_coord(py, H, Hg) - (float)c.y0;
      int z0;
      float tz;
      bg_guide(bg_luma(x), L, z0, tz);
      float lo[12], hi[12];
      bg_level_matrix(nodes + z0 * BG_LEVEL, tx, ty, lo);
      bg_level_matrix(nodes + (z0 + 1) * BG_LEVEL, tx, ty, hi);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {  // one product, two fused multiply-adds, one addition
        float t = bg_lerp(lo[4 * ch], hi[4 * ch], tz) * x[0];
        t = fmaf(bg_lerp(lo[4 * ch + 1], hi[4 * ch + 1], tz), x[1], t);
        t = fmaf(bg_lerp(lo[4 * ch + 2], hi[4 * ch + 2], tz), x[2], t);
        yv.p[yo + ch * yv.sc] = t + bg_lerp(lo[4 * ch + 3], hi[4 * ch + 3], tz);
      }
    }
  }
}

// v_x may alias g (the same view): a lane reads the g of its own pixels before it writes their v_x and no lane reads
// another lane's pixels, so g and v_x carry no __restrict__.
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_bwd_kernel(int H, int W, ImgView xv, const float* __restrict__ G, int L, int Hg, int Wg, ImgView gv, ImgView vv,
                    float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float nodes[BG_MAX_L * BG_LEVEL];
  __shared__ float wsum[BG_WAVES][BG_MAX_L * BG_ROW];  // per wave: its running L x 48 block
  const BgCell c = bg_cell(blockIdx.y, H, W, Hg, Wg);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n_row = L * BG_ROW;
  float* out = partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * n_row;
  if ((int64_t)blockIdx.x * BG_CHUNK >= c.npx) {  // block-uniform: a workgroup without pixels stores zeros
    for (int t = tid; t < n_row; t += BG_THREADS) out[t] = 0.f;
    return;
  }
  bg_stage(nodes, G, c, L, Hg, Wg);
  for (int t = lane; t < n_row; t += 64) wsum[wave][t] = 0.f;
  __syncthreads();
  const float lumL[3] = {0.299f * (float)(L - 1), 0.587f * (float)(L - 1), 0.114f * (float)(L - 1)};
  for (int64_t q0 = (int64_t)blockIdx.x * BG_CHUNK; q0 < c.npx; q0 += (int64_t)gridDim.x * BG_CHUNK) {
    float gx[BG_P][12], wxy[BG_P][4], tzs[BG_P];
    int z0s[BG_P];
    int zlo = L, zhi = -1;
#pragma unroll
    for (int i = 0; i < BG_P; ++i) {
      const uint32_t q = (uint32_t)q0 + i * BG_THREADS + tid;  // 32-bit division; q < 2^31 + BG_CHUNK
      z0s[i] = -4;  // no level matches: the pixel adds exact zeros
      tzs[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 12; ++j) gx[i][j] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) wxy[i][j] = 0.f;
      if (q < (uint32_t)c.npx) {
        const int row = (int)(q / (uint32_t)c.cw), px = c.xa + (int)(q - (uint32_t)row * (uint32_t)c.cw), py = c.ya + row;
        const int64_t xo = (int64_t)py * xv.sy + (int64_t)px * xv.sx, go = py * gv.sy + px * gv.sx, vo = py * vv.sy + px * vv.sx;
        float x[3], g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          x[k] = xv.p[xo + k * xv.sc];
          g[k] = gv.p[go + k * gv.sc];
        }
        const float tx = bg_coord(px, W, Wg) - (float)c.x0, ty = bg_coord(py, H, Hg) - (float)c.y0;
        const float s = bg_luma(x);
        int z0;
        float tz;
        bg_guide(s, L, z0, tz);
        float lo[12], hi[12];
        bg_level_matrix(nodes + z0 * BG_LEVEL, tx, ty, lo);
        bg_level_matrix(nodes + (z0 + 1) * BG_LEVEL, tx, ty, hi);
        // d = sum_c g[c] (D[c][0] x[0] + D[c][1] x[1] + D[c][2] x[2] + D[c][3]), D = A_hi - A_lo: the guidance term
        float d = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          float t = (hi[4 * ch] - lo[4 * ch]) * x[0];
          t = fmaf(hi[4 * ch + 1] - lo[4 * ch + 1], x[1], t);
          t = fmaf(hi[4 * ch + 2] - lo[4 * ch + 2], x[2], t);
          t += hi[4 * ch + 3] - lo[4 * ch + 3];
          d = ch == 0 ? t * g[0] : fmaf(t, g[ch], d);
        }
        const bool inside = s > 0.f && s < 1.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // one product, two fused multiply-adds (+ one for the guidance term)
          float t = bg_lerp(lo[k], hi[k], tz) * g[0];
          t = fmaf(bg_lerp(lo[4 + k], hi[4 + k], tz), g[1], t);
          t = fmaf(bg_lerp(lo[8 + k], hi[8 + k], tz), g[2], t);
          vv.p[vo + k * vv.sc] = inside ? fmaf(lumL[k], d, t) : t;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
          for (int k = 0; k < 3; ++k) gx[i][4 * ch + k] = g[ch] * x[k];
          gx[i][4 * ch + 3] = g[ch];
        }
        const float ux = 1.f - tx, uy = 1.f - ty;
        wxy[i][0] = uy * ux; wxy[i][1] = uy * tx; wxy[i][2] = ty * ux; wxy[i][3] = ty * tx;
        z0s[i] = z0;
        tzs[i] = tz;
        zlo = min(zlo, z0);
        zhi = max(zhi, z0 + 1);
      }
    }
    // the levels this wave's pixels touch (wave-uniform); every other level would add exact zeros
    zlo = __builtin_amdgcn_readfirstlane(-wave_max_i32(-zlo));
    zhi = __builtin_amdgcn_readfirstlane(wave_max_i32(zhi));
    for (int z = zlo; z <= zhi; ++z) {
      float acc[48];
#pragma unroll
      for (int a = 0; a < 48; ++a) acc[a] = 0.f;
#pragma unroll
      for (int i = 0; i < BG_P; ++i) {
        const float wz = z == z0s[i] ? 1.f - tzs[i] : (z == z0s[i] + 1 ? tzs[i] : 0.f);
#pragma unroll
        for (int cn = 0; cn < 4; ++cn) {
          const float w = wxy[i][cn] * wz;
#pragma unroll
          for (int j = 0; j < 12; ++j) acc[cn * 12 + j] = fmaf(w, gx[i][j], acc[cn * 12 + j]);
        }
      }
      float mine = 0.f;
#pragma unroll
      for (int a = 0; a < 48; ++a) {
        const float sum = wave_sum(acc[a]);
        mine = lane == a ? sum : mine;
      }
      if (lane < 48) wsum[wave][z * BG_ROW + lane] += mine;  // the wave's own block: no other wave touches it
    }
  }
  __syncthreads();
  for (int t = tid; t < n_row; t += BG_THREADS) {  // waves 0..3 in order
    float s = wsum[0][t];
#pragma unroll
    for (int w = 1; w < BG_WAVES; ++w) s += wsum[w][t];
    out[t] = s;
  }
}

// One lane per element of the gradient grid: the rows of the (at most four) cells the node is a corner of, cell by cell
// (y then x ascending) and chunk by chunk, summed serially with eight loads in flight, then ADDED into grad.
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_grad_finish_kernel(int chunks, int L, int Hg, int Wg, const float* __restrict__ partials,
                            float* __restrict__ grad) {
  const int e = blockIdx.x * BG_THREADS + threadIdx.x;
  if (e >= L * Hg * Wg * 12) return;
  const int j = e % 12, node = e / 12, x = node % Wg, y = (node / Wg) % Hg, z = node / (Wg * Hg);
  const int64_t row_floats = (int64_t)L * BG_ROW;
  float acc = 0.f;
  for (int dy = 1; dy >= 0; --dy) {
    const int cy = y - dy;
    if (cy < 0 || cy > Hg - 2) continue;
    for (int dx = 1; dx >= 0; --dx) {
      const int cx = x - dx;
      if (cx < 0 || cx > Wg - 2) continue;
      const float* src = partials + (int64_t)(cy * (Wg - 1) + cx) * chunks * row_floats + z * BG_ROW + (dy * 2 + dx) * 12 + j;
      acc = serial_sum8(acc, src, 0, 1, chunks, row_floats);  // rowsum.h: the chain goes on from cell to cell
    }
  }
  grad[e] += acc;
}

// grad += d(weight * tv)/dG, tv = (1/n) sum_axis sum (G[i+1] - G[i])^2 / count_axis: per element and axis
// c_axis ((G - G_prev) - (G_next - G)) with the missing neighbour's difference left out, c_axis = 2 weight / (n count_axis).
// One lane per float4 (a third of a node); no atomics.
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_tv_grad_kernel(int64_t n4, const float4* __restrict__ T, int L, int Hg, int Wg, float cz, float cy, float cx,
                        float4* __restrict__ grad) {
  const int64_t e = (int64_t)blockIdx.x * BG_THREADS + threadIdx.x;
  if (e >= n4) return;
  const int64_t node = e / 3;
  const int x = (int)(node % Wg), y = (int)((node / Wg) % Hg), z = (int)((node / ((int64_t)Wg * Hg)) % L);
  const int64_t sx = 3, sy = 3 * (int64_t)Wg, sz = sy * Hg;
  const float4 g0 = T[e];
  float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
  auto axis = [&](bool has_prev, bool has_next, int64_t st, float c) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_prev) {
      const float4 p = T[e - st];
      a.x = g0.x - p.x; a.y = g0.y - p.y; a.z = g0.z - p.z; a.w = g0.w - p.w;
    }
    if (has_next) {
      const float4 q = T[e + st];
      a.x -= q.x - g0.x; a.y -= q.y - g0.y; a.z -= q.z - g0.z; a.w -= q.w - g0.w;
    }
    d.x = fmaf(c, a.x, d.x); d.y = fmaf(c, a.y, d.y); d.z = fmaf(c, a.z, d.z); d.w = fmaf(c, a.w, d.w);
  };
  axis(z > 0, z < L - 1, sz, cz);
  axis(y > 0, y < Hg - 1, sy, cy);
  axis(x > 0, x < Wg - 1, sx, cx);
  float4 o = grad[e];
  o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w;
  grad[e] = o;
}

static bool bg_shape_ok(int L, int Hg, int Wg) {
  return L >= 2 && L <= BG_MAX_L && Hg >= 2 && Hg <= BG_MAX_XY && Wg >= 2 && Wg <= BG_MAX_XY;
}

// slab rows per cell: an upper bound of a cell's pixels (its sides are at most n / (m - 1) + 2 pixels, float32 rounding of
// the boundaries included) over BG_CHUNK.  The kernels stride over a cell by gridDim.x chunks, so a cell larger than the
// bound would still be covered.
static int bg_chunks(int H, int W, int Hg, int Wg) {
  const int64_t mw = std::min<int64_t>(W, W / (Wg - 1) + 2), mh = std::min<int64_t>(H, H / (Hg - 1) + 2);
  return std::max(1, ceil_div(mw * mh, BG_CHUNK));
}

static bool bg_image_ok(int H, int W) { return H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20) && (int64_t)H * W < (1ll << 31); }

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_bilagrid_partials_rows(int H, int W, int Hg, int Wg) {
  if (!bg_image_ok(H, W) || !bg_shape_ok(2, Hg, Wg)) return 0;
  return (Hg - 1) * (Wg - 1) * bg_chunks(H, W, Hg, Wg);
}

extern "C" int clmgs_bilagrid_fwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                                  int64_t stride_x, const float* grid_dev, int L, int Hg, int Wg, float* y,
                                  int64_t ystride_c, int64_t ystride_y, int64_t ystride_x) {
  CLMGS_CHECK_ARG(bg_image_ok(H, W) && x && grid_dev && y && x != y);
  CLMGS_CHECK_ARG(bg_shape_ok(L, Hg, Wg));
  ImgView xv{const_cast<float*>(x), stride_c, stride_y, stride_x}, yv{y, ystride_c, ystride_y, ystride_x};
  const dim3 grid((unsigned)bg_chunks(H, W, Hg, Wg), (unsigned)((Hg - 1) * (Wg - 1)));
  hipLaunchKernelGGL(bilagrid_fwd_kernel, grid, dim3(BG_THREADS), 0, (hipStream_t)stream, H, W, xv, grid_dev, L, Hg, Wg, yv);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_bilagrid_bwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                                  int64_t stride_x, const float* grid_dev, int L, int Hg, int Wg, const float* g,
                                  int64_t gstride_c, int64_t gstride_y, int64_t gstride_x, float* v_x, int64_t vstride_c,
                                  int64_t vstride_y, int64_t vstride_x, float* partials) {
  CLMGS_CHECK_ARG(bg_image_ok(H, W) && x && grid_dev && g && v_x && partials && x != v_x);
  CLMGS_CHECK_ARG(bg_shape_ok(L, Hg, Wg));
  ImgView xv{const_cast<float*>(x), stride_c, stride_y, stride_x};
  ImgView gv{const_cast<float*>(g), gstride_c, gstride_y, gstride_x}, vv{v_x, vstride_c, vstride_y, vstride_x};
  CLMGS_CHECK_ARG(distinct_or_same_view(gv, vv));
  const dim3 grid((unsigned)bg_chunks(H, W, Hg, Wg), (unsigned)((Hg - 1) * (Wg - 1)));
  hipLaunchKernelGGL(bilagrid_bwd_kernel, grid, dim3(BG_THREADS), 0, (hipStream_t)stream, H, W, xv, grid_dev, L, Hg, Wg, gv,
                     vv, partials);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_bilagrid_grad_finish(void* stream, int H, int W, int L, int Hg, int Wg, const float* partials,
                                          float* grad) {
  CLMGS_CHECK_ARG(bg_image_ok(H, W) && partials && grad);
  CLMGS_CHECK_ARG(bg_shape_ok(L, Hg, Wg));
  const int n = L * Hg * Wg * 12;
  hipLaunchKernelGGL(bilagrid_grad_finish_kernel, dim3((unsigned)ceil_div(n, BG_THREADS)), dim3(BG_THREADS), 0,
                     (hipStream_t)stream, bg_chunks(H, W, Hg, Wg), L, Hg, Wg, partials, grad);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_bilagrid_tv_grad(void* stream, const float* table, int64_t n, int L, int Hg, int Wg, float weight,
                                      float* grad) {
  CLMGS_CHECK_ARG(table && grad && table != grad && n >= 1 && n <= (1 << 24));
  CLMGS_CHECK_ARG(bg_shape_ok(L, Hg, Wg));
  CLMGS_CHECK_ARG(((uintptr_t)table & 15) == 0 && ((uintptr_t)grad & 15) == 0);
  const double per = 12.0 * (double)n, w2 = 2.0 * (double)weight;
  const float cz = (float)(w2 / (per * (L - 1) * Hg * Wg)), cy = (float)(w2 / (per * L * (Hg - 1) * Wg)),
              cx = (float)(w2 / (per * L * Hg * (Wg - 1)));
  const int64_t n4 = n * L * Hg * Wg * 3;
  CLMGS_CHECK_ARG((n4 + BG_THREADS - 1) / BG_THREADS <= INT32_MAX);  // the launch grid's x dimension
  hipLaunchKernelGGL(bilagrid_tv_grad_kernel, dim3((unsigned)((n4 + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0,
                     (hipStream_t)stream, n4, reinterpret_cast<const float4*>(table), L, Hg, Wg, cz, cy, cx,
                     reinterpret_cast<float4*>(grad));
  CLMGS_LAUNCH_CHECK();
  return 0;
}
