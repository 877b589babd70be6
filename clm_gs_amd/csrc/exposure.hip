// Per-camera exposure compensation ("Exposure"): a 3x4 affine colour transform between the
// rasterizer and the loss, E float32 [3][4] on the device (the convention of the INRIA 3DGS exposure.json):
//   y[c]        = x[0] E[0][c] + x[1] E[1][c] + x[2] E[2][c] + E[c][3]
//   dL/dx[k]    = E[k][0] g[0] + E[k][1] g[1] + E[k][2] g[2]                  (g = dL/dy)
//   dL/dE[k][c] = sum_p x[k] g[c]  (c < 3),   dL/dE[c][3] = sum_p g[c]
// The transform mixes the channels, so it is not part of the loss kernels (one channel per workgroup); it is a
// memory-bound pair of its own: 24 B per pixel forward, 36 B backward in place.  No LDS in the forward, no atomics
// anywhere: a workgroup STORES one row of 12 partial sums, clmgs_exposure_grad_finish sums the rows in a fixed
// order, so the parameter gradient is the same bit for bit on every run.
//
// Pixels are numbered p = y * W + x.  Two paths per kernel, chosen per WORKGROUP (block-uniform):
//   fast    : both images contiguous interleaved [H,W,3] with 16-byte aligned bases.  A lane takes 4 consecutive
//             pixels = 12 floats = three 16-byte loads and three 16-byte stores; the three wave instructions of a
//             group cover 3 KiB of contiguous memory, 1 KiB each, every 64-byte line used whole.
//   generic : any element strides (planar [3,H,W], an offset view), one pixel per lane and step, scalar accesses.
// The pixels [0, n_fast) go through fast workgroups, [n_fast, H*W) -- the last H*W mod 4 pixels of an eligible
// layout, everything of any other layout -- through generic ones.
#include "common.h"
#include "rowsum.h"

namespace clmgs {

constexpr int EXP_THREADS = 256;                                  // 4 waves
constexpr int EXP_WAVES = EXP_THREADS / 64;
constexpr int EXP_FWD_GROUPS = 4;                                 // forward: 4-pixel groups per lane
constexpr int EXP_FWD_PIXELS = EXP_THREADS * 4 * EXP_FWD_GROUPS;  // pixels per forward workgroup (4096)
constexpr int EXP_LANE_PIXELS = 64;                               // backward: pixels one lane accumulates, at most
constexpr int EXP_BWD_PIXELS = EXP_THREADS * EXP_LANE_PIXELS;     // pixels per backward workgroup = per partial row

struct ExpE {
  float m[3][4];
};

__device__ __forceinline__ ExpE load_E(const float* __restrict__ E) {
  ExpE e;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) e.m[k][c] = E[k * 4 + c];  // wave-uniform address: scalar loads
  return e;
}

// y[c] in the written order: one product, two fused multiply-adds, one addition = 4 roundings
__device__ __forceinline__ void exposure_apply(const ExpE& e, const float x[3], float y[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float t = x[0] * e.m[0][c];
    t = fmaf(x[1], e.m[1][c], t);
    t = fmaf(x[2], e.m[2][c], t);
    y[c] = t + e.m[c][3];
  }
}

// dL/dx[k]: one product, two fused multiply-adds = 3 roundings
__device__ __forceinline__ void exposure_vjp(const ExpE& e, const float g[3], float v[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float t = e.m[k][0] * g[0];
    t = fmaf(e.m[k][1], g[1], t);
    v[k] = fmaf(e.m[k][2], g[2], t);
  }
}

// acc[k*4+c] (+)= x[k] g[c] for c < 3, acc[c*4+3] (+)= g[c]: one rounding per element and pixel
__device__ __forceinline__ void exposure_accumulate(float acc[12], const float x[3], const float g[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[k * 4 + c] = fmaf(x[k], g[c], acc[k * 4 + c]);
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c * 4 + 3] += g[c];
}

__device__ __forceinline__ int64_t pixel_offset(const ImgView& v, int64_t p, int W) {
  const int64_t y = p / W, x = p - y * W;
  return y * v.sy + x * v.sx;
}

// 4 interleaved pixels <-> three float4
__device__ __forceinline__ void unpack4(const float4& a, const float4& b, const float4& c, float px[4][3]) {
  px[0][0] = a.x; px[0][1] = a.y; px[0][2] = a.z;
  px[1][0] = a.w; px[1][1] = b.x; px[1][2] = b.y;
  px[2][0] = b.z; px[2][1] = b.w; px[2][2] = c.x;
  px[3][0] = c.y; px[3][1] = c.z; px[3][2] = c.w;
}

__device__ __forceinline__ void pack4(const float px[4][3], float4& a, float4& b, float4& c) {
  a = make_float4(px[0][0], px[0][1], px[0][2], px[1][0]);
  b = make_float4(px[1][1], px[1][2], px[2][0], px[2][1]);
  c = make_float4(px[2][2], px[3][0], px[3][1], px[3][2]);
}

__global__ void __launch_bounds__(EXP_THREADS)
exposure_fwd_kernel(int64_t n_pix, int W, ImgView xv, const float* __restrict__ E_dev, ImgView yv, int64_t n_fast,
                    int fast_blocks) {
  const ExpE e = load_E(E_dev);
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < fast_blocks) {
    const int64_t n_groups = n_fast >> 2;
    const int64_t g0 = (int64_t)blockIdx.x * (EXP_THREADS * EXP_FWD_GROUPS) + tid;
    const float4* __restrict__ src = reinterpret_cast<const float4*>(xv.p);
    float4* __restrict__ dst = reinterpret_cast<float4*>(yv.p);
    float4 in[EXP_FWD_GROUPS][3];
#pragma unroll
    for (int t = 0; t < EXP_FWD_GROUPS; ++t) {  // all loads first: 12 x 16 B in flight per lane
      const int64_t g = g0 + (int64_t)t * EXP_THREADS;
      if (g < n_groups) {
        in[t][0] = src[g * 3 + 0];
        in[t][1] = src[g * 3 + 1];
        in[t][2] = src[g * 3 + 2];
      }
    }
#pragma unroll
    for (int t = 0; t < EXP_FWD_GROUPS; ++t) {
      const int64_t g = g0 + (int64_t)t * EXP_THREADS;
      if (g < n_groups) {
        float px[4][3], py[4][3];
        unpack4(in[t][0], in[t][1], in[t][2], px);
#pragma unroll
        for (int q = 0; q < 4; ++q) exposure_apply(e, px[q], py[q]);
        float4 a, b, c;
        pack4(py, a, b, c);
        dst[g * 3 + 0] = a;
        dst[g * 3 + 1] = b;
        dst[g * 3 + 2] = c;
      }
    }
    return;
  }
  const int64_t p0 = n_fast + (int64_t)((int)blockIdx.x - fast_blocks) * EXP_FWD_PIXELS + tid;
#pragma unroll 4
  for (int t = 0; t < EXP_FWD_PIXELS / EXP_THREADS; ++t) {
    const int64_t p = p0 + (int64_t)t * EXP_THREADS;
    if (p >= n_pix) break;
    const int64_t xo = pixel_offset(xv, p, W), yo = pixel_offset(yv, p, W);
    float x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = xv.p[xo + k * xv.sc];
    exposure_apply(e, x, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) yv.p[yo + c * yv.sc] = y[c];
  }
}

// v_x may alias g (equal strides): a lane reads the g of its own pixels before it writes their v_x, and no lane reads
// another lane's pixels, so g and v_x carry no __restrict__.
__global__ void __launch_bounds__(EXP_THREADS)
exposure_bwd_kernel(int64_t n_pix, int W, ImgView xv, const float* __restrict__ E_dev, ImgView gv, ImgView vv,
                    float* __restrict__ partials, int64_t n_fast, int fast_blocks) {
  __shared__ float red[EXP_WAVES][12];
  const ExpE e = load_E(E_dev);
  const int tid = threadIdx.x;
  float acc[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) acc[j] = 0.f;
  if ((int)blockIdx.x < fast_blocks) {
    const int64_t n_groups = n_fast >> 2;
    const int64_t g0 = (int64_t)blockIdx.x * (EXP_BWD_PIXELS / 4) + tid;
    const float4* __restrict__ xs = reinterpret_cast<const float4*>(xv.p);
    const float4* gs = reinterpret_cast<const float4*>(gv.p);
    float4* vs = reinterpret_cast<float4*>(vv.p);
#pragma unroll 2
    for (int t = 0; t < EXP_LANE_PIXELS / 4; ++t) {
      const int64_t g = g0 + (int64_t)t * EXP_THREADS;
      if (g >= n_groups) break;
      const float4 xa = xs[g * 3 + 0], xb = xs[g * 3 + 1], xc = xs[g * 3 + 2];
      const float4 ga = gs[g * 3 + 0], gb = gs[g * 3 + 1], gc = gs[g * 3 + 2];
      float px[4][3], pg[4][3], pv[4][3];
      unpack4(xa, xb, xc, px);
      unpack4(ga, gb, gc, pg);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        exposure_vjp(e, pg[q], pv[q]);
        exposure_accumulate(acc, px[q], pg[q]);
      }
      float4 a, b, c;
      pack4(pv, a, b, c);
      vs[g * 3 + 0] = a;
      vs[g * 3 + 1] = b;
      vs[g * 3 + 2] = c;
    }
  } else {
    const int64_t p0 = n_fast + (int64_t)((int)blockIdx.x - fast_blocks) * EXP_BWD_PIXELS + tid;
#pragma unroll 2
    for (int t = 0; t < EXP_LANE_PIXELS; ++t) {
      const int64_t p = p0 + (int64_t)t * EXP_THREADS;
      if (p >= n_pix) break;
      const int64_t xo = pixel_offset(xv, p, W), go = pixel_offset(gv, p, W), vo = pixel_offset(vv, p, W);
      float x[3], g[3], v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x[k] = xv.p[xo + k * xv.sc];
        g[k] = gv.p[go + k * gv.sc];
      }
      exposure_vjp(e, g, v);
      exposure_accumulate(acc, x, g);
#pragma unroll
      for (int k = 0; k < 3; ++k) vv.p[vo + k * vv.sc] = v[k];
    }
  }
  const float s = workgroup_row<EXP_WAVES, 12>(acc, red);  // rowsum.h: one stored row per workgroup
  if (tid < 12) partials[(int64_t)blockIdx.x * 12 + tid] = s;
}

static bool fast_layout(const void* base, int W, int64_t sc, int64_t sy, int64_t sx) {
  return sc == 1 && sx == 3 && sy == 3 * (int64_t)W && ((uintptr_t)base & 15) == 0;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_exposure_partials_rows(int H, int W) {
  if (H < 1 || W < 1) return 0;
  const int64_t n_pix = (int64_t)H * W, n_fast = n_pix & ~(int64_t)3;
  // the eligible layout's split (fast workgroups + one for the last H*W mod 4 pixels) is never smaller than the generic
  // layout's ceil(n_pix / EXP_BWD_PIXELS): every layout writes exactly this many rows
  return ceil_div(n_fast, EXP_BWD_PIXELS) + (n_pix > n_fast ? 1 : 0);
}

extern "C" int clmgs_exposure_fwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                                  int64_t stride_x, const float* E_dev, float* y, int64_t ystride_c,
                                  int64_t ystride_y, int64_t ystride_x) {
  CLMGS_CHECK_ARG(H >= 1 && W >= 1 && x && E_dev && y && x != y);
  const int64_t n_pix = (int64_t)H * W;
  const bool fast = fast_layout(x, W, stride_c, stride_y, stride_x) && fast_layout(y, W, ystride_c, ystride_y, ystride_x);
  const int64_t n_fast = fast ? (n_pix & ~(int64_t)3) : 0;
  const int fast_blocks = ceil_div(n_fast, EXP_FWD_PIXELS);
  const int blocks = fast_blocks + ceil_div(n_pix - n_fast, EXP_FWD_PIXELS);
  ImgView xv{const_cast<float*>(x), stride_c, stride_y, stride_x}, yv{y, ystride_c, ystride_y, ystride_x};
  hipLaunchKernelGGL(exposure_fwd_kernel, dim3((unsigned)blocks), dim3(EXP_THREADS), 0, (hipStream_t)stream, n_pix, W,
                     xv, E_dev, yv, n_fast, fast_blocks);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_exposure_bwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                                  int64_t stride_x, const float* E_dev, const float* g, int64_t gstride_c,
                                  int64_t gstride_y, int64_t gstride_x, float* v_x, int64_t vstride_c,
                                  int64_t vstride_y, int64_t vstride_x, float* partials) {
  CLMGS_CHECK_ARG(H >= 1 && W >= 1 && x && E_dev && g && v_x && partials && x != v_x);
  ImgView xv{const_cast<float*>(x), stride_c, stride_y, stride_x};
  ImgView gv{const_cast<float*>(g), gstride_c, gstride_y, gstride_x}, vv{v_x, vstride_c, vstride_y, vstride_x};
  CLMGS_CHECK_ARG(distinct_or_same_view(gv, vv));
  const int64_t n_pix = (int64_t)H * W;
  const bool fast = fast_layout(x, W, stride_c, stride_y, stride_x) && fast_layout(g, W, gstride_c, gstride_y, gstride_x) &&
                    fast_layout(v_x, W, vstride_c, vstride_y, vstride_x);
  const int64_t n_fast = fast ? (n_pix & ~(int64_t)3) : 0;
  const int fast_blocks = ceil_div(n_fast, EXP_BWD_PIXELS);
  const int rows = clmgs_exposure_partials_rows(H, W);  // workgroups without pixels store a row of zeros
  CLMGS_CHECK_ARG(fast_blocks + ceil_div(n_pix - n_fast, EXP_BWD_PIXELS) <= rows);
  hipLaunchKernelGGL(exposure_bwd_kernel, dim3((unsigned)rows), dim3(EXP_THREADS), 0, (hipStream_t)stream, n_pix, W, xv,
                     E_dev, gv, vv, partials, n_fast, fast_blocks);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_exposure_grad_finish(void* stream, int rows, const float* partials, float* grad12) {
  CLMGS_CHECK_ARG(rows >= 0 && partials && grad12);
  hipLaunchKernelGGL((rows_finish_kernel<16, 12, true>), dim3(1), dim3(64), 0, (hipStream_t)stream, rows, partials, grad12,
                     12);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
