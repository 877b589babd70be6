// Learnable sky ("Sky"): one equirectangular environment map S float32 [Hs,Ws,3] in world axes,
// composited behind the splats between the tile kernels and the camera's colour stage.  For pixel (px, py) of a camera
// with world->camera rotation R = viewmat[:3,:3] and intrinsics fx fy cx cy:
//   dc = ((px + .5 - cx) / fx, (py + .5 - cy) / fy, 1),   d = R^T dc / |dc|
//   u  = (atan2(d.x, d.z) / 2pi + .5) Ws - .5      column index wraps mod Ws
//   v  = (asin(clamp(d.y)) / pi + .5) Hs - .5      row index clamps to [0, Hs - 1]
//   s[c] = bilinear(S[..., c]; u, v)               four texels k, weights w_k >= 0
//   y[c] = x[c] + (1 - alpha) s[c]
//   dL/dalpha   = -(g[0] s[0] + g[1] s[1] + g[2] s[2])          (g = dL/dy; dL/dx = g: nothing to write)
//   dL/dS[k][c] += (1 - alpha) w_k g[c]
// The map gradient is accumulated in SIGNED 64-BIT FIXED POINT, unit 2^-48: each addend is formed in fp32 in the written
// order t = 1 - alpha, tw = t * w_k, a = tw * g[c], scaled by 2^48 (a power of two: exact) and rounded ONCE to an
// integer; from there everything is integer addition, which is associative -- the accumulator holds the same bits
// whatever the order of pixels, workgroups, calls, cameras and code paths.  An addend of magnitude >= 2^-24 converts
// exactly (24 significant bits above 2^-48), a smaller one loses at most 2^-49; CONTRACT: every texel sum, and every
// partial sum on the way, stays below 2^15 in magnitude (2^63 units).
//
// Backward, contention: a texel is usually many pixels wide, so thousands of pixels add into the same 3 words.  A workgroup
// owns a fixed 16x16 pixel tile, works out the window of texels its pixels touch (unwrapped columns, clamped rows),
// accumulates into an LDS window of int64 words with LDS integer atomics and flushes the non-zero words with global
// integer atomics (a zero word adds nothing: skipping it changes no bit).  A tile whose window exceeds SKY_WIN_TEXELS
// -- a map finer than the image, a tile on the u seam (its unwrapped columns span the whole map), a tile with a pole in
// it -- adds to global memory directly.  On either path a wave whose pixels share their four texels sums its integers
// first (sky_scatter).  All paths add the same integers.
#include "common.h"

namespace clmgs {

constexpr int SKY_TILE = 16;
constexpr int SKY_THREADS = SKY_TILE * SKY_TILE;  // 4 waves
// make DEFS=-DCLMGS_SKY_WIN_TEXELS=0: every tile adds to global memory directly (profiles/sky_microbench.py times it)
#ifndef CLMGS_SKY_WIN_TEXELS
#define CLMGS_SKY_WIN_TEXELS 256
#endif
constexpr int SKY_WIN_TEXELS = CLMGS_SKY_WIN_TEXELS;  // LDS window: 256 texels x 3 int64 = 6 KiB
constexpr float SKY_UNIT = 281474976710656.f;     // 2^48
constexpr float SKY_INV_2PI = 0.15915494309189535f;
constexpr float SKY_INV_PI = 0.3183098861837907f;

struct SkyCam {
  float r[9];  // world->camera rotation, row-major
  float fx, fy, cx, cy;
};

// The four texels of a pixel and their weights.  iu in [-1, Ws - 1] is the UNWRAPPED left column (columns iu, iu + 1
// wrap mod Ws), r0 <= r1 the clamped rows.  The half-texel shift is split into its integer and fractional part so that
// floor() and the weight are taken on a number of the magnitude of the angle, not of the map's width.
struct SkyTap {
  int iu, r0, r1;
  float fu, fv;
};

__device__ __forceinline__ int sky_split(float a, int n, float& frac) {  // floor and fraction of a + n/2 - 1/2
  const float h = 0.5f * (float)n - 0.5f;  // exact
  const float hi = floorf(h);
  const float b = a + (h - hi);
  const float ib = floorf(b);
  frac = b - ib;
  const int i = (int)ib + (int)hi;
  return min(max(i, -1), n - 1);  // the range of the definition; a NaN direction lands on 0
}

__device__ __forceinline__ SkyTap sky_tap(const SkyCam& cam, int px, int py, int Hs, int Ws) {
  const float dcx = (((float)px + 0.5f) - cam.cx) / cam.fx;
  const float dcy = (((float)py + 0.5f) - cam.cy) / cam.fy;
  const float inv = 1.f / sqrtf(fmaf(dcx, dcx, fmaf(dcy, dcy, 1.f)));
  const float dx = fmaf(cam.r[0], dcx, fmaf(cam.r[3], dcy, cam.r[6])) * inv;  // R^T dc / |dc|
  const float dy = fmaf(cam.r[1], dcx, fmaf(cam.r[4], dcy, cam.r[7])) * inv;
  const float dz = fmaf(cam.r[2], dcx, fmaf(cam.r[5], dcy, cam.r[8])) * inv;
  SkyTap t;
  t.iu = sky_split(atan2f(dx, dz) * SKY_INV_2PI * (float)Ws, Ws, t.fu);
  const int jv = sky_split(asinf(fminf(1.f, fmaxf(-1.f, dy))) * SKY_INV_PI * (float)Hs, Hs, t.fv);
  t.r0 = max(jv, 0);
  t.r1 = min(jv + 1, Hs - 1);
  return t;
}

__device__ __forceinline__ int sky_wrap(int c, int Ws) {  // c in [-1, Ws]
  return c < 0 ? c + Ws : (c >= Ws ? c - Ws : c);
}

// weights in texel order (r0,c0) (r0,c1) (r1,c0) (r1,c1): one rounding each after the two complements
__device__ __forceinline__ void sky_weights(const SkyTap& t, float w[4]) {
  const float gu = 1.f - t.fu, gv = 1.f - t.fv;
  w[0] = gu * gv;
  w[1] = t.fu * gv;
  w[2] = gu * t.fv;
  w[3] = t.fu * t.fv;
}

// s[c]: one product and three fused multiply-adds, texel order as above
__device__ __forceinline__ void sky_sample(const float* __restrict__ S, int Ws, const SkyTap& t, const float w[4],
                                           float s[3]) {
  const int c0 = sky_wrap(t.iu, Ws), c1 = sky_wrap(t.iu + 1, Ws);
  const float* a = S + ((int64_t)t.r0 * Ws + c0) * 3;
  const float* b = S + ((int64_t)t.r0 * Ws + c1) * 3;
  const float* c = S + ((int64_t)t.r1 * Ws + c0) * 3;
  const float* d = S + ((int64_t)t.r1 * Ws + c1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = fmaf(w[3], d[k], fmaf(w[2], c[k], fmaf(w[1], b[k], w[0] * a[k])));
}

// y may be x itself (same view): a lane reads its own pixel before it writes it
__global__ void __launch_bounds__(SKY_THREADS)
sky_fwd_kernel(int H, int W, ImgView xv, const float* __restrict__ alphas, SkyCam cam, const float* __restrict__ S, int Hs,
               int Ws, ImgView yv) {
  const int64_t p = (int64_t)blockIdx.x * SKY_THREADS + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int py = (int)(p / W), px = (int)(p - (int64_t)py * W);
  const int64_t xo = py * xv.sy + px * xv.sx, yo = py * yv.sy + px * yv.sx;
  float x[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = xv.p[xo + c * xv.sc];
  const float t = 1.f - alphas[p];
  const SkyTap tap = sky_tap(cam, px, py, Hs, Ws);
  float w[4], s[3];
  sky_weights(tap, w);
  sky_sample(S, Ws, tap, w, s);
#pragma unroll
  for (int c = 0; c < 3; ++c) yv.p[yo + c * yv.sc] = fmaf(t, s[c], x[c]);
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ void sky_add(unsigned long long* dst, long long q) {
  atomicAdd(dst, (unsigned long long)q);  // two's complement: the unsigned add is the signed add
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_add_i32(int v) {
  return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, true);
}
// lane 63 holds the sum of the wave; the lane order of wave_sum_to_lane63 (common.h), on integers
__device__ __forceinline__ int wave_sum_i32_to_lane63(int v) {
  v = dpp_add_i32<0x111>(v);
  v = dpp_add_i32<0x112>(v);
  v = dpp_add_i32<0x114>(v);
  v = dpp_add_i32<0x118>(v);
  v = dpp_add_i32<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
  v = dpp_add_i32<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}
// The exact sum of 64 int64 values in lane 63, without the LDS pipe: q = l2 2^44 + l1 2^22 + l0 with 0 <= l0, l1 < 2^22 and
// l2 signed; 64 limbs sum below 2^28 (l2: the contract |sum| < 2^63 units keeps it in 32 bits), so each limb is one
// 32-bit DPP reduction.
__device__ __forceinline__ long long wave_sum_i64_to_lane63(long long q) {
  const int s0 = wave_sum_i32_to_lane63((int)(q & 0x3fffff));
  const int s1 = wave_sum_i32_to_lane63((int)((q >> 22) & 0x3fffff));
  const int s2 = wave_sum_i32_to_lane63((int)(q >> 44));
  return (long long)(((unsigned long long)(long long)s2 << 44) + ((unsigned long long)(long long)s1 << 22) +
                     (unsigned long long)(long long)s0);
}

// The 12 integers of every pixel of a wave into `dst` (the LDS window or the accumulator: one instantiation each, so the
// adds are ds_add_u64 resp. global_atomic_add_x2 and not flat atomics) at word index(row, unwrapped column) + channel.
// A texel is usually many pixels wide: all pixels of a wave (4 rows of 16) then share their four texels, and 64 lanes
// would queue on the same 12 words.  Such a wave sums its integers first (integer addition: the same sum in any
// order) and one lane adds them.  Lanes outside the image hold t = 0, g = 0: their integers are 0.
template <typename Dst, typename Index>
__device__ __forceinline__ void sky_scatter(Dst dst, bool inside, const SkyTap& tap, float t, const float w[4],
                                            const float g[3], int lane, Index index) {
  const unsigned long long in_m = __builtin_amdgcn_ballot_w64(inside);
  if (in_m == 0ull) return;  // wave-uniform
  const int first = __ffsll((long long)in_m) - 1;
  const int iu0 = __shfl(tap.iu, first, 64), r00 = __shfl(tap.r0, first, 64), r10 = __shfl(tap.r1, first, 64);
  const bool shared = __builtin_amdgcn_ballot_w64(inside && tap.iu == iu0 && tap.r0 == r00 && tap.r1 == r10) == in_m;
  const int rows[2] = {shared ? r00 : tap.r0, shared ? r10 : tap.r1};
  const int iu = shared ? iu0 : tap.iu;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float tw = t * w[k];
    const auto base = index(rows[k >> 1], iu + (k & 1));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      long long q = __float2ll_rn((tw * g[c]) * SKY_UNIT);
      if (shared) {  // wave-uniform
        q = wave_sum_i64_to_lane63(q);
        if (lane == 63 && q != 0) sky_add(&dst[base + c], q);
      } else if (inside && q != 0) {
        sky_add(&dst[base + c], q);
      }
    }
  }
}

__global__ void __launch_bounds__(SKY_THREADS)
sky_bwd_kernel(int H, int W, ImgView gv, const float* __restrict__ alphas, SkyCam cam, const float* __restrict__ S, int Hs,
               int Ws, float* __restrict__ v_alphas, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long win[SKY_WIN_TEXELS > 0 ? SKY_WIN_TEXELS * 3 : 1];
  __shared__ int box[4];  // min column, max column (unwrapped), min row, max row
  const int tid = threadIdx.x;
  const int px = blockIdx.x * SKY_TILE + (tid & (SKY_TILE - 1)), py = blockIdx.y * SKY_TILE + (tid >> 4);
  const bool inside = px < W && py < H;
  if (tid == 0) {
    box[0] = INT32_MAX; box[1] = INT32_MIN; box[2] = INT32_MAX; box[3] = INT32_MIN;
  }
  SkyTap tap = {0, 0, 0, 0.f, 0.f};
  float w[4] = {0.f, 0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f}, t = 0.f;
  if (inside) {
    const int64_t p = (int64_t)py * W + px, go = py * gv.sy + px * gv.sx;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = gv.p[go + c * gv.sc];
    t = 1.f - alphas[p];
    tap = sky_tap(cam, px, py, Hs, Ws);
    sky_weights(tap, w);
    float s[3];
    sky_sample(S, Ws, tap, w, s);
    v_alphas[p] = -fmaf(g[2], s[2], fmaf(g[1], s[1], g[0] * s[0]));
  }
  __syncthreads();  // box initialised
  {
    const int c_lo = wave_min_i32(inside ? tap.iu : INT32_MAX), c_hi = wave_max_i32(inside ? tap.iu + 1 : INT32_MIN);
    const int r_lo = wave_min_i32(inside ? tap.r0 : INT32_MAX), r_hi = wave_max_i32(inside ? tap.r1 : INT32_MIN);
    if ((tid & 63) == 0) {
      atomicMin(&box[0], c_lo); atomicMax(&box[1], c_hi); atomicMin(&box[2], r_lo); atomicMax(&box[3], r_hi);
    }
  }
  __syncthreads();
  // the tile (blockIdx) has at least one pixel inside the image, so the box is a real one
  const int c_lo = box[0], r_lo = box[2];
  const int wc = box[1] - c_lo + 1, wr = box[3] - r_lo + 1;  // wc <= Ws + 2, wr <= Hs
  const bool windowed = (int64_t)wc * wr <= SKY_WIN_TEXELS;   // workgroup-uniform
  const int n_words = windowed ? wc * wr * 3 : 0;
  for (int i = tid; i < n_words; i += SKY_THREADS) win[i] = 0ull;
  __syncthreads();
  if (windowed)
    sky_scatter(win, inside, tap, t, w, g, tid & 63, [&](int r, int cu) { return ((r - r_lo) * wc + (cu - c_lo)) * 3; });
  else
    sky_scatter(acc, inside, tap, t, w, g, tid & 63,
                [&](int r, int cu) { return ((int64_t)r * Ws + sky_wrap(cu, Ws)) * 3; });
  if (!windowed) return;
  __syncthreads();
  for (int i = tid; i < n_words; i += SKY_THREADS) {
    const unsigned long long q = win[i];
    if (q != 0ull) {
      const int texel = i / 3, c = i - texel * 3;
      const int r = r_lo + texel / wc, cu = c_lo + texel % wc;
      // cu in [-1, Ws]: one wrap suffices (wc <= Ws + 2)
      sky_add(acc + ((int64_t)r * Ws + sky_wrap(cu, Ws)) * 3 + c, (long long)q);
    }
  }
}

__global__ void __launch_bounds__(256)
sky_acc_add_kernel(int64_t n, const long long* __restrict__ src, unsigned long long* __restrict__ dst) {
  // atomic, so that two cameras' adds into one accumulator may run on different streams; a zero adds nothing
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const long long q = src[i];
    if (q != 0) sky_add(dst + i, q);
  }
}

__global__ void __launch_bounds__(256)
sky_grad_convert_kernel(int64_t n, long long* __restrict__ acc, float* __restrict__ grad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    grad[i] += (float)((double)acc[i] * 0x1p-48);  // int64 -> double (exact below 2^53 units), the scaling is exact, double -> float rounds once
    acc[i] = 0;
  }
}

static SkyCam sky_cam(const float* vm, const float* K) {
  SkyCam cam;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) cam.r[i * 3 + j] = vm[i * 4 + j];
  cam.fx = K[0]; cam.fy = K[4]; cam.cx = K[2]; cam.cy = K[5];
  return cam;
}

}  // namespace clmgs

using namespace clmgs;

#define SKY_CHECK_COMMON()                                                                              \
  CLMGS_CHECK_ARG(H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1 && (int64_t)Hs * Ws * 3 <= INT32_MAX);         \
  CLMGS_CHECK_ARG(alphas && viewmat_host && K_host && sky);                                             \
  CLMGS_CHECK_ARG(K_host[0] != 0.f && K_host[4] != 0.f)

extern "C" int clmgs_sky_fwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                             int64_t stride_x, const float* alphas, const float* viewmat_host, const float* K_host,
                             const float* sky, int Hs, int Ws, float* y, int64_t ystride_c, int64_t ystride_y,
                             int64_t ystride_x) {
  SKY_CHECK_COMMON();
  CLMGS_CHECK_ARG(x && y);
  ImgView xv{const_cast<float*>(x), stride_c, stride_y, stride_x}, yv{y, ystride_c, ystride_y, ystride_x};
  CLMGS_CHECK_ARG(distinct_or_same_view(xv, yv));
  const int blocks = ceil_div((int64_t)H * W, SKY_THREADS);
  hipLaunchKernelGGL(sky_fwd_kernel, dim3((unsigned)blocks), dim3(SKY_THREADS), 0, (hipStream_t)stream, H, W, xv, alphas,
                     sky_cam(viewmat_host, K_host), sky, Hs, Ws, yv);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_sky_bwd(void* stream, int H, int W, const float* g, int64_t gstride_c, int64_t gstride_y,
                             int64_t gstride_x, const float* alphas, const float* viewmat_host, const float* K_host,
                             const float* sky, int Hs, int Ws, float* v_alphas, int64_t* acc) {
  SKY_CHECK_COMMON();
  CLMGS_CHECK_ARG(g && v_alphas && acc);
  const int gx = ceil_div(W, SKY_TILE), gy = ceil_div(H, SKY_TILE);
  CLMGS_CHECK_ARG(gy <= 65535);
  ImgView gv{const_cast<float*>(g), gstride_c, gstride_y, gstride_x};
  hipLaunchKernelGGL(sky_bwd_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(SKY_THREADS), 0, (hipStream_t)stream, H, W, gv,
                     alphas, sky_cam(viewmat_host, K_host), sky, Hs, Ws, v_alphas, (unsigned long long*)acc);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_sky_acc_add(void* stream, int64_t n, const int64_t* src, int64_t* dst) {
  CLMGS_CHECK_ARG(n >= 0 && (n == 0 || (src && dst)));
  if (n == 0) return 0;
  hipLaunchKernelGGL(sky_acc_add_kernel, dim3(min(ceil_div(n, 256), 256 * 8)), dim3(256), 0, (hipStream_t)stream, n,
                     (const long long*)src, (unsigned long long*)dst);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_sky_grad_convert(void* stream, int64_t n, int64_t* acc, float* grad) {
  CLMGS_CHECK_ARG(n >= 0 && (n == 0 || (acc && grad)));
  if (n == 0) return 0;
  hipLaunchKernelGGL(sky_grad_convert_kernel, dim3(min(ceil_div(n, 256), 256 * 8)), dim3(256), 0, (hipStream_t)stream, n,
                     (long long*)acc, grad);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
