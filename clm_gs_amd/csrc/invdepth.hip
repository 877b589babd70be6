// Depth regularisation ("Depth regularisation"): an L1 loss between the rendered inverse depth
//   I_p = sum_i w_i / z_i   (the fourth blended channel of the 4-channel tile kernels, 1/z as fourth colour, background 0)
// and a monocular inverse-depth prior kept as uint16 [H,W] plus two floats per image (the INRIA 3DGS convention),
//   prior_p = raw_p / 65536 * scale + offset,
//   L_depth = weight * sum_p m_p |I_p - prior_p| / (H*W),     v_I_p = weight * m_p * sign(I_p - prior_p) / (H*W).
// Three memory-bound kernels around the tile kernels, none of which changes a front-end or tile kernel:
//   invdepth_pack     : 1/z into the spare word (word 9) of the 64 B raster records the front end left;
//   invdepth_l1       : one streaming pass, loss partial sums + cotangent;
//   invdepth_rows_bwd : g_d = dL/d(1/z) of a row (word 9 of its gradient lines) -> dL/dz = -g_d / z^2 -> xyz gradient
//                       dL/dz * R[2,:]  (z = R[2,:] . xyz + t[2], third row of the world-to-camera matrix).
// No float atomics anywhere: a workgroup STORES one partial sum, clmgs_invdepth_finish adds the rows in a fixed order.
#include "common.h"
#include "rowsum.h"

namespace clmgs {

constexpr int INV_THREADS = 256;                            // 4 waves
constexpr int INV_WAVES = INV_THREADS / 64;
constexpr int INV_LANE_PIXELS = 32;                         // pixels one lane accumulates
constexpr int INV_WG_PIXELS = INV_THREADS * INV_LANE_PIXELS;  // pixels per workgroup = per partial row (8192)
constexpr int INV_UNROLL = 8;                               // pixels of a lane in flight

__global__ void __launch_bounds__(256)
invdepth_pack_kernel(int V, const int32_t* __restrict__ radii, const float* __restrict__ depths,
                     float* __restrict__ packed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x)
    packed[16 * i + 9] = radii[i] > 0 ? 1.f / depths[i] : 0.f;  // IEEE division: the test holds it to 1/z exactly
}

// prior in ONE rounding: raw 2^-16 is exact, the fused multiply-add rounds raw/65536 * scale + offset once
__device__ __forceinline__ float prior_of(unsigned raw, float scale, float offset) {
  return fmaf((float)raw * (1.f / 65536.f), scale, offset);
}

// ENGINE = true : I and v_I are channel 3 of [H,W,4] buffers whose pixels are contiguous (strides 4W, 4) -- flat pixel
//                 indexing, no division: one dword load and one dword store per pixel at a 16 B stride (a wave
//                 instruction touches 1 KiB of contiguous memory, every 64 B line of it, a quarter of each).  A 16 B load
//                 of the whole pixel would fetch the same lines; the compiler narrows it to the one word that is used.
// ENGINE = false: any element strides (a planar map, an offset view): (y, x) by division, scalar accesses.
template <bool ENGINE>
__global__ void __launch_bounds__(INV_THREADS)
invdepth_l1_kernel(int64_t n_pix, int W, const float* __restrict__ I, int64_t sy, int64_t sx,
                   const uint16_t* __restrict__ prior, float scale, float offset, const uint8_t* __restrict__ mask,
                   float coef, float* __restrict__ v_I, int64_t vsy, int64_t vsx, float* __restrict__ partials) {
  __shared__ float red[INV_WAVES][1];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * INV_WG_PIXELS + tid;
  float acc[1] = {0.f};
#pragma unroll 1
  for (int t0 = 0; t0 < INV_LANE_PIXELS; t0 += INV_UNROLL) {
    float x[INV_UNROLL];
    unsigned raw[INV_UNROLL];
    unsigned m[INV_UNROLL];
    int64_t vo[INV_UNROLL];
#pragma unroll
    for (int u = 0; u < INV_UNROLL; ++u) {  // all loads first
      const int64_t p = p0 + (int64_t)(t0 + u) * INV_THREADS;
      x[u] = 0.f; raw[u] = 0u; m[u] = 0u; vo[u] = 0;
      if (p < n_pix) {
        if constexpr (ENGINE) {
          x[u] = I[4 * p];
          vo[u] = 4 * p;
        } else {
          const int64_t y = p / W, xx = p - y * W;
          x[u] = I[y * sy + xx * sx];
          vo[u] = y * vsy + xx * vsx;
        }
        raw[u] = prior[p];
        m[u] = mask ? mask[p] : 1u;
      }
    }
#pragma unroll
    for (int u = 0; u < INV_UNROLL; ++u) {
      const int64_t p = p0 + (int64_t)(t0 + u) * INV_THREADS;
      if (p < n_pix) {
        const float d = x[u] - prior_of(raw[u], scale, offset);
        const bool on = m[u] != 0u;
        acc[0] += on ? fabsf(d) : 0.f;
        const float sg = d > 0.f ? coef : (d < 0.f ? -coef : 0.f);  // d|x|/dx at 0 is 0
        v_I[vo[u]] = on ? sg : 0.f;
      }
    }
  }
  const float r = workgroup_row<INV_WAVES, 1>(acc, red);  // rowsum.h: one stored row per workgroup
  if (tid == 0) partials[blockIdx.x] = r;
}

// One lane per position i.  pitch 12: the [N,12] packed gradient table (words 0..2 of a row); pitch 3: [N,3].
__global__ void __launch_bounds__(256)
invdepth_rows_bwd_kernel(int V, const int64_t* __restrict__ filter, const int32_t* __restrict__ radii,
                         const float* __restrict__ depths, float r20, float r21, float r22,
                         const float4* __restrict__ partials, const int64_t* __restrict__ row_cum,
                         const float* __restrict__ packed_grad, float* __restrict__ g_xyz, int pitch) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
    if (!(radii[i] > 0)) continue;
    float g_d = 0.f;
    if (partials) {
      const int64_t s0 = i ? row_cum[i - 1] : 0;
      const int cnt = (int)(row_cum[i] - s0);
      const float* src = reinterpret_cast<const float*>(partials + PART_F4 * (size_t)s0) + 9;
      for (int t = 0; t < cnt; t += 4) {  // four lines in flight per step (clamped; extra ones masked), ascending slots
        float d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) d[u] = src[(size_t)(4 * PART_F4) * min(t + u, cnt - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (t + u < cnt) g_d += d[u];
      }
    } else {
      g_d = packed_grad[16 * i + 9];
    }
    const float z = depths[i];
    const float c = -g_d / (z * z);  // dL/dz
    float* dst = g_xyz + (size_t)pitch * (size_t)(filter ? filter[i] : i);
    // plain read-modify-write: the row was initialised for this step by the preprocess backward that ran before
    dst[0] = fmaf(c, r20, dst[0]);
    dst[1] = fmaf(c, r21, dst[1]);
    dst[2] = fmaf(c, r22, dst[2]);
  }
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_invdepth_partials_rows(int H, int W) {
  if (H < 1 || W < 1) return 0;
  return ceil_div((int64_t)H * W, INV_WG_PIXELS);
}

extern "C" int clmgs_invdepth_pack(void* stream, int V, const int32_t* radii, const float* depths, void* packed) {
  CLMGS_CHECK_ARG(V >= 0);
  if (V == 0) return 0;
  CLMGS_CHECK_ARG(radii && depths && packed && (((uintptr_t)packed & 63) == 0));
  hipLaunchKernelGGL(invdepth_pack_kernel, dim3(min(ceil_div(V, 256), 256 * 8)), dim3(256), 0, (hipStream_t)stream, V,
                     radii, depths, (float*)packed);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_invdepth_l1_fwd_bwd(void* stream, int H, int W, const float* I, int64_t stride_y,
                                         int64_t stride_x, const uint16_t* prior_u16, float scale, float offset,
                                         const uint8_t* mask, float weight, float* v_I, int64_t vstride_y,
                                         int64_t vstride_x, float* partials) {
  CLMGS_CHECK_ARG(H >= 1 && W >= 1 && I && prior_u16 && v_I && partials && I != v_I);
  // no two pixels of v_I share a word
  CLMGS_CHECK_ARG(vstride_x >= 1 && (H == 1 || vstride_y >= (int64_t)W * vstride_x));
  CLMGS_CHECK_ARG(weight == weight && scale == scale && offset == offset);
  const int64_t n_pix = (int64_t)H * W;
  const int rows = clmgs_invdepth_partials_rows(H, W);
  const float coef = (float)((double)weight / (double)n_pix);  // the one rounding of weight / (H*W)
  const bool engine = stride_x == 4 && (H == 1 || stride_y == 4 * (int64_t)W) &&
                      vstride_x == 4 && (H == 1 || vstride_y == 4 * (int64_t)W);
  hipLaunchKernelGGL(engine ? invdepth_l1_kernel<true> : invdepth_l1_kernel<false>, dim3((unsigned)rows),
                     dim3(INV_THREADS), 0, (hipStream_t)stream, n_pix, W, I, stride_y, stride_x, prior_u16, scale, offset,
                     mask, coef, v_I, vstride_y, vstride_x, partials);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_invdepth_finish(void* stream, int rows, const float* partials, float* sum_out) {
  CLMGS_CHECK_ARG(rows >= 0 && partials && sum_out);
  hipLaunchKernelGGL((rows_finish_kernel<1, 1, false>), dim3(1), dim3(64), 0, (hipStream_t)stream, rows, partials, sum_out, 1);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_invdepth_rows_bwd(void* stream, int V, const int64_t* filter, const int32_t* radii,
                                       const float* depths, const float* viewmat, const void* partials,
                                       const int64_t* row_cum, const void* packed_grad, float* g_xyz,
                                       int packed_grads) {
  CLMGS_CHECK_ARG(V >= 0 && (packed_grads == 0 || packed_grads == 1));
  CLMGS_CHECK_ARG((partials != nullptr) != (packed_grad != nullptr));
  CLMGS_CHECK_ARG(!partials || (row_cum && (((uintptr_t)partials & 15) == 0)));
  CLMGS_CHECK_ARG(radii && depths && viewmat && g_xyz);
  if (V == 0) return 0;
  hipLaunchKernelGGL(invdepth_rows_bwd_kernel, dim3(min(ceil_div(V, 256), 256 * 16)), dim3(256), 0, (hipStream_t)stream, V,
                     filter, radii, depths, viewmat[8], viewmat[9], viewmat[10], (const float4*)partials, row_cum,
                     (const float*)packed_grad, g_xyz, packed_grads ? 12 : 3);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
