// Lens distortion ("Lens distortion"): an inverse-map bilinear remap of a distorted source image
// [planes,Hs,Ws] (uint8 ground truth / mask, or the uint16 inverse-depth prior) onto an ideal centred pinhole
// [planes,Ho,Wo].  For every output pixel lens_math.h gives, in float64, the position (u, v) its ray has in the source
// and `mono`; the pixel is valid iff mono > 0 and (u, v) lies inside the source's pixel centres (slack 2^-20 px) and,
// with a source mask, all four taps are counted there.  out = floor(blend + 0.5) where valid, 0 elsewhere.
//
// A lane makes UD_PX = 4 adjacent pixels of the flattened output plane: the map, the taps and the weights once per
// pixel, then per plane four taps per pixel (plain global loads: neighbouring lanes read neighbouring source pixels) and
// ONE store of the four results (a 32-bit word for uint8, 64 bits for uint16).  The flattened plane is walked, not rows,
// so a group may straddle a row end; a plane of n = Ho Wo pixels starts at any byte when n is no multiple of 4, hence
// the stores are declared unaligned (gfx950 global stores allow it); only the last n % 4 pixels of a plane are stored
// one by one.  The grid is capped and strides over the groups; the number of valid pixels is summed per lane, per wave
// (shuffles), per workgroup (four words of LDS) and added with one integer atomic per workgroup.  The arithmetic is
// float64 on purpose (as mcmc.hip's relocation): it runs once per image at load, ~100 flops and at most one atan per
// pixel next to the image bytes it moves, and its result is comparable to a float64 reference pixel for pixel.
#include "common.h"
#include "lens_math.h"

namespace clmgs {

constexpr int UD_THREADS = 256;
constexpr int UD_PX = 4;             // pixels of a lane's group
constexpr int UD_MAX_BLOCKS = 4096;  // 256 CUs x 16: the rest of the groups by grid stride
constexpr int UD_MAX_SIDE = 32768;   // y * Ws + x and Ho * Wo stay inside 31 bits

struct __attribute__((packed)) UdWord8 { uint32_t w; };                   // 4 uint8 at any address
struct __attribute__((packed, aligned(2))) UdWord16 { uint32_t w[2]; };   // 4 uint16 at an even address

__device__ __forceinline__ void ud_store4(uint8_t* p, const uint32_t (&q)[UD_PX]) {
  UdWord8 v;
  v.w = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
  *reinterpret_cast<UdWord8*>(p) = v;
}
__device__ __forceinline__ void ud_store4(uint16_t* p, const uint32_t (&q)[UD_PX]) {
  UdWord16 v;
  v.w[0] = q[0] | (q[1] << 16);
  v.w[1] = q[2] | (q[3] << 16);
  *reinterpret_cast<UdWord16*>(p) = v;
}

template <typename T>
__device__ __forceinline__ void ud_store(T* p, const uint32_t (&q)[UD_PX], int npx) {
  if (npx == UD_PX) {
    ud_store4(p, q);
  } else {  // the tail of a plane
#pragma unroll
    for (int e = 0; e < UD_PX; ++e)
      if (e < npx) p[e] = (T)q[e];
  }
}

template <typename T>
__global__ void __launch_bounds__(UD_THREADS)
undistort_kernel(const T* __restrict__ src, const uint8_t* __restrict__ src_mask, T* __restrict__ dst,
                 uint8_t* __restrict__ valid_out, unsigned long long* __restrict__ count, int planes, int Hs, int Ws,
                 int Ho, int Wo, LensRec L, double fxo, double fyo) {
  __shared__ int red[UD_THREADS / 64];
  const int n = Ho * Wo;                      // <= 2^30
  const int groups = (n + UD_PX - 1) / UD_PX;
  const int64_t src_plane = (int64_t)Hs * Ws;
  int counted = 0;
  for (int g = blockIdx.x * UD_THREADS + threadIdx.x; g < groups; g += gridDim.x * UD_THREADS) {
    const int idx0 = g * UD_PX;
    const int npx = min(UD_PX, n - idx0);
    int i = idx0 / Wo, j = idx0 - i * Wo;
    int o00[UD_PX], o01[UD_PX], o10[UD_PX], o11[UD_PX];  // the taps' offsets inside a source plane (< 2^30)
    double a[UD_PX], b[UD_PX];
    bool ok[UD_PX];
#pragma unroll
    for (int e = 0; e < UD_PX; ++e) {
      ok[e] = false;
      o00[e] = o01[e] = o10[e] = o11[e] = 0;
      a[e] = b[e] = 0.0;
      if (e < npx) {
        double u, v, mono;
        lens_map(L, fxo, fyo, Ho, Wo, i, j, u, v, mono);
        ok[e] = lens_valid(u, v, mono, Hs, Ws);
        int x0, x1, y0, y1;
        lens_taps(u, Ws, x0, x1, a[e]);
        lens_taps(v, Hs, y0, y1, b[e]);
        o00[e] = y0 * Ws + x0; o01[e] = y0 * Ws + x1;
        o10[e] = y1 * Ws + x0; o11[e] = y1 * Ws + x1;
        if (src_mask != nullptr && ok[e])  // a pixel blended from an ignored pixel is ignored
          ok[e] = src_mask[o00[e]] != 0 && src_mask[o01[e]] != 0 && src_mask[o10[e]] != 0 && src_mask[o11[e]] != 0;
        counted += ok[e] ? 1 : 0;
        if (++j == Wo) { j = 0; ++i; }
      }
    }
    for (int p = 0; p < planes; ++p) {
      const T* sp = src + p * src_plane;
      uint32_t q[UD_PX];
#pragma unroll
      for (int e = 0; e < UD_PX; ++e) {
        q[e] = 0u;
        if (ok[e])
          q[e] = (uint32_t)lens_blend(a[e], b[e], (double)sp[o00[e]], (double)sp[o01[e]], (double)sp[o10[e]],
                                      (double)sp[o11[e]]);
      }
      ud_store(dst + (int64_t)p * n + idx0, q, npx);
    }
    if (valid_out != nullptr) {
      uint32_t q[UD_PX];
#pragma unroll
      for (int e = 0; e < UD_PX; ++e) q[e] = ok[e] ? 255u : 0u;
      ud_store(valid_out + idx0, q, npx);
    }
  }
  if (count != nullptr) {  // (uniform: every lane of the workgroup is here)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) counted += __shfl_xor(counted, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = counted;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
#pragma unroll
      for (int k = 0; k < UD_THREADS / 64; ++k) total += red[k];
      if (total) atomicAdd(count, (unsigned long long)total);
    }
  }
}

static bool lens_finite(const double* lens, double fxo, double fyo) {
  for (int k = 0; k < 10; ++k)
    if (!isfinite(lens[k])) return false;
  return isfinite(fxo) && isfinite(fyo);
}

template <typename T>
static int undistort(hipStream_t stream, int planes, int Hs, int Ws, int Ho, int Wo, const double* lens, int fisheye,
                     double fxo, double fyo, const T* src, const uint8_t* src_mask, T* dst, uint8_t* valid,
                     int64_t* count) {
  CLMGS_CHECK_ARG(planes >= 1 && planes <= 65535);
  CLMGS_CHECK_ARG(Hs >= 1 && Ws >= 1 && Ho >= 1 && Wo >= 1);
  CLMGS_CHECK_ARG(Hs <= UD_MAX_SIDE && Ws <= UD_MAX_SIDE && Ho <= UD_MAX_SIDE && Wo <= UD_MAX_SIDE);
  CLMGS_CHECK_ARG(lens != nullptr && (fisheye == 0 || fisheye == 1));
  CLMGS_CHECK_ARG(lens_finite(lens, fxo, fyo));
  CLMGS_CHECK_ARG(lens[0] > 0.0 && lens[1] > 0.0 && fxo > 0.0 && fyo > 0.0);
  CLMGS_CHECK_ARG(src && dst && ((uintptr_t)src % sizeof(T)) == 0 && ((uintptr_t)dst % sizeof(T)) == 0);
  CLMGS_CHECK_ARG(count == nullptr || ((uintptr_t)count & 7) == 0);
  const int64_t n_src = (int64_t)planes * Hs * Ws, n_dst = (int64_t)planes * Ho * Wo, n_out = (int64_t)Ho * Wo;
  {  // what is written overlaps nothing that is read, nor the other output
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + n_src * sizeof(T), d0 = (uintptr_t)dst, d1 = d0 + n_dst * sizeof(T);
    const uintptr_t m0 = (uintptr_t)src_mask, m1 = m0 + (uintptr_t)Hs * Ws, v0 = (uintptr_t)valid, v1 = v0 + n_out;
    CLMGS_CHECK_ARG(d1 <= s0 || s1 <= d0);
    CLMGS_CHECK_ARG(src_mask == nullptr || d1 <= m0 || m1 <= d0);
    CLMGS_CHECK_ARG(valid == nullptr || ((v1 <= s0 || s1 <= v0) && (v1 <= d0 || d1 <= v0)));
    CLMGS_CHECK_ARG(valid == nullptr || src_mask == nullptr || v1 <= m0 || m1 <= v0);
  }
  if (count) CLMGS_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), stream));
  LensRec L;
  L.fx = lens[0]; L.fy = lens[1]; L.cx = lens[2]; L.cy = lens[3];
  L.k1 = lens[4]; L.k2 = lens[5]; L.k3 = lens[6]; L.k4 = lens[7];
  L.p1 = lens[8]; L.p2 = lens[9];
  L.fisheye = fisheye;
  const int groups = ceil_div(n_out, UD_PX);
  const dim3 grid((unsigned)min(ceil_div(groups, UD_THREADS), UD_MAX_BLOCKS));
  hipLaunchKernelGGL(undistort_kernel<T>, grid, dim3(UD_THREADS), 0, stream, src, src_mask, dst, valid,
                     (unsigned long long*)count, planes, Hs, Ws, Ho, Wo, L, fxo, fyo);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_undistort_u8(void* stream, int planes, int Hs, int Ws, int Ho, int Wo, const double* lens,
                                  int fisheye, double fxo, double fyo, const uint8_t* src, const uint8_t* src_mask,
                                  uint8_t* dst, uint8_t* valid, int64_t* count) {
  return undistort<uint8_t>((hipStream_t)stream, planes, Hs, Ws, Ho, Wo, lens, fisheye, fxo, fyo, src, src_mask, dst,
                            valid, count);
}

extern "C" int clmgs_undistort_u16(void* stream, int Hs, int Ws, int Ho, int Wo, const double* lens, int fisheye,
                                   double fxo, double fyo, const uint16_t* src, uint16_t* dst) {
  return undistort<uint16_t>((hipStream_t)stream, 1, Hs, Ws, Ho, Wo, lens, fisheye, fxo, fyo, src, nullptr, dst, nullptr,
                             nullptr);
}
