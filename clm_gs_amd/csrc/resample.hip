// Resolution schedule ("Resolution schedule"): an exact integer area filter that resamples the
// uint8 ground truth [planes,H,W], the uint16 inverse-depth prior [H,W] and the uint8 loss mask [H,W] to level L,
//   f = 2^L,  Ho = ceil(H / f),  Wo = ceil(W / f)     (the image EXTENT is kept: pixel pitch W/Wo x H/Ho, not f),
//   wx(j, x) = max(0, min((x+1) Wo, (j+1) W) - max(x Wo, j W)),      sum over x = W
//   wy(i, y) = max(0, min((y+1) Ho, (i+1) H) - max(y Ho, i H)),      sum over y = H
//   S(i, j)  = sum_y sum_x wy(i, y) wx(j, x) p[y, x],      out = (2 S + W H) / (2 W H)      (round half up)
//   mask:      p = [m != 0],  out = 2 S >= W H ? 255 : 0,  and the number of 255s is added to one device int64.
// When f divides W and H every weight is Wo Ho and the result is the f x f block mean (S with unit weights + f^2/2) >> 2L:
// the EXACT instantiations use unit weights and the shift.
//
// One wave owns one output row i and RS_SPAN / f output columns; four waves (four output rows) make a workgroup.
//   pass 1: the lane reads 16 B of each of the <= f + 1 source rows of the output row (up to four rows in flight) and
//           keeps the wy-weighted COLUMN sums of its 16 (uint8) or 8 (uint16) columns in registers: <= H * 65535 < 2^32.
//           The sums go to the wave's strip of LDS.
//   pass 2: the lane takes an output column j and adds wx(j, x) * column sum over the j's <= f + 1 source columns in 64
//           bits (S reaches W H 65535), rounds, divides.  The quotient is at most 8 or 16 bits wide: a restoring division
//           of that many steps, not a 64-bit divide.  The columns of j lie in (j f - f, j f + f]; wx is 0 outside the
//           true span, so the lane walks those 2 f columns and needs no division to find its first one.
// A source row starts at any byte (W is arbitrary): the 16 B reads are not aligned in general, which gfx950 global
// loads allow; they are aligned whenever W * sizeof(pixel) is a multiple of 16 (4608 is).  A read that would end past
// the last source element is done element by element.  Integer arithmetic only; no atomics except the mask count (one
// per workgroup, after a wave and an LDS reduction).
#include "common.h"

namespace clmgs {

constexpr int RS_WAVES = 4;               // output rows per workgroup
constexpr int RS_THREADS = 64 * RS_WAVES;
constexpr int RS_MAX_LEVEL = 8;           // f <= 256: a wave's 64 x 8 uint16 columns still hold two output columns
constexpr int RS_MAX_SIDE = 32768;        // (x+1) * Wo and H * 65535 stay inside 31 / 32 bits

template <typename T>
struct RsPix {
  static constexpr int VPX = 16 / (int)sizeof(T);  // pixels of one 16 B read
  static constexpr int SPAN = 64 * VPX;            // source columns one wave reads per step
  static constexpr int COLS = SPAN + 2 * VPX;      // + the one extra column an inexact pitch can add, rounded up
  static constexpr int QBITS = 8 * (int)sizeof(T);
};

struct __attribute__((packed)) RsVec8 { uint32_t w[4]; };                 // 16 B at any address
struct __attribute__((packed, aligned(2))) RsVec16 { uint32_t w[4]; };    // 16 B at an even address

__device__ __forceinline__ void rs_load(const uint8_t* p, uint32_t (&w)[4]) {
  const RsVec8 v = *reinterpret_cast<const RsVec8*>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = v.w[k];
}
__device__ __forceinline__ void rs_load(const uint16_t* p, uint32_t (&w)[4]) {
  const RsVec16 v = *reinterpret_cast<const RsVec16*>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = v.w[k];
}

template <typename T>
__device__ __forceinline__ uint32_t rs_unpack(const uint32_t (&w)[4], int e) {
  if constexpr (sizeof(T) == 1) return (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
  else return (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
}

// the overlap of source cell x (of n_src) and destination cell j (of n_dst) in units of 1 / (n_src n_dst) of the extent
__device__ __forceinline__ int rs_weight(int j, int x, int n_src, int n_dst) {
  return max(0, min((x + 1) * n_dst, (j + 1) * n_src) - max(x * n_dst, j * n_src));
}

// floor and ceil of j * n_src / n_dst without a division (the compiler's integer division goes through a float
// reciprocal): n_src = f n_dst - r with 0 <= r < f, so both lie in (j f - f, j f] and a walk down from j f finds them
__device__ __forceinline__ int rs_floor(int j, int n_src, int n_dst, int L) {
  int x = j << L;
  while (x * n_dst > j * n_src) --x;
  return x;
}
__device__ __forceinline__ int rs_ceil(int j, int n_src, int n_dst, int L) {
  int x = j << L;
  while ((x - 1) * n_dst >= j * n_src) --x;
  return x;
}

template <typename T, bool MASK, bool EXACT>
__global__ void __launch_bounds__(RS_THREADS)
area_resample_kernel(const T* __restrict__ src, T* __restrict__ dst, int H, int W, int Ho, int Wo, int L,
                     int64_t n_src, unsigned long long* __restrict__ count) {
  using P = RsPix<T>;
  __shared__ __attribute__((aligned(16))) uint32_t cols[RS_WAVES][P::COLS];
  __shared__ int red[RS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = 1 << L;
  const int jw = P::SPAN >> L;                      // output columns of a wave
  const int i = blockIdx.y * RS_WAVES + wave;       // its output row
  const int j0 = blockIdx.x * jw;
  const int nj = i < Ho ? min(jw, Wo - j0) : 0;     // a wave past the last row does nothing (it still meets the barriers)
  const int64_t plane = blockIdx.z;
  int x0 = 0, x1 = 0, ya = 0, yb = 0;
  if (nj > 0) {
    if constexpr (EXACT) {
      x0 = j0 << L; x1 = (j0 + nj) << L; ya = i << L; yb = ya + f;
    } else {  // wave-uniform, once per wave
      x0 = rs_floor(j0, W, Wo, L);
      x1 = rs_ceil(j0 + nj, W, Wo, L);
      ya = rs_floor(i, H, Ho, L);
      yb = rs_ceil(i + 1, H, Ho, L);
    }
  }
  const int ncols = x1 - x0;  // <= jw * f + 2 <= SPAN + 2
  uint32_t* strip = cols[wave];

  // ---- pass 1: weighted column sums of the rows [ya, yb)
  for (int v = lane; v * P::VPX < ncols; v += 64) {  // one trip; a second one for the few extra columns of an inexact pitch
    uint32_t acc[P::VPX];
#pragma unroll
    for (int e = 0; e < P::VPX; ++e) acc[e] = 0u;
    const int64_t col0 = (plane * H) * (int64_t)W + x0 + v * P::VPX;
    for (int y = ya; y < yb; y += 4) {
      uint32_t w[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // all reads of the step first
#pragma unroll
        for (int k = 0; k < 4; ++k) w[u][k] = 0u;
        if (y + u < yb) {
          const int64_t at = col0 + (int64_t)(y + u) * W;
          if (at + P::VPX <= n_src) {
            rs_load(src + at, w[u]);
          } else {  // the last elements of the tensor: never read past them
#pragma unroll
            for (int e = 0; e < P::VPX; ++e)
              if (at + e < n_src) {
                if constexpr (sizeof(T) == 1) w[u][e >> 2] |= (uint32_t)src[at + e] << (8 * (e & 3));
                else w[u][e >> 1] |= (uint32_t)src[at + e] << (16 * (e & 1));
              }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (y + u < yb) {
          const uint32_t wy = EXACT ? 1u : (uint32_t)rs_weight(i, y + u, H, Ho);
#pragma unroll
          for (int e = 0; e < P::VPX; ++e) {
            uint32_t p = rs_unpack<T>(w[u], e);
            if constexpr (MASK) p = p != 0u ? 1u : 0u;
            acc[e] += EXACT ? p : wy * p;
          }
        }
      }
    }
    // (columns at and past x1 belong to the next wave or the next row: stored, never read)
#pragma unroll
    for (int e = 0; e < P::VPX; e += 4)
      *reinterpret_cast<uint4*>(strip + v * P::VPX + e) = make_uint4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
  }
  __syncthreads();

  // ---- pass 2: one output column per lane
  const uint64_t WH = (uint64_t)W * (uint64_t)H;
  int counted = 0;
  for (int jj = lane; jj < nj; jj += 64) {
    const int j = j0 + jj;
    uint64_t S = 0;
    if constexpr (EXACT) {
      const uint32_t* c = strip + (jj << L);
      for (int t = 0; t < f; ++t) S += c[t];
    } else {
      const int xa = max((j << L) - f + 1, x0), xb = min((j << L) + f + 1, x1);
      for (int x = xa; x < xb; ++x) S += (uint64_t)(uint32_t)rs_weight(j, x, W, Wo) * strip[x - x0];
    }
    uint32_t out;
    if constexpr (MASK) {
      const bool on = EXACT ? (2 * S >= ((uint64_t)1 << (2 * L))) : (2 * S >= WH);
      out = on ? 255u : 0u;
      counted += on ? 1 : 0;
    } else if constexpr (EXACT) {
      out = (uint32_t)((S + ((uint64_t)1 << (2 * L - 1))) >> (2 * L));
    } else {
      uint64_t n = 2 * S + WH;  // < 2 W H * 2^QBITS: the quotient has QBITS bits
      const uint64_t d = 2 * WH;
      out = 0u;
#pragma unroll
      for (int b = P::QBITS - 1; b >= 0; --b) {
        const uint64_t db = d << b;
        if (n >= db) { n -= db; out |= 1u << b; }
      }
    }
    dst[(plane * Ho + i) * (int64_t)Wo + j] = (T)out;
  }
  if constexpr (MASK) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) counted += __shfl_xor(counted, o, 64);
    if (lane == 0) red[wave] = counted;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
#pragma unroll
      for (int k = 0; k < RS_WAVES; ++k) total += red[k];
      if (total) atomicAdd(count, (unsigned long long)total);
    }
  }
}

template <typename T, bool MASK>
static int area_resample(hipStream_t stream, int planes, int H, int W, int level, const T* src, T* dst, int64_t* count) {
  CLMGS_CHECK_ARG(planes >= 1 && planes <= 65535 && H >= 1 && W >= 1 && H <= RS_MAX_SIDE && W <= RS_MAX_SIDE);
  CLMGS_CHECK_ARG(level >= 1 && level <= RS_MAX_LEVEL);  // level 0 is the input itself: the operator returns it
  CLMGS_CHECK_ARG(src && dst && ((uintptr_t)src % sizeof(T)) == 0 && ((uintptr_t)dst % sizeof(T)) == 0);
  const int f = 1 << level;
  const int Ho = (H + f - 1) / f, Wo = (W + f - 1) / f;
  const int64_t n_src = (int64_t)planes * H * W, n_dst = (int64_t)planes * Ho * Wo;
  {  // the two ranges do not overlap
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + n_src * sizeof(T), d0 = (uintptr_t)dst, d1 = d0 + n_dst * sizeof(T);
    CLMGS_CHECK_ARG(d1 <= s0 || s1 <= d0);
  }
  if (MASK) {
    CLMGS_CHECK_ARG(count && ((uintptr_t)count & 7) == 0);
    CLMGS_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), stream));
  }
  const bool exact = (W % f) == 0 && (H % f) == 0;
  const int jw = RsPix<T>::SPAN >> level;
  const dim3 grid((unsigned)ceil_div(Wo, jw), (unsigned)ceil_div(Ho, RS_WAVES), (unsigned)planes);
  auto kernel = exact ? area_resample_kernel<T, MASK, true> : area_resample_kernel<T, MASK, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(RS_THREADS), 0, stream, src, dst, H, W, Ho, Wo, level, n_src,
                     (unsigned long long*)count);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" int clmgs_area_resample_u8(void* stream, int planes, int H, int W, int level, const uint8_t* src,
                                      uint8_t* dst) {
  return area_resample<uint8_t, false>((hipStream_t)stream, planes, H, W, level, src, dst, nullptr);
}

extern "C" int clmgs_area_resample_u16(void* stream, int H, int W, int level, const uint16_t* src, uint16_t* dst) {
  return area_resample<uint16_t, false>((hipStream_t)stream, 1, H, W, level, src, dst, nullptr);
}

extern "C" int clmgs_area_resample_mask(void* stream, int H, int W, int level, const uint8_t* src, uint8_t* dst,
                                        int64_t* count) {
  return area_resample<uint8_t, true>((hipStream_t)stream, 1, H, W, level, src, dst, count);
}
