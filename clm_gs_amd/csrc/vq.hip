// Compressed models ("Compressed models"): vector quantisation of the 45 higher-order SH
// coefficients of a row [48] (coefficient-major, DC in columns 0..2) against a codebook [K,48].
//
// clmgs_vq_assign: idx[n] = argmin_k sum_{j=3..47} (x_nj - c_kj)^2, the lowest k on an exact tie, scored as
//   score(n,k) = |c_k|^2 - 2 x_n . c_k   on the exact f32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain),
// the codebook as A and the data rows as B, so that in the C/D map (col = lane & 31, row = (reg&3) + 8 (reg>>2) +
// 4 (lane>>5)) a lane's 16 registers are 16 centroids of ITS OWN data row: the running (min, index) is per lane and
// per register, no cross-lane step per tile, and one exchange with lane l ^ 32 at the very end.
//
// The offset 3 of the 45 columns in a 192-B row rules out 16-B loads of them; instead the whole aligned row is loaded
// and columns 0..2 are replaced by zeros on BOTH sides (in the B registers and in the staged codebook), so the DC drops
// out of x . c whatever the caller's arrays hold there.  K-dim 48 = 24 steps of 32x32x2, no remainder.
//
// A workgroup is VQ_WAVES = 8 waves; a wave owns VQ_RG = 2 groups of 32 data rows (48 B registers, 2 accumulators: every
// A fragment read from LDS feeds two MFMAs), a workgroup 512 rows.  The codebook goes through LDS in tiles of VQ_KT = 128
// centroids (24 KiB), double buffered: the next tile's global loads are issued before the MFMAs of the current one and
// written to the other buffer after them, one barrier per tile.  The LDS image of a 32-centroid sub-tile is in A-fragment
// order, [q = 0..5][lane][e = 0..3] = c[lane & 31][k = 2 (4q + e) + (lane >> 5)], so a lane reads its 24 A values with six
// conflict-free 16-B reads.  |c_k|^2 (columns 3..47, a fixed left-to-right float sum) comes from a pre-pass into the
// caller's temp; a centroid past K is staged as zeros with |c|^2 = +inf and never wins.  `dist` is not |x|^2 + score:
// at the end each row gathers its winning centroid once and sums (x - c)^2 directly, exactly 0 for a row equal to it.
//
// clmgs_vq_accumulate / clmgs_vq_finish: the Lloyd update in fixed point, as sky.hip sums its map: rint(x * scale) as
// int64 by integer atomics only, so the sums do not depend on the order of the rows and are the same bits on every run.
#include "common.h"

namespace clmgs {

constexpr int VQ_COLS = 48;          // floats of a row
constexpr int VQ_REST = 45;          // columns 3..47
constexpr int VQ_STEPS = 24;         // k-steps of 32x32x2
constexpr int VQ_WAVES = 8;
constexpr int VQ_THREADS = VQ_WAVES * 64;
constexpr int VQ_RG = 2;             // groups of 32 data rows per wave
constexpr int VQ_ROWS = VQ_WAVES * VQ_RG * 32;  // data rows per workgroup
constexpr int VQ_KT = 128;           // centroids per staged tile
constexpr int VQ_SUB = VQ_KT / 32;   // 32-centroid sub-tiles of a tile
constexpr int VQ_TILE_F = VQ_KT * VQ_COLS;            // floats of a tile
constexpr int VQ_LOADS = VQ_TILE_F / 4 / VQ_THREADS;  // float4 per thread and tile
static_assert(VQ_LOADS * 4 * VQ_THREADS == VQ_TILE_F, "a tile is a whole number of float4 per thread");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// |c_k|^2 over columns 3..47: one thread per centroid, a fixed left-to-right sum.
__global__ void __launch_bounds__(256) vq_cnorm_kernel(const float* __restrict__ cb, float* __restrict__ cn, int K) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const float4* r = reinterpret_cast<const float4*>(cb + (int64_t)k * VQ_COLS);
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < VQ_COLS / 4; ++q) {
    const float4 v = r[q];
    if (q > 0) s = fmaf(v.x, v.x, s), s = fmaf(v.y, v.y, s), s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
  cn[k] = s;
}

// float4 f of tile `k0` (centroid ci = 4f / 48, columns col..col+3 of it); zeros past K, zeros in columns 0..2
__device__ __forceinline__ float4 vq_tile_load(const float* __restrict__ cb, int K, int k0, int f) {
  const int ci = (4 * f) / VQ_COLS, col = (4 * f) % VQ_COLS;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k0 + ci < K) {
    v = *reinterpret_cast<const float4*>(cb + (int64_t)(k0 + ci) * VQ_COLS + col);
    if (col == 0) v.x = v.y = v.z = 0.f;
  }
  return v;
}

// the same float4 into the A-fragment image: columns col, col+2 belong to lane half 0 (k even), col+1, col+3 to half 1
__device__ __forceinline__ void vq_tile_store(float* __restrict__ tile, int f, const float4& v) {
  const int ci = (4 * f) / VQ_COLS, col = (4 * f) % VQ_COLS;
  const int st = ci >> 5, i = ci & 31, s = col >> 1;  // s even: e = s & 3 is 0 or 2
  float* p = tile + st * (32 * VQ_COLS) + (s >> 2) * 256 + i * 4 + (s & 3);
  *reinterpret_cast<float2*>(p) = make_float2(v.x, v.z);
  *reinterpret_cast<float2*>(p + 32 * 4) = make_float2(v.y, v.w);
}

__global__ void __launch_bounds__(VQ_THREADS)
vq_assign_kernel(const float* __restrict__ rows, const float* __restrict__ cb, const float* __restrict__ cn,
                 int* __restrict__ idx, float* __restrict__ dist, int64_t N, int K) {
  __shared__ __attribute__((aligned(16))) float tile[2][VQ_TILE_F];
  __shared__ __attribute__((aligned(16))) float cnl[2][VQ_KT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * VQ_ROWS + wave * (VQ_RG * 32);

  // B fragments: xb[g][s] = x[row0 + 32 g + j][2 s + h], columns 0..2 as zeros; rows past N are zeros, never read
  float xb[VQ_RG][VQ_STEPS];
#pragma unroll
  for (int g = 0; g < VQ_RG; ++g) {
    const int64_t r = row0 + 32 * g + j;
#pragma unroll
    for (int q = 0; q < VQ_COLS / 4; ++q) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < N) v = *reinterpret_cast<const float4*>(rows + r * VQ_COLS + 4 * q);
      if (q == 0) v.x = v.y = v.z = 0.f;
      xb[g][2 * q] = h ? v.y : v.x;
      xb[g][2 * q + 1] = h ? v.w : v.z;
    }
  }

  float best[VQ_RG];
  int besti[VQ_RG];
#pragma unroll
  for (int g = 0; g < VQ_RG; ++g) best[g] = __builtin_inff(), besti[g] = 0;

  const int tiles = (K + VQ_KT - 1) / VQ_KT;
  {  // tile 0 -> buffer 0
#pragma unroll
    for (int u = 0; u < VQ_LOADS; ++u) {
      const int f = threadIdx.x + u * VQ_THREADS;
      vq_tile_store(tile[0], f, vq_tile_load(cb, K, 0, f));
    }
    if (threadIdx.x < VQ_KT) cnl[0][threadIdx.x] = threadIdx.x < K ? cn[threadIdx.x] : __builtin_inff();
  }
  __syncthreads();

  for (int t = 0; t < tiles; ++t) {
    const int k0 = t * VQ_KT, buf = t & 1;
    const bool more = t + 1 < tiles;
    float4 pre[VQ_LOADS];
    float pre_cn = __builtin_inff();
    if (more) {  // the next tile's loads stay in flight under the MFMAs below
#pragma unroll
      for (int u = 0; u < VQ_LOADS; ++u) pre[u] = vq_tile_load(cb, K, k0 + VQ_KT, threadIdx.x + u * VQ_THREADS);
      if (threadIdx.x < VQ_KT && k0 + VQ_KT + (int)threadIdx.x < K) pre_cn = cn[k0 + VQ_KT + threadIdx.x];
    }
    const int subs = min(VQ_SUB, (K - k0 + 31) >> 5);  // sub-tiles that hold a centroid (uniform)
    for (int st = 0; st < subs; ++st) {
      const float* a_img = tile[buf] + st * (32 * VQ_COLS) + lane * 4;
      float a[VQ_STEPS];
#pragma unroll
      for (int q = 0; q < VQ_STEPS / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(a_img + q * 256);
        a[4 * q] = v.x, a[4 * q + 1] = v.y, a[4 * q + 2] = v.z, a[4 * q + 3] = v.w;
      }
      f32x16 acc[VQ_RG];
#pragma unroll
      for (int g = 0; g < VQ_RG; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
#pragma unroll
      for (int s = 0; s < VQ_STEPS; ++s)
#pragma unroll
        for (int g = 0; g < VQ_RG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], xb[g][s], acc[g], 0, 0, 0);
      // register r of this lane: centroid k0 + 32 st + (r & 3) + 8 (r >> 2) + 4 h, increasing in r
      const float* cn_sub = cnl[buf] + st * 32 + 4 * h;
      const int kb = k0 + st * 32 + 4 * h;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const float4 c4 = *reinterpret_cast<const float4*>(cn_sub + 8 * r4);
        const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int g = 0; g < VQ_RG; ++g) {
            const float sc = fmaf(-2.f, acc[g][4 * r4 + e], cc[e]);
            if (sc < best[g]) best[g] = sc, besti[g] = kb + 8 * r4 + e;
          }
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < VQ_LOADS; ++u) vq_tile_store(tile[buf ^ 1], threadIdx.x + u * VQ_THREADS, pre[u]);
      if (threadIdx.x < VQ_KT) cnl[buf ^ 1][threadIdx.x] = pre_cn;
    }
    __syncthreads();
  }

  float dsum[VQ_RG];
#pragma unroll
  for (int g = 0; g < VQ_RG; ++g) dsum[g] = 0.f;
#pragma unroll
  for (int g = 0; g < VQ_RG; ++g) {  // the other half of this data row's centroids lives in lane ^ 32
    const float ob = __shfl_xor(best[g], 32, 64);
    const int oi = __shfl_xor(besti[g], 32, 64);
    if (ob < best[g] || (ob == best[g] && oi < besti[g])) best[g] = ob, besti[g] = oi;
    const int64_t r = row0 + 32 * g + j;
    if (r >= N) continue;  // (the shuffles are above: every lane took part)
    if (h == 0) idx[r] = besti[g];
    if (dist != nullptr) {
      // the distance itself, not |x|^2 + score: one gather of the winning centroid per row, each half its own columns
      // (2 s + h), so that a row equal to its centroid has distance exactly 0
      const float* c = cb + (int64_t)besti[g] * VQ_COLS;
      float d = 0.f;
#pragma unroll
      for (int q = 0; q < VQ_COLS / 4; ++q) {
        float4 v = *reinterpret_cast<const float4*>(c + 4 * q);
        if (q == 0) v.x = v.y = v.z = 0.f;
        const float da = xb[g][2 * q] - (h ? v.y : v.x), db = xb[g][2 * q + 1] - (h ? v.w : v.z);
        d = fmaf(da, da, d);
        d = fmaf(db, db, d);
      }
      dsum[g] = d;
    }
  }
  if (dist != nullptr) {
#pragma unroll
    for (int g = 0; g < VQ_RG; ++g) {
      const float d = dsum[g] + __shfl_xor(dsum[g], 32, 64);
      const int64_t r = row0 + 32 * g + j;
      if (h == 0 && r < N) dist[r] = d;
    }
  }
}

// one thread per element of rows [n,48]: column 0 counts the row, columns 3..47 add rint(x * scale)
__global__ void __launch_bounds__(256)
vq_accumulate_kernel(const float* __restrict__ rows, const int* __restrict__ idx, long long* __restrict__ acc,
                     long long* __restrict__ counts, int64_t N, int K, double scale) {
  const int64_t total = N * VQ_COLS;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / VQ_COLS;
    const int col = (int)(e - r * VQ_COLS);
    if (col == 1 || col == 2) continue;
    const int k = idx[r];
    if (k < 0 || k >= K) continue;  // an index outside the codebook adds nothing
    if (col == 0) {
      atomicAdd(reinterpret_cast<unsigned long long*>(counts + k), 1ull);
    } else {
      const long long v = __double2ll_rn((double)rows[e] * scale);
      if (v != 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(acc + (int64_t)k * VQ_REST + (col - 3)), (unsigned long long)v);
    }
  }
}

__global__ void __launch_bounds__(256)
vq_finish_kernel(const long long* __restrict__ acc, const long long* __restrict__ counts, float* __restrict__ cb, int K,
                 double scale) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= K * VQ_COLS) return;
  const int k = e / VQ_COLS, col = e - k * VQ_COLS;
  if (col < 3) {
    cb[e] = 0.f;
    return;
  }
  const long long c = counts[k];
  if (c > 0) cb[e] = (float)((double)acc[(int64_t)k * VQ_REST + (col - 3)] / (double)c / scale);
}

static bool vq_pow2(double s) {
  if (!(s > 0.0) || s > 0x1p1000) return false;
  while (s < 1.0) s *= 2.0;  // exact: only a power of two arrives at 1
  while (s > 1.0) s *= 0.5;
  return s == 1.0;
}

static bool vq_disjoint(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + na <= b0 || b0 + nb <= a0;
}

}  // namespace clmgs

using namespace clmgs;

extern "C" size_t clmgs_vq_assign_temp_bytes(int K) { return K < 1 ? 0 : align_up((size_t)K * sizeof(float), 256); }

extern "C" int clmgs_vq_assign(void* stream_, int64_t n, int K, const float* rows, const float* codebook, int32_t* idx,
                               float* dist, void* temp, size_t temp_bytes) {
  hipStream_t stream = (hipStream_t)stream_;
  CLMGS_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31));
  CLMGS_CHECK_ARG(K >= 1 && K <= 65536);
  CLMGS_CHECK_ARG(rows && codebook && idx && temp);
  CLMGS_CHECK_ARG(((uintptr_t)rows & 15) == 0 && ((uintptr_t)codebook & 15) == 0 && ((uintptr_t)temp & 15) == 0);
  CLMGS_CHECK_ARG(((uintptr_t)idx & 3) == 0 && ((uintptr_t)dist & 3) == 0);
  CLMGS_CHECK_ARG(temp_bytes >= clmgs_vq_assign_temp_bytes(K));
  const size_t rows_b = (size_t)n * VQ_COLS * 4, cb_b = (size_t)K * VQ_COLS * 4;
  CLMGS_CHECK_ARG(vq_disjoint(idx, (size_t)n * 4, rows, rows_b) && vq_disjoint(idx, (size_t)n * 4, codebook, cb_b));
  CLMGS_CHECK_ARG(vq_disjoint(temp, (size_t)K * 4, rows, rows_b) && vq_disjoint(temp, (size_t)K * 4, codebook, cb_b) &&
                  vq_disjoint(temp, (size_t)K * 4, idx, (size_t)n * 4));
  CLMGS_CHECK_ARG(dist == nullptr ||
                  (vq_disjoint(dist, (size_t)n * 4, rows, rows_b) && vq_disjoint(dist, (size_t)n * 4, codebook, cb_b) &&
                   vq_disjoint(dist, (size_t)n * 4, idx, (size_t)n * 4) && vq_disjoint(dist, (size_t)n * 4, temp, (size_t)K * 4)));
  float* cn = (float*)temp;
  hipLaunchKernelGGL(vq_cnorm_kernel, dim3(ceil_div(K, 256)), dim3(256), 0, stream, codebook, cn, K);
  CLMGS_LAUNCH_CHECK();
  hipLaunchKernelGGL(vq_assign_kernel, dim3((unsigned)ceil_div(n, VQ_ROWS)), dim3(VQ_THREADS), 0, stream, rows, codebook,
                     (const float*)cn, idx, dist, n, K);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_vq_accumulate(void* stream_, int64_t n, int K, const float* rows, const int32_t* idx, double scale,
                                   int64_t* acc, int64_t* counts) {
  hipStream_t stream = (hipStream_t)stream_;
  CLMGS_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31));
  CLMGS_CHECK_ARG(K >= 1 && K <= 65536);
  CLMGS_CHECK_ARG(rows && idx && acc && counts && vq_pow2(scale));
  CLMGS_CHECK_ARG(((uintptr_t)rows & 3) == 0 && ((uintptr_t)idx & 3) == 0);
  CLMGS_CHECK_ARG(((uintptr_t)acc & 7) == 0 && ((uintptr_t)counts & 7) == 0);
  const size_t acc_b = (size_t)K * VQ_REST * 8, cnt_b = (size_t)K * 8;
  CLMGS_CHECK_ARG(vq_disjoint(acc, acc_b, counts, cnt_b));
  CLMGS_CHECK_ARG(vq_disjoint(acc, acc_b, rows, (size_t)n * VQ_COLS * 4) && vq_disjoint(acc, acc_b, idx, (size_t)n * 4));
  CLMGS_CHECK_ARG(vq_disjoint(counts, cnt_b, rows, (size_t)n * VQ_COLS * 4) && vq_disjoint(counts, cnt_b, idx, (size_t)n * 4));
  const int64_t blocks = (n * VQ_COLS + 255) / 256;
  hipLaunchKernelGGL(vq_accumulate_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, rows,
                     idx, (long long*)acc, (long long*)counts, n, K, scale);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_vq_finish(void* stream_, int K, const int64_t* acc, const int64_t* counts, double scale,
                               float* codebook) {
  hipStream_t stream = (hipStream_t)stream_;
  CLMGS_CHECK_ARG(K >= 1 && K <= 65536);
  CLMGS_CHECK_ARG(acc && counts && codebook && vq_pow2(scale));
  CLMGS_CHECK_ARG(((uintptr_t)acc & 7) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)codebook & 3) == 0);
  const size_t cb_b = (size_t)K * VQ_COLS * 4;
  CLMGS_CHECK_ARG(vq_disjoint(codebook, cb_b, acc, (size_t)K * VQ_REST * 8) && vq_disjoint(codebook, cb_b, counts, (size_t)K * 8));
  hipLaunchKernelGGL(vq_finish_kernel, dim3(ceil_div((int64_t)K * VQ_COLS, 256)), dim3(256), 0, stream,
                     (const long long*)acc, (const long long*)counts, codebook, K, scale);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
