// The deterministic row sum of the per-camera gradients ("Row sums"): device only.
//   lane -> wave (wave_sum) -> workgroup (waves in order, through LDS) -> one STORED row per workgroup   workgroup_row
//   a one-wave finish kernel then sums the rows in a fixed order                                          rows_finish_kernel
// No float atomics: the order of every addition is written here, once, so the same inputs give the same bits on every
// run.  tests/test_gpu_rowsum.py holds the finish order to a float32 emulation bit for bit.
#pragma once
#include "common.h"

namespace clmgs {

// acc + src[first * pitch] + src[(first + step) * pitch] + ... over the rows first + k * step < rows, added one at a time
// in ascending row order.  Eight loads are in flight per step (one memory latency per 8 rows, not per row); a
// one-at-a-time tail takes the rest.  `acc` is the chain so far: 0.f, or what a caller has already summed.
__device__ __forceinline__ float serial_sum8(float acc, const float* __restrict__ src, int first, int step, int rows,
                                             int64_t pitch) {
  constexpr int B = 8;
  int r = first;
  for (; r + (B - 1) * step < rows; r += B * step) {
    float t[B];
#pragma unroll
    for (int i = 0; i < B; ++i) t[i] = src[(int64_t)(r + i * step) * pitch];
#pragma unroll
    for (int i = 0; i < B; ++i) acc += t[i];
  }
  for (; r < rows; r += step) acc += src[(int64_t)r * pitch];
  return acc;
}

// The K sums of a workgroup of WAVES wavefronts: every acc[k] through wave_sum, lane 0 of a wave stores red[wave][k],
// thread k < K then adds red[0][k] + red[1][k] + ... in wave order and returns the sum (every other thread: 0.f); the
// caller stores it.  Contains the workgroup's barrier: every thread calls it.
template <int WAVES, int K>
__device__ __forceinline__ float workgroup_row(const float (&acc)[K], float (&red)[WAVES][K]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  float s = 0.f;
  if (tid < K) {
    s = red[0][tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w][tid];
  }
  return s;
}

// One wave per table blockIdx.x of rows x PITCH floats.  Lane l = COLS * slice + j: slice s of the 64 / COLS sums rows
// s, s + slices, ... of column j < PITCH with serial_sum8, the slices are joined by the xor tree COLS, 2 COLS, ... 32.
// ADD: lane j < n_out adds the total into dst[j] (one table).  Otherwise lane j < COLS stores it into word j of the
// block's 16 floats of dst, the words n_out.. as 0.f (a fresh result, pads included).
// PITCH is a template parameter: as a kernel argument the eight addresses of a step become a chain of seven dependent
// 64-bit additions in front of the loads instead of immediate offsets (measured: 1.3 us more over 3072 rows).
template <int COLS, int PITCH, bool ADD>
__global__ void __launch_bounds__(64)
rows_finish_kernel(int rows, const float* __restrict__ partials, float* __restrict__ dst, int n_out) {
  static_assert(COLS >= 1 && COLS <= 16 && 64 % COLS == 0 && PITCH <= COLS, "the store form writes the 16 words of a block");
  const int lane = threadIdx.x, j = lane % COLS, s = lane / COLS;
  const float* src = partials + (size_t)blockIdx.x * rows * PITCH;
  float acc = 0.f;
  if (j < PITCH) acc = serial_sum8(0.f, src + j, s, 64 / COLS, rows, PITCH);
#pragma unroll
  for (int o = COLS; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
  if (ADD) {
    if (lane < n_out) dst[lane] += acc;
  } else {
    if (lane < COLS) dst[(size_t)blockIdx.x * 16 + lane] = lane < n_out ? acc : 0.f;
  }
}

}  // namespace clmgs
