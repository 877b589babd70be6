// 3DGS-MCMC densification ("MCMC"; gsplat's MCMCStrategy): the three per-row operators of a training
// run with a fixed Gaussian budget.  None of them changes a front-end, tile or optimizer kernel.
//   mcmc_relocation : opacity and scale of a Gaussian that is about to exist `ratio` times (once per refinement, a few
//                     thousand rows; double arithmetic, one rounding at the store);
//   mcmc_reg_grad   : the gradients of w_o mean(sigmoid(opacity_raw)) + w_s mean(exp(scaling_raw)) ADDED into existing
//                     gradient storage, four separate tensors or the packed [N,12] tables (every batch, all N rows);
//   mcmc_noise      : xyz += Sigma (noise * gate * scaler), in place, optionally mirrored into the packed [N,12]
//                     parameter table (every batch, all N rows).
// The two per-batch passes are memory-bound; see the notes at each kernel for what is done in which precision and why.
#include "common.h"

namespace clmgs {

constexpr int MCMC_MAX_RATIO = 51;
constexpr float MCMC_GATE_K = 100.f;

// o' = 1 - (1 - o)^(1/r);  D = sum_{i=1..r} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1);  scale factor o / D.
// The inner sums share their k: sum_{i=k+1..r} C(i-1,k) = C(r,k+1) (hockey stick), so
//   D = sum_{k=0..r-1} (-1)^k C(r,k+1) o'^(k+1) / sqrt(k+1)
// -- the same terms grouped by k (same-signed terms are added first, so the sum is no worse conditioned), r of them
// instead of r(r+1)/2.  C(r,k+1) by the recurrence C(r,k+2) = C(r,k+1) (r-k-1) / (k+2): every product stays below 2^53
// (C(51,25) * 26 = 6.4e15), every quotient is an integer, so the binomials are exact doubles.  Powers by running product.
__global__ void __launch_bounds__(256)
mcmc_relocation_kernel(int64_t n, const float* __restrict__ opacities, const float* __restrict__ scales,
                       const int32_t* __restrict__ ratios, float* __restrict__ new_opacities,
                       float* __restrict__ new_scales) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = min(max(ratios[i], 1), MCMC_MAX_RATIO);
    const double o = (double)opacities[i];
    const double op = -expm1(log1p(-o) / (double)r);
    double c = (double)r, p = op, D = 0.0;
    for (int k = 0; k < r; ++k) {
      const double term = c * p / sqrt((double)(k + 1));
      D += (k & 1) ? -term : term;
      c = c * (double)(r - k - 1) / (double)(k + 2);
      p *= op;
    }
    const double f = o / D;
    new_opacities[i] = (float)op;
#pragma unroll
    for (int j = 0; j < 3; ++j) new_scales[3 * i + j] = (float)(f * (double)scales[3 * i + j]);
  }
}

// g_o += c_o s (1 - s), s = sigmoid(opacity_raw);  g_s[j] += c_s exp(scaling_raw[j]).
// PACKED: parameters and gradients are rows of [N,12] tables (xyz 3 | opacity 1 | scaling 3 | rotation 4 | pad): the two
// 16 B words of a row that hold the four columns are loaded as float4 (the lines of a 48 B row are fetched whole either
// way); the STORES are the four gradient columns only (4 B, 8 B, 4 B: column 7, a rotation gradient, is not written).
template <bool PACKED>
__global__ void __launch_bounds__(256)
mcmc_reg_grad_kernel(int64_t n, const float* __restrict__ o_raw, int64_t o_st, const float* __restrict__ s_raw,
                     int64_t s_st, float* __restrict__ g_o, int64_t go_st, float* __restrict__ g_s, int64_t gs_st,
                     float c_o, float c_s) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float po, ps[3], go, gs[3];
    float *dst_o, *dst_s;
    if constexpr (PACKED) {
      const float4* prow = reinterpret_cast<const float4*>(o_raw - 3 + 12 * i);
      float4* grow = reinterpret_cast<float4*>(g_o - 3 + 12 * i);
      const float4 p0 = prow[0], p1 = prow[1], g0 = grow[0], g1 = grow[1];
      po = p0.w; ps[0] = p1.x; ps[1] = p1.y; ps[2] = p1.z;
      go = g0.w; gs[0] = g1.x; gs[1] = g1.y; gs[2] = g1.z;
      dst_o = g_o + 12 * i;
      dst_s = dst_o + 1;
    } else {
      po = o_raw[o_st * i];
      dst_o = g_o + go_st * i;
      dst_s = g_s + gs_st * i;
      go = dst_o[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) { ps[j] = s_raw[s_st * i + j]; gs[j] = dst_s[j]; }
    }
    // s (1 - s) = e / (1 + e)^2 with e = exp(-|x|): no 1 - s, which cancels for large opacities
    const float e = expf(-fabsf(po)), d = 1.f + e;
    dst_o[0] = fmaf(c_o, e / (d * d), go);
    const float r0 = fmaf(c_s, expf(ps[0]), gs[0]), r1 = fmaf(c_s, expf(ps[1]), gs[1]), r2 = fmaf(c_s, expf(ps[2]), gs[2]);
    if constexpr (PACKED) {
      *reinterpret_cast<float2*>(dst_s) = make_float2(r0, r1);  // (column 4 of a 48 B row: 8 B aligned)
      dst_s[2] = r2;
    } else {
      dst_s[0] = r0; dst_s[1] = r1; dst_s[2] = r2;
    }
  }
}

// One row of the noise operator.  What is computed how:
//   gate = 1 / (1 + exp(-k ((1 - sigmoid(o_raw)) - x0))),  k = 100, x0 = 0.995:  float, written as k (0.005 - sigmoid).
//     The factor 100 turns an ABSOLUTE error of the sigmoid into a RELATIVE error of the gate; the float sigmoid's error
//     is relative to its own value, i.e. ~1e-9 absolute where the gate is not negligible (opacity <= ~0.05), and the
//     form 0.005 - s does not round s against 1 first.
//   Sigma v = R S^2 R^T v: double (the half-rate class; ~70 instructions, hidden behind the row's 68-80 B of traffic:
//     the pass runs at 1.03x a device copy of its bytes).
//     Off-diagonal entries of Sigma cancel (exactly, for equal scales), and the accuracy wanted is relative to the
//     entries, not to S^2.  R = M / |q|^2 with M the rotation formula of gs_math.h on the RAW quaternion: the
//     normalisation is one division by |q|^4 at the end and no square root.
//   xyz + dx: double, rounded once; dx == 0 keeps the stored bits (zero noise, a closed gate).
__device__ __forceinline__ void mcmc_noise_row(const float x[3], float o_raw, const float s_raw[3], const float q[4],
                                               const float e[3], float scaler, float out[3]) {
  const float o = 1.f / (1.f + expf(-o_raw));
  const float gate = 1.f / (1.f + expf(-MCMC_GATE_K * (0.005f - o)));
  const double g = (double)gate * (double)scaler;
  const double w = q[0], a = q[1], b = q[2], c = q[3];
  const double n2 = w * w + a * a + b * b + c * c;
  const double M[9] = {n2 - 2.0 * (b * b + c * c), 2.0 * (a * b - w * c),      2.0 * (a * c + w * b),
                       2.0 * (a * b + w * c),      n2 - 2.0 * (a * a + c * c), 2.0 * (b * c - w * a),
                       2.0 * (a * c - w * b),      2.0 * (b * c + w * a),      n2 - 2.0 * (a * a + b * b)};
  const double v[3] = {(double)e[0] * g, (double)e[1] * g, (double)e[2] * g};
  const double inv_n4 = 1.0 / (n2 * n2);
  double z[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double s = (double)expf(s_raw[k]);
    z[k] = s * s * (M[k] * v[0] + M[3 + k] * v[1] + M[6 + k] * v[2]);  // S^2 (M^T v)
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double dx = (M[3 * i] * z[0] + M[3 * i + 1] * z[1] + M[3 * i + 2] * z[2]) * inv_n4;
    out[i] = dx == 0.0 ? x[i] : (float)((double)x[i] + dx);
  }
}

__device__ __forceinline__ void mcmc_mirror_store(float* __restrict__ mirror, int64_t row, const float out[3]) {
  float* m = mirror + 12 * row;  // columns 0..2 of a 48 B row: 8 B + 4 B, columns 3..11 are not written
  *reinterpret_cast<float2*>(m) = make_float2(out[0], out[1]);
  m[2] = out[2];
}

// One lane per row.  The [n,3] tables are read with dword accesses at a 12 B stride: a wave instruction then covers 768
// contiguous bytes, and the three of a table hit the same twelve lines.  (Measured at 28 M rows against the form that
// gives a lane four rows and three 16 B accesses per table, i.e. a 48 B stride between lanes: 0.37 ms against 0.74 ms,
// profiles/mcmc_microbench.txt -- each 16 B access of that form touches 48 lines for a third of their bytes.)  Q16: the
// rotation, the one table whose rows ARE 16 B, is one 16 B load per lane when its base is aligned.
template <bool Q16>
__global__ void __launch_bounds__(256)
mcmc_noise_kernel(int64_t n, float* __restrict__ xyz, const float* __restrict__ o_raw, const float* __restrict__ s_raw,
                  const float* __restrict__ q_raw, const float* __restrict__ noise, float scaler,
                  float* __restrict__ mirror) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float x[3], s[3], e[3], q[4], out[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { x[j] = xyz[3 * i + j]; s[j] = s_raw[3 * i + j]; e[j] = noise[3 * i + j]; }
    if constexpr (Q16) {
      const float4 Q = reinterpret_cast<const float4*>(q_raw)[i];
      q[0] = Q.x; q[1] = Q.y; q[2] = Q.z; q[3] = Q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = q_raw[4 * i + j];
    }
    mcmc_noise_row(x, o_raw[i], s, q, e, scaler, out);
#pragma unroll
    for (int j = 0; j < 3; ++j) xyz[3 * i + j] = out[j];
    if (mirror) mcmc_mirror_store(mirror, i, out);
  }
}

}  // namespace clmgs

using namespace clmgs;

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int clmgs_mcmc_relocation(void* stream, int64_t n, const float* opacities, const float* scales,
                                     const int32_t* ratios, float* new_opacities, float* new_scales) {
  CLMGS_CHECK_ARG(n >= 0);
  if (n == 0) return 0;
  CLMGS_CHECK_ARG(opacities && scales && ratios && new_opacities && new_scales);
  hipLaunchKernelGGL(mcmc_relocation_kernel, dim3(min(ceil_div(n, 256), 256 * 8)), dim3(256), 0, (hipStream_t)stream, n,
                     opacities, scales, ratios, new_opacities, new_scales);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mcmc_reg_grad(void* stream, int64_t n, const float* opacity_raw, int64_t opacity_stride,
                                   const float* scaling_raw, int64_t scaling_stride, float* g_opacity,
                                   int64_t g_opacity_stride, float* g_scaling, int64_t g_scaling_stride, float c_o,
                                   float c_s) {
  CLMGS_CHECK_ARG(n >= 0);
  if (n == 0) return 0;
  CLMGS_CHECK_ARG(opacity_raw && scaling_raw && g_opacity && g_scaling);
  CLMGS_CHECK_ARG(opacity_stride >= 1 && scaling_stride >= 3 && g_opacity_stride >= 1 && g_scaling_stride >= 3);
  CLMGS_CHECK_ARG(c_o == c_o && c_s == c_s);
  const bool packed = opacity_stride == 12 && scaling_stride == 12 && g_opacity_stride == 12 && g_scaling_stride == 12 &&
                      scaling_raw == opacity_raw + 1 && g_scaling == g_opacity + 1 && aligned16(opacity_raw - 3) &&
                      aligned16(g_opacity - 3);
  hipLaunchKernelGGL(packed ? mcmc_reg_grad_kernel<true> : mcmc_reg_grad_kernel<false>,
                     dim3(min(ceil_div(n, 256), 256 * 32)), dim3(256), 0, (hipStream_t)stream, n, opacity_raw,
                     opacity_stride, scaling_raw, scaling_stride, g_opacity, g_opacity_stride, g_scaling, g_scaling_stride,
                     c_o, c_s);
  CLMGS_LAUNCH_CHECK();
  return 0;
}

extern "C" int clmgs_mcmc_noise(void* stream, int64_t n, float* xyz, const float* opacity_raw, const float* scaling_raw,
                                const float* rotation_raw, const float* noise, float scaler, float* packed_mirror) {
  CLMGS_CHECK_ARG(n >= 0);
  if (n == 0) return 0;
  CLMGS_CHECK_ARG(xyz && opacity_raw && scaling_raw && rotation_raw && noise && scaler == scaler);
  CLMGS_CHECK_ARG(!packed_mirror || (((uintptr_t)packed_mirror & 7) == 0));
  hipLaunchKernelGGL(aligned16(rotation_raw) ? mcmc_noise_kernel<true> : mcmc_noise_kernel<false>,
                     dim3(min(ceil_div(n, 256), 256 * 32)), dim3(256), 0, (hipStream_t)stream, n, xyz, opacity_raw,
                     scaling_raw, rotation_raw, noise, scaler, packed_mirror);
  CLMGS_LAUNCH_CHECK();
  return 0;
}
