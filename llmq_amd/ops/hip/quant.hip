// Row-wise dynamic fp8 (OCP e4m3fn) activation quantisation for the W8A8
// projection GEMMs (gfx950), stand-alone and fused behind the producers of
// every GEMM input: the residual-add norms and the gated activations.
//
// Contract, for a bf16 row x[0..K):
//   a     = max(max_k |x[k]|, 1e-30f)
//   scale = a / 448.0f          inv = 448.0f / a        (IEEE fp32 divisions)
//   q[k]  = e4m3fn_rne(clamp(float(x[k]) * inv, -448, 448))
//
// The row maximum is needed before the first store, so one workgroup of 256
// threads holds its row in registers as the bf16 values the unfused kernel
// would have written (NV 16-byte vectors per thread, thread t owning
// elements t*8 + k*2048 as in elementwise.hip): each input is read from HBM
// once and the bf16 intermediate is never written. Stores are 8 packed fp8
// bytes per vector. The producers' arithmetic comes from elementwise.hip's
// helpers, so q and scale are those of quantising the unfused kernel's output.
// Included after elementwise.hip in the umbrella TU.

#include "common.h"

typedef __hip_bfloat16 bf16_t;
typedef Vec8<bf16_t> BVec;

#define QUANT_FP8_MAX 448.0f

DEVINL float amax8(const BVec& v, float m) {
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(to_f32(v.data[j])));
  return m;
}

DEVINL void store_quant8(__hip_fp8_e4m3* q, const BVec& v, float inv) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f[j] = fminf(fmaxf(to_f32(v.data[j]) * inv, -QUANT_FP8_MAX), QUANT_FP8_MAX);
  int2 w;
  w.x = pack4_fp8(f[0], f[1], f[2], f[3]);
  w.y = pack4_fp8(f[4], f[5], f[6], f[7]);
  *reinterpret_cast<int2*>(q) = w;
}

// Quantise the row this workgroup holds in v. q and scale point at the row.
template <int NV>
DEVINL void quant_row_regs(const BVec (&v)[NV], int hidden,
                           __hip_fp8_e4m3* __restrict__ q,
                           float* __restrict__ scale, float* red) {
  float amax = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) amax = amax8(v[k], amax);
  }
  const float a = fmaxf(block_reduce_max(amax, red), 1e-30f);
  const float inv = QUANT_FP8_MAX / a;
  if (threadIdx.x == 0) *scale = a / QUANT_FP8_MAX;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) store_quant8(q + i, v[k], inv);
  }
}

// ------------------------------------------------------------ stand-alone --

template <int NV>
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(
    __hip_fp8_e4m3* __restrict__ q, float* __restrict__ scale,
    const bf16_t* __restrict__ x, int hidden, long x_stride) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const bf16_t* xr = x + row * x_stride;
  BVec v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) v[k] = load16(xr + i);
  }
  quant_row_regs<NV>(v, hidden, q + row * hidden, scale + row, red);
}

// Rows longer than the register form covers: the second trip re-reads the
// row (from L2 at these sizes).
__global__ __launch_bounds__(256) void quant_fp8_rows_long_kernel(
    __hip_fp8_e4m3* __restrict__ q, float* __restrict__ scale,
    const bf16_t* __restrict__ x, int hidden, long x_stride) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const bf16_t* xr = x + row * x_stride;
  float amax = 0.f;
  for (int i = threadIdx.x * 8; i < hidden; i += 256 * 8)
    amax = amax8(load16(xr + i), amax);
  const float a = fmaxf(block_reduce_max(amax, red), 1e-30f);
  const float inv = QUANT_FP8_MAX / a;
  if (threadIdx.x == 0) scale[row] = a / QUANT_FP8_MAX;
  for (int i = threadIdx.x * 8; i < hidden; i += 256 * 8)
    store_quant8(q + row * hidden + i, load16(xr + i), inv);
}

// ------------------------------------------------------------ activations --
// in: [rows, 2*d] (gate || up) -> q [rows, d], scale [rows]

template <bool GELU, int NV>
__global__ __launch_bounds__(256) void act_and_mul_quant_kernel(
    __hip_fp8_e4m3* __restrict__ q, float* __restrict__ scale,
    const bf16_t* __restrict__ in, int d) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const bf16_t* g = in + row * 2 * d;
  BVec v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < d) {
      const BVec a = load16(g + i);
      const BVec b = load16(g + d + i);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[k].data[j] = from_f32<bf16_t>(
            act_mul_elem<GELU>(to_f32(a.data[j]), to_f32(b.data[j])));
    }
  }
  quant_row_regs<NV>(v, d, q + row * d, scale + row, red);
}

// ------------------------------------------------------------------ norms --

template <int NV>
__global__ __launch_bounds__(256) void rmsnorm_quant_kernel(
    __hip_fp8_e4m3* __restrict__ q, float* __restrict__ scale,
    const bf16_t* __restrict__ in, const bf16_t* __restrict__ weight,
    int hidden, float eps, float offset) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const bf16_t* x = in + row * hidden;
  BVec v[NV], w[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) {
      v[k] = load16(x + i);
      w[k] = load16(weight + i);
    }
  }
  // summation order of rmsnorm_kernel
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = to_f32(v[k].data[j]);
        ss += f * f;
      }
    }
  }
  ss = block_reduce_sum(ss, red);
  const float inv = rsqrtf(ss / hidden + eps);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[k].data[j] = from_f32<bf16_t>(
            norm_elem(to_f32(v[k].data[j]), inv, to_f32(w[k].data[j]), offset));
    }
  }
  quant_row_regs<NV>(v, hidden, q + row * hidden, scale + row, red);
}

// residual += x; (q, scale) = quant(rmsnorm(residual)). x is only read.
template <int NV>
__global__ __launch_bounds__(256) void fused_add_rmsnorm_quant_kernel(
    __hip_fp8_e4m3* __restrict__ q, float* __restrict__ scale,
    const bf16_t* __restrict__ x, bf16_t* __restrict__ residual,
    const bf16_t* __restrict__ weight, int hidden, float eps, float offset) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  const bf16_t* xr = x + row * hidden;
  bf16_t* rr = residual + row * hidden;
  BVec v[NV], w[NV];
  // summation order and rounding of fused_add_rmsnorm_kernel
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) {
      const BVec vx = load16(xr + i);
      const BVec vr = load16(rr + i);
      w[k] = load16(weight + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = to_f32(vx.data[j]) + to_f32(vr.data[j]);
        v[k].data[j] = from_f32<bf16_t>(f);
        f = to_f32(v[k].data[j]);
        ss += f * f;
      }
      store16(rr + i, v[k]);  // new residual
    }
  }
  ss = block_reduce_sum(ss, red);
  const float inv = rsqrtf(ss / hidden + eps);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = threadIdx.x * 8 + k * 256 * 8;
    if (i < hidden) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[k].data[j] = from_f32<bf16_t>(
            norm_elem(to_f32(v[k].data[j]), inv, to_f32(w[k].data[j]), offset));
    }
  }
  quant_row_regs<NV>(v, hidden, q + row * hidden, scale + row, red);
}

// Gemma-2 sandwich (norm_add_norm_regs_kernel's row body) with the normed
// row quantised instead of stored. x is only read.
template <int NV>
__global__ __launch_bounds__(256) void norm_add_norm_quant_kernel(
    __hip_fp8_e4m3* __restrict__ q, float* __restrict__ scale,
    const bf16_t* __restrict__ x, bf16_t* __restrict__ residual,
    const bf16_t* __restrict__ w_post, const bf16_t* __restrict__ w_pre,
    int hidden, float eps, float offset) {
  __shared__ float red[4];
  const long row = blockIdx.x;
  BVec o[NV];
  norm_add_norm_regs_row<bf16_t, NV>(x + row * hidden, residual + row * hidden,
                                     w_post, w_pre, hidden, eps, offset, red, o);
  quant_row_regs<NV>(o, hidden, q + row * hidden, scale + row, red);
}
