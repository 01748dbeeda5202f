// Torch bindings for the llmq-amd CDNA4 kernels.
// Registered under torch.ops.llmq_amd.* ; loaded via torch.ops.load_library.

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <torch/library.h>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

// Kernel definitions are included BEFORE this file in the umbrella TU
// (ops.hip) — no forward declarations needed (stale declarations with
// narrower template parameter lists silently generate dead launch stubs).

namespace {

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda(), #x " must be on GPU")
#define CHECK_LASTDIM(x) \
  TORCH_CHECK(x.stride(-1) == 1, #x " innermost dim must be contiguous")

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

template <typename F>
void dispatch_dtype(const at::Tensor& t, const char* name, F&& f) {
  switch (t.scalar_type()) {
    case at::kBFloat16:
      f.template operator()<__hip_bfloat16>();
      break;
    case at::kHalf:
      f.template operator()<_Float16>();
      break;
    case at::kFloat:
      f.template operator()<float>();
      break;
    default:
      TORCH_CHECK(false, name, ": unsupported dtype ", t.scalar_type());
  }
}

// Calls f.template operator()<HD>() for the compile-time HD equal to D.
template <int... HDs, typename F>
void dispatch_head_dim(int D, F&& f) {
  const bool hit =
      ((D == HDs ? (f.template operator()<HDs>(), true) : false) || ...);
  TORCH_CHECK(hit, "unsupported head_dim ", D);
}

// KV-cache element type for activations T: T itself, or fp8 (bf16 only).
template <typename T, typename F>
void dispatch_cache_type(bool fp8_cache, F&& f) {
  if (!fp8_cache) {
    f.template operator()<T>();
  } else if constexpr (std::is_same_v<T, __hip_bfloat16>) {
    f.template operator()<__hip_fp8_e4m3>();
  } else {
    TORCH_CHECK(false, "fp8 KV cache requires bf16 activations");
  }
}

// ---------------------------------------------------------------- norms --

void rmsnorm(at::Tensor out, at::Tensor in, at::Tensor weight, double eps,
             double offset) {
  CHECK_GPU(in);
  CHECK_LASTDIM(in);
  const int hidden = in.size(-1);
  const long rows = in.numel() / hidden;
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  dispatch_dtype(in, "rmsnorm", [&]<typename T>() {
    hipLaunchKernelGGL(rmsnorm_kernel<T>, dim3(rows), dim3(256), 0, stream(),
                       reinterpret_cast<T*>(out.data_ptr()),
                       reinterpret_cast<const T*>(in.data_ptr()),
                       reinterpret_cast<const T*>(weight.data_ptr()), hidden,
                       (float)eps, (float)offset);
  });
}

void fused_add_rmsnorm(at::Tensor x, at::Tensor residual, at::Tensor weight,
                       double eps, double offset) {
  CHECK_GPU(x);
  CHECK_LASTDIM(x);
  const int hidden = x.size(-1);
  const long rows = x.numel() / hidden;
  dispatch_dtype(x, "fused_add_rmsnorm", [&]<typename T>() {
    hipLaunchKernelGGL(fused_add_rmsnorm_kernel<T>, dim3(rows), dim3(256), 0,
                       stream(), reinterpret_cast<T*>(x.data_ptr()),
                       reinterpret_cast<T*>(residual.data_ptr()),
                       reinterpret_cast<const T*>(weight.data_ptr()), hidden,
                       (float)eps, (float)offset);
  });
}

// ----------------------------------------------------------- activations --

template <bool GELU>
void act_and_mul(at::Tensor out, at::Tensor in) {
  CHECK_GPU(in);
  CHECK_LASTDIM(in);
  const int d = out.size(-1);
  const long rows = out.numel() / d;
  TORCH_CHECK(in.size(-1) == 2 * d, "in must be [..., 2*d]");
  const long chunks = rows * (d / 8);
  const int grid = std::min<long>((chunks + 255) / 256, 2048);
  dispatch_dtype(in, "act_and_mul", [&]<typename T>() {
    hipLaunchKernelGGL((act_and_mul_kernel<T, GELU>), dim3(grid), dim3(256), 0,
                       stream(), reinterpret_cast<T*>(out.data_ptr()),
                       reinterpret_cast<const T*>(in.data_ptr()), rows, d);
  });
}

void silu_and_mul(at::Tensor out, at::Tensor in) { act_and_mul<false>(out, in); }
void gelu_tanh_and_mul(at::Tensor out, at::Tensor in) { act_and_mul<true>(out, in); }

// ----------------------------------------------------------------- rope --

void rope_inplace(at::Tensor q, at::Tensor k, at::Tensor positions,
                  at::Tensor cos_sin) {
  CHECK_GPU(q);
  CHECK_LASTDIM(q);
  CHECK_LASTDIM(k);
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3, "q/k must be [T, H, D]");
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat, "cos_sin must be f32");
  const int T_ = q.size(0);
  if (T_ == 0) return;
  const int hq = q.size(1), hk = k.size(1), d = q.size(2);
  TORCH_CHECK(q.stride(1) == d && k.stride(1) == d, "head dim must be packed");
  dispatch_dtype(q, "rope", [&]<typename T>() {
    hipLaunchKernelGGL(rope_kernel<T>, dim3(T_), dim3(256), 0, stream(),
                       reinterpret_cast<T*>(q.data_ptr()),
                       reinterpret_cast<T*>(k.data_ptr()),
                       positions.data_ptr<long>(), cos_sin.data_ptr<float>(),
                       hq, hk, d, q.stride(0), k.stride(0));
  });
}

void norm_add_norm(at::Tensor x, at::Tensor residual, at::Tensor w_post,
                   at::Tensor w_pre, double eps, double offset) {
  CHECK_GPU(x);
  CHECK_LASTDIM(x);
  const int hidden = x.size(-1);
  const long rows = x.numel() / hidden;
  // Rows of up to 8192 bf16/half values are held in registers (2 or 4
  // 16-byte vectors per thread); anything else takes the three-trip kernel.
  // LLMQ_NORM_SANDWICH_REGS=0 selects the three-trip kernel everywhere (A/B
  // and the bitwise-equality test). Read per call, like LLMQ_DECODE_PIPE.
  const char* re = getenv("LLMQ_NORM_SANDWICH_REGS");
  const bool regs = (!re || atoi(re) != 0) && x.element_size() == 2 &&
                    hidden % 8 == 0 && hidden <= 8192;
  dispatch_dtype(x, "norm_add_norm", [&]<typename T>() {
    auto launch = [&](void (*kernel)(T*, T*, const T*, const T*, int, float,
                                     float)) {
      hipLaunchKernelGGL(kernel, dim3(rows), dim3(256), 0, stream(),
                         reinterpret_cast<T*>(x.data_ptr()),
                         reinterpret_cast<T*>(residual.data_ptr()),
                         reinterpret_cast<const T*>(w_post.data_ptr()),
                         reinterpret_cast<const T*>(w_pre.data_ptr()), hidden,
                         (float)eps, (float)offset);
    };
    if constexpr (sizeof(T) == 2) {
      if (regs) {
        launch(hidden <= 4096 ? norm_add_norm_regs_kernel<T, 2>
                              : norm_add_norm_regs_kernel<T, 4>);
        return;
      }
    }
    launch(norm_add_norm_kernel<T>);
  });
}

// ------------------------------------------------ fp8 row quantisation --

// Calls f.template operator()<NV>() for the smallest listed NV whose NV
// vectors per thread (256 threads x 8 elements) cover `hidden`.
template <int... NVs, typename F>
void dispatch_row_vecs(int hidden, const char* name, F&& f) {
  const bool hit = ((hidden <= NVs * 2048 ? (f.template operator()<NVs>(), true)
                                          : false) || ...);
  TORCH_CHECK(hit, name, ": row of ", hidden, " exceeds the register form");
}

// q [rows, hidden] fp8 and scale [rows] fp32 for `rows` bf16 rows.
void check_quant_out(const at::Tensor& q, const at::Tensor& scale, long rows,
                     int hidden) {
  CHECK_GPU(q);
  CHECK_GPU(scale);
  TORCH_CHECK(q.scalar_type() == at::kFloat8_e4m3fn && q.is_contiguous() &&
                  q.numel() == rows * hidden,
              "q must be contiguous float8_e4m3fn [rows, hidden]");
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.is_contiguous() &&
                  scale.numel() == rows,
              "scale must be contiguous float32 [rows]");
  TORCH_CHECK(hidden % 8 == 0, "row length must be a multiple of 8");
}

void check_bf16_rows(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                  t.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              what, " must be a contiguous, 16-byte aligned bf16 GPU tensor");
}

auto* fp8_ptr(at::Tensor& q) {
  return reinterpret_cast<__hip_fp8_e4m3*>(q.data_ptr());
}
const bf16_t* bf16_ptr(const at::Tensor& t) {
  return reinterpret_cast<const bf16_t*>(t.data_ptr());
}

constexpr int kQuantRegsMax = 16 * 2048;  // longest row quant.hip holds in registers
constexpr int kNormQuantMax = 4 * 2048;   // same for the fused norms

void quant_fp8_rows(at::Tensor q, at::Tensor scale, at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 &&
                  x.stride(1) == 1 && x.stride(0) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "x must be a 16-byte aligned bf16 [T, K] GPU tensor with unit "
              "inner stride and a row stride that is a multiple of 8");
  const int hidden = x.size(1);
  const long rows = x.size(0);
  check_quant_out(q, scale, rows, hidden);
  if (rows == 0) return;
  if (hidden > kQuantRegsMax) {
    hipLaunchKernelGGL(quant_fp8_rows_long_kernel, dim3(rows), dim3(256), 0,
                       stream(), fp8_ptr(q), scale.data_ptr<float>(),
                       bf16_ptr(x), hidden, (long)x.stride(0));
    return;
  }
  dispatch_row_vecs<1, 2, 4, 8, 16>(hidden, "quant_fp8_rows", [&]<int NV>() {
    hipLaunchKernelGGL(quant_fp8_rows_kernel<NV>, dim3(rows), dim3(256), 0,
                       stream(), fp8_ptr(q), scale.data_ptr<float>(),
                       bf16_ptr(x), hidden, (long)x.stride(0));
  });
}

template <bool GELU>
void act_and_mul_quant(at::Tensor q, at::Tensor scale, at::Tensor in) {
  check_bf16_rows(in, "gate_up");
  TORCH_CHECK(in.dim() == 2 && in.size(1) % 2 == 0, "gate_up must be [T, 2*d]");
  const int d = in.size(1) / 2;
  const long rows = in.size(0);
  check_quant_out(q, scale, rows, d);
  if (rows == 0) return;
  dispatch_row_vecs<1, 2, 4, 8, 16>(d, "act_and_mul_quant_fp8", [&]<int NV>() {
    hipLaunchKernelGGL((act_and_mul_quant_kernel<GELU, NV>), dim3(rows),
                       dim3(256), 0, stream(), fp8_ptr(q),
                       scale.data_ptr<float>(), bf16_ptr(in), d);
  });
}

void silu_and_mul_quant_fp8(at::Tensor q, at::Tensor scale, at::Tensor in) {
  act_and_mul_quant<false>(q, scale, in);
}
void gelu_tanh_and_mul_quant_fp8(at::Tensor q, at::Tensor scale, at::Tensor in) {
  act_and_mul_quant<true>(q, scale, in);
}

void check_norm_weight(const at::Tensor& w, int hidden) {
  check_bf16_rows(w, "norm weight");
  TORCH_CHECK(w.numel() == hidden, "norm weight must have `hidden` elements");
}

void rmsnorm_quant_fp8(at::Tensor q, at::Tensor scale, at::Tensor x,
                       at::Tensor weight, double eps, double offset) {
  check_bf16_rows(x, "x");
  TORCH_CHECK(x.dim() == 2, "x must be [T, hidden]");
  const int hidden = x.size(1);
  const long rows = x.size(0);
  check_quant_out(q, scale, rows, hidden);
  check_norm_weight(weight, hidden);
  if (rows == 0) return;
  dispatch_row_vecs<1, 2, 4>(hidden, "rmsnorm_quant_fp8", [&]<int NV>() {
    hipLaunchKernelGGL(rmsnorm_quant_kernel<NV>, dim3(rows), dim3(256), 0,
                       stream(), fp8_ptr(q), scale.data_ptr<float>(),
                       bf16_ptr(x), bf16_ptr(weight), hidden, (float)eps,
                       (float)offset);
  });
}

void fused_add_rmsnorm_quant_fp8(at::Tensor q, at::Tensor scale, at::Tensor x,
                                 at::Tensor residual, at::Tensor weight,
                                 double eps, double offset) {
  check_bf16_rows(x, "x");
  check_bf16_rows(residual, "residual");
  TORCH_CHECK(x.dim() == 2 && residual.sizes() == x.sizes(),
              "x and residual must both be [T, hidden]");
  const int hidden = x.size(1);
  const long rows = x.size(0);
  check_quant_out(q, scale, rows, hidden);
  check_norm_weight(weight, hidden);
  if (rows == 0) return;
  dispatch_row_vecs<1, 2, 4>(hidden, "fused_add_rmsnorm_quant_fp8", [&]<int NV>() {
    hipLaunchKernelGGL(fused_add_rmsnorm_quant_kernel<NV>, dim3(rows),
                       dim3(256), 0, stream(), fp8_ptr(q),
                       scale.data_ptr<float>(), bf16_ptr(x),
                       reinterpret_cast<bf16_t*>(residual.data_ptr()),
                       bf16_ptr(weight), hidden, (float)eps, (float)offset);
  });
}

void norm_add_norm_quant_fp8(at::Tensor q, at::Tensor scale, at::Tensor x,
                             at::Tensor residual, at::Tensor w_post,
                             at::Tensor w_pre, double eps, double offset) {
  check_bf16_rows(x, "x");
  check_bf16_rows(residual, "residual");
  TORCH_CHECK(x.dim() == 2 && residual.sizes() == x.sizes(),
              "x and residual must both be [T, hidden]");
  const int hidden = x.size(1);
  const long rows = x.size(0);
  check_quant_out(q, scale, rows, hidden);
  check_norm_weight(w_post, hidden);
  check_norm_weight(w_pre, hidden);
  if (rows == 0) return;
  dispatch_row_vecs<1, 2, 4>(hidden, "norm_add_norm_quant_fp8", [&]<int NV>() {
    hipLaunchKernelGGL(norm_add_norm_quant_kernel<NV>, dim3(rows), dim3(256),
                       0, stream(), fp8_ptr(q), scale.data_ptr<float>(),
                       bf16_ptr(x),
                       reinterpret_cast<bf16_t*>(residual.data_ptr()),
                       bf16_ptr(w_post), bf16_ptr(w_pre), hidden, (float)eps,
                       (float)offset);
  });
}

// ------------------------------------------------------------- KV cache --

void reshape_and_cache(at::Tensor key, at::Tensor value, at::Tensor k_cache,
                       at::Tensor v_cache, at::Tensor slot_mapping) {
  CHECK_GPU(key);
  CHECK_LASTDIM(key);
  const int T_ = key.size(0);
  if (T_ == 0) return;
  const int kvh = key.size(1), d = key.size(2);
  const int bs = k_cache.size(2);
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
  TORCH_CHECK(slot_mapping.scalar_type() == at::kLong);
  const bool fp8_cache = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  dispatch_dtype(key, "reshape_and_cache", [&]<typename T>() {
    dispatch_cache_type<T>(fp8_cache, [&]<typename TC>() {
      hipLaunchKernelGGL((reshape_and_cache_kernel<T, TC>), dim3(T_), dim3(128),
                         0, stream(), reinterpret_cast<const T*>(key.data_ptr()),
                         reinterpret_cast<const T*>(value.data_ptr()),
                         reinterpret_cast<TC*>(k_cache.data_ptr()),
                         reinterpret_cast<TC*>(v_cache.data_ptr()),
                         slot_mapping.data_ptr<long>(), kvh, d, bs,
                         key.stride(0), value.stride(0));
    });
  });
}

void rope_and_cache(at::Tensor q, at::Tensor k, at::Tensor value,
                    at::Tensor k_cache, at::Tensor v_cache,
                    at::Tensor positions, at::Tensor cos_sin,
                    at::Tensor slot_mapping) {
  CHECK_GPU(q);
  CHECK_LASTDIM(q);
  CHECK_LASTDIM(k);
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3, "q/k must be [T, H, D]");
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kLong);
  const int T_ = q.size(0);
  if (T_ == 0) return;
  const int hq = q.size(1), hk = k.size(1), d = q.size(2);
  const int bs = k_cache.size(2);
  TORCH_CHECK(q.stride(1) == d && k.stride(1) == d, "head dim must be packed");
  const bool fp8_cache = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  // Vector path: the fused QK-norm kernel's mapping with the norm compiled
  // out (16-lane group per head, 16-byte accesses, no per-element divide),
  // bit-identical to rope_and_cache_kernel. It covers 2-byte T at head dims
  // 64/128/256 when every address it forms is aligned for its pieces (see
  // qknorm_rope_and_cache); everything else keeps the scalar kernel.
  // LLMQ_ROPE_VEC=0 selects the scalar kernel everywhere (A/B and the
  // bitwise-equality test). Read per call, like LLMQ_DECODE_PIPE.
  const char* ve = getenv("LLMQ_ROPE_VEC");
  bool vec = !(ve && atoi(ve) == 0) && q.element_size() == 2 &&
             (d == 64 || d == 128 || d == 256);
  if (vec) {
    const long piece = std::min<long>(16, (d / 32) * 2);
    auto aligned = [&](const at::Tensor& t, long row_stride, long align) {
      return reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0 &&
             (row_stride * t.element_size()) % align == 0;
    };
    vec = value.dim() == 3 && value.stride(2) == 1 && value.stride(1) == d &&
          cos_sin.is_contiguous() && cos_sin.size(-1) == d &&
          k_cache.is_contiguous() && v_cache.is_contiguous() &&
          aligned(q, q.stride(0), piece) && aligned(k, k.stride(0), piece) &&
          aligned(value, value.stride(0), 16) && aligned(k_cache, 0, 16) &&
          aligned(v_cache, 0, 16) && aligned(cos_sin, 0, 16);
  }
  dispatch_dtype(q, "rope_and_cache", [&]<typename T>() {
    dispatch_cache_type<T>(fp8_cache, [&]<typename TC>() {
      if constexpr (sizeof(T) == 2) {
        if (vec) {
          dispatch_head_dim<64, 128, 256>(d, [&]<int HD>() {
            hipLaunchKernelGGL(
                (qknorm_rope_and_cache_kernel<T, TC, HD, false>), dim3(T_),
                dim3(256), 0, stream(), reinterpret_cast<T*>(q.data_ptr()),
                reinterpret_cast<T*>(k.data_ptr()),
                reinterpret_cast<const T*>(value.data_ptr()),
                reinterpret_cast<TC*>(k_cache.data_ptr()),
                reinterpret_cast<TC*>(v_cache.data_ptr()),
                (const T*)nullptr, (const T*)nullptr, 0.f, 0.f,
                positions.data_ptr<long>(), cos_sin.data_ptr<float>(),
                slot_mapping.data_ptr<long>(), hq, hk, bs, q.stride(0),
                k.stride(0), value.stride(0));
          });
          return;
        }
      }
      hipLaunchKernelGGL((rope_and_cache_kernel<T, TC>), dim3(T_), dim3(256), 0,
                         stream(), reinterpret_cast<T*>(q.data_ptr()),
                         reinterpret_cast<T*>(k.data_ptr()),
                         reinterpret_cast<const T*>(value.data_ptr()),
                         reinterpret_cast<TC*>(k_cache.data_ptr()),
                         reinterpret_cast<TC*>(v_cache.data_ptr()),
                         positions.data_ptr<long>(), cos_sin.data_ptr<float>(),
                         slot_mapping.data_ptr<long>(), hq, hk, d, bs,
                         q.stride(0), k.stride(0), value.stride(0));
    });
  });
}

// Qwen3: per-head RMSNorm on q and k fused in front of rope_and_cache.
void qknorm_rope_and_cache(at::Tensor q, at::Tensor k, at::Tensor value,
                           at::Tensor k_cache, at::Tensor v_cache,
                           at::Tensor q_weight, at::Tensor k_weight,
                           double eps, double offset, at::Tensor positions,
                           at::Tensor cos_sin, at::Tensor slot_mapping) {
  CHECK_GPU(q);
  CHECK_LASTDIM(q);
  CHECK_LASTDIM(k);
  CHECK_LASTDIM(value);
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && value.dim() == 3,
              "q/k/v must be [T, H, D]");
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kLong);
  TORCH_CHECK(positions.scalar_type() == at::kLong);
  const int T_ = q.size(0);
  if (T_ == 0) return;
  const int hq = q.size(1), hk = k.size(1), d = q.size(2);
  const int bs = k_cache.size(2);
  TORCH_CHECK(d == 64 || d == 128 || d == 256,
              "qknorm_rope_and_cache: head_dim must be 64, 128 or 256, got ", d);
  TORCH_CHECK(k.size(0) == T_ && value.size(0) == T_ &&
              positions.numel() == T_ && slot_mapping.numel() == T_,
              "k/v/positions/slot_mapping must have one row per token");
  TORCH_CHECK(k.size(2) == d && value.size(2) == d && value.size(1) == hk,
              "k/v head shape mismatch");
  TORCH_CHECK(k.scalar_type() == q.scalar_type() &&
              value.scalar_type() == q.scalar_type(), "q/k/v dtype mismatch");
  TORCH_CHECK(q.stride(1) == d && k.stride(1) == d && value.stride(1) == d,
              "head dim must be packed");
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
  TORCH_CHECK(k_cache.size(1) == hk && k_cache.size(3) == d &&
              v_cache.sizes() == k_cache.sizes(), "cache shape mismatch");
  TORCH_CHECK(cos_sin.is_contiguous() && cos_sin.size(-1) == d,
              "cos_sin must be contiguous [max_pos, head_dim]");
  for (const at::Tensor* w : {&q_weight, &k_weight}) {
    TORCH_CHECK(w->is_cuda() && w->is_contiguous() && w->numel() == d &&
                w->scalar_type() == q.scalar_type(),
                "q/k norm weights must be contiguous [head_dim] of q's dtype");
  }
  // A lane moves D/32 elements per half in pieces of at most 16 bytes; every
  // address it forms is base + row*stride + a multiple of that piece.
  const long esz = q.element_size();
  const long piece = std::min<long>(16, (d / 32) * esz);
  auto aligned = [&](const at::Tensor& t, long row_stride, long align) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0 &&
           (row_stride * t.element_size()) % align == 0;
  };
  TORCH_CHECK(aligned(q, q.stride(0), piece) && aligned(k, k.stride(0), piece) &&
              aligned(q_weight, 0, piece) && aligned(k_weight, 0, piece),
              "q/k/weights must be aligned to ", piece, " bytes");
  TORCH_CHECK(aligned(value, value.stride(0), 16) && aligned(k_cache, 0, 16) &&
              aligned(v_cache, 0, 16) && aligned(cos_sin, 0, 16),
              "value/caches/cos_sin must be 16-byte aligned");
  const bool fp8_cache = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(fp8_cache || k_cache.scalar_type() == q.scalar_type(),
              "cache dtype must be q's dtype or float8_e4m3fn");
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type());
  dispatch_dtype(q, "qknorm_rope_and_cache", [&]<typename T>() {
    dispatch_cache_type<T>(fp8_cache, [&]<typename TC>() {
      dispatch_head_dim<64, 128, 256>(d, [&]<int HD>() {
        hipLaunchKernelGGL(
            (qknorm_rope_and_cache_kernel<T, TC, HD>), dim3(T_), dim3(256), 0,
            stream(), reinterpret_cast<T*>(q.data_ptr()),
            reinterpret_cast<T*>(k.data_ptr()),
            reinterpret_cast<const T*>(value.data_ptr()),
            reinterpret_cast<TC*>(k_cache.data_ptr()),
            reinterpret_cast<TC*>(v_cache.data_ptr()),
            reinterpret_cast<const T*>(q_weight.data_ptr()),
            reinterpret_cast<const T*>(k_weight.data_ptr()), (float)eps,
            (float)offset, positions.data_ptr<long>(),
            cos_sin.data_ptr<float>(), slot_mapping.data_ptr<long>(), hq, hk,
            bs, q.stride(0), k.stride(0), value.stride(0));
      });
    });
  });
}

// Packed attention context of a prefill segment: gathered past rows from the
// paged cache followed by this step's fresh rows, per sequence. The caller
// guarantees what cannot be read here without a device sync: per sequence
// cu_seqlens_k spans at least cu_seqlens' rows, block_tables is wide enough
// for the longest past (W >= ceil(max P / bs)) and holds valid block ids,
// and the offsets stay inside k_out / k_fresh.
void gather_paged_kv(at::Tensor k_out, at::Tensor v_out, at::Tensor k_cache,
                     at::Tensor v_cache, at::Tensor k_fresh, at::Tensor v_fresh,
                     at::Tensor block_tables, at::Tensor cu_seqlens,
                     at::Tensor cu_seqlens_k, long max_seqlen_k) {
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda(), "caches must be on GPU");
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes(),
              "caches must be [blocks, kv_heads, block_size, head_dim]");
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous(),
              "caches must be contiguous");
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type(),
              "k_cache/v_cache dtype mismatch");
  const int kvh = k_cache.size(1), bs = k_cache.size(2), d = k_cache.size(3);
  const bool fp8_cache = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(fp8_cache || k_cache.scalar_type() == k_out.scalar_type(),
              "cache dtype must be the output dtype or float8_e4m3fn");
  // Rows move in 16-byte pieces of the cache dtype and of the output dtype.
  TORCH_CHECK(bs > 0 && d > 0 && (d * k_cache.element_size()) % 16 == 0 &&
                  (d * k_out.element_size()) % 16 == 0,
              "head_dim rows must be a multiple of 16 bytes");
  auto check_rows = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.dim() == 3 && t.size(1) == kvh && t.size(2) == d, name,
                " must be [rows, kv_heads, head_dim] of the cache's heads");
    TORCH_CHECK(t.scalar_type() == k_out.scalar_type(), name,
                " must have k_out's dtype");
    TORCH_CHECK(t.stride(2) == 1 && t.stride(1) == d, name,
                " must have unit last-dim stride and head stride == head_dim");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 &&
                    t.stride(0) * t.element_size() % 16 == 0,
                name, " must be 16-byte aligned with a row stride that is a "
                "multiple of 16 bytes");
  };
  check_rows(k_out, "k_out");
  check_rows(v_out, "v_out");
  check_rows(k_fresh, "k_fresh");
  check_rows(v_fresh, "v_fresh");
  TORCH_CHECK(v_out.size(0) == k_out.size(0) && v_fresh.size(0) == k_fresh.size(0),
              "k/v row counts must match");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % 16 == 0,
              "caches must be 16-byte aligned");
  auto check_offsets = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.dim() == 1 &&
                    t.is_contiguous(),
                name, " must be a contiguous 1-D int32 GPU tensor");
  };
  check_offsets(cu_seqlens, "cu_seqlens");
  check_offsets(cu_seqlens_k, "cu_seqlens_k");
  TORCH_CHECK(cu_seqlens.size(0) >= 1 &&
                  cu_seqlens.size(0) == cu_seqlens_k.size(0),
              "cu_seqlens and cu_seqlens_k must have equal length >= 1");
  const int B = cu_seqlens.size(0) - 1;
  TORCH_CHECK(block_tables.is_cuda() && block_tables.scalar_type() == at::kInt &&
                  block_tables.dim() == 2 && block_tables.size(0) == B &&
                  (block_tables.size(1) <= 1 || block_tables.stride(1) == 1),
              "block_tables must be a [B, W] int32 GPU tensor with contiguous rows");
  TORCH_CHECK(max_seqlen_k >= 0, "max_seqlen_k must be >= 0");
  if (B == 0 || max_seqlen_k == 0) return;
  dim3 grid((unsigned)((max_seqlen_k + GATHER_ROWS - 1) / GATHER_ROWS), B);
  dispatch_dtype(k_out, "gather_paged_kv", [&]<typename T>() {
    dispatch_cache_type<T>(fp8_cache, [&]<typename TC>() {
      hipLaunchKernelGGL(
          (gather_paged_kv_kernel<T, TC>), grid, dim3(GATHER_THREADS), 0,
          stream(), reinterpret_cast<T*>(k_out.data_ptr()),
          reinterpret_cast<T*>(v_out.data_ptr()),
          reinterpret_cast<const TC*>(k_cache.data_ptr()),
          reinterpret_cast<const TC*>(v_cache.data_ptr()),
          reinterpret_cast<const T*>(k_fresh.data_ptr()),
          reinterpret_cast<const T*>(v_fresh.data_ptr()),
          block_tables.data_ptr<int>(), cu_seqlens.data_ptr<int>(),
          cu_seqlens_k.data_ptr<int>(), kvh, d, bs, block_tables.stride(0),
          k_out.stride(0), v_out.stride(0), k_fresh.stride(0),
          v_fresh.stride(0));
    });
  });
}

// ------------------------------------------------------------ attention --

template <typename T>
void launch_decode(at::Tensor& out, const at::Tensor& q, const at::Tensor& kc,
                   const at::Tensor& vc, const at::Tensor& bt,
                   const at::Tensor& cl, double scale, double softcap,
                   long window) {
  const int B = q.size(0), H = q.size(1), D = q.size(2);
  const int KVH = kc.size(1);
  const int bs = kc.size(2);
  const int max_blocks = bt.size(1);
  const int G = H / KVH;
  TORCH_CHECK(H % KVH == 0, "num_heads must divide num_kv_heads");
  TORCH_CHECK(bs == 16 || bs == 32, "block_size must be 16 or 32");
  dim3 grid(B, KVH);
  // bf16 + MFMA-supported head dims → matrix-core kernels (G padded to 16),
  // 8 waves per workgroup.
  if constexpr (std::is_same_v<T, __hip_bfloat16>) {
    if ((D == 128 || D == 256) && G <= 16) {
      using BF = __hip_bfloat16;
      using F8 = __hip_fp8_e4m3;
      // Split-KV: when B×KVH under-fills the chip (TP ranks hold few kv
      // heads; small batches), split the context across z-workgroups and
      // merge fp32 partials. Target ≥512 workgroups (2 resident per CU).
      int nsplit = 1;
      while (B * KVH * nsplit < 512 && nsplit < 16) nsplit *= 2;
      at::Tensor scratch;
      float* scratch_ptr = nullptr;
      if (nsplit > 1) {
        scratch = at::empty({(long)B, KVH, nsplit, G, D + 2},
                            q.options().dtype(at::kFloat));
        scratch_ptr = scratch.data_ptr<float>();
      }
      dim3 sgrid(B, KVH, nsplit);
      // One launch for the whole MFMA family (one parameter list up to the
      // cache element type TC), then the split-KV merge if the context
      // was split.
      auto launch = [&]<int HD, typename TC>(void (*kernel)(
          BF*, const BF*, const TC*, const TC*, const int*, const int*, float*,
          int, int, int, int, float, float, int, long, long)) {
        hipLaunchKernelGGL(kernel, sgrid, dim3(8 * 64), 0, stream(),
                           reinterpret_cast<BF*>(out.data_ptr()),
                           reinterpret_cast<const BF*>(q.data_ptr()),
                           reinterpret_cast<const TC*>(kc.data_ptr()),
                           reinterpret_cast<const TC*>(vc.data_ptr()),
                           bt.data_ptr<int>(), cl.data_ptr<int>(), scratch_ptr,
                           H, KVH, bs, max_blocks, (float)scale,
                           (float)softcap, (int)window, q.stride(0),
                           out.stride(0));
        if (nsplit > 1) {
          hipLaunchKernelGGL((decode_splitkv_merge_kernel<HD>),
                             dim3(B, KVH, G), dim3(64), 0, stream(),
                             reinterpret_cast<BF*>(out.data_ptr()),
                             scratch_ptr, KVH, G, nsplit, out.stride(0));
        }
      };
      const bool fp8_cache = kc.scalar_type() == at::kFloat8_e4m3fn;
      // Software-pipelined glds kernels (default): LLMQ_DECODE_PIPE selects
      // the bf16 chunk size (>= 128 → 128 keys, else 64) or 0 = the
      // plain-staged kernel. Read per call so microbenches can A/B
      // in-process. Precondition: the whole block table staged in LDS (no
      // per-granule LDS-vs-global select — guide §5 trap 4c). fp8 caches
      // have their own pipe kernel (raw-fp8 staging + native packed cvt
      // VOPs: glds cannot convert during the LDS write).
      const char* pe = getenv("LLMQ_DECODE_PIPE");
      const int pipe_kt = pe ? atoi(pe) : 64;
      const bool pipe = pipe_kt > 0 && max_blocks <= PD_MAX_BT;
      // Cache policy of the pipe kernels' K/V stream: `nt` (default) on
      // the DMAs that consume whole lines streams the once-read cache past
      // L2 and the Infinity Cache. LLMQ_DECODE_KV_NT: 0 = the default-policy
      // instantiation (A/B runs and the equality tests), 1 = K only (bf16)
      // / K and raw V (fp8), 2 = also the bf16 V DMAs, which consume whole
      // lines only in the line image (fp8 and the subtile image: same as 1).
      // Read per call, like LLMQ_DECODE_PIPE.
      constexpr int DECODE_KV_NT_DEFAULT = 2;
      const char* nte = getenv("LLMQ_DECODE_KV_NT");
      const int kv_nt_env = nte ? atoi(nte) : DECODE_KV_NT_DEFAULT;
      const bool kv_nt = kv_nt_env != 0;
      auto dispatch_kv_nt = [&](auto&& f) {
        if (kv_nt) f.template operator()<true>();
        else f.template operator()<false>();
      };
      // V image of the bf16 pipe kernel: the line image (default), or
      // LLMQ_DECODE_V_LINES=0 = the tr16 subtile image (A/B baseline and the
      // equality test's other side). Read per call.
      const char* vle = getenv("LLMQ_DECODE_V_LINES");
      const bool v_lines = !(vle && atoi(vle) == 0);
      const int pipe_nt = kv_nt_env <= 0 ? 0 : (kv_nt_env >= 2 && v_lines) ? 2 : 1;
      auto dispatch_pipe_img = [&](auto&& f) {  // <KV_NT, V_LINES>
        if (!v_lines) {
          if (pipe_nt) f.template operator()<1, false>();
          else f.template operator()<0, false>();
        } else if (pipe_nt == 2) {
          f.template operator()<2, true>();
        } else if (pipe_nt == 1) {
          f.template operator()<1, true>();
        } else {
          f.template operator()<0, true>();
        }
      };
      // NREG: how many of a lane's 4 softmax registers hold q-heads with
      // the kernels' row placement (heads 4*reg .. 4*reg+3 in register reg):
      // ceil(G/4), with 3 rounded up to 4.
      auto dispatch_nreg = [&](auto&& f) {
        if (G <= 4) f.template operator()<1>();
        else if (G <= 8) f.template operator()<2>();
        else f.template operator()<4>();
      };
      dispatch_head_dim<128, 256>(D, [&]<int HD>() {
        dispatch_nreg([&]<int NREG>() {
          if (fp8_cache && pipe) {
            dispatch_kv_nt([&]<bool NT>() {
              launch.template operator()<HD, F8>(
                  paged_decode_pipe_fp8_kernel<HD, 8, NREG, NT>);
            });
          } else if (fp8_cache) {
            launch.template operator()<HD, F8>(
                paged_decode_mfma_kernel<HD, 8, NREG, F8>);
          } else if (pipe) {
            dispatch_pipe_img([&]<int NT, bool VL>() {
              launch.template operator()<HD, BF>(
                  pipe_kt >= 128 ? paged_decode_pipe_kernel<HD, 8, 128, NREG, NT, VL>
                                 : paged_decode_pipe_kernel<HD, 8, 64, NREG, NT, VL>);
            });
          } else {
            launch.template operator()<HD, BF>(
                paged_decode_mfma_kernel<HD, 8, NREG, BF>);
          }
        });
      });
      return;
    }
  }
  // The VALU fallback reads the cache as T; an fp8 cache reaching it would
  // be silently reinterpreted as bf16 (garbage, no error).
  TORCH_CHECK(kc.scalar_type() != at::kFloat8_e4m3fn,
              "fp8 KV cache requires the MFMA decode path (bf16 q, head_dim "
              "128/256, GQA group <= 16); got head_dim=", D, " group=", G);
  TORCH_CHECK(G <= 8, "GQA group must be <= 8 for the VALU decode kernel");
  const int subs = 256 / (32 * G);
  const int lds = (G * D + DECODE_CHUNK * G + subs * G * (D + 2)) * sizeof(float) +
                  16 * sizeof(int);
  dispatch_head_dim<64, 128, 256>(D, [&]<int HD>() {
    hipLaunchKernelGGL((paged_decode_attention_kernel<T, HD>), grid, dim3(256),
                       lds, stream(), reinterpret_cast<T*>(out.data_ptr()),
                       reinterpret_cast<const T*>(q.data_ptr()),
                       reinterpret_cast<const T*>(kc.data_ptr()),
                       reinterpret_cast<const T*>(vc.data_ptr()),
                       bt.data_ptr<int>(), cl.data_ptr<int>(), H, KVH, bs,
                       max_blocks, (float)scale, (float)softcap, (int)window,
                       q.stride(0), out.stride(0));
  });
}

void paged_decode_attention(at::Tensor out, at::Tensor q, at::Tensor k_cache,
                            at::Tensor v_cache, at::Tensor block_tables,
                            at::Tensor context_lens, double scale,
                            double softcap, long window) {
  CHECK_GPU(q);
  CHECK_LASTDIM(q);
  TORCH_CHECK(block_tables.scalar_type() == at::kInt);
  TORCH_CHECK(context_lens.scalar_type() == at::kInt);
  dispatch_dtype(q, "paged_decode_attention", [&]<typename T>() {
    launch_decode<T>(out, q, k_cache, v_cache, block_tables, context_lens,
                     scale, softcap, window);
  });
}

template <typename T>
void launch_prefill(at::Tensor& out, const at::Tensor& q, const at::Tensor& k,
                    const at::Tensor& v, const at::Tensor& cu,
                    const at::Tensor& cu_k, int B,
                    double scale, double softcap, long window, long max_seqlen) {
  const int H = q.size(1), D = q.size(2);
  const int KVH = k.size(1);
  // One launch for the two MFMA flash kernels and the VALU kernel (one
  // parameter list up to the element type).
  auto launch = [&]<typename E>(void (*kernel)(
      E*, const E*, const E*, const E*, const int*, const int*, int, int, float,
      float, int, long, long, long, long), dim3 grid) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream(),
                       reinterpret_cast<E*>(out.data_ptr()),
                       reinterpret_cast<const E*>(q.data_ptr()),
                       reinterpret_cast<const E*>(k.data_ptr()),
                       reinterpret_cast<const E*>(v.data_ptr()),
                       cu.data_ptr<int>(), cu_k.data_ptr<int>(), H, KVH,
                       (float)scale, (float)softcap, (int)window, q.stride(0),
                       k.stride(0), v.stride(0), out.stride(0));
  };
  if constexpr (std::is_same_v<T, __hip_bfloat16>) {
    // MFMA flash path (bf16): grid (seq, head, q-tile). Default: the glds
    // software-pipelined kernel; LLMQ_PREFILL_PIPE=0 selects the plain-
    // staged one (A/B). Read per call for in-process microbenches.
    const int qtiles = (int)((max_seqlen + 63) / 64);
    dim3 fgrid(B, H, std::max(qtiles, 1));
    const char* ppe = getenv("LLMQ_PREFILL_PIPE");
    const bool use_pipe = !ppe || atoi(ppe) != 0;
    dispatch_head_dim<64, 128, 256>(D, [&]<int HD>() {
      launch.template operator()<T>(use_pipe ? flash_prefill_pipe_kernel<HD>
                                             : flash_prefill_bf16_kernel<HD>,
                                    fgrid);
    });
    return;
  }
  dispatch_head_dim<64, 128, 256>(D, [&]<int HD>() {
    launch.template operator()<T>(varlen_prefill_attention_kernel<T, HD>,
                                  dim3(B, H));
  });
}

void varlen_prefill_attention(at::Tensor out, at::Tensor q, at::Tensor k,
                              at::Tensor v, at::Tensor cu_seqlens,
                              at::Tensor cu_seqlens_k,
                              long max_seqlen, double scale, double softcap,
                              long window) {
  // The kernels address row*stride(0) + head*D + d and stage K/V (bf16: Q
  // too) with 16-byte loads; anything else would be reinterpreted silently.
  auto check_operand = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.dim() == 3, name, " must be [tokens, heads, head_dim]");
    TORCH_CHECK(t.scalar_type() == q.scalar_type(), name,
                " must have q's dtype");
    TORCH_CHECK(t.size(2) == q.size(2), name, " must have q's head_dim");
    TORCH_CHECK(t.stride(2) == 1 && t.stride(1) == t.size(2), name,
                " must have unit last-dim stride and head stride == head_dim");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 &&
                    t.stride(0) * t.element_size() % 16 == 0,
                name, " must be 16-byte aligned with a row stride that is a "
                "multiple of 16 bytes");
  };
  TORCH_CHECK(q.dim() == 3, "q must be [tokens, heads, head_dim]");
  check_operand(q, "q");
  check_operand(k, "k");
  check_operand(v, "v");
  check_operand(out, "out");
  TORCH_CHECK(out.sizes() == q.sizes(), "out must have q's shape");
  TORCH_CHECK(v.sizes() == k.sizes(), "v must have k's shape");
  TORCH_CHECK(k.size(1) > 0 && q.size(1) % k.size(1) == 0,
              "num_heads must be a multiple of num_kv_heads");
  auto check_offsets = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.dim() == 1 &&
                    t.is_contiguous(),
                name, " must be a contiguous 1-D int32 GPU tensor");
  };
  check_offsets(cu_seqlens, "cu_seqlens");
  check_offsets(cu_seqlens_k, "cu_seqlens_k");
  TORCH_CHECK(cu_seqlens.size(0) >= 1 &&
                  cu_seqlens.size(0) == cu_seqlens_k.size(0),
              "cu_seqlens and cu_seqlens_k must have equal length >= 1");
  TORCH_CHECK(window >= 0 && max_seqlen >= 0,
              "window and max_seqlen must be >= 0");
  const int B = cu_seqlens.size(0) - 1;
  if (B == 0 || q.size(0) == 0) return;
  dispatch_dtype(q, "varlen_prefill_attention", [&]<typename T>() {
    launch_prefill<T>(out, q, k, v, cu_seqlens, cu_seqlens_k, B, scale,
                      softcap, window, max_seqlen);
  });
}

// ---------------------------------------------------------- skinny GEMM --

void skinny_gemm(at::Tensor out, at::Tensor x, at::Tensor w,
                 c10::optional<at::Tensor> bias, long splitk) {
  CHECK_GPU(x);
  CHECK_GPU(w);
  CHECK_GPU(out);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && out.dim() == 2);
  CHECK_LASTDIM(x);
  CHECK_LASTDIM(w);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16);
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.is_contiguous());
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && out.size(0) == M && out.size(1) == N);
  TORCH_CHECK(M > 0 && N > 0 && K > 0);
  TORCH_CHECK(K % SKG_BK == 0, "K must be a multiple of 64");
  TORCH_CHECK(N % 4 == 0, "N must be a multiple of 4");
  // Staging moves 16-byte granules from src + row * stride + col (col a
  // multiple of 8 elements): base and row pitch must keep them aligned.
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "x and w must be 16-byte aligned");
  TORCH_CHECK(x.stride(0) % 8 == 0 && w.stride(0) % 8 == 0,
              "x and w row strides must be multiples of 8 elements");
  TORCH_CHECK(splitk >= 0, "splitk must be >= 0 (0 = auto)");
  const __hip_bfloat16* bias_ptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    CHECK_GPU((*bias));
    TORCH_CHECK(bias->scalar_type() == at::kBFloat16 && bias->numel() == N);
    TORCH_CHECK(bias->is_contiguous(), "bias must be contiguous");
    bias_ptr = reinterpret_cast<const __hip_bfloat16*>(bias->data_ptr());
  }
  const int mt = (M + SKG_BM - 1) / SKG_BM;
  const int nt = (N + SKG_BN - 1) / SKG_BN;
  const int ksteps = K / SKG_BK;
  int z = (int)splitk;
  if (z <= 0) {  // auto: fill the chip (>=256 blocks), keep >=8 K-steps/slice
    z = 1;
    while (mt * nt * z < 256 && ksteps / (z * 2) >= 8 && z < 8) z *= 2;
  }
  // The kernel gives each slice per = ceil(ksteps / z) steps; drop the
  // slices that rule leaves empty, so the reduce only reads written slabs.
  const int per = (ksteps + z - 1) / z;
  z = (ksteps + per - 1) / per;
  dim3 grid(mt, nt, z);
  // Debug staging (plain loads + __syncthreads instead of the glds
  // pipeline). Read per call, like LLMQ_DECODE_PIPE.
  const char* sync_env = getenv("LLMQ_SKG_SYNC");
  const bool sync_dbg = sync_env && atoi(sync_env) != 0;
  auto launch = [&](void (*kernel)(void*, const __hip_bfloat16*,
                                   const __hip_bfloat16*, const __hip_bfloat16*,
                                   int, int, int, long, long),
                    void* dst, const __hip_bfloat16* bias_arg) {
    hipLaunchKernelGGL(kernel, grid, dim3(SKG_NT), 0, stream(), dst,
                       reinterpret_cast<const __hip_bfloat16*>(x.data_ptr()),
                       reinterpret_cast<const __hip_bfloat16*>(w.data_ptr()),
                       bias_arg, M, N, K, x.stride(0), w.stride(0));
  };
  if (z == 1) {
    launch(sync_dbg ? skinny_gemm_kernel<0, 1> : skinny_gemm_kernel<0>,
           out.data_ptr(), bias_ptr);
    return;
  }
  at::Tensor slabs = at::empty({z, (long)M * N}, x.options().dtype(at::kFloat));
  launch(sync_dbg ? skinny_gemm_kernel<1, 1> : skinny_gemm_kernel<1>,
         slabs.data_ptr(), nullptr);
  const long MN = (long)M * N;
  const long blocks = (MN / 4 + 255) / 256;
  hipLaunchKernelGGL(skinny_gemm_reduce_kernel, dim3(blocks), dim3(256), 0,
                     stream(),
                     reinterpret_cast<__hip_bfloat16*>(out.data_ptr()),
                     slabs.data_ptr<float>(), bias_ptr, z, MN, N);
}

// ------------------------------------------------------------- sampling --

// Logits arrive as the lm_head GEMM stored them (bf16/half) or as fp32;
// softcap > 0 applies cap * tanh(x / cap) in registers (logit_value), with
// the reciprocal formed here in fp32 as torch forms it for `logits / cap`.
float softcap_reciprocal(double softcap) {
  return softcap > 0 ? 1.0f / (float)softcap : 0.0f;
}

// The penalty arguments of the two sampler ops: the count table [nslots, vpad]
// (int16, read as unsigned), a per-row int32 slot (-1 = none) and per-row
// fp32 (r, freq, pres). All three or none.
struct PenaltyArgs {
  const unsigned short* table = nullptr;
  const int* slots = nullptr;
  const float* params = nullptr;
  int nslots = 0;
  long vpad = 0;
};

PenaltyArgs penalty_args(const c10::optional<at::Tensor>& table,
                         const c10::optional<at::Tensor>& slots,
                         const c10::optional<at::Tensor>& params, int B, int V) {
  PenaltyArgs a;
  const bool has = table.has_value() && table->defined();
  TORCH_CHECK(has == (slots.has_value() && slots->defined()) &&
                  has == (params.has_value() && params->defined()),
              "pen_table, pen_slots and pen_params go together");
  if (!has) return a;
  CHECK_GPU((*table));
  CHECK_GPU((*slots));
  CHECK_GPU((*params));
  TORCH_CHECK(table->scalar_type() == at::kShort && table->dim() == 2 &&
              table->is_contiguous() && table->size(1) >= V);
  TORCH_CHECK(slots->scalar_type() == at::kInt && slots->is_contiguous() &&
              slots->numel() == B);
  TORCH_CHECK(params->scalar_type() == at::kFloat && params->is_contiguous() &&
              params->dim() == 2 && params->size(0) == B && params->size(1) == 3);
  a.table = reinterpret_cast<const unsigned short*>(table->data_ptr());
  a.slots = slots->data_ptr<int>();
  a.params = params->data_ptr<float>();
  a.nslots = table->size(0);
  a.vpad = table->size(1);
  return a;
}

void topk_topp_bound(at::Tensor out_bound, at::Tensor logits, at::Tensor temps,
                     at::Tensor top_ps, at::Tensor top_ks, double softcap,
                     c10::optional<at::Tensor> min_ps,
                     c10::optional<at::Tensor> pen_table,
                     c10::optional<at::Tensor> pen_slots,
                     c10::optional<at::Tensor> pen_params) {
  CHECK_GPU(logits);
  CHECK_LASTDIM(logits);
  TORCH_CHECK(logits.dim() == 2);
  TORCH_CHECK(out_bound.scalar_type() == at::kFloat);
  TORCH_CHECK(temps.scalar_type() == at::kFloat);
  TORCH_CHECK(top_ps.scalar_type() == at::kFloat);
  TORCH_CHECK(top_ks.scalar_type() == at::kLong);
  const int B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(out_bound.numel() == B && temps.numel() == B &&
              top_ps.numel() == B && top_ks.numel() == B);
  const float* min_ps_ptr = nullptr;
  if (min_ps.has_value() && min_ps->defined()) {
    CHECK_GPU((*min_ps));
    TORCH_CHECK(min_ps->scalar_type() == at::kFloat && min_ps->numel() == B &&
                min_ps->is_contiguous());
    min_ps_ptr = min_ps->data_ptr<float>();
  }
  const PenaltyArgs pen = penalty_args(pen_table, pen_slots, pen_params, B, V);
  if (B == 0) return;
  dispatch_dtype(logits, "topk_topp_bound", [&]<typename T>() {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, stream(),
                         out_bound.data_ptr<float>(),
                         reinterpret_cast<const T*>(logits.data_ptr()),
                         temps.data_ptr<float>(), top_ps.data_ptr<float>(),
                         top_ks.data_ptr<long>(), V, logits.stride(0),
                         (float)softcap, softcap_reciprocal(softcap),
                         min_ps_ptr, pen.table, pen.slots, pen.params,
                         pen.nslots, pen.vpad);
    };
    // without min_p and penalties: the kernel as it was before it had them
    if (min_ps_ptr || pen.table) launch(topk_topp_bound_kernel<T, true>);
    else launch(topk_topp_bound_kernel<T, false>);
  });
}

void sample_gumbel_argmax(at::Tensor out, at::Tensor keys, at::Tensor logits,
                          at::Tensor temps, at::Tensor req_seeds,
                          at::Tensor req_pos, long seed, long step,
                          c10::optional<at::Tensor> bounds, double softcap,
                          c10::optional<at::Tensor> pen_table,
                          c10::optional<at::Tensor> pen_slots,
                          c10::optional<at::Tensor> pen_params) {
  CHECK_GPU(logits);
  CHECK_LASTDIM(logits);
  TORCH_CHECK(logits.dim() == 2);
  TORCH_CHECK(temps.scalar_type() == at::kFloat);
  TORCH_CHECK(out.scalar_type() == at::kLong);
  TORCH_CHECK(keys.scalar_type() == at::kLong && keys.numel() == logits.size(0));
  TORCH_CHECK(req_seeds.scalar_type() == at::kInt);
  TORCH_CHECK(req_pos.scalar_type() == at::kInt);
  const int B = logits.size(0), V = logits.size(1);
  const float* bounds_ptr = nullptr;
  if (bounds.has_value() && bounds->defined()) {
    TORCH_CHECK(bounds->scalar_type() == at::kFloat && bounds->numel() == B);
    bounds_ptr = bounds->data_ptr<float>();
  }
  const PenaltyArgs pen = penalty_args(pen_table, pen_slots, pen_params, B, V);
  // enough splits to fill the chip at small B
  int nsplit = 1;
  while (B * nsplit < 2048 && nsplit < 64 && (V / nsplit) > 4096) nsplit *= 2;
  // chunk a multiple of 8: with V % 8 == 0 every split starts on a 16-byte
  // boundary of its row and is all vector loads
  const int chunk = ((V + nsplit - 1) / nsplit + 7) / 8 * 8;
  dispatch_dtype(logits, "sample_gumbel_argmax", [&]<typename T>() {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(
          kernel, dim3(B, nsplit), dim3(256), 0, stream(),
          reinterpret_cast<unsigned long long*>(keys.data_ptr()),
          reinterpret_cast<const T*>(logits.data_ptr()), temps.data_ptr<float>(),
          reinterpret_cast<const unsigned int*>(req_seeds.data_ptr()),
          reinterpret_cast<const unsigned int*>(req_pos.data_ptr()), bounds_ptr,
          V, logits.stride(0), chunk, (float)softcap,
          softcap_reciprocal(softcap), (unsigned int)seed, (unsigned int)step,
          pen.table, pen.slots, pen.params, pen.nslots, pen.vpad);
    };
    // without a table: the kernel as it was before it had penalties
    if (pen.table) launch(sample_argmax_kernel<T, true>);
    else launch(sample_argmax_kernel<T, false>);
  });
  hipLaunchKernelGGL(unpack_keys_kernel, dim3((B + 255) / 256), dim3(256), 0,
                     stream(), out.data_ptr<long>(),
                     reinterpret_cast<const unsigned long long*>(keys.data_ptr()),
                     B);
}

// Adds the tokens just sampled to their rows' output counts, on the current
// stream, reading the token tensor on the device.
void penalty_count_tokens(at::Tensor table, at::Tensor slots, at::Tensor tokens) {
  CHECK_GPU(table);
  CHECK_GPU(slots);
  CHECK_GPU(tokens);
  TORCH_CHECK(table.scalar_type() == at::kShort && table.dim() == 2 &&
              table.is_contiguous());
  TORCH_CHECK(slots.scalar_type() == at::kInt && slots.is_contiguous());
  TORCH_CHECK(tokens.scalar_type() == at::kLong && tokens.is_contiguous() &&
              tokens.numel() == slots.numel());
  const int B = slots.numel();
  if (B == 0) return;
  hipLaunchKernelGGL(penalty_count_tokens_kernel, dim3((B + 255) / 256),
                     dim3(256), 0, stream(),
                     reinterpret_cast<unsigned short*>(table.data_ptr()),
                     slots.data_ptr<int>(), tokens.data_ptr<long>(), B,
                     (int)table.size(0), (long)table.size(1));
}

// Logprob of tokens[rows[r]], its rank and the K most likely tokens of row
// rows[r], for each requested row r (torch_ref.token_logprobs), on the
// current stream. The outputs may be column slices of wider buffers.
// threads: workgroup size, 0 = the default.
void token_logprobs(at::Tensor lp_out, at::Tensor ids_out, at::Tensor rank_out,
                    at::Tensor logits, at::Tensor rows, at::Tensor tokens,
                    long K, double softcap, long threads) {
  CHECK_GPU(logits);
  CHECK_GPU(rows);
  CHECK_GPU(tokens);
  CHECK_GPU(lp_out);
  CHECK_GPU(ids_out);
  CHECK_GPU(rank_out);
  CHECK_LASTDIM(logits);
  TORCH_CHECK(logits.dim() == 2);
  const int B = logits.size(0), V = logits.size(1);
  const long R = rows.numel();
  TORCH_CHECK(B >= 1 && V >= 1);
  TORCH_CHECK(K >= 0 && K <= LP_MAX_K && K <= V, "token_logprobs: K must be in "
              "[0, min(", LP_MAX_K, ", V)], got ", K);
  TORCH_CHECK(rows.scalar_type() == at::kInt && rows.is_contiguous());
  TORCH_CHECK(tokens.scalar_type() == at::kLong && tokens.is_contiguous() &&
              tokens.numel() == B);
  TORCH_CHECK(lp_out.scalar_type() == at::kFloat && lp_out.dim() == 2 &&
              lp_out.size(0) == R && lp_out.size(1) == 1 + K);
  TORCH_CHECK(ids_out.scalar_type() == at::kInt && ids_out.dim() == 2 &&
              ids_out.size(0) == R && ids_out.size(1) == 1 + K);
  TORCH_CHECK(rank_out.scalar_type() == at::kInt && rank_out.dim() == 1 &&
              rank_out.size(0) == R);
  CHECK_LASTDIM(lp_out);
  CHECK_LASTDIM(ids_out);
  TORCH_CHECK(threads == 0 || threads == 512 || threads == 1024,
              "token_logprobs: threads must be 0, 512 or 1024");
  if (R == 0) return;
  dispatch_dtype(logits, "token_logprobs", [&]<typename T>() {
    auto launch = [&](auto kernel, int nt) {
      hipLaunchKernelGGL(
          kernel, dim3(R), dim3(nt), 0, stream(), lp_out.data_ptr<float>(),
          ids_out.data_ptr<int>(), rank_out.data_ptr<int>(),
          reinterpret_cast<const T*>(logits.data_ptr()), rows.data_ptr<int>(),
          tokens.data_ptr<long>(), B, V, logits.stride(0), (int)K,
          lp_out.stride(0), ids_out.stride(0), rank_out.stride(0),
          (float)softcap, softcap_reciprocal(softcap));
    };
    if (threads == 512) {
      if (K > 0) launch(token_logprobs_kernel<T, 512, true>, 512);
      else launch(token_logprobs_kernel<T, 512, false>, 512);
    } else {
      if (K > 0) launch(token_logprobs_kernel<T, 1024, true>, 1024);
      else launch(token_logprobs_kernel<T, 1024, false>, 1024);
    }
  });
}

}  // namespace

TORCH_LIBRARY(llmq_amd, m) {
  m.def("token_logprobs(Tensor(a!) lp_out, Tensor(b!) ids_out, Tensor(c!) rank_out, Tensor logits, Tensor rows, Tensor tokens, int K, float softcap=0.0, int threads=0) -> ()");
  m.def("rmsnorm(Tensor(a!) out, Tensor input, Tensor weight, float eps, float offset) -> ()");
  m.def("fused_add_rmsnorm(Tensor(a!) x, Tensor(b!) residual, Tensor weight, float eps, float offset) -> ()");
  m.def("silu_and_mul(Tensor(a!) out, Tensor input) -> ()");
  m.def("gelu_tanh_and_mul(Tensor(a!) out, Tensor input) -> ()");
  m.def("rope_inplace(Tensor(a!) q, Tensor(b!) k, Tensor positions, Tensor cos_sin) -> ()");
  m.def("reshape_and_cache(Tensor key, Tensor value, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor slot_mapping) -> ()");
  m.def("paged_decode_attention(Tensor(a!) out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor context_lens, float scale, float softcap, int window) -> ()");
  m.def("varlen_prefill_attention(Tensor(a!) out, Tensor q, Tensor k, Tensor v, Tensor cu_seqlens, Tensor cu_seqlens_k, int max_seqlen, float scale, float softcap, int window) -> ()");
  m.def("sample_gumbel_argmax(Tensor(a!) out, Tensor(b!) keys, Tensor logits, Tensor temps, Tensor req_seeds, Tensor req_pos, int seed, int step, Tensor? bounds=None, float softcap=0.0, Tensor? pen_table=None, Tensor? pen_slots=None, Tensor? pen_params=None) -> ()");
  m.def("topk_topp_bound(Tensor(a!) out_bound, Tensor logits, Tensor temps, Tensor top_ps, Tensor top_ks, float softcap=0.0, Tensor? min_ps=None, Tensor? pen_table=None, Tensor? pen_slots=None, Tensor? pen_params=None) -> ()");
  m.def("penalty_count_tokens(Tensor(a!) table, Tensor slots, Tensor tokens) -> ()");
  m.def("skinny_gemm(Tensor(a!) out, Tensor x, Tensor w, Tensor? bias, int splitk) -> ()");
  m.def("quant_fp8_rows(Tensor(a!) q, Tensor(b!) scale, Tensor x) -> ()");
  m.def("silu_and_mul_quant_fp8(Tensor(a!) q, Tensor(b!) scale, Tensor gate_up) -> ()");
  m.def("gelu_tanh_and_mul_quant_fp8(Tensor(a!) q, Tensor(b!) scale, Tensor gate_up) -> ()");
  m.def("rmsnorm_quant_fp8(Tensor(a!) q, Tensor(b!) scale, Tensor x, Tensor weight, float eps, float offset) -> ()");
  m.def("fused_add_rmsnorm_quant_fp8(Tensor(a!) q, Tensor(b!) scale, Tensor x, Tensor(c!) residual, Tensor weight, float eps, float offset) -> ()");
  m.def("norm_add_norm_quant_fp8(Tensor(a!) q, Tensor(b!) scale, Tensor x, Tensor(c!) residual, Tensor w_post, Tensor w_pre, float eps, float offset) -> ()");
  m.def("norm_add_norm(Tensor(a!) x, Tensor(b!) residual, Tensor w_post, Tensor w_pre, float eps, float offset) -> ()");
  m.def("rope_and_cache(Tensor(a!) q, Tensor(b!) k, Tensor value, Tensor(c!) k_cache, Tensor(d!) v_cache, Tensor positions, Tensor cos_sin, Tensor slot_mapping) -> ()");
  m.def("qknorm_rope_and_cache(Tensor(a!) q, Tensor(b!) k, Tensor value, Tensor(c!) k_cache, Tensor(d!) v_cache, Tensor q_weight, Tensor k_weight, float eps, float offset, Tensor positions, Tensor cos_sin, Tensor slot_mapping) -> ()");
  m.def("gather_paged_kv(Tensor(a!) k_out, Tensor(b!) v_out, Tensor k_cache, Tensor v_cache, Tensor k_fresh, Tensor v_fresh, Tensor block_tables, Tensor cu_seqlens, Tensor cu_seqlens_k, int max_seqlen_k) -> ()");
}

TORCH_LIBRARY_IMPL(llmq_amd, CUDA, m) {
  m.impl("rmsnorm", &rmsnorm);
  m.impl("fused_add_rmsnorm", &fused_add_rmsnorm);
  m.impl("silu_and_mul", &silu_and_mul);
  m.impl("gelu_tanh_and_mul", &gelu_tanh_and_mul);
  m.impl("rope_inplace", &rope_inplace);
  m.impl("reshape_and_cache", &reshape_and_cache);
  m.impl("paged_decode_attention", &paged_decode_attention);
  m.impl("varlen_prefill_attention", &varlen_prefill_attention);
  m.impl("sample_gumbel_argmax", &sample_gumbel_argmax);
  m.impl("topk_topp_bound", &topk_topp_bound);
  m.impl("penalty_count_tokens", &penalty_count_tokens);
  m.impl("token_logprobs", &token_logprobs);
  m.impl("skinny_gemm", &skinny_gemm);
  m.impl("norm_add_norm", &norm_add_norm);
  m.impl("quant_fp8_rows", &quant_fp8_rows);
  m.impl("silu_and_mul_quant_fp8", &silu_and_mul_quant_fp8);
  m.impl("gelu_tanh_and_mul_quant_fp8", &gelu_tanh_and_mul_quant_fp8);
  m.impl("rmsnorm_quant_fp8", &rmsnorm_quant_fp8);
  m.impl("fused_add_rmsnorm_quant_fp8", &fused_add_rmsnorm_quant_fp8);
  m.impl("norm_add_norm_quant_fp8", &norm_add_norm_quant_fp8);
  m.impl("rope_and_cache", &rope_and_cache);
  m.impl("qknorm_rope_and_cache", &qknorm_rope_and_cache);
  m.impl("gather_paged_kv", &gather_paged_kv);
}
