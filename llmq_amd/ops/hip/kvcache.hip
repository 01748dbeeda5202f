// Paged-KV scatter: write this step's k/v vectors into the paged cache.
// Cache layout: [num_blocks, kv_heads, block_size, head_dim] (a (block,head)
// pair is a contiguous [block_size, head_dim] tile for the decode kernel).

#include "common.h"

template <typename T, typename TC = T>
__global__ void reshape_and_cache_kernel(
    const T* __restrict__ key,     // [T, kv_heads, D] (row stride key_stride)
    const T* __restrict__ value,
    TC* __restrict__ k_cache,      // [blocks, kv_heads, bs, D]
    TC* __restrict__ v_cache,
    const long* __restrict__ slots,  // [T] global slot id
    int kv_heads, int head_dim, int block_size,
    long key_stride, long val_stride) {
  constexpr int VE = Vec8<T>::kElems;
  const int token = blockIdx.x;
  const long slot = slots[token];
  if (slot < 0) return;  // padding
  const long block = slot / block_size;
  const int off = (int)(slot % block_size);
  const int chunks = (kv_heads * head_dim) / VE;
  for (int i = threadIdx.x; i < chunks; i += blockDim.x) {
    const int h = (i * VE) / head_dim;
    const int d = (i * VE) % head_dim;
    const long dst =
        ((block * kv_heads + h) * (long)block_size + off) * head_dim + d;
    Vec8<T> kv = load16(key + (long)token * key_stride + (long)h * head_dim + d);
    Vec8<T> vv = load16(value + (long)token * val_stride + (long)h * head_dim + d);
    if constexpr (std::is_same_v<T, TC>) {
      store16(k_cache + dst, kv);
      store16(v_cache + dst, vv);
    } else {  // quantizing cache write (e.g. bf16 → fp8)
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        k_cache[dst + j] = from_f32<TC>(to_f32(kv.data[j]));
        v_cache[dst + j] = from_f32<TC>(to_f32(vv.data[j]));
      }
    }
  }
}

// Fused RoPE + cache write: rotates q and k in place AND scatters the
// rotated k plus v into the paged cache in one launch (the decode step is
// launch-bound on these per-layer elementwise kernels at M=256).
// Grid: one workgroup per token.
template <typename T, typename TC = T>
__global__ void rope_and_cache_kernel(
    T* __restrict__ q,             // [T, Hq, D] (row stride q_stride)
    T* __restrict__ k,             // [T, Hk, D]
    const T* __restrict__ value,   // [T, Hk, D]
    TC* __restrict__ k_cache,      // [blocks, Hk, bs, D]
    TC* __restrict__ v_cache,
    const long* __restrict__ positions,
    const float* __restrict__ cos_sin,  // [max_pos, D] f32
    const long* __restrict__ slots,
    int num_q_heads, int num_k_heads, int head_dim, int block_size,
    long q_stride, long k_stride, long v_stride) {
  const int token = blockIdx.x;
  const long pos = positions[token];
  const float* cs = cos_sin + pos * head_dim;
  const int half = head_dim / 2;
  const long slot = slots[token];
  const long block = slot / block_size;
  const int off = (int)(slot % block_size);

  // rotate q heads; rotate k heads and write both halves to the cache
  const int total = (num_q_heads + num_k_heads) * half;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int h = i / half;
    const int d = i % half;
    const float c = cs[d];
    const float s = cs[half + d];
    if (h < num_q_heads) {
      T* base = q + (long)token * q_stride + (long)h * head_dim;
      const float x1 = to_f32(base[d]);
      const float x2 = to_f32(base[half + d]);
      base[d] = from_f32<T>(x1 * c - x2 * s);
      base[half + d] = from_f32<T>(x2 * c + x1 * s);
    } else {
      const int kh = h - num_q_heads;
      T* base = k + (long)token * k_stride + (long)kh * head_dim;
      const float x1 = to_f32(base[d]);
      const float x2 = to_f32(base[half + d]);
      const T r1 = from_f32<T>(x1 * c - x2 * s);
      const T r2 = from_f32<T>(x2 * c + x1 * s);
      base[d] = r1;
      base[half + d] = r2;
      if (slot >= 0) {
        TC* kdst = k_cache +
            ((block * num_k_heads + kh) * (long)block_size + off) * head_dim;
        if constexpr (std::is_same_v<T, TC>) {
          kdst[d] = r1;
          kdst[half + d] = r2;
        } else {
          kdst[d] = from_f32<TC>(to_f32(r1));
          kdst[half + d] = from_f32<TC>(to_f32(r2));
        }
      }
    }
  }
  if (slot < 0) return;
  // copy v (vectorized; untouched by rope)
  constexpr int VE = Vec8<T>::kElems;
  const int vchunks = (num_k_heads * head_dim) / VE;
  for (int i = threadIdx.x; i < vchunks; i += blockDim.x) {
    const int h = (i * VE) / head_dim;
    const int d = (i * VE) % head_dim;
    Vec8<T> vv = load16(value + (long)token * v_stride + (long)h * head_dim + d);
    TC* vdst = v_cache +
        ((block * num_k_heads + h) * (long)block_size + off) * head_dim + d;
    if constexpr (std::is_same_v<T, TC>) {
      store16(vdst, vv);
    } else {
#pragma unroll
      for (int j = 0; j < VE; ++j) vdst[j] = from_f32<TC>(to_f32(vv.data[j]));
    }
  }
}

// ---- fused QK-norm + RoPE + cache write (Qwen3) ----------------------------
// Qwen3 applies a per-head RMSNorm over head_dim to q and k between the QKV
// projection and RoPE. This kernel does that norm where rope_and_cache_kernel
// already touches every q/k element, so the layer keeps ONE launch here
// instead of rmsnorm(q) + rmsnorm(k) + rope_and_cache and a second pass over
// q and k.
//
// Mapping: a 16-lane group owns one head (a wave covers 4 heads, the 256-
// thread block 16 heads per pass). Lane l of the group holds E = D/32
// contiguous elements of the low half at [l*E, l*E+E) and the matching E
// elements of the high half at D/2 + [l*E, l*E+E), so a rotate-half partner
// pair (d, d + D/2) is lane-local and the only cross-lane traffic is the
// sum of squares: four __shfl_xor steps that never leave the group. No LDS,
// no __syncthreads. Groups of one wave may run different trip counts of the
// head loop; a group is wholly active or wholly inactive, and xor offsets
// below 16 stay inside it, so an active lane never reads an inactive one.
//
// Each half is moved in pieces of min(16, E*sizeof(T)) bytes: 4/8/16 bytes
// for 2-byte T at D = 64/128/256 and 8/16/2x16 bytes for fp32.
//
// Rounding: the normed value stays fp32 into the rotation; the only rounding
// to T is at the store. An fp8 cache gets the quantization of that T-rounded
// k, exactly as rope_and_cache_kernel writes it.
//
// NORM == false drops the norm (no weight loads, no sum of squares, no
// shuffle reduction, no `inv`; q_weight/k_weight/eps/offset are unused and
// the weights may be null): the same mapping then does rope_and_cache_kernel's
// job with 16-byte accesses and no per-element divide. The rotation is
// written with that kernel's compiled fma order, so all four outputs are
// bit-identical to it (tests/test_rope_cache_vec.py).

template <int BYTES> struct RawBytes;
template <> struct RawBytes<2> { using type = unsigned short; };
template <> struct RawBytes<4> { using type = unsigned int; };
template <> struct RawBytes<8> { using type = uint2; };
template <> struct RawBytes<16> { using type = uint4; };

// N elements of T in registers, loaded/stored in pieces of at most 16 bytes.
// The address must be aligned to kPiece.
template <typename T, int N>
struct Frag {
  static constexpr int kBytes = N * (int)sizeof(T);
  static constexpr int kPiece = kBytes < 16 ? kBytes : 16;
  static constexpr int kPieces = kBytes / kPiece;
  using Raw = typename RawBytes<kPiece>::type;
  alignas(kPiece) T data[N];

  DEVINL void load(const T* p) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i)
      reinterpret_cast<Raw*>(data)[i] = reinterpret_cast<const Raw*>(p)[i];
  }
  DEVINL void store(T* p) const {
#pragma unroll
    for (int i = 0; i < kPieces; ++i)
      reinterpret_cast<Raw*>(p)[i] = reinterpret_cast<const Raw*>(data)[i];
  }
};

template <typename T, typename TC, int D, bool NORM = true>
__global__ __launch_bounds__(256) void qknorm_rope_and_cache_kernel(
    T* __restrict__ q,             // [T, Hq, D] (row stride q_stride)
    T* __restrict__ k,             // [T, Hk, D]
    const T* __restrict__ value,   // [T, Hk, D]
    TC* __restrict__ k_cache,      // [blocks, Hk, bs, D]
    TC* __restrict__ v_cache,
    const T* __restrict__ q_weight,  // [D]
    const T* __restrict__ k_weight,  // [D]
    float eps, float offset,
    const long* __restrict__ positions,
    const float* __restrict__ cos_sin,  // [max_pos, D] f32
    const long* __restrict__ slots,
    int num_q_heads, int num_k_heads, int block_size,
    long q_stride, long k_stride, long v_stride) {
  constexpr int GROUP = 16;        // lanes per head
  constexpr int HALF = D / 2;
  constexpr int E = D / 32;        // elements per lane per half
  const int token = blockIdx.x;
  const long pos = positions[token];
  const long slot = slots[token];
  const long block = slot / block_size;
  const int off = (int)(slot % block_size);
  const int gl = threadIdx.x % GROUP;   // lane within the head's group
  const int groups = blockDim.x / GROUP;
  const int d0 = gl * E;                // this lane's offset in each half

  Frag<float, E> c, s;
  c.load(cos_sin + pos * D + d0);
  s.load(cos_sin + pos * D + HALF + d0);

  const int heads = num_q_heads + num_k_heads;
  for (int h = threadIdx.x / GROUP; h < heads; h += groups) {
    const bool is_q = h < num_q_heads;
    const int kh = h - num_q_heads;
    T* base = is_q ? q + (long)token * q_stride + (long)h * D
                   : k + (long)token * k_stride + (long)kh * D;
    Frag<T, E> lo, hi;
    lo.load(base + d0);
    hi.load(base + HALF + d0);
    if constexpr (NORM) {
      const T* w = is_q ? q_weight : k_weight;
      Frag<T, E> wlo, whi;
      wlo.load(w + d0);
      whi.load(w + HALF + d0);

      float x1[E], x2[E];
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        x1[j] = to_f32(lo.data[j]);
        x2[j] = to_f32(hi.data[j]);
        ss += x1[j] * x1[j] + x2[j] * x2[j];
      }
      ss = group_reduce_sum<GROUP>(ss);
      const float inv = rsqrtf(ss / D + eps);
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const float y1 = x1[j] * inv * (to_f32(wlo.data[j]) + offset);
        const float y2 = x2[j] * inv * (to_f32(whi.data[j]) + offset);
        lo.data[j] = from_f32<T>(y1 * c.data[j] - y2 * s.data[j]);
        hi.data[j] = from_f32<T>(y2 * c.data[j] + y1 * s.data[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const float x1 = to_f32(lo.data[j]);
        const float x2 = to_f32(hi.data[j]);
        // rope_and_cache_kernel's `x1 * c - x2 * s` and `x2 * c + x1 * s`
        // compile to one rounded product and one fma each: x2*s and x2*c are
        // the rounded products (its ISA; confirmed on the GPU, where the
        // other choice for the high half differs in about 1 element in
        // 10^5). Spelled out, because left to contraction this body rounds
        // x1*s instead.
        lo.data[j] = from_f32<T>(fmaf(x1, c.data[j], -(x2 * s.data[j])));
        hi.data[j] = from_f32<T>(fmaf(x1, s.data[j], x2 * c.data[j]));
      }
    }
    lo.store(base + d0);
    hi.store(base + HALF + d0);
    if (!is_q && slot >= 0) {
      TC* kdst = k_cache +
          ((block * num_k_heads + kh) * (long)block_size + off) * D;
      if constexpr (std::is_same_v<T, TC>) {
        lo.store(kdst + d0);
        hi.store(kdst + HALF + d0);
      } else {  // quantize the T-rounded rotated k
        Frag<TC, E> clo, chi;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          clo.data[j] = from_f32<TC>(to_f32(lo.data[j]));
          chi.data[j] = from_f32<TC>(to_f32(hi.data[j]));
        }
        clo.store(kdst + d0);
        chi.store(kdst + HALF + d0);
      }
    }
  }
  if (slot < 0) return;
  // copy v (vectorized; untouched by norm and rope)
  constexpr int VE = Vec8<T>::kElems;
  const int vchunks = (num_k_heads * D) / VE;
  for (int i = threadIdx.x; i < vchunks; i += blockDim.x) {
    const int h = (i * VE) / D;
    const int d = (i * VE) % D;
    Vec8<T> vv = load16(value + (long)token * v_stride + (long)h * D + d);
    TC* vdst = v_cache +
        ((block * num_k_heads + h) * (long)block_size + off) * D + d;
    if constexpr (std::is_same_v<T, TC>) {
      store16(vdst, vv);
    } else {
#pragma unroll
      for (int j = 0; j < VE; ++j) vdst[j] = from_f32<TC>(to_f32(vv.data[j]));
    }
  }
}

// ---- paged K/V gather (chunked prefill, prefix-cache hits) -----------------
// Assembles the packed attention context of a prefill segment: for sequence b
// with Lq fresh rows and Lk context rows (P = Lk - Lq rows already in the
// paged cache), context row r comes from cache block block_tables[b, r / bs],
// row r % bs when r < P, and from fresh row cu_q[b] + r - P otherwise; it
// lands in packed row cu_k[b] + r of k_out / v_out ([total_k, KVH, D]).
//
// A memory-bound copy: no LDS, every global access is 16 bytes. Grid
// (ceil(max Lk / GATHER_ROWS), B); a workgroup owns GATHER_ROWS consecutive
// context rows and splits them at P into a past range and a fresh range with
// workgroup-uniform bounds, so no lane ever chooses between the two sources.
// Past range: in the cache the rows of one head inside a block are
// contiguous, so the item index runs head-major with (row, 16-byte piece)
// fastest; a wave's loads walk one head's run of rows. Fresh range: a row's
// KVH*D elements are contiguous on both sides, so (row, piece) order.
//
// An fp8 cache is widened to T (bf16): a lane loads 16 fp8 bytes and stores
// two 16-byte vectors. e4m3 -> f32 -> bf16 is exact (3 mantissa bits).
// All cache offsets are 64-bit: a pool can exceed 2^31 elements.

constexpr int GATHER_ROWS = 16;
constexpr int GATHER_THREADS = 256;

typedef float gather_f32x2 __attribute__((ext_vector_type(2)));

// 16 bytes of cache at src -> kItem elements of T at dst.
template <typename T, typename TC>
DEVINL void gather_copy16(T* __restrict__ dst, const TC* __restrict__ src) {
  if constexpr (std::is_same_v<T, TC>) {
    store16(dst, load16(src));
  } else {  // fp8 cache, bf16 output
    const int4 raw = *reinterpret_cast<const int4*>(src);
    const int words[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      Vec8<T> out;
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const int word = words[half * 2 + w];
        const gather_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(word, false);
        const gather_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(word, true);
        out.data[w * 4 + 0] = from_f32<T>(lo[0]);
        out.data[w * 4 + 1] = from_f32<T>(lo[1]);
        out.data[w * 4 + 2] = from_f32<T>(hi[0]);
        out.data[w * 4 + 3] = from_f32<T>(hi[1]);
      }
      store16(dst + half * 8, out);
    }
  }
}

template <typename T, typename TC = T>
__global__ __launch_bounds__(GATHER_THREADS) void gather_paged_kv_kernel(
    T* __restrict__ k_out,           // [total_k, kv_heads, D] (row stride out_stride)
    T* __restrict__ v_out,
    const TC* __restrict__ k_cache,  // [blocks, kv_heads, bs, D]
    const TC* __restrict__ v_cache,
    const T* __restrict__ k_fresh,   // [Tq, kv_heads, D] (row stride kf_stride)
    const T* __restrict__ v_fresh,
    const int* __restrict__ block_tables,  // [B, bt_stride]
    const int* __restrict__ cu_q,          // [B+1]
    const int* __restrict__ cu_k,          // [B+1]
    int kv_heads, int head_dim, int block_size, long bt_stride,
    long ko_stride, long vo_stride, long kf_stride, long vf_stride) {
  const int b = blockIdx.y;
  const int q0 = cu_q[b];
  const int k0 = cu_k[b];
  const int Lk = cu_k[b + 1] - k0;
  const int P = Lk - (cu_q[b + 1] - q0);
  const int r0 = blockIdx.x * GATHER_ROWS;
  if (r0 >= Lk) return;
  const int r1 = min(r0 + GATHER_ROWS, Lk);

  // ---- past rows [r0, pe): cache -> out
  const int pe = min(r1, P);
  if (r0 < pe) {
    constexpr int CE = 16 / (int)sizeof(TC);  // cache elements per item
    const int pieces = head_dim / CE;         // items per (row, head)
    const int nrows = pe - r0;
    const int per_head = nrows * pieces;
    const int items = kv_heads * per_head;
    const int* bt = block_tables + (long)b * bt_stride;
    for (int i = threadIdx.x; i < items; i += GATHER_THREADS) {
      const int h = i / per_head;
      const int rem = i - h * per_head;
      const int r = r0 + rem / pieces;
      const int d = (rem % pieces) * CE;
      const long block = bt[r / block_size];
      const long src = ((block * kv_heads + h) * (long)block_size +
                        (r % block_size)) * head_dim + d;
      const long col = (long)h * head_dim + d;
      gather_copy16<T, TC>(k_out + (long)(k0 + r) * ko_stride + col, k_cache + src);
      gather_copy16<T, TC>(v_out + (long)(k0 + r) * vo_stride + col, v_cache + src);
    }
  }

  // ---- fresh rows [fs, r1): this step's k/v -> out
  const int fs = max(r0, P);
  if (fs < r1) {
    constexpr int VE = Vec8<T>::kElems;
    const int pieces = (kv_heads * head_dim) / VE;  // items per row
    const int items = (r1 - fs) * pieces;
    for (int i = threadIdx.x; i < items; i += GATHER_THREADS) {
      const int r = fs + i / pieces;
      const long col = (long)(i % pieces) * VE;
      const long srow = (long)(q0 + r - P);
      store16(k_out + (long)(k0 + r) * ko_stride + col,
              load16(k_fresh + srow * kf_stride + col));
      store16(v_out + (long)(k0 + r) * vo_stride + col,
              load16(v_fresh + srow * vf_stride + col));
    }
  }
}
