// Fused token sampling for gfx950.
//
// One pass over the logits [B, V] as the lm_head GEMM stored them (bf16/fp16
// or fp32): each workgroup scans a vocab chunk of one row, widens and
// soft-caps every logit in registers (logit_value) and computes a local
// argmax of
//   temp <= 0:  logit                      (greedy)
//   temp  > 0:  logit / temp + Gumbel(g)   (Gumbel-max == softmax sampling)
// then publishes via one atomicMax on a packed (orderable-f32 | index) key.
// Replaces the torch sampler's 4+ full passes (softmax, multinomial, ...)
// with a single logits read — at B=256, V=256k fp32 that is 262 MB ≈ 35 µs
// at stream rate. Top-k/top-p rows fall back to the torch path (wrapper).
//
// RNG: counter-based (seed, step, element) hash — deterministic per engine
// step, independent of launch geometry, so eager and hipGraph runs sample
// identical tokens.

#include <type_traits>

#include "common.h"

DEVINL unsigned int hash_u32(unsigned int x) {
  // finalizer-strength integer hash (xxhash/murmur-style avalanche)
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

DEVINL float uniform01(unsigned int seed, unsigned int step, unsigned int b,
                       unsigned int v) {
  // Weyl-style multiplicative mixing of the coordinates BEFORE the
  // finalizers: xor-combining (b<<20)^v leaves nearby (b, v) pairs
  // jointly dependent enough to bias argmax sampling by ~3% (verified
  // against the softmax distribution; see TestFusedSampler).
  unsigned int key = b * 0x9E3779B9u ^ v * 0x85EBCA6Bu ^ step * 0xC2B2AE35u ^ seed;
  unsigned int h = hash_u32(hash_u32(key));
  // (0, 1]: avoid 0 so log() is finite
  return (h + 1u) * (1.0f / 4294967296.0f);
}

DEVINL unsigned long long pack_key(float val, int idx) {
  unsigned int u = __float_as_uint(val);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving map
  // index bits inverted so equal values tie-break toward the LOWER index
  // (matches torch argmax) under atomicMax
  return ((unsigned long long)u << 32) | (unsigned int)(~idx);
}

// Stored logit -> the fp32 value the sampler and the bound kernel work on:
// widen, then Gemma-2's final soft-cap cap * tanh(x / cap) when softcap > 0.
// Reproduces the eager tail `torch.tanh(logits.float() / cap) * cap` bit for
// bit: torch divides by a host scalar as a multiply with the fp32
// reciprocal (inv_cap = 1.0f / cap, formed on the host), tanhf is the device
// library's function, and contraction is off so that the multiply feeding
// tanhf is never fused into the function's first add.
template <typename T>
DEVINL float logit_value(T raw, float softcap, float inv_cap) {
#pragma clang fp contract(off)
  float x = to_f32(raw);
  if (softcap > 0.f) {
    x = x * inv_cap;
    x = tanhf(x);
    x = x * softcap;
  }
  return x;
}

// Sampling penalties. A penalised row has a row of the dense count table
// [slots, vpad]: one unsigned 16-bit word per vocab entry, bit 15 = "occurs
// in the prompt", bits 0-14 = occurrences in the output so far (saturating
// at 32767). Applied to the capped fp32 logit in the order of
// torch_ref.apply_penalties, with a true division and contraction off, so
// the result equals the torch expression bit for bit:
//   seen = in_prompt | (c > 0);  l = seen ? (l > 0 ? l / r : l * r) : l
//   l = l - freq * float(c);     l = l - pres * float(c > 0)
struct PenaltyRow {
  const unsigned short* cnt;  // the row's counts, or null: row not penalised
  float r, freq, pres;
};

DEVINL PenaltyRow penalty_row(const unsigned short* table, const int* slots,
                              const float* params, int nslots, long vpad,
                              int b) {
  PenaltyRow p{nullptr, 1.0f, 0.0f, 0.0f};
  if (!table) return p;
  const int slot = slots[b];
  if (slot < 0 || slot >= nslots) return p;
  p.cnt = table + (long)slot * vpad;
  p.r = params[3 * b];
  p.freq = params[3 * b + 1];
  p.pres = params[3 * b + 2];
  return p;
}

DEVINL float penalize(float l, unsigned short word, const PenaltyRow& p) {
#pragma clang fp contract(off)
  const unsigned int c = word & 0x7fffu;
  if (word) l = l > 0.f ? l / p.r : l * p.r;
  l = l - p.freq * (float)c;
  l = l - p.pres * (c ? 1.0f : 0.0f);
  return l;
}

// Per-row RNG keying: rows with a user seed (req_seeds[b] != 0) draw from
// (request_seed, output_position) — REPRODUCIBLE for a given request
// regardless of batch placement or engine step. Unseeded rows draw from
// (engine seed, step, row).
//
// Each workgroup scans [v0, v1) = split blockIdx.y of row b: a scalar head up
// to the first 16-byte-aligned address, 16-byte vectors (8 bf16 / 4 fp32 per
// lane), and a scalar tail. Every logit is loaded once. A thread's indices
// ascend (head < vectors < tail), the RNG is keyed on the element index, and
// ties go to the lower index, so the token does not depend on alignment or
// on the split.
//
// PEN = false is the kernel for a batch without penalties. With PEN = true a
// row whose slot is >= 0 reads its counts alongside the logits, in the same
// head / vector / tail pieces (each count loaded once): 16-byte (8-byte for
// fp32 logits) count loads when the count row is aligned like the logits,
// scalar loads otherwise. A workgroup is one row, so the branch is uniform,
// and a row with slot -1 runs the plain loops with no table traffic.
template <typename T, bool PEN>
__global__ __launch_bounds__(256) void sample_argmax_kernel(
    unsigned long long* __restrict__ out_keys,  // [B], pre-zeroed
    const T* __restrict__ logits,               // [B, V], row stride `stride`
    const float* __restrict__ temps,            // [B]
    const unsigned int* __restrict__ req_seeds, // [B] (0 = unseeded)
    const unsigned int* __restrict__ req_pos,   // [B] output position
    const float* __restrict__ bounds,           // [B] top-k/p keep-bound or null
    int V, long stride, int chunk, float softcap, float inv_cap,
    unsigned int seed, unsigned int step,
    const unsigned short* __restrict__ pen_table,  // [nslots, vpad] or null
    const int* __restrict__ pen_slots,             // [B], -1 = none
    const float* __restrict__ pen_params,          // [B, 3] (r, freq, pres)
    int nslots, long vpad) {
  constexpr int VE = Vec8<T>::kElems;
  const int b = blockIdx.x;
  const int v0 = blockIdx.y * chunk;
  if (v0 >= V) return;
  const int v1 = min(v0 + chunk, V);
  const float temp = temps[b];
  const bool greedy = temp <= 0.f;
  const float inv_t = greedy ? 1.0f : 1.0f / temp;
  const T* row = logits + (long)b * stride;
  const unsigned int rs = req_seeds[b];
  const unsigned int kseed = rs ? rs : seed;
  const unsigned int kstep = rs ? req_pos[b] : step;
  const unsigned int kb = rs ? 0u : (unsigned int)b;
  // top-k/top-p truncation: only logits >= bound are candidates (the
  // bound kernel guarantees the row max passes; greedy rows get -inf)
  const float bound = bounds ? bounds[b] : -3e38f;

  float best = -3e38f;
  int best_i = v0;
  auto consider_l = [&](int v, float l) {
    if (l < bound) return;
    float x = l * inv_t;
    if (!greedy) {
      const float u = uniform01(kseed, kstep, kb, v);
      x += -__logf(-__logf(u));  // Gumbel(0,1)
    }
    if (x > best) { best = x; best_i = v; }
  };
  auto consider = [&](int v, T raw) {
    consider_l(v, logit_value(raw, softcap, inv_cap));
  };
  // elements before the first 16-byte boundary at or after row + v0
  const int mis = (int)(((unsigned long)(row + v0) / sizeof(T)) % VE);
  const int vb = min(v1, v0 + (mis ? VE - mis : 0));
  const int ve = vb + (v1 - vb) / VE * VE;
  PenaltyRow pen{nullptr, 1.0f, 0.0f, 0.0f};
  if constexpr (PEN)
    pen = penalty_row(pen_table, pen_slots, pen_params, nslots, vpad, b);
  if (PEN && pen.cnt) {
    const unsigned short* cnt = pen.cnt;
    auto consider_p = [&](int v, T raw, unsigned short word) {
      consider_l(v, penalize(logit_value(raw, softcap, inv_cap), word, pen));
    };
    if (v0 + (int)threadIdx.x < vb)
      consider_p(v0 + threadIdx.x, row[v0 + threadIdx.x], cnt[v0 + threadIdx.x]);
    if ((unsigned long)(cnt + vb) % (VE * sizeof(unsigned short)) == 0) {
      for (int v = vb + threadIdx.x * VE; v < ve; v += 256 * VE) {
        const Vec8<T> vec = load16(row + v);
        unsigned short words[VE];
        if constexpr (VE == 8)
          *reinterpret_cast<int4*>(words) = *reinterpret_cast<const int4*>(cnt + v);
        else
          *reinterpret_cast<int2*>(words) = *reinterpret_cast<const int2*>(cnt + v);
#pragma unroll
        for (int j = 0; j < VE; ++j) consider_p(v + j, vec.data[j], words[j]);
      }
    } else {
      for (int v = vb + threadIdx.x * VE; v < ve; v += 256 * VE) {
        const Vec8<T> vec = load16(row + v);
        unsigned short words[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) words[j] = cnt[v + j];
#pragma unroll
        for (int j = 0; j < VE; ++j) consider_p(v + j, vec.data[j], words[j]);
      }
    }
    if (ve + (int)threadIdx.x < v1)
      consider_p(ve + threadIdx.x, row[ve + threadIdx.x], cnt[ve + threadIdx.x]);
  } else {
    if (v0 + (int)threadIdx.x < vb) consider(v0 + threadIdx.x, row[v0 + threadIdx.x]);
    for (int v = vb + threadIdx.x * VE; v < ve; v += 256 * VE) {
      const Vec8<T> vec = load16(row + v);
#pragma unroll
      for (int j = 0; j < VE; ++j) consider(v + j, vec.data[j]);
    }
    if (ve + (int)threadIdx.x < v1) consider(ve + threadIdx.x, row[ve + threadIdx.x]);
  }
  // wave reduce (value, index)
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, WAVE);
    const int oi = __shfl_xor(best_i, off, WAVE);
    if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
  }
  __shared__ float vals[4];
  __shared__ int idxs[4];
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { vals[wid] = best; idxs[wid] = best_i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      if (vals[w] > best || (vals[w] == best && idxs[w] < best_i)) {
        best = vals[w]; best_i = idxs[w];
      }
    }
    atomicMax(out_keys + b, pack_key(best, best_i));
  }
}

// ------------------------------------------------- top-k / top-p select --
// Per-row LOGIT-space bound L_min such that keeping {v : logit_v >= L_min}
// realises nucleus (top-p) ∧ top-k truncation, WITHOUT the full-vocab sort
// the torch path needs (at B=256 × V=256k that sort is a multi-ms cliff;
// this is 3 streaming passes ≈ 100 µs). Histogram select: pass 1 = row max;
// pass 2 = 512-bin histogram of x=(l−m)/T over [-32, 0] with exp-mass and
// counts; scan from the top bin until Σp ≥ top_p·Z or count ≥ k; pass 3
// refines 512× within the crossing bin. The crossing sub-bin is kept whole
// (overshoot ≤ its mass ≈ Z·p/512² resolution — statistically invisible;
// the reference's vLLM sorts exactly, our CPU torch_ref too, and the
// distribution tests compare against it with tolerance).
// Sampling from the truncated set then uses the same one-pass gumbel-max
// (argmax over {x: logit ≥ L_min} == renormalised truncated softmax).

#define TH_NBINS 512
#define TH_TPB 256
#define TH_XMIN -32.0f

// EXT = false is the kernel for a batch with neither min_p nor penalties.
// With EXT = true a penalised row (slot >= 0) bounds the penalised logits,
// reading each count next to its logit in every pass, and min_p adds the
// bound m + T * ln(min_p) ("probability >= min_p x the most likely token's"):
// the row keeps the intersection, i.e. the larger bound, and a row with
// min_p alone is done after pass 1, which already has the row max m.
template <typename T, bool EXT>
__global__ __launch_bounds__(TH_TPB) void topk_topp_bound_kernel(
    float* __restrict__ out_bound,     // [B] keep-bound on logit_value()
    const T* __restrict__ logits,      // [B, V] as stored
    const float* __restrict__ temps,   // [B]
    const float* __restrict__ top_ps,  // [B]
    const long* __restrict__ top_ks,   // [B] (0 = off)
    int V, long stride, float softcap, float inv_cap,
    const float* __restrict__ min_ps,              // [B] (0 = off) or null
    const unsigned short* __restrict__ pen_table,  // [nslots, vpad] or null
    const int* __restrict__ pen_slots,             // [B], -1 = none
    const float* __restrict__ pen_params,          // [B, 3] (r, freq, pres)
    int nslots, long vpad) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float T0 = temps[b];
  const float p_lim = top_ps[b];
  const long k_lim = top_ks[b];
  const bool need_p = p_lim < 1.0f;
  const bool need_k = k_lim > 0 && k_lim < V;
  float min_p = 0.f;
  if constexpr (EXT) min_p = min_ps ? min_ps[b] : 0.f;
  const bool need_m = EXT && min_p > 0.f;
  if (T0 <= 0.f || !(need_p || need_k || need_m)) {
    // greedy rows take argmax regardless; unconstrained rows keep all
    if (tid == 0) out_bound[b] = -3e38f;
    return;
  }
  const float inv_t = 1.0f / T0;
  const T* row = logits + (long)b * stride;
  PenaltyRow pen{nullptr, 1.0f, 0.0f, 0.0f};
  if constexpr (EXT)
    pen = penalty_row(pen_table, pen_slots, pen_params, nslots, vpad, b);
  // The streaming loops exist twice, for rows with and without a count row
  // (the choice is uniform per workgroup): the penalised one issues the
  // count load next to the logit load instead of behind a branch that waits
  // for the logit, the plain one is the loop as it was.
  const bool penalised = EXT && pen.cnt;
  auto value = [&](auto with_counts, int v) {
    const T raw = row[v];
    if constexpr (decltype(with_counts)::value) {
      const unsigned short word = pen.cnt[v];
      return penalize(logit_value(raw, softcap, inv_cap), word, pen);
    } else {
      return logit_value(raw, softcap, inv_cap);
    }
  };

  __shared__ float h_sum[TH_NBINS];
  __shared__ int h_cnt[TH_NBINS];
  __shared__ float red[TH_TPB / WAVE];
  __shared__ float sh_state[6];  // new-xlo, flag, new-xhi, Z, keep_above

  // ---- pass 1: row max
  float m = -3e38f;
  auto row_max = [&](auto with_counts) {
    for (int v = tid; v < V; v += TH_TPB)
      m = fmaxf(m, value(with_counts, v));
  };
  if (penalised) row_max(std::true_type{});
  else row_max(std::false_type{});
  for (int off = WAVE / 2; off > 0; off >>= 1)
    m = fmaxf(m, __shfl_xor(m, off, WAVE));
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < TH_TPB / WAVE; ++w) m = fmaxf(m, red[w]);
    red[0] = m;
  }
  __syncthreads();
  m = red[0];

  // min_p bound in logit space; logf (not __logf): the bound is compared
  // with the fp32 torch expression to a few ulp
  float min_p_bound = -3e38f;
  if (need_m) {
#pragma clang fp contract(off)
    const float t_ln = T0 * logf(min_p);
    min_p_bound = m + t_ln;
  }
  if (EXT && !(need_p || need_k)) {
    if (tid == 0) out_bound[b] = min_p_bound;
    return;
  }

  // Histogram window [xlo, xhi) in x-space; elements >= keep_above are
  // already-kept (counted in p_above), elements < xlo already-dropped.
  // Boundary discipline matters: an element EXACTLY at the crossing bin's
  // lower edge belongs to the refinement window (a `<=` exclusion here
  // silently lost it and the refinement found no crossing).
  float xlo = TH_XMIN, xhi = 0.0f;
  float keep_above = 3e38f;
  float p_above = 0.f;
  long n_above = 0;
  float Z = 0.f;         // total exp-mass (fixed after iter 0)
  float bound_x = TH_XMIN;
  bool done = false;

  for (int iter = 0; iter < 2 && !done; ++iter) {
    for (int i = tid; i < TH_NBINS; i += TH_TPB) { h_sum[i] = 0.f; h_cnt[i] = 0; }
    __syncthreads();
    const float w = (xhi - xlo) / TH_NBINS;
    const float inv_w = 1.0f / w;
    float tail = 0.f;  // mass below xlo (iter 0 only; used for Z)
    auto histogram = [&](auto with_counts) {
      for (int v = tid; v < V; v += TH_TPB) {
        const float x = (value(with_counts, v) - m) * inv_t;
        if (x >= keep_above) continue;   // already kept (counted in p_above)
        if (x < xlo) { if (iter == 0) tail += __expf(fmaxf(x, -80.f)); continue; }
        int bin = (int)((x - xlo) * inv_w);
        bin = bin < 0 ? 0 : (bin >= TH_NBINS ? TH_NBINS - 1 : bin);
        atomicAdd(&h_sum[bin], __expf(x));
        atomicAdd(&h_cnt[bin], 1);
      }
    };
    if (penalised) histogram(std::true_type{});
    else histogram(std::false_type{});
    // reduce tail mass (iter 0: completes Z)
    for (int off = WAVE / 2; off > 0; off >>= 1) tail += __shfl_xor(tail, off, WAVE);
    if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = tail;
    __syncthreads();
    if (tid == 0) {
      if (iter == 0) {
        Z = red[0] + red[1] + red[2] + red[3];
        for (int i = 0; i < TH_NBINS; ++i) Z += h_sum[i];
        sh_state[3] = Z;
      } else {
        Z = sh_state[3];
      }
      const float p_target = need_p ? p_lim * Z : 3e38f;
      const long k_target = need_k ? k_lim : 0x7fffffffffffffffL;
      float cum = p_above;
      long cnt = n_above;
      int cross = -1;
      for (int i = TH_NBINS - 1; i >= 0; --i) {
        cum += h_sum[i];
        cnt += h_cnt[i];
        if (cum >= p_target || cnt >= k_target) { cross = i; break; }
      }
      if (cross < 0) {
        // No crossing inside the window. Iter 0: the target needs mass
        // below XMIN too -> keep everything. Refinements: cannot happen
        // with exact arithmetic (iter 0 placed the crossing here); under
        // fp drift keep the WHOLE window (conservative over-keep).
        sh_state[0] = (iter == 0) ? -3e38f : xlo;
        sh_state[1] = 1.0f;  // done marker
      } else {
        float pa = p_above;
        long na = n_above;
        for (int i = TH_NBINS - 1; i > cross; --i) { pa += h_sum[i]; na += h_cnt[i]; }
        sh_state[0] = xlo + cross * w;        // new xlo (crossing bin lo)
        sh_state[1] = 0.0f;                   // continue refining
        sh_state[2] = xlo + (cross + 1) * w;  // new xhi (bin geometry)
        // keep_above: elements EXACTLY at a bin edge were binned below it
        // (clamp puts the window top INSIDE the top bin) — so when the
        // crossing IS the top bin, its upper boundary stays the previous
        // exclusive bound, or the row max itself would be excluded from
        // the refinement and the bound would land a whole bin low.
        sh_state[4] = (cross == TH_NBINS - 1) ? keep_above
                                              : (xlo + (cross + 1) * w);
        red[0] = pa;
        red[1] = (float)na;  // counts <= V = 262k << 2^24: exact in fp32
      }
    }
    __syncthreads();
    if (sh_state[1] != 0.0f) {
      bound_x = sh_state[0];
      done = true;
    } else {
      xlo = sh_state[0];
      xhi = sh_state[2];
      keep_above = sh_state[4];
      p_above = red[0];
      n_above = (long)red[1];
      bound_x = xlo;  // best-so-far: the crossing bin's lower edge
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float kp_bound = (bound_x <= -3e37f) ? -3e38f : (m + bound_x * T0);
    out_bound[b] = EXT ? fmaxf(kp_bound, min_p_bound) : kp_bound;
  }
}

// After a sampling call: one thread per row adds the sampled token to the
// row's count (bits 0-14, saturating; bit 15 kept). Slots are distinct per
// row, so plain loads and stores suffice.
__global__ void penalty_count_tokens_kernel(
    unsigned short* __restrict__ table,  // [nslots, vpad]
    const int* __restrict__ slots,       // [B], -1 = none
    const long* __restrict__ tokens,     // [B]
    int B, int nslots, long vpad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int slot = slots[b];
  const long tok = tokens[b];
  if (slot < 0 || slot >= nslots || tok < 0 || tok >= vpad) return;
  unsigned short* p = table + (long)slot * vpad + tok;
  const unsigned short word = *p;
  if ((word & 0x7fffu) != 0x7fffu) *p = (unsigned short)(word + 1);
}

__global__ void unpack_keys_kernel(long* __restrict__ out,
                                   const unsigned long long* __restrict__ keys,
                                   int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = (long)(unsigned int)(~(keys[b] & 0xffffffffu));
}

// ------------------------------------------------------- token logprobs --
// Log-probability of the sampled token, its rank, and the K most likely
// alternatives, from one more read of a logits row: the specification is
// torch_ref.token_logprobs. One workgroup per requested row; every logit is
// loaded once, walked like the sampler walks it (scalar head to the first
// 16-byte boundary, 16-byte vectors, scalar tail).
//
// The vocabulary order is pack_key's: value descending, ties toward the lower
// index (-0 is folded onto +0 first, as a sort sees them equal). Each thread
// keeps an online (max, sum of exp) pair and counts the keys above the
// token's; the top K live in LDS: an element whose key exceeds the threshold
// `thr` is appended to a candidate buffer, and when the buffer could no
// longer take a whole tile it is compacted to its K largest keys (lp_select),
// with thr = the K-th. thr starts just below the K-th largest of the first
// tile's group maxima (lp_seed_threshold).
// Invariant: at most LP_SLACK candidates before a tile, and a tile appends at
// most TILE, so CAP = LP_SLACK + TILE never overflows. On random rows the
// walk appends ~ K ln(V / K) candidates and only the final compaction runs;
// an ascending row compacts on every tile, slowly but correctly.

#define LP_MAX_K 20
#define LP_SLACK 1024
#define LP_RANK_MAX 1024

DEVINL float unpack_key_value(unsigned long long key) {
  unsigned int u = (unsigned int)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}

DEVINL unsigned long long wave_reduce_max_u64(unsigned long long x) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(x, off, WAVE);
    x = o > x ? o : x;
  }
  return x;
}

// Selects the `rounds` largest of keys[0, n) into win[0, rounds), in
// descending order. Up to LP_RANK_MAX keys by counting: the thread that holds
// a key counts the keys above it, and that count is the key's place (keys
// differ, or are 0 and at the bottom, where equal places hold equal values).
// All lanes read the same address, so the LDS reads are broadcasts, and there
// is one barrier; the work is n^2 compares, ~1 us at the few hundred
// candidates a random row leaves. Beyond that by `rounds` rounds of workgroup
// argmax, each below the previous winner (~1.7 us per round). `win` is all
// zero on entry; n >= rounds >= 1, uniform.
template <int NT>
DEVINL void lp_select(const unsigned long long* keys, unsigned long long* win,
                      int n, int rounds) {
  const int tid = threadIdx.x;
  if (n <= LP_RANK_MAX) {
    for (int i = tid; i < n; i += NT) {
      const unsigned long long k = keys[i];
      int place = 0;
      for (int j = 0; j < n; ++j) place += keys[j] > k ? 1 : 0;
      if (place < rounds) win[place] = k;
    }
    __syncthreads();
    return;
  }
  unsigned long long prev = ~0ull;
  for (int r = 0; r < rounds; ++r) {
    unsigned long long best = 0;
    for (int i = tid; i < n; i += NT) {
      const unsigned long long k = keys[i];
      if (k < prev && k > best) best = k;
    }
    best = wave_reduce_max_u64(best);
    if ((tid & (WAVE - 1)) == 0 && best) atomicMax(&win[r], best);
    __syncthreads();
    prev = win[r];
  }
}

// Keeps the min(K, n) largest of keys[0, n) at the front, in descending
// order, and sets *n_keys to that number. `n` and `K` are uniform, `win` is
// all zero on entry and on return. Returns the new threshold: the K-th
// largest key, or 0 while fewer than K exist.
template <int NT>
DEVINL unsigned long long lp_compact(unsigned long long* keys,
                                     unsigned long long* win, int* n_keys,
                                     int n, int K) {
  const int tid = threadIdx.x;
  const int rounds = min(K, n);
  if (rounds == 0) return 0ull;
  lp_select<NT>(keys, win, n, rounds);
  const unsigned long long mine = tid < rounds ? win[tid] : 0ull;
  const unsigned long long kth = win[rounds - 1];
  __syncthreads();
  if (tid < rounds) { keys[tid] = mine; win[tid] = 0ull; }
  if (tid == 0) *n_keys = rounds;
  __syncthreads();
  return rounds == K ? kth : 0ull;
}

// A first threshold before the walk, while the candidate buffer is empty:
// the maxima of the first tile's groups of four vectors (0 = group without
// one) go through the buffer, and the threshold is their K-th largest, less
// one. At least K keys of the row are above it, so nothing of the row's top
// K is lost, and on a random row the first tile appends a few dozen
// candidates instead of all of its elements. 0 while fewer than K groups
// hold a key. `win` is all zero on entry and on return, *n_keys stays 0.
template <int NT>
DEVINL unsigned long long lp_seed_threshold(unsigned long long mine,
                                            unsigned long long* keys,
                                            unsigned long long* win, int K) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 1; off < 4; off <<= 1) {
    const unsigned long long o = __shfl_xor(mine, off, WAVE);
    mine = o > mine ? o : mine;
  }
  if ((tid & 3) == 0) keys[tid >> 2] = mine;
  __syncthreads();
  lp_select<NT>(keys, win, NT / 4, K);
  const unsigned long long kth = win[K - 1];
  __syncthreads();
  if (tid < LP_MAX_K) win[tid] = 0ull;
  __syncthreads();
  return kth ? kth - 1 : 0ull;
}

template <typename T, int NT, bool TOPK>
__global__ __launch_bounds__(NT) void token_logprobs_kernel(
    float* __restrict__ lp_out,    // [R, 1+K], row stride lp_stride
    int* __restrict__ ids_out,     // [R, 1+K], row stride ids_stride
    int* __restrict__ rank_out,    // [R], stride rank_stride
    const T* __restrict__ logits,  // [B, V], row stride `stride`
    const int* __restrict__ rows,  // [R] batch rows that asked
    const long* __restrict__ tokens,  // [B] sampled tokens
    int B, int V, long stride, int K, long lp_stride, long ids_stride,
    long rank_stride, float softcap, float inv_cap) {
  constexpr int VE = Vec8<T>::kElems;
  constexpr int TILE = NT * VE;
  constexpr int CAP = TOPK ? LP_SLACK + TILE : 1;
  constexpr int NW = NT / WAVE;
  static_assert(NT >= LP_MAX_K && LP_SLACK >= LP_MAX_K + 2 * 8);
  __shared__ unsigned long long keys[CAP];
  __shared__ unsigned long long win[LP_MAX_K];
  __shared__ int n_keys;
  __shared__ float red_m[NW], red_s[NW];
  __shared__ int red_c[NW];
  __shared__ float sh_lse;

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int b = min(max(rows[r], 0), B - 1);
  const T* row = logits + (long)b * stride;
  const int tok = (int)min(max(tokens[b], 0L), (long)V - 1);
  const float c = logit_value(row[tok], softcap, inv_cap) + 0.0f;
  const unsigned long long ckey = pack_key(c, tok);

  if constexpr (TOPK) {
    if (tid < LP_MAX_K) win[tid] = 0ull;
    if (tid == 0) n_keys = 0;
    __syncthreads();
  }
  float m = -3e38f, s = 0.f;
  int above = 0;
  unsigned long long thr = 0ull;  // uniform; below every key

  // l is at most the running max m
  auto visit = [&](int v, float l) {
    s += __expf(l - m);
    const unsigned long long key = pack_key(l, v);
    above += key > ckey ? 1 : 0;
    if constexpr (TOPK) {
      if (key > thr) {
        const int p = atomicAdd(&n_keys, 1);
        if (p < CAP) keys[p] = key;
      }
    }
  };
  auto visit_one = [&](int v, T raw) {
    const float l = logit_value(raw, softcap, inv_cap) + 0.0f;
    if (l > m) { s *= __expf(m - l); m = l; }
    visit(v, l);
  };

  const int mis = (int)(((unsigned long)row / sizeof(T)) % VE);
  const int vb = min(V, mis ? VE - mis : 0);
  const int ve = vb + (V - vb) / VE * VE;
  int v = vb + tid * VE;
  Vec8<T> cur;
  if (v < ve) cur = load16(row + v);
  if constexpr (TOPK) {
    unsigned long long mine = 0ull;
    if (v < ve) {
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const unsigned long long key = pack_key(
            logit_value(cur.data[j], softcap, inv_cap) + 0.0f, v + j);
        mine = key > mine ? key : mine;
      }
    }
    thr = lp_seed_threshold<NT>(mine, keys, win, K);
  }
  if (tid < vb) visit_one(tid, row[tid]);
  // Tiles of NT vectors, the next tile's load issued before this tile's work.
  // The trip count is uniform, so the barriers are legal.
  for (int base = vb; base < ve; base += TILE, v += TILE) {
    Vec8<T> nxt;
    if (v + TILE < ve) nxt = load16(row + v + TILE);
    if (v < ve) {
      float l[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j)
        l[j] = logit_value(cur.data[j], softcap, inv_cap) + 0.0f;
      float vm = l[0];
#pragma unroll
      for (int j = 1; j < VE; ++j) vm = fmaxf(vm, l[j]);
      if (vm > m) { s *= __expf(m - vm); m = vm; }
#pragma unroll
      for (int j = 0; j < VE; ++j) visit(v + j, l[j]);
    }
    if constexpr (TOPK) {
      __syncthreads();
      const int n = min(n_keys, CAP);
      // every thread has read n before the next tile appends
      __syncthreads();
      if (n > LP_SLACK) thr = lp_compact<NT>(keys, win, &n_keys, n, K);
    }
    cur = nxt;
  }
  if (ve + tid < V) visit_one(ve + tid, row[ve + tid]);

  // (m, s) and the count across the workgroup
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off, WAVE);
    const float os = __shfl_xor(s, off, WAVE);
    const float nm = fmaxf(m, om);
    s = s * __expf(m - nm) + os * __expf(om - nm);
    m = nm;
    above += __shfl_xor(above, off, WAVE);
  }
  if ((tid & (WAVE - 1)) == 0) {
    red_m[tid / WAVE] = m;
    red_s[tid / WAVE] = s;
    red_c[tid / WAVE] = above;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NW; ++w) {
      const float nm = fmaxf(m, red_m[w]);
      s = s * __expf(m - nm) + red_s[w] * __expf(red_m[w] - nm);
      m = nm;
      above += red_c[w];
    }
    const float lse = m + logf(s);
    sh_lse = lse;
    lp_out[(long)r * lp_stride] = c - lse;
    ids_out[(long)r * ids_stride] = tok;
    rank_out[(long)r * rank_stride] = above + 1;
  }
  if constexpr (TOPK) {
    const int n = min(n_keys, CAP);  // complete: the barrier above follows every append
    __syncthreads();
    lp_compact<NT>(keys, win, &n_keys, n, K);
    if (tid < min(K, n)) {
      const unsigned long long key = keys[tid];
      lp_out[(long)r * lp_stride + 1 + tid] = unpack_key_value(key) - sh_lse;
      ids_out[(long)r * ids_stride + 1 + tid] =
          (int)(unsigned int)(~(key & 0xffffffffu));
    }
  }
}
