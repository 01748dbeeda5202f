// Shared-prefix (cascade) decode attention for gfx950: the prefix pass and the
// merge of prefix and suffix partials.
//
// A decode batch rendered from one template shares the physical KV blocks of
// its common prefix (prefix caching), but the decode kernels stream the whole
// context once per (sequence, kv head): the prefix K/V crosses the memory
// system B times. Here all B*G query rows of a kv head attend to the shared
// prefix as ONE GEMM-shaped problem:
//
//   grid (ceil(B*G / 128), KVH, NP), 8 waves, each wave owns 16 query rows
//   (tile row r -> sequence r / G, q-head r % G) for the whole key walk,
//   flash-prefill style: row max and row sum never leave the wave.
//   Per 64-key chunk the workgroup stages K (swizzled rows) and V (tr16
//   subtile image) ONCE, with global_load_lds, into two separate buffers:
//
//     top      vmcnt(NI_V) barrier  K(i) landed (V(i) still streaming)
//     S        4 slabs x D/32 MFMA, scale/softcap/mask, online softmax,
//              P -> the wave's own [16][64] LDS tile, alpha -> its 16 floats
//     barrier  K buffer free -> issue K(i+1)
//     vmcnt(NI_K) barrier  V(i) landed (K(i+1) streaming under PV)
//     PV       OT[D, 16q] += V^T P^T, D/16 MFMA tiles x 2 key groups
//     barrier  V buffer free -> issue V(i+1)
//
// so one of the two DMA streams is always in flight under the MFMA work.
// LDS: K 32 KiB + V 33 KiB + P 16 KiB + table 4 KiB at D = 256.
//
// The key range splits over NP z-blocks in whole chunks; the split is a
// function of the shapes only and prefix_len is read from device memory, so a
// captured graph replays while the prefix grows or vanishes. A z-block whose
// slice holds no key returns at once and writes nothing: the merge kernel
// derives the number of live slices from the same arithmetic (sp_split) and
// reads only those, so prefix_len == 0 costs one empty launch.
//
// No causal mask (every prefix key precedes every query). A sliding window is
// a per-row lower bound: the row of sequence b keeps keys
// j >= prefix_len + context_lens[b] - window; a fully masked row stores the
// empty partial (m = -1e30, l = 0, acc = 0).

#include "attention_common.h"

// The kernels of this file are built without packed-fp32 VALU ops
// (v_pk_mul_f32 and kin): a per-function target feature, device pass only.
#if defined(__HIP_DEVICE_COMPILE__)
#define SP_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SP_NO_PK_F32
#endif

constexpr int SP_ROWS = 128;  // query rows per workgroup (8 waves x 16)
constexpr int SP_KT = 64;     // keys per chunk
constexpr int SP_NW = 8;
constexpr int SP_MAX_BT = 1024;  // prefix-table entries staged in LDS

// Clamped prefix length, chunks per z-slice and the number of slices that
// hold at least one key. Shared by the prefix kernel and the merge kernel.
struct SpSplit { int plen, per, live; };
DEVINL SpSplit sp_split(const int* prefix_len, int wp, int block_size, int np) {
  SpSplit s;
  s.plen = min(max(prefix_len[0], 0), wp * block_size);
  const int nchunks = (s.plen + SP_KT - 1) / SP_KT;
  s.per = (nchunks + np - 1) / np;
  s.live = s.per > 0 ? (nchunks + s.per - 1) / s.per : 0;
  return s;
}

template <int HEAD_DIM>
__global__ SP_NO_PK_F32 __launch_bounds__(SP_NW * WAVE) void shared_prefix_attention_kernel(
    float* __restrict__ scratch,              // [B, KVH, NP, G, D+2]
    const __hip_bfloat16* __restrict__ q,     // [B, H, D]
    const __hip_bfloat16* __restrict__ k_cache,  // [nb, KVH, bs, D]
    const __hip_bfloat16* __restrict__ v_cache,
    const int* __restrict__ prefix_table,     // [wp]
    const int* __restrict__ prefix_len,       // [1]
    const int* __restrict__ context_lens,     // [B] suffix tokens
    int B, int num_heads, int num_kv_heads, int block_size, int wp,
    float scale, float softcap, int window, long q_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int KS = D / 32;
  constexpr int KT = SP_KT;
  constexpr int NT = SP_NW * WAVE;
  constexpr int DT = D / 16;            // a wave owns every dim tile of its rows
  constexpr int CPK = D / 8;            // 16B granules per key row
  constexpr int NI_K = KT * CPK / NT;   // K DMAs per wave per chunk
  constexpr int NSUB = v_img_nsub(KT, D);
  constexpr int NI_V = NSUB / SP_NW;    // V DMAs per wave per chunk
  static_assert(KT * CPK % NT == 0 && NSUB % SP_NW == 0 && (D / 16) % NI_V == 0, "");
  static_assert(SP_ROWS == SP_NW * 16, "");

  const int np = gridDim.z;
  const SpSplit sp = sp_split(prefix_len, wp, block_size, np);
  const int range_lo = (int)blockIdx.z * sp.per * KT;
  const int range_hi = min(sp.plen, range_lo + sp.per * KT);
  if (range_lo >= range_hi) return;  // workgroup-uniform, before any barrier

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int kgrp = lane >> 4;
  const int kh = blockIdx.y;
  const int G = num_heads / num_kv_heads;
  const int nrows = B * G;
  const int row0 = blockIdx.x * SP_ROWS + wid * 16;  // this wave's first row

  // ONE shared array (a second __shared__ object makes hipcc drain vmcnt
  // before every ds_read while a DMA is in flight).
  constexpr int K_ELEMS = KT * D;
  constexpr int V_ELEMS = v_img_elems(KT, D);
  constexpr int P_OFF = K_ELEMS + V_ELEMS;             // shorts
  constexpr int F_BASE = (P_OFF + SP_NW * 16 * KT) / 2;  // float index
  constexpr int BT_I = F_BASE + SP_NW * 16;
  static_assert((K_ELEMS * 2) % 16 == 0 && (P_OFF * 2) % 16 == 0, "");
  __shared__ __attribute__((aligned(16))) char smem[(BT_I + SP_MAX_BT) * 4];
  short* const kbuf = reinterpret_cast<short*>(smem);
  short* const vbuf = kbuf + K_ELEMS;
  short* const p_w = kbuf + P_OFF + wid * 16 * KT;     // [16 q][KT] bf16
  float* const alpha_w = reinterpret_cast<float*>(smem) + F_BASE + wid * 16;
  int* const bt_l = reinterpret_cast<int*>(smem) + BT_I;

  // plen <= wp * block_size <= SP_MAX_BT blocks (launcher precondition)
  for (int i = tid; i < (sp.plen + block_size - 1) / block_size; i += NT)
    bt_l[i] = prefix_table[i];

  // ---- Q fragments: A row = lane & 15 -> query row row0 + col
  bf16x8_t qfrag[KS];
  {
    const int r = row0 + col;
    const bool live = r < nrows && context_lens[min(r, nrows - 1) / G] > 0;
    const int b = live ? r / G : 0, g = live ? r % G : 0;
    const __hip_bfloat16* qp = q + (long)b * q_stride + (long)(kh * G + g) * D;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(qp + ks * 32 + kgrp * 8);
      reg_fence(qfrag[ks]);  // wait here, not inside the DMA loop
    }
  }
  // ---- softmax rows of this lane: r = row0 + kgrp*4 + reg. key_lo = first
  // key the row keeps (window), INT_MAX for pad rows (nothing kept).
  int key_lo[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int r = row0 + kgrp * 4 + reg;
    const int ctx = r < nrows ? context_lens[r / G] : 0;
    key_lo[reg] = ctx <= 0 ? 0x7fffffff
                           : (window > 0 ? sp.plen + ctx - window : 0);
    asm volatile("" : "+v"(key_lo[reg]));
  }
  float m_regs[4], l_regs[4];  // l: this lane's share of the row sum
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) { m_regs[reg] = -1e30f; l_regs[reg] = 0.f; }
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  const int bs_shift = 31 - __builtin_clz(block_size);
  const int bs_mask = block_size - 1;
  const long blk_stride = (long)num_kv_heads * block_size * D;
  const long head_off = (long)kh * block_size * D;

  // DMA sources: the LDS image is lane-linear, so K's swizzle and V's image
  // permutation sit on the source address. Keys past the slice end (last
  // chunk only) clamp to key plen-1: finite data, masked in S, P == 0 in PV.
  auto issue_k = [&](int base) {
    const __hip_bfloat16* src[NI_K];
#pragma unroll
    for (int j = 0; j < NI_K; ++j) {
      const int g = (wid * NI_K + j) * 64 + lane;
      const int key = g / CPK;
      const int d = ((g % CPK) * 8) ^ ((key & 7) << 3);
      const int gkey = min(base + key, sp.plen - 1);
      const long blk = bt_l[gkey >> bs_shift];
      src[j] = k_cache + head_off + blk * blk_stride + ((gkey & bs_mask) * D + d);
    }
#pragma unroll
    for (int j = 0; j < NI_K; ++j) {
      const int off = __builtin_amdgcn_readfirstlane((wid * NI_K + j) * 512);
      glds16(src[j], kbuf + off);
    }
  };
  // A wave's NI_V subtiles are consecutive 16-dim tiles of one 32-key group.
  auto issue_v = [&](int base) {
    const VImgSrc s = v_img_source<D>(wid * NI_V, lane);
    const int gkey = min(base + s.key, sp.plen - 1);
    const long blk = bt_l[gkey >> bs_shift];
    const __hip_bfloat16* const row =
        v_cache + head_off + blk * blk_stride + ((gkey & bs_mask) * D + s.dim);
#pragma unroll
    for (int j = 0; j < NI_V; ++j) {
      const int off =
          __builtin_amdgcn_readfirstlane((wid * NI_V + j) * V_SUB_STRIDE);
      glds16(row + j * 16, vbuf + off);
    }
  };

  pipe_barrier_vm<0>();  // table visible
  issue_k(range_lo);
  issue_v(range_lo);

  for (int base = range_lo; base < range_hi; base += KT) {
    pipe_barrier_vm<NI_V>();  // K(base) landed

    // ---- S[16 rows, 64 keys], scale / softcap / mask, row max
    float sv[4][4];  // [slab][reg]
    float m_tile[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
#pragma unroll
    for (int slab = 0; slab < KT / 16; ++slab) {
      const f32x4_t s = attn_s_slab<D>(qfrag, kbuf, slab * 16 + col, kgrp);
      const int key = base + slab * 16 + col;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float x = s[reg] * scale;
        if (softcap > 0.f) x = tanhf(x / softcap) * softcap;
        const bool dead = key >= range_hi || key < key_lo[reg];
        sv[slab][reg] = dead ? -1e30f : x;
        m_tile[reg] = fmaxf(m_tile[reg], sv[slab][reg]);
      }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float m = m_tile[reg];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, WAVE));
      const float m_new = fmaxf(m_regs[reg], m);
      const float alpha = (m_new > -1e30f) ? __expf(m_regs[reg] - m_new) : 1.f;
      float lsum = 0.f;
#pragma unroll
      for (int slab = 0; slab < KT / 16; ++slab) {
        const float pe = (m_new > -1e30f && sv[slab][reg] > -1e29f)
                             ? __expf(sv[slab][reg] - m_new) : 0.f;
        lsum += pe;
        p_w[(kgrp * 4 + reg) * KT + slab * 16 + col] =
            __bfloat16_as_short(__float2bfloat16(pe));
      }
      l_regs[reg] = l_regs[reg] * alpha + lsum;
      m_regs[reg] = m_new;
      if (col == 0) alpha_w[kgrp * 4 + reg] = alpha;
    }
    pipe_barrier();  // every wave is past its K reads; P and alpha visible

    const int next = base + KT;
    const bool more = next < range_hi;
    if (more) {
      issue_k(next);
      pipe_barrier_vm<NI_K>();  // V(base) landed; K(next) stays in flight
    } else {
      pipe_barrier_vm<0>();
    }

    // ---- OT[dims, 16 q] = alpha * OT + V^T P^T, all D dims of this wave's rows
    attn_pv_tile<D, KT, DT>(vbuf, p_w, alpha_w, true, ot, 0, lane);
    pipe_barrier();  // V consumed everywhere
    if (more) issue_v(next);
  }

  // ---- store the unnormalised partial: OT column col is query row row0 + col
  const long slot0 = ((long)kh * np + blockIdx.z) * G;
  const long bstride = (long)num_kv_heads * np * G;
  {
    const int r = row0 + col;
    if (r < nrows && context_lens[r / G] > 0) {
      float* rowp = scratch + ((r / G) * bstride + slot0 + r % G) * (D + 2);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          rowp[dt * 16 + kgrp * 4 + reg] = ot[dt][reg];
    }
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    float l = l_regs[reg];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) l += __shfl_xor(l, off, WAVE);
    const int r = row0 + kgrp * 4 + reg;
    if (col == 0 && key_lo[reg] != 0x7fffffff) {
      float* rowp = scratch + ((r / G) * bstride + slot0 + r % G) * (D + 2);
      rowp[D] = m_regs[reg];
      rowp[D + 1] = l;
    }
  }
}

// out[b, kh*G+g] = sum_s w_s acc_s / sum_s w_s l_s over the NS suffix slices
// (written by the decode family with gridDim.z = NS) and the live prefix
// slices, w_s = exp(m_s - max m). One wave per (b, kh, g); rows of sequences
// with context_lens[b] <= 0 are not written.
template <int HEAD_DIM>
__global__ SP_NO_PK_F32 __launch_bounds__(64) void shared_prefix_merge_kernel(
    __hip_bfloat16* __restrict__ out,
    const float* __restrict__ suffix_part,  // [B, KVH, NS, G, D+2]
    const float* __restrict__ prefix_part,  // [B, KVH, NP, G, D+2]
    const int* __restrict__ prefix_len, const int* __restrict__ context_lens,
    int num_kv_heads, int G, int ns, int np, int wp, int block_size,
    long out_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int DPL = D / WAVE;
  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int g = blockIdx.z;
  const int lane = threadIdx.x;
  if (context_lens[b] <= 0) return;
  const int live = sp_split(prefix_len, wp, block_size, np).live;
  const long sstride = (long)G * (D + 2);
  const float* sbase = suffix_part +
      ((((long)b * num_kv_heads + kh) * ns) * G + g) * (D + 2);
  const float* pbase = prefix_part +
      ((((long)b * num_kv_heads + kh) * np) * G + g) * (D + 2);
  float m_max = -1e30f;
  for (int s = 0; s < ns; ++s) m_max = fmaxf(m_max, sbase[s * sstride + D]);
  for (int s = 0; s < live; ++s) m_max = fmaxf(m_max, pbase[s * sstride + D]);
  float acc[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
  float l = 0.f;
  for (int s = 0; s < ns + live; ++s) {
    const float* row = s < ns ? sbase + s * sstride : pbase + (s - ns) * sstride;
    const float w = __expf(row[D] - m_max);
    const float lw = row[D + 1];
    if (w > 0.f && lw > 0.f) {
      l += w * lw;
#pragma unroll
      for (int i = 0; i < DPL; ++i) acc[i] += w * row[lane * DPL + i];
    }
  }
  const float inv = (l > 0.f) ? 1.0f / l : 0.f;
  __hip_bfloat16* op =
      out + (long)b * out_stride + (long)(kh * G + g) * D + lane * DPL;
#pragma unroll
  for (int i = 0; i < DPL; ++i) op[i] = __float2bfloat16(acc[i] * inv);
}
