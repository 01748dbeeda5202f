// Prefill attention for gfx950.
//
// varlen_prefill_attention_kernel: correctness-first packed varlen causal
// attention on the VALU (one wave per query row, keys across lanes, online
// softmax); serves fp32/fp16. bf16 runs the MFMA flash kernels below:
// flash_prefill_pipe_kernel (default, glds software pipeline) and
// flash_prefill_bf16_kernel (plain staging, LLMQ_PREFILL_PIPE=0), which
// share the pf_* helpers and differ only in how K/V reach LDS and where the
// barriers sit. At the serving shapes prefill attention is a small share of
// prefill FLOPs (see SURVEY §7 risk list).

#include "attention_common.h"

// --------------------------------------------------------------- prefill --
// Packed varlen causal attention. Grid: (seq, head). 4 waves per block;
// each wave owns query rows i = wave_id + 4*n. Keys go across lanes (one
// key per lane per 64-key chunk), V accumulation is lane-dim-parallel via
// shfl broadcast of the probabilities.

template <typename T, int HEAD_DIM>
__global__ __launch_bounds__(256) void varlen_prefill_attention_kernel(
    T* __restrict__ out,            // [Tq, H, D]
    const T* __restrict__ q,        // [Tq, H, D] (row strides below)
    const T* __restrict__ k,        // [Tk, KVH, D]
    const T* __restrict__ v,
    const int* __restrict__ cu_seqlens,    // [B+1] query offsets
    const int* __restrict__ cu_seqlens_k,  // [B+1] key offsets (chunked)
    int num_heads, int num_kv_heads, float scale, float softcap, int window,
    long q_stride, long k_stride, long v_stride, long o_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int VE = Vec8<T>::kElems;
  constexpr int DPT = D / WAVE;  // dims per lane (1/2/4)
  const int seq = blockIdx.x;
  const int h = blockIdx.y;
  const int kvh = h / (num_heads / num_kv_heads);
  const int s0 = cu_seqlens[seq], s1 = cu_seqlens[seq + 1];
  const int L = s1 - s0;
  const int s0k = cu_seqlens_k[seq];
  const int Lk = cu_seqlens_k[seq + 1] - s0k;
  const int off = Lk - L;  // abs position of q row 0
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);

  __shared__ __attribute__((aligned(16))) float q_lds[4][D];

  for (int i = wid; i < L; i += 4) {  // query row
    // stage q row (pre-scaled) into this wave's LDS slot
    for (int d = lane; d < D; d += WAVE)
      q_lds[wid][d] = to_f32(q[(long)(s0 + i) * q_stride + (long)h * D + d]) * scale;
    __builtin_amdgcn_wave_barrier();

    float m_run = -1e30f, l_run = 0.f;
    float acc[DPT];
#pragma unroll
    for (int t = 0; t < DPT; ++t) acc[t] = 0.f;

    const int iabs = off + i;  // absolute position of this query row
    const int kstart = (window > 0 && iabs + 1 > window) ? (iabs + 1 - window) : 0;
    for (int base = (kstart / WAVE) * WAVE; base <= iabs; base += WAVE) {
      const int j = base + lane;  // this lane's key (absolute)
      float score = -1e30f;
      if (j <= iabs && j >= kstart && j < Lk) {
        const T* krow = k + (long)(s0k + j) * k_stride + (long)kvh * D;
        float dot = 0.f;
#pragma unroll 4
        for (int d = 0; d < D; d += VE) {
          Vec8<T> kv = load16(krow + d);
#pragma unroll
          for (int e = 0; e < VE; ++e) dot += q_lds[wid][d + e] * to_f32(kv.data[e]);
        }
        score = (softcap > 0.f) ? tanhf(dot / softcap) * softcap : dot;
      }
      const float m_chunk = wave_reduce_max(score);
      const float m_new = fmaxf(m_run, m_chunk);
      const float alpha = __expf(m_run - m_new);
      const float p = (score > -1e29f) ? __expf(score - m_new) : 0.f;
      const float psum = wave_reduce_sum(p);
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int t = 0; t < DPT; ++t) acc[t] *= alpha;
      const int jn = min(iabs - base + 1, WAVE);
      for (int jj = 0; jj < jn; ++jj) {
        const float pj = __shfl(p, jj, WAVE);
        if (pj != 0.f) {
          const T* vrow = v + (long)(s0k + base + jj) * v_stride + (long)kvh * D;
#pragma unroll
          for (int t = 0; t < DPT; ++t)
            acc[t] += pj * to_f32(vrow[lane * DPT + t]);
        }
      }
    }
    const float inv = (l_run > 0.f) ? 1.0f / l_run : 0.f;
    T* orow = out + (long)(s0 + i) * o_stride + (long)h * D;
#pragma unroll
    for (int t = 0; t < DPT; ++t) orow[lane * DPT + t] = from_f32<T>(acc[t] * inv);
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------ MFMA flash prefill --
// Packed varlen causal GQA attention on matrix cores (bf16).
// Grid: (seq, q_head, q_tile). Workgroup: 4 waves; each wave owns 16 query
// rows of a 64-row Q tile. KV tiles of 64 keys in LDS (shared by the 4
// waves: K rows XOR-swizzled, V as the tr16 subtile image); per KV tile each
// wave computes
//   S[16q,64k]  via mfma_f32_16x16x32_bf16 (Q frags in registers, K^T frags
//               from LDS b128 reads)
//   online softmax in the MFMA C-layout (row r = (lane>>4)*4+reg lives on
//               the 16 col-lanes -> shfl_xor over the low 4 lane bits)
//   OT[D,16q] += mfma(A=V^T, B=P^T)  -- transposed PV so the P fragment is a
//               contiguous b128 read of the per-wave P tile and the softmax
//               rescale factor is lane-uniform (qrow = lane&15).
// Epilogue transposes OT back with scalar stores.
//
// cu_seqlens_k: key-side offsets — equal to cu_seqlens for plain prefill;
// for CHUNKED prefill a sequence's K/V covers its full context so far
// (gathered past + fresh chunk) while Q is only the new chunk, and q row i
// sits at absolute position (Lk - Lq) + i.

#define PF_QT 64   // q rows per workgroup
#define PF_KT 64   // keys per kv tile

// ---- device helpers shared by the two flash kernels, on the conventions of
// the decode family's pd_* helpers: forced inline, registers by reference,
// LDS as pointers into the CALLER's storage, never a __shared__ object of
// their own. Lane coordinates: col = lane & 15 (key for S, q row for OT),
// kgrp = lane >> 4; a wave's softmax rows are r = kgrp*4 + reg, i.e. q rows
// qrow0 + r with qrow0 = q_base + wid*16. Per-wave LDS: a [16][PF_KT] bf16 P
// tile and two 16-float stat rows (alpha, 1/l) indexed by row.

// Q fragments: A-operand row = lane&15 (rows past L repeat row L-1; they are
// masked in S and never stored). FENCE as in pd_load_qfrag.
template <int D, bool FENCE>
DEVINL void pf_load_qfrag(bf16x8_t (&qfrag)[D / 32], const __hip_bfloat16* q,
                          int s0, int L, int h, long q_stride, int qrow,
                          int kgrp) {
  const int r = (qrow < L) ? qrow : (L - 1);
  const __hip_bfloat16* qp = q + (long)(s0 + r) * q_stride + (long)h * D;
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(qp + ks * 32 + kgrp * 8);
    if constexpr (FENCE) reg_fence(qfrag[ks]);  // wait HERE, not in the pipeline
  }
}

// Absolute key range [kv_begin, kv_end) of the workgroup's 64 q rows (causal
// bound above, tile-aligned sliding-window bound below) and the last
// absolute row of this wave: tiles past it are skipped by the wave.
DEVINL void pf_tile_range(int off, int L, int q_base, int wid, int window,
                          int& wave_max_row, int& kv_begin, int& kv_end) {
  wave_max_row = off + min(q_base + wid * 16 + 15, L - 1);
  kv_end = off + min(q_base + PF_QT - 1, L - 1) + 1;
  kv_begin = 0;
  if (window > 0)
    kv_begin = max(0, ((off + q_base + 1 - window) / PF_KT) * PF_KT);
}

// S = Q K^T over the tile's four 16-key slabs, then scale, softcap and the
// causal / window / length mask -> p[reg][slab], and the row max over the
// tile -> mx[reg].
template <int D>
DEVINL void pf_scores(const bf16x8_t (&qfrag)[D / 32], const short* kbuf,
                      int kt, int qrow0, int off, int L, int Lk, float scale,
                      float softcap, int window, int col, int kgrp,
                      float (&p)[4][4], float (&mx)[4]) {
  f32x4_t s[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
    s[ct] = attn_s_slab<D>(qfrag, kbuf, ct * 16 + col, kgrp);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int qrow = qrow0 + kgrp * 4 + reg;
    const int row = off + qrow;  // absolute position
    float m = -1e30f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int key = kt + ct * 16 + col;
      float x = s[ct][reg] * scale;
      if (softcap > 0.f) x = tanhf(x / softcap) * softcap;
      const bool dead = key > row || key >= Lk || qrow >= L ||
                        (window > 0 && key <= row - window);
      x = dead ? -1e30f : x;
      p[reg][ct] = x;
      m = fmaxf(m, x);
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    mx[reg] = m;
  }
}

// Online-softmax update: new running max / sum, p exponentiated in place,
// alpha stored to the wave's alpha row for the OT lanes. Returns whether OT
// must be rescaled by alpha this tile: always, except in the -DLLMQ_DEFER_ON
// build for a kernel that asks for it (DEFER).
// defer-max (guide T13): when no row of this wave grew its max by more than
// THR, keep the old maxes — P is then bounded by e^THR (fp32 accumulators
// tolerate it) and the whole O-rescale pass is skipped. The decision covers
// the ENTIRE tile before any P of it is exponentiated (the T13 ordering
// hazard), and every l-update uses alpha==1 on the defer path. Accuracy cost
// ≈3× max-abs error (bounded-P bf16 quantisation) — inside the test
// tolerances. Measured a loss (see pd_softmax_tile), hence off by default.
template <bool DEFER>
DEVINL bool pf_softmax_update(float (&p)[4][4], const float (&mx)[4],
                              float (&m_run)[4], float (&l_run)[4],
                              float* alpha_s, int col, int kgrp) {
  bool rescale = true;
#ifdef LLMQ_DEFER_ON
  if constexpr (DEFER) {
    bool grow = false;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) grow |= mx[reg] > m_run[reg] + 8.0f;
    rescale = __any(grow);
  }
#endif
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float m_new = rescale ? fmaxf(m_run[reg], mx[reg]) : m_run[reg];
    const float alpha = (rescale && m_new > -1e30f)
                            ? __expf(m_run[reg] - m_new) : 1.f;
    float lsum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float pe = (m_new > -1e30f && p[reg][ct] > -1e29f)
                           ? __expf(p[reg][ct] - m_new) : 0.f;
      p[reg][ct] = pe;
      lsum += pe;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) lsum += __shfl_xor(lsum, o, WAVE);
    l_run[reg] = l_run[reg] * alpha + lsum;
    m_run[reg] = m_new;
    if (rescale && col == 0) alpha_s[kgrp * 4 + reg] = alpha;
  }
  return rescale;
}

// P rows (bf16) -> the wave's [16 q][PF_KT] tile.
DEVINL void pf_write_p(const float (&p)[4][4], short* p_tile, int col, int kgrp) {
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
      p_tile[(kgrp * 4 + reg) * PF_KT + ct * 16 + col] =
          __bfloat16_as_short(__float2bfloat16(p[reg][ct]));
  }
}

// Epilogue, first half: 1/l goes through the wave's inv row (softmax rows ->
// OT lanes, q row = lane&15); returns this lane's 1/l. The row is written
// and read by the SAME wave, so an lgkm drain orders it; the pipe kernel
// (BARRIER) keeps its raw-barrier form of that drain. The second half, the
// normalise + transpose store of OT, stays written out in each kernel: as a
// helper taking `ot` by reference (so that the kernel touches `ot` through
// helpers only) hipcc carries the accumulators through the tile loop twice,
// and the D=256 pipe kernel goes from 232 VGPRs to 256 with 16 spilled.
template <bool BARRIER>
DEVINL float pf_inv_l(const float (&l_run)[4], float* inv_s, int col, int kgrp) {
  if (col == 0) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float l = l_run[reg];
      inv_s[kgrp * 4 + reg] = (l > 0.f) ? 1.0f / l : 0.f;
    }
  }
  if constexpr (BARRIER) pipe_barrier();
  else __builtin_amdgcn_s_waitcnt(0);
  return inv_s[col];
}

// Plain-staged kernel (LLMQ_PREFILL_PIPE=0): K/V tiles go through VGPRs into
// LDS between two __syncthreads(); keys past Lk are zero-filled.
template <int HEAD_DIM>
__global__ __launch_bounds__(256) void flash_prefill_bf16_kernel(
    __hip_bfloat16* __restrict__ out,      // [Tq, H, D]
    const __hip_bfloat16* __restrict__ q,  // [Tq, H, D]
    const __hip_bfloat16* __restrict__ k,  // [Tk, KVH, D]
    const __hip_bfloat16* __restrict__ v,
    const int* __restrict__ cu_seqlens, const int* __restrict__ cu_seqlens_k,
    int num_heads, int num_kv_heads,
    float scale, float softcap, int window, long q_stride, long k_stride,
    long v_stride, long o_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int DT = D / 16;
  const int seq = blockIdx.x;
  const int h = blockIdx.y;
  const int kvh = h / (num_heads / num_kv_heads);
  const int s0 = cu_seqlens[seq];
  const int L = cu_seqlens[seq + 1] - s0;       // query rows
  const int s0k = cu_seqlens_k[seq];
  const int Lk = cu_seqlens_k[seq + 1] - s0k;   // key rows (>= L)
  const int off = Lk - L;                       // abs position of q row 0
  const int q_base = blockIdx.z * PF_QT;
  if (q_base >= L) return;

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;        // MFMA col lane (key for S, qrow for OT)
  const int kgrp = lane >> 4;       // 0..3
  const int qrow0 = q_base + wid * 16;

  // LDS: K tile | V image | per-wave P tiles | per-wave row stats
  __shared__ __attribute__((aligned(16))) short k_lds[PF_KT * D];
  __shared__ __attribute__((aligned(16))) short v_lds[v_img_elems(PF_KT, D)];
  __shared__ __attribute__((aligned(16))) short p_lds[4][16 * PF_KT];
  __shared__ float stat_lds[4][2][16];  // [wave][alpha|inv_l][row]

  bf16x8_t qfrag[D / 32];
  pf_load_qfrag<D, false>(qfrag, q, s0, L, h, q_stride, qrow0 + col, kgrp);

  float m_run[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
  float l_run[4] = {0.f, 0.f, 0.f, 0.f};
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  int wave_max_row, kv_begin, kv_end;
  pf_tile_range(off, L, q_base, wid, window, wave_max_row, kv_begin, kv_end);

  for (int kt = kv_begin; kt < kv_end; kt += PF_KT) {
    // ---- stage K/V tile (zero-fill beyond Lk so garbage never reaches MFMA)
    {
      constexpr int CPK = D / 8;  // 16B chunks per key row
      for (int c = tid; c < PF_KT * CPK; c += 256) {
        const int key = c / CPK;
        const int d8 = (c % CPK) * 8;
        const int dst = key * D + swz(key, d8);
        const int vdst = v_img_index<D>(key, d8);
        const int gkey = kt + key;
        if (gkey < Lk) {
          *reinterpret_cast<bf16x8_t*>(&k_lds[dst]) =
              *reinterpret_cast<const bf16x8_t*>(
                  k + (long)(s0k + gkey) * k_stride + (long)kvh * D + d8);
          *reinterpret_cast<bf16x8_t*>(&v_lds[vdst]) =
              *reinterpret_cast<const bf16x8_t*>(
                  v + (long)(s0k + gkey) * v_stride + (long)kvh * D + d8);
        } else {
          *reinterpret_cast<bf16x8_t*>(&k_lds[dst]) = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
          *reinterpret_cast<bf16x8_t*>(&v_lds[vdst]) = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
    }
    __syncthreads();

    if (kt <= wave_max_row) {  // this wave has rows that see this tile
      float p[4][4], mx[4];
      pf_scores<D>(qfrag, k_lds, kt, qrow0, off, L, Lk, scale, softcap, window,
                   col, kgrp, p, mx);
      pf_softmax_update<false>(p, mx, m_run, l_run, stat_lds[wid][0], col, kgrp);
      pf_write_p(p, p_lds[wid], col, kgrp);
      // ---- OT += V^T P^T (A = V^T frags via tr16 reads, B = P^T b128);
      // alpha and P were written by this wave: no barrier needed
      attn_pv_tile<D, PF_KT, DT>(v_lds, p_lds[wid], stat_lds[wid][0], true, ot,
                                 0, lane);
    }
    __syncthreads();
  }

  const float inv = pf_inv_l<false>(l_run, stat_lds[wid][1], col, kgrp);
  const int orow = qrow0 + col;
  if (orow < L) {
    __hip_bfloat16* op = out + (long)(s0 + orow) * o_stride + (long)h * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        op[dt * 16 + kgrp * 4 + reg] = __float2bfloat16(ot[dt][reg] * inv);
    }
  }
}

// ---------------------------------------------- pipelined MFMA flash prefill --
// flash_prefill_bf16_kernel with the decode kernel's glds software pipeline
// (see paged_decode_pipe_kernel in decode_attention.hip for the full
// rationale): the serial stage→sync→S→softmax→PV structure exposes the K/V
// staging latency every tile (L2-resident for the reuse across
// q-heads/q-tiles, but the VGPR round-trip + barrier drain still serialize).
// Two buffers: V(kt) overwrites K(kt)'s buffer after S, K(kt+1) prefetches
// into the other; raw barriers with counted vmcnt keep the DMA in flight
// through PV. glds cannot zero-fill: keys past Lk (the tile containing Lk)
// clamp their source to row Lk-1, so every tile stays on the pipeline.

template <int HEAD_DIM>
__global__ __launch_bounds__(256, (HEAD_DIM <= 128 ? 4 : 2)) void flash_prefill_pipe_kernel(
    __hip_bfloat16* __restrict__ out,      // [Tq, H, D]
    const __hip_bfloat16* __restrict__ q,  // [Tq, H, D]
    const __hip_bfloat16* __restrict__ k,  // [Tk, KVH, D]
    const __hip_bfloat16* __restrict__ v,
    const int* __restrict__ cu_seqlens, const int* __restrict__ cu_seqlens_k,
    int num_heads, int num_kv_heads,
    float scale, float softcap, int window, long q_stride, long k_stride,
    long v_stride, long o_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int DT = D / 16;
  constexpr int NT = 256;
  constexpr int CPK = D / 8;                        // 16B granules per key row
  constexpr int NI_K = PF_KT * CPK / NT;            // K glds per wave per tile
  constexpr int NI_V = v_img_nsub(PF_KT, D) / 4;    // V glds per wave per tile
  constexpr int KV_ELEMS = kv_tile_elems(PF_KT, D);
  const int seq = blockIdx.x;
  const int h = blockIdx.y;
  const int kvh = h / (num_heads / num_kv_heads);
  const int s0 = cu_seqlens[seq];
  const int L = cu_seqlens[seq + 1] - s0;       // query rows
  const int s0k = cu_seqlens_k[seq];
  const int Lk = cu_seqlens_k[seq + 1] - s0k;   // key rows (>= L)
  const int off = Lk - L;                       // abs position of q row 0
  const int q_base = blockIdx.z * PF_QT;
  if (q_base >= L) return;

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int kgrp = lane >> 4;
  const int qrow0 = q_base + wid * 16;

  // ONE shared array (glds pipeline: hipcc drains vmcnt(0) before ds_reads
  // when a second __shared__ object exists)
  constexpr int P_OFF = 2 * KV_ELEMS;                    // shorts
  // float index of the stat region: 16B-align past P (8 shorts per 16B
  // unit, 4 floats per unit)
  constexpr int STAT_F = (P_OFF + 4 * 16 * PF_KT + 7) / 8 * 4;
  constexpr int TOTAL_BYTES = STAT_F * 4 + 4 * 2 * 16 * 4;
  __shared__ __attribute__((aligned(16))) char smem[TOTAL_BYTES];
  short* const kv0 = reinterpret_cast<short*>(smem);
  short* const kv1 = kv0 + KV_ELEMS;
  short* const p_tile = kv0 + P_OFF + wid * 16 * PF_KT;  // this wave's [16][PF_KT]
  float* const alpha_s =
      reinterpret_cast<float*>(smem) + STAT_F + wid * 2 * 16;  // [alpha|inv_l][16]
  float* const inv_s = alpha_s + 16;

  bf16x8_t qfrag[D / 32];
  pf_load_qfrag<D, true>(qfrag, q, s0, L, h, q_stride, qrow0 + col, kgrp);

  float m_run[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
  float l_run[4] = {0.f, 0.f, 0.f, 0.f};
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  int wave_max_row, kv_begin, kv_end;
  pf_tile_range(off, L, q_base, wid, window, wave_max_row, kv_begin, kv_end);

  // Out-of-range keys clamp to row Lk-1 (real finite data): K garbage is
  // masked in S, dead keys carry P == 0 into PV — every tile stays on the
  // glds pipeline (see the decode kernel's note). The LDS image is
  // lane-linear, so K's swizzle and V's image permutation move to the source.
  auto issue_k = [&](int kt, short* dst) {
#pragma unroll
    for (int j = 0; j < NI_K; ++j) {
      const int g = (wid * NI_K + j) * 64 + lane;  // granule
      const int key = g / CPK;
      const int d = swz(key, (g % CPK) * 8);
      const int gk = min(kt + key, Lk - 1);
      const int o2 = __builtin_amdgcn_readfirstlane((wid * NI_K + j) * 512);
      glds16(k + (long)(s0k + gk) * k_stride + (long)kvh * D + d, dst + o2);
    }
  };
  auto issue_v = [&](int kt, short* dst) {
#pragma unroll
    for (int j = 0; j < NI_V; ++j) {
      const int st = wid * NI_V + j;
      const VImgSrc s = v_img_source<D>(st, lane);
      const int gk = min(kt + s.key, Lk - 1);
      const int o2 = __builtin_amdgcn_readfirstlane(st * V_SUB_STRIDE);
      glds16(v + (long)(s0k + gk) * v_stride + (long)kvh * D + s.dim, dst + o2);
    }
  };
  // ---- prologue
  if (kv_begin < kv_end) issue_k(kv_begin, kv0);
  int cur = 0;
  for (int kt = kv_begin; kt < kv_end; kt += PF_KT, cur ^= 1) {
    short* const X = cur ? kv1 : kv0;
    short* const Y = cur ? kv0 : kv1;
    pipe_barrier_vm<0>();  // K(kt) landed (all waves)

    const bool active = kt <= wave_max_row;  // wave-uniform
    float p[4][4];
    bool rescale = false;
    if (active) {
      float mx[4];
      pf_scores<D>(qfrag, X, kt, qrow0, off, L, Lk, scale, softcap, window, col,
                   kgrp, p, mx);
      rescale = pf_softmax_update<true>(p, mx, m_run, l_run, alpha_s, col, kgrp);
    }
    pipe_barrier();  // S reads of X done; alpha visible

    // ---- issue V(kt)->X, K(kt+PF_KT)->Y under the P build + PV
    const int nxt = kt + PF_KT;
    const bool prefetch = nxt < kv_end;
    issue_v(kt, X);
    if (prefetch) issue_k(nxt, Y);

    if (active) pf_write_p(p, p_tile, col, kgrp);
    if (prefetch) {
      pipe_barrier_vm<NI_K>();  // V landed; K(next) stays in flight
    } else {
      pipe_barrier_vm<0>();
    }

    // ---- OT += V^T P^T (O-rescale skipped entirely on the defer path)
    if (active)
      attn_pv_tile<D, PF_KT, DT>(X, p_tile, alpha_s, rescale, ot, 0, lane);
    // next loop-top barrier protects X (overwritten two iterations out)
  }

  const float inv = pf_inv_l<true>(l_run, inv_s, col, kgrp);
  const int orow = qrow0 + col;
  if (orow < L) {
    __hip_bfloat16* op = out + (long)(s0 + orow) * o_stride + (long)h * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        op[dt * 16 + kgrp * 4 + reg] = __float2bfloat16(ot[dt][reg] * inv);
    }
  }
}

