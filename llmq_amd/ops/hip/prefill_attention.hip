// Prefill attention for gfx950.
//
// PREFILL (varlen_prefill_attention_kernel): correctness-first packed
// varlen causal attention (one wave per query row, keys across lanes,
// online softmax). GEMM-shaped MFMA flash prefill is the planned
// replacement; at the serving shapes prefill attention is a small share of
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
// rows of a 64-row Q tile. KV tiles of 64 keys staged in XOR-swizzled LDS
// (shared by the 4 waves); per KV tile each wave computes
//   S[16q,64k]  via mfma_f32_16x16x32_bf16 (Q frags in registers, K^T frags
//               from LDS b128 reads)
//   online softmax in the MFMA C-layout (row r = (lane>>4)*4+reg lives on
//               the 16 col-lanes -> shfl_xor over the low 4 lane bits)
//   OT[D,16q] += mfma(A=V^T, B=P^T)  -- transposed PV so the P fragment is a
//               contiguous b128 read of the per-wave P_lds tile and the
//               softmax rescale factor is lane-uniform (qrow = lane&15).
// Epilogue transposes OT back with scalar stores.

#define PF_QT 64   // q rows per workgroup
#define PF_KT 64   // keys per kv tile

// cu_seqlens_k: key-side offsets — equal to cu_seqlens for plain prefill;
// for CHUNKED prefill a sequence's K/V covers its full context so far
// (gathered past + fresh chunk) while Q is only the new chunk, and q row i
// sits at absolute position (Lk - Lq) + i.
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

  // LDS: K tile | V tile | per-wave P tiles | per-wave row stats
  __shared__ __attribute__((aligned(16))) short k_lds[PF_KT * D];
  // V: tr-subtile image, 528-elem stride per subtile (bank rotation)
  __shared__ __attribute__((aligned(16))) short v_lds[(PF_KT / 32) * (D / 16) * 528];
  __shared__ __attribute__((aligned(16))) short p_lds[4][16 * PF_KT];
  __shared__ float stat_lds[4][2][16];  // [wave][alpha|inv_l][row]

  // ---- load Q fragments (registers): frag[ks] covers dims ks*32+(kgrp*8..+7)
  constexpr int KS = D / 32;
  bf16x8_t qfrag[KS];
  const int my_qrow = q_base + wid * 16 + col;  // A-frag row = lane&15
  {
    const int r = (my_qrow < L) ? my_qrow : (L - 1);
    const __hip_bfloat16* qrow_p = q + (long)(s0 + r) * q_stride + (long)h * D;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(qrow_p + ks * 32 + kgrp * 8);
  }

  // per-lane softmax state for rows rr = wid*16 + kgrp*4 + reg
  float m_run[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
  float l_run[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int DT = D / 16;
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  const int wave_max_row = off + min(q_base + wid * 16 + 15, L - 1);
  const int block_max_row = off + min(q_base + PF_QT - 1, L - 1);
  const int kv_end = block_max_row + 1;  // causal bound (absolute keys)
  int kv_begin = 0;
  if (window > 0) {
    const int wave_min_needed = off + q_base + 1 - window;
    kv_begin = max(0, (wave_min_needed / PF_KT) * PF_KT);
  }

  for (int kt = kv_begin; kt < kv_end; kt += PF_KT) {
    // ---- stage K/V tile (zero-fill beyond L so garbage never reaches MFMA)
    {
      constexpr int CHW = 8;  // elems per 16B chunk
      const int chunks = PF_KT * D / CHW;
      for (int c = tid; c < chunks; c += 256) {
        const int key = c / (D / CHW);
        const int d8 = (c % (D / CHW)) * CHW;
        const int dst = key * D + swz(key, d8);
        // V uses the tr-read subtile image (quad-permuted 32-key × 16-dim
        // blocks) so PV A-fragments load via ds_read_b64_tr_b16
        const int dtile = d8 / 16, col0 = d8 & 15;
        const int qq = (key & 31) >> 2;
        const int bpos = ((qq & 1) << 2) + (qq >> 1);
        const int vdst = ((key >> 5) * (D / 16) + dtile) * 528 + bpos * 64 +
                         (key & 3) * 16 + col0;
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
      // ---- S = Q K^T for 4 column tiles of 16 keys
      f32x4_t s[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        s[ct] = {0.f, 0.f, 0.f, 0.f};
        const int key = ct * 16 + col;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int d8 = ks * 32 + kgrp * 8;
          bf16x8_t bfrag = *reinterpret_cast<const bf16x8_t*>(
              &k_lds[key * D + swz(key, d8)]);
          s[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[ks], bfrag, s[ct], 0, 0, 0);
        }
      }
      // ---- scale, softcap, mask; rows rr = wid*16+kgrp*4+reg
      float m_tile[4], l_tile[4], p[4][4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int qrow = q_base + wid * 16 + kgrp * 4 + reg;
        const int row = off + qrow;  // absolute position
        float mx = -1e30f;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int key = kt + ct * 16 + col;
          float x = s[ct][reg] * scale;
          if (softcap > 0.f) x = tanhf(x / softcap) * softcap;
          const bool dead = key > row || key >= Lk || qrow >= L ||
                            (window > 0 && key <= row - window);
          x = dead ? -1e30f : x;
          p[reg][ct] = x;
          mx = fmaxf(mx, x);
        }
        // reduce max over the 16 col lanes
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
        m_tile[reg] = mx;
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float m_new = fmaxf(m_run[reg], m_tile[reg]);
        const float alpha = (m_new > -1e30f) ? __expf(m_run[reg] - m_new) : 1.f;
        float lsum = 0.f;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float pe = (m_new > -1e30f && p[reg][ct] > -1e29f)
                               ? __expf(p[reg][ct] - m_new) : 0.f;
          p[reg][ct] = pe;
          lsum += pe;
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) lsum += __shfl_xor(lsum, off, WAVE);
        l_run[reg] = l_run[reg] * alpha + lsum;
        m_run[reg] = m_new;
        // stash alpha for the OT lanes (indexed by qrow = lane&15)
        if (col == 0) stat_lds[wid][0][kgrp * 4 + reg] = alpha;
        // write P row to the wave's P tile (bf16)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          p_lds[wid][(kgrp * 4 + reg) * PF_KT + ct * 16 + col] =
              __bfloat16_as_short(__float2bfloat16(p[reg][ct]));
        }
      }
      // ---- OT += V^T P^T  (A = V^T frags via scalar LDS reads, B = P^T b128)
      const float alpha_q = stat_lds[wid][0][col];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        ot[dt][0] *= alpha_q; ot[dt][1] *= alpha_q;
        ot[dt][2] *= alpha_q; ot[dt][3] *= alpha_q;
#pragma unroll
        for (int ks = 0; ks < PF_KT / 32; ++ks) {
          const int sub = (ks * (D / 16) + dt) * 528 + lane * 4;
          bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)&v_lds[sub]);
          bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)&v_lds[sub + 4 * 64]);
          bf16x8_t a;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            a[j] = __bfloat16_as_short((__hip_bfloat16)lo[j]);
            a[4 + j] = __bfloat16_as_short((__hip_bfloat16)hi[j]);
          }
          bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(
              &p_lds[wid][col * PF_KT + ks * 32 + kgrp * 8]);
          ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, ot[dt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: normalise and store (transpose OT back per lane)
  if (col == 0) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float l = l_run[reg];
      stat_lds[wid][1][kgrp * 4 + reg] = (l > 0.f) ? 1.0f / l : 0.f;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);  // lgkm drain before same-wave read
  const float inv = stat_lds[wid][1][col];
  const int orow = q_base + wid * 16 + col;
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
// (see paged_decode_pipe_kernel below for the full rationale): the serial
// stage→sync→S→softmax→PV structure exposes the K/V staging latency every
// tile (L2-resident for the reuse across q-heads/q-tiles, but the VGPR
// round-trip + barrier drain still serialize). Two buffers: V(kt)
// overwrites K(kt)'s buffer after S, K(kt+1) prefetches into the other;
// raw barriers with counted vmcnt keep the DMA in flight through PV.
// The tile containing Lk falls back to plain zero-filled staging.

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
  constexpr int NT = 256;
  constexpr int CPK = D / 8;                        // 16B granules per key row
  constexpr int NI_K = PF_KT * CPK / NT;            // K glds per wave per tile
  constexpr int NSUB = (PF_KT / 32) * (D / 16);     // V tr-subtiles per tile
  constexpr int NI_V = NSUB / 4;                    // V glds per wave per tile
  constexpr int KV_ELEMS = (PF_KT * D > NSUB * 528) ? PF_KT * D : NSUB * 528;
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
  short* const p_base = kv0 + P_OFF;            // [4 waves][16][PF_KT]
  float* const stat = reinterpret_cast<float*>(smem) + STAT_F;  // [4][2][16]

  // ---- Q fragments
  constexpr int KS = D / 32;
  bf16x8_t qfrag[KS];
  const int my_qrow = q_base + wid * 16 + col;
  {
    const int r = (my_qrow < L) ? my_qrow : (L - 1);
    const __hip_bfloat16* qrow_p = q + (long)(s0 + r) * q_stride + (long)h * D;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(qrow_p + ks * 32 + kgrp * 8);
      reg_fence(qfrag[ks]);  // wait HERE, not inside the glds pipeline
    }
  }

  float m_run[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
  float l_run[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int DT = D / 16;
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  const int wave_max_row = off + min(q_base + wid * 16 + 15, L - 1);
  const int block_max_row = off + min(q_base + PF_QT - 1, L - 1);
  const int kv_end = block_max_row + 1;
  int kv_begin = 0;
  if (window > 0) {
    const int wave_min_needed = off + q_base + 1 - window;
    kv_begin = max(0, (wave_min_needed / PF_KT) * PF_KT);
  }

  // Out-of-range keys clamp to row Lk-1 (real finite data): K garbage is
  // masked in S, dead keys carry P == 0 into PV — every tile stays on the
  // glds pipeline (see the decode kernel's note).
  auto issue_k = [&](int kt, short* dst) {
#pragma unroll
    for (int j = 0; j < NI_K; ++j) {
      const int g = (wid * NI_K + j) * 64 + lane;  // granule
      const int key = g / CPK;
      const int r8 = (g % CPK) * 8;
      const int d = r8 ^ ((key & 7) << 3);
      const int gk = min(kt + key, Lk - 1);
      const int o2 = __builtin_amdgcn_readfirstlane((wid * NI_K + j) * 512);
      glds16(k + (long)(s0k + gk) * k_stride + (long)kvh * D + d, dst + o2);
    }
  };
  auto issue_v = [&](int kt, short* dst) {
#pragma unroll
    for (int j = 0; j < NI_V; ++j) {
      const int st = wid * NI_V + j;
      const int ks = st / (D / 16), dtile = st % (D / 16);
      const int pos = lane * 8;
      const int bpos = pos / 64, rem = pos % 64;
      const int qq = ((bpos >> 2) & 1) | ((bpos & 3) << 1);
      const int key = ks * 32 + qq * 4 + rem / 16;
      const int dim = dtile * 16 + (rem & 15);
      const int gk = min(kt + key, Lk - 1);
      const int o2 = __builtin_amdgcn_readfirstlane(st * 528);
      glds16(v + (long)(s0k + gk) * v_stride + (long)kvh * D + dim, dst + o2);
    }
  };
  // ---- prologue
  if (kv_begin < kv_end) issue_k(kv_begin, kv0);
  int cur = 0;
  for (int kt = kv_begin; kt < kv_end; kt += PF_KT, cur ^= 1) {
    short* const X = cur ? kv1 : kv0;
    short* const Y = cur ? kv0 : kv1;
    pipe_barrier_vm<0>();

    const bool active = kt <= wave_max_row;  // wave-uniform
    float p[4][4];
    bool rescale = false;  // defer-max decision (set in the S phase)
    if (active) {
      // ---- S = Q K^T for 4 column tiles of 16 keys
      f32x4_t s[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        s[ct] = {0.f, 0.f, 0.f, 0.f};
        const int key = ct * 16 + col;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int d8 = ks * 32 + kgrp * 8;
          bf16x8_t bfrag = *reinterpret_cast<const bf16x8_t*>(
              &X[key * D + swz(key, d8)]);
          s[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[ks], bfrag, s[ct], 0, 0, 0);
        }
      }
      // scale, softcap, mask, row max
      float mx[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int qrow = q_base + wid * 16 + kgrp * 4 + reg;
        const int row = off + qrow;
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
        for (int o3 = 1; o3 < 16; o3 <<= 1) m = fmaxf(m, __shfl_xor(m, o3, WAVE));
        mx[reg] = m;
      }
      // defer-max (guide T13): when no row of this wave grew its max by
      // more than THR, keep the old maxes — P is then bounded by e^THR
      // (fp32 accumulators tolerate it) and the whole O-rescale pass is
      // skipped. The decision covers the ENTIRE tile before any P of it
      // is exponentiated (the T13 ordering hazard), and every l-update
      // uses alpha==1 on the defer path. Accuracy cost ≈3× max-abs error
      // (bounded-P bf16 quantisation) — inside the test tolerances.
      constexpr float DEFER_THR = 8.0f;
      bool grow = false;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        grow |= mx[reg] > m_run[reg] + DEFER_THR;
#ifdef LLMQ_DEFER_ON
      rescale = __any(grow);
#else
      rescale = true; (void)grow;  // defer-max measured a loss; see above
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
        for (int o3 = 1; o3 < 16; o3 <<= 1) lsum += __shfl_xor(lsum, o3, WAVE);
        l_run[reg] = l_run[reg] * alpha + lsum;
        m_run[reg] = m_new;
        if (rescale && col == 0) stat[(wid * 2 + 0) * 16 + kgrp * 4 + reg] = alpha;
      }
    }
    pipe_barrier();  // S reads of X done; alpha visible

    // ---- issue V(kt)->X, K(kt+PF_KT)->Y under the P build + PV
    const int nxt = kt + PF_KT;
    const bool prefetch = nxt < kv_end;
    issue_v(kt, X);
    if (prefetch) issue_k(nxt, Y);

    if (active) {
      // write P rows (bf16) to this wave's tile
      short* const p_lds_w = p_base + wid * 16 * PF_KT;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          p_lds_w[(kgrp * 4 + reg) * PF_KT + ct * 16 + col] =
              __bfloat16_as_short(__float2bfloat16(p[reg][ct]));
        }
      }
    }
    if (prefetch) {
      pipe_barrier_vm<NI_K>();
    } else {
      pipe_barrier_vm<0>();
    }

    if (active) {
      // ---- OT += V^T P^T (O-rescale skipped entirely on the defer path)
      const float alpha_q = rescale ? stat[(wid * 2 + 0) * 16 + col] : 1.f;
      short* const p_lds_w = p_base + wid * 16 * PF_KT;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        if (rescale) {
          ot[dt][0] *= alpha_q; ot[dt][1] *= alpha_q;
          ot[dt][2] *= alpha_q; ot[dt][3] *= alpha_q;
        }
#pragma unroll
        for (int ks = 0; ks < PF_KT / 32; ++ks) {
          const int sub = (ks * (D / 16) + dt) * 528 + lane * 4;
          bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)&X[sub]);
          bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)&X[sub + 4 * 64]);
          bf16x8_t a;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            a[j] = __bfloat16_as_short((__hip_bfloat16)lo[j]);
            a[4 + j] = __bfloat16_as_short((__hip_bfloat16)hi[j]);
          }
          bf16x8_t bb = *reinterpret_cast<const bf16x8_t*>(
              &p_lds_w[col * PF_KT + ks * 32 + kgrp * 8]);
          ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, ot[dt], 0, 0, 0);
        }
      }
    }
    // next loop-top barrier protects X (overwritten two iterations out)
  }

  // ---- epilogue: normalise and store
  if (col == 0) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float l = l_run[reg];
      stat[(wid * 2 + 1) * 16 + kgrp * 4 + reg] = (l > 0.f) ? 1.0f / l : 0.f;
    }
  }
  pipe_barrier();
  const float inv = stat[(wid * 2 + 1) * 16 + col];
  const int orow = q_base + wid * 16 + col;
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
