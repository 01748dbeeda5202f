// Paged attention for gfx950.
//
// DECODE (paged_decode_attention_kernel): the serving hot path. One
// workgroup per (sequence, kv_head); all GQA query heads of that kv head
// are processed together so the KV stream is read ONCE (decode attention
// at D=128/G<=8 is ~4 FLOP/byte — far below the 25:1 VALU roofline, so the
// kernel is designed as a clean HBM stream: 16-byte coalesced K loads,
// two-phase chunk processing with scores staged in LDS, fp32 online
// softmax).
//
//   phase A: 16-lane groups compute q·k for CHUNK tokens -> s[CHUNK][G] LDS
//   phase B: thread (h, d-slice) runs online softmax over the chunk and
//            accumulates p·V into per-thread fp32 registers; V rows are
//            read coalesced by each 32-thread head-group (L1 serves the
//            G-way reuse across head-groups).
//

#include "attention_common.h"

#define DECODE_CHUNK 128  // tokens per two-phase iteration (8 KV blocks @ bs 16)

template <typename T, int HEAD_DIM>
__global__ __launch_bounds__(256) void paged_decode_attention_kernel(
    T* __restrict__ out,                  // [B, H, D] (row stride out_stride)
    const T* __restrict__ q,              // [B, H, D] (row stride q_stride)
    const T* __restrict__ k_cache,        // [nb, KVH, bs, D]
    const T* __restrict__ v_cache,
    const int* __restrict__ block_tables, // [B, max_blocks]
    const int* __restrict__ context_lens, // [B]
    int num_heads, int num_kv_heads, int block_size, int max_blocks,
    float scale, float softcap, int window,
    long q_stride, long out_stride) {
  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int G = num_heads / num_kv_heads;  // <= 8
  const int L = context_lens[b];
  if (L <= 0) return;

  constexpr int VE = Vec8<T>::kElems;        // 8 for bf16, 4 for f32
  constexpr int D = HEAD_DIM;
  constexpr int CHUNK = DECODE_CHUNK;
  const int lane16 = threadIdx.x & 15;       // lane within 16-lane score group
  const int g16 = threadIdx.x >> 4;          // score group id (0..15)

  // Phase-B decomposition: SUBS token-parallel sub-groups per head, each of
  // 32 threads covering all D dims. All 256 threads work for G*32*SUBS==256.
  const int tph = 32 * G;                    // threads per head-set
  const int SUBS = 256 / tph;                // 8,4,2,2,1,1,1,1 for G=1..8
  const int sub = threadIdx.x / tph;         // token sub-group (>=SUBS: idle)
  const int h_b = (threadIdx.x % tph) >> 5;  // head
  constexpr int DPT = D / 32;                // dims per thread (2/4/8)
  const int d0 = (threadIdx.x & 31) * DPT;

  // LDS: q (G x D f32, pre-scaled) | scores (CHUNK x G) | chunk block ids |
  //      merge buffers (SUBS x G x (D + 2))
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* q_s = reinterpret_cast<float*>(smem);              // [G][D]
  float* s_s = q_s + G * D;                                 // [CHUNK][G]
  int* bt_s = reinterpret_cast<int*>(s_s + CHUNK * G);      // [CHUNK/bs up to 16]
  float* merge_s = reinterpret_cast<float*>(bt_s + 16);     // [SUBS][G][D+2]

  for (int i = threadIdx.x; i < G * D; i += blockDim.x) {
    const int h = i / D, d = i % D;
    q_s[i] = to_f32(q[(long)b * q_stride + (long)(kh * G + h) * D + d]) * scale;
  }

  const int start = (window > 0 && L > window) ? (L - window) : 0;
  const int* bt = block_tables + (long)b * max_blocks;
  const int base0 = (start / CHUNK) * CHUNK;

  float acc[DPT];
#pragma unroll
  for (int i = 0; i < DPT; ++i) acc[i] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  for (int base = base0; base < L; base += CHUNK) {
    const int chunk_end = min(base + CHUNK, L);
    const int n = chunk_end - base;
    // stage this chunk's block ids (removes a dependent global load from the
    // phase-B address chain)
    if (threadIdx.x < (unsigned)((n + block_size - 1) / block_size))
      bt_s[threadIdx.x] = bt[(base + threadIdx.x * block_size) / block_size];
    __syncthreads();
    // ---- phase A: scores for tokens [base, chunk_end)
    for (int t0 = g16; t0 < n; t0 += 16) {
      const int t = base + t0;
      const long blk = bt_s[t0 / block_size];
      const int off = t % block_size;
      const T* krow =
          k_cache + (((blk * num_kv_heads + kh) * (long)block_size + off)) * D;
      constexpr int DL = D / 16;  // elems per lane16
      float kf[DL];
      if constexpr (DL % VE == 0) {
#pragma unroll
        for (int c = 0; c < DL; c += VE) {
          Vec8<T> kv = load16(krow + lane16 * DL + c);
#pragma unroll
          for (int j = 0; j < VE; ++j) kf[c + j] = to_f32(kv.data[j]);
        }
      } else {  // e.g. D=64 bf16: 4 elems per lane — scalar loads
#pragma unroll
        for (int c = 0; c < DL; ++c) kf[c] = to_f32(krow[lane16 * DL + c]);
      }
      for (int h = 0; h < G; ++h) {
        float dot = 0.f;
        const float* qrow = q_s + h * D + lane16 * DL;
#pragma unroll
        for (int j = 0; j < DL; ++j) dot += qrow[j] * kf[j];
        dot = group_reduce_sum<16>(dot);
        if (lane16 == 0) {
          if (softcap > 0.f) dot = tanhf(dot / softcap) * softcap;
          if (t < start) dot = -1e30f;
          s_s[t0 * G + h] = dot;
        }
      }
    }
    __syncthreads();
    // ---- phase B: online softmax + V accumulation (sub-group token split)
    if (sub < SUBS) {
      float m_chunk = -1e30f;
      for (int t = sub; t < n; t += SUBS)
        m_chunk = fmaxf(m_chunk, s_s[t * G + h_b]);
      const float m_new = fmaxf(m_run, m_chunk);
      if (m_new > -1e30f) {
        const float alpha = __expf(m_run - m_new);
#pragma unroll
        for (int i = 0; i < DPT; ++i) acc[i] *= alpha;
        l_run *= alpha;
        m_run = m_new;
        // Iterations are independent (chunk-max softmax, no rescale inside)
        // so V loads pipeline across tokens.
        for (int t = sub; t < n; t += SUBS) {
          const float p = __expf(s_s[t * G + h_b] - m_new);
          l_run += p;
          const int tok = base + t;
          const long blk = bt_s[t / block_size];
          const int off = tok % block_size;
          const T* vrow =
              v_cache + (((blk * num_kv_heads + kh) * (long)block_size + off)) * D + d0;
          // Vectorized V row slice: DPT contiguous elems per thread
          // (16B for bf16 D=256, 8B for D=128) — scalar 2B loads here
          // were the v2 bandwidth ceiling.
          if constexpr (DPT % Vec8<T>::kElems == 0) {
            constexpr int VE8 = Vec8<T>::kElems;
#pragma unroll
            for (int c = 0; c < DPT; c += VE8) {
              Vec8<T> vv = load16(vrow + c);
#pragma unroll
              for (int j = 0; j < VE8; ++j) acc[c + j] += p * to_f32(vv.data[j]);
            }
          } else if constexpr (DPT % Vec4<T>::kElems == 0) {
            constexpr int VE4 = Vec4<T>::kElems;
#pragma unroll
            for (int c = 0; c < DPT; c += VE4) {
              Vec4<T> vv = load8(vrow + c);
#pragma unroll
              for (int j = 0; j < VE4; ++j) acc[c + j] += p * to_f32(vv.data[j]);
            }
          } else {
#pragma unroll
            for (int i = 0; i < DPT; ++i) acc[i] += p * to_f32(vrow[i]);
          }
        }
      }
    }
    __syncthreads();  // protect s_s / bt_s for the next chunk
  }

  // ---- merge sub-group partials (flash-decoding style, within the block)
  const int d2 = D + 2;
  if (sub < SUBS && SUBS > 1) {
    float* slot = merge_s + (sub * G + h_b) * d2;
#pragma unroll
    for (int i = 0; i < DPT; ++i) slot[d0 + i] = acc[i];
    if (d0 == 0) {
      slot[D] = m_run;
      slot[D + 1] = l_run;
    }
  }
  __syncthreads();
  if (sub == 0) {
    float m_tot = m_run, l_tot = 0.f;
    if (SUBS > 1) {
      for (int s2 = 0; s2 < SUBS; ++s2)
        m_tot = fmaxf(m_tot, merge_s[(s2 * G + h_b) * d2 + D]);
      float accm[DPT];
#pragma unroll
      for (int i = 0; i < DPT; ++i) accm[i] = 0.f;
      for (int s2 = 0; s2 < SUBS; ++s2) {
        const float* slot = merge_s + (s2 * G + h_b) * d2;
        const float w = __expf(slot[D] - m_tot);
        l_tot += w * slot[D + 1];
#pragma unroll
        for (int i = 0; i < DPT; ++i) accm[i] += w * slot[d0 + i];
      }
#pragma unroll
      for (int i = 0; i < DPT; ++i) acc[i] = accm[i];
    } else {
      l_tot = l_run;
    }
    const float inv = (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
    T* orow = out + (long)b * out_stride + (long)(kh * G + h_b) * D + d0;
#pragma unroll
    for (int i = 0; i < DPT; ++i) orow[i] = from_f32<T>(acc[i] * inv);
  }
}

// ------------------------------------------------------- MFMA paged decode --
// Single-token GQA decode attention on matrix cores (bf16, D in {128,256},
// G <= 16). One workgroup per (sequence, kv_head); the GQA query group is
// padded to a 16-row MFMA tile: q-head g sits in tile row pd_row_head(g), so
// the real rows fill softmax register 0 of every lane first and only
// NREG = ceil(G/4) of a lane's 4 accumulator registers carry a q-head (pad
// rows repeat q-head 0 and are never stored). K and V SHARE one LDS tile
// buffer: per 64-key chunk
//   stage K -> sync -> S = QK^T (wave w: 16-key slab, MFMA 16x16x32) ->
//   sync -> stage V into the same buffer (its HBM latency hides under the
//   softmax VALU work) + combine row maxes / build P / update per-wave l ->
//   sync -> PV: wave w owns dim slab [w*D/4,(w+1)*D/4): OT[dims,16q] +=
//   mfma(A = V^T frags, B = P^T b128 reads) -> sync.
// The block table is staged to LDS once up front (the per-load global
// bt[] read was a dependent-latency chain on every staging address).
// Sharing the tile keeps LDS ~36 KB -> 4 workgroups/CU (the v1 split-K/V
// layout was 68 KB -> 2 WGs/CU and ran SLOWER than the VALU kernel).
// The VALU kernel above is issue-bound (~120 cyc/token/wave); this one
// targets the KV HBM stream rate.

#define PD_MAX_BT 1024  // block-table entries staged in LDS (tail from global)


// KV-cache load: 8 cache elements → bf16x8 fragment. bf16 caches are a raw
// 16-byte load; fp8 (OCP e4m3) caches load 8 bytes and convert on the fly —
// the fp8 KV option halves the decode KV stream.
DEVINL bf16x8_t kv8_to_bf16(const __hip_bfloat16* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}
DEVINL bf16x8_t kv8_to_bf16(const __hip_fp8_e4m3* p) {
  const uint2 raw = *reinterpret_cast<const uint2*>(p);
  return fp8x8_to_bf16(raw.x, raw.y);
}

// ---- device helpers shared by the MFMA decode family (plain, pipe, fp8
// pipe). The kernels differ only in K/V staging and barrier choreography;
// everything below is the common per-lane arithmetic. All are forced inline,
// take registers by reference and LDS regions as pointers into the CALLER's
// storage — a helper must never declare a __shared__ object of its own (the
// pipe kernels rely on having exactly one; see "trap 4a" there). Lane
// coordinates throughout: col = lane & 15 (key for S, q row for OT),
// kgrp = lane >> 4, softmax rows r = kgrp*4 + reg.

// Tile row <-> q-head: a self-inverse 4x4 transpose of the index. Row
// r = kgrp*4 + reg holds head reg*4 + kgrp, so heads 0..3 are register 0 of
// kgrp 0..3, heads 4..7 register 1, ... and registers >= NREG = ceil(G/4)
// hold pad rows only: the per-chunk softmax work (scale, softcap, row max,
// exp, row sum) runs for reg < NREG and skips them.
DEVINL int pd_row_head(int r) { return (r & 3) * 4 + (r >> 2); }

// Q fragments: A-operand rows = padded GQA q rows (row = lane&15 holds
// q-head pd_row_head(row); pad rows repeat q-head 0 and are never stored).
template <int D, bool FENCE>
DEVINL void pd_load_qfrag(bf16x8_t (&qfrag)[D / 32], const __hip_bfloat16* q,
                          int b, int kh, int G, long q_stride, int col, int kgrp) {
  const int g = pd_row_head(col);
  const int qrow = (g < G) ? g : 0;
  const __hip_bfloat16* qp = q + (long)b * q_stride + (long)(kh * G + qrow) * D;
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(qp + ks * 32 + kgrp * 8);
    // FENCE (pipe kernels): wait the load NOW — a first-use inside the
    // loop would make hipcc place `s_waitcnt vmcnt(0)` there, draining
    // the glds pipeline on every iteration (guide §5 trap 4b).
    if constexpr (FENCE) reg_fence(qfrag[ks]);
  }
}

// Sliding-window start, chunk-aligned base, and (gridDim.z > 1) this
// z-block's split-KV slice [range_lo, range_hi) of the chunk range.
template <int PD_KT>
DEVINL void pd_chunk_range(int L, int window, int& start, int& range_lo,
                           int& range_hi) {
  start = (window > 0 && L > window) ? (L - window) : 0;
  const int base0 = (start / PD_KT) * PD_KT;
  const int nsplit = gridDim.z;
  range_lo = base0;
  range_hi = L;
  if (nsplit > 1) {
    const int nchunks = (L - base0 + PD_KT - 1) / PD_KT;
    const int per = (nchunks + nsplit - 1) / nsplit;
    range_lo = base0 + (int)blockIdx.z * per * PD_KT;
    range_hi = min(L, range_lo + per * PD_KT);
  }
}

// Scale, softcap and dead-key mask of this lane's S column (absolute key
// `key`), then the row max over the 16 col lanes, for the NREG registers
// that hold q-heads. The caller stores mx to its per-slab max partials.
template <int NREG>
DEVINL void pd_scale_mask_rowmax(const f32x4_t& s, int key, int L, int start,
                                 float scale, float softcap, float (&sv)[NREG],
                                 float (&mx)[NREG]) {
  const bool dead = key >= L || key < start;
#pragma unroll
  for (int reg = 0; reg < NREG; ++reg) {
    float x = s[reg] * scale;
    if (softcap > 0.f) x = tanhf(x / softcap) * softcap;
    sv[reg] = dead ? -1e30f : x;
    float m = sv[reg];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, WAVE));
    mx[reg] = m;
  }
}

// The chunk loop writes P rows and alpha entries of registers < NREG only;
// the rest still feed the PV MFMA's pad columns and their `ot *= alpha`.
// Set them once (P = 0, alpha = 1) so the kernel never multiplies
// uninitialised LDS. Prologue only: the caller's next barrier publishes it.
template <int NREG, int PD_KT, int NT>
DEVINL void pd_init_pad_rows(short* p_lds, float* alpha_s, int tid) {
  if constexpr (NREG < 4) {
    for (int i = tid; i < 16 * PD_KT; i += NT)
      if (((i / PD_KT) & 3) >= NREG) p_lds[i] = 0;
    if (tid < 16 && (tid & 3) >= NREG) alpha_s[tid] = 1.f;
  }
}

// Combine the per-slab maxes (identical on every wave that runs this), build
// P, update l; stores alpha (wave 0) and this wave's P slab. Returns whether
// OT must be rescaled by alpha this chunk (always, in the default build).
// Used by the two pipe kernels; the plain kernel keeps a fused copy (see
// there).
template <int SLABS, int PD_KT, int NREG>
DEVINL bool pd_softmax_tile(const float* mpart, float* alpha_s, short* p_lds,
                            int slab, int wid, int col, int kgrp,
                            const float (&sv)[NREG], float (&m_regs)[NREG],
                            float (&l_regs)[NREG]) {
  float m_tile[NREG];
#pragma unroll
  for (int reg = 0; reg < NREG; ++reg) {
    const int row = kgrp * 4 + reg;
    float m = mpart[row];
#pragma unroll
    for (int w = 1; w < SLABS; ++w) m = fmaxf(m, mpart[w * 16 + row]);
    m_tile[reg] = m;
  }
  // defer-max (guide T13): every wave computes m_regs/m_tile from the
  // same mpart values with the same op order, so the ballot below is
  // workgroup-uniform with no extra LDS flag. On the defer path
  // alpha==1 exactly: the alpha_s store AND the whole OT-rescale pass
  // are skipped; P is bounded by e^THR (l/OT accumulate in fp32).
  bool grow = false;
#pragma unroll
  for (int reg = 0; reg < NREG; ++reg) grow |= m_tile[reg] > m_regs[reg] + 8.0f;
#ifdef LLMQ_DEFER_ON
  const bool rescale = __any(grow);
#else
  // Measured: the T13 defer guard LOSES here (decode 0.458 vs 0.442 ms,
  // prefill 0.282 vs 0.261 ms same-box A/B) — the branch around the
  // O-rescale disturbs the pipelined PV scheduling more than the skipped
  // VALU pays. Kept compilable behind -DLLMQ_DEFER_ON for re-testing.
  const bool rescale = true; (void)grow;
#endif
#pragma unroll
  for (int reg = 0; reg < NREG; ++reg) {
    const int row = kgrp * 4 + reg;
    const float m_new = rescale ? fmaxf(m_regs[reg], m_tile[reg]) : m_regs[reg];
    const float alpha = (rescale && m_new > -1e30f)
                            ? __expf(m_regs[reg] - m_new) : 1.f;
    const float pe = (m_new > -1e30f && sv[reg] > -1e29f)
                         ? __expf(sv[reg] - m_new) : 0.f;
    float lsum = pe;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) lsum += __shfl_xor(lsum, off, WAVE);
    l_regs[reg] = l_regs[reg] * alpha + lsum;
    m_regs[reg] = m_new;
    if (rescale && wid == 0 && col == 0) alpha_s[row] = alpha;
    p_lds[row * PD_KT + slab * 16 + col] =
        __bfloat16_as_short(__float2bfloat16(pe));
  }
  return rescale;
}

// Epilogue after the per-slab l partials are visible in l_part: sum l, then
// either (gridDim.z > 1) write this z-block's UNNORMALISED fp32 partial rows
// and their (m, l) stats to scratch, or normalise and store bf16 to out.
// OT column `col` is tile row col, i.e. q-head g = pd_row_head(col): both
// paths index out / scratch by g (the merge kernel reads scratch rows by g).
template <int D, int SLABS, int DT, int NREG>
DEVINL void pd_store(__hip_bfloat16* out, float* scratch, const float* l_part,
                     const f32x4_t (&ot)[DT], const float (&m_regs)[NREG], int b,
                     int kh, int G, int num_kv_heads, long out_stride, int wid,
                     int col, int kgrp) {
  constexpr int D4 = DT * 16;  // dim slab per wave
  const int nsplit = gridDim.z;
  const int g = pd_row_head(col);
  if (nsplit > 1) {
    float* slot = scratch +
        ((((long)b * num_kv_heads + kh) * nsplit + blockIdx.z) * G) * (D + 2);
    if (g < G) {
      float* row = slot + (long)g * (D + 2);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int dim0 = wid * D4 + dt * 16 + kgrp * 4;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) row[dim0 + reg] = ot[dt][reg];
      }
    }
    // Row stats: wave-0 lanes with col==0 cover rows r = kgrp*4+reg, which
    // hold heads reg*4+kgrp (wave 0 always runs the shared-max combine).
    if (wid == 0 && col == 0) {
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg) {
        const int r = kgrp * 4 + reg;
        const int gr = reg * 4 + kgrp;
        if (gr < G) {
          float* row = slot + (long)gr * (D + 2);
          row[D] = m_regs[reg];
          float lt = l_part[r];
          for (int w = 1; w < SLABS; ++w) lt += l_part[w * 16 + r];
          row[D + 1] = lt;
        }
      }
    }
    return;
  }
  if (g < G) {
    float l_tot = l_part[col];
#pragma unroll
    for (int w = 1; w < SLABS; ++w) l_tot += l_part[w * 16 + col];
    const float inv = (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
    __hip_bfloat16* op = out + (long)b * out_stride + (long)(kh * G + g) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int dim0 = wid * D4 + dt * 16 + kgrp * 4;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        op[dim0 + reg] = __float2bfloat16(ot[dt][reg] * inv);
    }
  }
}

// NW = waves per workgroup (4 -> 256 threads/64-key chunks; 8 -> 512
// threads/128-key chunks: same waves/SIMD at half the barriers per token).
// With gridDim.z == NSPLIT > 1 (flash-decoding split-KV: small B×KVH, e.g.
// tensor-parallel ranks holding one kv head), each z-workgroup covers a
// slice of the context and writes UNNORMALISED fp32 partials
// (acc[G][D], m, l) to scratch[B][KVH][NSPLIT][G][D+2]; the
// decode_splitkv_merge_kernel combines them. NSPLIT==1 writes out directly.
// NREG = softmax registers that hold q-heads (ceil(G/4) rounded to 1/2/4;
// the launcher picks it from G).
template <int HEAD_DIM, int NW, int NREG, typename TC = __hip_bfloat16>
__global__ __launch_bounds__(NW * WAVE) void paged_decode_mfma_kernel(
    __hip_bfloat16* __restrict__ out,      // [B, H, D]
    const __hip_bfloat16* __restrict__ q,  // [B, H, D]
    const TC* __restrict__ k_cache,        // [nb, KVH, bs, D]
    const TC* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [B, max_blocks]
    const int* __restrict__ context_lens,  // [B]
    float* __restrict__ scratch,           // [B,KVH,NSPLIT,G,D+2] (NSPLIT>1)
    int num_heads, int num_kv_heads, int block_size, int max_blocks,
    float scale, float softcap, int window, long q_stride, long out_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int KS = D / 32;      // MFMA K-steps over the head dim
  constexpr int PD_KT = NW * 16;  // keys per chunk
  constexpr int NT = NW * WAVE;   // threads per workgroup
  constexpr int D4 = D / NW;      // dim slab per wave
  constexpr int DT = D4 / 16;     // 16-dim MFMA tiles per wave
  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int G = num_heads / num_kv_heads;  // <= 16
  const int L = context_lens[b];
  if (L <= 0) return;

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;   // MFMA col lane (key for S, qrow for OT)
  const int kgrp = lane >> 4;  // 0..3

  __shared__ __attribute__((aligned(16))) short kv_lds[kv_tile_elems(PD_KT, D)];  // K then V
  __shared__ __attribute__((aligned(16))) short p_lds[16 * PD_KT];  // [qrow][key]
  __shared__ float mpart_lds[NW][16];  // per-wave row-max partials
  __shared__ float alpha_lds[16];      // per-row rescale for the OT lanes
  __shared__ float l_lds[NW][16];      // per-wave l_run (end merge)
  __shared__ int bt_lds[PD_MAX_BT];

  // ---- stage the block table once (removes a dependent global load from
  // every staging address); contexts past PD_MAX_BT blocks (16k tokens at
  // bs 16) read the tail entries from global instead
  const int* bt_glob = block_tables + (long)b * max_blocks;
  {
    const int nb = (L + block_size - 1) / block_size;
    const int nstage = nb < PD_MAX_BT ? nb : PD_MAX_BT;
    for (int i = tid; i < nstage; i += NT) bt_lds[i] = bt_glob[i];
  }

  // ---- Q fragments: A-operand rows = padded q rows (row = lane&15)
  bf16x8_t qfrag[KS];
  pd_load_qfrag<D, false>(qfrag, q, b, kh, G, q_stride, col, kgrp);

  // softmax state: every wave redundantly tracks rows r = kgrp*4 + reg
  float m_regs[NREG], l_regs[NREG];
#pragma unroll
  for (int reg = 0; reg < NREG; ++reg) { m_regs[reg] = -1e30f; l_regs[reg] = 0.f; }
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  int start, range_lo, range_hi;
  pd_chunk_range<PD_KT>(L, window, start, range_lo, range_hi);
  constexpr int CPK = D / 8;    // 16B chunks per key row
  constexpr int NCK = PD_KT * CPK;
  // block_size is 16 or 32 (launcher precondition): shift and mask, not
  // a runtime divide, on every staged granule
  const int bs_shift = 31 - __builtin_clz(block_size);
  const int bs_mask = block_size - 1;
  pd_init_pad_rows<NREG, PD_KT, NT>(p_lds, alpha_lds, tid);
  __syncthreads();  // bt_lds ready

  for (int base = range_lo; base < range_hi; base += PD_KT) {
    // ---- stage K chunk (gather via LDS block table; zeros beyond L)
    for (int c = tid; c < NCK; c += NT) {
      const int key = c / CPK;
      const int d8 = (c % CPK) * 8;
      const int dst = key * D + swz(key, d8);
      const int gkey = base + key;
      if (gkey < L) {
        const int bidx = gkey >> bs_shift;
        const long blk = (bidx < PD_MAX_BT) ? bt_lds[bidx] : bt_glob[bidx];
        const long rowoff =
            ((blk * num_kv_heads + kh) * block_size + (gkey & bs_mask)) * D + d8;
        *reinterpret_cast<bf16x8_t*>(&kv_lds[dst]) = kv8_to_bf16(k_cache + rowoff);
      } else {
        *reinterpret_cast<bf16x8_t*>(&kv_lds[dst]) = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    __syncthreads();

    // ---- S[16, 16] for this wave's key slab
    const f32x4_t s = attn_s_slab<D>(qfrag, kv_lds, wid * 16 + col, kgrp);
    // scale, softcap, bounds mask; rows r = kgrp*4 + reg
    float sv[NREG], mx[NREG];
    pd_scale_mask_rowmax<NREG>(s, base + wid * 16 + col, L, start, scale, softcap,
                               sv, mx);
    if (col == 0) {
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg) mpart_lds[wid][kgrp * 4 + reg] = mx[reg];
    }
    __syncthreads();  // mparts ready; every wave is past its K reads

    // ---- stage V into the SAME buffer; its latency hides under softmax VALU.
    // V uses the tr16 subtile image (NOT K's swizzled rows).
    for (int c = tid; c < NCK; c += NT) {
      const int key = c / CPK;
      const int d8 = (c % CPK) * 8;
      const int dst = v_img_index<D>(key, d8);
      const int gkey = base + key;
      if (gkey < L) {
        const int bidx = gkey >> bs_shift;
        const long blk = (bidx < PD_MAX_BT) ? bt_lds[bidx] : bt_glob[bidx];
        const long rowoff =
            ((blk * num_kv_heads + kh) * block_size + (gkey & bs_mask)) * D + d8;
        *reinterpret_cast<bf16x8_t*>(&kv_lds[dst]) = kv8_to_bf16(v_cache + rowoff);
      } else {
        *reinterpret_cast<bf16x8_t*>(&kv_lds[dst]) = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }

    // ---- combine maxes (identical on every wave), build P, update l
    // Same arithmetic as pd_softmax_tile<NW, PD_KT, NREG> with slab == wid,
    // kept as one fused loop: with NW max partials per row, the helper's
    // combine-all-rows-first order costs this kernel 14 VGPRs at D=256.
#pragma unroll
    for (int reg = 0; reg < NREG; ++reg) {
      const int row = kgrp * 4 + reg;
      float m_tile = mpart_lds[0][row];
#pragma unroll
      for (int w = 1; w < NW; ++w) m_tile = fmaxf(m_tile, mpart_lds[w][row]);
      const float m_new = fmaxf(m_regs[reg], m_tile);
      const float alpha = (m_new > -1e30f) ? __expf(m_regs[reg] - m_new) : 1.f;
      const float pe = (m_new > -1e30f && sv[reg] > -1e29f)
                           ? __expf(sv[reg] - m_new) : 0.f;
      float lsum = pe;
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) lsum += __shfl_xor(lsum, off, WAVE);
      l_regs[reg] = l_regs[reg] * alpha + lsum;
      m_regs[reg] = m_new;
      if (wid == 0 && col == 0) alpha_lds[row] = alpha;
      p_lds[row * PD_KT + wid * 16 + col] =
          __bfloat16_as_short(__float2bfloat16(pe));
    }
    __syncthreads();  // V + P + alpha ready

    // ---- OT[dims, 16q] += V^T P^T over this wave's dim slab
    attn_pv_tile<D, PD_KT, DT>(kv_lds, p_lds, alpha_lds, true, ot, wid * DT, lane);
    __syncthreads();  // V/P consumed; next chunk may overwrite
  }

  // ---- merge per-wave l, then store (normalised out, or raw partials)
  if (col == 0) {
#pragma unroll
    for (int reg = 0; reg < NREG; ++reg) l_lds[wid][kgrp * 4 + reg] = l_regs[reg];
  }
  __syncthreads();
  pd_store<D, NW, DT, NREG>(out, scratch, &l_lds[0][0], ot, m_regs, b, kh, G,
                            num_kv_heads, out_stride, wid, col, kgrp);
}

// -------------------------------------------- pipelined MFMA paged decode --
// Software-pipelined variant of paged_decode_mfma_kernel (round-2 item from
// profiles/r1_step6_decode_tuning_story.md: the stage→S→stats→PV phase
// serialization left ~30% of the KV stream rate on the table, and both
// register-prefetch and occupancy-costing fixes measured WORSE — the fix
// has to add zero VGPRs and keep the 2-workgroups/CU residency).
//
// Structure (per CDNA4 guide §5 "Pipelining across barriers" + §5.5 T3/T4):
//   - TWO chunk buffers A/B; chunk i's K lives in buf[i&1], V overwrites the
//     same buffer after S (the r1 shared-buffer trick), K(i+1) prefetches
//     into buf[(i+1)&1].
//   - ALL staging is `global_load_lds` (no VGPR round-trip, no staging
//     instructions on the VALU): the LDS image is lane-linear per wave
//     instruction, so K's XOR swizzle and V's image permutation (line image
//     or tr16 subtile image, see V_LINES) move to the per-lane SOURCE
//     address (guide §5.4 rule 21).
//   - Raw `s_barrier` + counted `s_waitcnt vmcnt(N)`: V(i)+K(i+1) issue
//     back-to-back right after the post-S barrier; the pre-PV barrier waits
//     vmcnt(NI_K) (V landed, K still streaming); the loop-top barrier waits
//     vmcnt(0) (K landed). A `__syncthreads()` would drain the glds queue
//     at every barrier (the documented HIP-compiler ceiling).
//   - glds cannot zero-fill, so keys past L (the chunk containing L) clamp
//     their source to cache row L-1: finite real data, masked in S and
//     carrying P == 0 into PV. Every chunk stays on the pipeline.
// Per-workgroup timeline: the only window with no HBM traffic in flight is
// the S phase (~hundreds of cycles vs ~6 µs of stream per chunk).

// min waves/SIMD: the 64-key chunk fits 2 workgroups/CU by LDS (4 waves/
// SIMD) — force the register allocator to <=128 VGPRs so VGPRs don't cap
// occupancy below that (the r1 lesson: this kernel is governed by
// waves/SIMD, every latency trick that cost occupancy lost). The 128-key
// chunk is 1 workgroup/CU by LDS (2 waves/SIMD) — let it use 196.
// V_LINES: which LDS image V is staged in. false = the tr16 subtile image
// (one V DMA takes 32 bytes from each of 32 cache rows); true = the line
// image of attention_common.h (one V DMA takes eight whole 128-byte lines of
// eight rows, 2 KiB less LDS per buffer pair). Same DMA count, same PV
// operands and MFMA order: outputs are bitwise equal.
// KV_NT: cache policy of the K/V DMAs. The decode K/V stream is read once per
// step, so it can go `nt` past L2 and the Infinity Cache wherever ONE
// instruction consumes the whole 128-byte line: 0 = default policy, 1 = K
// `nt` (a K DMA covers two 512-byte key rows), 2 = K and V `nt` (line image
// only: a subtile DMA leaves 96 bytes of every line to the same wave's next
// three DMAs, which must hit the line in L2; with `nt` there the kernel
// measured 0.468 against 0.369 ms, profiles/decode_kv_stream.md).
// Block-table loads, q loads and stores keep the default policy.
template <int HEAD_DIM, int NW, int PD_KT, int NREG, int KV_NT, bool V_LINES>
__global__ __launch_bounds__(NW * WAVE, (PD_KT <= 64 ? 4 : 2)) void paged_decode_pipe_kernel(
    __hip_bfloat16* __restrict__ out,      // [B, H, D]
    const __hip_bfloat16* __restrict__ q,  // [B, H, D]
    const __hip_bfloat16* __restrict__ k_cache,  // [nb, KVH, bs, D]
    const __hip_bfloat16* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [B, max_blocks<=PD_MAX_BT]
    const int* __restrict__ context_lens,  // [B]
    float* __restrict__ scratch,           // [B,KVH,NSPLIT,G,D+2] (NSPLIT>1)
    int num_heads, int num_kv_heads, int block_size, int max_blocks,
    float scale, float softcap, int window, long q_stride, long out_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int KS = D / 32;        // MFMA K-steps over the head dim
  constexpr int NT = NW * WAVE;     // threads per workgroup
  constexpr int SLABS = PD_KT / 16; // 16-key S slabs (<= NW; extra waves skip S)
  constexpr int D4 = D / NW;        // dim slab per wave (PV)
  constexpr int DT = D4 / 16;       // 16-dim MFMA tiles per wave
  constexpr int CPK = D / 8;        // 16B granules per key row
  constexpr int NI_K = PD_KT * CPK / NT;          // K glds per wave per chunk
  // V DMAs per chunk: tr-subtiles, or 8-key × 64-dim pieces (as many)
  constexpr int NSUB = V_LINES ? v_line_npiece(PD_KT, D) : v_img_nsub(PD_KT, D);
  constexpr int NI_V = NSUB / NW;                 // V glds per wave per chunk
  constexpr int KV_ELEMS = V_LINES ? PD_KT * D : kv_tile_elems(PD_KT, D);
  constexpr int PPO = D / 64;                     // line image: pieces per key octet
  constexpr int NVB = v_line_nbase<D, DT>();
  static_assert(PD_KT % 32 == 0 && SLABS <= NW && NSUB % NW == 0, "");
  static_assert(PD_KT * CPK % NT == 0 && D % NW == 0 && D4 % 16 == 0, "");
  static_assert(!V_LINES || (v_line_layout_ok_v<PD_KT, D, DT> &&
                             v_line_elems(PD_KT, D) <= KV_ELEMS),
                "V line image layout");
  static_assert(V_LINES || KV_NT < 2, "the subtile image cannot stream V nt");

  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int G = num_heads / num_kv_heads;  // <= 16
  const int L = context_lens[b];
  if (L <= 0) return;

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int kgrp = lane >> 4;
  const int slab = wid % SLABS;
  // Waves beyond the S slabs (64-key chunks: waves 4..7 of 8) have no slab
  // of their own: their S, softcap, row max and softmax would repeat a
  // lower wave's, on the same SIMD, and nothing reads the copy. They skip
  // that work (wave-uniform branches, no barrier inside) and still reach
  // every barrier, issue their share of the DMA and run PV. The defer-max
  // build keeps the copies: its ballot needs m_regs current on every wave.
#ifdef LLMQ_DEFER_ON
  constexpr bool s_wave = true;
#else
  const bool s_wave =
      SLABS == NW || __builtin_amdgcn_readfirstlane(wid) < SLABS;
#endif
  // block_size is 16 or 32 (launcher precondition): shift and mask, not a
  // runtime divide, in every DMA source address; the kv-head base and the
  // per-block stride are chunk-invariant scalars
  const int bs_shift = 31 - __builtin_clz(block_size);
  const int bs_mask = block_size - 1;
  const long blk_stride = (long)num_kv_heads * block_size * D;
  const long head_off = (long)kh * block_size * D;

  // ONE shared array (guide §5 trap 4a: a second __shared__ object makes
  // hipcc drain vmcnt(0) before every ds_read while a glds is in flight).
  constexpr int P_OFF = 2 * KV_ELEMS;                  // shorts
  constexpr int MPART_OFF = P_OFF + 16 * PD_KT;        // floats from here
  constexpr int F_BASE = (MPART_OFF * 2 + 15) / 16 * 4;  // float index base
  constexpr int ALPHA_F = F_BASE + SLABS * 16;
  constexpr int LPART_F = ALPHA_F + 16;
  constexpr int BT_I = LPART_F + SLABS * 16;           // int index base
  constexpr int TOTAL_BYTES = BT_I * 4 + PD_MAX_BT * 4;
  __shared__ __attribute__((aligned(16))) char smem[TOTAL_BYTES];
  short* const kv0 = reinterpret_cast<short*>(smem);
  short* const kv1 = kv0 + KV_ELEMS;
  short* const p_lds2 = kv0 + P_OFF;                   // [16][PD_KT] bf16
  float* const fbase = reinterpret_cast<float*>(smem);
  float* const mpart = fbase + F_BASE;                 // [SLABS][16]
  float* const alpha_s = fbase + ALPHA_F;              // [16]
  float* const l_part = fbase + LPART_F;               // [SLABS][16]
  int* const bt_l = reinterpret_cast<int*>(smem) + BT_I;  // [PD_MAX_BT]

  // ---- stage the block table once (plain loads; nb <= PD_MAX_BT is a
  // dispatch precondition for this kernel)
  const int* bt_glob = block_tables + (long)b * max_blocks;
  {
    const int nb = (L + block_size - 1) / block_size;
    for (int i = tid; i < nb; i += NT) bt_l[i] = bt_glob[i];
  }

  // ---- Q fragments (padded GQA rows; row = lane&15)
  bf16x8_t qfrag[KS];
  pd_load_qfrag<D, true>(qfrag, q, b, kh, G, q_stride, col, kgrp);

  float m_regs[NREG], l_regs[NREG];
#pragma unroll
  for (int reg = 0; reg < NREG; ++reg) { m_regs[reg] = -1e30f; l_regs[reg] = 0.f; }
  pd_init_pad_rows<NREG, PD_KT, NT>(p_lds2, alpha_s, tid);
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  int start, range_lo, range_hi;
  pd_chunk_range<PD_KT>(L, window, start, range_lo, range_hi);

  // Per-lane source row+offset for K granule g of a chunk (inverse swizzle
  // on the source: LDS image is lane-linear, content matches swz()).
  // Out-of-range keys (tail chunk / z-range end) clamp to row L-1: a real
  // written cache row, so the staged garbage is FINITE; K garbage is
  // masked in S (-1e30) and dead keys carry P == 0, so finite V garbage
  // contributes exactly 0 to PV. This keeps EVERY chunk on the glds
  // pipeline (no zero-filled plain-staged tail).
  auto k_src = [&](int base, int g) -> const __hip_bfloat16* {
    const int key = g / CPK;
    const int r8 = (g % CPK) * 8;
    const int d = r8 ^ ((key & 7) << 3);
    const int gkey = min(base + key, L - 1);
    const long blk = bt_l[gkey >> bs_shift];
    return k_cache + head_off + blk * blk_stride + ((gkey & bs_mask) * D + d);
  };
  // V: subtile st, in-subtile granule = lane (tr16 image inverse mapping).
  // Line image: piece st, in-piece slot = lane (v_line_source).
  auto v_src = [&](int base, int st) -> const __hip_bfloat16* {
    const VImgSrc s = V_LINES ? v_line_source<D>(st, lane) : v_img_source<D>(st, lane);
    const int gkey = min(base + s.key, L - 1);
    const long blk = bt_l[gkey >> bs_shift];
    return v_cache + head_off + blk * blk_stride + ((gkey & bs_mask) * D + s.dim);
  };

  // All source addresses first, then the DMAs back to back: glds16 is an
  // asm with a memory clobber, so a block-table read placed between two of
  // them cannot be batched or shared with its neighbours by the compiler.
  auto issue_k = [&](int base, short* dst) {
    const __hip_bfloat16* src[NI_K];
#pragma unroll
    for (int j = 0; j < NI_K; ++j) src[j] = k_src(base, (wid * NI_K + j) * 64 + lane);
#pragma unroll
    for (int j = 0; j < NI_K; ++j) {
      const int off = __builtin_amdgcn_readfirstlane((wid * NI_K + j) * 512);
      glds16<(KV_NT >= 1)>(src[j], dst + off);
    }
  };
  // A wave's NI_V subtiles are consecutive 16-dim tiles of ONE 32-key group,
  // so its lanes read the same cache row for all of them: one row address
  // per chunk, then a 16-element step per subtile (v_img_source's key/dim
  // progression, part of the compile-time layout check).
  // Line image: a wave's NI_V pieces are the PPO pieces of NI_V/PPO whole key
  // octets (one for 64-key chunks, two for 128), so again one row address
  // per octet and a 64-element step per piece, each DMA eight whole lines.
  static_assert(V_LINES || (D / 16) % NI_V == 0, "a wave's V subtiles share their keys");
  static_assert(!V_LINES || NI_V % PPO == 0, "a wave's V pieces are whole key octets");
  auto issue_v = [&](int base, short* dst) {
    if constexpr (V_LINES) {
      const __hip_bfloat16* row[NI_V / PPO];
#pragma unroll
      for (int oo = 0; oo < NI_V / PPO; ++oo) row[oo] = v_src(base, wid * NI_V + oo * PPO);
#pragma unroll
      for (int j = 0; j < NI_V; ++j) {
        const int off =
            __builtin_amdgcn_readfirstlane((wid * NI_V + j) * V_PIECE_ELEMS);
        glds16<(KV_NT >= 2)>(row[j / PPO] + (j % PPO) * 64, dst + off);
      }
    } else {
      const __hip_bfloat16* const row = v_src(base, wid * NI_V);
#pragma unroll
      for (int j = 0; j < NI_V; ++j) {
        const int off =
            __builtin_amdgcn_readfirstlane((wid * NI_V + j) * V_SUB_STRIDE);
        glds16(row + j * 16, dst + off);  // default policy: see KV_NT
      }
    }
  };
  // Line image: this lane's PV read bases for the wave's dim slab, in
  // elements; a PV read is base + compile-time offset (v_line_rd_off).
  int vb[NVB];
#pragma unroll
  for (int i = 0; i < NVB; ++i) vb[i] = v_line_rd_base<D>(wid * DT, i, lane);
  // ---- prologue: block table visible, then K(first) in flight
  pipe_barrier();  // bt_l ready (plain ds_writes; lgkm drain)
  if (range_lo < range_hi) issue_k(range_lo, kv0);

  int cur = 0;
  for (int base = range_lo; base < range_hi; base += PD_KT, cur ^= 1) {
    short* const X = cur ? kv1 : kv0;
    short* const Y = cur ? kv0 : kv1;
    pipe_barrier_vm<0>();  // K(base) landed (all waves)

    // ---- S[16,16] for this wave's slab
    float sv[NREG];
    if (s_wave) {
      const int key = slab * 16 + col;
      const f32x4_t s = attn_s_slab<D>(qfrag, X, key, kgrp);
      float mx[NREG];
      pd_scale_mask_rowmax<NREG>(s, base + key, L, start, scale, softcap, sv, mx);
      if (col == 0 && wid < SLABS) {
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg) mpart[slab * 16 + kgrp * 4 + reg] = mx[reg];
      }
    }
    pipe_barrier();  // S reads of X done everywhere; mpart visible

    // ---- issue V(base)->X then K(next)->Y; both stream under softmax/PV
    const int next = base + PD_KT;
    const bool prefetch = next < range_hi;
    issue_v(base, X);
    if (prefetch) issue_k(next, Y);

    // ---- combine maxes, build P, update l (one wave per slab)
    bool rescale = true;
    if (s_wave)
      rescale = pd_softmax_tile<SLABS, PD_KT, NREG>(
          mpart, alpha_s, p_lds2, slab, wid, col, kgrp, sv, m_regs, l_regs);
    if (prefetch) {
      pipe_barrier_vm<NI_K>();  // V landed; K(next) stays in flight
    } else {
      pipe_barrier_vm<0>();
    }

    // ---- OT[dims,16q] += V^T P^T over this wave's dim slab
    if constexpr (V_LINES)
      attn_pv_tile_lines<D, PD_KT, DT>(X, vb, p_lds2, alpha_s, rescale, ot, lane);
    else
      attn_pv_tile<D, PD_KT, DT>(X, p_lds2, alpha_s, rescale, ot, wid * DT, lane);
    // No trailing barrier: the next loop-top barrier (vmcnt(0)) both
    // protects X against the glds of chunk base+2 (issued only after the
    // NEXT post-S barrier) and confirms K(next) landed in Y.
  }

  // ---- merge per-slab l, then store (normalised out, or raw partials)
  if (col == 0 && wid < SLABS) {
#pragma unroll
    for (int reg = 0; reg < NREG; ++reg) l_part[slab * 16 + kgrp * 4 + reg] = l_regs[reg];
  }
  pipe_barrier();
  pd_store<D, SLABS, DT, NREG>(out, scratch, l_part, ot, m_regs, b, kh, G,
                               num_kv_heads, out_stride, wid, col, kgrp);
}

// --------------------------------------- fp8-KV pipelined MFMA decode --
// The glds pipeline for fp8 (OCP e4m3) caches: HALF the KV stream of
// bf16. glds cannot convert during the LDS write, so:
//   - K stays fp8 IN LDS ([PD_KT][D] bytes, 16B-granule XOR swizzle on
//     the source); the S phase reads 8-byte fragments and converts with
//     the native packed cvt VOPs (one v_cvt_pk_f32_fp8 per 4 elems).
//   - V stages RAW fp8 into the scratch back-half of the OTHER K/V-image
//     buffer, then a convert pass (during the softmax window) writes the
//     bf16 tr16 subtile image the PV path expects.
// Buffer choreography per chunk i (X = img[i&1], Y = img[(i+1)&1]):
//   top: vm(0) barrier [K(i) in X front]  ->  S(i) from X (fp8+cvt)
//   post-S barrier -> issue V(i)raw -> Y back;  K(i+1) -> Y front
//   softmax/P  ->  vm(NI_K) barrier [V raw landed; K(i+1) flying]
//   convert pass: Y back (raw) -> X image (overwrites K(i): dead)
//   lgkm barrier -> PV(i) from X image
// Y-back is free during i (its image is only rebuilt by i+1's convert);
// Y-front K(i+1) and Y-back V(i)raw are disjoint ranges. LDS stays at
// 2 × image + p + bt ≈ 74 KB -> 2 workgroups/CU, same as the bf16 pipe.
// KV_NT: both DMAs (fp8 K rows and the linear raw V) consume whole lines, so
// both stream `nt`.

template <int HEAD_DIM, int NW, int NREG, bool KV_NT>
__global__ __launch_bounds__(NW * WAVE, 4) void paged_decode_pipe_fp8_kernel(
    __hip_bfloat16* __restrict__ out,      // [B, H, D]
    const __hip_bfloat16* __restrict__ q,  // [B, H, D]
    const __hip_fp8_e4m3* __restrict__ k_cache,  // [nb, KVH, bs, D]
    const __hip_fp8_e4m3* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [B, max_blocks<=PD_MAX_BT]
    const int* __restrict__ context_lens,  // [B]
    float* __restrict__ scratch,           // [B,KVH,NSPLIT,G,D+2] (NSPLIT>1)
    int num_heads, int num_kv_heads, int block_size, int max_blocks,
    float scale, float softcap, int window, long q_stride, long out_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int KS = D / 32;
  constexpr int PD_KT = 64;
  constexpr int NT = NW * WAVE;
  constexpr int SLABS = PD_KT / 16;     // 4 (waves 4..7 skip S when NW=8)
  constexpr int D4 = D / NW;
  constexpr int DT = D4 / 16;
  constexpr int G16B = D / 16;          // 16B granules per fp8 key row
  constexpr int NI_K = PD_KT * G16B / NT;   // fp8-K glds per wave
  constexpr int NI_VR = NI_K;               // raw fp8-V glds per wave
  constexpr int IMG_ELEMS = v_img_elems(PD_KT, D);  // bf16 tr16 image (shorts)
  constexpr int RAW_BYTES = PD_KT * D;      // fp8 K front == raw V size
  static_assert(IMG_ELEMS * 2 >= 2 * RAW_BYTES,
                "image must cover K-front + V-raw back");
  static_assert(NI_K >= 1 && D % NW == 0 && D4 % 16 == 0, "");

  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int G = num_heads / num_kv_heads;
  const int L = context_lens[b];
  if (L <= 0) return;

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int col = lane & 15;
  const int kgrp = lane >> 4;
  const int slab = wid % SLABS;
  // Waves beyond the S slabs (64-key chunks: waves 4..7 of 8) have no slab
  // of their own: their S, softcap, row max and softmax would repeat a
  // lower wave's, on the same SIMD, and nothing reads the copy. They skip
  // that work (wave-uniform branches, no barrier inside) and still reach
  // every barrier, issue their share of the DMA and run PV. The defer-max
  // build keeps the copies: its ballot needs m_regs current on every wave.
#ifdef LLMQ_DEFER_ON
  constexpr bool s_wave = true;
#else
  const bool s_wave =
      SLABS == NW || __builtin_amdgcn_readfirstlane(wid) < SLABS;
#endif
  // block_size is 16 or 32 (launcher precondition): shift and mask, not a
  // runtime divide, in every DMA source address; the kv-head base and the
  // per-block stride are chunk-invariant scalars
  const int bs_shift = 31 - __builtin_clz(block_size);
  const int bs_mask = block_size - 1;
  const long blk_stride = (long)num_kv_heads * block_size * D;
  const long head_off = (long)kh * block_size * D;

  constexpr int P_OFF = 2 * IMG_ELEMS;                   // shorts
  constexpr int F_BASE = (P_OFF + 16 * PD_KT + 7) / 8 * 4;
  constexpr int ALPHA_F = F_BASE + SLABS * 16;
  constexpr int LPART_F = ALPHA_F + 16;
  constexpr int BT_I = LPART_F + SLABS * 16;
  constexpr int TOTAL_BYTES = BT_I * 4 + PD_MAX_BT * 4;
  __shared__ __attribute__((aligned(16))) char smem[TOTAL_BYTES];
  short* const img0 = reinterpret_cast<short*>(smem);
  short* const img1 = img0 + IMG_ELEMS;
  short* const p_lds2 = img0 + P_OFF;
  float* const fbase = reinterpret_cast<float*>(smem);
  float* const mpart = fbase + F_BASE;
  float* const alpha_s = fbase + ALPHA_F;
  float* const l_part = fbase + LPART_F;
  int* const bt_l = reinterpret_cast<int*>(smem) + BT_I;

  const int* bt_glob = block_tables + (long)b * max_blocks;
  {
    const int nb = (L + block_size - 1) / block_size;
    for (int i = tid; i < nb; i += NT) bt_l[i] = bt_glob[i];
  }

  bf16x8_t qfrag[KS];
  pd_load_qfrag<D, true>(qfrag, q, b, kh, G, q_stride, col, kgrp);

  float m_regs[NREG], l_regs[NREG];
#pragma unroll
  for (int reg = 0; reg < NREG; ++reg) { m_regs[reg] = -1e30f; l_regs[reg] = 0.f; }
  pd_init_pad_rows<NREG, PD_KT, NT>(p_lds2, alpha_s, tid);
  f32x4_t ot[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) ot[dt] = {0.f, 0.f, 0.f, 0.f};

  int start, range_lo, range_hi;
  pd_chunk_range<PD_KT>(L, window, start, range_lo, range_hi);

  auto kv_row = [&](int gkey, const __hip_fp8_e4m3* cache) -> const __hip_fp8_e4m3* {
    const int ck = min(gkey, L - 1);  // clamp: finite real data (masked)
    const long blk = bt_l[ck >> bs_shift];
    return cache + head_off + blk * blk_stride + (ck & bs_mask) * D;
  };
  // K fp8 image: [PD_KT][D] bytes, 16B-granule XOR swizzle (col16 ^ key&7)
  // (both issue all source addresses first, then the DMAs back to back:
  // see the bf16 pipe kernel)
  auto issue_k = [&](int base, short* dst) {
    const __hip_fp8_e4m3* src[NI_K];
#pragma unroll
    for (int j = 0; j < NI_K; ++j) {
      const int g = (wid * NI_K + j) * 64 + lane;  // 16B granule
      const int key = g / G16B;
      const int c16 = g % G16B;
      const int src_col = swz_gran(key, c16, G16B) << 4;
      src[j] = kv_row(base + key, k_cache) + src_col;
    }
#pragma unroll
    for (int j = 0; j < NI_K; ++j) {
      const int off = __builtin_amdgcn_readfirstlane((wid * NI_K + j) * 512);
      glds16<KV_NT>(src[j], reinterpret_cast<char*>(dst) + off * 2);
    }
  };
  // V raw fp8, linear [PD_KT][D] bytes into the back half of `dst`
  auto issue_v_raw = [&](int base, short* dst) {
    char* const back = reinterpret_cast<char*>(dst) + RAW_BYTES;
    const __hip_fp8_e4m3* src[NI_VR];
#pragma unroll
    for (int j = 0; j < NI_VR; ++j) {
      const int g = (wid * NI_VR + j) * 64 + lane;
      const int key = g / G16B;
      const int colb = (g % G16B) * 16;
      src[j] = kv_row(base + key, v_cache) + colb;
    }
#pragma unroll
    for (int j = 0; j < NI_VR; ++j) {
      const int off = __builtin_amdgcn_readfirstlane((wid * NI_VR + j) * 1024);
      glds16<KV_NT>(src[j], back + off);
    }
  };

  pipe_barrier();  // bt_l ready
  if (range_lo < range_hi) issue_k(range_lo, img0);

  int cur = 0;
  for (int base = range_lo; base < range_hi; base += PD_KT, cur ^= 1) {
    short* const X = cur ? img1 : img0;
    short* const Y = cur ? img0 : img1;
    pipe_barrier_vm<0>();  // K(base) landed in X front

    // ---- S from fp8 K (convert per fragment with packed cvt VOPs)
    float sv[NREG];
    if (s_wave) {
      f32x4_t s = {0.f, 0.f, 0.f, 0.f};
      const int key = slab * 16 + col;
      const char* krow = reinterpret_cast<const char*>(X) + key * D;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int d8 = ks * 32 + kgrp * 8;
        const int lds_col = swz_gran(key, d8 >> 4, G16B) * 16 + (d8 & 15);
        const uint2 raw = *reinterpret_cast<const uint2*>(krow + lds_col);
        const bf16x8_t bfrag = fp8x8_to_bf16(raw.x, raw.y);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[ks], bfrag, s, 0, 0, 0);
      }
      float mx[NREG];
      pd_scale_mask_rowmax<NREG>(s, base + key, L, start, scale, softcap, sv, mx);
      if (col == 0 && wid < SLABS) {
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg) mpart[slab * 16 + kgrp * 4 + reg] = mx[reg];
      }
    }
    pipe_barrier();  // S reads of X-front done; mparts visible

    // ---- issue V(base) raw -> Y back, K(next) -> Y front. (Issuing V at
    // the loop TOP — its buffer is already free there — measured 0.390 vs
    // 0.373 ms: no win, the post-S window already covers the V stream.)
    const int next = base + PD_KT;
    const bool prefetch = next < range_hi;
    issue_v_raw(base, Y);
    if (prefetch) issue_k(next, Y);

    // ---- softmax combine + P (one wave per slab)
    bool rescale = true;
    if (s_wave)
      rescale = pd_softmax_tile<SLABS, PD_KT, NREG>(
          mpart, alpha_s, p_lds2, slab, wid, col, kgrp, sv, m_regs, l_regs);
    if (prefetch) {
      pipe_barrier_vm<NI_K>();  // V raw landed; K(next) stays in flight
    } else {
      pipe_barrier_vm<0>();
    }

    // ---- convert pass: Y back (raw fp8) -> X bf16 tr16 image
    {
      const char* const raw = reinterpret_cast<const char*>(Y) + RAW_BYTES;
      constexpr int CPK = D / 8;          // 8-elem granules per key row
      constexpr int NG = PD_KT * CPK;     // 512 at D=256
#pragma unroll
      for (int j = 0; j < NG / NT; ++j) {
        const int c = tid + j * NT;
        const int key = c / CPK;
        const int d8 = (c % CPK) * 8;
        const uint2 rr = *reinterpret_cast<const uint2*>(raw + key * D + d8);
        *reinterpret_cast<bf16x8_t*>(&X[v_img_index<D>(key, d8)]) =
            fp8x8_to_bf16(rr.x, rr.y);
      }
    }
    pipe_barrier();  // image + P + alpha visible

    // ---- PV from the bf16 tr16 image
    attn_pv_tile<D, PD_KT, DT>(X, p_lds2, alpha_s, rescale, ot, wid * DT, lane);
    // next loop-top barrier (vm0) protects X/Y rotation
  }

  // ---- merge per-slab l, then store (normalised out, or raw partials)
  if (col == 0 && wid < SLABS) {
#pragma unroll
    for (int reg = 0; reg < NREG; ++reg) l_part[slab * 16 + kgrp * 4 + reg] = l_regs[reg];
  }
  pipe_barrier();
  pd_store<D, SLABS, DT, NREG>(out, scratch, l_part, ot, m_regs, b, kh, G,
                               num_kv_heads, out_stride, wid, col, kgrp);
}

// Combine split-KV partials: out[b, kh*G+g] = Σ_s w_s·acc_s / Σ_s w_s·l_s,
// w_s = exp(m_s − max_s m). One wave per (b, kh, g).
template <int HEAD_DIM>
__global__ __launch_bounds__(64) void decode_splitkv_merge_kernel(
    __hip_bfloat16* __restrict__ out, const float* __restrict__ scratch,
    int num_kv_heads, int G, int nsplit, long out_stride) {
  constexpr int D = HEAD_DIM;
  constexpr int DPL = D / WAVE;  // dims per lane (2 or 4)
  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int g = blockIdx.z;
  const int lane = threadIdx.x;
  const float* base = scratch +
      ((((long)b * num_kv_heads + kh) * nsplit) * G + g) * (D + 2);
  const long sstride = (long)G * (D + 2);
  float m_max = -1e30f;
  for (int s2 = 0; s2 < nsplit; ++s2) m_max = fmaxf(m_max, base[s2 * sstride + D]);
  float acc[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
  float l = 0.f;
  for (int s2 = 0; s2 < nsplit; ++s2) {
    const float* row = base + s2 * sstride;
    const float w = __expf(row[D] - m_max);
    if (w > 0.f) {
      l += w * row[D + 1];
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
