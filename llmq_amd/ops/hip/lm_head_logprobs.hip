// Prompt logprobs: lm_head GEMM fused with log-sum-exp and the target pick.
//
//   lp[r] = l[r, targets[r]] - logsumexp_j l[r, j],
//   l[r, j] = softcap(bf16(hidden[rows[r]] . w[j]))
//
// i.e. torch_ref.token_logprobs of the logits "as the lm_head stored them"
// (fp32 accumulator rounded to bf16, widened, soft-capped), without ever
// storing a logit: at Gemma-2's vocabulary an 8192-row prefill segment would
// be a 4.2 GB [R, V] matrix.
//
// Main loop = skinny_gemm_kernel's (256x256x64 tile, 8 waves as 2 (M) x 4
// (N), glds staging with the source-side st_16x32 swizzle, counted-vmcnt
// double buffer); this file is compiled after skinny_gemm.hip and
// sampling.hip in ops.hip and uses their skg_* helpers and logit_value.
//
// Work split: grid (ceil(R/256), NSPLIT). A workgroup owns one 256-row M tile
// and walks the vocabulary tiles slice, slice + NSPLIT, ... The walk is ONE
// flat pipeline over (tile, k-step): the last k-step of a tile prefetches the
// first k-step of the next tile, so the buffer parity simply continues (an
// odd K/64 needs no special case) and the pipeline never drains between
// tiles. Rows are gathered at staging time: the A-tile source row is
// rows[min(r, R-1)], read once per thread (a thread stages the same four
// tile rows at every step).
//
// Epilogue per vocabulary tile, registers only: round/widen/cap each
// accumulator, -inf past V, fold the lane's 4 columns of a row into that
// row's lane-local running (max, sum). 32 rows per lane -> 64 state
// registers next to the 128 accumulators (2 waves/SIMD: 256 are available).
// The lane holding column targets[r] drops that value into LDS. After the
// walk the (max, sum) pairs fold across the 16 column lanes by shuffles and
// across the 4 N-waves through LDS; one pair per row goes to the
// [NSPLIT, R] workspace, the target value to tgt[R] from the one workgroup
// whose walk contains the target's tile. lm_head_logprobs_merge_kernel folds
// the slices. No atomics: the result does not depend on scheduling.

#include "common.h"
#include "attention_common.h"

#define LHL_NEG_INF (-__builtin_inff())

// (m, s) <- (m, s) (+) (om, os) for running max / scaled sum pairs. An empty
// side is (-inf, 0): the reference max is then moved to 0 so that no
// exp(-inf - -inf) is formed.
DEVINL void lhl_fold(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  const float ref = nm == LHL_NEG_INF ? 0.f : nm;
  s = s * __expf(m - ref) + os * __expf(om - ref);
  m = nm;
}

// skg_stage for the gathered A tile: the thread's four source rows come in
// as srow[] (already clamped to the tensor).
DEVINL void lhl_stage_rows(const __hip_bfloat16* __restrict__ src,
                           long src_stride, const int (&srow)[4], int k0,
                           short* dst, int wid, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wid * 4 + j) * 8 + (lane >> 3);
    const int col = (lane & 7) * 8;
    const int scol = k0 + skg_swz(row, col);
    const int off = __builtin_amdgcn_readfirstlane((wid * 4 + j) * 512);
    glds16(src + (long)srow[j] * src_stride + scol, dst + off);
  }
}

__global__ __launch_bounds__(SKG_NT, 2) void lm_head_logprobs_kernel(
    float* __restrict__ ws_m,               // [NSPLIT, R] slice row max
    float* __restrict__ ws_s,               // [NSPLIT, R] slice row sum
    float* __restrict__ tgt,                // [R] target logit (capped)
    const __hip_bfloat16* __restrict__ hidden,  // [T, K]
    const __hip_bfloat16* __restrict__ w,       // [V, K]
    const int* __restrict__ rows,           // [R] rows of hidden
    const int* __restrict__ targets,        // [R] token ids
    int R, int T, int V, int K, long h_stride, long w_stride, float softcap,
    float inv_cap) {
  const int mtile = blockIdx.x;
  const int slice = blockIdx.y;
  const int nsplit = gridDim.y;
  const int ksteps = K / SKG_BK;
  const int ntiles = (V + SKG_BN - 1) / SKG_BN;
  const int my_tiles =
      slice < ntiles ? (ntiles - slice + nsplit - 1) / nsplit : 0;
  const int nsteps = my_tiles * ksteps;

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int wm = wid >> 2;       // 0..1  (M half)
  const int wn = wid & 3;        // 0..3  (N quarter: 64 cols)
  const int col16 = lane & 15;
  const int kgrp = lane >> 4;
  const int row_a0 = mtile * SKG_BM;

  if (nsteps == 0) {  // more slices than tiles: an empty walk
    const int r = row_a0 + tid;
    if (tid < SKG_BM && r < R) {
      ws_m[(long)slice * R + r] = LHL_NEG_INF;
      ws_s[(long)slice * R + r] = 0.f;
    }
    return;
  }

  __shared__ __attribute__((aligned(16))) short smem[4 * SKG_TILE_ELEMS];
  __shared__ __attribute__((aligned(16))) int s_tcol[SKG_BM];
  __shared__ float s_tval[SKG_BM];
  __shared__ float s_m[4][SKG_BM];
  __shared__ float s_s[4][SKG_BM];
  short* const a0 = smem;
  short* const b0 = smem + SKG_TILE_ELEMS;
  short* const a1 = smem + 2 * SKG_TILE_ELEMS;
  short* const b1 = smem + 3 * SKG_TILE_ELEMS;

  // target column per tile row (published by the first pipeline barrier)
  if (tid < SKG_BM) {
    const int r = row_a0 + tid;
    s_tcol[tid] = r < R ? targets[r] : -1;
    s_tval[tid] = 0.f;
  }
  // the four hidden rows this thread stages, at every step
  int srow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wid * 4 + j) * 8 + (lane >> 3);
    srow[j] = min(max(rows[min(row_a0 + row, R - 1)], 0), T - 1);
  }

  skg_f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  // running (max, sum) of row wm*128 + mf*16 + kgrp*4 + reg over this
  // lane's columns, index mf*4 + reg
  float rm[32], rs[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) { rm[i] = LHL_NEG_INF; rs[i] = 0.f; }

  lhl_stage_rows(hidden, h_stride, srow, 0, a0, wid, lane);
  skg_stage(w, w_stride, slice * SKG_BN, V, 0, b0, wid, lane);

  int tile = slice;
  int ks = 0;
  for (int i = 0; i < nsteps; ++i) {
    short* const a = i & 1 ? a1 : a0;
    short* const b = i & 1 ? b1 : b0;
    short* const an = i & 1 ? a0 : a1;
    short* const bn = i & 1 ? b0 : b1;
    const bool tile_done = ks + 1 == ksteps;
    // current step landed; every wave is past its reads of the other buffer
    pipe_barrier_vm<0>();
    if (i + 1 < nsteps) {  // next k-step, or the next tile's first one
      const int nk0 = tile_done ? 0 : (ks + 1) * SKG_BK;
      const int ntile = tile_done ? tile + nsplit : tile;
      lhl_stage_rows(hidden, h_stride, srow, nk0, an, wid, lane);
      skg_stage(w, w_stride, ntile * SKG_BN, V, nk0, bn, wid, lane);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      skg_bf16x8 bf[4];
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const int brow = wn * 64 + nf * 16 + col16;
        const int bcol = kk * 32 + kgrp * 8;
        bf[nf] = *reinterpret_cast<const skg_bf16x8*>(
            &b[brow * SKG_BK + skg_swz(brow, bcol)]);
      }
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) {
        const int arow = wm * 128 + mf * 16 + col16;
        const int acol = kk * 32 + kgrp * 8;
        const skg_bf16x8 af = *reinterpret_cast<const skg_bf16x8*>(
            &a[arow * SKG_BK + skg_swz(arow, acol)]);
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af, bf[nf], acc[mf][nf], 0, 0, 0);
        }
      }
    }
    if (!tile_done) {
      ++ks;
      continue;
    }
    // ---- tile epilogue: C fragment (row = kgrp*4+reg, col = col16). The
    // next step's glds are in flight meanwhile; nothing here touches the
    // staging buffers or global memory.
    const int col0 = tile * SKG_BN + wn * 64 + col16;
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) {
      const int lrow0 = wm * 128 + mf * 16 + kgrp * 4;
      const int4 tc = *reinterpret_cast<const int4*>(&s_tcol[lrow0]);
      const int tcs[4] = {tc.x, tc.y, tc.z, tc.w};
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float v[4];
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
          const int gn = col0 + nf * 16;
          const float l = logit_value(__float2bfloat16(acc[mf][nf][reg]),
                                      softcap, inv_cap);
          v[nf] = gn < V ? l : LHL_NEG_INF;
          if (gn == tcs[reg]) s_tval[lrow0 + reg] = v[nf];
          acc[mf][nf][reg] = 0.f;
        }
        const int idx = mf * 4 + reg;
        const float nm =
            fmaxf(rm[idx], fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
        const float ref = nm == LHL_NEG_INF ? 0.f : nm;
        rs[idx] = rs[idx] * __expf(rm[idx] - ref) +
                  ((__expf(v[0] - ref) + __expf(v[1] - ref)) +
                   (__expf(v[2] - ref) + __expf(v[3] - ref)));
        rm[idx] = nm;
      }
    }
    ks = 0;
    tile += nsplit;
  }

  // ---- fold the 16 column lanes, then the 4 N-waves
#pragma unroll
  for (int idx = 0; idx < 32; ++idx) {
    float m = rm[idx], s = rs[idx];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
      lhl_fold(m, s, __shfl_xor(m, off, WAVE), __shfl_xor(s, off, WAVE));
    if (col16 == 0) {
      const int lrow = wm * 128 + (idx >> 2) * 16 + kgrp * 4 + (idx & 3);
      s_m[wn][lrow] = m;
      s_s[wn][lrow] = s;
    }
  }
  __syncthreads();
  const int r = row_a0 + tid;
  if (tid < SKG_BM && r < R) {
    float m = s_m[0][tid], s = s_s[0][tid];
#pragma unroll
    for (int q = 1; q < 4; ++q) lhl_fold(m, s, s_m[q][tid], s_s[q][tid]);
    ws_m[(long)slice * R + r] = m;
    ws_s[(long)slice * R + r] = s;
    // The walk that holds the target's tile wrote s_tval; a target outside
    // [0, V) belongs to nobody and slice 0 marks the row NaN.
    const int tcol = s_tcol[tid];
    const bool valid = tcol >= 0 && tcol < V;
    if (valid ? (tcol / SKG_BN) % nsplit == slice : slice == 0)
      tgt[r] = valid ? s_tval[tid] : __builtin_nanf("");
  }
}

// lp[r] = tgt[r] - logsumexp over the slices' (max, sum) pairs.
__global__ __launch_bounds__(256) void lm_head_logprobs_merge_kernel(
    float* __restrict__ lp, const float* __restrict__ ws_m,
    const float* __restrict__ ws_s, const float* __restrict__ tgt, int nsplit,
    int R) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float M = LHL_NEG_INF;
  for (int i = 0; i < nsplit; ++i) M = fmaxf(M, ws_m[(long)i * R + r]);
  float s = 0.f;  // empty slices: 0 * exp(-inf - M) = 0 (slice 0 is never empty)
  for (int i = 0; i < nsplit; ++i)
    s += ws_s[(long)i * R + r] * expf(ws_m[(long)i * R + r] - M);
  lp[r] = tgt[r] - (M + logf(s));
}
