// W4A8 GEMM on the CDNA4 block-scaled matrix core:
//   out[T,N] bf16 = (A_fp8[T,K] . dequant(W_mxfp4)[N,K]^T) * a_scale[t] + bias[n]
//
// One v_mfma_scale_f32_16x16x128_f8f6f4 multiplies a 16x128 e4m3 fragment by
// a 128x16 e2m1 fragment and applies an e8m0 scale per 32 K-elements of each
// operand inside the instruction. Operand layout (lane = 16 * kgrp + r):
//   A (src0, cbsz 0, 8 VGPRs): row r of the fragment, one byte per element;
//       VGPRs 0-3 hold K = 16*kgrp .. +15 and VGPRs 4-7 K = 64 + 16*kgrp ..
//       +15 (read off the hardware with identity operands: an 8-bit operand
//       is two 64-wide halves, NOT 32 consecutive K per lane);
//   B (src1, blgp 4, 4 VGPRs): column r, K = 32*kgrp .. +31, two elements per
//       byte, the even one in the low nibble;
//   scale (one VGPR per operand): the byte selected by op_sel scales exactly
//       the 32 B elements that lane holds, so an MX block == a lane's B
//       fragment (A's scale blocks are not MX blocks; they are all 2^0);
//   C/D (4 VGPRs): row 4*kgrp + reg, column r.
// A's block scales are the constant 127 (2^0): the per-row fp32 a_scale and
// the bias are applied in the epilogue (or in the split-K reduce).
//
// B never touches LDS. Weights are static, so mxfp4_pack_weight reorders
// them once into fragment order: codes [N/16][K/128][64 lanes][16 B], so a
// wave's B fragment of one (16-row group, K step) is 1 KB contiguous and
// each lane takes it with one 16-byte load straight into the MFMA operand
// registers; scales [N/16][ceil(K/512)][64 lanes][4 B], byte j of a lane's
// dword being its block scale at K step 4*q + j, picked by op_sel: one dword
// load per 4 K steps. Both are double-buffered in registers one step ahead.
//
// A goes through LDS: [BM][128 B] per stage, two stages, staged by
// global_load_lds in 16-byte granules (lane-linear destination) with the
// swizzle carried by the source address. A lane reads its fragment as two
// ds_read_b128 (granules kgrp and 4 + kgrp) at row r of its 16-row group; rows are 128 B apart, so
// without a swizzle rows r and r+2 of a group meet in the same banks. The
// physical granule is g ^ ((row >> 1) & 7): the 16 rows of a group then
// cover 16 distinct (row parity, granule) positions, 256 B, conflict-free.
//
// Tiles (one template): 256x128 with 8 waves as 4 (M) x 2 (N), each wave
// 64x64 = 4x4 fragments, for prefill and large decode batches; 32x64 with 4
// waves side by side along N, each 32x16, for small batches where the kernel
// is a weight stream (B loads `nt` there: each byte is read once) and more
// workgroups along N matter more than reuse. Split-K over fp32 slabs
// [Z, M, N] with a reduce kernel that applies a_scale and the bias, when the
// grid would leave most CUs idle.
//
// Edges: M tails clamp the SOURCE row and N tails clamp the 16-row weight
// group (finite real data); out-of-range outputs are not stored.

#include "common.h"
#include "attention_common.h"

typedef __attribute__((ext_vector_type(8))) int mx4_i32x8;
typedef __attribute__((ext_vector_type(4))) int mx4_i32x4;
typedef __attribute__((ext_vector_type(4))) float mx4_f32x4;

#define MX4_BK 128            // K elements per step = one MFMA
#define MX4_A_SCALES 0x7f7f7f7f  // e8m0 127 = 2^0 in every byte
// fp32 epilogue math stays scalar: no packed-fp32 VALU ops in these kernels
#if defined(__HIP_DEVICE_COMPILE__)
#define MX4_NOPK __attribute__((target("no-packed-fp32-ops")))
#else
#define MX4_NOPK
#endif

DEVINL int mx4_swz(int row, int granule) { return granule ^ ((row >> 1) & 7); }

// Stage one [BM][128] fp8 A tile: BM * 8 granules of 16 B, BM * 8 / NT glds
// per lane, each wave instruction filling 1 KB of LDS lane-linearly.
template <int BM, int NT>
DEVINL void mx4_stage_a(const unsigned char* __restrict__ a, long lda, int row0,
                        int M, int k0, char* dst, int wid, int lane) {
  constexpr int NA = BM * 8 / NT;
  static_assert(NA >= 1 && NA * NT == BM * 8, "tile must fill whole glds waves");
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int g = (wid * NA + j) * 64 + lane;
    const int row = g >> 3;
    const int srow = min(row0 + row, M - 1);
    const int off = __builtin_amdgcn_readfirstlane((wid * NA + j) * 1024);
    glds16(a + (long)srow * lda + k0 + mx4_swz(row, g & 7) * 16, dst + off);
  }
}

// A wave's B fragments of K step ks: one 16-byte load per lane and 16-row
// group, 1 KB contiguous per group (`nt` where each byte is read once).
template <int NF, bool NT_B>
DEVINL void mx4_load_b(const unsigned char* const (&bq)[NF], int ks,
                       mx4_i32x4 (&bv)[NF]) {
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const mx4_i32x4* p =
        reinterpret_cast<const mx4_i32x4*>(bq[nf] + (long)ks * (WAVE * 16));
    bv[nf] = NT_B ? __builtin_nontemporal_load(p) : *p;
  }
}

// The scale dwords that cover K steps 4 * (ks / 4) .. + 3.
template <int NF>
DEVINL void mx4_load_s(const unsigned char* const (&bs)[NF], int ks,
                       int (&sv)[NF]) {
#pragma unroll
  for (int nf = 0; nf < NF; ++nf)
    sv[nf] = *reinterpret_cast<const int*>(bs[nf] + (long)(ks >> 2) * (WAVE * 4));
}

// One K step of a wave: MF x NF scaled MFMAs; SEL = which byte of the scale
// dwords belongs to this step.
template <int SEL, int MF, int NF>
DEVINL void mx4_mma(mx4_f32x4 (&acc)[MF][NF], const char* a_lds, int arow0,
                    int col16, int kgrp, const mx4_i32x4 (&b)[NF],
                    const int (&sc)[NF]) {
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int row = arow0 + mf * 16 + col16;
    const char* rp = a_lds + row * MX4_BK;
    const mx4_i32x4 lo =
        *reinterpret_cast<const mx4_i32x4*>(rp + mx4_swz(row, kgrp) * 16);
    const mx4_i32x4 hi =
        *reinterpret_cast<const mx4_i32x4*>(rp + mx4_swz(row, 4 + kgrp) * 16);
    const mx4_i32x8 af = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const mx4_i32x8 bf = {b[nf].x, b[nf].y, b[nf].z, b[nf].w, 0, 0, 0, 0};
      acc[mf][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          af, bf, acc[mf][nf], /*cbsz: A e4m3*/ 0, /*blgp: B e2m1*/ 4,
          0, MX4_A_SCALES, SEL, sc[nf]);
    }
  }
}

template <int BM, int BN, int WM, int WN, bool SPLIT, bool NT_B>
__global__ __launch_bounds__(WM * WN * WAVE) MX4_NOPK void mxfp4_gemm_kernel(
    void* __restrict__ out_raw,                 // bf16 [M,N] or f32 [Z,M,N]
    const unsigned char* __restrict__ a,        // e4m3 [M,K], row pitch lda
    const float* __restrict__ a_scale,          // [M]
    const unsigned char* __restrict__ wq,       // packed codes
    const unsigned char* __restrict__ ws,       // packed scales
    const __hip_bfloat16* __restrict__ bias,    // [N] or null
    int M, int N, int K, long lda) {
  constexpr int NT = WM * WN * WAVE;
  constexpr int MF = BM / (WM * 16);
  constexpr int NF = BN / (WN * 16);
  static_assert(MF * WM * 16 == BM && NF * WN * 16 == BN, "tile / wave split");

  const int mtile = blockIdx.x;
  const int ntile = blockIdx.y;
  const int kslice = blockIdx.z;
  const int ksteps = K / MX4_BK;
  const int per = (ksteps + (int)gridDim.z - 1) / (int)gridDim.z;
  const int ks0 = kslice * per;
  const int ks1 = min(ksteps, ks0 + per);
  if (ks0 >= ks1) return;  // the launcher drops empty slices; guard anyway

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int wm = wid / WN;
  const int wn = wid % WN;
  const int col16 = lane & 15;
  const int kgrp = lane >> 4;

  __shared__ __attribute__((aligned(16))) char smem[2 * BM * MX4_BK];

  // this wave's B fragments: 16-row weight groups, clamped at the N tail
  const int ngroups = N / 16;
  const int qsteps = (ksteps + 3) / 4;
  const int ng0 = ntile * (BN / 16) + wn * NF;
  const unsigned char* bq[NF];
  const unsigned char* bs[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const long ng = min(ng0 + nf, ngroups - 1);
    bq[nf] = wq + (ng * ksteps * WAVE + lane) * 16;
    bs[nf] = ws + (ng * qsteps * WAVE + lane) * 4;
  }
  mx4_f32x4 acc[MF][NF];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int row_a0 = mtile * BM;
  const int arow0 = wm * MF * 16;
  mx4_i32x4 bcur[NF], bnext[NF];
  int scur[NF], snext[NF];

  // prologue: K step ks0 into stage 0 and the current registers
  mx4_stage_a<BM, NT>(a, lda, row_a0, M, ks0 * MX4_BK, smem, wid, lane);
  mx4_load_b<NF, NT_B>(bq, ks0, bcur);
  mx4_load_s<NF>(bs, ks0, scur);

  for (int ks = ks0; ks < ks1; ++ks) {
    char* const cur = smem + ((ks - ks0) & 1) * (BM * MX4_BK);
    char* const nxt = smem + (((ks - ks0) & 1) ^ 1) * (BM * MX4_BK);
    // this step's A tile landed, and every wave is done reading the other
    // stage (its ds_reads were consumed by the previous step's MFMAs)
    pipe_barrier_vm<0>();
    if (ks + 1 < ks1) {  // next step: in flight through the MFMA phase
      mx4_stage_a<BM, NT>(a, lda, row_a0, M, (ks + 1) * MX4_BK, nxt, wid, lane);
      mx4_load_b<NF, NT_B>(bq, ks + 1, bnext);
      if (((ks + 1) & 3) == 0) {
        mx4_load_s<NF>(bs, ks + 1, snext);
      } else {
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) snext[nf] = scur[nf];
      }
    }
    switch (ks & 3) {
      case 0: mx4_mma<0, MF, NF>(acc, cur, arow0, col16, kgrp, bcur, scur); break;
      case 1: mx4_mma<1, MF, NF>(acc, cur, arow0, col16, kgrp, bcur, scur); break;
      case 2: mx4_mma<2, MF, NF>(acc, cur, arow0, col16, kgrp, bcur, scur); break;
      default: mx4_mma<3, MF, NF>(acc, cur, arow0, col16, kgrp, bcur, scur); break;
    }
    if (ks + 1 < ks1) {
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        bcur[nf] = bnext[nf];
        scur[nf] = snext[nf];
      }
    }
  }

  // ---- epilogue: C fragment (row = kgrp*4 + reg, col = col16)
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int gm_base = row_a0 + arow0 + mf * 16 + kgrp * 4;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      if (ng0 + nf >= ngroups) continue;
      const int gn = (ng0 + nf) * 16 + col16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gm = gm_base + reg;
        if (gm >= M) continue;
        if constexpr (!SPLIT) {
          float v = acc[mf][nf][reg] * a_scale[gm];
          if (bias != nullptr) v += __bfloat162float(bias[gn]);
          reinterpret_cast<__hip_bfloat16*>(out_raw)[(long)gm * N + gn] =
              __float2bfloat16(v);
        } else {
          reinterpret_cast<float*>(out_raw)[((long)kslice * M + gm) * N + gn] =
              acc[mf][nf][reg];
        }
      }
    }
  }
}

// Fold split-K fp32 slabs [Z,M,N], apply a_scale[m] and the bias -> bf16.
// N % 16 == 0, so a thread's 4 outputs share a row.
__global__ __launch_bounds__(256) MX4_NOPK void mxfp4_gemm_reduce_kernel(
    __hip_bfloat16* __restrict__ out, const float* __restrict__ slabs,
    const float* __restrict__ a_scale, const __hip_bfloat16* __restrict__ bias,
    int nsplit, long MN, int N) {
  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= MN) return;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsplit; ++s) {
    const float4 sl = *reinterpret_cast<const float4*>(&slabs[s * MN + i0]);
    v[0] += sl.x; v[1] += sl.y; v[2] += sl.z; v[3] += sl.w;
  }
  const float sa = a_scale[i0 / N];
  const int n0 = (int)(i0 % N);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float r = v[j] * sa;
    if (bias != nullptr) r += __bfloat162float(bias[n0 + j]);
    out[i0 + j] = __float2bfloat16(r);
  }
}
