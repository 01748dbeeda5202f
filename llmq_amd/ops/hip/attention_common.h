// Shared device helpers for the attention kernels (prefill + decode): MFMA
// fragment vector types, the K swizzle and its S slab, the V tr16 subtile
// image (index maps, A-fragment read, PV tile), the hidden-from-hipcc
// global->LDS DMA with its hand-counted barriers, and the packed fp8
// converter. Helpers are forced inline, take registers by reference and LDS
// as pointers into the CALLER's storage: none declares a __shared__ object
// (the pipe kernels rely on having exactly one).
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4v;
typedef __attribute__((address_space(3))) bf16x4v lds_bf16x4;

DEVINL int swz(int row, int d) {  // element-index XOR swizzle (16B granules)
  return d ^ ((row & 7) << 3);
}

// The same XOR on 16-byte granule indices, for rows of NGRAN granules (the
// fp8 K image: glds source column and S-phase LDS column).
DEVINL int swz_gran(int row, int c16, int ngran) {
  return (c16 ^ (row & 7)) & (ngran - 1);
}

// S[16q, 16 keys] = Q K^T for one key slab: this lane's key row `key` of the
// swizzled K tile `kbuf` ([keys][D] bf16), q fragments in registers
// (frag[ks] covers dims ks*32 + kgrp*8 .. +7).
template <int D>
DEVINL f32x4_t attn_s_slab(const bf16x8_t (&qfrag)[D / 32], const short* kbuf,
                           int key, int kgrp) {
  f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    const int d8 = ks * 32 + kgrp * 8;
    bf16x8_t bfrag =
        *reinterpret_cast<const bf16x8_t*>(&kbuf[key * D + swz(key, d8)]);
    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[ks], bfrag, s, 0, 0, 0);
  }
  return s;
}

// ---- V "tr16 subtile image" --
// V is staged NOT as K's swizzled rows but as 32-key × 16-dim subtiles,
// subtile st = (key/32) * (D/16) + dim/16, key quads permuted
// (0,2,4,6,1,3,5,7) inside a subtile, so one uniform-base ds_read_b64_tr_b16
// delivers each 16-lane group its MFMA A-fragment quad (guide T10: +11% on
// the PV path vs scalar ds_read_u16). Subtiles are strided by 528 elements
// (512 + 16): the unpadded 1 KB stride lands every subtile on the same banks
// (16-way staging-write conflicts).
constexpr int V_SUB_STRIDE = 528;

constexpr int v_img_nsub(int kt, int d) { return (kt / 32) * (d / 16); }
constexpr int v_img_elems(int kt, int d) { return v_img_nsub(kt, d) * V_SUB_STRIDE; }
// K and V share one tile buffer: max(K rows, padded V image), in elements.
constexpr int kv_tile_elems(int kt, int d) {
  return kt * d > v_img_elems(kt, d) ? kt * d : v_img_elems(kt, d);
}

// Forward map: 8-element granule (key, d8) of the tile -> image element index
// (plain staging and the fp8 convert pass write here).
template <int D>
constexpr int v_img_index(int key, int d8) {
  const int dtile = d8 / 16, col0 = d8 & 15;
  const int qq = (key & 31) >> 2;
  const int bpos = ((qq & 1) << 2) + (qq >> 1);
  return ((key >> 5) * (D / 16) + dtile) * V_SUB_STRIDE + bpos * 64 +
         (key & 3) * 16 + col0;
}

// Inverse map: glds writes lane-linear, so lane `lane` of the DMA that fills
// subtile st (elements st*V_SUB_STRIDE + lane*8 .. +7) must SOURCE this
// (key, dim). Subtiles st..st+n of one 32-key group share `key` and step
// `dim` by 16.
struct VImgSrc { int key, dim; };
template <int D>
constexpr VImgSrc v_img_source(int st, int lane) {
  const int ks = st / (D / 16), dtile = st % (D / 16);
  const int pos = lane * 8;
  const int bpos = pos / 64, rem = pos % 64;
  const int qq = ((bpos >> 2) & 1) | ((bpos & 3) << 1);
  return {ks * 32 + qq * 4 + rem / 16, dtile * 16 + (rem & 15)};
}

// Compile-time proof that the two maps are inverses and that the DMA covers
// every granule of the tile exactly once.
template <int KT, int D>
constexpr bool v_img_maps_agree() {
  bool seen[KT * D / 8] = {};
  for (int st = 0; st < v_img_nsub(KT, D); ++st) {
    for (int lane = 0; lane < WAVE; ++lane) {
      const VImgSrc s = v_img_source<D>(st, lane);
      if (s.key < 0 || s.key >= KT || s.dim < 0 || s.dim >= D || s.dim % 8) return false;
      if (v_img_index<D>(s.key, s.dim) != st * V_SUB_STRIDE + lane * 8) return false;
      bool& hit = seen[s.key * (D / 8) + s.dim / 8];
      if (hit) return false;
      hit = true;
      // consecutive dim tiles of one key group: same key, dim + 16
      if ((st + 1) % (D / 16) != 0) {
        const VImgSrc n = v_img_source<D>(st + 1, lane);
        if (n.key != s.key || n.dim != s.dim + 16) return false;
      }
    }
  }
  for (bool hit : seen)
    if (!hit) return false;
  return true;
}
static_assert(v_img_maps_agree<64, 64>() && v_img_maps_agree<128, 64>() &&
              v_img_maps_agree<64, 128>() && v_img_maps_agree<128, 128>() &&
              v_img_maps_agree<64, 256>() && v_img_maps_agree<128, 256>(),
              "V tr16 image: forward and inverse index maps disagree");

// PV A-fragment (8 keys × this lane's dim) of subtile `sub`: two transpose
// reads — each lane reads 4 contiguous bf16 at its own 8-byte slot and the
// hardware redistributes so lane l receives column (l&15) of its 16-lane
// group's [4-key][16-dim] block.
DEVINL bf16x8_t v_img_afrag(const short* img, int sub, int lane) {
  const int e = sub * V_SUB_STRIDE + lane * 4;
  bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&img[e]);
  bf16x4v hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&img[e + 4 * 64]);
  bf16x8_t a;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = __bfloat16_as_short((__hip_bfloat16)lo[j]);
    a[4 + j] = __bfloat16_as_short((__hip_bfloat16)hi[j]);
  }
  return a;
}

// OT[dims, 16q] = alpha * OT + V^T P^T over the DT 16-dim tiles from dim tile
// `dtile0`: V from the tr16 image `img` (KT keys), P^T as b128 reads of the
// [16 q][KT] bf16 tile `p_tile`, alpha per q row (= lane&15) from `alpha_s`.
// rescale == false (defer-max build only) skips the alpha pass.
template <int D, int KT, int DT>
DEVINL void attn_pv_tile(const short* img, const short* p_tile,
                         const float* alpha_s, bool rescale, f32x4_t (&ot)[DT],
                         int dtile0, int lane) {
  const int col = lane & 15, kgrp = lane >> 4;
  const float alpha_q = rescale ? alpha_s[col] : 1.f;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    if (rescale) {
      ot[dt][0] *= alpha_q; ot[dt][1] *= alpha_q;
      ot[dt][2] *= alpha_q; ot[dt][3] *= alpha_q;
    }
#pragma unroll
    for (int ks = 0; ks < KT / 32; ++ks) {
      const bf16x8_t a = v_img_afrag(img, ks * (D / 16) + dtile0 + dt, lane);
      const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(
          &p_tile[col * KT + ks * 32 + kgrp * 8]);
      ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, ot[dt], 0, 0, 0);
    }
  }
}

// 16-B-per-lane global→LDS DMA, HIDDEN from hipcc in inline asm: with the
// builtin form the compiler conservatively re-inserts `s_waitcnt vmcnt(0)`
// before the first ds_read that may alias the DMA destination (verified in
// the .s: it landed ahead of the PV tr16 reads, draining the K prefetch
// every chunk). Hand-counted vmcnt in pipe_barrier_vm is the only wait
// discipline for these, per guide §5.7 (its LDS-DMA recipe: M0 carries the
// wave-uniform LDS byte address, saved/written/restored in ONE statement;
// the s_nop is the SALU-write→M0-read wait state).
//
// NT selects the cache policy of the load, one asm statement per policy:
// false = default (the line allocates in L2 and the Infinity Cache: tiles
// that other workgroups re-read, i.e. prefill K/V and GEMM operands), true =
// `nt` (non-temporal: a once-read stream, i.e. the decode K/V cache, does not
// evict what the neighbouring kernels re-read). The policy cannot change a
// loaded value.
template <bool NT = false>
DEVINL void glds16(const void* src, void* lds_dst_uniform) {
  unsigned lds_off = (unsigned)(unsigned long)(
      (__attribute__((address_space(3))) char*)lds_dst_uniform);
  lds_off = __builtin_amdgcn_readfirstlane(lds_off);
  unsigned keep;
  if constexpr (NT) {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off nt\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(lds_off)
        : "memory");
  } else {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(lds_off)
        : "memory");
  }
}

DEVINL void pipe_barrier() {  // lgkm drain + raw barrier (glds may span)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int N>
DEVINL void pipe_barrier_vm() {  // + counted vmcnt: N glds may stay in flight
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "i"(N) : "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

DEVINL void reg_fence(bf16x8_t& v) {  // force materialisation (wait) HERE
  asm volatile("" : "+v"(v));
}

// 8 packed OCP e4m3 bytes -> bf16x8. gfx950 native packed converts:
// v_cvt_pk_f32_fp8 turns two fp8 (low/high half of a 16-bit pair) into two
// f32 in one VOP. The generic static_cast<float>(__hip_fp8_e4m3) lowers to a
// multi-op bit sequence per ELEMENT and made fp8 staging VALU-bound (fp8
// decode measured SLOWER than bf16 at batch 512 before this).
DEVINL bf16x8_t fp8x8_to_bf16(unsigned lo, unsigned hi) {
  typedef __attribute__((ext_vector_type(2))) float cvt_f32x2;
  bf16x8_t out;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int w = h ? (int)hi : (int)lo;
    const cvt_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
    const cvt_f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
    out[h * 4 + 0] = __bfloat16_as_short(__float2bfloat16(a[0]));
    out[h * 4 + 1] = __bfloat16_as_short(__float2bfloat16(a[1]));
    out[h * 4 + 2] = __bfloat16_as_short(__float2bfloat16(b[0]));
    out[h * 4 + 3] = __bfloat16_as_short(__float2bfloat16(b[1]));
  }
  return out;
}
