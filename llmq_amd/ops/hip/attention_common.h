// Shared device helpers for the attention kernels (prefill + decode): MFMA
// fragment vector types, the K swizzle and its S slab, the V tr16 subtile
// image (index maps, A-fragment read, PV tile) and the bf16 pipe decode
// kernel's V line image (the same, cut along cache lines), the hidden-from-hipcc
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

// ---- V "line image" (bf16 pipe decode kernel only) --
// The subtile image above makes one V DMA take 32 bytes from each of 32 cache
// rows: every 128-byte line is requested by four instructions, so V cannot
// stream `nt`. ds_read_b64_tr_b16 takes per-lane addresses, so the image can
// be cut along cache lines instead: a PIECE is 8 keys × 64 dims = eight whole
// 128-byte lines, filled by ONE lane-linear 1 KiB DMA. Piece p = (key octet
// o) * (D/64) + dim/64 sits at element p * 512, unpadded (the image is
// exactly the K tile's size). Inside a piece, lane = 16-byte slot, with
// kk = key & 7 and gg = (dim & 63) / 8, in one of two orders:
//   1: slot = gg * 8 + (kk ^ ((o & 1) << 2))
//   2: slot = kk * 8 + (gg ^ (2 * ((kk >> 1) & 1)) ^ (4 * (o & 1)))
// Both make every PV A-fragment read conflict-free under the tr16 bank model
// (two groups of 32 lanes, bank = (byte address / 4) mod 64): the 32 lanes of
// a group read four keys of each of two octets o, o+1, two granules and two
// halves each, and the XORs spread them over 32 distinct 8-byte bank pairs.
// In order 1 adjacent lanes read different rows, in order 2 one line.
// D = 256 uses order 2: it measured faster than order 1 wherever the two
// differ (ragged batch, split-KV, 128-key chunks) and needs fewer VGPRs
// there (order 1 spills at NREG = 4). D = 128 uses order 1: order 2 costs
// the NREG = 4 instantiation a wave of occupancy (98 VGPRs against 94) and
// measured 3.5 % slower there with K-only `nt`.
// profiles/decode_v_lines.md has both.
constexpr int v_line_order(int d) { return d >= 256 ? 2 : 1; }
constexpr int V_PIECE_ELEMS = 512;

constexpr int v_line_npiece(int kt, int d) { return (kt / 8) * (d / 64); }
constexpr int v_line_elems(int kt, int d) { return v_line_npiece(kt, d) * V_PIECE_ELEMS; }

template <int D>
constexpr int v_line_slot(int o, int kk, int gg) {
  if (v_line_order(D) == 1) return gg * 8 + (kk ^ ((o & 1) << 2));
  return kk * 8 + (gg ^ (2 * ((kk >> 1) & 1)) ^ (4 * (o & 1)));
}

// Forward map: element (key, d) of the tile, d a multiple of 4 -> image
// element index.
template <int D>
constexpr int v_line_index(int key, int d) {
  const int o = key >> 3;
  return (o * (D / 64) + d / 64) * V_PIECE_ELEMS +
         v_line_slot<D>(o, key & 7, (d & 63) >> 3) * 8 + (d & 7);
}

// Inverse map: lane `lane` of the DMA that fills piece p (elements
// p*512 + lane*8 .. +7) must SOURCE this (key, dim). The pieces of one key
// octet are consecutive, share `key` and step `dim` by 64.
template <int D>
constexpr VImgSrc v_line_source(int piece, int lane) {
  const int o = piece / (D / 64), pj = piece % (D / 64);
  int kk = 0, gg = 0;
  if (v_line_order(D) == 1) {
    gg = lane >> 3;
    kk = (lane & 7) ^ ((o & 1) << 2);
  } else {
    kk = lane >> 3;
    gg = (lane & 7) ^ (2 * ((kk >> 1) & 1)) ^ (4 * (o & 1));
  }
  return {o * 8 + kk, pj * 64 + gg * 8};
}

// Image element read by `lane` for the PV A-fragment of 16-dim tile `dtile`,
// 32-key group `ks`, half h (0 = lo, 1 = hi): v_img_afrag's semantics, i.e. 4
// bf16 of key ks*32 + kgrp*8 + h*4 + i/4 at dims dtile*16 + (i%4)*4, with
// kgrp = lane/16 and i = lane%16.
template <int D>
constexpr int v_line_afrag_elem(int dtile, int ks, int h, int lane) {
  const int kgrp = lane >> 4, i = lane & 15;
  return v_line_index<D>(ks * 32 + kgrp * 8 + h * 4 + (i >> 2),
                         dtile * 16 + (i & 3) * 4);
}

// The PV reads of a wave that owns DT dim tiles from `dtile0` (a multiple of
// DT) decompose into NB chunk-invariant per-lane bases plus compile-time
// offsets: order 1 keeps one base per half h (the XOR flips bit 2 of the
// slot lane-dependently) and steps dim tiles by a constant; order 2 the
// reverse.
template <int D, int DT>
constexpr int v_line_nbase() { return v_line_order(D) == 1 ? 2 : DT; }
template <int D>
constexpr int v_line_rd_base(int dtile0, int b, int lane) {
  return v_line_order(D) == 1 ? v_line_afrag_elem<D>(dtile0, 0, b, lane)
                              : v_line_afrag_elem<D>(dtile0 + b, 0, 0, lane);
}
template <int D>
constexpr int v_line_rd_sel(int dt, int h) { return v_line_order(D) == 1 ? h : dt; }
template <int D>
constexpr int v_line_rd_off(int dt, int ks, int h) {
  return ks * (D / 2) * 64 + (v_line_order(D) == 1 ? dt * 128 : h * 256);
}

// Compile-time proof for one (KT, D) and DT dim tiles per wave:
//  1. forward and inverse maps are inverses; the DMAs cover every granule of
//     the tile exactly once;
//  2. every piece is eight whole 128-byte-aligned line segments, one from
//     each of the eight rows of ONE key octet, and the next piece of the
//     octet is the same rows 64 dims on;
//  3. the A-fragment reads of every (dtile, ks, h) are conflict-free: within
//     each group of 32 lanes no two lanes touch the same 4-byte bank;
//  4. every such read is v_line_rd_base + v_line_rd_off.
// 1-2 are v_line_maps_ok, 3-4 v_line_reads_ok for one 32-key group; each is
// evaluated as a constant of its own (the constexpr step budget is per
// constant) and v_line_layout_ok is their conjunction.
template <int KT, int D>
constexpr bool v_line_maps_ok() {
  if (D % 64 || KT % 32) return false;
  bool seen[KT * D / 8] = {};
  for (int p = 0; p < v_line_npiece(KT, D); ++p) {
    unsigned segs[8] = {};
    const int o = p / (D / 64), pj = p % (D / 64);
    for (int lane = 0; lane < WAVE; ++lane) {
      const VImgSrc s = v_line_source<D>(p, lane);
      if (s.key < 0 || s.key >= KT || s.dim < 0 || s.dim >= D || s.dim % 8) return false;
      if (v_line_index<D>(s.key, s.dim) != p * V_PIECE_ELEMS + lane * 8) return false;
      bool& hit = seen[s.key * (D / 8) + s.dim / 8];
      if (hit) return false;
      hit = true;
      // rows of octet o, bytes [128*pj, 128*pj + 128) of the row
      if (s.key >> 3 != o || s.dim / 64 != pj) return false;
      segs[s.key & 7] |= 1u << ((s.dim & 63) >> 3);
      if (pj + 1 < D / 64) {
        const VImgSrc n = v_line_source<D>(p + 1, lane);
        if (n.key != s.key || n.dim != s.dim + 64) return false;
      }
    }
    for (unsigned m : segs)
      if (m != 0xffu) return false;
  }
  for (bool hit : seen)
    if (!hit) return false;
  return true;
}

template <int KT, int D, int DT>
constexpr bool v_line_reads_ok(int ks) {
  if ((D / 16) % DT || 4 % DT) return false;
  if (ks >= KT / 32) return true;
  for (int dtile = 0; dtile < D / 16; ++dtile)
    for (int h = 0; h < 2; ++h)
      for (int grp = 0; grp < 2; ++grp) {
        unsigned long long busy = 0;  // one bit per 4-byte bank
        for (int l = 0; l < 32; ++l) {
          const int lane = grp * 32 + l;
          const int e = v_line_afrag_elem<D>(dtile, ks, h, lane);
          if (e % 4 || e < 0 || e + 4 > v_line_elems(KT, D)) return false;
          const int dt = dtile % DT;
          if (e != v_line_rd_base<D>(dtile - dt, v_line_rd_sel<D>(dt, h), lane) +
                       v_line_rd_off<D>(dt, ks, h))
            return false;
          // an 8-byte read spans two banks
          const unsigned long long m = 3ull << ((e / 2) % 64);
          if (busy & m) return false;
          busy |= m;
        }
      }
  return true;
}

template <int KT, int D>
constexpr bool v_line_maps_ok_v = v_line_maps_ok<KT, D>();
template <int KT, int D, int DT, int KS>
constexpr bool v_line_reads_ok_v = v_line_reads_ok<KT, D, DT>(KS);
template <int KT, int D, int DT>
constexpr bool v_line_layout_ok_v =
    KT <= 128 && v_line_maps_ok_v<KT, D> && v_line_reads_ok_v<KT, D, DT, 0> &&
    v_line_reads_ok_v<KT, D, DT, 1> && v_line_reads_ok_v<KT, D, DT, 2> &&
    v_line_reads_ok_v<KT, D, DT, 3>;
static_assert(v_line_layout_ok_v<64, 128, 1> && v_line_layout_ok_v<128, 128, 1> &&
              v_line_layout_ok_v<64, 256, 2> && v_line_layout_ok_v<128, 256, 2>,
              "V line image: maps disagree, a piece is not eight whole lines, or "
              "a PV read has a bank conflict");

// PV A-fragment from the line image: the two transpose reads of v_img_afrag
// at this lane's own element indices.
DEVINL bf16x8_t v_line_afrag(const short* img, int e_lo, int e_hi) {
  bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&img[e_lo]);
  bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&img[e_hi]);
  bf16x8_t a;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = __bfloat16_as_short((__hip_bfloat16)lo[j]);
    a[4 + j] = __bfloat16_as_short((__hip_bfloat16)hi[j]);
  }
  return a;
}

// attn_pv_tile on the line image: same operands, same MFMA order. `vb` holds
// the lane's v_line_rd_base values for this wave's dim slab (chunk-invariant).
template <int D, int KT, int DT>
DEVINL void attn_pv_tile_lines(const short* img, const int (&vb)[v_line_nbase<D, DT>()],
                               const short* p_tile, const float* alpha_s,
                               bool rescale, f32x4_t (&ot)[DT], int lane) {
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
      const bf16x8_t a = v_line_afrag(
          img, vb[v_line_rd_sel<D>(dt, 0)] + v_line_rd_off<D>(dt, ks, 0),
          vb[v_line_rd_sel<D>(dt, 1)] + v_line_rd_off<D>(dt, ks, 1));
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
