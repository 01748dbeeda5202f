// Shared device helpers for the attention kernels (prefill + decode): MFMA
// fragment vector types, the LDS swizzle, the hidden-from-hipcc global->LDS
// DMA with its hand-counted barriers, and the packed fp8 converter.
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4v;
typedef __attribute__((address_space(3))) bf16x4v lds_bf16x4;

DEVINL int swz(int row, int d) {  // element-index XOR swizzle (16B granules)
  return d ^ ((row & 7) << 3);
}

// 16-B-per-lane global→LDS DMA, HIDDEN from hipcc in inline asm: with the
// builtin form the compiler conservatively re-inserts `s_waitcnt vmcnt(0)`
// before the first ds_read that may alias the DMA destination (verified in
// the .s: it landed ahead of the PV tr16 reads, draining the K prefetch
// every chunk). Hand-counted vmcnt in pipe_barrier_vm is the only wait
// discipline for these, per guide §5.7 (its LDS-DMA recipe: M0 carries the
// wave-uniform LDS byte address, saved/written/restored in ONE statement;
// the s_nop is the SALU-write→M0-read wait state).
DEVINL void glds16(const void* src, void* lds_dst_uniform) {
  unsigned lds_off = (unsigned)(unsigned long)(
      (__attribute__((address_space(3))) char*)lds_dst_uniform);
  lds_off = __builtin_amdgcn_readfirstlane(lds_off);
  unsigned keep;
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
