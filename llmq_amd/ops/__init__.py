"""Op dispatch: hand-written CDNA4 HIP kernels on GPU, torch reference on CPU.

Policy (per the build contract): on a GPU box the HIP extension MUST be
present and is ALWAYS used — if `torch.cuda.is_available()` and the
extension failed to load, every op raises instead of silently falling back
to eager PyTorch. On CPU (tests, this dev container) the torch reference
implementations run.
"""

from __future__ import annotations

import os
from pathlib import Path
from typing import Optional, Tuple

import torch

from llmq_amd.ops import torch_ref

_EXT = None
_EXT_ERROR: Optional[str] = None
_EXT_TRIED = False


def _try_load_extension() -> None:
    """Lazy: called on first use, NOT at import (so `python -m
    llmq_amd.ops.build` can rebuild without a namespace clash against a
    stale loaded .so)."""
    global _EXT, _EXT_ERROR, _EXT_TRIED
    if _EXT_TRIED:
        return
    _EXT_TRIED = True
    here = Path(__file__).parent
    override = os.environ.get("LLMQ_OPS_SO")
    if override:
        candidates = [Path(override)]
    else:
        candidates = sorted(here.glob("_hip_ops*.so"))
    if not candidates:
        _EXT_ERROR = (
            f"HIP extension not built (no _hip_ops*.so under {here}). "
            "Run `python -m llmq_amd.ops.build` (or __graft_entry__.build())."
        )
        return
    try:
        torch.ops.load_library(str(candidates[0]))
        _EXT = torch.ops.llmq_amd
        _EXT_ERROR = None
    except Exception as exc:  # noqa: BLE001
        # If an identical build was already loaded in this process (e.g.
        # right after `build()`), the namespace exists — use it.
        try:
            torch.ops.llmq_amd.rmsnorm  # noqa: B018
            _EXT = torch.ops.llmq_amd
            _EXT_ERROR = None
        except Exception:
            _EXT_ERROR = f"failed to load {candidates[0]}: {exc}"


def has_hip_ext() -> bool:
    _try_load_extension()
    return _EXT is not None


def _use_hip(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    _try_load_extension()
    if _EXT is None:
        raise RuntimeError(
            f"llmq_amd HIP extension required for GPU execution but unavailable: {_EXT_ERROR}"
        )
    return True


# ---------------------------------------------------------------- norms --


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, offset: float = 0.0) -> torch.Tensor:
    if _use_hip(x):
        out = torch.empty_like(x)
        _EXT.rmsnorm(out, x, weight, eps, offset)
        return out
    return torch_ref.rmsnorm(x, weight, eps, offset)


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float, offset: float = 0.0
) -> Tuple[torch.Tensor, torch.Tensor]:
    """In place on GPU: residual += x, x = rmsnorm(residual). Returns (x, residual)."""
    if _use_hip(x):
        _EXT.fused_add_rmsnorm(x, residual, weight, eps, offset)
        return x, residual
    return torch_ref.fused_add_rmsnorm(x, residual, weight, eps, offset)


def norm_add_norm(
    x: torch.Tensor, residual: torch.Tensor, w_post: torch.Tensor,
    w_pre: torch.Tensor, eps: float, offset: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gemma-2 sandwich: residual += rmsnorm(x, w_post);
    x = rmsnorm(residual, w_pre). In place on GPU; returns (x, residual)."""
    if _use_hip(x):
        _EXT.norm_add_norm(x, residual, w_post, w_pre, eps, offset)
        return x, residual
    return torch_ref.norm_add_norm(x, residual, w_post, w_pre, eps, offset)


# ---------------------------------------------- fp8 quantisation (W8A8) --
# Row-wise dynamic activation quantisation under torch_ref.quant_fp8_rows'
# contract, stand-alone and fused behind each producer of a GEMM input. Every
# function returns (q [T, K] float8_e4m3fn, scale [T] fp32, ...). On the GPU
# the inputs are bf16 [T, K]; the fused kernels hold a row in registers, and
# rows longer than that compose the unfused kernel with quant_fp8_rows (same
# bits, one more trip through HBM).

_QUANT_NORM_MAX_HIDDEN = 8192    # fused norm kernels (4 vectors per thread)
_QUANT_ACT_MAX_INTER = 32768     # fused activation kernels (16 vectors)


def _quant_out(rows: int, k: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    return (torch.empty(rows, k, dtype=torch.float8_e4m3fn, device=device),
            torch.empty(rows, dtype=torch.float32, device=device))


def quant_fp8_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if _use_hip(x):
        q, scale = _quant_out(x.shape[0], x.shape[1], x.device)
        _EXT.quant_fp8_rows(q, scale, x)
        return q, scale
    return torch_ref.quant_fp8_rows(x)


def _act_and_mul_quant_fp8(x: torch.Tensor, gelu: bool):
    d = x.shape[-1] // 2
    if _use_hip(x) and d <= _QUANT_ACT_MAX_INTER:
        q, scale = _quant_out(x.shape[0], d, x.device)
        (_EXT.gelu_tanh_and_mul_quant_fp8 if gelu
         else _EXT.silu_and_mul_quant_fp8)(q, scale, x)
        return q, scale
    return quant_fp8_rows(gelu_tanh_and_mul(x) if gelu else silu_and_mul(x))


def silu_and_mul_quant_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """quant_fp8_rows(silu_and_mul(x)) without the [T, d] intermediate."""
    return _act_and_mul_quant_fp8(x, gelu=False)


def gelu_tanh_and_mul_quant_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """quant_fp8_rows(gelu_tanh_and_mul(x)) without the [T, d] intermediate."""
    return _act_and_mul_quant_fp8(x, gelu=True)


def rmsnorm_quant_fp8(
    x: torch.Tensor, weight: torch.Tensor, eps: float, offset: float = 0.0
) -> Tuple[torch.Tensor, torch.Tensor]:
    """quant_fp8_rows(rmsnorm(x, ...)) in one kernel."""
    if _use_hip(x) and x.shape[-1] <= _QUANT_NORM_MAX_HIDDEN:
        q, scale = _quant_out(x.shape[0], x.shape[1], x.device)
        _EXT.rmsnorm_quant_fp8(q, scale, x, weight, eps, offset)
        return q, scale
    return quant_fp8_rows(rmsnorm(x, weight, eps, offset))


def fused_add_rmsnorm_quant_fp8(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float,
    offset: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fused_add_rmsnorm with the normed rows quantised: returns (h_q,
    h_scale, residual). On the GPU residual is updated in place and x is
    left as it was when the one-kernel form runs."""
    if _use_hip(x) and x.shape[-1] <= _QUANT_NORM_MAX_HIDDEN:
        q, scale = _quant_out(x.shape[0], x.shape[1], x.device)
        _EXT.fused_add_rmsnorm_quant_fp8(q, scale, x, residual, weight, eps, offset)
        return q, scale, residual
    h, residual = fused_add_rmsnorm(x, residual, weight, eps, offset)
    return (*quant_fp8_rows(h), residual)


def norm_add_norm_quant_fp8(
    x: torch.Tensor, residual: torch.Tensor, w_post: torch.Tensor,
    w_pre: torch.Tensor, eps: float, offset: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """norm_add_norm (Gemma-2 sandwich) with the normed rows quantised:
    returns (h_q, h_scale, residual), as fused_add_rmsnorm_quant_fp8."""
    if _use_hip(x) and x.shape[-1] <= _QUANT_NORM_MAX_HIDDEN:
        q, scale = _quant_out(x.shape[0], x.shape[1], x.device)
        _EXT.norm_add_norm_quant_fp8(q, scale, x, residual, w_post, w_pre, eps, offset)
        return q, scale, residual
    h, residual = norm_add_norm(x, residual, w_post, w_pre, eps, offset)
    return (*quant_fp8_rows(h), residual)


def fp8_linear(
    a_q: torch.Tensor,      # [T, K] float8_e4m3fn
    a_scale: torch.Tensor,  # [T] fp32 per-row scale
    w_q: torch.Tensor,      # [N, K] float8_e4m3fn (torch linear weight layout)
    w_scale: torch.Tensor,  # [N] fp32 per-output-channel scale
    bias: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """(a_q * a_scale[:, None]) @ (w_q * w_scale[:, None]).T + bias. On the
    GPU the hipBLASLt fp8 GEMM with row-wise scales, bf16 [T, N] out; on CPU
    the fp32 fake-quant reference."""
    if not a_q.is_cuda:
        return torch_ref.fp8_linear(a_q, a_scale, w_q, w_scale, bias)
    return torch._scaled_mm(
        a_q, w_q.t(), scale_a=a_scale.unsqueeze(1), scale_b=w_scale.unsqueeze(0),
        bias=bias, out_dtype=torch.bfloat16)


# ------------------------------------------------ MXFP4 weights (W4A8) --
# Weights in OCP MXFP4 (torch_ref.quant_mxfp4_weight), activations as the
# fp8 mode carries them. On the GPU the GEMM is the hand-written scaled-MFMA
# kernel of hip/mxfp4_gemm.hip, which reads the weight in fragment order.

quant_mxfp4_weight = torch_ref.quant_mxfp4_weight
dequant_mxfp4_weight = torch_ref.dequant_mxfp4_weight


def mxfp4_supported(K: int, N: int) -> bool:
    """The envelope of the MXFP4 GEMM kernel for a weight [N, K]."""
    return K > 0 and N > 0 and K % 128 == 0 and N % 16 == 0


def mxfp4_pack_weight(
    codes: torch.Tensor,   # [N, K/2] uint8
    scales: torch.Tensor,  # [N, K/32] uint8
) -> Tuple[torch.Tensor, torch.Tensor]:
    """The weight as mxfp4_linear takes it on the tensors' device. On CPU the
    pair itself. On the GPU the kernel's fragment order, done once at load:
    codes [N/16, K/128, 64 lanes, 16 B] with lane 16 * kgrp + r holding
    elements 32 * kgrp .. + 31 of K step s of row 16 * g + r, and scales
    [N/16, ceil(K/512), 64 lanes, 4 B] with byte j the lane's block scale at
    K step 4 * q + j (steps past K padded with 127)."""
    if not codes.is_cuda:
        return codes, scales
    N, K = codes.shape[0], codes.shape[1] * 2
    assert mxfp4_supported(K, N), f"[N={N}, K={K}] outside the MXFP4 kernel's envelope"
    steps = K // 128
    pc = codes.view(N // 16, 16, steps, 4, 16).permute(0, 2, 3, 1, 4).contiguous()
    qsteps = (steps + 3) // 4
    ps = torch.full((N, qsteps * 4, 4), 127, dtype=torch.uint8, device=codes.device)
    ps[:, :steps] = scales.view(N, steps, 4)
    ps = ps.view(N // 16, 16, qsteps, 4, 4).permute(0, 2, 4, 1, 3).contiguous()
    return pc.view(N // 16, steps, 64, 16), ps.view(N // 16, qsteps, 64, 4)


def mxfp4_linear(
    a_q: torch.Tensor,      # [T, K] float8_e4m3fn
    a_scale: torch.Tensor,  # [T] fp32 per-row scale
    w_packed: Tuple[torch.Tensor, torch.Tensor],  # mxfp4_pack_weight's result
    bias: Optional[torch.Tensor] = None,
    splitk: int = 0,        # 0 = auto
) -> torch.Tensor:
    """(a_q * a_scale[:, None]) @ dequant_mxfp4_weight(w).T + bias. On the GPU
    the scaled-MFMA kernel, bf16 [T, N] out; on CPU the fp32 fake-quant
    reference."""
    codes, scales = w_packed
    if not _use_hip(a_q):
        return torch_ref.mxfp4_linear(a_q, a_scale, codes, scales, bias)
    out = torch.empty(a_q.shape[0], codes.shape[0] * 16, dtype=torch.bfloat16,
                      device=a_q.device)
    if a_q.shape[0]:
        _EXT.mxfp4_gemm(out, a_q, a_scale, codes, scales, bias, splitk)
    return out


# ----------------------------------------------------------------- rope --


def rope_inplace(
    q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor
) -> None:
    if _use_hip(q):
        _EXT.rope_inplace(q, k, positions, cos_sin)
        return
    torch_ref.rope_inplace(q, k, positions, cos_sin)


build_rope_cache = torch_ref.build_rope_cache


# ----------------------------------------------------------- activations --


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    if _use_hip(x):
        d = x.shape[-1] // 2
        out = torch.empty(*x.shape[:-1], d, dtype=x.dtype, device=x.device)
        _EXT.silu_and_mul(out, x)
        return out
    return torch_ref.silu_and_mul(x)


def gelu_tanh_and_mul(x: torch.Tensor) -> torch.Tensor:
    if _use_hip(x):
        d = x.shape[-1] // 2
        out = torch.empty(*x.shape[:-1], d, dtype=x.dtype, device=x.device)
        _EXT.gelu_tanh_and_mul(out, x)
        return out
    return torch_ref.gelu_tanh_and_mul(x)


def rope_and_cache(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
    k_cache: torch.Tensor, v_cache: torch.Tensor,
    positions: torch.Tensor, cos_sin: torch.Tensor, slot_mapping: torch.Tensor,
) -> None:
    """Fused: RoPE(q, k) in place + scatter rotated k and v into the paged
    cache (one launch instead of two per layer)."""
    if _use_hip(q):
        _EXT.rope_and_cache(q, k, v, k_cache, v_cache, positions, cos_sin, slot_mapping)
        return
    torch_ref.rope_inplace(q, k, positions, cos_sin)
    torch_ref.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)


_QKNORM_HEAD_DIMS = (64, 128, 256)  # qknorm_rope_and_cache_kernel's envelope


def qknorm_rope_and_cache(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
    k_cache: torch.Tensor, v_cache: torch.Tensor,
    q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float, offset: float,
    positions: torch.Tensor, cos_sin: torch.Tensor, slot_mapping: torch.Tensor,
) -> None:
    """Qwen3 attention prologue, fused: per-head RMSNorm over head_dim on q
    and k, RoPE in place, rotated k and v scattered into the paged cache
    (one launch per layer). Head dims outside the fused kernel's set compose
    the rmsnorm and rope_and_cache kernels instead (three launches, and one
    extra rounding to the storage dtype between norm and rotation)."""
    if _use_hip(q):
        D = q.shape[-1]
        if D in _QKNORM_HEAD_DIMS:
            _EXT.qknorm_rope_and_cache(
                q, k, v, k_cache, v_cache, q_weight, k_weight, eps, offset,
                positions, cos_sin, slot_mapping)
            return
        for t, w in ((q, q_weight), (k, k_weight)):
            t.copy_(rmsnorm(t.reshape(-1, D), w, eps, offset).view(t.shape))
        rope_and_cache(q, k, v, k_cache, v_cache, positions, cos_sin, slot_mapping)
        return
    torch_ref.qknorm_rope_and_cache(
        q, k, v, k_cache, v_cache, q_weight, k_weight, eps, offset,
        positions, cos_sin, slot_mapping)


# ------------------------------------------------------------- KV cache --


def reshape_and_cache(
    key: torch.Tensor,
    value: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    if _use_hip(key):
        _EXT.reshape_and_cache(key, value, k_cache, v_cache, slot_mapping)
        return
    torch_ref.reshape_and_cache(key, value, k_cache, v_cache, slot_mapping)


def gather_paged_kv(
    k_cache: torch.Tensor,       # [num_blocks, kv_heads, block_size, head_dim]
    v_cache: torch.Tensor,
    k_fresh: torch.Tensor,       # [Tq, kv_heads, head_dim] (views of the qkv GEMM output)
    v_fresh: torch.Tensor,
    block_tables: torch.Tensor,  # [B, W] int32, W >= ceil(max past / block_size)
    cu_seqlens: torch.Tensor,    # [B+1] int32 fresh-row offsets
    cu_seqlens_k: torch.Tensor,  # [B+1] int32 context-row offsets
    total_k: int,
    max_seqlen_k: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Assemble the packed attention context of a prefill segment whose
    sequences have part of their context in the paged cache (chunked
    prefill, prefix-cache hits): per sequence the past rows gathered through
    its block table, then its fresh rows. One launch per layer. Returns
    (k_att, v_att), each [total_k, kv_heads, head_dim] in k_fresh's dtype; an
    fp8 cache is dequantised exactly as `.to(bfloat16)` would."""
    KVH, D = k_fresh.shape[1], k_fresh.shape[2]
    k_att = k_fresh.new_empty(total_k, KVH, D)
    v_att = k_fresh.new_empty(total_k, KVH, D)
    if _use_hip(k_fresh):
        _EXT.gather_paged_kv(k_att, v_att, k_cache, v_cache, k_fresh, v_fresh,
                             block_tables, cu_seqlens, cu_seqlens_k,
                             int(max_seqlen_k))
    else:
        torch_ref.gather_paged_kv(k_att, v_att, k_cache, v_cache, k_fresh,
                                  v_fresh, block_tables, cu_seqlens,
                                  cu_seqlens_k, int(max_seqlen_k))
    return k_att, v_att


# ------------------------------------------------------------ attention --


def paged_decode_attention(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
    softcap: float = 0.0,
    window: int = 0,
) -> torch.Tensor:
    if _use_hip(q):
        out = torch.empty_like(q)
        _EXT.paged_decode_attention(
            out, q, k_cache, v_cache, block_tables, context_lens, scale, softcap, window
        )
        return out
    return torch_ref.paged_decode_attention(
        q, k_cache, v_cache, block_tables, context_lens, scale, softcap, window
    )


SHARED_PREFIX_MAX_BT = 1024  # table entries the cascade kernels stage in LDS


def shared_prefix_kernel_supported(
    dtype: torch.dtype, cache_dtype: torch.dtype, head_dim: int, group: int,
    block_size: int, prefix_blocks: int, suffix_blocks: int,
) -> bool:
    """The envelope of the HIP cascade kernels (bf16 q and KV cache)."""
    return (
        dtype == torch.bfloat16 and cache_dtype == torch.bfloat16
        and head_dim in (128, 256) and 1 <= group <= 16
        and block_size in (16, 32)
        and 1 <= prefix_blocks <= SHARED_PREFIX_MAX_BT
        and 1 <= suffix_blocks <= SHARED_PREFIX_MAX_BT
    )


def shared_prefix_decode_attention(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    prefix_table: torch.Tensor,
    prefix_len: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
    softcap: float = 0.0,
    window: int = 0,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Decode attention for a batch that shares one prefix: sequence b attends
    to `prefix_len` tokens ([1] int32, on q's device, a multiple of the block
    size) through `prefix_table` ([Wp] int32) and then to `context_lens[b]`
    tokens through `block_tables[b]`. On the GPU the prefix is attended once
    per 128 query rows instead of once per sequence (cascade attention);
    outside the kernels' envelope the tables are concatenated and the plain
    decode op runs: same answer, no saving. Rows with context_lens <= 0 are
    not written (pass `out` to keep their content)."""
    if not _use_hip(q):
        res = torch_ref.shared_prefix_decode_attention(
            q, k_cache, v_cache, prefix_table, prefix_len, block_tables,
            context_lens, scale, softcap, window)
        if out is None:
            return res
        live = context_lens > 0
        out[live] = res[live]
        return out
    keep_dead_rows = out is not None
    if out is None:
        out = torch.empty_like(q)
    H, D = q.shape[1], q.shape[2]
    KVH, bs = k_cache.shape[1], k_cache.shape[2]
    if shared_prefix_kernel_supported(
            q.dtype, k_cache.dtype, D, H // KVH, bs, prefix_table.shape[0],
            block_tables.shape[1]):
        _EXT.shared_prefix_decode_attention(
            out, q, k_cache, v_cache, prefix_table, prefix_len, block_tables,
            context_lens, scale, softcap, window)
        return out
    tables, lens = torch_ref.concat_prefix_tables(
        prefix_table, prefix_len, block_tables, context_lens, bs)
    # the plain op's split-KV merge writes rows of empty sequences too
    res = torch.empty_like(q) if keep_dead_rows else out
    _EXT.paged_decode_attention(
        res, q, k_cache, v_cache, tables, lens, scale, softcap, window)
    if keep_dead_rows:
        out.copy_(torch.where((lens > 0)[:, None, None], res, out))
    return out


def varlen_prefill_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,
    max_seqlen: int,
    scale: float,
    softcap: float = 0.0,
    window: int = 0,
    cu_seqlens_k: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Packed causal attention; cu_seqlens_k (key offsets per seq, >= query
    lengths) enables chunked prefill: Q is the last Lq positions of a
    Lk-long context."""
    cu_k = cu_seqlens if cu_seqlens_k is None else cu_seqlens_k
    if _use_hip(q):
        out = torch.empty_like(q)
        _EXT.varlen_prefill_attention(
            out, q, k, v, cu_seqlens, cu_k, int(max_seqlen), scale, softcap, window
        )
        return out
    return torch_ref.varlen_prefill_attention(
        q, k, v, cu_seqlens, scale, softcap, window, cu_seqlens_k=cu_k
    )


# ---------------------------------------------------------- skinny GEMM --


def _skg_stageable(t: torch.Tensor) -> bool:
    """The binding's preconditions on a skinny_gemm operand (x or w)."""
    return (t.stride(-1) == 1 and t.stride(0) % 8 == 0
            and t.data_ptr() % 16 == 0)


def skinny_gemm(
    x: torch.Tensor,          # [M, K] bf16
    w: torch.Tensor,          # [N, K] bf16 (torch linear weight layout)
    bias: Optional[torch.Tensor] = None,
    splitk: int = 0,          # 0 = auto
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Hand-written skinny-M decode-projection GEMM (out = x @ w.T + bias).

    256x256x64 MFMA tile, glds-staged with source-side st_16x32 swizzle,
    counted-vmcnt pipeline; split-K slabs + fused reduce for narrow-N
    shapes. Falls back to F.linear off-GPU / unsupported shapes, and for
    views the 16-byte staging loads cannot take: x and w need a 16-byte
    aligned base, unit inner stride and a row stride that is a multiple of
    8 elements; bias must be contiguous."""
    M, K = x.shape
    N = w.shape[0]
    if not (x.is_cuda and x.dtype == torch.bfloat16 and K % 64 == 0
            and N % 4 == 0 and M > 0 and K > 0 and N > 0
            and _skg_stageable(x) and _skg_stageable(w)
            and (bias is None or bias.is_contiguous()) and has_hip_ext()):
        import torch.nn.functional as F

        out_ref = F.linear(x, w, bias)
        if out is None:
            return out_ref
        out.copy_(out_ref)
        return out
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _EXT.skinny_gemm(out, x, w, bias, splitk)
    return out


# ------------------------------------------------------------- sampling --


def sample_gumbel_argmax(
    out: torch.Tensor,        # [B] int64
    keys: torch.Tensor,       # [B] int64 scratch (packed value|~index)
    logits: torch.Tensor,     # [B, V] fp32, or bf16/fp16 as the GEMM wrote them
    temps: torch.Tensor,      # [B] fp32 (<= 0 → greedy row)
    req_seeds: torch.Tensor,  # [B] int32 (0 = unseeded)
    req_pos: torch.Tensor,    # [B] int32 output position (seeded rows)
    seed: int,
    step: int,
    bounds: Optional[torch.Tensor] = None,  # [B] fp32 top-k/p keep-bound
    softcap: float = 0.0,     # > 0: sample from cap * tanh(logit / cap)
    pen_table: Optional[torch.Tensor] = None,   # [slots, Vpad] int16 counts
    pen_slots: Optional[torch.Tensor] = None,   # [B] int32 table row (-1 = none)
    pen_params: Optional[torch.Tensor] = None,  # [B, 3] fp32 (r, freq, pres)
) -> None:
    """Fused one-pass sampler: per-row Gumbel-max (== softmax sampling) or
    argmax for greedy rows, optionally truncated to {logit >= bounds[b]}
    (top-k/top-p, from topk_topp_bound). Unseeded rows draw from the
    counter-based (engine seed, step, row) stream; rows with a request seed
    draw from (request_seed, output_position) — reproducible for a given
    request regardless of batch placement. The kernel widens the logits and
    applies the final soft-cap in registers: tokens equal those sampled from
    `torch.tanh(logits.float() / softcap) * softcap`. With a count table,
    rows whose slot is >= 0 sample from `torch_ref.apply_penalties` of those
    logits (bit 15 of a table word = in the prompt, bits 0-14 = output
    count); without one the call runs the kernel it ran before."""
    assert _use_hip(logits)
    keys.zero_()
    _EXT.sample_gumbel_argmax(out, keys, logits, temps, req_seeds, req_pos,
                              seed, step, bounds, softcap, pen_table,
                              pen_slots, pen_params)


def topk_topp_bound(
    logits: torch.Tensor,   # [B, V] fp32, or bf16/fp16 as the GEMM wrote them
    temps: torch.Tensor,    # [B] fp32
    top_ps: torch.Tensor,   # [B] fp32
    top_ks: torch.Tensor,   # [B] int64 (0 = off)
    softcap: float = 0.0,   # > 0: bound on cap * tanh(logit / cap)
    min_ps: Optional[torch.Tensor] = None,      # [B] fp32 (0 = off)
    pen_table: Optional[torch.Tensor] = None,   # as in sample_gumbel_argmax
    pen_slots: Optional[torch.Tensor] = None,
    pen_params: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Per-row logit-space keep-bound realising top-p ∧ top-k truncation
    via histogram select (3 streaming passes; no full-vocab sort). With a
    soft-cap the bound is in capped-logit space, the space the sampler
    compares in when given the same `softcap`. min_p adds the bound
    max + T * ln(min_p); a row keeps the larger of the two bounds. With a
    count table the bound is on the penalised logits."""
    assert _use_hip(logits)
    out = torch.empty(logits.size(0), dtype=torch.float32, device=logits.device)
    _EXT.topk_topp_bound(out, logits, temps, top_ps, top_ks, softcap, min_ps,
                         pen_table, pen_slots, pen_params)
    return out


def penalty_count_tokens(
    table: torch.Tensor,   # [slots, Vpad] int16 counts
    slots: torch.Tensor,   # [B] int32 (-1 = none); distinct where >= 0
    tokens: torch.Tensor,  # [B] int64 sampled tokens
) -> None:
    """table[slots[b], tokens[b]] += 1 on bits 0-14 (saturating at 32767, bit
    15 kept) for rows with a slot. On the GPU one kernel on the current
    stream; on CPU tensors the same update with torch ops."""
    if _use_hip(table):
        _EXT.penalty_count_tokens(table, slots, tokens)
        return
    rows = (slots >= 0).nonzero(as_tuple=True)[0]
    if rows.numel() == 0:
        return
    s, t = slots[rows].long(), tokens[rows].long()
    words = table[s, t]
    table.index_put_((s, t), torch.where((words & 0x7FFF) == 0x7FFF, words, words + 1))


MAX_LOGPROBS = torch_ref.MAX_LOGPROBS


def token_logprobs(
    logits: torch.Tensor,   # [B, V] fp32, or bf16/fp16 as the GEMM wrote them
    tokens: torch.Tensor,   # [B] int64 sampled tokens
    k: int,                 # alternatives per row, 0..min(MAX_LOGPROBS, V)
    softcap: float = 0.0,   # > 0: logprobs of cap * tanh(logit / cap)
    rows: Optional[torch.Tensor] = None,  # [R] int32 rows that asked (None = all)
    out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
    threads: int = 0,       # workgroup size of the kernel, 0 = default
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ids [R, 1+k] int32, lp [R, 1+k] fp32, rank [R] int32) of
    torch_ref.token_logprobs: the sampled token's log-probability under
    log_softmax of the soft-capped logits, its rank, and the k most likely
    tokens in (value descending, index ascending) order. On the GPU one
    kernel, one workgroup per requested row, reading each logit once; no
    launch when no row asked. `out` = (ids, lp, rank) tensors to fill, which
    may be column slices of a wider buffer."""
    V = logits.size(1)
    assert 0 <= k <= min(MAX_LOGPROBS, V), f"k={k} outside [0, min({MAX_LOGPROBS}, {V})]"
    if not _use_hip(logits):
        res = torch_ref.token_logprobs(logits, tokens, k, softcap, rows)
        if out is None:
            return res
        for dst, src in zip(out, res):
            dst.copy_(src)
        return out
    dev = logits.device
    if rows is None:
        rows = torch.arange(logits.size(0), dtype=torch.int32, device=dev)
    R = rows.numel()
    if out is None:
        out = (torch.empty(R, 1 + k, dtype=torch.int32, device=dev),
               torch.empty(R, 1 + k, dtype=torch.float32, device=dev),
               torch.empty(R, dtype=torch.int32, device=dev))
    ids, lp, rank = out
    if R:
        _EXT.token_logprobs(lp, ids, rank, logits, rows, tokens, k, softcap, threads)
    return out


def lm_head_logprobs_supported(hidden: torch.Tensor, w: torch.Tensor) -> bool:
    """Whether the fused HIP kernel can take (hidden [T, K], w [V, K]): bf16
    on the GPU, K a multiple of 64, and skinny_gemm's staging rules (16-byte
    aligned base, unit inner stride, row stride a multiple of 8 elements)."""
    return (hidden.is_cuda and hidden.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16 and hidden.dim() == 2 and w.dim() == 2
            and hidden.size(0) > 0 and hidden.size(1) == w.size(1)
            and hidden.size(1) % 64 == 0
            and _skg_stageable(hidden) and _skg_stageable(w) and has_hip_ext())


def lm_head_logprobs(
    hidden: torch.Tensor,   # [T, K] final-norm hidden states
    w: torch.Tensor,        # [V, K] lm_head, or the tied embedding
    rows: torch.Tensor,     # [R] int rows of hidden to score
    targets: torch.Tensor,  # [R] int token id in [0, V) per scored row
    softcap: float = 0.0,
    nsplit: int = 0,        # vocabulary slices per 256-row tile, 0 = auto
    block_rows: int = 1024,
) -> torch.Tensor:
    """lp [R] fp32 of torch_ref.lm_head_logprobs: the log-probability of
    targets[r] given hidden[rows[r]], for prompt logprobs. On the GPU one
    fused kernel: the lm_head GEMM with an epilogue that reduces every
    vocabulary tile to a running log-sum-exp per row and picks the target
    logit, so no logit is stored (workspace: (2 nsplit + 1) R floats).
    Outside the kernel's envelope (CPU, fp16/fp32, odd K) and with
    LLMQ_FUSED_PROMPT_LOGPROBS=0 the blocked composition runs instead: the
    lm_head GEMM and token_logprobs over block_rows rows at a time."""
    fused = os.environ.get("LLMQ_FUSED_PROMPT_LOGPROBS", "1") not in ("0", "false", "")
    if not (fused and lm_head_logprobs_supported(hidden, w)):
        return torch_ref.lm_head_logprobs(
            hidden, w, rows, targets, softcap, block_rows,
            token_logprobs_fn=token_logprobs)
    lp = torch.empty(rows.numel(), dtype=torch.float32, device=hidden.device)
    _EXT.lm_head_logprobs(
        lp, hidden, w, rows.to(torch.int32).contiguous(),
        targets.to(torch.int32).contiguous(), softcap, nsplit)
    return lp


# ----------------------------------------------------------- multi-LoRA --
# Per-token adapters on top of a layer projection. The data structures and
# the numeric contract live in torch_ref. There is no HIP kernel for it yet,
# and a GPU call raises: no GPU hot path runs eager PyTorch.

LoraStacks = torch_ref.LoraStacks
LoraMeta = torch_ref.LoraMeta
lora_meta = torch_ref.lora_meta
lora_meta_arrays = torch_ref.lora_meta_arrays


def lora_apply(
    out: torch.Tensor,     # [T, N] the projection's output, updated in place
    x: torch.Tensor,       # [T, K] the projection's input
    stacks: LoraStacks,
    meta: LoraMeta,
) -> torch.Tensor:
    """torch_ref.lora_apply: out[t] += scale * B_a (A_a x[t]) for the rows t
    that meta lists under an adapter a. CPU only."""
    if x.is_cuda:
        raise RuntimeError(
            "lora_apply has no HIP kernel yet: LoRA adapters run on the CPU path only")
    return torch_ref.lora_apply(out, x, stacks, meta)


def sample_tokens(
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_ps: torch.Tensor,
    top_ks: torch.Tensor,
    generator: Optional[torch.Generator] = None,
    min_p: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    # Generic path (top-k/top-p/min_p capable). The serving hot loop uses the
    # fused sample_gumbel_argmax above when no top-k/top-p is requested.
    if logits.is_cuda:
        return _sample_tokens_gpu(logits, temperatures, top_ps, top_ks, generator, min_p)
    return torch_ref.sample_tokens(logits, temperatures, top_ps, top_ks, generator, min_p)


def _sample_tokens_gpu(
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_ps: torch.Tensor,
    top_ks: torch.Tensor,
    generator: Optional[torch.Generator],
    min_p: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Batched GPU sampling without per-sequence python loops."""
    B, V = logits.shape
    greedy = temperatures <= 0
    temps = torch.where(greedy, torch.ones_like(temperatures), temperatures)
    scaled = logits.float() / temps.unsqueeze(1)
    need_topk = bool((top_ks > 0).any()) and bool((top_ks < V).any())
    need_topp = bool((top_ps < 1.0).any())
    need_minp = min_p is not None and bool((min_p > 0).any())
    if need_topk or need_topp or need_minp:
        # histogram-select keep-bound (3 streaming passes) instead of the
        # full-vocab sort — at B=256 × V=256k the sort was a multi-ms cliff
        bound = topk_topp_bound(logits.float(), temperatures.float(),
                                top_ps.float(), top_ks,
                                min_ps=min_p.float() if need_minp else None)
        scaled = torch.where(logits.float() >= bound.unsqueeze(1), scaled,
                             torch.full_like(scaled, float("-inf")))
    # Gumbel-max trick: single fused sample, no multinomial sync.
    u = torch.rand(B, V, device=logits.device, generator=generator)
    gumbel = -torch.log(-torch.log(u.clamp_min(1e-20)).clamp_min(1e-20))
    sampled = (scaled + gumbel).argmax(dim=-1)
    greedy_choice = logits.argmax(dim=-1)
    return torch.where(greedy, greedy_choice, sampled)
