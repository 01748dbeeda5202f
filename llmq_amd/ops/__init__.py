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
