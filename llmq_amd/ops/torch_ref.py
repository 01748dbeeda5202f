"""Reference implementations of the engine's hot ops in plain PyTorch.

These are the NUMERICS ORACLES for the HIP kernels (tests compare the
CDNA4 kernels against these at fp32) and the CPU execution path for tests.
They are deliberately simple; nothing here runs in the GPU hot loop.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, offset: float = 0.0) -> torch.Tensor:
    """RMSNorm. Gemma uses weight offset +1 (x * (1 + w))."""
    dtype = x.dtype
    xf = x.float()
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    xf = xf * torch.rsqrt(var + eps)
    return (xf * (weight.float() + offset)).to(dtype)


def norm_add_norm(x, residual, w_post, w_pre, eps, offset=0.0):
    """residual += rmsnorm(x, w_post); x = rmsnorm(residual, w_pre)."""
    t = rmsnorm(x, w_post, eps, offset)
    residual = (residual.float() + t.float()).to(x.dtype)
    out = rmsnorm(residual, w_pre, eps, offset)
    return out, residual


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float, offset: float = 0.0
) -> Tuple[torch.Tensor, torch.Tensor]:
    """residual += x; out = rmsnorm(residual). Returns (out, new_residual)."""
    new_residual = (residual.float() + x.float()).to(x.dtype)
    return rmsnorm(new_residual, weight, eps, offset), new_residual


def build_rope_cache(
    max_positions: int, rotary_dim: int, theta: float, device,
    dtype=torch.float32, rope_scaling=None,
) -> torch.Tensor:
    """[max_positions, rotary_dim]: first half cos, second half sin.

    rope_scaling: HF config.json dict. Supported: "llama3" (Llama-3.1/3.2
    wavelength remap, transformers modeling_rope_utils
    _compute_llama3_parameters) and "linear" (position interpolation —
    dividing inv_freq by factor is identical to dividing positions).
    Unknown types raise rather than silently serving wrong rotations.
    """
    import math as _math

    inv_freq = 1.0 / (
        theta ** (torch.arange(0, rotary_dim, 2, device=device, dtype=torch.float32) / rotary_dim)
    )
    if rope_scaling:
        rtype = rope_scaling.get("rope_type") or rope_scaling.get("type")
        factor = float(rope_scaling.get("factor", 1.0))
        if rtype == "llama3":
            low = float(rope_scaling["low_freq_factor"])
            high = float(rope_scaling["high_freq_factor"])
            orig = float(rope_scaling["original_max_position_embeddings"])
            wavelen = 2 * _math.pi / inv_freq
            smooth = (orig / wavelen - low) / (high - low)
            smoothed = (1 - smooth) * inv_freq / factor + smooth * inv_freq
            inv_freq = torch.where(
                wavelen < orig / high, inv_freq,
                torch.where(wavelen > orig / low, inv_freq / factor, smoothed),
            )
        elif rtype == "linear":
            inv_freq = inv_freq / factor
        elif rtype in (None, "default"):
            pass
        else:
            raise ValueError(f"unsupported rope_scaling type: {rtype!r}")
    t = torch.arange(max_positions, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)  # [P, rotary_dim/2]
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).to(dtype)


def rope_inplace(
    q: torch.Tensor,  # [T, num_heads, head_dim]
    k: torch.Tensor,  # [T, num_kv_heads, head_dim]
    positions: torch.Tensor,  # [T]
    cos_sin: torch.Tensor,  # [max_pos, head_dim] (cos || sin)
) -> None:
    """NeoX-style (rotate-half) RoPE applied in place to q and k."""
    half = q.shape[-1] // 2
    cs = cos_sin[positions]  # [T, head_dim]
    cos = cs[:, :half].unsqueeze(1)  # [T, 1, half]
    sin = cs[:, half:].unsqueeze(1)
    for t in (q, k):
        # clone: for f32 inputs .float() aliases, and the first write below
        # would corrupt x1 before the second line reads it
        x1 = t[..., :half].float().clone()
        x2 = t[..., half:].float().clone()
        t[..., :half] = (x1 * cos - x2 * sin).to(t.dtype)
        t[..., half:] = (x2 * cos + x1 * sin).to(t.dtype)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    """x = [*, 2*d]: silu(x[..., :d]) * x[..., d:]."""
    d = x.shape[-1] // 2
    a, b = x[..., :d], x[..., d:]
    return (torch.nn.functional.silu(a.float()) * b.float()).to(x.dtype)


def gelu_tanh_and_mul(x: torch.Tensor) -> torch.Tensor:
    d = x.shape[-1] // 2
    a, b = x[..., :d], x[..., d:]
    return (torch.nn.functional.gelu(a.float(), approximate="tanh") * b.float()).to(x.dtype)


FP8_MAX = 448.0  # largest finite float8_e4m3fn


def quant_fp8_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-wise dynamic fp8 quantisation, the contract of the HIP quant
    kernels: a = max(amax |x|, 1e-30), scale = a / 448, q = e4m3fn(clamp(x *
    (448 / a), ±448)), all in fp32 with true divisions (tensor divisors: a
    Python-scalar divisor may become a multiply by its reciprocal).
    x [..., K] → (q [..., K] float8_e4m3fn, scale [...] fp32)."""
    xf = x.float()
    a = xf.abs().amax(dim=-1).clamp_min(1e-30)
    top = torch.full_like(a, FP8_MAX)
    q = (xf * (top / a).unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX)
    return q.to(torch.float8_e4m3fn), a / top


def quant_fp8_weight(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-output-channel fp8 weight [N, K] + fp32 scale [N] of the bf16
    rounding of w: what a bf16 engine would have held, whatever dtype and
    device w is in, so CPU and GPU engines quantise the same values."""
    return quant_fp8_rows(w.to(torch.bfloat16))


def fp8_linear(
    a_q: torch.Tensor, a_scale: torch.Tensor, w_q: torch.Tensor,
    w_scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Fake-quant reference of the W8A8 GEMM: dequantise both operands to
    fp32, fp32 matmul, add the bias. Returns fp32 [T, N]."""
    a = a_q.float() * a_scale.unsqueeze(-1)
    w = w_q.float() * w_scale.unsqueeze(-1)
    out = a @ w.t()
    return out if bias is None else out + bias.float()


def reshape_and_cache(
    key: torch.Tensor,  # [T, kv_heads, head_dim]
    value: torch.Tensor,
    k_cache: torch.Tensor,  # [num_blocks, kv_heads, block_size, head_dim]
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,  # [T] int32/int64 global slot ids
) -> None:
    block_size = k_cache.shape[2]
    slots = slot_mapping.long()
    blocks = slots // block_size
    offs = slots % block_size
    k_cache[blocks, :, offs, :] = key.to(k_cache.dtype)
    v_cache[blocks, :, offs, :] = value.to(v_cache.dtype)


def gather_paged_kv(
    k_out: torch.Tensor,  # [>= total_k, kv_heads, head_dim]
    v_out: torch.Tensor,
    k_cache: torch.Tensor,  # [num_blocks, kv_heads, block_size, head_dim]
    v_cache: torch.Tensor,
    k_fresh: torch.Tensor,  # [Tq, kv_heads, head_dim] (may be strided views)
    v_fresh: torch.Tensor,
    block_tables: torch.Tensor,  # [B, W] int32
    cu_seqlens: torch.Tensor,    # [B+1] int32 fresh-row offsets
    cu_seqlens_k: torch.Tensor,  # [B+1] int32 context-row offsets
    max_seqlen_k: int,
) -> None:
    """Packed attention context per sequence: P = Lk - Lq rows gathered from
    the paged cache through the sequence's block table, then its Lq fresh
    rows, written to rows [cu_seqlens_k[b], cu_seqlens_k[b+1]) of k_out /
    v_out. Cache rows are cast to the output dtype (fp8 → bf16 is exact)."""
    B = cu_seqlens.numel() - 1
    if B == 0 or max_seqlen_k == 0:
        return
    dev = k_out.device
    bs = k_cache.shape[2]
    cu_q = cu_seqlens.long()
    cu_k = cu_seqlens_k.long()
    total_k = int(cu_k[-1])
    lens_k = cu_k[1:] - cu_k[:-1]
    past = lens_k - (cu_q[1:] - cu_q[:-1])                      # [B]
    rows = torch.arange(total_k, device=dev)
    seq = torch.repeat_interleave(torch.arange(B, device=dev), lens_k)
    r = rows - cu_k[seq]                                        # row in context
    is_past = r < past[seq]
    # past rows: cache[block_tables[b, r // bs], :, r % bs]
    pr, ps = r[is_past], seq[is_past]
    blocks = block_tables.long()[ps, pr // bs]
    k_out[rows[is_past]] = k_cache[blocks, :, pr % bs].to(k_out.dtype)
    v_out[rows[is_past]] = v_cache[blocks, :, pr % bs].to(v_out.dtype)
    # fresh rows: k_fresh[cu_seqlens[b] + r - P]
    fr, fsq = r[~is_past], seq[~is_past]
    src = cu_q[fsq] + fr - past[fsq]
    k_out[rows[~is_past]] = k_fresh[src]
    v_out[rows[~is_past]] = v_fresh[src]


def qknorm_rope_and_cache(
    q: torch.Tensor,  # [T, num_heads, head_dim]
    k: torch.Tensor,  # [T, num_kv_heads, head_dim]
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    q_weight: torch.Tensor,  # [head_dim]
    k_weight: torch.Tensor,
    eps: float,
    offset: float,
    positions: torch.Tensor,
    cos_sin: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    """Qwen3 attention prologue: per-head RMSNorm over head_dim on q and k,
    NeoX RoPE, then the paged-cache write. Mirrors the fused kernel's
    rounding: the normed values stay fp32 into the rotation and are cast to
    q.dtype ONCE (rmsnorm + rope_inplace would round in between). Rows with
    a negative slot (graph padding) are normed and rotated but not cached."""
    half = q.shape[-1] // 2
    cs = cos_sin[positions].float()
    cos = cs[:, :half].unsqueeze(1)
    sin = cs[:, half:].unsqueeze(1)
    for t, w in ((q, q_weight), (k, k_weight)):
        xf = t.float()
        var = xf.pow(2).mean(dim=-1, keepdim=True)
        xf = xf * torch.rsqrt(var + eps) * (w.float() + offset)
        x1, x2 = xf[..., :half], xf[..., half:]
        t.copy_(torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1))
    keep = slot_mapping >= 0
    if bool(keep.all()):
        reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)
    else:
        reshape_and_cache(k[keep], v[keep], k_cache, v_cache, slot_mapping[keep])


def _softcap(scores: torch.Tensor, cap: float) -> torch.Tensor:
    if cap and cap > 0:
        return torch.tanh(scores / cap) * cap
    return scores


def paged_decode_attention(
    q: torch.Tensor,  # [B, num_heads, head_dim]
    k_cache: torch.Tensor,  # [num_blocks, kv_heads, block_size, head_dim]
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,  # [B, max_blocks] int32
    context_lens: torch.Tensor,  # [B] int32 (length INCLUDING current token)
    scale: float,
    softcap: float = 0.0,
    window: int = 0,
) -> torch.Tensor:
    """Single-token decode attention over the paged cache (reference)."""
    B, H, D = q.shape
    KVH = k_cache.shape[1]
    bs = k_cache.shape[2]
    group = H // KVH
    out = torch.empty_like(q)
    for b in range(B):
        L = int(context_lens[b])
        nblocks = (L + bs - 1) // bs
        blocks = block_tables[b, :nblocks].long()
        k = k_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, nblocks * bs, D)[:, :L]
        v = v_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, nblocks * bs, D)[:, :L]
        start = max(0, L - window) if window else 0
        k, v = k[:, start:], v[:, start:]
        qb = q[b].view(KVH, group, D).float()  # [KVH, G, D]
        scores = torch.einsum("hgd,hld->hgl", qb, k.float()) * scale
        scores = _softcap(scores, softcap)
        probs = torch.softmax(scores, dim=-1)
        ob = torch.einsum("hgl,hld->hgd", probs, v.float())
        out[b] = ob.reshape(H, D).to(q.dtype)
    return out


def varlen_prefill_attention(
    q: torch.Tensor,  # [Tq, num_heads, head_dim]
    k: torch.Tensor,  # [Tk, kv_heads, head_dim]
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,  # [B+1] query offsets
    scale: float,
    softcap: float = 0.0,
    window: int = 0,
    cu_seqlens_k: "Optional[torch.Tensor]" = None,  # [B+1] key offsets
) -> torch.Tensor:
    """Causal attention over packed variable-length sequences (reference).

    With cu_seqlens_k, each sequence's K/V may be LONGER than its Q (chunked
    prefill: the queries are the last Tq positions of a Tk-long context);
    query row i has absolute position (Tk - Tq) + i."""
    T, H, D = q.shape
    KVH = k.shape[1]
    group = H // KVH
    cu_k = cu_seqlens if cu_seqlens_k is None else cu_seqlens_k
    out = torch.empty_like(q)
    for b in range(len(cu_seqlens) - 1):
        s, e = int(cu_seqlens[b]), int(cu_seqlens[b + 1])
        sk, ek = int(cu_k[b]), int(cu_k[b + 1])
        Lq, Lk = e - s, ek - sk
        off = Lk - Lq  # absolute position of q row 0
        qb = q[s:e].float()  # [Lq, H, D]
        kb = k[sk:ek].float().repeat_interleave(group, dim=1)  # [Lk, H, D]
        vb = v[sk:ek].float().repeat_interleave(group, dim=1)
        scores = torch.einsum("ihd,jhd->hij", qb, kb) * scale
        scores = _softcap(scores, softcap)
        i = torch.arange(Lq, device=q.device).view(-1, 1) + off
        j = torch.arange(Lk, device=q.device).view(1, -1)
        mask = j > i
        if window:
            mask = mask | (j <= i - window)
        scores.masked_fill_(mask.unsqueeze(0), float("-inf"))
        probs = torch.softmax(scores, dim=-1)
        ob = torch.einsum("hij,jhd->ihd", probs, vb)
        out[s:e] = ob.to(q.dtype)
    return out


def _per_row(x, like: torch.Tensor) -> torch.Tensor:
    """A float or a [B] tensor as an fp32 [B, 1] column on `like`'s device."""
    t = torch.as_tensor(x, dtype=torch.float32, device=like.device)
    return t.reshape(-1, 1).expand(like.size(0), 1)


def apply_penalties(
    logits: torch.Tensor,     # [B, vocab] fp32, soft-cap already applied
    counts: torch.Tensor,     # [B, vocab] int: occurrences in the output so far
    in_prompt: torch.Tensor,  # [B, vocab] bool: token occurs in the prompt
    r,                        # repetition penalty, float or [B]
    freq,                     # frequency penalty, float or [B]
    pres,                     # presence penalty, float or [B]
) -> torch.Tensor:
    """Repetition, frequency and presence penalties, in this order. r, freq
    and pres are held as fp32 tensors, so `l / r` is a true fp32 division
    (torch turns a division by a Python scalar into a multiply by its
    reciprocal); the HIP sampler computes the same expression bit for bit."""
    l = logits.float()
    r, freq, pres = _per_row(r, l), _per_row(freq, l), _per_row(pres, l)
    seen = in_prompt | (counts > 0)
    l = torch.where(seen, torch.where(l > 0, l / r, l * r), l)
    l = l - freq * counts.float()
    l = l - pres * (counts > 0).float()
    return l


MAX_LOGPROBS = 20


def token_logprobs(
    logits: torch.Tensor,  # [B, vocab] as the lm_head stored them, or fp32
    tokens: torch.Tensor,  # [B] int: the sampled token of every row
    k: int,                # alternatives per row, 0..MAX_LOGPROBS
    softcap: float = 0.0,  # > 0: the model's final soft-cap, still to apply
    rows: Optional[torch.Tensor] = None,  # [R] int: rows that asked (None = all)
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Log-probabilities of the sampled tokens under the model's own
    distribution: log_softmax of the fp32 logits after the final soft-cap,
    before penalties, temperature and top-k/top-p/min_p.

    The vocabulary is ordered by (value descending, index ascending), a
    stable descending sort; torch.topk leaves the order of ties open. Returns
    for each requested row (ids [R, 1+k] int32, lp [R, 1+k] fp32, rank [R]
    int32): column 0 is the sampled token, columns 1..k the first k entries
    of that order, lp = l[id] - logsumexp(l), and rank the 1-based position
    of the sampled token in the order."""
    V = logits.size(1)
    if not 0 <= k <= min(MAX_LOGPROBS, V):
        raise ValueError(f"k must be in [0, min({MAX_LOGPROBS}, vocab)], got {k}")
    if rows is not None:
        rows = rows.long()
        logits, tokens = logits[rows], tokens[rows]
    l = logits.float()
    if softcap > 0:
        l = torch.tanh(l / softcap) * softcap
    tok = tokens.long().reshape(-1, 1)
    ids = tok
    if k > 0:
        order = torch.sort(l, dim=-1, descending=True, stable=True).indices
        ids = torch.cat([tok, order[:, :k]], dim=1)
    lp = l.gather(1, ids) - torch.logsumexp(l, dim=-1, keepdim=True)
    c = l.gather(1, tok)
    idx = torch.arange(V, device=l.device).unsqueeze(0)
    rank = ((l > c) | ((l == c) & (idx < tok))).sum(dim=-1) + 1
    return ids.to(torch.int32), lp, rank.to(torch.int32)


def sample_tokens(
    logits: torch.Tensor,  # [B, vocab] float
    temperatures: torch.Tensor,  # [B]
    top_ps: torch.Tensor,  # [B]
    top_ks: torch.Tensor,  # [B] int (0 = off)
    generator: Optional[torch.Generator] = None,
    min_p: Optional[torch.Tensor] = None,  # [B] (0 = off)
) -> torch.Tensor:
    """Temperature / top-k / top-p / min_p sampling; greedy where temperature
    == 0. min_p keeps {v : l[v] >= max l + T * ln(min_p)} of the unscaled
    logits l, i.e. probability >= min_p x the most likely token's, and is
    intersected with the top-k/top-p keep set."""
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.long, device=logits.device)
    greedy_mask = temperatures <= 0
    if greedy_mask.any():
        out[greedy_mask] = logits[greedy_mask].argmax(dim=-1)
    sample_idx = (~greedy_mask).nonzero(as_tuple=True)[0]
    for i in sample_idx.tolist():
        l = logits[i].float() / float(temperatures[i])
        drop = None
        if min_p is not None and float(min_p[i]) > 0:
            raw = logits[i].float()
            bound = raw.max() + temperatures[i].float() * torch.log(min_p[i].float())
            drop = raw < bound
        k = int(top_ks[i])
        if k > 0 and k < V:
            kth = torch.topk(l, k).values[-1]
            l = torch.where(l < kth, torch.full_like(l, float("-inf")), l)
        p = float(top_ps[i])
        if p < 1.0:
            sorted_l, sorted_i = torch.sort(l, descending=True)
            probs = torch.softmax(sorted_l, dim=-1)
            cum = torch.cumsum(probs, dim=-1)
            cut = (cum - probs) >= p  # keep tokens whose preceding mass < p
            sorted_l[cut] = float("-inf")
            l = torch.full_like(l, float("-inf")).scatter(0, sorted_i, sorted_l)
        if drop is not None:
            l = l.masked_fill(drop, float("-inf"))
        probs = torch.softmax(l, dim=-1)
        out[i] = torch.multinomial(probs, 1, generator=generator).squeeze(0)
    return out
