"""Decoder-only transformer covering the Llama / Mistral / Qwen2 / Qwen3 /
Gemma-2 families.

One functional implementation driven by ModelSpec switches (SURVEY §2.9:
the model set the reference serves through vLLM). Design notes, MI355X-first:

- Weights are plain tensors (no nn.Module graph): qkv packed into ONE GEMM
  [q+2kv, hidden], gate+up packed into ONE GEMM [2*inter, hidden] — fewer,
  larger hipBLASLt GEMMs (xGMI-budgeted TP shards stay big).
- Hot elementwise/normalisation ops go through llmq_amd.ops → hand-written
  CDNA4 kernels on GPU (fused residual+RMSNorm, fused RoPE q‖k, fused
  SiLU·mul / GeGLU, paged attention, KV scatter; Qwen3's per-head q/k norm
  is fused into the RoPE + cache-write launch).
- Tensor parallelism: column-shard qkv & gate_up, row-shard o & down with a
  single RCCL all-reduce after each of the two row GEMMs per layer (the
  standard 2-allreduce/layer Megatron split; over 7×153 GB/s xGMI links the
  payloads at decode batch sizes are latency-bound, so fewer+larger
  collectives win — SURVEY §2.9 TP note).
"""

from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Union

import torch
import torch.nn.functional as F

from llmq_amd import ops
from llmq_amd.ops import torch_ref
from llmq_amd.engine.forward_meta import DecodeMeta, MixedMeta, PrefillMeta
from llmq_amd.engine.kv_cache import KVCache
from llmq_amd.engine.model_specs import ModelSpec
from llmq_amd.parallel import get_tp_group


# Decode projection GEMMs through the hand-written skinny-M kernel
# (ops.skinny_gemm) instead of hipBLASLt. Opt-in while A/B-ing
# (LLMQ_SKINNY_GEMM=1); shapes outside the kernel's envelope fall back.
_USE_SKINNY_GEMM = os.environ.get("LLMQ_SKINNY_GEMM", "0") not in ("0", "false", "")


def _proj(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    if (_USE_SKINNY_GEMM and x.is_cuda and x.dtype == torch.bfloat16
            and x.shape[0] <= 1024 and w.shape[1] % 64 == 0
            and w.shape[0] % 4 == 0):
        return ops.skinny_gemm(x, w, bias)
    return F.linear(x, w, bias)


# The four projection weights of a layer: the tensors quantization="fp8"
# stores as float8_e4m3fn [N, K] with an fp32 per-output-channel scale [N]
# in LayerWeights.<name>_scale.
LINEARS = ("qkv", "o", "gate_up", "down")


class LayerWeights:
    __slots__ = (
        "input_norm", "qkv", "qkv_bias", "q_norm", "k_norm", "o", "post_attn_norm",
        "pre_mlp_norm", "gate_up", "down", "post_mlp_norm",
        "qkv_scale", "o_scale", "gate_up_scale", "down_scale",
    )

    def __init__(self):
        self.qkv_scale = None
        self.o_scale = None
        self.gate_up_scale = None
        self.down_scale = None
        self.input_norm = None
        self.qkv = None
        self.qkv_bias = None
        self.q_norm = None
        self.k_norm = None
        self.o = None
        self.post_attn_norm = None
        self.pre_mlp_norm = None
        self.gate_up = None
        self.down = None
        self.post_mlp_norm = None


class CausalLM:
    def __init__(
        self,
        spec: ModelSpec,
        device: torch.device,
        dtype: torch.dtype,
        tp_rank: int = 0,
        tp_size: int = 1,
        quantization: Optional[str] = None,
    ):
        if quantization not in (None, "fp8"):
            raise ValueError(f"unknown quantization {quantization!r}")
        self.fp8 = quantization == "fp8"
        self.spec = spec
        self.device = device
        self.dtype = dtype
        self.tp_rank = tp_rank
        self.tp_size = tp_size
        if spec.num_heads % tp_size or spec.num_kv_heads % max(
            1, min(tp_size, spec.num_kv_heads)
        ):
            raise ValueError(
                f"num_heads={spec.num_heads} not divisible by tp_size={tp_size}"
            )
        self.heads = spec.num_heads // tp_size
        # KV heads replicate when tp_size > num_kv_heads is not supported; shard.
        if spec.num_kv_heads % tp_size:
            raise ValueError(
                f"num_kv_heads={spec.num_kv_heads} not divisible by tp_size={tp_size}"
            )
        self.kv_heads = spec.num_kv_heads // tp_size
        self.q_size = self.heads * spec.head_dim
        self.kv_size = self.kv_heads * spec.head_dim
        self.inter = spec.intermediate_size // tp_size
        if spec.intermediate_size % tp_size:
            raise ValueError("intermediate_size not divisible by tp_size")
        # Gemma norms use the (1 + w) convention.
        self.norm_offset = 1.0 if spec.family == "gemma2" else 0.0

        self.embedding: Optional[torch.Tensor] = None
        self.layers: List[LayerWeights] = []
        self.final_norm: Optional[torch.Tensor] = None
        self.lm_head: Optional[torch.Tensor] = None
        self.rope_cache = ops.build_rope_cache(
            spec.max_position_embeddings, spec.head_dim, spec.rope_theta, device,
            rope_scaling=spec.rope_scaling,
        )
        self._alloc()

    # -- weights ---------------------------------------------------------

    def _empty(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, device=self.device, dtype=self.dtype)

    def linear_shape(self, name: str) -> tuple:
        """[N, K] of this rank's shard of a layer projection."""
        h = self.spec.hidden_size
        return {
            "qkv": (self.q_size + 2 * self.kv_size, h),
            "o": (h, self.q_size),
            "gate_up": (2 * self.inter, h),
            "down": (h, self.inter),
        }[name]

    def _empty_linear(self, name: str) -> Optional[torch.Tensor]:
        # fp8: no storage in the compute dtype; set_linear installs the
        # quantised tensor, one projection at a time
        return None if self.fp8 else self._empty(*self.linear_shape(name))

    @torch.no_grad()
    def set_linear(self, lw: LayerWeights, name: str, src: torch.Tensor) -> None:
        """Install this rank's shard `src` [N, K] (any dtype or device) as
        projection `name` of `lw`. Under fp8 it is quantised here, after
        sharding, so a row-sharded projection gets scales over its local K;
        the copy in the compute dtype lives only inside this call, and the
        model never holds two full sets of weights."""
        if tuple(src.shape) != self.linear_shape(name):
            raise ValueError(
                f"shape mismatch: {self.linear_shape(name)} vs {tuple(src.shape)}")
        if not self.fp8:
            getattr(lw, name).copy_(src.to(self.dtype))
            return
        w = src.to(device=self.device, dtype=torch.bfloat16)
        w_q, w_scale = torch_ref.quant_fp8_weight(w)
        setattr(lw, name, w_q)
        setattr(lw, name + "_scale", w_scale)

    def _alloc(self) -> None:
        s = self.spec
        self.embedding = self._empty(s.vocab_size, s.hidden_size)
        for _ in range(s.num_layers):
            lw = LayerWeights()
            lw.input_norm = self._empty(s.hidden_size)
            lw.qkv = self._empty_linear("qkv")
            if s.qkv_bias:
                lw.qkv_bias = self._empty(self.q_size + 2 * self.kv_size)
            if s.qk_norm:
                lw.q_norm = self._empty(s.head_dim)
                lw.k_norm = self._empty(s.head_dim)
            lw.o = self._empty_linear("o")
            lw.pre_mlp_norm = self._empty(s.hidden_size)
            lw.gate_up = self._empty_linear("gate_up")
            lw.down = self._empty_linear("down")
            if s.post_norms:
                lw.post_attn_norm = self._empty(s.hidden_size)
                lw.post_mlp_norm = self._empty(s.hidden_size)
            self.layers.append(lw)
        self.final_norm = self._empty(s.hidden_size)
        self.lm_head = self.embedding if s.tied_embeddings else self._empty(
            s.vocab_size, s.hidden_size
        )

    @torch.no_grad()
    def random_init(self, seed: int = 0, fast: bool = False) -> None:
        """Random weights for synthetic benchmarking (no network for real
        checkpoints here). Scaled so activations stay finite in bf16.

        fast=True generates on-device (needed for multi-B-param models:
        host-side generation of a 9B model costs ~40 s); fast=False uses a
        CPU generator so CPU and GPU engines with the same seed get
        bit-identical weights (consistency tests)."""
        if fast and self.device.type == "cuda":
            gen = torch.Generator(device=self.device).manual_seed(seed)

            def fill(t: torch.Tensor, std: float) -> None:
                t.normal_(0.0, std, generator=gen)
        else:
            gen = torch.Generator(device="cpu").manual_seed(seed)

            def fill(t: torch.Tensor, std: float) -> None:
                cpu = torch.randn(t.shape, generator=gen, dtype=torch.float32) * std
                t.copy_(cpu.to(t.dtype))

        def fill_linear(lw: LayerWeights, name: str, std: float) -> None:
            if not self.fp8:
                fill(getattr(lw, name), std)
                return
            # the tensor the unquantised model would hold, then its fp8 form
            w = self._empty(*self.linear_shape(name))
            fill(w, std)
            self.set_linear(lw, name, w)

        h = self.spec.hidden_size
        std = 0.02
        out_std = std / math.sqrt(2 * self.spec.num_layers)
        fill(self.embedding, std)
        for lw in self.layers:
            lw.input_norm.fill_(1.0 - self.norm_offset)
            fill_linear(lw, "qkv", std)
            if lw.qkv_bias is not None:
                lw.qkv_bias.zero_()
            if lw.q_norm is not None:
                lw.q_norm.fill_(1.0)
                lw.k_norm.fill_(1.0)
            fill_linear(lw, "o", out_std)
            lw.pre_mlp_norm.fill_(1.0 - self.norm_offset)
            fill_linear(lw, "gate_up", std)
            fill_linear(lw, "down", out_std)
            if lw.post_attn_norm is not None:
                lw.post_attn_norm.fill_(1.0 - self.norm_offset)
                lw.post_mlp_norm.fill_(1.0 - self.norm_offset)
        self.final_norm.fill_(1.0 - self.norm_offset)
        if not self.spec.tied_embeddings:
            fill(self.lm_head, std)

    def named_tensors(self) -> Dict[str, torch.Tensor]:
        out = {"embedding": self.embedding, "final_norm": self.final_norm}
        if not self.spec.tied_embeddings:
            out["lm_head"] = self.lm_head
        for i, lw in enumerate(self.layers):
            p = f"layers.{i}."
            out[p + "input_norm"] = lw.input_norm
            out[p + "qkv"] = lw.qkv
            if lw.qkv_bias is not None:
                out[p + "qkv_bias"] = lw.qkv_bias
            if lw.q_norm is not None:
                out[p + "q_norm"] = lw.q_norm
                out[p + "k_norm"] = lw.k_norm
            out[p + "o"] = lw.o
            out[p + "pre_mlp_norm"] = lw.pre_mlp_norm
            out[p + "gate_up"] = lw.gate_up
            out[p + "down"] = lw.down
            if lw.post_attn_norm is not None:
                out[p + "post_attn_norm"] = lw.post_attn_norm
                out[p + "post_mlp_norm"] = lw.post_mlp_norm
            if self.fp8:
                for name in LINEARS:
                    out[p + name + "_scale"] = getattr(lw, name + "_scale")
        return out

    def weight_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.named_tensors().values())

    # -- forward ---------------------------------------------------------

    def _norm(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        return ops.rmsnorm(x, w, self.spec.rms_eps, self.norm_offset)

    # Under fp8 the input of every layer projection travels as a pair
    # (q [T, K] float8_e4m3fn, scale [T] fp32) from the kernel that produced
    # it (a fused norm, the gated activation, or quant_fp8_rows after
    # attention) to the fp8 GEMM; otherwise it is the plain tensor.

    def _linear(self, h, lw: LayerWeights, name: str, bias=None) -> torch.Tensor:
        w = getattr(lw, name)
        if self.fp8:
            return ops.fp8_linear(h[0], h[1], w, getattr(lw, name + "_scale"), bias)
        return _proj(h, w, bias)

    def _add_norm(self, x, residual, w_post, w, quant: bool):
        """residual += x (Gemma-2: += norm(x, w_post)); h = norm(residual, w).
        Returns (h, residual), h quantised when `quant`."""
        s = self.spec
        if s.post_norms:
            # Gemma-2 sandwich fused
            if quant:
                q, scale, residual = ops.norm_add_norm_quant_fp8(
                    x, residual, w_post, w, s.rms_eps, self.norm_offset)
                return (q, scale), residual
            return ops.norm_add_norm(
                x, residual, w_post, w, s.rms_eps, self.norm_offset,
            )
        if quant:
            q, scale, residual = ops.fused_add_rmsnorm_quant_fp8(
                x, residual, w, s.rms_eps, self.norm_offset)
            return (q, scale), residual
        return ops.fused_add_rmsnorm(x, residual, w, s.rms_eps, self.norm_offset)

    def _prefill_attn(self, q, k, v, pmeta, kv_cache, layer: int, window: int):
        """Packed varlen attention; chunk continuations assemble their full
        context (gathered past from the paged cache + fresh rows)."""
        s = self.spec
        g = pmeta.gather
        if g is None:
            return ops.varlen_prefill_attention(
                q, k, v, pmeta.cu_seqlens, pmeta.max_seqlen, s.scale,
                s.attn_softcap, window,
            )
        ti = g.torch_indices
        if ti is None:
            k_att, v_att = ops.gather_paged_kv(
                kv_cache.k[layer], kv_cache.v[layer], k, v, g.block_tables,
                pmeta.cu_seqlens, g.cu_seqlens_k, g.total_k, g.max_seqlen_k,
            )
        else:  # LLMQ_PAGED_GATHER=0: the torch composition (A/B, bisection)
            KVH, D = k.shape[1], k.shape[2]
            k_att = q.new_empty(g.total_k, KVH, D)
            v_att = q.new_empty(g.total_k, KVH, D)
            past_k = kv_cache.k[layer][ti.blocks, :, ti.offs].to(q.dtype)
            past_v = kv_cache.v[layer][ti.blocks, :, ti.offs].to(q.dtype)
            k_att.index_copy_(0, ti.past_dst, past_k)
            v_att.index_copy_(0, ti.past_dst, past_v)
            k_att.index_copy_(0, ti.fresh_dst, k)
            v_att.index_copy_(0, ti.fresh_dst, v)
        return ops.varlen_prefill_attention(
            q, k_att, v_att, pmeta.cu_seqlens, pmeta.max_seqlen, s.scale,
            s.attn_softcap, window, cu_seqlens_k=g.cu_seqlens_k,
        )

    @torch.no_grad()
    def forward(
        self,
        input_ids: torch.Tensor,  # [T]
        positions: torch.Tensor,  # [T]
        kv_cache: KVCache,
        meta: Union[PrefillMeta, DecodeMeta, MixedMeta],
    ) -> torch.Tensor:
        s = self.spec
        tp = get_tp_group() if self.tp_size > 1 else None
        x = F.embedding(input_ids, self.embedding)
        if s.embedding_scale:
            x = x * math.sqrt(s.hidden_size)
            x = x.to(self.dtype)
        residual = x
        fp8 = self.fp8
        if fp8:
            h = ops.rmsnorm_quant_fp8(
                x, self.layers[0].input_norm, s.rms_eps, self.norm_offset)
        else:
            h = self._norm(x, self.layers[0].input_norm)
        n_layers = len(self.layers)
        for i, lw in enumerate(self.layers):
            # ---- attention block (h = normed input, set by the previous
            # block's fused norm — launch count is the decode-step bound)
            qkv = self._linear(h, lw, "qkv", lw.qkv_bias)
            q, k, v = qkv.split([self.q_size, self.kv_size, self.kv_size], dim=-1)
            T = q.shape[0]
            q = q.view(T, self.heads, s.head_dim)
            k = k.view(T, self.kv_heads, s.head_dim)
            v = v.view(T, self.kv_heads, s.head_dim)
            if s.qk_norm:
                ops.qknorm_rope_and_cache(
                    q, k, v, kv_cache.k[i], kv_cache.v[i], lw.q_norm,
                    lw.k_norm, s.rms_eps, 0.0, positions, self.rope_cache,
                    meta.slot_mapping,
                )
            else:
                ops.rope_and_cache(
                    q, k, v, kv_cache.k[i], kv_cache.v[i], positions,
                    self.rope_cache, meta.slot_mapping,
                )
            window = s.sliding_window if s.layer_uses_sliding_window(i) else 0
            if meta.is_prefill:
                attn = self._prefill_attn(q, k, v, meta, kv_cache, i, window)
            elif meta.is_mixed:
                # per-segment attention; GEMMs/norms already ran packed
                nd = meta.n_decode
                attn_d = ops.paged_decode_attention(
                    q[:nd], kv_cache.k[i], kv_cache.v[i],
                    meta.decode.block_tables, meta.decode.context_lens,
                    s.scale, s.attn_softcap, window,
                )
                attn_p = self._prefill_attn(
                    q[nd:], k[nd:], v[nd:], meta.prefill, kv_cache, i, window
                )
                attn = torch.cat([attn_d, attn_p], dim=0)
            else:
                attn = ops.paged_decode_attention(
                    q, kv_cache.k[i], kv_cache.v[i], meta.block_tables,
                    meta.context_lens, s.scale, s.attn_softcap, window,
                )
            attn = attn.reshape(T, self.q_size)
            attn_out = self._linear(
                ops.quant_fp8_rows(attn) if fp8 else attn, lw, "o")
            if tp is not None:
                attn_out = tp.all_reduce(attn_out)
            # residual += attn_out (Gemma-2: its post norm); h = norm(residual)
            h, residual = self._add_norm(
                attn_out, residual, lw.post_attn_norm, lw.pre_mlp_norm, fp8)
            # ---- MLP block
            gate_up = self._linear(h, lw, "gate_up")
            if fp8:
                act = (ops.gelu_tanh_and_mul_quant_fp8(gate_up) if s.gelu
                       else ops.silu_and_mul_quant_fp8(gate_up))
            else:
                act = ops.gelu_tanh_and_mul(gate_up) if s.gelu else ops.silu_and_mul(gate_up)
            mlp_out = self._linear(act, lw, "down")
            if tp is not None:
                mlp_out = tp.all_reduce(mlp_out)
            # The next block's input norm (or the final norm) fuses with this
            # block's residual add (+ post norm for Gemma-2).
            w_next = (
                self.layers[i + 1].input_norm if i + 1 < n_layers else self.final_norm
            )
            # The last block's output feeds the bf16 lm_head: not quantised.
            h, residual = self._add_norm(
                mlp_out, residual, lw.post_mlp_norm, w_next,
                fp8 and i + 1 < n_layers)
        return h

    @torch.no_grad()
    def lm_head_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        """hidden [N, hidden] → the lm_head GEMM's output [N, vocab] in the
        model dtype: not widened, final soft-cap NOT applied. For the fused
        GPU sampler, which does both on the values it loads."""
        return _proj(hidden, self.lm_head)

    @torch.no_grad()
    def compute_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        """hidden [N, hidden] → logits [N, vocab] (fp32)."""
        logits = _proj(hidden, self.lm_head).float()
        cap = self.spec.final_softcap
        if cap and cap > 0:
            logits = torch.tanh(logits / cap) * cap
        return logits
