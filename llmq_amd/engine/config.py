"""Engine configuration (the AsyncEngineArgs analogue)."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import torch


@dataclass
class EngineConfig:
    model: str = "tiny-llama"
    dtype: str = "bfloat16"  # compute dtype on GPU; float32 on CPU
    max_num_seqs: int = 256
    max_model_len: Optional[int] = None
    max_prefill_tokens: int = 8192  # token budget per prefill step
    gpu_memory_utilization: float = 0.9
    kv_block_size: int = 16
    # "auto" = model dtype; "fp8" = OCP e4m3 KV storage (bf16 compute) —
    # halves the decode KV stream; opt-in, off by default.
    kv_cache_dtype: str = "auto"
    enable_hipgraph: bool = True
    hipgraph_max_batch: int = 512
    tensor_parallel_size: int = 1
    seed: int = 0
    device: str = "auto"  # "auto" | "cuda" | "cpu"
    load_weights: bool = True  # False → random init (synthetic benchmarking)
    fast_init: bool = False  # device-side random init (large models)
    # CPU-test override: number of KV blocks (None → sized from free HBM)
    num_kv_blocks: Optional[int] = None
    enforce_eager: bool = False
    # Automatic prefix caching: full KV blocks of finished/running prompts
    # are kept and shared with later prompts that start with the same tokens.
    enable_prefix_caching: bool = False
    # Cascade decode attention for batches that share a prompt prefix: the
    # blocks common to every sequence of a decode step are attended once per
    # 128 query rows instead of once per sequence. Needs prefix caching (that
    # is what makes the blocks common). Opt-in.
    shared_prefix_decode: bool = False
    # "none" = weights in the compute dtype; "fp8" = W8A8: the layer
    # projection weights stored as OCP e4m3 with a per-output-channel scale,
    # activations quantised per row on the fly, fp8 GEMMs. "mxfp4" = W4A8:
    # the same fp8 activations against OCP MXFP4 weights (4.25 bits each)
    # through the scaled-MFMA GEMM; projections outside that kernel's
    # envelope stay fp8. Opt-in.
    quantization: str = "none"
    # Multi-LoRA: adapter name -> PEFT directory (adapter_config.json +
    # adapter_model.safetensors). All adapters stay resident; a request picks
    # one with SamplingParams.lora. Ranks up to max_lora_rank. Not with
    # quantization or tensor parallelism, and on the CPU path only: there are
    # no HIP kernels for it yet, and a GPU engine refuses the setting.
    lora_adapters: Dict[str, str] = field(default_factory=dict)
    max_lora_rank: int = 64

    def __post_init__(self) -> None:
        self._check_quantization()
        if self.lora_adapters:
            if self.quantization != "none":
                raise ValueError(
                    "lora_adapters cannot be combined with quantization="
                    f"{self.quantization!r} (adapters need unquantised projections)")
            if self.tensor_parallel_size > 1:
                raise ValueError(
                    "lora_adapters cannot be combined with tensor_parallel_size > 1")
            if not 1 <= self.max_lora_rank <= 64:
                raise ValueError("max_lora_rank must be in [1, 64]")
        if self.shared_prefix_decode and not self.enable_prefix_caching:
            raise ValueError("shared_prefix_decode requires enable_prefix_caching")

    def _check_quantization(self) -> None:
        if self.quantization not in ("none", "fp8", "mxfp4"):
            raise ValueError(
                f"unknown quantization {self.quantization!r} "
                "(expected 'none', 'fp8' or 'mxfp4')"
            )

    def resolve_quantization(self, device: torch.device) -> Optional[str]:
        """None, or "fp8" / "mxfp4" after checking that the device can run
        it: the quantised GEMMs need bf16 compute on the GPU; on CPU the fp32
        fake-quant reference path runs."""
        self._check_quantization()
        if self.quantization == "none":
            return None
        if device.type == "cuda" and self.resolve_dtype(device) != torch.bfloat16:
            raise ValueError(
                f"quantization={self.quantization} requires bf16 execution on GPU")
        return self.quantization

    def resolve_device(self) -> torch.device:
        if self.device == "auto":
            return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        return torch.device(self.device)

    def resolve_kv_dtype(self, device: torch.device) -> torch.dtype:
        model_dtype = self.resolve_dtype(device)
        if self.kv_cache_dtype == "auto":
            return model_dtype
        if self.kv_cache_dtype == "fp8":
            if device.type != "cuda" or model_dtype != torch.bfloat16:
                raise ValueError("kv_cache_dtype=fp8 requires GPU bf16 execution")
            return torch.float8_e4m3fn
        raise ValueError(f"unknown kv_cache_dtype {self.kv_cache_dtype!r}")

    def resolve_dtype(self, device: torch.device) -> torch.dtype:
        if device.type == "cpu":
            return torch.float32
        return {
            "bfloat16": torch.bfloat16,
            "bf16": torch.bfloat16,
            "float16": torch.float16,
            "fp16": torch.float16,
            "float32": torch.float32,
        }[self.dtype]
