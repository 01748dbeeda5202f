"""PEFT LoRA adapter loading (HF layout -> the stacks ops.lora_apply reads).

Every configured adapter stays resident. Per layer projection (the packed
qkv / o / gate_up / down GEMMs of CausalLM) the adapters are stacked into one
ops.LoraStacks: A [n_adapters, S*R, K], B [n_adapters, N, R], scale
[n_adapters], with S the HF modules packed into the projection and R the
largest loaded rank. Smaller ranks and modules an adapter does not target are
zero padded, so every adapter of a batch has one shape.
"""

from __future__ import annotations

import json
import logging
import math
from pathlib import Path
from typing import Dict, List, Tuple

import torch

from llmq_amd import ops

logger = logging.getLogger(__name__)

# projection -> its HF modules, in packing order
PROJ_MODULES: Dict[str, Tuple[str, ...]] = {
    "qkv": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"),
    "o": ("self_attn.o_proj",),
    "gate_up": ("mlp.gate_proj", "mlp.up_proj"),
    "down": ("mlp.down_proj",),
}
TARGETS = tuple(m.split(".")[1] for mods in PROJ_MODULES.values() for m in mods)


class LoraError(ValueError):
    """An adapter this engine cannot serve."""


def proj_slices(model, name: str) -> Tuple[Tuple[int, int], ...]:
    """(column start, width) of each HF module in projection `name`."""
    if name == "qkv":
        widths = (model.q_size, model.kv_size, model.kv_size)
    elif name == "gate_up":
        widths = (model.inter, model.inter)
    else:
        widths = (model.linear_shape(name)[0],)
    out, start = [], 0
    for w in widths:
        out.append((start, w))
        start += w
    return tuple(out)


def read_adapter_config(name: str, path: Path, max_rank: int) -> dict:
    """adapter_config.json, checked against what lora_apply implements."""
    cfg_path = path / "adapter_config.json"
    if not cfg_path.is_file():
        raise LoraError(f"LoRA adapter {name!r}: no adapter_config.json under {path}")
    cfg = json.loads(cfg_path.read_text())

    def bad(why: str) -> LoraError:
        return LoraError(f"LoRA adapter {name!r} ({path}): {why}")

    if cfg.get("peft_type", "LORA") != "LORA":
        raise bad(f"peft_type {cfg.get('peft_type')!r} is not LORA")
    if cfg.get("use_dora"):
        raise bad("DoRA (use_dora) is not supported")
    if cfg.get("bias", "none") != "none":
        raise bad(f"bias={cfg['bias']!r} is not supported (only 'none')")
    if cfg.get("modules_to_save"):
        raise bad("modules_to_save is not supported")
    for key in ("rank_pattern", "alpha_pattern"):
        if cfg.get(key):
            raise bad(f"{key} is not supported (one rank and alpha per adapter)")
    targets = cfg.get("target_modules")
    if isinstance(targets, str) or not targets:
        raise bad(f"target_modules must be a list of module names, got {targets!r}")
    other = sorted(set(targets) - set(TARGETS))
    if other:
        raise bad(f"target modules {other} are not supported (embedding and "
                  f"lm_head adapters included); supported: {list(TARGETS)}")
    r = int(cfg.get("r", 0))
    if not 1 <= r <= max_rank:
        raise bad(f"rank {r} outside [1, max_lora_rank={max_rank}]")
    return cfg


def load_lora_adapters(model, adapters: Dict[str, str], max_rank: int) -> List[str]:
    """Load `adapters` (name -> PEFT directory) into model.lora, one
    {projection: LoraStacks} dict per layer, and return the adapter names in
    stack order."""
    from safetensors import safe_open  # noqa: PLC0415

    names = list(adapters)
    loaded = []
    for name in names:
        path = Path(adapters[name])
        cfg = read_adapter_config(name, path, max_rank)
        st = path / "adapter_model.safetensors"
        if not st.is_file():
            raise LoraError(f"LoRA adapter {name!r}: no adapter_model.safetensors under {path}")
        tensors = {}
        with safe_open(str(st), framework="pt", device="cpu") as sf:
            for key in sf.keys():
                tensors[key] = sf.get_tensor(key)
        r, alpha = int(cfg["r"]), float(cfg.get("lora_alpha", cfg["r"]))
        scale = alpha / math.sqrt(r) if cfg.get("use_rslora") else alpha / r
        loaded.append((name, r, scale, set(cfg["target_modules"]), tensors))

    R = max(r for _n, r, *_ in loaded)
    nA = len(loaded)
    dev, dtype = model.device, model.dtype
    scale_t = torch.tensor([s for _n, _r, s, *_ in loaded], dtype=torch.float32, device=dev)
    model.lora = []
    for i in range(len(model.layers)):
        layer = {}
        for proj, modules in PROJ_MODULES.items():
            N, K = model.linear_shape(proj)
            slices = proj_slices(model, proj)
            a = torch.zeros(nA, len(modules) * R, K, dtype=torch.float32)
            b = torch.zeros(nA, N, R, dtype=torch.float32)
            for ai, (name, r, _s, targets, tensors) in enumerate(loaded):
                for s, (module, (start, width)) in enumerate(zip(modules, slices)):
                    if module.split(".")[1] not in targets:
                        continue
                    key = f"base_model.model.model.layers.{i}.{module}."
                    try:
                        wa = tensors[key + "lora_A.weight"]
                        wb = tensors[key + "lora_B.weight"]
                    except KeyError as exc:
                        raise LoraError(
                            f"LoRA adapter {name!r}: missing tensor {exc.args[0]}") from None
                    if tuple(wa.shape) != (r, K) or tuple(wb.shape) != (width, r):
                        raise LoraError(
                            f"LoRA adapter {name!r}: layer {i} {module} has A "
                            f"{tuple(wa.shape)} / B {tuple(wb.shape)}, the base "
                            f"model needs A {(r, K)} / B {(width, r)}")
                    a[ai, s * R:s * R + r] = wa.float()
                    b[ai, start:start + width, :r] = wb.float()
            layer[proj] = ops.LoraStacks(
                a.to(device=dev, dtype=dtype), b.to(device=dev, dtype=dtype),
                scale_t, slices)
        model.lora.append(layer)
    logger.info("loaded %d LoRA adapter(s) %s, stacked rank %d", nA, names, R)
    return names
