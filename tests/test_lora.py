"""Multi-LoRA on the CPU path: contract, loader, request path, prefix cache."""

import pytest
import torch

from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.forward_meta import PrefillMeta
from llmq_amd.engine.lora import PROJ_MODULES, LoraError, proj_slices
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.ops import torch_ref
from llmq_amd.utils.tiny_checkpoint import build_tiny_lora_adapter

TOKENS = [1, 7, 42, 99, 123, 250, 3, 17, 300]


def make_engine(model="tiny-llama", **kw):
    return LLMEngine(EngineConfig(
        model=model, device="cpu", enforce_eager=True, load_weights=False, seed=3,
        max_num_seqs=4, max_model_len=128, num_kv_blocks=64, **kw))


def prefill_logits(engine, lora_rows=None):
    n, bs = len(TOKENS), engine.config.kv_block_size
    meta = PrefillMeta(
        cu_seqlens=torch.tensor([0, n], dtype=torch.int32), max_seqlen=n,
        slot_mapping=torch.arange(n, dtype=torch.long) + bs,
        lora=None if lora_rows is None else torch_ref.lora_meta(lora_rows, 2))
    hidden = engine.model.forward(
        torch.tensor(TOKENS), torch.arange(n), engine.kv_cache, meta)
    return engine.model.compute_logits(hidden)


@pytest.mark.parametrize("model", ["tiny-llama", "tiny-qwen3", "tiny-gemma2"])
def test_adapter_equals_merged_weights(tmp_path, model):
    """W + scale * B A merged from the file, at test_hf_parity's fp32 tolerance."""
    from safetensors.torch import load_file
    a = build_tiny_lora_adapter(tmp_path / "a", model, rank=4, seed=1,
                                target_modules=("q_proj", "down_proj"))
    b = build_tiny_lora_adapter(tmp_path / "b", model, rank=16, alpha=8.0, seed=2,
                                use_rslora=True)
    eng = make_engine(model, lora_adapters={"a": a, "b": b})
    ours = prefill_logits(eng, [1] * len(TOKENS))
    merged = make_engine(model)
    tensors, scale = load_file(b + "/adapter_model.safetensors"), 8.0 / 16 ** 0.5
    for i, lw in enumerate(merged.model.layers):
        for proj, modules in PROJ_MODULES.items():
            for module, (start, width) in zip(modules, proj_slices(merged.model, proj)):
                key = f"base_model.model.model.layers.{i}.{module}."
                getattr(lw, proj)[start:start + width] += scale * (
                    tensors[key + "lora_B.weight"] @ tensors[key + "lora_A.weight"])
    ref = prefill_logits(merged)
    base = prefill_logits(make_engine(model))
    tol = 1e-3 * max(1.0, ref.abs().max().item())
    assert (ours - ref).abs().max().item() < tol < 0.1 * (base - ref).abs().max().item()
    assert torch.equal(prefill_logits(eng, [-1] * len(TOKENS)), base)


@pytest.mark.parametrize("extra, match", [
    (dict(use_dora=True), "DoRA"),
    (dict(bias="all"), "bias"),
    (dict(modules_to_save=["lm_head"]), "modules_to_save"),
    (dict(rank_pattern={"q_proj": 4}), "rank_pattern"),
    (dict(alpha_pattern={"q_proj": 4}), "alpha_pattern"),
    (dict(target_modules=["q_proj", "embed_tokens", "lm_head"]), "embed_tokens.*lm_head"),
    (dict(r=128), "rank 128"),
])
def test_loader_rejects(tmp_path, extra, match):
    path = build_tiny_lora_adapter(tmp_path / "x", "tiny-llama", **extra)
    with pytest.raises(LoraError, match=match):
        make_engine(lora_adapters={"x": path})


def test_rejects_shape_mismatch_bad_configs_and_unknown_names(tmp_path):
    path = build_tiny_lora_adapter(tmp_path / "x", "tiny-llama-d128")
    with pytest.raises(LoraError, match="base model needs"):
        make_engine(lora_adapters={"x": path})
    with pytest.raises(ValueError, match="quantization"):
        EngineConfig(lora_adapters={"x": path}, quantization="fp8")
    with pytest.raises(ValueError, match="tensor_parallel_size"):
        EngineConfig(lora_adapters={"x": path}, tensor_parallel_size=2)
    eng = make_engine(lora_adapters={"x": build_tiny_lora_adapter(tmp_path / "y", "tiny-llama")})
    with pytest.raises(ValueError, match="unknown LoRA adapter 'y'"):
        eng.add_request("r", prompt_token_ids=TOKENS, params=SamplingParams(lora="y"))
    eng.add_request("r", prompt_token_ids=TOKENS, params=SamplingParams(lora="x"))
    assert eng._seqs["r"].lora == "x"


def test_prefix_cache_is_keyed_by_adapter(tmp_path):
    paths = {n: build_tiny_lora_adapter(tmp_path / n, "tiny-llama", seed=i, std=0.3)
             for i, n in enumerate("ab")}
    prompt = [(5 * i) % 500 + 3 for i in range(70)]
    params = {n: SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True, lora=n)
              for n in ("a", "b", None)}

    def run(eng, order):
        cached, toks = [], {}
        for i, n in enumerate(order):
            eng.add_request(f"r{i}", prompt_token_ids=prompt, params=params[n])
            while eng.has_unfinished():
                for o in eng.step():
                    toks.setdefault(i, []).extend(o.new_token_ids)
                    if o.finished:
                        cached.append(o.cached_tokens)
        return cached, toks
    order = ["a", "b", None, "a"]  # only the last one hits
    cached, toks = run(make_engine(lora_adapters=paths, enable_prefix_caching=True), order)
    assert cached == [0, 0, 0, 64]
    assert toks == run(make_engine(lora_adapters=paths), order)[1]  # as uncached
    assert toks[0] == toks[3] and len({tuple(toks[i]) for i in range(3)}) == 3


@pytest.mark.parametrize("widths", [(256, 64, 64), (128, 128), (192,)])
@pytest.mark.parametrize("pattern", ["one", "seg17", "mixed", "all", "none"])
def test_bf16_contract_exact_integers(pattern, widths):
    """Integers <= 228 are exact in bf16: lora_apply equals fp64 bit for bit,
    and a slip in ranks, slices, strides or the row tiles is a wrong integer."""
    g = torch.Generator().manual_seed(0)
    mixed = [0] * 1 + [1] * 16 + [2] * 17 + [-1] * 66
    rows = {"one": [1], "seg17": [2] * 17, "none": [-1] * 17,
            "all": torch.randint(0, 3, (100,), generator=g).tolist(),
            "mixed": [mixed[i] for i in torch.randperm(100, generator=g).tolist()]}[pattern]
    K, R, T, S, N = 96, 64, len(rows), len(widths), sum(widths) + 16
    A, B = torch.zeros(3, S * R, K), torch.zeros(3, N, R)
    for a, r in enumerate((8, 16, 64)):
        for s in range(S):
            sign = torch.randint(0, 2, (r, 2), generator=g) * 2.0 - 1
            A[a, s * R:s * R + r].scatter_(1, torch.randint(0, K, (r, 2), generator=g), sign)
        B[a, :, :r] = torch.randint(-1, 2, (N, r), generator=g).float()
    x = torch.randint(-1, 2, (T, K + 8), generator=g).bfloat16()[:, :K]
    out0 = torch.randint(-100, 101, (T, N), generator=g).bfloat16()
    slices = tuple((sum(widths[:s]), widths[s]) for s in range(S))
    stacks = torch_ref.LoraStacks(A.bfloat16(), B.bfloat16(), torch.ones(3), slices)
    ref = out0.double().clone()
    for t, a in enumerate(rows):
        if a >= 0:
            h = A[a].double() @ x[t].double()
            for s, (st, w) in enumerate(slices):
                ref[t, st:st + w] += B[a, st:st + w].double() @ h[s * R:(s + 1) * R]
    got = torch_ref.lora_apply(out0.clone(), x, stacks, torch_ref.lora_meta(rows, 3))
    assert ref.abs().max() <= 228 and torch.equal(got.double(), ref)
    assert (pattern == "none") == torch.equal(got, out0)
