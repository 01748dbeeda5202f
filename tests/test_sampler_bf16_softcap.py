"""Sampler kernels on the lm_head GEMM's bf16 logits with the final soft-cap
applied in registers.

`sample_gumbel_argmax` and `topk_topp_bound` take the logits as stored (bf16)
and a `softcap`; they must pick exactly the tokens / bounds of the eager tail

    l = logits.float(); l = torch.tanh(l / cap) * cap

followed by the fp32 op without a cap: `torch.equal`, no tolerance. Shapes
cover the 16-byte vector path with many splits, an odd row stride (scalar
head and tail), one and two splits with and without V % 8 == 0, and a batch
large enough for nsplit == 1. Inputs are seeded randn * 20 rounded to bf16, so
|x| / cap spans the curved part of tanh; the references are built once per
(shape, cap) and shared.

Which division matched: the kernel multiplies by the fp32 reciprocal
1.0f / cap formed on the host, as torch does for a Python-scalar divisor.
"""

from __future__ import annotations

import functools

import pytest
import torch

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

CAPS = (30.0, 50.0)
STEPS = range(1, 9)
SHAPES = (
    (16, 256000),  # vector path, many splits
    (3, 32003),    # odd row stride: scalar head and tail
    (1, 4104),     # multiple of 8; just over 4096, so two splits (2056 + 2048)
    (1, 4099),     # odd V, two splits (2056 + 2043)
    (1, 4096),     # multiple of 8, one split
    (1, 4091),     # odd V, one split
    (2048, 4104),  # nsplit == 1 because the batch is large
)
TEMPS = (0.0, 0.7, 1.3)


def split_rule(B: int, V: int):
    """Pure-Python mirror of the launcher's split rule: (nsplit, chunk)."""
    nsplit = 1
    while B * nsplit < 2048 and nsplit < 64 and (V // nsplit) > 4096:
        nsplit *= 2
    chunk = ((V + nsplit - 1) // nsplit + 7) // 8 * 8
    return nsplit, chunk


@functools.lru_cache(maxsize=None)
def _logits_cpu(B: int, V: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(B * 1000003 + V)
    return (torch.randn(B, V, generator=gen) * 20.0).to(torch.bfloat16)


def _capped(logits: torch.Tensor, cap: float) -> torch.Tensor:
    """Today's eager tail (CausalLM.compute_logits)."""
    l = logits.float()
    return torch.tanh(l / cap) * cap


@functools.lru_cache(maxsize=None)
def _case(B: int, V: int, cap: float):
    """bf16 logits and the capped fp32 reference on the GPU, made once per
    (shape, cap) and left unchanged."""
    dev = torch.device("cuda:0")
    raw = _logits_cpu(B, V).to(dev)
    return raw, _capped(raw, cap)


def _rows(B: int, dev):
    """Per-row temperatures mixed over TEMPS; every fourth row carries a
    request seed and an output position."""
    idx = torch.arange(B)
    temps = torch.tensor(TEMPS)[idx % 3].to(dev)
    seeds = torch.where(idx % 4 == 1, 1000 + idx, torch.zeros_like(idx))
    pos = (idx * 7) % 13
    return temps, seeds.to(torch.int32).to(dev), pos.to(torch.int32).to(dev)


def _sample(logits, temps, seeds, pos, step, bounds=None, softcap=None):
    from llmq_amd import ops

    B = logits.shape[0]
    out = torch.empty(B, dtype=torch.int64, device=logits.device)
    keys = torch.empty(B, dtype=torch.int64, device=logits.device)
    if softcap is None:  # the call as it was before the op took a cap
        ops.sample_gumbel_argmax(out, keys, logits, temps, seeds, pos, 1234,
                                 step, bounds)
    else:
        ops.sample_gumbel_argmax(out, keys, logits, temps, seeds, pos, 1234,
                                 step, bounds, softcap)
    return out.clone()


# ------------------------------------------------- CPU preconditions --


@pytest.mark.parametrize("B,V", SHAPES + ((512, 256000), (1, 8), (7, 131)))
def test_split_rule_covers_row_once(B, V):
    nsplit, chunk = split_rule(B, V)
    assert chunk % 8 == 0 and chunk > 0
    covered = []
    for y in range(nsplit):
        v0 = y * chunk
        if v0 >= V:
            continue  # the kernel returns at once for such a split
        covered.extend(range(v0, min(v0 + chunk, V)))
        if V % 8 == 0:
            assert v0 % 8 == 0  # 16-byte aligned start within a bf16 row
    assert covered == list(range(V))


def test_split_rule_hits_the_intended_paths():
    assert split_rule(16, 256000)[0] > 1
    assert split_rule(1, 4104) == (2, 2056) and split_rule(1, 4099) == (2, 2056)
    assert split_rule(1, 4096)[0] == 1 and split_rule(1, 4091)[0] == 1
    assert split_rule(2048, 4104)[0] == 1
    assert split_rule(3, 32003)[0] > 1 and 32003 % 8 != 0


@pytest.mark.parametrize("cap", CAPS)
def test_reference_transform_is_finite_and_curved(cap):
    raw = _logits_cpu(3, 32003)
    ref = _capped(raw, cap)
    assert bool(torch.isfinite(ref).all())
    assert float(ref.abs().max()) <= cap
    ratio = raw.float().abs() / cap
    # inputs reach the linear, the curved and the saturating part of tanh
    assert bool((ratio < 0.1).any()) and bool(((ratio > 0.5) & (ratio < 2)).any())
    assert bool((ratio > 1.5).any())


# ------------------------------------------------------ GPU: sampler --


@gpu
@needs_gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("B,V", SHAPES)
def test_bf16_softcap_tokens_equal_eager_tail(B, V, cap):
    raw, ref = _case(B, V, cap)
    temps, seeds, pos = _rows(B, raw.device)
    for step in STEPS:
        want = _sample(ref, temps, seeds, pos + step, step)
        got = _sample(raw, temps, seeds, pos + step, step, None, cap)
        assert torch.equal(got, want), (step, (got != want).nonzero().flatten()[:8])


@gpu
@needs_gpu
@pytest.mark.parametrize("B,V", SHAPES)
def test_bf16_without_cap_equals_fp32_path(B, V):
    raw, _ = _case(B, V, CAPS[0])
    wide = raw.float()
    temps, seeds, pos = _rows(B, raw.device)
    for step in STEPS:
        want = _sample(wide, temps, seeds, pos, step)
        assert torch.equal(_sample(raw, temps, seeds, pos, step, None, 0.0), want)
        assert torch.equal(_sample(raw, temps, seeds, pos, step), want)


@gpu
@needs_gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("V", [4099, 256000])
def test_saturated_row_ties_go_to_lowest_index(V, cap):
    """Every logit at +-400: tanh saturates (exactly +-1 at cap 30) and all
    maxima tie."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(V)
    signs = torch.where(torch.rand(V, generator=gen) < 0.5, -1.0, 1.0)
    signs[:3] = -1.0
    raw = torch.stack([signs * 400.0, torch.full((V,), 400.0),
                       -signs * 400.0]).to(torch.bfloat16).to(dev)
    ref = _capped(raw, cap)
    assert ref.abs().unique().numel() == 1  # the whole row ties
    first = torch.tensor([int((signs > 0).nonzero()[0]), 0, 0], device=dev)
    zeros = torch.zeros(3, dtype=torch.int32, device=dev)
    greedy = torch.zeros(3, device=dev)
    want = _sample(ref, greedy, zeros, zeros, 1)
    got = _sample(raw, greedy, zeros, zeros, 1, None, cap)
    assert torch.equal(want, first) and torch.equal(got, first)
    warm = torch.full((3,), 0.7, device=dev)
    for step in STEPS:
        assert torch.equal(_sample(raw, warm, zeros, zeros, step, None, cap),
                           _sample(ref, warm, zeros, zeros, step))


# ------------------------------------------------- GPU: top-k / top-p --


@gpu
@needs_gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("B,V", [(16, 256000), (3, 32003), (1, 4099)])
def test_bound_and_truncated_sampling_equal_eager_tail(B, V, cap):
    from llmq_amd import ops

    raw, ref = _case(B, V, cap)
    dev = raw.device
    idx = torch.arange(B)
    temps = torch.tensor((0.7, 1.3))[idx % 2].to(dev)
    tks = torch.where(idx % 2 == 0, 5, 0).to(torch.int64).to(dev)   # top-k 5 rows
    tps = torch.where(idx % 2 == 0, 1.0, 0.9).to(dev)               # top-p 0.9 rows
    want_b = ops.topk_topp_bound(ref, temps, tps, tks)
    got_b = ops.topk_topp_bound(raw, temps, tps, tks, cap)
    assert torch.equal(got_b, want_b), (got_b, want_b)
    assert bool((got_b > -1e30).all())  # every row is really truncated
    _, seeds, pos = _rows(B, dev)
    for step in STEPS:
        want = _sample(ref, temps, seeds, pos, step, want_b)
        got = _sample(raw, temps, seeds, pos, step, got_b, cap)
        assert torch.equal(got, want), step
        assert bool((ref.gather(1, got[:, None])[:, 0] >= got_b).all())


# ------------------------------------------------------- GPU: engine --


@gpu
@needs_gpu
def test_engine_tokens_equal_with_and_without_fused_tail(monkeypatch):
    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine
    from llmq_amd.engine.sampling_params import SamplingParams

    def run(flag):
        if flag is None:
            monkeypatch.delenv("LLMQ_FUSED_LOGIT_TAIL", raising=False)
        else:
            monkeypatch.setenv("LLMQ_FUSED_LOGIT_TAIL", flag)
        eng = LLMEngine(EngineConfig(
            model="tiny-gemma2", max_num_seqs=4, max_model_len=256,
            load_weights=False, num_kv_blocks=128, seed=7,
        ))
        assert eng.runner.use_graphs
        assert eng.runner.fused_logit_tail == (flag is None)
        params = SamplingParams(temperature=0.7, max_tokens=24, ignore_eos=True)
        for i in range(4):
            eng.add_request(f"r{i}", prompt=f"request number {i}", params=params)
        tokens = {}
        while eng.has_unfinished():
            for out in eng.step():
                tokens.setdefault(out.request_id, []).extend(out.new_token_ids)
        del eng
        torch.cuda.empty_cache()
        return tokens

    old = run("0")
    new = run(None)
    assert sorted(old) == [f"r{i}" for i in range(4)]
    assert all(len(v) == 24 for v in old.values())
    assert old == new
