"""ops.lm_head_logprobs (fused lm_head + log-sum-exp kernel) against fp64, and
the engine path that carries its values.

Exact cases: integer-valued bf16 inputs, so every fp32 partial sum is exact
and the reference logit is the fp64 product rounded to bf16 (max |l| <= 160);
LP_TOL as in test_logprobs_gpu.py. Each plants a logit of 128 in column V - 1
(the last tile walked) of the row whose target is column 0, far above that
row's other logits: a sum not rescaled when the max moves misses by orders of
magnitude."""

from __future__ import annotations

import functools

import pytest
import torch

from llmq_amd import ops
from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.sampling_params import SamplingParams

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

LP_TOL = 1e-4
# (R, K, V, nsplit, cap). R: M tail, second M tile; K: one step, odd count; V:
# under a tile, one tile, one-column tail, tiles + tail; nsplit: one walker, a
# split, more slices than tiles, 0 = auto.
EXACT = [
    (1, 64, 5, 1, 0.0),
    (255, 64, 256, 1, 30.0),
    (257, 192, 257, 1, 0.0),
    (257, 192, 1000, 1, 30.0),
    (257, 192, 1000, 3, 0.0),
    (1, 192, 257, 3, 0.0),
    (255, 64, 1000, 8, 30.0),
    (257, 64, 1000, 0, 0.0),
]


def _strided(values):  # a row-strided bf16 view (stride K + 8) on the GPU
    buf = torch.zeros(values.size(0), values.size(1) + 8, dtype=torch.bfloat16, device="cuda")
    return buf[:, :values.size(1)].copy_(values)


def _reference(l64, targets, cap):
    if cap > 0:
        l64 = torch.tanh(l64 / cap) * cap
    return l64.gather(1, targets.view(-1, 1))[:, 0] - torch.logsumexp(l64, dim=-1)


@functools.lru_cache(maxsize=None)
def _exact_case(R, K, V):
    gen = torch.Generator().manual_seed(R * 1000003 + K * 1009 + V)
    T = R + 7
    hidden = torch.randint(-1, 2, (T, K), generator=gen).float()
    w = torch.randint(-2, 3, (V, K), generator=gen).float()
    rows = torch.randint(0, T, (R,), generator=gen)  # repeats, any order
    hidden[rows[0]] = 1.0
    w[V - 1] = 0.0
    w[V - 1, :64] = 2.0  # l[0, V - 1] = 128
    l64 = (hidden[rows].double() @ w.double().T).to(torch.bfloat16).double()
    assert l64.abs().max() <= 160 and l64[0, V - 1] == 128 and l64[0, :V - 1].max() < 90
    # column 0, column V - 1 and the tail tile's first column, in every case
    special = torch.tensor([0, V - 1, (V - 1) // 256 * 256])
    targets = torch.randint(0, V, (max(R, 3),), generator=gen)
    targets[:3] = special
    runs = [targets] if R >= 3 else list(special.view(3, 1))
    return _strided(hidden), _strided(w), rows.cuda(), l64, runs


@pytest.mark.parametrize("R,K,V,nsplit,cap", EXACT)
def test_exact_inputs(R, K, V, nsplit, cap):
    hidden, w, rows, l64, runs = _exact_case(R, K, V)
    for targets in runs:
        lp = ops.lm_head_logprobs(hidden, w, rows, targets.cuda(), cap, nsplit=nsplit)
        err = (lp.double().cpu() - _reference(l64, targets, cap)).abs().max().item()
        print(f"R={R} K={K} V={V} nsplit={nsplit} cap={cap}: max err {err:.3e}")
        assert lp.dtype == torch.float32 and lp.shape == (R,) and err <= LP_TOL


def _derived_bound(a, b):
    """2 (2^-9 max|l| + K 2^-24 max sum_k |a||b|) + 1e-4 for l = a @ b^T."""
    a, b = a.double(), b.double()
    K = a.size(1)
    return (2 * (2.0 ** -9 * (a @ b.T).abs().max().item()
                 + K * 2.0 ** -24 * (a.abs() @ b.abs().T).max().item()) + 1e-4)


def test_random_inputs():
    """Against unrounded fp64 logits: each logit moves by at most half a bf16
    ulp plus the fp32 accumulation error; lse, pick and tanh are 1-Lipschitz."""
    R, K, V, cap = 257, 192, 1000, 30.0
    gen = torch.Generator().manual_seed(5)
    hidden = torch.randn(R + 7, K, generator=gen).to(torch.bfloat16)
    w = torch.randn(V, K, generator=gen).to(torch.bfloat16)
    rows = torch.randint(0, R + 7, (R,), generator=gen)
    targets = torch.randint(0, V, (R,), generator=gen)
    lp = ops.lm_head_logprobs(_strided(hidden), _strided(w), rows.cuda(), targets.cuda(), cap)
    want = _reference(hidden[rows].double() @ w.double().T, targets, cap)
    bound, err = _derived_bound(hidden[rows], w), (lp.double().cpu() - want).abs().max().item()
    print(f"random: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


PROMPTS = [[(37 * i + 11 * j) % 500 + 5 for j in range(n)] for i, n in enumerate((45, 23, 9))]


def test_engine_fused_equals_blocked_composition(monkeypatch):
    bounds, inner = [], ops.lm_head_logprobs

    def measured(hidden, w, rows, targets, **kw):
        assert ops.lm_head_logprobs_supported(hidden, w)
        bounds.append(_derived_bound(hidden[rows.long()].cpu(), w.cpu()))
        return inner(hidden, w, rows, targets, **kw)

    monkeypatch.setattr(ops, "lm_head_logprobs", measured)

    def run(fused, asked):
        monkeypatch.setenv("LLMQ_FUSED_PROMPT_LOGPROBS", fused)
        eng = LLMEngine(EngineConfig(
            model="tiny-gemma2", max_num_seqs=4, max_model_len=256,
            load_weights=False, num_kv_blocks=128, seed=7, max_prefill_tokens=32))
        for i, p in enumerate(PROMPTS):
            eng.add_request(f"r{i}", prompt_token_ids=p, params=SamplingParams(
                temperature=0.0, max_tokens=6, ignore_eos=True, prompt_logprobs=asked))
        final, tokens = {}, {}
        while eng.has_unfinished():
            for out in eng.step():
                tokens.setdefault(out.request_id, []).extend(out.new_token_ids)
                final[out.request_id] = out  # the last one is the finishing output
        return final, tokens

    (fused, tokens), (blocked, _), (plain, plain_tokens) = (
        run("1", True), run("0", True), run("1", False))
    assert tokens == plain_tokens and len(bounds) >= 4  # 45 tokens: two chunks
    for i, p in enumerate(PROMPTS):
        got, ref = fused[f"r{i}"].prompt_logprobs, blocked[f"r{i}"].prompt_logprobs
        assert [t for t, _ in got] == p and got[0][1] is None and ref[0][1] is None
        err = max(abs(a - b) for (_, a), (_, b) in zip(got[1:], ref[1:]))
        print(f"prompt {i}: max |fused - blocked| {err:.3e}, bound {max(bounds):.3e}")
        assert len(got) == len(ref) == len(p) and err <= max(bounds)
        assert plain[f"r{i}"].prompt_logprobs is None
