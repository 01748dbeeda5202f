"""GPU tests for the paged K/V gather kernel and the engine paths that run it
(chunked prefill, prefix-cache hits). Run with `pytest -m gpu` on an MI355X.
"""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from llmq_amd import ops
    from llmq_amd.ops import torch_ref
else:
    pytest.skip("no GPU", allow_module_level=True)

from llmq_amd.engine.config import EngineConfig  # noqa: E402
from llmq_amd.engine.engine import LLMEngine  # noqa: E402
from llmq_amd.engine.sampling_params import SamplingParams  # noqa: E402
from tests.test_prefix_cache import (  # noqa: E402
    GATHER_PARAMS, PROMPTS, drain, gather_case, run_prompts,
)

DEV = torch.device("cuda:0")


def _launch(c):
    assert ops.has_hip_ext()
    torch.ops.llmq_amd.gather_paged_kv(
        c["k_out"], c["v_out"], c["k_cache"], c["v_cache"], c["k_fresh"],
        c["v_fresh"], c["block_tables"], c["cu_seqlens"], c["cu_seqlens_k"],
        c["max_seqlen_k"])
    torch.cuda.synchronize()


# ---------------------------------------------------------------- kernel --


@pytest.mark.parametrize("D,dtype,cache_dtype", GATHER_PARAMS)
def test_kernel_bitwise_matches_torch_ref(D, dtype, cache_dtype):
    """bs = 16, KVH = 3; (P, Lq) = (0, 5), (16, 1), (37, 20) over shuffled
    block ids, (1, 33). Same seed on both devices: the CPU case is the GPU
    case's copy."""
    ref = gather_case(D, dtype, cache_dtype)
    torch_ref.gather_paged_kv(
        ref["k_out"], ref["v_out"], ref["k_cache"], ref["v_cache"],
        ref["k_fresh"], ref["v_fresh"], ref["block_tables"], ref["cu_seqlens"],
        ref["cu_seqlens_k"], ref["max_seqlen_k"])
    c = gather_case(D, dtype, cache_dtype, device=DEV)
    before = {n: c[n].clone() for n in ("k_cache", "v_cache", "qkv", "block_tables")}
    _launch(c)
    # every row, the sentinel rows after total_k included
    assert torch.equal(c["k_out"].cpu(), ref["k_out"])
    assert torch.equal(c["v_out"].cpu(), ref["v_out"])
    assert (c["k_out"][c["total_k"]:] == -7.0).all()
    assert (c["v_out"][c["total_k"]:] == -7.0).all()
    # the sentinel block behind the table's padding was never read
    assert not (c["k_out"][: c["total_k"]].float() == 96.0).any()
    assert not (c["v_out"][: c["total_k"]].float() == -96.0).any()
    for n, t in before.items():
        assert torch.equal(c[n].view(torch.uint8), t.view(torch.uint8)), n


def test_ops_wrapper_allocates_and_matches():
    c = gather_case(128, torch.bfloat16, device=DEV)
    k_att, v_att = ops.gather_paged_kv(
        c["k_cache"], c["v_cache"], c["k_fresh"], c["v_fresh"],
        c["block_tables"], c["cu_seqlens"], c["cu_seqlens_k"], c["total_k"],
        c["max_seqlen_k"])
    _launch(c)
    assert k_att.shape == (c["total_k"], 3, 128)
    assert torch.equal(k_att, c["k_out"][: c["total_k"]])
    assert torch.equal(v_att, c["v_out"][: c["total_k"]])


# --------------------------------------------------------------- binding --


class TestBinding:
    def test_mismatched_dtypes_raise(self):
        c = gather_case(128, torch.bfloat16, device=DEV)
        c["k_fresh"] = c["k_fresh"].float()
        with pytest.raises(RuntimeError, match="dtype"):
            _launch(c)
        c = gather_case(128, torch.bfloat16, device=DEV)
        c["k_cache"] = c["k_cache"].float()
        c["v_cache"] = c["v_cache"].float()
        with pytest.raises(RuntimeError, match="dtype"):
            _launch(c)

    def test_int64_offsets_raise(self):
        for name in ("cu_seqlens", "cu_seqlens_k", "block_tables"):
            c = gather_case(128, torch.bfloat16, device=DEV)
            c[name] = c[name].long()
            with pytest.raises(RuntimeError, match="int32"):
                _launch(c)

    def test_misaligned_view_raises(self):
        c = gather_case(128, torch.bfloat16, device=DEV)
        n = c["k_out"].numel()
        flat = torch.empty(n + 1, dtype=torch.bfloat16, device=DEV)
        c["k_out"] = flat[1:].view(c["k_out"].shape)  # base off by 2 bytes
        with pytest.raises(RuntimeError, match="aligned"):
            _launch(c)
        c = gather_case(128, torch.bfloat16, device=DEV)
        T = c["qkv"].shape[0]
        odd = torch.empty(T, 3 * 128 + 4, dtype=torch.bfloat16, device=DEV)
        c["k_fresh"] = odd[:, : 3 * 128].view(T, 3, 128)  # 8-byte row pitch
        with pytest.raises(RuntimeError, match="aligned"):
            _launch(c)

    def test_empty_is_a_no_op(self):
        c = gather_case(128, torch.bfloat16, device=DEV)
        c["max_seqlen_k"] = 0
        _launch(c)
        assert (c["k_out"] == -7.0).all()


# ---------------------------------------------------------------- engine --


def _engine(caching, budget=8192, **kw):
    cfg = dict(
        model="tiny-llama-d128", max_num_seqs=8, max_model_len=512,
        load_weights=False, num_kv_blocks=256, enforce_eager=True,
        max_prefill_tokens=budget, enable_prefix_caching=caching,
    )
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


@pytest.fixture(scope="module")
def cold_tokens():
    eng = _engine(False)
    outs, _ = run_prompts(eng, PROMPTS, same_step=True)
    del eng
    torch.cuda.empty_cache()
    return outs


@pytest.mark.parametrize("budget", [8192, 64])
def test_engine_warm_run_hits_and_agrees(cold_tokens, budget):
    """200 shared + 30 distinct tokens: the warm requests report 192 cached
    tokens, share the head's block ids, and agree with a caching-off engine
    on the first 4 greedy tokens (the convention of TestEngineFamiliesGPU:
    the warm GEMMs run another M, so bf16 near-ties may flip later)."""
    eng = _engine(True, budget)
    params = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    outs, cached = {}, {}
    eng.add_request("r0", prompt_token_ids=PROMPTS[0], params=params)
    drain(eng, outs, cached)
    for i in (1, 2):
        eng.add_request(f"r{i}", prompt_token_ids=PROMPTS[i], params=params)
    s1, s2 = eng._seqs["r1"], eng._seqs["r2"]
    for _ in range(3):  # budget 64 admits r2 one step after r1
        for o in eng.step():
            outs.setdefault(o.request_id, []).extend(o.new_token_ids)
            cached[o.request_id] = o.cached_tokens
        if s2.block_table:
            break
    assert s1.block_table and s2.block_table
    assert s1.block_table[:12] == s2.block_table[:12]
    assert all(eng.allocator.refcount(b) == 2 for b in s1.block_table[:12])
    drain(eng, outs, cached)
    assert cached == {"r0": 0, "r1": 192, "r2": 192}
    for rid, toks in cold_tokens.items():
        assert outs[rid][:4] == toks[:4], (rid, outs[rid], toks)
    del eng
    torch.cuda.empty_cache()


def test_chunked_prefill_same_under_both_gathers(monkeypatch):
    """The chunked-prefill setup of test_engine_chunked_matches_whole_gpu
    under the kernel (default) and the torch composition it replaced."""
    prompt = "the quick brown fox " * 20
    params = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)

    def run(switch):
        monkeypatch.setenv("LLMQ_PAGED_GATHER", switch)
        eng = LLMEngine(EngineConfig(
            model="tiny-llama-d128", max_num_seqs=4, max_model_len=512,
            load_weights=False, num_kv_blocks=256,
            max_prefill_tokens=96, enforce_eager=True,
        ))
        assert eng.runner.paged_gather is (switch == "1")
        eng.add_request("r", prompt=prompt, params=params)
        outs, _ = drain(eng)
        del eng
        torch.cuda.empty_cache()
        return outs["r"]

    torch_path, kernel = run("0"), run("1")
    assert len(kernel) == 8
    assert kernel[:4] == torch_path[:4], (kernel, torch_path)
