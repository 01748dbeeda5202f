"""Automatic prefix caching on CPU (fp32 tiny models, exact token counts).

Covers the allocator's hit arithmetic, greedy-output equality against a
caching-off engine in both arrival orders, real block sharing (ids and
refcounts), tail-first eviction, preemption recovery, exact-content identity
(no false hits), the user-facing plumbing, and `torch_ref.gather_paged_kv`
against a per-token loop.
"""

from __future__ import annotations

import random

import pytest
import torch

from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.kv_cache import BlockAllocator, PrefixCachingAllocator
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.ops import torch_ref

BS = 16


def make_engine(model="tiny-llama", caching=True, **kw) -> LLMEngine:
    defaults = dict(
        model=model, max_num_seqs=8, max_model_len=512, device="cpu",
        load_weights=False, kv_block_size=BS, num_kv_blocks=128,
        enable_prefix_caching=caching,
    )
    defaults.update(kw)
    return LLMEngine(EngineConfig(**defaults))


def greedy(max_tokens=8) -> SamplingParams:
    return SamplingParams(temperature=0.0, max_tokens=max_tokens, ignore_eos=True)


def tokens(seed: int, n: int):
    rng = random.Random(seed)
    return [rng.randrange(3, 200) for _ in range(n)]


HEAD = tokens(1, 200)
PROMPTS = [HEAD + tokens(10 + i, 30) for i in range(3)]  # n = 230


def drain(eng: LLMEngine, outs=None, cached=None):
    outs = {} if outs is None else outs
    cached = {} if cached is None else cached
    guard = 0
    while eng.has_unfinished():
        for o in eng.step():
            outs.setdefault(o.request_id, []).extend(o.new_token_ids)
            cached[o.request_id] = o.cached_tokens
        guard += 1
        assert guard < 2000, "engine failed to drain"
    return outs, cached


def run_prompts(eng, prompts, same_step, params=None):
    """Owner-first (the first prompt finishes before the rest arrive) or
    same-step (all added before the first step)."""
    params = params or greedy()
    outs, cached = {}, {}
    if same_step:
        for i, p in enumerate(prompts):
            eng.add_request(f"r{i}", prompt_token_ids=p, params=params)
        drain(eng, outs, cached)
    else:
        eng.add_request("r0", prompt_token_ids=prompts[0], params=params)
        drain(eng, outs, cached)
        for i, p in enumerate(prompts[1:], 1):
            eng.add_request(f"r{i}", prompt_token_ids=p, params=params)
        drain(eng, outs, cached)
    return outs, cached


# ------------------------------------------------------------ arithmetic --


class TestHitArithmetic:
    def test_shared_head_hits_full_blocks(self):
        eng = make_engine()
        _, cached = run_prompts(eng, PROMPTS, same_step=False)
        # 200 shared tokens = 12 full blocks (the cap would allow 224)
        assert cached == {"r0": 0, "r1": 192, "r2": 192}
        stats = eng.prefix_cache_stats()
        assert stats["lookup_tokens"] == 3 * 230
        assert stats["hit_tokens"] == 2 * 192
        assert stats["evictions"] == 0
        assert eng.allocator.num_free == eng.allocator.num_blocks

    @pytest.mark.parametrize("n,hit", [(32, 16), (33, 32)])
    def test_identical_prompt_keeps_one_token_to_compute(self, n, hit):
        eng = make_engine()
        p = tokens(5, n)
        eng.add_request("a", prompt_token_ids=p, params=greedy(4))
        _, cached = drain(eng)
        assert cached["a"] == 0
        eng.add_request("b", prompt_token_ids=p, params=greedy(4))
        _, cached = drain(eng)
        assert cached["b"] == hit  # cap ((n - 1) // 16) * 16


# -------------------------------------------------------------- equality --


@pytest.fixture(scope="module")
def baseline():
    """Caching-off greedy outputs per (model, budget), computed once."""
    memo = {}

    def get(model, budget):
        key = (model, budget)
        if key not in memo:
            eng = make_engine(model, caching=False, max_prefill_tokens=budget)
            memo[key] = run_prompts(eng, PROMPTS, same_step=True)[0]
        return memo[key]

    return get


class TestEquality:
    @pytest.mark.parametrize("same_step", [False, True],
                             ids=["owner-first", "same-step"])
    @pytest.mark.parametrize("model,budget", [
        ("tiny-llama", 8192), ("tiny-qwen3", 8192),
        ("tiny-gemma2", 8192),  # window 64: the 200-token head crosses it
        ("tiny-llama", 48),     # a hit sequence also chunks
    ])
    def test_outputs_equal_caching_off(self, baseline, model, budget, same_step):
        eng = make_engine(model, max_prefill_tokens=budget)
        outs, cached = run_prompts(eng, PROMPTS, same_step)
        # the first request never hits; later ones do, even when all three
        # were admitted before the first step ran (same-step sharing)
        assert cached == {"r0": 0, "r1": 192, "r2": 192}
        assert outs == baseline(model, budget)
        assert all(len(t) == 8 for t in outs.values())


# --------------------------------------------------------------- sharing --


def test_sharing_is_real():
    eng = make_engine()
    alloc = eng.allocator
    eng.add_request("r0", prompt_token_ids=PROMPTS[0], params=greedy(4))
    drain(eng)
    assert alloc.num_free == alloc.num_blocks
    free_before = alloc.num_free
    for i in (1, 2):
        eng.add_request(f"r{i}", prompt_token_ids=PROMPTS[i], params=greedy(16))
    eng.step()  # both admitted as hits
    s1, s2 = eng._seqs["r1"], eng._seqs["r2"]
    assert s1.cached_tokens == 192 and s2.cached_tokens == 192
    shared = s1.block_table[:12]
    assert shared == s2.block_table[:12]
    assert all(alloc.refcount(b) == 2 for b in shared)
    private = s1.block_table[12:] + s2.block_table[12:]
    assert len(set(private)) == len(private) and not set(private) & set(shared)
    assert all(alloc.refcount(b) == 1 for b in private)
    # the shared head left the evictable list once; only private blocks are new
    assert alloc.num_free == free_before - 12 - len(private)
    drain(eng)
    assert alloc.num_free == alloc.num_blocks


# -------------------------------------------------------------- eviction --


def test_tail_first_eviction():
    a = tokens(21, 70)
    b = tokens(22, 200)

    def run(caching):
        eng = make_engine(caching=caching, num_kv_blocks=16)
        outs, cached = {}, {}
        for rid, p in (("a1", a), ("b", b), ("a2", a)):
            eng.add_request(rid, prompt_token_ids=p, params=greedy(4))
            drain(eng, outs, cached)
        return eng, outs, cached

    eng, outs, cached = run(True)
    # A: 4 full blocks cached, 1 plain-freed. B needs 13: 12 truly free + one
    # eviction, which under tail-first is A's fourth block.
    assert cached == {"a1": 0, "b": 0, "a2": 48}
    stats = eng.prefix_cache_stats()
    assert stats["evictions"] >= 1
    assert eng.allocator.num_free == 16
    _, ref_outs, _ = run(False)
    assert outs == ref_outs


# ------------------------------------------------------------ preemption --


def _run_pool(caching, num_kv_blocks, prompts, max_tokens, **kw):
    eng = make_engine(caching=caching, num_kv_blocks=num_kv_blocks,
                      max_num_seqs=4, **kw)
    params = greedy(max_tokens)
    for i, p in enumerate(prompts):
        if isinstance(p, str):
            eng.add_request(f"p{i}", prompt=p, params=params)
        else:
            eng.add_request(f"p{i}", prompt_token_ids=p, params=params)
    seqs = list(eng._seqs.values())  # keep refs past finish-time pop
    outs, _ = drain(eng)
    return eng, outs, seqs


def test_preemption_recovers_with_caching():
    """The setup of TestSchedulerBehavior.test_preemption_recovers (8 blocks,
    three "x" * 10 prompts, 20 tokens each) with caching on: every sequence
    finishes with the caching-off outputs and all blocks come back."""
    prompts = ["x" * 10] * 3
    eng, outs, _ = _run_pool(True, 8, prompts, 20, max_model_len=256)
    _, ref_outs, _ = _run_pool(False, 8, prompts, 20, max_model_len=256)
    assert set(outs) == {"p0", "p1", "p2"}
    assert all(len(t) == 20 for t in outs.values())
    assert outs == ref_outs
    assert eng.allocator.num_free == 8


def test_preempted_sequence_readmission_hits():
    """That setup's sequences never outgrow the pool (3 x 2 blocks of 8), so
    nothing is preempted there. This pool is too small for its batch (the
    setup of test_preemption_recompute_matches_unpreempted: 4 sequences want
    ~19 of 13 blocks): a preempted sequence releases its blocks through
    free(), its prompt blocks stay cached, and its recompute hits them."""
    prompts = [list(range(1 + 7 * i, 40 + 5 * i)) for i in range(4)]
    kw = dict(max_model_len=128, max_prefill_tokens=64)
    eng, outs, seqs = _run_pool(True, 13, prompts, 24, **kw)
    _, ref_outs, ref_seqs = _run_pool(False, 64, prompts, 24, **kw)
    assert max(s.num_preemptions for s in ref_seqs) == 0
    preempted = [s for s in seqs if s.num_preemptions > 0]
    assert preempted, "pool never forced a preemption - shrink it"
    assert all(len(t) == 24 for t in outs.values())
    assert outs == ref_outs
    assert any(s.cached_tokens > 0 for s in preempted)
    assert eng.prefix_cache_stats()["hit_tokens"] > 0
    assert eng.allocator.num_free == 13


# ---------------------------------------------------------- no false hits --


class TestNoFalseHits:
    def test_same_second_block_different_first(self):
        second = tokens(31, 16)
        p1 = tokens(32, 16) + second + tokens(33, 8)
        p2 = tokens(34, 16) + second + tokens(35, 8)
        eng = make_engine()
        eng.add_request("a", prompt_token_ids=p1, params=greedy(2))
        drain(eng)
        eng.add_request("b", prompt_token_ids=p2, params=greedy(2))
        eng.step()
        assert eng._seqs["b"].cached_tokens == 0
        assert eng.prefix_cache_stats()["hit_tokens"] == 0
        drain(eng)

    def test_last_token_of_first_block_differs(self):
        p1 = tokens(41, 40)
        p2 = list(p1)
        p2[15] = p1[15] + 1
        eng = make_engine()
        eng.add_request("a", prompt_token_ids=p1, params=greedy(2))
        drain(eng)
        eng.add_request("b", prompt_token_ids=p2, params=greedy(2))
        _, cached = drain(eng)
        assert cached["b"] == 0

    def test_reused_block_id_does_not_revive_children(self):
        """A child registered under an evicted parent must not match once the
        parent's block id holds other content."""
        alloc = PrefixCachingAllocator(4, 2)
        t1 = alloc.allocate(2)
        alloc.register([1, 2, 3, 4], t1, 4)
        alloc.free(t1[:1])          # parent evictable, child still held
        t2 = alloc.allocate(3)      # two free blocks, then evicts the parent
        assert t1[0] in t2
        reused = [t1[0]] + [b for b in t2 if b != t1[0]]
        alloc.register([9, 9, 3, 4], reused, 2)  # parent id, other content
        assert alloc.lookup([9, 9, 3, 4, 0]) == [t1[0]]


# -------------------------------------------------------------- plumbing --


class TestPlumbing:
    def test_off_by_default_is_plain_allocator(self):
        assert EngineConfig().enable_prefix_caching is False
        eng = make_engine(caching=False)
        assert type(eng.allocator) is BlockAllocator
        assert eng.prefix_cache_stats()["hit_tokens"] == 0
        assert isinstance(make_engine().allocator, PrefixCachingAllocator)

    def test_env_var_reaches_engine_config(self, monkeypatch):
        from llmq_amd.core.config import Config
        from llmq_amd.workers.engine_worker import EngineWorker

        assert Config().enable_prefix_caching is False
        monkeypatch.setenv("LLMQ_PREFIX_CACHING", "1")
        w = EngineWorker("q", model="tiny-llama", config=Config())
        assert EngineConfig(**w._engine_kwargs(1)).enable_prefix_caching is True

    def test_cli_flag_reaches_engine_config(self, monkeypatch):
        from click.testing import CliRunner

        import llmq_amd.cli.worker as cli_worker
        from llmq_amd.cli.main import cli
        from llmq_amd.core.config import Config
        from llmq_amd.workers.engine_worker import EngineWorker

        seen = {}
        monkeypatch.setattr(cli_worker, "run_engine_worker",
                            lambda *a, **kw: seen.update(kw))
        res = CliRunner().invoke(
            cli, ["worker", "run", "tiny-llama", "q", "--enable-prefix-caching"])
        assert res.exit_code == 0, res.output
        w = EngineWorker("q", model="tiny-llama", config=Config(),
                         engine_overrides=seen["engine_overrides"])
        assert EngineConfig(**w._engine_kwargs(1)).enable_prefix_caching is True
        seen.clear()
        res = CliRunner().invoke(cli, ["worker", "run", "tiny-llama", "q"])
        assert res.exit_code == 0, res.output
        assert not (seen["engine_overrides"] or {}).get("enable_prefix_caching")

    def test_engine_worker_copies_cached_tokens(self):
        from llmq_amd.core.models import Job
        from llmq_amd.workers.engine_worker import EngineWorker, _FinishedRequest

        w = EngineWorker.__new__(EngineWorker)
        w.worker_id = "w"
        w._stats = {"j": _FinishedRequest(
            text="t", prompt_tokens=230, output_tokens=4, finish_reason="length",
            queue_wait_ms=0.0, prefill_ms=0.0, decode_ms=0.0, cached_tokens=192)}
        result = w._build_result(Job(id="j", prompt="p"), "t", 1.0)
        assert result.prompt_tokens == 230
        assert result.cached_tokens == 192

    def test_bridge_reports_cached_tokens(self):
        """Through the engine thread: RequestOutput.cached_tokens reaches the
        finished-request record the worker builds its Result from."""
        from llmq_amd.workers.engine_worker import AsyncEngineBridge
        from tests.conftest import run_async

        async def main():
            bridge = AsyncEngineBridge(lambda: make_engine(max_model_len=256))
            await bridge.start()
            try:
                prompt = "shared template " * 4  # 64 chars
                first = await bridge.generate("a", prompt + "one", greedy(2))
                second = await bridge.generate("b", prompt + "two", greedy(2))
                n_head = len(bridge.engine.tokenizer.encode(prompt))
            finally:
                bridge.shutdown()
            return first, second, n_head

        first, second, n_head = run_async(main())
        assert first.cached_tokens == 0
        assert second.cached_tokens == (n_head // BS) * BS > 0


# ------------------------------------------------------- torch reference --

GATHER_SEQS = [(0, 5), (16, 1), (37, 20), (1, 33)]  # (P, Lq)


def gather_case(D, dtype, cache_dtype=None, KVH=3, HQ=6, device="cpu", seed=0):
    """Inputs of the gather shape set: fresh K/V as views into one qkv
    buffer, shuffled non-adjacent block ids, a block table wider than needed
    and padded with the id of a sentinel-filled block, sentinel rows after
    total_k in the outputs."""
    g = torch.Generator().manual_seed(seed)
    NB = 12
    cache_dtype = cache_dtype or dtype
    kc = torch.randn(NB, KVH, BS, D, generator=g).to(cache_dtype)
    vc = torch.randn(NB, KVH, BS, D, generator=g).to(cache_dtype)
    sentinel_block = NB - 1
    kc[sentinel_block] = torch.full((KVH, BS, D), 96.0).to(cache_dtype)
    vc[sentinel_block] = torch.full((KVH, BS, D), -96.0).to(cache_dtype)
    T = sum(lq for _, lq in GATHER_SEQS)
    qkv = torch.randn(T, (HQ + 2 * KVH) * D, generator=g).to(dtype)
    bt = torch.full((len(GATHER_SEQS), 5), sentinel_block, dtype=torch.int32)
    bt[1, 0] = 3
    bt[2, :3] = torch.tensor([7, 2, 9])
    bt[3, 0] = 5
    cu, cu_k = [0], [0]
    for p, lq in GATHER_SEQS:
        cu.append(cu[-1] + lq)
        cu_k.append(cu_k[-1] + p + lq)
    tensors = dict(
        k_cache=kc, v_cache=vc, qkv=qkv, block_tables=bt,
        cu_seqlens=torch.tensor(cu, dtype=torch.int32),
        cu_seqlens_k=torch.tensor(cu_k, dtype=torch.int32),
    )
    tensors = {k: v.to(device) for k, v in tensors.items()}
    qkv = tensors["qkv"]
    tensors["k_fresh"] = qkv[:, HQ * D:(HQ + KVH) * D].view(T, KVH, D)
    tensors["v_fresh"] = qkv[:, (HQ + KVH) * D:].view(T, KVH, D)
    tensors["k_out"] = torch.full((cu_k[-1] + 3, KVH, D), -7.0, dtype=dtype, device=device)
    tensors["v_out"] = torch.full((cu_k[-1] + 3, KVH, D), -7.0, dtype=dtype, device=device)
    tensors["total_k"] = cu_k[-1]
    tensors["max_seqlen_k"] = max(p + lq for p, lq in GATHER_SEQS)
    return tensors


def gather_loop_reference(c):
    """Plain per-token loop over the op's definition."""
    ke = torch.full_like(c["k_out"], -7.0)
    ve = torch.full_like(c["v_out"], -7.0)
    cu, cu_k = c["cu_seqlens"].tolist(), c["cu_seqlens_k"].tolist()
    bt = c["block_tables"].tolist()
    for b, (p, lq) in enumerate(GATHER_SEQS):
        for r in range(p + lq):
            dst = cu_k[b] + r
            if r < p:
                ke[dst] = c["k_cache"][bt[b][r // BS], :, r % BS].to(ke.dtype)
                ve[dst] = c["v_cache"][bt[b][r // BS], :, r % BS].to(ve.dtype)
            else:
                ke[dst] = c["k_fresh"][cu[b] + r - p]
                ve[dst] = c["v_fresh"][cu[b] + r - p]
    return ke, ve


GATHER_PARAMS = [
    pytest.param(D, dt, None, id=f"{name}-D{D}")
    for D in (64, 128, 256)
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32))
] + [pytest.param(128, torch.bfloat16, torch.float8_e4m3fn, id="fp8-D128")]


@pytest.mark.parametrize("D,dtype,cache_dtype", GATHER_PARAMS)
def test_torch_ref_gather_matches_token_loop(D, dtype, cache_dtype):
    c = gather_case(D, dtype, cache_dtype)
    torch_ref.gather_paged_kv(
        c["k_out"], c["v_out"], c["k_cache"], c["v_cache"], c["k_fresh"],
        c["v_fresh"], c["block_tables"], c["cu_seqlens"], c["cu_seqlens_k"],
        c["max_seqlen_k"])
    ke, ve = gather_loop_reference(c)
    assert torch.equal(c["k_out"], ke)
    assert torch.equal(c["v_out"], ve)
    assert (c["k_out"][c["total_k"]:] == -7.0).all()
