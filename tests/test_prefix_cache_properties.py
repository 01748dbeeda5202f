"""Property-based allocator/scheduler invariants with prefix caching on.

Random add / step / abort over a tiny engine on a tight pool, with prompts
drawn from a few shared heads plus random tails so that blocks really are
shared, parked on the evictable list, revived and evicted. After every
operation the refcounts must equal the number of live holders, no block may
be both held and free/evictable, and nothing may leak.
"""

from __future__ import annotations

from collections import Counter

import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.kv_cache import PrefixCachingAllocator
from llmq_amd.engine.sampling_params import SamplingParams

pytestmark = pytest.mark.integration

HEADS = [
    list(range(10, 10 + 48)),        # three full blocks
    list(range(10, 10 + 32)) + [7] * 20,  # shares two blocks with the first
    list(range(100, 100 + 70)),      # four full blocks + 6
]


def make_engine() -> LLMEngine:
    return LLMEngine(EngineConfig(
        model="tiny-llama", device="cpu", load_weights=False,
        max_num_seqs=4, max_model_len=128, num_kv_blocks=20,
        max_prefill_tokens=40, kv_block_size=16,
        enable_prefix_caching=True,
    ))


def check_invariants(eng: LLMEngine) -> None:
    sched = eng.scheduler
    alloc = eng.allocator
    assert isinstance(alloc, PrefixCachingAllocator)
    live = list(sched.running) + list(sched.prefilling) + list(sched.waiting)
    holders = Counter()
    for seq in live:
        assert len(seq.block_table) == len(set(seq.block_table)), (
            "block twice in one table")
        holders.update(seq.block_table)
    # conservation over DISTINCT held blocks (shared ones count once)
    assert alloc.num_free + len(holders) == alloc.num_blocks, (
        f"leak: free={alloc.num_free} held={len(holders)} total={alloc.num_blocks}"
    )
    # refcount == number of live sequences holding the block
    for b in range(alloc.num_blocks):
        assert alloc.refcount(b) == holders.get(b, 0), (
            f"block {b}: refcount {alloc.refcount(b)} != holders {holders.get(b, 0)}"
        )
    # free, evictable and held are disjoint
    free, evictable = set(alloc._free), set(alloc._lru)
    assert len(free) == len(alloc._free), "block twice on the free list"
    assert not free & evictable
    assert not (free | evictable) & set(holders)
    # evictable blocks are exactly the cached blocks nobody holds
    assert evictable == {b for b in alloc._node_of if alloc.refcount(b) == 0}
    assert set(alloc._cache.values()) == set(alloc._node_of)
    # the invariants of test_scheduler_properties: seat cap, chunk bookkeeping
    assert len(sched.running) + len(sched.prefilling) <= sched.max_num_seqs
    for seq in sched.prefilling:
        assert 0 < seq.prefilled < seq.num_tokens
        assert seq not in sched.running
    for seq in sched.waiting:
        assert not seq.block_table
    bs = sched.block_size
    for seq in list(sched.running) + list(sched.prefilling):
        assert len(seq.block_table) * bs >= seq.prefilled


@settings(max_examples=20, deadline=None)
@given(st.lists(
    st.one_of(
        st.tuples(st.just("add"), st.integers(0, len(HEADS) - 1),
                  st.integers(0, 3), st.integers(0, 30)),  # head, cut, tail
        st.tuples(st.just("step")),
        st.tuples(st.just("abort"), st.integers(0, 30)),   # request index
    ),
    min_size=5, max_size=40,
))
def test_shared_blocks_never_leak_or_miscount(ops):
    eng = make_engine()
    params = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    n = 0
    for op in ops:
        if op[0] == "add":
            _, head, cut, tail = op
            # cut drops the head's last tokens: prompts that end inside, at
            # the edge of, or past their head's full blocks
            prompt = HEADS[head][: len(HEADS[head]) - 8 * cut]
            prompt = prompt + [200 + (n * 7 + j) % 50 for j in range(tail)]
            eng.add_request(f"r{n}", prompt_token_ids=prompt, params=params)
            n += 1
        elif op[0] == "step":
            eng.step()
        else:
            eng.abort_request(f"r{op[1] % max(n, 1)}")
        check_invariants(eng)
    guard = 0
    while eng.has_unfinished() and guard < 500:
        eng.step()
        check_invariants(eng)
        guard += 1
    assert guard < 500, "engine failed to drain"
    assert eng.allocator.num_free == eng.allocator.num_blocks
    # every prompt token admitted was looked up; hits never exceed lookups
    stats = eng.prefix_cache_stats()
    assert 0 <= stats["hit_tokens"] <= stats["lookup_tokens"]
