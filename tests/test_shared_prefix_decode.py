"""Shared-prefix decode on the CPU: the reference op is the plain op on the
concatenated tables, and an engine with shared_prefix_decode on emits the
tokens of one with it off while the shared block count rises and falls."""

from __future__ import annotations

import pytest
import torch

from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.ops import torch_ref
from tests.test_prefix_cache import HEAD, drain, make_engine, tokens


@pytest.mark.parametrize("G,bs,plen,lens", [(2, 16, 32, [1, 17, 40]), (3, 8, 0, [9, 8])])
def test_reference_is_the_plain_op_on_concatenated_tables(G, bs, plen, lens):
    g = torch.Generator().manual_seed(0)
    B, KVH, D, W, Wp = len(lens), 2, 16, 5, 6
    k = torch.randn(Wp + B * W, KVH, bs, D, generator=g)
    v = torch.randn(Wp + B * W, KVH, bs, D, generator=g)
    q = torch.randn(B, KVH * G, D, generator=g)
    perm = torch.randperm(Wp + B * W, generator=g).to(torch.int32)
    ptab, bt = perm[:Wp], perm[Wp:].view(B, W)
    cl = torch.tensor(lens, dtype=torch.int32)
    got = torch_ref.shared_prefix_decode_attention(
        q, k, v, ptab, torch.tensor([plen], dtype=torch.int32), bt, cl, 0.25, 30.0, 24)
    cat = torch.cat([ptab[: plen // bs].expand(B, -1), bt], dim=1).contiguous()
    want = torch_ref.paged_decode_attention(q, k, v, cat, cl + plen, 0.25, 30.0, 24)
    torch.testing.assert_close(got, want, rtol=0, atol=0)


def shared_prefix_schedule(eng):
    """r0 owns the 192-token head; r1 (4 tokens) and r2 (12) arrive together
    and share its 12 blocks; after three steps r3 arrives without the head.
    Returns the tokens and the shared block count of every decode step."""
    seen = []
    count = eng.runner._shared_prefix_blocks
    eng.runner._shared_prefix_blocks = lambda seqs, ctx: seen.append(count(seqs, ctx)) or seen[-1]

    def greedy(n):
        return SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True)

    outs = {}
    eng.add_request("r0", prompt_token_ids=HEAD + tokens(10, 30), params=greedy(2))
    drain(eng, outs)
    eng.add_request("r1", prompt_token_ids=HEAD + tokens(11, 30), params=greedy(4))
    eng.add_request("r2", prompt_token_ids=HEAD + tokens(12, 30), params=greedy(12))
    for _ in range(3):
        for o in eng.step():
            outs.setdefault(o.request_id, []).extend(o.new_token_ids)
    eng.add_request("r3", prompt_token_ids=tokens(13, 150), params=greedy(12))
    drain(eng, outs)
    return outs, seen


def test_engine_tokens_do_not_depend_on_the_flag():
    want, _ = shared_prefix_schedule(make_engine())
    got, shared = shared_prefix_schedule(make_engine(shared_prefix_decode=True))
    assert got == want
    assert 12 in shared and shared[-1] == 0, shared  # shared, then r3 broke it


def test_flag_needs_prefix_caching():
    with pytest.raises(ValueError, match="enable_prefix_caching"):
        EngineConfig(shared_prefix_decode=True)
    assert EngineConfig().shared_prefix_decode is False
