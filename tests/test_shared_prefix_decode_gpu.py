"""Shared-prefix (cascade) decode attention on the GPU against attention
computed in float64 from the bf16-rounded inputs.

Tolerance: the decode family's (tests/test_decode_gqa_rows.py). It is loose,
so the boundary case plants large distinct V spikes on the last prefix key and
the first suffix key: losing or double-counting either moves the output by
about 400/133 = 3 against a bound of about 0.25 (checked on the CPU below)."""

from __future__ import annotations

import pytest
import torch

ATOL, RTOL = 2e-2, 1e-1
KVH = 2
gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _inputs(D, G, bs, B, plen, suffix_lens, Wp, dev, kscale=1.0, seed=0):
    """q, caches, the prefix table and per-sequence suffix tables over
    disjoint, shuffled cache blocks."""
    g = torch.Generator().manual_seed(seed)
    W = max(1, max(-(-n // bs) for n in suffix_lens))
    nb = Wp + B * W + 1
    perm = torch.randperm(nb, generator=g).to(torch.int32)
    k = (torch.randn(nb, KVH, bs, D, generator=g) * kscale).to(torch.bfloat16)
    v = torch.randn(nb, KVH, bs, D, generator=g).to(torch.bfloat16)
    q = torch.randn(B, KVH * G, D, generator=g).to(torch.bfloat16)
    return dict(
        q=q.to(dev), k=k.to(dev), v=v.to(dev),
        ptab=perm[:Wp].contiguous().to(dev),
        plen=torch.tensor([plen], dtype=torch.int32, device=dev),
        bt=perm[Wp:Wp + B * W].view(B, W).contiguous().to(dev),
        cl=torch.tensor(suffix_lens, dtype=torch.int32, device=dev),
        scale=D ** -0.5, bs=bs)


def _ref64(c, softcap=0.0, window=0, drop=None, twice=None):
    """float64 attention over prefix + suffix keys; rows with no suffix stay
    NaN. `drop` / `twice`: leave out / count twice that key of every row."""
    q, k, v = (c[n].float().double() for n in ("q", "k", "v"))
    B, H, D = q.shape
    plen, bs = int(c["plen"]), c["bs"]
    out = torch.full((B, H, D), float("nan"), dtype=torch.float64, device=q.device)
    for b in range(B):
        n = int(c["cl"][b])
        if n <= 0:
            continue
        blocks = torch.cat([c["ptab"][: plen // bs], c["bt"][b, : -(-n // bs)]]).long()
        keep = list(range(plen)) + [plen // bs * bs + j for j in range(n)]
        keep = keep[max(0, len(keep) - window):] if window else keep
        keep = [j for j in keep if j != drop] + ([twice] if twice in keep else [])
        kk = k[blocks].permute(1, 0, 2, 3).reshape(KVH, -1, D)[:, keep]
        vv = v[blocks].permute(1, 0, 2, 3).reshape(KVH, -1, D)[:, keep]
        s = torch.einsum("hgd,hld->hgl", q[b].view(KVH, -1, D), kk) * c["scale"]
        if softcap:
            s = torch.tanh(s / softcap) * softcap
        out[b] = torch.einsum("hgl,hld->hgd", s.softmax(-1), vv).reshape(H, D)
    return out


def _run(c, softcap=0.0, window=0):
    from llmq_amd import ops

    out = torch.full_like(c["q"], 7.0)
    ops.shared_prefix_decode_attention(
        c["q"], c["k"], c["v"], c["ptab"], c["plen"], c["bt"], c["cl"],
        c["scale"], softcap, window, out=out)
    return out


def _check(out, ref, cl):
    live = (cl > 0).cpu()
    err = (out.double().cpu() - ref.cpu())[live].abs()
    bound = ATOL + RTOL * ref.cpu()[live].abs()
    print("max err", float(err.max()), "worst err/bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    assert bool((out[~live.to(out.device)] == 7.0).all()), "a dead row was written"


# prefix lengths: nothing, one block, one chunk + one block, and 20 chunks +
# one block (21 chunks over the 16 key slices: 2 per slice, 11 live slices)
_PLEN = {"none": lambda bs: 0, "block": lambda bs: bs, "chunk+block": lambda bs: 64 + bs,
         "uneven": lambda bs: 20 * 64 + bs}
# windows: none; 170 ends inside the prefix for every suffix length used (if
# the prefix is that long); 20 ends inside the suffix of the long rows and
# inside the prefix of the short ones
_CASES = [  # D, G, bs, B, prefix, softcap, window
    (128, 2, 16, 70, "uneven", 0.0, 0),
    (256, 7, 32, 70, "chunk+block", 50.0, 170),
    (256, 16, 16, 70, "block", 0.0, 20),
    (128, 16, 32, 3, "none", 50.0, 0),
    (256, 1, 16, 3, "uneven", 0.0, 170),
    (128, 7, 16, 3, "chunk+block", 50.0, 20),
    (256, 2, 32, 70, "none", 0.0, 20),
    (128, 1, 32, 70, "block", 50.0, 0),
]


@gpu
@needs_gpu
@pytest.mark.parametrize("D,G,bs,B,prefix,softcap,window", _CASES)
def test_cascade_matches_float64(D, G, bs, B, prefix, softcap, window):
    from llmq_amd import ops
    from llmq_amd.ops import torch_ref

    plen = _PLEN[prefix](bs)
    lens = [[1, 0, 130, bs - 1, bs, bs + 1][i % 6] for i in range(B)]
    c = _inputs(D, G, bs, B, plen, lens, max(1, plen // bs) + 3, "cuda")
    ref = _ref64(c, softcap, window)
    _check(_run(c, softcap, window), ref, c["cl"])
    # the plain decode op on the concatenated tables: same inputs, same bound
    tables, tl = torch_ref.concat_prefix_tables(c["ptab"], c["plen"], c["bt"], c["cl"], bs)
    plain = torch.full_like(c["q"], 7.0)
    plain[c["cl"] > 0] = ops.paged_decode_attention(
        c["q"], c["k"], c["v"], tables, tl, c["scale"], softcap, window)[c["cl"] > 0]
    _check(plain, ref, c["cl"])


def _spiked(dev):
    """Near-uniform weights over 128 prefix + 5 suffix keys; V of the last
    prefix key is +400 and of the first suffix key -704 (exact in bf16)."""
    c = _inputs(128, 2, 16, 3, 128, [5, 5, 5], 8, dev, kscale=0.05, seed=1)
    c["v"][c["ptab"][7].long(), :, 15] = 400.0
    for b in range(3):
        c["v"][c["bt"][b, 0].long(), :, 0] = -704.0
    return c


def test_reference_sees_a_lost_or_doubled_boundary_key():
    c = _spiked("cpu")
    ref = _ref64(c)
    for kw in (dict(drop=127), dict(drop=128), dict(twice=127), dict(twice=128)):
        bad = _ref64(c, **kw)
        assert bool(((bad - ref).abs() > 4 * (ATOL + RTOL * ref.abs())).all()), kw


@gpu
@needs_gpu
def test_cascade_keeps_both_boundary_keys_once():
    c = _spiked("cuda")
    _check(_run(c), _ref64(c), c["cl"])


@gpu
@needs_gpu
def test_fp8_cache_takes_the_fallback():
    c = _inputs(128, 2, 16, 3, 64 + 16, [1, 0, 130], 8, "cuda")
    c["k"], c["v"] = c["k"].to(torch.float8_e4m3fn), c["v"].to(torch.float8_e4m3fn)
    _check(_run(c), _ref64(c), c["cl"])


@gpu
@needs_gpu
def test_engine_graphs_with_the_flag_match_eager_without():
    """Decode graphs captured with the cascade op against eager plain decode:
    12 shared blocks, then r1 finishes and r3 joins without them."""
    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine
    from tests.test_shared_prefix_decode import shared_prefix_schedule

    def run(**kw):
        eng = LLMEngine(EngineConfig(
            model="tiny-llama-d128", max_num_seqs=8, max_model_len=512,
            load_weights=False, num_kv_blocks=256, enable_prefix_caching=True, **kw))
        assert eng.runner.shared_prefix is bool(kw.get("shared_prefix_decode"))
        res = shared_prefix_schedule(eng)
        del eng
        torch.cuda.empty_cache()
        return res

    want, _ = run(enforce_eager=True)
    got, shared = run(shared_prefix_decode=True)
    print("shared blocks per decode step", shared)
    assert 12 in shared and shared[-1] == 0, shared
    assert got == want
