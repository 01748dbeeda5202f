"""GQA row placement in the MFMA paged-decode kernels.

The kernels put q-head g in MFMA tile row (g & 3) * 4 + (g >> 2) and run the
per-chunk softmax only for the NREG = ceil(G/4) accumulator registers that
hold q-heads. These tests sweep G over every NREG boundary and every row of
that transpose, through all three kernels (plain, pipe, pipe_fp8), the
split-KV scratch path and block size 32, against the fp32 reference with the
tolerances of test_gpu_kernels.py::test_pipe_variants.

Inputs are made on the CPU from a seed with a PEAKED softmax (q = 4 * randn),
so every head's output is distinct: test_reference_sees_a_head_swap checks,
on the reference alone and without a GPU, that exchanging any two heads of
the expected output would fail the comparison the GPU tests make.
"""

from __future__ import annotations

import functools
import itertools

import pytest
import torch

from llmq_amd.ops import torch_ref

ATOL, RTOL = 2e-2, 1e-1  # test_pipe_variants
CTX = (1, 63, 65, 130)   # straddle the 64- and 128-key chunk edges
ALL_G = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16)

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@functools.lru_cache(maxsize=None)
def _case(G, D, softcap=0.0, window=0, fp8=False, split=False, bs=16):
    """Seeded CPU inputs + fp32 reference, built once per input set and
    shared (read-only) by every kernel variant that runs it."""
    gen = torch.Generator().manual_seed(1000 * G + D + bs + int(softcap) + window)
    B, KVH, ctx = (1, 1, (300,)) if split else (4, 2, CTX)
    max_blocks = (max(ctx) + bs - 1) // bs
    NB = B * max_blocks + 1  # block 0 stays unused to catch indexing bugs
    rnd = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)
    kc, vc = rnd(NB, KVH, bs, D), rnd(NB, KVH, bs, D)
    if fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
    bt = (torch.randperm(NB - 1, generator=gen)[: B * max_blocks] + 1)
    bt = bt.reshape(B, max_blocks).to(torch.int32)
    q = (4.0 * torch.randn(B, G * KVH, D, generator=gen)).to(torch.bfloat16)
    cl = torch.tensor(ctx, dtype=torch.int32)
    scale = D ** -0.5
    ref = torch_ref.paged_decode_attention(
        q.float(), kc.float(), vc.float(), bt, cl, scale, softcap, window)
    return dict(q=q, kc=kc, vc=vc, bt=bt, cl=cl, scale=scale, softcap=softcap,
                window=window, ref=ref)


def _grid():
    """(case kwargs, LLMQ_DECODE_PIPE values) for every input set."""
    bf16_pipes, fp8_pipes = ("0", "64", "128"), ("0", "64")
    out = []
    for D in (128, 256):
        for G in ALL_G:
            out.append((dict(G=G, D=D), bf16_pipes))
        for G in (2, 5, 12):  # one G per NREG: softcap + window mid-chunk
            out.append((dict(G=G, D=D, softcap=50.0, window=40), bf16_pipes))
        for G in (2, 5, 16):
            out.append((dict(G=G, D=D, fp8=True), fp8_pipes))
            out.append((dict(G=G, D=D, split=True), bf16_pipes))
    out.append((dict(G=2, D=256, bs=32), bf16_pipes))
    return out


def _id(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


def _mismatch(a, b):
    return bool(((a - b).abs() > ATOL + RTOL * b.abs()).any())


@pytest.mark.parametrize("kw", [kw for kw, _ in _grid()], ids=_id)
def test_reference_sees_a_head_swap(kw):
    """Precondition (no GPU): a kernel that returned any two heads exchanged
    would fail the tolerance of the GPU tests below."""
    ref = _case(**kw)["ref"]
    H = ref.shape[1]
    assert H >= 2
    for h1, h2 in itertools.combinations(range(H), 2):
        swapped = ref.clone()
        swapped[:, h1], swapped[:, h2] = ref[:, h2], ref[:, h1]
        assert _mismatch(swapped, ref), (kw, h1, h2)


@gpu
@needs_gpu
@pytest.mark.parametrize(
    "kw,pipe", [(kw, p) for kw, pipes in _grid() for p in pipes],
    ids=lambda v: v if isinstance(v, str) else _id(v))
def test_decode_matches_reference(kw, pipe, monkeypatch):
    from llmq_amd import ops

    monkeypatch.setenv("LLMQ_DECODE_PIPE", pipe)
    c = _case(**kw)
    dev = torch.device("cuda:0")
    out = ops.paged_decode_attention(
        c["q"].to(dev), c["kc"].to(dev), c["vc"].to(dev), c["bt"].to(dev),
        c["cl"].to(dev), c["scale"], c["softcap"], c["window"])
    assert out.dtype == torch.bfloat16
    torch.testing.assert_close(out.float().cpu(), c["ref"], atol=ATOL, rtol=RTOL)
