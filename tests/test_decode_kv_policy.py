"""Cache policy of the decode K/V stream: `nt` against the default policy.

The pipe decode kernels stream K and V with `global_load_lds ... nt` by
default; LLMQ_DECODE_KV_NT=0 (read per call) selects the instantiation with
the default policy. A cache policy decides where a line is kept, never what a
load returns, so the two must agree bit for bit: every case runs both and
compares with torch.equal. The inputs (and, for its own context lengths, the
fp32 reference) are those of test_decode_gqa_rows._case; further context
lengths re-use its tensors with other `context_lens`.
"""

from __future__ import annotations

import pytest
import torch

from tests.test_decode_gqa_rows import ATOL, CTX, RTOL, _case, _id

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from llmq_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")

# Context lengths per 4-sequence batch, all within _case's block tables
# (max(CTX) = 130 keys): _case's own set (1, 63, 65, 130: has the reference),
# the 64- and 128-key chunk edges from the other side, and a ragged batch.
LENS = (CTX, (64, 129, 1, 65), (17, 100, 128, 33))
assert all(len(ls) == len(CTX) and max(ls) <= max(CTX) for ls in LENS)


def _grid():
    """(case kwargs, LLMQ_DECODE_PIPE values). The fp8 pipe kernel has one
    chunk size, so it runs once."""
    both, one = ("64", "128"), ("64",)
    out = []
    for D in (128, 256):
        for G in (1, 2, 5, 12):
            for softcap in (0.0, 50.0):
                out.append((dict(G=G, D=D, softcap=softcap), both))
            out.append((dict(G=G, D=D, fp8=True), one))
        out.append((dict(G=2, D=D, softcap=50.0, window=40), both))
        out.append((dict(G=2, D=D, softcap=50.0, fp8=True), one))
        out.append((dict(G=5, D=D, bs=32), both))
        # split-KV: one sequence, one kv head, 16 z-slices
        out.append((dict(G=2, D=D, split=True), both))
    out.append((dict(G=2, D=256, softcap=50.0, window=40, fp8=True), one))
    out.append((dict(G=2, D=256, fp8=True, bs=32), one))
    out.append((dict(G=5, D=256, fp8=True, split=True), one))
    return out


@pytest.mark.parametrize(
    "kw,pipe", [(kw, p) for kw, pipes in _grid() for p in pipes],
    ids=lambda v: v if isinstance(v, str) else _id(v))
def test_nt_equals_default_policy(kw, pipe, monkeypatch):
    monkeypatch.setenv("LLMQ_DECODE_PIPE", pipe)
    c = _case(**kw)
    q, kc, vc, bt = (c[n].to(DEV) for n in ("q", "kc", "vc", "bt"))
    lens = (tuple(c["cl"].tolist()),) if kw.get("split") else LENS
    for ls in lens:
        cl = torch.tensor(ls, dtype=torch.int32, device=DEV)
        outs = {}
        for policy in ("0", "1"):
            monkeypatch.setenv("LLMQ_DECODE_KV_NT", policy)
            outs[policy] = ops.paged_decode_attention(
                q, kc, vc, bt, cl, c["scale"], c["softcap"], c["window"])
        monkeypatch.delenv("LLMQ_DECODE_KV_NT")
        unset = ops.paged_decode_attention(
            q, kc, vc, bt, cl, c["scale"], c["softcap"], c["window"])
        assert torch.equal(outs["0"], outs["1"]), (kw, pipe, ls)
        assert torch.equal(unset, outs["1"]), (kw, pipe, ls)
        if ls == tuple(c["cl"].tolist()):  # both are the right answer
            torch.testing.assert_close(
                outs["1"].float().cpu(), c["ref"], atol=ATOL, rtol=RTOL)
