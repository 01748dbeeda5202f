"""norm_add_norm with the row held in registers vs the three-trip kernel.

For bf16 rows of up to 8192 values the launcher picks
norm_add_norm_regs_kernel (2 or 4 16-byte vectors per thread); larger rows
and LLMQ_NORM_SANDWICH_REGS=0 (read per call) take norm_add_norm_kernel. The
register variant keeps element assignment, summation order and reductions,
so both outputs must be bitwise equal: `torch.equal`, no tolerance.
"""

from __future__ import annotations

import functools

import pytest
import torch

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

HIDDEN = (
    3584,  # the flagship: threads 192-255 hold one vector
    4096,  # exactly fills NV=2
    4608,  # NV=4, partly filled
    8192,  # fills NV=4
    8200,  # three-trip kernel either way
)
ROWS = (1, 5, 512)


def vectors_per_thread(hidden: int):
    """Mirror of the launcher's choice: NV, or None for the three-trip kernel."""
    if hidden % 8 or hidden > 8192:
        return None
    return 2 if hidden <= 4096 else 4


@functools.lru_cache(maxsize=None)
def _inputs(rows: int, hidden: int):
    gen = torch.Generator().manual_seed(rows * 10007 + hidden)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)
    return rnd(rows, hidden), rnd(rows, hidden), rnd(hidden), rnd(hidden)


@pytest.mark.parametrize("hidden", HIDDEN)
def test_every_vector_has_a_register_slot(hidden):
    nv = vectors_per_thread(hidden)
    if hidden == 8200:
        assert nv is None
        return
    assert nv == (2 if hidden <= 4096 else 4)
    # vector k of thread t starts at t*8 + k*2048: slots cover the row once
    starts = sorted(t * 8 + k * 2048 for t in range(256) for k in range(nv)
                    if t * 8 + k * 2048 < hidden)
    assert starts == list(range(0, hidden, 8))


@gpu
@needs_gpu
@pytest.mark.parametrize("offset", [1.0, 0.0])
@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("rows", ROWS)
def test_bitwise_equal_to_three_trip_kernel(rows, hidden, offset, monkeypatch):
    from llmq_amd import ops

    dev = torch.device("cuda:0")
    x, res, w_post, w_pre = (t.to(dev) for t in _inputs(rows, hidden))

    def run(flag):
        if flag is None:
            monkeypatch.delenv("LLMQ_NORM_SANDWICH_REGS", raising=False)
        else:
            monkeypatch.setenv("LLMQ_NORM_SANDWICH_REGS", flag)
        xo, ro = x.clone(), res.clone()
        ops.norm_add_norm(xo, ro, w_post, w_pre, 1e-6, offset)
        torch.cuda.synchronize()
        return xo, ro

    want_x, want_r = run("0")
    got_x, got_r = run(None)
    assert bool(torch.isfinite(got_x.float()).all())
    assert not torch.equal(got_x, x) and not torch.equal(got_r, res)
    assert torch.equal(got_r, want_r)
    assert torch.equal(got_x, want_x)
