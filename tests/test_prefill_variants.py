"""Both MFMA flash-prefill kernels (LLMQ_PREFILL_PIPE=1: glds pipeline,
=0: plain staging) vs the fp32 reference, at the smallest shapes that reach
every branch of the shared pf_* helpers. Tolerances are the ones the bf16
prefill tests in test_gpu_kernels.py use for the same kind of case.
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

DEV = torch.device("cuda:0")
DTYPE = torch.bfloat16


def prefill_case(H, KVH, D, q_lens, k_lens, seed):
    """Seeded q/k/v and offsets; K/V are k_lens long, Q the last q_lens rows."""
    g = torch.Generator().manual_seed(seed)
    Tq, Tk = sum(q_lens), sum(k_lens)
    q = torch.randn(Tq, H, D, generator=g).to(DTYPE)
    k = torch.randn(Tk, KVH, D, generator=g).to(DTYPE)
    v = torch.randn(Tk, KVH, D, generator=g).to(DTYPE)
    cu_q = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(torch.tensor(k_lens).cumsum(0)), dtype=torch.int32)
    return q, k, v, cu_q, cu_k


def run_and_check(case, max_q, scale, softcap, window, chunked, atol, rtol):
    q, k, v, cu_q, cu_k = case
    out = ops.varlen_prefill_attention(
        q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), max_q, scale, softcap,
        window, cu_seqlens_k=cu_k.to(DEV) if chunked else None,
    )
    ref = torch_ref.varlen_prefill_attention(
        q.float(), k.float(), v.float(), cu_q, scale, softcap, window,
        cu_seqlens_k=cu_k if chunked else None,
    )
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("pipe", ["0", "1"])
class TestFlashPrefillVariants:
    @pytest.mark.parametrize("D", [64, 128, 256])
    def test_head_dim_and_length_sweep(self, pipe, D, monkeypatch):
        """One q row, a partial 16-row wave, an exact tile, a tile plus one
        row, two tiles plus a remainder with inactive upper waves."""
        monkeypatch.setenv("LLMQ_PREFILL_PIPE", pipe)
        lens = [1, 15, 64, 65, 130]
        case = prefill_case(4, 2, D, lens, lens, seed=3)
        run_and_check(case, max(lens), D ** -0.5, 0.0, 0, False, 4e-2, 1e-1)

    def test_softcap_window(self, pipe, monkeypatch):
        """kv_begin > 0 and a window that crosses a tile edge."""
        monkeypatch.setenv("LLMQ_PREFILL_PIPE", pipe)
        lens = [33, 129]
        case = prefill_case(4, 2, 128, lens, lens, seed=4)
        run_and_check(case, 129, 0.1, 30.0, 64, False, 2e-2, 1e-1)

    def test_chunked_prefill(self, pipe, monkeypatch):
        """cu_seqlens_k: q row 0 at an offset that is no multiple of 64, and
        an Lq=1 continuation."""
        monkeypatch.setenv("LLMQ_PREFILL_PIPE", pipe)
        q_lens, k_lens = [16, 33, 1], [80, 33, 129]
        case = prefill_case(4, 2, 128, q_lens, k_lens, seed=6)
        run_and_check(case, max(q_lens), 128 ** -0.5, 0.0, 0, True, 4e-2, 1e-1)
