"""rope_and_cache on the vector path (the fused QK-norm kernel's mapping with
the norm compiled out) against the scalar rope_and_cache_kernel.

The scalar kernel is the reference: LLMQ_ROPE_VEC=0 selects it per call. All
four outputs (q, k, the cache's K rows, the cache's V rows) must be
bit-identical, for bf16 and fp8-e4m3 caches, pad rows (slot -1) included:
those rotate q and k and leave the cache untouched. q/k/v are `split` views
of one packed qkv buffer, as the model passes them.

Shapes outside the vector envelope (a head dim other than 64/128/256, fp32)
must keep the scalar kernel: they are held to torch_ref.
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
BS, NB, MAX_POS = 16, 4, 512
SENTINEL = -3.0  # exact in fp32, bf16 and e4m3
TOL = {torch.float32: (1e-5, 1e-5), torch.bfloat16: (2e-2, 2e-2)}


def _inputs(T, HQ, HK, D, dtype, cache_dtype, seed, nb=NB):
    gen = torch.Generator().manual_seed(seed)
    cos_sin = torch_ref.build_rope_cache(MAX_POS, D, 10000.0, DEV)
    qkv = torch.randn(T, (HQ + 2 * HK) * D, generator=gen).to(dtype).to(DEV)
    # positions include 0 and the table's last row
    pos = torch.randint(0, MAX_POS, (T,), generator=gen)
    pos[0] = MAX_POS - 1
    if T > 1:
        pos[1] = 0
    # valid slots include the first and the last slot of the pool; every
    # fourth row from row 2 on is a pad row
    slots = torch.randperm(nb * BS - 2, generator=gen)[:T] + 1
    slots[0] = nb * BS - 1
    if T > 1:
        slots[1] = 0
    slots[2::4] = -1
    assert len(set(slots[slots >= 0].tolist())) == int((slots >= 0).sum())
    kc = torch.full((nb, HK, BS, D), SENTINEL, dtype=torch.float32).to(cache_dtype).to(DEV)
    return qkv, pos.to(DEV), slots.to(DEV), cos_sin, kc, kc.clone()


def _run(qkv, HQ, HK, D, pos, slots, cos_sin, kc, vc):
    """rope_and_cache on fresh copies; q/k/v are split views of the packed
    buffer (row stride (HQ + 2 HK) * D, not the view's own width)."""
    qkv, kc, vc = qkv.clone(), kc.clone(), vc.clone()
    T = qkv.shape[0]
    q, k, v = qkv.split([HQ * D, HK * D, HK * D], dim=-1)
    q, k, v = q.view(T, HQ, D), k.view(T, HK, D), v.view(T, HK, D)
    if T > 1:  # a one-row view is contiguous and its row stride arbitrary
        assert q.stride(0) == (HQ + 2 * HK) * D and not q.is_contiguous()
    ops.rope_and_cache(q, k, v, kc, vc, pos, cos_sin, slots)
    torch.cuda.synchronize()
    return qkv, kc, vc


def _bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int16)


# T = 257 (one shape) is there for the rounding: the two kernels differ only
# if the compiler contracts the rotation differently, which changes one bf16
# result in about 10^5 (with the other contraction of the high half, T = 17
# showed ONE differing element at three of the four shapes and none at the
# fourth). 257 rows x 24 heads x 256 are 1.6 million results.
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
@pytest.mark.parametrize(
    "T,HQ,HK,D",
    [(T, *s) for T in (1, 3, 17)
     for s in [(16, 8, 256), (32, 8, 128), (4, 4, 64), (2, 1, 256)]]
    + [(257, 16, 8, 256)])
def test_vector_path_is_bit_identical(T, HQ, HK, D, cache, monkeypatch):
    cdt = torch.bfloat16 if cache == "bf16" else torch.float8_e4m3fn
    nb = max(NB, (T + 2 + BS - 1) // BS)
    qkv, pos, slots, cos_sin, kc, vc = _inputs(
        T, HQ, HK, D, torch.bfloat16, cdt, seed=T * 1000 + HQ * 10 + D, nb=nb)
    monkeypatch.setenv("LLMQ_ROPE_VEC", "0")
    old = _run(qkv, HQ, HK, D, pos, slots, cos_sin, kc, vc)
    monkeypatch.delenv("LLMQ_ROPE_VEC")
    new = _run(qkv, HQ, HK, D, pos, slots, cos_sin, kc, vc)

    # q, k (rotated in place) and v (only read), as one packed buffer
    assert torch.equal(_bits(old[0]), _bits(new[0]))
    assert torch.equal(_bits(old[1]), _bits(new[1]))  # cache K rows
    assert torch.equal(_bits(old[2]), _bits(new[2]))  # cache V rows

    # the comparison is not vacuous: the reference rotated and cached
    qk = (HQ + HK) * D
    assert not torch.equal(old[0][:, :qk], qkv[:, :qk])
    assert torch.equal(old[0][:, qk:], qkv[:, qk:])
    written = torch.zeros(nb * BS, dtype=torch.bool)
    written[slots[slots >= 0].cpu()] = True
    for cache_t in (new[1], new[2]):
        rows = cache_t.float().cpu().transpose(1, 2).reshape(nb * BS, HK * D)
        assert (rows[~written] == SENTINEL).all()  # pad rows wrote nothing
        assert not (rows[written] == SENTINEL).all(dim=1).any()
    # cached K is the rotated k (quantized for fp8), cached V is v
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            k_t = new[0][t, HQ * D:qk].view(HK, D)
            v_t = new[0][t, qk:].view(HK, D)
            assert torch.equal(new[1][s // BS, :, s % BS].float(), k_t.to(cdt).float())
            assert torch.equal(new[2][s // BS, :, s % BS].float(), v_t.to(cdt).float())


@pytest.mark.parametrize("D,dtype", [(96, torch.bfloat16), (96, torch.float32),
                                     (128, torch.float32)])
def test_outside_the_envelope_keeps_scalar_kernel(D, dtype, monkeypatch):
    """D = 96 has no vector instantiation and fp32 is not a 2-byte T: both
    take rope_and_cache_kernel whatever the switch says, and match the
    reference."""
    T, HQ, HK = 17, 4, 2
    qkv, pos, slots, cos_sin, kc, vc = _inputs(T, HQ, HK, D, dtype, dtype, seed=D)
    q_ref, k_ref, v_ref = (
        t.reshape(T, -1, D).float().cpu().clone()
        for t in qkv.split([HQ * D, HK * D, HK * D], dim=-1))
    torch_ref.rope_inplace(q_ref, k_ref, pos.cpu(), cos_sin.cpu())
    keep = (slots >= 0).cpu()
    kc_ref, vc_ref = kc.float().cpu().clone(), vc.float().cpu().clone()
    torch_ref.reshape_and_cache(k_ref[keep], v_ref[keep], kc_ref, vc_ref,
                                slots.cpu()[keep])

    outs = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("LLMQ_ROPE_VEC", sw)
        outs[sw] = _run(qkv, HQ, HK, D, pos, slots, cos_sin, kc, vc)
    for a, b in zip(outs["0"], outs["1"]):
        assert torch.equal(a, b)
    got, kc_out, vc_out = outs["1"]
    atol, rtol = TOL[dtype]
    q, k, v = got.split([HQ * D, HK * D, HK * D], dim=-1)
    torch.testing.assert_close(q.reshape(T, HQ, D).float().cpu(), q_ref, atol=atol, rtol=rtol)
    torch.testing.assert_close(k.reshape(T, HK, D).float().cpu(), k_ref, atol=atol, rtol=rtol)
    torch.testing.assert_close(kc_out.float().cpu(), kc_ref, atol=atol, rtol=rtol)
    assert torch.equal(vc_out.float().cpu(), vc_ref)  # pure copy
