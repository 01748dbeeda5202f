"""V "line image" of the bf16 pipe decode kernel.

The kernel stages V in LDS as pieces of 8 keys x 64 dims (eight whole
128-byte cache lines per DMA instruction, so V can stream `nt`);
LLMQ_DECODE_V_LINES=0 (read per call) selects the earlier tr16 subtile image.
The PV operands and the MFMA order are the same in both, so:

(a) the two images agree bit for bit, under every LLMQ_DECODE_KV_NT value
    (0 = default cache policy, 1 = K `nt`, 2 = K and V `nt`), on the bf16
    cases and context lengths of test_decode_kv_policy; where _case has the
    fp32 reference, the result also matches it within that file's tolerances;

(b) a one-key "needle" run returns V[t] bit for bit. K is zero except row t,
    which is aligned with q: the needle's logit is at least 16 * sqrt(D) >=
    181 after scaling and every other key's is 0, a margin > 104, so expf of
    every other key is exactly 0 in fp32, l = 1, P is a one-hot bf16 row and
    the output row is exactly row t of V for every q head. Each element of V
    is a distinct bf16-exact code of (key, 16-byte granule, position in the
    granule), so exchanging any two granules of the LDS image changes the
    output of the sequence whose needle is one of their keys. The targets are
    every key of the first chunk, three of the second and three of the
    partial tail chunk, one sequence each (cycled up to 512 sequences so that
    the launch is not split-KV), all in one launch per configuration.
"""

from __future__ import annotations

import functools

import pytest
import torch

from tests.test_decode_gqa_rows import ATOL, CTX, RTOL, _case, _id

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from llmq_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")

# test_decode_kv_policy's context lengths: _case's own set (1, 63, 65, 130:
# has the reference), the chunk edges from the other side, a ragged batch.
LENS = (CTX, (64, 129, 1, 65), (17, 100, 128, 33))
POLICIES = ("0", "1", "2")


def _grid():
    """The bf16 cases of test_decode_kv_policy._grid."""
    out = []
    for D in (128, 256):
        for G in (1, 2, 5, 12):
            for softcap in (0.0, 50.0):
                out.append(dict(G=G, D=D, softcap=softcap))
        out.append(dict(G=2, D=D, softcap=50.0, window=40))
        out.append(dict(G=5, D=D, bs=32))
        out.append(dict(G=2, D=D, split=True))  # one sequence, 16 z-slices
    return out


@pytest.mark.parametrize(
    "kw,pipe", [(kw, p) for kw in _grid() for p in ("64", "128")],
    ids=lambda v: v if isinstance(v, str) else _id(v))
def test_line_image_equals_subtile_image(kw, pipe, monkeypatch):
    monkeypatch.setenv("LLMQ_DECODE_PIPE", pipe)
    c = _case(**kw)
    q, kc, vc, bt = (c[n].to(DEV) for n in ("q", "kc", "vc", "bt"))
    lens = (tuple(c["cl"].tolist()),) if kw.get("split") else LENS

    def run(cl):
        return ops.paged_decode_attention(
            q, kc, vc, bt, cl, c["scale"], c["softcap"], c["window"])

    for ls in lens:
        cl = torch.tensor(ls, dtype=torch.int32, device=DEV)
        monkeypatch.delenv("LLMQ_DECODE_KV_NT", raising=False)
        monkeypatch.delenv("LLMQ_DECODE_V_LINES", raising=False)
        unset = run(cl)
        for policy in POLICIES:
            monkeypatch.setenv("LLMQ_DECODE_KV_NT", policy)
            monkeypatch.setenv("LLMQ_DECODE_V_LINES", "0")
            subtile = run(cl)
            monkeypatch.setenv("LLMQ_DECODE_V_LINES", "1")
            lines = run(cl)
            monkeypatch.delenv("LLMQ_DECODE_V_LINES")
            default = run(cl)
            assert torch.equal(subtile, lines), (kw, pipe, ls, policy)
            assert torch.equal(default, lines), (kw, pipe, ls, policy)
            assert torch.equal(unset, lines), (kw, pipe, ls, policy)
        if ls == tuple(c["cl"].tolist()):  # all are the right answer
            torch.testing.assert_close(
                unset.float().cpu(), c["ref"], atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------- needle --

NEEDLE_B = 512  # B x 1 kv head >= 512 workgroups: the launcher does not split


def _v_code(L, D):
    """[L, D] fp32, every value exact in bf16 (<= 8 significant bits), every
    16-byte granule (key, g = dim // 8) distinct from every other and its
    eight positions j = dim % 8 distinct from each other:
      j 0  1 + (key % 128) / 128        j 4  -(1 + (key % 128) / 128)
      j 1  2 + key // 128               j 5  128 + 2 g
      j 2  8 + g                        j 6  -(8 + g)
      j 3  64 + key % 64                j 7  256 + 2 (key % 64)
    """
    key = torch.arange(L, dtype=torch.float32)[:, None].expand(L, D)
    dim = torch.arange(D)[None, :].expand(L, D)
    g, j = (dim // 8).float(), dim % 8
    k128 = 1.0 + torch.remainder(key, 128) / 128.0
    k64 = torch.remainder(key, 64)
    fields = [k128, 2.0 + torch.div(key, 128, rounding_mode="floor"), 8.0 + g,
              64.0 + k64, -k128, 128.0 + 2.0 * g, -(8.0 + g), 256.0 + 2.0 * k64]
    v = torch.zeros(L, D)
    for jj, f in enumerate(fields):
        v = torch.where(j == jj, f, v)
    assert torch.equal(v.to(torch.bfloat16).float(), v)
    gran = v.view(L, D // 8, 8)
    assert len({tuple(r) for r in gran.reshape(-1, 8).tolist()}) == L * D // 8
    return v


@functools.lru_cache(maxsize=None)
def _needle(D, G, KT, bs):
    L = 2 * KT + 21  # two whole chunks and a partial tail chunk
    targets = list(range(KT)) + [KT, KT + 9, 2 * KT - 1, 2 * KT, 2 * KT + 7, L - 1]
    t = torch.tensor([targets[i % len(targets)] for i in range(NEEDLE_B)])
    nblk = (L + bs - 1) // bs
    gen = torch.Generator().manual_seed(D + G + KT + bs)
    # every sequence has blocks of its own, in a random order; block 0 unused
    bt = (torch.randperm(NEEDLE_B * nblk, generator=gen) + 1).to(torch.int32)
    bt = bt.view(NEEDLE_B, nblk)
    u = torch.where(torch.rand(D, generator=gen) < 0.5, -1.0, 1.0)  # +-1 per dim
    heads = 4.0 + (torch.arange(G) % 4).float()                     # 4..7
    q = (heads[None, :, None] * u[None, None, :]).expand(NEEDLE_B, G, D)
    v_seq = _v_code(L, D)
    pad = nblk * bs - L
    v_blocks = torch.cat([v_seq, torch.full((pad, D), 999.0)]).view(nblk, bs, D)
    return dict(L=L, t=t, bt=bt, q=q.contiguous().to(torch.bfloat16), u=u,
                v_seq=v_seq, v_blocks=v_blocks.to(torch.bfloat16), nblk=nblk)


@pytest.mark.parametrize("D,G,KT,bs", [
    (D, G, KT, 16) for D in (128, 256) for G in (2, 5) for KT in (64, 128)
] + [(256, 2, 64, 32)], ids=lambda v: str(v))
def test_needle_returns_v_row(D, G, KT, bs, monkeypatch):
    monkeypatch.setenv("LLMQ_DECODE_PIPE", str(KT))
    c = _needle(D, G, KT, bs)
    B, L, nblk = NEEDLE_B, c["L"], c["nblk"]
    bt, t = c["bt"].to(DEV), c["t"].to(DEV)
    seq = torch.arange(B, device=DEV)
    kc = torch.zeros(B * nblk + 1, 1, bs, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.full_like(kc, 777.0)
    vc[bt.long().view(-1), 0] = c["v_blocks"].to(DEV).repeat(B, 1, 1)
    kc[bt[seq, t // bs].long(), 0, t % bs] = (4.0 * c["u"]).to(DEV, torch.bfloat16)
    cl = torch.full((B,), L, dtype=torch.int32, device=DEV)
    want = c["v_seq"].to(DEV, torch.bfloat16)[t][:, None, :].expand(B, G, D)
    assert 16.0 * D ** 0.5 > 104.0  # the needle's margin after scaling
    for lines in ("1", "0"):
        monkeypatch.setenv("LLMQ_DECODE_V_LINES", lines)
        for policy in ("2", "0"):
            monkeypatch.setenv("LLMQ_DECODE_KV_NT", policy)
            out = ops.paged_decode_attention(
                c["q"].to(DEV), kc, vc, bt, cl, D ** -0.5, 0.0, 0)
            bad = (out != want).any(dim=-1).any(dim=-1).nonzero().flatten()
            assert bad.numel() == 0, (
                lines, policy, "first wrong sequences (target keys):",
                t[bad[:8]].tolist())
