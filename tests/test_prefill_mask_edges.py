"""Mask edges of the prefill attention kernels, on inputs where one key too
many or too few cannot pass.

Kernels: flash_prefill_pipe_kernel (bf16, LLMQ_PREFILL_PIPE=1),
flash_prefill_bf16_kernel (bf16, LLMQ_PREFILL_PIPE=0) and the VALU
varlen_prefill_attention_kernel (fp32 / fp16).

Inputs (built on the CPU from a seed, rounded to the storage dtype before
the reference is taken). v = randn; q and k are 0.5 * randn except in dims 0
and D-1, which carry a positional feature: q at absolute position a holds
amp * (cos ta, sin ta), k at position j holds amp * (cos tj, sin tj), with
amp = sqrt(beta / scale) and t = 2 pi / period. The score is then
beta * cos(t (a - j)) plus noise of std ~0.25. With the window a whole
number of periods the keys just inside and just outside the causal edge AND
the window edge all sit at the score peak, so each of them carries several
percent of its row's weight, and adding or losing one moves the row far.
period = window up to 32, window / 2 above, 16 without a window. (Not
simply `window`, or 32: a key base off by +1 row costs the LAST row of a
sequence only its key 0, in exchange for the neighbour's key 0, both at
score beta * cos(t (L - 1)). Lengths 17 and 33 leave that row alone in its
wave slab, and with period 32 or 64 they put key 0 at the score's minimum,
where the mutant is invisible. The periods above keep it near the peak.)

Tolerance (derived, never tuned). Let A be the reference evaluated with |v|
in place of v: the softmax-weighted mean of |v|, per row and dim.
  * bf16 MFMA kernels round P to bf16 (unit roundoff 2^-8) and the output to
    bf16 (2^-8 again): |out - ref| <= 2^-8 A + 2^-8 |ref| <= 2^-7 A. The
    tests assert 2^-6 A + 2e-5; the factor 2 covers the fp32 terms (l summed
    from unrounded p, __expf, accumulation order) and 2e-5 is the fp32 atol.
  * fp16 VALU kernel: P stays fp32, only the output is rounded (2^-11
    relative): assert 2^-10 A + 2e-5.
  * fp32: 2e-5 + 5e-5 |ref|, as TestPrefillAttention.

Mutants. _attn64 below is an independent fp64 implementation with knobs that
each reproduce one plausible kernel bug (the comparisons of pf_scores, the
rounding of pf_tile_range, the kv-head map, the key base). With every knob
at 0 it must agree with torch_ref. The CPU tests then prove, for every case
of the GPU grid, that each mutant breaks the bf16 tolerance (the loosest of
the three) wherever it changes anything:
  * edge mutants (causal / window / chunk offset, each +-1): EVERY
    (row, head) whose visible key set changes violates;
  * structural mutants (h % KVH head map, key base +-1 row, first in-window
    key tile dropped, last partial key tile dropped): every (sequence, head,
    16-row wave slab) the mutant touches has a violating row.
Measured error ratios and mutant counts: profiles/prefill_mask_edges.md.
"""

from __future__ import annotations

import functools
import math
import zlib
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

from llmq_amd.ops import torch_ref

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TILE = 64  # PF_QT == PF_KT
SLAB = 16  # q rows per wave


class Case(NamedTuple):
    H: int
    KVH: int
    D: int
    q_lens: Tuple[int, ...]
    k_lens: Optional[Tuple[int, ...]] = None  # None: plain prefill
    window: int = 0
    softcap: float = 0.0
    beta: float = 6.0

    @property
    def klens(self):
        return self.q_lens if self.k_lens is None else self.k_lens

    @property
    def period(self):
        # window (16 without one), halved above 32: see the module docstring
        if self.window <= 1:
            return 16.0
        return float(self.window) if self.window <= 32 else self.window / 2.0

    @property
    def scale(self):
        return self.D ** -0.5

    def id(self):
        s = f"H{self.H}k{self.KVH}D{self.D}-q{'_'.join(map(str, self.q_lens))}"
        if self.k_lens is not None:
            s += f"-k{'_'.join(map(str, self.k_lens))}"
        if self.window:
            s += f"-w{self.window}"
        if self.softcap:
            s += f"-cap{self.softcap:g}"
        return s


CAUSAL_LENS = (1, 15, 16, 17, 63, 64, 65, 130)
WINDOW_LENS = (33, 129, 200)
CHUNK_Q, CHUNK_K = (16, 33, 1, 64), (80, 33, 129, 130)

CAUSAL = [Case(H, KVH, D, CAUSAL_LENS)
          for D in (64, 128, 256) for H, KVH in ((4, 2), (6, 2), (4, 4))]
WINDOW = [Case(4, 2, 128, WINDOW_LENS, window=w, softcap=cap)
          for w in (1, 17, 64, 65) for cap in (0.0, 30.0)]
CHUNKED = [Case(4, 2, 128, CHUNK_Q, CHUNK_K, window=w, softcap=cap)
           for w, cap in ((0, 0.0), (17, 0.0), (64, 0.0), (64, 30.0))]
# chunks of more than one q tile at offsets that are no multiple of 64:
# kv_begin differs per q tile and is not the tile of row 0
CHUNKED += [Case(4, 2, 128, (70, 130), (100, 201), window=w, softcap=cap)
            for w, cap in ((17, 0.0), (64, 30.0))]
ZERO_LEN = Case(4, 2, 128, (33, 0, 65))  # cu = [0, 33, 33, 98]
PACKED = Case(4, 2, 128, (33, 65), window=17)
CALL_SITE = [ZERO_LEN, PACKED]
ALL_CASES = CAUSAL + WINDOW + CHUNKED + CALL_SITE

# fp32 / fp16 (VALU kernel): D=128 only, plus one D=64 and one D=256 case.
VALU_CASES = ([c for c in ALL_CASES if c.D == 128]
              + [Case(4, 2, 64, CAUSAL_LENS), Case(6, 2, 256, CAUSAL_LENS)])


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


@functools.lru_cache(maxsize=None)
def _inputs(case: Case, dtype: str = "bf16"):
    """Seeded edge-spiked q/k/v, rounded to `dtype`, plus the offsets."""
    gen = torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()))
    H, KVH, D = case.H, case.KVH, case.D
    cu_q, cu_k = _cu(case.q_lens), _cu(case.klens)
    q = 0.5 * torch.randn(cu_q[-1], H, D, generator=gen, dtype=torch.float64)
    k = 0.5 * torch.randn(cu_k[-1], KVH, D, generator=gen, dtype=torch.float64)
    v = torch.randn(cu_k[-1], KVH, D, generator=gen, dtype=torch.float64)
    amp = math.sqrt(case.beta / case.scale)
    theta = 2.0 * math.pi / case.period
    for b, (Lq, Lk) in enumerate(zip(case.q_lens, case.klens)):
        a = theta * (Lk - Lq + torch.arange(Lq, dtype=torch.float64))
        j = theta * torch.arange(Lk, dtype=torch.float64)
        q[cu_q[b]:cu_q[b + 1], :, 0] = (amp * a.cos())[:, None]
        q[cu_q[b]:cu_q[b + 1], :, D - 1] = (amp * a.sin())[:, None]
        k[cu_k[b]:cu_k[b + 1], :, 0] = (amp * j.cos())[:, None]
        k[cu_k[b]:cu_k[b + 1], :, D - 1] = (amp * j.sin())[:, None]
    dt = DTYPES[dtype]
    return dict(q=q.to(dt), k=k.to(dt), v=v.to(dt),
                cu_q=torch.tensor(cu_q, dtype=torch.int32),
                cu_k=torch.tensor(cu_k, dtype=torch.int32))


def _attn64(case: Case, inp, *, causal=0, win=0, offs=0, head_mod=False,
            leak=0, drop_first=False, drop_last=False, absv=False):
    """Plain fp64 varlen causal/window/chunked GQA attention with mutation
    knobs (all 0 / False: the operation itself). Returns (out [Tq,H,D],
    vis [Tq,Tk] bool: which packed key rows each q row attends to).

      causal    key j visible iff j <= i + causal
      win       ... and j > i - (window + win)           (window cases only)
      offs      i = (Lk - Lq + offs) + row
      head_mod  kv head h % KVH instead of h // (H // KVH)
      leak      key rows start at s0k + leak
      drop_first  the 64-key tile at the q-tile's kv_begin is skipped
      drop_last   the last, partial key tile is skipped
    Rows that see no key are 0."""
    H, KVH, D = case.H, case.KVH, case.D
    q, k = inp["q"].double(), inp["k"].double()
    v = inp["v"].double().abs() if absv else inp["v"].double()
    Tq, Tk = q.shape[0], k.shape[0]
    G = H // KVH
    kv_of = [(h % KVH) if head_mod else (h // G) for h in range(H)]
    kh, vh = k[:, kv_of], v[:, kv_of]  # [Tk, H, D]
    out = torch.zeros(Tq, H, D, dtype=torch.float64)
    vis_all = torch.zeros(Tq, Tk, dtype=torch.bool)
    cu_q, cu_k = inp["cu_q"].tolist(), inp["cu_k"].tolist()
    for b in range(len(cu_q) - 1):
        s, e, sk, ek = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        Lq, Lk = e - s, ek - sk
        if Lq == 0:
            continue
        off = Lk - Lq
        row = torch.arange(Lq).view(-1, 1)
        i = off + offs + row
        j = torch.arange(Lk).view(1, -1)
        vis = j <= i + causal
        if case.window > 0:
            vis &= j > i - (case.window + win)
        if drop_first:
            q_base = (row // TILE) * TILE
            kvb = torch.zeros_like(q_base)
            if case.window > 0:  # pf_tile_range
                kvb = ((off + q_base + 1 - case.window).clamp(min=0)
                       // TILE) * TILE
            vis &= ~((j >= kvb) & (j < kvb + TILE))
        if drop_last and Lk % TILE:
            vis &= j < (Lk // TILE) * TILE
        g = sk + leak + torch.arange(Lk)
        ok = (g >= 0) & (g < Tk)
        vis_g = torch.zeros(Lq, Tk, dtype=torch.bool)
        vis_g[:, g[ok]] = vis[:, ok]
        sc = torch.einsum("ihd,jhd->hij", q[s:e], kh) * case.scale
        if case.softcap > 0:
            sc = torch.tanh(sc / case.softcap) * case.softcap
        sc = sc.masked_fill(~vis_g.unsqueeze(0), float("-inf"))
        p = torch.nan_to_num(torch.softmax(sc, dim=-1), nan=0.0)
        out[s:e] = torch.einsum("hij,jhd->ihd", p, vh)
        vis_all[s:e] = vis_g
    return out, vis_all


@functools.lru_cache(maxsize=None)
def _reference(case: Case, dtype: str = "bf16"):
    """(ref, A, vis) in fp64 from the rounded inputs; shared, read-only."""
    inp = _inputs(case, dtype)
    ref, vis = _attn64(case, inp)
    A, _ = _attn64(case, inp, absv=True)
    return ref, A, vis


def _tolerance(dtype: str, ref, A):
    if dtype == "bf16":
        return 2.0 ** -6 * A + 2e-5
    if dtype == "fp16":
        return 2.0 ** -10 * A + 2e-5
    return 2e-5 + 5e-5 * ref.abs()


def _violating_rows(case, mutant_out, dtype="bf16"):
    """[Tq, H] bool: rows of a mutant output that break the bf16 tolerance
    (the fp16 and fp32 ones lie inside it: |ref| <= A)."""
    ref, A, _ = _reference(case, dtype)
    return ((mutant_out - ref).abs() > _tolerance("bf16", ref, A)).any(dim=-1)


EDGE_MUTANTS = {
    "causal+1": dict(causal=1), "causal-1": dict(causal=-1),
    "window+1": dict(win=1), "window-1": dict(win=-1),
    "offset+1": dict(offs=1), "offset-1": dict(offs=-1),
}
STRUCT_MUTANTS = {
    "head_mod": dict(head_mod=True),
    "leak+1": dict(leak=1), "leak-1": dict(leak=-1),
    "drop_first_tile": dict(drop_first=True),
    "drop_last_tile": dict(drop_last=True),
}


def _touched(case, knobs, vis_mut):
    """[Tq, H] bool: the (row, head) pairs a mutant changes the inputs of."""
    _, _, vis = _reference(case)  # visibility is the same for every dtype
    rows = (vis_mut != vis).any(dim=-1)  # [Tq]
    heads = torch.ones(case.H, dtype=torch.bool)
    if knobs.get("head_mod"):
        G = case.H // case.KVH
        heads = torch.tensor([h % case.KVH != h // G for h in range(case.H)])
        rows = torch.ones_like(rows)
    return rows[:, None] & heads[None, :]


def mutant_census(case):
    """{mutant: (touched (row, head) pairs, violating among them)}."""
    inp = _inputs(case)
    res = {}
    for name, knobs in {**EDGE_MUTANTS, **STRUCT_MUTANTS}.items():
        if name.startswith("window") and not case.window:
            continue
        out, vis_mut = _attn64(case, inp, **knobs)
        t = _touched(case, knobs, vis_mut)
        res[name] = (int(t.sum()), int((t & _violating_rows(case, out)).sum()))
    return res


# ------------------------------------------------------------- CPU tests --

_ids = lambda c: c.id()
# every input set a GPU test runs: all cases in bf16, the VALU ones in its dtypes
INPUT_SETS = ([pytest.param(c, "bf16", id=c.id()) for c in ALL_CASES]
              + [pytest.param(c, d, id=f"{c.id()}-{d}")
                 for c in VALU_CASES for d in ("fp16", "fp32")])


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids)
def test_unmutated_reference_agrees_with_torch_ref(case):
    for dtype in ("bf16", "fp32"):
        inp = _inputs(case, dtype)
        mine, _ = _attn64(case, inp)
        theirs = torch_ref.varlen_prefill_attention(
            inp["q"].float(), inp["k"].float(), inp["v"].float(), inp["cu_q"],
            case.scale, case.softcap, case.window, cu_seqlens_k=inp["cu_k"])
        assert torch.isfinite(mine).all()
        assert (mine - theirs.double()).abs().max().item() <= 1e-5


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids)
def test_edge_keys_sit_at_the_score_peak(case):
    """Construction: the key at the causal edge, and the last key inside the
    window, score within 2 of the row's best key (beta minus noise), so
    each carries at least e^-2 of the heaviest key's weight, in every head."""
    inp = _inputs(case)
    G = case.H // case.KVH
    q, k = inp["q"].double(), inp["k"].double()[:, [h // G for h in range(case.H)]]
    _, _, vis = _reference(case)
    sc = torch.einsum("ihd,jhd->hij", q, k) * case.scale
    if case.softcap > 0:
        sc = torch.tanh(sc / case.softcap) * case.softcap
    p = torch.softmax(sc.masked_fill(~vis.unsqueeze(0), float("-inf")), dim=-1)
    n_vis = vis.sum(dim=-1)  # [Tq]
    assert (n_vis > 0).all()
    last = vis.int().cumsum(dim=-1).argmax(dim=-1)   # causal-edge key
    first = vis.int().argmax(dim=-1)                 # window-edge key
    rows = torch.arange(vis.shape[0])
    floor = math.exp(-2.0) * p.max(dim=-1).values  # [H, Tq]
    assert (p[:, rows, last] >= floor).all()
    if case.window > 1:
        full = n_vis == case.window  # rows whose window is not cut by key 0
        assert full.any()
        assert (p[:, rows, first] >= floor)[:, full].all()


@pytest.mark.parametrize("case,dtype", INPUT_SETS)
def test_edge_mutants_break_every_changed_row(case, dtype):
    """Precondition (no GPU): causal / window / chunk-offset bound off by one
    -> EVERY (row, head) whose visible key set changes breaks the bf16
    tolerance of the GPU tests."""
    inp = _inputs(case, dtype)
    for name, knobs in EDGE_MUTANTS.items():
        if name.startswith("window") and not case.window:
            continue
        out, vis_mut = _attn64(case, inp, **knobs)
        touched = _touched(case, knobs, vis_mut)
        assert touched.any(), name
        missed = touched & ~_violating_rows(case, out, dtype)
        assert not missed.any(), (name, missed.nonzero()[:8].tolist())
        # and rows the mutant leaves alone are bit-equal to the reference
        ref = _reference(case, dtype)[0]
        assert torch.equal(out[~touched], ref[~touched]), name


@pytest.mark.parametrize("case,dtype", INPUT_SETS)
def test_structural_mutants_break_every_touched_slab(case, dtype):
    """Precondition (no GPU): wrong kv-head map, key base off by one row,
    kv_begin one tile late, last partial tile skipped -> every (sequence,
    head, 16-row wave slab) the mutant touches has a violating row."""
    inp = _inputs(case, dtype)
    cu_q = inp["cu_q"].tolist()
    for name, knobs in STRUCT_MUTANTS.items():
        out, vis_mut = _attn64(case, inp, **knobs)
        touched = _touched(case, knobs, vis_mut)
        bad = _violating_rows(case, out, dtype)
        if name == "head_mod" and case.H == case.KVH:
            assert not touched.any()  # G == 1: the two maps coincide
            continue
        if name == "drop_last_tile" and all(n % TILE == 0 for n in case.klens):
            continue
        assert touched.any(), name
        for b in range(len(cu_q) - 1):
            for r0 in range(cu_q[b], cu_q[b + 1], SLAB):
                r1 = min(r0 + SLAB, cu_q[b + 1])
                t, v = touched[r0:r1].any(dim=0), (touched & bad)[r0:r1].any(dim=0)
                assert not (t & ~v).any(), (name, b, r0 - cu_q[b], (t & ~v).tolist())


# ------------------------------------------------------------- GPU tests --

DEV = torch.device("cuda:0")


def _run(case, dtype, max_seqlen=None, packed=False):
    """The op on the GPU at `case`; returns the output on the CPU in fp64."""
    from llmq_amd import ops

    inp = _inputs(case, dtype)
    q, k, v = inp["q"].to(DEV), inp["k"].to(DEV), inp["v"].to(DEV)
    if packed:  # the engine's layout: views of one [T, (H + 2 KVH) D] row
        H, KVH, D = case.H, case.KVH, case.D
        T = q.shape[0]
        qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1)
        q = qkv[:, :H * D].view(T, H, D)
        k = qkv[:, H * D:(H + KVH) * D].view(T, KVH, D)
        v = qkv[:, (H + KVH) * D:].view(T, KVH, D)
        assert not k.is_contiguous()
    if max_seqlen is None:
        max_seqlen = max(case.q_lens)
    out = ops.varlen_prefill_attention(
        q, k, v, inp["cu_q"].to(DEV), max_seqlen, case.scale, case.softcap,
        case.window,
        cu_seqlens_k=None if case.k_lens is None else inp["cu_k"].to(DEV))
    assert out.dtype == DTYPES[dtype] and out.shape == inp["q"].shape
    return out.cpu().double()


def _check(case, dtype, out, label):
    ref, A, _ = _reference(case, dtype)
    err = (out - ref).abs()
    print(f"ERR_RATIO {label} {dtype} {case.id()} "
          f"max|out-ref|/A={(err / A.clamp(min=1e-3)).max().item():.3e} "
          f"max|out-ref|={err.max().item():.3e}")
    assert torch.isfinite(out).all()
    over = err > _tolerance(dtype, ref, A)
    assert not over.any(), (
        label, dtype, case.id(), int(over.sum()), over.nonzero()[:8].tolist(),
        (err / A.clamp(min=1e-3)).max().item())


def _bf16_params(cases):
    return [pytest.param(c, p, id=f"{c.id()}-pipe{p}") for c in cases for p in "01"]


def _valu_params(cases):
    return [pytest.param(c, d, id=f"{c.id()}-{d}")
            for c in cases for d in ("fp32", "fp16")]


@gpu
@needs_gpu
@pytest.mark.parametrize("case,pipe", _bf16_params(CAUSAL + WINDOW + CHUNKED))
def test_flash_prefill_mask_edges(case, pipe, monkeypatch):
    monkeypatch.setenv("LLMQ_PREFILL_PIPE", pipe)
    _check(case, "bf16", _run(case, "bf16"), f"flash_pipe{pipe}")


@gpu
@needs_gpu
@pytest.mark.parametrize(
    "case,dtype",
    _valu_params([c for c in VALU_CASES if c not in CALL_SITE]))
def test_valu_prefill_mask_edges(case, dtype):
    _check(case, dtype, _run(case, dtype), "valu")


def _kernel_params():
    return [pytest.param("bf16", "1", id="pipe"), pytest.param("bf16", "0", id="plain"),
            pytest.param("fp16", None, id="valu-fp16"),
            pytest.param("fp32", None, id="valu-fp32")]


def _select(monkeypatch, pipe):
    if pipe is not None:
        monkeypatch.setenv("LLMQ_PREFILL_PIPE", pipe)


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype,pipe", _kernel_params())
class TestCallSiteShapes:
    def test_packed_qkv_views(self, dtype, pipe, monkeypatch):
        """q/k/v as strided views of one packed qkv row, as the engine passes
        them (row strides differ from H*D / KVH*D)."""
        _select(monkeypatch, pipe)
        _check(PACKED, dtype, _run(PACKED, dtype, packed=True), f"packed-{pipe}")

    @pytest.mark.parametrize("extra", [1, 64])
    def test_max_seqlen_past_longest(self, dtype, pipe, extra, monkeypatch):
        """Extra q-tiles in the grid exit early and write nothing."""
        _select(monkeypatch, pipe)
        case = CAUSAL[3]  # H4 KVH2 D128
        out = _run(case, dtype, max_seqlen=max(case.q_lens) + extra)
        _check(case, dtype, out, f"maxlen+{extra}-{pipe}")

    def test_zero_length_sequence(self, dtype, pipe, monkeypatch):
        """cu = [0, 33, 33, 98]: an empty sequence between two real ones."""
        _select(monkeypatch, pipe)
        assert _inputs(ZERO_LEN, dtype)["cu_q"].tolist() == [0, 33, 33, 98]
        _check(ZERO_LEN, dtype, _run(ZERO_LEN, dtype), f"zero-len-{pipe}")

    def test_out_halo_stays_intact(self, dtype, pipe, monkeypatch):
        """The raw op with `out` an inner row-slice of a canary buffer: rows
        before and after stay bit-intact, every row inside is written."""
        from llmq_amd import ops

        _select(monkeypatch, pipe)
        assert ops.has_hip_ext()
        case = CHUNKED[1]  # chunked + window 17: every index path at once
        inp = _inputs(case, dtype)
        T, PAD = inp["q"].shape[0], 5
        buf = torch.full((T + 2 * PAD, case.H, case.D), -7.25,
                         dtype=DTYPES[dtype], device=DEV)
        canary = buf.cpu().clone()
        out = buf[PAD:PAD + T]
        torch.ops.llmq_amd.varlen_prefill_attention(
            out, inp["q"].to(DEV), inp["k"].to(DEV), inp["v"].to(DEV),
            inp["cu_q"].to(DEV), inp["cu_k"].to(DEV), max(case.q_lens) + 64,
            case.scale, case.softcap, case.window)
        torch.cuda.synchronize()
        got = buf.cpu()
        as_bits = lambda t: t.contiguous().view(torch.uint8)
        assert torch.equal(as_bits(got[:PAD]), as_bits(canary[:PAD]))
        assert torch.equal(as_bits(got[PAD + T:]), as_bits(canary[PAD + T:]))
        assert torch.isfinite(got[PAD:PAD + T]).all()
        _check(case, dtype, got[PAD:PAD + T].double(), f"canary-{pipe}")


@gpu
@needs_gpu
def test_binding_rejects_bad_operands():
    """Every precondition of the binding raises on the host, before any
    launch; the unmodified call passes."""
    from llmq_amd import ops

    assert ops.has_hip_ext()
    op = torch.ops.llmq_amd.varlen_prefill_attention
    H, KVH, D, T = 4, 2, 128, 40
    bf = dict(dtype=torch.bfloat16, device=DEV)

    def good():
        return dict(
            out=torch.zeros(T, H, D, **bf), q=torch.zeros(T, H, D, **bf),
            k=torch.zeros(T, KVH, D, **bf), v=torch.zeros(T, KVH, D, **bf),
            cu=torch.tensor([0, 7, T], dtype=torch.int32, device=DEV),
            cu_k=torch.tensor([0, 7, T], dtype=torch.int32, device=DEV),
            max_seqlen=T, scale=0.1, softcap=0.0, window=0)

    def call(a):
        op(a["out"], a["q"], a["k"], a["v"], a["cu"], a["cu_k"], a["max_seqlen"],
           a["scale"], a["softcap"], a["window"])

    call(good())
    torch.cuda.synchronize()

    def shifted(t, elems):  # same shape and strides, base moved by `elems`
        flat = torch.zeros(t.numel() + 64, **bf)
        return flat.as_strided(t.shape, t.stride(), elems)

    def padded_rows(t, pad):  # row stride = heads*D + pad
        wide = torch.zeros(t.shape[0], t.shape[1] * D + pad, **bf)
        return wide[:, :t.shape[1] * D].view(t.shape)

    bad = {
        "k on the CPU": lambda a: a.update(k=a["k"].cpu()),
        "q on the CPU": lambda a: a.update(q=a["q"].cpu()),
        "out on the CPU": lambda a: a.update(out=a["out"].cpu()),
        "v dtype": lambda a: a.update(v=a["v"].half()),
        "k dtype": lambda a: a.update(k=a["k"].float()),
        "out dtype": lambda a: a.update(out=a["out"].float()),
        "q 2-D": lambda a: a.update(q=a["q"].view(T, H * D)),
        "k 4-D": lambda a: a.update(k=a["k"].view(T, KVH, 2, D // 2)),
        "v last-dim stride 2": lambda a: a.update(
            v=torch.zeros(T, KVH, 2 * D, **bf)[:, :, ::2]),
        "k head stride 2D": lambda a: a.update(
            k=torch.zeros(T, KVH, 2 * D, **bf)[:, :, :D]),
        "q head stride 2D": lambda a: a.update(
            q=torch.zeros(T, H, 2 * D, **bf)[:, :, :D]),
        "k head_dim": lambda a: a.update(k=torch.zeros(T, KVH, 64, **bf)),
        "v rows": lambda a: a.update(v=torch.zeros(T - 1, KVH, D, **bf)),
        "out rows": lambda a: a.update(out=torch.zeros(T + 1, H, D, **bf)),
        "H % KVH": lambda a: a.update(k=torch.zeros(T, 3, D, **bf),
                                      v=torch.zeros(T, 3, D, **bf)),
        "cu lengths differ": lambda a: a.update(cu_k=a["cu_k"][:2]),
        "cu empty": lambda a: a.update(cu=a["cu"][:0], cu_k=a["cu_k"][:0]),
        "cu int64": lambda a: a.update(cu=a["cu"].long()),
        "cu_k on the CPU": lambda a: a.update(cu_k=a["cu_k"].cpu()),
        "window < 0": lambda a: a.update(window=-1),
        "max_seqlen < 0": lambda a: a.update(max_seqlen=-1),
        "k base 8-byte aligned": lambda a: a.update(k=shifted(a["k"], 4)),
        "q base 2-byte aligned": lambda a: a.update(q=shifted(a["q"], 1)),
        "out base 8-byte aligned": lambda a: a.update(out=shifted(a["out"], 4)),
        "v row stride % 8": lambda a: a.update(v=padded_rows(a["v"], 4)),
        "q row stride % 8": lambda a: a.update(q=padded_rows(a["q"], 4)),
    }
    for name, mutate in bad.items():
        args = good()
        mutate(args)
        with pytest.raises(RuntimeError):
            call(args)
            raise AssertionError(f"the binding accepted: {name}")
    # strided but legal operands (row padding of 8 elements) still pass
    args = good()
    args.update(k=padded_rows(args["k"], 8), v=padded_rows(args["v"], 8))
    call(args)
    torch.cuda.synchronize()
