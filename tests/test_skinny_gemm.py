"""Skinny-M projection GEMM (ops/hip/skinny_gemm.hip) against an exact reference.

x, w and bias are small integers stored as bf16 (x in {-1,0,1}, w in {-2..2},
bias in {-3..3}). Every product and every partial sum is then an integer far
below 2^24, so fp32 accumulation is exact in ANY order: any MFMA ordering, any
split-K partition, any slab refold. The only rounding left is the kernel's
final __float2bfloat16, which the fp64 reference applies too, so the GPU tests
compare with torch.equal and carry no tolerance. The sums stay at or below
256 (checked for K <= 128, where it is also a hard bound), so they are exact
in bf16 and one missing, duplicated or misplaced nonzero term changes bits.

The CPU-only tests check those preconditions on the very inputs the GPU tests
use, check that the reference can see the faults this kernel could make (rows
or columns exchanged, a lost 16-byte K granule, the st_16x32 swizzle applied
on one side only), and mirror the binding's split-K slice rule.

Shapes are the smallest that reach every branch of the 256x256x64 tile: M and
N tails in every wave half/quarter, a nearly empty second tile, and K-step
counts of 1 (prologue only), 2 (both LDS buffers), 3 (buffer reuse) and 5.
"""

from __future__ import annotations

import functools
import json
import os
import subprocess
import sys

import pytest
import torch

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
SEED = 20242  # one at which every detectability check below holds
BK = 64  # SKG_BK

MS = (1, 7, 129, 255, 256, 257)
NS = (4, 60, 252, 256, 260, 516)
KS = (64, 128, 192, 320)


def _grid():
    """Every (M, N) at K=192, every K at (257, 260), and a few more corners
    at the other K-step counts."""
    cases = [(M, N, 192) for M in MS for N in NS]
    cases += [(257, 260, K) for K in KS if K != 192]
    cases += [(1, 4, 64), (7, 60, 128), (129, 252, 320), (255, 516, 64),
              (256, 256, 128), (256, 256, 320), (1, 516, 320)]
    return cases


SPLIT_M, SPLIT_N = 129, 260
SPLIT_CASES = [(K, z) for K in (64, 192, 320, 512) for z in (1, 2, 3, 4, 8)]
AUTO_M, AUTO_N = 16, 256
AUTO_CASES = [(1024, 2), (2048, 4), (4096, 8)]  # (K, z the auto rule picks)


def _id(case):
    return "x".join(str(v) for v in case)


def _reference(x, w, bias):
    ref = x.double() @ w.double().T
    if bias is not None:
        ref = ref + bias.double()
    return ref


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Seeded integer inputs and their exact references, built once on the
    CPU and shared (read-only) by every test that runs the shape."""
    gen = torch.Generator().manual_seed(SEED + 1000003 * M + 1009 * N + K)
    x = torch.randint(-1, 2, (M, K), generator=gen)
    # no all-zero 16-byte granule: losing one must always change the sums
    xg = x.view(M, K // 8, 8)
    xg[..., 0] += (xg == 0).all(dim=2).to(x.dtype)
    x = x.to(BF16)
    w = torch.randint(-2, 3, (N, K), generator=gen).to(BF16)
    bias = torch.randint(-3, 4, (N,), generator=gen).to(BF16)
    refd = {False: _reference(x, w, None), True: _reference(x, w, bias)}
    ref = {b: r.float().to(BF16) for b, r in refd.items()}
    return dict(x=x, w=w, bias=bias, refd=refd, ref=ref)


def _all_shapes():
    shapes = list(_grid())
    shapes += [(SPLIT_M, SPLIT_N, K) for K in (64, 192, 320, 512)]
    shapes += [(AUTO_M, AUTO_N, K) for K, _ in AUTO_CASES]
    return sorted(set(shapes))


# ------------------------------------------------ split-K slice rule (CPU) --


def _auto_z(M, N, K):
    """splitk=0 in bindings.cpp: fill the chip, keep >= 8 K-steps a slice."""
    mt, nt, ksteps = -(-M // 256), -(-N // 256), K // BK
    z = 1
    while mt * nt * z < 256 and ksteps // (z * 2) >= 8 and z < 8:
        z *= 2
    return z


def _kernel_slices(ksteps, nsplit):
    """The kernel's K-step range per blockIdx.z, for gridDim.z = nsplit."""
    per = -(-ksteps // nsplit)
    return [(s * per, min(ksteps, s * per + per)) for s in range(nsplit)]


def _binding_z(ksteps, z):
    """The binding's trim: drop the slices ceil-division leaves empty."""
    per = -(-ksteps // z)
    return -(-ksteps // per)


def _slices(ksteps, z):
    return _kernel_slices(ksteps, _binding_z(ksteps, z))


def test_slice_rule_covers_k_exactly_once():
    for ksteps in range(1, 65):
        for z in range(1, 17):
            sl = _slices(ksteps, z)
            assert 1 <= len(sl) <= z
            assert all(a < b for a, b in sl), (ksteps, z, sl)  # non-empty
            assert sl[0][0] == 0 and sl[-1][1] == ksteps, (ksteps, z, sl)
            assert all(p[1] == n[0] for p, n in zip(sl, sl[1:])), (ksteps, z, sl)


def test_untrimmed_slice_rule_leaves_empty_slices():
    """What the trim is for: with gridDim.z = splitk as requested, these
    combinations (all in SPLIT_CASES) have a slice with no K-step, whose
    fp32 slab the kernel never writes and the reduce still sums."""
    for K, z in ((320, 4), (192, 8), (64, 2), (320, 8)):
        assert (K, z) in SPLIT_CASES
        assert any(a >= b for a, b in _kernel_slices(K // BK, z)), (K, z)
        assert all(a < b for a, b in _slices(K // BK, z)), (K, z)


def test_auto_split_is_unchanged_by_the_trim():
    for K, z in AUTO_CASES:
        assert _auto_z(AUTO_M, AUTO_N, K) == z
    for M, N, K in _grid():
        assert _auto_z(M, N, K) == 1
    for tiles in (1, 2, 3, 7, 31, 32, 64, 128, 255, 256):
        for ksteps in range(1, 513):
            z = _auto_z(256 * tiles, 256, BK * ksteps)
            assert _binding_z(ksteps, z) == z, (tiles, ksteps, z)


# ------------------------------------------- exactness preconditions (CPU) --


@pytest.mark.parametrize("shape", _all_shapes(), ids=_id)
def test_partial_sums_stay_exact_in_fp32(shape):
    c = _case(*shape)
    worst = (c["x"].double().abs() @ c["w"].double().abs().T).max().item()
    worst += c["bias"].double().abs().max().item()
    assert worst < 2 ** 24  # bounds every partial sum, in any order
    for refd in c["refd"].values():
        assert torch.equal(refd, refd.round())


@pytest.mark.parametrize("shape", [s for s in _all_shapes() if s[2] <= 128], ids=_id)
def test_small_k_outputs_are_exact_in_bf16(shape):
    c = _case(*shape)
    for b in (False, True):
        refd = c["refd"][b]
        assert torch.equal(refd, refd.round())
        assert refd.abs().max().item() <= 256
        assert torch.equal(c["ref"][b].double(), refd)


def _swz_cols(K):
    return torch.arange(K) ^ 16  # skg_swz: col ^= ((row >> 3) & 1) << 4


@pytest.mark.parametrize("shape", _grid(), ids=_id)
def test_reference_sees_kernel_faults(shape):
    """Precondition (no GPU): each fault below, applied to the expected
    output, fails the torch.equal the GPU tests make."""
    M, N, K = shape
    c = _case(*shape)
    x, w, bias = c["x"], c["w"], c["bias"]
    for b in (False, True):
        ref = c["ref"][b]
        bb = bias if b else None
        rnd = lambda d: d.float().to(BF16)  # noqa: E731
        # two output rows / columns exchanged
        for i, j in ((0, M - 1), (0, 1), (M // 2, M - 1)):
            if M >= 2 and i != j:
                sw = ref.clone()
                sw[i], sw[j] = ref[j], ref[i]
                assert not torch.equal(sw, ref), ("rows", shape, i, j)
        for i, j in ((0, N - 1), (0, 1), (N // 2, N - 1)):
            sw = ref.clone()
            sw[:, i], sw[:, j] = ref[:, j], ref[:, i]
            assert not torch.equal(sw, ref), ("cols", shape, i, j)
        # with enough entries per row / column, no two are alike at all
        if N >= 60:
            assert torch.unique(ref, dim=0).shape[0] == M
        if M >= 129:
            assert torch.unique(ref, dim=1).shape[1] == N
        # one 8-element (16-byte) K granule of x lost, in all rows ...
        xg = x.double().view(M, K // 8, 8)
        wg = w.double().view(N, K // 8, 8)
        part = torch.einsum("mgk,ngk->gmn", xg, wg)  # per-granule terms
        full = c["refd"][b]
        for g in range(K // 8):
            assert not torch.equal(rnd(full - part[g]), ref), ("granule", shape, g)
        # ... or in a single row (needs enough columns to show)
        if N >= 60:
            seen = (rnd(full.unsqueeze(0) - part) != ref.unsqueeze(0)).any(dim=2)
            assert bool(seen.all()), ("row granule", shape)
        # the swizzle applied to one operand only: rows with bit 3 set read
        # their two 16-column halves exchanged
        for name, t, rows in (("x", x, M), ("w", w, N)):
            hit = ((torch.arange(rows) >> 3) & 1).bool()
            if not bool(hit.any()):
                continue  # fewer than 9 rows: the swizzle is the identity
            f = t.clone()
            f[hit] = t[hit][:, _swz_cols(K)]
            bad = _reference(f, w, bb) if name == "x" else _reference(x, f, bb)
            assert not torch.equal(rnd(bad), ref), ("swizzle", name, shape)


def test_wrapper_preconditions_on_cpu_views():
    """The staging predicate of ops.skinny_gemm, and its F.linear fallback
    (exact on this data, out= honoured) -- no GPU involved."""
    from llmq_amd import ops

    K = 64
    buf = torch.zeros(8, K + 64, dtype=BF16)
    assert buf.data_ptr() % 16 == 0
    assert ops._skg_stageable(buf)
    assert ops._skg_stageable(buf[:, :K])          # row-strided, legal
    assert ops._skg_stageable(buf[:, 8:8 + K])     # 16-byte column offset
    assert not ops._skg_stageable(buf[:, 4:4 + K])  # 8-byte column offset
    assert not ops._skg_stageable(torch.zeros(8, K + 4, dtype=BF16)[:, :K])
    assert not ops._skg_stageable(torch.zeros(8, 2 * K, dtype=BF16)[:, ::2])
    c = _case(7, 60, 128)
    out = torch.full((7, 60), float("nan"), dtype=BF16)
    got = ops.skinny_gemm(c["x"], c["w"], c["bias"], out=out)
    assert got is out
    assert torch.equal(out, c["ref"][True])


# ------------------------------------------------------------------- GPU --


def _dev():
    return torch.device("cuda:0")


def _poison(n):
    """Best effort: leave NaNs in the block the caching allocator will most
    likely hand out next for an fp32 tensor of n elements."""
    junk = torch.full((n,), float("nan"), dtype=torch.float32, device=_dev())
    del junk


def _run(x, w, bias, splitk, poison=0):
    """The raw op (no wrapper, so no fallback) into a NaN-filled output: an
    element the kernel does not write cannot pass as a stale right answer."""
    from llmq_amd import ops

    assert ops.has_hip_ext()
    M, N = x.shape[0], w.shape[0]
    out = torch.full((M, N), float("nan"), dtype=BF16, device=x.device)
    if poison:
        _poison(poison)
    torch.ops.llmq_amd.skinny_gemm(out, x, w, bias, splitk)
    return out.cpu()


@gpu
@needs_gpu
@pytest.mark.parametrize("sync", ("0", "1"))
@pytest.mark.parametrize("with_bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("shape", _grid(), ids=_id)
def test_exact_over_shape_grid(shape, with_bias, sync, monkeypatch):
    monkeypatch.setenv("LLMQ_SKG_SYNC", sync)
    c = _case(*shape)
    dev = _dev()
    bias = c["bias"].to(dev) if with_bias else None
    out = _run(c["x"].to(dev), c["w"].to(dev), bias, 0)
    assert torch.equal(out, c["ref"][with_bias])


@gpu
@needs_gpu
@pytest.mark.parametrize("sync", ("0", "1"))
@pytest.mark.parametrize("K,splitk", SPLIT_CASES)
def test_exact_with_explicit_splitk(K, splitk, sync, monkeypatch):
    """Includes (320,4), (192,8), (64,2), (320,8): a slice without K-steps
    if gridDim.z were the requested splitk."""
    monkeypatch.setenv("LLMQ_SKG_SYNC", sync)
    M, N = SPLIT_M, SPLIT_N
    c = _case(M, N, K)
    dev = _dev()
    x, w = c["x"].to(dev), c["w"].to(dev)
    for with_bias in (False, True):
        bias = c["bias"].to(dev) if with_bias else None
        out = _run(x, w, bias, splitk, poison=splitk * M * N)
        assert torch.equal(out, c["ref"][with_bias]), (K, splitk, with_bias)


@gpu
@needs_gpu
@pytest.mark.parametrize("sync", ("0", "1"))
@pytest.mark.parametrize("K,z", AUTO_CASES)
def test_exact_with_auto_splitk(K, z, sync, monkeypatch):
    monkeypatch.setenv("LLMQ_SKG_SYNC", sync)
    M, N = AUTO_M, AUTO_N
    assert _auto_z(M, N, K) == z
    c = _case(M, N, K)
    dev = _dev()
    out = _run(c["x"].to(dev), c["w"].to(dev), c["bias"].to(dev), 0,
               poison=z * M * N)
    assert torch.equal(out, c["ref"][True])


@functools.lru_cache(maxsize=None)
def _randn_case():
    M, N, K = 129, 260, 4096
    gen = torch.Generator().manual_seed(SEED + 7)
    x = (torch.randn(M, K, generator=gen) * 0.5).to(BF16)
    w = (torch.randn(N, K, generator=gen) * 0.02).to(BF16)
    bias = torch.randn(N, generator=gen).to(BF16)
    ref = _reference(x, w, bias)
    # one bf16 rounding + twice the worst-case fp32 summation bound
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (
        x.double().abs() @ w.double().abs().T)
    return dict(x=x, w=w, bias=bias, ref=ref, bound=bound)


@gpu
@needs_gpu
@pytest.mark.parametrize("splitk", (1, 3, 0), ids=("direct", "split3", "auto"))
def test_randn_within_derived_bound(splitk):
    """Realistic magnitudes at K=4096, one case per split mode (auto picks
    z=8). The bound is derived, not fitted; the largest error/bound seen
    on an MI355X was 0.383 in all three modes (the bf16 rounding term)."""
    c = _randn_case()
    dev = _dev()
    out = _run(c["x"].to(dev), c["w"].to(dev), c["bias"].to(dev), splitk)
    assert bool(out.isfinite().all())
    ratio = ((out.double() - c["ref"]).abs() / c["bound"]).max().item()
    print(f"skinny_gemm randn splitk={splitk}: max error/bound = {ratio:.4f}")
    assert ratio < 1.0


PAD = 4096  # canary elements on each side
CANARY = 0x5A


class _Guarded:
    """Tensors carved out of byte buffers with a canary halo on both sides."""

    def __init__(self):
        self._bufs = []

    def like(self, vals):
        vals = vals.contiguous()
        esz, n = vals.element_size(), vals.numel()
        raw = torch.full(((n + 2 * PAD) * esz,), CANARY, dtype=torch.uint8,
                         device=_dev())
        mid = raw[PAD * esz:(PAD + n) * esz].view(vals.dtype).view(vals.shape)
        mid.copy_(vals)
        self._bufs.append((raw, esz, n))
        return mid

    def verify(self):
        torch.cuda.synchronize()
        for i, (raw, esz, n) in enumerate(self._bufs):
            assert bool((raw[:PAD * esz] == CANARY).all()), f"buffer {i}: low halo"
            assert bool((raw[(PAD + n) * esz:] == CANARY).all()), f"buffer {i}: high halo"


@gpu
@needs_gpu
def test_canary_halos_stay_intact():
    M, N, K = 257, 260, 192
    c = _case(M, N, K)
    for z in (1, 3):
        g = _Guarded()
        x, w, bias = g.like(c["x"]), g.like(c["w"]), g.like(c["bias"])
        out = g.like(torch.full((M, N), float("nan"), dtype=BF16))
        torch.ops.llmq_amd.skinny_gemm(out, x, w, bias, z)
        g.verify()
        assert torch.equal(out.cpu(), c["ref"][True]), z
        assert torch.equal(x.cpu(), c["x"]) and torch.equal(w.cpu(), c["w"])


def _no_fallback(*a, **k):
    raise AssertionError("ops.skinny_gemm fell back to F.linear")


@gpu
@needs_gpu
def test_legal_row_strided_views_and_out(monkeypatch):
    """x and w as views of wider buffers (row stride K+64, other integers
    beside them), result through out=: the kernel path, exact."""
    from llmq_amd import ops

    M, N, K = 129, 260, 192
    c = _case(M, N, K)
    dev = _dev()
    gen = torch.Generator().manual_seed(SEED + 11)
    bx = torch.randint(-1, 2, (M, K + 64), generator=gen).to(BF16)
    bw = torch.randint(-2, 3, (N, K + 64), generator=gen).to(BF16)
    bx[:, :K], bw[:, :K] = c["x"], c["w"]
    xv, wv = bx.to(dev)[:, :K], bw.to(dev)[:, :K]
    assert not xv.is_contiguous() and not wv.is_contiguous()
    monkeypatch.setattr(torch.nn.functional, "linear", _no_fallback)
    for z in (0, 2):
        out = torch.full((M, N), float("nan"), dtype=BF16, device=dev)
        got = ops.skinny_gemm(xv, wv, c["bias"].to(dev), splitk=z, out=out)
        assert got is out
        assert torch.equal(out.cpu(), c["ref"][True]), z


@gpu
@needs_gpu
def test_misaligned_views_fall_back_or_raise():
    """Operands the 16-byte staging loads cannot take: the wrapper answers
    through F.linear (exact on this data), the raw op raises on the host,
    before any launch."""
    from llmq_amd import ops

    M, N, K = 129, 260, 192
    c = _case(M, N, K)
    dev = _dev()
    x, w, bias = c["x"].to(dev), c["w"].to(dev), c["bias"].to(dev)
    raw = torch.ops.llmq_amd.skinny_gemm
    out = torch.empty(M, N, dtype=BF16, device=dev)

    def shifted(t, width, off):
        buf = torch.zeros(t.shape[0], width, dtype=BF16, device=dev)
        view = buf[:, off:off + K]
        view.copy_(t)
        return view

    bias2 = torch.zeros(2 * N, dtype=BF16, device=dev)[::2]
    bias2.copy_(bias)
    bad = [
        (shifted(x, K + 64, 4), w, bias),   # x base 8 bytes off
        (x, shifted(w, K + 64, 4), bias),   # w base 8 bytes off
        (shifted(x, K + 4, 0), w, bias),    # x row stride not a multiple of 8
        (x, shifted(w, K + 4, 0), bias),    # w row stride not a multiple of 8
        (x, w, bias2),                      # strided bias
    ]
    for xa, wa, ba in bad:
        got = ops.skinny_gemm(xa, wa, ba)
        assert torch.equal(got.cpu(), c["ref"][True])
        with pytest.raises(RuntimeError):
            raw(out, xa, wa, ba, 0)
    with pytest.raises(RuntimeError):
        raw(out, x, w, bias, -1)


_ENGINE_MODELS = ("tiny-llama-d128", "tiny-qwen2", "tiny-gemma2")
_ENGINE_PROMPTS = ["hello world test", "abcdefgh" * 12]  # TestEngineFamiliesGPU

_ENGINE_CHILD = r"""
import json, sys
import torch
from llmq_amd import ops
from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.sampling_params import SamplingParams

models, prompts = json.loads(sys.argv[1])
assert ops.has_hip_ext()
calls = {"wrapper": 0, "kernel": 0}
ext = ops._EXT
inner = ops.skinny_gemm


class CountingExt:
    def __getattr__(self, name):
        return getattr(ext, name)

    def skinny_gemm(self, *a):
        calls["kernel"] += 1
        return ext.skinny_gemm(*a)


def counted(*a, **k):
    calls["wrapper"] += 1
    return inner(*a, **k)


ops._EXT = CountingExt()
ops.skinny_gemm = counted
result = {}
for model in models:
    calls["wrapper"] = calls["kernel"] = 0
    params = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    eng = LLMEngine(EngineConfig(
        model=model, max_num_seqs=2, max_model_len=256, load_weights=False,
        num_kv_blocks=128, device="cuda", enforce_eager=True))
    outs = {}
    for i, p in enumerate(prompts):
        eng.add_request(f"r{i}", prompt=p, params=params)
    while eng.has_unfinished():
        for out in eng.step():
            outs.setdefault(out.request_id, []).extend(out.new_token_ids)
    torch.cuda.synchronize()
    result[model] = {"tokens": [outs[f"r{i}"] for i in range(len(prompts))],
                     "calls": dict(calls)}
    del eng
print("RESULT " + json.dumps(result))
"""


@gpu
@needs_gpu
def test_engine_families_through_skinny_gemm():
    """LLMQ_SKINNY_GEMM=1 is read when the model module is imported, so a
    fresh child process runs the three tiny families with every projection
    on the kernel. The child runs eagerly, so each forward makes 4 calls per
    layer plus the lm_head; the counters keep the test from passing through
    F.linear unnoticed. Token criterion of TestEngineFamiliesGPU."""
    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine
    from llmq_amd.engine.model_specs import resolve_spec
    from llmq_amd.engine.sampling_params import SamplingParams

    env = {**os.environ, "LLMQ_SKINNY_GEMM": "1"}
    proc = subprocess.run(
        [sys.executable, "-c", _ENGINE_CHILD,
         json.dumps([_ENGINE_MODELS, _ENGINE_PROMPTS])],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    result = json.loads(line[len("RESULT "):])

    params = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    for model in _ENGINE_MODELS:
        eng = LLMEngine(EngineConfig(
            model=model, max_num_seqs=2, max_model_len=256, load_weights=False,
            num_kv_blocks=128, device="cpu", enforce_eager=True))
        outs = {}
        for i, p in enumerate(_ENGINE_PROMPTS):
            eng.add_request(f"r{i}", prompt=p, params=params)
        while eng.has_unfinished():
            for out in eng.step():
                outs.setdefault(out.request_id, []).extend(out.new_token_ids)
        del eng
        cpu_tokens = [outs[f"r{i}"] for i in range(len(_ENGINE_PROMPTS))]
        gpu_tokens = result[model]["tokens"]
        for c, g in zip(cpu_tokens, gpu_tokens):
            assert len(g) == 12
            assert c[:4] == g[:4], (model, c, g)
        calls = result[model]["calls"]
        per_forward = 4 * resolve_spec(model).num_layers + 1
        assert calls["wrapper"] > 0, (model, calls)
        assert calls["wrapper"] % per_forward == 0, (model, calls)
        assert calls["wrapper"] >= 12 * per_forward, (model, calls)
        assert calls["kernel"] == calls["wrapper"], (model, calls)
