"""The token_logprobs HIP kernel and the engine path that carries its output.

Kernel: ids and rank must equal the specification exactly, lp within 1e-4 of
an fp64 log_softmax. The reference is built ON THE DEVICE: the capped fp32
value `torch.tanh(logits.float() / cap) * cap` there is bit-equal to the
kernel's logit_value, while the CPU's tanh may differ by an ulp and reorder
ties; it is stable-sorted descending (ties toward the lower index) once per
case and shared by every K and token placement.

The 1e-4 bound: fp32 rounding of values up to ~160 (ulp 1.5e-5) plus a
V-term fp32 sum; torch's own fp32 log_softmax is 3.0e-5 from fp64 at
V = 262144.

Shapes: the sampler tests' small set (one and two 16-byte-vector tiles per
workgroup, V % 8 != 0 with scalar head and tail), (2, 37) with fewer elements
than threads, and (2, 256000). Every logits tensor is a column slice of a
wider buffer: odd row stride, misaligned base. Constructed rows at V = 32003
(several tiles for fp32 and bf16 alike) cover the candidate buffer's
compaction: ascending rows compact on every tile.
"""

from __future__ import annotations

import functools
import math

import pytest
import torch

from llmq_amd import ops

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

SMALL = ((3, 32003), (1, 4104), (1, 4099), (1, 4096), (1, 4091))
SHAPES = SMALL + ((2, 37), (2, 256000))
# (dtype, logit scale, cap)
BF16_VARIANTS = ((torch.bfloat16, 3.0, 0.0), (torch.bfloat16, 20.0, 30.0))
OTHER = (((3, 32003), torch.float32, 20.0, 30.0), ((1, 4099), torch.float32, 3.0, 0.0),
         ((3, 32003), torch.float16, 3.0, 0.0), ((1, 4091), torch.float16, 20.0, 30.0))
KS = (0, 1, 5, 20)
LP_TOL = 1e-4
SENT_I = -12345
SENT_F = 777.0


def _sliced(values: torch.Tensor) -> torch.Tensor:
    """`values` [B, V] as a column slice of a wider device buffer with an odd
    row stride, starting 3 elements into it."""
    B, V = values.shape
    width = V + (13 if V % 2 == 0 else 12)
    wide = torch.full((B, width), 99.0, dtype=values.dtype, device="cuda")
    view = wide[:, 3:3 + V]
    view.copy_(values)
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 != 0
    return view


@functools.lru_cache(maxsize=None)
def _random_case(shape, dtype, scale, cap):
    B, V = shape
    gen = torch.Generator().manual_seed(B * 1000003 + V + int(scale))
    values = (torch.randn(B, V, generator=gen) * scale).to(dtype)
    return _with_reference(_sliced(values), cap)


def _with_reference(logits, cap):
    l = logits.float()
    if cap > 0:
        l = torch.tanh(l / cap) * cap
    order = torch.sort(l, dim=-1, descending=True, stable=True).indices
    lp64 = torch.log_softmax(l.double(), dim=-1)
    pos = torch.empty_like(order)
    pos.scatter_(1, order, torch.arange(l.size(1), device=l.device).expand_as(order))
    return logits, cap, order, lp64, pos + 1


def _head_tail(logits, b):
    """An index in row b's scalar head and one in its scalar tail (or the
    nearest there is when the row has none)."""
    V = logits.size(1)
    ve = 16 // logits.element_size()
    mis = (logits[b].data_ptr() // logits.element_size()) % ve
    head = min(V, (ve - mis) % ve)
    end = head + (V - head) // ve * ve
    return max(head - 1, 0), (end if end < V else V - 1)


def _placements(case):
    logits, cap, order, lp64, rank = case
    B, V = logits.shape
    gen = torch.Generator().manual_seed(V)
    ht = [_head_tail(logits, b) for b in range(B)]
    return {
        "first": [0] * B,
        "last": [V - 1] * B,
        "head": [h for h, _ in ht],
        "tail": [t for _, t in ht],
        "best": order[:, 0].tolist(),
        "random": torch.randint(0, V, (B,), generator=gen).tolist(),
    }


_max_err = [0.0]


def _check(case, tokens, rows, k, threads=0):
    logits, cap, order, lp64, rank_ref = case
    R = len(rows)
    tok = torch.tensor(tokens, dtype=torch.int64, device="cuda")
    rows_t = torch.tensor(rows, dtype=torch.int32, device="cuda")
    big_ids = torch.full((R + 2, k + 3), SENT_I, dtype=torch.int32, device="cuda")
    big_lp = torch.full((R + 2, k + 3), SENT_F, dtype=torch.float32, device="cuda")
    big_rank = torch.full((R + 2,), SENT_I, dtype=torch.int32, device="cuda")
    out = (big_ids[1:-1, 1:-1], big_lp[1:-1, 1:-1], big_rank[1:-1])
    ids, lp, rank = ops.token_logprobs(logits, tok, k, cap, rows=rows_t, out=out,
                                       threads=threads)
    rl = rows_t.long()
    want_ids = torch.cat([tok[rl, None], order[rl, :k]], dim=1)
    assert torch.equal(ids.long(), want_ids), (tokens, rows, k)
    assert torch.equal(rank.long(), rank_ref[rl, tok[rl]]), (tokens, rows, k)
    want_lp = lp64[rl].gather(1, want_ids)
    err = float((lp.double() - want_lp).abs().max())
    _max_err[0] = max(_max_err[0], err)
    print(f"lp max abs error {err:.3e} (V={logits.size(1)} k={k} cap={cap})")
    assert torch.isfinite(lp).all()
    assert err <= LP_TOL, (err, tokens, rows, k)
    if k > 1:
        assert bool((lp[:, 2:] <= lp[:, 1:-1]).all())
    # the frame of sentinels around the R rows and 1 + k columns
    frame = torch.ones_like(big_ids, dtype=torch.bool)
    frame[1:-1, 1:-1] = False
    assert bool((big_ids[frame] == SENT_I).all())
    assert bool((big_lp[frame] == SENT_F).all())
    assert int(big_rank[0]) == SENT_I and int(big_rank[-1]) == SENT_I
    return ids, lp, rank


def _rows_for(B):
    return {1: [0], 2: [1, 0], 3: [2, 0]}.get(B, list(range(B - 1, -1, -2)))


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", BF16_VARIANTS, ids=["x3", "x20cap30"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_specification_bf16(shape, variant):
    case = _random_case(shape, *variant)
    B = shape[0]
    for k in KS:
        if k > shape[1]:
            continue
        for name, tokens in _placements(case).items():
            _check(case, tokens, _rows_for(B), k)
    _check(case, _placements(case)["random"], list(range(B)), 20)


@gpu
@needs_gpu
@pytest.mark.parametrize("shape,dtype,scale,cap", OTHER,
                         ids=["f32-cap", "f32-4099", "f16", "f16-cap"])
def test_kernel_equals_specification_fp32_fp16(shape, dtype, scale, cap):
    case = _random_case(shape, dtype, scale, cap)
    for k in KS:
        for name, tokens in _placements(case).items():
            _check(case, tokens, _rows_for(shape[0]), k)


@gpu
@needs_gpu
def test_smaller_workgroup_gives_the_same_results():
    case = _random_case((3, 32003), torch.bfloat16, 20.0, 30.0)
    tokens = _placements(case)["random"]
    for k in (0, 5, 20):
        a = _check(case, tokens, [2, 0], k, threads=1024)
        b = _check(case, tokens, [2, 0], k, threads=512)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


CV = 32003


@functools.lru_cache(maxsize=None)
def _constructed(dtype, cap):
    """Rows: 0 ascending, 1 descending, 2 constant, 3 one +80 among -80,
    4 with 64 copies of its maximum over head, vector body and tail, 5 with a
    three-way tie at the top and a 30-way tie below it (K = 1, 5 and 20 each
    end inside a tie group). Returns (case, indices of the 64, the 30)."""
    V = CV
    gen = torch.Generator().manual_seed(11)
    rows = torch.empty(6, V)
    rows[0] = torch.linspace(-10.0, 10.0, V)
    rows[1] = torch.linspace(10.0, -10.0, V)
    rows[2] = 1.5
    rows[3] = -80.0
    rows[3, 12345] = 80.0
    rows[4] = torch.randn(V, generator=gen).clamp(max=2.0)
    body = (torch.randperm(V - 40, generator=gen)[:52] + 20).sort().values
    sixty_four = torch.cat([torch.arange(6), body, torch.arange(V - 6, V)])
    rows[4, sixty_four] = 5.0
    rows[5] = torch.randn(V, generator=gen).clamp(max=2.0)
    thirty = (torch.randperm(V, generator=gen)[:33]).sort().values
    three, thirty = thirty[[1, 7, 20]], thirty[[i for i in range(33) if i not in (1, 7, 20)]]
    rows[5, thirty] = 8.0
    rows[5, three] = 9.0
    case = _with_reference(_sliced(rows.to(dtype)), cap)
    return case, sixty_four.tolist(), thirty.tolist(), three.tolist()


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype,cap", [(torch.float32, 0.0), (torch.bfloat16, 0.0),
                                       (torch.bfloat16, 30.0)],
                         ids=["f32", "bf16", "bf16-cap30"])
def test_constructed_rows(dtype, cap):
    case, sixty_four, thirty, three = _constructed(dtype, cap)
    V = CV
    rows = [5, 3, 0, 4, 1, 2]
    placements = [
        [0] * 6,
        [V - 1] * 6,
        # inside the tie groups of rows 4 and 5; the +80 itself in row 3
        [V // 2, 7, 100, 12345, sixty_four[40], thirty[12]],
        [V - 2, 1, 31000, 12346, sixty_four[63], three[2]],
    ]
    for k in KS:
        for tokens in placements:
            ids, lp, rank = _check(case, tokens, rows, k)
            got = {b: (ids[j].tolist(), lp[j].tolist(), int(rank[j]))
                   for j, b in enumerate(rows)}
            # independent of the sorted reference:
            if dtype == torch.float32:  # strictly monotonic there
                assert got[0][0][1:] == list(range(V - 1, V - 1 - k, -1))
                assert got[1][0][1:] == list(range(k))
            assert got[2][0][1:] == list(range(k))
            assert got[2][2] == tokens[2] + 1
            assert got[2][1] == pytest.approx([-math.log(V)] * (1 + k), abs=LP_TOL)
            assert got[4][0][1:] == sixty_four[:k]
            assert got[5][0][1:] == (sorted(three) + thirty)[:k]
            if cap == 0.0:
                want = [0.0 if t == 12345 else -160.0 for t in got[3][0]]
                assert got[3][1] == want
                assert got[3][0][1:] == ([12345] + list(range(k)))[:k]
    # rank inside a tie group counts the equal values at lower indices
    ids, lp, rank = _check(case, placements[2], rows, 0)
    assert int(rank[rows.index(4)]) == 41
    assert int(rank[rows.index(5)]) == 3 + 13


@gpu
@needs_gpu
def test_wrapper_limits_and_empty_request():
    case = _random_case((2, 37), torch.bfloat16, 3.0, 0.0)
    logits = case[0]
    tok = torch.zeros(2, dtype=torch.int64, device="cuda")
    for k in (-1, 21):
        with pytest.raises(AssertionError):
            ops.token_logprobs(logits, tok, k)
    with pytest.raises(AssertionError):
        ops.token_logprobs(logits[:, :4], tok, 5)
    none = torch.empty(0, dtype=torch.int32, device="cuda")
    ids, lp, rank = ops.token_logprobs(logits, tok, 5, rows=none)
    assert ids.shape == (0, 6) and lp.shape == (0, 6) and rank.shape == (0,)
    # all rows by default, fresh outputs
    ids, lp, rank = ops.token_logprobs(logits, tok, 3)
    assert torch.equal(ids[:, 1:].long(), case[2][:, :3])


# ------------------------------------------------------- GPU: engine --


def _engine(**kw):
    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine

    cfg = dict(model="llama-3.2-1b", max_num_seqs=8, max_model_len=256,
               load_weights=False, num_kv_blocks=512, seed=7)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _prompt(i: int, n: int = 10):
    return [(37 * i + 11 * j) % 1000 + 5 for j in range(n)] + [5 + i, 5 + i]


def _two_waves(eng, params_for, first=4, second=4, warm_steps=6):
    tokens, entries, final, kinds = {}, {}, {}, set()

    def step():
        for out in eng.step():
            tokens.setdefault(out.request_id, []).extend(out.new_token_ids)
            entries.setdefault(out.request_id, []).append(out.new_logprobs)
            if out.finished:
                final[out.request_id] = out
        kinds.add(eng.last_step_kind)

    for i in range(first):
        eng.add_request(f"a{i}", prompt_token_ids=_prompt(i), params=params_for(i))
    for _ in range(warm_steps):
        step()
    for i in range(second):
        eng.add_request(f"b{i}", prompt_token_ids=_prompt(10 + i, 14),
                        params=params_for(first + i))
    guard = 0
    while eng.has_unfinished() and guard < 2000:
        step()
        guard += 1
    assert guard < 2000
    return tokens, entries, final, kinds


ENGINE_KS = (None, 0, 3, 20)


def _engine_run(asking: bool, **kw):
    from llmq_amd.engine.sampling_params import SamplingParams

    def params_for(i):
        return SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True,
                              logprobs=ENGINE_KS[i % 4] if asking else None)

    # fast_init: the weights are drawn on the device, which is most of the
    # cost of building a random 1B engine; equal seeds give equal weights
    eng = _engine(fast_init=True, **kw)
    records, preempted = [], []
    inner = eng.runner._sample
    inner_preempt = eng.scheduler._preempt

    def record(logits, seqs, buf_name="main", softcap=0.0):
        out = inner(logits, seqs, buf_name, softcap=softcap)
        records.append((logits.clone(), [(s.request_id, s.output_len) for s in seqs],
                        out.clone(), softcap))
        return out

    def spy(seq):
        preempted.append(seq.uid)
        inner_preempt(seq)

    if asking:
        eng.runner._sample = record
    eng.scheduler._preempt = spy
    tokens, entries, final, kinds = _two_waves(eng, params_for)
    torch.cuda.synchronize()
    use_graphs = eng.runner.use_graphs
    del eng
    torch.cuda.empty_cache()
    return tokens, entries, final, kinds, records, preempted, use_graphs


def _engine_check(**kw):
    tokens, entries, final, kinds, records, preempted, graphs = _engine_run(True, **kw)
    plain = _engine_run(False, **kw)
    assert len(tokens) == 8 and all(len(v) == 40 for v in tokens.values())
    assert tokens == plain[0], "asking for logprobs changed the tokens"
    assert all(o.logprobs is None for o in plain[2].values())
    assert kinds == plain[3] and len(preempted) == len(plain[5])
    ks = {f"{w}{i}": ENGINE_KS[(i + (4 if w == "b" else 0)) % 4]
          for w in "ab" for i in range(4)}
    checked = 0
    for logits, who, out, cap in records:
        ask = [b for b, (rid, _) in enumerate(who) if ks[rid] is not None]
        if not ask:
            continue
        _, _, order, lp64, rank = _with_reference(logits, cap)
        for b in ask:
            rid, pos = who[b]
            k = ks[rid]
            tid, tlp, trank, top = final[rid].logprobs[pos]
            assert tid == int(out[b]) == tokens[rid][pos]
            assert trank == int(rank[b, tid]) == 1
            assert [i for i, _ in top] == order[b, :k].tolist()
            want = lp64[b, [tid] + [i for i, _ in top]].tolist()
            assert [tlp] + [l for _, l in top] == pytest.approx(want, abs=LP_TOL)
            checked += 1
    assert checked == 6 * 40
    for rid, k in ks.items():
        if k is None:
            assert final[rid].logprobs is None and entries[rid] == [None] * 40
            assert final[rid].cumulative_logprob is None
        else:
            assert len(final[rid].logprobs) == 40 == final[rid].output_tokens
            assert final[rid].logprobs == entries[rid]
            assert final[rid].cumulative_logprob == pytest.approx(
                sum(e[1] for e in final[rid].logprobs))
    return kinds, preempted, graphs


@gpu
@needs_gpu
def test_engine_logprobs_equal_specification_on_recorded_logits():
    """hipGraph decode, mixed steps on two streams and preemption: every
    reported entry equals the specification on the logits the sampler read."""
    kinds, preempted, graphs = _engine_check(num_kv_blocks=24)
    assert graphs
    assert "mixed" in kinds and "decode" in kinds
    assert preempted, "never preempted - shrink the pool"


@gpu
@needs_gpu
def test_engine_logprobs_equal_specification_eager():
    kinds, _, graphs = _engine_check(enforce_eager=True)
    assert not graphs
