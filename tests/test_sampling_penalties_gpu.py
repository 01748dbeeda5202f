"""Sampling penalties and min_p inside the HIP sampler kernels.

The kernels read bf16 logits, soft-cap them in registers and apply the
penalties from a row of the dense count table; they must pick exactly the
tokens / bounds of the torch specification

    l = capped fp32 logits;  l = torch_ref.apply_penalties(l, counts, ...)

fed to the same op as fp32 without a table: `torch.equal`, no tolerance.
min_p's bound is compared with `m + T * log(min_p)` in fp32 torch.

Shapes: the small ones of test_sampler_bf16_softcap.py (odd row stride with
scalar head and tail and count rows misaligned against the logits; one and
two splits with and without V % 8 == 0) plus (16, 256000) for the vector
path with many splits. Logits are seeded randn * 20 in bf16 without a cap
and with cap 30, and randn * 3 without a cap: at * 20 an uncapped row keeps
one or two tokens, which would leave truncation untested. References are
built once per case and shared.

Measured on CPU (test_min_p_preconditions asserts the share): of the
(row, T, min_p) cases over the five min_p shapes, cap 30 at * 20 and no cap
at * 3, T in {0.7, 1.3}, min_p in {0.02, 0.1, 0.5}, fewer than a quarter have
a logit within 1e-3 of the bound; only those are exempt from the keep-set
comparison against the probability definition.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from llmq_amd.ops import torch_ref

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

SMALL = ((3, 32003), (1, 4104), (1, 4099), (1, 4096), (1, 4091))
SHAPES = SMALL + ((16, 256000),)
# (logit scale, cap): capped and uncapped at * 20, uncapped at * 3
VARIANTS = ((20.0, 0.0), (20.0, 30.0), (3.0, 0.0))
STEPS = range(1, 9)
TEMPS = (0.0, 0.7, 1.3)
PARAMS = ((1.3, 0.0, 0.0), (0.8, -0.5, 1.5), (1.0, 0.4, 0.6), (1.0, 0.0, 0.0))
EXTRA_SLOTS = 3
MINP_SHAPES = tuple(s for s in SHAPES if s != (1, 4096))
MINP_VARIANTS = ((20.0, 30.0), (3.0, 0.0))
MINP_TS = (0.7, 1.3)
MIN_PS = (0.02, 0.1, 0.5)
NEAR = 1e-3


def aligned_vpad(V: int) -> int:
    return (V + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _logits_cpu(B: int, V: int, scale: float) -> torch.Tensor:
    gen = torch.Generator().manual_seed(B * 1000003 + V + int(scale))
    return (torch.randn(B, V, generator=gen) * scale).to(torch.bfloat16)


def _capped(logits: torch.Tensor, cap: float) -> torch.Tensor:
    l = logits.float()
    return torch.tanh(l / cap) * cap if cap > 0 else l


@functools.lru_cache(maxsize=None)
def _table_cpu(B: int, V: int, vpad: int):
    """(table int16 [B + EXTRA_SLOTS, vpad], slots int32 [B], words int32
    [B, V] as each row sees them, params fp32 [B, 3]). Slots are a
    permutation; every third row has none. A few hundred entries per row
    mix prompt-only, count-only and both, among them the first and last two
    vocab entries and the dozen largest logits of the row that owns the
    slot, so that the penalties decide which token wins; one word is 0xFFFF
    and one exactly 32767."""
    rng = np.random.default_rng(B * 7919 + V)
    nslots = B + EXTRA_SLOTS
    top = torch.cat([_logits_cpu(B, V, sc).float().topk(12, dim=1).indices
                     for sc in (20.0, 3.0)], dim=1).numpy()
    table = np.zeros((nslots, vpad), dtype=np.uint16)
    # words outside [0, V) must never be read: make them loud
    table[:, V:] = 0xFFFF
    perm = rng.permutation(nslots)
    slots = np.full(B, -1, dtype=np.int32)
    words = np.zeros((B, V), dtype=np.int32)
    owner = {int(perm[b]): b for b in range(B)}
    for s in range(nslots):
        n = min(300, V // 4)
        idx = rng.choice(V, size=n, replace=False)
        idx[:4] = (0, 1, V - 2, V - 1)
        if s in owner:
            idx = np.concatenate([idx, top[owner[s]]])
        idx = np.unique(idx)
        kind = rng.integers(0, 3, size=idx.size)
        cnt = rng.integers(1, 21, size=idx.size).astype(np.uint16)
        w = np.where(kind == 0, 0x8000, np.where(kind == 1, cnt, 0x8000 | cnt))
        table[s, idx] = w.astype(np.uint16)
        table[s, idx[idx.size // 2]] = 0xFFFF      # a signed read fails here
        table[s, idx[idx.size // 3]] = 32767       # saturated, no prompt bit
    for b in range(B):
        if b % 3 != 2:
            slots[b] = perm[b]
            words[b] = table[perm[b], :V]
    params = np.array([PARAMS[b % 4] for b in range(B)], dtype=np.float32)
    return (torch.from_numpy(table.view(np.int16)), torch.from_numpy(slots),
            torch.from_numpy(words), torch.from_numpy(params))


def _reference(capped: torch.Tensor, words: torch.Tensor, params: torch.Tensor):
    return torch_ref.apply_penalties(
        capped, words & 0x7FFF, (words & 0x8000) != 0,
        params[:, 0], params[:, 1], params[:, 2])


@functools.lru_cache(maxsize=None)
def _case(B: int, V: int, scale: float, cap: float, vpad: int = 0):
    """bf16 logits, the table and the penalised fp32 reference on the GPU,
    made once and left unchanged."""
    dev = torch.device("cuda:0")
    raw = _logits_cpu(B, V, scale).to(dev)
    table, slots, words, params = (
        t.to(dev) for t in _table_cpu(B, V, vpad or aligned_vpad(V)))
    capped = _capped(raw, cap)
    return raw, capped, _reference(capped, words, params), table, slots, params


def _seeded(B: int, dev, on: bool):
    idx = torch.arange(B)
    seeds = torch.where(idx % 4 == 1, 1000 + idx, torch.zeros_like(idx))
    if not on:
        seeds = torch.zeros_like(idx)
    pos = (idx * 7) % 13
    return seeds.to(torch.int32).to(dev), pos.to(torch.int32).to(dev)


def _sample(logits, temps, seeds, pos, step, bounds=None, softcap=0.0, **pen):
    from llmq_amd import ops

    B = logits.shape[0]
    out = torch.empty(B, dtype=torch.int64, device=logits.device)
    keys = torch.empty(B, dtype=torch.int64, device=logits.device)
    ops.sample_gumbel_argmax(out, keys, logits, temps, seeds, pos, 1234, step,
                             bounds, softcap, **pen)
    return out.clone()


# ------------------------------------------------- CPU preconditions --


@pytest.mark.parametrize("B,V", SHAPES)
def test_table_fixture_is_what_the_tests_assume(B, V):
    table, slots, words, params = _table_cpu(B, V, aligned_vpad(V))
    u = table.numpy().view(np.uint16)
    assert table.shape[0] > B and aligned_vpad(V) % 8 == 0
    have = slots[slots >= 0]
    assert have.unique().numel() == have.numel()           # distinct
    assert bool((slots[2::3] == -1).all()) and int(slots[0]) >= 0
    assert not torch.equal(have, torch.arange(have.numel(), dtype=torch.int32)) or B == 1
    for s in range(table.shape[0]):
        row = u[s, :V]
        assert (row == 0xFFFF).sum() == 1 and (row == 32767).sum() == 1
        assert ((row & 0x8000 != 0) & (row & 0x7FFF == 0)).any()   # prompt-only
        assert ((row & 0x8000 == 0) & (row != 0)).any()            # count-only
        assert ((row & 0x8000 != 0) & (row & 0x7FFF != 0)).any()   # both
        assert row[0] and row[1] and row[V - 2] and row[V - 1]     # head, tail
    assert bool((words[slots < 0] == 0).all())


def test_penalties_move_the_reference():
    """The penalised reference differs from the capped logits and changes
    the greedy token of some row: a kernel that ignored the table fails."""
    for scale, cap in VARIANTS:
        raw = _logits_cpu(3, 32003, scale)
        _, slots, words, params = _table_cpu(3, 32003, aligned_vpad(32003))
        capped = _capped(raw, cap)
        ref = _reference(capped, words, params)
        assert bool(torch.isfinite(ref).all())
        assert torch.equal(ref[2], capped[2])          # the row without a slot
        assert not torch.equal(ref[:2], capped[:2])
    # a row with a slot and neutral parameters is unchanged bit for bit
    raw = _logits_cpu(16, 256000, 20.0)
    _, slots, words, params = _table_cpu(16, 256000, aligned_vpad(256000))
    capped = _capped(raw, 30.0)
    ref = _reference(capped, words, params)
    neutral = [b for b in range(16) if b % 4 == 3 and int(slots[b]) >= 0]
    assert neutral and all(torch.equal(ref[b], capped[b]) for b in neutral)
    moved = (ref.argmax(-1) != capped.argmax(-1)).sum()
    assert int(moved) > 0


def _min_p_bound_ref(l: torch.Tensor, T: float, min_p: float):
    """m + T * log(min_p), every step rounded to fp32, as the kernel forms it."""
    m = l.max(dim=1).values
    t_ln = torch.tensor(T, dtype=torch.float32, device=l.device) * torch.log(
        torch.tensor(min_p, dtype=torch.float32, device=l.device))
    return m, t_ln, m + t_ln


def _near_rows(l: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    return (l - bound[:, None]).abs().min(dim=1).values < NEAR


def test_min_p_preconditions():
    cases = near = 0
    for B, V in MINP_SHAPES:
        for scale, cap in MINP_VARIANTS:
            l = _capped(_logits_cpu(B, V, scale), cap)
            for T in MINP_TS:
                for mp in MIN_PS:
                    _, _, bound = _min_p_bound_ref(l, T, mp)
                    cases += B
                    near += int(_near_rows(l, bound).sum())
                    kept = (l >= bound[:, None]).sum(dim=1)
                    assert bool((kept < V).all())      # truncation is real
                    if cap > 0:
                        # capped rows saturate towards the cap, so many
                        # tokens sit just under the maximum
                        assert bool((kept > 1).all()), (B, V, T, mp)
    assert cases == 22 * 2 * 2 * 3
    assert near * 4 <= cases, (near, cases)


# ------------------------------------------------------ GPU: sampler --


@gpu
@needs_gpu
@pytest.mark.parametrize("scale,cap", VARIANTS)
@pytest.mark.parametrize("B,V", SHAPES)
def test_penalised_tokens_equal_the_specification(B, V, scale, cap):
    raw, _, ref, table, slots, params = _case(B, V, scale, cap)
    dev = raw.device
    pen = dict(pen_table=table, pen_slots=slots, pen_params=params)
    for seeded in (False, True):
        seeds, pos = _seeded(B, dev, seeded)
        for T in TEMPS:
            temps = torch.full((B,), T, device=dev)
            for step in STEPS:
                want = _sample(ref, temps, seeds, pos + step, step)
                got = _sample(raw, temps, seeds, pos + step, step, None, cap, **pen)
                assert torch.equal(got, want), (
                    seeded, T, step, (got != want).nonzero().flatten()[:8])


@gpu
@needs_gpu
@pytest.mark.parametrize("B,V,pad", [(3, 32003, 3), (1, 4104, 3), (16, 256000, 4),
                                     (1, 4099, 1)])
def test_misaligned_count_rows(B, V, pad):
    """vpad not a multiple of 8: count rows no longer line up with the
    logits' 16-byte vectors, the kernel falls back to narrower loads."""
    raw, _, ref, table, slots, params = _case(B, V, 20.0, 30.0, V + pad)
    assert table.shape[1] == V + pad
    dev = raw.device
    pen = dict(pen_table=table, pen_slots=slots, pen_params=params)
    seeds, pos = _seeded(B, dev, True)
    for T in TEMPS:
        temps = torch.full((B,), T, device=dev)
        for step in (1, 2, 3):
            want = _sample(ref, temps, seeds, pos, step)
            got = _sample(raw, temps, seeds, pos, step, None, 30.0, **pen)
            assert torch.equal(got, want), (T, step)


@gpu
@needs_gpu
@pytest.mark.parametrize("B,V", SHAPES)
def test_fp32_logits_with_a_table(B, V):
    """fp32 logits take 8-byte count loads next to 16-byte logit loads."""
    raw, capped, ref, table, slots, params = _case(B, V, 20.0, 0.0)
    pen = dict(pen_table=table, pen_slots=slots, pen_params=params)
    dev = raw.device
    seeds, pos = _seeded(B, dev, True)
    for T in TEMPS:
        temps = torch.full((B,), T, device=dev)
        want = _sample(ref, temps, seeds, pos, 5)
        assert torch.equal(_sample(capped, temps, seeds, pos, 5, None, 0.0, **pen), want)


@gpu
@needs_gpu
@pytest.mark.parametrize("scale,cap", VARIANTS)
@pytest.mark.parametrize("B,V", SHAPES)
def test_slot_with_neutral_parameters_equals_no_slot(B, V, scale, cap):
    raw, _, _, table, _, _ = _case(B, V, scale, cap)
    dev = raw.device
    slots = torch.arange(B, dtype=torch.int32, device=dev)        # every row
    neutral = torch.tensor([[1.0, 0.0, 0.0]], device=dev).repeat(B, 1).contiguous()
    none = torch.full((B,), -1, dtype=torch.int32, device=dev)
    hot = torch.tensor([[1.7, 1.0, 1.0]], device=dev).repeat(B, 1).contiguous()
    seeds, pos = _seeded(B, dev, True)
    for T in TEMPS:
        temps = torch.full((B,), T, device=dev)
        for step in (1, 2):
            want = _sample(raw, temps, seeds, pos, step, None, cap)
            got = _sample(raw, temps, seeds, pos, step, None, cap, pen_table=table,
                          pen_slots=slots, pen_params=neutral)
            assert torch.equal(got, want), (T, step)
            # and slot -1 ignores both the table and the parameters
            got = _sample(raw, temps, seeds, pos, step, None, cap, pen_table=table,
                          pen_slots=none, pen_params=hot)
            assert torch.equal(got, want), (T, step)


# ------------------------------------------------- GPU: top-k / top-p --


@gpu
@needs_gpu
@pytest.mark.parametrize("scale,cap", VARIANTS)
@pytest.mark.parametrize("B,V", [(16, 256000), (3, 32003), (1, 4099)])
def test_bound_and_truncated_sampling_equal_the_specification(B, V, scale, cap):
    from llmq_amd import ops

    raw, _, ref, table, slots, params = _case(B, V, scale, cap)
    dev = raw.device
    pen = dict(pen_table=table, pen_slots=slots, pen_params=params)
    idx = torch.arange(B)
    temps = torch.tensor((0.7, 1.3))[idx % 2].to(dev)
    tks = torch.where(idx % 2 == 0, 5, 0).to(torch.int64).to(dev)   # top-k 5 rows
    tps = torch.where(idx % 2 == 0, 1.0, 0.9).to(dev)               # top-p 0.9 rows
    want_b = ops.topk_topp_bound(ref, temps, tps, tks)
    got_b = ops.topk_topp_bound(raw, temps, tps, tks, cap, **pen)
    assert torch.equal(got_b, want_b), (got_b, want_b)
    assert bool((got_b > -1e30).all())  # every row is really truncated
    seeds, pos = _seeded(B, dev, True)
    for step in STEPS:
        want = _sample(ref, temps, seeds, pos, step, want_b)
        got = _sample(raw, temps, seeds, pos, step, got_b, cap, **pen)
        assert torch.equal(got, want), step
        assert bool((ref.gather(1, got[:, None])[:, 0] >= got_b).all())


# ------------------------------------------------------- GPU: min_p --


@gpu
@needs_gpu
@pytest.mark.parametrize("scale,cap", MINP_VARIANTS)
@pytest.mark.parametrize("B,V", MINP_SHAPES)
def test_min_p_bound_tokens_and_keep_set(B, V, scale, cap):
    from llmq_amd import ops

    raw, capped, ref, table, slots, params = _case(B, V, scale, cap)
    dev = raw.device
    ones = torch.ones(B, device=dev)
    zeros = torch.zeros(B, dtype=torch.int64, device=dev)
    seeds, pos = _seeded(B, dev, True)
    cases = skipped = 0
    for with_table in (False, True):
        l = ref if with_table else capped
        pen = (dict(pen_table=table, pen_slots=slots, pen_params=params)
               if with_table else {})
        for T in MINP_TS:
            temps = torch.full((B,), T, device=dev)
            for mp in MIN_PS:
                min_ps = torch.full((B,), mp, device=dev)
                got_b = ops.topk_topp_bound(raw, temps, ones, zeros, cap,
                                            min_ps=min_ps, **pen)
                m, t_ln, want_b = _min_p_bound_ref(l, T, mp)
                tol = 8 * 2.0 ** -24 * torch.maximum(m.abs(), t_ln.abs().expand_as(m))
                err = (got_b - want_b).abs()
                assert bool((err <= tol).all()), (T, mp, err.max(), tol.min())
                # the op without a cap or a table, given the same bound
                for step in (1, 2, 3):
                    want = _sample(l, temps, seeds, pos, step, got_b)
                    got = _sample(raw, temps, seeds, pos, step, got_b, cap, **pen)
                    assert torch.equal(got, want), (T, mp, step)
                    assert bool((l.gather(1, got[:, None])[:, 0] >= got_b).all())
                # the probability definition, away from the boundary
                probs = torch.softmax(l / T, dim=1)
                keep_def = probs >= mp * probs.max(dim=1, keepdim=True).values
                keep = l >= got_b[:, None]
                near = _near_rows(l, got_b)
                cases += B
                skipped += int(near.sum())
                same = (keep == keep_def).all(dim=1)
                assert bool((same | near).all()), (T, mp, (~same).nonzero().flatten())
    assert skipped * 4 <= cases, (skipped, cases)


@gpu
@needs_gpu
def test_min_p_combines_with_top_k_and_skips_greedy_rows():
    from llmq_amd import ops

    B, V = 16, 256000
    raw, capped, _, _, _, _ = _case(B, V, 20.0, 30.0)
    dev = raw.device
    idx = torch.arange(B)
    temps = torch.tensor((0.7, 1.3, 0.0, 0.7))[idx % 4].to(dev)
    tks = torch.where(idx % 2 == 0, 40, 0).to(torch.int64).to(dev)
    tps = torch.where(idx % 2 == 0, 1.0, 0.9).to(dev)
    # min_p off on some rows, loose on some, tight on others
    min_ps = torch.tensor((0.0, 0.0005, 0.3, 0.6, 1.0))[idx % 5].to(dev)
    kp = ops.topk_topp_bound(raw, temps, tps, tks, 30.0)
    mp_only = ops.topk_topp_bound(raw, temps, torch.ones(B, device=dev),
                                  torch.zeros(B, dtype=torch.int64, device=dev),
                                  30.0, min_ps=min_ps)
    both = ops.topk_topp_bound(raw, temps, tps, tks, 30.0, min_ps=min_ps)
    greedy = temps <= 0
    assert bool((both[greedy] < -1e30).all()) and bool((mp_only[greedy] < -1e30).all())
    assert bool((mp_only[(min_ps == 0)] < -1e30).all())
    assert torch.equal(both, torch.maximum(kp, mp_only))   # intersection of keep sets
    live = ~greedy
    assert bool((both[live] > kp[live]).any()) and bool((both[live] == kp[live]).any())
    # min_p = 1 keeps exactly the row maximum
    one = (min_ps == 1.0) & live
    assert bool(one.any())
    assert torch.equal(mp_only[one], capped.max(dim=1).values[one])
    # an all-off min_ps tensor gives the bounds of the call without one
    assert torch.equal(
        ops.topk_topp_bound(raw, temps, tps, tks, 30.0,
                            min_ps=torch.zeros(B, device=dev)), kp)


# ------------------------------------------- GPU: penalty_count_tokens --


@gpu
@needs_gpu
@pytest.mark.parametrize("B,V", [(16, 4099), (600, 131)])
def test_penalty_count_tokens(B, V):
    from llmq_amd import ops

    dev = torch.device("cuda:0")
    table, slots, _, _ = _table_cpu(B, V, aligned_vpad(V))
    nslots, vpad = table.shape
    big = torch.full((nslots + 2, vpad), 0x5A5A, dtype=torch.int16)  # guard rows
    big[1:-1] = table
    u = table.numpy().view(np.uint16)
    gen = torch.Generator().manual_seed(B + V)
    tokens = torch.randint(0, V, (B,), generator=gen)
    live = [b for b in range(B) if int(slots[b]) >= 0]
    # aim at the saturated word, the 0xFFFF word, and a zero word
    tokens[live[0]] = int(np.flatnonzero(u[int(slots[live[0]]), :V] == 32767)[0])
    tokens[live[1]] = int(np.flatnonzero(u[int(slots[live[1]]), :V] == 0xFFFF)[0])
    tokens[live[2]] = int(np.flatnonzero(u[int(slots[live[2]]), :V] == 0)[0])
    want = big.clone()
    wu = want.numpy().view(np.uint16)
    bumped = 0
    for b in live:
        s, t = int(slots[b]) + 1, int(tokens[b])
        if wu[s, t] & 0x7FFF != 0x7FFF:
            wu[s, t] += 1
            bumped += 1
    assert 0 < bumped < len(live)
    assert wu[int(slots[live[0]]) + 1, int(tokens[live[0]])] == 32767
    assert wu[int(slots[live[1]]) + 1, int(tokens[live[1]])] == 0xFFFF
    assert wu[int(slots[live[2]]) + 1, int(tokens[live[2]])] == 1
    big_d = big.to(dev)
    view = big_d[1:-1]
    assert view.is_contiguous()
    ops.penalty_count_tokens(view, slots.to(dev), tokens.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(big_d.cpu(), want)   # guards, slot -1 rows, all the rest
    # the CPU fallback of the op does the same
    cpu = big.clone()
    ops.penalty_count_tokens(cpu[1:-1], slots, tokens)
    assert torch.equal(cpu, want)


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
    tokens, kinds = {}, set()

    def step():
        for out in eng.step():
            tokens.setdefault(out.request_id, []).extend(out.new_token_ids)
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
    return tokens, kinds


@gpu
@needs_gpu
def test_engine_tokens_equal_reference_on_recorded_logits():
    """Every token the engine produced equals the torch specification on the
    logits and the token history the sampler saw at that moment: the count
    table's life on the device (rebuild, increment, preemption, slot reuse,
    mixed steps on two streams), independent of bf16 model numerics."""
    from llmq_amd.engine.sampling_params import SamplingParams

    pen = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True,
                         repetition_penalty=1.3, frequency_penalty=0.5,
                         presence_penalty=0.2)
    plain = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True)
    eng = _engine(num_kv_blocks=24)   # 8 sequences want ~32 blocks: preempts
    table = eng.runner.penalty_table
    assert eng.runner.use_graphs and table.table is None
    records, preempted = [], []
    inner = eng.runner._sample
    inner_preempt = eng.scheduler._preempt

    def record(logits, seqs, buf_name="main", softcap=0.0):
        out = inner(logits, seqs, buf_name, softcap=softcap)
        records.append((logits.clone(), [list(s.token_ids) for s in seqs],
                        [(s.prompt_len, s.params) for s in seqs], out.clone(),
                        softcap))
        return out

    def spy(seq):
        preempted.append(seq.uid)
        inner_preempt(seq)

    eng.runner._sample = record
    eng.scheduler._preempt = spy
    tokens, kinds = _two_waves(eng, lambda i: pen if i % 3 != 2 else plain)
    torch.cuda.synchronize()
    assert "mixed" in kinds and "decode" in kinds
    assert preempted, "never preempted - shrink the pool"
    assert len(tokens) == 8 and all(len(v) == 40 for v in tokens.values())
    assert table.table is not None and table.num_free == table.num_slots
    checked = 0
    for logits, histories, meta, out, cap in records:
        V = logits.size(1)
        l = _capped(logits, cap)
        counts = torch.zeros(len(histories), V, dtype=torch.long)
        in_prompt = torch.zeros(len(histories), V, dtype=torch.bool)
        for b, (hist, (plen, _)) in enumerate(zip(histories, meta)):
            in_prompt[b, hist[:plen]] = True
            counts[b] = torch.bincount(torch.tensor(hist[plen:], dtype=torch.long),
                                       minlength=V)
        ps = [p for _, p in meta]
        ref = torch_ref.apply_penalties(
            l, counts.to(l.device), in_prompt.to(l.device),
            torch.tensor([p.repetition_penalty for p in ps]),
            torch.tensor([p.frequency_penalty for p in ps]),
            torch.tensor([p.presence_penalty for p in ps]))
        assert torch.equal(ref.argmax(-1), out), (checked, histories)
        checked += len(histories)
    assert checked == 8 * 40
    del eng
    torch.cuda.empty_cache()


@gpu
@needs_gpu
def test_engine_graphs_equal_eager_with_penalties():
    from llmq_amd.engine.sampling_params import SamplingParams

    params = SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True,
                            repetition_penalty=1.3, frequency_penalty=0.5)
    runs = {}
    for eager in (False, True):
        eng = _engine(max_model_len=512, enforce_eager=eager, seed=1234)
        assert eng.runner.use_graphs == (not eager)
        # 8 prompts == a graph bucket: both paths run identical kernel shapes
        for i in range(8):
            eng.add_request(f"s{i}", prompt_token_ids=_prompt(i), params=params)
        ids = {}
        while eng.has_unfinished():
            for out in eng.step():
                ids.setdefault(out.request_id, []).extend(out.new_token_ids)
        runs[eager] = ids
        del eng
        torch.cuda.empty_cache()
    assert all(len(v) == 32 for v in runs[False].values())
    assert runs[False] == runs[True]


@gpu
@needs_gpu
def test_overlapped_mixed_step_matches_sequential_with_penalties(monkeypatch):
    from llmq_amd.engine.sampling_params import SamplingParams

    params = SamplingParams(temperature=0.7, min_p=0.05, max_tokens=24,
                            ignore_eos=True, repetition_penalty=1.3,
                            frequency_penalty=0.5)

    def run(overlap: str):
        monkeypatch.setenv("LLMQ_OVERLAP_MIXED", overlap)
        eng = _engine()
        tokens, kinds = _two_waves(eng, lambda i: params)
        assert "mixed" in kinds
        del eng
        torch.cuda.empty_cache()
        return tokens

    seq = run("0")
    ovl = run("1")
    assert seq.keys() == ovl.keys() and len(seq) == 8
    for k in seq:
        assert seq[k] == ovl[k], (k, seq[k][:6], ovl[k][:6])
