"""Sampling penalties and min_p on the CPU: parameter validation, job ->
stage -> default precedence, the torch specification on hand-written cases,
the count table's lifecycle on CPU tensors, and the tiny CPU engine
(teacher-forced replay, preemption equality, neutral parameters).
"""

from __future__ import annotations

import asyncio
import random
import types

import numpy as np
import pytest
import torch

from llmq_amd.core.models import Job
from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.penalty_table import (
    COUNT_MASK, PROMPT_BIT, PenaltyTable, count_words, wants_penalties,
)
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.engine.scheduler import Sequence
from llmq_amd.ops import torch_ref
from llmq_amd.workers.engine_worker import EngineWorker

# ------------------------------------------------------ SamplingParams --


def test_defaults_are_neutral():
    p = SamplingParams()
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty,
            p.min_p) == (1.0, 0.0, 0.0, 0.0)
    assert not wants_penalties(p)
    assert wants_penalties(SamplingParams(repetition_penalty=1.1))
    assert wants_penalties(SamplingParams(presence_penalty=-0.5))
    assert wants_penalties(SamplingParams(frequency_penalty=0.1))
    assert not wants_penalties(SamplingParams(min_p=0.2))  # no table needed


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
    dict(repetition_penalty=float("nan")),
    dict(presence_penalty=2.01), dict(presence_penalty=-2.01),
    dict(frequency_penalty=2.5), dict(frequency_penalty=-3.0),
    dict(min_p=-0.01), dict(min_p=1.01),
])
def test_validation_rejects(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        SamplingParams(**kw)


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.5), dict(repetition_penalty=5.0),
    dict(presence_penalty=2.0), dict(presence_penalty=-2.0),
    dict(frequency_penalty=2.0), dict(frequency_penalty=-2.0),
    dict(min_p=0.0), dict(min_p=1.0),
])
def test_validation_accepts_the_edges(kw):
    SamplingParams(**kw)


# ----------------------------------------------- job / stage precedence --


def _bare_worker(stage_config):
    worker = EngineWorker.__new__(EngineWorker)
    worker.stage_config = stage_config
    worker.config = types.SimpleNamespace(max_tokens=8192)
    return worker


def test_job_then_stage_then_neutral():
    stage = dict(repetition_penalty=1.1, presence_penalty=0.3,
                 frequency_penalty=0.2, min_p=0.05)
    job = Job(id="a", prompt="p", repetition_penalty=1.2, presence_penalty=-1.0,
              frequency_penalty=0.7, min_p=0.1)
    p = _bare_worker(stage)._sampling_params(job)
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty,
            p.min_p) == (1.2, -1.0, 0.7, 0.1)
    p = _bare_worker(stage)._sampling_params(Job(id="b", prompt="p"))
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty,
            p.min_p) == (1.1, 0.3, 0.2, 0.05)
    p = _bare_worker({})._sampling_params(Job(id="c", prompt="p", min_p=0.3))
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty,
            p.min_p) == (1.0, 0.0, 0.0, 0.3)
    # a job value of 0 is a value, not "unset"
    p = _bare_worker(stage)._sampling_params(
        Job(id="d", prompt="p", presence_penalty=0.0))
    assert p.presence_penalty == 0.0 and p.frequency_penalty == 0.2


def test_the_four_names_are_control_fields():
    job = Job(id="a", prompt="{text}", text="hello", repetition_penalty=1.2,
              min_p=0.1, presence_penalty=0.1, frequency_penalty=0.1)
    assert job.extra_fields() == {"text": "hello"}
    assert job.get_formatted_prompt() == "hello"


def test_invalid_job_value_is_rejected_when_params_are_built():
    with pytest.raises(ValueError, match="repetition_penalty"):
        _bare_worker({})._sampling_params(
            Job(id="a", prompt="p", repetition_penalty=0.0))


def _tiny_engine(**kw):
    cfg = dict(model="tiny-llama", device="cpu", load_weights=False,
               max_num_seqs=4, max_model_len=128, num_kv_blocks=64,
               max_prefill_tokens=64, kv_block_size=16)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def test_submitted_job_line_reaches_the_sampler():
    """The JSON line `llmq submit` publishes, through EngineWorker._process_job
    into an engine whose _sample is watched."""
    eng = _tiny_engine()
    seen = []
    inner = eng.runner._sample

    def watch(logits, seqs, *a, **kw):
        seen.extend(s.params for s in seqs)
        return inner(logits, seqs, *a, **kw)

    eng.runner._sample = watch

    class Bridge:
        engine = eng

        async def generate(self, request_id, prompt, params):
            eng.add_request(request_id, prompt=prompt, params=params)
            out = None
            while eng.has_unfinished():
                for o in eng.step():
                    if o.finished:
                        out = o
            return types.SimpleNamespace(
                text=out.text, prompt_tokens=out.prompt_tokens,
                output_tokens=out.output_tokens, finish_reason=out.finish_reason,
                queue_wait_ms=0.0, prefill_ms=0.0, decode_ms=0.0, cached_tokens=0)

    worker = _bare_worker({"min_p": 0.05})
    worker.bridge = Bridge()
    worker._stats = {}
    line = '{"id": "1", "prompt": "hello world", "repetition_penalty": 1.2, "max_tokens": 3}'
    job = Job.model_validate_json(line)
    asyncio.run(worker._process_job(job))
    assert len(seen) == 3
    assert all(p.repetition_penalty == 1.2 and p.min_p == 0.05 for p in seen)


# ------------------------------------------------ torch_ref, by hand --


def test_apply_penalties_hand_written():
    l = torch.tensor([[2.0, -1.0, 0.5, 3.0, -2.0, 1.0, 0.0, 4.0]])
    counts = torch.tensor([[0, 0, 2, 1, 3, 0, 0, 0]])
    # 0 and 1 occur in the prompt only (a positive and a negative logit);
    # 3 occurs in both
    in_prompt = torch.tensor([[True, True, False, True, False, False, False, False]])
    got = torch_ref.apply_penalties(l, counts, in_prompt, 2.0, 0.5, 0.25)
    want = torch.tensor([[1.0, -2.0, -1.0, 0.75, -5.75, 1.0, 0.0, 4.0]])
    assert torch.equal(got, want)
    # repetition alone reaches prompt-only tokens; the other two do not
    got = torch_ref.apply_penalties(l, counts, in_prompt, 1.0, 0.5, 0.25)
    want = torch.tensor([[2.0, -1.0, -0.75, 2.25, -3.75, 1.0, 0.0, 4.0]])
    assert torch.equal(got, want)
    # neutral values change nothing, bit for bit
    assert torch.equal(
        torch_ref.apply_penalties(l, counts, in_prompt, 1.0, 0.0, 0.0), l)
    # negative penalties reward repetition
    got = torch_ref.apply_penalties(l, counts, in_prompt, 0.5, -1.0, -2.0)
    want = torch.tensor([[4.0, -0.5, 5.0, 9.0, 4.0, 1.0, 0.0, 4.0]])
    assert torch.equal(got, want)


def test_apply_penalties_per_row_and_true_division():
    l = torch.tensor([[1.1, -0.7, 2.3, 0.0, 1.0, 1.0, 1.0, 1.0]]).repeat(2, 1)
    counts = torch.zeros(2, 8, dtype=torch.long)
    counts[:, :3] = 1
    in_prompt = torch.zeros(2, 8, dtype=torch.bool)
    r = torch.tensor([1.3, 0.8])
    got = torch_ref.apply_penalties(l, counts, in_prompt, r, torch.zeros(2),
                                    torch.zeros(2))
    f = np.float32
    for b, rb in enumerate((f(1.3), f(0.8))):
        assert got[b, 0].item() == f(1.1) / rb   # division, not * (1 / r)
        assert got[b, 1].item() == f(-0.7) * rb
        assert got[b, 2].item() == f(2.3) / rb
        assert torch.equal(got[b, 3:], l[b, 3:])
    assert f(1.1) / f(1.3) != f(1.1) * (f(1.0) / f(1.3))  # the two do differ


def test_min_p_in_the_reference_sampler():
    # softmax(l / T): token 0 dominates; min_p 0.5 leaves it alone
    l = torch.tensor([[5.0, 4.0, 1.0, 0.0, -1.0, 4.9, 2.0, 3.0]])
    temps = torch.tensor([1.0])
    tps, tks = torch.ones(1), torch.zeros(1, dtype=torch.long)
    g = torch.Generator().manual_seed(0)
    draws = {int(torch_ref.sample_tokens(l, temps, tps, tks, g,
                                         torch.tensor([0.5]))[0])
             for _ in range(200)}
    assert draws == {0, 5}  # p >= 0.5 * p_max  <=>  l >= 5 + ln 0.5 = 4.31
    draws = {int(torch_ref.sample_tokens(l, temps, tps, tks, g,
                                         torch.tensor([1.0]))[0])
             for _ in range(20)}
    assert draws == {0}
    # intersected with top-k: top-2 = {0, 5}, min_p 0.95 keeps {0} of them
    draws = {int(torch_ref.sample_tokens(l, temps, tps, torch.tensor([2]), g,
                                         torch.tensor([0.95]))[0])
             for _ in range(50)}
    assert draws == {0}


# ------------------------------------------------- table lifecycle --


def _recount(seq, width):
    return torch.from_numpy(
        count_words(seq.token_ids, seq.prompt_len, width).view(np.int16))


def test_count_words_layout_and_saturation():
    words = count_words([3, 3, 5, 3, 7, 7], 3, 16)
    assert words[3] == PROMPT_BIT | 1 and words[5] == PROMPT_BIT
    assert words[7] == 2 and words.sum() == 2 * PROMPT_BIT + 3
    many = count_words([1] + [2] * 40000, 1, 8)
    assert many[2] == COUNT_MASK and many[1] == PROMPT_BIT


def test_cpu_increment_saturates_and_keeps_the_prompt_bit():
    from llmq_amd import ops

    table = torch.zeros(3, 8, dtype=torch.int16)
    table[1, 2] = 32767
    table[1, 3] = -1          # 0xFFFF
    table[2, 3] = -32768      # prompt bit alone
    before = table.clone()
    ops.penalty_count_tokens(table, torch.tensor([1, -1, 2], dtype=torch.int32),
                             torch.tensor([2, 0, 3]))
    assert table[1, 2] == 32767 and table[2, 3] == -32767
    table[2, 3] = -32768
    assert torch.equal(table, before)
    ops.penalty_count_tokens(table, torch.tensor([1, 0], dtype=torch.int32),
                             torch.tensor([3, 5]))
    assert table[1, 3] == -1 and table[0, 5] == 1


@pytest.mark.parametrize("seed", range(4))
def test_table_lifecycle_under_churn(seed):
    rng = random.Random(seed)
    V, SLOTS = 50, 3
    tab = PenaltyTable(SLOTS, V, torch.device("cpu"))
    assert tab.table is None
    pen = SamplingParams(repetition_penalty=1.3, frequency_penalty=0.5)
    plain = SamplingParams()
    running, waiting = [], []   # waiting: preempted, will be re-admitted
    penalised_ever = 0
    n = 0

    def live_penalised():
        return [s for s in running if wants_penalties(s.params)]

    for _ in range(400):
        op = rng.choice(["admit", "sample", "sample", "sample", "preempt",
                         "abort", "finish", "readmit", "desync"])
        if op == "admit" and len(running) < SLOTS:
            params = pen if rng.random() < 0.7 else plain
            prompt = [rng.randrange(V) for _ in range(rng.randint(1, 12))]
            running.append(Sequence(f"r{n % 5}", prompt, params))  # ids reused
            penalised_ever += wants_penalties(params)
            n += 1
        elif op == "readmit" and waiting and len(running) < SLOTS:
            running.append(waiting.pop(0))
        elif op == "sample" and running:
            batch = rng.sample(running, rng.randint(1, len(running)))
            slots = tab.slots_for(batch)
            for s, slot in zip(batch, slots):
                assert (slot >= 0) == wants_penalties(s.params)
            # every live row equals the recount from token_ids
            for s in live_penalised():
                slot = tab.slot_of(s)
                if s in batch:
                    assert slot >= 0
                if slot >= 0 and s in batch:
                    assert torch.equal(tab.table[slot], _recount(s, tab.vpad)), s.uid
            held = [tab.slot_of(s) for s in running + waiting if tab.slot_of(s) >= 0]
            assert len(held) == len(set(held)), "two live sequences share a slot"
            assert len(held) + tab.num_free == SLOTS
            toks = [rng.randrange(V) for _ in batch]
            if any(sl >= 0 for sl in slots):
                tab.count_sampled(batch, torch.tensor(slots, dtype=torch.int32),
                                  torch.tensor(toks))
            for s, t in zip(batch, toks):
                s.token_ids.append(t)
            for s in batch:  # and still equal after the append
                if tab.slot_of(s) >= 0:
                    assert torch.equal(tab.table[tab.slot_of(s)], _recount(s, tab.vpad))
        elif op == "preempt" and running:
            s = running.pop(rng.randrange(len(running)))
            tab.release(s)
            waiting.append(s)
        elif op in ("abort", "finish") and (running or waiting):
            pool = running if (running and (op == "finish" or not waiting)) else waiting
            s = pool.pop(rng.randrange(len(pool)))
            tab.release(s)
            tab.release(s)  # releasing twice is harmless
        elif op == "desync" and running:
            # a token appended behind the table's back: the next sampling
            # call must notice and rebuild
            rng.choice(running).token_ids.append(rng.randrange(V))
    assert penalised_ever > SLOTS, "fewer penalised sequences than slots: vacuous"
    for s in running + waiting:
        tab.release(s)
    assert tab.num_free == SLOTS and not tab._rows


def test_table_is_lazy_and_reports_exhaustion():
    tab = PenaltyTable(1, 16, torch.device("cpu"))
    plain = Sequence("a", [1, 2], SamplingParams())
    assert tab.slots_for([plain]) == [-1] and tab.table is None
    pen = SamplingParams(presence_penalty=1.0)
    a, b = Sequence("a", [1, 2], pen), Sequence("b", [3], pen)
    assert tab.slots_for([a]) == [0] and tab.table.shape == (1, 64)
    with pytest.raises(RuntimeError, match="out of slots"):
        tab.slots_for([b])
    tab.release(a)
    assert tab.slots_for([b]) == [0]
    assert torch.equal(tab.table[0], _recount(b, 64))


def test_allocation_failure_fails_the_request_not_the_engine(monkeypatch):
    from llmq_amd.engine import penalty_table as pt

    def oom(*a, **kw):
        raise torch.OutOfMemoryError("out of memory")

    tab = PenaltyTable(4, 512, torch.device("cpu"))
    monkeypatch.setattr(pt.torch, "zeros", oom)
    with pytest.raises(pt.PenaltyTableError, match="gpu_memory_utilization") as err:
        tab.ensure_allocated()
    # a ValueError: the worker's bridge fails that request and keeps stepping
    assert isinstance(err.value, ValueError) and tab.table is None
    monkeypatch.undo()
    tab.ensure_allocated()   # memory came back: the next request succeeds
    assert tab.table.shape == (4, 512)


# ------------------------------------------------------- tiny engine --


def _run(eng, prompts, params):
    plist = params if isinstance(params, list) else [params] * len(prompts)
    for i, (p, sp) in enumerate(zip(prompts, plist)):
        eng.add_request(f"r{i}", prompt_token_ids=p, params=sp)
    seqs = list(eng._seqs.values())
    toks = {f"r{i}": [] for i in range(len(prompts))}
    guard = 0
    while eng.has_unfinished() and guard < 400:
        for out in eng.step():
            toks[out.request_id].extend(out.new_token_ids)
        guard += 1
    assert guard < 400, "engine failed to drain"
    return toks, seqs


def test_teacher_forced_replay_matches_the_specification():
    params = SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True,
                            repetition_penalty=1.3, frequency_penalty=0.5)
    prompt = [5, 9, 5, 300, 17, 9, 44, 5]
    toks, _ = _run(_tiny_engine(), [prompt], params)
    got = toks["r0"]
    assert len(got) == 16

    # a fresh engine (same seeded weights): full forward of every prefix
    eng = _tiny_engine()
    captured = []
    inner = eng.runner._sample

    def capture(logits, seqs, *a, **kw):
        captured.append(logits.clone())
        return inner(logits, seqs, *a, **kw)

    eng.runner._sample = capture
    one = SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True)
    plain_tokens = []
    for i in range(16):
        prefix = prompt + got[:i]
        t, _ = _run(eng, [prefix], one)
        plain_tokens.append(t["r0"][0])
        logits = captured[-1]
        V = logits.size(1)
        out = torch.tensor(got[:i], dtype=torch.long)
        counts = torch.bincount(out, minlength=V)[None]
        in_prompt = torch.zeros(1, V, dtype=torch.bool)
        in_prompt[0, prompt] = True
        l = torch_ref.apply_penalties(logits, counts, in_prompt, 1.3, 0.5, 0.0)
        assert int(l.argmax(-1)) == got[i], (i, got)
    assert plain_tokens != got, "the penalties never changed a token: vacuous"
    assert eng.runner.penalty_table.table is None  # the CPU path needs no table


def test_preemption_recompute_matches_unpreempted_with_penalties():
    params = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True,
                            repetition_penalty=1.3, frequency_penalty=0.5,
                            presence_penalty=0.2)
    prompts = [list(range(1 + 7 * i, 40 + 5 * i)) for i in range(4)]

    def run(num_blocks):
        toks, seqs = _run(_tiny_engine(num_kv_blocks=num_blocks), prompts, params)
        return toks, max(s.num_preemptions for s in seqs)

    roomy, p0 = run(64)
    tight, p1 = run(13)
    assert p0 == 0, "roomy run unexpectedly preempted"
    assert p1 > 0, "tight run never preempted - test is vacuous, shrink the pool"
    for rid in roomy:
        assert len(roomy[rid]) == 24
        assert roomy[rid] == tight[rid], f"{rid}: preemption changed tokens"
    plain, _ = _run(_tiny_engine(), prompts, SamplingParams(
        temperature=0.0, max_tokens=24, ignore_eos=True))
    assert plain != roomy, "the penalties never changed a token: vacuous"


def test_neutral_parameters_take_the_plain_path(monkeypatch):
    prompts = [[3, 1, 4, 1, 5, 9, 2, 6], [2, 7, 1, 8, 2, 8]]
    base = dict(temperature=0.7, max_tokens=12, ignore_eos=True, seed=11)
    want, _ = _run(_tiny_engine(), prompts, SamplingParams(**base))
    eng = _tiny_engine()

    def boom(*a, **kw):
        raise AssertionError("neutral parameters reached the penalty path")

    monkeypatch.setattr(eng.runner, "_penalised_logits_cpu", boom)
    monkeypatch.setattr(eng.runner.penalty_table, "slots_for", boom)
    got, _ = _run(eng, prompts, SamplingParams(
        **base, repetition_penalty=1.0, presence_penalty=0.0,
        frequency_penalty=0.0, min_p=0.0))
    assert got == want
    assert eng.runner.penalty_table.table is None


def test_min_p_one_is_greedy_on_the_engine():
    prompts = [[3, 1, 4, 1, 5, 9, 2, 6]]
    greedy, _ = _run(_tiny_engine(), prompts, SamplingParams(
        temperature=0.0, max_tokens=10, ignore_eos=True))
    top, _ = _run(_tiny_engine(), prompts, SamplingParams(
        temperature=1.3, min_p=1.0, max_tokens=10, ignore_eos=True))
    assert top == greedy


def test_slots_are_released_on_finish_abort_and_preemption():
    """On the CPU engine the table is unused, so drive it as the GPU path
    does: claim a row for every sampled sequence."""
    eng = _tiny_engine(num_kv_blocks=13)
    tab = eng.runner.penalty_table
    inner = eng.runner._sample

    def claim(logits, seqs, *a, **kw):
        tab.slots_for(seqs)
        held = [tab.slot_of(s) for s in eng.scheduler.running]
        assert len(set(held)) == len(held)
        return inner(logits, seqs, *a, **kw)

    eng.runner._sample = claim
    params = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True,
                            repetition_penalty=1.2)
    prompts = [list(range(1 + 7 * i, 40 + 5 * i)) for i in range(4)]
    for i, p in enumerate(prompts):
        eng.add_request(f"r{i}", prompt_token_ids=p, params=params)
    seqs = list(eng._seqs.values())
    aborted = None
    guard = 0
    while eng.has_unfinished() and guard < 400:
        eng.step()
        for s in eng.scheduler.waiting:  # preempted: row given back
            assert tab.slot_of(s) == -1
        if aborted is None and any(s.num_preemptions for s in seqs):
            aborted = eng.scheduler.running[0]
            assert tab.slot_of(aborted) >= 0
            eng.abort_request(aborted.request_id)
            assert tab.slot_of(aborted) == -1
        guard += 1
    assert aborted is not None, "never preempted - test is vacuous, shrink the pool"
    assert tab.num_free == tab.num_slots and not tab._rows
