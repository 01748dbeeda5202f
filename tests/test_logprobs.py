"""Token logprobs on the CPU: parameter validation, the torch specification
(ties, rank), the tiny CPU engine (greedy rank 1, one entry per token across
preemption, entries equal to the specification on the logits the sampler
saw) and the worker's Result structure.
"""

from __future__ import annotations

import asyncio
import dataclasses
import json
import types

import pytest
import torch

from llmq_amd.core.models import Job, Result
from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.ops import torch_ref
from llmq_amd.workers.engine_worker import AsyncEngineBridge, EngineWorker

# ------------------------------------------------------ SamplingParams --


@pytest.mark.parametrize("k", [-1, 21])
def test_validation_rejects(k):
    with pytest.raises(ValueError, match="logprobs"):
        SamplingParams(logprobs=k)


@pytest.mark.parametrize("k", [None, 0, 20])
def test_validation_accepts_the_edges(k):
    assert SamplingParams(logprobs=k).logprobs == k


def test_logprobs_is_a_control_field():
    job = Job(id="a", prompt="{text}", text="hi", logprobs=2)
    assert job.extra_fields() == {"text": "hi"}


# ------------------------------------------------ torch_ref, by hand --


def test_ties_go_to_the_lower_index():
    """64 copies of the maximum: the 20 lowest of their indices, in order."""
    V = 500
    gen = torch.Generator().manual_seed(3)
    row = torch.randn(V, generator=gen).clamp(max=2.0)
    where = torch.randperm(V, generator=gen)[:64].sort().values
    row[where] = 5.0
    tok = int(where[30])
    ids, lp, rank = torch_ref.token_logprobs(row[None], torch.tensor([tok]), 20)
    assert ids.dtype == torch.int32 and lp.dtype == torch.float32
    assert ids.shape == lp.shape == (1, 21) and rank.shape == (1,)
    assert ids[0, 0] == tok
    assert ids[0, 1:].tolist() == where[:20].tolist()
    # rank counts the equal values at lower indices
    assert int(rank[0]) == 31
    want = torch.log_softmax(row.double(), -1)
    assert torch.allclose(lp[0].double(), want[ids[0].long()], atol=1e-5)
    assert torch.equal(lp[0, 1:], lp[0, 1:2].expand(20))


def test_rank_and_k_zero():
    row = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5]])
    for tok, want in ((1, 1), (2, 2), (4, 3), (0, 4), (5, 5), (3, 6)):
        ids, lp, rank = torch_ref.token_logprobs(row, torch.tensor([tok]), 0)
        assert ids.tolist() == [[tok]] and int(rank[0]) == want
        assert lp.shape == (1, 1)
        assert abs(float(lp[0, 0]) - float(torch.log_softmax(row, -1)[0, tok])) < 1e-6


def test_softcap_rows_and_limits():
    gen = torch.Generator().manual_seed(5)
    logits = (torch.randn(3, 300, generator=gen) * 20).to(torch.bfloat16)
    tokens = torch.tensor([0, 299, 17])
    rows = torch.tensor([2, 0], dtype=torch.int32)
    ids, lp, rank = torch_ref.token_logprobs(logits, tokens, 5, 30.0, rows)
    l = torch.tanh(logits.float() / 30.0) * 30.0
    order = torch.sort(l, dim=-1, descending=True, stable=True).indices
    for j, b in enumerate((2, 0)):
        assert ids[j].tolist() == [int(tokens[b])] + order[b, :5].tolist()
        assert int(order[b, int(rank[j]) - 1]) == int(tokens[b])
        want = torch.log_softmax(l[b].double(), -1)[ids[j].long()]
        assert torch.allclose(lp[j].double(), want, atol=1e-5)
    for k in (-1, 21):
        with pytest.raises(ValueError):
            torch_ref.token_logprobs(logits, tokens, k)
    with pytest.raises(ValueError):
        torch_ref.token_logprobs(logits[:, :4], tokens.clamp(max=3), 5)


# ------------------------------------------------------- tiny engine --


def _tiny_engine(**kw):
    cfg = dict(model="tiny-llama", device="cpu", load_weights=False,
               max_num_seqs=4, max_model_len=128, num_kv_blocks=64,
               max_prefill_tokens=64, kv_block_size=16)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _run(eng, prompts, params):
    """tokens, per-step entries, finishing outputs and sequences by request."""
    for i, (p, sp) in enumerate(zip(prompts, params)):
        eng.add_request(f"r{i}", prompt_token_ids=p, params=sp)
    seqs = {rid: s for rid, s in eng._seqs.items()}
    toks = {rid: [] for rid in seqs}
    steps = {rid: [] for rid in seqs}
    final = {}
    guard = 0
    while eng.has_unfinished() and guard < 400:
        for out in eng.step():
            toks[out.request_id].extend(out.new_token_ids)
            steps[out.request_id].append(out.new_logprobs)
            if out.finished:
                final[out.request_id] = out
        guard += 1
    assert guard < 400, "engine failed to drain"
    return toks, steps, final, seqs


PROMPTS = [list(range(1 + 7 * i, 40 + 5 * i)) for i in range(4)]


def _params(k, **kw):
    base = dict(temperature=0.0, max_tokens=24, ignore_eos=True)
    base.update(kw)
    return SamplingParams(logprobs=k, **base)


def test_greedy_engine_reports_rank_one_and_leaves_tokens_alone():
    params = [_params(3), _params(None), _params(0), _params(None)]
    toks, steps, final, _ = _run(_tiny_engine(), PROMPTS, params)
    plain, _, plain_final, _ = _run(_tiny_engine(), PROMPTS, [_params(None)] * 4)
    assert toks == plain, "asking for logprobs changed the tokens"
    assert all(o.logprobs is None and o.cumulative_logprob is None
               for o in plain_final.values())
    for rid, k in (("r0", 3), ("r2", 0)):
        out = final[rid]
        assert len(out.logprobs) == out.output_tokens == 24
        assert out.logprobs == steps[rid]
        assert out.cumulative_logprob == pytest.approx(
            sum(e[1] for e in out.logprobs), abs=1e-9)
        for tok, (tid, lp, rank, top) in zip(toks[rid], out.logprobs):
            assert tid == tok and rank == 1 and lp <= 0.0
            assert len(top) == k
            if k:
                assert top[0] == (tid, lp)
                assert [l for _, l in top] == sorted((l for _, l in top), reverse=True)
    for rid in ("r1", "r3"):
        assert final[rid].logprobs is None and final[rid].cumulative_logprob is None
        assert steps[rid] == [None] * 24


def test_sampled_tokens_and_stop_strings_keep_one_entry_per_token():
    params = [_params(2, temperature=0.9, seed=5, max_tokens=12, ignore_eos=False,
                      stop=["a"]),
              _params(1, temperature=1.2, max_tokens=12)]
    toks, steps, final, _ = _run(_tiny_engine(), PROMPTS[:2], params)
    for rid in ("r0", "r1"):
        out = final[rid]
        assert len(out.logprobs) == out.output_tokens == len(toks[rid])
        assert [e[0] for e in out.logprobs] == toks[rid]
        assert all(e[2] >= 1 for e in out.logprobs)


def test_logprobs_clamp_to_the_vocabulary():
    eng = _tiny_engine()
    assert eng.spec.vocab_size > 20
    eng.add_request("x", prompt_token_ids=[1, 2, 3], params=_params(20, max_tokens=2))
    assert eng._seqs["x"].params.logprobs == 20
    # add_request clamps against the model's vocabulary (on a copy of the
    # spec: resolved specs are shared between engines)
    eng.spec = dataclasses.replace(eng.spec, vocab_size=7)
    eng.add_request("y", prompt_token_ids=[1, 2, 3], params=_params(20, max_tokens=2))
    assert eng._seqs["y"].params.logprobs == 7


def test_preempted_run_keeps_one_entry_per_token_equal_to_the_specification():
    ks = [3, 20, 0, 5]
    eng = _tiny_engine(num_kv_blocks=13)
    records = []
    inner = eng.runner._sample

    def record(logits, seqs, buf_name="main", softcap=0.0):
        out = inner(logits, seqs, buf_name, softcap=softcap)
        records.append((logits.clone(), [(s.request_id, s.output_len) for s in seqs],
                        out.clone(), softcap))
        return out

    eng.runner._sample = record
    toks, steps, final, seqs = _run(eng, PROMPTS, [_params(k) for k in ks])
    assert max(s.num_preemptions for s in seqs.values()) > 0, \
        "never preempted - test is vacuous, shrink the pool"
    roomy, _, roomy_final, _ = _run(_tiny_engine(), PROMPTS, [_params(k) for k in ks])
    assert toks == roomy
    checked = 0
    for logits, who, out, cap in records:
        for b, (rid, pos) in enumerate(who):
            k = ks[int(rid[1:])]
            ids, lp, rank = torch_ref.token_logprobs(
                logits[b:b + 1], out[b:b + 1], k, cap)
            tid, tlp, trank, top = final[rid].logprobs[pos]
            assert tid == int(out[b]) == toks[rid][pos]
            assert trank == int(rank[0])
            assert [i for i, _ in top] == ids[0, 1:].tolist()
            assert [tlp] + [l for _, l in top] == pytest.approx(lp[0].tolist(), abs=1e-6)
            checked += 1
    assert checked == 4 * 24
    for rid in toks:
        assert len(final[rid].logprobs) == 24 == final[rid].output_tokens
        assert final[rid].logprobs == steps[rid]
        got = [e[1] for e in final[rid].logprobs]
        assert got == pytest.approx([e[1] for e in roomy_final[rid].logprobs], abs=1e-4)


def test_penalties_do_not_change_the_reported_distribution():
    """Logprobs are the model's: taken before the penalties."""
    pen = dict(repetition_penalty=1.5, frequency_penalty=0.8)
    eng = _tiny_engine()
    captured = []
    inner = eng.runner._sample

    def capture(logits, seqs, *a, **kw):
        out = inner(logits, seqs, *a, **kw)
        captured.append((logits.clone(), out.clone()))
        return out

    eng.runner._sample = capture
    toks, _, final, _ = _run(eng, PROMPTS[:1], [_params(2, max_tokens=12, **pen)])
    ranks = [e[2] for e in final["r0"].logprobs]
    for (logits, out), (tid, lp, rank, top) in zip(captured, final["r0"].logprobs):
        want = torch.log_softmax(logits.float(), -1)[0]
        assert lp == pytest.approx(float(want[tid]), abs=1e-5)
        assert top[0][0] == int(want.argmax())
    assert any(r > 1 for r in ranks), "the penalties never changed a token: vacuous"


# ------------------------------------------------------------- worker --


def _worker(stage_config):
    worker = EngineWorker.__new__(EngineWorker)
    worker.stage_config = stage_config
    worker.config = types.SimpleNamespace(max_tokens=8192)
    worker.worker_id = "w"
    worker._stats = {}
    return worker


def test_job_then_stage_then_off():
    assert _worker({})._sampling_params(Job(id="a", prompt="p")).logprobs is None
    assert _worker({"logprobs": 2})._sampling_params(
        Job(id="a", prompt="p")).logprobs == 2
    assert _worker({"logprobs": 2})._sampling_params(
        Job(id="a", prompt="p", logprobs=0)).logprobs == 0
    with pytest.raises(ValueError, match="logprobs"):
        _worker({})._sampling_params(Job(id="a", prompt="p", logprobs=21))


@pytest.mark.parametrize("where", ["job", "stage"])
def test_worker_result_carries_logprobs(where):
    stage = {"logprobs": 2} if where == "stage" else {}
    line = {"id": "1", "prompt": "hello world", "max_tokens": 5, "temperature": 0.0}
    if where == "job":
        line["logprobs"] = 2
    plain_line = dict(line, id="2", logprobs=None)
    return_plain = where == "job"  # a stage default applies to every job

    async def main():
        bridge = AsyncEngineBridge(_tiny_engine)
        await bridge.start()
        try:
            worker = _worker(stage)
            worker.bridge = bridge
            results = []
            for ln in (line, plain_line):
                job = Job.model_validate_json(json.dumps(ln))
                text = await worker._process_job(job)
                results.append(worker._build_result(job, text, 1.0))
            return results, bridge.engine.tokenizer
        finally:
            bridge.shutdown()

    (res, plain), tok = asyncio.run(main())
    back = Result.model_validate_json(res.model_dump_json())
    assert back.logprobs == res.logprobs and len(back.logprobs) == back.output_tokens
    assert back.cumulative_logprob == pytest.approx(
        sum(e["logprob"] for e in back.logprobs))
    for e in back.logprobs:
        assert set(e) == {"token_id", "token", "logprob", "rank", "top_logprobs"}
        assert e["rank"] == 1 and isinstance(e["token_id"], int)
        assert e["token"] == tok.decode([e["token_id"]], skip_special_tokens=False)
        assert len(e["top_logprobs"]) == 2
        for t in e["top_logprobs"]:
            assert set(t) == {"token_id", "token", "logprob"}
            assert t["token"] == tok.decode([t["token_id"]], skip_special_tokens=False)
        assert e["top_logprobs"][0]["token_id"] == e["token_id"]
        assert e["top_logprobs"][0]["logprob"] == e["logprob"]
    if return_plain:
        assert plain.logprobs is None and plain.cumulative_logprob is None
    else:
        assert len(plain.logprobs) == plain.output_tokens
    assert plain.result == res.result
