"""Prompt logprobs through the engine on the CPU (torch_ref path): values by
position against log_softmax of the model's own logits, chunked prefill,
prefix caching, preemption, and the Job -> Result round trip."""

from __future__ import annotations

import asyncio
import json
import types

import pytest
import torch

from llmq_amd.core.models import Job, Result
from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.forward_meta import PrefillMeta
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.workers.engine_worker import AsyncEngineBridge, EngineWorker

PROMPTS = [list(range(1 + 7 * i, 40 + 5 * i)) for i in range(4)]


def _tiny_engine(**kw):
    cfg = dict(model="tiny-llama", device="cpu", load_weights=False,
               max_num_seqs=4, max_model_len=128, num_kv_blocks=64,
               max_prefill_tokens=64, kv_block_size=16)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _run(eng, prompts, asked=True, max_tokens=4):
    for i, p in enumerate(prompts):
        eng.add_request(f"r{i}", prompt_token_ids=p, params=SamplingParams(
            temperature=0.0, max_tokens=max_tokens, ignore_eos=True,
            prompt_logprobs=asked))
    seqs, final, guard = list(eng._seqs.values()), {}, 0
    while eng.has_unfinished() and guard < 400:
        final.update({o.request_id: o for o in eng.step() if o.finished})
        guard += 1
    assert guard < 400, "engine failed to drain"
    return final, seqs


def _values(out):
    return [lp for _tid, lp in out.prompt_logprobs]


def _specification(prompt):
    """log_softmax(compute_logits(forward(prompt))) at the next tokens."""
    n = len(prompt)
    eng = _tiny_engine()  # same seed: same weights
    meta = PrefillMeta(
        cu_seqlens=torch.tensor([0, n], dtype=torch.int32), max_seqlen=n,
        slot_mapping=torch.arange(n, dtype=torch.long), gather=None)
    hidden = eng.model.forward(torch.tensor(prompt), torch.arange(n), eng.kv_cache, meta)
    lsm = torch.log_softmax(eng.model.compute_logits(hidden), dim=-1)
    return lsm[torch.arange(n - 1), torch.tensor(prompt[1:])].tolist()


def test_values_match_the_models_distribution_chunked_or_not():
    whole, _ = _run(_tiny_engine(), PROMPTS)
    chunked, _ = _run(_tiny_engine(max_prefill_tokens=16), PROMPTS)
    for i, prompt in enumerate(PROMPTS):
        out = whole[f"r{i}"]
        assert [t for t, _ in out.prompt_logprobs] == prompt
        got = _values(out)
        assert got[0] is None and len(got) == len(prompt)
        assert got[1:] == pytest.approx(_specification(prompt), abs=1e-5)
        assert _values(chunked[f"r{i}"])[1:] == pytest.approx(got[1:], abs=1e-5)


def test_prefix_cache_is_bypassed_and_others_run_as_before():
    eng = _tiny_engine(enable_prefix_caching=True)
    first, _ = _run(eng, PROMPTS[:1])
    second, _ = _run(eng, PROMPTS[:1])
    assert second["r0"].cached_tokens == 0
    assert None not in _values(second["r0"])[1:]
    assert _values(second["r0"]) == _values(first["r0"])
    plain, _ = _run(eng, PROMPTS[:1], asked=False)
    assert plain["r0"].prompt_logprobs is None
    assert plain["r0"].cached_tokens > 0  # the scored run published its blocks


def test_preempted_sequence_returns_one_full_list():
    final, seqs = _run(_tiny_engine(num_kv_blocks=13), PROMPTS, max_tokens=24)
    assert max(s.num_preemptions for s in seqs) > 0, "never preempted: vacuous"
    roomy, _ = _run(_tiny_engine(), PROMPTS, max_tokens=24)
    for rid, out in final.items():
        assert len(out.prompt_logprobs) == out.prompt_tokens
        assert _values(out)[1:] == pytest.approx(_values(roomy[rid])[1:], abs=1e-5)


@pytest.mark.parametrize("where", ["job", "stage"])
def test_worker_result_carries_prompt_logprobs(where):
    line = {"id": "1", "prompt": "hello wide world", "max_tokens": 3, "temperature": 0.0}
    line.update({"prompt_logprobs": True} if where == "job" else {})
    worker = EngineWorker.__new__(EngineWorker)
    worker.stage_config = {"prompt_logprobs": True} if where == "stage" else {}
    worker.config = types.SimpleNamespace(max_tokens=8192)
    worker.worker_id, worker._stats = "w", {}

    async def main():
        worker.bridge = AsyncEngineBridge(_tiny_engine)
        await worker.bridge.start()
        try:
            results = []
            for ln in (line, dict(line, id="2", prompt_logprobs=False)):
                job = Job.model_validate_json(json.dumps(ln))
                text = await worker._process_job(job)
                results.append(worker._build_result(job, text, 1.0))
            return results
        finally:
            worker.bridge.shutdown()

    res, plain = asyncio.run(main())
    back = Result.model_validate_json(res.model_dump_json())
    assert back.prompt_logprobs == res.prompt_logprobs
    assert len(back.prompt_logprobs) == back.prompt_tokens > 1
    assert back.prompt_logprobs[0]["logprob"] is None
    assert all(set(e) == {"token_id", "token", "logprob"} for e in back.prompt_logprobs)
    assert back.prompt_cumulative_logprob == pytest.approx(
        sum(e["logprob"] for e in back.prompt_logprobs[1:]))
    assert plain.prompt_logprobs is None and plain.prompt_cumulative_logprob is None
    assert plain.result == res.result
