"""Prefix-caching engine benchmark (MI355X): a burst of same-template jobs
with enable_prefix_caching off and on.

One engine per setting (llama-3.1-8b, random init, fast_init). Each run
submits 256 prompts = a 1,024-token shared head + 64 distinct tokens (fresh
tails every run), max_tokens=16, all before the first step. Off and on run
twice each, alternating, in one process, with mixed steps run sequentially
(LLMQ_OVERLAP_MIXED=0) in both settings. The first caching-on run is the
cold burst (the head is computed once, by the first prompt of the step, and
shared within the step); the second finds the head already cached.

Reported per run: tokens actually prefilled (a count: it drops by the hit
total), wall time to the last first-token, wall time of the host-side meta
build, prefill steps, and the hit rate.

Usage (repository root): python tests/prefix_cache_bench.py [out.json]
Results: profiles/prefix_cache.md"""
import faulthandler
import json
import os
import random
import sys
import time

# Both settings run their mixed steps sequentially (decode graph, then the
# prefill segment, one stream). The decode-beside-prefill overlap deadlocks
# when a GEMM shape selects a stream-k kernel (profiles/r2_step5_model_breadth.md),
# and this burst's 7 x 1,088-row segments are shapes no other tool has run.
os.environ.setdefault("LLMQ_OVERLAP_MIXED", "0")

import torch  # noqa: E402

# where the host is, should a stage stall (stderr, does not stop the run)
faulthandler.dump_traceback_later(150, repeat=True)


def say(msg):
    print(f"[prefix_cache_bench] {msg}", file=sys.stderr, flush=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llmq_amd.engine.config import EngineConfig  # noqa: E402
from llmq_amd.engine.engine import LLMEngine  # noqa: E402
from llmq_amd.engine.sampling_params import SamplingParams  # noqa: E402

N_PROMPTS, HEAD, TAIL, MAX_TOKENS = 256, 1024, 64, 16
rng = random.Random(0)
head = [rng.randrange(3, 1000) for _ in range(HEAD)]


def make_engine(caching):
    eng = LLMEngine(EngineConfig(
        model="llama-3.1-8b", load_weights=False, fast_init=True,
        max_num_seqs=N_PROMPTS, max_model_len=2048, num_kv_blocks=20000,
        enable_prefix_caching=caching,
    ))
    meter = {"prefilled": 0, "meta_s": 0.0, "prefill_steps": 0}
    build = eng.runner._build_prefill_meta

    def timed_build(pseqs, chunks, dev):
        t0 = time.perf_counter()
        out = build(pseqs, chunks, dev)
        meter["meta_s"] += time.perf_counter() - t0
        meter["prefilled"] += sum(e - st for st, e in chunks)
        meter["prefill_steps"] += 1
        return out

    eng.runner._build_prefill_meta = timed_build
    say(f"engine caching={caching} ready, overlap={eng._overlap_mixed}")
    return eng, meter


def run(eng, meter, tag):
    for k in meter:
        meter[k] = 0
    before = eng.prefix_cache_stats()
    params = SamplingParams(temperature=0.0, max_tokens=MAX_TOKENS, ignore_eos=True)
    tail_rng = random.Random(tag)
    for i in range(N_PROMPTS):
        tail = [tail_rng.randrange(3, 1000) for _ in range(TAIL)]
        eng.add_request(f"{tag}-{i}", prompt_token_ids=head + tail, params=params)
    first = set()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t_first = None
    while eng.has_unfinished():
        for out in eng.step():
            first.add(out.request_id)
        if eng.steps % 8 == 0:
            say(f"{tag}: step {eng.steps}, {len(first)} first tokens")
        if t_first is None and len(first) == N_PROMPTS:
            torch.cuda.synchronize()
            t_first = time.perf_counter() - t0
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    after = eng.prefix_cache_stats()
    looked = after["lookup_tokens"] - before["lookup_tokens"]
    hit = after["hit_tokens"] - before["hit_tokens"]
    return {
        "prompt_tokens": N_PROMPTS * (HEAD + TAIL),
        "prefilled_tokens": meter["prefilled"],
        "hit_tokens": hit,
        "hit_rate": round(hit / looked, 4) if looked else 0.0,
        "prefill_steps": meter["prefill_steps"],
        "last_first_token_s": round(t_first, 4),
        "meta_build_s": round(meter["meta_s"], 4),
        "total_s": round(total, 4),
    }


engines = {"off": make_engine(False), "on": make_engine(True)}
# untimed warm-up of both engines (allocator, GEMM selection, lazy init)
for name, (eng, meter) in engines.items():
    eng.add_request("warm", prompt_token_ids=list(range(3, 300)),
                    params=SamplingParams(temperature=0.0, max_tokens=4,
                                          ignore_eos=True))
    while eng.has_unfinished():
        eng.step()
    say(f"warm-up {name} done")
results = {}
for rnd in (1, 2):
    for name, (eng, meter) in engines.items():
        results[f"{name}_{rnd}"] = run(eng, meter, f"{name}{rnd}")
        print(f"{name}_{rnd}", json.dumps(results[f"{name}_{rnd}"]), flush=True)
for rnd in (1, 2):
    off, on = results[f"off_{rnd}"], results[f"on_{rnd}"]
    assert off["prefilled_tokens"] == off["prompt_tokens"]
    assert on["prefilled_tokens"] == on["prompt_tokens"] - on["hit_tokens"], (
        "prefilled tokens did not drop by the hit total")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(results, fh, indent=1)
faulthandler.cancel_dump_traceback_later()
print(json.dumps(results, indent=1))
