"""Microbenchmark (MI355X): ops.lm_head_logprobs, the fused lm_head +
log-sum-exp kernel, against the blocked composition it replaces
(LLMQ_FUSED_PROMPT_LOGPROBS=0: lm_head GEMM + token_logprobs over 1024 rows
at a time), at R = 512, 2048, 8192 scored rows for

  gemma    V = 256000, K = 3584, soft-cap 30 (and cap 0 at R = 2048: the
           price of the epilogue's tanhf)
  llama    V = 128256, K = 4096, no cap

Device-event timing around REPS back-to-back calls, variants alternating
round by round; TF/s = 2 R V K / time. Peak memory is
torch.cuda.max_memory_allocated over one call minus the allocation before it
(inputs excluded); `unblocked` is the composition with all R rows in one
block, i.e. the [R, V] logits matrix, at R = 8192. Prints one JSON object.

Usage (repository root): python tests/prompt_logprobs_bench.py [out.json]
Results: profiles/prompt_logprobs.md"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llmq_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 5
MODELS = {"gemma": (256000, 3584, 30.0), "llama": (128256, 4096, 0.0)}
RS = (512, 2048, 8192)

assert ops.has_hip_ext()
torch.manual_seed(0)


def call(fused, hidden, w, rows, targets, cap, block_rows=1024):
    os.environ["LLMQ_FUSED_PROMPT_LOGPROBS"] = "1" if fused else "0"
    return ops.lm_head_logprobs(hidden, w, rows, targets, cap, block_rows=block_rows)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


res = {}
for model, (V, K, cap) in MODELS.items():
    w = (torch.randn(V, K, device=DEV) * 0.02).to(torch.bfloat16)
    for R in RS:
        hidden = torch.randn(R + 64, K, device=DEV).to(torch.bfloat16)
        rows = torch.randperm(R + 64, device=DEV)[:R].to(torch.int32)
        targets = torch.randint(0, V, (R,), device=DEV, dtype=torch.int32)
        variants = {"fused": (True, cap), "blocked": (False, cap)}
        if model == "gemma" and R == 2048:
            variants["fused_nocap"] = (True, 0.0)
        entry = {}
        for name, (fused, c) in variants.items():
            call(fused, hidden, w, rows, targets, c)  # warm-up (GEMM workspace)
            entry[name] = {"peak_bytes": peak_above_inputs(
                lambda: call(fused, hidden, w, rows, targets, c))}
        diff = (call(True, hidden, w, rows, targets, cap)
                - call(False, hidden, w, rows, targets, cap)).abs().max().item()
        entry["max_abs_fused_minus_blocked"] = diff
        if R == 8192:
            entry["unblocked"] = {"peak_bytes": peak_above_inputs(
                lambda: call(False, hidden, w, rows, targets, cap, block_rows=R))}
        reps = max(2, 4096 // R)
        times = {n: [] for n in variants}
        for _ in range(ROUNDS):
            for name, (fused, c) in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(reps):
                    call(fused, hidden, w, rows, targets, c)
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) / reps)  # ms per call
        for name, ts in times.items():
            ms = statistics.median(ts)
            entry[name].update(ms=round(ms, 3), min_ms=round(min(ts), 3),
                               max_ms=round(max(ts), 3),
                               tflops=round(2.0 * R * V * K / ms / 1e9, 1))
        res[f"{model}_R{R}"] = entry
        print(f"{model}_R{R}", json.dumps(entry), flush=True)
        del hidden
    del w
    torch.cuda.empty_cache()

if sys.argv[1:]:
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1)
print(json.dumps(res))
