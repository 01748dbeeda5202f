"""Microbenchmark (MI355X): the token_logprobs kernel at B x V = 512 x 256000
bf16 logits with soft-cap 30, against the torch composition it replaces and
the plain sampler call for scale.

  sampler            sample_gumbel_argmax alone (one read of the logits)
  lp_k{0,5,20}       token_logprobs, every row asking, default workgroup
  lp_k{..}_t512      the same with 512-thread workgroups
  lp8_k{0,5,20}      every eighth row asking
  asc_k20            every row ascending: the candidate buffer compacts on
                     every tile (the kernel's worst case)
  torch_k0           log_softmax(capped fp32) + gather of the token
  torch_k20          + stable descending sort, first 20, gather

Device-event timing around REPS back-to-back calls on one stream (each call
is tens of microseconds or more, so launches stay ahead of the device);
variants alternate round by round. Prints one JSON object (µs per call).

Usage (repository root): python tests/logprobs_microbench.py [out.json]
Results: profiles/logprobs.md"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llmq_amd import ops  # noqa: E402

args = sys.argv[1:]
DEV = torch.device("cuda:0")
B, V, CAP = 512, 256000, 30.0
REPS = 10
ROUNDS = 10

assert ops.has_hip_ext()
ext = torch.ops.llmq_amd

torch.manual_seed(0)
logits = (torch.randn(B, V, device=DEV) * 20.0).to(torch.bfloat16)
ascending = torch.linspace(-60.0, 60.0, V, device=DEV).to(torch.bfloat16).repeat(B, 1)
temps = torch.full((B,), 0.7, device=DEV)
seeds = torch.zeros(B, dtype=torch.int32, device=DEV)
pos = torch.zeros(B, dtype=torch.int32, device=DEV)
out = torch.empty(B, dtype=torch.int64, device=DEV)
keys = torch.empty(B, dtype=torch.int64, device=DEV)
tokens = torch.randint(0, V, (B,), device=DEV)
rows_all = torch.arange(B, dtype=torch.int32, device=DEV)
rows_8th = rows_all[::8].contiguous()


def sampler():
    keys.zero_()
    ext.sample_gumbel_argmax(out, keys, logits, temps, seeds, pos, 1234, 1, None, CAP)


def kernel(rows, k, threads=0, src=logits):
    R = rows.numel()
    outs = (torch.empty(R, 1 + k, dtype=torch.int32, device=DEV),
            torch.empty(R, 1 + k, dtype=torch.float32, device=DEV),
            torch.empty(R, dtype=torch.int32, device=DEV))
    return lambda: ops.token_logprobs(src, tokens, k, CAP, rows=rows, out=outs,
                                      threads=threads)


def torch_composition(k):
    def run():
        l = torch.tanh(logits.float() / CAP) * CAP
        lp = torch.log_softmax(l, dim=-1)
        ids = tokens[:, None]
        if k:
            order = torch.sort(l, dim=-1, descending=True, stable=True).indices
            ids = torch.cat([ids, order[:, :k]], dim=1)
        return lp.gather(1, ids)
    return run


variants = {"sampler": sampler, "sampler_again": sampler}
for k in (0, 5, 20):
    variants[f"lp_k{k}"] = kernel(rows_all, k)
    variants[f"lp_k{k}_t512"] = kernel(rows_all, k, 512)
    variants[f"lp8_k{k}"] = kernel(rows_8th, k)
variants["asc_k20"] = kernel(rows_all, 20, 0, ascending)
variants["torch_k0"] = torch_composition(0)
variants["torch_k20"] = torch_composition(20)

for fn in variants.values():
    for _ in range(2):
        fn()
torch.cuda.synchronize()

times = {n: [] for n in variants}
for r in range(ROUNDS + 1):
    for name, fn in variants.items():
        reps = 2 if name.startswith(("torch", "asc")) else REPS
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r >= 1:
            times[name].append(a.elapsed_time(b) * 1000.0 / reps)  # us per call

res = {}
for n, ts in times.items():
    res[n] = {"median_us": round(statistics.median(ts), 2),
              "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
res["logit_bytes"] = B * V * 2
if args:
    with open(args[0], "w") as fh:
        json.dump(res, fh, indent=1)
print(json.dumps(res))
