"""Microbenchmark (MI355X): the sampler kernels with and without sampling
penalties and min_p, at B x V = 512 x 256000 bf16 logits with soft-cap 30.

  a_plain / a_topkp  no count table: the sampler alone, and top-k/top-p bound
                     + sampler (the calls as they were before the penalties)
  b_plain / b_topkp  every row penalised
  c_plain / c_topkp  every second row penalised
  d_minp             min_p only: bound kernel (one pass) + sampler

Device-event timing; variants alternate round by round; each timed window
replays a captured graph of REPS calls. Prints one JSON object (µs per call).
The `a_*` cases call the ops with the arguments they had before the
penalties, so `--cases a` also runs against an older build of the extension
selected with LLMQ_OPS_SO (for a before/after comparison in separate
processes).

Usage (repository root): python tests/sampler_penalty_microbench.py [--cases abcd] [out.json]
Results: profiles/sampling_penalties.md"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llmq_amd import ops  # noqa: E402

args = sys.argv[1:]
cases = "abcd"
if "--cases" in args:
    i = args.index("--cases")
    cases = args[i + 1]
    del args[i:i + 2]

DEV = torch.device("cuda:0")
B, V, CAP = 512, 256000, 30.0
VPAD = (V + 63) // 64 * 64
REPS = 10
ROUNDS = 12

assert ops.has_hip_ext()
ext = torch.ops.llmq_amd

torch.manual_seed(0)
logits = (torch.randn(B, V, device=DEV) * 20.0).to(torch.bfloat16)
idx = torch.arange(B, device=DEV)
temps = torch.tensor((0.7, 1.3), device=DEV)[idx % 2].contiguous()
seeds = torch.zeros(B, dtype=torch.int32, device=DEV)
pos = torch.zeros(B, dtype=torch.int32, device=DEV)
tks = torch.where(idx % 2 == 0, 40, 0).to(torch.int64)
tps = torch.where(idx % 2 == 0, 1.0, 0.9).to(torch.float32)
out = torch.empty(B, dtype=torch.int64, device=DEV)
keys = torch.empty(B, dtype=torch.int64, device=DEV)
bound = torch.empty(B, dtype=torch.float32, device=DEV)

variants = {}


def plain(pen=()):
    keys.zero_()
    ext.sample_gumbel_argmax(out, keys, logits, temps, seeds, pos, 1234, 1,
                             None, CAP, *pen)


def topkp(min_ps=None, pen=(), p=tps, k=tks):
    if min_ps is None and not pen:
        ext.topk_topp_bound(bound, logits, temps, p, k, CAP)
    else:
        ext.topk_topp_bound(bound, logits, temps, p, k, CAP, min_ps,
                            *(pen or (None, None, None)))
    keys.zero_()
    ext.sample_gumbel_argmax(out, keys, logits, temps, seeds, pos, 1234, 1,
                             bound, CAP, *pen)


if "a" in cases:
    variants["a_plain"] = plain
    variants["a_plain_again"] = lambda: plain()  # run-to-run spread
    variants["a_topkp"] = topkp

if set(cases) & set("bcd"):
    table = torch.zeros(B, VPAD, dtype=torch.int16, device=DEV)
    hit = torch.randint(0, V, (B, 2000), device=DEV)
    table.scatter_(1, hit, torch.randint(1, 9, hit.shape, device=DEV).to(torch.int16))
    params = torch.tensor([[1.3, 0.5, 0.2]], device=DEV).repeat(B, 1).contiguous()
    all_slots = torch.randperm(B, device=DEV).to(torch.int32)
    half_slots = torch.where(idx % 2 == 0, all_slots, torch.full_like(all_slots, -1))
    ones = torch.ones(B, device=DEV)
    zeros = torch.zeros(B, dtype=torch.int64, device=DEV)
    min_ps = torch.full((B,), 0.05, device=DEV)
    if "b" in cases:
        pen_all = (table, all_slots, params)
        variants["b_plain"] = lambda: plain(pen_all)
        variants["b_topkp"] = lambda: topkp(None, pen_all)
    if "c" in cases:
        pen_half = (table, half_slots, params)
        variants["c_plain"] = lambda: plain(pen_half)
        variants["c_topkp"] = lambda: topkp(None, pen_half)
    if "d" in cases:
        variants["d_minp"] = lambda: topkp(min_ps, (), ones, zeros)

graphs = {}
side = torch.cuda.Stream()
for name, fn in variants.items():
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(REPS):
            fn()
    graphs[name] = g
torch.cuda.synchronize()

times = {n: [] for n in variants}
for r in range(ROUNDS + 2):
    for name, g in graphs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        if r >= 2:
            times[name].append(a.elapsed_time(b) * 1000.0 / REPS)  # us per call

res = {"so": os.environ.get("LLMQ_OPS_SO", "in-tree")}
for n, ts in times.items():
    res[n] = {"median_us": round(statistics.median(ts), 2),
              "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
res["logit_bytes"] = B * V * 2
res["count_bytes_all_rows"] = B * V * 2
if args:
    with open(args[0], "w") as fh:
        json.dump(res, fh, indent=1)
print(json.dumps(res))
