"""Microbenchmark (MI355X): the fused qknorm_rope_and_cache kernel vs the
three-launch composition (rmsnorm on the q and k head views, then
rope_and_cache) vs rope_and_cache alone (same q/k/v/cache bytes: the floor),
at the Qwen3-8B decode shape. The floor runs twice (floor_a / floor_b) to
show the run-to-run spread.

Device-event timing; variants alternate round by round; each timed window
replays a captured graph of REPS launches so that launch gaps are the
graph's, as in the decode step. Prints one JSON object (µs per call).

Usage (repository root): python tests/qknorm_microbench.py [out.json]
Results: profiles/qwen3_qknorm.md"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llmq_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
T, HQ, HK, D, BS = 512, 32, 8, 128, 16
NB = 4096
REPS = 50
ROUNDS = 15
dtype = torch.bfloat16

torch.manual_seed(0)
cos_sin = ops.build_rope_cache(40960, D, 1e6, DEV)
qkv0 = torch.randn(T, (HQ + 2 * HK) * D, device=DEV, dtype=dtype)
qkv = qkv0.clone()
q = qkv[:, : HQ * D].view(T, HQ, D)
k = qkv[:, HQ * D : (HQ + HK) * D].view(T, HK, D)
v = qkv[:, (HQ + HK) * D :].view(T, HK, D)
qw = torch.ones(D, device=DEV, dtype=dtype)
kw = torch.ones(D, device=DEV, dtype=dtype)
pos = torch.randint(0, 4096, (T,), device=DEV)
slots = torch.randperm(NB * BS, device=DEV)[:T]
kc = torch.zeros(NB, HK, BS, D, device=DEV, dtype=dtype)
vc = torch.zeros_like(kc)


def fused():
    ops.qknorm_rope_and_cache(q, k, v, kc, vc, qw, kw, 1e-6, 0.0, pos, cos_sin, slots)


def unfused():
    # what ops.qknorm_rope_and_cache composes outside the kernel's envelope
    for t, w in ((q, qw), (k, kw)):
        t.copy_(ops.rmsnorm(t.reshape(-1, D), w, 1e-6, 0.0).view(t.shape))
    ops.rope_and_cache(q, k, v, kc, vc, pos, cos_sin, slots)


qc = torch.empty(T, HQ, D, device=DEV, dtype=dtype)
kcont = torch.empty(T, HK, D, device=DEV, dtype=dtype)


def unfused_kernels_only():
    # the three kernels alone on contiguous q/k (no strided copies): the
    # most favourable three-launch composition
    ops.rmsnorm(qc.view(-1, D), qw, 1e-6, 0.0)
    ops.rmsnorm(kcont.view(-1, D), kw, 1e-6, 0.0)
    ops.rope_and_cache(qc, kcont, v, kc, vc, pos, cos_sin, slots)


def floor():
    ops.rope_and_cache(q, k, v, kc, vc, pos, cos_sin, slots)


def floor_b():
    ops.rope_and_cache(q, k, v, kc, vc, pos, cos_sin, slots)


variants = {"floor_a": floor, "floor_b": floor_b, "fused": fused,
            "unfused": unfused, "unfused_kernels_only": unfused_kernels_only}

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
        qkv.copy_(qkv0)  # keep values bounded (in-place ops compound)
        qc.normal_()
        kcont.normal_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        if r >= 2:
            times[name].append(a.elapsed_time(b) * 1000.0 / REPS)  # us per call

res = {}
for n, ts in times.items():
    res[n] = {"median_us": round(statistics.median(ts), 3),
              "min_us": round(min(ts), 3), "max_us": round(max(ts), 3)}
# bytes moved by the floor: q,k read+write, v read, k/v cache write
esz = 2
bytes_floor = T * D * esz * (2 * HQ + 2 * HK + HK + 2 * HK)
res["bytes_floor"] = bytes_floor
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1)
print(json.dumps(res, indent=1))
