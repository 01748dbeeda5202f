"""Microbenchmark (MI355X): the gather_paged_kv kernel vs the torch
composition it replaces in CausalLM._prefill_attn (two advanced-index cache
reads, two casts, four index_copy_), at the prefix-hit shape: 64 sequences x
(1,024 past + 64 fresh rows), KVH = 8, D in {128, 256}, bf16 and fp8 caches.
The composition runs twice (torch_a / torch_b) to show the run-to-run spread.

Device-event timing over REPS eager calls per window (the prefill segment
runs eager, so launch gaps count); warm-up rounds are dropped; variants
alternate round by round in one process. Prints one JSON object: µs per call
and achieved bytes/s from the bytes read plus written, computed from the
shapes.

Usage (repository root): python tests/paged_gather_microbench.py [out.json]
Results: profiles/prefix_cache.md"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llmq_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
B, P, LQ, KVH, HQ, BS = 64, 1024, 64, 8, 32, 16
REPS = 20
ROUNDS = 12
WARMUP = 3
dtype = torch.bfloat16


def bench_shape(D, cache_dtype):
    torch.manual_seed(0)
    nb_seq = P // BS
    NB = B * nb_seq + 8
    kc = torch.randn(NB, KVH, BS, D, device=DEV, dtype=dtype).to(cache_dtype)
    vc = torch.randn(NB, KVH, BS, D, device=DEV, dtype=dtype).to(cache_dtype)
    qkv = torch.randn(B * LQ, (HQ + 2 * KVH) * D, device=DEV, dtype=dtype)
    k = qkv[:, HQ * D:(HQ + KVH) * D].view(B * LQ, KVH, D)
    v = qkv[:, (HQ + KVH) * D:].view(B * LQ, KVH, D)
    ids = torch.randperm(NB)[: B * nb_seq].view(B, nb_seq)  # scattered blocks
    bt = ids.to(torch.int32).to(DEV)
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV) * LQ
    cu_k = torch.arange(B + 1, dtype=torch.int32, device=DEV) * (P + LQ)
    total_k = B * (P + LQ)

    # the per-token index tensors the composition needs
    rows = torch.arange(P)
    blocks = ids[:, rows // BS].reshape(-1).to(DEV)
    offs = (rows % BS).repeat(B).to(DEV)
    base = (torch.arange(B) * (P + LQ)).view(B, 1)
    past_dst = (base + rows.view(1, P)).reshape(-1).to(DEV)
    fresh_dst = (base + P + torch.arange(LQ).view(1, LQ)).reshape(-1).to(DEV)

    def kernel():
        return ops.gather_paged_kv(kc, vc, k, v, bt, cu, cu_k, total_k, P + LQ)

    def torch_comp():
        k_att = k.new_empty(total_k, KVH, D)
        v_att = k.new_empty(total_k, KVH, D)
        past_k = kc[blocks, :, offs].to(dtype)
        past_v = vc[blocks, :, offs].to(dtype)
        k_att.index_copy_(0, past_dst, past_k)
        v_att.index_copy_(0, past_dst, past_v)
        k_att.index_copy_(0, fresh_dst, k)
        v_att.index_copy_(0, fresh_dst, v)
        return k_att, v_att

    ka, va = kernel()
    kb, vb = torch_comp()
    assert torch.equal(ka, kb) and torch.equal(va, vb), "variants disagree"
    del ka, va, kb, vb

    variants = {"torch_a": torch_comp, "kernel": kernel, "torch_b": torch_comp}
    times = {n: [] for n in variants}
    for r in range(ROUNDS + WARMUP):
        for name, fn in variants.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(REPS):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[name].append(a.elapsed_time(b) * 1000.0 / REPS)
    csz = kc.element_size()
    nbytes = 2 * KVH * D * B * (P * csz + LQ * 2 + (P + LQ) * 2)  # k and v
    res = {"bytes": nbytes}
    for n, ts in times.items():
        med = statistics.median(ts)
        res[n] = {"median_us": round(med, 2), "min_us": round(min(ts), 2),
                  "max_us": round(max(ts), 2),
                  "GB_per_s": round(nbytes / med / 1e3, 1)}
    spread = abs(res["torch_a"]["median_us"] - res["torch_b"]["median_us"])
    best_torch = min(res["torch_a"]["median_us"], res["torch_b"]["median_us"])
    res["torch_ab_spread_us"] = round(spread, 2)
    res["kernel_not_slower"] = res["kernel"]["median_us"] <= best_torch + spread
    return res


out = {}
for D in (128, 256):
    for cname, cdt in (("bf16", torch.bfloat16), ("fp8", torch.float8_e4m3fn)):
        out[f"D{D}_{cname}"] = bench_shape(D, cdt)
        torch.cuda.empty_cache()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out, indent=1))
