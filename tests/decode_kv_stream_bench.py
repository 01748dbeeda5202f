#!/usr/bin/env python3
"""Decode K/V stream and rope_and_cache microbenchmark (GPU box tool, not a
pytest). Covers what tests/attn_microbench.py cannot: the cache policy of the
pipe decode kernels' K/V DMAs (LLMQ_DECODE_KV_NT, read per call, so the two
policies alternate inside one process), ragged and split-KV shapes, and the
rope_and_cache kernel pair (LLMQ_ROPE_VEC) inside a captured graph.

Shapes (16 q heads / 8 kv heads, D = 256, block 16 unless noted):
  headline  B = 256, L = 1064                      2.2 GB of K/V
  bench     B = 512, L = 1064, softcap 50          4.5 GB (bench.py's layer)
  fp8       headline with an e4m3 cache
  ragged    B = 512, L uniform in 64..2048, seed 0
  splitkv   B = 2, L = 4096, ONE kv head (G = 2)   8 MB: fits the caches

Timing: one untimed round, then `--rounds` rounds with the variants' order
flipped every round; in a round each variant runs 3 warm-up calls and then
`--iters` calls between two HIP events. Reported per variant: the
rounds, their median, max - min, and effective TB/s = K/V bytes from the
shapes / median. Back-to-back replays re-read the same K/V, which only
matters when it fits the 256 MB Infinity Cache (splitkv): `--cold` times
every call on its own after a 512 MiB write to another buffer, the state a
layer's K/V is in when the step comes back to it.

  python tests/decode_kv_stream_bench.py [--shapes headline,bench] [--cold]
  python tests/decode_kv_stream_bench.py --rope
A build that predates the switches ignores them: run it with LLMQ_OPS_SO and
read either column.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from llmq_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = {
    "headline": dict(B=256, L=1064),
    "bench": dict(B=512, L=1064, softcap=50.0),
    "fp8": dict(B=256, L=1064, fp8=True),
    "ragged": dict(B=512, L=None),
    "splitkv": dict(B=2, L=4096, H=2, KVH=1),
}


def make_case(B, L, H=16, KVH=8, D=256, bs=16, fp8=False, softcap=0.0):
    gen = torch.Generator().manual_seed(0)
    if L is None:
        lens = torch.randint(64, 2049, (B,), generator=gen)
    else:
        lens = torch.full((B,), L)
    nblk = (lens + bs - 1) // bs
    width = int(nblk.max())
    first = torch.cumsum(nblk, 0) - nblk + 1  # block 0 stays unused
    bt = first[:, None] + torch.arange(width)[None, :]
    bt = torch.minimum(bt, (first + nblk - 1)[:, None]).to(torch.int32)
    num_blocks = int(nblk.sum()) + 1
    torch.manual_seed(0)
    q = torch.randn(B, H, D, device=DEV, dtype=torch.bfloat16)
    kc = torch.randn(num_blocks, KVH, bs, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn(num_blocks, KVH, bs, D, device=DEV, dtype=torch.bfloat16)
    if fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
    kv_bytes = 2 * int(lens.sum()) * KVH * D * (1 if fp8 else 2)
    args = (q, kc, vc, bt.to(DEV), lens.to(torch.int32).to(DEV), D ** -0.5,
            softcap, 0)
    return args, kv_bytes


def _report(name, variants, times, nbytes):
    for v in variants:
        ts = times[v]
        med = statistics.median(ts)
        rounds = " ".join(f"{t * 1e3:.4f}" for t in ts)
        print(f"  {name:<9} {v:<12} ms: {rounds}  median {med * 1e3:.4f}  "
              f"spread {(max(ts) - min(ts)) * 1e3:.4f}  "
              f"{nbytes / med / 1e12:.2f} TB/s", flush=True)


def _order(variants, r):
    """Round -1 is an untimed warm-up (clock ramp); the order of the variants
    flips every round, because the later slot of a round measured about 1 %
    faster than the earlier one with the SAME kernel in both."""
    items = list(variants.items())
    return items if r % 2 == 0 else items[::-1]


def time_calls(fn, iters, cold_buf=None):
    """Seconds per call: back to back, or (cold_buf) each call alone after a
    write that evicts the caches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if cold_buf is None:
        for _ in range(3):
            fn()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / iters
    fn()
    per = []
    for _ in range(iters):
        cold_buf.add_(1)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(per)


def decode_bench(args):
    variants = {f"kv_nt={p}": p for p in args.policies.split(",")}
    cold_buf = (torch.zeros(512 << 20, dtype=torch.uint8, device=DEV)
                if args.cold else None)
    print(f"decode K/V stream, LLMQ_DECODE_PIPE={os.environ.get('LLMQ_DECODE_PIPE', '64')}"
          f" {'cold (512 MiB write before each call)' if args.cold else 'back to back'},"
          f" {args.rounds} rounds x {args.iters} calls")
    for name in args.shapes.split(","):
        case, kv_bytes = make_case(**SHAPES[name])
        outs = {}
        for v, env in variants.items():
            os.environ["LLMQ_DECODE_KV_NT"] = env
            outs[v] = ops.paged_decode_attention(*case)
        first = next(iter(outs.values()))
        assert all(torch.equal(first, o) for o in outs.values()), name
        times = {v: [] for v in variants}
        for r in range(-1, args.rounds):
            for v, env in _order(variants, r):
                os.environ["LLMQ_DECODE_KV_NT"] = env
                t = time_calls(
                    lambda: ops.paged_decode_attention(*case), args.iters, cold_buf)
                if r >= 0:
                    times[v].append(t)
        print(f" {name}: K/V {kv_bytes / 1e9:.3f} GB")
        _report(name, variants, times, kv_bytes)
        del case, outs
        torch.cuda.empty_cache()


def rope_bench(args):
    """rope_and_cache at [512 tokens, 16/8 heads, D = 256], bf16 cache, 200
    calls per captured graph, 10 replays per round."""
    T, HQ, HK, D, bs = 512, 16, 8, 256, 16
    torch.manual_seed(0)
    qkv = torch.randn(T, (HQ + 2 * HK) * D, device=DEV, dtype=torch.bfloat16)
    q, k, v = qkv.split([HQ * D, HK * D, HK * D], dim=-1)
    q, k, v = q.view(T, HQ, D), k.view(T, HK, D), v.view(T, HK, D)
    nb = T * 70 // bs
    kc = torch.zeros(nb, HK, bs, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    cos_sin = ops.build_rope_cache(4096, D, 10000.0, DEV)
    pos = torch.full((T,), 1063, device=DEV, dtype=torch.long)
    slots = (torch.arange(T, device=DEV) * (nb * bs // T) + 1063 % bs).long()
    # q, k read + written, v read, two cache rows written, cos/sin row read
    nbytes = T * ((2 * HQ + 2 * HK + HK + 2 * HK) * D * 2) + T * D * 4
    variants = {"rope_vec=0": "0", "rope_vec=1": "1"}
    graphs = {}
    for name, env in variants.items():
        os.environ["LLMQ_ROPE_VEC"] = env
        ops.rope_and_cache(q, k, v, kc, vc, pos, cos_sin, slots)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(200):
                ops.rope_and_cache(q, k, v, kc, vc, pos, cos_sin, slots)
        graphs[name] = g
    times = {n: [] for n in variants}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(-1, args.rounds):
        for name, g in _order(graphs, r):
            g.replay()
            a.record()
            for _ in range(10):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            if r >= 0:
                times[name].append(a.elapsed_time(b) * 1e-3 / 2000)
    print(f"rope_and_cache [{T} tokens, {HQ}/{HK} heads, D={D}] in a graph, "
          f"{nbytes / 1e6:.1f} MB per call (values below are us, not ms)")
    _report("rope", variants, {n: [t * 1e3 for t in ts] for n, ts in times.items()},
            nbytes * 1e3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--policies", default="0,1",
                    help="LLMQ_DECODE_KV_NT values to alternate")
    ap.add_argument("--rope", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.has_hip_ext()
    if args.rope:
        rope_bench(args)
    else:
        decode_bench(args)


if __name__ == "__main__":
    main()
