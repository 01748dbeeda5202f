#!/usr/bin/env python3
"""Decode V image microbenchmark (GPU box tool, not a pytest): the bf16 pipe
decode kernel with V staged as the tr16 subtile image against the line image
(LLMQ_DECODE_V_LINES, read per call), and the cache policy of the line
image's V DMAs (LLMQ_DECODE_KV_NT = 1: K `nt`, 2: K and V `nt`). The variants
alternate inside one process; shapes, timing and the report are those of
tests/decode_kv_stream_bench.py (one untimed round, then `--rounds` rounds of
`--iters` calls with the variants' order flipped every round; `--cold` times
each call alone after a 512 MiB write).

  python tests/decode_v_lines_bench.py [--shapes headline,bench] [--cold]
  python tests/decode_v_lines_bench.py --shapes d128,d128g12,d128split
  LLMQ_DECODE_PIPE=128 python tests/decode_v_lines_bench.py

A variant wins a shape only if its median beats the subtile column's by more
than twice the larger of the two spreads.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from llmq_amd import ops  # noqa: E402
from tests.decode_kv_stream_bench import (  # noqa: E402
    SHAPES, _order, _report, make_case, time_calls)

DEV = torch.device("cuda:0")
# the head dim the bench model does not have: D = 128 at the headline batch,
# with 12 q heads per kv head (NREG = 4), and split-KV
SHAPES = dict(SHAPES)
SHAPES.update({
    "d128": dict(B=256, L=1064, D=128),
    "d128g12": dict(B=256, L=1064, D=128, H=96, KVH=8),
    "d128split": dict(B=2, L=4096, H=2, KVH=1, D=128),
})
# name -> (LLMQ_DECODE_V_LINES, LLMQ_DECODE_KV_NT)
VARIANTS = {
    "subtile+K": ("0", "1"),
    "lines+K": ("1", "1"),
    "lines+KV": ("1", "2"),
}


def _select(env):
    os.environ["LLMQ_DECODE_V_LINES"], os.environ["LLMQ_DECODE_KV_NT"] = env


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,bench,ragged,splitkv")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.has_hip_ext()
    variants = {v: VARIANTS[v] for v in args.variants.split(",")}
    cold_buf = (torch.zeros(512 << 20, dtype=torch.uint8, device=DEV)
                if args.cold else None)
    print(f"decode V image, LLMQ_DECODE_PIPE={os.environ.get('LLMQ_DECODE_PIPE', '64')}"
          f" {'cold (512 MiB write before each call)' if args.cold else 'back to back'},"
          f" {args.rounds} rounds x {args.iters} calls")
    for name in args.shapes.split(","):
        case, kv_bytes = make_case(**SHAPES[name])
        outs = {}
        for v, env in variants.items():
            _select(env)
            outs[v] = ops.paged_decode_attention(*case)
        first = next(iter(outs.values()))
        assert all(torch.equal(first, o) for o in outs.values()), name
        times = {v: [] for v in variants}
        for r in range(-1, args.rounds):
            for v, env in _order(variants, r):
                _select(env)
                t = time_calls(
                    lambda: ops.paged_decode_attention(*case), args.iters, cold_buf)
                if r >= 0:
                    times[v].append(t)
        print(f" {name}: K/V {kv_bytes / 1e9:.3f} GB")
        _report(name, variants, times, kv_bytes)
        base = next(iter(variants))
        for v in list(variants)[1:]:
            mb, mv = statistics.median(times[base]), statistics.median(times[v])
            spread = max(max(times[x]) - min(times[x]) for x in (base, v))
            verdict = ("wins" if mb - mv > 2 * spread
                       else "slower" if mv - mb > spread else "within spread")
            print(f"  {name:<9} {v} vs {base}: {(mv / mb - 1) * 100:+.2f} %  {verdict}",
                  flush=True)
        del case, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
