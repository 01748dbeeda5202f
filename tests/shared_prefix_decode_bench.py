#!/usr/bin/env python3
"""Shared-prefix decode microbenchmark (GPU box tool, not a pytest): the
cascade op against paged_decode_attention on the concatenated tables, same
process, same inputs, at B = 512, 16 heads / 8 kv heads, D = 256, for
(prefix, suffix) token pairs; (0, 512) is the cost of the flag when nothing is
shared. Timing and report are those of tests/decode_kv_stream_bench.py (one
untimed round, then `--rounds` rounds of `--iters` calls, order flipped every
round).

  python tests/shared_prefix_decode_bench.py [--pairs 1024:256,256:256,0:512]
  python tests/shared_prefix_decode_bench.py --engine   # tokens/s, flag off/on
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from llmq_amd import ops  # noqa: E402
from llmq_amd.ops import torch_ref  # noqa: E402
from tests.decode_kv_stream_bench import _order, _report, time_calls  # noqa: E402

DEV = torch.device("cuda:0")


def make_case(prefix, suffix, B=512, H=16, KVH=8, D=256, bs=16):
    pb, sb = prefix // bs, -(-suffix // bs)
    torch.manual_seed(0)
    q = torch.randn(B, H, D, device=DEV, dtype=torch.bfloat16)
    kc = torch.randn(1 + pb + B * sb, KVH, bs, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    ptab = torch.arange(1, 1 + max(pb, 1), dtype=torch.int32, device=DEV)
    bt = (1 + pb + torch.arange(B * sb, dtype=torch.int32, device=DEV)).view(B, sb)
    plen = torch.tensor([prefix], dtype=torch.int32, device=DEV)
    cl = torch.full((B,), suffix, dtype=torch.int32, device=DEV)
    tables, lens = torch_ref.concat_prefix_tables(ptab, plen, bt, cl, bs)
    tables = tables[:, : pb + sb].contiguous()
    kv_bytes = 2 * B * KVH * (prefix + suffix) * D * 2  # what the plain op streams
    return (q, kc, vc), (ptab, plen, bt, cl), (tables, lens), kv_bytes


def op_bench(args) -> None:
    print(f"shared-prefix decode, B=512 16/8 heads D=256, {args.rounds} rounds x "
          f"{args.iters} calls; TB/s counts the plain op's K/V stream for both")
    for pair in args.pairs.split(","):
        prefix, suffix = (int(x) for x in pair.split(":"))
        qkv, cascade, plain, kv_bytes = make_case(prefix, suffix)
        scale = 256 ** -0.5
        fns = {
            "plain": lambda: ops.paged_decode_attention(*qkv, *plain, scale),
            "cascade": lambda: ops.shared_prefix_decode_attention(*qkv, *cascade, scale),
        }
        err = (fns["plain"]().float() - fns["cascade"]().float()).abs().max()
        assert float(err) < 2e-2, float(err)
        times = {v: [] for v in fns}
        for r in range(-1, args.rounds):
            for v, fn in _order(fns, r):
                t = time_calls(fn, args.iters)
                if r >= 0:
                    times[v].append(t)
        name = f"{prefix}+{suffix}"
        _report(name, fns, times, kv_bytes)
        mp, mc = (statistics.median(times[v]) for v in ("plain", "cascade"))
        spread = max(max(t) - min(t) for t in times.values())
        print(f"  {name:<9} cascade vs plain: {(mc / mp - 1) * 100:+.1f} %  "
              f"({'outside' if abs(mc - mp) > 2 * spread else 'within'} 2x spread)",
              flush=True)
        del qkv, cascade, plain
        torch.cuda.empty_cache()


def engine_bench(args) -> None:
    """Decode tokens/s of the bench model on prompts that share a 1024-token
    head (the owner runs first), with the flag off and on, alternating."""
    import random

    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine
    from llmq_amd.engine.sampling_params import SamplingParams

    rng = random.Random(0)
    head = [rng.randrange(3, 30000) for _ in range(1024)]
    prompts = [head + [rng.randrange(3, 30000) for _ in range(32)] for _ in range(args.seqs)]
    params = SamplingParams(temperature=0.0, max_tokens=args.tokens, ignore_eos=True)
    rates = {False: [], True: []}
    for r in range(args.rounds):
        for flag in ((False, True) if r % 2 == 0 else (True, False)):
            eng = LLMEngine(EngineConfig(
                model=args.model, max_num_seqs=args.seqs, max_model_len=2048,
                max_prefill_tokens=16384, load_weights=False, fast_init=True,
                hipgraph_max_batch=args.seqs, enable_prefix_caching=True,
                shared_prefix_decode=flag))
            eng.add_request("own", prompt_token_ids=prompts[0],
                            params=SamplingParams(temperature=0.0, max_tokens=1))
            while eng.has_unfinished():
                eng.step()
            for i, p in enumerate(prompts):
                eng.add_request(f"r{i}", prompt_token_ids=p, params=params)
            while eng.scheduler.num_waiting > 0 or eng.scheduler.prefilling:
                eng.step()  # admission; the timed phase is pure decode
            torch.cuda.synchronize()
            n, t0 = 0, time.perf_counter()
            while eng.has_unfinished():
                n += sum(len(o.new_token_ids) for o in eng.step())
            torch.cuda.synchronize()
            rates[flag].append(n / (time.perf_counter() - t0))
            del eng
            torch.cuda.empty_cache()
    for flag, rs in rates.items():
        print(f"  shared_prefix_decode={flag}: tokens/s "
              + " ".join(f"{x:.0f}" for x in rs) + f"  median {statistics.median(rs):.0f}",
              flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1024:256,256:256,0:512")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--model", default="tower-plus-9b")
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.has_hip_ext()
    engine_bench(args) if args.engine else op_bench(args)


if __name__ == "__main__":
    main()
