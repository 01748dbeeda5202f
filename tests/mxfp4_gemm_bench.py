"""Benchmark (MI355X): the MXFP4 (W4A8) GEMM against the fp8 and bf16 GEMMs.

  kernels  ops.mxfp4_linear, ops.fp8_linear and bf16 F.linear on the four
           layer projections of gemma-2-9b and qwen2.5-72b (one GPU) at T in
           {1, 16, 64, 256, 512, 4096}. Device events around REPS back-to-back
           calls after a warm-up; the three versions alternate round by round
           in this process; median over ROUNDS. Reports us per call, the
           weight + activation + output bytes each version has to move per
           second, and FLOP/s (2 T N K), all computed from the shapes.
  engine   fp8_weights_bench.bench_engine for quantization none / fp8 / mxfp4:
           decode ms/step, weight bytes and KV blocks.

Usage (repository root):
  python tests/mxfp4_gemm_bench.py kernels [out.json]
  python tests/mxfp4_gemm_bench.py engine {headline,72b} [out.json]
Prints one JSON object. Results: profiles/mxfp4_weights.md"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llmq_amd import ops  # noqa: E402
from llmq_amd.engine.model_specs import resolve_spec  # noqa: E402

MODELS = ("gemma-2-9b", "qwen2.5-72b")
TS = (1, 16, 64, 256, 512, 4096)
REPS, ROUNDS = 10, 7
DEV = torch.device("cuda:0")


def projections(model: str) -> dict:
    s = resolve_spec(model)
    q, kv = s.num_heads * s.head_dim, s.num_kv_heads * s.head_dim
    return {"qkv": (q + 2 * kv, s.hidden_size), "o": (s.hidden_size, q),
            "gate_up": (2 * s.intermediate_size, s.hidden_size),
            "down": (s.hidden_size, s.intermediate_size)}


def time_round(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / REPS  # us per call


def bench_shape(T: int, N: int, K: int) -> dict:
    torch.manual_seed(0)
    w = torch.randn(N, K, device=DEV).bfloat16() * 0.02
    a = torch.randn(T, K, device=DEV).bfloat16()
    a_q, a_s = ops.quant_fp8_rows(a)
    w_q, w_s = ops.quant_fp8_rows(w)
    w4 = ops.mxfp4_pack_weight(*ops.quant_mxfp4_weight(w))
    variants = {
        "mxfp4": (lambda: ops.mxfp4_linear(a_q, a_s, w4), T * K + N * K * 17 // 32),
        "fp8": (lambda: ops.fp8_linear(a_q, a_s, w_q, w_s), T * K + N * K),
        "bf16": (lambda: F.linear(a, w), 2 * T * K + 2 * N * K),
    }
    for fn, _ in variants.values():
        for _ in range(3):
            fn()
    times = {n: [] for n in variants}
    for _ in range(ROUNDS):
        for name, (fn, _) in variants.items():
            times[name].append(time_round(fn))
    res = {}
    for name, (_, in_bytes) in variants.items():
        us = statistics.median(times[name])
        res[name] = {"us": round(us, 2), "min_us": round(min(times[name]), 2),
                     "GB_per_s": round((in_bytes + 2 * T * N) / us / 1e3, 1),
                     "TFLOP_per_s": round(2.0 * T * N * K / us / 1e6, 2)}
    return res


def main() -> None:
    args = sys.argv[1:]
    if not args or args[0] not in ("kernels", "engine"):
        raise SystemExit(__doc__)
    assert torch.cuda.is_available() and ops.has_hip_ext(), "needs the GPU and the HIP extension"
    res = {"mode": args[0]}
    if args[0] == "kernels":
        out = args[1] if len(args) > 1 else None
        for model in MODELS:
            for name, (N, K) in projections(model).items():
                for T in TS:
                    key = f"{model}/{name}/N{N}/K{K}/T{T}"
                    res[key] = bench_shape(T, N, K)
                    print(f"[mxfp4_gemm_bench] {key}: {res[key]}", file=sys.stderr, flush=True)
    else:
        from fp8_weights_bench import SHAPES, bench_engine

        out = args[2] if len(args) > 2 else None
        res["shape_name"] = args[1]
        for q in ("none", "fp8", "mxfp4"):
            res[q] = bench_engine(SHAPES[args[1]], q)
            print(f"[mxfp4_gemm_bench] {q}: {res[q]}", file=sys.stderr, flush=True)
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
