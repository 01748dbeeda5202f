"""Benchmark (MI355X): quantization="fp8" (W8A8) against the bf16 engine.

  engine   Builds the engine twice in this process, quantization "none" then
           "fp8", fills the resident batch and times decode steps the way
           bench.py does (host clock around steps that end in a device
           synchronise). Reports ms/step, tokens/s, weight bytes and the KV
           blocks the engine sized from free HBM for each.
  kernels  Each fused quant kernel against the composition it replaces
           (unfused kernel + quant_fp8_rows), the stand-alone quant_fp8_rows,
           and each layer GEMM in bf16 (F.linear) and fp8 (ops.fp8_linear) at
           the shape's decode batch. Device events around REPS back-to-back
           calls; variants alternate round by round; median over ROUNDS.

Shapes: "headline" = bench.py's (tower-plus-9b, batch 512, prompt 1024,
model len 4096); "72b" = qwen2.5-72b, batch 256, prompt 128, model len 4096.

Usage (repository root):
  python tests/fp8_weights_bench.py {engine,kernels} {headline,72b} [out.json]
Prints one JSON object. Results: profiles/fp8_weights.md"""
import gc
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llmq_amd import ops  # noqa: E402
from llmq_amd.engine.model_specs import resolve_spec  # noqa: E402

SHAPES = {
    "headline": dict(model="tower-plus-9b", batch=512, prompt_len=1024,
                     max_model_len=4096),
    "72b": dict(model="qwen2.5-72b", batch=256, prompt_len=128,
                max_model_len=4096),
}
STEPS, WARMUP = 32, 8
REPS, ROUNDS = 10, 10
DEV = torch.device("cuda:0")


def bench_engine(shape: dict, quantization: str) -> dict:
    import numpy as np

    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine
    from llmq_amd.engine.sampling_params import SamplingParams

    batch = shape["batch"]
    t0 = time.perf_counter()
    engine = LLMEngine(EngineConfig(
        model=shape["model"], max_num_seqs=batch,
        max_model_len=shape["max_model_len"], max_prefill_tokens=16384,
        load_weights=False, fast_init=True, device="cuda:0",
        hipgraph_max_batch=batch, seed=1234, quantization=quantization,
    ))
    init_s = time.perf_counter() - t0
    rng = np.random.default_rng(42)
    params = SamplingParams(temperature=0.7, max_tokens=shape["max_model_len"],
                            ignore_eos=True)
    for i in range(batch):
        ids = rng.integers(0, engine.spec.vocab_size, size=shape["prompt_len"]).tolist()
        engine.add_request(f"b{i}", prompt_token_ids=ids, params=params)
    t0 = time.perf_counter()
    guard = 0
    while engine.scheduler.num_waiting > 0 or engine.scheduler.prefilling:
        engine.step()
        guard += 1
        assert guard < 10000, "admission stalled"
    torch.cuda.synchronize()
    admit_s = time.perf_counter() - t0
    for _ in range(WARMUP):
        engine.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        engine.step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    assert engine.scheduler.num_running == batch
    res = {
        "ms_per_step": round(elapsed / STEPS * 1000.0, 3),
        "tokens_per_s": round(batch * STEPS / elapsed, 1),
        "weight_gb": round(engine.model.weight_bytes() / 2 ** 30, 2),
        "kv_blocks": engine.allocator.num_blocks,
        "graphs": bool(engine.runner.use_graphs),
        "init_s": round(init_s, 1),
        "admission_s": round(admit_s, 2),
    }
    del engine
    gc.collect()
    torch.cuda.empty_cache()
    return res


def bench_kernels(shape: dict) -> dict:
    spec = resolve_spec(shape["model"])
    T, H, I = shape["batch"], spec.hidden_size, spec.intermediate_size
    q_size = spec.num_heads * spec.head_dim
    kv_size = spec.num_kv_heads * spec.head_dim
    offset = 1.0 if spec.family == "gemma2" else 0.0
    torch.manual_seed(0)

    def t(*s):
        return torch.randn(*s, device=DEV).bfloat16()

    x, r, gu, attn = t(T, H), t(T, H), t(T, 2 * I), t(T, q_size)
    w, w2 = t(H), t(H)
    eps = spec.rms_eps
    act, act_q = (("gelu_tanh_and_mul", ops.gelu_tanh_and_mul_quant_fp8) if spec.gelu
                  else ("silu_and_mul", ops.silu_and_mul_quant_fp8))
    act_fn = getattr(ops, act)
    variants = {
        "quant_fp8_rows_attn": lambda: ops.quant_fp8_rows(attn),
        "act_quant_fused": lambda: act_q(gu),
        "act_quant_composed": lambda: ops.quant_fp8_rows(act_fn(gu)),
        "act_bf16_only": lambda: act_fn(gu),
        "add_norm_quant_fused": lambda: ops.fused_add_rmsnorm_quant_fp8(x, r, w, eps, offset),
        "add_norm_quant_composed": lambda: ops.quant_fp8_rows(
            ops.fused_add_rmsnorm(x, r, w, eps, offset)[0]),
        "add_norm_bf16_only": lambda: ops.fused_add_rmsnorm(x, r, w, eps, offset),
        "sandwich_quant_fused": lambda: ops.norm_add_norm_quant_fp8(x, r, w, w2, eps, offset),
        "sandwich_quant_composed": lambda: ops.quant_fp8_rows(
            ops.norm_add_norm(x, r, w, w2, eps, offset)[0]),
        "sandwich_bf16_only": lambda: ops.norm_add_norm(x, r, w, w2, eps, offset),
        "rmsnorm_quant_fused": lambda: ops.rmsnorm_quant_fp8(x, w, eps, offset),
        "rmsnorm_quant_composed": lambda: ops.quant_fp8_rows(ops.rmsnorm(x, w, eps, offset)),
    }
    for name, (n, k) in {"qkv": (q_size + 2 * kv_size, H), "o": (H, q_size),
                         "gate_up": (2 * I, H), "down": (H, I)}.items():
        a, wt = t(T, k), t(n, k) * 0.02
        a_q, a_s = ops.quant_fp8_rows(a)
        w_q, w_s = ops.quant_fp8_rows(wt)
        variants[f"gemm_{name}_bf16"] = lambda a=a, wt=wt: F.linear(a, wt)
        variants[f"gemm_{name}_fp8"] = (
            lambda a_q=a_q, a_s=a_s, w_q=w_q, w_s=w_s: ops.fp8_linear(a_q, a_s, w_q, w_s))

    def reset():
        # the in-place norms feed their output back in: keep the values tame
        r.normal_()
        x.normal_()

    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for rnd in range(ROUNDS + 1):
        for name, fn in variants.items():
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(REPS):
                fn()
            b.record()
            torch.cuda.synchronize()
            if rnd >= 1:
                times[name].append(a.elapsed_time(b) * 1000.0 / REPS)  # us per call
    res = {n: {"median_us": round(statistics.median(ts), 2),
               "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
           for n, ts in times.items()}
    res["shape"] = {"T": T, "hidden": H, "intermediate": I, "q_size": q_size}
    return res


def main() -> None:
    args = sys.argv[1:]
    if len(args) < 2 or args[0] not in ("engine", "kernels") or args[1] not in SHAPES:
        raise SystemExit(__doc__)
    assert torch.cuda.is_available() and ops.has_hip_ext(), "needs the GPU and the HIP extension"
    shape = SHAPES[args[1]]
    res = {"mode": args[0], "shape_name": args[1], **shape}
    if args[0] == "engine":
        for q in ("none", "fp8"):
            res[q] = bench_engine(shape, q)
            print(f"[fp8_weights_bench] {q}: {res[q]}", file=sys.stderr, flush=True)
        res["fp8_over_none_step_time"] = round(
            res["fp8"]["ms_per_step"] / res["none"]["ms_per_step"], 4)
    else:
        res["kernels"] = bench_kernels(shape)
    if len(args) > 2:
        with open(args[2], "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
