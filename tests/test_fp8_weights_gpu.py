"""quantization="fp8" (W8A8) on the GPU: the HIP quant kernels bit for bit
against the torch contract, the fp8 GEMM against an fp64 reference, and the
engine end to end. Run with `pytest -m gpu` on an MI355X."""

from __future__ import annotations

import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from llmq_amd import ops
    from llmq_amd.ops import torch_ref
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
TS = [1, 3, 65]
KS = [64, 1008, 3584, 14336]  # 14336 is past the fused norms' register form
EPS = 1e-6


def _gen(*salt) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(salt).encode()))


def _rows(T, K, g) -> torch.Tensor:
    """T bf16 rows whose magnitudes run from 1e-6 to 1e4."""
    mag = torch.logspace(-6, 4, T) if T > 1 else torch.tensor([1.0])
    return (torch.randn(T, K, generator=g) * mag.unsqueeze(1)).bfloat16()


def _special_rows(K, g) -> torch.Tensor:
    x = _rows(6, K, g)
    x[0] = 0                                    # all-zero row
    x[1] = 0
    x[1, -1] = 0.37                             # single nonzero, last element
    x[2, K // 3] = -x[2].float().abs().max() * 4  # the amax element negative
    x[3, K - 3] = x[3].float().abs().max() * 2  # amax in the final partial vector
    x[4] = (torch.randn(K, generator=g) * 1e-6).bfloat16()
    x[5] = (torch.randn(K, generator=g) * 1e4).bfloat16()
    return x


def assert_same_quant(got, x_ref: torch.Tensor):
    """got = (q, scale) from the GPU; x_ref = the bf16 rows it stands for."""
    q, scale = got[0], got[1]
    rq, rs = torch_ref.quant_fp8_rows(x_ref.cpu())
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert q.shape == rq.shape and scale.shape == rs.shape
    assert torch.equal(scale.cpu(), rs)
    assert torch.equal(q.view(torch.uint8).cpu(), rq.view(torch.uint8))


class TestQuantRows:
    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("T", TS)
    def test_matches_contract(self, T, K):
        x = _rows(T, K, _gen("rows", T, K))
        assert_same_quant(ops.quant_fp8_rows(x.to(DEV)), x)

    @pytest.mark.parametrize("K", KS + [29568, 40000])  # 40000: two-trip kernel
    def test_edge_rows(self, K):
        x = _special_rows(K, _gen("special", K))
        q, scale = ops.quant_fp8_rows(x.to(DEV))
        assert_same_quant((q, scale), x)
        qf = q.float().cpu()
        assert not qf.isnan().any()
        assert (qf[0] == 0).all() and qf[1, -1] == 448 and (qf[1, :-1] == 0).all()
        assert qf[2, K // 3] == -448 and qf[3, K - 3] == 448

    def test_strided_rows(self):
        """A column slice of a wider tensor (the attention output's layout
        when it is a view): rows are read through the row stride."""
        wide = _rows(5, 256, _gen("strided")).to(DEV)
        x = wide[:, 64:192]
        assert not x.is_contiguous()
        assert_same_quant(ops.quant_fp8_rows(x), x)


class TestFusedQuant:
    """Each fused kernel against the contract applied to the output of the
    kernel it extends (which has its own fp32-reference tests)."""

    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("T", TS)
    @pytest.mark.parametrize("act", ["silu_and_mul", "gelu_tanh_and_mul"])
    def test_act_and_mul(self, act, T, K):
        gu = _rows(T, 2 * K, _gen(act, T, K)).to(DEV)
        before = gu.clone()
        got = getattr(ops, act + "_quant_fp8")(gu)
        assert_same_quant(got, getattr(ops, act)(gu))
        assert torch.equal(gu, before)

    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("T", TS)
    @pytest.mark.parametrize("offset", [0.0, 1.0])
    def test_rmsnorm(self, offset, T, K):
        g = _gen("rms", T, K)
        x = _rows(T, K, g).to(DEV)
        w = torch.randn(K, generator=g).bfloat16().to(DEV)
        assert_same_quant(ops.rmsnorm_quant_fp8(x, w, EPS, offset),
                          ops.rmsnorm(x, w, EPS, offset))

    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("T", TS)
    def test_fused_add_rmsnorm(self, T, K):
        g = _gen("far", T, K)
        x, r = _rows(T, K, g).to(DEV), _rows(T, K, g).to(DEV)
        w = torch.randn(K, generator=g).bfloat16().to(DEV)
        h, r_ref = ops.fused_add_rmsnorm(x.clone(), r.clone(), w, EPS, 0.0)
        q, scale, r_new = ops.fused_add_rmsnorm_quant_fp8(x.clone(), r.clone(), w, EPS, 0.0)
        assert_same_quant((q, scale), h)
        assert torch.equal(r_new.view(torch.int16), r_ref.view(torch.int16))

    @pytest.mark.parametrize("K", KS)  # 3584: register form; 14336: not
    @pytest.mark.parametrize("T", TS)
    def test_norm_add_norm(self, T, K):
        g = _gen("nan", T, K)
        x, r = _rows(T, K, g).to(DEV), _rows(T, K, g).to(DEV)
        w_post = torch.randn(K, generator=g).bfloat16().to(DEV)
        w_pre = torch.randn(K, generator=g).bfloat16().to(DEV)
        h, r_ref = ops.norm_add_norm(x.clone(), r.clone(), w_post, w_pre, EPS, 1.0)
        q, scale, r_new = ops.norm_add_norm_quant_fp8(
            x.clone(), r.clone(), w_post, w_pre, EPS, 1.0)
        assert_same_quant((q, scale), h)
        assert torch.equal(r_new.view(torch.int16), r_ref.view(torch.int16))


class TestFp8Linear:
    @pytest.mark.parametrize("bias", [False, True])
    @pytest.mark.parametrize("N", [48, 512])
    @pytest.mark.parametrize("K", [64, 1008])
    @pytest.mark.parametrize("T", [1, 17, 64])
    def test_against_fp64(self, T, K, N, bias):
        g = _gen("gemm", T, K, N, bias)
        # distinct per-row and per-channel scales over 1e-3..1e3, running in
        # opposite directions: a transposed or swapped scale cannot pass
        a = torch.randn(T, K, generator=g) * torch.logspace(-3, 3, max(T, 2))[:T, None]
        w = torch.randn(N, K, generator=g) * torch.logspace(3, -3, N)[:, None]
        a_q, a_s = torch_ref.quant_fp8_rows(a.bfloat16())
        w_q, w_s = torch_ref.quant_fp8_rows(w.bfloat16())
        b = torch.randn(N, generator=g).bfloat16() if bias else None
        ad = a_q.double() * a_s.double()[:, None]
        wd = w_q.double() * w_s.double()[:, None]
        ref = ad @ wd.T
        if bias:
            ref = ref + b.double()
        out = ops.fp8_linear(a_q.to(DEV), a_s.to(DEV), w_q.to(DEV), w_s.to(DEV),
                             b.to(DEV) if bias else None)
        assert out.dtype == torch.bfloat16 and out.shape == (T, N)
        # bf16 rounding of the output + fp32 accumulation of K products
        bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (ad.abs() @ wd.abs().T)
        err = (out.double().cpu() - ref).abs()
        print(f"fp8_linear T={T} K={K} N={N} bias={bias}: "
              f"max err/bound = {(err / bound).max().item():.3f}")
        assert (err <= bound).all()


# -------------------------------------------------------------- end to end --

PROMPTS = ["hello world test", "abcdefgh" * 12]  # TestEngineFamiliesGPU's


def _engine(model, device, **kw):
    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine

    kw.setdefault("max_num_seqs", 2)
    kw.setdefault("max_model_len", 256)
    kw.setdefault("num_kv_blocks", 128)
    if device == "cpu":
        kw["enforce_eager"] = True
    return LLMEngine(EngineConfig(model=model, load_weights=False, device=device, **kw))


def _final_logits(engine) -> torch.Tensor:
    """One packed prefill of PROMPTS; fp32 logits of each prompt's last
    position, on the CPU."""
    from llmq_amd.engine.forward_meta import PrefillMeta

    dev = engine.device
    bs = engine.config.kv_block_size
    seqs = [engine.tokenizer.encode(p) for p in PROMPTS]
    ids, pos, slots, cu = [], [], [], [0]
    for toks in seqs:
        blocks = engine.allocator.allocate((len(toks) + bs - 1) // bs)
        ids += toks
        pos += range(len(toks))
        slots += [blocks[p // bs] * bs + p % bs for p in range(len(toks))]
        cu.append(len(ids))
    meta = PrefillMeta(
        cu_seqlens=torch.tensor(cu, dtype=torch.int32, device=dev),
        max_seqlen=max(len(t) for t in seqs),
        slot_mapping=torch.tensor(slots, dtype=torch.long, device=dev),
    )
    hidden = engine.model.forward(
        torch.tensor(ids, dtype=torch.long, device=dev),
        torch.tensor(pos, dtype=torch.long, device=dev), engine.kv_cache, meta)
    last = torch.tensor(cu[1:], device=dev) - 1
    return engine.model.compute_logits(hidden[last]).float().cpu()


def _greedy(engine, n=12):
    from llmq_amd.engine.sampling_params import SamplingParams

    params = SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True)
    for i, p in enumerate(PROMPTS):
        engine.add_request(f"r{i}", prompt=p, params=params)
    outs = {}
    while engine.has_unfinished():
        for out in engine.step():
            outs.setdefault(out.request_id, []).extend(out.new_token_ids)
    return [outs[f"r{i}"] for i in range(len(PROMPTS))]


def _rel_l2(a, b) -> float:
    return ((a - b).norm() / b.norm()).item()


class TestEngineFp8:
    @pytest.mark.parametrize("model", ["tiny-llama", "tiny-qwen3", "tiny-gemma2"])
    def test_gpu_noise_below_quantisation_error(self, model):
        """The GPU fp8 engine is closer to the CPU fake-quant engine than
        fake-quant is to the unquantised fp32 model. The yardstick e_quant
        comes from reference code alone."""
        cpu_plain = _final_logits(_engine(model, "cpu"))
        cpu_eng = _engine(model, "cpu", quantization="fp8")
        cpu_fp8 = _final_logits(cpu_eng)
        gpu_eng = _engine(model, "cuda", quantization="fp8", enforce_eager=True)
        # same seed, same fp8 weights on both devices
        for (k, a), (_, b) in zip(cpu_eng.model.named_tensors().items(),
                                  gpu_eng.model.named_tensors().items()):
            if a.dtype == torch.float8_e4m3fn:
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8).cpu()), k
            elif k.endswith("_scale"):
                assert torch.equal(a, b.cpu()), k
        gpu_fp8 = _final_logits(gpu_eng)
        e_impl = _rel_l2(gpu_fp8, cpu_fp8)
        e_quant = _rel_l2(cpu_fp8, cpu_plain)
        print(f"{model}: e_impl={e_impl:.5f} e_quant={e_quant:.5f}")
        assert e_quant > 0
        assert e_impl < e_quant

    def test_hipgraph_equals_eager(self):
        graphs = _engine("tiny-llama", "cuda", quantization="fp8")
        assert graphs.runner.use_graphs
        eager = _engine("tiny-llama", "cuda", quantization="fp8", enforce_eager=True)
        assert not eager.runner.use_graphs
        toks = _greedy(graphs)
        assert [len(t) for t in toks] == [12, 12]
        assert toks == _greedy(eager)

    def test_with_fp8_kv_cache(self):
        eng = _engine("tiny-llama-d128", "cuda", quantization="fp8",
                      kv_cache_dtype="fp8", max_num_seqs=4, num_kv_blocks=512)
        assert eng.kv_cache.k[0].dtype == torch.float8_e4m3fn
        assert eng.model.layers[0].qkv.dtype == torch.float8_e4m3fn
        toks = _greedy(eng, n=8)
        assert [len(t) for t in toks] == [8, 8]
        assert all(0 <= t < eng.spec.vocab_size for seq in toks for t in seq)

    def test_fp16_rejected(self):
        with pytest.raises(ValueError, match="bf16"):
            _engine("tiny-llama", "cuda", quantization="fp8", dtype="float16")
