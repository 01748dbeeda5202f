"""quantization="mxfp4" (W4A8) on the MI355X: the scaled-MFMA GEMM against an
exact and an fp64 reference, and the engine end to end (`pytest -m gpu`)."""

from __future__ import annotations

import functools
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from llmq_amd import ops
    from llmq_amd.ops import torch_ref
    from test_fp8_weights_gpu import _engine, _final_logits, _greedy, _rel_l2
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
T_MAX = 257


def _gen(*salt) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(salt).encode()))


def _to_dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@functools.lru_cache(maxsize=None)
def _exact_case(K: int, N: int):
    """Operands whose every partial sum is a multiple of 2^-2 below 2^22: A
    integers in [-4, 4], W all 16 codes with block scales 2^-1..2^1, a_scale a
    power of two, integer bias; rows, columns and K blocks drawn independently."""
    g = _gen("exact", K, N)
    a = torch.randint(-4, 5, (T_MAX, K), generator=g).float()
    a_s = 2.0 ** (torch.arange(T_MAX) % 5 - 2).float()
    codes = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, generator=g)
    scales = torch.randint(126, 129, (N, K // 32), dtype=torch.uint8, generator=g)
    bias = torch.randint(-8, 9, (N,), generator=g).bfloat16()
    w = torch_ref.dequant_mxfp4_weight(codes, scales)
    ref = (a.double() @ w.double().T) * a_s.double()[:, None]
    a_q = a.to(torch.float8_e4m3fn)
    # exact in fp32 in any summation order: the fp32 reference agrees
    assert torch.equal(torch_ref.mxfp4_linear(a_q, a_s, codes, scales).double(), ref)
    assert torch.equal((ref + bias.double()).float().double(), ref + bias.double())
    return a_q, a_s, codes, scales, bias, ref


class TestGemm:
    @pytest.mark.parametrize("bias", [False, True])
    @pytest.mark.parametrize("N", [48, 272, 512])
    @pytest.mark.parametrize("K", [128, 384, 3584])
    @pytest.mark.parametrize("T", [1, 17, 64, 257])
    def test_exact_layout(self, T, K, N, bias):
        a_q, a_s, codes, scales, b, ref = _exact_case(K, N)
        want = (ref[:T] + b.double() if bias else ref[:T]).to(torch.bfloat16)
        a_q, a_s, codes, scales, b = _to_dev(
            a_q[:T].contiguous(), a_s[:T].contiguous(), codes, scales, b if bias else None)
        out = ops.mxfp4_linear(a_q, a_s, ops.mxfp4_pack_weight(codes, scales), b)
        assert out.dtype == torch.bfloat16 and out.shape == (T, N)
        bad = (out.cpu().view(torch.int16) != want.view(torch.int16)).nonzero()
        assert bad.numel() == 0, f"{len(bad)} wrong, first (t, n) = {bad[0].tolist()}"

    @pytest.mark.parametrize("bias", [False, True])
    @pytest.mark.parametrize("N", [48, 512])
    @pytest.mark.parametrize("K", [128, 1024])
    @pytest.mark.parametrize("T", [1, 17, 64])
    def test_random_operands(self, T, K, N, bias):
        g = _gen("random", T, K, N, bias)
        a = torch.randn(T, K, generator=g) * torch.logspace(-3, 3, max(T, 2))[:T, None]
        w = torch.randn(N, K, generator=g) * torch.logspace(3, -3, N)[:, None]
        a_q, a_s = torch_ref.quant_fp8_rows(a.bfloat16())
        codes, scales = torch_ref.quant_mxfp4_weight(w)
        b = torch.randn(N, generator=g).bfloat16() if bias else None
        ad = a_q.double() * a_s.double()[:, None]
        wd = torch_ref.dequant_mxfp4_weight(codes, scales).double()
        ref = ad @ wd.T + (b.double() if bias else 0)
        a_q, a_s, codes, scales, b = _to_dev(a_q, a_s, codes, scales, b)
        out = ops.mxfp4_linear(a_q, a_s, ops.mxfp4_pack_weight(codes, scales), b)
        # bf16 rounding of the output + fp32 accumulation of K products
        bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (ad.abs() @ wd.abs().T)
        err = (out.double().cpu() - ref).abs()
        print(f"mxfp4_linear T={T} K={K} N={N} bias={bias}: "
              f"max err/bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert (err <= bound).all()

    def test_weight_bits_same_on_gpu(self):
        w = torch.randn(64, 256, generator=_gen("bits")) * torch.logspace(-30, 30, 64)[:, None]
        w[3, 32:64] = 0
        cpu = torch_ref.quant_mxfp4_weight(w)
        gpu = torch_ref.quant_mxfp4_weight(w.to(DEV))
        assert torch.equal(gpu[0].cpu(), cpu[0]) and torch.equal(gpu[1].cpu(), cpu[1])


@pytest.fixture(scope="module")
def k512_checkpoint(tmp_path_factory):
    """hidden 512, 8 heads of 64, intermediate 1024: every local K is a
    multiple of 128 and every N a multiple of 16."""
    from llmq_amd.utils.tiny_checkpoint import build_tiny_checkpoint

    return build_tiny_checkpoint(tmp_path_factory.mktemp("mxfp4") / "ck", family="llama")


class TestEngineMxfp4:
    @pytest.mark.parametrize("model", ["checkpoint", "tiny-llama"])
    def test_gpu_noise_below_quantisation_error(self, model, k512_checkpoint):
        """The GPU mxfp4 engine is closer to the CPU fake-quant engine than
        fake-quant is to the unquantised fp32 model. No projection of the
        checkpoint falls back to fp8; on tiny-llama qkv and gate_up (K = 64)
        do, and o and down run the MXFP4 kernel."""
        fallbacks = set() if model == "checkpoint" else {"qkv", "gate_up"}
        model = k512_checkpoint if model == "checkpoint" else model
        cpu_plain = _final_logits(_engine(model, "cpu"))
        cpu_eng = _engine(model, "cpu", quantization="mxfp4")
        cpu_q = _final_logits(cpu_eng)
        gpu_eng = _engine(model, "cuda", quantization="mxfp4", enforce_eager=True)
        lw = gpu_eng.model.layers[0]
        assert {n for n in ("qkv", "o", "gate_up", "down")
                if getattr(lw, n).dtype != torch.uint8} == fallbacks
        e_impl = _rel_l2(_final_logits(gpu_eng), cpu_q)
        e_quant = _rel_l2(cpu_q, cpu_plain)
        print(f"{model}: e_impl={e_impl:.5f} e_quant={e_quant:.5f}")
        assert e_quant > 0
        assert e_impl < e_quant

    def test_hipgraph_equals_eager(self):
        graphs = _engine("tiny-llama", "cuda", quantization="mxfp4")
        assert graphs.runner.use_graphs
        eager = _engine("tiny-llama", "cuda", quantization="mxfp4", enforce_eager=True)
        toks = _greedy(graphs)
        assert toks == _greedy(eager)

    def test_fp16_rejected(self):
        with pytest.raises(ValueError, match="bf16"):
            _engine("tiny-llama", "cuda", quantization="mxfp4", dtype="float16")
