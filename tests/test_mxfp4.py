"""quantization="mxfp4" (W4A8) on the CPU reference path: the OCP MXFP4
weight format bit by bit, the switch and its plumbing, and generation through
the fake-quant ops."""

from __future__ import annotations

import pytest
import torch

from llmq_amd import ops
from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.forward_meta import PrefillMeta
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.ops import torch_ref

CPU = torch.device("cpu")


def _nibbles(codes: torch.Tensor) -> list:
    """Codes of one row in element order (element 2j = low nibble of byte j)."""
    return torch.stack((codes & 0xF, codes >> 4), dim=-1).flatten().tolist()


class TestQuantiser:
    def test_ties_saturation_sign_and_nibble_order(self):
        # block 0: amax 6 -> X = 0; the seven ties, then in-grid values
        vals = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, -0.75, -3.0, -6.0, 0.5]
        want = [0, 2, 2, 4, 4, 6, 6, 7, 8 + 2, 8 + 5, 8 + 7, 1]
        w = torch.zeros(2, 64)
        w[0, :len(vals)] = torch.tensor(vals)
        # block 1: amax 7 * 2^-3 -> X = floor(log2(.875)) - 2 = -3; 7 saturates to 6
        w[0, 32:36] = torch.tensor([7.0, -7.0, 1.0, 0.0]) * 2.0 ** -3
        # row 1: an all-zero block, then amax 2^10 -> X = 8, 2^10 / 2^8 = 4
        w[1, 32] = -(2.0 ** 10)
        codes, scales = torch_ref.quant_mxfp4_weight(w)
        assert codes.dtype == torch.uint8 and codes.shape == (2, 32)
        assert scales.dtype == torch.uint8 and scales.shape == (2, 2)
        assert scales.tolist() == [[127, 124], [0, 135]]
        row0, row1 = _nibbles(codes[0]), _nibbles(codes[1])
        assert row0[:len(vals)] == want and set(row0[len(vals):32]) == {0}
        assert row0[32:36] == [7, 8 + 7, 2, 0]
        assert set(row1[:32]) == {0} and row1[32] == 8 + 6
        assert codes[0, 0].item() == (2 << 4) | 0  # element 0 low, element 1 high
        deq = torch_ref.dequant_mxfp4_weight(codes, scales)
        assert deq[0, :8].tolist() == [0, 1, 1, 2, 2, 4, 4, 6]
        assert deq[0, 32:35].tolist() == [0.75, -0.75, 0.125] and deq[1, 32] == -1024

    def test_grid_values_round_trip_exactly(self):
        g = torch.Generator().manual_seed(0)
        codes = torch.randint(0, 256, (48, 128), dtype=torch.uint8, generator=g)
        codes[:, ::16] |= 0x07  # every block holds a 6: its scale is the block's X
        scales = torch.randint(100, 150, (48, 8), dtype=torch.uint8, generator=g)
        w = torch_ref.dequant_mxfp4_weight(codes, scales)
        c2, s2 = torch_ref.quant_mxfp4_weight(w)
        assert torch.equal(s2, scales)
        assert torch.equal(torch_ref.dequant_mxfp4_weight(c2, s2), w)
        # only the sign of a zero may differ between the codes
        assert torch.equal(c2 & 0x77, codes & 0x77)

    def test_linear_is_the_dequantised_product(self):
        g = torch.Generator().manual_seed(1)
        a_q, a_s = torch_ref.quant_fp8_rows(torch.randn(5, 128, generator=g))
        w = torch.randn(32, 128, generator=g)
        packed = ops.mxfp4_pack_weight(*torch_ref.quant_mxfp4_weight(w))
        bias = torch.randn(32, generator=g)
        wd = torch_ref.dequant_mxfp4_weight(*packed)
        assert 0 < ((wd - w).norm() / w.norm()).item() < 0.2
        want = (a_q.float() * a_s[:, None]) @ wd.t() + bias
        assert torch.equal(ops.mxfp4_linear(a_q, a_s, packed, bias), want)
        assert ops.mxfp4_supported(128, 32) and not ops.mxfp4_supported(64, 32)
        assert not ops.mxfp4_supported(3696, 8192) and not ops.mxfp4_supported(128, 24)


def _engine(quantization):
    return LLMEngine(EngineConfig(
        model="tiny-llama", device="cpu", enforce_eager=True, load_weights=False,
        max_num_seqs=2, max_model_len=128, num_kv_blocks=64, quantization=quantization))


class TestEngine:
    def test_generates_and_differs_from_unquantised(self):
        """tiny-llama: o (K=256) and down (K=128) are MXFP4, qkv and gate_up
        (K=64) fall back to fp8. Measured e_quant = 0.096 (profiles/mxfp4_weights.md)."""
        eng = _engine("mxfp4")
        lw = eng.model.layers[0]
        assert lw.o.dtype == lw.down.dtype == lw.o_scale.dtype == torch.uint8
        assert lw.qkv.dtype == lw.gate_up.dtype == torch.float8_e4m3fn
        assert lw.o.shape == (64, 128) and lw.o_scale.shape == (64, 8)
        plain = _engine("none")
        assert eng.model.weight_bytes() < plain.model.weight_bytes()
        params = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
        toks = {}
        eng.add_request("r", prompt="hello world test", params=params)
        while eng.has_unfinished():
            for out in eng.step():
                toks.setdefault(out.request_id, []).extend(out.new_token_ids)
        assert len(toks["r"]) == 6

        ids = torch.tensor(eng.tokenizer.encode("abcdefgh" * 6))
        logits = []
        for e in (eng, plain):
            bs = e.config.kv_block_size
            blocks = e.allocator.allocate(len(ids) // bs + 1)
            slots = [blocks[p // bs] * bs + p % bs for p in range(len(ids))]
            meta = PrefillMeta(cu_seqlens=torch.tensor([0, len(ids)], dtype=torch.int32),
                               max_seqlen=len(ids), slot_mapping=torch.tensor(slots))
            h = e.model.forward(ids, torch.arange(len(ids)), e.kv_cache, meta)
            logits.append(e.model.compute_logits(h[-1:]).float())
        e_quant = ((logits[0] - logits[1]).norm() / logits[1].norm()).item()
        print(f"tiny-llama mxfp4 e_quant = {e_quant:.4f}")
        assert e_quant > 0


class TestSwitch:
    def test_engine_config(self):
        cuda = torch.device("cuda")
        assert EngineConfig(quantization="mxfp4").resolve_quantization(CPU) == "mxfp4"
        assert EngineConfig(quantization="mxfp4").resolve_quantization(cuda) == "mxfp4"
        with pytest.raises(ValueError, match="bf16"):
            EngineConfig(quantization="mxfp4", dtype="float16").resolve_quantization(cuda)

    def test_env_stage_config_and_cli_reach_engine_config(self, monkeypatch):
        from click.testing import CliRunner

        import llmq_amd.cli.worker as cli_worker
        from llmq_amd.cli.main import cli
        from llmq_amd.core.config import Config
        from llmq_amd.workers.engine_worker import EngineWorker

        w = EngineWorker("q", model="tiny-llama", config=Config(),
                         stage_config={"quantization": "mxfp4"})
        assert EngineConfig(**w._engine_kwargs(2)).quantization == "mxfp4"
        seen = {}
        monkeypatch.setattr(cli_worker, "run_engine_worker",
                            lambda *a, **kw: seen.update(kw))
        res = CliRunner().invoke(
            cli, ["worker", "run", "tiny-llama", "q", "--quantization", "mxfp4"])
        assert res.exit_code == 0, res.output
        w = EngineWorker("q", model="tiny-llama", config=Config(),
                         engine_overrides=seen["engine_overrides"])
        assert EngineConfig(**w._engine_kwargs(1)).quantization == "mxfp4"
        monkeypatch.setenv("LLMQ_QUANTIZATION", "mxfp4")
        w = EngineWorker("q", model="tiny-llama", config=Config())
        assert EngineConfig(**w._engine_kwargs(1)).quantization == "mxfp4"
