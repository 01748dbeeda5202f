"""quantization="fp8" (W8A8) on the CPU reference path: the public switch and
its plumbing, the weight format the loader and random_init produce, sharded
quantisation, and generation through the fake-quant ops."""

from __future__ import annotations

import pytest
import torch

from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.engine import LLMEngine
from llmq_amd.engine.models.llama import LINEARS, CausalLM
from llmq_amd.engine.model_specs import resolve_spec
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.ops import torch_ref

CPU = torch.device("cpu")


def _engine(model="tiny-llama", **kw):
    kw.setdefault("max_num_seqs", 2)
    kw.setdefault("max_model_len", 128)
    kw.setdefault("num_kv_blocks", 64)
    return LLMEngine(EngineConfig(
        model=str(model), device="cpu", enforce_eager=True, load_weights=False, **kw))


def _greedy(engine, prompts, n=8):
    params = SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True)
    for i, p in enumerate(prompts):
        engine.add_request(f"r{i}", prompt=p, params=params)
    outs = {}
    while engine.has_unfinished():
        for out in engine.step():
            outs.setdefault(out.request_id, []).extend(out.new_token_ids)
    return [outs[f"r{i}"] for i in range(len(prompts))]


# ------------------------------------------------------------- the switch --


class TestSwitch:
    def test_default_and_accepted_values(self):
        assert EngineConfig().quantization == "none"
        assert EngineConfig().resolve_quantization(CPU) is None
        assert EngineConfig(quantization="fp8").resolve_quantization(CPU) == "fp8"

    @pytest.mark.parametrize("bad", ["int4", "FP8", "", "fp8_e5m2"])
    def test_unknown_value_raises(self, bad):
        with pytest.raises(ValueError, match="quantization"):
            EngineConfig(quantization=bad)
        cfg = EngineConfig()
        cfg.quantization = bad  # set after construction: caught when resolved
        with pytest.raises(ValueError, match="quantization"):
            cfg.resolve_quantization(CPU)

    @pytest.mark.parametrize("dtype", ["float16", "float32"])
    def test_gpu_needs_bf16(self, dtype):
        cfg = EngineConfig(quantization="fp8", dtype=dtype)
        with pytest.raises(ValueError, match="bf16"):
            cfg.resolve_quantization(torch.device("cuda"))
        assert EngineConfig(quantization="fp8").resolve_quantization(
            torch.device("cuda")) == "fp8"
        # nothing to check when the switch is off
        assert EngineConfig(dtype=dtype).resolve_quantization(torch.device("cuda")) is None

    def test_model_rejects_unknown(self):
        with pytest.raises(ValueError, match="quantization"):
            CausalLM(resolve_spec("tiny-llama"), CPU, torch.float32, quantization="int4")

    def test_env_var_reaches_engine_config(self, monkeypatch):
        from llmq_amd.core.config import Config
        from llmq_amd.workers.engine_worker import EngineWorker

        assert Config().quantization == "none"
        w = EngineWorker("q", model="tiny-llama", config=Config())
        assert "quantization" not in w._engine_kwargs(1)
        monkeypatch.setenv("LLMQ_QUANTIZATION", "fp8")
        w = EngineWorker("q", model="tiny-llama", config=Config())
        assert EngineConfig(**w._engine_kwargs(1)).quantization == "fp8"

    def test_stage_config_reaches_engine_config(self, monkeypatch):
        from llmq_amd.core.config import Config
        from llmq_amd.workers.engine_worker import EngineWorker

        w = EngineWorker("q", model="tiny-llama", config=Config(),
                         stage_config={"model": "tiny-llama", "quantization": "fp8"})
        # the kwargs every TP follower builds its EngineConfig from
        assert EngineConfig(**w._engine_kwargs(2)).quantization == "fp8"
        # a stage's own setting wins over the environment's
        monkeypatch.setenv("LLMQ_QUANTIZATION", "fp8")
        w = EngineWorker("q", model="tiny-llama", config=Config(),
                         stage_config={"quantization": "none"})
        assert EngineConfig(**w._engine_kwargs(1)).quantization == "none"
        w = EngineWorker("q", model="tiny-llama", config=Config(),
                         stage_config={"quantization": "int4"})
        with pytest.raises(ValueError, match="quantization"):
            EngineConfig(**w._engine_kwargs(1))

    def test_cli_flag_reaches_engine_config(self, monkeypatch):
        from click.testing import CliRunner

        import llmq_amd.cli.worker as cli_worker
        from llmq_amd.cli.main import cli
        from llmq_amd.core.config import Config
        from llmq_amd.workers.engine_worker import EngineWorker

        seen = {}
        monkeypatch.setattr(cli_worker, "run_engine_worker",
                            lambda *a, **kw: seen.update(kw))
        res = CliRunner().invoke(
            cli, ["worker", "run", "tiny-llama", "q", "--quantization", "fp8"])
        assert res.exit_code == 0, res.output
        w = EngineWorker("q", model="tiny-llama", config=Config(),
                         engine_overrides=seen["engine_overrides"])
        assert EngineConfig(**w._engine_kwargs(1)).quantization == "fp8"
        seen.clear()
        res = CliRunner().invoke(cli, ["worker", "run", "tiny-llama", "q"])
        assert res.exit_code == 0, res.output
        assert "quantization" not in (seen["engine_overrides"] or {})
        res = CliRunner().invoke(
            cli, ["worker", "run", "tiny-llama", "q", "--quantization", "int4"])
        assert res.exit_code != 0

    def test_prequantised_checkpoint_rejected(self, tmp_path):
        import json

        (tmp_path / "config.json").write_text(json.dumps({
            "architectures": ["LlamaForCausalLM"], "model_type": "llama",
            "quantization_config": {"quant_method": "fp8"},
            "num_attention_heads": 4, "hidden_size": 64,
        }))
        with pytest.raises(ValueError, match="already quantised"):
            resolve_spec(str(tmp_path))


# ---------------------------------------------------- reference functions --


class TestReference:
    def test_quant_rows_contract(self):
        torch.manual_seed(0)
        x = torch.randn(12, 64) * 10 ** torch.linspace(-6, 4, 12).unsqueeze(1)
        x = x.bfloat16()
        x[3] = 0                       # all-zero row
        x[4] = 0
        x[4, -1] = -3.0                # single (negative) nonzero
        q, scale = torch_ref.quant_fp8_rows(x)
        assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
        qf = q.float()
        assert not qf.isnan().any()
        amax = x.float().abs().amax(dim=1)
        live = amax > 0
        assert (qf.abs().amax(dim=1)[live] == 448).all()
        assert (qf[3] == 0).all() and qf[4, -1] == -448
        # e4m3 keeps 3 mantissa bits: half an ulp is at most 1/16 of the
        # value, and values under 2^-6 * scale round on a fixed grid
        err = (qf * scale.unsqueeze(1) - x.float()).abs()
        assert (err <= (amax / 28).unsqueeze(1)).all()
        assert torch.equal(scale[live], (amax / torch.full_like(amax, 448.0))[live])

    def test_weight_quant_rounds_to_bf16_first(self):
        torch.manual_seed(1)
        w = torch.randn(16, 32) * 0.02
        q32, s32 = torch_ref.quant_fp8_weight(w)
        q16, s16 = torch_ref.quant_fp8_weight(w.bfloat16())
        assert torch.equal(q32.view(torch.uint8), q16.view(torch.uint8))
        assert torch.equal(s32, s16)

    def test_fp8_linear_is_the_dequantised_product(self):
        torch.manual_seed(2)
        a_q, a_s = torch_ref.quant_fp8_rows(torch.randn(5, 64))
        w_q, w_s = torch_ref.quant_fp8_rows(torch.randn(48, 64))
        bias = torch.randn(48)
        ref = (a_q.double() * a_s.double()[:, None]) @ (
            w_q.double() * w_s.double()[:, None]).T + bias.double()
        out = torch_ref.fp8_linear(a_q, a_s, w_q, w_s, bias)
        assert out.dtype == torch.float32
        torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------- weight format --


class TestWeightFormat:
    @pytest.mark.parametrize("model", ["tiny-llama", "tiny-qwen2", "tiny-gemma2"])
    def test_layer_linears_are_fp8_with_channel_scales(self, model):
        spec = resolve_spec(model)
        plain = CausalLM(spec, CPU, torch.float32)
        quant = CausalLM(spec, CPU, torch.float32, quantization="fp8")
        plain.random_init(3)
        quant.random_init(3)
        assert quant.weight_bytes() < plain.weight_bytes()
        named = quant.named_tensors()
        for i, (lq, lp) in enumerate(zip(quant.layers, plain.layers)):
            for name in LINEARS:
                w_q, w_s = getattr(lq, name), getattr(lq, name + "_scale")
                ref = getattr(lp, name)
                assert w_q.dtype == torch.float8_e4m3fn and w_q.shape == ref.shape
                assert w_s.dtype == torch.float32 and w_s.shape == (ref.shape[0],)
                assert named[f"layers.{i}.{name}"] is w_q
                assert named[f"layers.{i}.{name}_scale"] is w_s
                # the bf16 tensor the unquantised model would hold, quantised
                rq, rs = torch_ref.quant_fp8_rows(ref.bfloat16())
                assert torch.equal(w_q.view(torch.uint8), rq.view(torch.uint8))
                assert torch.equal(w_s, rs)
                amax = ref.bfloat16().float().abs().amax(dim=1)
                assert torch.equal(w_s, amax.clamp_min(1e-30) / torch.full_like(amax, 448.0))
            if lq.qkv_bias is not None:
                assert lq.qkv_bias.dtype == torch.float32
            assert lq.input_norm.dtype == torch.float32
        # everything that is not a layer projection is untouched
        assert quant.embedding.dtype == torch.float32
        assert quant.lm_head.dtype == torch.float32
        assert torch.equal(quant.embedding, plain.embedding)
        assert torch.equal(quant.lm_head, plain.lm_head)
        assert torch.equal(quant.final_norm, plain.final_norm)
        expected = plain.weight_bytes() - sum(
            getattr(lw, n).numel() * 3 - getattr(lw, n).shape[0] * 4
            for lw in plain.layers for n in LINEARS)
        assert quant.weight_bytes() == expected

    def test_unquantised_model_reports_no_scales(self):
        m = CausalLM(resolve_spec("tiny-llama"), CPU, torch.float32)
        assert not any(k.endswith("_scale") for k in m.named_tensors())
        assert all(getattr(lw, n + "_scale") is None for lw in m.layers for n in LINEARS)

    def test_tp2_shards_quantised_after_sharding(self, tmp_path):
        """Loading a checkpoint on 2 ranks: every rank's fp8 tensor and scale
        are those of quantising that rank's own bf16 shard, so the row-sharded
        o and down get scales over the local K."""
        from safetensors.torch import save_file

        from llmq_amd.engine.weights import load_safetensors_weights

        spec = resolve_spec("tiny-qwen2")  # has a qkv bias
        h, d = spec.hidden_size, spec.head_dim
        inter = spec.intermediate_size
        g = torch.Generator().manual_seed(4)

        def rnd(*shape):
            # per-row magnitudes differ, so a scale taken over the wrong rows
            # or the whole K cannot match
            t = torch.randn(*shape, generator=g)
            return t * torch.logspace(-2, 0, shape[0]).reshape(-1, *([1] * (len(shape) - 1)))

        ckpt = {"model.embed_tokens.weight": rnd(spec.vocab_size, h),
                "model.norm.weight": rnd(h)}
        if not spec.tied_embeddings:
            ckpt["lm_head.weight"] = rnd(spec.vocab_size, h)
        for i in range(spec.num_layers):
            p = f"model.layers.{i}."
            ckpt[p + "input_layernorm.weight"] = rnd(h)
            ckpt[p + "post_attention_layernorm.weight"] = rnd(h)
            for n, rows in (("q", spec.num_heads * d), ("k", spec.num_kv_heads * d),
                            ("v", spec.num_kv_heads * d)):
                ckpt[p + f"self_attn.{n}_proj.weight"] = rnd(rows, h)
                ckpt[p + f"self_attn.{n}_proj.bias"] = rnd(rows)
            ckpt[p + "self_attn.o_proj.weight"] = rnd(h, spec.num_heads * d) * torch.logspace(
                -1, 1, spec.num_heads * d)
            ckpt[p + "mlp.gate_proj.weight"] = rnd(inter, h)
            ckpt[p + "mlp.up_proj.weight"] = rnd(inter, h)
            ckpt[p + "mlp.down_proj.weight"] = rnd(h, inter) * torch.logspace(-1, 1, inter)
        save_file({k: v.contiguous() for k, v in ckpt.items()},
                  str(tmp_path / "model.safetensors"))

        for rank in range(2):
            plain = CausalLM(spec, CPU, torch.float32, rank, 2)
            quant = CausalLM(spec, CPU, torch.float32, rank, 2, quantization="fp8")
            load_safetensors_weights(plain, tmp_path)
            load_safetensors_weights(quant, tmp_path)
            for lq, lp in zip(quant.layers, plain.layers):
                for name in LINEARS:
                    rq, rs = torch_ref.quant_fp8_rows(getattr(lp, name).bfloat16())
                    assert torch.equal(getattr(lq, name).view(torch.uint8),
                                       rq.view(torch.uint8)), (rank, name)
                    assert torch.equal(getattr(lq, name + "_scale"), rs), (rank, name)
                assert torch.equal(lq.qkv_bias, lp.qkv_bias)
            if rank == 0:
                # down's columns grow with k, so rank 0's local-K scale is
                # not the full-K one: the check above could not pass with
                # quantise-then-shard
                full = ckpt["model.layers.0.mlp.down_proj.weight"].bfloat16()
                _, full_scale = torch_ref.quant_fp8_rows(full)
                assert (quant.layers[0].down_scale < full_scale).all()


# -------------------------------------------------------------- the engine --


class TestEngine:
    PROMPTS = ["hello world test", "abcdefgh" * 12]

    @pytest.mark.parametrize(
        "model", ["tiny-llama", "tiny-qwen2", "tiny-qwen3", "tiny-gemma2"])
    def test_generates(self, model):
        eng = _engine(model, quantization="fp8")
        assert eng.model.fp8
        if model == "tiny-qwen2":
            for lw in eng.model.layers:  # random_init zeroes it: exercise the bias
                lw.qkv_bias.normal_(0.0, 0.5, generator=torch.Generator().manual_seed(5))
        toks = _greedy(eng, self.PROMPTS)
        assert [len(t) for t in toks] == [8, 8]
        vocab = eng.spec.vocab_size
        assert all(0 <= t < vocab for seq in toks for t in seq)
        # deterministic: a second engine repeats it
        eng2 = _engine(model, quantization="fp8")
        if model == "tiny-qwen2":
            for lw in eng2.model.layers:
                lw.qkv_bias.normal_(0.0, 0.5, generator=torch.Generator().manual_seed(5))
        assert _greedy(eng2, self.PROMPTS) == toks

    def test_forward_is_fake_quant_of_the_unquantised_one(self):
        """The fp8 engine's logits are near the unquantised engine's (same
        seed) but not equal to them: the quantised path really ran."""
        from llmq_amd.engine.forward_meta import PrefillMeta

        ids = list(range(3, 40))

        def _prefill_logits(engine):
            bs = engine.config.kv_block_size
            blocks = engine.allocator.allocate((len(ids) + bs - 1) // bs)
            slots = [blocks[p // bs] * bs + p % bs for p in range(len(ids))]
            meta = PrefillMeta(
                cu_seqlens=torch.tensor([0, len(ids)], dtype=torch.int32),
                max_seqlen=len(ids),
                slot_mapping=torch.tensor(slots, dtype=torch.long),
            )
            hidden = engine.model.forward(
                torch.tensor(ids), torch.arange(len(ids)), engine.kv_cache, meta)
            return engine.model.compute_logits(hidden)

        ref = _prefill_logits(_engine("tiny-llama"))
        out = _prefill_logits(_engine("tiny-llama", quantization="fp8"))
        rel = ((out - ref).norm() / ref.norm()).item()
        # two e4m3 operands per product, 2^-4 worst-case each, averaged over
        # K >= 64 terms and a few layers: percent level, never tens of percent
        assert 0.0 < rel < 0.1, rel

    def test_none_is_the_default_path(self):
        base = _engine("tiny-llama")
        named = _engine("tiny-llama", quantization="none")
        assert not base.model.fp8 and not named.model.fp8
        for (ka, a), (kb, b) in zip(base.model.named_tensors().items(),
                                    named.model.named_tensors().items()):
            assert ka == kb and a.dtype == b.dtype and torch.equal(a, b)
        assert _greedy(base, self.PROMPTS) == _greedy(named, self.PROMPTS)
