"""GPU tests for the fused QK-norm + RoPE + cache-write kernel (Qwen3) and
the engine paths that run it. Run with `pytest -m gpu` on an MI355X.
"""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from llmq_amd import ops
    from llmq_amd.ops import torch_ref
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")

TOL = {torch.float32: (1e-5, 1e-5), torch.bfloat16: (2e-2, 2e-2)}

# T is no multiple of the block or group size. HQ + HK = 8 heads are no
# multiple of the 16 heads a block covers per pass, and with HQ = 5 the
# second wave (heads 4..7) straddles the q/k boundary.
T, HQ, HK, BS, NB = 37, 5, 3, 16, 8
PAD_ROWS = [0, 9, 17, 30, 36]
SENTINEL = -3.0  # exact in fp32, bf16 and e4m3


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def _inputs(D, dtype, cache_dtype=None, max_pos=512):
    cos_sin = torch_ref.build_rope_cache(max_pos, D, 1000000.0, DEV)
    qkv = torch.randn(T, (HQ + 2 * HK) * D, device=DEV, dtype=dtype)
    q = qkv[:, : HQ * D].view(T, HQ, D)
    k = qkv[:, HQ * D : (HQ + HK) * D].view(T, HK, D)
    v = qkv[:, (HQ + HK) * D :].view(T, HK, D)
    qw = torch.randn(D, device=DEV, dtype=dtype)
    kw = torch.randn(D, device=DEV, dtype=dtype)
    pos = torch.randint(0, max_pos, (T,), device=DEV)
    slots = torch.randperm(NB * BS, device=DEV)[:T]
    slots[PAD_ROWS] = -1
    cdt = cache_dtype or dtype
    kc = torch.full((NB, HK, BS, D), SENTINEL, device=DEV, dtype=torch.float32).to(cdt)
    vc = kc.clone()
    return q, k, v, qw, kw, pos, slots, cos_sin, kc, vc


def _written_mask(slots):
    """[NB, BS] bool: cache rows addressed by a non-negative slot."""
    mask = torch.zeros(NB, BS, dtype=torch.bool)
    for s in slots.tolist():
        if s >= 0:
            mask[s // BS, s % BS] = True
    return mask


class TestQKNormRopeCache:
    @pytest.mark.parametrize("offset", [0.0, 1.0])
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("D", [64, 128, 256])
    def test_matches_torch_ref(self, D, dtype, offset):
        q, k, v, qw, kw, pos, slots, cos_sin, kc, vc = _inputs(D, dtype)
        # reference on fp32 CPU copies of the (dtype-rounded) inputs
        q_ref, k_ref = q.float().cpu().clone(), k.float().cpu().clone()
        v_ref = v.float().cpu().clone()
        kc_ref, vc_ref = kc.float().cpu().clone(), vc.float().cpu().clone()
        torch_ref.qknorm_rope_and_cache(
            q_ref, k_ref, v_ref, kc_ref, vc_ref, qw.float().cpu(),
            kw.float().cpu(), 1e-6, offset, pos.cpu(), cos_sin.cpu(), slots.cpu())
        q_in, k_in, v_in = q.clone(), k.clone(), v.clone()

        ops.qknorm_rope_and_cache(
            q, k, v, kc, vc, qw, kw, 1e-6, offset, pos, cos_sin, slots)
        torch.cuda.synchronize()

        atol, rtol = TOL[dtype]
        # q and k, pad rows included: normed and rotated like the rest
        torch.testing.assert_close(q.float().cpu(), q_ref, atol=atol, rtol=rtol)
        torch.testing.assert_close(k.float().cpu(), k_ref, atol=atol, rtol=rtol)
        for t in PAD_ROWS:
            assert not torch.equal(q[t], q_in[t])
            assert not torch.equal(k[t], k_in[t])
        assert torch.equal(v, v_in)  # v is only read

        mask = _written_mask(slots.cpu())
        assert int(mask.sum()) == T - len(PAD_ROWS)
        kc_rows = kc.float().cpu().transpose(1, 2)  # [NB, BS, HK, D]
        vc_rows = vc.float().cpu().transpose(1, 2)
        torch.testing.assert_close(
            kc_rows[mask], kc_ref.transpose(1, 2)[mask], atol=atol, rtol=rtol)
        # the cached k is the very value written back in place
        for t, s in enumerate(slots.tolist()):
            if s >= 0:
                assert torch.equal(kc[s // BS, :, s % BS], k[t])
        assert torch.equal(vc_rows[mask], vc_ref.transpose(1, 2)[mask])  # copy
        # nothing else was touched
        assert (kc_rows[~mask] == SENTINEL).all()
        assert (vc_rows[~mask] == SENTINEL).all()

    def test_fp8_cache_roundtrip(self):
        """bf16 inputs, e4m3 cache: written rows are the bf16-rounded rotated
        k (and v) quantized to e4m3, bit for bit."""
        D = 128
        q, k, v, qw, kw, pos, slots, cos_sin, kc8, vc8 = _inputs(
            D, torch.bfloat16, cache_dtype=torch.float8_e4m3fn)
        k_before = k.clone()
        ops.qknorm_rope_and_cache(
            q, k, v, kc8, vc8, qw, kw, 1e-6, 0.0, pos, cos_sin, slots)
        torch.cuda.synchronize()
        for t in range(T):
            s = int(slots[t])
            if s < 0:
                continue
            blk, off = s // BS, s % BS
            got_k = kc8[blk, :, off].float()
            want_k = k[t].to(torch.float8_e4m3fn).float()
            assert torch.equal(got_k.cpu(), want_k.cpu())
            got_v = vc8[blk, :, off].float()
            want_v = v[t].to(torch.float8_e4m3fn).float()
            assert torch.equal(got_v.cpu(), want_v.cpu())
        assert not torch.equal(k_before, k)
        mask = _written_mask(slots.cpu())
        assert (kc8.float().cpu().transpose(1, 2)[~mask] == SENTINEL).all()
        assert (vc8.float().cpu().transpose(1, 2)[~mask] == SENTINEL).all()

    def test_zero_tokens_is_noop(self):
        D = 128
        q, k, v, qw, kw, pos, slots, cos_sin, kc, vc = _inputs(D, torch.bfloat16)
        kc_in, vc_in = kc.clone(), vc.clone()
        ops.qknorm_rope_and_cache(
            q[:0], k[:0], v[:0], kc, vc, qw, kw, 1e-6, 0.0, pos[:0], cos_sin,
            slots[:0])
        torch.cuda.synchronize()
        assert torch.equal(kc, kc_in) and torch.equal(vc, vc_in)

    def test_unsupported_head_dim_composes_kernels(self):
        """D outside {64, 128, 256} takes rmsnorm x2 + rope_and_cache; the
        fused op itself rejects it."""
        D = 32
        q, k, v, qw, kw, pos, slots, cos_sin, kc, vc = _inputs(D, torch.float32)
        q_ref, k_ref = q.cpu().clone(), k.cpu().clone()
        kc_ref, vc_ref = kc.cpu().clone(), vc.cpu().clone()
        torch_ref.qknorm_rope_and_cache(
            q_ref, k_ref, v.cpu(), kc_ref, vc_ref, qw.cpu(), kw.cpu(), 1e-6,
            0.0, pos.cpu(), cos_sin.cpu(), slots.cpu())
        with pytest.raises(RuntimeError, match="head_dim"):
            torch.ops.llmq_amd.qknorm_rope_and_cache(
                q, k, v, kc, vc, qw, kw, 1e-6, 0.0, pos, cos_sin, slots)
        ops.qknorm_rope_and_cache(
            q, k, v, kc, vc, qw, kw, 1e-6, 0.0, pos, cos_sin, slots)
        torch.testing.assert_close(q.cpu(), q_ref, atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(k.cpu(), k_ref, atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(kc.cpu(), kc_ref, atol=1e-5, rtol=1e-5)
        assert torch.equal(vc.cpu(), vc_ref)


def _greedy_tokens(eng, prompts, max_tokens):
    from llmq_amd.engine.sampling_params import SamplingParams

    params = SamplingParams(temperature=0.0, max_tokens=max_tokens, ignore_eos=True)
    outs = {}
    for i, p in enumerate(prompts):
        eng.add_request(f"r{i}", prompt=p, params=params)
    while eng.has_unfinished():
        for out in eng.step():
            outs.setdefault(out.request_id, []).extend(out.new_token_ids)
    return [outs[f"r{i}"] for i in range(len(prompts))]


class TestQwen3EngineGPU:
    PROMPTS = ["hello world test", "abcdefgh" * 12]  # crosses block bound

    def _engine(self, device, eager):
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine

        return LLMEngine(EngineConfig(
            model="tiny-qwen3", max_num_seqs=2, max_model_len=256,
            load_weights=False, num_kv_blocks=128, device=device,
            enforce_eager=eager,
        ))

    def test_gpu_matches_cpu_reference_tokens(self):
        cpu = _greedy_tokens(self._engine("cpu", True), self.PROMPTS, 12)
        eng = self._engine("cuda", False)
        assert eng.spec.qk_norm
        gpu = _greedy_tokens(eng, self.PROMPTS, 12)
        del eng
        torch.cuda.empty_cache()
        # bf16 vs f32 can diverge once logits are near-ties in a random-init
        # model; require agreement on the first few steps for every prompt.
        for c, g in zip(cpu, gpu):
            assert c[:4] == g[:4], (c, g)

    def test_graph_replay_matches_eager(self):
        runs = {}
        for eager in (False, True):
            eng = self._engine("cuda", eager)
            runs[eager] = _greedy_tokens(eng, self.PROMPTS, 12)
            del eng
            torch.cuda.empty_cache()
        assert all(len(t) == 12 for t in runs[True])
        assert runs[False] == runs[True], runs

    def test_real_layout_checkpoint_generates_text(self, tmp_path):
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams
        from llmq_amd.engine.tokenizer import HFTokenizer
        from llmq_amd.utils.tiny_checkpoint import build_tiny_checkpoint

        ckpt = build_tiny_checkpoint(tmp_path / "ck", family="qwen3")
        eng = LLMEngine(EngineConfig(
            model=ckpt, device="cuda:0", load_weights=True,
            max_num_seqs=4, max_model_len=256,
        ))
        assert eng.spec.family == "qwen3" and eng.spec.qk_norm
        assert eng.spec.head_dim == 64
        assert isinstance(eng.tokenizer, HFTokenizer)
        w = eng.model.layers[0].q_norm
        assert not torch.equal(w, torch.ones_like(w))  # loaded, not default
        prompt = eng.tokenizer.apply_chat_template(
            [{"role": "user", "content": "translate the quick brown fox"}])
        outs = eng.generate_batch(
            [prompt], SamplingParams(temperature=0.0, max_tokens=12,
                                     ignore_eos=True))
        assert len(outs) == 1 and outs[0].strip(), f"empty text: {outs!r}"
