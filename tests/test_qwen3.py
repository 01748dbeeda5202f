"""Qwen3 support (CPU): per-head q/k RMSNorm before RoPE, no QKV bias,
explicit head_dim.

The anchor is logit and greedy-token parity against transformers'
Qwen3ForCausalLM on a tiny checkpoint whose q_norm/k_norm weights are
overwritten with distinct random values (HF initialises them to ones, which
would hide a q/k swap or a dropped weight). The rest covers the op-level
reference, the spec plumbing, the synthetic preset and the TP=2 sharded load.
"""

from __future__ import annotations

import dataclasses
import json
import os

import pytest
import torch

pytestmark = pytest.mark.integration

transformers = pytest.importorskip("transformers")

# Seed of the tiny checkpoint. Chosen so that at each of the greedy steps
# compared below HF's top-1/top-2 logit gap exceeds the logit parity bound
# (the test checks that itself).
SEED = 0
TOKEN_IDS = [1, 7, 42, 99, 123, 250, 3]


def _save_tiny_qwen3(path, hidden=64, inter=128, heads=4, kv_heads=2,
                     head_dim=32, vocab=300, seed=SEED):
    torch.manual_seed(seed)
    cfg = transformers.Qwen3Config(
        vocab_size=vocab, hidden_size=hidden, intermediate_size=inter,
        num_hidden_layers=2, num_attention_heads=heads,
        num_key_value_heads=kv_heads, head_dim=head_dim,
        max_position_embeddings=256, rope_theta=10000.0, rms_norm_eps=1e-6,
        tie_word_embeddings=False,
    )
    model = transformers.Qwen3ForCausalLM(cfg).eval().float()
    gen = torch.Generator().manual_seed(seed + 1)
    n_norms = 0
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith(("q_norm.weight", "k_norm.weight")):
                prm.copy_(0.5 + torch.rand(prm.shape, generator=gen))
                n_norms += 1
    assert n_norms == 4  # q and k, two layers
    model.save_pretrained(path, safe_serialization=True)
    # minimal tokenizer marker so load_tokenizer falls back to bytes
    (path / "tokenizer_config.json").write_text(json.dumps({}))
    return model


def _cpu_engine(model, **kw):
    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine

    kw.setdefault("max_num_seqs", 2)
    kw.setdefault("max_model_len", 128)
    kw.setdefault("num_kv_blocks", 64)
    return LLMEngine(EngineConfig(
        model=str(model), device="cpu", enforce_eager=True, **kw))


def _prefill_logits(engine, token_ids, n_blocks=1):
    from llmq_amd.engine.forward_meta import PrefillMeta

    dev = engine.device
    blocks = engine.allocator.allocate(n_blocks)
    bs = engine.config.kv_block_size
    slots = [blocks[p // bs] * bs + p % bs for p in range(len(token_ids))]
    meta = PrefillMeta(
        cu_seqlens=torch.tensor([0, len(token_ids)], dtype=torch.int32, device=dev),
        max_seqlen=len(token_ids),
        slot_mapping=torch.tensor(slots, dtype=torch.long, device=dev),
    )
    ids = torch.tensor(token_ids, dtype=torch.long, device=dev)
    pos = torch.arange(len(token_ids), dtype=torch.long, device=dev)
    hidden = engine.model.forward(ids, pos, engine.kv_cache, meta)
    return engine.model.compute_logits(hidden)


def _greedy(engine, token_ids, n):
    from llmq_amd.engine.sampling_params import SamplingParams

    engine.add_request("g", prompt_token_ids=list(token_ids),
                       params=SamplingParams(temperature=0.0, max_tokens=n,
                                             ignore_eos=True))
    toks = []
    while engine.has_unfinished():
        for out in engine.step():
            toks.extend(out.new_token_ids)
    return toks


def test_logits_match_transformers(tmp_path):
    hf = _save_tiny_qwen3(tmp_path)
    engine = _cpu_engine(tmp_path)
    spec = engine.spec
    assert spec.family == "qwen3"
    assert spec.qk_norm
    assert not spec.qkv_bias
    assert spec.head_dim == 32
    assert spec.num_layers == 2
    assert spec.num_heads == 4 and spec.num_kv_heads == 2
    assert spec.sliding_window == 0

    ours = _prefill_logits(engine, TOKEN_IDS)
    with torch.no_grad():
        theirs = hf(torch.tensor([TOKEN_IDS])).logits[0]
    diff = (ours - theirs).abs().max().item()
    ref_scale = theirs.abs().max().item()
    assert diff < 1e-3 * max(1.0, ref_scale), f"logits diverge: {diff}"


def test_greedy_continuation_matches_transformers(tmp_path):
    """Decode reads the normalised-then-rotated k back from the paged cache:
    6 greedy tokens through add_request/step must equal HF's."""
    hf = _save_tiny_qwen3(tmp_path)
    hf_toks, cur = [], list(TOKEN_IDS)
    for _ in range(6):
        with torch.no_grad():
            logits = hf(torch.tensor([cur])).logits[0, -1]
        top2 = logits.topk(2).values
        bound = 1e-3 * max(1.0, logits.abs().max().item())
        # no step may hinge on a near-tie: the gap must exceed the parity
        # bound both sides are held to
        assert (top2[0] - top2[1]).item() > bound, (top2, bound)
        nxt = int(logits.argmax())
        hf_toks.append(nxt)
        cur.append(nxt)
    toks = _greedy(_cpu_engine(tmp_path), TOKEN_IDS, 6)
    assert toks == hf_toks, (toks, hf_toks)


@pytest.mark.parametrize("offset", [0.0, 1.0])
def test_torch_ref_equals_separate_ops_fp32(offset):
    """In fp32 there is no rounding between norm and rotation, so the fused
    reference equals rmsnorm on the head views + rope_inplace +
    reshape_and_cache."""
    from llmq_amd.ops import torch_ref

    torch.manual_seed(3)
    T, HQ, HK, D, BS, NB = 11, 5, 3, 32, 4, 6
    qkv = torch.randn(T, (HQ + 2 * HK) * D)
    q = qkv[:, : HQ * D].view(T, HQ, D)
    k = qkv[:, HQ * D : (HQ + HK) * D].view(T, HK, D)
    v = qkv[:, (HQ + HK) * D :].view(T, HK, D)
    qw, kw = torch.randn(D), torch.randn(D)
    cos_sin = torch_ref.build_rope_cache(64, D, 10000.0, "cpu")
    pos = torch.randint(0, 64, (T,))
    slots = torch.randperm(NB * BS)[:T]
    kc = torch.full((NB, HK, BS, D), -7.0)
    vc = torch.full((NB, HK, BS, D), -7.0)

    q_ref = torch_ref.rmsnorm(q.reshape(-1, D), qw, 1e-6, offset).view(T, HQ, D)
    k_ref = torch_ref.rmsnorm(k.reshape(-1, D), kw, 1e-6, offset).view(T, HK, D)
    torch_ref.rope_inplace(q_ref, k_ref, pos, cos_sin)
    kc_ref, vc_ref = kc.clone(), vc.clone()
    torch_ref.reshape_and_cache(k_ref, v, kc_ref, vc_ref, slots)

    torch_ref.qknorm_rope_and_cache(
        q, k, v, kc, vc, qw, kw, 1e-6, offset, pos, cos_sin, slots)
    torch.testing.assert_close(q, q_ref, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(k, k_ref, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(kc, kc_ref, atol=1e-6, rtol=1e-6)
    assert torch.equal(vc, vc_ref)


def test_torch_ref_skips_pad_rows():
    """slot < 0 rows are normed and rotated but leave both caches alone."""
    from llmq_amd.ops import torch_ref

    torch.manual_seed(4)
    T, H, D, BS, NB = 5, 2, 16, 4, 3
    q, k, v = (torch.randn(T, H, D) for _ in range(3))
    w = torch.ones(D)
    cos_sin = torch_ref.build_rope_cache(16, D, 10000.0, "cpu")
    pos = torch.arange(T)
    slots = torch.tensor([0, -1, 5, -1, 9])
    kc = torch.full((NB, H, BS, D), -7.0)
    vc = torch.full((NB, H, BS, D), -7.0)
    k_in = k.clone()
    torch_ref.qknorm_rope_and_cache(
        q, k, v, kc, vc, w, w, 1e-6, 0.0, pos, cos_sin, slots)
    assert not torch.equal(k[1], k_in[1])  # pad row still transformed
    written = torch.zeros(NB, BS, dtype=torch.bool)
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            written[s // BS, s % BS] = True
            assert torch.equal(kc[s // BS, :, s % BS], k[t])
            assert torch.equal(vc[s // BS, :, s % BS], v[t])
    assert (kc.transpose(1, 2)[~written] == -7.0).all()
    assert (vc.transpose(1, 2)[~written] == -7.0).all()


def _write_config(path, **overrides):
    cfg = {
        "architectures": ["Qwen3ForCausalLM"], "model_type": "qwen3",
        "vocab_size": 300, "hidden_size": 64, "intermediate_size": 128,
        "num_hidden_layers": 2, "num_attention_heads": 4,
        "num_key_value_heads": 2, "head_dim": 32,
    }
    cfg.update(overrides)
    path.mkdir(parents=True, exist_ok=True)
    (path / "config.json").write_text(json.dumps(cfg))
    return path


def test_unsupported_qwen3_variants_raise(tmp_path):
    from llmq_amd.engine.model_specs import spec_from_hf_config

    ok = spec_from_hf_config(_write_config(tmp_path / "ok"), "ok")
    assert ok.family == "qwen3" and ok.qk_norm and not ok.qkv_bias
    biased = spec_from_hf_config(
        _write_config(tmp_path / "b", attention_bias=True), "b")
    assert biased.qkv_bias
    with pytest.raises(ValueError, match="sliding"):
        spec_from_hf_config(
            _write_config(tmp_path / "sw", use_sliding_window=True,
                          sliding_window=64), "sw")
    with pytest.raises(ValueError, match="not supported"):
        spec_from_hf_config(
            _write_config(tmp_path / "moe", model_type="qwen3_moe",
                          architectures=["Qwen3MoeForCausalLM"]), "moe")


def test_presets():
    from llmq_amd.engine.model_specs import PRESETS, resolve_spec

    spec = resolve_spec("Qwen/Qwen3-8B")
    assert spec is PRESETS["qwen3-8b"]
    assert spec.family == "qwen3" and spec.qk_norm and not spec.qkv_bias
    assert spec.head_dim == 128 and spec.num_kv_heads == 8
    assert abs(spec.param_count() - 8.19e9) < 0.01 * 8.19e9
    # the q/k norms are counted: 2 * head_dim per layer
    plain = dataclasses.replace(spec, qk_norm=False)
    assert spec.param_count() - plain.param_count() == 2 * 128 * 36
    for size in ("0.6b", "1.7b", "4b", "8b", "14b", "32b"):
        assert resolve_spec(f"Qwen/Qwen3-{size.upper()}").name == f"qwen3-{size}"
    tiny, base = PRESETS["tiny-qwen3"], PRESETS["tiny-qwen2"]
    assert tiny.qk_norm and not tiny.qkv_bias and tiny.head_dim == 64
    for f in ("vocab_size", "hidden_size", "intermediate_size", "num_layers",
              "num_heads", "num_kv_heads", "tied_embeddings"):
        assert getattr(tiny, f) == getattr(base, f), f


def test_tiny_qwen3_preset_generates_on_cpu():
    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine

    eng = LLMEngine(EngineConfig(
        model="tiny-qwen3", device="cpu", enforce_eager=True,
        load_weights=False, max_num_seqs=2, max_model_len=128,
        num_kv_blocks=64,
    ))
    names = eng.model.named_tensors()
    assert names["layers.0.q_norm"].shape == (64,)
    assert names["layers.1.k_norm"].shape == (64,)
    assert torch.equal(names["layers.0.q_norm"], torch.ones(64))
    toks = _greedy(eng, [1, 5, 9, 200], 8)
    assert len(toks) == 8 and all(0 <= t < 512 for t in toks)


def test_random_init_of_other_families_unchanged():
    """q/k norm weights are filled, not drawn: a qk_norm model's other
    tensors get the values the same model gets without it."""
    from llmq_amd.engine.model_specs import PRESETS
    from llmq_amd.engine.models.llama import CausalLM

    spec = PRESETS["tiny-qwen3"]
    plain = dataclasses.replace(spec, qk_norm=False)
    a = CausalLM(spec, torch.device("cpu"), torch.float32)
    b = CausalLM(plain, torch.device("cpu"), torch.float32)
    a.random_init(seed=11)
    b.random_init(seed=11)
    ta, tb = a.named_tensors(), b.named_tensors()
    assert set(ta) - set(tb) == {f"layers.{i}.{n}" for i in range(2)
                                 for n in ("q_norm", "k_norm")}
    for name, t in tb.items():
        assert torch.equal(ta[name], t), name


# ---- TP=2 over gloo (method of test_tp_numerics.test_tp2_logits_match_unsharded)

TP_TOKEN_IDS = [1, 9, 77, 123, 200, 314, 5, 42]


def _save_tp_checkpoint(path):
    return _save_tiny_qwen3(path, hidden=128, inter=256, heads=8, kv_heads=4,
                            head_dim=16, vocab=320)


def _rank_main(rank, world, ckpt, out_file):
    import torch.distributed as dist

    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine
    from llmq_amd.parallel import init_tp

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29599"
    init_tp(world, rank=rank, backend="gloo")
    engine = LLMEngine(EngineConfig(
        model=ckpt, device="cpu", enforce_eager=True,
        max_num_seqs=2, max_model_len=128, num_kv_blocks=64,
    ), tp_rank=rank, tp_size=world)
    logits = _prefill_logits(engine, TP_TOKEN_IDS, n_blocks=4)
    tokens = _greedy(engine, TP_TOKEN_IDS, 6)
    if rank == 0:
        torch.save({"logits": logits, "decode_tokens": tokens}, out_file)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
@pytest.mark.timeout(300)
def test_tp2_logits_match_unsharded(tmp_path):
    hf = _save_tp_checkpoint(tmp_path)

    import torch.multiprocessing as mp

    out_file = str(tmp_path / "tp_logits.pt")
    mp.spawn(_rank_main, args=(2, str(tmp_path), out_file), nprocs=2, join=True)
    saved = torch.load(out_file)

    solo = _cpu_engine(tmp_path)
    assert solo.spec.qk_norm
    solo_logits = _prefill_logits(solo, TP_TOKEN_IDS, n_blocks=4)
    with torch.no_grad():
        ref = hf(torch.tensor([TP_TOKEN_IDS])).logits[0]
    scale = ref.abs().max().item()
    for name, other in (("unsharded engine", solo_logits), ("transformers", ref)):
        diff = (saved["logits"] - other).abs().max().item()
        assert diff < 1e-3 * max(1.0, scale), f"TP logits vs {name}: {diff}"

    solo_tokens = _greedy(_cpu_engine(tmp_path), TP_TOKEN_IDS, 6)
    assert saved["decode_tokens"] == solo_tokens, (
        saved["decode_tokens"], solo_tokens)
