"""GPU numerics tests: every CDNA4 HIP kernel vs the plain-PyTorch fp32
reference (llmq_amd.ops.torch_ref). Run with `pytest -m gpu` on an MI355X.
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


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def assert_close_to_f32_ref(hip_out: torch.Tensor, ref_f32: torch.Tensor, atol, rtol):
    torch.testing.assert_close(hip_out.float(), ref_f32.float(), atol=atol, rtol=rtol)


TOL = {torch.float32: (1e-5, 1e-5), torch.bfloat16: (2e-2, 2e-2)}


class TestRMSNorm:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("hidden", [64, 3584, 8192])
    @pytest.mark.parametrize("offset", [0.0, 1.0])
    def test_rmsnorm(self, dtype, hidden, offset):
        x = torch.randn(129, hidden, device=DEV, dtype=dtype)
        w = torch.randn(hidden, device=DEV, dtype=dtype)
        out = ops.rmsnorm(x, w, 1e-6, offset)
        ref = torch_ref.rmsnorm(x.float().cpu(), w.float().cpu(), 1e-6, offset)
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(out.cpu(), ref, atol, rtol)

    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    def test_fused_add_rmsnorm(self, dtype):
        hidden = 2048
        x = torch.randn(65, hidden, device=DEV, dtype=dtype)
        res = torch.randn(65, hidden, device=DEV, dtype=dtype)
        w = torch.randn(hidden, device=DEV, dtype=dtype)
        ref_out, ref_res = torch_ref.fused_add_rmsnorm(
            x.clone().cpu(), res.clone().cpu(), w.cpu(), 1e-5
        )
        out, new_res = ops.fused_add_rmsnorm(x, res, w, 1e-5)
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(new_res.cpu(), ref_res.float(), atol, rtol)
        assert_close_to_f32_ref(out.cpu(), ref_out.float(), atol, rtol)


class TestActivations:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("d", [128, 8960, 14336])
    def test_silu_and_mul(self, dtype, d):
        x = torch.randn(33, 2 * d, device=DEV, dtype=dtype)
        out = ops.silu_and_mul(x)
        ref = torch_ref.silu_and_mul(x.float().cpu())
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(out.cpu(), ref, atol, rtol)

    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    def test_gelu_tanh_and_mul(self, dtype):
        d = 14336
        x = torch.randn(17, 2 * d, device=DEV, dtype=dtype)
        out = ops.gelu_tanh_and_mul(x)
        ref = torch_ref.gelu_tanh_and_mul(x.float().cpu())
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(out.cpu(), ref, atol, rtol)


class TestRoPE:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("head_dim", [64, 128, 256])
    def test_rope_matches_ref(self, dtype, head_dim):
        T, HQ, HK = 37, 8, 2
        cos_sin = torch_ref.build_rope_cache(512, head_dim, 500000.0, DEV)
        # q/k as non-contiguous views of a packed qkv row (the real call site)
        qkv = torch.randn(T, (HQ + 2 * HK) * head_dim, device=DEV, dtype=dtype)
        q = qkv[:, : HQ * head_dim].view(T, HQ, head_dim)
        k = qkv[:, HQ * head_dim : (HQ + HK) * head_dim].view(T, HK, head_dim)
        pos = torch.randint(0, 512, (T,), device=DEV)
        q_ref = q.float().cpu().clone()
        k_ref = k.float().cpu().clone()
        torch_ref.rope_inplace(q_ref, k_ref, pos.cpu(), cos_sin.cpu())
        ops.rope_inplace(q, k, pos, cos_sin)
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(q.cpu(), q_ref, atol, rtol)
        assert_close_to_f32_ref(k.cpu(), k_ref, atol, rtol)


class TestKVCache:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    def test_reshape_and_cache_exact(self, dtype):
        T, KVH, D, BS, NB = 50, 4, 128, 16, 8
        qkv = torch.randn(T, 2 * KVH * D, device=DEV, dtype=dtype)
        k = qkv[:, : KVH * D].view(T, KVH, D)
        v = qkv[:, KVH * D :].view(T, KVH, D)
        kc = torch.zeros(NB, KVH, BS, D, device=DEV, dtype=dtype)
        vc = torch.zeros_like(kc)
        slots = torch.randperm(NB * BS, device=DEV)[:T]
        kc_ref, vc_ref = kc.cpu().clone(), vc.cpu().clone()
        torch_ref.reshape_and_cache(k.cpu(), v.cpu(), kc_ref, vc_ref, slots.cpu())
        ops.reshape_and_cache(k, v, kc, vc, slots)
        assert torch.equal(kc.cpu(), kc_ref)  # pure scatter: bitwise
        assert torch.equal(vc.cpu(), vc_ref)


def _build_cache(B, KVH, D, BS, max_ctx, dtype):
    max_blocks = (max_ctx + BS - 1) // BS
    NB = B * max_blocks + 1
    kc = torch.randn(NB, KVH, BS, D, device=DEV, dtype=dtype)
    vc = torch.randn(NB, KVH, BS, D, device=DEV, dtype=dtype)
    bt = torch.zeros(B, max_blocks, dtype=torch.int32, device=DEV)
    perm = torch.randperm(NB - 1) + 1  # block 0 reserved to catch indexing bugs
    i = 0
    for b in range(B):
        for j in range(max_blocks):
            bt[b, j] = perm[i]
            i += 1
    return kc, vc, bt


class TestDecodeAttention:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("G,KVH,D", [(4, 8, 128), (8, 8, 128), (2, 8, 256), (7, 4, 128), (4, 8, 64), (1, 8, 128)])
    def test_vs_ref(self, dtype, G, KVH, D):
        B, BS = 9, 16
        H = G * KVH
        torch.manual_seed(1)
        ctx = torch.tensor([1, 5, 16, 17, 63, 64, 65, 200, 333][:B], dtype=torch.int32, device=DEV)
        kc, vc, bt = _build_cache(B, KVH, D, BS, 333, dtype)
        q = torch.randn(B, H, D, device=DEV, dtype=dtype)
        scale = D ** -0.5
        out = ops.paged_decode_attention(q, kc, vc, bt, ctx, scale)
        ref = torch_ref.paged_decode_attention(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), ctx.cpu(), scale
        )
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(out.cpu(), ref, atol, 5 * rtol)

    @pytest.mark.parametrize("G,D", [(12, 128), (16, 256)])
    def test_wide_gqa_group_bf16(self, G, D):
        """G > 8 is only supported by the MFMA decode kernel (padded 16-row
        Q tile); the VALU kernel caps at 8."""
        dtype = torch.bfloat16
        B, KVH, BS = 5, 2, 16
        H = G * KVH
        torch.manual_seed(3)
        ctx = torch.tensor([1, 31, 64, 129, 333], dtype=torch.int32, device=DEV)
        kc, vc, bt = _build_cache(B, KVH, D, BS, 333, dtype)
        q = torch.randn(B, H, D, device=DEV, dtype=dtype)
        scale = D ** -0.5
        out = ops.paged_decode_attention(q, kc, vc, bt, ctx, scale)
        ref = torch_ref.paged_decode_attention(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), ctx.cpu(), scale
        )
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(out.cpu(), ref, atol, 5 * rtol)

    @pytest.mark.parametrize("pipe", ["0", "64", "128"])
    @pytest.mark.parametrize("B,G,KVH,D,softcap,window", [
        (9, 2, 8, 256, 0.0, 0),    # headline gemma2 shape
        (9, 4, 8, 128, 0.0, 0),
        (5, 2, 8, 256, 50.0, 100), # softcap + window (start mid-chunk)
        (2, 16, 1, 256, 0.0, 0),   # TP-rank shape: split-KV z-grid engaged
    ])
    def test_pipe_variants(self, pipe, B, G, KVH, D, softcap, window, monkeypatch):
        """The software-pipelined glds decode kernel (LLMQ_DECODE_PIPE=64/128)
        must match the plain-staged kernel's reference across chunk-boundary
        contexts (tail chunk short/exact/overflowing) and the split-KV path."""
        monkeypatch.setenv("LLMQ_DECODE_PIPE", pipe)
        dtype = torch.bfloat16
        H = G * KVH
        torch.manual_seed(4)
        all_ctx = [1, 63, 64, 65, 127, 128, 129, 200, 1025]
        ctx = torch.tensor(all_ctx[-B:], dtype=torch.int32, device=DEV)
        kc, vc, bt = _build_cache(B, KVH, D, 16, 1025, dtype)
        q = torch.randn(B, H, D, device=DEV, dtype=dtype)
        scale = D ** -0.5
        out = ops.paged_decode_attention(q, kc, vc, bt, ctx, scale, softcap, window)
        ref = torch_ref.paged_decode_attention(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), ctx.cpu(),
            scale, softcap, window,
        )
        assert_close_to_f32_ref(out.cpu(), ref, 2e-2, 1e-1)

    def test_block_table_wider_than_lds_stage(self):
        """A block table wider than the 1024 entries the MFMA kernels stage
        in LDS sends the default dispatch to the plain-staged kernel, whose
        row-0 context (16,400 tokens = 1025 blocks) reads the tail entries
        from global memory."""
        dtype = torch.bfloat16
        B, G, KVH, D, BS = 2, 4, 1, 128, 16
        H = G * KVH
        torch.manual_seed(7)
        ctx = torch.tensor([16400, 100], dtype=torch.int32, device=DEV)
        kc, vc, bt = _build_cache(B, KVH, D, BS, 1030 * BS, dtype)
        assert bt.size(1) == 1030
        q = torch.randn(B, H, D, device=DEV, dtype=dtype)
        scale = D ** -0.5
        out = ops.paged_decode_attention(q, kc, vc, bt, ctx, scale)
        ref = torch_ref.paged_decode_attention(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), ctx.cpu(), scale
        )
        assert_close_to_f32_ref(out.cpu(), ref, 2e-2, 1e-1)

    @pytest.mark.parametrize("softcap,window", [(50.0, 0), (0.0, 64), (50.0, 64)])
    def test_softcap_window(self, softcap, window):
        dtype = torch.bfloat16
        B, G, KVH, D, BS = 5, 2, 8, 256, 16
        H = G * KVH
        torch.manual_seed(2)
        ctx = torch.tensor([3, 63, 64, 100, 180], dtype=torch.int32, device=DEV)
        kc, vc, bt = _build_cache(B, KVH, D, BS, 180, dtype)
        q = torch.randn(B, H, D, device=DEV, dtype=dtype)
        scale = 1.0 / 16.0
        out = ops.paged_decode_attention(q, kc, vc, bt, ctx, scale, softcap, window)
        ref = torch_ref.paged_decode_attention(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), ctx.cpu(),
            scale, softcap, window,
        )
        assert_close_to_f32_ref(out.cpu(), ref, 2e-2, 1e-1)


class TestPrefillAttention:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("H,KVH,D", [(8, 2, 128), (16, 8, 256), (4, 4, 64)])
    def test_vs_ref(self, dtype, H, KVH, D):
        torch.manual_seed(3)
        lens = [1, 7, 64, 65, 190]
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
        T = sum(lens)
        q = torch.randn(T, H, D, device=DEV, dtype=dtype)
        k = torch.randn(T, KVH, D, device=DEV, dtype=dtype)
        v = torch.randn(T, KVH, D, device=DEV, dtype=dtype)
        scale = D ** -0.5
        out = ops.varlen_prefill_attention(q, k, v, cu, max(lens), scale)
        ref = torch_ref.varlen_prefill_attention(
            q.float().cpu(), k.float().cpu(), v.float().cpu(), cu.cpu(), scale
        )
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(out.cpu(), ref, atol * 2, 5 * rtol)

    def test_defer_max_forced_rescale(self):
        """Forces the defer-max (T13) branch BOTH ways (guide rule 26).

        Early K rows are tiny, so every tile's max drifts < THR and the
        kernel takes the defer path (no O-rescale) for ~11 tiles; key 700
        is a spiked row aligned with late queries, so the tile containing
        it jumps the running max far past THR and the rescale path must
        fire late in the loop. Causality means q-rows < 700 exercise
        defer-only while rows >= 700 exercise the late rescale.
        """
        dtype = torch.bfloat16
        H, KVH, D = 8, 2, 128
        torch.manual_seed(11)
        L = 740
        cu = torch.tensor([0, L], dtype=torch.int32, device=DEV)
        q = torch.randn(L, H, D, device=DEV, dtype=dtype)
        k = torch.randn(L, KVH, D, device=DEV, dtype=dtype) * 0.05
        v = torch.randn(L, KVH, D, device=DEV, dtype=dtype)
        k[700] = (q[L - 1, :KVH].float() * 6.0).to(dtype)
        out = ops.varlen_prefill_attention(q, k, v, cu, L, D ** -0.5)
        ref = torch_ref.varlen_prefill_attention(
            q.float().cpu(), k.float().cpu(), v.float().cpu(), cu.cpu(), D ** -0.5
        )
        assert_close_to_f32_ref(out.cpu(), ref, 2e-2, 1e-1)

    def test_softcap_window(self):
        dtype = torch.bfloat16
        H, KVH, D = 8, 4, 128
        torch.manual_seed(4)
        lens = [33, 129]
        cu = torch.tensor([0, 33, 162], dtype=torch.int32, device=DEV)
        T = sum(lens)
        q = torch.randn(T, H, D, device=DEV, dtype=dtype)
        k = torch.randn(T, KVH, D, device=DEV, dtype=dtype)
        v = torch.randn(T, KVH, D, device=DEV, dtype=dtype)
        out = ops.varlen_prefill_attention(q, k, v, cu, 129, 0.1, 30.0, 64)
        ref = torch_ref.varlen_prefill_attention(
            q.float().cpu(), k.float().cpu(), v.float().cpu(), cu.cpu(), 0.1, 30.0, 64
        )
        assert_close_to_f32_ref(out.cpu(), ref, 2e-2, 1e-1)


class TestEngineGPU:
    def test_engine_generates_and_graphs_match_eager(self):
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        prompts = ["hello world", "the quick brown fox", "MI355X"]
        params = SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True)

        def run(eager: bool):
            eng = LLMEngine(EngineConfig(
                model="llama-3.2-1b", max_num_seqs=4, max_model_len=256,
                load_weights=False, enforce_eager=eager, num_kv_blocks=512,
            ))
            tokens = {}
            for i, p in enumerate(prompts):
                eng.add_request(f"r{i}", prompt=p, params=params)
            while eng.has_unfinished():
                for out in eng.step():
                    tokens.setdefault(out.request_id, []).extend(out.new_token_ids)
            del eng
            torch.cuda.empty_cache()
            return [tokens[f"r{i}"] for i in range(len(prompts))]

        eager_out = run(True)
        graph_out = run(False)
        vocab = 128256
        for toks in eager_out + graph_out:
            assert len(toks) == 16
            assert all(0 <= t < vocab for t in toks)
            # random-weight greedy output must not be a degenerate all-zero
            # stream (the NaN signature: argmax of NaN logits returns 0)
            assert toks.count(0) < 16
        # Each mode must be deterministic run-to-run. (Eager and graph can
        # legitimately diverge after a few tokens: the graph pads the batch
        # to its bucket size, and hipBLASLt GEMMs at different M round bf16
        # differently — with random weights near-tie argmax flips amplify.)
        assert run(True) == eager_out
        assert run(False) == graph_out
        # First sampled token comes from the SAME prefill path in both modes.
        for e, g in zip(eager_out, graph_out):
            assert e[0] == g[0]


class TestFusedSampler:
    def _run(self, logits, temps, seed=7, step=3, req_seeds=None, req_pos=None):
        B = logits.shape[0]
        out = torch.empty(B, dtype=torch.int64, device=DEV)
        keys = torch.empty(B, dtype=torch.int64, device=DEV)
        if req_seeds is None:
            req_seeds = torch.zeros(B, dtype=torch.int32, device=DEV)
        if req_pos is None:
            req_pos = torch.zeros(B, dtype=torch.int32, device=DEV)
        ops.sample_gumbel_argmax(out, keys, logits, temps, req_seeds, req_pos,
                                 seed, step)
        return out

    def test_greedy_matches_argmax(self):
        torch.manual_seed(0)
        logits = torch.randn(16, 50000, device=DEV, dtype=torch.float32)
        temps = torch.zeros(16, device=DEV)
        out = self._run(logits, temps)
        assert torch.equal(out, logits.argmax(dim=-1))

    def test_topk_topp_bound_matches_exact_sort(self):
        """The histogram-select keep-bound must reproduce the exact
        (sort-based) nucleus/top-k keep set up to the documented sub-bin
        overshoot: every exactly-kept id passes the bound, and the bound
        admits at most a sliver of extra probability mass."""
        torch.manual_seed(3)
        B, V = 32, 50000
        logits = (torch.randn(B, V, device=DEV) * 3.0).float()
        temps = torch.full((B,), 0.8, device=DEV)
        tps = torch.tensor([0.3, 0.7, 0.9, 0.95] * (B // 4), device=DEV)
        tks = torch.tensor([0, 5, 100, 0] * (B // 4), dtype=torch.int64, device=DEV)
        bound = ops.topk_topp_bound(logits, temps, tps, tks)
        scaled = logits / temps.unsqueeze(1)
        probs = torch.softmax(scaled, dim=-1)
        sorted_p, sorted_i = torch.sort(probs, dim=-1, descending=True)
        cum = torch.cumsum(sorted_p, dim=-1)
        for b in range(B):
            keep_p = (cum[b] - sorted_p[b]) < tps[b]
            if tks[b] > 0:
                keep_k = torch.arange(V, device=DEV) < tks[b]
                keep = keep_p & keep_k
            else:
                keep = keep_p
            keep[0] = True
            exact_ids = sorted_i[b][keep]
            passed = logits[b] >= bound[b]
            # every exactly-kept id passes the bound
            assert bool(passed[exact_ids].all()), f"row {b} drops exact ids"
            # overshoot bounded: extra admitted mass < 1% of the target
            extra = probs[b][passed].sum() - probs[b][exact_ids].sum()
            assert float(extra) < 0.01, f"row {b} overshoot {float(extra)}"

    def test_topk1_is_argmax_topk5_stays_in_set(self):
        torch.manual_seed(4)
        B, V = 8, 8192
        logits = torch.randn(B, V, device=DEV).float()
        temps = torch.full((B,), 1.0, device=DEV)
        out = torch.empty(B, dtype=torch.int64, device=DEV)
        keys = torch.empty(B, dtype=torch.int64, device=DEV)
        zs = torch.zeros(B, dtype=torch.int32, device=DEV)
        # top_k=1 → only the argmax can ever be drawn
        b1 = ops.topk_topp_bound(logits, temps, torch.ones(B, device=DEV),
                                 torch.ones(B, dtype=torch.int64, device=DEV))
        for step in range(20):
            ops.sample_gumbel_argmax(out, keys, logits, temps, zs, zs, 11, step, b1)
            assert torch.equal(out, logits.argmax(dim=-1)), step
        # top_k=5 → draws stay inside the top-5 set; all 5 seen eventually
        top5 = logits.topk(5, dim=-1).indices
        b5 = ops.topk_topp_bound(logits, temps, torch.ones(B, device=DEV),
                                 torch.full((B,), 5, dtype=torch.int64, device=DEV))
        seen = [set() for _ in range(B)]
        for step in range(400):
            ops.sample_gumbel_argmax(out, keys, logits, temps, zs, zs, 11, step, b5)
            o = out.cpu()
            for b in range(B):
                assert int(o[b]) in set(top5[b].cpu().tolist()), (b, int(o[b]))
                seen[b].add(int(o[b]))
        assert all(len(s2) >= 3 for s2 in seen)  # not stuck on one token

    def test_topp_distribution_matches_truncated_softmax(self):
        """Gumbel-max over the bound-truncated set == renormalised nucleus
        distribution (statistical check on a small crafted vocab)."""
        V = 1024
        base = torch.full((V,), -8.0, device=DEV)
        base[:4] = torch.tensor([3.0, 2.5, 2.0, 1.0], device=DEV)
        B = 512  # draw many rows at once (rows are independent RNG streams)
        logits = base.expand(B, V).contiguous().float()
        temps = torch.ones(B, device=DEV)
        tps = torch.full((B,), 0.8, device=DEV)
        tks = torch.zeros(B, dtype=torch.int64, device=DEV)
        bound = ops.topk_topp_bound(logits, temps, tps, tks)
        out = torch.empty(B, dtype=torch.int64, device=DEV)
        keys = torch.empty(B, dtype=torch.int64, device=DEV)
        zs = torch.zeros(B, dtype=torch.int32, device=DEV)
        counts = torch.zeros(V)
        iters = 40
        for step in range(iters):
            ops.sample_gumbel_argmax(out, keys, logits, temps, zs, zs, 5, step, bound)
            counts += torch.bincount(out.cpu(), minlength=V)
        # exact nucleus at p=0.8 keeps ids {0,1,2} (cum-before .47/.76/.93)
        probs = torch.softmax(base, dim=-1)
        keep = [0, 1, 2]
        assert counts[3:].sum() == 0, counts[:8]
        trunc = probs[keep] / probs[keep].sum()
        freq = counts[keep] / counts.sum()
        assert torch.allclose(freq, trunc.cpu(), atol=0.02), (freq, trunc)

    def test_deterministic_per_step(self):
        torch.manual_seed(0)
        logits = torch.randn(8, 4096, device=DEV)
        temps = torch.full((8,), 0.7, device=DEV)
        a = self._run(logits, temps, seed=1, step=5)
        b = self._run(logits, temps, seed=1, step=5)
        c = self._run(logits, temps, seed=1, step=6)
        assert torch.equal(a, b)
        assert not torch.equal(a, c)  # different step → different draws

    def test_request_seed_reproducible_and_position_keyed(self):
        """Rows with a request seed draw from (seed, position): identical
        across engine steps and batch rows; rows differ by position."""
        torch.manual_seed(0)
        logits = torch.randn(4, 4096, device=DEV)
        same_logits = logits[0:1].expand(4, -1).contiguous()
        temps = torch.full((4,), 0.8, device=DEV)
        seeds = torch.full((4,), 99, dtype=torch.int32, device=DEV)
        pos0 = torch.zeros(4, dtype=torch.int32, device=DEV)
        a = self._run(same_logits, temps, seed=1, step=5, req_seeds=seeds, req_pos=pos0)
        b = self._run(same_logits, temps, seed=2, step=9, req_seeds=seeds, req_pos=pos0)
        assert torch.equal(a, b)  # engine step/seed irrelevant for seeded rows
        assert (a == a[0]).all()  # batch row irrelevant
        pos1 = torch.ones(4, dtype=torch.int32, device=DEV)
        c = self._run(same_logits, temps, seed=1, step=5, req_seeds=seeds, req_pos=pos1)
        assert not torch.equal(a, c)  # position advances the stream

    def test_distribution_matches_softmax(self):
        """Gumbel-max sampling must match the softmax distribution."""
        torch.manual_seed(0)
        V = 8
        logits_row = torch.tensor([2.0, 1.0, 0.0, -1.0, 3.0, 0.5, -2.0, 1.5],
                                  device=DEV)
        temp = 0.8
        N = 20000
        logits = logits_row.expand(N, V).contiguous()
        temps = torch.full((N,), temp, device=DEV)
        out = self._run(logits, temps, seed=123, step=1)
        counts = torch.bincount(out.cpu(), minlength=V).float()
        expected = torch.softmax(logits_row.cpu() / temp, dim=-1) * N
        # chi-square-ish check: every bucket within 5 sigma
        sigma = (expected.clamp_min(1.0)).sqrt()
        assert ((counts - expected).abs() < 5 * sigma + 10).all(), (
            counts, expected)


class TestFusedNormSandwich:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    def test_norm_add_norm(self, dtype):
        hidden = 3584
        x = torch.randn(65, hidden, device=DEV, dtype=dtype)
        res = torch.randn(65, hidden, device=DEV, dtype=dtype)
        w1 = torch.randn(hidden, device=DEV, dtype=dtype)
        w2 = torch.randn(hidden, device=DEV, dtype=dtype)
        ref_out, ref_res = torch_ref.norm_add_norm(
            x.float().cpu(), res.float().cpu(), w1.float().cpu(),
            w2.float().cpu(), 1e-6, 1.0,
        )
        out, new_res = ops.norm_add_norm(x, res, w1, w2, 1e-6, 1.0)
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(new_res.cpu(), ref_res, atol, 2 * rtol)
        assert_close_to_f32_ref(out.cpu(), ref_out, 2 * atol, 4 * rtol)


class TestFusedRopeCache:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("head_dim", [128, 256])
    def test_matches_separate_ops(self, dtype, head_dim):
        T, HQ, HK, BS, NB = 37, 8, 2, 16, 8
        cos_sin = torch_ref.build_rope_cache(512, head_dim, 500000.0, DEV)
        qkv = torch.randn(T, (HQ + 2 * HK) * head_dim, device=DEV, dtype=dtype)
        q = qkv[:, : HQ * head_dim].view(T, HQ, head_dim)
        k = qkv[:, HQ * head_dim : (HQ + HK) * head_dim].view(T, HK, head_dim)
        v = qkv[:, (HQ + HK) * head_dim :].view(T, HK, head_dim)
        pos = torch.randint(0, 512, (T,), device=DEV)
        slots = torch.randperm(NB * BS, device=DEV)[:T]
        kc = torch.zeros(NB, HK, BS, head_dim, device=DEV, dtype=dtype)
        vc = torch.zeros_like(kc)
        # reference: separate ops on fp32 CPU copies
        q_ref, k_ref = q.float().cpu().clone(), k.float().cpu().clone()
        kc_ref = kc.float().cpu().clone()
        vc_ref = vc.float().cpu().clone()
        torch_ref.rope_inplace(q_ref, k_ref, pos.cpu(), cos_sin.cpu())
        torch_ref.reshape_and_cache(k_ref, v.float().cpu(), kc_ref, vc_ref, slots.cpu())
        ops.rope_and_cache(q, k, v, kc, vc, pos, cos_sin, slots)
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(q.cpu(), q_ref, atol, rtol)
        assert_close_to_f32_ref(k.cpu(), k_ref, atol, rtol)
        assert_close_to_f32_ref(kc.cpu(), kc_ref, atol, rtol)
        assert torch.equal(vc.cpu().float(), vc_ref)  # pure copy: bitwise


class TestMixedOverlapGPU:
    def test_overlapped_mixed_step_matches_sequential(self, monkeypatch):
        """The split mixed step runs decode (hipGraph, side stream) and
        prefill (default stream) CONCURRENTLY; tokens must be identical to
        the sequential split (same kernels, same counter-based RNG)."""
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        def run(overlap: str):
            monkeypatch.setenv("LLMQ_OVERLAP_MIXED", overlap)
            eng = LLMEngine(EngineConfig(
                model="llama-3.2-1b", max_num_seqs=8, max_model_len=256,
                load_weights=False, num_kv_blocks=512, seed=7,
            ))
            params = SamplingParams(temperature=0.7, max_tokens=24, ignore_eos=True)
            tokens = {}
            for i in range(4):
                eng.add_request(f"a{i}", prompt=f"first wave {i}", params=params)
            # a few decode-only steps, then admit more -> MIXED steps
            for _ in range(6):
                for out in eng.step():
                    tokens.setdefault(out.request_id, []).extend(out.new_token_ids)
            for i in range(4):
                eng.add_request(f"b{i}", prompt=f"second wave {i} arrives later",
                                params=params)
            while eng.has_unfinished():
                for out in eng.step():
                    tokens.setdefault(out.request_id, []).extend(out.new_token_ids)
            del eng
            torch.cuda.empty_cache()
            return tokens

        seq = run("0")
        ovl = run("1")
        assert seq.keys() == ovl.keys()
        for k in seq:
            assert seq[k] == ovl[k], (k, seq[k][:6], ovl[k][:6])


class TestEngineFamiliesGPU:
    """GPU vs CPU engine consistency per model family: the same seeded
    random-init model must sample the same greedy tokens through the HIP
    path (bf16, graphs) as through the fp32 CPU reference path — covers the
    full layer stack (norm sandwich, rope+cache, attention, softcaps,
    sliding window) per family."""

    @pytest.mark.parametrize("model", ["tiny-llama", "tiny-qwen2", "tiny-gemma2"])
    def test_gpu_matches_cpu_reference_tokens(self, model):
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        params = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
        prompts = ["hello world test", "abcdefgh" * 12]  # crosses block bound

        def run(device):
            eng = LLMEngine(EngineConfig(
                model=model, max_num_seqs=2, max_model_len=256,
                load_weights=False, num_kv_blocks=128, device=device,
                enforce_eager=device == "cpu",
            ))
            outs = {}
            for i, p in enumerate(prompts):
                eng.add_request(f"r{i}", prompt=p, params=params)
            while eng.has_unfinished():
                for out in eng.step():
                    outs.setdefault(out.request_id, []).extend(out.new_token_ids)
            del eng
            torch.cuda.empty_cache()
            return [outs[f"r{i}"] for i in range(len(prompts))]

        cpu_tokens = run("cpu")
        gpu_tokens = run("cuda")
        # bf16 vs f32 can diverge once logits are near-ties in a random-init
        # model; require agreement on the first few steps for every prompt.
        for c, g in zip(cpu_tokens, gpu_tokens):
            assert c[:4] == g[:4], (c, g)


class TestFp8KVCache:
    def test_decode_matches_quantized_ref(self):
        """fp8 KV decode vs an fp32 reference computed on the DEQUANTIZED
        cache — isolates kernel correctness from quantization error."""
        B, G, KVH, D, BS = 6, 2, 8, 256, 16
        H = G * KVH
        torch.manual_seed(5)
        ctx = torch.tensor([1, 17, 64, 100, 150, 333], dtype=torch.int32, device=DEV)
        kc8, vc8, bt = None, None, None
        kc, vc, bt = _build_cache(B, KVH, D, BS, 333, torch.bfloat16)
        kc8 = kc.to(torch.float8_e4m3fn)
        vc8 = vc.to(torch.float8_e4m3fn)
        q = torch.randn(B, H, D, device=DEV, dtype=torch.bfloat16)
        scale = D ** -0.5
        out = ops.paged_decode_attention(q, kc8, vc8, bt, ctx, scale)
        ref = torch_ref.paged_decode_attention(
            q.float().cpu(), kc8.float().cpu(), vc8.float().cpu(),
            bt.cpu(), ctx.cpu(), scale,
        )
        assert_close_to_f32_ref(out.cpu(), ref, 2e-2, 1e-1)

    @pytest.mark.parametrize("pipe", ["0", "64"])
    @pytest.mark.parametrize("B,G,KVH,D,softcap,window", [
        (9, 4, 8, 128, 0.0, 0),
        (5, 2, 8, 256, 50.0, 100),  # softcap + window (start mid-chunk)
        (2, 16, 1, 256, 0.0, 0),    # split-KV z-grid engaged
    ])
    def test_pipe_and_plain_variants(self, pipe, B, G, KVH, D, softcap, window,
                                     monkeypatch):
        """fp8 KV through both the fp8 glds pipeline (LLMQ_DECODE_PIPE=64) and
        the plain-staged kernel (=0), at D=128, with softcap/window and on
        the split-KV path, vs the fp32 reference on the DEQUANTIZED cache."""
        monkeypatch.setenv("LLMQ_DECODE_PIPE", pipe)
        H = G * KVH
        torch.manual_seed(6)
        all_ctx = [1, 63, 64, 65, 127, 128, 129, 200, 1025]
        ctx = torch.tensor(all_ctx[-B:], dtype=torch.int32, device=DEV)
        kc, vc, bt = _build_cache(B, KVH, D, 16, 1025, torch.bfloat16)
        kc8 = kc.to(torch.float8_e4m3fn)
        vc8 = vc.to(torch.float8_e4m3fn)
        q = torch.randn(B, H, D, device=DEV, dtype=torch.bfloat16)
        scale = D ** -0.5
        out = ops.paged_decode_attention(q, kc8, vc8, bt, ctx, scale, softcap, window)
        ref = torch_ref.paged_decode_attention(
            q.float().cpu(), kc8.float().cpu(), vc8.float().cpu(),
            bt.cpu(), ctx.cpu(), scale, softcap, window,
        )
        assert_close_to_f32_ref(out.cpu(), ref, 2e-2, 1e-1)

    def test_cache_write_roundtrip(self):
        """rope_and_cache with an fp8 cache: written values must equal the
        bf16-rotated values quantized to e4m3."""
        T, HQ, HK, D, BS, NB = 16, 4, 2, 128, 16, 4
        cos_sin = torch_ref.build_rope_cache(64, D, 10000.0, DEV)
        qkv = torch.randn(T, (HQ + 2 * HK) * D, device=DEV, dtype=torch.bfloat16)
        q = qkv[:, : HQ * D].view(T, HQ, D)
        k = qkv[:, HQ * D : (HQ + HK) * D].view(T, HK, D)
        v = qkv[:, (HQ + HK) * D :].view(T, HK, D)
        pos = torch.randint(0, 64, (T,), device=DEV)
        slots = torch.randperm(NB * BS, device=DEV)[:T]
        kc8 = torch.zeros(NB, HK, BS, D, device=DEV, dtype=torch.float8_e4m3fn)
        vc8 = torch.zeros_like(kc8)
        k_before = k.clone()
        ops.rope_and_cache(q, k, v, kc8, vc8, pos, cos_sin, slots)
        # k was rotated in place (bf16); cache rows must equal fp8(k)
        for t in range(T):
            s = int(slots[t])
            blk, off = s // BS, s % BS
            got_k = kc8[blk, :, off].float()
            want_k = k[t].to(torch.float8_e4m3fn).float()
            assert torch.equal(got_k.cpu(), want_k.cpu())
            got_v = vc8[blk, :, off].float()
            want_v = v[t].to(torch.float8_e4m3fn).float()
            assert torch.equal(got_v.cpu(), want_v.cpu())
        assert not torch.equal(k_before, k)  # rope actually applied

    def test_engine_runs_with_fp8_kv(self):
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        eng = LLMEngine(EngineConfig(
            model="tiny-llama-d128", max_num_seqs=4, max_model_len=256,
            load_weights=False, num_kv_blocks=512, kv_cache_dtype="fp8",
        ))
        outs = eng.generate_batch(
            ["hello", "world"], SamplingParams(temperature=0.0, max_tokens=8,
                                               ignore_eos=True))
        assert len(outs) == 2
        assert eng.kv_cache.k[0].dtype == torch.float8_e4m3fn

    def test_fp8_kv_with_chunked_prefill(self):
        """Long prompt + fp8 cache: the chunk continuation GATHERS past K/V
        from the quantised cache (dequantised via .to(dtype)). A dtype
        reinterpret bug there produces NaN logits → degenerate token-0
        spam; assert the output is sane and matches the bf16-cache engine's
        shape of behaviour (token ids legal, not constant)."""
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        # tiny specs cap max_model_len at 512 positions — keep prompt+output
        # inside that (the original 600-token prompt was silently truncated
        # to 511 and the request length-finished after ONE token).
        eng = LLMEngine(EngineConfig(
            model="tiny-llama-d128", max_num_seqs=2, max_model_len=512,
            load_weights=False, num_kv_blocks=512, kv_cache_dtype="fp8",
            max_prefill_tokens=128,  # forces a 400-token prompt into chunks
        ))
        assert eng.max_model_len == 512
        torch.manual_seed(11)
        ids = torch.randint(0, eng.spec.vocab_size, (400,)).tolist()
        eng.add_request("long", prompt_token_ids=ids,
                        params=SamplingParams(temperature=0.0, max_tokens=12,
                                              ignore_eos=True))
        toks = []
        steps = 0
        while eng.has_unfinished() and steps < 64:
            for out in eng.step():
                toks.extend(out.new_token_ids)
            steps += 1
        assert len(toks) == 12, f"expected 12 decode tokens, got {toks}"
        assert all(0 <= t < eng.spec.vocab_size for t in toks)
        # The dtype-reinterpret bug this guards against produces all-NaN
        # logits, whose argmax is constant token 0. A random-init greedy
        # chain CAN legitimately settle on one (nonzero) token — split-KV
        # atomics make logits run-to-run noisy — so only the NaN signature
        # is asserted.
        assert set(toks) != {0}, f"all-token-0 output (NaN logits?) {toks}"


class TestChunkedPrefillAttention:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    def test_chunk_queries_vs_ref(self, dtype):
        """Q = last Lq rows of an Lk-long context (cu_seqlens_k path)."""
        H, KVH, D = 8, 2, 128
        torch.manual_seed(6)
        q_lens = [16, 33, 1]
        k_lens = [80, 33, 129]  # seq 2 is a pure continuation (Lq=1)
        cu_q = torch.tensor([0, 16, 49, 50], dtype=torch.int32, device=DEV)
        cu_k = torch.tensor([0, 80, 113, 242], dtype=torch.int32, device=DEV)
        Tq, Tk = 50, 242
        q = torch.randn(Tq, H, D, device=DEV, dtype=dtype)
        k = torch.randn(Tk, KVH, D, device=DEV, dtype=dtype)
        v = torch.randn(Tk, KVH, D, device=DEV, dtype=dtype)
        scale = D ** -0.5
        out = ops.varlen_prefill_attention(
            q, k, v, cu_q, max(q_lens), scale, cu_seqlens_k=cu_k
        )
        ref = torch_ref.varlen_prefill_attention(
            q.float().cpu(), k.float().cpu(), v.float().cpu(), cu_q.cpu(),
            scale, cu_seqlens_k=cu_k.cpu(),
        )
        atol, rtol = TOL[dtype]
        assert_close_to_f32_ref(out.cpu(), ref, 2 * atol, 5 * rtol)

    def test_engine_chunked_matches_whole_gpu(self):
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        prompt = "the quick brown fox " * 20  # ~400 byte tokens
        greedy = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)

        def run(budget):
            eng = LLMEngine(EngineConfig(
                model="tiny-llama-d128", max_num_seqs=4, max_model_len=512,
                load_weights=False, num_kv_blocks=256,
                max_prefill_tokens=budget, enforce_eager=True,
            ))
            out = eng.generate_batch([prompt], greedy)[0]
            del eng
            torch.cuda.empty_cache()
            return out

        assert run(4096) == run(96)


class TestPreemptionGPU:
    def test_preemption_under_graphs(self):
        """KV pressure forces evict+recompute while hipGraphs replay decode:
        every sequence must still complete with the right output lengths."""
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        eng = LLMEngine(EngineConfig(
            model="tiny-llama-d128", max_num_seqs=8, max_model_len=192,
            load_weights=False, num_kv_blocks=48,  # tight: 768 tokens total
            enforce_eager=False,
        ))
        params = SamplingParams(temperature=0.0, max_tokens=64, ignore_eos=True)
        prompts = [f"prompt number {i} " * 6 for i in range(8)]
        outs = {}
        for i, p in enumerate(prompts):
            eng.add_request(f"p{i}", prompt=p, params=params)
        guard = 0
        while eng.has_unfinished() and guard < 2000:
            for out in eng.step():
                if out.finished:
                    outs[out.request_id] = out
            guard += 1
        assert guard < 2000
        assert len(outs) == 8
        for o in outs.values():
            assert o.output_tokens == 64
        assert eng.allocator.num_free == eng.allocator.num_blocks


class TestMixedStepGPU:
    def test_tiny_admission_uses_graph_split_path(self):
        """A 1-seq admission riding a running decode batch takes the
        graph-replay + separate-prefill path; outputs must be complete and
        greedy-consistent with a fused-only engine."""
        from llmq_amd.engine.config import EngineConfig
        from llmq_amd.engine.engine import LLMEngine
        from llmq_amd.engine.sampling_params import SamplingParams

        def run(enforce_eager):
            eng = LLMEngine(EngineConfig(
                model="tiny-llama-d128", max_num_seqs=8, max_model_len=256,
                load_weights=False, num_kv_blocks=512,
                enforce_eager=enforce_eager,
            ))
            greedy = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
            for i in range(4):
                eng.add_request(f"a{i}", prompt=f"base {i}", params=greedy)
            eng.step()  # prefill the base batch
            for _ in range(3):
                eng.step()  # decoding
            eng.add_request("late", prompt="xy", params=greedy)  # tiny admission
            outs = {}
            while eng.has_unfinished():
                for out in eng.step():
                    if out.finished:
                        outs[out.request_id] = out.text
            del eng
            torch.cuda.empty_cache()
            return outs

        graphs = run(False)
        eager = run(True)
        assert set(graphs) == set(eager) == {"a0", "a1", "a2", "a3", "late"}
        assert graphs == eager
