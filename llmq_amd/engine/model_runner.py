"""Model runner: batch tensor prep, forward execution, sampling, hipGraphs.

Decode steps are captured as hipGraphs per batch-size bucket (the vLLM
capability the reference relies on, SURVEY §2.9 "CUDA graph capture of
decode" → hipGraph here): all decode inputs live in static device buffers;
a step copies the small int tensors in, replays the graph, and samples from
the static logits buffer. Python/launch overhead per decode step drops to
one replay + one sampler call regardless of model depth.
"""

from __future__ import annotations

import logging
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from llmq_amd import ops
from llmq_amd.engine.config import EngineConfig
from llmq_amd.engine.forward_meta import (
    ChunkGather, DecodeMeta, MixedMeta, PrefillMeta, TorchGatherIndices,
)
from llmq_amd.engine.kv_cache import KVCache, blocks_needed
from llmq_amd.engine.models.llama import CausalLM
from llmq_amd.engine.penalty_table import (
    COUNT_MASK, PROMPT_BIT, PenaltyTable, count_words, wants_penalties,
)
from llmq_amd.ops import torch_ref
from llmq_amd.engine.scheduler import ScheduledBatch, Sequence

logger = logging.getLogger(__name__)

# One packed int32 record per row that asked for logprobs: 1 + MAX_LOGPROBS
# token ids, as many fp32 logprobs (bit patterns), and the rank.
_LP_W = 1 + ops.MAX_LOGPROBS
_LP_PACK = 2 * _LP_W + 1


def _logprob_entries(ids, lp, rank, ks) -> List[tuple]:
    """Per-row (token_id, logprob, rank, [(id, logprob) x k]) from the arrays
    of ops.token_logprobs, each row cut to the k it asked for."""
    ids, lp, rank = ids.tolist(), lp.tolist(), rank.tolist()
    return [
        (ids[j][0], lp[j][0], rank[j],
         list(zip(ids[j][1:1 + k], lp[j][1:1 + k])))
        for j, k in enumerate(ks)
    ]


def _buckets(max_bs: int) -> List[int]:
    sizes = [1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512]
    out = [b for b in sizes if b < max_bs]
    out.append(max_bs)
    return out


class ModelRunner:
    def __init__(
        self,
        model: CausalLM,
        kv_cache: KVCache,
        config: EngineConfig,
        device: torch.device,
        max_model_len: int,
    ):
        self.model = model
        self.kv_cache = kv_cache
        self.config = config
        self.device = device
        self.max_model_len = max_model_len
        self.block_size = kv_cache.block_size
        self.max_blocks_per_seq = (max_model_len + self.block_size - 1) // self.block_size
        self.use_graphs = (
            config.enable_hipgraph
            and not config.enforce_eager
            and device.type == "cuda"
        )
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._graph_pool = None
        self.sampling_generator = torch.Generator(device=device if device.type == "cuda" else "cpu")
        self.sampling_generator.manual_seed(config.seed)
        self._sample_step = 0
        # Persistent sampler buffers, keyed by caller ("main" for the
        # decode path, "prefill" for the prefill segment of an OVERLAPPED
        # split mixed step — two concurrent streams must not share them).
        self._sample_bufs: Dict[str, Dict[str, torch.Tensor]] = {}
        # Token logprobs of the latest _sample call per buffer name, until
        # take_logprobs collects them: (asking rows, their k, batch size,
        # then either the entries (CPU) or the pinned record + copy event).
        self._logprobs: Dict[str, tuple] = {}
        # Count table of the repetition/presence/frequency penalties; holds no
        # memory until the first penalised request (PenaltyTable docstring).
        self.penalty_table = PenaltyTable(
            config.max_num_seqs, model.spec.vocab_size, device)
        # GPU logit tail: the sampler kernels read the lm_head GEMM's output
        # in the model dtype and apply the final soft-cap in registers, so no
        # fp32 [B, vocab] matrix is ever materialised. LLMQ_FUSED_LOGIT_TAIL=0
        # keeps the eager tail (compute_logits: widen, / cap, tanh, * cap)
        # for comparison; both sample identical tokens.
        self.fused_logit_tail = device.type == "cuda" and os.environ.get(
            "LLMQ_FUSED_LOGIT_TAIL", "1") not in ("0", "false", "")
        # Chunk continuations and prefix-cache hits assemble their attention
        # context with the gather_paged_kv kernel. LLMQ_PAGED_GATHER=0 keeps
        # the torch composition it replaced (advanced-index reads + casts +
        # index_copy_, per-token index lists) for A/B and bisection.
        self.paged_gather = os.environ.get(
            "LLMQ_PAGED_GATHER", "1") not in ("0", "false", "")
        if self.use_graphs:
            self._alloc_static_buffers()

    # -- static buffers / graph capture ---------------------------------

    def _alloc_static_buffers(self) -> None:
        B = min(self.config.max_num_seqs, self.config.hipgraph_max_batch)
        dev = self.device
        self.graph_max_bs = B
        self.in_ids = torch.zeros(B, dtype=torch.long, device=dev)
        self.in_pos = torch.zeros(B, dtype=torch.long, device=dev)
        self.in_slots = torch.zeros(B, dtype=torch.long, device=dev)
        self.in_block_tables = torch.zeros(
            B, self.max_blocks_per_seq, dtype=torch.int32, device=dev
        )
        self.in_context_lens = torch.ones(B, dtype=torch.int32, device=dev)
        self.out_hidden = torch.zeros(
            B, self.model.spec.hidden_size, dtype=self.model.dtype, device=dev
        )
        # pinned host staging for fast H2D of the per-step metadata
        self.h_ids = torch.zeros(B, dtype=torch.long, pin_memory=True)
        self.h_pos = torch.zeros(B, dtype=torch.long, pin_memory=True)
        self.h_slots = torch.zeros(B, dtype=torch.long, pin_memory=True)
        self.h_block_tables = torch.zeros(
            B, self.max_blocks_per_seq, dtype=torch.int32, pin_memory=True
        )
        self.h_context_lens = torch.ones(B, dtype=torch.int32, pin_memory=True)
        # (seq uid, preemption count, staged_len) per row — incremental
        # block-table staging. Keyed on Sequence.uid (monotonic, never
        # reused), NOT request_id: callers may reuse request ids across
        # sequence lifetimes, and a reused id at the same row with an equal
        # table length but different blocks would leave the hipGraph reading
        # the old sequence's block ids. num_preemptions guards the same-life
        # case where preemption-by-recompute reassigns the whole table.
        self._staged_rows: List[Tuple[int, int, int]] = [(-1, -1, 0)] * B

    def capture_graphs(self) -> None:
        """Capture the decode forward for each batch-size bucket."""
        if not self.use_graphs:
            return
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        for bs in reversed(_buckets(self.graph_max_bs)):  # large→small shares pool
            meta = DecodeMeta(
                block_tables=self.in_block_tables[:bs],
                context_lens=self.in_context_lens[:bs],
                slot_mapping=self.in_slots[:bs],
            )
            # warmup (also materialises workspace allocations)
            out = self.model.forward(self.in_ids[:bs], self.in_pos[:bs], self.kv_cache, meta)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=self._graph_pool):
                out = self.model.forward(
                    self.in_ids[:bs], self.in_pos[:bs], self.kv_cache, meta
                )
                self.out_hidden[:bs].copy_(out)
            if self._graph_pool is None:
                self._graph_pool = graph.pool()
            self._graphs[bs] = graph
        torch.cuda.synchronize()
        logger.info(
            "captured %d decode hipGraphs (max_bs=%d) in %.1fs",
            len(self._graphs), self.graph_max_bs, time.perf_counter() - t0,
        )

    def _bucket_for(self, bs: int) -> Optional[int]:
        for b in _buckets(self.graph_max_bs):
            if b >= bs:
                return b
        return None

    # -- prefill / mixed (chunk-aware, eager) ----------------------------

    def _build_prefill_meta(self, pseqs, chunks, dev) -> tuple:
        """Packed ids/pos/slots for the prefill segment + optional gather
        plan for chunk continuations. Returns (ids, pos, slots, meta,
        rel_last_idx) where rel_last_idx are within-segment row indices of
        FINAL chunks (the rows that sample)."""
        bs = self.block_size
        ids: List[int] = []
        pos: List[int] = []
        slots: List[int] = []
        cu = [0]
        cu_k = [0]
        rel_last: List[int] = []
        any_chunk = any(start > 0 for (start, _e) in chunks)
        for seq, (start, end) in zip(pseqs, chunks):
            n = end - start
            ids.extend(seq.token_ids[start:end])
            pos.extend(range(start, end))
            bt = seq.block_table
            slots.extend(bt[p // bs] * bs + (p % bs) for p in range(start, end))
            if end == seq.num_tokens:
                rel_last.append(cu[-1] + n - 1)
            cu.append(cu[-1] + n)
            cu_k.append(cu_k[-1] + end)  # keys = full context so far
        slot_mapping = torch.tensor(slots, dtype=torch.long, device=dev)
        gather = None
        if any_chunk:
            # One padded block-table row per sequence covering its past rows
            # [0, start): O(blocks) host work. Pad entries are never read
            # (rows past a sequence's own past come from the fresh chunk);
            # block 0 keeps them valid ids all the same.
            width = max(1, max(blocks_needed(st, bs) for (st, _e) in chunks))
            bt_np = np.zeros((len(pseqs), width), dtype=np.int32)
            for i, (seq, (start, _e)) in enumerate(zip(pseqs, chunks)):
                nb = blocks_needed(start, bs)
                bt_np[i, :nb] = seq.block_table[:nb]
            gather = ChunkGather(
                cu_seqlens_k=torch.tensor(cu_k, dtype=torch.int32, device=dev),
                block_tables=torch.from_numpy(bt_np).to(dev),
                total_k=cu_k[-1],
                max_seqlen_k=max(e for (_st, e) in chunks),
            )
            if not self.paged_gather:
                gather.torch_indices = self._torch_gather_indices(
                    pseqs, chunks, dev)
        meta = PrefillMeta(
            cu_seqlens=torch.tensor(cu, dtype=torch.int32, device=dev),
            max_seqlen=max(e - st for (st, e) in chunks),
            slot_mapping=slot_mapping,
            gather=gather,
        )
        return ids, pos, slot_mapping, meta, rel_last

    def _torch_gather_indices(self, pseqs, chunks, dev) -> TorchGatherIndices:
        """Per-token indices of the torch gather composition
        (LLMQ_PAGED_GATHER=0 only: O(tokens) host work)."""
        bs = self.block_size
        g_blocks: List[int] = []
        g_offs: List[int] = []
        past_dst: List[int] = []
        fresh_dst: List[int] = []
        krow = 0
        for seq, (start, end) in zip(pseqs, chunks):
            bt = seq.block_table
            for p in range(start):  # past rows gathered from the cache
                g_blocks.append(bt[p // bs])
                g_offs.append(p % bs)
                past_dst.append(krow)
                krow += 1
            fresh_dst.extend(range(krow, krow + end - start))
            krow += end - start
        return TorchGatherIndices(
            blocks=torch.tensor(g_blocks, dtype=torch.long, device=dev),
            offs=torch.tensor(g_offs, dtype=torch.long, device=dev),
            past_dst=torch.tensor(past_dst, dtype=torch.long, device=dev),
            fresh_dst=torch.tensor(fresh_dst, dtype=torch.long, device=dev),
        )

    @torch.no_grad()
    def execute_prefill(self, seqs: List[Sequence], chunks=None, buf_name: str = "main") -> torch.Tensor:
        """Run a packed prefill segment; returns sampled next tokens for the
        rows whose context completed this step (all rows when no chunking)."""
        if chunks is None:
            chunks = [(0, s.num_tokens) for s in seqs]
        dev = self.device
        ids, pos, slot_mapping, meta, rel_last = self._build_prefill_meta(
            seqs, chunks, dev
        )
        input_ids = torch.tensor(ids, dtype=torch.long, device=dev)
        positions = torch.tensor(pos, dtype=torch.long, device=dev)
        hidden = self.model.forward(input_ids, positions, self.kv_cache, meta)
        if not rel_last:
            return torch.empty(0, dtype=torch.long, device=dev)
        last_hidden = hidden[torch.tensor(rel_last, dtype=torch.long, device=dev)]
        logits, cap = self._logits_for_sampling(last_hidden)
        sample_seqs = [s for s, (st, e) in zip(seqs, chunks) if e == s.num_tokens]
        return self._sample(logits, sample_seqs, buf_name, softcap=cap)

    # -- mixed (decode rows + ride-along prefill rows, eager) ------------

    @torch.no_grad()
    def execute_mixed(self, batch: "ScheduledBatch") -> torch.Tensor:
        """Decode seqs[:n_decode] and prefill seqs[n_decode:] in ONE forward:
        shared GEMMs/norms over the packed rows, per-segment attention.
        Runs eager (prefill shapes vary); pure-decode steps keep hipGraphs.
        Returns tokens for [decode rows] + [final-chunk prefill rows]."""
        dev = self.device
        dseqs = batch.seqs[: batch.n_decode]
        pseqs = batch.seqs[batch.n_decode :]
        chunks = batch.chunks or [(0, s.num_tokens) for s in pseqs]
        bs = self.block_size
        nd = len(dseqs)

        ids = [s.token_ids[-1] for s in dseqs]
        pos = [s.num_tokens - 1 for s in dseqs]
        slots = [s.block_table[p // bs] * bs + (p % bs) for s, p in zip(dseqs, pos)]
        ctx = [s.num_tokens for s in dseqs]
        p_ids, p_pos, p_slots, pmeta, rel_last = self._build_prefill_meta(
            pseqs, chunks, dev
        )
        ids.extend(p_ids)
        pos.extend(p_pos)

        block_tables = torch.zeros(
            nd, max(len(s.block_table) for s in dseqs), dtype=torch.int32, device=dev
        )
        bt_np = np.zeros(tuple(block_tables.shape), dtype=np.int32)
        for i, s in enumerate(dseqs):
            bt_np[i, : len(s.block_table)] = s.block_table
        block_tables.copy_(torch.from_numpy(bt_np))
        d_slots = torch.tensor(slots, dtype=torch.long, device=dev)
        slot_mapping = torch.cat([d_slots, p_slots])
        meta = MixedMeta(
            n_decode=nd,
            decode=DecodeMeta(
                block_tables=block_tables,
                context_lens=torch.tensor(ctx, dtype=torch.int32, device=dev),
                slot_mapping=d_slots,
            ),
            prefill=pmeta,
            slot_mapping=slot_mapping,
        )
        input_ids = torch.tensor(ids, dtype=torch.long, device=dev)
        positions = torch.tensor(pos, dtype=torch.long, device=dev)
        hidden = self.model.forward(input_ids, positions, self.kv_cache, meta)
        last_idx = list(range(nd)) + [nd + r for r in rel_last]
        last_hidden = hidden[torch.tensor(last_idx, dtype=torch.long, device=dev)]
        logits, cap = self._logits_for_sampling(last_hidden)
        sample_seqs = list(dseqs) + [
            s for s, (st, e) in zip(pseqs, chunks) if e == s.num_tokens
        ]
        return self._sample(logits, sample_seqs, softcap=cap)

    # -- decode ----------------------------------------------------------

    @torch.no_grad()
    def execute_decode(self, seqs: List[Sequence], force_eager: bool = False) -> torch.Tensor:
        dev = self.device
        B = len(seqs)
        bs = self.block_size
        ids = [s.token_ids[-1] for s in seqs]
        pos = [s.num_tokens - 1 for s in seqs]
        slots = [s.block_table[p // bs] * bs + (p % bs) for s, p in zip(seqs, pos)]
        ctx = [s.num_tokens for s in seqs]

        bucket = self._bucket_for(B) if (self.use_graphs and not force_eager) else None
        if bucket is not None and bucket in self._graphs:
            return self._decode_with_graph(seqs, bucket, ids, pos, slots, ctx)

        block_tables = torch.zeros(
            B, max(len(s.block_table) for s in seqs), dtype=torch.int32, device=dev
        )
        bt_np = np.zeros(tuple(block_tables.shape), dtype=np.int32)
        for i, s in enumerate(seqs):
            bt_np[i, : len(s.block_table)] = s.block_table
        block_tables.copy_(torch.from_numpy(bt_np))
        meta = DecodeMeta(
            block_tables=block_tables,
            context_lens=torch.tensor(ctx, dtype=torch.int32, device=dev),
            slot_mapping=torch.tensor(slots, dtype=torch.long, device=dev),
        )
        input_ids = torch.tensor(ids, dtype=torch.long, device=dev)
        positions = torch.tensor(pos, dtype=torch.long, device=dev)
        hidden = self.model.forward(input_ids, positions, self.kv_cache, meta)
        logits, cap = self._logits_for_sampling(hidden)
        return self._sample(logits, seqs, softcap=cap)

    def _decode_with_graph(
        self, seqs: List[Sequence], bucket: int, ids, pos, slots, ctx
    ) -> torch.Tensor:
        B = len(seqs)
        # Stage metadata through pinned host buffers, one async copy each.
        self.h_ids[:B] = torch.tensor(ids, dtype=torch.long)
        self.h_pos[:B] = torch.tensor(pos, dtype=torch.long)
        self.h_slots[:B] = torch.tensor(slots, dtype=torch.long)
        self.h_context_lens[:B] = torch.tensor(ctx, dtype=torch.int32)
        self.h_context_lens[B:bucket] = 1
        # Block tables are staged INCREMENTALLY: a row is rewritten only when
        # its (request, table length) changed since the last stage. With
        # max_model_len in the 100k class the table is thousands of columns
        # wide — rewriting every row every step cost more host time than the
        # whole decode step (measured on llama-3.2-3b, max_blocks=8192).
        bt_np = self.h_block_tables.numpy()
        max_w = 1
        for i, s in enumerate(seqs):
            n = len(s.block_table)
            if n > max_w:
                max_w = n
            if self._staged_rows[i] != (s.uid, s.num_preemptions, n):
                bt_np[i, :n] = s.block_table
                self._staged_rows[i] = (s.uid, s.num_preemptions, n)
        if B < bucket:
            # pad rows: context_len 1 pointing at block 0 (defined garbage,
            # their logits are never read)
            self.h_slots[B:bucket] = 0
            self.h_ids[B:bucket] = 0
            self.h_pos[B:bucket] = 0
            for i in range(B, bucket):
                if self._staged_rows[i] != (-1, -1, 0):
                    bt_np[i, :1] = 0
                    self._staged_rows[i] = (-1, -1, 0)
        self.in_ids[:bucket].copy_(self.h_ids[:bucket], non_blocking=True)
        self.in_pos[:bucket].copy_(self.h_pos[:bucket], non_blocking=True)
        self.in_slots[:bucket].copy_(self.h_slots[:bucket], non_blocking=True)
        self.in_context_lens[:bucket].copy_(self.h_context_lens[:bucket], non_blocking=True)
        self.in_block_tables[:bucket, :max_w].copy_(
            self.h_block_tables[:bucket, :max_w], non_blocking=True
        )
        self._graphs[bucket].replay()
        logits, cap = self._logits_for_sampling(self.out_hidden[:B])
        return self._sample(logits, seqs, softcap=cap)

    # -- sampling --------------------------------------------------------

    def _sample_buf(self, name: str, B: int, dev) -> Dict[str, torch.Tensor]:
        buf = self._sample_bufs.get(name)
        if buf is None or buf["out"].numel() < B:
            cap = max(B, self.config.max_num_seqs)
            buf = {
                "out": torch.empty(cap, dtype=torch.int64, device=dev),
                "keys": torch.empty(cap, dtype=torch.int64, device=dev),
                "temps": torch.empty(cap, dtype=torch.float32, device=dev),
                "temps_h": torch.empty(cap, dtype=torch.float32, pin_memory=True),
                "seeds": torch.empty(cap, dtype=torch.int32, device=dev),
                "seeds_h": torch.empty(cap, dtype=torch.int32, pin_memory=True),
                "pos": torch.empty(cap, dtype=torch.int32, device=dev),
                "pos_h": torch.empty(cap, dtype=torch.int32, pin_memory=True),
                "minp": torch.empty(cap, dtype=torch.float32, device=dev),
                "minp_h": torch.empty(cap, dtype=torch.float32, pin_memory=True),
                "slots": torch.empty(cap, dtype=torch.int32, device=dev),
                "slots_h": torch.empty(cap, dtype=torch.int32, pin_memory=True),
                "pen": torch.empty(cap, 3, dtype=torch.float32, device=dev),
                "pen_h": torch.empty(cap, 3, dtype=torch.float32, pin_memory=True),
                # token logprobs: the rows that asked, and one packed int32
                # record per row (ids | lp bits | rank) so that the results
                # reach the host in a single copy
                "lp_rows": torch.empty(cap, dtype=torch.int32, device=dev),
                "lp_rows_h": torch.empty(cap, dtype=torch.int32, pin_memory=True),
                "lp_pack": torch.empty(cap, _LP_PACK, dtype=torch.int32, device=dev),
                "lp_pack_h": torch.empty(cap, _LP_PACK, dtype=torch.int32, pin_memory=True),
            }
            self._sample_bufs[name] = buf
        return buf

    def _logits_for_sampling(self, hidden: torch.Tensor) -> Tuple[torch.Tensor, float]:
        """(logits, softcap) for _sample: the raw lm_head output plus the cap
        the sampler kernels still have to apply, or fully formed fp32 logits
        and 0 (CPU, LLMQ_FUSED_LOGIT_TAIL=0)."""
        if self.fused_logit_tail:
            cap = self.model.spec.final_softcap
            return self.model.lm_head_logits(hidden), float(cap) if cap and cap > 0 else 0.0
        return self.model.compute_logits(hidden), 0.0

    @staticmethod
    def _penalised_logits_cpu(logits: torch.Tensor, seqs: List[Sequence]) -> torch.Tensor:
        V = logits.size(1)
        words = torch.from_numpy(np.stack([
            count_words(s.token_ids, s.prompt_len, V).astype(np.int32) for s in seqs
        ]))
        p = [s.params for s in seqs]
        return torch_ref.apply_penalties(
            logits, words & COUNT_MASK, (words & PROMPT_BIT) != 0,
            torch.tensor([q.repetition_penalty for q in p]),
            torch.tensor([q.frequency_penalty for q in p]),
            torch.tensor([q.presence_penalty for q in p]),
        )

    def _sample(self, logits: torch.Tensor, seqs: List[Sequence],
                buf_name: str = "main", softcap: float = 0.0) -> torch.Tensor:
        dev = logits.device
        self._sample_step += 1
        self._logprobs.pop(buf_name, None)
        V = logits.size(1)
        lp_rows = [i for i, s in enumerate(seqs) if s.params.logprobs is not None]
        lp_ks = [min(seqs[i].params.logprobs, ops.MAX_LOGPROBS, V) for i in lp_rows]
        simple = all(
            s.params.top_k == 0 and s.params.top_p >= 1.0 and s.params.min_p <= 0.0
            for s in seqs
        )
        penalised = any(wants_penalties(s.params) for s in seqs)
        if dev.type == "cuda":
            # Fused one-pass HIP sampler (gumbel-max / greedy argmax).
            # Top-k/top-p rows reduce to a per-row logit keep-bound via
            # histogram select — no full-vocab sort, no CPU round trips,
            # seeded rows stay on-device (ADVICE r1 low #4 / weakness 6).
            B = len(seqs)
            buf = self._sample_buf(buf_name, B, dev)
            th = buf["temps_h"]
            sh = buf["seeds_h"]
            ph = buf["pos_h"]
            for i, s in enumerate(seqs):
                th[i] = s.params.temperature
                rs = s.params.seed
                if rs is None:
                    sh[i] = 0  # unseeded sentinel
                else:
                    v = rs & 0x7FFFFFFF
                    sh[i] = v if v else 0x1E3779B9  # remap literal seed 0
                ph[i] = s.output_len
            buf["temps"][:B].copy_(th[:B], non_blocking=True)
            buf["seeds"][:B].copy_(sh[:B], non_blocking=True)
            buf["pos"][:B].copy_(ph[:B], non_blocking=True)
            # fused tail: logits stay in the GEMM's dtype (no fp32 copy)
            logits_f = logits if self.fused_logit_tail else logits.float()
            # Penalised rows read their row of the count table inside the
            # kernels; a batch without any passes no table and runs the
            # kernels it ran before the table existed.
            pen = {}
            if penalised:
                slots = self.penalty_table.slots_for(seqs)
                slh, pnh = buf["slots_h"], buf["pen_h"]
                for i, s in enumerate(seqs):
                    slh[i] = slots[i]
                    pnh[i, 0] = s.params.repetition_penalty
                    pnh[i, 1] = s.params.frequency_penalty
                    pnh[i, 2] = s.params.presence_penalty
                buf["slots"][:B].copy_(slh[:B], non_blocking=True)
                buf["pen"][:B].copy_(pnh[:B], non_blocking=True)
                pen = dict(pen_table=self.penalty_table.table,
                           pen_slots=buf["slots"][:B], pen_params=buf["pen"][:B])
            bounds = None
            if not simple:
                tps = torch.tensor([s.params.top_p for s in seqs],
                                   dtype=torch.float32, device=dev)
                tks = torch.tensor([s.params.top_k for s in seqs],
                                   dtype=torch.int64, device=dev)
                min_ps = None
                if any(s.params.min_p > 0.0 for s in seqs):
                    mh = buf["minp_h"]
                    for i, s in enumerate(seqs):
                        mh[i] = s.params.min_p
                    buf["minp"][:B].copy_(mh[:B], non_blocking=True)
                    min_ps = buf["minp"][:B]
                bounds = ops.topk_topp_bound(
                    logits_f, buf["temps"][:B], tps, tks, softcap,
                    min_ps=min_ps, **pen)
            ops.sample_gumbel_argmax(
                buf["out"][:B], buf["keys"][:B], logits_f,
                buf["temps"][:B], buf["seeds"][:B],
                buf["pos"][:B], self.config.seed, self._sample_step, bounds,
                softcap, **pen,
            )
            if penalised:
                self.penalty_table.count_sampled(
                    seqs, buf["slots"][:B], buf["out"][:B])
            if lp_rows:
                # One more read of the asking rows, of the logits the sampler
                # read (before penalties and temperature): one launch and one
                # device-to-host copy, on this call's stream.
                R, K = len(lp_rows), max(lp_ks)
                rh = buf["lp_rows_h"]
                for j, i in enumerate(lp_rows):
                    rh[j] = i
                buf["lp_rows"][:R].copy_(rh[:R], non_blocking=True)
                pack = buf["lp_pack"]
                ops.token_logprobs(
                    logits_f, buf["out"][:B], K, softcap, rows=buf["lp_rows"][:R],
                    out=(pack[:R, : 1 + K],
                         pack[:R, _LP_W : _LP_W + 1 + K].view(torch.float32),
                         pack[:R, 2 * _LP_W]))
                buf["lp_pack_h"][:R].copy_(pack[:R], non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                self._logprobs[buf_name] = (lp_rows, lp_ks, B, buf["lp_pack_h"], done)
            return buf["out"][:B]
        raw_logits = logits
        if penalised:
            # CPU: the specification itself, from the token histories
            logits = self._penalised_logits_cpu(logits, seqs)
        temps = torch.tensor([s.params.temperature for s in seqs], dtype=torch.float32, device=dev)
        tps = torch.tensor([s.params.top_p for s in seqs], dtype=torch.float32, device=dev)
        tks = torch.tensor([s.params.top_k for s in seqs], dtype=torch.int64, device=dev)
        mps = torch.tensor([s.params.min_p for s in seqs], dtype=torch.float32, device=dev)
        out = ops.sample_tokens(logits, temps, tps, tks, self.sampling_generator, mps)
        # Per-request seeds (reproducible sampling): re-draw those rows with
        # a generator keyed on (seed, output position) — batch-independent.
        # Gathered in ONE device→host transfer (a per-row .cpu() would sync
        # the stream once per seeded row per step).
        seeded = [
            i for i, s in enumerate(seqs)
            if s.params.seed is not None and s.params.temperature > 0
        ]
        if seeded:
            idx = torch.tensor(seeded, dtype=torch.long, device=dev)
            rows = logits[idx].float().cpu()
            temps_c, tps_c, tks_c = temps[idx].cpu(), tps[idx].cpu(), tks[idx].cpu()
            mps_c = mps[idx].cpu()
            redraw = torch.empty(len(seeded), dtype=out.dtype)
            for j, i in enumerate(seeded):
                s = seqs[i]
                g = torch.Generator(device="cpu")
                g.manual_seed((s.params.seed << 20) ^ s.output_len)
                redraw[j] = ops.sample_tokens(
                    rows[j : j + 1], temps_c[j : j + 1], tps_c[j : j + 1],
                    tks_c[j : j + 1], g, mps_c[j : j + 1],
                )[0]
            out[idx] = redraw.to(out.device)
        if lp_rows:
            # CPU: the specification, on the logits before penalties
            ids, lp, rank = torch_ref.token_logprobs(
                raw_logits, out, max(lp_ks), softcap,
                rows=torch.tensor(lp_rows, dtype=torch.int32))
            self._logprobs[buf_name] = (
                lp_rows, lp_ks, len(seqs), _logprob_entries(ids, lp, rank, lp_ks))
        return out

    def take_logprobs(self, buf_name: str = "main") -> Optional[List[Optional[tuple]]]:
        """Token logprobs of the latest _sample call on `buf_name`, once: one
        entry per sampled row, (token_id, logprob, rank, [(id, logprob) x k])
        for rows that asked and None for the others; None when no row asked.
        On the GPU this waits for that call's result copy, so in an overlapped
        step call it after the streams have joined."""
        res = self._logprobs.pop(buf_name, None)
        if res is None:
            return None
        rows, ks, B = res[:3]
        if len(res) == 4:
            entries = res[3]
        else:
            host, done = res[3:]
            done.synchronize()
            rec = host[: len(rows)].numpy()
            entries = _logprob_entries(
                rec[:, :_LP_W], rec[:, _LP_W : 2 * _LP_W].view(np.float32),
                rec[:, 2 * _LP_W], ks)
        out: List[Optional[tuple]] = [None] * B
        for i, e in zip(rows, entries):
            out[i] = e
        return out
