"""Token-count table behind the sampler's repetition / presence / frequency
penalties.

One row per penalised sequence, one 16-bit word per vocab entry: bit 15 says
the token occurs in the prompt, bits 0-14 count its occurrences in the output
(saturating at 32767). The table is dense on purpose: 2 bytes per vocab entry
per row (512 KB at V = 256k, 256 MB for 512 rows) buys a sampler that needs
neither a de-duplication pass nor a per-step host upload growing with the
context length. The sampler kernels read a row next to the logits, and
`ops.penalty_count_tokens` adds each sampled token on the device.

This class owns the tensor, the free list of rows ("slots") and the map
`seq.uid -> (slot, accounted_len)`. It is device-agnostic (on CPU tensors the
increment is a torch index_put), so the lifecycle is testable without a GPU.

Invariant: at the moment a sequence is sampled, its row equals the counts
recomputed from `seq.token_ids`. `slots_for` restores it where it does not
hold (first sampling, after preemption-by-recompute, after the slot was
released) by rebuilding the row from `seq.token_ids`; `count_sampled` keeps
it by adding the token the engine is about to append.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence as Seq

import numpy as np
import torch

from llmq_amd import ops

PROMPT_BIT = 0x8000
COUNT_MASK = 0x7FFF


class PenaltyTableError(ValueError):
    """The table could not be allocated; fails the request, not the engine."""


def wants_penalties(params) -> bool:
    """True when any of the three penalties is away from its neutral value."""
    return (
        params.repetition_penalty != 1.0
        or params.frequency_penalty != 0.0
        or params.presence_penalty != 0.0
    )


def count_words(token_ids: Seq[int], prompt_len: int, width: int) -> np.ndarray:
    """The table row for a token history, as uint16[width]."""
    row = np.zeros(width, dtype=np.uint16)
    ids = np.asarray(token_ids, dtype=np.int64)
    row[ids[:prompt_len]] = PROMPT_BIT
    out = np.bincount(ids[prompt_len:], minlength=width)[:width]
    row |= np.minimum(out, COUNT_MASK).astype(np.uint16)
    return row


class PenaltyTable:
    def __init__(self, num_slots: int, vocab_size: int, device: torch.device):
        self.num_slots = num_slots
        self.vocab_size = vocab_size
        # rows padded to 128 bytes: with the allocator's aligned base every
        # row starts 16-byte aligned, like the rows of a V % 8 == 0 logits
        # matrix, so the kernels read the counts with 16-byte loads
        self.vpad = (vocab_size + 63) // 64 * 64
        self.device = device
        self.table: Optional[torch.Tensor] = None  # [num_slots, vpad] int16
        self._free: List[int] = list(range(num_slots - 1, -1, -1))
        self._rows: Dict[int, List[int]] = {}  # uid -> [slot, accounted_len]

    # -- allocation ------------------------------------------------------

    def ensure_allocated(self) -> None:
        """Lazy: an engine that never sees a penalised request holds no table."""
        if self.table is not None:
            return
        try:
            self.table = torch.zeros(
                self.num_slots, self.vpad, dtype=torch.int16, device=self.device)
            if self.device.type == "cuda":
                # one-time: the zero fill must not race a row rebuild issued
                # on the other stream of an overlapped mixed step
                torch.cuda.synchronize(self.device)
        except torch.OutOfMemoryError as exc:
            need = self.num_slots * self.vpad * 2 / 2 ** 20
            raise PenaltyTableError(
                f"no memory for the sampling-penalty count table ({need:.0f} MB: "
                f"{self.num_slots} sequences x {self.vpad} vocab entries x 2 "
                "bytes); lower gpu_memory_utilization or max_num_seqs, or send "
                "requests without repetition/presence/frequency penalties"
            ) from exc

    @property
    def num_free(self) -> int:
        return len(self._free)

    def slot_of(self, seq) -> int:
        entry = self._rows.get(seq.uid)
        return entry[0] if entry is not None else -1

    # -- per sampling call -----------------------------------------------

    def slots_for(self, seqs) -> List[int]:
        """The table row of each sequence about to be sampled, -1 for those
        without penalties. Rows that do not account for exactly
        `seq.token_ids` are (re)built first."""
        slots = []
        for seq in seqs:
            if not wants_penalties(seq.params):
                slots.append(-1)
                continue
            self.ensure_allocated()
            entry = self._rows.get(seq.uid)
            if entry is None:
                if not self._free:
                    raise RuntimeError(
                        "penalty table out of slots: more penalised sequences "
                        f"sampling than max_num_seqs={self.num_slots}")
                entry = [self._free.pop(), -1]
                self._rows[seq.uid] = entry
            if entry[1] != len(seq.token_ids):
                self._rebuild(entry[0], seq)
                entry[1] = len(seq.token_ids)
            slots.append(entry[0])
        return slots

    def _rebuild(self, slot: int, seq) -> None:
        # one-time row setup: built on the host, one row copy on the current
        # stream (which the step's wait_stream calls order against the
        # sampler on the other stream)
        words = count_words(seq.token_ids, seq.prompt_len, self.vpad)
        self.table[slot].copy_(torch.from_numpy(words.view(np.int16)))

    def count_sampled(self, seqs, slots: torch.Tensor, tokens: torch.Tensor) -> None:
        """After sampling: add each row's token to its counts (on the device,
        no host sync) and account for the append the engine does next."""
        if self.table is None:
            return
        ops.penalty_count_tokens(self.table, slots, tokens)
        for seq in seqs:
            entry = self._rows.get(seq.uid)
            if entry is not None:
                entry[1] = len(seq.token_ids) + 1

    # -- release ---------------------------------------------------------

    def release(self, seq) -> None:
        """Finish, abort, preemption: the row goes back to the free list. The
        map is keyed on uid, so a reused request_id never finds a stale row."""
        entry = self._rows.pop(seq.uid, None)
        if entry is not None:
            self._free.append(entry[0])
