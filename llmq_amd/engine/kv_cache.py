"""Paged KV cache + block allocator.

Layout per layer: [num_blocks, num_kv_heads, block_size, head_dim] — a
(block, kv_head) pair is a contiguous [block_size, head_dim] tile, which is
what one workgroup of the CDNA4 decode kernel streams with coalesced
dwordx4 loads (PagedAttention equivalent).

Sizing: the engine claims ``gpu_memory_utilization`` × free HBM after
weights are resident (MI355X: 288 GB per GPU, so 9B-bf16 leaves ~240 GB of
KV — tens of thousands of 8k contexts; the scheduler, not memory, is the
usual admission limit)."""

from __future__ import annotations

import logging
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch

logger = logging.getLogger(__name__)


class KVCache:
    def __init__(
        self,
        num_layers: int,
        num_blocks: int,
        num_kv_heads: int,
        block_size: int,
        head_dim: int,
        device: torch.device,
        dtype: torch.dtype,
    ):
        self.num_layers = num_layers
        self.num_blocks = num_blocks
        self.block_size = block_size
        self.k: List[torch.Tensor] = []
        self.v: List[torch.Tensor] = []
        for _ in range(num_layers):
            self.k.append(
                torch.zeros(
                    num_blocks, num_kv_heads, block_size, head_dim, device=device, dtype=dtype
                )
            )
            self.v.append(
                torch.zeros(
                    num_blocks, num_kv_heads, block_size, head_dim, device=device, dtype=dtype
                )
            )

    @staticmethod
    def block_bytes(num_layers, num_kv_heads, block_size, head_dim, dtype) -> int:
        elem = torch.tensor([], dtype=dtype).element_size()
        return 2 * num_layers * num_kv_heads * block_size * head_dim * elem

    @classmethod
    def num_blocks_for_budget(
        cls, budget_bytes: int, num_layers, num_kv_heads, block_size, head_dim, dtype
    ) -> int:
        per_block = cls.block_bytes(num_layers, num_kv_heads, block_size, head_dim, dtype)
        return max(budget_bytes // per_block, 0)


class BlockAllocator:
    """Free-list allocator over block ids [0, num_blocks)."""

    def __init__(self, num_blocks: int):
        self.num_blocks = num_blocks
        self._free: List[int] = list(range(num_blocks - 1, -1, -1))

    @property
    def num_free(self) -> int:
        return len(self._free)

    def can_allocate(self, n: int) -> bool:
        return len(self._free) >= n

    def allocate(self, n: int) -> Optional[List[int]]:
        if len(self._free) < n:
            return None
        if n == 0:
            return []
        blocks = self._free[-n:][::-1]
        del self._free[-n:]
        return blocks

    def free(self, blocks: List[int]) -> None:
        self._free.extend(reversed(blocks))


class PrefixCachingAllocator:
    """BlockAllocator with automatic prefix caching over full blocks.

    A registered block is a node of a prefix tree: its identity is the tuple
    of its ``block_size`` token ids plus the node id of the cached block
    before it (0 = root). The dict lookup compares that exact content, so a
    hash collision can never serve another prompt's KV; keys are tuples of
    ints, whose hashes are not salted per process, so TP ranks running their
    own scheduler over one request stream take identical decisions.

    Node ids are handed out once and never reused. A block id is reused
    after eviction, so linking children to the parent's BLOCK id would let a
    stale child match under whatever content the id holds next; under a
    retired node id it is simply unreachable until it is evicted itself.

    Blocks are reference counted. ``free`` drops one reference; at zero a
    registered block parks on an LRU list with its contents (and cache
    entry) kept, an unregistered one returns to the free list. ``allocate``
    takes truly free blocks first, then evicts from the LRU's old end. A
    released table enters the LRU tail first, so the tail of a chain is
    evicted before its head and a half-evicted chain still serves its head.
    """

    _ROOT = 0

    def __init__(self, num_blocks: int, block_size: int):
        self.num_blocks = num_blocks
        self.block_size = block_size
        self._free: List[int] = list(range(num_blocks - 1, -1, -1))
        self._ref: List[int] = [0] * num_blocks
        self._cache: Dict[Tuple[int, Tuple[int, ...]], int] = {}  # key -> block
        self._key_of: Dict[int, Tuple[int, Tuple[int, ...]]] = {}  # block -> key
        self._node_of: Dict[int, int] = {}                          # block -> node id
        self._lru: "OrderedDict[int, None]" = OrderedDict()  # oldest first
        self._next_node = 1
        self.lookup_tokens = 0
        self.hit_tokens = 0
        self.evictions = 0

    # -- BlockAllocator interface ------------------------------------------

    @property
    def num_free(self) -> int:
        return len(self._free) + len(self._lru)

    def can_allocate(self, n: int) -> bool:
        return self.num_free >= n

    def allocate(self, n: int) -> Optional[List[int]]:
        if self.num_free < n:
            return None
        blocks: List[int] = []
        take = min(n, len(self._free))
        if take:
            blocks = self._free[-take:][::-1]
            del self._free[-take:]
        while len(blocks) < n:
            block, _ = self._lru.popitem(last=False)
            del self._cache[self._key_of.pop(block)]
            del self._node_of[block]
            self.evictions += 1
            blocks.append(block)
        for b in blocks:
            self._ref[b] = 1
        return blocks

    def free(self, blocks: List[int]) -> None:
        for b in reversed(blocks):
            assert self._ref[b] > 0, f"block {b} freed more often than held"
            self._ref[b] -= 1
            if self._ref[b] == 0:
                if b in self._node_of:
                    self._lru[b] = None
                else:
                    self._free.append(b)

    # -- prefix cache --------------------------------------------------------

    def refcount(self, block: int) -> int:
        return self._ref[block]

    def lookup(self, token_ids: List[int]) -> List[int]:
        """Longest chain of cached blocks matching the head of ``token_ids``;
        takes a reference on each. Capped at ((n - 1) // block_size) blocks so
        at least one prompt token is always computed and sampled from."""
        bs = self.block_size
        hit: List[int] = []
        parent = self._ROOT
        for i in range((len(token_ids) - 1) // bs):
            block = self._cache.get((parent, tuple(token_ids[i * bs:(i + 1) * bs])))
            if block is None:
                break
            hit.append(block)
            parent = self._node_of[block]
        for b in hit:
            if self._ref[b] == 0:
                del self._lru[b]
            self._ref[b] += 1
        return hit

    def register(self, seq_tokens: List[int], block_table: List[int],
                 upto_tokens: int) -> None:
        """Enter the full blocks covering [0, upto_tokens) into the cache.
        Idempotent. A block whose content is already cached under another id
        stays unregistered (the chain continues under the cached one)."""
        bs = self.block_size
        parent = self._ROOT
        for i in range(upto_tokens // bs):
            block = block_table[i]
            node = self._node_of.get(block)
            if node is None:
                key = (parent, tuple(seq_tokens[i * bs:(i + 1) * bs]))
                other = self._cache.get(key)
                if other is not None:
                    node = self._node_of[other]
                else:
                    node = self._next_node
                    self._next_node += 1
                    self._cache[key] = block
                    self._key_of[block] = key
                    self._node_of[block] = node
            parent = node

    def note_admission(self, prompt_tokens: int, hit_tokens: int) -> None:
        self.lookup_tokens += prompt_tokens
        self.hit_tokens += hit_tokens

    def stats(self) -> Dict[str, int]:
        return {
            "lookup_tokens": self.lookup_tokens,
            "hit_tokens": self.hit_tokens,
            "cached_blocks": len(self._cache),
            "evictions": self.evictions,
        }


def blocks_needed(num_tokens: int, block_size: int) -> int:
    return (num_tokens + block_size - 1) // block_size
