"""Per-request sampling parameters.

The reference hardcodes temperature 0.7 and exposes only max_tokens/stop
(vllm_worker.py:161-165). Here every job can override (core.models.Job
sampling fields)."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional


MAX_LOGPROBS = 20  # the token_logprobs kernel's top-k limit


@dataclass
class SamplingParams:
    temperature: float = 0.7
    top_p: float = 1.0
    top_k: int = 0  # 0 = disabled
    max_tokens: int = 8192
    stop: Optional[List[str]] = None
    seed: Optional[int] = None
    ignore_eos: bool = False
    # Applied by the sampler to the (soft-capped) logits in this order:
    # tokens seen in the prompt or the output: l > 0 ? l / r : l * r; then
    # l -= frequency_penalty * count_in_output; then l -= presence_penalty
    # for tokens in the output. Greedy rows take the argmax of the result.
    repetition_penalty: float = 1.0  # 1 = off
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # keep tokens with probability >= min_p x the most likely token's
    min_p: float = 0.0  # 0 = off
    # Return the log-probability and rank of every generated token plus the
    # `logprobs` most likely alternatives (0 = the token alone, None = off),
    # under log_softmax of the model's (soft-capped) logits: before penalties,
    # temperature and top-k/top-p/min_p.
    logprobs: Optional[int] = None

    def __post_init__(self) -> None:
        if self.temperature < 0:
            raise ValueError("temperature must be >= 0")
        if not 0 < self.top_p <= 1.0:
            raise ValueError("top_p must be in (0, 1]")
        if self.top_k < 0:
            raise ValueError("top_k must be >= 0")
        if self.max_tokens < 1:
            raise ValueError("max_tokens must be >= 1")
        if not self.repetition_penalty > 0:
            raise ValueError("repetition_penalty must be > 0")
        if not -2.0 <= self.presence_penalty <= 2.0:
            raise ValueError("presence_penalty must be in [-2, 2]")
        if not -2.0 <= self.frequency_penalty <= 2.0:
            raise ValueError("frequency_penalty must be in [-2, 2]")
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError("min_p must be in [0, 1]")
        if self.logprobs is not None and not 0 <= self.logprobs <= MAX_LOGPROBS:
            raise ValueError(f"logprobs must be in [0, {MAX_LOGPROBS}]")

    @property
    def greedy(self) -> bool:
        return self.temperature == 0.0
