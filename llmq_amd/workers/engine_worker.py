"""GPU inference worker backed by the in-tree MI355X engine.

Replaces the reference's vLLM worker (llmq/workers/vllm_worker.py:11-201):
where the reference hands each job to vLLM's AsyncLLMEngine
(vllm_worker.py:183-186), this worker owns an in-tree ``LLMEngine``
(continuous batching + paged KV + CDNA4 HIP kernels) and bridges the
asyncio consume loop to a dedicated engine thread so the AMQP-style
broker connection and heartbeats stay live while the GPU steps
(SURVEY §7 "Keeping asyncio + engine thread + AMQP heartbeats live").

Tensor parallelism (vllm_worker.py:59-108 passthrough in the reference):
rank 0 runs this worker; ranks 1..tp-1 are follower processes executing
the same deterministic engine replica. Rank 0 broadcasts control ops
(request adds) over a gloo control group before each step; model
all-reduces run over RCCL/xGMI ("nccl" backend). Logits are identical on
every rank after the final all-reduce (lm_head is replicated) and the
sampler generators share a seed, so every rank appends identical tokens
without an extra token broadcast on the hot path.

Per-job sampling honours job fields then stage config then defaults —
fixing the reference's hardcoded temperature 0.7 (vllm_worker.py:162) and
ignored per-stage temperature (pipeline.py:132) while keeping 0.7 as the
default.
"""

from __future__ import annotations

import asyncio
import logging
import os
import threading
import time
import uuid
from collections import deque
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional

from llmq_amd.core.config import Config
from llmq_amd.core.models import Job, Result
from llmq_amd.core.pipeline import PipelineConfig
from llmq_amd.engine.sampling_params import SamplingParams
from llmq_amd.workers.base import BaseWorker

logger = logging.getLogger(__name__)

DEFAULT_TEMPERATURE = 0.7  # reference default, vllm_worker.py:162


@dataclass
class _FinishedRequest:
    text: str
    prompt_tokens: int
    output_tokens: int
    finish_reason: Optional[str]
    queue_wait_ms: Optional[float]
    prefill_ms: Optional[float]
    decode_ms: Optional[float]
    cached_tokens: int = 0
    logprobs: Optional[List[Dict[str, Any]]] = None
    cumulative_logprob: Optional[float] = None


def format_logprobs(entries: List[tuple], tokenizer: Any) -> List[Dict[str, Any]]:
    """The engine's (token_id, logprob, rank, [(id, logprob)]) entries of one
    finished request as the Result's list of dicts, with every token id
    decoded on its own (special tokens kept)."""
    strings: Dict[int, str] = {}

    def text(tid: int) -> str:
        if tid not in strings:
            strings[tid] = tokenizer.decode([tid], skip_special_tokens=False)
        return strings[tid]

    return [
        {
            "token_id": tid, "token": text(tid), "logprob": lp, "rank": rank,
            "top_logprobs": [
                {"token_id": i, "token": text(i), "logprob": l} for i, l in top
            ],
        }
        for tid, lp, rank, top in entries
    ]


@dataclass
class _Submission:
    request_id: str
    prompt: str
    params: SamplingParams


class AsyncEngineBridge:
    """asyncio ⇄ engine-thread bridge.

    ``generate()`` is awaitable from any asyncio task; the engine thread
    drains submissions, steps the engine continuously while work exists,
    and resolves futures on the event loop via call_soon_threadsafe. The
    event loop is therefore never blocked by a GPU step — broker
    heartbeats and prefetched deliveries keep flowing, which is what lets
    queue-prefetch ≫ max_num_seqs keep the admission queue full
    (the reference's core throughput trick).
    """

    IDLE_POLL_S = 0.005

    def __init__(
        self,
        engine_factory: Callable[[], Any],
        tp_size: int = 1,
    ):
        self._factory = engine_factory
        self.tp_size = tp_size
        self._loop: Optional[asyncio.AbstractEventLoop] = None
        self._pending: deque[_Submission] = deque()
        self._pending_lock = threading.Lock()
        self._wakeup = threading.Event()
        self._futures: Dict[str, asyncio.Future] = {}
        self._thread: Optional[threading.Thread] = None
        self._ready = threading.Event()
        self._init_error: Optional[BaseException] = None
        self._stop = False
        self._fatal: Optional[BaseException] = None
        self.engine: Any = None
        self._ctrl_group = None

    # -- asyncio side ----------------------------------------------------

    async def start(self) -> None:
        self._loop = asyncio.get_running_loop()
        self._thread = threading.Thread(
            target=self._run, name="engine-thread", daemon=True
        )
        self._thread.start()
        while not self._ready.is_set():
            await asyncio.sleep(0.05)
        if self._init_error is not None:
            raise RuntimeError("engine initialisation failed") from self._init_error

    async def generate(
        self, request_id: str, prompt: str, params: SamplingParams
    ) -> _FinishedRequest:
        assert self._loop is not None, "bridge not started"
        if self._fatal is not None:
            raise RuntimeError("engine thread crashed") from self._fatal
        fut: asyncio.Future = self._loop.create_future()
        self._futures[request_id] = fut
        with self._pending_lock:
            self._pending.append(_Submission(request_id, prompt, params))
        self._wakeup.set()
        try:
            return await fut
        finally:
            self._futures.pop(request_id, None)

    def shutdown(self) -> None:
        self._stop = True
        self._wakeup.set()
        if self._thread is not None:
            self._thread.join(timeout=60.0)

    @property
    def num_in_flight(self) -> int:
        return len(self._futures)

    # -- engine thread ---------------------------------------------------

    def _drain(self) -> List[_Submission]:
        with self._pending_lock:
            out = list(self._pending)
            self._pending.clear()
        self._wakeup.clear()
        return out

    def _run(self) -> None:
        try:
            self.engine = self._factory()
            if self.tp_size > 1:
                import torch.distributed as dist

                # Control ops over gloo (CPU, cheap); model collectives use
                # the default device group (RCCL on GPU).
                self._ctrl_group = dist.new_group(
                    list(range(self.tp_size)), backend="gloo"
                )
        except BaseException as exc:  # noqa: BLE001 — surfaced to start()
            self._init_error = exc
            self._ready.set()
            return
        self._ready.set()
        engine = self.engine
        last_log = time.monotonic()
        steps_since = 0
        try:
            while not self._stop:
                now = time.monotonic()
                if now - last_log >= 10.0:
                    sched = engine.scheduler
                    logger.info(
                        "engine: %.1f steps/s, running=%d waiting=%d in_flight=%d "
                        "free_blocks=%d",
                        steps_since / (now - last_log), sched.num_running,
                        sched.num_waiting, len(self._futures),
                        engine.allocator.num_free,
                    )
                    last_log, steps_since = now, 0
                subs = self._drain()
                if not subs and not engine.has_unfinished():
                    self._wakeup.wait(timeout=self.IDLE_POLL_S)
                    continue
                if self.tp_size > 1:
                    self._broadcast_ctrl(
                        ("work", [(s.request_id, s.prompt, s.params) for s in subs])
                    )
                for s in subs:
                    try:
                        engine.add_request(s.request_id, prompt=s.prompt, params=s.params)
                    except ValueError as exc:
                        self._resolve_error(s.request_id, exc)
                steps_since += 1
                for out in engine.step():
                    if out.finished:
                        # token strings: decoded here, once per request
                        entries = getattr(out, "logprobs", None)
                        self._resolve(
                            out.request_id,
                            _FinishedRequest(
                                text=out.text,
                                prompt_tokens=out.prompt_tokens,
                                output_tokens=out.output_tokens,
                                finish_reason=out.finish_reason,
                                queue_wait_ms=out.queue_wait_ms,
                                prefill_ms=out.prefill_ms,
                                decode_ms=out.decode_ms,
                                # engines without a prefix cache report none
                                cached_tokens=getattr(out, "cached_tokens", 0),
                                logprobs=None if entries is None else
                                format_logprobs(entries, engine.tokenizer),
                                cumulative_logprob=getattr(
                                    out, "cumulative_logprob", None),
                            ),
                        )
        except BaseException as exc:  # noqa: BLE001 — engine died: fail fast
            logger.exception("engine thread crashed; failing %d in-flight requests",
                             len(self._futures))
            self._fatal = exc
            for request_id in list(self._futures):
                self._resolve_error(
                    request_id, RuntimeError(f"engine thread crashed: {exc}")
                )
        finally:
            if self.tp_size > 1:
                try:
                    self._broadcast_ctrl(("stop", None))
                except Exception:  # noqa: BLE001
                    pass

    def _broadcast_ctrl(self, msg: Any) -> None:
        import torch.distributed as dist

        dist.broadcast_object_list([msg], src=0, group=self._ctrl_group)

    def _resolve(self, request_id: str, result: _FinishedRequest) -> None:
        fut = self._futures.get(request_id)
        if fut is not None and self._loop is not None:
            self._loop.call_soon_threadsafe(
                lambda: fut.set_result(result) if not fut.done() else None
            )

    def _resolve_error(self, request_id: str, exc: BaseException) -> None:
        fut = self._futures.get(request_id)
        if fut is not None and self._loop is not None:
            self._loop.call_soon_threadsafe(
                lambda: fut.set_exception(exc) if not fut.done() else None
            )


def _tp_follower_main(
    rank: int,
    tp_size: int,
    engine_kwargs: Dict[str, Any],
    master_port: int,
) -> None:
    """Follower process (TP rank > 0): replicate the rank-0 engine and
    execute the broadcast op stream. Deterministic scheduling + identical
    logits (post all-reduce) + same-seed samplers keep all replicas in
    lockstep without per-token synchronisation."""
    import torch
    import torch.distributed as dist

    from llmq_amd.engine.config import EngineConfig
    from llmq_amd.engine.engine import LLMEngine
    from llmq_amd.parallel import init_tp

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(master_port))
    use_gpu = torch.cuda.is_available()
    if use_gpu:
        torch.cuda.set_device(rank)
    init_tp(tp_size, rank=rank)
    cfg = EngineConfig(**engine_kwargs)
    if use_gpu:
        cfg.device = f"cuda:{rank}"
    engine = LLMEngine(cfg, tp_rank=rank, tp_size=tp_size)
    ctrl = dist.new_group(list(range(tp_size)), backend="gloo")
    while True:
        buf: List[Any] = [None]
        dist.broadcast_object_list(buf, src=0, group=ctrl)
        kind, payload = buf[0]
        if kind == "stop":
            break
        for request_id, prompt, params in payload:
            try:
                engine.add_request(request_id, prompt=prompt, params=params)
            except ValueError:
                pass  # rank 0 rejected it too (deterministic)
        engine.step()


class EngineWorker(BaseWorker):
    """The VLLMWorker replacement (reference vllm_worker.py:11-201)."""

    def __init__(
        self,
        queue_name: str,
        model: str,
        tensor_parallel_size: Optional[int] = None,
        max_num_seqs: Optional[int] = None,
        max_model_len: Optional[int] = None,
        prefetch: Optional[int] = None,
        pipeline: Optional[PipelineConfig] = None,
        stage_name: Optional[str] = None,
        stage_config: Optional[Dict[str, Any]] = None,
        config: Optional[Config] = None,
        engine_overrides: Optional[Dict[str, Any]] = None,
    ):
        self.model = model
        self._tp = tensor_parallel_size
        self._max_num_seqs = max_num_seqs
        self._max_model_len = max_model_len
        self.stage_config = stage_config or {}
        self.engine_overrides = engine_overrides or {}
        self.bridge: Optional[AsyncEngineBridge] = None
        self._followers: List[Any] = []
        self._stats: Dict[str, _FinishedRequest] = {}
        super().__init__(
            queue_name,
            config=config,
            pipeline=pipeline,
            stage_name=stage_name,
            prefetch=prefetch,
        )

    def _generate_worker_id(self) -> str:
        # reference format: model basename + uuid8 (vllm_worker.py:39-50)
        base = self.model.split("/")[-1].lower()
        return f"engine-{base}-{uuid.uuid4().hex[:8]}"

    # -- engine lifecycle ------------------------------------------------

    def _resolve_tp(self) -> int:
        if self._tp is not None:
            return self._tp
        if "tensor_parallel_size" in self.stage_config:
            return int(self.stage_config["tensor_parallel_size"])
        # reference auto-TP = all visible GPUs (vllm_worker.py:62-89)
        import torch

        if torch.cuda.is_available():
            vis = os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get(
                "CUDA_VISIBLE_DEVICES"
            )
            if vis is not None:
                return max(1, len([d for d in vis.split(",") if d.strip()]))
            return max(1, torch.cuda.device_count())
        return 1

    def _engine_kwargs(self, tp: int) -> Dict[str, Any]:
        kwargs: Dict[str, Any] = dict(
            model=self.model,
            max_num_seqs=self._max_num_seqs or self.config.max_num_seqs,
            gpu_memory_utilization=self.config.gpu_memory_utilization,
            tensor_parallel_size=tp,
        )
        max_len = self._max_model_len or self.config.max_model_len
        if max_len:
            kwargs["max_model_len"] = max_len
        if self.config.enable_prefix_caching:
            kwargs["enable_prefix_caching"] = True
        # a pipeline stage's own setting wins over the environment's
        quantization = self.stage_config.get("quantization", self.config.quantization)
        if quantization != "none":
            kwargs["quantization"] = str(quantization)
        kwargs.update(self.engine_overrides)
        return kwargs

    async def _initialize_processor(self) -> None:
        import torch

        tp = self._resolve_tp()
        master_port = int(os.environ.get("LLMQ_TP_MASTER_PORT", "29517"))
        engine_kwargs = self._engine_kwargs(tp)
        if tp > 1:
            import torch.multiprocessing as mp

            ctx = mp.get_context("spawn")
            for rank in range(1, tp):
                p = ctx.Process(
                    target=_tp_follower_main,
                    args=(rank, tp, engine_kwargs, master_port),
                    daemon=True,
                )
                p.start()
                self._followers.append(p)

        def factory() -> Any:
            from llmq_amd.engine.config import EngineConfig
            from llmq_amd.engine.engine import LLMEngine
            from llmq_amd.parallel import init_tp

            if tp > 1:
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(master_port))
                if torch.cuda.is_available():
                    torch.cuda.set_device(0)
                init_tp(tp, rank=0)
            cfg = EngineConfig(**engine_kwargs)
            if tp > 1 and torch.cuda.is_available():
                cfg.device = "cuda:0"
            return LLMEngine(cfg, tp_rank=0, tp_size=tp)

        self.bridge = AsyncEngineBridge(factory, tp_size=tp)
        await self.bridge.start()
        logger.info(
            "engine worker %s ready: model=%s tp=%d max_num_seqs=%s",
            self.worker_id, self.model, tp, engine_kwargs["max_num_seqs"],
        )

    async def _cleanup_processor(self) -> None:
        if self.bridge is not None:
            self.bridge.shutdown()
        for p in self._followers:
            p.join(timeout=30.0)
            if p.is_alive():
                p.terminate()
        self._followers.clear()

    # -- job processing --------------------------------------------------

    def _sampling_params(self, job: Job) -> SamplingParams:
        stage = self.stage_config

        def pick(job_val: Any, stage_key: str, default: Any) -> Any:
            if job_val is not None:
                return job_val
            if stage.get(stage_key) is not None:
                return stage[stage_key]
            return default

        stop = job.stop if job.stop else stage.get("stop")
        lp = pick(job.logprobs, "logprobs", None)
        return SamplingParams(
            temperature=float(pick(job.temperature, "temperature", DEFAULT_TEMPERATURE)),
            top_p=float(pick(job.top_p, "top_p", 1.0)),
            top_k=int(pick(job.top_k, "top_k", 0)),
            max_tokens=int(pick(job.max_tokens, "max_tokens", self.config.max_tokens)),
            stop=list(stop) if stop else None,
            seed=job.seed,
            repetition_penalty=float(
                pick(job.repetition_penalty, "repetition_penalty", 1.0)),
            presence_penalty=float(
                pick(job.presence_penalty, "presence_penalty", 0.0)),
            frequency_penalty=float(
                pick(job.frequency_penalty, "frequency_penalty", 0.0)),
            min_p=float(pick(job.min_p, "min_p", 0.0)),
            logprobs=None if lp is None else int(lp),
        )

    def _format_prompt(self, job: Job) -> str:
        assert self.bridge is not None and self.bridge.engine is not None
        tokenizer = self.bridge.engine.tokenizer
        if job.messages is not None:
            return tokenizer.apply_chat_template(job.messages)
        prompt = job.get_formatted_prompt()
        if job.chat_mode:
            return tokenizer.apply_chat_template(
                [{"role": "user", "content": prompt}]
            )
        return prompt

    async def _process_job(self, job: Job) -> str:
        assert self.bridge is not None
        prompt = self._format_prompt(job)
        params = self._sampling_params(job)
        # At-least-once redelivery can overlap the original in-flight
        # request; suffix a nonce so engine request ids stay unique.
        request_id = f"{job.id}#{uuid.uuid4().hex[:6]}"
        t0 = time.perf_counter()
        finished = await self.bridge.generate(request_id, prompt, params)
        self._stats[job.id] = finished
        logger.debug(
            "job %s: %d prompt + %d output tokens in %.1f ms",
            job.id, finished.prompt_tokens, finished.output_tokens,
            (time.perf_counter() - t0) * 1e3,
        )
        return finished.text

    def _build_result(self, job: Job, output: str, duration_ms: float) -> Result:
        result = super()._build_result(job, output, duration_ms)
        stats = self._stats.pop(job.id, None)
        if stats is not None:
            result.prompt_tokens = stats.prompt_tokens
            result.cached_tokens = stats.cached_tokens
            result.output_tokens = stats.output_tokens
            result.finish_reason = stats.finish_reason
            result.queue_wait_ms = stats.queue_wait_ms
            result.prefill_ms = stats.prefill_ms
            result.decode_ms = stats.decode_ms
            result.logprobs = getattr(stats, "logprobs", None)
            result.cumulative_logprob = getattr(stats, "cumulative_logprob", None)
        return result
