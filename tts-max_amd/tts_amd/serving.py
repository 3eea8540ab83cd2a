"""Continuous-batching serving on the MI355X engine.

The reference serves its SpeechLM through vLLM for RLHF rollouts (``trl vllm-serve``,
``run_rlhf_combine.sh:60``) and the ``--use_vllm`` CLI path (``tools/serving/inference.py:
83-95``, ``inferencing.py:75-92``: ``LLM.generate(prompt_token_ids=..., sampling_params=...)``
-> ``outputs[0].outputs[0].token_ids``).  This module provides the same duck-typed surface
backed by the engine's slot API (``tts_slots_*``):

* ``ContinuousBatcher`` — S persistent decode rows; queued requests are admitted into free
  rows between decode chunks and retired when they stop (EOS / max_tokens), so long and short
  utterances share the GPU without padding or waiting for the longest one.  Every request's
  tokens equal a batch-1 generate of its prompt with the batcher's settings (up to 256 rows; above
  64 the step sums K in another order and the equality holds where margins are decisive, see
  tts_slots_open in include/tts_mi355x.h) (rows never mix;
  tests/test_gpu_serving.py).
* ``LLM`` — vLLM-shaped facade: ``generate(prompt_token_ids=list | list[list], sampling_params)``.
* ``create_app`` — a FastAPI app (``POST /generate``: ``{"prompt_token_ids": [...],
  "max_tokens": n}`` -> ``{"token_ids": [...]}``) over one batcher; run with uvicorn.

Settings (penalty, EOS, min_tokens, sampling) are per batcher, as the reference's
InferenceSettings are per process; requests differ in prompt and max_tokens.

``per_request=True`` (``ContinuousBatcher``, ``LLM``) lifts that: every request may carry its
own ``RequestSettings`` (``tts_slots_open_per_request`` / ``tts_slots_add_params``: the captured
step reads each row's settings from a device table), so callers that differ in temperature,
top_k, top_p, penalties, min_tokens or stop id share one running batch, as vLLM's do.  Each
request's tokens still equal a uniform batcher's with that request's settings and seed
(tests/test_gpu_slots_per_request.py).
"""

from __future__ import annotations

import collections
import ctypes
import dataclasses
import threading
from concurrent.futures import Future
from typing import Any, Sequence

import numpy as np
import torch

from . import _lib

try:  # the HTTP front end is optional (fastapi / pydantic are in the image)
    from pydantic import BaseModel as _BaseModel

    class GenerateRequest(_BaseModel):
        prompt_token_ids: list[int]
        max_tokens: int = 16
        # the request's own settings (a per-request batcher only; all None: the batcher's defaults)
        temperature: float | None = None
        top_k: int | None = None
        top_p: float | None = None
        repetition_penalty: float | None = None
        frequency_penalty: float | None = None
        min_new_tokens: int | None = None
        eos_token_id: int | None = None
        seed: int | None = None
except ImportError:  # pragma: no cover
    GenerateRequest = None


@dataclasses.dataclass
class RequestSettings:
    """One request's sampling settings (a per-request batcher).  temperature 0 = greedy
    (do_sample = temperature > 0, inferencing.py:100)."""
    temperature: float = 0.0
    top_k: int = 50
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    frequency_penalty: float = 0.0
    min_new_tokens: int = 0
    eos_token_id: int = -1

    @property
    def do_sample(self) -> bool:
        return self.temperature > 0

    def gen_params(self) -> "_lib.GenParams":
        return _lib.GenParams(max_length=0, min_new_tokens=int(self.min_new_tokens), eos_token_id=int(self.eos_token_id),
                              do_sample=1 if self.do_sample else 0, repetition_penalty=float(self.repetition_penalty),
                              temperature=float(self.temperature), top_p=float(self.top_p), top_k=int(self.top_k),
                              seed=0, frequency_penalty=float(self.frequency_penalty))


@dataclasses.dataclass
class _Req:
    prompt: list[int]
    max_new: int
    future: Future
    seed: int | None = None  # the request's own sampling key (vLLM SamplingParams.seed)
    settings: RequestSettings | None = None  # the request's own settings (per-request batcher)


class ContinuousBatcher:
    def __init__(self, lm, n_slots: int, eos_token_id: int = -1, min_new_tokens: int = 0,
                 repetition_penalty: float = 1.0, do_sample: bool = False, temperature: float = 1.0,
                 top_k: int = 50, top_p: float = 1.0, frequency_penalty: float = 0.0, seed: int | None = None,
                 chunk: int = 8, per_request: bool = False):
        if n_slots < 1 or n_slots > lm.max_batch:
            raise ValueError(f"n_slots {n_slots} outside [1, max_batch={lm.max_batch}]")
        if (do_sample or per_request) and seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        self.lm, self.S, self.chunk = lm, n_slots, chunk
        self.per_request = per_request  # requests may carry their own RequestSettings (the rest: defaults)
        self._p = _lib.GenParams(max_length=0, min_new_tokens=min_new_tokens, eos_token_id=eos_token_id,
                                 do_sample=1 if do_sample else 0, repetition_penalty=repetition_penalty,
                                 temperature=temperature, top_p=top_p, top_k=top_k, seed=seed or 0,
                                 frequency_penalty=frequency_penalty)
        self._queue: collections.deque[_Req] = collections.deque()  # (O(1) admission at any slot count)
        self._slot_req: list[_Req | None] = [None] * n_slots
        self._lock = threading.Lock()
        self._wake = threading.Event()
        self._stop = False
        self._opened = False
        self._thread: threading.Thread | None = None
        self._buf = np.zeros(lm.max_seq_len, dtype=np.int32)
        self.error: BaseException | None = None  # set when the engine loop failed (batcher dead)

    # ------------------------------------------------------------------ requests -------
    def submit(self, prompt_ids: Sequence[int], max_new_tokens: int, seed: int | None = None,
               settings: RequestSettings | None = None) -> Future:
        """Queues a request.  `seed` fixes the request's sampling stream (vLLM per-request
        seed); None draws a fresh stream per request from the batcher's seed.  `settings`: the
        request's own sampling settings (a per_request batcher only; None: the batcher's)."""
        if settings is not None and not self.per_request:
            raise ValueError("per-request settings need ContinuousBatcher(..., per_request=True)")
        fut: Future = Future()
        if self.error is not None:
            fut.set_exception(RuntimeError(f"batcher stopped after an engine error: {self.error}"))
            return fut
        with self._lock:
            self._queue.append(_Req(list(map(int, prompt_ids)), int(max_new_tokens), fut,
                                    None if seed is None else int(seed) & (2**64 - 1), settings))
        self._wake.set()
        return fut

    def busy(self) -> bool:
        with self._lock:
            return bool(self._queue) or any(r is not None for r in self._slot_req)

    def generate(self, prompts: Sequence[Sequence[int]], max_new_tokens: int | Sequence[int],
                 seed: int | None | Sequence[int | None] = None,
                 settings: RequestSettings | None | Sequence[RequestSettings | None] = None) -> list[list[int]]:
        """Blocking: all prompts through the continuous batch, results in order.  seed and
        settings: one for all prompts, or a list with one entry per prompt."""
        if isinstance(max_new_tokens, int):
            max_new_tokens = [max_new_tokens] * len(prompts)
        seeds = list(seed) if isinstance(seed, (list, tuple)) else [seed] * len(prompts)
        sets = list(settings) if isinstance(settings, (list, tuple)) else [settings] * len(prompts)
        futs = [self.submit(p, n, sd, st) for p, n, sd, st in zip(prompts, max_new_tokens, seeds, sets)]
        if self._thread is None:  # no background loop: drive it here
            while not all(f.done() for f in futs):
                self._run_guarded()
        return [f.result() for f in futs]

    # ------------------------------------------------------------------ engine loop ----
    def _open(self):
        if not self._opened or self.lm._slot_batcher is not self:
            opener = self.lm._lib.tts_slots_open_per_request if self.per_request else self.lm._lib.tts_slots_open
            _lib.check(opener(self.lm._h, ctypes.byref(self._p), self.S, None))
            self.lm._slot_batcher = self
            self._opened = True

    def _fail_all(self, ex: BaseException) -> None:
        """An engine error ends the batcher: every active and queued request fails with it
        (no future is left pending), and later submissions fail at once."""
        self.error = ex
        with self._lock:
            reqs = [r for r in self._slot_req if r is not None] + list(self._queue)
            self._slot_req = [None] * self.S
            self._queue.clear()
        for r in reqs:
            if not r.future.done():
                r.future.set_exception(ex)
        if self.lm._slot_batcher is self:
            self.lm._slot_batcher = None
        self._opened = False

    def _run_guarded(self) -> int:
        try:
            return self.run_once()
        except Exception as ex:  # noqa: BLE001 (TtsError and anything else: fail loudly, never hang)
            self._fail_all(ex)
            return 0

    def run_once(self) -> int:
        """Admit queued requests into free slots, run one chunk of decode steps, retire the
        stopped sequences.  Returns the number of rows still generating."""
        with self.lm.lock:
            return self._run_once_locked()

    def _run_once_locked(self) -> int:
        self._open()
        h, L = self.lm._h, self.lm._lib
        pi32 = ctypes.POINTER(ctypes.c_int32)
        with self._lock:
            for s in range(self.S):
                if self._slot_req[s] is None and self._queue:
                    r = self._queue.popleft()
                    arr = np.ascontiguousarray(np.asarray(r.prompt, dtype=np.int32))
                    try:
                        if r.settings is not None:
                            gp = r.settings.gen_params()
                            sd = None if r.seed is None else ctypes.byref(ctypes.c_uint64(r.seed))
                            _lib.check(L.tts_slots_add_params(h, s, arr.ctypes.data_as(pi32), len(arr), r.max_new,
                                                              ctypes.byref(gp), sd))
                        elif r.seed is None:
                            _lib.check(L.tts_slots_add(h, s, arr.ctypes.data_as(pi32), len(arr), r.max_new))
                        else:
                            _lib.check(L.tts_slots_add_seeded(h, s, arr.ctypes.data_as(pi32), len(arr), r.max_new,
                                                              r.seed))
                    except _lib.TtsError as ex:  # bad request: fail it, keep serving
                        r.future.set_exception(ex)
                        continue
                    self._slot_req[s] = r
        act = ctypes.c_int32(0)
        if any(r is not None for r in self._slot_req):
            _lib.check(L.tts_slots_step(h, self.chunk, ctypes.byref(act)))
        n, fin = ctypes.c_int32(0), ctypes.c_int32(0)
        for s, r in enumerate(self._slot_req):
            if r is None:
                continue
            _lib.check(L.tts_slots_read(h, s, self._buf.ctypes.data_as(pi32), len(self._buf), ctypes.byref(n),
                                        ctypes.byref(fin)))
            if fin.value:
                r.future.set_result(self._buf[:n.value].tolist())
                _lib.check(L.tts_slots_release(h, s))
                self._slot_req[s] = None
        return act.value

    def start(self):
        """Serve from a background thread (one engine = one thread, as the C ABI requires)."""
        if self._thread is not None:
            return

        def loop():
            while not self._stop:
                busy = any(r is not None for r in self._slot_req)
                with self._lock:
                    busy = busy or bool(self._queue)
                if not busy:
                    self._wake.wait(0.05)
                    self._wake.clear()
                    continue
                self._run_guarded()
                if self.error is not None:
                    return

        self._thread = threading.Thread(target=loop, name="tts-mi355x-batcher", daemon=True)
        self._thread.start()

    def close(self):
        self._stop = True
        self._wake.set()
        if self._thread is not None:
            self._thread.join()
            self._thread = None


@dataclasses.dataclass
class CompletionOutput:
    token_ids: list[int]


@dataclasses.dataclass
class RequestOutput:
    prompt_token_ids: list[int]
    outputs: list[CompletionOutput]


class LLM:
    """vLLM-shaped facade (inferencing.py:75-92): one ContinuousBatcher per distinct
    SamplingParams configuration, or (per_request=True) one batcher that serves every
    SamplingParams, each request with its own settings in the shared batch."""

    def __init__(self, lm, n_slots: int = 16, chunk: int = 8, per_request: bool = False):
        self.lm, self.n_slots, self.chunk, self.per_request = lm, n_slots, chunk, per_request
        self._batchers: dict[tuple, ContinuousBatcher] = {}

    @staticmethod
    def _settings_key(sp: Any) -> tuple:
        temperature = float(getattr(sp, "temperature", 1.0) or 0.0)
        stop = list(getattr(sp, "stop_token_ids", None) or [])
        if len(stop) > 1:
            raise NotImplementedError("one stop token id is supported")
        if float(getattr(sp, "presence_penalty", 0.0) or 0.0) != 0.0:
            raise NotImplementedError("vLLM presence_penalty is not implemented")
        top_k = int(getattr(sp, "top_k", -1) or -1)
        if temperature > 0 and top_k <= 0:
            raise NotImplementedError("full-vocabulary sampling (vLLM top_k=-1) is not built; pass top_k")
        return (temperature, stop[0] if stop else -1, int(getattr(sp, "min_tokens", 0) or 0),
                float(getattr(sp, "repetition_penalty", 1.0) or 1.0), top_k, float(getattr(sp, "top_p", 1.0) or 1.0),
                float(getattr(sp, "frequency_penalty", 0.0) or 0.0))

    @classmethod
    def _request_settings(cls, sp: Any) -> RequestSettings:
        key = cls._settings_key(sp)
        return RequestSettings(temperature=key[0], eos_token_id=key[1], min_new_tokens=key[2], repetition_penalty=key[3],
                               top_k=key[4] if key[4] > 0 else 50, top_p=key[5], frequency_penalty=key[6])

    def _shared_batcher(self) -> ContinuousBatcher:
        old = self._batchers.get(())
        if old is not None and old.error is not None:
            old.close()
            del self._batchers[()]
        if () not in self._batchers:
            self._batchers[()] = ContinuousBatcher(self.lm, self.n_slots, chunk=self.chunk, per_request=True)
        return self._batchers[()]

    def _batcher(self, sp: Any) -> ContinuousBatcher:
        key = self._settings_key(sp)
        temperature, top_k = key[0], key[4]
        old = self._batchers.get(key)
        if old is not None and old.error is not None:  # a batcher that died on an engine error:
            old.close()                                 # replace it instead of failing every later call
            del self._batchers[key]
        if key not in self._batchers:
            for b in self._batchers.values():  # one slot batch open per engine at a time
                b._opened = False
            self._batchers = {}
            self._batchers[key] = ContinuousBatcher(
                self.lm, self.n_slots, eos_token_id=key[1], min_new_tokens=key[2], repetition_penalty=key[3],
                do_sample=temperature > 0, temperature=temperature or 1.0, top_k=top_k if top_k > 0 else 50,
                top_p=key[5], frequency_penalty=key[6], seed=None, chunk=self.chunk)
        return self._batchers[key]

    def generate(self, prompt_token_ids: Sequence[int] | Sequence[Sequence[int]], sampling_params: Any = None,
                 **unused) -> list[RequestOutput]:
        prompts = prompt_token_ids
        if prompts and isinstance(prompts[0], (int, np.integer)):
            prompts = [prompts]
        if self.per_request:  # one batcher; sampling_params may be a list, one entry per prompt (as vLLM)
            sps = list(sampling_params) if isinstance(sampling_params, (list, tuple)) else [sampling_params] * len(prompts)
            if len(sps) != len(prompts):
                raise ValueError("sampling_params: one entry per prompt")
            outs = self._shared_batcher().generate(
                prompts, [int(getattr(sp, "max_tokens", 16)) for sp in sps],
                seed=[getattr(sp, "seed", None) for sp in sps], settings=[self._request_settings(sp) for sp in sps])
            return [RequestOutput(prompt_token_ids=list(p), outputs=[CompletionOutput(token_ids=o)])
                    for p, o in zip(prompts, outs)]
        b = self._batcher(sampling_params)
        outs = b.generate(prompts, int(getattr(sampling_params, "max_tokens", 16)),
                          seed=getattr(sampling_params, "seed", None))
        return [RequestOutput(prompt_token_ids=list(p), outputs=[CompletionOutput(token_ids=o)])
                for p, o in zip(prompts, outs)]


def create_app(batcher: ContinuousBatcher):
    """FastAPI app over a started batcher: POST /generate {"prompt_token_ids", "max_tokens"}."""
    import asyncio

    from fastapi import FastAPI, HTTPException

    app = FastAPI(title="tts-mi355x")
    batcher.start()

    @app.post("/generate")
    async def generate(req: GenerateRequest):
        if not req.prompt_token_ids or req.max_tokens < 1:
            raise HTTPException(status_code=400, detail="empty prompt or max_tokens < 1")
        own = {k: getattr(req, k) for k in ("temperature", "top_k", "top_p", "repetition_penalty", "frequency_penalty",
                                            "min_new_tokens", "eos_token_id") if getattr(req, k) is not None}
        settings = None
        if own:
            if not batcher.per_request:
                raise HTTPException(status_code=400, detail="this server's batcher takes no per-request settings")
            p = batcher._p  # fields not given: the batcher's defaults
            base = RequestSettings(temperature=p.temperature if p.do_sample else 0.0, top_k=p.top_k, top_p=p.top_p,
                                   repetition_penalty=p.repetition_penalty, frequency_penalty=p.frequency_penalty,
                                   min_new_tokens=p.min_new_tokens, eos_token_id=p.eos_token_id)
            settings = dataclasses.replace(base, **own)
        fut = batcher.submit(req.prompt_token_ids, req.max_tokens, seed=req.seed, settings=settings)
        try:
            ids = await asyncio.wrap_future(fut)
        except Exception as ex:  # engine rejected the request
            raise HTTPException(status_code=400, detail=str(ex))
        return {"token_ids": ids}

    @app.get("/health")
    async def health():
        if batcher.error is not None:
            raise HTTPException(status_code=503, detail=f"engine error: {batcher.error}")
        return {"ok": True}

    return app
