"""On-device LLM generation engine (replaces the reference's OpenAI-compatible
HTTP calls, reference src/core/llm/providers/openai.py:117-121; K6/K7 in
SURVEY §2.3).

Llama-3-class decoder: batched prefill (flash-style MFMA attention) + KV-cache
decode (single-pass online-softmax kernel), on-device sampling, optional
per-token streaming callback (the reference streamed SSE chunks).
Temperature-per-mode mirrors reference generator.py:262-267
(fast=0.0, balanced=0.3, quality=0.2, creative=0.7).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, Iterator

import torch

from sentio_amd import ops
from sentio_amd.engines.configs import get_model_config
from sentio_amd.engines.bpe import get_tokenizer
from sentio_amd.engines.tokenizer import EOS_ID
from sentio_amd.engines.transformer import (KVCache, Transformer,
                                            check_kv_dtype, write_kv_scales)

MODE_TEMPERATURE = {"fast": 0.0, "balanced": 0.3, "quality": 0.2, "creative": 0.7}


@dataclass(frozen=True)
class SamplingParams:
    """Per-request sampling controls.  top_k = 0 and top_p = 1.0 switch the
    filters off; seed = None lets the engine derive one."""

    temperature: float = 0.3
    top_k: int = 0
    top_p: float = 1.0
    seed: int | None = None
    # a Grammar or a GrammarHandle of the engine: constrained decoding
    grammar: Any = None

    @property
    def filtered(self) -> bool:
        """True when the request needs the per-row nucleus kernel
        (ops.sample_filtered) instead of the default sampling path."""
        return (int(self.top_k or 0) > 0 or float(self.top_p) < 1.0
                or self.seed is not None)


@dataclass(frozen=True, eq=False)
class GrammarHandle:
    """A grammar registered with an engine: where its states sit in the
    engine-wide table.  `min_tokens` = dist[start], the smallest token
    budget a request with this grammar can have."""

    index: int
    start: int          # global start state
    n_states: int       # with DONE
    min_tokens: int
    grammar: Any


class SlotSampler:
    """Per-slot sampling state of a continuous-batching session: the [S]
    device arrays ops.sample_slots reads (temperature, top_k, top_p, seed,
    active) and the step counter it advances.  admit() is the only
    host-to-device traffic; a decode step is one kernel launch that writes
    the loop's `cur` buffer in place."""

    def __init__(self, engine: "GeneratorEngine", slots: int):
        self.engine = engine
        self.slots = int(slots)
        dev = engine.device
        S = self.slots
        self.temperature = torch.zeros(S, dtype=torch.float32, device=dev)
        self.top_k = torch.zeros(S, dtype=torch.int32, device=dev)
        self.top_p = torch.ones(S, dtype=torch.float32, device=dev)
        self.seed = torch.zeros(S, dtype=torch.int64, device=dev)
        self.step = torch.zeros(S, dtype=torch.int32, device=dev)
        self.active = torch.zeros(S, dtype=torch.uint8, device=dev)
        # automaton state and remaining budget of constrained slots;
        # state = -1: the slot samples unconstrained
        self.state = torch.full((S,), -1, dtype=torch.int32, device=dev)
        self.left = torch.zeros(S, dtype=torch.int32, device=dev)
        self._constrained: set[int] = set()

    @torch.inference_mode()
    def admit(self, rows: list[int], params: list[SamplingParams],
              max_new: list[int] | None = None) -> None:
        """Write each request's parameters into its slot: step = 0,
        active = 1.  A request without a seed gets engine.derive_seed().
        A request with a grammar starts at the grammar's start state with
        left = its max_new entry (ValueError when that is below the
        grammar's shortest completion); the others get state = -1."""
        rows = [int(r) for r in rows]
        if any(r < 0 or r >= self.slots for r in rows) \
                or len(set(rows)) != len(rows):
            raise ValueError(f"bad slot rows {rows} for {self.slots} slots")
        if len(params) != len(rows):
            raise ValueError(f"{len(params)} parameter sets for "
                             f"{len(rows)} rows")
        if not rows:
            return
        handles = [self.engine.resolve_grammar(p.grammar) for p in params]
        budgets = [0] * len(rows)
        if any(h is not None for h in handles):
            if max_new is None or len(max_new) != len(rows):
                raise ValueError("constrained slots need max_new per row")
            for i, h in enumerate(handles):
                if h is not None:
                    budgets[i] = int(max_new[i])
                    self.engine.check_grammar_budget(h, budgets[i])
        dev = self.engine.device
        seeds = [int(p.seed) if p.seed is not None
                 else self.engine.derive_seed() for p in params]
        idx = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.temperature[idx] = torch.tensor(
            [float(p.temperature) for p in params], dtype=torch.float32,
            device=dev)
        self.top_k[idx] = torch.tensor(
            [int(p.top_k or 0) for p in params], dtype=torch.int32,
            device=dev)
        self.top_p[idx] = torch.tensor(
            [float(p.top_p) for p in params], dtype=torch.float32,
            device=dev)
        self.seed[idx] = torch.tensor(seeds, dtype=torch.int64, device=dev)
        self.step[idx] = 0
        self.active[idx] = 1
        self.state[idx] = torch.tensor(
            [h.start if h is not None else -1 for h in handles],
            dtype=torch.int32, device=dev)
        self.left[idx] = torch.tensor(budgets, dtype=torch.int32, device=dev)
        for r, h in zip(rows, handles):
            if h is not None:
                self._constrained.add(r)
            else:
                self._constrained.discard(r)

    @torch.inference_mode()
    def release(self, row: int) -> None:
        """The slot is free: later sample() calls skip it."""
        self.active[int(row)] = 0
        self._constrained.discard(int(row))

    @torch.inference_mode()
    def sample(self, logits: torch.Tensor, cur: torch.Tensor,
               rows: list[int] | None = None) -> None:
        """Draw one token per active slot into `cur` [S] int64, in place,
        and advance those slots' step counters on the device.  With `rows`:
        the admission call, logits [len(rows), V] scattered to those slots
        (their step-0 draw; ops.sample_slots checks the list for range and
        duplicates).  Without: the per-step call, logits [S, V]."""
        if not self._constrained:
            ops.sample_slots(logits, rows, self.temperature, self.top_k,
                             self.top_p, self.seed, self.step, self.active,
                             cur)
            return
        ops.sample_slots_constrained(
            logits, rows, self.temperature, self.top_k, self.top_p, self.seed,
            self.step, self.active, cur, self.state, self.left,
            self.engine.grammar_tables())


class _DecodeSession:
    """One (batch, cache-size) decode context: preallocated KV cache plus an
    optional hipGraph capture of the whole per-token decode step."""

    def __init__(self, engine: "GeneratorEngine", batch: int, cache_len: int,
                 use_graphs: bool):
        self.engine = engine
        self.cache = engine._new_cache(batch, cache_len)
        self.graph = None
        self.static_tok = None
        self.static_logits = None
        self.use_graphs = use_graphs
        self.batch = batch

    def prefill(self, tokens: torch.Tensor,
                lens: torch.Tensor | None = None) -> torch.Tensor:
        self.cache.seq_lens.zero_()
        engine = self.engine
        if not self.cache.fp8:
            return engine.model.prefill(tokens, self.cache, lens=lens)
        # FP8 session: prompt attention sees exact K/V in a staging cache
        # exactly as long as the prompt; only decode reads quantised rows
        B, S = tokens.shape
        stage = engine._staging_cache(B, S)
        logits = engine.model.prefill(tokens, stage, lens=lens)
        engine._splice_kv(self.cache, list(range(B)), stage.k, stage.v, S)
        self.cache.seq_lens.copy_(stage.seq_lens)
        return logits

    def prefill_with_prefix(self, prefix_ids: list[int],
                            suffix_tokens: torch.Tensor,
                            suffix_lens: torch.Tensor | None = None
                            ) -> torch.Tensor:
        """Copy the (cached) prefix KV into every batch slot, then prefill
        only the suffix (prefix-KV caching: the shared system-prompt +
        instruction header is prefilled ONCE per prefix, not per request)."""
        engine = self.engine
        pk, pv = engine._prefix_kv(tuple(prefix_ids))
        P = len(prefix_ids)
        B, S = suffix_tokens.shape
        # FP8 session: prefix + suffix go through a staging cache of P+S
        dst = engine._staging_cache(B, P + S) if self.cache.fp8 \
            else self.cache
        for i in range(engine.cfg.n_layers):
            dst.k[i][:, :, :P].copy_(pk[i])   # [1,...] broadcasts
            dst.v[i][:, :, :P].copy_(pv[i])
        logits = engine.model.prefill_suffix(suffix_tokens, dst, P,
                                             suffix_lens=suffix_lens)
        if dst is not self.cache:
            engine._splice_kv(self.cache, list(range(B)), dst.k, dst.v, P + S)
            self.cache.seq_lens.copy_(dst.seq_lens)
        return logits

    def _capture(self):
        model = self.engine.model
        dev = self.engine.device
        self.static_tok = torch.zeros(self.batch, 1, dtype=torch.int64,
                                      device=dev)
        # warmup on a side stream (required before capture), then capture.
        # seq_lens must be restored: warmup/capture each advance it.
        saved = self.cache.seq_lens.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model.decode_step(self.static_tok, self.cache)
        torch.cuda.current_stream().wait_stream(s)
        self.cache.seq_lens.copy_(saved)
        self.graph = torch.cuda.CUDAGraph()
        # relaxed capture: concurrent engine work on OTHER threads
        # (pipelined retrieval, encoder graph replays, allocator traffic)
        # must not invalidate this capture — global/thread_local modes abort
        # on foreign allocator calls; the captured region itself only
        # contains this stream's decode ops
        from sentio_amd.engines.graphed import capture_gc_guard

        with capture_gc_guard(), \
                torch.cuda.graph(self.graph, capture_error_mode="relaxed"):
            self.static_logits = model.decode_step(self.static_tok, self.cache)
        self.cache.seq_lens.copy_(saved)

    def decode_step(self, tok: torch.Tensor) -> torch.Tensor:
        if not self.use_graphs:
            return self.engine.model.decode_step(tok.view(self.batch, 1),
                                                 self.cache)
        if self.graph is None:
            self._capture()
        self.static_tok.copy_(tok.view(self.batch, 1))
        self.graph.replay()
        return self.static_logits


class GeneratorEngine:
    def __init__(self, model: str = "llama3-8b", device: str = "cpu",
                 dtype: str = "bf16", max_seq: int = 4096, seed: int = 303,
                 tp=None, kv_cache_dtype: str = "bf16"):
        self.cfg = get_model_config(model)
        # "fp8": session caches hold e4m3fn bytes (half the HBM and half the
        # bytes a decode step streams); prefill and the prefix store stay in
        # the model dtype.  Raises here for a model the FP8 kernel cannot
        # serve, not at the first step.
        self.kv_cache_dtype = check_kv_dtype(kv_cache_dtype, self.cfg)
        self.device = device
        self.max_seq = min(max_seq, self.cfg.max_seq)
        self.tokenizer = get_tokenizer()
        self.model = Transformer(self.cfg, device=device, dtype=dtype,
                                 seed=seed, tp=tp)
        if self.kv_cache_dtype == "fp8" and device != "cpu" \
                and self.model.dtype != torch.bfloat16:
            raise ValueError("the fp8 KV cache needs a bf16 model on the GPU")
        # one set of static scales, [4, Hkv] per layer (k_scale, v_scale and
        # their reciprocals), shared by every session cache: set_kv_scales
        # updates them in place, captured decode graphs read the new values
        self._kv_scales = None
        if self.kv_cache_dtype == "fp8":
            self._kv_scales = [
                torch.ones(4, self.model.hkv_local, dtype=torch.float32,
                           device=device)
                for _ in range(self.cfg.n_layers)]
        self._step_seed = 0
        self._derived_seeds = 0     # derive_seed()'s own counter
        import threading

        self._gen_lock = threading.Lock()   # decode sessions hold static state
        # registered grammars: one append-only table, global state numbers
        self._grammar_handles: dict = {}
        self._grammar_host: list = []       # per grammar (next, mask, dist)
        self._grammar_states = 0
        self._grammar_tables = None         # ops.GrammarTables on the device

    def _new_cache(self, batch: int, max_seq: int) -> KVCache:
        """A session cache, in the engine's KV dtype."""
        return KVCache(self.cfg, batch, max_seq, self.device, self.model.dtype,
                       n_kv_heads=self.model.hkv_local,
                       kv_dtype=self.kv_cache_dtype, scales=self._kv_scales)

    def _staging_cache(self, batch: int, max_seq: int) -> KVCache:
        """A prefill target in the model dtype, whatever the KV dtype."""
        return KVCache(self.cfg, batch, max_seq, self.device, self.model.dtype,
                       n_kv_heads=self.model.hkv_local)

    def _splice_kv(self, cache: KVCache, rows: list[int], src_k: list,
                   src_v: list, S: int, sel: torch.Tensor | None = None
                   ) -> None:
        """Copy the first S rows of per-layer staging K/V [n, Hkv, >=S, D]
        into cache rows `rows`: an index copy for a bf16 cache, the
        quantising ops.kv_store_fp8 for an fp8 one.  `sel` picks a subset
        of the staging batch."""
        if cache.fp8:
            B = cache.k[0].shape[0]
            if any(r < 0 or r >= B for r in rows) \
                    or len(set(rows)) != len(rows):
                raise ValueError(f"bad cache rows {rows} for batch {B}")
            rows_t = torch.tensor(rows, dtype=torch.int32, device=self.device)
        else:
            rows_t = torch.tensor(rows, dtype=torch.int64, device=self.device)
        for li in range(self.cfg.n_layers):
            k, v = src_k[li], src_v[li]
            if sel is not None:
                k, v = k[sel], v[sel]
            if cache.fp8:
                sc = cache.scales[li]
                ops.kv_store_fp8(k, v, cache.k[li], cache.v[li], rows_t, S,
                                 sc[2], sc[3])
            else:
                cache.k[li][rows_t, :, :S] = k[:, :, :S]
                cache.v[li][rows_t, :, :S] = v[:, :, :S]

    # ----- FP8 KV cache: scales -----
    @property
    def kv_bytes_per_token(self) -> int:
        """KV-cache bytes one token occupies on this device, for the
        engine's KV dtype at its serving width (bf16: 2 bytes, fp8: 1; a CPU
        engine's fp32 stand-in tensors are not what is reported)."""
        width = 1 if self.kv_cache_dtype == "fp8" else 2
        return (2 * self.cfg.n_layers * self.model.hkv_local
                * self.cfg.head_dim * width)

    def set_kv_scales(self, k_scales, v_scales) -> None:
        """Per-layer [Hkv] K and V scales of the fp8 cache, updated in place
        with their reciprocals; no decode graph needs recapturing."""
        if self._kv_scales is None:
            raise ValueError("kv scales exist only with kv_cache_dtype='fp8'")
        with self._gen_lock:
            write_kv_scales(self._kv_scales, k_scales, v_scales)

    @torch.inference_mode()
    def calibrate_kv_scales(self, prompts: list[str], margin: float = 2.0):
        """Static scales from a bf16 prefill of `prompts`: per layer and kv
        head, scale = max(amax * margin / 448, 2**-20) for K and for V.
        Sets them (set_kv_scales) and returns (k_scales, v_scales)."""
        if self._kv_scales is None:
            raise ValueError("kv scales exist only with kv_cache_dtype='fp8'")
        if not prompts:
            raise ValueError("calibration needs at least one prompt")
        with self._gen_lock:
            pre = self.prefill_admission(prompts, [1] * len(prompts))
        tmp, S = pre["tmp"], pre["S"]
        valid = (torch.arange(S, device=self.device)[None, :]
                 < pre["lens"][:, None])[:, None, :, None]
        ks, vs = [], []
        for li in range(self.cfg.n_layers):
            for src, dst in ((tmp.k[li], ks), (tmp.v[li], vs)):
                amax = (src.float().abs() * valid).amax(dim=(0, 2, 3))
                dst.append((amax * (float(margin) / 448.0))
                           .clamp_min(2.0 ** -20).cpu())
        self.set_kv_scales(ks, vs)
        return ks, vs

    # ----- grammar-constrained decoding -----
    def register_grammar(self, grammar) -> GrammarHandle:
        """Build the grammar's token tables (once per distinct grammar) and
        append them to the engine-wide device table.  States are numbered
        globally and the table only grows, so states held by running
        requests stay valid.  At most 32766 states in all."""
        import numpy as np

        from sentio_amd.engines.grammar import MAX_STATES, Grammar

        if not isinstance(grammar, Grammar):
            raise ValueError("register_grammar takes a Grammar")
        key = grammar.pattern or id(grammar)
        with self._gen_lock:
            hit = self._grammar_handles.get(key)
            if hit is not None:
                return hit
            tb = grammar.token_tables(self.tokenizer)
            base, n = self._grammar_states, tb.n_states
            if base + n > MAX_STATES + 1:
                raise ValueError(
                    f"grammar table full: {base} states registered, this "
                    f"grammar needs {n}, the limit is {MAX_STATES + 1}")
            nxt = np.where(tb.next >= 0, tb.next.astype(np.int32) + base,
                           -1).astype(np.int16)
            self._grammar_host.append((nxt, tb.mask, tb.dist))
            self._grammar_states = base + n
            self._grammar_tables = ops.GrammarTables.from_numpy(
                np.concatenate([h[0] for h in self._grammar_host]),
                np.concatenate([h[1] for h in self._grammar_host]),
                np.concatenate([h[2] for h in self._grammar_host]),
                device=self.device)
            handle = GrammarHandle(len(self._grammar_host) - 1,
                                   base + tb.start, n, int(tb.dist[tb.start]),
                                   grammar)
            self._grammar_handles[key] = handle
            return handle

    def resolve_grammar(self, grammar) -> GrammarHandle | None:
        """None, a handle of this engine or a Grammar (registered on first
        use) -> handle."""
        if grammar is None:
            return None
        if isinstance(grammar, GrammarHandle):
            g = grammar.grammar
            if self._grammar_handles.get(g.pattern or id(g)) is not grammar:
                raise ValueError("grammar handle of another engine")
            return grammar
        return self.register_grammar(grammar)

    @staticmethod
    def check_grammar_budget(handle: GrammarHandle, max_new_tokens: int):
        if handle.min_tokens > int(max_new_tokens):
            raise ValueError(
                f"max_new_tokens={int(max_new_tokens)} is below the "
                f"grammar's shortest completion ({handle.min_tokens} tokens)")

    def grammar_tables(self):
        """The current engine-wide ops.GrammarTables (None before the first
        registration)."""
        return self._grammar_tables

    # ----- prefix-KV cache (shared prompt prefixes prefilled once) -----
    _PREFIX_MIN_TOKENS = 64

    def _split_shared_prefix(self, clipped: list[str], prompt_budget: int
                             ) -> tuple[list[int], list[str]]:
        """Split the batch's longest common prompt prefix from the per-prompt
        suffixes such that prefix_ids + encode(suffix, add_bos=False) is
        EXACTLY encode(full prompt) for every prompt.  The cap is computed in
        TOKENS via tokenizer.prefix_split — a char-based cap overshoots the
        budget for multi-byte UTF-8 prefixes (len(prefix_ids) > chars) and
        crashed prefill with negative suffix budgets."""
        import os as _os

        if len(clipped) < 2:
            return [], clipped
        prefix_txt = _os.path.commonprefix(clipped)
        # leave >= 1 suffix char per prompt and >= 8 suffix tokens of budget
        limit_chars = min(len(prefix_txt), min(len(c) for c in clipped) - 1)
        if limit_chars <= 0 or prompt_budget <= 9:
            return [], clipped
        n, prefix_ids = self.tokenizer.prefix_split(
            prefix_txt[:limit_chars], prompt_budget - 8)
        if n <= 0 or not prefix_ids:
            return [], clipped
        return prefix_ids, [c[n:] for c in clipped]

    def _prefix_kv(self, prefix_ids: tuple):
        """Per-prefix KV, computed once with a batch-1 forward and kept in
        HBM (a few tens of MB per distinct prefix; LRU of 4)."""
        store = getattr(self, "_prefix_store", None)
        if store is None:
            store = self._prefix_store = {}
        hit = store.get(prefix_ids)
        if hit is not None:
            return hit
        P = len(prefix_ids)
        tmp = self._staging_cache(1, P)
        toks = torch.tensor([list(prefix_ids)], dtype=torch.int64,
                            device=self.device)
        self.model.forward_hidden(toks, cache=tmp)
        entry = ([k.clone() for k in tmp.k], [v.clone() for v in tmp.v])
        if len(store) >= 4:
            store.pop(next(iter(store)))
        store[prefix_ids] = entry
        return entry

    # ----- hipGraph-captured decode session -----
    # The per-token decode step launches ~10 kernels per layer; on MI355X the
    # wall time at small batch is launch-bound, so the whole step is captured
    # once as a hipGraph and replayed per token (sampling stays outside: its
    # seed changes per step).  Sessions are pooled by (batch, cache size).
    _GRAPHS_ENABLED = True

    def _use_graphs(self) -> bool:
        """Whether a NEW decode session captures its step into a hipGraph
        (the environment is read here, at session creation)."""
        import os

        return (
            self._GRAPHS_ENABLED
            and self.device != "cpu"
            # TP decode: the chunked async all-reduces (parallel/tp.py)
            # are stream-ordered and RCCL supports graph capture, but this
            # environment has no multi-GPU lease to validate the captured
            # collective schedule on real xGMI — graphed TP decode is
            # therefore opt-in (SENTIO_TP_HIPGRAPH=1); the default stays
            # eager, correct by construction.
            and (not self.model.tp.enabled
                 or os.environ.get("SENTIO_TP_HIPGRAPH", "0") == "1")
            and os.environ.get("SENTIO_DISABLE_HIPGRAPH", "0") != "1"
        )

    def _decode_session(self, batch: int, cache_len: int):
        key = (batch, cache_len)
        pool = getattr(self, "_sessions", None)
        if pool is None:
            pool = self._sessions = {}
        if key in pool:
            sess = pool[key]
            sess.cache.seq_lens.zero_()
            return sess
        sess = _DecodeSession(self, batch, cache_len, self._use_graphs())
        pool[key] = sess
        return sess

    # ----- continuous-batching support (serving.ContinuousBatcher) -----
    def make_slot_session(self, slots: int) -> "_DecodeSession":
        """A PRIVATE decode session for the continuous batcher: its KV
        slots persist across requests, so it must never come from (or be
        reset by) the shared _decode_session pool."""
        return _DecodeSession(self, slots, self.max_seq, self._use_graphs())

    def make_slot_sampler(self, slots: int) -> SlotSampler:
        """Per-slot sampling state for a slot session of `slots` rows."""
        return SlotSampler(self, slots)

    @torch.inference_mode()
    def prefill_admission(self, prompts: list[str],
                          max_new_list: list[int]) -> dict:
        """Admission prefill (continuous batching), LOCK-FREE: encode +
        prefill the prompts into a temporary cache on the CALLER's stream.
        Touches only the temp cache and read-only weights, so it may run
        on a side stream CONCURRENTLY with the decode loop's graph
        replays — a joining request's prefill never stalls resident
        requests.  integrate_admission() splices the result into slots."""
        ids_list = []
        for p, mn in zip(prompts, max_new_list):
            budget = max(self.max_seq - mn - 1, 8)
            ids_list.append(self.tokenizer.encode(p[-4 * budget:], budget))
        lens = [len(i) for i in ids_list]
        S = max(lens)
        padded = [i + [0] * (S - len(i)) for i in ids_list]
        tokens = torch.tensor(padded, dtype=torch.int64, device=self.device)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=self.device)
        tmp = self._staging_cache(len(prompts), S)
        logits = self.model.prefill(tokens, tmp, lens=lens_t)
        return {"tmp": tmp, "lens": lens_t, "logits": logits, "S": S,
                "lens_host": lens}

    @torch.inference_mode()
    def integrate_admission(self, sess: "_DecodeSession", rows: list[int],
                            pre: dict,
                            idx: list[int] | None = None) -> torch.Tensor:
        """Copy a prefill_admission's KV into sess.cache rows and set their
        seq_lens (run on the decode loop's stream, AFTER syncing with the
        admission stream).  `idx` selects a SUBSET of the admission's
        requests (partial integration when fewer slots are free than the
        admission holds).  Returns those requests' logits."""
        tmp, lens_t, S = pre["tmp"], pre["lens"], pre["S"]
        logits = pre["logits"]
        with self._gen_lock:
            rows_t = torch.tensor(rows, dtype=torch.int64, device=self.device)
            sel = None
            if idx is not None:
                sel = torch.tensor(idx, dtype=torch.int64, device=self.device)
                lens_t = lens_t[sel]
                logits = logits[sel]
            self._splice_kv(sess.cache, rows, tmp.k, tmp.v, S, sel=sel)
            sess.cache.seq_lens[rows_t] = lens_t
        return logits

    @torch.inference_mode()
    def prefill_into_slots(self, sess: "_DecodeSession", rows: list[int],
                           prompts: list[str],
                           max_new_list: list[int]) -> torch.Tensor:
        """prefill_admission + integrate_admission in one call (same-thread
        admission path / tests)."""
        with self._gen_lock:
            pre = self.prefill_admission(prompts, max_new_list)
        return self.integrate_admission(sess, rows, pre)

    @torch.inference_mode()
    def decode_step_session(self, sess: "_DecodeSession",
                            cur: torch.Tensor) -> torch.Tensor:
        """One decode step over ALL slots (hipGraph replay when captured)."""
        with self._gen_lock:
            return sess.decode_step(cur)

    @torch.inference_mode()
    def sample_rows(self, logits: torch.Tensor,
                    temps: torch.Tensor) -> torch.Tensor:
        """Per-ROW-temperature sampling — continuous batches mix requests
        with different temperatures: greedy rows take argmax, the rest
        Gumbel-argmax (torch eager; the split sampling kernel takes one
        scalar temperature and stays on the uniform-batch path).  Noise
        comes from a SEEDED per-engine generator so stochastic decodes are
        reproducible, matching the wave path's seeded sample_token."""
        self._step_seed += 1
        rng = getattr(self, "_sample_rng", None)
        if rng is None or str(rng.device) != str(logits.device):
            rng = self._sample_rng = torch.Generator(device=logits.device)
            rng.manual_seed(909)
        t = temps.to(logits.device).view(-1, 1)
        u = torch.rand(logits.shape, device=logits.device, generator=rng)
        g = -torch.log(-torch.log(u.clamp_min(1e-20)).clamp_min(1e-20))
        scores = torch.where(t > 0, logits / t.clamp_min(1e-6) + g, logits)
        return scores.argmax(-1)

    @torch.inference_mode()
    def generate(
        self,
        prompts: list[str],
        max_new_tokens: int = 128,
        temperature: float = 0.3,
        stop_on_eos: bool = True,
        on_token: Callable[[int, list[int]], None] | None = None,
        top_k: int = 0,
        top_p: float = 1.0,
        seed: int | None = None,
        grammar=None,
    ) -> list[str]:
        """Batched generation.  Returns decoded completions (prompt excluded).

        on_token(step, token_ids_per_batch) fires after every decode step —
        the serving layer turns it into SSE streaming.

        top_k / top_p / seed at their defaults keep the scalar-temperature
        path (ops.sample_token).  Otherwise every step samples through
        ops.sample_filtered; prompt i draws with seed + i, so a seeded
        request reproduces its text whatever else shares the engine.

        grammar (a Grammar or a handle from register_grammar): every row
        decodes under the grammar through ops.sample_constrained at any
        temperature, with left = max_new_tokens, so each completion matches
        the grammar even when the budget runs out.  ValueError, before any
        forward, when max_new_tokens is below the grammar's shortest
        completion.
        """
        if not prompts:
            return []
        # a request cannot generate past the cache: clamp so the prompt
        # budget stays positive and decode never writes beyond max_seq
        max_new_tokens = max(1, min(max_new_tokens, self.max_seq - 9))
        handle = self.resolve_grammar(grammar)
        if handle is not None:
            self.check_grammar_budget(handle, max_new_tokens)
        import time as _time

        from sentio_amd.observability.kernel_timer import get_timer

        self._gen_lock.acquire()
        try:
            with get_timer("generate").measure():
                return self._generate_locked(
                    prompts, max_new_tokens, temperature, stop_on_eos,
                    on_token, _time,
                    SamplingParams(temperature, top_k, top_p, seed, handle))
        finally:
            self._gen_lock.release()

    # Decode-session batch buckets: serving batches arrive at arbitrary
    # sizes, and every DISTINCT (batch, cache) shape costs a fresh KV-cache
    # allocation + hipGraph capture (~1 s) — the GPU load test spent more
    # wall on captures than on decoding.  Padding rows are near-free
    # (decode streams the same weights either way), so round up and slice.
    _BATCH_BUCKETS = (1, 2, 4, 8, 16, 24, 32, 48, 64)

    def _bucket_batch(self, b: int) -> int:
        for cap in self._BATCH_BUCKETS:
            if b <= cap:
                return cap
        return b

    def _generate_locked(self, prompts, max_new_tokens, temperature,
                         stop_on_eos, on_token, _time,
                         sampling: SamplingParams | None = None) -> list[str]:
        B_req = len(prompts)
        if self.device != "cpu":
            pad = self._bucket_batch(B_req) - B_req
            if pad:
                prompts = list(prompts) + [prompts[-1]] * pad
        B = len(prompts)
        prompt_budget = self.max_seq - max_new_tokens - 1
        # prefix-KV caching: requests share the system-prompt + instruction
        # header; prefill it once per distinct prefix and only forward each
        # request's suffix (byte tokenizer → char-exact prefix alignment)
        import os as _os

        clipped = [p[-4 * prompt_budget:] for p in prompts]
        prefix_ids, suffixes = self._split_shared_prefix(clipped, prompt_budget)
        use_prefix = (len(prefix_ids) >= self._PREFIX_MIN_TOKENS
                      and _os.environ.get("SENTIO_PREFIX_KV", "1") != "0")
        sess = self._decode_session(B, self.max_seq)
        _t0 = _time.perf_counter()
        if use_prefix:
            P = len(prefix_ids)
            # suffixes continue the stream: NO second BOS
            padded, lens = self.tokenizer.encode_batch(
                suffixes, prompt_budget - P, add_bos=False)
            tokens = torch.tensor(padded, dtype=torch.int64,
                                  device=self.device)
            lens_t = torch.tensor(lens, dtype=torch.int32, device=self.device)
            sess.cache.seq_lens.zero_()
            logits = sess.prefill_with_prefix(prefix_ids, tokens, lens_t)
            n_prompt = B_req * P + sum(lens[:B_req])
        else:
            padded, lens = self.tokenizer.encode_batch(clipped, prompt_budget)
            tokens = torch.tensor(padded, dtype=torch.int64,
                                  device=self.device)
            lens_t = torch.tensor(lens, dtype=torch.int32, device=self.device)
            logits = sess.prefill(tokens, lens_t)
            n_prompt = sum(lens[:B_req])
        if self.device != "cpu":
            torch.cuda.synchronize()
        self.last_prefill_s = _time.perf_counter() - _t0
        self.last_prompt_tokens = n_prompt
        _t0 = _time.perf_counter()

        # tokens accumulate on-device; the host syncs only for EOS checks
        # (every 16 steps) or the streaming callback — not per token.
        toks_buf = torch.zeros(B, max_new_tokens, dtype=torch.int64,
                               device=self.device)
        sampler = self._make_sampler(sampling, temperature, B,
                                     max_new_tokens)
        cur = sampler(logits, 0)
        n_steps = max_new_tokens
        for step in range(max_new_tokens):
            toks_buf[:, step] = cur
            if on_token is not None:
                on_token(step, cur.cpu().tolist()[:B_req])
            if stop_on_eos and (step % 16 == 15 or on_token is not None):
                done = (toks_buf[:, : step + 1] == EOS_ID).any(dim=1)
                if bool(done.all()):
                    n_steps = step + 1
                    break
            if step == max_new_tokens - 1:
                break
            logits = sess.decode_step(cur)
            cur = sampler(logits, step + 1)
        if self.device != "cpu":
            torch.cuda.synchronize()
        self.last_decode_s = _time.perf_counter() - _t0
        self.last_decode_steps = n_steps
        try:
            from sentio_amd.observability.metrics import metrics_collector

            metrics_collector.inc("rag_llm_tokens_total",
                                  float(n_prompt), kind="prompt")
            metrics_collector.inc("rag_llm_tokens_total",
                                  float(B_req * n_steps), kind="completion")
        except Exception:
            pass
        rows = toks_buf[:B_req, :n_steps].cpu().tolist()
        out = []
        for row in rows:
            ids = []
            for t in row:
                if stop_on_eos and t == EOS_ID:
                    break
                ids.append(t)
            out.append(self.tokenizer.decode(ids))
        return out

    def _sample(self, logits: torch.Tensor, temperature: float) -> torch.Tensor:
        self._step_seed += 1
        return ops.sample_token(logits, temperature, seed=self._step_seed)

    def derive_seed(self) -> int:
        """Seed for a filtered request that did not bring one."""
        # its own counter: _step_seed feeds the default path's sample_token
        # seeds, which filtered requests must not perturb
        n = self._derived_seeds = self._derived_seeds + 1
        return (n * 0x9E3779B1 + 909) & 0x7FFFFFFF

    def _make_sampler(self, sampling: SamplingParams | None,
                      temperature: float, batch: int,
                      max_new_tokens: int = 0):
        """sampler(logits, step) for one generate/stream call.  Default
        parameters: the present path (_sample -> ops.sample_token, same
        seeds, same tokens).  Otherwise ops.sample_filtered with per-row
        arrays built once; only the step counter changes per token.  With a
        grammar: ops.sample_constrained for any parameters, every row (the
        padding rows of a bucketed batch too) from the grammar's start
        state with left = max_new_tokens."""
        handle = sampling.grammar if sampling is not None else None
        if handle is None and (sampling is None or not sampling.filtered):
            return lambda logits, _step: self._sample(logits, temperature)
        dev = self.device
        base = sampling.seed if sampling.seed is not None \
            else self.derive_seed()
        temps = torch.full((batch,), float(sampling.temperature), device=dev)
        ks = torch.full((batch,), int(sampling.top_k or 0), dtype=torch.int32,
                        device=dev)
        ps = torch.full((batch,), float(sampling.top_p), device=dev)
        seeds = int(base) + torch.arange(batch, dtype=torch.int64, device=dev)

        if handle is not None:
            tables = self._grammar_tables
            state = torch.full((batch,), int(handle.start), dtype=torch.int32,
                               device=dev)
            left = torch.full((batch,), int(max_new_tokens),
                              dtype=torch.int32, device=dev)

            def constrained(logits, step):
                steps = torch.full((batch,), int(step), dtype=torch.int32,
                                   device=dev)
                return ops.sample_constrained(logits, temps, ks, ps, seeds,
                                              steps, state, left, tables)

            return constrained

        def sampler(logits, step):
            steps = torch.full((batch,), int(step), dtype=torch.int32,
                               device=dev)
            return ops.sample_filtered(logits, temps, ks, ps, seeds, steps)

        return sampler

    @torch.inference_mode()
    def stream(self, prompt: str, max_new_tokens: int = 128,
               temperature: float = 0.3, top_k: int = 0, top_p: float = 1.0,
               seed: int | None = None, grammar=None) -> Iterator[str]:
        """Yield text deltas token-by-token (single prompt) — the on-device
        equivalent of the reference's SSE streaming (openai.py:149-157).
        Holds the generation lock for the stream's duration (the pooled
        decode sessions are engine-level state)."""
        handle = self.resolve_grammar(grammar)
        if handle is not None:
            self.check_grammar_budget(handle, max_new_tokens)
        with self._gen_lock:
            yield from self._stream_locked(prompt, max_new_tokens, temperature,
                                           top_k, top_p, seed, handle)

    def _stream_locked(self, prompt: str, max_new_tokens: int,
                       temperature: float, top_k: int = 0,
                       top_p: float = 1.0,
                       seed: int | None = None,
                       grammar=None) -> Iterator[str]:
        prompt_budget = self.max_seq - max_new_tokens - 1
        ids = self.tokenizer.encode(prompt[-4 * prompt_budget:], prompt_budget)
        tokens = torch.tensor([ids], dtype=torch.int64, device=self.device)
        sess = self._decode_session(1, self.max_seq)
        logits = sess.prefill(tokens)
        sampler = self._make_sampler(
            SamplingParams(temperature, top_k, top_p, seed, grammar),
            temperature, 1, max_new_tokens)
        cur = sampler(logits, 0)
        generated: list[int] = []
        emitted = ""
        for step in range(max_new_tokens):
            t = int(cur.item())
            if t == EOS_ID:
                break
            generated.append(t)
            text = self.tokenizer.decode(generated)
            if len(text) > len(emitted):
                delta = text[len(emitted):]
                emitted = text
                yield delta
            if step == max_new_tokens - 1:
                break
            logits = sess.decode_step(cur)
            cur = sampler(logits, step + 1)
