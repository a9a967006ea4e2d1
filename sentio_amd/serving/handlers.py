"""Request handlers (reference src/api/handlers/chat.py:25-274 and
health.py:20-344 capability): chat orchestration with the fallback chain
cached-response → template → apology, plus health probes."""

from __future__ import annotations

import logging
import threading
import time
import uuid
from typing import Any

from sentio_amd.caching.manager import CacheManager
from sentio_amd.models.document import Document
from sentio_amd.pipeline.state import create_initial_state
from sentio_amd.resilience.fallbacks import fallback_manager, llm_fallback
from sentio_amd.serving.container import ServiceContainer

logger = logging.getLogger(__name__)


def resolve_sampling(settings, top_p: float | None = None,
                     sampling_top_k: int | None = None,
                     seed: int | None = None) -> dict[str, Any]:
    """Request-level nucleus sampling controls as pipeline metadata.  A field
    the request leaves unset takes the service-wide default (GEN_TOP_P /
    GEN_TOP_K); values that switch a filter off are dropped, so a request
    with nothing set yields {} and stays on the default sampling path."""
    p = top_p if top_p is not None else getattr(settings, "gen_top_p", 1.0)
    k = sampling_top_k if sampling_top_k is not None \
        else getattr(settings, "gen_top_k", 0)
    if seed is None and getattr(settings, "gen_seed", -1) >= 0:
        seed = settings.gen_seed
    out: dict[str, Any] = {}
    if p is not None and float(p) < 1.0:
        out["top_p"] = float(p)
    if k is not None and int(k) > 0:
        out["sampling_top_k"] = int(k)
    if seed is not None:
        out["seed"] = int(seed)
    return out


# pattern -> Grammar, or the ValueError of a pattern that did not compile
# (a hostile pattern costs its compile budget once, not once per request)
_grammar_cache: dict[str, Any] = {}
_grammar_cache_lock = threading.Lock()
_GRAMMAR_CACHE_MAX = 64
# An engine's grammar table is append-only (32766 states for the life of the
# process), so the patterns that arrive through the API share a budget that
# leaves half of it to the service's own grammars.
API_GRAMMAR_STATE_BUDGET = 16384
_api_patterns: dict[str, int] = {}          # pattern -> table states


class GrammarBudgetError(ValueError):
    """The process has no room for another API grammar."""


def compile_response_format(fmt: dict | None, tokenizer=None,
                            max_new_tokens: int | None = None):
    """A request's `response_format` -> Grammar (None for None).
    {"type": "regex", "pattern": ...} or {"type": "json_object", "fields":
    [...]} (see engines/grammar.py).  Compiled grammars are cached per
    process by pattern, failures included.  ValueError, with the compiler's
    message, for unsupported syntax, more than API_MAX_STATES automaton
    states, a compile that exceeds its work or time budget
    (API_COMPILE_SECONDS), or a grammar whose shortest completion does not
    fit max_new_tokens; GrammarBudgetError once the distinct patterns seen
    by this process hold API_GRAMMAR_STATE_BUDGET table states."""
    if fmt is None:
        return None
    from sentio_amd.engines.grammar import (API_COMPILE_SECONDS,
                                            API_MAX_STATES, Grammar,
                                            json_object_regex)

    if not isinstance(fmt, dict):
        raise ValueError("response_format must be an object")
    kind = fmt.get("type")
    if kind == "regex":
        pattern = fmt.get("pattern")
        if not isinstance(pattern, str) or not pattern:
            raise ValueError("response_format.pattern must be a string")
        if len(pattern) > 4096:
            raise ValueError("response_format.pattern is too long")
    elif kind == "json_object":
        pattern = json_object_regex(fmt.get("fields"))
    else:
        raise ValueError("response_format.type must be 'regex' or "
                         "'json_object'")
    with _grammar_cache_lock:
        grammar = _grammar_cache.get(pattern)
    if grammar is None:
        try:
            grammar = Grammar.from_regex(pattern, max_states=API_MAX_STATES,
                                         seconds=API_COMPILE_SECONDS)
        except ValueError as exc:
            grammar = exc
        with _grammar_cache_lock:
            if len(_grammar_cache) >= _GRAMMAR_CACHE_MAX:
                _grammar_cache.pop(next(iter(_grammar_cache)))
            grammar = _grammar_cache.setdefault(pattern, grammar)
    if isinstance(grammar, ValueError):
        raise ValueError(str(grammar))
    with _grammar_cache_lock:
        if pattern not in _api_patterns:
            used = sum(_api_patterns.values())
            if used + grammar.n_states + 1 > API_GRAMMAR_STATE_BUDGET:
                raise GrammarBudgetError(
                    f"no room for another response_format grammar: {used} of "
                    f"{API_GRAMMAR_STATE_BUDGET} states are in use")
            _api_patterns[pattern] = grammar.n_states + 1
    if tokenizer is not None and max_new_tokens is not None:
        tb = grammar.token_tables(tokenizer)
        if int(tb.dist[tb.start]) > int(max_new_tokens):
            raise ValueError(
                f"the shortest reply of this response_format takes "
                f"{int(tb.dist[tb.start])} tokens, the limit is "
                f"{int(max_new_tokens)}")
    return grammar


class ChatHandler:
    def __init__(self, container: ServiceContainer):
        self.container = container
        self.cache: CacheManager = container.cache_manager()

    def process(self, question: str, top_k: int | None = None,
                temperature: float | None = None,
                history: list[dict[str, str]] | None = None,
                top_p: float | None = None,
                sampling_top_k: int | None = None,
                seed: int | None = None,
                grammar=None) -> dict[str, Any]:
        """top_k is the RETRIEVAL depth; sampling_top_k / top_p / seed are
        the generator's sampling controls; grammar (a compiled
        response_format) constrains the answer."""
        query_id = str(uuid.uuid4())
        meta: dict[str, Any] = {"query_id": query_id}
        if grammar is not None:
            meta["grammar"] = grammar
        meta.update(resolve_sampling(getattr(self.container, "settings", None), top_p,
                                     sampling_top_k, seed))
        if top_k is not None:
            meta["user_top_k"] = int(top_k)
        if temperature is not None:
            meta["temperature"] = float(temperature)
        if history:
            meta["history"] = history

        cached = self.cache.l1.get_query(question)
        try:
            state = create_initial_state(question, meta)
            state = self.container.pipeline().invoke(state)
            answer = state.get("response", "")
            if not answer:
                raise RuntimeError("empty response from pipeline")
            sources = self._shape_sources(state.get("selected_documents") or
                                          state.get("retrieved_documents") or [])
            result = {
                "answer": answer,
                "sources": sources,
                "metadata": {
                    "query_id": query_id,
                    "pipeline_ms": state.get("metadata", {}).get("pipeline_ms"),
                    "retrieved_count": state.get("metadata", {}).get("retrieved_count"),
                    "selected_count": state.get("metadata", {}).get("selected_count"),
                    "verification": state.get("evaluation", {}).get("verification"),
                },
            }
            self.cache.l1.set_query(question, result)
            fallback_manager.cache_response(question, answer)
            self.container.heartbeat.beat()
            return result
        except Exception as exc:
            logger.error("chat pipeline failed: %s", exc)
            # fallback chain (reference chat.py:195-239)
            if cached is not None:
                cached = dict(cached)
                cached.setdefault("metadata", {})["fallback"] = "cached"
                return cached
            disk_cached = fallback_manager.get_cached_response(question)
            if disk_cached:
                return {"answer": disk_cached, "sources": [],
                        "metadata": {"query_id": query_id, "fallback": "disk_cache"}}
            template = llm_fallback.generate_fallback_response(question, "error")
            return {"answer": template, "sources": [],
                    "metadata": {"query_id": query_id, "fallback": "template",
                                 "error": str(exc)}}

    @staticmethod
    def _shape_sources(docs: list[Document]) -> list[dict[str, Any]]:
        out = []
        for d in docs:
            raw = d.metadata.get("score", 0.0)
            try:
                score = max(0.0, min(1.0, float(raw)))
            except (TypeError, ValueError):
                score = 0.0
            out.append({
                "text": (d.text or "")[:1000],
                "source": str(d.metadata.get("source", d.id)),
                "score": score,
                "metadata": {k: v for k, v in d.metadata.items()
                             if k not in ("content",)},
            })
        return out

    def probe(self, timeout_s: float = 5.0) -> bool:
        """Health probe: run the retriever stage only (reference chat.py:241-274)."""
        try:
            t0 = time.time()
            self.container.retriever().retrieve("health probe", top_k=1)
            return (time.time() - t0) <= timeout_s
        except Exception:
            return False


class HealthHandler:
    def __init__(self, container: ServiceContainer):
        self.container = container
        self._cache: tuple[float, dict] | None = None
        self._cache_ttl = 10.0  # reference health.py:28-30

    def basic(self) -> dict[str, Any]:
        return {
            "status": "healthy",
            "timestamp": time.time(),
            "version": __import__("sentio_amd").__version__,
            "services": {"engine": "ok", "device": self.container.device},
        }

    def detailed(self) -> dict[str, Any]:
        now = time.time()
        if self._cache and now - self._cache[0] < self._cache_ttl:
            return self._cache[1]
        from sentio_amd.observability.monitoring import resource_monitor

        checks: dict[str, Any] = {}
        try:
            self.container.encoder().embed(["health"])
            checks["encoder"] = "ok"
        except Exception as exc:
            checks["encoder"] = f"error: {exc}"
        checks["index"] = {"dense": len(self.container.dense_index()),
                           "bm25": self.container.bm25_index().n_docs}
        checks["breakers"] = {k: b.health()["state"]
                              for k, b in self.container.breakers.items()}
        checks["heartbeat"] = self.container.heartbeat.snapshot()
        # request/engine coalescing evidence (dynamic + micro batchers)
        gen = self.container._cache.get("generator_frontend")
        if gen is not None and hasattr(gen, "batcher"):
            checks["batcher"] = gen.batcher.health()
        checks["micro_batchers"] = {
            k: m.health() for k, m in (
                (k, getattr(self.container._cache.get(k), "micro", None))
                for k in ("encoder", "reranker"))
            if m is not None
        }
        status = "healthy" if checks.get("encoder") == "ok" else "degraded"
        result = {
            "status": status,
            "timestamp": now,
            "checks": checks,
            "periodic": self.container.health_checker().status(),
            "resources": resource_monitor.snapshot(),
        }
        self._cache = (now, result)
        return result

    def ready(self) -> bool:
        try:
            self.container.pipeline()
            return True
        except Exception:
            return False

    def live(self) -> bool:
        return True
