"""Grammar-constrained decoding on the CPU tiny decoder: engine, slot
sampler, batchers, verifier and /chat.  `re.fullmatch` is the oracle for
every constrained completion; the unconstrained paths are compared with
values computed through ops.sample_token / ops.sample_filtered."""

import re

import pytest
import torch

from sentio_amd import ops
from sentio_amd.engines.generator import GeneratorEngine, SamplingParams
from sentio_amd.engines.grammar import VERDICT_GRAMMAR, Grammar

PATTERN = r"(yes|no), [a-c]{2,5}!"
PROMPTS = ["answer yes or no", "a second, other prompt"]


@pytest.fixture(scope="module")
def engine():
    return GeneratorEngine(model="tiny-decoder", device="cpu", dtype="fp32",
                           max_seq=256)


@pytest.fixture(scope="module")
def grammar():
    return Grammar.from_regex(PATTERN)


@pytest.mark.parametrize("T,extra", [
    (0.0, {}), (0.7, {}), (1.0, {}),
    (0.7, {"top_k": 20}), (1.0, {"top_p": 0.9, "seed": 5}),
])
def test_generate_matches_the_grammar(engine, grammar, T, extra):
    h = engine.register_grammar(grammar)
    assert engine.register_grammar(grammar) is h          # built once
    for budget in (h.min_tokens, h.min_tokens + 3, 40):
        outs = engine.generate(PROMPTS, max_new_tokens=budget, temperature=T,
                               grammar=grammar, **extra)
        for o in outs:
            assert re.fullmatch(PATTERN, o), (T, extra, budget, o)


def test_unconstrained_output_does_not_match(engine):
    for T in (0.0, 0.7):
        outs = engine.generate(PROMPTS, max_new_tokens=12, temperature=T)
        assert not any(re.fullmatch(PATTERN, o) for o in outs)


def test_budget_below_the_shortest_completion_raises(engine, grammar):
    h = engine.register_grammar(grammar)
    calls = []
    orig = engine.model.prefill
    engine.model.prefill = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        with pytest.raises(ValueError):
            engine.generate(PROMPTS, max_new_tokens=h.min_tokens - 1,
                            grammar=grammar)
        with pytest.raises(ValueError):
            list(engine.stream("x", max_new_tokens=h.min_tokens - 1,
                               grammar=grammar))
    finally:
        engine.model.prefill = orig
    assert not calls                                      # before any forward


def test_seeded_constrained_requests_reproduce(engine, grammar):
    kw = dict(max_new_tokens=12, temperature=1.0, top_p=0.95, seed=11,
              grammar=grammar)
    a = engine.generate(PROMPTS, **kw)
    engine.generate(["something else in between"], max_new_tokens=4)
    assert engine.generate(PROMPTS, **kw) == a
    assert "".join(engine.stream(PROMPTS[0], **kw)) == a[0]


def test_grammar_none_keeps_the_present_paths(engine, grammar):
    """Default, top-k and seeded calls sample through ops.sample_token /
    ops.sample_filtered with the present seeds, grammar registered or not."""
    engine.register_grammar(grammar)
    seen = []
    real_tok, real_filt = ops.sample_token, ops.sample_filtered

    def spy_tok(logits, temperature, seed=0):
        out = real_tok(logits, temperature, seed=seed)
        seen.append(("token", seed, out.tolist()))
        return out

    def spy_filt(logits, t, k, p, sd, st):
        out = real_filt(logits, t, k, p, sd, st)
        seen.append(("filtered", sd.tolist(), out.tolist()))
        return out

    ops.sample_token, ops.sample_filtered = spy_tok, spy_filt
    try:
        seed0 = engine._step_seed
        out = engine.generate(PROMPTS, max_new_tokens=4, temperature=0.7,
                              stop_on_eos=False, grammar=None)
        assert [s[0] for s in seen] == ["token"] * 4
        assert [s[1] for s in seen] == [seed0 + i + 1 for i in range(4)]
        rows = list(zip(*[s[2] for s in seen]))
        assert out == [engine.tokenizer.decode(list(r)) for r in rows]
        seen.clear()
        out = engine.generate(PROMPTS, max_new_tokens=3, temperature=0.7,
                              top_k=10, seed=4, stop_on_eos=False)
        assert [s[0] for s in seen] == ["filtered"] * 3
        assert all(s[1] == [4, 5] for s in seen)
        rows = list(zip(*[s[2] for s in seen]))
        assert out == [engine.tokenizer.decode(list(r)) for r in rows]
        # top-k without a seed: the filtered path on a derived seed
        seen.clear()
        n0 = engine._derived_seeds
        out = engine.generate(PROMPTS, max_new_tokens=3, temperature=0.7,
                              top_k=10, stop_on_eos=False)
        base = ((n0 + 1) * 0x9E3779B1 + 909) & 0x7FFFFFFF
        assert [s[0] for s in seen] == ["filtered"] * 3
        assert all(s[1] == [base, base + 1] for s in seen)
        rows = list(zip(*[s[2] for s in seen]))
        assert out == [engine.tokenizer.decode(list(r)) for r in rows]
    finally:
        ops.sample_token, ops.sample_filtered = real_tok, real_filt


def test_slot_sampler_constrained_and_plain_side_by_side(engine, grammar):
    h = engine.register_grammar(grammar)
    sess = engine.make_slot_session(4)
    rows = [2, 0]
    logits = engine.prefill_into_slots(sess, rows, PROMPTS, [12, 12])
    sp = engine.make_slot_sampler(4)
    params = [SamplingParams(0.8, 0, 1.0, seed=17, grammar=grammar),
              SamplingParams(0.8, 0, 1.0, seed=23)]
    with pytest.raises(ValueError):
        sp.admit(rows, params, [h.min_tokens - 1, 12])
    sp.admit(rows, params, [12, 12])
    assert sp.state.tolist() == [-1, -1, h.start, -1]
    cur = torch.zeros(4, dtype=torch.int64)
    ids = {2: [], 0: []}
    want_plain = []
    sp.sample(logits, cur, rows=rows)
    want_plain.append(int(ops.sample_filtered(logits[1:2], 0.8, 0, 1.0, 23,
                                              0)[0]))
    for step in range(1, 12):
        for r in rows:
            ids[r].append(int(cur[r]))
        logits = engine.decode_step_session(sess, cur)
        sp.sample(logits, cur)
        want_plain.append(int(ops.sample_filtered(logits[0:1], 0.8, 0, 1.0,
                                                  23, step)[0]))
    for r in rows:
        ids[r].append(int(cur[r]))
    assert ids[0] == want_plain                   # the plain slot: as before
    text = ids[2][: ids[2].index(2)] if 2 in ids[2] else ids[2]
    assert re.fullmatch(PATTERN, engine.tokenizer.decode(text))
    assert sp.left.tolist()[2] == 0 and sp.step.tolist() == [12, 0, 12, 0]


def test_batchers_group_and_route_by_grammar(engine, grammar):
    from sentio_amd.serving.batcher import (ContinuousGenerator, _make_item,
                                            _sampling_only)

    h = engine.register_grammar(grammar)
    h2 = engine.register_grammar(Grammar.from_regex(r"[0-9]{1,3}"))
    a = _make_item("p", 8, 0.3, True, grammar=h)
    b = _make_item("q", 8, 0.3, True, grammar=h)
    c = _make_item("r", 8, 0.3, True, grammar=h2)
    d = _make_item("s", 8, 0.3, True)
    assert a.group_key == b.group_key != c.group_key
    assert len(d.group_key) == 3 and d.group_key == a.group_key[:3]
    assert d.group_key != a.group_key       # a plain request: its own wave
    assert a.sampling_kwargs["grammar"] is h
    for slot_sampling in (False, True):
        gen = ContinuousGenerator(engine, slots=2,
                                  slot_sampling=slot_sampling)
        try:
            assert gen._joins_loop({}) is True
            assert gen._joins_loop(_sampling_only({"grammar": grammar})) \
                is slot_sampling
            assert gen._joins_loop(_sampling_only(
                {"grammar": grammar, "seed": 3})) is False
            out = gen.generate(["route me"], max_new_tokens=12,
                               temperature=0.7, grammar=grammar)[0]
            assert re.fullmatch(PATTERN, out), out
            loop, wave = gen.batcher.stats, gen.sampled_batcher.stats
            assert (loop["completed"], wave["requests"]) == \
                ((1, 0) if slot_sampling else (0, 1))
            with pytest.raises(ValueError):
                gen.generate(["too short"], max_new_tokens=2, grammar=grammar)
        finally:
            gen.batcher.stop()
            gen.sampled_batcher.stop()


def test_verifier_constrained_and_default(engine):
    from sentio_amd.pipeline.verifier import AnswerVerifier

    v = AnswerVerifier(engine, max_tokens=8, constrained=True)
    out = v.verify("what is it?", "[1] some context", "an answer [1]")
    assert out["verdict"] in ("pass", "warn", "fail")
    assert out["notes"] != ["invalid_json"] and "verifier_error" not in out["notes"]

    class Spy:
        tokenizer = engine.tokenizer

        def generate(self, *args, **kwargs):
            self.call = (args, kwargs)
            return ["free text"]

    spy = Spy()
    off = AnswerVerifier(spy, max_tokens=64).verify("q", "c", "a")
    assert off["notes"] == ["invalid_json"]
    assert len(spy.call[0]) == 1 and spy.call[1] == {
        "max_new_tokens": 64, "temperature": 0.0}
    on = AnswerVerifier(spy, max_tokens=8, constrained=True)
    on.verify("q", "c", "a")
    tb = VERDICT_GRAMMAR.token_tables(engine.tokenizer)
    assert spy.call[1]["grammar"] is VERDICT_GRAMMAR
    assert spy.call[1]["max_new_tokens"] == int(tb.dist[tb.start]) > 8


def test_chat_response_format(fresh_container):
    from fastapi.testclient import TestClient

    from sentio_amd.serving.app import create_app
    from sentio_amd.serving.handlers import compile_response_format

    g = compile_response_format({"type": "regex", "pattern": PATTERN})
    assert compile_response_format({"type": "regex", "pattern": PATTERN}) is g
    j = compile_response_format({"type": "json_object", "fields": [
        {"name": "ok", "type": "boolean"}]})
    assert j.matches('{"ok": true}')
    seen = {}
    gen = fresh_container.generator()
    real = gen.generate

    def spy(prompts, **kw):
        seen.update(kw)
        return real(prompts, **kw)

    gen.generate = spy
    fresh_container.settings.disable_auth = True
    client = TestClient(create_app(container=fresh_container))
    r = client.post("/chat", json={"question": "is it so?", "response_format":
                                   {"type": "regex", "pattern": PATTERN}})
    assert r.status_code == 200, r.text
    assert seen.get("grammar") is g
    for bad in ({"type": "regex", "pattern": r"(?=a)b"},
                {"type": "regex", "pattern": r"[ab]{3000}"},
                {"type": "xml"},
                {"type": "json_object", "fields": [{"name": "a",
                                                    "type": "float"}]}):
        r = client.post("/chat", json={"question": "is it so?",
                                       "response_format": bad})
        assert r.status_code == 422, (bad, r.text)
        r = client.post("/chat/stream", json={"question": "is it so?",
                                              "response_format": bad})
        assert r.status_code == 422, (bad, r.text)
    # the streaming route with a valid format: the grammar reaches stream()
    got = {}
    front = fresh_container.generator_frontend()
    real_stream = front.stream

    def spy_stream(prompt, **kw):
        got.update(kw)
        return real_stream(prompt, **kw)

    front.stream = spy_stream
    r = client.post("/chat/stream", json={
        "question": "is it so?",
        "response_format": {"type": "regex", "pattern": PATTERN}})
    assert r.status_code == 200 and r.text.rstrip().endswith("data: [DONE]")
    assert got.get("grammar") is g


def test_hostile_pattern_is_refused_quickly_and_once(fresh_container):
    """A short pattern whose automaton explodes must cost the server a
    bounded compile, off the event loop, and only once.  The bound: the
    compile's own wall-clock budget (API_COMPILE_SECONDS), doubled for the
    request around it, plus a second for a loaded machine."""
    import time

    from fastapi.testclient import TestClient

    from sentio_amd.engines import grammar as G
    from sentio_amd.serving import handlers
    from sentio_amd.serving.app import create_app

    fresh_container.settings.disable_auth = True
    client = TestClient(create_app(container=fresh_container))
    limit = 2 * G.API_COMPILE_SECONDS + 1.0
    compiles = []
    real = G.Grammar.from_regex.__func__

    def counting(cls, pattern, *a, **k):
        compiles.append(pattern)
        return real(cls, pattern, *a, **k)

    G.Grammar.from_regex = classmethod(counting)
    try:
        for pattern in (r"(.{1,60}){1,60}", r"(a|b)*a(a|b){20}",
                        r"((a{1,40}){1,40}){1,40}", r"[ab]{2999}"):
            for attempt in range(2):
                t0 = time.perf_counter()
                r = client.post("/chat", json={
                    "question": "is it so?",
                    "response_format": {"type": "regex", "pattern": pattern}})
                took = time.perf_counter() - t0
                assert r.status_code == 422, (pattern, r.text)
                assert "too large" in r.text
                assert took < limit, (pattern, took)
            assert compiles.count(pattern) == 1          # the failure is cached
        with pytest.raises(ValueError):
            G.Grammar.from_regex(r"(.{1,60}){1,60}", max_states=G.API_MAX_STATES)
    finally:
        G.Grammar.from_regex = classmethod(real)


def test_api_grammar_budget_and_full_table_are_503(fresh_container, grammar):
    from fastapi.testclient import TestClient

    from sentio_amd.serving import handlers
    from sentio_amd.serving.app import create_app

    fresh_container.settings.disable_auth = True
    client = TestClient(create_app(container=fresh_container))
    body = {"question": "is it so?", "response_format":
            {"type": "regex", "pattern": r"[xyz]{3}budget"}}
    saved = handlers.API_GRAMMAR_STATE_BUDGET
    handlers.API_GRAMMAR_STATE_BUDGET = sum(handlers._api_patterns.values())
    try:
        r = client.post("/chat", json=body)
        assert r.status_code == 503, r.text
    finally:
        handlers.API_GRAMMAR_STATE_BUDGET = saved
    gen = fresh_container.generator()

    def full(_grammar):
        raise ValueError("grammar table full")

    gen.register_grammar = full
    try:
        r = client.post("/chat", json=body)
        assert r.status_code == 503 and "table full" in r.text
    finally:
        del gen.register_grammar


def test_clamped_budget_is_checked_in_the_callers_thread(grammar):
    """max_new_tokens near max_seq: the slot loop would grant only
    max_seq - 9 tokens at worst, so the request is refused when it is made,
    not in the loop thread where it would fail its co-tenants."""
    from sentio_amd.serving.batcher import _resolve_grammar

    small = GeneratorEngine(model="tiny-decoder", device="cpu", dtype="fp32",
                            max_seq=12)
    h = small.register_grammar(grammar)
    assert h.min_tokens == 4
    with pytest.raises(ValueError):
        _resolve_grammar(small, grammar, 10)     # granted: 12 - 9 = 3 < 4
    roomy = GeneratorEngine(model="tiny-decoder", device="cpu", dtype="fp32",
                            max_seq=13)
    assert _resolve_grammar(roomy, grammar, 10).min_tokens == 4
