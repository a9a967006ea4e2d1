"""Slot sampling on the CPU path: torch_ref.sample_slots semantics, the input
checks of ops.sample_slots, the SLOT_SAMPLING setting, and the continuous
frontend's routing and slot loop with slot_sampling=True (tiny-decoder)."""

import pytest
import torch

PROMPT = "slot sampling keeps the nucleus request inside the loop"


def _rows(R: int, V: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (2.0 * torch.randn(R, V, generator=g)).contiguous()


def _slot_state(S: int):
    """Distinct per-slot parameters, seeds and non-zero starting steps."""
    params = [(0.0, 0, 1.0), (0.7, 0, 0.9), (1.0, 20, 1.0), (0.5, 50, 0.9),
              (2.0, 1, 1.0), (1.0, 0, 1.0), (0.3, 8, 0.5), (1.5, 0, 0.95)][:S]
    t = torch.tensor([p[0] for p in params], dtype=torch.float32)
    k = torch.tensor([p[1] for p in params], dtype=torch.int32)
    p_ = torch.tensor([p[2] for p in params], dtype=torch.float32)
    seed = torch.arange(S, dtype=torch.int64) * 7919 + 11
    step = torch.arange(S, dtype=torch.int32) * 3 + 2
    return t, k, p_, seed, step


# ---------------------------------------------------------------- reference

def test_torch_ref_sample_slots_semantics():
    from sentio_amd.ops import torch_ref

    S, R, V = 6, 4, 300
    slot = [5, 0, 3, 2]
    x = _rows(R, V, 1)
    t, k, p, seed, step0 = _slot_state(S)
    active = torch.ones(S, dtype=torch.uint8)
    active[3] = 0                                   # a listed slot, inactive
    step = step0.clone()
    tok = torch.full((S,), -7, dtype=torch.int64)
    torch_ref.sample_slots(x, slot, t, k, p, seed, step, active, tok)
    for r, s in enumerate(slot):
        if s == 3:
            continue
        want = torch_ref.sample_filtered(x[r:r + 1], t[s], k[s], p[s],
                                         seed[s], step0[s])
        assert int(tok[s]) == int(want[0]), (r, s)
        assert int(step[s]) == int(step0[s]) + 1
    for s in (1, 3, 4):                             # unlisted / inactive
        assert int(tok[s]) == -7 and int(step[s]) == int(step0[s])

    # the same through ops (CPU dispatch), with a tensor slot table
    step2 = step0.clone()
    tok2 = torch.full((S,), -7, dtype=torch.int64)
    from sentio_amd import ops

    ops.sample_slots(x, torch.tensor(slot, dtype=torch.int32), t, k, p, seed,
                     step2, active, tok2)
    assert torch.equal(tok2, tok) and torch.equal(step2, step)


def test_torch_ref_sample_slots_identity_and_all_inactive():
    from sentio_amd.ops import torch_ref

    S, V = 5, 200
    x = _rows(S, V, 2)
    t, k, p, seed, step0 = _slot_state(S)
    step = step0.clone()
    tok = torch.full((S,), -7, dtype=torch.int64)
    torch_ref.sample_slots(x, None, t, k, p, seed, step, None, tok)
    want = torch_ref.sample_filtered(x, t, k, p, seed, step0)
    assert torch.equal(tok, want)
    assert torch.equal(step, step0 + 1)

    # every slot inactive: nothing changes
    before_tok, before_step = tok.clone(), step.clone()
    torch_ref.sample_slots(x, None, t, k, p, seed, step,
                           torch.zeros(S, dtype=torch.uint8), tok)
    assert torch.equal(tok, before_tok) and torch.equal(step, before_step)


# ---------------------------------------------------------------- checks

def test_ops_sample_slots_rejects_bad_input():
    from sentio_amd import ops

    S, R, V = 4, 2, 50
    x = _rows(R, V, 3)
    t, k, p, seed, step = _slot_state(S)
    active = torch.ones(S, dtype=torch.uint8)
    tok = torch.zeros(S, dtype=torch.int64)

    def call(**over):
        a = dict(logits=x, slot=[1, 3], temperature=t, top_k=k, top_p=p,
                 seed=seed, step=step.clone(), active=active, tok=tok.clone())
        a.update(over)
        return ops.sample_slots(a["logits"], a["slot"], a["temperature"],
                                a["top_k"], a["top_p"], a["seed"], a["step"],
                                a["active"], a["tok"])

    call()                                              # the valid call
    with pytest.raises(ValueError, match="duplicate"):
        call(slot=[1, 1])
    with pytest.raises(ValueError, match="outside"):
        call(slot=[1, S])
    with pytest.raises(ValueError, match="outside"):
        call(slot=[-1, 2])
    with pytest.raises(ValueError):
        call(slot=[1, 2, 3])                            # R slots expected
    with pytest.raises(ValueError):
        call(slot=None)                                 # R != S
    with pytest.raises(ValueError):
        call(slot=torch.tensor([1, 3]))                 # int64 slot tensor
    with pytest.raises(ValueError):
        call(logits=x.double())
    with pytest.raises(ValueError):
        call(logits=x[0])
    with pytest.raises(ValueError):
        call(top_k=k.long())
    with pytest.raises(ValueError):
        call(step=step.long())
    with pytest.raises(ValueError):
        call(seed=seed.int())
    with pytest.raises(ValueError):
        call(tok=tok.int())
    with pytest.raises(ValueError):
        call(active=active.bool())
    with pytest.raises(ValueError):
        call(temperature=t[:3])
    with pytest.raises(ValueError):
        call(top_p=0.9)
    with pytest.raises(ValueError):
        call(active=torch.ones(S + 1, dtype=torch.uint8))
    assert "sample_slots" in ops.__all__


# ---------------------------------------------------------------- settings

def test_slot_sampling_setting(monkeypatch):
    from sentio_amd.config import Settings

    monkeypatch.delenv("SLOT_SAMPLING", raising=False)
    assert Settings().slot_sampling is False
    assert Settings.from_env().slot_sampling is False
    monkeypatch.setenv("SLOT_SAMPLING", "1")
    assert Settings.from_env().slot_sampling is True


# ---------------------------------------------------------------- engine

def test_slot_sampler_state():
    from sentio_amd.engines.generator import GeneratorEngine, SamplingParams
    from sentio_amd.ops import torch_ref

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=64)
    sp = eng.make_slot_sampler(4)
    assert sp.active.tolist() == [0, 0, 0, 0]
    sp.admit([2, 0], [SamplingParams(0.7, 20, 0.9),
                      SamplingParams(1.0, 0, 1.0, seed=41)])
    assert sp.active.tolist() == [1, 0, 1, 0]
    assert sp.top_k.tolist() == [0, 0, 20, 0]
    assert int(sp.seed[0]) == 41 and int(sp.seed[2]) != 0   # derived seed
    x = _rows(2, eng.cfg.vocab_size, 4)
    cur = torch.full((4,), -7, dtype=torch.int64)
    sp.sample(x, cur, rows=[2, 0])
    want = torch_ref.sample_filtered(x, sp.temperature[[2, 0]],
                                     sp.top_k[[2, 0]], sp.top_p[[2, 0]],
                                     sp.seed[[2, 0]], 0)
    assert cur.tolist() == [int(want[1]), -7, int(want[0]), -7]
    assert sp.step.tolist() == [1, 0, 1, 0]
    sp.release(2)
    sp.sample(_rows(4, eng.cfg.vocab_size, 5), cur)
    assert sp.step.tolist() == [2, 0, 1, 0] and int(cur[2]) == int(want[0])
    sp.admit([2], [SamplingParams(0.5)])                   # re-admission
    assert int(sp.step[2]) == 0 and int(sp.active[2]) == 1
    with pytest.raises(ValueError):
        sp.admit([4], [SamplingParams()])
    with pytest.raises(ValueError):
        sp.sample(x, cur, rows=[1, 1])


# ---------------------------------------------------------------- frontend

def _frontend(slots=2, **kw):
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.serving.batcher import ContinuousGenerator

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=64)
    return eng, ContinuousGenerator(eng, slots=slots, **kw)


def _stop(gen):
    gen.batcher.stop()
    gen.sampled_batcher.stop()


def test_routing_with_slot_sampling():
    _, gen = _frontend(slot_sampling=True)
    try:
        kw = dict(max_new_tokens=6, temperature=1.0, stop_on_eos=False)
        a = gen.generate(["nucleus"], top_p=0.9, **kw)
        assert isinstance(a[0], str)
        assert gen.batcher.stats["requests"] == 1
        b = gen.generate(["top-k"], top_k=20, **kw)
        assert isinstance(b[0], str)
        assert gen.batcher.stats["requests"] == 2
        s = "".join(gen.stream("streamed", max_new_tokens=6, temperature=1.0,
                               top_k=20, top_p=0.9))
        assert isinstance(s, str)
        assert gen.batcher.stats["requests"] == 3
        assert gen.sampled_batcher.stats["requests"] == 0
        assert gen.batcher._thread is not None \
            and gen.batcher._thread.is_alive()
        # a seed keeps the request on the wave path
        c = gen.generate(["seeded"], top_p=0.9, seed=5, **kw)
        assert c == gen.generate(["seeded"], top_p=0.9, seed=5, **kw)
        assert gen.sampled_batcher.stats["requests"] == 2
        assert gen.batcher.stats["requests"] == 3
    finally:
        _stop(gen)


def test_routing_default_is_unchanged():
    _, gen = _frontend()
    try:
        assert gen.slot_sampling is False
        assert gen.batcher.slot_sampling is False
        kw = dict(max_new_tokens=4, temperature=1.0, stop_on_eos=False)
        gen.generate(["nucleus"], top_p=0.9, **kw)
        gen.generate(["top-k"], top_k=20, **kw)
        assert gen.batcher._thread is None               # loop never started
        assert gen.sampled_batcher.stats["requests"] == 2
        gen.generate(["plain"], **kw)
        assert gen.batcher.stats["requests"] == 1
        # the loop itself refuses what it cannot sample
        with pytest.raises(ValueError, match="slot_sampling"):
            gen.batcher.generate("direct", top_p=0.9, **kw)
    finally:
        _stop(gen)


def test_parameters_reach_the_slot():
    """top_k = 1 and top_p = 1e-6 at T = 1 keep the arg-max alone, so the
    text equals the greedy one.  Condition, asserted through the raw engine:
    on each of the 8 greedy steps the two best fp32 logits differ by at
    least 1e-4 (a nearer runner-up could tie with tau, or flip the arg-max
    between batch shapes)."""
    eng, gen = _frontend(slot_sampling=True)
    try:
        n = 8
        sess = eng.make_slot_session(1)
        logits = eng.prefill_into_slots(sess, [0], [PROMPT], [n])
        ids = []
        for i in range(n):
            top2 = torch.topk(logits[0].float(), 2).values
            assert float(top2[0] - top2[1]) >= 1e-4, (i, top2.tolist())
            cur = logits.argmax(-1)
            ids.append(int(cur[0]))
            if i < n - 1:
                logits = eng.decode_step_session(sess, cur)
        greedy_text = eng.tokenizer.decode(ids)

        kw = dict(max_new_tokens=n, stop_on_eos=False)
        greedy = gen.generate([PROMPT], temperature=0.0, **kw)[0]
        assert greedy == greedy_text
        assert gen.generate([PROMPT], temperature=1.0, top_k=1, **kw)[0] \
            == greedy
        assert gen.generate([PROMPT], temperature=1.0, top_p=1e-6, **kw)[0] \
            == greedy
        assert gen.batcher.stats["requests"] == 3
        assert gen.sampled_batcher.stats["requests"] == 0
    finally:
        _stop(gen)


def test_mixed_residency():
    """A default and a top_p request queued BEFORE the loop starts: one
    admission takes both, so they are resident together whatever the
    timing."""
    from sentio_amd.serving.batcher import _make_item

    _, gen = _frontend(slot_sampling=True)
    try:
        a = _make_item("a default request", 6, 0.7, False)
        b = _make_item("a nucleus request", 6, 0.7, False, top_p=0.9)
        gen.batcher._q.put(a)
        gen.batcher._q.put(b)
        gen.batcher.start()
        ra, rb = a.future.result(timeout=60), b.future.result(timeout=60)
        assert isinstance(ra, str) and isinstance(rb, str)
        assert gen.batcher.stats["max_concurrent"] == 2
        assert gen.batcher.stats["completed"] == 2
        assert gen.sampled_batcher.stats["requests"] == 0
    finally:
        _stop(gen)
