"""Penalties off the GPU: the spec (torch_ref.apply_penalties) against a
per-token loop, then the engine keywords, the settings and the batcher."""

import math

import numpy as np
import pytest
import torch


def _by_hand(logits, out_buf, out_len, rep, freq, pres):
    """Every operation in float64, rounded to fp32 at once (exact for one
    +, -, * or / of fp32 operands)."""
    f32, f64 = np.float32, np.float64
    out = logits.clone()
    for b in range(logits.shape[0]):
        hist = out_buf[b, :min(int(out_len[b]), out_buf.shape[1])].tolist()
        for v in {t for t in hist if 0 <= t < logits.shape[1]}:
            x = f32(logits[b, v])
            x = f32(-math.inf) if math.isnan(x) else x
            r, f, p = f32(rep[b]), f32(freq[b]), f32(pres[b])
            x = f32(f64(x) * f64(r)) if x < 0 else f32(f64(x) / f64(r))
            x = f32(f64(x) - f64(f32(f64(f) * f64(hist.count(v)))))
            out[b, v] = float(f32(f64(x) - f64(p)))
    return out.nan_to_num(nan=123.0)


@pytest.mark.parametrize("V", (67, 4097))
def test_apply_penalties_equals_the_per_token_loop(V):
    from sentio_amd.ops import torch_ref

    g = torch.Generator().manual_seed(V)
    hists = ([], [V - 1], [7] * 300 + [9], torch.randperm(V, generator=g)
             .tolist()[:4096], [3, V, -1, 3, 5, V + 70000])
    out_buf = torch.zeros(5, 4096, dtype=torch.int64)
    for b, h in enumerate(hists):
        out_buf[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
    out_len = torch.tensor([len(h) for h in hists], dtype=torch.int32)
    out_len[2] = 4101                       # clamped to L: counts the zeros
    logits = 3.0 * torch.randn(5, V, generator=g)
    logits[:, 7], logits[:, 3], logits[:, 5] = -math.inf, math.nan, math.inf
    for pens in ((torch.tensor([1.3, 0.7, 2.0, 1.1, 9.99]),
                  torch.tensor([0.4, -0.3, 1.1, 2.0, -2.0]),
                  torch.tensor([0.6, 1.5, -0.2, 0.1, 0.3])),
                 (torch.ones(5), torch.zeros(5), torch.zeros(5))):
        got = torch_ref.apply_penalties(logits, out_buf, out_len, *pens)
        assert got.dtype == torch.float32
        assert torch.equal(got.nan_to_num(nan=123.0),
                           _by_hand(logits, out_buf, out_len, *pens))


def test_engine_keyword_contract(monkeypatch):
    from sentio_amd import ops
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.engines.grammar import Grammar

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=96,
                          spec_tokens=2)
    kw = dict(max_new_tokens=5, temperature=0.0, stop_on_eos=False)
    calls, real = [], ops.sample_penalized
    monkeypatch.setattr(ops, "sample_penalized",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    assert eng.generate(["alpha beta"], repetition_penalty=1.0,
                        frequency_penalty=0.0, presence_penalty=0.0,
                        **kw) == eng.generate(["alpha beta"], **kw)
    assert calls == []                      # neutral: the old path
    # the engine's default speculation gives way to the one-token path
    monkeypatch.setattr(eng, "_spec_step", lambda *a, **k: pytest.fail("spec"))
    eng.generate(["alpha beta"], presence_penalty=0.5, **kw)
    list(eng.stream("alpha beta", max_new_tokens=3, repetition_penalty=1.2))
    assert len(calls) == 5 + 3
    for bad in (dict(repetition_penalty=0.0), dict(frequency_penalty=2.5),
                dict(presence_penalty=-2.5),
                dict(frequency_penalty=0.5, speculative=2),
                dict(frequency_penalty=0.5,
                     grammar=Grammar.from_regex("[0-9]{1,3}"))):
        with pytest.raises(ValueError):
            eng.generate(["alpha"], max_new_tokens=4, **bad)
        with pytest.raises(ValueError):
            list(eng.stream("alpha", max_new_tokens=4, **bad))


def test_settings_and_request_defaults(monkeypatch):
    from sentio_amd.config import Settings
    from sentio_amd.serving.handlers import resolve_sampling

    assert resolve_sampling(Settings()) == {}
    want = {"repetition_penalty": 1.15, "frequency_penalty": 0.4,
            "presence_penalty": -0.5}
    for key, value in want.items():
        monkeypatch.setenv("GEN_" + key.upper(), str(value))
    s = Settings.from_env()
    assert {k: getattr(s, "gen_" + k) for k in want} == want
    assert resolve_sampling(s) == want
    # a request's own value wins, "off" included
    assert resolve_sampling(s, repetition_penalty=1.0, frequency_penalty=0.0,
                            presence_penalty=0.7) == {"presence_penalty": 0.7}


@pytest.mark.parametrize("slot_sampling", (False, True))
def test_batcher_routes_a_penalised_request_to_its_own_wave(slot_sampling):
    from types import SimpleNamespace

    from sentio_amd.serving import batcher

    calls = []
    raw = SimpleNamespace(tokenizer=None, generate=lambda prompts, **kw: (
        calls.append(kw) or ["wave"] * len(prompts)))
    front = batcher.ContinuousGenerator(raw, slots=2,
                                        slot_sampling=slot_sampling)
    try:
        assert front.generate(["q"], max_new_tokens=4, top_p=0.9,
                              frequency_penalty=0.5) == ["wave"]
        assert calls[-1]["frequency_penalty"] == 0.5
        with pytest.raises(ValueError):     # never the slot loop
            front.batcher.generate("q", presence_penalty=0.5)
    finally:
        front.sampled_batcher.stop()
    keys = {batcher._make_item("q", 4, 0.3, True, top_p=0.9, **kw).group_key
            for kw in ({}, dict(frequency_penalty=0.5),
                       dict(frequency_penalty=0.6),
                       dict(presence_penalty=0.5))}
    assert len(keys) == 4
    assert type(batcher._make_item("q", 4, 0.3, True)) is batcher._Item
