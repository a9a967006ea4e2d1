"""ops.sample_penalized against torch_ref.apply_penalties +
ops.sample_filtered: the same sampling arithmetic, so the tokens are equal."""

import math

import pytest
import torch

from sentio_amd import ops
from sentio_amd.ops import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

VOCABS = (4097, 32000, 152064)
L = 4096
PARAMS = ((0.0, 0, 1.0), (0.8, 8, 0.9), (1.0, 0, 0.5))


def _history(kind: str, V: int) -> list[int]:
    g = torch.Generator().manual_seed(V + len(kind))
    if kind == "colliding":
        # ids of 16 neighbouring slots of the kernel's hash, from the fullest
        # on: shared slots and probe chains (V <= 8192 ids never collide)
        v = torch.arange(V, dtype=torch.int64)
        h = ((v * 0x9E3779B1) & 0xFFFFFFFF) >> 19
        fill = torch.bincount(h, minlength=8192)
        ids = v[((h - int(fill.argmax())) % 8192) < 16].tolist()
        assert len(ids) >= 9 and (V <= 8192 or int(fill.max()) >= 6)
        return ids + ids[::-1] + ids[:1]
    return {"empty": [], "one": [V - 1], "repeat300": [7] * 300 + [V - 2, 11],
            # a full row of distinct ids: the table at its load bound
            "distinct4096": torch.randperm(V, generator=g)[:L].tolist(),
            "out_of_range": [3, V, -1, V + 70000, 3, 5, -(2 ** 40)],
            "random": torch.randint(0, V, (301,), generator=g).tolist()}[kind]


def _inputs(kinds, V: int):
    """logits with +, -, -inf and NaN at penalised positions; out_buf [B, L]
    and out_len of `kinds`."""
    g = torch.Generator().manual_seed(V)
    logits = 3.0 * torch.randn(len(kinds), V, generator=g)
    out_buf = torch.zeros(len(kinds), L, dtype=torch.int64)
    out_len = torch.zeros(len(kinds), dtype=torch.int32)
    for b, kind in enumerate(kinds):
        h = _history(kind, V)
        out_buf[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
        out_len[b] = len(h)
        seen = [t for t in dict.fromkeys(h) if 0 <= t < V]
        for t, x in zip(seen, (2.5, -2.5, -math.inf, math.nan, 9.0, -9.0)):
            logits[b, t] = x
    return logits.to(DEV), out_buf.to(DEV), out_len.to(DEV)


def _params(params):
    T, k, p = params
    return (torch.full((3,), T, device=DEV),
            torch.full((3,), k, dtype=torch.int32, device=DEV),
            torch.full((3,), p, device=DEV),
            torch.arange(3, dtype=torch.int64, device=DEV) + 41)


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("params", PARAMS)
def test_neutral_penalties_equal_sample_filtered(V, params):
    logits, out_buf, out_len = _inputs(("random", "repeat300", "one"), V)
    step = torch.tensor([0, 5, 77], dtype=torch.int32, device=DEV)
    ref = ops.sample_filtered(logits, *_params(params), step)
    buf0, len0, step0 = out_buf.clone(), out_len.clone(), step.clone()
    tok = ops.sample_penalized(logits, *_params(params), step, out_buf,
                               out_len, 1.0, 0.0, 0.0)
    assert torch.equal(tok, ref)
    assert torch.equal(out_len, len0 + 1) and torch.equal(step, step0 + 1)
    buf0[torch.arange(3, device=DEV), len0.long()] = tok
    assert torch.equal(out_buf, buf0)


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("kinds", (("empty", "one", "repeat300"),
                                   ("distinct4096", "colliding",
                                    "out_of_range")))
def test_equals_filtered_sampling_of_penalised_logits(V, params, kinds):
    logits, out_buf, out_len = _inputs(kinds, V)
    step = torch.tensor([3, 0, 9], dtype=torch.int32, device=DEV)
    pens = (torch.tensor([1.3, 0.7, 2.0]), torch.tensor([0.4, -0.3, 1.1]),
            torch.tensor([0.6, 1.5, -0.2]))
    pen = torch_ref.apply_penalties(logits, out_buf, out_len, *pens)
    assert pen.device == logits.device and pen.dtype == torch.float32
    ref = ops.sample_filtered(pen, *_params(params), step)
    buf0, len0 = out_buf.clone(), out_len.clone()
    tok = ops.sample_penalized(logits, *_params(params), step, out_buf,
                               out_len, *pens)
    assert torch.equal(tok, ref) and step.tolist() == [4, 1, 10]
    # a full row (out_len == L) samples but appends nothing
    assert torch.equal(out_len, len0 + (len0 < L))
    assert torch.equal(out_buf[len0 == L], buf0[len0 == L])


@pytest.mark.parametrize("xa,xr,count,rep,freq,pres,winner", (
    (2.0, 1.5, 3, 2.0, 0.0, 0.0, "r"),      # 2 / 2 = 1 < 1.5
    (-1.0, -1.5, 3, 2.0, 0.0, 0.0, "r"),    # -1 * 2 = -2 (-1 / 2 would win)
    (2.0, 1.5, 3, 1.0, 0.25, 0.0, "r"),     # 2 - 3 * 0.25 = 1.25
    (2.0, 1.5, 1, 1.0, 0.25, 0.0, "a"),     # 2 - 1 * 0.25 = 1.75
    (2.0, 1.5, 3, 1.0, 0.0, 0.75, "r"),     # once, whatever the count: 1.25
    (2.0, 1.5, 3, 1.0, 0.0, 0.25, "a"),     # 1.75
))
def test_greedy_winner_flips_as_worked_out_by_hand(xa, xr, count, rep,
                                                   freq, pres, winner):
    V, a, r = 4097, 4096, 1234
    logits = torch.full((1, V), -10.0, device=DEV)
    logits[0, a], logits[0, r] = xa, xr
    out_buf = torch.full((1, 16), a, dtype=torch.int64, device=DEV)
    out_len = torch.tensor([count], dtype=torch.int32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    tok = ops.sample_penalized(logits, 0.0, 0, 1.0, 0, step, out_buf, out_len,
                               rep, freq, pres)
    assert int(tok) == (a if winner == "a" else r)


@pytest.mark.parametrize("change", (
    dict(rep=0.0), dict(rep=-1.0), dict(rep=10.5), dict(freq=2.5),
    dict(freq=-2.5), dict(pres=2.5), dict(L=4097), dict(V=1 << 18),
    dict(step=torch.int64), dict(out_len=torch.int64),
    dict(out_buf=torch.int32)))
def test_bad_arguments_raise_before_any_launch(monkeypatch, change):
    monkeypatch.setattr(ops, "_require_hip", lambda: pytest.fail("launched"))
    c = dict(rep=1.2, freq=0.1, pres=0.1, L=8, V=64, step=torch.int32,
             out_len=torch.int32, out_buf=torch.int64)
    c.update(change)
    with pytest.raises(ValueError):
        ops.sample_penalized(
            torch.zeros(2, c["V"], device=DEV), 0.0, 0, 1.0, 0,
            torch.zeros(2, dtype=c["step"], device=DEV),
            torch.zeros(2, c["L"], dtype=c["out_buf"], device=DEV),
            torch.zeros(2, dtype=c["out_len"], device=DEV),
            c["rep"], c["freq"], c["pres"])


def _looping_tokens(device: str, **kw) -> list[int]:
    """tiny-decoder64 made to give logits 4.5 / 3.25 / 2 for tokens 1000 /
    2000 / 3000 and -8 elsewhere, whatever came before: greedy decoding
    loops on 1000.  Exact in bf16 and 0.25 apart modulo the penalty 0.75."""
    from sentio_amd.engines.generator import GeneratorEngine

    eng = GeneratorEngine("tiny-decoder64", device=device, max_seq=128)
    w = eng.model.w
    for layer in w.layers:
        layer["wo"].zero_()
        layer["w_down"].zero_()
    rows = torch.arange(w.tok_emb.shape[0])
    w.tok_emb.zero_()
    w.tok_emb[rows, rows % w.tok_emb.shape[1]] = 1.0
    w.lm_head.fill_(-8.0 / 16)
    for t, x in ((1000, 4.5), (2000, 3.25), (3000, 2.0)):
        w.lm_head[t] = x / 16
    seen = []
    eng.generate(["loop"], max_new_tokens=12, temperature=0.0,
                 stop_on_eos=False, on_token=lambda _s, t: seen.append(t[0]),
                 **kw)
    return seen


def test_engine_penalty_breaks_a_greedy_loop_like_the_cpu_engine():
    plain = _looping_tokens(DEV)
    assert plain == [1000] * 12
    assert _looping_tokens(DEV, repetition_penalty=1.0, presence_penalty=0.0,
                           frequency_penalty=0.0) == plain
    out = _looping_tokens(DEV, frequency_penalty=0.75)
    assert out == _looping_tokens("cpu", frequency_penalty=0.75)
    assert out[:3] == [1000, 1000, 2000] and 3000 in out
