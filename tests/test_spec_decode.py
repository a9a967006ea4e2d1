"""Prompt-lookup speculative decoding: ops.decode_attention_verify
(verify_attn_kernel), ops.ngram_draft / ops.spec_accept, Transformer.verify_step
and the engine loop.

Kernel shapes are the smallest at which it can go wrong: a wave takes 32 keys
per chunk in two 16-key MFMA tiles, a block has 4 or 8 waves, a split is one
block, the last split owns the T-token window.  Lengths 0 / 1 leave every
wave but the window's without a key, 15 / 16 / 17 straddle a tile, 33 a
chunk, 257 is ragged over the waves, Smax-T is the last window that fits and
Smax-1 overflows (no write, zero rows)."""

import functools

import pytest
import torch

gpu = pytest.mark.gpu
DEVICES = ["cpu", pytest.param("cuda:0", marks=gpu)]

HKV, SMAX = 2, 768
LOUD_ROWS = (3, 6)      # K scaled by 8
TOL = dict(rtol=3e-2, atol=3e-2)
SHAPES = [(128, 4, 4), (128, 4, 8), (128, 8, 4), (64, 7, 4), (64, 1, 2),
          (64, 2, 8)]
SPLITS = [None, "1", "2", "3"]
WAVES = ["4", "8"]


def _lens(T):
    # the overflowing row is last: the decode_qkv_prep calls below take the
    # rows in front of it
    return [0, 1, 15, 16, 17, 33, 257, SMAX - T, SMAX - 1]


@functools.lru_cache(maxsize=None)
def _verify_case(D, G, T):
    """CPU inputs and the fp32 reference (output and caches), once per shape."""
    from sentio_amd import ops

    lens = torch.tensor(_lens(T), dtype=torch.int32)
    B = lens.numel()
    g = torch.Generator().manual_seed(300 + D + 10 * G + T)
    kc = torch.randn(B, HKV, SMAX, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, HKV, SMAX, D, generator=g).to(torch.bfloat16)
    for b in LOUD_ROWS:
        kc[b] *= 8
    qkv = torch.randn(B * T, (G + 2) * HKV * D, generator=g).to(torch.bfloat16)
    cos, sin = ops.torch_ref.rope_tables(SMAX, D)
    want = ops.torch_ref.decode_attention_verify(
        qkv.float(), kc.float(), vc.float(), cos, sin, lens, T)
    return qkv, kc, vc, cos, sin, lens, want


@gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D,G,T", SHAPES)
def test_verify_attention_kernel(monkeypatch, D, G, T, splits, waves):
    """Output against the fp32 reference; the caches against T successive
    decode_qkv_prep calls on a clone, bit for bit, every other byte kept."""
    from sentio_amd import ops

    assert ops.hip_available(), "HIP extension must be built: no fallback"
    if splits is None:
        monkeypatch.delenv("SENTIO_DECODE_SPLITS", raising=False)
    else:
        monkeypatch.setenv("SENTIO_DECODE_SPLITS", splits)
    monkeypatch.setenv("SENTIO_DECODE_WAVES", waves)
    dev = "cuda:0"
    qkv, kc, vc, cos, sin, lens, want = _verify_case(D, G, T)
    qkv_d, cos_d, sin_d, lens_d = (t.to(dev) for t in (qkv, cos, sin, lens))
    kc_f, vc_f, kc_p, vc_p = kc.to(dev), vc.to(dev), kc.to(dev), vc.to(dev)
    B = lens.numel()

    got = ops.decode_attention_verify(qkv_d, kc_f, vc_f, cos_d, sin_d, lens_d,
                                      T)
    rows = qkv_d.view(B, T, -1)
    for t in range(T):
        n = B if t == 0 else B - 1      # the last row overflows from t = 1
        ops.decode_qkv_prep(rows[:n, t].contiguous(), kc_p, vc_p, cos_d,
                            sin_d, (lens_d[:n] + t).contiguous())
    torch.cuda.synchronize()

    assert lens_d.tolist() == lens.tolist()
    assert got.shape == (B * T, G * HKV * D)
    got = got.float().cpu()
    assert float(got.view(B, T, -1)[-1, 1:].abs().max()) == 0.0
    torch.testing.assert_close(got, want.float(), **TOL)
    bits = lambda t: t.cpu().view(torch.int16)
    assert torch.equal(bits(kc_f), bits(kc_p))
    assert torch.equal(bits(vc_f), bits(vc_p))
    written = torch.zeros(B, SMAX, dtype=torch.bool)
    for b, s in enumerate(lens.tolist()):
        written[b, s:min(s + T, SMAX)] = True
    keep = ~written[:, None, :, None].expand(B, HKV, SMAX, D)
    assert torch.equal(bits(kc_f)[keep], bits(kc)[keep])
    assert torch.equal(bits(vc_f)[keep], bits(vc)[keep])
    assert not torch.equal(bits(kc_f)[~keep], bits(kc)[~keep])


def test_verify_wrapper_rejects_bad_arguments():
    from sentio_amd import ops

    D, T = 64, 4
    kc = torch.zeros(2, 1, 16, D)
    qkv = torch.zeros(2 * T, 4 * D)
    cos, sin = ops.torch_ref.rope_tables(16, D)
    lens = torch.zeros(2, dtype=torch.int32)
    for bad, match in (
            (dict(T=1), "T must"), (dict(T=9), "T must"),
            (dict(qkv=torch.zeros(2 * T, 11 * D)), "at most 32"),
            (dict(qkv=qkv[:, :-8]), "qkv width"),
            (dict(qkv=qkv[:7]), "multiple of T"),
            (dict(seq_lens=lens.long()), "seq_lens"),
            (dict(kc=torch.zeros(2, 1, 16, 96)), "head dim")):
        a = dict(qkv=qkv, kc=kc, seq_lens=lens, T=T)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.decode_attention_verify(a["qkv"], a["kc"], a["kc"].clone(),
                                        cos, sin, a["seq_lens"], a["T"])


# ---- draft / accept bookkeeping against plain Python loops

def _draft_ref(h, room, K, n_max):
    if room <= 0:
        return []
    for n in range(min(n_max, len(h) - 1), 0, -1):
        hits = [i for i in range(len(h) - n) if h[i:i + n] == h[len(h) - n:]]
        full = [i for i in hits if i + n + K <= len(h)]
        if hits:
            start = (full or hits)[-1] + n
            return h[start:start + min(K, room)]
    return []


DRAFT_ROWS = [                               # (history, room)
    ([5, 6, 7, 8, 9], 9),                    # no match
    ([7, 1, 2, 3, 4, 5, 7], 9),              # match only at the start
    ([1, 2, 3] * 3 + [1], 9),                # periodic: K followers preferred
    ([1, 2, 3] * 3 + [1], 2),                # room clamps
    ([1, 2, 3] * 3 + [1], 0),                # no room
    ([1, 2, 3, 9, 9, 8, 3, 7, 7, 1, 2, 3], 9),   # longest n wins
    ([4, 4], 9),                             # shorter than n_max
    ([6, 5, 6, 5, 6], 9),                    # no occurrence has K followers
]


@pytest.mark.parametrize("dev", DEVICES)
def test_ngram_draft(dev):
    from sentio_amd import ops

    K, L = 4, 16
    hist = torch.tensor([h + [99] * (L - len(h)) for h, _ in DRAFT_ROWS],
                        dtype=torch.int64, device=dev)
    hist_len = torch.tensor([len(h) for h, _ in DRAFT_ROWS],
                            dtype=torch.int32, device=dev)
    room = torch.tensor([r for _, r in DRAFT_ROWS], dtype=torch.int32,
                        device=dev)
    draft, n_draft = ops.ngram_draft(hist, hist_len, room, K, 3)
    want = [_draft_ref(h, r, K, 3) for h, r in DRAFT_ROWS]
    assert [len(w) for w in want] == [0, 4, 4, 2, 0, 4, 1, 2]   # the cases bite
    assert want[2] == [2, 3, 1, 2] and want[5] == [9, 9, 8, 3]
    assert n_draft.tolist() == [len(w) for w in want]
    assert draft.tolist() == [w + [0] * (K - len(w)) for w in want]


@pytest.mark.parametrize("dev", DEVICES)
def test_spec_accept(dev):
    from sentio_amd import ops

    T, max_new, L = 5, 10, 12
    draft = [[1, 2, 3, 4]] * 6
    sampled = [[9, 2, 3, 4, 5],      # nothing accepted: one token
               [1, 2, 8, 4, 5],      # two accepted + the target's own
               [1, 2, 3, 4, 5],      # all four + the bonus token
               [1, 2, 3, 4, 5],      # budget leaves room for two
               [1, 2, 3, 4, 5],      # at its budget: nothing
               [1, 2, 3, 4, 5]]      # only one token was drafted
    n_draft, out_len0 = [4, 4, 4, 4, 4, 1], [1, 2, 3, 8, 10, 1]
    hist_len0, seq0 = [3, 4, 5, 6, 7, 3], [20, 21, 22, 23, 24, 25]
    B = len(sampled)
    ti = lambda x, dt: torch.tensor(x, dtype=dt, device=dev)
    out_buf = torch.full((B, max_new), -1, dtype=torch.int64, device=dev)
    hist = torch.full((B, L), -1, dtype=torch.int64, device=dev)
    out_len, hist_len = ti(out_len0, torch.int32), ti(hist_len0, torch.int32)
    seq, cur = ti(seq0, torch.int32), ti([77] * B, torch.int64)
    room = torch.zeros(B, dtype=torch.int32, device=dev)
    stats = ops.spec_accept(ti(sampled, torch.int64), ti(draft, torch.int64),
                            ti(n_draft, torch.int32), out_buf, out_len,
                            max_new, hist, hist_len, seq, cur, room=room,
                            smax=30)
    for b in range(B):
        a = 0
        while a < n_draft[b] and sampled[b][a] == draft[b][a]:
            a += 1
        e = max(0, min(a + 1, max_new - out_len0[b]))
        assert e == [1, 3, 5, 2, 0, 2][b]
        row = [-1] * max_new
        row[out_len0[b]:out_len0[b] + e] = sampled[b][:e]
        assert out_buf[b].tolist() == row
        row = [-1] * L
        row[hist_len0[b]:hist_len0[b] + e] = sampled[b][:e]
        assert hist[b].tolist() == row
        assert int(out_len[b]) == out_len0[b] + e
        assert int(hist_len[b]) == hist_len0[b] + e
        assert int(seq[b]) == seq0[b] + e
        assert int(cur[b]) == (sampled[b][e - 1] if e else 77)
        assert stats[b].tolist() == ([n_draft[b], min(a, e)] if e else [0, 0])
        assert int(room[b]) == min(max_new - out_len0[b] - e - 1,
                                   30 - 1 - seq0[b] - e)


# ---- model and engine

@gpu
def test_verify_step_matches_decode_steps():
    """verify_step over T tokens against T decode_steps from a copied cache;
    seq_lens untouched; captured replays equal the eager logits."""
    from sentio_amd.engines.configs import MODEL_CONFIGS
    from sentio_amd.engines.transformer import KVCache, Transformer

    dev, Bm, S, T = "cuda:0", 2, 24, 4
    cfg = MODEL_CONFIGS["llama3-1b"]
    m = Transformer(cfg, device=dev, dtype="bf16", seed=11)
    torch.manual_seed(7)
    toks = torch.randint(0, cfg.vocab_size, (Bm, S + T), device=dev)
    cache_a = KVCache(cfg, Bm, 64, dev, m.dtype)
    cache_b = KVCache(cfg, Bm, 64, dev, m.dtype)
    m.prefill(toks[:, :S], cache_a)
    m.prefill(toks[:, :S], cache_b)
    new = toks[:, S:].contiguous()

    got = m.verify_step(new, cache_a)
    assert cache_a.seq_lens.tolist() == [S, S]
    want = torch.stack([m.decode_step(new[:, t:t + 1], cache_b)
                        for t in range(T)], dim=1).view(Bm * T, -1)
    torch.cuda.synchronize()
    torch.testing.assert_close(got, want, rtol=5e-2, atol=5e-1)
    assert (got.argmax(-1) == want.argmax(-1)).all()

    static = new.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.verify_step(static, cache_a)              # warm-up before capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_logits = m.verify_step(static, cache_a)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert cache_a.seq_lens.tolist() == [S, S]
        assert torch.equal(static_logits, got)


PROMPTS = ["one a", "two b", "three c", "four d"]   # cycles 3, 5, EOS, long
MAX_NEW = 40


@functools.lru_cache(maxsize=None)
def _orbit_engine(model, dev):
    """An engine whose greedy decoding follows a permutation's orbit: wo and
    w_down zeroed, lm_head[pi(i)] = tok_emb[i]."""
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.engines.tokenizer import EOS_ID

    eng = GeneratorEngine(model, device=dev, max_seq=256)
    enc, lens = eng.tokenizer.encode_batch(PROMPTS, 64)
    last = [row[n - 1] for row, n in zip(enc, lens)]
    assert len(set(last)) == 4 and EOS_ID not in last
    free = iter(i for i in range(3000, 4000) if i not in last)
    fill = lambda n: [next(free) for _ in range(n)]
    cycles = [[last[0]] + fill(2), [last[1]] + fill(4),
              [last[2]] + fill(3) + [EOS_ID] + fill(2),
              [last[3]] + fill(MAX_NEW + 10)]
    pi = list(range(eng.cfg.vocab_size))
    for cyc in cycles:
        for i, tok in enumerate(cyc):
            pi[tok] = cyc[(i + 1) % len(cyc)]
    w = eng.model.w
    for layer in w.layers:
        layer["wo"].zero_()
        layer["w_down"].zero_()
    w.lm_head[torch.tensor(pi, device=w.lm_head.device)] = w.tok_emb
    want = []
    for tok in last:
        ids = []
        while len(ids) < MAX_NEW and pi[tok] != EOS_ID:
            tok = pi[tok]
            ids.append(tok)
        want.append(eng.tokenizer.decode(ids))
    return eng, want


@pytest.mark.parametrize("model,dev", [
    ("tiny-decoder", "cpu"),
    pytest.param("tiny-decoder64", "cuda:0", marks=gpu)])
def test_engine_speculative_bookkeeping(model, dev):
    eng, want = _orbit_engine(model, dev)
    gen = lambda p, **kw: eng.generate(p, max_new_tokens=MAX_NEW,
                                       temperature=0.0, **kw)
    assert gen(PROMPTS, speculative=0) == want
    assert gen(PROMPTS, speculative=4) == want
    assert eng.last_spec["accepted"] > 0
    assert gen(PROMPTS[:1], speculative=4) == want[:1]
    assert eng.last_decode_steps <= 20
    assert eng.last_spec["steps"] == eng.last_decode_steps
    assert 0 < eng.last_spec["accepted"] <= eng.last_spec["drafted"]
    assert "".join(eng.stream(PROMPTS[2], MAX_NEW, 0.0, speculative=4)) \
        == want[2]
    if dev == "cpu":
        seeded = lambda k: eng.generate(PROMPTS, max_new_tokens=MAX_NEW,
                                        temperature=0.7, seed=1,
                                        speculative=k)
        assert seeded(4) == seeded(0)


def test_speculative_unsupported_combinations_raise():
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.engines.grammar import Grammar
    from sentio_amd.parallel.tp import TPContext

    eng = GeneratorEngine("tiny-decoder64", device="cpu", spec_tokens=2)
    grammar = Grammar.from_regex(r"[0-9]{1,3}")
    with pytest.raises(ValueError, match="grammar"):
        eng.generate(["p"], 8, speculative=2, grammar=grammar)
    with pytest.raises(ValueError, match="on_token"):
        eng.generate(["p"], 8, speculative=2, on_token=lambda s, t: None)
    with pytest.raises(ValueError, match="grammar"):
        next(eng.stream("p", 8, speculative=2, grammar=grammar))
    with pytest.raises(ValueError, match=r"\[0, 7\]"):
        eng.generate(["p"], 8, speculative=8)
    # the engine default runs the loop, on a head dim the GPU kernel lacks too
    dflt = GeneratorEngine("tiny-decoder", device="cpu", spec_tokens=2)
    text = dflt.generate(["p q p q p q"], 12, temperature=0.0)
    assert dflt.last_spec["steps"] > 0 and dflt.last_decode_steps <= 11
    assert text == dflt.generate(["p q p q p q"], 12, temperature=0.0,
                                 speculative=0)
    assert list(dflt.stream("p", 0)) == []
    # where it cannot serve a call it gives way to the one-token path
    seen = []
    eng.last_spec = None
    eng.generate(["p"], 4, on_token=lambda s, t: seen.append(s))
    assert seen == [0, 1, 2, 3] and eng.last_spec is None
    fp8 = GeneratorEngine("tiny-decoder64", device="cpu",
                          kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        fp8.generate(["p"], 8, speculative=2)
    tp = GeneratorEngine("tiny-decoder", device="cpu",
                         tp=TPContext(rank=0, world=2))
    with pytest.raises(ValueError, match="tensor parallel"):
        tp.generate(["p"], 8, speculative=2)


def test_settings_spec_decode_tokens(monkeypatch):
    from sentio_amd.config import Settings

    monkeypatch.delenv("SPEC_DECODE_TOKENS", raising=False)
    assert Settings.from_env().spec_decode_tokens == 0
    monkeypatch.setenv("SPEC_DECODE_TOKENS", "4")
    assert Settings.from_env().spec_decode_tokens == 4
    monkeypatch.setenv("SPEC_DECODE_TOKENS", "9")
    with pytest.raises(ValueError, match="SPEC_DECODE_TOKENS"):
        Settings.from_env()
