"""Wave-private decode attention and its fused RoPE + KV-write variant
(ops.decode_attention / ops.decode_attention_fused) against the fp32
references in ops.torch_ref, at the tolerance of the other decode tests.

Shapes are the smallest at which the kernel can go wrong: a wave takes 32
keys per batch (16 for G > 4, 8 for G > 6), a block has 4 or 8 waves, a
split is one block.  Lengths 1 and 31 leave most groups, waves and splits
without a key (the -inf merges), 32/33 straddle one batch of a wave, 257 is
a ragged second tile, 768 the full cache."""

import functools

import pytest
import torch

gpu = pytest.mark.gpu

B, HKV, SMAX = 7, 2, 768
LENS = [1, 31, 32, 33, 257, 700, 768]
POSITIONS = [0, 1, 255, 256, 700, 766, 767]
LOUD_ROWS = (3, 5)      # K scaled by 8: score scale far from the other rows
TOL = dict(rtol=3e-2, atol=3e-2)

SPLITS = [None, "1", "2", "3"]
WAVES = ["4", "8"]
HEADS = [(D, G) for D in (128, 64) for G in (1, 4, 7)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sentio_amd import ops

    assert ops.hip_available(), (
        "HIP extension must be built/loaded on a GPU box — no eager fallback")
    return "cuda:0"


def _set_env(monkeypatch, splits, waves):
    if splits is None:
        monkeypatch.delenv("SENTIO_DECODE_SPLITS", raising=False)
    else:
        monkeypatch.setenv("SENTIO_DECODE_SPLITS", splits)
    monkeypatch.setenv("SENTIO_DECODE_WAVES", waves)


def _caches(D, seed):
    g = torch.Generator().manual_seed(seed)
    kc = torch.randn(B, HKV, SMAX, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, HKV, SMAX, D, generator=g).to(torch.bfloat16)
    for b in LOUD_ROWS:
        kc[b] *= 8
    return kc, vc, g


@functools.lru_cache(maxsize=None)
def _attn_case(D, G):
    """CPU inputs and the fp32 reference, computed once per (D, G)."""
    from sentio_amd import ops

    kc, vc, g = _caches(D, 100 + D + G)
    q = torch.randn(B, G * HKV, D, generator=g).to(torch.bfloat16)
    lens = torch.tensor(LENS, dtype=torch.int32)
    want = ops.torch_ref.decode_attention(q.float(), kc.float(), vc.float(),
                                          lens)
    return q, kc, vc, lens, want


@functools.lru_cache(maxsize=None)
def _fused_case(D, G):
    from sentio_amd import ops

    kc, vc, g = _caches(D, 200 + D + G)
    qkv = torch.randn(B, (G + 2) * HKV * D, generator=g).to(torch.bfloat16)
    cos, sin = ops.torch_ref.rope_tables(SMAX, D)
    pos = torch.tensor(POSITIONS, dtype=torch.int32)
    want = ops.torch_ref.decode_attention_fused(
        qkv.float(), kc.float(), vc.float(), cos, sin, pos)
    return qkv, kc, vc, cos, sin, pos, want


@gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D,G", HEADS)
def test_wave_private_merge_edges(dev, monkeypatch, D, G, splits, waves):
    from sentio_amd import ops

    _set_env(monkeypatch, splits, waves)
    q, kc, vc, lens, want = _attn_case(D, G)
    got = ops.decode_attention(q.to(dev), kc.to(dev), vc.to(dev),
                               lens.to(dev))
    torch.testing.assert_close(got.float().cpu(), want, **TOL)


@gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D,G", HEADS)
def test_fused_matches_two_op_path(dev, monkeypatch, D, G, splits, waves):
    """Output against torch_ref; the caches against what decode_qkv_prep
    writes on a clone, bit for bit, and untouched everywhere else."""
    from sentio_amd import ops

    _set_env(monkeypatch, splits, waves)
    qkv, kc, vc, cos, sin, pos, want = _fused_case(D, G)
    qkv_d, cos_d, sin_d, pos_d = (t.to(dev) for t in (qkv, cos, sin, pos))
    kc_f, vc_f = kc.to(dev), vc.to(dev)
    kc_p, vc_p = kc.to(dev), vc.to(dev)

    got = ops.decode_attention_fused(qkv_d, kc_f, vc_f, cos_d, sin_d, pos_d)
    ops.decode_qkv_prep(qkv_d, kc_p, vc_p, cos_d, sin_d, pos_d)
    torch.cuda.synchronize()

    torch.testing.assert_close(got.float().cpu(), want, **TOL)
    kc_f, vc_f, kc_p, vc_p = (t.cpu() for t in (kc_f, vc_f, kc_p, vc_p))
    rows = torch.tensor(POSITIONS, dtype=torch.long)
    bidx = torch.arange(B)
    # bf16 payloads compared as raw bits
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(kc_f[bidx, :, rows]), bits(kc_p[bidx, :, rows]))
    assert torch.equal(bits(vc_f[bidx, :, rows]), bits(vc_p[bidx, :, rows]))
    # the prep kernel really wrote something there
    assert not torch.equal(bits(kc_p[bidx, :, rows]), bits(kc[bidx, :, rows]))
    other = torch.ones(B, SMAX, dtype=torch.bool)
    other[bidx, rows] = False
    other = other[:, None, :, None].expand(B, HKV, SMAX, D)
    assert torch.equal(bits(kc_f)[other], bits(kc)[other])
    assert torch.equal(bits(vc_f)[other], bits(vc)[other])


@gpu
def test_model_decode_through_fused_path(dev):
    """Construction of test_forward_decode_matches_prefill: the decode step
    (now the fused op) agrees with prefill; two steps advance seq_lens and
    fill rows S and S+1; a hipGraph-captured step replays to the same
    logits."""
    from sentio_amd import ops
    from sentio_amd.engines.configs import MODEL_CONFIGS
    from sentio_amd.engines.transformer import KVCache, Transformer

    cfg = MODEL_CONFIGS["llama3-1b"]
    m = Transformer(cfg, device=dev, dtype="bf16", seed=11)
    assert m.decode_attn is ops.decode_attention
    Bm, S = 2, 24
    torch.manual_seed(7)
    toks = torch.randint(0, cfg.vocab_size, (Bm, S + 2), device=dev)

    cache_a = KVCache(cfg, Bm, 64, dev, m.dtype)
    logits_all = m.prefill(toks[:, :S + 1], cache_a)

    cache_b = KVCache(cfg, Bm, 64, dev, m.dtype)
    m.prefill(toks[:, :S], cache_b)
    assert cache_b.seq_lens.tolist() == [S, S]
    logits_dec = m.decode_step(toks[:, S:S + 1], cache_b)
    torch.cuda.synchronize()
    assert (logits_all.argmax(-1) == logits_dec.argmax(-1)).all()
    torch.testing.assert_close(logits_all, logits_dec, rtol=5e-2, atol=5e-1)
    assert cache_b.seq_lens.tolist() == [S + 1, S + 1]

    # second step, eager and captured, from the same cache state
    cache_g = KVCache(cfg, Bm, 64, dev, m.dtype)
    for i in range(cfg.n_layers):
        cache_g.k[i].copy_(cache_b.k[i])
        cache_g.v[i].copy_(cache_b.v[i])
    cache_g.seq_lens.copy_(cache_b.seq_lens)

    logits_2 = m.decode_step(toks[:, S + 1:S + 2], cache_b)
    torch.cuda.synchronize()
    assert cache_b.seq_lens.tolist() == [S + 2, S + 2]
    for kv in (cache_b.k, cache_b.v):
        for layer in (0, cfg.n_layers - 1):
            assert (kv[layer][:, :, S].float().abs().sum(-1) > 0).all()
            assert (kv[layer][:, :, S + 1].float().abs().sum(-1) > 0).all()
            assert float(kv[layer][:, :, S + 2:].float().abs().sum()) == 0.0

    static_tok = toks[:, S + 1:S + 2].clone()
    saved = cache_g.seq_lens.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.decode_step(static_tok, cache_g)          # warm-up before capture
    torch.cuda.current_stream().wait_stream(side)
    cache_g.seq_lens.copy_(saved)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_logits = m.decode_step(static_tok, cache_g)
    cache_g.seq_lens.copy_(saved)
    graph.replay()
    torch.cuda.synchronize()
    assert cache_g.seq_lens.tolist() == [S + 2, S + 2]
    torch.testing.assert_close(static_logits, logits_2, rtol=5e-2, atol=5e-1)
    assert (static_logits.argmax(-1) == logits_2.argmax(-1)).all()


@gpu
def test_fused_binding_rejects_bad_arguments(dev):
    from sentio_amd import ops
    from sentio_amd.ops import _sentio_hip as hip

    D, G = 128, 4
    qkv, kc, vc, cos, sin, pos, _ = _fused_case(D, G)
    qkv, kc, vc, cos, sin, pos = (t.to(dev) for t in
                                  (qkv, kc, vc, cos, sin, pos))
    before = kc.clone()
    with pytest.raises(RuntimeError, match="qkv width"):
        hip.decode_attn_fused(qkv[:, :-D].contiguous(), kc, vc, cos, sin,
                              pos, 0.1)
    with pytest.raises(RuntimeError, match="seq_lens"):
        hip.decode_attn_fused(qkv, kc, vc, cos, sin, pos.long(), 0.1)
    with pytest.raises(RuntimeError, match="seq_lens"):
        hip.decode_attn_fused(qkv, kc, vc, cos, sin,
                              pos.repeat_interleave(2)[::2], 0.1)
    D96 = 96
    kc96 = torch.zeros(B, HKV, 32, D96, dtype=torch.bfloat16, device=dev)
    qkv96 = torch.zeros(B, (G + 2) * HKV * D96, dtype=torch.bfloat16,
                        device=dev)
    cos96, sin96 = ops.torch_ref.rope_tables(32, D96, device=dev)
    with pytest.raises(RuntimeError, match="head dim"):
        hip.decode_attn_fused(qkv96, kc96, kc96.clone(), cos96, sin96, pos,
                              0.1)
    torch.cuda.synchronize()
    assert torch.equal(kc, before)      # nothing was launched


# ---- launcher contract and policy, no GPU needed

def _cpu_fused_args(D=64, G=2, smax=16):
    from sentio_amd import ops

    kc = torch.zeros(2, 1, smax, D)
    vc = torch.zeros(2, 1, smax, D)
    qkv = torch.randn(2, (G + 2) * D)
    cos, sin = ops.torch_ref.rope_tables(smax, D)
    pos = torch.tensor([0, 5], dtype=torch.int32)
    return qkv, kc, vc, cos, sin, pos


def test_fused_wrapper_contract_cpu():
    from sentio_amd import ops

    qkv, kc, vc, cos, sin, pos = _cpu_fused_args()
    with pytest.raises(ValueError, match="qkv width"):
        ops.decode_attention_fused(qkv[:, :-8], kc, vc, cos, sin, pos)
    with pytest.raises(ValueError, match="seq_lens"):
        ops.decode_attention_fused(qkv, kc, vc, cos, sin, pos.long())
    with pytest.raises(ValueError, match="seq_lens"):
        ops.decode_attention_fused(qkv, kc, vc, cos, sin, pos[:1])
    q96, k96, v96, c96, s96, p96 = _cpu_fused_args(D=96)
    with pytest.raises(ValueError, match="head dim"):
        ops.decode_attention_fused(q96, k96, v96, c96, s96, p96)
    assert float(kc.abs().sum()) == 0.0 and float(vc.abs().sum()) == 0.0


def test_fused_cpu_reference_composes_the_two_ops():
    from sentio_amd import ops

    qkv, kc, vc, cos, sin, pos = _cpu_fused_args()
    torch.manual_seed(3)
    kc.normal_()
    vc.normal_()
    kc2, vc2 = kc.clone(), vc.clone()
    got = ops.decode_attention_fused(qkv, kc, vc, cos, sin, pos)
    q = ops.decode_qkv_prep(qkv, kc2, vc2, cos, sin, pos)
    want = ops.decode_attention(q, kc2, vc2, pos + 1)
    torch.testing.assert_close(got, want)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert got.shape == (2, 2, 64)


def test_decode_attn_plan(monkeypatch):
    """(splits, waves): one 8-wave block per (b, kv-head) once B*Hkv fills
    the 256 CUs, split-S over 4-wave blocks below; env overrides clamp."""
    from sentio_amd import ops

    if not ops.hip_available():
        pytest.skip("extension not built")
    plan = ops._require_hip().decode_attn_plan
    monkeypatch.delenv("SENTIO_DECODE_SPLITS", raising=False)
    monkeypatch.delenv("SENTIO_DECODE_WAVES", raising=False)
    assert plan(32, 8, 2120) == (1, 8)          # flagship
    assert plan(64, 8, 2120) == (1, 8)
    assert plan(16, 8, 2120) == (4, 4)          # ceil(512/128)
    assert plan(4, 2, 768) == (3, 4)            # 64 clamped to 768/256
    assert plan(4, 2, 200) == (1, 4)            # short cache: never split
    monkeypatch.setenv("SENTIO_DECODE_SPLITS", "2")
    assert plan(32, 8, 2120) == (2, 8)
    assert plan(4, 2, 200) == (1, 4)
    monkeypatch.setenv("SENTIO_DECODE_SPLITS", "0")
    assert plan(16, 8, 2120) == (1, 4)
    monkeypatch.setenv("SENTIO_DECODE_SPLITS", "99")
    assert plan(16, 8, 2120) == (8, 4)
    monkeypatch.delenv("SENTIO_DECODE_SPLITS")
    monkeypatch.setenv("SENTIO_DECODE_WAVES", "4")
    assert plan(32, 8, 2120) == (1, 4)
    monkeypatch.setenv("SENTIO_DECODE_WAVES", "16")
    with pytest.raises(RuntimeError, match="SENTIO_DECODE_WAVES"):
        plan(32, 8, 2120)
