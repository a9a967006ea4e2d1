"""ops.prefill_qkv_prep on the GPU: the fused kernel against the ops it
replaces (rope_apply on contiguous slices plus the indexed cache writes),
bit for bit; its rejections; and the fused route of Transformer against
SENTIO_PREFILL_PREP=legacy at model level.

The kernel and rope_kernel share one rotation helper in one translation
unit, so equality is exact, not a tolerance.  At model level the attention
kernel is the same template on both routes (only the K/V addressing
differs), so logits and cache contents are compared with torch.equal too.
"""

from __future__ import annotations

import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(128, 4, 2), (64, 4, 4), (64, 7, 1), (16, 4, 2)]   # D, H, Hkv
K_FILL, V_FILL = -7.0, -9.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(autouse=True)
def _require_hip_ext():
    from sentio_amd import ops

    if torch.cuda.is_available():
        assert ops.hip_available(), "HIP extension must be built on a GPU box"


def _inputs(D, H, Hkv, B, S, rows, dev, seed):
    from sentio_amd.ops import torch_ref

    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g).to(
        device=dev, dtype=torch.bfloat16)
    cos, sin = torch_ref.rope_tables(rows, D, 10000.0, dev)
    return qkv, cos, sin


def _legacy_ops(qkv, cos, sin, pos0, H, Hkv, kc=None, vc=None):
    """Transformer._attn's legacy sequence on the existing GPU ops."""
    from sentio_amd import ops

    B, S, W = qkv.shape
    D = W // (H + 2 * Hkv)
    pos = torch.arange(pos0, pos0 + S, device=qkv.device
                       ).unsqueeze(0).expand(B, S)
    q_end, k_end = H * D, (H + Hkv) * D
    q = qkv[..., :q_end].reshape(B, S, H, D)
    k = qkv[..., q_end:k_end].reshape(B, S, Hkv, D)
    v = qkv[..., k_end:].reshape(B, S, Hkv, D)
    q = ops.rope_apply(q, cos, sin, pos)
    k = ops.rope_apply(k, cos, sin, pos)
    if kc is not None:
        bidx = torch.arange(B, device=qkv.device).unsqueeze(1).expand(B, S)
        kc[bidx.reshape(-1), :, pos.reshape(-1)] = k.reshape(B * S, Hkv, D)
        vc[bidx.reshape(-1), :, pos.reshape(-1)] = v.reshape(B * S, Hkv, D)
    return q, k, v


@pytest.mark.parametrize("D,H,Hkv", SHAPES)
@pytest.mark.parametrize("S", [1, 5, 37])
def test_kernel_equals_rope_and_indexed_writes(dev, D, H, Hkv, S):
    from sentio_amd import ops

    B, Bc = 2, 3
    for pos0 in (0, 3):
        qkv, cos, sin = _inputs(D, H, Hkv, B, S, pos0 + S, dev,
                                seed=1000 * D + 10 * S + pos0)
        wq, wk, wv = _legacy_ops(qkv, cos, sin, pos0, H, Hkv)
        q, k, v = ops.prefill_qkv_prep(qkv, cos, sin, pos0, H, Hkv)
        for got, want in ((q, wq), (k, wk), (v, wv)):
            assert got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got, want)
        for slack in (0, 9):
            Smax = pos0 + S + slack
            kc = torch.full((Bc, Hkv, Smax, D), K_FILL, device=dev,
                            dtype=torch.bfloat16)
            vc = torch.full((Bc, Hkv, Smax, D), V_FILL, device=dev,
                            dtype=torch.bfloat16)
            kc2, vc2 = kc.clone(), vc.clone()
            _legacy_ops(qkv, cos, sin, pos0, H, Hkv, kc2, vc2)
            qc = ops.prefill_qkv_prep(qkv, cos, sin, pos0, H, Hkv, kc, vc)
            assert torch.equal(qc, wq)
            assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
            # every element outside rows [pos0, pos0+S) of batch rows < B,
            # the third batch row included, still holds the sentinel
            keep = torch.ones(Bc, Smax, dtype=torch.bool, device=dev)
            keep[:B, pos0:pos0 + S] = False
            assert (kc.permute(0, 2, 1, 3)[keep] == K_FILL).all()
            assert (vc.permute(0, 2, 1, 3)[keep] == V_FILL).all()
            # and the written rows are the rotated k / the copied v
            assert torch.equal(kc[:B, :, pos0:pos0 + S],
                               wk.permute(0, 2, 1, 3))
            assert torch.equal(vc[:B, :, pos0:pos0 + S],
                               wv.permute(0, 2, 1, 3))


def test_more_than_one_block_and_a_partial_last_block(dev):
    """Row widths whose tokens-per-block differ (768, 288 and 72 pieces),
    with S no multiple of any of them."""
    from sentio_amd import ops

    for D, H, Hkv, S in ((128, 32, 8, 19), (64, 12, 12, 43), (64, 7, 1, 83)):
        qkv, cos, sin = _inputs(D, H, Hkv, 3, S, 5 + S, dev, seed=S)
        want = _legacy_ops(qkv, cos, sin, 5, H, Hkv)
        got = ops.prefill_qkv_prep(qkv, cos, sin, 5, H, Hkv)
        for g, w in zip(got, want):
            assert torch.equal(g, w)


def test_rejections_raise_before_any_launch(dev):
    from sentio_amd import ops
    from sentio_amd.ops import _sentio_hip

    D, H, Hkv, B, S = 64, 4, 2, 2, 5
    qkv, cos, sin = _inputs(D, H, Hkv, B, S, 16, dev, seed=1)
    kc = torch.full((3, Hkv, 8, D), K_FILL, device=dev, dtype=torch.bfloat16)
    vc = torch.full((3, Hkv, 8, D), V_FILL, device=dev, dtype=torch.bfloat16)
    bad = [
        dict(pos0=4),                                   # pos0 + S > Smax
        dict(pos0=3, cos=cos[:7], sin=sin[:7]),         # > table rows
        dict(pos0=0, kc=kc[:1], vc=vc[:1]),             # Bc < B
        dict(pos0=0, qkv=qkv[..., :-4].contiguous()),   # wrong width
        dict(pos0=0, qkv=qkv[:, ::2]),                  # not contiguous
        dict(pos0=-1),
        dict(pos0=0, cos=cos.cpu()),                    # another device
    ]
    for kw in bad:
        a = dict(qkv=qkv, cos=cos, sin=sin, pos0=0, kc=kc, vc=vc)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.prefill_qkv_prep(a["qkv"], a["cos"], a["sin"], a["pos0"], H,
                                 Hkv, a["kc"], a["vc"])
        # the binding checks for itself, whatever the wrapper did
        with pytest.raises(RuntimeError):
            _sentio_hip.prefill_qkv_prep(a["qkv"], a["cos"], a["sin"],
                                         a["pos0"], H, Hkv, a["kc"], a["vc"])
    torch.cuda.synchronize()
    assert (kc == K_FILL).all() and (vc == V_FILL).all()


def _model(cfg, dev, monkeypatch, mode):
    from sentio_amd.engines.transformer import Transformer

    if mode is None:
        monkeypatch.delenv("SENTIO_PREFILL_PREP", raising=False)
    else:
        monkeypatch.setenv("SENTIO_PREFILL_PREP", mode)
    m = Transformer(cfg, device=dev, dtype="bf16", seed=21)
    assert m.prefill_fused == (mode is None)
    return m


def _count_prep_calls(monkeypatch):
    from sentio_amd import ops

    calls = []
    real = ops.prefill_qkv_prep

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "prefill_qkv_prep", counted)
    return calls


def _cfg(name):
    from sentio_amd.engines.configs import MODEL_CONFIGS

    cfg = MODEL_CONFIGS[name]
    # two layers exercise everything the route changes
    return dataclasses.replace(cfg, n_layers=min(cfg.n_layers, 2))


@pytest.mark.parametrize("name", ["tiny-decoder64", "llama3-1b"])
def test_prefill_and_suffix_equal_the_legacy_route(dev, monkeypatch, name):
    from sentio_amd.engines.transformer import KVCache

    cfg = _cfg(name)
    B, P, S, Smax = 2, 8, 24, 40
    g = torch.Generator(device="cpu").manual_seed(9)
    toks = torch.randint(0, cfg.vocab_size, (B, P + S), generator=g).to(dev)
    lens = torch.tensor([S, 17], device=dev)
    outs = {}
    for mode in (None, "legacy"):
        m = _model(cfg, dev, monkeypatch, mode)
        calls = _count_prep_calls(monkeypatch)
        c1 = KVCache(cfg, B, Smax, dev, m.dtype)
        full = m.prefill(toks[:, :S], c1, lens=lens)
        c2 = KVCache(cfg, B, Smax, dev, m.dtype)
        m.prefill(toks[:, :P], c2)
        suf = m.prefill_suffix(toks[:, P:], c2, P, suffix_lens=lens)
        torch.cuda.synchronize()
        assert len(calls) == (3 * cfg.n_layers if mode is None else 0)
        outs[mode] = (full, suf, c1, c2)
        monkeypatch.undo()
    (f_new, s_new, a1, a2), (f_old, s_old, b1, b2) = outs[None], outs["legacy"]
    assert torch.isfinite(f_new).all() and torch.isfinite(s_new).all()
    assert torch.equal(f_new, f_old)
    assert torch.equal(s_new, s_old)
    for ca, cb in ((a1, b1), (a2, b2)):
        assert torch.equal(ca.seq_lens, cb.seq_lens)
        for i in range(cfg.n_layers):
            assert torch.equal(ca.k[i], cb.k[i])
            assert torch.equal(ca.v[i], cb.v[i])


def test_encoder_forward_equals_the_legacy_route(dev, monkeypatch):
    """Plain mode under a non-causal model with kv_lens.  tiny-encoder has
    head dim 16, which the prefill attention kernel does not serve on the
    GPU on either route, so this takes two layers of the small encoder."""
    cfg = _cfg("sentio-encoder-small")
    g = torch.Generator(device="cpu").manual_seed(4)
    toks = torch.randint(0, cfg.vocab_size, (3, 21), generator=g).to(dev)
    kv_lens = torch.tensor([21, 9, 1], dtype=torch.int32, device=dev)
    hs = []
    for mode in (None, "legacy"):
        m = _model(cfg, dev, monkeypatch, mode)
        calls = _count_prep_calls(monkeypatch)
        hs.append(m.forward_hidden(toks, kv_lens=kv_lens))
        torch.cuda.synchronize()
        assert len(calls) == (cfg.n_layers if mode is None else 0)
        monkeypatch.undo()
    assert torch.isfinite(hs[0]).all()
    assert torch.equal(hs[0], hs[1])


def test_explicit_pos_and_single_token_keep_the_legacy_sequence(
        dev, monkeypatch):
    """An explicit position tensor, and S == 1 into a cache (the
    decode-attention branch), do not take the fused op."""
    from sentio_amd.engines.transformer import KVCache

    cfg = _cfg("tiny-decoder64")
    m = _model(cfg, dev, monkeypatch, None)
    calls = _count_prep_calls(monkeypatch)
    g = torch.Generator(device="cpu").manual_seed(6)
    toks = torch.randint(0, cfg.vocab_size, (2, 6), generator=g).to(dev)
    pos = torch.arange(6, device=dev).unsqueeze(0).expand(2, 6)
    c1 = KVCache(cfg, 2, 16, dev, m.dtype)
    h1 = m.forward_hidden(toks, pos=pos, cache=c1)
    assert len(calls) == 0
    c2 = KVCache(cfg, 2, 16, dev, m.dtype)
    h2 = m.forward_hidden(toks, cache=c2)
    assert len(calls) == cfg.n_layers
    assert torch.equal(h1, h2)
    m.prefill_suffix(toks[:, :1], c2, 6)
    assert len(calls) == cfg.n_layers
