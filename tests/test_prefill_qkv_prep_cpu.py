"""ops.prefill_qkv_prep on the CPU: the reference against the sequence it
replaces (slice, rope_apply, indexed cache write), the wrapper's
rejections, and the SENTIO_PREFILL_PREP switch being a no-op without a GPU.
"""

from __future__ import annotations

import pytest
import torch

from sentio_amd import ops
from sentio_amd.ops import torch_ref

SHAPES = [(128, 4, 2), (64, 4, 4), (64, 7, 1), (16, 4, 2)]   # D, H, Hkv


def _inputs(D, H, Hkv, B, S, rows, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g)
    cos, sin = torch_ref.rope_tables(rows, D, 10000.0)
    return qkv, cos, sin


def _legacy(qkv, cos, sin, pos0, H, Hkv, kc=None, vc=None):
    """Transformer._attn's sequence, written out."""
    B, S, W = qkv.shape
    D = W // (H + 2 * Hkv)
    pos = (pos0 + torch.arange(S)).unsqueeze(0).expand(B, S)
    q_end, k_end = H * D, (H + Hkv) * D
    q = qkv[..., :q_end].reshape(B, S, H, D)
    k = qkv[..., q_end:k_end].reshape(B, S, Hkv, D)
    v = qkv[..., k_end:].reshape(B, S, Hkv, D)
    q = torch_ref.rope_apply(q, cos, sin, pos)
    k = torch_ref.rope_apply(k, cos, sin, pos)
    if kc is not None:
        idx = pos.long()
        bidx = torch.arange(B).unsqueeze(1).expand(B, S)
        kc[bidx.reshape(-1), :, idx.reshape(-1)] = k.reshape(B * S, Hkv, D)
        vc[bidx.reshape(-1), :, idx.reshape(-1)] = v.reshape(B * S, Hkv, D)
    return q, k, v


@pytest.mark.parametrize("D,H,Hkv", SHAPES)
@pytest.mark.parametrize("S,pos0", [(1, 0), (5, 3), (37, 0)])
def test_reference_plain_mode_equals_legacy_sequence(D, H, Hkv, S, pos0):
    qkv, cos, sin = _inputs(D, H, Hkv, 2, S, pos0 + S)
    got = ops.prefill_qkv_prep(qkv, cos, sin, pos0, H, Hkv)
    want = _legacy(qkv, cos, sin, pos0, H, Hkv)
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g, w)
        assert g.is_contiguous()


@pytest.mark.parametrize("D,H,Hkv", SHAPES)
@pytest.mark.parametrize("S,pos0,slack", [(1, 0, 0), (5, 3, 9), (37, 3, 0)])
def test_reference_cache_mode_equals_legacy_sequence(D, H, Hkv, S, pos0,
                                                     slack):
    B, Bc, Smax = 2, 3, pos0 + S + slack
    qkv, cos, sin = _inputs(D, H, Hkv, B, S, Smax)
    kc = torch.full((Bc, Hkv, Smax, D), -7.0)
    vc = torch.full((Bc, Hkv, Smax, D), -9.0)
    kc2, vc2 = kc.clone(), vc.clone()
    q = ops.prefill_qkv_prep(qkv, cos, sin, pos0, H, Hkv, kc, vc)
    q2, _, _ = _legacy(qkv, cos, sin, pos0, H, Hkv, kc2, vc2)
    assert torch.equal(q, q2)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    # nothing outside rows [pos0, pos0+S) of batch rows < B was touched
    keep = torch.ones(Bc, Smax, dtype=torch.bool)
    keep[:B, pos0:pos0 + S] = False
    assert (kc.permute(0, 2, 1, 3)[keep] == -7.0).all()
    assert (vc.permute(0, 2, 1, 3)[keep] == -9.0).all()


def test_wrapper_rejections():
    D, H, Hkv, B, S = 16, 4, 2, 2, 5
    qkv, cos, sin = _inputs(D, H, Hkv, B, S, 16)
    kc = torch.zeros(3, Hkv, 8, D)
    vc = torch.zeros(3, Hkv, 8, D)
    ok = ops.prefill_qkv_prep(qkv, cos, sin, 3, H, Hkv, kc, vc)
    assert ok.shape == (B, S, H, D)
    with pytest.raises(ValueError, match="exceed the cache"):
        ops.prefill_qkv_prep(qkv, cos, sin, 4, H, Hkv, kc, vc)
    with pytest.raises(ValueError, match="rope table rows"):
        ops.prefill_qkv_prep(qkv, cos[:7], sin[:7], 3, H, Hkv, kc, vc)
    with pytest.raises(ValueError, match="batch rows"):
        ops.prefill_qkv_prep(qkv, cos, sin, 0, H, Hkv, kc[:1], vc[:1])
    with pytest.raises(ValueError, match="pos0"):
        ops.prefill_qkv_prep(qkv, cos, sin, -1, H, Hkv, kc, vc)
    with pytest.raises(ValueError, match="width"):
        ops.prefill_qkv_prep(qkv[..., :-4].contiguous(), cos, sin, 0, H, Hkv)
    with pytest.raises(ValueError, match="contiguous"):
        ops.prefill_qkv_prep(qkv[:, ::2], cos, sin, 0, H, Hkv)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.prefill_qkv_prep(torch.zeros(1, 2, 8 * 12), cos, sin, 0, H, Hkv)
    with pytest.raises(ValueError, match="cos must be"):
        ops.prefill_qkv_prep(qkv, cos.double(), sin, 0, H, Hkv)
    with pytest.raises(ValueError, match="sin must be"):
        ops.prefill_qkv_prep(qkv, cos, sin[:, :4], 0, H, Hkv)
    with pytest.raises(ValueError, match="both caches"):
        ops.prefill_qkv_prep(qkv, cos, sin, 0, H, Hkv, kc, None)
    with pytest.raises(ValueError, match="caches must both be"):
        ops.prefill_qkv_prep(qkv, cos, sin, 0, H, Hkv, kc,
                             torch.zeros(3, Hkv, 9, D))
    with pytest.raises(ValueError, match="k_cache must be"):
        ops.prefill_qkv_prep(qkv, cos, sin, 0, H, Hkv, kc.double(), vc)


def _build(name, monkeypatch, mode):
    from sentio_amd.engines.configs import MODEL_CONFIGS
    from sentio_amd.engines.transformer import Transformer

    if mode is None:
        monkeypatch.delenv("SENTIO_PREFILL_PREP", raising=False)
    else:
        monkeypatch.setenv("SENTIO_PREFILL_PREP", mode)
    m = Transformer(MODEL_CONFIGS[name], device="cpu", seed=5)
    assert not m.prefill_fused          # the CPU keeps the rope sequence
    return m


def test_switch_is_a_noop_on_the_cpu_decoder(monkeypatch):
    from sentio_amd.engines.transformer import KVCache

    B, P, S = 2, 8, 11
    g = torch.Generator().manual_seed(3)
    toks = torch.randint(0, 4608, (B, P + S), generator=g)
    lens = torch.tensor([P + S, P + 4])
    outs = []
    for mode in (None, "legacy"):
        m = _build("tiny-decoder", monkeypatch, mode)
        c1 = KVCache(m.cfg, B, 32, "cpu", m.dtype)
        full = m.prefill(toks, c1, lens=lens)
        c2 = KVCache(m.cfg, B, 32, "cpu", m.dtype)
        m.prefill(toks[:, :P], c2)
        suf = m.prefill_suffix(toks[:, P:], c2, P, suffix_lens=lens - P)
        outs.append((full, suf, c1.k, c1.v, c2.k, c2.v, c2.seq_lens))
    a, b = outs
    for x, y in zip(a[:2], b[:2]):
        assert torch.equal(x, y)
    for xs, ys in zip(a[2:6], b[2:6]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    assert torch.equal(a[6], b[6])
    # the suffix forward continues the prefix: same logits as one prefill
    torch.testing.assert_close(a[1], a[0], rtol=1e-4, atol=1e-4)


def test_switch_is_a_noop_on_the_cpu_encoder(monkeypatch):
    g = torch.Generator().manual_seed(4)
    toks = torch.randint(0, 4608, (3, 9), generator=g)
    kv_lens = torch.tensor([9, 4, 1], dtype=torch.int32)
    hs = [_build("tiny-encoder", monkeypatch, mode).forward_hidden(
        toks, kv_lens=kv_lens) for mode in (None, "legacy")]
    assert torch.equal(hs[0], hs[1])
