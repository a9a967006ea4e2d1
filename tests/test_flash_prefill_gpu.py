"""Tile edges of the prefill attention kernel (flash_prefill_kernel).

The kernel gives a wave R = 32 query rows (two 16-row MFMA tiles) and a
block Rb = 128, stages 64-key tiles, and takes an unmasked path on tiles
that lie wholly inside every row's causal horizon and the length.  The
shapes of test_attn_key_accounting.py were chosen for 16-row waves; these
sit on the new edges.  Inputs, reference and bound are that module's: an
fp64 softmax over an explicit allowed-key mask, poison in every K / V row
no query may attend, |got - want| <= 2^-7 |want| on the counting families
and 2^-8 (sum p|v| + |want|) on the staircase and random ones.
"""

import pytest
import torch

from test_attn_key_accounting import (BF16, F64, KINDS, POISON_K, POISON_V,
                                      attn_case, check, key_mask, make_case)

gpu = pytest.mark.gpu

R, RB = 32, 128                  # query rows per wave / per block
ROW_EDGES = (1, R - 1, R, R + 1, RB - 1, RB, RB + 1)
HEAD_DIMS = (32, 64, 96, 128)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sentio_amd import ops

    assert ops.hip_available(), (
        "HIP extension must be built/loaded on a GPU box — no eager fallback")
    return "cuda:0"


def _bf(t, dev):
    return t.to(BF16).contiguous().to(dev)


def _attention(case, lens, causal, dev):
    from sentio_amd import ops

    return ops.attention(
        _bf(case.q, dev), _bf(case.k.permute(0, 2, 1, 3), dev),
        _bf(case.v.permute(0, 2, 1, 3), dev), causal=causal, scale=case.scale,
        kv_lens=None if lens is None else lens.to(torch.int32).to(dev)).cpu()


def _attention_cache(case, lens, q_off, dev, extra_row=True):
    """One poisoned cache batch row more than q has."""
    from sentio_amd import ops

    k, v = case.k, case.v
    if extra_row:
        ek = torch.zeros_like(k[:1])
        ek[..., 0] = POISON_K
        k = torch.cat([k, ek])
        v = torch.cat([v, torch.full_like(v[:1], POISON_V)])
    return ops.attention_cache(_bf(case.q, dev), _bf(k, dev), _bf(v, dev),
                               lens.to(torch.int32).to(dev), q_off,
                               scale=case.scale).cpu()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("S", ROW_EDGES)
def test_row_edges(dev, S, D, causal, kind):
    """S on either side of a wave's and a block's rows, ragged lengths."""
    case, lens = attn_case(kind, D, S, 4, 2, causal, True)
    check(case, _attention(case, lens, causal, dev),
          f"attention {kind} S={S} D={D} causal={causal}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("n", [63, 64, 65, 127, 129])
def test_key_counts(dev, n, D, kind):
    """A five-row suffix whose last row counts n keys: the last tile holds
    63, 64 (full), 1, 63 and 1 keys.  Row 1 is shorter than q_off + S, row
    2 has kv_len = q_off + 1."""
    S, q_off = 5, n - 5
    lens = torch.tensor([n, n - 2, q_off + 1])
    allowed = key_mask(3, S, 136, lens, True, q_off)
    case = make_case(kind, 8, 2, D, allowed, seed=n + D)
    check(case, _attention_cache(case, lens, q_off, dev),
          f"attention_cache {kind} n={n} D={D}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (6, 2), (8, 2), (28, 4)])
@pytest.mark.parametrize("causal", [False, True])
def test_group_sizes(dev, H, Hkv, causal, kind):
    """G = 1, 2, 3, 4, 7 query heads per kv head."""
    S, D = R + 1, 64
    lens = torch.tensor([S, 17])
    case = make_case(kind, H, Hkv, D, key_mask(2, S, S, lens, causal),
                     seed=H)
    check(case, _attention(case, lens, causal, dev),
          f"attention {kind} H={H} Hkv={Hkv}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [32, 96, 128])
@pytest.mark.parametrize("q_off", [0, 1, 63, 64, 70])
def test_cache_offsets(dev, q_off, D, kind):
    """A suffix of R + 8 rows (two waves) at offsets around the 64-key
    tile: the interior / diagonal split moves with q_off.  kv_lens: the
    whole suffix, a row shorter than q_off + S, and q_off + 1."""
    S, smax = R + 8, 120
    lens = torch.tensor([q_off + S, q_off + S - 9, q_off + 1])
    allowed = key_mask(3, S, smax, lens, True, q_off)
    case = make_case(kind, 8, 2, D, allowed, seed=q_off + D)
    check(case, _attention_cache(case, lens, q_off, dev),
          f"attention_cache {kind} q_off={q_off} D={D}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [64, 128])
def test_noncausal_lens(dev, D, kind):
    """Non-causal with lengths full, 17 and 1 at S = Rb + 1."""
    S = RB + 1
    lens = torch.tensor([S, 17, 1])
    case = make_case(kind, 4, 2, D, key_mask(3, S, S, lens, False), seed=D)
    check(case, _attention(case, lens, False, dev),
          f"attention {kind} D={D} lens {lens.tolist()}")


@gpu
def test_deterministic(dev):
    from sentio_amd import ops

    g = torch.Generator().manual_seed(3)
    B, S, H, Hkv, D = 2, RB + 1, 8, 2, 128
    q = torch.randn(B, S, H, D, generator=g).to(BF16).to(dev)
    k = torch.randn(B, S, Hkv, D, generator=g).to(BF16).to(dev)
    v = torch.randn(B, S, Hkv, D, generator=g).to(BF16).to(dev)
    lens = torch.tensor([S, 70], dtype=torch.int32, device=dev)
    a = ops.attention(q, k, v, causal=True, kv_lens=lens)
    b = ops.attention(q, k, v, causal=True, kv_lens=lens)
    assert torch.equal(a, b)
    kc = k.permute(0, 2, 1, 3).contiguous()
    vc = v.permute(0, 2, 1, 3).contiguous()
    a = ops.attention_cache(q[:, 40:], kc, vc, lens, 40)
    b = ops.attention_cache(q[:, 40:], kc, vc, lens, 40)
    assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("D", [64, 128])
def test_rows_past_the_length_stay_out(dev, D):
    """NaN and Inf in K / V rows at or past kv_lens[b] reach no query row:
    the output is finite and bit-equal to the one with zeros there."""
    from sentio_amd import ops

    g = torch.Generator().manual_seed(D)
    B, S, H, Hkv = 3, 70, 4, 2
    lens = torch.tensor([S, 37, 1])
    q = torch.randn(B, S, H, D, generator=g).to(BF16)
    k = torch.randn(B, S, Hkv, D, generator=g).to(BF16)
    v = torch.randn(B, S, Hkv, D, generator=g).to(BF16)
    past = torch.arange(S).view(1, S, 1, 1) >= lens.view(B, 1, 1, 1)
    bad = torch.where(torch.arange(S).view(1, S, 1, 1) % 2 == 0,
                      float("nan"), float("inf")).to(BF16)
    lens_d = lens.to(torch.int32).to(dev)
    for causal in (False, True):
        clean = ops.attention(q.to(dev), torch.where(past, 0, k).to(dev),
                              torch.where(past, 0, v).to(dev), causal=causal,
                              kv_lens=lens_d)
        dirty = ops.attention(q.to(dev), torch.where(past, bad, k).to(dev),
                              torch.where(past, bad, v).to(dev),
                              causal=causal, kv_lens=lens_d)
        assert torch.isfinite(dirty).all()
        assert torch.equal(clean, dirty)
    pc = past.permute(0, 2, 1, 3)
    kc, vc = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    args = (lens_d, 0)
    clean = ops.attention_cache(
        q.to(dev), torch.where(pc, 0, kc).contiguous().to(dev),
        torch.where(pc, 0, vc).contiguous().to(dev), *args)
    dirty = ops.attention_cache(
        q.to(dev), torch.where(pc, bad.permute(0, 2, 1, 3), kc)
        .contiguous().to(dev),
        torch.where(pc, bad.permute(0, 2, 1, 3), vc).contiguous().to(dev),
        *args)
    assert torch.isfinite(dirty).all()
    assert torch.equal(clean, dirty)
