"""ops.mmr_select (mmr_select_kernel on the GPU, torch_ref.mmr_select on the
CPU) against a plain fp64 loop over the stored values.

Shapes: the kernel walks D in 128-dim slabs (32 and 96: a partial slab, 160:
one and a quarter, 256 and 1024: whole slabs, 1024 the most), a wave owns 16
candidates (1, 15 | 16 | 17, 33 and 128 = every wave), lane l owns candidates
l and l + 64 and picks l and l + 64 (k = 128).  Rows are drawn around a few
cluster centres, so the redundancy term decides picks."""

import functools

import pytest
import torch

gpu = pytest.mark.gpu
DEVICES = ["cpu", pytest.param("cuda:0", marks=gpu)]
SHAPES = [(32, 1, 1), (32, 16, 16), (96, 17, 5), (160, 15, 15),
          (256, 128, 128), (1024, 128, 10), (1024, 33, 33)]
N, B = 300, 3
# an fp32-accumulated dot product of <= 1024 exact fp16 x fp16 products whose
# absolute values sum to about 1 is off by at most 1024 * 2^-24 = 6.1e-5; the
# objective is a convex combination of two such values, comparing two
# objectives doubles the error, and EPS is twice that doubled bound
EPS = 2.5e-4


def _stored(x, fp8):
    """(rows, scales, the stored values in fp64) of an index over x."""
    from sentio_amd.ops import torch_ref

    if not fp8:
        return x.half(), None, x.half().double()
    codes, scales = torch_ref.index_quantize(x)
    return codes, scales, \
        codes.view(torch.float8_e4m3fn).double() * scales.double()[:, None]


@functools.lru_cache(maxsize=None)
def _case(D, C, k, fp8):
    g = torch.Generator().manual_seed(1000 + D + 7 * C + k)
    centres = torch.randn(5, D, generator=g)
    x = centres[torch.randint(0, 5, (N,), generator=g)] \
        + 0.3 * torch.randn(N, D, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    q = centres[0] + 0.5 * torch.randn(B, D, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).half()
    cand = torch.stack([torch.randperm(N, generator=g)[:C] for _ in range(B)])
    cand[B - 1, min(C // 2, k - 1):] = -1       # fewer than k valid entries
    return (q, cand) + _stored(x, fp8)


def _check(q, xs, cand, k, lam, vals, idx):
    """The issue's assertions, list by list, in fp64."""
    for b in range(cand.shape[0]):
        c = cand[b].tolist()
        valid = cand[b] >= 0
        n = min(k, int(valid.sum()))
        picks = idx[b].tolist()
        assert picks[n:] == [-1] * (k - n) and -1 not in picks[:n]
        assert torch.isneginf(vals[b, n:]).all()
        pos = [c.index(p) for p in picks[:n]]           # members of the list
        assert len(set(pos)) == n
        g = xs[cand[b].clamp_min(0)]
        rel, S = g @ q[b].double(), g @ g.T
        red, open_ = torch.zeros_like(rel), valid.clone()
        for t, p in enumerate(pos):
            obj = (lam * rel - (1 - lam) * red).masked_fill(~open_, -torch.inf)
            assert abs(float(vals[b, t]) - float(rel[p])) <= 1e-4
            assert float(obj[p]) >= float(obj.max()) - EPS, (b, t)
            if lam == 0.0 and t == 0:
                assert p == 0                           # every objective is 0
            open_[p] = False
            red = torch.maximum(red, S[:, p])


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("fp8", [False, True], ids=["fp16", "fp8"])
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("D,C,k", SHAPES)
def test_mmr_select_matches_fp64(D, C, k, lam, fp8, dev):
    from sentio_amd import ops

    q, cand, rows, scales, xs = _case(D, C, k, fp8)
    vals, idx = ops.mmr_select(
        q.to(dev), rows.to(dev), None if scales is None else scales.to(dev),
        cand.to(dev), k, lam)
    assert vals.shape == idx.shape == (B, k)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64
    _check(q, xs, cand, k, lam, vals.cpu(), idx.cpu())


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("fp8", [False, True], ids=["fp16", "fp8"])
def test_mmr_select_ties(fp8, dev):
    """Positions 2 and 5 hold one vector under two row numbers, alone in
    their cluster; every cluster is equally near the query."""
    from sentio_amd import ops

    D, C = 64, 8
    g = torch.Generator().manual_seed(7)
    x = 0.05 * torch.randn(N, D, generator=g)   # near-copies: S about 0.9
    x[:, 0] = 1.0
    for pos, cl in enumerate([1, 1, 0, 2, 2, 0, 3, 3]):
        x[10 * pos + 3, 1 + cl] += 0.7
    x[53] = x[23]
    x = x / x.norm(dim=1, keepdim=True)
    q = torch.zeros(1, D, dtype=torch.float16)
    q[0, 0] = 1.0
    cand = torch.tensor([[10 * pos + 3 for pos in range(C)]])
    rows, scales, xs = _stored(x, fp8)
    args = (q.to(dev), rows.to(dev),
            None if scales is None else scales.to(dev), cand.to(dev), C, 0.5)
    vals, idx = ops.mmr_select(*args)
    again = ops.mmr_select(*args)
    assert torch.equal(vals, again[0]) and torch.equal(idx, again[1])
    _check(q, xs, cand, C, 0.5, vals.cpu(), idx.cpu())
    picks = idx[0].tolist()
    assert picks.index(23) < picks.index(53)
    assert picks.index(53) - picks.index(23) > 1


def _good():
    return dict(q=torch.zeros(2, 64, dtype=torch.float16),
                rows=torch.zeros(200, 64, dtype=torch.float16), scales=None,
                cand=torch.arange(16).view(2, 8), k=4, lam=0.5)


@pytest.mark.parametrize("bad", [
    dict(cand=torch.zeros(2, 129, dtype=torch.int64)),
    dict(k=9),
    dict(k=0),
    dict(q=torch.zeros(2, 48, dtype=torch.float16),
         rows=torch.zeros(200, 48, dtype=torch.float16)),
    dict(lam=1.5),
    dict(lam=float("nan")),
    dict(cand=torch.arange(32).view(2, 16)[:, ::2]),
    dict(cand=torch.arange(16, dtype=torch.int32).view(2, 8)),
    dict(cand=torch.arange(16).view(2, 8).to("meta")),
    dict(rows=torch.zeros(200, 64, dtype=torch.uint8)),
], ids=["C=129", "k>C", "k=0", "D=48", "lam=1.5", "lam=nan", "strided-cand",
        "int32-cand", "mixed-devices", "uint8-without-scales"])
def test_mmr_select_rejects(bad):
    from sentio_amd import ops

    ops.mmr_select(**_good())                           # the base case is fine
    with pytest.raises(ValueError):
        ops.mmr_select(**{**_good(), **bad})
