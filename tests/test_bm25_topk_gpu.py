"""ops.bm25_topk (tiled BM25 scoring with the top-k and the row mask inside
the kernel) against an fp64 reference over the same fp32 CSR arrays."""
import functools

import pytest
import torch

from sentio_amd import ops
from sentio_amd.ops import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# contributions are >= 0 (no cancellation); <= 16 terms of about 6 roundings
# each: relative error below (16 + 6) * 2^-24 = 1.3e-6
RTOL = 1e-5
K1, B_, DELTA = 1.5, 0.75, 1.0
EVERY, RARE, LAST, EMPTY, EDGE = 0, 1, 2, 3, 4    # terms 5..20 are random

# N (in tiles: offset, or (tiles per block, extra docs)), B, k, variant
SHAPES = [((1, -1), 1, 5, "okapi"), ((1, 1), 17, 128, "plus"),
          ((2, 0), 32, 128, "okapi"), ((2, 0), 33, 5, "plus"),
          ("big", 3, 5, "okapi"), ("big", 3, 128, "okapi")]


@functools.lru_cache(maxsize=None)
def _index(nspec):
    """Seeded CSR arrays: per term a sorted random subset of the documents."""
    blocks, tile, _ = ops.bm25_topk_plan(1 << 30)
    N = 2 * blocks * tile + 37 if nspec == "big" else nspec[0] * tile + nspec[1]
    g = torch.Generator(device=DEV).manual_seed(N)
    r = torch.arange(N, device=DEV)
    some = lambda p: r[torch.rand(N, generator=g, device=DEV) < p]  # noqa: E731
    docs = [r, some(0.01), r[-1:], r[:0], r[(r == tile - 1) | (r == tile)]] \
        + [some(0.02 + 0.02 * i) for i in range(16)]
    lens = torch.tensor([len(d) for d in docs])
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    nnz = int(indptr[-1])
    a = {"indptr": indptr.to(DEV), "post_doc": torch.cat(docs).int(),
         "post_tf": torch.randint(1, 6, (nnz,), generator=g,
                                  device=DEV).float(),
         "doc_len": torch.randint(5, 201, (N,), generator=g,
                                  device=DEV).float()}
    df = lens.double()
    a["okapi"] = torch.log((N - df + 0.5) / (df + 0.5) + 1.0).float().to(DEV)
    a["plus"] = torch.log((N + 1.0) / df.clamp(min=1.0)).float().to(DEV)
    a["avgdl"] = float(a["doc_len"].mean())      # an fp32 value
    return a, N, tile


QUERIES = [[EVERY, RARE], list(range(5, 21)), [RARE, RARE], [EMPTY], [LAST],
           [RARE], [EVERY, 7, EDGE], [LAST, EMPTY, EDGE]]


@functools.lru_cache(maxsize=None)
def _data(shape):
    nspec, B, k, variant = shape
    a, N, tile = _index(nspec)
    delta = DELTA if variant == "plus" else 0.0
    qs = [QUERIES[i % len(QUERIES)] for i in range(B)]
    tids = torch.tensor([t for q in qs for t in q], device=DEV)
    qoff = torch.tensor([0] + [len(q) for q in qs]).cumsum(0).int()
    nd = K1 * (1 - B_ + B_ * a["doc_len"].double() / a["avgdl"])
    ref = torch.zeros(B, N, dtype=torch.float64, device=DEV)
    for i, q in enumerate(qs):
        for t in q:
            lo, hi = a["indptr"][t], a["indptr"][t + 1]
            d, tf = a["post_doc"][lo:hi].long(), a["post_tf"][lo:hi].double()
            ref[i, d] += a[variant][t].double() * (
                tf * (K1 + 1) / (tf + nd[d]) + delta)
    kw = dict(n_docs=N, k=k, k1=K1, b=B_, avgdl=a["avgdl"], plus_delta=delta)
    args = (tids, qoff, a["indptr"], a["post_doc"], a["post_tf"], a[variant],
            a["doc_len"])
    return args, kw, ref, N, tile


def _mask(pattern, N, B, tile):
    g = torch.Generator().manual_seed(N + B)
    r = torch.arange(N)
    if pattern == "per_query":
        m = torch.rand(B, N, generator=g) < 0.3
        m[0], m[B - 1] = False, True
        return m
    return {
        "ones": r >= 0, "zeros": r < 0, "last_row": r == N - 1,
        "alt_tiles": (r // tile) % 2 == 1,
        "stray": torch.rand((N + 127) // 128 * 128, generator=g) < 0.5,  # >= N
    }[pattern][None]


PATTERNS = [None, "ones", "zeros", "last_row", "alt_tiles", "per_query",
            "stray"]


def _check(vals, rows, ref, ok, k):
    """The criteria of test_dense_filter_gpu._check over the allowed
    documents with a positive score; every returned score is > 0."""
    B, N = ref.shape
    ok = ok.expand(B, N) & (ref > 0)
    assert vals.shape == (B, k) and rows.shape == (B, k)
    assert vals.dtype == torch.float32 and rows.dtype == torch.int64
    cnt = ok.sum(1, keepdim=True).clamp(max=k)
    valid = torch.arange(k, device=DEV)[None] < cnt
    assert torch.all(rows[~valid] == -1)
    assert torch.all(vals[~valid] == float("-inf"))
    assert torch.all(vals[:, :-1] >= vals[:, 1:]), "not sorted"
    assert torch.all((rows[valid] >= 0) & (rows[valid] < N))
    assert torch.all(vals[valid] > 0)
    safe = rows.clamp(min=0)
    assert torch.all(torch.gather(ok, 1, safe)[valid]), "a masked row"
    for r in rows.tolist():
        r = [x for x in r if x >= 0]
        assert len(set(r)) == len(r), "row twice"
    got = torch.gather(ref, 1, safe)
    err = ((vals.double() - got).abs() / got)[valid]
    print(f"max rel err = {err.max().item() if err.numel() else 0:.3e}")
    assert torch.all(err <= RTOL)
    top = torch.topk(ref.masked_fill(~ok, float("-inf")), min(k, N), 1).values
    kth = torch.gather(top, 1, (cnt - 1).clamp(min=0))
    # both scores of a comparison carry the error
    assert torch.all((got >= kth * (1 - 2 * RTOL))[valid]), "outside the top k"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_matches_fp64_reference(shape, pattern):
    args, kw, ref, N, tile = _data(shape)
    m = torch.ones(1, N, dtype=torch.bool) if pattern is None \
        else _mask(pattern, N, shape[1], tile)
    allow = None if pattern is None else ops.pack_row_mask(m).to(DEV)
    vals, rows = ops.bm25_topk(*args, allow=allow, **kw)
    _check(vals, rows, ref, m[:, :N].to(DEV), shape[2])


def test_exact_ties_come_back_in_row_order():
    blocks, tile, _ = ops.bm25_topk_plan(1 << 30)
    N = 3 * tile + 5                          # four tiles, four blocks
    dups = [3, 20, tile + 2, 2 * tile + 7, N - 1]
    g = torch.Generator().manual_seed(7)
    other = torch.rand(N, generator=g) < 0.3
    other[dups] = True
    d1 = torch.nonzero(other)[:, 0]
    tf1 = torch.ones(len(d1))
    tf1[torch.isin(d1, torch.tensor(dups))] = 3.0
    doc_len = torch.randint(5, 201, (N,), generator=g).float()
    doc_len[dups] = 50.0
    a = [torch.tensor([0, 1]), torch.tensor([0, 2], dtype=torch.int32),
         torch.tensor([0, len(dups), len(dups) + len(d1)]),
         torch.cat([torch.tensor(dups), d1]).int(),
         torch.cat([torch.full((len(dups),), 2.0), tf1]),
         torch.tensor([1.25, 0.5]), doc_len]
    m = torch.rand(1, N, generator=g) < 0.5
    m[0, dups] = True
    m[0, 20] = False                          # a masked duplicate stays out
    allow = ops.pack_row_mask(m)
    kw = dict(n_docs=N, k=10, k1=K1, b=B_, avgdl=float(doc_len.mean()))
    rows = ops.bm25_topk(*[t.to(DEV) for t in a], allow=allow.to(DEV), **kw)[1]
    assert rows[0, :4].tolist() == [3, tile + 2, 2 * tile + 7, N - 1]
    assert torch.equal(rows.cpu(), torch_ref.bm25_topk(*a, allow=allow, **kw)[1])


def test_index_in_fused_mode_searches_through_the_kernel():
    from sentio_amd.index.bm25 import BM25Index

    # a score depends on the length alone: exact ties or clear gaps
    idx = BM25Index(search_mode="fused")
    idx.build([f"d{i}" for i in range(300)],
              ["common " + "pad " * (i % 7) + ("rare" if i % 50 == 9 else "")
               for i in range(300)])
    qs = ["common", "rare common", "absent"]
    vals, rows = idx.search_batch(qs, 8, device=DEV)
    cv, cr = idx.search_batch(qs, 8)             # the CPU reference
    assert torch.equal(rows.cpu(), cr)
    torch.testing.assert_close(vals.cpu(), cv, rtol=RTOL, atol=0)
    assert [d for d, _ in idx.search(qs[1], 8, device=DEV)] == \
        [idx.doc_ids[i] for i in cr[1].tolist()]
    assert torch.equal(idx.search_rows(qs[1], 8, device=DEV)[1].cpu(), cr[1])


def test_two_calls_give_the_same_bits():
    args, kw, _, N, _ = _data(("big", 3, 128, "okapi"))
    one, two = ops.bm25_topk(*args, **kw), ops.bm25_topk(*args, **kw)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


def test_wrapper_rejects_bad_arguments():
    args, kw, _, N, _ = _data(((1, 1), 17, 128, "plus"))
    allow = ops.pack_row_mask(torch.ones(1, N, dtype=torch.bool)).to(DEV)
    W = allow.shape[1]
    pad = torch.zeros(1, W + 1, dtype=torch.int32, device=DEV)
    bad = [dict(allow=allow[:, :4].contiguous()), dict(allow=allow.repeat(1, 2)),
           dict(allow=allow.repeat(2, 1)), dict(allow=allow.long()),
           dict(allow=allow.cpu()), dict(k=129),
           dict(allow=pad[:, 1:]),                        # misaligned
           dict(allow=allow.repeat(1, 2)[:, ::2])]        # strided
    for over in bad:
        with pytest.raises(ValueError):
            ops.bm25_topk(*args, **{**kw, **over})
    with pytest.raises(ValueError):                       # qoff != len(tids)
        ops.bm25_topk(args[0][:-1], *args[1:], **kw)
