"""DenseIndex(filter_mode="exact"), search_rows(allow=) and DENSE_FILTER."""
import pytest
import torch

from sentio_amd import ops
from sentio_amd.config import Settings
from sentio_amd.index.dense import DenseIndex
from sentio_amd.models.document import Document
from sentio_amd.ops import torch_ref

DIM, N_DOCS, TOP_K = 64, 400, 5
DTYPES = [torch.float16, "fp8"]


def _tenant_corpus():
    """One document in 40 is tenant "a".  Along the query, tenant document j
    has 0.5 * 0.8^j (no index dtype reorders these), any other 0.7 .. 0.95."""
    g = torch.Generator().manual_seed(0)
    rest = torch.randn(N_DOCS, DIM - 1, generator=g)
    rest = rest / rest.norm(dim=1, keepdim=True)
    a = 0.7 + 0.25 * torch.rand(N_DOCS, generator=g)
    mine = torch.arange(0, N_DOCS, 40)
    a[mine] = 0.5 * 0.8 ** torch.arange(len(mine), dtype=torch.float32)
    emb = torch.cat([a[:, None], (1 - a * a).sqrt()[:, None] * rest], 1)
    docs = [Document(text=f"doc {i}", id=f"d{i}",
                     metadata={"tenant": "a" if i % 40 == 0 else "b"})
            for i in range(N_DOCS)]
    query = torch.zeros(DIM)
    query[0] = 1.0
    return docs, emb, query, [f"d{i}" for i in mine.tolist()]


def _index(mode, dtype, device="cpu"):
    docs, emb, query, best = _tenant_corpus()
    idx = DenseIndex(dim=DIM, device=device, dtype=dtype, filter_mode=mode)
    idx.add(docs, emb)
    return idx, query, best


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_filter_returns_the_best_matching_documents(dtype):
    post, query, best = _index("post", dtype)
    hits = post.search(query, TOP_K, metadata_filter={"tenant": "a"})[0]
    assert len(hits) < TOP_K, "the over-fetching post-filter's gap"
    exact, query, best = _index("exact", dtype)
    hits = exact.search(query, TOP_K, metadata_filter={"tenant": "a"})[0]
    assert [h[0] for h in hits] == best[:TOP_K]
    # more asked for than match: every matching document, no padding
    hits = exact.search(query, 40, metadata_filter={"tenant": "a"})[0]
    assert [h[0] for h in hits] == best
    assert exact.search(query, TOP_K, metadata_filter={"tenant": "c"}) == [[]]
    # 40 hits wanted: on an fp8 "post" index that over-fetch (160) raises
    hits = exact.search(query, 40, metadata_filter={"tenant": "b"})[0]
    assert len(hits) == 40
    assert all(exact.get_document(h[0]).metadata["tenant"] == "b" for h in hits)
    # unfiltered searches are those of a "post" index
    assert exact.search(query, TOP_K) == post.search(query, TOP_K)


def test_cached_filter_sees_rows_added_later():
    (exact, query, best), flt = _index("exact", torch.float16), {"tenant": "a"}
    assert [h[0] for h in exact.search(query, 2, metadata_filter=flt)[0]] \
        == best[:2]
    new = torch.zeros(3, DIM)
    new[:, 0] = 1.0
    new[:, 1] = torch.tensor([0.1, 0.2, 0.3])
    exact.add([Document(text="n0", id="n0", metadata={"tenant": "a"}),
               Document(text="n1", id="n1", metadata={"tenant": "b"}),
               Document(text="n2", id="n2", metadata={"tenant": "a"})], new)
    assert [h[0] for h in exact.search(query, 3, metadata_filter=flt)[0]] \
        == ["n0", "n2", best[0]]
    exact.clear()                             # drops the cached mask too
    exact.add([Document(text="m", id="m", metadata={"tenant": "b"})], new[:1])
    assert exact.search(query, 3, metadata_filter=flt) == [[]]


@pytest.mark.parametrize("mode", ["post", "exact"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_rows_takes_a_mask_per_query(dtype, mode):
    idx, _, _ = _index(mode, dtype)
    g = torch.Generator().manual_seed(1)
    q = torch.randn(3, DIM, generator=g)
    ok = torch.rand(3, N_DOCS, generator=g) < 0.05
    ok[1] = False
    ok[1, :3] = True                          # fewer than k allowed
    vals, rows = idx.search_rows(q, 7, allow=ops.pack_row_mask(ok))
    qn = q / q.norm(dim=1, keepdim=True)
    args = (qn.half(), idx._codes[:N_DOCS], idx._scales[:N_DOCS]) \
        if dtype == "fp8" else (qn, idx._vecs[:N_DOCS], None)
    want = torch_ref.cosine_topk_masked(*args, 7, torch_ref.pack_row_mask(ok))
    assert torch.equal(rows, want[1]) and torch.equal(vals, want[0])


def test_settings_dense_filter(monkeypatch):
    monkeypatch.delenv("DENSE_FILTER", raising=False)
    assert Settings.from_env().dense_filter == "post"
    monkeypatch.setenv("DENSE_FILTER", "exact")
    assert Settings.from_env().dense_filter == "exact"
    monkeypatch.setenv("DENSE_FILTER", "pre")
    with pytest.raises(ValueError, match="DENSE_FILTER"):
        Settings.from_env()
    with pytest.raises(ValueError):
        DenseIndex(dim=DIM, filter_mode="pre")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_index_on_the_gpu_matches_the_cpu(dtype):
    gpu, query, best = _index("exact", dtype, "cuda:0")
    cpu, _, _ = _index("exact", dtype)
    flt = {"tenant": "a"}
    got = gpu.search(query, TOP_K, metadata_filter=flt)[0]
    assert [h[0] for h in got] == best[:TOP_K]
    allow = cpu._filter_mask(flt)
    gv, gr = gpu.search_rows(query, 40, allow=allow.to("cuda:0"))
    cv, cr = cpu.search_rows(query, 40, allow=allow)
    assert gr.is_cuda and torch.equal(gr.cpu(), cr)
    assert torch.allclose(gv.cpu(), cv, atol=1e-4 if dtype == "fp8" else 1e-3,
                          rtol=0)
