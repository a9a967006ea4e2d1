"""MMR through the search path: DenseIndex.search / search_rows with
mmr_lambda, DenseRetriever and the DENSE_MMR_* settings.

64 rows at dim 64: rows 8j .. 8j+7 are near-copies of cluster j (j < 4), the
clusters sit around the query at falling cosine (0.78 .. 0.67, about 0.55
to one another), rows 32 .. 63 point away from it.  Even rows are "en"."""

import pytest
import torch

from sentio_amd.index.bm25 import BM25Index
from sentio_amd.index.dense import DenseIndex
from sentio_amd.models.document import Document

gpu = pytest.mark.gpu
CASES = [("cpu", torch.float16), ("cpu", "fp8"),
         pytest.param("cuda:0", torch.float16, marks=gpu),
         pytest.param("cuda:0", "fp8", marks=gpu)]
DIM = 64


def _corpus():
    g = torch.Generator().manual_seed(11)
    x = 0.01 * torch.randn(64, DIM, generator=g)
    x[32:] = torch.randn(32, DIM, generator=g) / 8
    x[:32, 0] += 1.0
    x[32:, 0] = -0.5
    for j in range(4):
        x[8 * j:8 * j + 8, j + 1] += 0.8 + 0.1 * j
    q = torch.zeros(DIM)
    q[0] = 1.0
    return x, q


def _index(dev, dtype, filter_mode="exact"):
    x, q = _corpus()
    idx = DenseIndex(dim=DIM, device=dev, dtype=dtype, filter_mode=filter_mode)
    idx.add([Document(text=f"t{i}", id=f"d{i}",
                      metadata={"lang": "en" if i % 2 == 0 else "de"})
             for i in range(64)], x)
    return idx, q


def _rows(hits):
    return [int(doc_id[1:]) for doc_id, _ in hits]


@pytest.mark.parametrize("dev,dtype", CASES)
def test_search_mmr(dev, dtype):
    idx, q = _index(dev, dtype)
    plain = idx.search(q, 4)
    assert all(r < 8 for r in _rows(plain[0]))          # the nearest cluster

    hits = idx.search(q, 4, mmr_lambda=0.5)[0]
    assert sorted(r // 8 for r in _rows(hits)) == [0, 1, 2, 3]
    assert _rows(hits)[0] == _rows(plain[0])[0]
    vals, rows = idx.search_rows(q, 4, mmr_lambda=0.5)
    assert rows.dtype == torch.int64 and rows[0].tolist() == _rows(hits)
    assert vals[0].tolist() == [s for _, s in hits]

    filt = idx.search(q, 4, {"lang": "en"}, mmr_lambda=0.5)[0]
    assert all(r % 2 == 0 for r in _rows(filt))
    assert sorted(r // 8 for r in _rows(filt)) == [0, 1, 2, 3]
    # lambda = 1 is the plain order; more asked for than the index holds
    assert _rows(idx.search(q, 4, mmr_lambda=1.0, fetch_k=8)[0]) == \
        _rows(plain[0])
    assert len(idx.search(q, 100, mmr_lambda=0.5)[0]) == 64
    assert idx.search(q, 4) == plain                    # no state is shared

    for kw in (dict(mmr_lambda=1.5), dict(mmr_lambda=0.5, fetch_k=3),
               dict(mmr_lambda=0.5, fetch_k=129)):
        with pytest.raises(ValueError):
            idx.search(q, 4, **kw)


def test_mmr_with_post_filter_raises():
    idx, q = _index("cpu", torch.float16, filter_mode="post")
    with pytest.raises(ValueError, match="exact"):
        idx.search(q, 4, {"lang": "en"}, mmr_lambda=0.5)
    assert len(idx.search(q, 4, {"lang": "en"})[0]) == 4


def test_retriever_and_settings(monkeypatch):
    from sentio_amd.config import Settings
    from sentio_amd.retrieval.dense import DenseRetriever
    from sentio_amd.retrieval.factory import create_retriever

    idx, q = _index("cpu", torch.float16)

    class Embedder:
        def embed(self, texts):
            return q[None]

    docs = DenseRetriever(Embedder(), idx, mmr_lambda=0.5).retrieve("x", 4)
    assert [d.metadata["mmr_rank"] for d in docs] == [0, 1, 2, 3]
    assert sorted(int(d.id[1:]) // 8 for d in docs) == [0, 1, 2, 3]
    plain = DenseRetriever(Embedder(), idx)
    assert "mmr_rank" not in plain.retrieve("x", 4)[0].metadata
    assert [d.id for d in plain.retrieve("x", 4, mmr_lambda=0.5)] == \
        [d.id for d in docs]

    monkeypatch.delenv("DENSE_MMR_LAMBDA", raising=False)
    monkeypatch.delenv("DENSE_MMR_FETCH_K", raising=False)
    assert Settings.from_env().dense_mmr_lambda is None
    monkeypatch.setenv("DENSE_MMR_LAMBDA", "0.25")
    monkeypatch.setenv("DENSE_MMR_FETCH_K", "16")
    monkeypatch.setenv("RETRIEVAL_STRATEGY", "dense")
    s = Settings.from_env()
    assert (s.dense_mmr_lambda, s.dense_mmr_fetch_k) == (0.25, 16)
    made = create_retriever(s, Embedder(), idx, BM25Index())
    assert (made.mmr_lambda, made.mmr_fetch_k) == (0.25, 16)
    for name, bad in (("DENSE_MMR_LAMBDA", "2"), ("DENSE_MMR_FETCH_K", "129"),
                      ("DENSE_MMR_FETCH_K", "0")):
        monkeypatch.setenv(name, bad)
        with pytest.raises(ValueError, match=name):
            Settings.from_env()
        monkeypatch.setenv(name, "1")
