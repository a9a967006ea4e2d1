"""torch_ref.bm25_topk, BM25Index.search_batch / search_mode and metadata
filters through BM25Retriever and HybridRetriever, on the CPU."""
import numpy as np
import pytest
import torch

from sentio_amd import ops
from sentio_amd.config import Settings
from sentio_amd.engines.mock import MockEncoderEngine
from sentio_amd.index.bm25 import BM25Index
from sentio_amd.index.dense import DenseIndex
from sentio_amd.models.document import Document
from sentio_amd.retrieval.dense import DenseRetriever
from sentio_amd.retrieval.hybrid import HybridRetriever
from sentio_amd.retrieval.sparse import BM25Retriever

QUERIES = ["common", "common topic 3", "number 13 number", "absent", "word 7"]


def _docs(n=60, first=0):
    return [Document(text=f"common topic {i % 5} number {i} " + "word " * (i % 7),
                     id=f"d{i}", metadata={"tenant": "a" if i % 6 == 0 else "b"})
            for i in range(first, first + n)]


def _index(variant, mode="scores"):
    docs = _docs()
    idx = BM25Index(variant=variant, search_mode=mode)
    idx.build([d.id for d in docs], [d.text for d in docs])
    return idx, docs


@pytest.mark.parametrize("variant", ["okapi", "plus"])
def test_reference_order_is_get_scores_by_score_then_row(variant):
    idx, _ = _index(variant)
    allow = ops.pack_row_mask(torch.arange(idx.n_docs)[None] % 3 != 0)
    for al, ok in ((None, np.ones(idx.n_docs, bool)),
                   (allow, np.arange(idx.n_docs) % 3 != 0)):
        vals, rows = idx.search_batch(QUERIES, 8, allow=al)
        assert vals.shape == (len(QUERIES), 8) and rows.dtype == torch.int64
        for q, v, r in zip(QUERIES, vals, rows.tolist()):
            s = idx.get_scores(q)
            want = [i for i in np.lexsort((np.arange(len(s)), -s))
                    if s[i] > 0 and ok[i]][:8]
            assert r == want + [-1] * (8 - len(want))
            assert torch.all(v[len(want):] == float("-inf"))
            np.testing.assert_allclose(v[:len(want)].numpy(), s[want], rtol=1e-6)


def test_fused_mode_on_cpu_falls_back_and_agrees_with_search():
    fused, _ = _index("okapi", "fused")
    plain, _ = _index("okapi")
    for q in QUERIES:
        assert fused.search(q, 5) == plain.search(q, 5)
        assert torch.equal(fused.search_rows(q, 5)[1], plain.search_rows(q, 5)[1])
    s = Settings()
    assert s.bm25_search == "scores"


def test_metadata_filter_reaches_both_sides_of_hybrid_retrieval():
    idx, docs = _index("okapi")
    enc = MockEncoderEngine(dim=64)
    dense = DenseIndex(dim=64, device="cpu", filter_mode="exact")
    dense.add(docs, enc.embed([d.text for d in docs]))
    sparse = BM25Retriever(idx, doc_lookup=dense.get_document)
    hits = sparse.retrieve("common topic 3", 5, metadata_filter={"tenant": "a"})
    assert len(hits) == 5, "ten documents match: top_k of them come back"
    assert all(h.metadata["tenant"] == "a" for h in hits)
    assert sparse.retrieve("common", 5, metadata_filter={"tenant": "c"}) == []
    hyb = HybridRetriever(dense=DenseRetriever(enc, dense), sparse=sparse)
    hits = hyb.retrieve("common topic 3", 5, metadata_filter={"tenant": "a"})
    assert len(hits) == 5 and all(h.metadata["tenant"] == "a" for h in hits)
    assert len(hyb.retrieve("common", 5)) == 5        # no filter: as before


def test_mask_cache_is_extended_after_add():
    idx, docs = _index("okapi")
    more = _docs(12, first=60)
    lookup = {d.id: d for d in docs + more}
    sparse = BM25Retriever(idx, doc_lookup=lookup.get)
    flt = {"tenant": "a"}
    first = sparse._filter_mask(flt)
    assert sparse._filter_mask(flt) is first          # cached
    idx.add([d.id for d in more], [d.text for d in more])
    ent = sparse._masks[repr(sorted(flt.items()))]
    old = ent[0]
    hits = sparse.retrieve("common", 72, metadata_filter=flt)
    assert {h.id for h in hits} == {f"d{i}" for i in range(0, 72, 6)}
    assert ent[1] == 72 and torch.equal(ent[0][:60], old)
