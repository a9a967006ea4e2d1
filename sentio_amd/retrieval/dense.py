"""Dense retriever over the in-HBM index
(reference src/core/retrievers/dense.py:21-119 semantics: embed the query,
cosine top-k, text-key fallbacks, score into metadata)."""

from __future__ import annotations

from sentio_amd.index.dense import DenseIndex
from sentio_amd.models.document import Document
from sentio_amd.retrieval.base import BaseRetriever


def _doc_text(doc: Document) -> str:
    """Text-key fallback chain text → metadata.content
    (reference dense.py:80-86)."""
    if doc.text:
        return doc.text
    return str(doc.metadata.get("content", ""))


class DenseRetriever(BaseRetriever):
    def __init__(self, embedder, index: DenseIndex,
                 mmr_lambda: float | None = None,
                 mmr_fetch_k: int | None = None):
        self.embedder = embedder
        self.index = index
        self.mmr_lambda = mmr_lambda
        self.mmr_fetch_k = mmr_fetch_k

    def retrieve(self, query: str, top_k: int = 10,
                 metadata_filter: dict | None = None,
                 *, mmr_lambda: float | None = None) -> list[Document]:
        """metadata_filter: equality conditions on document metadata; exact
        with a DENSE_FILTER=exact index, a post-filter otherwise.
        mmr_lambda: overrides the retriever's default (DENSE_MMR_LAMBDA) for
        this call; when either is set the hits are diversified by maximal
        marginal relevance (DenseIndex.search) and carry metadata["mmr_rank"],
        their place in pick order; "score" stays the cosine."""
        qv = self.embedder.embed([query])
        lam = self.mmr_lambda if mmr_lambda is None else mmr_lambda
        if lam is None:
            hits = self.index.search(qv, top_k, metadata_filter)[0]
        else:
            hits = self.index.search(qv, top_k, metadata_filter,
                                     mmr_lambda=lam,
                                     fetch_k=self.mmr_fetch_k)[0]
        out: list[Document] = []
        for rank, (doc_id, score) in enumerate(hits):
            src = self.index.get_document(doc_id)
            if src is None:
                continue
            doc = Document(text=_doc_text(src), metadata=dict(src.metadata), id=src.id)
            doc.metadata["score"] = float(score)
            doc.metadata["dense_score"] = float(score)
            doc.metadata["retrieval_method"] = "dense"
            if lam is not None:
                doc.metadata["mmr_rank"] = rank
            out.append(doc)
        return out
