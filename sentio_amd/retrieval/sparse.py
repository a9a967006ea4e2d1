"""BM25 retriever over the CSR postings index
(reference src/core/retrievers/sparse.py:33-204 semantics: score>0 filter,
bm25_score into metadata, okapi/plus variants)."""

from __future__ import annotations

from sentio_amd.index.bm25 import BM25Index
from sentio_amd.models.document import Document
from sentio_amd.retrieval.base import BaseRetriever


class BM25Retriever(BaseRetriever):
    MASK_CACHE = 16

    def __init__(self, index: BM25Index, doc_lookup=None, device: str = "cpu"):
        """doc_lookup: callable doc_id → Document (usually DenseIndex.get_document
        or the store's payload map)."""
        self.index = index
        self.doc_lookup = doc_lookup or (lambda _id: None)
        self.device = device
        # filter key -> [bool [n], n, last doc id, packed int32 [1, W]]
        self._masks: dict[str, list] = {}

    def _filter_mask(self, metadata_filter: dict):
        """The filter's int32 [1, W] row mask on the search device, in the
        BM25 index's own row numbering (index.doc_ids; not promised to equal
        the dense index's rows).  The metadata is matched on the host once
        per row: add() appends rows, so a cached filter is extended over
        them; an index rebuilt under other ids starts over."""
        import torch

        from sentio_amd.ops import torch_ref

        ids = self.index.doc_ids
        n = len(ids)
        key = repr(sorted(metadata_filter.items(), key=lambda kv: str(kv[0])))
        ent = self._masks.pop(key, None)
        if ent is None or ent[1] > n or (ent[1] and ids[ent[1] - 1] != ent[2]):
            ent = [torch.empty(0, dtype=torch.bool), 0, None, None]
        if ent[1] < n or ent[3] is None:
            def match(doc_id):
                src = self.doc_lookup(doc_id)
                return src is not None and all(
                    src.metadata.get(f) == v
                    for f, v in metadata_filter.items())

            new = [match(d) for d in ids[ent[1]:n]]
            ent[0] = torch.cat([ent[0], torch.tensor(new, dtype=torch.bool)])
            ent[1], ent[2] = n, ids[n - 1] if n else None
            ent[3] = torch_ref.pack_row_mask(ent[0][None]).to(self.device)
        self._masks[key] = ent                   # most recently used last
        while len(self._masks) > self.MASK_CACHE:
            self._masks.pop(next(iter(self._masks)))
        return ent[3]

    def retrieve(self, query: str, top_k: int = 10,
                 metadata_filter: dict | None = None) -> list[Document]:
        """metadata_filter: equality conditions on document metadata, applied
        as a row mask inside the search: up to top_k matching documents."""
        if metadata_filter and self.index.n_docs:
            vals, rows = self.index.search_batch(
                [query], top_k, device=self.device,
                allow=self._filter_mask(metadata_filter))
            hits = [(self.index.doc_ids[i], v) for i, v in
                    zip(rows[0].cpu().tolist(), vals[0].cpu().tolist())
                    if i >= 0]
        else:
            hits = self.index.search(query, top_k, device=self.device)
        out: list[Document] = []
        for doc_id, score in hits:
            src = self.doc_lookup(doc_id)
            if src is None:
                doc = Document(text="", id=doc_id)
            else:
                doc = Document(text=src.text, metadata=dict(src.metadata), id=src.id)
            doc.metadata["bm25_score"] = float(score)
            doc.metadata["score"] = float(score)
            doc.metadata["retrieval_method"] = "bm25"
            out.append(doc)
        return out
