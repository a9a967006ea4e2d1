"""In-HBM dense vector index with fused cosine top-k.

Replaces the reference's remote Qdrant store + dense retriever
(reference src/core/vector_store/qdrant_store.py:37, src/core/retrievers/
dense.py:46-64: cosine distance, size-1024 collections, payload
{content, metadata}) with a row-major matrix resident in the GPU's 288 GB
HBM3E.  Vectors are L2-normalized at insert so cosine similarity is a plain
dot product; search streams the index through a hipBLASLt TN GEMM
(ops.cosine_topk — the [N, dim] matrix is already F.linear's weight layout)
+ batched top-k: memory-bandwidth-bound, measured ≈6 ms per 10M fp16 rows.

The doc payloads (text + metadata) stay on host — only vectors and the
id-mapping live in HBM.  Multi-GPU sharding wraps this class (parallel/shard).

dtype="fp8" (opt-in) stores e4m3fn codes with one fp32 scale per row instead
(dim + 4 bytes per document against 2 * dim; torch_ref.index_quantize is the
spec) and searches with ops.cosine_topk_fp8, a fused scan + top-k kernel
that writes no [B, N] score matrix.

filter_mode="exact" (opt-in) turns search(metadata_filter=...) from an
over-fetch of top_k * 4 hits filtered on the host into an exact filtered
search: the filter becomes a row bit mask (built on the host from the
payloads, cached per filter, extended as rows are added) and
ops.cosine_topk_masked selects top_k among the allowed rows only.
search_rows(allow=...) takes such masks directly, one per query if wanted.

search(..., mmr_lambda=...) (opt-in) diversifies: fetch_k candidates come
from the path the search would take anyway and ops.mmr_select picks top_k of
them by maximal marginal relevance, from the rows stored here (one kernel:
their Gram matrix on MFMA and the greedy picks).
"""

from __future__ import annotations

import threading
from typing import Any

import torch

from sentio_amd.models.document import Document


class DenseIndex:
    GROW = 65536

    def __init__(
        self,
        dim: int = 1024,
        device: str = "cpu",
        dtype: torch.dtype | str = torch.float16,
        filter_mode: str = "post",
    ) -> None:
        if filter_mode not in ("post", "exact"):
            raise ValueError(f"unknown filter_mode {filter_mode!r}")
        self.filter_mode = filter_mode
        # filter key -> [host bool rows, rows covered, packed device mask]
        self._masks: dict[str, list] = {}
        self.dim = dim
        self.device = device
        self.fp8 = dtype in ("fp8", torch.float8_e4m3fn)
        if isinstance(dtype, str) and not self.fp8:
            raise ValueError(f"unknown index dtype {dtype!r}")
        if self.fp8:
            from sentio_amd import ops

            if not ops.fp8_index_dim_ok(dim):
                raise ValueError("the fp8 index serves dim % 32 == 0 and "
                                 f"dim <= 1024, got {dim}")
            # codes on the CPU too; _vecs stays empty
            self.dtype = torch.float8_e4m3fn
            self._vecs = torch.empty(0, dim, dtype=torch.float16, device=device)
        else:
            # fp16 halves scan bytes vs fp32; fp32 used on CPU for exactness
            self.dtype = dtype if device != "cpu" else torch.float32
            self._vecs = torch.empty(0, dim, dtype=self.dtype, device=device)
        self._codes = torch.empty(0, dim, dtype=torch.uint8, device=device)
        self._scales = torch.empty(0, dtype=torch.float32, device=device)
        self._size = 0
        self.doc_ids: list[str] = []
        self._docs: dict[str, Document] = {}
        self._lock = threading.Lock()

    def __len__(self) -> int:
        return self._size

    # ----- build -----
    def _ensure_capacity(self, extra: int) -> None:
        need = self._size + extra
        cap = self._codes.shape[0] if self.fp8 else self._vecs.shape[0]
        if need <= cap:
            return
        new_cap = max(need, cap + self.GROW, int(cap * 1.5))
        if self.fp8:
            codes = torch.empty(new_cap, self.dim, dtype=torch.uint8,
                                device=self.device)
            scales = torch.empty(new_cap, dtype=torch.float32,
                                 device=self.device)
            if self._size:
                codes[: self._size] = self._codes[: self._size]
                scales[: self._size] = self._scales[: self._size]
            self._codes, self._scales = codes, scales
            return
        new = torch.empty(new_cap, self.dim, dtype=self.dtype, device=self.device)
        if self._size:
            new[: self._size] = self._vecs[: self._size]
        self._vecs = new

    def add(self, docs: list[Document], embeddings: torch.Tensor) -> None:
        """Append documents with their embeddings (L2-normalized on insert)."""
        if embeddings.ndim != 2 or embeddings.shape[1] != self.dim:
            raise ValueError(f"expected [N,{self.dim}] embeddings, got {tuple(embeddings.shape)}")
        if len(docs) != embeddings.shape[0]:
            raise ValueError("docs / embeddings length mismatch")
        with self._lock:
            n = embeddings.shape[0]
            self._ensure_capacity(n)
            emb = embeddings.to(self.device, torch.float32)
            emb = emb / emb.norm(dim=1, keepdim=True).clamp_min(1e-12)
            if self.fp8:
                from sentio_amd.ops import torch_ref

                codes, scales = torch_ref.index_quantize(emb)
                self._codes[self._size : self._size + n] = codes
                self._scales[self._size : self._size + n] = scales
            else:
                self._vecs[self._size : self._size + n] = emb.to(self.dtype)
            self._size += n
            for d in docs:
                self.doc_ids.append(d.id)
                self._docs[d.id] = d

    def add_vectors(self, ids: list[str], embeddings: torch.Tensor,
                    payloads: list[dict[str, Any]] | None = None) -> None:
        docs = [
            Document(text=(p or {}).get("content", ""), metadata=dict(p or {}), id=i)
            for i, p in zip(ids, payloads or [{} for _ in ids])
        ]
        self.add(docs, embeddings)

    # ----- search -----
    def search(
        self, query: torch.Tensor, top_k: int,
        metadata_filter: dict | None = None,
        *, mmr_lambda: float | None = None, fetch_k: int | None = None,
    ) -> list[list[tuple[str, float]]]:
        """Batched cosine top-k.  query: [B, dim] or [dim].
        metadata_filter: equality conditions on document metadata (the
        reference's Qdrant FieldCondition filters, qdrant_store.py:456-471)
        applied as a post-filter over an over-fetched candidate set.
        mmr_lambda in [0, 1]: return top_k of the fetch_k nearest rows
        (default min(max(4 * top_k, 32), 128, size)) picked by maximal
        marginal relevance, in pick order; the scores stay cosines.  With a
        metadata_filter this needs filter_mode="exact"."""
        if query.ndim == 1:
            query = query.unsqueeze(0)
        if self._size == 0:
            return [[] for _ in range(query.shape[0])]
        if mmr_lambda is not None:
            if metadata_filter and self.filter_mode != "exact":
                raise ValueError("mmr_lambda with a metadata_filter needs "
                                 'filter_mode="exact"')
            q = query.to(self.device, torch.float32)
            q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
            allow = self._filter_mask(metadata_filter) \
                if metadata_filter else None
            vals, idx = self._topk_mmr(q, top_k, allow, mmr_lambda, fetch_k)
            return [[(self.doc_ids[i], float(v)) for v, i in zip(vr, ir)
                     if i >= 0]
                    for vr, ir in zip(vals.cpu().tolist(), idx.cpu().tolist())]
        if metadata_filter and self.filter_mode == "exact":
            q = query.to(self.device, torch.float32)
            q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
            vals, idx = self._topk_masked(q, top_k,
                                          self._filter_mask(metadata_filter))
            return [[(self.doc_ids[i], float(v)) for v, i in zip(vr, ir)
                     if i >= 0]
                    for vr, ir in zip(vals.cpu().tolist(), idx.cpu().tolist())]
        fetch_k = min(top_k * 4, self._size) if metadata_filter else top_k
        k = min(fetch_k, self._size)
        q = query.to(self.device, torch.float32)
        q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)

        if self.fp8:
            vals, idx = self._topk_fp8(q, k)
        elif self.device != "cpu":
            from sentio_amd import ops

            vals, idx = ops.cosine_topk(q.to(self.dtype), self._vecs[: self._size], k)
        else:
            scores = q @ self._vecs[: self._size].T.float()
            vals, idx = torch.topk(scores, k, dim=1)
        vals_l = vals.cpu().tolist()
        idx_l = idx.cpu().tolist()
        out = []
        for bi in range(len(vals_l)):
            hits = [(self.doc_ids[i], float(v))
                    for v, i in zip(vals_l[bi], idx_l[bi])]
            if metadata_filter:
                hits = [
                    (doc_id, v) for doc_id, v in hits
                    if all(self._docs[doc_id].metadata.get(key) == val
                           for key, val in metadata_filter.items())
                ][:top_k]
            out.append(hits)
        return out

    def search_rows(self, query: torch.Tensor, top_k: int,
                    allow: torch.Tensor | None = None,
                    *, mmr_lambda: float | None = None,
                    fetch_k: int | None = None
                    ) -> tuple[torch.Tensor, torch.Tensor]:
        """Tensor-only batched cosine top-k: (scores [B,k] f32, rows [B,k]
        i64), padded with (-inf, -1) when the shard holds fewer than top_k
        rows.  NO host sync — the multi-GPU merge all-gathers these tensors
        directly (no pickled objects on the query hot path).
        allow: int32 [1 or B, W] row mask on the index device
        (ops.pack_row_mask), one for all queries or one per query: the
        search runs over the allowed rows only, in either filter_mode.
        mmr_lambda, fetch_k: as in search(); rows come in pick order."""
        if query.ndim == 1:
            query = query.unsqueeze(0)
        B = query.shape[0]
        if self._size == 0:
            return (torch.full((B, top_k), float("-inf"), device=self.device),
                    torch.full((B, top_k), -1, dtype=torch.int64,
                               device=self.device))
        if mmr_lambda is not None:
            q = query.to(self.device, torch.float32)
            q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
            return self._topk_mmr(q, top_k, allow, mmr_lambda, fetch_k)
        k = min(top_k, self._size)
        q = query.to(self.device, torch.float32)
        q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
        if allow is not None:
            return self._topk_masked(q, top_k, allow)
        if self.fp8:
            vals, idx = self._topk_fp8(q, k)
        elif self.device != "cpu":
            from sentio_amd import ops

            vals, idx = ops.cosine_topk(q.to(self.dtype),
                                        self._vecs[: self._size], k)
        else:
            scores = q @ self._vecs[: self._size].T.float()
            vals, idx = torch.topk(scores, k, dim=1)
        vals = vals.float()
        idx = idx.long()
        if k < top_k:
            vals = torch.cat([vals, torch.full((B, top_k - k), float("-inf"),
                                               device=vals.device)], 1)
            idx = torch.cat([idx, torch.full((B, top_k - k), -1,
                                             dtype=torch.int64,
                                             device=idx.device)], 1)
        return vals, idx

    def _topk_fp8(self, q: torch.Tensor, k: int
                  ) -> tuple[torch.Tensor, torch.Tensor]:
        """k <= size best rows of the fp8 index for normalised fp32 queries
        (fp16 into the kernel, as on the fp16 path).  The kernel selects at
        most 128 per query: a larger k (top_k, or a filtered search's
        top_k * 4) raises ValueError."""
        from sentio_amd import ops

        return ops.cosine_topk_fp8(q.to(torch.float16),
                                   self._codes[: self._size],
                                   self._scales[: self._size], k)

    MASK_CACHE = 16

    def _topk_masked(self, q: torch.Tensor, k: int, allow: torch.Tensor
                     ) -> tuple[torch.Tensor, torch.Tensor]:
        """The k best allowed rows for normalised fp32 queries, padded with
        (-inf, -1).  The masked scan kernel serves GPU fp8 and fp16 indexes
        at dim % 32 == 0, dim <= 1024 and k <= 128; any other shape and the
        CPU take the reference."""
        from sentio_amd import ops
        from sentio_amd.ops import torch_ref

        n = self._size
        if allow.dtype != torch.int32 or allow.dim() != 2 or \
                allow.shape[0] not in (1, q.shape[0]) or \
                allow.shape[1] != 4 * ((n + 127) // 128) or \
                allow.device != q.device:
            raise ValueError(f"allow must be int32 [1 or {q.shape[0]}, "
                             f"{4 * ((n + 127) // 128)}] on {q.device}")
        rows = self._codes[:n] if self.fp8 else self._vecs[:n]
        scales = self._scales[:n] if self.fp8 else None
        if self.device != "cpu" and ops.fp8_index_dim_ok(self.dim) \
                and k <= 128 and (self.fp8 or self.dtype == torch.float16):
            return ops.cosine_topk_masked(q.to(torch.float16), rows, scales,
                                          k, allow.contiguous())
        qq = q.to(torch.float16) if self.fp8 else q
        return torch_ref.cosine_topk_masked(qq, rows, scales, k, allow)

    def _topk_mmr(self, q: torch.Tensor, top_k: int,
                  allow: torch.Tensor | None, lam: float,
                  fetch_k: int | None) -> tuple[torch.Tensor, torch.Tensor]:
        """top_k of the fetch_k nearest (allowed) rows for normalised fp32
        queries, picked by maximal marginal relevance over the stored rows;
        (cosine, row) in pick order, padded with (-inf, -1).  The candidates
        come from the path a plain search takes; ops.mmr_select serves GPU
        fp8 and fp16 indexes at dim % 32 == 0 and dim <= 1024, any other
        shape and the CPU take the reference.  No host sync."""
        from sentio_amd import ops
        from sentio_amd.ops import torch_ref

        n, lam = self._size, float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"mmr_lambda must be in [0, 1], got {lam}")
        if fetch_k is None:
            fetch_k = min(max(4 * top_k, 32), 128)
        if not 1 <= top_k <= fetch_k <= 128:
            raise ValueError("mmr needs 1 <= top_k <= fetch_k <= 128, got "
                             f"top_k {top_k}, fetch_k {fetch_k}")
        fetch = min(fetch_k, n)
        if allow is not None:
            _, cand = self._topk_masked(q, fetch, allow)
        elif self.fp8:
            _, cand = self._topk_fp8(q, fetch)
        elif self.device != "cpu":
            _, cand = ops.cosine_topk(q.to(self.dtype), self._vecs[:n], fetch)
        else:
            _, cand = torch.topk(q @ self._vecs[:n].T.float(), fetch, dim=1)
        cand = cand.long().contiguous()
        k = min(top_k, fetch)
        rows = self._codes[:n] if self.fp8 else self._vecs[:n]
        scales = self._scales[:n] if self.fp8 else None
        if self.device != "cpu" and ops.fp8_index_dim_ok(self.dim) \
                and (self.fp8 or self.dtype == torch.float16):
            vals, idx = ops.mmr_select(q.to(torch.float16), rows, scales,
                                       cand, k, lam)
        else:
            qq = q.to(torch.float16) if self.fp8 else q
            vals, idx = torch_ref.mmr_select(qq, rows, scales, cand, k, lam)
        if k < top_k:
            B = q.shape[0]
            vals = torch.cat([vals, vals.new_full((B, top_k - k),
                                                  float("-inf"))], 1)
            idx = torch.cat([idx, idx.new_full((B, top_k - k), -1)], 1)
        return vals, idx

    def _filter_mask(self, metadata_filter: dict) -> torch.Tensor:
        """The filter's int32 [1, W] row mask on the index device.  The
        metadata is matched on the host once per row: a cached filter is
        extended over the rows added since, never rebuilt."""
        from sentio_amd.ops import torch_ref

        key = repr(sorted(metadata_filter.items(), key=lambda kv: str(kv[0])))
        with self._lock:
            n = self._size
            ent = self._masks.pop(key, None) or \
                [torch.empty(0, dtype=torch.bool), 0, None]
            if ent[1] < n:
                new = [all(self._docs[d].metadata.get(f) == v
                           for f, v in metadata_filter.items())
                       for d in self.doc_ids[ent[1]:n]]
                ent[0] = torch.cat([ent[0], torch.tensor(new, dtype=torch.bool)])
                ent[1] = n
                ent[2] = torch_ref.pack_row_mask(ent[0][None]).to(self.device)
            self._masks[key] = ent               # most recently used last
            while len(self._masks) > self.MASK_CACHE:
                self._masks.pop(next(iter(self._masks)))
            return ent[2]

    def get_document(self, doc_id: str) -> Document | None:
        return self._docs.get(doc_id)

    def get_document_by_row(self, row: int) -> Document | None:
        if 0 <= row < self._size and self.doc_ids:
            return self._docs.get(self.doc_ids[row])
        return None

    def clear(self) -> None:
        with self._lock:
            self._vecs = torch.empty(0, self.dim, dtype=self._vecs.dtype,
                                     device=self.device)
            self._codes = torch.empty(0, self.dim, dtype=torch.uint8,
                                      device=self.device)
            self._scales = torch.empty(0, dtype=torch.float32,
                                       device=self.device)
            self._size = 0
            self.doc_ids.clear()
            self._docs.clear()
            self._masks.clear()

    # ----- snapshot save/load (reference had BM25 pickle + external Qdrant;
    # here the index itself persists: HBM→disk) -----
    def save(self, path: str) -> None:
        with self._lock:
            state = {
                "dim": self.dim,
                "doc_ids": self.doc_ids,
                "docs": [self._docs[d].to_dict() for d in self.doc_ids],
            }
            if self.fp8:
                state["dtype"] = "fp8"
                state["codes"] = self._codes[: self._size].to("cpu")
                state["scales"] = self._scales[: self._size].to("cpu")
            else:
                state["vecs"] = self._vecs[: self._size].to("cpu")
            torch.save(state, path)

    @classmethod
    def load(cls, path: str, device: str = "cpu") -> "DenseIndex":
        state = torch.load(path, map_location="cpu", weights_only=False)
        docs = [Document.from_dict(d) for d in state["docs"]]
        if state.get("dtype") == "fp8":
            # codes and scales byte for byte: no re-quantisation
            idx = cls(dim=state["dim"], device=device, dtype="fp8")
            n = len(docs)
            idx._ensure_capacity(n)
            idx._codes[:n] = state["codes"].to(device)
            idx._scales[:n] = state["scales"].to(device)
            idx._size = n
            for d in docs:
                idx.doc_ids.append(d.id)
                idx._docs[d.id] = d
            return idx
        idx = cls(dim=state["dim"], device=device)
        vecs = state["vecs"].to(torch.float32)
        if len(docs):
            idx.add(docs, vecs)
        return idx

    # ----- stats -----
    def stats(self) -> dict[str, Any]:
        return {
            "size": self._size,
            "dim": self.dim,
            "device": str(self.device),
            "dtype": "fp8" if self.fp8 else str(self.dtype),
            "filter_mode": self.filter_mode,
            "cached_filter_masks": len(self._masks),
            "hbm_bytes": (self._codes.nelement() + 4 * self._scales.nelement()
                          if self.fp8 else
                          self._vecs.element_size() * self._vecs.nelement()),
        }
