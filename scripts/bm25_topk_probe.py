"""BM25 search microbenchmark: the fused batched kernel (ops.bm25_topk)
beside the scores path (one ops.bm25_score launch per query, stack,
torch.topk: what bench.py's bm25_search_batch and BM25Index do by default)
over one synthetic index, B = 32, k = 10, the paths alternating inside every
repeat; then the fused kernel under a mask that allows 1 % of the documents.
Run: python scripts/bm25_topk_probe.py [N_DOCS]     (default 10M, 32
     term draws per document as bench.py draws them, a (term, document)
     pair drawn twice becoming tf = 2: ~200M postings)
Two query sets: "uniform" is bench.py's (4 terms drawn uniformly from the
vocabulary: mostly rare terms), "zipf" draws 4 terms as the corpus draws them
(mostly common terms: long postings lists).  Bytes are counted from shapes."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

VOCAB, PER_DOC, B, K = 30000, 32, 32, 10
K1, B_ = 1.5, 0.75


def build(n, dev):
    from bench import _zipf_terms

    g = torch.Generator(device=dev).manual_seed(2000)
    key = _zipf_terms(n * PER_DOC, 1.3, VOCAB, g, dev) * n \
        + torch.arange(n * PER_DOC, device=dev) // PER_DOC
    key, tf = torch.unique(key, return_counts=True)      # sorted (term, doc)
    counts = torch.bincount(key // n, minlength=VOCAB)
    indptr = torch.zeros(VOCAB + 1, dtype=torch.int64, device=dev)
    indptr[1:] = counts.cumsum(0)
    df = counts.double()
    return {"indptr": indptr, "post_doc": (key % n).int(), "post_tf": tf.float(),
            "idf": torch.log((n - df + 0.5) / (df + 0.5) + 1.0).float(),
            "doc_len": torch.randint(40, 200, (n,), generator=g,
                                     device=dev).float()}, g


def event_median(fn, iters):
    """Median HIP-event time of one call, in seconds."""
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True),
           torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[iters // 2] / 1e3


def main(n, repeats=3, iters=20):
    from bench import _zipf_terms
    from sentio_amd import ops

    dev = "cuda:0"
    a, g = build(n, dev)
    arrays = (a["indptr"], a["post_doc"], a["post_tf"], a["idf"], a["doc_len"])
    kw = dict(n_docs=n, k1=K1, b=B_, avgdl=float(a["doc_len"].mean()))
    blocks, tile, _ = ops.bm25_topk_plan(n)
    print(f"--- N={n} postings={a['post_doc'].numel()} B={B} k={K}: blocks "
          f"{blocks}, tile {tile}, median of {iters} event-timed calls, "
          f"{repeats} repeats")
    allow = ops.pack_row_mask(
        (torch.rand(n, generator=g, device=dev) < 0.01)[None])
    sets = {"uniform": torch.randint(0, VOCAB, (B * 4,), generator=g,
                                     device=dev),
            "zipf": _zipf_terms(B * 4, 1.3, VOCAB, g, dev)}
    qoff = torch.arange(0, B * 4 + 1, 4, dtype=torch.int32)
    for name, tids in sets.items():
        per_q = [tids[i:i + 4] for i in range(0, B * 4, 4)]

        def scores_path():
            s = torch.stack([ops.bm25_score(t, *arrays, **kw) for t in per_q])
            vals, idx = torch.topk(s, K, dim=1)
            dead = vals <= 0.0
            return vals.masked_fill(dead, float("-inf")), idx.masked_fill(dead, -1)

        def fused(al=None):
            return ops.bm25_topk(tids, qoff, *arrays, k=K, allow=al, **kw)

        variants = [("scores path (32 launches + topk)", scores_path),
                    ("fused, unfiltered", fused),
                    ("fused, 1 % of rows allowed", lambda: fused(allow))]
        times = {v: [] for v, _ in variants}
        for _ in range(repeats):
            for v, fn in variants:
                times[v].append(event_median(fn, iters))
        touched = int((a["indptr"][tids + 1] - a["indptr"][tids]).sum())
        tiles = (n + tile - 1) // tile
        print(f"query set {name}: {touched} postings in the queries' lists")
        # scores path: zero + atomics (read-modify-write) per query, stack
        # (read + write), topk (read); per posting doc, tf, doc_len, score rmw
        print(f"  bytes, scores path: {(B * n * 4 * 4 + touched * 20) / 1e9:.3f}"
              f" GB; fused: "
              f"{(touched * 8 + n * 4 + tiles * B * 4 * 2 * 28 * 4) / 1e9:.3f}"
              " GB (postings, doc_len, ~28 search loads per term bound)")
        for v, ts in times.items():
            print(f"  {v:34s} " + " ".join(f"{t * 1e3:8.3f}" for t in ts) + " ms")
        t0, t1 = min(times[variants[0][0]]), min(times[variants[1][0]])
        print(f"  scores path / fused = {t0 / t1:.2f}x")
        # the timed paths must agree: same rows wherever scores are not tied
        (sv, sr), (fv, fr) = scores_path(), fused()
        tied = (fv[:, 1:] == fv[:, :-1]).any().item()
        print(f"  max |score diff| = {(sv - fv).nan_to_num(0, 0, 0).abs().max():.3e}"
              f", rows equal: {torch.equal(sr, fr)} (ties present: {tied})")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit(f"{__file__}: needs a GPU (MI355X)")
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000)
