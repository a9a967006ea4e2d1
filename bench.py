"""Flagship benchmark: end-to-end /chat serving steps on N GPUs of one node.

Measures BASELINE.json's north-star metric — end-to-end /chat QPS (+p50) on
a hybrid-RAG pipeline with a Llama-3-8B-class generator — on synthetic
corpora and random-init weights (no network for datasets/checkpoints).

One step = one batch of `--batch` concurrent /chat requests per rank through
the full pipeline: query embed (encoder engine) → sharded dense cosine top-k
(RCCL all-gather merge) → GPU BM25 → RRF fusion → cross-encoder rerank →
selection → batched generation (prefill + `--gen-tokens` KV-cache decode
steps) [→ optional verifier].  Weak scaling: each GPU holds a fixed
`--docs-per-gpu` corpus shard and serves its own request batch; value is the
whole-job aggregate QPS over all ranks.

Driver contract: `python bench.py --gpus N --steps K --warmup W`; for N>1
launched under torch.distributed.run with one rank per GPU over RCCL.
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times `--steps` steps and prints the line.
`--dump-outputs DIR` also writes the last timed step's retrieval results as
DIR/<name>.npy (same arguments → same corpus, weights and queries, and the
same values up to rounding, so two builds can be compared output for
output); `--full` is where any further measurement goes.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from sentio_amd.index.bm25 import BM25Index
from sentio_amd.index.dense import DenseIndex
from sentio_amd.models.document import Document
from sentio_amd.parallel import dist as D
from sentio_amd.parallel.shard import ShardedIndex
from sentio_amd.pipeline.context import prepare_context
from sentio_amd.pipeline.prompt_builder import PromptBuilder


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--batch", type=int, default=32,
                   help="concurrent /chat requests per rank per step")
    p.add_argument("--docs-per-gpu", type=int, default=None,
                   help="synthetic corpus shard per GPU; default sizes the "
                        "TOTAL corpus to 10M docs at any world size "
                        "(BASELINE config #4 — it fits in one GPU's 288 GB)")
    p.add_argument("--gen-tokens", type=int, default=128)
    p.add_argument("--model", type=str, default="llama3-8b")
    p.add_argument("--encoder", type=str, default="sentio-encoder-base")
    p.add_argument("--reranker", type=str, default="sentio-reranker-base")
    p.add_argument("--top-k", type=int, default=10)
    p.add_argument("--rerank-top-k", type=int, default=5)
    p.add_argument("--select-top-k", type=int, default=3)
    p.add_argument("--verify", default=True,
                   action=argparse.BooleanOptionalAction,
                   help="include the verifier pass (BASELINE config #4 is "
                        "the FULL graph incl. verifier — default on; "
                        "--no-verify for the generation-only envelope)")
    p.add_argument("--verify-tokens", type=int, default=64)
    p.add_argument("--vocab-terms", type=int, default=30000)
    p.add_argument("--seq-len", type=int, default=2048,
                   help="generation context budget (prompt cap)")
    p.add_argument("--tp", type=int, default=1,
                   help="tensor-parallel degree for the generator "
                        "(must equal world size; config #5: --model "
                        "llama3-70b --tp 8)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write the last timed step's "
                        "retrieval results (query embeddings; dense, "
                        "sparse and fused top-k scores) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the benchmark's secondary measurements "
                        "(everything beyond the headline figure belongs "
                        "here; there is none at present — the stage "
                        "breakdown on stderr costs no run of its own)")
    return p.parse_args()


class SyntheticCorpus:
    """Deterministic on-the-fly document payloads — 10M stored texts would
    be pure host-RAM waste; content derives from the doc ref."""

    WORDS = ["gpu", "hbm", "kernel", "index", "retrieval", "engine", "tensor",
             "wave", "cache", "stream", "graph", "shard", "fusion", "decode"]

    def __init__(self, shard: int):
        self.shard = shard

    def text_for(self, idx: int, shard: int | None = None) -> str:
        shard = self.shard if shard is None else shard
        rng = np.random.RandomState((shard << 20) ^ idx)
        words = rng.choice(self.WORDS, size=60)
        return (f"synthetic document {shard}:{idx} " + " ".join(words))

    def doc_for(self, ref: str) -> Document:
        shard_s, idx_s = ref.split(":", 1)
        return Document(text=self.text_for(int(idx_s), shard=int(shard_s)),
                        metadata={"source": f"doc-{ref}"}, id=ref)


def _zipf_terms(nnz: int, a: float, vocab: int, gen: torch.Generator,
                device: str) -> torch.Tensor:
    """nnz draws of (Zipf(a) - 1) % vocab as int64 on `device`: the rejection
    sampler of Devroye (Non-Uniform Random Variate Generation, X.6.1 — the
    one numpy's zipf uses), run on whole tensors.  Seeded by `gen`, so the
    same arguments give the same draws."""
    am1 = a - 1.0
    b = 2.0 ** am1
    out = torch.empty(nnz, dtype=torch.int64, device=device)
    filled = 0
    while filled < nnz:
        n = min(int((nnz - filled) * 1.25) + 4096, 1 << 26)
        u = 1.0 - torch.rand(n, generator=gen, device=device,
                             dtype=torch.float64)          # (0, 1]
        v = torch.rand(n, generator=gen, device=device, dtype=torch.float64)
        x = torch.floor(u.pow(-1.0 / am1))
        t = (1.0 + 1.0 / x).pow(am1)
        ok = (x >= 1.0) & (x < 2.0 ** 63) & (v * x * (t - 1.0) / (b - 1.0)
                                             <= t / b)
        acc = x[ok][: nnz - filled]
        out[filled: filled + acc.numel()] = torch.fmod(acc - 1.0, vocab).long()
        filled += acc.numel()
    return out


def build_synthetic_indexes(n_docs: int, dim: int, vocab: int, device: str,
                            rank: int):
    """Dense: random unit vectors in HBM.  BM25: synthetic CSR postings
    (zipf-ish doc frequencies) drawn, sorted and kept on `device` — at 10M
    docs the 200M postings took most of a minute to draw and sort on the
    host, all of it outside the timed steps."""
    # same corpus every run: the dense fill draws from the default
    # generator, the postings from their own
    torch.manual_seed(1000 + rank)
    g = torch.Generator(device=device)
    g.manual_seed(2000 + rank)
    dense = DenseIndex(dim=dim, device=device,
                       dtype=torch.float16 if device != "cpu" else torch.float32)
    # bulk vector fill without Document objects (payloads are synthetic)
    chunk = 262144
    dense._ensure_capacity(n_docs)
    for i0 in range(0, n_docs, chunk):
        n = min(chunk, n_docs - i0)
        v = torch.randn(n, dim, device=device)
        v = v / v.norm(dim=1, keepdim=True)
        dense._vecs[i0:i0 + n] = v.to(dense.dtype)
    dense._size = n_docs
    dense.doc_ids = None  # replaced by int refs below

    # BM25 postings: ~20 distinct terms per doc
    per_doc = 20
    nnz = n_docs * per_doc
    # zipf-flavored term draw, clipped to vocab; posting p of the unsorted
    # draw belongs to doc p // per_doc
    terms = _zipf_terms(nnz, 1.3, vocab, g, device)
    terms_sorted, order = torch.sort(terms, stable=True)
    del terms
    post_doc = (order // per_doc).to(torch.int32)
    del order
    post_tf = torch.randint(1, 5, (nnz,), generator=g,
                            device=device).to(torch.float32)
    counts = torch.bincount(terms_sorted, minlength=vocab)
    del terms_sorted
    indptr = torch.zeros(vocab + 1, dtype=torch.int64, device=device)
    indptr[1:] = torch.cumsum(counts, 0)
    doc_len = torch.randint(40, 200, (n_docs,), generator=g,
                            device=device).to(torch.float32)
    df = counts.to(torch.float64)
    idf = torch.log((n_docs - df + 0.5) / (df + 0.5) + 1.0).to(torch.float32)

    bm = BM25Index()
    bm.doc_ids = None
    bm.vocab = {f"term{i}": i for i in range(vocab)}
    bm.doc_len = doc_len.cpu().numpy()
    bm.indptr = indptr.cpu().numpy()
    bm.post_doc = post_doc.cpu().numpy()
    bm.post_tf = post_tf.cpu().numpy()
    bm.idf = idf.cpu().numpy()
    if device != "cpu":
        # already resident: no second upload at the first search
        bm._device_arrays = {"indptr": indptr, "post_doc": post_doc,
                             "post_tf": post_tf, "idf": idf,
                             "doc_len": doc_len}
    return dense, bm


def dense_search_ids(dense: DenseIndex, q: torch.Tensor, k: int):
    """Index-level search returning integer row ids (bulk synthetic corpus
    has no Document list)."""
    if dense._size == 0:
        return [[] for _ in range(q.shape[0])]
    k = min(k, dense._size)
    qq = q.to(dense.device, torch.float32)
    qq = qq / qq.norm(dim=1, keepdim=True).clamp_min(1e-12)
    if dense.device != "cpu":
        from sentio_amd import ops

        vals, idx = ops.cosine_topk(qq.to(dense.dtype), dense._vecs[: dense._size], k)
    else:
        scores = qq @ dense._vecs[: dense._size].T.float()
        vals, idx = torch.topk(scores, k, dim=1)
    return vals, idx


def bm25_search_batch(bm: BM25Index, term_id_lists: list[np.ndarray], k: int,
                      device: str):
    """Score a whole query batch; NO host sync: launch every query's scoring
    kernel back-to-back, stack, one batched top-k.  Returns device tensors
    (vals [Q,k] f32, rows [Q,k] i64) with score<=0 padded to (-inf, -1)."""
    import torch as T

    if device != "cpu":
        from sentio_amd import ops

        if not bm._device_arrays:
            bm._device_arrays = {
                "indptr": T.from_numpy(bm.indptr).to(device),
                "post_doc": T.from_numpy(bm.post_doc).to(device),
                "post_tf": T.from_numpy(bm.post_tf).to(device),
                "idf": T.from_numpy(bm.idf).to(device),
                "doc_len": T.from_numpy(bm.doc_len).to(device),
            }
        a = bm._device_arrays
        avgdl = float(bm.doc_len.mean())
        per_q = []
        for term_ids in term_id_lists:
            tids = T.from_numpy(term_ids).to(device)
            per_q.append(ops.bm25_score(
                tids, a["indptr"], a["post_doc"], a["post_tf"], a["idf"],
                a["doc_len"], n_docs=len(bm.doc_len), k1=bm.k1, b=bm.b,
                avgdl=avgdl, plus_delta=0.0))
        S = T.stack(per_q)                       # [Q, N]
    else:
        avgdl = max(float(bm.doc_len.mean()), 1e-9)
        den = bm.k1 * (1 - bm.b + bm.b * bm.doc_len / avgdl)
        rows = []
        for term_ids in term_id_lists:
            scores = np.zeros(len(bm.doc_len), np.float32)
            for t in term_ids:
                lo, hi = bm.indptr[t], bm.indptr[t + 1]
                d = bm.post_doc[lo:hi]
                tf = bm.post_tf[lo:hi]
                scores[d] += bm.idf[t] * tf * (bm.k1 + 1) / (tf + den[d])
            rows.append(T.from_numpy(scores))
        S = T.stack(rows)
    vals, idx = T.topk(S, min(k, S.shape[1]), dim=1)
    dead = vals <= 0.0
    return (vals.masked_fill(dead, float("-inf")),
            idx.long().masked_fill(dead, -1))


def dump_outputs(directory: str, last_out: dict) -> None:
    """Write the last step's retrieval results, one DIR/<name>.npy each
    (float32, shapes fixed by the arguments): the query embeddings, each
    query's dense and sparse top-k scores (descending; 0 where BM25 found
    fewer than k hits) and its fused top-k scores.

    Only what repeats from run to run up to rounding is written.  The
    step's retrieval overlaps the previous step's generation, and under
    that contention the library GEMMs' accumulation order is not fixed, so
    scores move in their last bits; the score VALUES written here follow
    continuously, but ids flip at near-ties, and with them the rerank
    candidates, sources and prompts.  Generated text is further out of
    reach: the decode kernels accumulate through atomics and their GEMM
    algorithm is picked by timing, and sampled decoding from random-init
    weights turns a last-bit difference into another token."""
    os.makedirs(directory, exist_ok=True)
    sparse = last_out["sparse_scores"].float()
    arrays = {
        "query_embeddings": last_out["query_embeddings"].float(),
        "dense_scores": last_out["dense_scores"].float(),
        "sparse_scores": sparse.masked_fill(torch.isinf(sparse), 0.0),
        "fused_scores": last_out["fused_scores"].float(),
    }
    for name, t in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), t.cpu().numpy())


def main():
    args = parse_args()
    rank, world = D.init_distributed()
    on_gpu = torch.cuda.is_available()
    device = f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}" if on_gpu else "cpu"
    if on_gpu:
        torch.cuda.set_device(device)

    if args.docs_per_gpu is None:
        # BASELINE config #4: 10M docs TOTAL at any world size
        args.docs_per_gpu = 10_000_000 // max(world, 1)

    # CPU plumbing fallback (no GPU in the dev container)
    if not on_gpu:
        args.model = "tiny-decoder64"
        args.encoder = "tiny-encoder"
        args.reranker = "tiny-reranker"
        args.docs_per_gpu = min(args.docs_per_gpu, 2000)
        args.batch = min(args.batch, 2)
        args.gen_tokens = min(args.gen_tokens, 8)

    from sentio_amd.engines.encoder import EncoderEngine
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.engines.reranker import RerankerEngine
    from sentio_amd.parallel.tp import TPContext

    tp_mode = args.tp > 1
    if tp_mode:
        assert world == args.tp, (
            f"--tp {args.tp} requires world size {args.tp} (got {world}); "
            "all ranks form one TP group")

    t_init = time.time()
    encoder = EncoderEngine(args.encoder, device=device, max_seq=128)
    reranker = RerankerEngine(args.reranker, device=device, max_seq=256)
    generator = GeneratorEngine(args.model, device=device,
                                max_seq=args.seq_len + args.gen_tokens + 8,
                                tp=TPContext.from_env() if tp_mode else None)
    dense, bm = build_synthetic_indexes(
        args.docs_per_gpu, encoder.dim, args.vocab_terms, device, rank)
    corpus = SyntheticCorpus(rank)
    builder = PromptBuilder("balanced")
    if on_gpu:
        torch.cuda.synchronize()
    init_s = time.time() - t_init

    # TP mode: every rank must build IDENTICAL queries (one shared batch
    # through the TP group); DP mode: per-rank query streams.
    rng = np.random.RandomState(42 if tp_mode else 42 + rank)

    def make_queries(step: int) -> list[str]:
        out = []
        for b in range(args.batch):
            terms = rng.randint(0, args.vocab_terms, size=4)
            out.append(
                f"what does term{terms[0]} term{terms[1]} mean for "
                f"term{terms[2]} term{terms[3]} retrieval step {step}?")
        return out

    stage_t: dict[str, float] = {}
    last_out: dict = {}     # --dump-outputs: what the latest step returned

    def _mark(name: str, t0: float) -> float:
        """Accumulate per-stage wall time for the stderr breakdown.  Syncs
        ONLY the current stream: retrieval stages run on a side stream
        under the previous step's generation, and a device-wide sync made
        every stage absorb the decode stream's backlog (r1's breakdown
        showed a 640 ms "embed" stage that is really ~6 ms isolated —
        VERDICT item 9).  Cross-stream contention still counts; these are
        in-context times, not isolated kernel rates (see profiles/)."""
        if on_gpu:
            torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        stage_t[name] = stage_t.get(name, 0.0) + (t1 - t0)
        return t1

    # The per-step pipeline is split into a retrieval phase (stages 1-6,
    # ends fully host-synced) and a generation phase (7-8).  Steps are
    # independent requests, so step N+1's retrieval runs on a side thread +
    # side HIP stream UNDER step N's generation — steady-state serving
    # overlap; ms_per_step stays wall-clock / completed batches.
    # global candidate id = (shard << SHARD_SHIFT) | local row — lets the
    # whole cross-shard merge + fusion stay in int64/fp32 tensors on device
    SHARD_SHIFT = 40
    from sentio_amd import ops

    def _merge_shards(vals_loc, ids_loc, rows_sel=None):
        """all-gather per-shard candidate tensors and merge to a global
        per-query top-k — pure tensor collectives (no pickled objects,
        VERDICT r1 item 3).  vals_loc/ids_loc: [Q, k] local-shard top-k.
        rows_sel: slice of query rows this rank owns (None = all)."""
        k = vals_loc.shape[1]
        v_all = D.all_gather_tensor(vals_loc).view(world, -1, k)
        i_all = D.all_gather_tensor(ids_loc).view(world, -1, k)
        if rows_sel is not None:
            v_all = v_all[:, rows_sel]
            i_all = i_all[:, rows_sel]
        shard_tag = (torch.arange(world, device=v_all.device, dtype=torch.int64)
                     .view(world, 1, 1) << SHARD_SHIFT)
        gid = torch.where(i_all >= 0, i_all + shard_tag,
                          torch.full_like(i_all, -1))
        B_ = v_all.shape[1]
        v2 = v_all.permute(1, 0, 2).reshape(B_, world * k)
        g2 = gid.permute(1, 0, 2).reshape(B_, world * k)
        topv, topi = v2.topk(k, dim=1)
        return topv, g2.gather(1, topi)

    def retrieval_phase(step: int):
        t0 = time.perf_counter()
        queries = make_queries(step)
        # 1. embed queries (one encoder batch)
        qv = encoder.embed(queries)
        t0 = _mark("embed", t0)
        # 2. dense search over ALL ranks' shards (SPMD all-gather)
        if world > 1:
            q_all = D.all_gather_tensor(qv)
        else:
            q_all = qv
        vals, idx = dense_search_ids(dense, q_all, args.top_k)
        base = rank * args.batch
        if world > 1:
            d_scores, d_ids = _merge_shards(
                vals, idx.long(), rows_sel=slice(base, base + args.batch))
        else:
            d_scores, d_ids = vals, idx.long()
        t0 = _mark("dense", t0)
        # 3. sparse search: gather ALL ranks' query terms (padded int64
        # tensor), score them against the LOCAL postings shard, then the
        # same tensor merge as dense — every query is scored on every shard
        tid_lists = [
            np.array([int(tok[4:]) for tok in q.split()
                      if tok.startswith("term") and tok[4:].isdigit()],
                     np.int64)
            for q in queries
        ]
        if world > 1:
            TW = 8   # terms per query (4 by construction; headroom)
            tid_mat = torch.full((args.batch, TW), -1, dtype=torch.int64)
            for i, t in enumerate(tid_lists):
                tid_mat[i, : min(len(t), TW)] = torch.from_numpy(t[:TW])
            tid_all = D.all_gather_tensor(
                tid_mat.to(D.collective_device())).cpu().numpy()
            all_tids = [row[row >= 0] for row in tid_all]       # W*B queries
        else:
            all_tids = tid_lists
        s_vals, s_rows = bm25_search_batch(bm, all_tids, args.top_k, device)
        if world > 1:
            s_scores, s_ids = _merge_shards(
                s_vals, s_rows, rows_sel=slice(base, base + args.batch))
        else:
            s_scores, s_ids = s_vals, s_rows
        t0 = _mark("bm25", t0)

        # 4. device fusion (K4 kernel): ONE host sync for the whole batch's
        # fused top-k — the r1 host fuse.fuse loop cost ~22 ms/step
        f_ids, f_scores = ops.fuse_topk(
            d_ids.contiguous(), d_scores.contiguous(),
            s_ids.contiguous(), s_scores.contiguous(),
            method="rrf", top_k=args.top_k, rrf_k=60)
        ids_l = f_ids.cpu().tolist()
        sc_l = f_scores.cpu().tolist()
        mask = (1 << SHARD_SHIFT) - 1
        batch_docs = []
        for qi in range(args.batch):
            docs = []
            for g, s in zip(ids_l[qi], sc_l[qi]):
                if g < 0:
                    continue
                d = corpus.doc_for(f"{g >> SHARD_SHIFT}:{g & mask}")
                d.metadata["score"] = float(s)
                docs.append(d)
            batch_docs.append(docs)
        t0 = _mark("fuse", t0)

        # 5. rerank all queries' candidates in one cross-encoder batch
        pair_texts = []
        spans = []
        for qi, docs in enumerate(batch_docs):
            top_n = min(len(docs), 2 * args.rerank_top_k)
            spans.append((len(pair_texts), top_n))
            pair_texts.extend(f"{queries[qi]}\n{d.text}" for d in docs[:top_n])
        scores = reranker.score_packed(pair_texts) if pair_texts else []
        # NOTE: pair text already contains the query; score_pairs prefixes
        # query="" so the packed text is the pair.
        reranked = []
        for qi, (off, n) in enumerate(spans):
            cand = batch_docs[qi][:n]
            sc = scores[off: off + n]
            order = sorted(range(n), key=lambda i: sc[i], reverse=True)
            keep = []
            for i in order[: args.rerank_top_k]:
                cand[i].metadata["score"] = float(sc[i])
                keep.append(cand[i])
            reranked.append(keep)
        t0 = _mark("rerank", t0)

        # 6. select + prompts
        prompts = []
        for qi in range(args.batch):
            docs = reranked[qi][: args.select_top_k]
            ctx = prepare_context(docs)
            prompts.append(builder.system_prompt() + "\n\n" +
                           builder.build_qa_prompt(queries[qi], ctx))
        t0 = _mark("select", t0)
        if args.dump_outputs:
            # references only — converted after the timed region
            last_out.update(query_embeddings=qv, dense_scores=d_scores,
                            sparse_scores=s_scores, fused_scores=f_scores)
        return queries, reranked, prompts

    ret_stream = torch.cuda.Stream() if on_gpu else None

    def retrieval_phase_streamed(step: int):
        # side stream: retrieval kernels fill gaps under decode; the phase
        # returns host data only (every GPU result is .cpu()'d inside).
        # CUDA device selection is THREAD-LOCAL: this runs on the executor
        # thread, which would otherwise default to device 0 on every rank
        # and break NCCL object collectives at N >= 2.
        if on_gpu:
            torch.cuda.set_device(device)
            with torch.cuda.stream(ret_stream):
                return retrieval_phase(step)
        return retrieval_phase(step)

    def generate_phase(payload) -> None:
        queries, reranked, prompts = payload
        t0 = time.perf_counter()
        answers = generator.generate(prompts, max_new_tokens=args.gen_tokens,
                                     temperature=0.3, stop_on_eos=False)
        stage_t["gen.prefill"] = stage_t.get("gen.prefill", 0.0) + \
            getattr(generator, "last_prefill_s", 0.0)
        stage_t["gen.decode"] = stage_t.get("gen.decode", 0.0) + \
            getattr(generator, "last_decode_s", 0.0)
        t0 = _mark("generate", t0)
        # optional verify
        if args.verify:
            vprompts = [builder.build_verify_prompt(
                query=queries[qi], context=prepare_context(reranked[qi]),
                answer=answers[qi]) for qi in range(args.batch)]
            generator.generate(vprompts, max_new_tokens=args.verify_tokens,
                               temperature=0.0, stop_on_eos=False)

    from concurrent.futures import ThreadPoolExecutor

    ret_ex = ThreadPoolExecutor(max_workers=1)

    # TP mode interleaves generation all-reduces with retrieval all-gathers
    # from two threads — collective-order hazard across ranks — so TP runs
    # the phases back-to-back.  DP keeps ALL collectives on the retrieval
    # thread in deterministic step order.
    pipelined = not tp_mode

    step_times: list[float] = []

    def run_pipelined(base: int, count: int, record: bool = False) -> None:
        if count <= 0:
            return
        if not pipelined:
            for i in range(count):
                ts = time.perf_counter()
                generate_phase(retrieval_phase_streamed(base + i))
                if record:
                    step_times.append(time.perf_counter() - ts)
            return
        fut = ret_ex.submit(retrieval_phase_streamed, base)
        for i in range(count):
            ts = time.perf_counter()
            payload = fut.result()
            if i + 1 < count:
                fut = ret_ex.submit(retrieval_phase_streamed, base + i + 1)
            generate_phase(payload)
            if record:
                step_times.append(time.perf_counter() - ts)

    # pre-capture the decode hipGraph with NO concurrent retrieval thread:
    # graph capture and foreign allocator traffic race otherwise
    generator.generate(["capture warm-up prompt"] * args.batch,
                       max_new_tokens=2, temperature=0.0, stop_on_eos=False)
    if on_gpu:
        torch.cuda.synchronize()

    # ---- warmup ----
    run_pipelined(0, args.warmup)
    D.barrier()
    if on_gpu:
        torch.cuda.synchronize()

    # ---- timed ----
    t0 = time.perf_counter()
    run_pipelined(1000, args.steps, record=True)
    D.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    # MAX over ranks (NCCL reduces GPU tensors; gloo reduces CPU tensors)
    e = torch.tensor([elapsed], device=device if on_gpu else "cpu")
    if D.is_distributed():
        import torch.distributed as tdist

        tdist.all_reduce(e, op=tdist.ReduceOp.MAX)
    elapsed = float(e.item())

    if args.dump_outputs and rank == 0 and last_out:
        dump_outputs(args.dump_outputs, last_out)

    total_requests = args.batch * args.steps * (1 if tp_mode else world)
    qps = total_requests / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if rank == 0:
        per_step = {k: round(v / (args.steps + args.warmup) * 1e3, 1)
                    for k, v in sorted(stage_t.items(), key=lambda kv: -kv[1])}
        print(f"[stage ms/step] {per_step}", file=sys.stderr)
        result = {
            "metric": "chat_qps",
            "value": round(qps, 3),
            "unit": "requests/s",
            "n_gpus": world if on_gpu else args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 1),
            "higher_is_better": True,
            "scaling": "strong" if tp_mode else "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "encoder": args.encoder,
                "reranker": args.reranker,
                "global_batch": args.batch * (1 if tp_mode else world),
                "seq_len": args.seq_len,
                "gen_tokens": args.gen_tokens,
                "docs_per_gpu": args.docs_per_gpu,
                "total_docs": args.docs_per_gpu * world,
                "parallelism": (f"tp{world}+index-shard{world}" if tp_mode
                                else f"dp{world}+index-shard{world}"),
                "pipeline": "embed>hybrid(dense+bm25+rrf)>rerank>select>generate"
                            + (">verify" if args.verify else "")
                            + ("|retrieval pipelined under prior step's "
                               "generation" if pipelined else ""),
                "p50_ms_per_request_batch": round(
                    sorted(step_times)[len(step_times) // 2] * 1e3, 1)
                    if step_times else round(ms_per_step, 1),
                "p95_ms_per_request_batch": round(
                    sorted(step_times)[min(len(step_times) - 1,
                                           int(len(step_times) * 0.95))] * 1e3,
                    1) if step_times else None,
                "prompt_tokens_per_req": round(
                    getattr(generator, "last_prompt_tokens", 0)
                    / max(args.batch, 1)),
                "tokenizer": type(generator.tokenizer).__name__,
                "init_s": round(init_s, 1),
                "device": "cuda" if on_gpu else "cpu-plumbing",
            },
        }
        print(json.dumps(result))


if __name__ == "__main__":
    main()
