#!/usr/bin/env python
"""Isolated probe of the decode projections onto the model dimension.

For wo (K = dim) and down (K = ffn_dim) of llama3-8b, llama3-70b, qwen2-7b
and llama3-1b at B = 16, 24, 32 it times, per call,

  lt:      ops.lt_linear + ops.rmsnorm_residual              (library route)
  splitk:  ops.linear_splitk + ops.rmsnorm_residual_partials (hand route)

the hand route once per legal S (SENTIO_GEMM_SPLITK) and once with the
planner's own S, and prints microseconds and the weight stream in TB/s.

Every call of a timed sequence reads a DIFFERENT copy of the weight, and the
copies together exceed the 256 MiB Infinity Cache several times over (at
least 16 copies, at least 1 GiB), so each call streams its weight from HBM
as a decode step does.  scripts/gemm_probe.py re-reads one weight in a tight
loop; its numbers above ~5.5 TB/s are cache-inflated (profiles/README.md)
and must not be compared with these.  The sequence is captured into one
hipGraph and replayed, so the figure is GPU time with launches back to back
as in the captured decode step, not Python dispatch.

Usage: python scripts/decode_gemm_probe.py [--models llama3-8b,...]
           [--batches 16,24,32] [--splits 1,2,4,7,8,14,16] [--out FILE.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sentio_amd import ops  # noqa: E402
from sentio_amd.engines.configs import MODEL_CONFIGS  # noqa: E402

MODELS = ["llama3-8b", "llama3-70b", "qwen2-7b", "llama3-1b"]


def time_graph(fn, copies: int, reps: int = 5) -> float:
    """Microseconds per call of fn(i), i over the weight copies, replayed
    from one captured graph (best of reps replays)."""
    for i in range(min(copies, 2)):      # warm-up: autotune, allocator
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(copies):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        g.replay()
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1) * 1e3 / copies)
    return best


def probe_shape(model: str, proj: str, B: int, N: int, K: int,
                splits: list[int], dev: str) -> dict:
    wbytes = N * K * 2
    copies = max(16, -(-(1 << 30) // wbytes))
    ws = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.05
          for _ in range(copies)]
    x = torch.randn(B, K, device=dev, dtype=torch.bfloat16)
    res = torch.randn(B, N, device=dev, dtype=torch.bfloat16)
    wn = torch.randn(N, device=dev, dtype=torch.bfloat16)

    def lt(i):
        return ops.rmsnorm_residual(ops.lt_linear(x, ws[i]), res, wn, 1e-5)

    def sk(i):
        return ops.rmsnorm_residual_partials(ops.linear_splitk(x, ws[i]),
                                             res, wn, 1e-5)

    def gemm_lt(i):
        return ops.lt_linear(x, ws[i])

    def gemm_sk(i):
        return ops.linear_splitk(x, ws[i])

    os.environ.pop("SENTIO_GEMM_SPLITK", None)
    row = {"model": model, "proj": proj, "B": B, "N": N, "K": K,
           "copies": copies, "lt_pair_us": time_graph(lt, copies),
           "lt_gemm_us": time_graph(gemm_lt, copies), "splitk": []}
    plan_s = ops.decode_gemm_plan(B, N, K)[0]
    row["plan_S"] = plan_s
    for s in splits:
        if K % (32 * s) or s * B * N * 4 > 8 << 20:
            continue
        os.environ["SENTIO_GEMM_SPLITK"] = str(s)
        row["splitk"].append({"S": s, "pair_us": time_graph(sk, copies),
                              "gemm_us": time_graph(gemm_sk, copies)})
    os.environ.pop("SENTIO_GEMM_SPLITK", None)
    del ws
    torch.cuda.empty_cache()
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--batches", default="16,24,32")
    ap.add_argument("--splits", default="1,2,4,7,8,14,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    splits = [int(s) for s in args.splits.split(",")]
    rows = []
    for model in args.models.split(","):
        cfg = MODEL_CONFIGS[model]
        for proj, K in (("wo", cfg.dim), ("down", cfg.ffn_dim)):
            for B in (int(b) for b in args.batches.split(",")):
                r = probe_shape(model, proj, B, cfg.dim, K, splits, dev)
                rows.append(r)
                tb = lambda us: r["N"] * r["K"] * 2 / us / 1e6  # noqa: E731
                print(f"{model} {proj} B={B} N={r['N']} K={K} "
                      f"({r['copies']} copies): lt pair "
                      f"{r['lt_pair_us']:.1f} us (gemm {r['lt_gemm_us']:.1f}"
                      f" us, {tb(r['lt_gemm_us']):.2f} TB/s)", flush=True)
                for e in r["splitk"]:
                    mark = " <- plan" if e["S"] == r["plan_S"] else ""
                    print(f"    S={e['S']:<3d} pair {e['pair_us']:.1f} us "
                          f"(gemm {e['gemm_us']:.1f} us, "
                          f"{tb(e['gemm_us']):.2f} TB/s){mark}", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
