#!/usr/bin/env python
"""Isolated probe of the prefill attention kernel (ops.attention and
ops.attention_cache) at the shapes the pipeline runs it at.

  generator suffix   B 32,  S 384, q_off 832, H 32, Hkv 8, D 128, cache mode
  verifier suffix    B 32,  S and q_off from --verifier-shape, same heads
  causal prefill     B 8,   S 1024, q_off 0,  H 32, Hkv 8, D 128
  encoder            B 32,  S 32,   H 16, D 64, non-causal with lengths
  reranker           B 320, S 256,  H 12, D 64, non-causal with lengths

Every call of a timed sequence reads a DIFFERENT copy of q, K and V, and the
copies together exceed the 256 MiB Infinity Cache at least twice over.  The
sequence is captured into one hipGraph and replayed (best of 5): GPU time
with launches back to back, not Python dispatch.

TFLOP/s counts 4 * D FLOPs per (query, allowed key, head) pair: causal pairs
exactly, keys at or past a row's length not at all.

Usage: python scripts/flash_prefill_probe.py [--verifier-shape S,Q_OFF]
                                             [--out FILE.json]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sentio_amd import ops  # noqa: E402

ICACHE = 256 << 20


def shapes(ver_s: int, ver_off: int):
    # name, B, S, q_off, H, Hkv, D, mode
    return [
        ("generator suffix", 32, 384, 832, 32, 8, 128, "cache"),
        ("verifier suffix", 32, ver_s, ver_off, 32, 8, 128, "cache"),
        ("causal prefill", 8, 1024, 0, 32, 8, 128, "causal"),
        ("encoder", 32, 32, 0, 16, 16, 64, "lens"),
        ("reranker", 320, 256, 0, 12, 12, 64, "lens"),
    ]


def time_graph(fn, copies: int, reps: int = 5) -> float:
    """Microseconds per call of fn(i), i over the input copies, replayed
    from one captured graph (best of reps replays)."""
    for i in range(min(copies, 2)):
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


def pairs(S: int, q_off: int, lens: list[int], causal: bool) -> int:
    """(query, allowed key) pairs of one head over the batch."""
    n = 0
    for kv in lens:
        if causal:
            n += sum(min(kv, q_off + i + 1) for i in range(S))
        else:
            n += S * kv
    return n


def probe(name, B, S, q_off, H, Hkv, D, mode, dev) -> dict:
    bf = torch.bfloat16
    cache = mode == "cache"
    n_kv = q_off + S
    per_copy = (B * S * H * D * 2 + 2 * B * n_kv * Hkv * D) * 2
    copies = max(2, -(-(2 * ICACHE + 1) // per_copy))
    if mode == "lens":      # ragged: full down to about half, as padded text
        lens = [S - (i * 7) % (S // 2) for i in range(B)]
    else:
        lens = [n_kv] * B
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    qs = [torch.randn(B, S, H, D, device=dev, dtype=bf) for _ in range(copies)]
    kv_shape = (B, Hkv, n_kv, D) if cache else (B, S, Hkv, D)
    ks = [torch.randn(kv_shape, device=dev, dtype=bf) for _ in range(copies)]
    vs = [torch.randn(kv_shape, device=dev, dtype=bf) for _ in range(copies)]

    def run(i):
        if cache:
            return ops.attention_cache(qs[i], ks[i], vs[i], lens_t, q_off)
        return ops.attention(qs[i], ks[i], vs[i], causal=mode == "causal",
                             kv_lens=lens_t)

    us = time_graph(run, copies)
    flops = 4 * D * H * pairs(S, q_off, lens, mode != "lens")
    row = {"shape": name, "B": B, "S": S, "q_off": q_off, "H": H, "Hkv": Hkv,
           "D": D, "mode": mode, "copies": copies, "flops": flops, "us": us,
           "tflops": flops / us / 1e6}
    del qs, ks, vs
    torch.cuda.empty_cache()
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--verifier-shape", default="512,832",
                    help="S,q_off of the verifier's suffix forward")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flash_prefill_probe needs a GPU")
    assert ops.hip_available(), "HIP extension must be built"
    ver_s, ver_off = (int(x) for x in args.verifier_shape.split(","))
    rows = []
    for shape in shapes(ver_s, ver_off):
        r = probe(*shape, "cuda:0")
        rows.append(r)
        print(f"{r['shape']:<17s} B={r['B']} S={r['S']} q_off={r['q_off']} "
              f"H={r['H']}/{r['Hkv']} D={r['D']} {r['mode']} "
              f"({r['copies']} copies): {r['us']:.1f} us, "
              f"{r['tflops']:.0f} TFLOP/s", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
