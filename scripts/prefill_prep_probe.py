#!/usr/bin/env python
"""Isolated probe of the prefill head prep between the QKV GEMM and attention.

For three shapes of the flagship run it times, per layer call,

  legacy:  three slice copies, two ops.rope_apply and (cache mode) the two
           indexed cache writes, as Transformer._attn runs them under
           SENTIO_PREFILL_PREP=legacy
  fused:   ops.prefill_qkv_prep

and prints microseconds and the GB/s of the bytes the fused op has to move
(qkv read once, every value written once; the rope tables are not counted).

  llama3-8b suffix   B 32,  S 384, pos0 832, cache mode (Smax 1216)
  encoder            B 32,  S 32,  plain
  reranker           B 320, S 256, plain

Every call of a timed sequence reads a DIFFERENT copy of qkv (and writes a
different cache), and the copies together exceed the 256 MiB Infinity Cache
at least twice over, so the inputs come from HBM as they do behind a GEMM
that has just streamed its weights.  The sequence is captured into one
hipGraph and replayed: GPU time with launches back to back, not Python
dispatch.

Usage: python scripts/prefill_prep_probe.py [--out FILE.json]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sentio_amd import ops  # noqa: E402
from sentio_amd.engines.configs import MODEL_CONFIGS  # noqa: E402

SHAPES = [
    # name, model, B, S, pos0, cache mode
    ("llama3-8b suffix", "llama3-8b", 32, 384, 832, True),
    ("encoder", "sentio-encoder-base", 32, 32, 0, False),
    ("reranker", "sentio-reranker-base", 320, 256, 0, False),
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


def probe(name: str, model: str, B: int, S: int, pos0: int, cached: bool,
          dev: str) -> dict:
    cfg = MODEL_CONFIGS[model]
    H, Hkv, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    W = (H + 2 * Hkv) * D
    nbytes = B * S * W * 2
    copies = max(2, -(-(512 << 20) // nbytes))
    Smax = pos0 + S
    cos, sin = ops.torch_ref.rope_tables(cfg.max_seq, D, cfg.rope_base, dev)
    qkvs = [torch.randn(B, S, W, device=dev, dtype=torch.bfloat16)
            for _ in range(copies)]
    caches = [(torch.zeros(B, Hkv, Smax, D, device=dev, dtype=torch.bfloat16),
               torch.zeros(B, Hkv, Smax, D, device=dev, dtype=torch.bfloat16))
              for _ in range(copies)] if cached else None
    pos = torch.arange(pos0, pos0 + S, device=dev).unsqueeze(0).expand(B, S)
    q_end, k_end = H * D, (H + Hkv) * D

    def legacy(i):
        qkv = qkvs[i]
        q = qkv[..., :q_end].reshape(B, S, H, D)
        k = qkv[..., q_end:k_end].reshape(B, S, Hkv, D)
        v = qkv[..., k_end:].reshape(B, S, Hkv, D)
        q = ops.rope_apply(q, cos, sin, pos)
        k = ops.rope_apply(k, cos, sin, pos)
        if cached:
            kc, vc = caches[i]
            idx = pos.long()
            bidx = torch.arange(B, device=dev).unsqueeze(1).expand(B, S)
            kc[bidx.reshape(-1), :, idx.reshape(-1)] = \
                k.reshape(B * S, Hkv, D).to(kc.dtype)
            vc[bidx.reshape(-1), :, idx.reshape(-1)] = \
                v.reshape(B * S, Hkv, D).to(vc.dtype)
        return q, k, v

    def fused(i):
        if cached:
            return ops.prefill_qkv_prep(qkvs[i], cos, sin, pos0, H, Hkv,
                                        *caches[i])
        return ops.prefill_qkv_prep(qkvs[i], cos, sin, pos0, H, Hkv)

    row = {"shape": name, "B": B, "S": S, "pos0": pos0, "cache": cached,
           "H": H, "Hkv": Hkv, "D": D, "copies": copies,
           "bytes_moved": 2 * nbytes,
           "legacy_us": time_graph(legacy, copies),
           "fused_us": time_graph(fused, copies)}
    del qkvs, caches
    torch.cuda.empty_cache()
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_prep_probe needs a GPU")
    rows = []
    for shape in SHAPES:
        r = probe(*shape, "cuda:0")
        rows.append(r)
        gbs = lambda us: r["bytes_moved"] / us / 1e3  # noqa: E731
        print(f"{r['shape']:<17s} B={r['B']} S={r['S']} pos0={r['pos0']} "
              f"{'cache' if r['cache'] else 'plain'} ({r['copies']} copies, "
              f"{r['bytes_moved'] / 1e6:.1f} MB moved): legacy "
              f"{r['legacy_us']:.1f} us ({gbs(r['legacy_us']):.0f} GB/s), "
              f"fused {r['fused_us']:.1f} us ({gbs(r['fused_us']):.0f} GB/s)",
              flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
