"""Isolated time of the constrained sampler against ops.sample_filtered.

B = 32 rows of V = 128256 logits, the VERDICT_GRAMMAR tables over the
engine tokenizer (Vt = 4355).  Every row sits inside a JSON string, where
most of the vocabulary is allowed; `left` is either far above every dist
(the dist sweep is skipped) or exactly dist[state] (it binds).  The two
kernels alternate inside each round; a round's figure is the median of
its per-launch HIP-event times, and the spread over rounds is printed.

    python scripts/constrained_probe.py [--rounds 5] [--iters 200]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--vocab", type=int, default=128256)
    args = ap.parse_args()

    from sentio_amd import ops
    from sentio_amd.engines.bpe import get_tokenizer
    from sentio_amd.engines.grammar import VERDICT_GRAMMAR, Grammar

    dev = "cuda:0"
    tok = get_tokenizer()
    t0 = time.perf_counter()
    g = Grammar.from_regex(VERDICT_GRAMMAR.pattern)
    compile_s = time.perf_counter() - t0
    tb = g.token_tables(tok)
    tables = ops.GrammarTables.from_numpy(tb.next, tb.mask, tb.dist,
                                          device=dev)
    inside = g.walk(0, b'{"verdict": "pass", "citations_ok":true, '
                       b'"notes": ["a')
    B, V = args.batch, args.vocab
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(B, V, generator=gen) * 3.0).to(dev)
    seed = torch.arange(B, dtype=torch.int64, device=dev) + 17
    step = torch.zeros(B, dtype=torch.int32, device=dev)
    state0 = torch.full((B,), inside, dtype=torch.int32, device=dev)
    state = state0.clone()
    left = torch.zeros(B, dtype=torch.int32, device=dev)

    def timed(fn) -> float:
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3          # us

    out = {"n_states": tb.n_states, "vocab": tb.vocab,
           "table_bytes": tables.nbytes, "compile_s": round(compile_s, 4),
           "table_build_s": round(tb.build_s, 4), "cases": {}}
    for name, T, k, p in (("T0", 0.0, 0, 1.0), ("T0.7_p0.9", 0.7, 0, 0.9)):
        t = torch.full((B,), T, device=dev)
        kk = torch.full((B,), k, dtype=torch.int32, device=dev)
        pp = torch.full((B,), p, device=dev)
        for budget, lf in (("free", 200), ("binding", int(tb.dist[inside]))):
            def constrained():
                ops.sample_constrained(x, t, kk, pp, seed, step, state, left,
                                       tables)

            def filtered():
                ops.sample_filtered(x, t, kk, pp, seed, step)

            rounds = {"constrained": [], "filtered": []}
            for _ in range(args.rounds + 1):          # round 0 warms up
                per = {"constrained": [], "filtered": []}
                for _ in range(args.iters):
                    state.copy_(state0)
                    left.fill_(lf)
                    per["constrained"].append(timed(constrained))
                    per["filtered"].append(timed(filtered))
                for key in per:
                    rounds[key].append(statistics.median(per[key]))
            out["cases"][f"{name}/{budget}"] = {
                key: [round(min(v[1:]), 2), round(max(v[1:]), 2)]
                for key, v in rounds.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
