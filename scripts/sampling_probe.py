"""Probe the sampling kernels at serving shapes on MI355X.

Times, at B=64 and V in {128256, 152064} (fp32 logits resident on device):
  (a)  ops.sample_token            -- the existing scalar-temperature kernel
  (b)  ops.sample_filtered k=0 p=1 -- per-row kernel, filters off
  (c)  ops.sample_filtered k=50 p=0.9
  (d1) eager torch top-k/top-p     -- sort + cumsum + mask + Gumbel-argmax
  (d2) eager torch sample_rows     -- the continuous batcher's default code
  (e)  ops.sample_slots            -- the slot loop's sampler (slot sampling
       on) at S = 64 slots with 64, 8 and 1 of them active, for (k=0, p=1),
       (k=50, p=0.9) and (k=0, p=0.9); same logits, identity addressing,
       step counters advancing on the device as they do in the loop
on two input families: "peaked" (LLM-like: 200 geometric ranks over a flat
-30 tail) and "flat" (3*randn, a wide nucleus).

HIP-event timing: every variant is warmed up, then REPS windows of ITERS
back-to-back calls are timed with device events, alternating the variants
inside each repetition; the median window per call is reported with the
min..max spread.  Run on the GPU:  python scripts/sampling_probe.py
[--out FILE.md]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

B = 64
VOCABS = (128256, 152064)
ITERS = 20
REPS = 15


def make_logits(kind: str, V: int, dev: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(V)
    if kind == "flat":
        return (3.0 * torch.randn(B, V, generator=g)).to(dev)
    rows = []
    for _ in range(B):
        r = torch.arange(V, dtype=torch.float32)
        base = torch.where(r < 200, -0.05 * r, torch.full_like(r, -30.0))
        base = base + 1e-3 * torch.randn(V, generator=g)
        rows.append(base[torch.randperm(V, generator=g)])
    return torch.stack(rows).to(dev)


def eager_topk_topp(logits, t, k, p, rng):
    """What the op replaces when written in eager torch."""
    V = logits.shape[1]
    z = logits / t[:, None]
    sz, idx = torch.sort(z, dim=-1, descending=True)
    probs = torch.softmax(sz, dim=-1)
    rank = torch.arange(V, device=logits.device)[None, :]
    probs = torch.where(rank < k[:, None], probs, torch.zeros_like(probs))
    probs = probs / probs.sum(-1, keepdim=True)
    cs = torch.cumsum(probs, dim=-1)
    keep = ((cs - probs) < p[:, None]) & (rank < k[:, None])
    u = torch.rand(z.shape, device=z.device, generator=rng)
    g = -torch.log(-torch.log(u.clamp_min(1e-20)).clamp_min(1e-20))
    sc = torch.where(keep, sz + g, torch.full_like(sz, float("-inf")))
    return idx.gather(1, sc.argmax(-1, keepdim=True))[:, 0]


def eager_sample_rows(logits, temps, rng):
    """GeneratorEngine.sample_rows' default (eager) code."""
    t = temps.view(-1, 1)
    u = torch.rand(logits.shape, device=logits.device, generator=rng)
    g = -torch.log(-torch.log(u.clamp_min(1e-20)).clamp_min(1e-20))
    scores = torch.where(t > 0, logits / t.clamp_min(1e-6) + g, logits)
    return scores.argmax(-1)


def time_variants(variants: dict) -> dict:
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in variants}
    for _ in range(REPS):
        for name, fn in variants.items():       # alternate the variants
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) * 1e3 / ITERS)  # us
    return {n: (statistics.median(s), min(s), max(s))
            for n, s in samples.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write a markdown table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the GPU"
    from sentio_amd import ops

    assert ops.hip_available()
    dev = "cuda:0"
    rng = torch.Generator(device=dev)
    rng.manual_seed(909)
    lines = ["| input | V | variant | median us | min..max us |",
             "|---|---|---|---|---|"]
    for V in VOCABS:
        for kind in ("peaked", "flat"):
            x = make_logits(kind, V, dev)
            t = torch.full((B,), 0.7, device=dev)
            k0 = torch.zeros(B, dtype=torch.int32, device=dev)
            p1 = torch.ones(B, device=dev)
            k50 = torch.full((B,), 50, dtype=torch.int32, device=dev)
            p9 = torch.full((B,), 0.9, device=dev)
            kv = torch.full((B,), V, dtype=torch.int64, device=dev)
            seed = torch.arange(B, dtype=torch.int64, device=dev)
            step = torch.zeros(B, dtype=torch.int32, device=dev)
            slot_variants = {}
            tok = torch.zeros(B, dtype=torch.int64, device=dev)
            for n_act in (64, 8, 1):
                act = torch.zeros(B, dtype=torch.uint8, device=dev)
                act[:n_act] = 1
                for tag, kk, pp in (("k=0 p=1", k0, p1),
                                    ("k=50 p=0.9", k50, p9),
                                    ("k=0 p=0.9", k0, p9)):
                    st = torch.zeros(B, dtype=torch.int32, device=dev)
                    slot_variants[f"(e) sample_slots {tag} active={n_act}"] = (
                        lambda kk=kk, pp=pp, st=st, act=act: ops.sample_slots(
                            x, None, t, kk, pp, seed, st, act, tok))
            res = time_variants({
                "(a) sample_token": lambda: ops.sample_token(x, 0.7, 1),
                "(b) sample_filtered k=0 p=1": lambda: ops.sample_filtered(
                    x, t, k0, p1, seed, step),
                "(c) sample_filtered k=50 p=0.9": lambda: ops.sample_filtered(
                    x, t, k50, p9, seed, step),
                "(c') sample_filtered k=0 p=0.9": lambda: ops.sample_filtered(
                    x, t, k0, p9, seed, step),
                "(d1) eager sort+cumsum k=50 p=0.9": lambda: eager_topk_topp(
                    x, t, k50.long(), p9, rng),
                "(d1') eager sort+cumsum k=V p=0.9": lambda: eager_topk_topp(
                    x, t, kv, p9, rng),
                "(d2) eager sample_rows": lambda: eager_sample_rows(
                    x, t, rng),
                **slot_variants,
            })
            for name, (med, lo, hi) in res.items():
                lines.append(f"| {kind} | {V} | {name} | {med:.1f} | "
                             f"{lo:.1f}..{hi:.1f} |")
            a = res["(a) sample_token"][0]
            c = res["(c) sample_filtered k=50 p=0.9"][0]
            lines.append(f"| {kind} | {V} | (c)/(a) ratio | {c / a:.2f} | |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
