"""MMR selection microbenchmark: ops.mmr_select (mmr_select_kernel) beside
the same selection composed from torch ops on the device (index_select, one
batched matmul, a k-step loop of argmax and maximum, no host sync), on the
same inputs, for both index types; then the share of a filtered search's
time that the diversification adds.
Run: python scripts/mmr_probe.py [N]        (N index rows, default 1M)
C = 128 candidates, k = 10, dim 1024, B in {1, 32}.  Each figure is the
median HIP-event time of ITERS calls; the variants alternate inside every
repeat and every repeat is printed."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DIM, C, K, LAM = 1024, 128, 10, 0.5
ITERS, REPEATS = 200, 3


def event_median(fn, iters=ITERS):
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


def torch_mmr(q, rows, scales, cand, k, lam):
    """The selection in torch ops: what a caller without the kernel writes.
    Candidates are all valid here, so there is no padding to handle."""
    B, c = cand.shape
    x = rows.index_select(0, cand.reshape(-1))
    if scales is not None:                  # dequantise: codes reach 448
        x = (x.view(torch.float8_e4m3fn).float() * scales.index_select(
            0, cand.reshape(-1)).unsqueeze(1)).to(torch.float16)
    x = x.view(B, c, -1)
    sim = torch.bmm(x, torch.cat([x, q.unsqueeze(1)], 1).transpose(1, 2)).float()
    rel, S = sim[:, :, c], sim[:, :, :c]
    red = torch.zeros_like(rel)
    closed = torch.zeros_like(rel, dtype=torch.bool)
    picks = []
    for _ in range(k):
        obj = (lam * rel - (1.0 - lam) * red).masked_fill(closed, float("-inf"))
        p = obj.argmax(dim=1, keepdim=True)
        picks.append(p)
        closed = closed.scatter(1, p, True)
        red = torch.maximum(red, S.gather(2, p.unsqueeze(1).expand(B, c, 1))
                            .squeeze(2))
    p = torch.cat(picks, 1)
    return rel.gather(1, p), cand.gather(1, p)


def main(n):
    from sentio_amd import ops
    from sentio_amd.ops import torch_ref

    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    # clustered rows, so that the redundancy term moves picks
    centres = torch.randn(n // 64 + 1, DIM, generator=g, device=dev)
    mat = torch.empty(n, DIM, dtype=torch.float16, device=dev)
    codes = torch.empty(n, DIM, dtype=torch.uint8, device=dev)
    scales = torch.empty(n, device=dev)
    for i in range(0, n, 1 << 18):
        m = min(1 << 18, n - i)
        x = centres[torch.arange(i, i + m, device=dev) // 64] \
            + 0.3 * torch.randn(m, DIM, generator=g, device=dev)
        x = x / x.norm(dim=1, keepdim=True)
        mat[i:i + m] = x.half()
        codes[i:i + m], scales[i:i + m] = torch_ref.index_quantize(x)
    allow = ops.pack_row_mask(
        (torch.rand(n, generator=g, device=dev) < 0.1)[None])
    print(f"--- mmr_select, N={n} dim={DIM} C={C} k={K} lam={LAM}: median of "
          f"{ITERS} event-timed calls, {REPEATS} repeats")
    for B in (1, 32):
        q = centres[:B] + 0.3 * torch.randn(B, DIM, generator=g, device=dev)
        q = (q / q.norm(dim=1, keepdim=True)).half()
        for name, rows, sc in (("fp16", mat, None), ("fp8 ", codes, scales)):
            cand = ops.cosine_topk_masked(q, rows, sc, C, allow)[1]
            variants = [
                ("hip kernel", lambda: ops.mmr_select(q, rows, sc, cand, K, LAM)),
                ("torch ops ", lambda: torch_mmr(q, rows, sc, cand, K, LAM)),
                ("masked search, k=128       ",
                 lambda: ops.cosine_topk_masked(q, rows, sc, C, allow)),
                ("masked search + hip kernel ", lambda: ops.mmr_select(
                    q, rows, sc,
                    ops.cosine_topk_masked(q, rows, sc, C, allow)[1], K, LAM)),
                ("masked search, k=10 (plain)",
                 lambda: ops.cosine_topk_masked(q, rows, sc, K, allow)),
                # DenseIndex's default fetch_k for top_k = 10
                ("masked search, k=40        ",
                 lambda: ops.cosine_topk_masked(q, rows, sc, 40, allow)),
                ("masked k=40 + hip kernel   ", lambda: ops.mmr_select(
                    q, rows, sc,
                    ops.cosine_topk_masked(q, rows, sc, 40, allow)[1], K, LAM)),
            ]
            times = {v: [] for v, _ in variants}
            for _ in range(REPEATS):              # alternate the variants
                for v, fn in variants:
                    times[v].append(event_median(fn))
            for v, ts in times.items():
                print(f"B={B:2d} {name} {v}: "
                      + " ".join(f"{t * 1e6:8.1f}" for t in ts) + " us")
            a = ops.mmr_select(q, rows, sc, cand, K, LAM)[1]
            b = torch_mmr(q, rows, sc, cand, K, LAM)[1]
            print(f"B={B:2d} {name} picks equal to the torch composition's: "
                  f"{int((a == b).sum())} of {a.numel()}")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit(f"{__file__}: needs a GPU (MI355X)")
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000)
