"""Dense-index search microbenchmark: the fp8 index's fused scan + top-k
(ops.cosine_topk_fp8) beside the fp16 index's GEMM + topk (ops.cosine_topk)
over the same vectors, alternating the two inside every repeat, plus recall
of both indexes against exact fp32 search.
Run: python scripts/dense_index_probe.py            (every step, each in a
                                                     child with a time limit)
     python scripts/dense_index_probe.py time N     (N rows, dim 1024)
     python scripts/dense_index_probe.py recall     (N = 1M, 256 queries)
     python scripts/dense_index_probe.py --mask [N] (filtered search: the
         masked scan, ops.cosine_topk_masked, at B = 32, k = 10 over both
         index types beside the unfiltered search of each; HIP-event medians
         per call, the variants alternating inside every repeat; not part of
         the default steps)
TB/s counts each path's own index bytes: N * 2048 (fp16) or N * 1028 (fp8)."""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DIM = 1024
STEPS = [(["time", "1000000"], 240), (["time", "10000000"], 420),
         (["recall"], 300)]


def unit_rows(n, seed, dev):
    """Random unit vectors, generated in slices (10M x 1024 fp32 is 41 GB)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, DIM, device=dev)
    for i in range(0, n, 1 << 18):
        x = torch.randn(min(1 << 18, n - i), DIM, generator=g, device=dev)
        out[i:i + x.shape[0]] = x / x.norm(dim=1, keepdim=True)
    return out


def build(n, seed, dev):
    from sentio_amd.ops import torch_ref

    mat = torch.empty(n, DIM, dtype=torch.float16, device=dev)
    codes = torch.empty(n, DIM, dtype=torch.uint8, device=dev)
    scales = torch.empty(n, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    for i in range(0, n, 1 << 18):
        x = torch.randn(min(1 << 18, n - i), DIM, generator=g, device=dev)
        x = x / x.norm(dim=1, keepdim=True)
        mat[i:i + len(x)] = x.half()
        codes[i:i + len(x)], scales[i:i + len(x)] = torch_ref.index_quantize(x)
    return mat, codes, scales


def bench(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def time_probe(n, repeats=3):
    from sentio_amd import ops

    dev = "cuda:0"
    mat, codes, scales = build(n, 0, dev)
    iters = max(5, min(100, 200_000_000 // n))
    print(f"--- N={n} dim={DIM}: fp16 {n * 2 * DIM / 1e9:.2f} GB, "
          f"fp8 {n * (DIM + 4) / 1e9:.2f} GB, {iters} calls per timing, "
          f"scan blocks {ops.cosine_topk_fp8_plan(n)[0]}")
    for B in (1, 8, 32):
        q = unit_rows(B, 1, dev).half()
        for k in (10, 100):
            t16, t8 = [], []
            for _ in range(repeats):            # alternate the two paths
                t16.append(bench(lambda: ops.cosine_topk(q, mat, k), iters))
                t8.append(bench(
                    lambda: ops.cosine_topk_fp8(q, codes, scales, k), iters))
            for name, ts, nbytes in (("fp16 gemm+topk", t16, n * 2 * DIM),
                                     ("fp8 fused     ", t8, n * (DIM + 4))):
                print(f"B={B:2d} k={k:3d} {name}: "
                      + " ".join(f"{t * 1e3:8.3f}" for t in ts)
                      + f" ms  {nbytes / min(ts) / 1e12:.2f} TB/s")


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


def mask_probe(n, repeats=3, B=32, k=10, run=1024):
    """Allowed fractions 1, 0.1 and 0.01, as random bits and as contiguous
    runs of `run` rows (documents ingested tenant by tenant)."""
    from sentio_amd import ops

    dev = "cuda:0"
    mat, codes, scales = build(n, 0, dev)
    q = unit_rows(B, 1, dev).half()
    g = torch.Generator(device=dev).manual_seed(2)
    masks = {"all ones": torch.ones(n, dtype=torch.bool, device=dev)}
    for frac in (0.1, 0.01):
        masks[f"{frac:.0%} random"] = torch.rand(n, generator=g,
                                                 device=dev) < frac
        runs = torch.rand((n + run - 1) // run, generator=g, device=dev) < frac
        masks[f"{frac:.0%} runs of {run}"] = runs.repeat_interleave(run)[:n]
    allow = {name: ops.pack_row_mask(m[None]) for name, m in masks.items()}
    iters = max(20, min(200, 200_000_000 // n))
    print(f"--- masked scan, N={n} dim={DIM} B={B} k={k}: median of {iters} "
          f"event-timed calls, {repeats} repeats, scan blocks "
          f"{ops.cosine_topk_fp8_plan(n)[0]}")
    variants = [("fp16 gemm+topk, unfiltered",
                 lambda: ops.cosine_topk(q, mat, k)),
                ("fp8 fused scan, unfiltered",
                 lambda: ops.cosine_topk_fp8(q, codes, scales, k))]
    for name, a in allow.items():
        variants.append((f"fp16 masked, {name}", lambda a=a:
                         ops.cosine_topk_masked(q, mat, None, k, a)))
        variants.append((f"fp8 masked, {name}", lambda a=a:
                         ops.cosine_topk_masked(q, codes, scales, k, a)))
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(event_median(fn, iters))
    for name, m in masks.items():
        print(f"mask {name}: {int(m.sum())} rows allowed")
    for name, ts in times.items():
        print(f"{name:34s} " + " ".join(f"{t * 1e3:8.3f}" for t in ts) + " ms")
    # the timed calls must agree with the unfiltered search where they can
    r8 = ops.cosine_topk_masked(q, codes, scales, k, allow["all ones"])[1]
    print("fp8 all-ones rows == unfiltered rows:",
          torch.equal(r8, ops.cosine_topk_fp8(q, codes, scales, k)[1]))


def recall_probe(n=1_000_000, nq=256):
    from sentio_amd import ops

    dev = "cuda:0"
    x = unit_rows(n, 0, dev)
    mat, codes, scales = build(n, 0, dev)
    q = unit_rows(nq, 1, dev)
    exact = torch.topk(q @ x.T, 100, dim=1).indices
    for name, fn in (
            ("fp16", lambda qq, k: ops.cosine_topk(qq, mat, k)[1]),
            ("fp8 ", lambda qq, k: ops.cosine_topk_fp8(qq, codes, scales,
                                                       k)[1])):
        for k in (10, 100):
            rows = torch.cat([fn(q[i:i + 32].half(), k)
                              for i in range(0, nq, 32)])
            hit = sum(len(set(a) & set(b)) for a, b in
                      zip(rows.tolist(), exact[:, :k].tolist()))
            print(f"{name} index recall@{k} vs fp32, N={n}, {nq} queries: "
                  f"{hit / (nq * k):.4f}")


if __name__ == "__main__":
    if len(sys.argv) == 1:
        for args, limit in STEPS:      # a fresh child and a limit per step
            rc = subprocess.run([sys.executable, __file__, *args],
                                timeout=limit).returncode
            if rc:
                sys.exit(f"step {args} exited with {rc}: stopping")
        sys.exit(0)
    if not torch.cuda.is_available():
        sys.exit(f"{__file__}: needs a GPU (MI355X)")
    if sys.argv[1] == "--mask":
        mask_probe(int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000)
    elif sys.argv[1] == "time":
        time_probe(int(sys.argv[2]))
    elif sys.argv[1] == "recall":
        recall_probe()
    else:
        sys.exit(f"unknown step {sys.argv[1]!r}")
