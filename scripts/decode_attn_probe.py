"""Isolated decode-attention microbenchmark (llama3-8b decode shape).
Prints achieved µs + effective KV TB/s per (splits, waves) setting for
ops.decode_attention, for the two-op chain decode_qkv_prep + decode_attention
and for the one-launch ops.decode_attention_fused.
Run: python scripts/decode_attn_probe.py [--repeats N] [--main-only]
     python scripts/decode_attn_probe.py --kv fp8 [--repeats N]
--kv fp8 times ops.decode_attention_fused_fp8 (uint8 e4m3fn caches) beside
the bf16 ops.decode_attention_fused on the same three shapes, alternating
the two inside every repeat."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sentio_amd import ops

def bench(fn, iters=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters

def setenv(name, val):
    if val: os.environ[name] = str(val)
    else: os.environ.pop(name, None)

def main(repeats=1):
    if not torch.cuda.is_available():
        print(f"{__file__}: needs a GPU (MI355X) — skipping")
        return

    dev = "cuda:0"
    has_fused = hasattr(ops, "decode_attention_fused")
    for B, slen in [(16, 1600), (32, 1600), (32, 512)]:
        H, Hkv, Smax, D = 32, 8, 2120, 128
        torch.manual_seed(0)
        q = torch.randn(B, H, D, dtype=torch.bfloat16, device=dev)
        qkv = torch.randn(B, (H + 2 * Hkv) * D, dtype=torch.bfloat16,
                          device=dev)
        kc = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev)
        vc = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev)
        cos, sin = ops.torch_ref.rope_tables(Smax, D, device=dev)
        lens = torch.full((B,), slen, dtype=torch.int32, device=dev)
        pos = lens - 1            # new token at slen-1: slen keys attended
        kv_bytes = 2 * B * Hkv * slen * D * 2
        print(f"--- B={B} slen={slen} (KV {kv_bytes/1e6:.0f} MB)")

        def attn():
            ops.decode_attention(q, kc, vc, lens)

        def two_op():
            ops.decode_attention(
                ops.decode_qkv_prep(qkv, kc, vc, cos, sin, pos), kc, vc, lens)

        def fused():
            ops.decode_attention_fused(qkv, kc, vc, cos, sin, pos)

        paths = [("attn", attn), ("prep+attn", two_op)]
        if has_fused:
            paths.append(("fused", fused))
        for waves in (0, 4, 8) if has_fused else (0,):
            setenv("SENTIO_DECODE_WAVES", waves)
            for splits in (0, 1, 2, 4, 8):
                setenv("SENTIO_DECODE_SPLITS", splits)
                for name, fn in paths:
                    ts = [bench(fn) for _ in range(repeats)]
                    print(f"waves={waves or 'auto'} splits={splits or 'auto'} "
                          f"{name:9s}: "
                          + " ".join(f"{t*1e6:7.1f}" for t in ts)
                          + f" us  {kv_bytes/min(ts)/1e12:.2f} TB/s")
        setenv("SENTIO_DECODE_WAVES", 0)
        setenv("SENTIO_DECODE_SPLITS", 0)




def kv_fp8_probe(repeats=3):
    """FP8-cache fused decode kernel against the bf16 fused kernel: same
    shapes, same launch plan; effective TB/s counts each kernel's own KV
    bytes."""
    if not torch.cuda.is_available():
        print(f"{__file__}: needs a GPU (MI355X) — skipping")
        return
    dev = "cuda:0"
    for B, slen in [(16, 1600), (32, 1600), (32, 512)]:
        H, Hkv, Smax, D = 32, 8, 2120, 128
        torch.manual_seed(0)
        qkv = torch.randn(B, (H + 2 * Hkv) * D, dtype=torch.bfloat16,
                          device=dev)
        kc = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev)
        vc = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev)
        ones = torch.ones(Hkv, device=dev)
        kc8 = torch.zeros(B, Hkv, Smax, D, dtype=torch.uint8, device=dev)
        vc8 = torch.zeros_like(kc8)
        ops.kv_store_fp8(kc, vc, kc8, vc8, list(range(B)), Smax, ones, ones)
        cos, sin = ops.torch_ref.rope_tables(Smax, D, device=dev)
        pos = torch.full((B,), slen - 1, dtype=torch.int32, device=dev)
        elems = 2 * B * Hkv * slen * D
        print(f"--- B={B} slen={slen} (KV bf16 {2*elems/1e6:.0f} MB, "
              f"fp8 {elems/1e6:.0f} MB)")

        def bf16():
            ops.decode_attention_fused(qkv, kc, vc, cos, sin, pos)

        def fp8():
            ops.decode_attention_fused_fp8(qkv, kc8, vc8, cos, sin, pos,
                                           ones, ones, ones, ones)

        for waves, splits in ((0, 0), (4, 0), (8, 1), (4, 2), (4, 4)):
            setenv("SENTIO_DECODE_WAVES", waves)
            setenv("SENTIO_DECODE_SPLITS", splits)
            tb, t8 = [], []
            for _ in range(repeats):        # alternate the two versions
                tb.append(bench(bf16))
                t8.append(bench(fp8))
            for name, ts, nbytes in (("fused bf16", tb, 2 * elems),
                                     ("fused fp8 ", t8, elems)):
                print(f"waves={waves or 'auto'} splits={splits or 'auto'} "
                      f"{name}: "
                      + " ".join(f"{t*1e6:7.1f}" for t in ts)
                      + f" us  {nbytes/min(ts)/1e12:.2f} TB/s")
        setenv("SENTIO_DECODE_WAVES", 0)
        setenv("SENTIO_DECODE_SPLITS", 0)


def bmm_probe():
    """Compare the hand decode-attention kernel against a batched-GEMM
    formulation (rocBLAS bmm): scores = Q·K^T and O = P·V per (b, kv-head)
    group, full-Smax with masking."""
    dev = "cuda:0"
    for B, slen in [(16, 1600), (32, 1600)]:
        H, Hkv, Smax, D = 32, 8, 2120, 128
        G = H // Hkv
        torch.manual_seed(0)
        q = torch.randn(B, H, D, dtype=torch.bfloat16, device=dev)
        kc = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev)
        vc = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev)
        lens = torch.full((B,), slen, dtype=torch.int32, device=dev)
        mask = (torch.arange(Smax, device=dev)[None, :]
                >= lens[:, None]).view(B, 1, 1, Smax)

        def bmm_path():
            qg = q.view(B * Hkv, G, D)
            kg = kc.view(B * Hkv, Smax, D)
            s_ = torch.bmm(qg, kg.transpose(1, 2)) * (D ** -0.5)
            s_ = s_.view(B, Hkv, G, Smax).masked_fill(mask, float("-inf"))
            p_ = torch.softmax(s_.float(), dim=-1).to(torch.bfloat16)
            return torch.bmm(p_.view(B * Hkv, G, Smax),
                             vc.view(B * Hkv, Smax, D))

        for name, fn in [("hand", lambda: ops.decode_attention(q, kc, vc, lens)),
                         ("bmm", bmm_path)]:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(100):
                fn()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) / 100
            kv_bytes = 2 * B * Hkv * slen * D * 2
            print(f"B={B} {name}: {t*1e6:7.1f}us  {kv_bytes/t/1e12:.2f} TB/s")


def flash_probe():
    """Prefill flash-attention microbench (llama3-8b shape)."""
    dev = "cuda:0"
    for B, S in [(16, 2048), (32, 2048)]:
        H, Hkv, D = 32, 8, 128
        q = torch.randn(B, S, H, D, dtype=torch.bfloat16, device=dev)
        k = torch.randn(B, S, Hkv, D, dtype=torch.bfloat16, device=dev)
        v = torch.randn(B, S, Hkv, D, dtype=torch.bfloat16, device=dev)
        for _ in range(5):
            ops.attention(q, k, v, causal=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iters = 20
        for _ in range(iters):
            ops.attention(q, k, v, causal=True)
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) / iters
        flops = 2.0 * B * H * S * S * D * 2 / 2  # causal half
        print(f"flash B={B} S={S}: {t*1e3:.2f} ms  {flops/t/1e12:.0f} TFLOP/s")


if __name__ == "__main__":
    reps = int(sys.argv[sys.argv.index("--repeats") + 1]) \
        if "--repeats" in sys.argv else 1
    if "--kv" in sys.argv:
        kv = sys.argv[sys.argv.index("--kv") + 1]
        if kv != "fp8":
            sys.exit(f"--kv takes fp8, got {kv!r}")
        kv_fp8_probe(max(reps, 3))
        sys.exit(0)
    main(reps)
    if "--main-only" not in sys.argv:
        bmm_probe()
        flash_probe()
