"""Split-K decode GEMM (ops.linear_splitk) and the residual RMSNorm that sums
its partials (ops.rmsnorm_residual_partials) on the GPU.

The kernel walks a K slice in chunks of CK k-values (512 when the slice K/S
is whole 512-deep chunks, else 256), split over two k-groups of 32-deep MFMA
steps; `_chunk` mirrors that so the one-hot positions can sit on both sides
of every boundary the index arithmetic has.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ONE_HOT_SHAPES = [(1, 128, 64), (7, 256, 192), (16, 512, 64),
                  (17, 2048, 2048), (32, 1792, 128), (32, 4096, 4096)]
FORCED_S = [1, 2, 4, 7, 8]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(autouse=True)
def _require_hip_ext():
    from sentio_amd import ops

    if torch.cuda.is_available():
        assert ops.hip_available(), "HIP extension must be built on a GPU box"


def _chunk(kslice: int) -> int:
    return 512 if kslice % 512 == 0 else 256


def _one_hot_positions(K: int, S: int) -> list[int]:
    """0, K-1, both sides of every slice boundary and of every chunk
    (unrolled-batch) boundary inside a slice; for K <= 512 also both sides
    of every 32-deep k-step."""
    kslice = K // S
    ck = _chunk(kslice)
    edges = set()
    for s in range(S):
        edges.add(s * kslice)
        for c in range(ck, kslice, ck):
            edges.add(s * kslice + c)
    if K <= 512:
        edges.update(range(0, K, 32))
    ks = {0, K - 1}
    for e in edges:
        if 0 < e < K:
            ks.update((e - 1, e))
    return sorted(ks)


def _weights(N: int, K: int, dev: str) -> torch.Tensor:
    """Random bf16 with row n scaled by a power of two that differs from
    every row within 60 of it: exact in bf16, so any m/n/k mix-up shows."""
    g = torch.Generator(device="cpu").manual_seed(N * 31 + K)
    w = torch.randn(N, K, generator=g)
    scale = torch.pow(2.0, (torch.arange(N) % 61 - 30).float())
    return (w * scale[:, None]).to(torch.bfloat16).to(dev)


@pytest.mark.parametrize("M,K,N", ONE_HOT_SHAPES)
def test_one_hot_rows_return_weight_columns_exactly(dev, monkeypatch, M, K, N):
    from sentio_amd import ops

    w = _weights(N, K, dev)
    wf = w.float()
    for S in FORCED_S + [None]:
        if S is None:
            monkeypatch.delenv("SENTIO_GEMM_SPLITK", raising=False)
            S_eff = ops.decode_gemm_plan(M, N, K)[0] or 1
        elif K % (32 * S):
            continue
        else:
            monkeypatch.setenv("SENTIO_GEMM_SPLITK", str(S))
            S_eff = S
        ks_all = _one_hot_positions(K, S_eff)
        for i in range(0, len(ks_all), M):
            ks = (ks_all[i:i + M] * M)[:M]      # cycle to fill the M rows
            x = torch.zeros(M, K, dtype=torch.bfloat16, device=dev)
            x[torch.arange(M), torch.tensor(ks)] = 1.0
            part = ops.linear_splitk(x, w, nan_fill=True)
            assert part.dtype == torch.float32
            assert tuple(part.shape) == (S_eff, M, N), (S, part.shape)
            assert torch.isfinite(part).all(), "an element was not written"
            want = wf[:, ks].T
            got = part.sum(0)
            assert torch.equal(got, want), (
                f"M={M} K={K} N={N} S={S}: "
                f"{(got != want).sum().item()} elements differ")


@pytest.mark.parametrize("M,K,N", [(32, 14336, 4096), (24, 8192, 2048),
                                   (32, 18944, 3584)])
def test_random_operands_within_fp32_accumulation_bound(dev, M, K, N):
    """|err| <= K * 2^-23 * (|x| @ |W|^T): the worst-case error of any fp32
    summation order, with one bit of slack for MFMA-internal rounding."""
    from sentio_amd import ops

    if ops.decode_gemm_plan(M, N, K)[0] == 0:
        pytest.skip(f"decode_gemm_plan does not accept M={M} N={N} K={K}")
    torch.manual_seed(9)
    x = (torch.randn(M, K) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.5 + 0.1).to(torch.bfloat16)
    part = ops.linear_splitk(x.to(dev), w.to(dev), nan_fill=True)
    assert tuple(part.shape[1:]) == (M, N) and part.shape[0] > 1
    assert torch.isfinite(part).all(), "an element was not written"
    want = F.linear(x.float(), w.float())
    bound = K * 2.0 ** -23 * F.linear(x.float().abs(), w.float().abs())
    err = (part.sum(0).cpu() - want).abs()
    print(f"M={M} K={K} N={N} S={part.shape[0]}: max err {err.max():.3e}, "
          f"max err/bound {(err / bound).max():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("M,K,N", [(33, 4096, 4096), (8, 100, 64),
                                   (8, 128, 100)])
def test_unsupported_shapes_fall_back_to_one_slice(dev, M, K, N):
    from sentio_amd import ops

    assert ops.decode_gemm_plan(M, N, K)[0] == 0
    torch.manual_seed(4)
    x = (torch.randn(M, K) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.5 + 0.1).to(torch.bfloat16)
    part = ops.linear_splitk(x.to(dev), w.to(dev))
    assert tuple(part.shape) == (1, M, N) and part.dtype == torch.float32
    torch.testing.assert_close(part.sum(0).cpu(),
                               F.linear(x.float(), w.float()),
                               rtol=3e-2, atol=3e-1)


def test_override_that_does_not_divide_names_the_value(dev, monkeypatch):
    from sentio_amd import ops

    monkeypatch.setenv("SENTIO_GEMM_SPLITK", "3")
    with pytest.raises(RuntimeError, match="SENTIO_GEMM_SPLITK='3'"):
        ops.decode_gemm_plan(32, 4096, 4096)


def test_rmsnorm_residual_partials(dev):
    from sentio_amd import ops

    torch.manual_seed(12)
    for D in (256, 2048, 3584, 4096):
        w = torch.randn(D).to(torch.bfloat16)
        for rows in (1, 32):
            res = torch.randn(rows, D).to(torch.bfloat16)
            for S in (1, 2, 8):
                part = torch.randn(S, rows, D) * 0.5
                y, h = ops.rmsnorm_residual_partials(
                    part.to(dev), res.to(dev), w.to(dev), 1e-5)
                assert y.shape == res.shape and h.shape == res.shape
                h_ref = part.double().sum(0) + res.double()
                gap = (h.double().cpu() - h_ref).abs()
                # one bf16 rounding of the exact sum
                assert (gap <= 2.0 ** -8 * h_ref.abs() + 2.0 ** -20).all(), (
                    D, rows, S, gap.max().item())
                wy, _ = ops.torch_ref.rmsnorm_residual_partials(
                    part, res.float(), w.float(), 1e-5)
                torch.testing.assert_close(y.float().cpu(), wy,
                                           rtol=2e-2, atol=2e-2)


def test_decode_routes_agree_on_llama3_1b(dev, monkeypatch):
    """Two decode steps after a 24-token prefill: the split-K route against
    SENTIO_DECODE_GEMM=lt, same weights, at the tolerance of
    test_forward_decode_matches_prefill."""
    from sentio_amd.engines.configs import MODEL_CONFIGS
    from sentio_amd.engines.transformer import KVCache, Transformer

    cfg = MODEL_CONFIGS["llama3-1b"]
    B, S = 2, 24
    torch.manual_seed(7)
    toks = torch.randint(0, cfg.vocab_size, (B, S + 2), device=dev)

    def run(mode):
        if mode is None:
            monkeypatch.delenv("SENTIO_DECODE_GEMM", raising=False)
        else:
            monkeypatch.setenv("SENTIO_DECODE_GEMM", mode)
        m = Transformer(cfg, device=dev, dtype="bf16", seed=11)
        cache = KVCache(cfg, B, 64, dev, m.dtype)
        m.prefill(toks[:, :S], cache)
        out = [m.decode_step(toks[:, S + i:S + i + 1], cache).clone()
               for i in range(2)]
        torch.cuda.synchronize()
        return m, out

    m_new, new = run(None)
    assert m_new.splitk_wo and m_new.splitk_down
    m_lt, lt = run("lt")
    assert not m_lt.splitk_wo and not m_lt.splitk_down
    del m_new, m_lt
    for step, (a, b) in enumerate(zip(new, lt)):
        print(f"decode step {step}: max logit gap "
              f"{(a - b).abs().max().item():.4f}")
        torch.testing.assert_close(a, b, rtol=5e-2, atol=5e-1)


def test_graph_captured_generate_on_both_routes(dev, monkeypatch):
    """tiny-decoder64 is too small for the planner, so the override puts its
    projections on the split-K pair; the captured step must replay."""
    from sentio_amd.engines.generator import GeneratorEngine

    import gc

    counts = {}
    try:
        for mode in ("auto", "lt"):
            monkeypatch.setenv("SENTIO_DECODE_GEMM", mode)
            monkeypatch.setenv("SENTIO_GEMM_SPLITK", "2")
            g = GeneratorEngine("tiny-decoder64", device=dev, max_seq=64)
            assert g.model.splitk_wo == (mode == "auto")
            steps = []
            out = g.generate(["graph parity"], max_new_tokens=8,
                             temperature=0.0, stop_on_eos=False,
                             on_token=lambda i, toks: steps.append(list(toks)))
            assert len(out) == 1
            counts[mode] = len(steps)
            del g
    finally:
        # A dead engine is a reference cycle that owns its captured graphs.
        # While one of them lives, the RNG's capture state stays the pair of
        # tensors this inference-mode capture created, and a later capture
        # outside inference mode cannot update them: free the engines here.
        g = None
        gc.collect()
        torch.cuda.synchronize()
    assert counts["auto"] == counts["lt"] > 0
