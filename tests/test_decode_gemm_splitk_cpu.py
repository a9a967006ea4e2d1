"""CPU side of the split-K decode projection: the torch reference pair and
the planner's arithmetic."""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from sentio_amd import ops
from sentio_amd.engines.configs import MODEL_CONFIGS


def test_reference_pair_equals_linear_then_rmsnorm_residual():
    torch.manual_seed(3)
    x = torch.randn(5, 48)
    w = torch.randn(24, 48)
    res = torch.randn(5, 24)
    w_norm = torch.randn(24)
    part = ops.linear_splitk(x, w)
    assert tuple(part.shape) == (1, 5, 24) and part.dtype == torch.float32
    y, h = ops.rmsnorm_residual_partials(part, res, w_norm, 1e-5)
    wy, wh = ops.rmsnorm_residual(F.linear(x, w), res, w_norm, 1e-5)
    torch.testing.assert_close(y, wy)
    torch.testing.assert_close(h, wh)


def test_reference_sums_partials_over_dim0():
    torch.manual_seed(4)
    part = torch.randn(3, 2, 1, 16)
    res = torch.randn(2, 1, 16)
    w = torch.randn(16)
    y, h = ops.rmsnorm_residual_partials(part, res, w)
    wy, wh = ops.rmsnorm_residual(part.sum(0), res, w)
    assert y.shape == res.shape
    torch.testing.assert_close(y, wy)
    torch.testing.assert_close(h, wh)


def test_cpu_model_keeps_the_library_route():
    from sentio_amd.engines.transformer import Transformer

    m = Transformer(MODEL_CONFIGS["tiny-decoder"], device="cpu", seed=5)
    assert not m.splitk_wo and not m.splitk_down


@pytest.mark.parametrize("name", sorted(MODEL_CONFIGS))
@pytest.mark.parametrize("M", [1, 16, 24, 32])
def test_planner_arithmetic(name, M, monkeypatch):
    """For wo (K = dim) and down (K = ffn_dim) of every model: an accepted
    shape splits K into whole 32-deep k-steps, has at least 128 blocks and at
    most 8 MB of slabs; a shape is refused only when the kernel cannot take
    it or no legal S reaches 128 blocks."""
    if not ops.hip_available():
        pytest.skip("HIP extension not importable here")
    monkeypatch.delenv("SENTIO_GEMM_SPLITK", raising=False)
    cfg = MODEL_CONFIGS[name]
    N = cfg.dim
    for K in (cfg.dim, cfg.ffn_dim):
        S, blocks, slab = ops.decode_gemm_plan(M, N, K)
        if S == 0:
            legal = [s for s in range(1, K // 32 + 1)
                     if K % (32 * s) == 0 and s * M * N * 4 <= 8 << 20]
            assert N % 64 or K % 32 or \
                all((N // 64) * s < 128 for s in legal), (name, M, K)
            continue
        assert K % (32 * S) == 0, (name, M, K, S)
        assert blocks == (N // 64) * S and blocks >= 128, (name, M, K, S)
        assert slab == S * M * N * 4 and slab <= 8 << 20, (name, M, K, S)
    if cfg.dim >= 2048:           # every real generator shape is planned
        assert ops.decode_gemm_plan(M, N, cfg.dim)[0] > 0
        assert ops.decode_gemm_plan(M, N, cfg.ffn_dim)[0] > 0


def test_planner_refuses_what_the_kernel_cannot_take():
    if not ops.hip_available():
        pytest.skip("HIP extension not importable here")
    assert ops.decode_gemm_plan(33, 4096, 4096)[0] == 0
    assert ops.decode_gemm_plan(8, 64, 100)[0] == 0
    assert ops.decode_gemm_plan(8, 100, 128)[0] == 0
