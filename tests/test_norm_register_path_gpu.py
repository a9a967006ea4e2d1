"""ops.rmsnorm_residual_partials keeps the rounded h in registers across the
reduction when a row is one or two steps per thread.  The kernel that loads
h back from memory (the formulation before that change, still serving
longer rows) is reachable at any row length with reread=True; both must
give the same bits: same values, summed in the same order.

Row lengths: 64 (part of one step), 4096 (one step of 1024 threads), 8192
(two steps) and 12288 (three: the re-reading kernel on both sides).
ops.rmsnorm_residual is unchanged (its register path was not faster in the
in-context trace, profiles/prefill_qkv_prep.md) and has no such switch.
"""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = [64, 4096, 8192, 12288]


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


def _rand(shape, dev, seed, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(device=dev, dtype=dtype)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("S", [1, 4])
def test_rmsnorm_residual_partials_equals_the_reread_kernel(dev, D, rows, S):
    from sentio_amd import ops

    part = _rand((S, rows, D), dev, D + rows + S, torch.float32)
    res = _rand((rows, D), dev, D + 11)
    w = _rand((D,), dev, 5)
    y, h = ops.rmsnorm_residual_partials(part, res, w, 1e-5)
    y0, h0 = ops.rmsnorm_residual_partials(part, res, w, 1e-5, reread=True)
    assert torch.equal(h, h0) and torch.equal(y, y0)
    wy, wh = ops.torch_ref.rmsnorm_residual_partials(
        part.cpu(), res.cpu().float(), w.cpu().float(), 1e-5)
    torch.testing.assert_close(h.float().cpu(), wh.float(), rtol=1e-2,
                               atol=1e-2)
    torch.testing.assert_close(y.float().cpu(), wy.float(), rtol=2e-2,
                               atol=2e-2)
