"""ops.cosine_topk_masked (masked scan + top-k over e4m3fn codes or fp16
rows) against an fp64 reference over the same rows, queries and masks."""
import functools

import pytest
import torch

from sentio_amd import ops
from sentio_amd.ops import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 1e-4     # fp32 accumulation: dim * 2^-24 * |q| * |x| at dim <= 1024
CHUNK = 128

# N (or (chunks per block, extra rows)), B, k, dim
SHAPES = [(31, 1, 5, 64), (33, 16, 10, 1024), (127, 17, 10, 96),
          (129, 33, 128, 1024), ((2, 37), 17, 10, 64), ((3, 5), 32, 128, 1024)]


def _unit(n, dim, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, dim, generator=g)
    return x / x.norm(dim=1, keepdim=True)


@functools.lru_cache(maxsize=None)
def _data(dtype, shape):
    N, B, k, dim = shape
    if not isinstance(N, int):
        blocks, chunk, _ = ops.cosine_topk_fp8_plan(1 << 30)
        N = N[0] * blocks * chunk + N[1]
    x, q = _unit(N, dim, N).to(DEV), _unit(B, dim, N + 1).to(DEV).half()
    if dtype == "fp16":
        rows, scales = x.half(), None
        ref = q.double() @ rows.double().T
    else:
        rows, scales = torch_ref.index_quantize(x)
        ref = (q.double() @ rows.view(torch.float8_e4m3fn).double().T) \
            * scales.double()
    return q, rows, scales, ref, N


def _mask(pattern, N, B, k):
    g = torch.Generator().manual_seed(N + B)
    r = torch.arange(N)
    if pattern == "per_query":
        m = torch.rand(B, N, generator=g) < 0.3
        m[0], m[B - 1] = False, True
        return m
    few = torch.zeros(N, dtype=torch.bool)
    few[torch.randperm(N, generator=g)[:k // 2]] = True     # fewer than k
    return {
        "ones": r >= 0, "zeros": r < 0, "last_row": r == N - 1, "few": few,
        "one_tile": r // 16 == (N - 1) // 16,   # last tile of the last chunk
        "alt_tiles": (r // 16) % 2 == 1, "alt_chunks": (r // CHUNK) % 2 == 0,
        "stray": torch.rand((N + 127) // 128 * 128, generator=g) < 0.5,  # >= N
    }[pattern][None]


PATTERNS = ["ones", "zeros", "last_row", "one_tile", "alt_tiles",
            "alt_chunks", "few", "per_query", "stray"]


def _check(vals, rows, ref, ok, k):
    """The criteria of test_dense_fp8_gpu._check over the allowed rows."""
    B, N = ref.shape
    ok = ok.expand(B, N)
    assert vals.shape == (B, k) and rows.shape == (B, k)
    assert vals.dtype == torch.float32 and rows.dtype == torch.int64
    cnt = ok.sum(1, keepdim=True).clamp(max=k)
    valid = torch.arange(k, device=DEV)[None] < cnt
    assert torch.all(rows[~valid] == -1)
    assert torch.all(vals[~valid] == float("-inf"))
    assert torch.all(vals[:, :-1] >= vals[:, 1:]), "not sorted"
    assert torch.all((rows[valid] >= 0) & (rows[valid] < N))
    safe = rows.clamp(min=0)
    assert torch.all(torch.gather(ok, 1, safe)[valid]), "a masked row"
    for r in rows.tolist():
        r = [x for x in r if x >= 0]
        assert len(set(r)) == len(r), "row twice"
    got = torch.gather(ref, 1, safe)
    err = (vals.double() - got)[valid].abs()
    print(f"max |score - ref| = {err.max().item() if err.numel() else 0:.3e}")
    assert torch.all(err <= ATOL)
    top = torch.topk(ref.masked_fill(~ok, float("-inf")), min(k, N), 1).values
    kth = torch.gather(top, 1, (cnt - 1).clamp(min=0))
    assert torch.all((got >= kth - ATOL)[valid]), "a row outside the top k"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", ["fp8", "fp16"])
def test_kernel_matches_fp64_reference(dtype, shape, pattern):
    q, rows, scales, ref, N = _data(dtype, shape)
    k = shape[2]
    m = _mask(pattern, N, shape[1], k)
    allow = ops.pack_row_mask(m).to(DEV)
    vals, idx = ops.cosine_topk_masked(q, rows, scales, k, allow)
    _check(vals, idx, ref, m[:, :N].to(DEV), k)


@pytest.mark.parametrize("dtype", ["fp8", "fp16"])
def test_duplicated_rows_under_a_mask_come_back_in_row_order(dtype):
    q, rows, scales, _, N = _data(dtype, ((1, 64), 2, 10, 64))
    rows = rows.clone()
    dups = [3, 20, 40, CHUNK + 2, N - 1]    # tiles, chunks and blocks apart
    rows[dups] = rows[3].clone()
    if scales is not None:
        scales = scales.clone()
        scales[dups] = scales[3].clone()
    q = q.clone()
    q[0] = _unit(N, 64, N)[3].half()         # the vector behind row 3
    m = torch.rand(1, N, generator=torch.Generator().manual_seed(5)) < 0.5
    m[0, dups] = True
    m[0, 20] = False                         # a masked duplicate stays out
    allow = ops.pack_row_mask(m).to(DEV)
    idx = ops.cosine_topk_masked(q, rows, scales, 10, allow)[1]
    assert idx[0, :4].tolist() == [3, 40, CHUNK + 2, N - 1]
    assert torch.equal(
        idx, torch_ref.cosine_topk_masked(q, rows, scales, 10, allow)[1])


def test_all_ones_mask_gives_the_rows_of_the_unmasked_scan():
    q, codes, scales, ref, N = _data("fp8", ((3, 5), 32, 128, 1024))
    top = torch.topk(ref, 129, dim=1).values
    assert torch.all(top[:, :-1] > top[:, 1:]), "exact tie in the data"
    allow = ops.pack_row_mask(torch.ones(1, N, dtype=torch.bool)).to(DEV)
    assert torch.equal(ops.cosine_topk_masked(q, codes, scales, 128, allow)[1],
                       ops.cosine_topk_fp8(q, codes, scales, 128)[1])


def test_wrapper_rejects_bad_arguments():
    q, codes, scales, _, N = _data("fp8", (129, 33, 128, 1024))
    x16 = _data("fp16", (129, 33, 128, 1024))[1]
    allow = ops.pack_row_mask(torch.ones(1, N, dtype=torch.bool)).to(DEV)
    pad = torch.zeros(1, 9, dtype=torch.int32, device=DEV)
    bad = [
        (q, codes, scales, 5, allow[:, :4].contiguous()),      # W, M ...
        (q, codes, scales, 5, allow.repeat(1, 2)),
        (q, codes, scales, 5, allow.repeat(2, 1)),
        (q, codes, scales, 5, allow.long()), (q, codes, scales, 5, allow.cpu()),
        (q, codes, scales, 129, allow),
        (q, codes, scales, 5, pad[:, 1:]),                     # misaligned
        (q, codes, scales, 5, allow.repeat(1, 2)[:, ::2]),     # strided
        (q, x16, scales, 5, allow), (q, codes, None, 5, allow),
        (q.float(), x16, None, 5, allow), (q, x16[:, :48], None, 5, allow),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.cosine_topk_masked(*args)
