"""FP8 (e4m3fn) dense index on the CPU: the quantisation and scoring specs
in torch_ref, and DenseIndex(dtype="fp8", device="cpu")."""
import pytest
import torch

from sentio_amd.index.dense import DenseIndex
from sentio_amd.models.document import Document
from sentio_amd.ops import torch_ref


def _unit(n, dim, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, dim, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def _docs(n):
    return [Document(text=f"doc {i}", id=f"d{i}") for i in range(n)]


def test_index_quantize_matches_spec():
    x = _unit(6, 64, 0)
    x[1] = 0.0                                   # zero row
    x[2] = 0.0
    x[2, 5] = -1.0                               # one-hot row
    x[3] = _unit(1, 64, 1)[0] * 2.0 ** -24       # amax below 2^-20
    codes, scales = torch_ref.index_quantize(x)
    amax = x.abs().amax(dim=1)
    want_scale = torch.maximum(amax, torch.tensor(2.0 ** -20)) / 448.0
    want = (x * (1.0 / want_scale)[:, None]).clamp(-448, 448) \
        .to(torch.float8_e4m3fn).view(torch.uint8)
    assert codes.dtype == torch.uint8 and scales.dtype == torch.float32
    assert torch.equal(scales, want_scale) and torch.equal(codes, want)
    vals = codes.view(torch.float8_e4m3fn).float()
    assert torch.all(vals[1] == 0) and scales[1] == 2.0 ** -20 / 448.0
    assert vals[2, 5] == -448.0 and vals[2].abs().sum() == 448.0
    assert scales[3] == 2.0 ** -20 / 448.0 and vals[3].abs().max() < 448.0 / 8
    assert torch.isfinite(vals).all()


def test_cosine_topk_fp8_ref_order_ties_padding():
    x = _unit(5, 32, 2)
    x[3] = x[1]                                  # duplicated row
    codes, scales = torch_ref.index_quantize(x)
    q = x[[1, 4]].half()
    full = (q.double() @ codes.view(torch.float8_e4m3fn).double().T) \
        * scales.double()
    vals, rows = torch_ref.cosine_topk_fp8(q, codes, scales, 8)
    assert vals.shape == (2, 8) and rows.dtype == torch.int64
    assert rows[0, :2].tolist() == [1, 3]        # tie: lower row first
    assert rows[1, 0] == 4
    assert torch.all(vals[:, :4] >= vals[:, 1:5])
    assert torch.allclose(vals[:, :5].double(),
                          torch.gather(full, 1, rows[:, :5]), atol=1e-6)
    assert torch.all(rows[:, 5:] == -1)
    assert torch.all(vals[:, 5:] == float("-inf"))


def test_fp8_index_search_stats_roundtrip(tmp_path):
    n, dim, k = 300, 64, 7
    emb = _unit(n, dim, 3) * 3.0                 # add() normalises
    idx = DenseIndex(dim=dim, device="cpu", dtype="fp8")
    idx.GROW = 0                                 # grow to exactly what is added
    idx.add(_docs(n), emb)
    assert idx._vecs.numel() == 0 and idx._codes.dtype == torch.uint8
    st = idx.stats()
    assert st["dtype"] == "fp8" and st["hbm_bytes"] == n * (dim + 4)

    q = _unit(4, dim, 4)
    deq = idx._codes.view(torch.float8_e4m3fn).double() \
        * idx._scales.double()[:, None]
    qn = (q / q.norm(dim=1, keepdim=True)).half().double()
    want = torch.topk(qn @ deq.T, k, dim=1).indices
    hits = idx.search(q, k)
    assert [[h[0] for h in row] for row in hits] == \
        [[f"d{i}" for i in row] for row in want.tolist()]
    assert torch.equal(idx.search_rows(q, k)[1], want)
    small = DenseIndex(dim=dim, device="cpu", dtype="fp8")
    small.add(_docs(3), emb[:3])
    vals, rows = small.search_rows(q, 5)         # fewer rows than top_k
    assert torch.all(rows[:, 3:] == -1) and torch.all(rows[:, :3] >= 0)
    assert torch.all(vals[:, 3:] == float("-inf"))
    with pytest.raises(ValueError, match="k must be"):
        idx.search(q, 129)

    path = str(tmp_path / "dense.pt")
    idx.save(path)
    state = torch.load(path, weights_only=False)
    assert state["dtype"] == "fp8" and "vecs" not in state
    back = DenseIndex.load(path, device="cpu")
    assert back.fp8 and len(back) == n and back.doc_ids == idx.doc_ids
    assert torch.equal(back._codes[:n], idx._codes[:n])
    assert torch.equal(back._scales[:n], idx._scales[:n])
    idx.clear()
    assert len(idx) == 0 and idx.stats()["hbm_bytes"] == 0


def test_fp16_snapshot_still_loads(tmp_path):
    idx = DenseIndex(dim=32, device="cpu")
    idx.add(_docs(3), _unit(3, 32, 5))
    path = str(tmp_path / "old.pt")
    idx.save(path)
    back = DenseIndex.load(path, device="cpu")
    assert not back.fp8 and torch.allclose(back._vecs[:3], idx._vecs[:3])


@pytest.mark.parametrize("dim", [16, 48, 1056])
def test_fp8_index_rejects_dim(dim):
    with pytest.raises(ValueError, match="fp8 index"):
        DenseIndex(dim=dim, device="cpu", dtype=torch.float8_e4m3fn)


def test_settings_dense_index_dtype(monkeypatch):
    from sentio_amd.config import Settings

    monkeypatch.delenv("DENSE_INDEX_DTYPE", raising=False)
    assert Settings.from_env().dense_index_dtype == "fp16"
    monkeypatch.setenv("DENSE_INDEX_DTYPE", "fp8")
    assert Settings.from_env().dense_index_dtype == "fp8"
    monkeypatch.setenv("DENSE_INDEX_DTYPE", "int8")
    with pytest.raises(ValueError, match="DENSE_INDEX_DTYPE"):
        Settings.from_env()


def test_fp8_recall_against_fp16_rounded_index(capsys):
    """recall@10 against exact fp32 search, N = 20 000, dim 1024, 64 queries
    of random unit vectors.  Printed; the fp8 index is compared only with the
    fp16-rounded index on the same data (profiles/dense_fp8.md has the
    figures: fp16 0.9984, fp8 0.9563 on this seed)."""
    n, dim, k = 20000, 1024, 10
    x, q = _unit(n, dim, 6), _unit(64, dim, 7)
    exact = torch.topk(q @ x.T, k, dim=1).indices

    def recall(rows):
        return sum(len(set(a) & set(b)) for a, b in
                   zip(rows.tolist(), exact.tolist())) / exact.numel()

    r16 = recall(torch.topk(q.half().float() @ x.half().float().T, k,
                            dim=1).indices)
    codes, scales = torch_ref.index_quantize(x)
    r8 = recall(torch_ref.cosine_topk_fp8(q.half(), codes, scales, k)[1])
    with capsys.disabled():
        print(f"\nrecall@10 vs fp32: fp16 index {r16:.4f}, fp8 index {r8:.4f}")
    # e4m3fn rounds each element by at most 2^-4 relative (rms 2^-4/sqrt(3)),
    # so a score moves by about 0.036 * sqrt(sum q_d^2 x_d^2) ~ 0.036 / 32 ~
    # 1e-3, the size of ONE gap between neighbours at rank 10 of 20 000
    # (score sigma 1/32, top-10 near 3.3 sigma: gap ~ sigma / (10 * 3.3)).
    # Only the 10th / 11th place can swap: at most one of a query's ten.
    assert r8 >= r16 - 0.1
