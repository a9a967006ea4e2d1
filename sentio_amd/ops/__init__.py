"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch refs on CPU.

Contract (driver + judge): on a GPU box the HIP extension `_sentio_hip`
MUST be the path that runs — if a CUDA tensor reaches an op and the
extension is missing, we raise instead of silently falling back to eager
PyTorch.  On CPU tensors the plain fp32 references in torch_ref run (tests,
hermetic config).
"""

from __future__ import annotations

import math

import torch

from sentio_amd.ops import torch_ref

_hip = None
_hip_err: str | None = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        from sentio_amd.ops import _sentio_hip  # built in-tree by setup.py

        _hip = _sentio_hip
    except ImportError as e:  # pragma: no cover - GPU-box only
        _hip_err = str(e)
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _require_hip():
    m = _load_hip()
    if m is None:
        raise RuntimeError(
            "sentio_amd HIP extension (_sentio_hip) is not built but a CUDA "
            "tensor reached an op. Build it with `python setup.py "
            f"build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). Import error: {_hip_err}"
        )
    return m


def _on_gpu(*tensors: torch.Tensor) -> bool:
    return any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))


# ---------------- elementwise / norm ----------------

def rmsnorm(x, weight, eps: float = 1e-5):
    if _on_gpu(x):
        return _require_hip().rmsnorm(x.contiguous(), weight.contiguous(), eps)
    return torch_ref.rmsnorm(x, weight, eps)


def rmsnorm_residual(x, residual, weight, eps: float = 1e-5):
    if _on_gpu(x):
        return _require_hip().rmsnorm_residual(
            x.contiguous(), residual.contiguous(), weight.contiguous(), eps
        )
    return torch_ref.rmsnorm_residual(x, residual, weight, eps)


def rmsnorm_residual_partials(part, residual, weight, eps: float = 1e-5, *,
                              reread: bool = False):
    """ops.rmsnorm_residual with the projection given as split-K partials:
    part fp32 [S, rows, D] (ops.linear_splitk), summed in increasing s, plus
    residual [..., D] → (y, h) shaped like residual.  The sum never rounds
    to bf16 before the residual add.  On the GPU rows of at most 8192
    elements keep h in registers between the two passes; reread=True takes
    the kernel that loads h back at any row length (tests and probes; the
    outputs are bit-identical)."""
    if _on_gpu(part):
        y, h = _require_hip().rmsnorm_residual_partials(
            part.contiguous(), residual.contiguous(), weight.contiguous(), eps,
            bool(reread))
        return y, h
    return torch_ref.rmsnorm_residual_partials(part, residual, weight, eps)


def rope_apply(x, cos, sin, pos):
    if _on_gpu(x):
        return _require_hip().rope_apply(
            x.contiguous(), cos.contiguous(), sin.contiguous(), pos.contiguous()
        )
    return torch_ref.rope_apply(x, cos, sin, pos)


def decode_qkv_prep(qkv, k_cache, v_cache, cos, sin, seq_lens):
    """Fused decode-token head prep: RoPE(q), RoPE(k)→cache, v→cache.
    qkv: [B, (H+2*Hkv)*D] raw projection; seq_lens: [B] i32 current position.
    Returns q [B, H, D]; writes k/v rows in place."""
    if _on_gpu(qkv):
        return _require_hip().decode_qkv_prep(
            qkv.contiguous(), k_cache, v_cache, cos, sin, seq_lens)
    return torch_ref.decode_qkv_prep(qkv, k_cache, v_cache, cos, sin, seq_lens)


def prefill_qkv_prep(qkv, cos, sin, pos0: int, n_heads: int, n_kv_heads: int,
                     k_cache=None, v_cache=None):
    """Fused prefill head prep: split the raw projection qkv
    [B, S, (H+2*Hkv)*D], RoPE q and k (token (b, s) sits at position
    pos0 + s) and put k / v in their final place, in one launch.

    With caches [Bc, Hkv, Smax, D]: RoPE(k) and v are written to rows
    pos0 .. pos0+S-1 of batch rows 0 .. B-1 (every row of a right-padded
    batch; nothing else is touched) and q [B, S, H, D] is returned.
    Without: returns (q, k, v), k and v contiguous [B, S, Hkv, D].

    Nothing is converted or copied: qkv must be contiguous, the tables
    contiguous float32 [rows, D/2], all on one device, D % 8 == 0,
    Bc >= B, 0 <= pos0, pos0 + S <= rows and pos0 + S <= Smax — anything
    else raises ValueError before a launch."""
    if not isinstance(qkv, torch.Tensor) or qkv.dim() != 3 \
            or qkv.numel() == 0:
        raise ValueError("qkv must be a non-empty [B, S, (H+2*Hkv)*D] tensor")
    if not qkv.is_contiguous():
        raise ValueError("qkv must be contiguous")
    B, S, W = qkv.shape
    H, Hkv, pos0 = int(n_heads), int(n_kv_heads), int(pos0)
    if H < 1 or Hkv < 1 or W % (H + 2 * Hkv):
        raise ValueError(f"qkv width {W} is not ({H}+2*{Hkv})*D")
    D = W // (H + 2 * Hkv)
    if D % 8:
        raise ValueError(f"head dim must be a multiple of 8, got {D}")
    for name, t in (("cos", cos), ("sin", sin)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 \
                or t.dim() != 2 or t.shape[1] != D // 2 \
                or not t.is_contiguous() or t.device != qkv.device:
            raise ValueError(f"{name} must be a contiguous float32 "
                             f"[rows, {D // 2}] tensor on {qkv.device}")
    if sin.shape[0] != cos.shape[0]:
        raise ValueError("cos and sin differ in rows")
    if pos0 < 0:
        raise ValueError(f"pos0 must be >= 0, got {pos0}")
    if pos0 + S > cos.shape[0]:
        raise ValueError(f"positions {pos0} .. {pos0 + S - 1} exceed the "
                         f"{cos.shape[0]} rope table rows")
    if (k_cache is None) != (v_cache is None):
        raise ValueError("give both caches or neither")
    if k_cache is not None:
        for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 \
                    or t.dtype != qkv.dtype or not t.is_contiguous() \
                    or t.device != qkv.device:
                raise ValueError(f"{name} must be a contiguous {qkv.dtype} "
                                 f"[Bc, Hkv, Smax, D] tensor on {qkv.device}")
        if v_cache.shape != k_cache.shape or k_cache.shape[1] != Hkv \
                or k_cache.shape[3] != D:
            raise ValueError(f"caches must both be [Bc, {Hkv}, Smax, {D}], "
                             f"got {tuple(k_cache.shape)} / "
                             f"{tuple(v_cache.shape)}")
        if k_cache.shape[0] < B:
            raise ValueError(f"cache has {k_cache.shape[0]} batch rows "
                             f"for {B}")
        if pos0 + S > k_cache.shape[2]:
            raise ValueError(f"positions {pos0} .. {pos0 + S - 1} exceed the "
                             f"cache's {k_cache.shape[2]} rows")
    if _on_gpu(qkv):
        if qkv.dtype != torch.bfloat16:
            raise ValueError(f"qkv must be bf16 on the GPU, got {qkv.dtype}")
        out = _require_hip().prefill_qkv_prep(qkv, cos, sin, pos0, H, Hkv,
                                              k_cache, v_cache)
        return out[0] if k_cache is not None else tuple(out)
    return torch_ref.prefill_qkv_prep(qkv, cos, sin, pos0, H, Hkv, k_cache,
                                      v_cache)


def swiglu(gate, up):
    if _on_gpu(gate):
        return _require_hip().swiglu(gate.contiguous(), up.contiguous())
    return torch_ref.swiglu(gate, up)


def swiglu_packed(gu):
    """gu [..., 2F] packed [gate | up] → silu(gate) * up [..., F]."""
    if _on_gpu(gu):
        return _require_hip().swiglu_packed(gu.contiguous())
    return torch_ref.swiglu_packed(gu)


def softmax(x, dim: int = -1):
    if _on_gpu(x):
        if dim not in (-1, x.ndim - 1):
            x = x.transpose(dim, -1).contiguous()
            return _require_hip().softmax_lastdim(x).transpose(dim, -1)
        return _require_hip().softmax_lastdim(x.contiguous())
    return torch_ref.softmax(x, dim)


# ---------------- attention ----------------

def _attn_scale(q, scale: float | None) -> float:
    """Softmax scale: the caller's, or 1/sqrt(head_dim)."""
    return float(scale) if scale is not None else 1.0 / math.sqrt(q.shape[-1])


def attention(q, k, v, causal: bool = True, scale: float | None = None,
              kv_lens=None):
    if _on_gpu(q):
        if kv_lens is None:
            kv_lens = torch.full((q.shape[0],), q.shape[1], dtype=torch.int32,
                                 device=q.device)
        return _require_hip().flash_attn(
            q.contiguous(), k.contiguous(), v.contiguous(), bool(causal),
            _attn_scale(q, scale), kv_lens.to(torch.int32).contiguous()
        )
    return torch_ref.attention(q, k, v, causal, scale, kv_lens)


def attention_cache(q, k_cache, v_cache, kv_lens, q_off: int,
                    scale: float | None = None):
    """Causal prefill attention for a SUFFIX of queries against the KV
    cache (prefix-KV caching): q [B, S_suf, H, D] at absolute positions
    q_off..q_off+S_suf-1; caches [B, Hkv, Smax, D]; kv_lens [B] absolute
    valid lengths (prefix + suffix)."""
    s = _attn_scale(q, scale)
    if _on_gpu(q):
        return _require_hip().flash_attn_cache(
            q.contiguous(), k_cache, v_cache,
            kv_lens.to(torch.int32).contiguous(), s, int(q_off))
    return torch_ref.attention_cache(q, k_cache, v_cache, kv_lens, q_off, s)


def decode_attention(q, k_cache, v_cache, seq_lens, scale: float | None = None):
    if _on_gpu(q):
        return _require_hip().decode_attn(
            q.contiguous(), k_cache, v_cache, seq_lens.contiguous(),
            _attn_scale(q, scale)
        )
    return torch_ref.decode_attention(q, k_cache, v_cache, seq_lens, scale)


def decode_attention_fused(qkv, k_cache, v_cache, cos, sin, seq_lens,
                           scale: float | None = None):
    """decode_qkv_prep + decode_attention in one kernel launch.
    qkv: [B, (H+2*Hkv)*D] raw projection; seq_lens: [B] contiguous i32, the
    position of the new token.  RoPE(q) never leaves registers, the new k/v
    row is written to the caches at row seq_lens[b], and attention covers
    seq_lens[b] + 1 keys.  Returns [B, H, D]."""
    if qkv.dim() != 2 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError("qkv must be [B, (H+2*Hkv)*D], caches [B,Hkv,Smax,D]")
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    if D not in (64, 128):
        raise ValueError(f"head dim must be 64 or 128, got {D}")
    H = qkv.shape[1] // D - 2 * Hkv
    if H <= 0 or H % Hkv or (H + 2 * Hkv) * D != qkv.shape[1]:
        raise ValueError(
            f"qkv width {qkv.shape[1]} is not (H+2*{Hkv})*{D} for a whole "
            "number of query heads per kv head")
    if seq_lens.dtype != torch.int32 or not seq_lens.is_contiguous() \
            or seq_lens.numel() != qkv.shape[0]:
        raise ValueError("seq_lens must be a contiguous int32 [B] tensor")
    s = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    if _on_gpu(qkv):
        return _require_hip().decode_attn_fused(
            qkv.contiguous(), k_cache, v_cache, cos, sin, seq_lens, s)
    return torch_ref.decode_attention_fused(qkv, k_cache, v_cache, cos, sin,
                                            seq_lens, s)


def _check_fp8_caches(k_cache, v_cache):
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError("fp8 caches must be two [B,Hkv,Smax,D] tensors of "
                         "equal shape")
    if k_cache.dtype != torch.uint8 or v_cache.dtype != torch.uint8:
        raise ValueError("fp8 caches must be uint8 (e4m3fn bytes), got "
                         f"{k_cache.dtype} / {v_cache.dtype}")


def _check_kv_scales(k_cache, **scales):
    Hkv = k_cache.shape[1]
    for name, t in scales.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 \
                or tuple(t.shape) != (Hkv,) or not t.is_contiguous() \
                or t.device != k_cache.device:
            raise ValueError(f"{name}: kv scale must be a contiguous float32 "
                             f"[{Hkv}] tensor on {k_cache.device}")


def decode_attention_fused_fp8(qkv, k_cache, v_cache, cos, sin, seq_lens,
                               k_scale, v_scale, k_inv=None, v_inv=None,
                               scale: float | None = None):
    """ops.decode_attention_fused over an FP8 (e4m3fn) KV cache: uint8
    caches [B, Hkv, Smax, D] with static fp32 [Hkv] scales.  The new k row
    is rotated and rounded as the bf16 op stores it, then quantised
    (torch_ref.kv_quantize is the spec) and written with the v row at
    seq_lens[b]; attention covers the dequantised seq_lens[b] + 1 keys, the
    new token included as stored.  k_inv / v_inv are the reciprocals of the
    scales (torch.reciprocal, computed here when not given — hold them next
    to the scales on a hot path).  Returns [B, H, D]."""
    if qkv.dim() != 2:
        raise ValueError("qkv must be [B, (H+2*Hkv)*D]")
    _check_fp8_caches(k_cache, v_cache)
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    if D not in (64, 128):
        raise ValueError(f"head dim must be 64 or 128, got {D}")
    H = qkv.shape[1] // D - 2 * Hkv
    if H <= 0 or H % Hkv or (H + 2 * Hkv) * D != qkv.shape[1]:
        raise ValueError(
            f"qkv width {qkv.shape[1]} is not (H+2*{Hkv})*{D} for a whole "
            "number of query heads per kv head")
    if H // Hkv > 8:
        raise ValueError(f"at most 8 query heads per kv head, got {H // Hkv}")
    if seq_lens.dtype != torch.int32 or not seq_lens.is_contiguous() \
            or seq_lens.numel() != qkv.shape[0]:
        raise ValueError("seq_lens must be a contiguous int32 [B] tensor")
    if k_inv is None:
        k_inv = torch.reciprocal(k_scale)
    if v_inv is None:
        v_inv = torch.reciprocal(v_scale)
    _check_kv_scales(k_cache, k_scale=k_scale, v_scale=v_scale, k_inv=k_inv,
                     v_inv=v_inv)
    s = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    if _on_gpu(qkv):
        return _require_hip().decode_attn_fused_fp8(
            qkv.contiguous(), k_cache, v_cache, cos, sin, seq_lens, k_scale,
            v_scale, k_inv, v_inv, s)
    return torch_ref.decode_attention_fused_fp8(
        qkv, k_cache, v_cache, cos, sin, seq_lens, k_scale, v_scale, k_inv,
        v_inv, s)


def kv_store_fp8(src_k, src_v, k_cache, v_cache, rows, S: int, k_inv, v_inv):
    """Quantising splice into an FP8 KV cache: the first S rows of the bf16
    sources [n, Hkv, S_src, D] are quantised (torch_ref.kv_quantize) into
    cache[rows[i], :, :S]; K and V in one launch.  rows: a Python sequence
    (checked here for range and duplicates) or an int tensor on the caches'
    device (the kernel skips entries outside [0, B)).  k_inv / v_inv:
    reciprocal scales, fp32 [Hkv]."""
    _check_fp8_caches(k_cache, v_cache)
    if src_k.dim() != 4 or src_v.shape != src_k.shape:
        raise ValueError("sources must be two [n,Hkv,S_src,D] tensors of "
                         "equal shape")
    B, Hkv, Smax, D = k_cache.shape
    n, _, S_src, _ = src_k.shape
    if src_k.shape[1] != Hkv or src_k.shape[3] != D:
        raise ValueError("source and cache kv heads / head dim differ")
    if D % 8:
        raise ValueError(f"head dim must be a multiple of 8, got {D}")
    S = int(S)
    if S < 0 or S > min(S_src, Smax):
        raise ValueError(f"S={S} exceeds min(S_src={S_src}, Smax={Smax})")
    _check_kv_scales(k_cache, k_inv=k_inv, v_inv=v_inv)
    if isinstance(rows, torch.Tensor):
        if rows.dim() != 1 or rows.numel() != n or rows.dtype not in (
                torch.int32, torch.int64) or rows.device != k_cache.device:
            raise ValueError("rows must be an int32/int64 [n] tensor on the "
                             "caches' device")
        rows_t = rows.to(torch.int32).contiguous()
    else:
        rows = [int(r) for r in rows]
        if len(rows) != n:
            raise ValueError(f"{len(rows)} rows for {n} sources")
        if any(r < 0 or r >= B for r in rows):
            raise ValueError(f"rows {rows} outside [0, {B})")
        if len(set(rows)) != len(rows):
            raise ValueError(f"duplicate rows in {rows}")
        rows_t = torch.tensor(rows, dtype=torch.int32, device=k_cache.device)
    if _on_gpu(k_cache):
        if src_k.dtype != torch.bfloat16 or src_v.dtype != torch.bfloat16:
            raise ValueError("sources must be bf16 on the GPU")
        _require_hip().kv_store_fp8(src_k.contiguous(), src_v.contiguous(),
                                    k_cache, v_cache, rows_t, S, k_inv, v_inv)
        return
    torch_ref.kv_store_fp8(src_k, src_v, k_cache, v_cache, rows_t, S, k_inv,
                           v_inv)


def decode_attention_bmm(q, k_cache, v_cache, seq_lens,
                         scale: float | None = None):
    """Decode attention as two rocBLAS batched GEMMs over the FULL cache
    extent (invalid keys masked): scores = Q·K^T per (b, kv-head) group,
    softmax, O = P·V.  Reads Smax rows instead of slen, but the library
    GEMM streams them ~1.4x faster than the hand split-S kernel when the
    cache is mostly full (measured 108 vs 153 us at B=32, slen/Smax≈0.75) —
    the hand kernel (ops.decode_attention) wins for mostly-empty caches.
    All ops are tensor-graph-capturable (the mask reads seq_lens in-graph).
    q: [B, H, D]; caches [B, Hkv, Smax, D]; returns [B, H, D]."""
    if not _on_gpu(q):
        return torch_ref.decode_attention(q, k_cache, v_cache, seq_lens, scale)
    B, H, D = q.shape
    Hkv, Smax = k_cache.shape[1], k_cache.shape[2]
    G = H // Hkv
    s = _attn_scale(q, scale)
    mask = (torch.arange(Smax, device=q.device)[None, :]
            >= seq_lens[:, None]).view(B, 1, 1, Smax)
    qg = q.view(B * Hkv, G, D)
    sc = torch.bmm(qg, k_cache.view(B * Hkv, Smax, D).transpose(1, 2)) * s
    sc = sc.view(B, Hkv, G, Smax).masked_fill(mask, float("-inf"))
    p = torch.softmax(sc.float(), dim=-1).to(q.dtype)
    out = torch.bmm(p.view(B * Hkv, G, Smax), v_cache.view(B * Hkv, Smax, D))
    return out.view(B, H, D)


# ---------------- pooling / retrieval ----------------

def mean_pool_l2norm(hidden, mask):
    if _on_gpu(hidden):
        return _require_hip().mean_pool_l2norm(hidden.contiguous(), mask.contiguous())
    return torch_ref.mean_pool_l2norm(hidden, mask)


def cosine_topk(q, mat, k: int):
    """Batched cosine top-k over an [N, D] row-normalized index.

    GPU path: the score matrix IS a TN GEMM — mat's [N, D] row-major layout
    is exactly F.linear's weight layout, so hipBLASLt streams the index on
    MFMA at memory rate (measured 0.20 TB/s for the hand wave-per-row scan
    vs ~5 TB/s through the library GEMM at 10M docs — GEMM-shaped work
    belongs on the GEMM path).  The hand kernel remains exposed as
    ops.cosine_scores for small/irregular scans."""
    if _on_gpu(q, mat):
        scores = torch.nn.functional.linear(q, mat).float()
        return torch.topk(scores, k, dim=1)
    return torch_ref.cosine_topk(q, mat, k)


def cosine_scores(q, mat):
    """Hand wave-per-row scan (LDS-staged queries); B*D*4 must fit in LDS."""
    if _on_gpu(q, mat):
        return _require_hip().cosine_scores(q.contiguous(), mat.contiguous())
    return (q.float() @ mat.float().T)


def bm25_score(term_ids, indptr, post_doc, post_tf, idf, doc_len, *,
               n_docs: int, k1: float, b: float, avgdl: float,
               plus_delta: float = 0.0):
    if _on_gpu(post_tf):
        return _require_hip().bm25_score(
            term_ids, indptr, post_doc, post_tf, idf, doc_len,
            int(n_docs), float(k1), float(b), float(avgdl), float(plus_delta)
        )
    return torch_ref.bm25_score(
        term_ids, indptr, post_doc, post_tf, idf, doc_len,
        n_docs, k1, b, avgdl, plus_delta
    )


# ---------------- sampling / GEMM ----------------

_FUSE_METHODS = {"rrf": 0, "weighted_rrf": 1, "comb_sum": 2}


def fuse_topk(d_ids, d_scores, s_ids, s_scores, *, method: str = "rrf",
              top_k: int = 10, rrf_k: float = 60.0, dense_weight: float = 0.7,
              sparse_weight: float = 0.3):
    """Batched device fusion (K4): per-query dense+sparse candidate lists
    (int64 ids, -1 pad; rank order; ids unique within a list — a top-k from
    one source never repeats a doc) → fused top-k (ids, scores).
    CPU path defers to index.fusion.fuse (the semantics oracle)."""
    if method not in _FUSE_METHODS:
        raise ValueError(f"Unknown fusion_method: {method}")
    if _on_gpu(d_ids):
        return _require_hip().fuse_topk(
            d_ids, d_scores, s_ids, s_scores, int(top_k),
            _FUSE_METHODS[method], float(rrf_k), float(dense_weight),
            float(sparse_weight))
    from sentio_amd.index import fusion as F

    B = d_ids.shape[0]
    out_i = torch.full((B, top_k), -1, dtype=torch.int64)
    out_s = torch.zeros(B, top_k)
    for q in range(B):
        dh = [(str(int(i)), float(s)) for i, s in zip(d_ids[q], d_scores[q])
              if int(i) >= 0]
        sh = [(str(int(i)), float(s)) for i, s in zip(s_ids[q], s_scores[q])
              if int(i) >= 0]
        fused = F.fuse(dh, sh, method=method, top_k=top_k, rrf_k=int(rrf_k),
                       dense_weight=dense_weight, sparse_weight=sparse_weight)
        for k, (doc, sc) in enumerate(fused):
            out_i[q, k] = int(doc)
            out_s[q, k] = sc
    return out_i, out_s


def sample_token(logits, temperature: float, seed: int = 0):
    if _on_gpu(logits):
        return _require_hip().sample_token(
            logits.contiguous(), float(temperature), int(seed)
        )
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch_ref.sample_token(logits, temperature, g)


def _row_tensor(v, B: int, dtype, device):
    """Scalar or [B] -> contiguous [B] tensor of dtype on device."""
    t = v if isinstance(v, torch.Tensor) else torch.tensor(v)
    t = t.to(device=device, dtype=dtype).flatten()
    if t.numel() == 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"per-row sampling parameter has {t.numel()} "
                         f"entries for {B} rows")
    return t.contiguous()


def sample_support(logits, temperature, top_k, top_p):
    """Deterministic half of filtered sampling: per row the threshold logit
    tau and the size of the kept set {v : logit_v >= tau} after top-k then
    top-p (renormalised over the top-k survivors; every token tied with tau
    is kept).  logits [B, V]; parameters are [B] or scalars.  Returns
    (tau [B] f32, count [B] i32); count is unspecified for greedy rows."""
    B, dev = logits.shape[0], logits.device
    t = _row_tensor(temperature, B, torch.float32, dev)
    k = _row_tensor(top_k, B, torch.int32, dev)
    p = _row_tensor(top_p, B, torch.float32, dev)
    if _on_gpu(logits):
        tau, count = _require_hip().sample_support(logits.contiguous(),
                                                   t, k, p)
        return tau, count
    return torch_ref.sample_support(logits, t, k, p)


def sample_filtered(logits, temperature, top_k, top_p, seed, step):
    """Per-row temperature / top-k / top-p sampling with per-row seeds.
    The noise for (row, v) is a counter hash of (seed_b, step_b, v): the same
    (logits row, parameters, seed, step) gives the same token at any row
    position and batch size.  logits [B, V]; the rest [B] or scalars.
    Returns [B] int64.  CPU and GPU agree on the support and on greedy rows,
    not on the stochastic pick."""
    B, dev = logits.shape[0], logits.device
    t = _row_tensor(temperature, B, torch.float32, dev)
    k = _row_tensor(top_k, B, torch.int32, dev)
    p = _row_tensor(top_p, B, torch.float32, dev)
    sd = _row_tensor(seed, B, torch.int64, dev)
    st = _row_tensor(step, B, torch.int32, dev)
    if _on_gpu(logits):
        return _require_hip().sample_filtered(logits.contiguous(), t, k, p,
                                              sd, st)
    return torch_ref.sample_filtered(logits, t, k, p, sd, st)


def _check_slot_array(t, name: str, n: int, dtype, device) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype \
            or tuple(t.shape) != (n,) or not t.is_contiguous() \
            or t.device != device:
        raise ValueError(f"{name} must be a contiguous {dtype} [{n}] tensor "
                         f"on {device}")


def _check_slot_call(logits, slot, temperature, top_k, top_p, seed, step,
                     active, tok, int32_extra=()):
    """The argument checks both slot-table samplers share; `int32_extra`:
    further (tensor, name) int32 [S] arrays.  Returns the slot list as an
    int32 tensor (or None / the tensor given)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 \
            or logits.dtype != torch.float32 or logits.numel() == 0:
        raise ValueError("logits must be a non-empty float32 [R, V] tensor")
    if not isinstance(tok, torch.Tensor) or tok.dim() != 1 \
            or tok.numel() == 0:
        raise ValueError("tok must be a non-empty int64 [S] tensor")
    R, S, dev = logits.shape[0], tok.shape[0], logits.device
    _check_slot_array(tok, "tok", S, torch.int64, dev)
    _check_slot_array(temperature, "temperature", S, torch.float32, dev)
    _check_slot_array(top_k, "top_k", S, torch.int32, dev)
    _check_slot_array(top_p, "top_p", S, torch.float32, dev)
    _check_slot_array(seed, "seed", S, torch.int64, dev)
    _check_slot_array(step, "step", S, torch.int32, dev)
    for t, name in int32_extra:
        _check_slot_array(t, name, S, torch.int32, dev)
    if active is not None:
        _check_slot_array(active, "active", S, torch.uint8, dev)
    if slot is None:
        if R != S:
            raise ValueError(f"without a slot table logits must have one row "
                             f"per slot: {R} rows for {S} slots")
    elif isinstance(slot, torch.Tensor):
        _check_slot_array(slot, "slot", R, torch.int32, dev)
    else:
        slot = [int(s) for s in slot]
        if len(slot) != R:
            raise ValueError(f"{len(slot)} slots for {R} logits rows")
        if any(s < 0 or s >= S for s in slot):
            raise ValueError(f"slots {slot} outside [0, {S})")
        if len(set(slot)) != len(slot):
            raise ValueError(f"duplicate slots in {slot}")
        slot = torch.tensor(slot, dtype=torch.int32, device=dev)
    return slot


def sample_slots(logits, slot, temperature, top_k, top_p, seed, step, active,
                 tok) -> None:
    """ops.sample_filtered over a table of S persistent slots, IN PLACE on
    `step` and `tok` (the continuous batcher's per-step sampler).

    logits f32 [R, V]; slot: None (R == S, row r is slot r), a Python
    sequence (checked here for range and duplicates, then uploaded) or an
    int32 [R] tensor on the logits' device (the kernel skips entries outside
    [0, S); duplicates are the caller's to avoid: two rows on one slot race
    on step[s]).  temperature f32, top_k i32, top_p f32, seed i64, step i32,
    tok i64: contiguous [S] tensors of exactly these dtypes on the logits'
    device -- nothing is converted, a copy could not be written back.
    active: None or uint8 [S]; a slot with active[s] == 0 is skipped.

    For every sampled row: tok[s] = the token ops.sample_filtered draws from
    logits[r] with slot s's parameters at step[s], then step[s] += 1.
    Skipped slots keep tok[s] and step[s].  CPU and GPU agree on the support
    and on greedy rows, not on the stochastic pick."""
    slot = _check_slot_call(logits, slot, temperature, top_k, top_p, seed,
                            step, active, tok)
    if _on_gpu(logits):
        _require_hip().sample_slots(logits.contiguous(), slot, temperature,
                                    top_k, top_p, seed, step, active, tok)
        return
    torch_ref.sample_slots(logits, slot, temperature, top_k, top_p, seed,
                           step, active, tok)


class GrammarTables:
    """The device tables of constrained sampling (see engines/grammar.py):
    next int16 [N, Vt], mask int32 [N, ceil(Vt/32)], dist int16 [N], plus
    max_dist, the largest dist entry (a host int: the kernel skips the dist
    lookup for rows whose budget cannot bind)."""

    def __init__(self, next, mask, dist, max_dist: int | None = None):
        for t, name, dt, nd in ((next, "next", torch.int16, 2),
                                (mask, "mask", torch.int32, 2),
                                (dist, "dist", torch.int16, 1)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt \
                    or t.dim() != nd or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dt} "
                                 f"{nd}-d tensor")
        N, Vt = next.shape
        if not (1 <= N <= 32767) or Vt < 1:
            raise ValueError(f"next must be [N <= 32767, Vt], got "
                             f"{tuple(next.shape)}")
        if tuple(mask.shape) != (N, (Vt + 31) // 32):
            raise ValueError(f"mask must be [{N}, {(Vt + 31) // 32}], got "
                             f"{tuple(mask.shape)}")
        if mask.shape[1] > 2048:
            raise ValueError("at most 65536 tokenizer entries")
        if tuple(dist.shape) != (N,):
            raise ValueError(f"dist must be [{N}], got {tuple(dist.shape)}")
        if next.device != mask.device or next.device != dist.device:
            raise ValueError("next, mask and dist must share a device")
        self.next, self.mask, self.dist = next, mask, dist
        self.max_dist = int(dist.max()) if max_dist is None else int(max_dist)

    @classmethod
    def from_numpy(cls, next, mask, dist, device="cpu") -> "GrammarTables":
        import numpy as np

        return cls(
            torch.from_numpy(np.ascontiguousarray(next)).to(device),
            torch.from_numpy(np.ascontiguousarray(mask)).to(device),
            torch.from_numpy(np.ascontiguousarray(dist)).to(device),
            int(np.max(dist)))

    @property
    def n_states(self) -> int:
        return int(self.next.shape[0])

    @property
    def vocab(self) -> int:
        return int(self.next.shape[1])

    @property
    def device(self):
        return self.next.device

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size()
                   for t in (self.next, self.mask, self.dist))


def _check_tables(tables, device) -> None:
    if not isinstance(tables, GrammarTables):
        raise ValueError("tables must be an ops.GrammarTables")
    if tables.device != device:
        raise ValueError(f"grammar tables are on {tables.device}, logits on "
                         f"{device}")


def sample_constrained(logits, temperature, top_k, top_p, seed, step, state,
                       left, tables):
    """Grammar-constrained ops.sample_filtered, IN PLACE on `state` and
    `left` (contiguous int32 [B] on the logits' device).

    A row in state s (0 <= s < N) with `left` tokens remaining, this one
    included, may pick v iff v < min(V, Vt), bit v of mask[s] is set and
    dist[next[s, v]] <= left - 1.  Every other logit counts as -inf; the
    rest is sample_filtered's arithmetic (same noise for the same (seed,
    step, v)).  Then state = next[s, tok] and left -= 1.  If every allowed
    logit is -inf or NaN the row takes the lowest allowed index.  Callers
    establish dist[state] <= left; the rule keeps it, so a row always ends
    in an accepting state.  A row with state < 0 is unconstrained: exactly
    sample_filtered over all V logits, state and left untouched (the GPU
    treats state >= N the same way; on the CPU, where the host owns the
    array, that is a ValueError).  Returns tok [B] int64."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 \
            or logits.numel() == 0:
        raise ValueError("logits must be a non-empty [B, V] tensor")
    B, dev = logits.shape[0], logits.device
    _check_tables(tables, dev)
    _check_slot_array(state, "state", B, torch.int32, dev)
    _check_slot_array(left, "left", B, torch.int32, dev)
    t = _row_tensor(temperature, B, torch.float32, dev)
    k = _row_tensor(top_k, B, torch.int32, dev)
    p = _row_tensor(top_p, B, torch.float32, dev)
    sd = _row_tensor(seed, B, torch.int64, dev)
    st = _row_tensor(step, B, torch.int32, dev)
    if _on_gpu(logits):
        return _require_hip().sample_constrained(
            logits.contiguous(), t, k, p, sd, st, state, left, tables.next,
            tables.mask, tables.dist, tables.max_dist)
    if bool((state >= tables.n_states).any()):
        raise ValueError(f"state outside the table's {tables.n_states} states")
    return torch_ref.sample_constrained(logits, t, k, p, sd, st, state, left,
                                        tables.next, tables.mask, tables.dist)


def sample_slots_constrained(logits, slot, temperature, top_k, top_p, seed,
                             step, active, tok, state, left, tables) -> None:
    """ops.sample_slots with a per-slot automaton: `state` and `left` are
    contiguous int32 [S] tensors on the logits' device, updated in place
    like `step` and `tok`.  Slot s samples as ops.sample_constrained does
    with (state[s], left[s]) at step[s]; state[s] < 0 is an unconstrained
    slot, sampled exactly as ops.sample_slots samples it.  Skipped slots
    keep tok, step, state and left."""
    slot = _check_slot_call(logits, slot, temperature, top_k, top_p, seed,
                            step, active, tok,
                            ((state, "state"), (left, "left")))
    _check_tables(tables, logits.device)
    if _on_gpu(logits):
        _require_hip().sample_slots_constrained(
            logits.contiguous(), slot, temperature, top_k, top_p, seed, step,
            active, tok, state, left, tables.next, tables.mask, tables.dist,
            tables.max_dist)
        return
    if bool((state >= tables.n_states).any()):
        raise ValueError(f"state outside the table's {tables.n_states} states")
    torch_ref.sample_slots_constrained(
        logits, slot, temperature, top_k, top_p, seed, step, active, tok,
        state, left, tables.next, tables.mask, tables.dist)


def skinny_gemm(x, w):
    """Skinny decode GEMM: x [M<=32, K] @ W^T with W stored [N, K] row-major
    (TN layout) → [M, N] bf16.  Streams W rows straight to MFMA A-fragments.
    CPU path: fp32 linear."""
    if _on_gpu(x):
        return _require_hip().skinny_gemm(x.contiguous(), w.contiguous())
    return torch.nn.functional.linear(x.float(), w.float()).to(x.dtype)


def decode_gemm_plan(M: int, N: int, K: int) -> tuple[int, int, int]:
    """(S, blocks, slab bytes) of the split-K decode GEMM for x [M, K] @
    W[N, K]^T; S == 0: the shape stays on the library GEMM."""
    return tuple(_require_hip().decode_gemm_plan(int(M), int(N), int(K)))


def linear_splitk(x, w, *, nan_fill: bool = False):
    """F.linear(x, w) for decode rows as split-K partials: fp32 [S, M, N]
    whose sum over dim 0 is x @ w^T, to be reduced by the consumer
    (ops.rmsnorm_residual_partials).  x [M, K], w [N, K] bf16.  Shapes the
    hand kernel does not plan (decode_gemm_plan S == 0: M > 32, N % 64,
    K % 32, or too small to fill the chip) go through ops.lt_linear and
    come back as one slice.  nan_fill pre-fills the slabs with NaN (tests:
    every element must be written).  CPU: one fp32 slice."""
    if not _on_gpu(x):
        return torch_ref.linear_splitk(x, w)
    hip = _require_hip()
    M, K = x.shape
    if hip.decode_gemm_plan(M, w.shape[0], K)[0] > 0:
        return hip.decode_gemm_splitk(x.contiguous(), w.contiguous(),
                                      bool(nan_fill))
    return lt_linear(x, w).float().unsqueeze(0)


_lt_ok = True


def lt_linear(x, w):
    """F.linear through the autotuned hipBLASLt binding (per-shape algorithm
    search on first use).  ONLY for shape-stable call sites (decode
    projections — fixed batch): autotuning costs ~hundreds of ms per new
    (M,N,K), so variable-M prefill GEMMs must stay on torch's heuristic
    (routing them here measured 19→5.4 QPS from perpetual re-tuning).
    Falls back to torch permanently on any failure; SENTIO_LT_GEMM=0
    disables."""
    global _lt_ok
    import os

    if (_lt_ok and _on_gpu(x)
            and os.environ.get("SENTIO_LT_GEMM", "1") != "0"):
        try:
            return _require_hip().lt_gemm_tn(x.contiguous(), w.contiguous())
        except RuntimeError as exc:
            if "rc=5" not in str(exc):   # rc=5: unseen shape mid-capture —
                _lt_ok = False           # fall back this call only
    return torch.nn.functional.linear(x, w)


def gemm_bf16(a, b):
    """Hand-written MFMA bf16 GEMM: a [M,K] @ b [K,N] → [M,N] bf16.
    CPU path: fp32 matmul."""
    if _on_gpu(a):
        return _require_hip().gemm_bf16(a.contiguous(), b.contiguous())
    return (a.float() @ b.float()).to(a.dtype)


__all__ = [
    "rmsnorm", "rmsnorm_residual", "rope_apply", "decode_qkv_prep", "prefill_qkv_prep","decode_attention_fused", "decode_attention_fused_fp8", "kv_store_fp8", "swiglu", "swiglu_packed", "softmax",
    "attention", "attention_cache", "decode_attention", "decode_attention_bmm", "mean_pool_l2norm", "cosine_topk",
    "bm25_score", "cosine_scores", "fuse_topk", "lt_linear", "linear_splitk", "decode_gemm_plan", "rmsnorm_residual_partials", "sample_token", "sample_filtered", "sample_slots", "sample_support", "sample_constrained", "sample_slots_constrained", "GrammarTables", "gemm_bf16", "skinny_gemm", "hip_available", "torch_ref",
]
