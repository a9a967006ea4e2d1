"""The shared transformer core for encoder / reranker / generator engines.

MI355X-first design notes:
* plain projection GEMMs (fused QKV, fused gate+up, down, lm_head) go through
  torch.matmul → hipBLASLt/rocBLAS on ROCm — library GEMMs for library-shaped
  work;
* everything between them is a hand-written gfx950 HIP kernel via sentio_amd.ops:
  fused RMSNorm (+residual), RoPE from precomputed tables, flash-style MFMA
  attention for prefill, single-pass online-softmax decode attention over the
  KV cache, fused SwiGLU, masked mean-pool + L2-norm for the encoder;
* KV caches are preallocated contiguous [B, Hkv, Smax, hd] tensors in HBM —
  288 GB/GPU means we size for residency, not paging;
* weights are bf16, random-init (no network for checkpoints).

Replaces (semantically) the reference's remote encoder/reranker/LLM calls
(reference src/core/embeddings/providers/jina.py:165,
src/core/rerankers/jina_reranker.py:172, src/core/llm/providers/openai.py:117).
"""

from __future__ import annotations

import math
import os

import torch

from sentio_amd import ops
from sentio_amd.engines.configs import ModelConfig
from sentio_amd.parallel.tp import (TPContext, linear_row_parallel,
                                    shard_columns, shard_qkv, shard_rows)


def _dtype(name: str) -> torch.dtype:
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[name]


class TransformerWeights:
    """Flat weight container (not nn.Module: no autograd needed for serving)."""

    def __init__(self, cfg: ModelConfig, device: str, dtype: torch.dtype,
                 seed: int = 1234, tp: TPContext | None = None):
        self.cfg = cfg
        self.device = device
        self.dtype = dtype
        self.tp = tp or TPContext()
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        d, hd = cfg.dim, cfg.head_dim
        qkv_out = (cfg.n_heads + 2 * cfg.n_kv_heads) * hd
        std = 0.02
        f = cfg.ffn_dim

        def init(*shape):
            # init on device when possible for speed; generator is CPU-side so
            # large models draw on device with a per-tensor seed instead.
            if device == "cpu":
                return torch.randn(*shape, generator=gen, dtype=torch.float32).mul_(std).to(dtype)
            t = torch.empty(*shape, dtype=dtype, device=device)
            t.normal_(0.0, std)
            return t

        if device != "cpu":
            torch.manual_seed(seed)

        tp = self.tp
        self.tok_emb = init(cfg.vocab_size, d)
        self.layers = []
        # Weights are STORED [out, in] (TN layout) and applied via F.linear:
        # hipBLASLt's TN path streams the weight rows coalesced for skinny
        # decode batches (measured 2.5x on the down projection vs [in, out],
        # profiles/gemm_probe) and is the layout checkpoints use.
        for _ in range(cfg.n_layers):
            # full tensors are drawn identically on every rank (same seed and
            # order), then sliced — TP=N matches TP=1 numerically.
            wqkv = shard_qkv(init(d, qkv_out), cfg.n_heads, cfg.n_kv_heads, hd, tp)
            wo = shard_rows(init(cfg.n_heads * hd, d), tp)
            wgu_full = init(d, 2 * f)
            if tp.enabled:
                w_gate_up = torch.cat(
                    [shard_columns(wgu_full[:, :f], tp),
                     shard_columns(wgu_full[:, f:], tp)], dim=1)
            else:
                w_gate_up = wgu_full
            w_down = shard_rows(init(f, d), tp)
            self.layers.append({
                "attn_norm": torch.ones(d, dtype=dtype, device=device),
                "wqkv": wqkv.t().contiguous(),
                "wo": wo.t().contiguous(),
                "ffn_norm": torch.ones(d, dtype=dtype, device=device),
                "w_gate_up": w_gate_up.t().contiguous(),
                "w_down": w_down.t().contiguous(),
            })
        self.final_norm = torch.ones(d, dtype=dtype, device=device)
        if cfg.causal:
            self.lm_head = init(d, cfg.vocab_size).t().contiguous()
        if cfg.pooled_head:
            self.head = init(d, cfg.pooled_head).t().contiguous()

    @property
    def n_bytes(self) -> int:
        total = self.tok_emb.nelement()
        for l in self.layers:
            total += sum(t.nelement() for t in l.values())
        total += self.final_norm.nelement()
        if hasattr(self, "lm_head"):
            total += self.lm_head.nelement()
        return total * self.tok_emb.element_size()


KV_DTYPES = ("bf16", "fp8")


def check_kv_dtype(kv_dtype: str, cfg: ModelConfig | None = None) -> str:
    """Validate a KV-cache dtype name, and for "fp8" that the model fits the
    FP8 decode kernel — raised where the cache or engine is BUILT, not at
    the first decode step."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv cache dtype must be one of {KV_DTYPES}, "
                         f"got {kv_dtype!r}")
    if kv_dtype == "fp8" and cfg is not None:
        if os.environ.get("SENTIO_DECODE_ATTN") == "bmm":
            raise ValueError("the fp8 KV cache has no bmm decode variant "
                             "(unset SENTIO_DECODE_ATTN=bmm)")
        if cfg.head_dim not in (64, 128):
            raise ValueError("the fp8 KV cache needs head dim 64 or 128, "
                             f"got {cfg.head_dim}")
        g = cfg.n_heads // cfg.n_kv_heads    # TP shards both alike
        if g > 8:
            raise ValueError("the fp8 KV cache serves at most 8 query heads "
                             f"per kv head, got {g}")
    return kv_dtype


class KVCache:
    """Contiguous [B, Hkv, Smax, hd] K and V per layer.  kv_dtype "bf16"
    stores `dtype`; "fp8" stores uint8 e4m3fn bytes (view as
    torch.float8_e4m3fn) plus static fp32 scales per layer and kv head:
    scales[layer] is [4, Hkv] = k_scale, v_scale, k_inv, v_inv, read by the
    kernels at run time — set_scales() updates them in place, captured
    graphs keep working."""

    def __init__(self, cfg: ModelConfig, batch: int, max_seq: int, device: str,
                 dtype: torch.dtype, n_kv_heads: int | None = None,
                 kv_dtype: str = "bf16", scales: list | None = None):
        nkv = n_kv_heads or cfg.n_kv_heads
        self.kv_dtype = check_kv_dtype(kv_dtype, cfg)
        self.fp8 = kv_dtype == "fp8"
        store = torch.uint8 if self.fp8 else dtype
        self.k = [
            torch.zeros(batch, nkv, max_seq, cfg.head_dim,
                        dtype=store, device=device)
            for _ in range(cfg.n_layers)
        ]
        self.v = [
            torch.zeros(batch, nkv, max_seq, cfg.head_dim,
                        dtype=store, device=device)
            for _ in range(cfg.n_layers)
        ]
        self.seq_lens = torch.zeros(batch, dtype=torch.int32, device=device)
        self.max_seq = max_seq
        # `scales` shares another owner's tensors (an engine keeps one set
        # for all its session caches)
        self.scales = None
        if self.fp8:
            self.scales = scales if scales is not None else [
                torch.ones(4, nkv, dtype=torch.float32, device=device)
                for _ in range(cfg.n_layers)]
            if len(self.scales) != cfg.n_layers or any(
                    tuple(t.shape) != (4, nkv) or t.dtype != torch.float32
                    for t in self.scales):
                raise ValueError(f"fp8 scales must be {cfg.n_layers} float32 "
                                 f"[4, {nkv}] tensors")

    def set_scales(self, k_scales, v_scales) -> None:
        """Per-layer [Hkv] k / v scales, written in place."""
        if not self.fp8:
            raise ValueError("only an fp8 KVCache has scales")
        write_kv_scales(self.scales, k_scales, v_scales)


def write_kv_scales(scales: list, k_scales, v_scales) -> None:
    """Write per-layer [Hkv] k / v scales and their reciprocals
    (torch.reciprocal: the kernels only multiply) IN PLACE into the
    [4, Hkv] tensors `scales`.  Validates everything before the first
    write."""
    if len(k_scales) != len(scales) or len(v_scales) != len(scales):
        raise ValueError(f"need {len(scales)} per-layer scale rows")
    rows = []
    for sc, ks, vs in zip(scales, k_scales, v_scales):
        k1 = torch.as_tensor(ks, dtype=torch.float32).reshape(-1).cpu()
        v1 = torch.as_tensor(vs, dtype=torch.float32).reshape(-1).cpu()
        if k1.numel() != sc.shape[1] or v1.numel() != sc.shape[1]:
            raise ValueError(f"scales must be [{sc.shape[1]}] per layer")
        kv = torch.stack([k1, v1])
        if not bool(torch.isfinite(kv).all()) or not bool((kv > 0).all()):
            raise ValueError("kv scales must be finite and positive")
        rows.append(kv)
    for sc, kv in zip(scales, rows):
        kv = kv.to(sc.device)
        sc[:2].copy_(kv)
        sc[2:].copy_(torch.reciprocal(kv))


class Transformer:
    """Forward-only transformer executing on sentio ops."""

    def __init__(self, cfg: ModelConfig, device: str = "cpu",
                 dtype: str | torch.dtype = "bf16", seed: int = 1234,
                 tp: TPContext | None = None):
        self.cfg = cfg
        self.device = device
        self.tp = tp or TPContext()
        if self.tp.enabled:
            assert cfg.n_heads % self.tp.world == 0
            assert cfg.n_kv_heads % self.tp.world == 0
        self.h_local = cfg.n_heads // self.tp.world
        self.hkv_local = cfg.n_kv_heads // self.tp.world
        self.dtype = _dtype(dtype) if isinstance(dtype, str) else dtype
        if device == "cpu":
            # bf16 matmuls on CPU are slow and loose; tests run fp32
            self.dtype = torch.float32
        self.w = TransformerWeights(cfg, device, self.dtype, seed, self.tp)
        cos, sin = ops.torch_ref.rope_tables(cfg.max_seq, cfg.head_dim,
                                             cfg.rope_base, device)
        self.rope_cos, self.rope_sin = cos, sin
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        # Decode-attention implementation, fixed for the model's lifetime
        # (forward_decode is captured into hipGraphs and prefill runs on the
        # batcher's admission stream beside it, so nothing may reassign it).
        # SENTIO_DECODE_ATTN=bmm selects the two-batched-GEMM formulation;
        # anything else (auto, hand) the hand split-S kernel.  bmm looked
        # ~1.4x faster in an isolated cold-box probe, but IN CONTEXT the
        # extra P-matrix traffic + per-layer kernel tail made the end-to-end
        # bench 7% slower (16.8 vs 18.1 QPS) — the hand kernel with fused
        # online softmax is the default at any cache fill.
        self.decode_attn = (
            ops.decode_attention_bmm
            if os.environ.get("SENTIO_DECODE_ATTN") == "bmm"
            else ops.decode_attention)
        # Decode projections onto the model dimension (wo, down), fixed for
        # the model's lifetime for the same reason: the split-K hand GEMM
        # whose fp32 partials the following residual RMSNorm sums
        # (ops.linear_splitk + ops.rmsnorm_residual_partials), or hipBLASLt
        # + rmsnorm_residual.  The hand pair needs the GPU, no TP (the
        # row-parallel all-reduce wants the bf16 output), at most 32 rows
        # and a shape ops.decode_gemm_plan accepts.  SENTIO_DECODE_GEMM=lt
        # keeps the library path; wo / down route only that projection.
        self.splitk_wo, self.splitk_down = self._plan_decode_gemm()
        # Multi-token head prep (generator / verifier prefill, prefix and
        # suffix forwards, encoder, reranker), fixed for the model's
        # lifetime like the two choices above: one ops.prefill_qkv_prep
        # launch splits the QKV projection, applies RoPE and writes K/V
        # into the cache, where the legacy sequence ran three slice copies,
        # two rope launches and two indexed writes per layer.  It needs the
        # GPU, bf16 and a head dim that is a multiple of 8.
        # SENTIO_PREFILL_PREP=legacy keeps the old sequence.
        self.prefill_fused = (
            os.environ.get("SENTIO_PREFILL_PREP", "auto") != "legacy"
            and str(self.device).startswith("cuda")
            and self.dtype == torch.bfloat16
            and ops.hip_available()
            and cfg.head_dim % 8 == 0)

    def _plan_decode_gemm(self) -> tuple[bool, bool]:
        mode = os.environ.get("SENTIO_DECODE_GEMM", "auto")
        if (mode == "lt" or self.tp.enabled or not ops.hip_available()
                or not str(self.device).startswith("cuda")
                or self.dtype != torch.bfloat16):
            return False, False
        cfg = self.cfg
        wo = ops.decode_gemm_plan(32, cfg.dim,
                                  self.h_local * cfg.head_dim)[0] > 0
        down = ops.decode_gemm_plan(32, cfg.dim, cfg.ffn_dim)[0] > 0
        return wo and mode != "down", down and mode != "wo"

    # ----- core blocks -----
    def _prep_fused(self, pos: torch.Tensor | None, cache: KVCache | None,
                    S: int) -> bool:
        """Whether a forward_hidden call takes ops.prefill_qkv_prep: the
        construction-time choice, positions q_off + arange(S) (no explicit
        pos), and with a cache a causal multi-token forward into bf16 rows
        (S == 1 keeps the decode-attention branch, an FP8 cache its
        error)."""
        if not self.prefill_fused or pos is not None:
            return False
        if cache is None:
            return True
        return (S > 1 and self.cfg.causal and not cache.fp8
                and cache.k[0].dtype == torch.bfloat16
                and cache.k[0].is_cuda)

    def _attn_fused(self, qkv: torch.Tensor, cache: KVCache | None,
                    layer_idx: int, kv_lens: torch.Tensor | None,
                    q_off: int) -> torch.Tensor:
        """Head prep in one launch, then attention: against the cache rows
        just written (kv_lens: absolute lengths, set by forward_hidden), or
        over the contiguous k / v without a cache."""
        H, Hkv = self.h_local, self.hkv_local
        if cache is not None:
            kc, vc = cache.k[layer_idx], cache.v[layer_idx]
            q = ops.prefill_qkv_prep(qkv, self.rope_cos, self.rope_sin, q_off,
                                     H, Hkv, kc, vc)
            return ops.attention_cache(q, kc, vc, kv_lens, q_off, self.scale)
        q, k, v = ops.prefill_qkv_prep(qkv, self.rope_cos, self.rope_sin,
                                       q_off, H, Hkv)
        return ops.attention(q, k, v, causal=self.cfg.causal,
                             scale=self.scale, kv_lens=kv_lens)

    def _attn(self, x: torch.Tensor, layer: dict, pos: torch.Tensor | None,
              cache: KVCache | None, layer_idx: int,
              kv_lens: torch.Tensor | None, q_off: int = 0) -> torch.Tensor:
        """pos None: the fused head prep (forward_hidden decided, see
        _prep_fused); otherwise the rope / indexed-write sequence."""
        cfg = self.cfg
        B, S, d = x.shape
        hd = cfg.head_dim
        H, Hkv = self.h_local, self.hkv_local
        qkv = torch.nn.functional.linear(x.view(B * S, d), layer["wqkv"])
        qkv = qkv.view(B, S, -1)
        if pos is None:
            out = self._attn_fused(qkv, cache, layer_idx, kv_lens, q_off)
            out = linear_row_parallel(out.reshape(B * S, H * hd), layer["wo"],
                                      self.tp)
            return out.view(B, S, d)
        q_end = H * hd
        k_end = q_end + Hkv * hd
        q = qkv[..., :q_end].reshape(B, S, H, hd)
        k = qkv[..., q_end:k_end].reshape(B, S, Hkv, hd)
        v = qkv[..., k_end:].reshape(B, S, Hkv, hd)
        q = ops.rope_apply(q, self.rope_cos, self.rope_sin, pos)
        k = ops.rope_apply(k, self.rope_cos, self.rope_sin, pos)

        if cache is not None and cache.fp8:
            raise ValueError("prefill writes exact K/V: run it into a bf16 "
                             "staging KVCache and splice with "
                             "ops.kv_store_fp8")
        if cache is not None:
            # write k/v at pos into the cache: [B, Hkv_local, Smax, hd]
            kc, vc = cache.k[layer_idx], cache.v[layer_idx]
            idx = pos.long()  # [B,S]
            bidx = torch.arange(B, device=x.device).unsqueeze(1).expand(B, S)
            kc[bidx.reshape(-1), :, idx.reshape(-1)] = \
                k.reshape(B * S, Hkv, hd).to(kc.dtype)
            vc[bidx.reshape(-1), :, idx.reshape(-1)] = \
                v.reshape(B * S, Hkv, hd).to(vc.dtype)

        if S == 1 and cache is not None:
            seq_lens = (pos[:, 0] + 1).to(torch.int32)
            out = ops.decode_attention(
                q.view(B, H, hd), cache.k[layer_idx],
                cache.v[layer_idx], seq_lens, self.scale,
            ).view(B, 1, H, hd)
        elif cache is not None and q_off > 0:
            # prefix-KV-cached suffix prefill: attend to cache rows
            # [0, kv_lens[b]) — the prefix KV was computed once and copied
            # in; kv_lens carries per-row ABSOLUTE lengths (prefix + true
            # suffix length), masking right-pad keys out of shorter rows
            lens_abs = (kv_lens if kv_lens is not None
                        else torch.full((B,), q_off + S, dtype=torch.int32,
                                        device=x.device))
            out = ops.attention_cache(q, cache.k[layer_idx],
                                      cache.v[layer_idx], lens_abs,
                                      q_off, self.scale)
        else:
            out = ops.attention(q, k, v, causal=cfg.causal, scale=self.scale,
                                kv_lens=kv_lens)
        # row-parallel output projection: partial-sum all-reduce overlapped
        # chunk-wise with the GEMM (parallel/tp.py)
        out = linear_row_parallel(out.reshape(B * S, H * hd), layer["wo"],
                                  self.tp)
        return out.view(B, S, d)

    def _ffn(self, x: torch.Tensor, layer: dict) -> torch.Tensor:
        B, S, d = x.shape
        # measured: hipBLASLt's TN path beats the hand skinny_gemm kernel on
        # the decode gate_up shape in context (52 us, 4.5 TB/s, at B=32 with
        # the autotuned algorithm; the hand kernel took ~87 us), so decode
        # rows go through the autotuned-algorithm binding
        rows = B * S
        xx = x.view(rows, d)
        if rows <= 64 and self.device != "cpu":
            gu = ops.lt_linear(xx, layer["w_gate_up"])
            y = ops.swiglu_packed(gu)   # fused [gate|up] split + silu·up
            out = linear_row_parallel(y, layer["w_down"], self.tp,
                                      linear=ops.lt_linear)
        else:
            gu = torch.nn.functional.linear(xx, layer["w_gate_up"])
            y = ops.swiglu_packed(gu)
            out = linear_row_parallel(y, layer["w_down"], self.tp)
        return out.view(B, S, d)

    def forward_hidden(
        self, tokens: torch.Tensor, pos: torch.Tensor | None = None,
        cache: KVCache | None = None, kv_lens: torch.Tensor | None = None,
        q_off: int = 0,
    ) -> torch.Tensor:
        """tokens: [B, S] int64 → hidden [B, S, dim] (after final norm).
        kv_lens: right-padding valid lengths for non-causal batches.
        Residual adds are fused into the next block's RMSNorm
        (ops.rmsnorm_residual) — one kernel instead of add + norm.
        pos None: token (b, s) sits at position q_off + s; on the fused
        head-prep route (_prep_fused) no position tensor is built at all."""
        B, S = tokens.shape
        if self._prep_fused(pos, cache, S):
            if cache is not None and kv_lens is None:
                kv_lens = torch.full((B,), q_off + S, dtype=torch.int32,
                                     device=tokens.device)
        elif pos is None:
            pos = torch.arange(q_off, q_off + S, device=tokens.device
                               ).unsqueeze(0).expand(B, S)
        x = self.w.tok_emb[tokens.reshape(-1)].view(B, S, self.cfg.dim)
        eps = self.cfg.norm_eps
        layers = self.w.layers
        n = len(layers)
        normed = ops.rmsnorm(x, layers[0]["attn_norm"], eps)
        for i, layer in enumerate(layers):
            a = self._attn(normed, layer, pos, cache, i, kv_lens, q_off=q_off)
            normed, x = ops.rmsnorm_residual(a, x, layer["ffn_norm"], eps)
            f = self._ffn(normed, layer)
            w_next = layers[i + 1]["attn_norm"] if i + 1 < n else self.w.final_norm
            normed, x = ops.rmsnorm_residual(f, x, w_next, eps)
        return normed

    # ----- decode fast path: fused RoPE + KV-cache write + fused norms -----
    def _decode_fused(self, x: torch.Tensor) -> bool:
        """RoPE + KV write + attention in one launch: the hand kernel on the
        GPU.  The bmm variant and the CPU keep the two-op path."""
        return self.decode_attn is ops.decode_attention and x.is_cuda

    def _attn_decode(self, normed: torch.Tensor, layer: dict, cache: KVCache,
                     layer_idx: int,
                     attn_lens: torch.Tensor | None) -> torch.Tensor:
        B = normed.shape[0]
        out = self._attn_decode_heads(normed, layer, cache, layer_idx,
                                      attn_lens)
        out = linear_row_parallel(out, layer["wo"], self.tp,
                                  linear=ops.lt_linear)
        return out.view(B, 1, self.cfg.dim)

    def _attn_decode_heads(self, normed: torch.Tensor, layer: dict,
                           cache: KVCache, layer_idx: int,
                           attn_lens: torch.Tensor | None) -> torch.Tensor:
        """Decode attention up to the output projection: [B, H_local * hd]."""
        B = normed.shape[0]
        d = self.cfg.dim
        hd = self.cfg.head_dim
        qkv = ops.lt_linear(normed.view(B, d), layer["wqkv"])
        if cache.fp8:
            # FP8 cache: one launch as below, quantising the new row
            sc = cache.scales[layer_idx]
            out = ops.decode_attention_fused_fp8(
                qkv, cache.k[layer_idx], cache.v[layer_idx], self.rope_cos,
                self.rope_sin, cache.seq_lens, sc[0], sc[1], sc[2], sc[3],
                self.scale)
        elif self._decode_fused(qkv):
            # one launch: RoPE(q) in registers, KV row written and attended
            out = ops.decode_attention_fused(
                qkv, cache.k[layer_idx], cache.v[layer_idx], self.rope_cos,
                self.rope_sin, cache.seq_lens, self.scale)
        else:
            q = ops.decode_qkv_prep(qkv, cache.k[layer_idx],
                                    cache.v[layer_idx], self.rope_cos,
                                    self.rope_sin, cache.seq_lens)
            out = self.decode_attn(q, cache.k[layer_idx], cache.v[layer_idx],
                                   attn_lens, self.scale)
        return out.view(B, self.h_local * hd)

    def forward_decode(self, tokens: torch.Tensor, cache: KVCache) -> torch.Tensor:
        """One-token decode: tokens [B, 1] → hidden [B, 1, dim].  RoPE and
        the cache write ride in the decode-attention launch
        (ops.decode_attention_fused; decode_qkv_prep + attention on the bmm
        and CPU paths).  decode_step advances cache.seq_lens on device
        (hipGraph-capturable)."""
        B = tokens.shape[0]
        x = self.w.tok_emb[tokens.reshape(-1)].view(B, 1, self.cfg.dim)
        eps = self.cfg.norm_eps
        layers = self.w.layers
        n = len(layers)
        # the fused op takes the new token's position; only the two-op
        # path needs the key count
        attn_lens = (None if self._decode_fused(x) else cache.seq_lens + 1)
        normed = ops.rmsnorm(x, layers[0]["attn_norm"], eps)
        # B is fixed per captured graph, so this is a per-graph constant
        sk_wo = self.splitk_wo and B <= 32
        sk_down = self.splitk_down and B <= 32
        for i, layer in enumerate(layers):
            if sk_wo:
                a = ops.linear_splitk(
                    self._attn_decode_heads(normed, layer, cache, i,
                                            attn_lens), layer["wo"])
                normed, x = ops.rmsnorm_residual_partials(
                    a, x, layer["ffn_norm"], eps)
            else:
                a = self._attn_decode(normed, layer, cache, i, attn_lens)
                normed, x = ops.rmsnorm_residual(a, x, layer["ffn_norm"], eps)
            w_next = layers[i + 1]["attn_norm"] if i + 1 < n else self.w.final_norm
            if sk_down:
                gu = ops.lt_linear(normed.view(B, self.cfg.dim),
                                   layer["w_gate_up"])
                f = ops.linear_splitk(ops.swiglu_packed(gu), layer["w_down"])
                normed, x = ops.rmsnorm_residual_partials(f, x, w_next, eps)
            else:
                f = self._ffn(normed, layer)
                normed, x = ops.rmsnorm_residual(f, x, w_next, eps)
        return normed

    # ----- decoder-specific -----
    def logits(self, hidden: torch.Tensor,
               last_idx: torch.Tensor | None = None) -> torch.Tensor:
        """lm_head at each row's LAST REAL position.  last_idx [B] selects
        per-row positions for right-padded batches — without it, shorter
        prompts in a batch would be conditioned on their PAD tail."""
        B, S, d = hidden.shape
        if last_idx is None:
            last = hidden[:, -1, :]
        else:
            last = hidden[torch.arange(B, device=hidden.device),
                          last_idx.to(hidden.device).long()]
        if B <= 64 and self.device != "cpu":
            return ops.lt_linear(last.contiguous(), self.w.lm_head).float()
        return torch.nn.functional.linear(last, self.w.lm_head).float()  # [B, V]

    def prefill(self, tokens: torch.Tensor, cache: KVCache,
                lens: torch.Tensor | None = None) -> torch.Tensor:
        """Prefill the cache; returns last-real-position logits [B, V].
        lens: per-row true prompt lengths for right-padded batches — masks
        pad keys out of attention, starts decode at each row's own length,
        and gathers logits at lens-1 (batch composition no longer changes a
        request's output).  Touches no model state: safe to run on a side
        stream while decode replays."""
        B, S = tokens.shape
        lens_i = None if lens is None else lens.to(torch.int32)
        hidden = self.forward_hidden(tokens, cache=cache, kv_lens=lens_i)
        if lens_i is None:
            cache.seq_lens[:] = S
            last_idx = None
        else:
            cache.seq_lens.copy_(lens_i)
            last_idx = lens_i.long() - 1
        return self.logits(hidden, last_idx)

    def prefill_suffix(self, suffix_tokens: torch.Tensor, cache: KVCache,
                       prefix_len: int,
                       suffix_lens: torch.Tensor | None = None) -> torch.Tensor:
        """Prefill only the suffix against a cache whose rows [0, prefix_len)
        already hold the shared prefix's KV (prefix-KV caching).  Returns
        last-real-position logits; suffix_lens: per-row true suffix lengths
        for right-padded suffix batches."""
        B, S = suffix_tokens.shape
        lens_abs = (None if suffix_lens is None
                    else (suffix_lens.to(torch.int32) + prefix_len))
        # positions prefix_len + s follow from q_off
        hidden = self.forward_hidden(suffix_tokens, cache=cache,
                                     q_off=prefix_len, kv_lens=lens_abs)
        if lens_abs is None:
            cache.seq_lens[:] = prefix_len + S
            last_idx = None
        else:
            cache.seq_lens.copy_(lens_abs)
            last_idx = suffix_lens.long() - 1
        return self.logits(hidden, last_idx)

    def decode_step(self, tokens: torch.Tensor, cache: KVCache) -> torch.Tensor:
        """tokens: [B, 1] the latest sampled token; returns logits [B, V]."""
        hidden = self.forward_decode(tokens, cache)
        cache.seq_lens += 1
        return self.logits(hidden)
