"""Plain-PyTorch fp32 reference implementations of every HIP op.

These are (a) the CPU execution path for tests and the hermetic config, and
(b) the numerics references the GPU tests compare the gfx950 kernels against
(driver contract: numerics tests compare HIP kernels vs plain PyTorch fp32).
Shapes/semantics documented per-op; the HIP kernels implement exactly these.
"""

from __future__ import annotations

import math

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """y = x / rms(x) * weight over the last dim."""
    xf = x.float()
    rms = xf.pow(2).mean(dim=-1, keepdim=True).add(eps).rsqrt()
    return (xf * rms * weight.float()).to(x.dtype)


def rmsnorm_residual(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5
) -> tuple[torch.Tensor, torch.Tensor]:
    """h = x + residual;  y = rmsnorm(h).  Returns (y, h) — the fused
    residual-add + norm used between transformer blocks."""
    h = (x.float() + residual.float())
    rms = h.pow(2).mean(dim=-1, keepdim=True).add(eps).rsqrt()
    y = (h * rms * weight.float()).to(x.dtype)
    return y, h.to(x.dtype)


def linear_splitk(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Split-K partials of F.linear(x, w) as fp32 [S, M, N]; the reference
    has one slice."""
    return torch.nn.functional.linear(x.float(), w.float()).unsqueeze(0)


def rmsnorm_residual_partials(
    part: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor,
    eps: float = 1e-5
) -> tuple[torch.Tensor, torch.Tensor]:
    """rmsnorm_residual on the sum of fp32 partials [S, ..., D] over dim 0:
    h = sum_s part[s] + residual;  y = rmsnorm(h).  Returns (y, h) in the
    residual's dtype."""
    h = part.float().sum(dim=0).reshape(residual.shape) + residual.float()
    rms = h.pow(2).mean(dim=-1, keepdim=True).add(eps).rsqrt()
    y = (h * rms * weight.float()).to(residual.dtype)
    return y, h.to(residual.dtype)


def rope_tables(
    max_seq: int, head_dim: int, base: float = 500000.0, device: str = "cpu"
) -> tuple[torch.Tensor, torch.Tensor]:
    """Precomputed cos/sin tables [max_seq, head_dim/2] (fp32).
    base=500000 is the Llama-3 rope theta."""
    inv = 1.0 / (
        base ** (torch.arange(0, head_dim, 2, device=device).float() / head_dim)
    )
    t = torch.arange(max_seq, device=device).float()
    freqs = torch.outer(t, inv)
    return freqs.cos(), freqs.sin()


def rope_apply(
    x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor
) -> torch.Tensor:
    """Rotate pairs (x[2i], x[2i+1]) by position angles.

    x: [B, S, H, D]; cos/sin: [max_seq, D/2]; pos: [B, S] int32 positions.
    """
    B, S, H, D = x.shape
    c = cos[pos.long()].unsqueeze(2)  # [B,S,1,D/2]
    s = sin[pos.long()].unsqueeze(2)
    xf = x.float().view(B, S, H, D // 2, 2)
    x0, x1 = xf[..., 0], xf[..., 1]
    out = torch.stack((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1)
    return out.view(B, S, H, D).to(x.dtype)


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up."""
    return (torch.nn.functional.silu(gate.float()) * up.float()).to(gate.dtype)


def softmax(x: torch.Tensor, dim: int = -1) -> torch.Tensor:
    return torch.softmax(x.float(), dim=dim).to(x.dtype)


def attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    scale: float | None = None,
    kv_lens: torch.Tensor | None = None,
) -> torch.Tensor:
    """Reference multi-head attention with GQA.

    q: [B, S, H, D];  k, v: [B, S, Hkv, D] with H % Hkv == 0.
    kv_lens: optional [B] int — right-padding mask: keys at position >= len
    are ignored (encoder batches).  Returns [B, S, H, D].  Computed in fp32.
    """
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    rep = H // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf = q.float().permute(0, 2, 1, 3)  # [B,H,S,D]
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    scores = (qf @ kf.transpose(-1, -2)) * scale  # [B,H,S,S]
    if causal:
        mask = torch.full((S, S), float("-inf"), device=q.device).triu(1)
        scores = scores + mask
    if kv_lens is not None:
        key_valid = (
            torch.arange(S, device=q.device).view(1, 1, 1, S)
            < kv_lens.view(B, 1, 1, 1)
        )
        scores = scores.masked_fill(~key_valid, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    out = probs @ vf  # [B,H,S,D]
    return out.permute(0, 2, 1, 3).contiguous().to(q.dtype)


def decode_attention(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: float | None = None,
) -> torch.Tensor:
    """Single-token decode attention over a contiguous KV cache.

    q: [B, H, D] (the new token's query);
    k_cache/v_cache: [B, Hkv, Smax, D]; seq_lens: [B] valid lengths.
    Returns [B, H, D].
    """
    B, H, D = q.shape
    Hkv = k_cache.shape[1]
    rep = H // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    out = torch.empty(B, H, D, dtype=q.dtype, device=q.device)
    for b in range(B):
        s = int(seq_lens[b])
        kf = k_cache[b, :, :s].float().repeat_interleave(rep, dim=0)  # [H,s,D]
        vf = v_cache[b, :, :s].float().repeat_interleave(rep, dim=0)
        qs = q[b].float().unsqueeze(1)  # [H,1,D]
        p = torch.softmax((qs @ kf.transpose(-1, -2)) * scale, dim=-1)
        out[b] = (p @ vf).squeeze(1).to(q.dtype)
    return out


def mean_pool_l2norm(hidden: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Masked mean-pool over sequence then L2-normalize.

    hidden: [B, S, D]; mask: [B, S] (1 = real token). Returns [B, D] fp32.
    """
    m = mask.float().unsqueeze(-1)
    summed = (hidden.float() * m).sum(dim=1)
    counts = m.sum(dim=1).clamp_min(1.0)
    pooled = summed / counts
    return pooled / pooled.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def cosine_topk(
    q: torch.Tensor, mat: torch.Tensor, k: int
) -> tuple[torch.Tensor, torch.Tensor]:
    """q: [B, D] (normalized), mat: [N, D] (normalized rows).
    Returns (values [B,k] fp32, indices [B,k] int64)."""
    scores = q.float() @ mat.float().T
    return torch.topk(scores, k, dim=1)


def bm25_score(
    term_ids: torch.Tensor,
    indptr: torch.Tensor,
    post_doc: torch.Tensor,
    post_tf: torch.Tensor,
    idf: torch.Tensor,
    doc_len: torch.Tensor,
    n_docs: int,
    k1: float,
    b: float,
    avgdl: float,
    plus_delta: float = 0.0,
) -> torch.Tensor:
    """Dense BM25 scores over all docs for one query's term ids."""
    scores = torch.zeros(n_docs, dtype=torch.float32, device=term_ids.device)
    norm_den = k1 * (1.0 - b + b * doc_len.float() / avgdl)
    for tid in term_ids.tolist():
        lo, hi = int(indptr[tid]), int(indptr[tid + 1])
        docs = post_doc[lo:hi].long()
        tf = post_tf[lo:hi].float()
        contrib = tf * (k1 + 1.0) / (tf + norm_den[docs])
        if plus_delta:
            contrib = contrib + plus_delta
        scores.index_add_(0, docs, float(idf[tid]) * contrib)
    return scores


def sample_token(
    logits: torch.Tensor, temperature: float, generator: torch.Generator | None = None
) -> torch.Tensor:
    """logits: [B, V] → [B] int64 sampled (or argmax at T==0)."""
    if temperature <= 0.0:
        return logits.float().argmax(dim=-1)
    probs = torch.softmax(logits.float() / temperature, dim=-1)
    return torch.multinomial(probs, 1, generator=generator).squeeze(-1)


def sample_support_row(row: torch.Tensor, temperature: float, top_k: int,
                       top_p: float) -> dict:
    """Sort-based fp64 oracle for ONE row [V] of the top-k -> top-p support.

    Kept set = {v : logit_v >= tau}.  T <= 0: greedy, tau = row max.  T > 0:
    z = logit/T, p = softmax(z); -inf logits are dropped; 1 <= top_k < (number
    of finite logits) keeps the top_k largest; top_p < 1 keeps the shortest
    prefix of those whose cumulative mass reaches top_p * M_k (M_k = mass of
    the top-k survivors), never fewer than one token; tau is the raw logit
    of the last kept token and EVERY token tied with tau is kept.

    Returns tau plus the sorted values / cumulative masses the tests use for
    their margin conditions (`vals`, `cs` normalised by the total row mass,
    `target` in the same unit, `n` the prefix length)."""
    x = row.detach().cpu().to(torch.float64).flatten()
    x = torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)
    xmax = float(x.max())
    if not (temperature > 0.0) or math.isinf(xmax):
        return {"tau": xmax, "greedy": True}
    vals = torch.sort(x[x > -math.inf], descending=True).values
    w = torch.exp((vals - vals[0]) / float(temperature))
    total = float(w.sum())
    n = vals.numel()
    if 1 <= top_k < n:
        n = int(top_k)
    cs = torch.cumsum(w, 0) / total
    target = None
    if top_p < 1.0:
        target = float(top_p) * float(cs[n - 1])
        idx = int(torch.searchsorted(cs[:n], torch.tensor(target,
                                                          dtype=torch.float64)))
        n = min(max(idx + 1, 1), n)
    return {"tau": float(vals[n - 1]), "greedy": False, "vals": vals,
            "cs": cs, "target": target, "n": n}


def _row_params(B: int, temperature, top_k, top_p):
    def bc(v, dtype):
        t = torch.as_tensor(v).detach().cpu().to(dtype).flatten()
        return t.expand(B) if t.numel() == 1 else t

    return (bc(temperature, torch.float32), bc(top_k, torch.int64),
            bc(top_p, torch.float32))


def sample_support(logits: torch.Tensor, temperature, top_k, top_p):
    """logits [B, V] -> (tau [B] f32, count [B] i32); see sample_support_row.
    Parameters are per-row [B] (scalars broadcast) and read at fp32, like the
    kernel reads them."""
    x = logits.detach().cpu().float()
    B = x.shape[0]
    t, k, p = _row_params(B, temperature, top_k, top_p)
    tau = torch.empty(B, dtype=torch.float32)
    for b in range(B):
        tau[b] = sample_support_row(x[b], float(t[b]), int(k[b]),
                                    float(p[b]))["tau"]
    xc = torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)
    count = (xc >= tau[:, None]).sum(dim=1).to(torch.int32)
    return tau, count


def sample_filtered(logits: torch.Tensor, temperature, top_k, top_p, seed,
                    step) -> torch.Tensor:
    """logits [B, V] -> [B] int64: mask to the support, then one draw per row
    from a generator seeded from (seed_b, step_b) alone -- a row's token does
    not depend on its position or on B.  Greedy rows take the lowest index of
    the maximum."""
    x = logits.detach().cpu().float()
    B = x.shape[0]
    t, _, _ = _row_params(B, temperature, top_k, top_p)
    sd = torch.as_tensor(seed).detach().cpu().to(torch.int64).flatten()
    st = torch.as_tensor(step).detach().cpu().to(torch.int64).flatten()
    sd = sd.expand(B) if sd.numel() == 1 else sd
    st = st.expand(B) if st.numel() == 1 else st
    tau, _ = sample_support(x, temperature, top_k, top_p)
    out = torch.empty(B, dtype=torch.int64)
    for b in range(B):
        row = torch.where(torch.isnan(x[b]), torch.full_like(x[b], -math.inf),
                          x[b])
        T = float(t[b])
        if not (T > 0.0) or math.isinf(float(row.max())):
            out[b] = int(row.argmax())
            continue
        z = (row.double() - float(row.max())) / T
        z = torch.where(row >= tau[b], z, torch.full_like(z, -math.inf))
        g = torch.Generator(device="cpu")
        g.manual_seed(((int(sd[b]) * 0x9E3779B1) ^ (int(st[b]) * 0x85EBCA6B
                                                   + 0x27D4EB2F))
                      & 0x7FFFFFFFFFFFFFFF)
        out[b] = int(torch.multinomial(torch.softmax(z, 0), 1, generator=g))
    return out


def sample_slots(logits: torch.Tensor, slot, temperature, top_k, top_p, seed,
                 step: torch.Tensor, active, tok: torch.Tensor) -> None:
    """sample_filtered over a slot table, in place on `step` and `tok`.

    logits [R, V]; slot [R] ints or None (None: R == S, row r is slot r);
    temperature / top_k / top_p / seed / step / tok are [S]; active [S] or
    None.  Row r belongs to slot s = slot[r].  A slot outside [0, S) or with
    active[s] == 0 is skipped: tok[s] and step[s] keep their values.
    Otherwise tok[s] = sample_filtered(logits[r], params[s], seed[s],
    step[s]) and step[s] += 1."""
    R, S = logits.shape[0], tok.shape[0]
    slots = list(range(R)) if slot is None \
        else [int(s) for s in torch.as_tensor(slot).flatten().tolist()]
    if len(slots) != R:
        raise ValueError(f"{len(slots)} slots for {R} logits rows")
    for r, s in enumerate(slots):
        if s < 0 or s >= S or (active is not None and int(active[s]) == 0):
            continue
        tok[s] = sample_filtered(logits[r:r + 1], temperature[s:s + 1],
                                 top_k[s:s + 1], top_p[s:s + 1],
                                 seed[s:s + 1], step[s:s + 1])[0]
        step[s] += 1


def constrained_allowed(state: int, left: int, V: int, nxt: torch.Tensor,
                        mask: torch.Tensor, dist: torch.Tensor) -> torch.Tensor:
    """bool [V]: the tokens a row in automaton state `state` with `left`
    tokens remaining may pick.  v is allowed iff v < min(V, Vt), bit v of
    mask[state] is set and dist[next[state, v]] <= left - 1."""
    Vt = nxt.shape[1]
    Vc = min(V, Vt)
    v = torch.arange(Vc)
    words = mask[state].to(torch.int64)[v >> 5]
    bit = ((words >> (v & 31)) & 1).bool()
    to = nxt[state, :Vc].to(torch.int64)
    ok = bit & (to >= 0)
    ok &= dist.to(torch.int64)[to.clamp_min(0)] <= int(left) - 1
    out = torch.zeros(V, dtype=torch.bool)
    out[:Vc] = ok
    return out


def _constrained_row(row, t, k, p, sd, st, state: int, left: int, nxt, mask,
                     dist):
    """One row of sample_constrained -> (token, new state, new left)."""
    N = nxt.shape[0]
    if state < 0 or state >= N:
        return int(sample_filtered(row[None], t, k, p, sd, st)[0]), state, left
    ok = constrained_allowed(state, left, row.shape[0], nxt, mask, dist)
    if not bool(ok.any()):
        return 0, state, left
    x = row.detach().cpu().float()
    masked = torch.where(ok, x, torch.full_like(x, -math.inf))
    finite = torch.isfinite(masked) | (masked == math.inf)
    if not bool(finite.any()):
        tok = int(torch.nonzero(ok)[0])      # lowest allowed index
    else:
        tok = int(sample_filtered(masked[None], t, k, p, sd, st)[0])
    return tok, int(nxt[state, tok]), left - 1


def sample_constrained(logits, temperature, top_k, top_p, seed, step,
                       state: torch.Tensor, left: torch.Tensor, nxt, mask,
                       dist) -> torch.Tensor:
    """Grammar-constrained sample_filtered, in place on `state` and `left`
    (int32 [B]).  Disallowed logits (constrained_allowed) count as -inf, the
    rest is sample_filtered; then state = next[state, tok], left -= 1.  A
    row whose allowed logits are all -inf / NaN takes the lowest allowed
    index.  A row with state outside [0, N) is sampled by sample_filtered
    over the whole row and keeps state and left."""
    x = logits.detach().cpu().float()
    B = x.shape[0]
    t, k, p = _row_params(B, temperature, top_k, top_p)
    sd = torch.as_tensor(seed).detach().cpu().to(torch.int64).flatten()
    st = torch.as_tensor(step).detach().cpu().to(torch.int64).flatten()
    sd = sd.expand(B) if sd.numel() == 1 else sd
    st = st.expand(B) if st.numel() == 1 else st
    out = torch.empty(B, dtype=torch.int64)
    for b in range(B):
        tok, ns, nl = _constrained_row(
            x[b], t[b:b + 1], k[b:b + 1], p[b:b + 1], sd[b:b + 1],
            st[b:b + 1], int(state[b]), int(left[b]), nxt, mask, dist)
        out[b] = tok
        state[b] = ns
        left[b] = nl
    return out


def sample_slots_constrained(logits, slot, temperature, top_k, top_p, seed,
                             step, active, tok, state, left, nxt, mask,
                             dist) -> None:
    """sample_slots with per-slot automaton state: slot s samples through
    sample_constrained with (state[s], left[s]), all in place."""
    R, S = logits.shape[0], tok.shape[0]
    slots = list(range(R)) if slot is None \
        else [int(s) for s in torch.as_tensor(slot).flatten().tolist()]
    if len(slots) != R:
        raise ValueError(f"{len(slots)} slots for {R} logits rows")
    for r, s in enumerate(slots):
        if s < 0 or s >= S or (active is not None and int(active[s]) == 0):
            continue
        tok[s] = sample_constrained(
            logits[r:r + 1], temperature[s:s + 1], top_k[s:s + 1],
            top_p[s:s + 1], seed[s:s + 1], step[s:s + 1], state[s:s + 1],
            left[s:s + 1], nxt, mask, dist)[0]
        step[s] += 1


def decode_qkv_prep(
    qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    cos: torch.Tensor, sin: torch.Tensor, seq_lens: torch.Tensor
) -> torch.Tensor:
    """CPU reference of the fused decode head prep (see ops.decode_qkv_prep):
    splits the raw S=1 QKV projection, RoPE-rotates q and k, writes k/v into
    the caches at row seq_lens[b], returns q [B, H, D]."""
    B = qkv.shape[0]
    Hkv, smax, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    H = qkv.shape[1] // D - 2 * Hkv
    pos = seq_lens.long().view(B, 1)
    q = qkv[:, : H * D].view(B, 1, H, D)
    k = qkv[:, H * D : (H + Hkv) * D].view(B, 1, Hkv, D)
    v = qkv[:, (H + Hkv) * D :].view(B, 1, Hkv, D)
    q = rope_apply(q, cos, sin, pos)
    k = rope_apply(k, cos, sin, pos)
    b_idx = torch.arange(B)
    k_cache[b_idx, :, seq_lens.long()] = k.view(B, Hkv, D).to(k_cache.dtype)
    v_cache[b_idx, :, seq_lens.long()] = v.view(B, Hkv, D).to(v_cache.dtype)
    return q.view(B, H, D)


def prefill_qkv_prep(
    qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: int,
    n_heads: int, n_kv_heads: int,
    k_cache: torch.Tensor | None = None, v_cache: torch.Tensor | None = None,
):
    """Reference of ops.prefill_qkv_prep: the split / rope_apply / indexed
    cache write sequence the fused kernel replaces.  qkv [B, S, (H+2Hkv)*D],
    token (b, s) at position pos0 + s.  With caches [Bc, Hkv, Smax, D]:
    writes RoPE(k) and v to rows pos0 .. pos0+S-1 of batch rows < B and
    returns q [B, S, H, D]; without: returns (q, k, v), k and v
    [B, S, Hkv, D]."""
    B, S, W = qkv.shape
    H, Hkv = n_heads, n_kv_heads
    D = W // (H + 2 * Hkv)
    q_end = H * D
    k_end = q_end + Hkv * D
    pos = (pos0 + torch.arange(S, device=qkv.device)).unsqueeze(0).expand(B, S)
    q = qkv[..., :q_end].reshape(B, S, H, D)
    k = qkv[..., q_end:k_end].reshape(B, S, Hkv, D)
    v = qkv[..., k_end:].reshape(B, S, Hkv, D)
    q = rope_apply(q, cos, sin, pos)
    k = rope_apply(k, cos, sin, pos)
    if k_cache is None:
        return q, k, v.contiguous()
    bidx = torch.arange(B, device=qkv.device).unsqueeze(1).expand(B, S)
    k_cache[bidx.reshape(-1), :, pos.reshape(-1)] = \
        k.reshape(B * S, Hkv, D).to(k_cache.dtype)
    v_cache[bidx.reshape(-1), :, pos.reshape(-1)] = \
        v.reshape(B * S, Hkv, D).to(v_cache.dtype)
    return q


def decode_attention_fused(
    qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    cos: torch.Tensor, sin: torch.Tensor, seq_lens: torch.Tensor,
    scale: float | None = None,
) -> torch.Tensor:
    """CPU reference of ops.decode_attention_fused: decode_qkv_prep (writes
    the k/v row at seq_lens[b]) followed by decode_attention over
    seq_lens[b] + 1 keys."""
    q = decode_qkv_prep(qkv, k_cache, v_cache, cos, sin, seq_lens)
    return decode_attention(q, k_cache, v_cache, seq_lens + 1, scale)


# ---- FP8 (e4m3fn) KV cache: uint8 storage, static fp32 scales per kv head
FP8_E4M3_MAX = 448.0


def _per_head(s: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """[Hkv] scale broadcast over x [..., Hkv, S, D]."""
    s = torch.as_tensor(s, dtype=torch.float32, device=x.device)
    return s.view(-1, 1, 1) if s.dim() == 1 else s


def kv_quantize(x: torch.Tensor, inv: torch.Tensor) -> torch.Tensor:
    """The quantisation spec: byte = RNE_e4m3fn(clamp(fp32(x) * inv, ±448)).
    x [..., Hkv, S, D]; inv [Hkv] (or broadcastable) reciprocal scales.
    Returns uint8.  The clamp is part of the spec: the bare cast yields NaN
    above 464."""
    y = (x.float() * _per_head(inv, x)).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def kv_dequantize(b: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn bytes [..., Hkv, S, D] * scale [Hkv] -> fp32."""
    return b.view(torch.float8_e4m3fn).float() * _per_head(scale, b)


def kv_store_fp8(src_k: torch.Tensor, src_v: torch.Tensor,
                 k_cache: torch.Tensor, v_cache: torch.Tensor, rows, S: int,
                 k_inv: torch.Tensor, v_inv: torch.Tensor) -> None:
    """Quantising splice: the first S rows of src [n, Hkv, S_src, D] go to
    cache[rows[i], :, :S] of the uint8 caches; rows outside [0, B) are
    skipped."""
    B = k_cache.shape[0]
    rows = [int(r) for r in (rows.tolist() if isinstance(rows, torch.Tensor)
                             else rows)]
    for i, r in enumerate(rows):
        if 0 <= r < B:
            k_cache[r, :, :S] = kv_quantize(src_k[i, :, :S], k_inv)
            v_cache[r, :, :S] = kv_quantize(src_v[i, :, :S], v_inv)


def decode_attention_fused_fp8(
    qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    cos: torch.Tensor, sin: torch.Tensor, seq_lens: torch.Tensor,
    k_scale: torch.Tensor, v_scale: torch.Tensor, k_inv: torch.Tensor,
    v_inv: torch.Tensor, scale: float | None = None,
) -> torch.Tensor:
    """CPU reference of ops.decode_attention_fused_fp8: the new k/v row
    (RoPE'd, in qkv's dtype) is quantised into the uint8 caches at row
    seq_lens[b]; attention then runs over the DEQUANTISED seq_lens[b] + 1
    keys, so the new token is seen as later steps will read it."""
    B = qkv.shape[0]
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    H = qkv.shape[1] // D - 2 * Hkv
    pos = seq_lens.long()
    q = rope_apply(qkv[:, : H * D].view(B, 1, H, D), cos, sin,
                   pos.view(B, 1)).view(B, H, D)
    k_new = rope_apply(qkv[:, H * D : (H + Hkv) * D].view(B, 1, Hkv, D),
                       cos, sin, pos.view(B, 1)).to(qkv.dtype)
    v_new = qkv[:, (H + Hkv) * D :].view(B, 1, Hkv, D)
    b_idx = torch.arange(B)
    # [B, 1, Hkv, D] -> [B, Hkv, 1, D] for the per-head scales
    k_cache[b_idx, :, pos] = kv_quantize(k_new.transpose(1, 2), k_inv)[:, :, 0]
    v_cache[b_idx, :, pos] = kv_quantize(v_new.transpose(1, 2), v_inv)[:, :, 0]
    return decode_attention(q, kv_dequantize(k_cache, k_scale),
                            kv_dequantize(v_cache, v_scale), seq_lens + 1,
                            scale)


def swiglu_packed(gu: torch.Tensor) -> torch.Tensor:
    """gu [..., 2F] rows packed [gate | up] → silu(gate) * up, [..., F]."""
    f = gu.shape[-1] // 2
    return swiglu(gu[..., :f], gu[..., f:])


def attention_cache(
    q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    kv_lens: torch.Tensor, q_off: int, scale: float | None = None,
) -> torch.Tensor:
    """Suffix-against-cache causal attention (prefix-KV-cached prefill).
    q: [B, S_suf, H, D] at absolute positions q_off + i;
    k_cache/v_cache: [B, Hkv, Smax, D]; kv_lens: [B] absolute lengths."""
    B, S, H, D = q.shape
    Hkv = k_cache.shape[1]
    rep = H // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    out = torch.empty_like(q, dtype=torch.float32)
    for b in range(B):
        L = int(kv_lens[b])
        kf = k_cache[b, :, :L].float().repeat_interleave(rep, dim=0)  # [H,L,D]
        vf = v_cache[b, :, :L].float().repeat_interleave(rep, dim=0)
        qf = q[b].float().permute(1, 0, 2)                            # [H,S,D]
        sc = (qf @ kf.transpose(-1, -2)) * scale                      # [H,S,L]
        pos = q_off + torch.arange(S).view(1, S, 1)
        key = torch.arange(L).view(1, 1, L)
        sc = sc.masked_fill(key > pos, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[b] = (p @ vf).permute(1, 0, 2)
    return out.to(q.dtype)
