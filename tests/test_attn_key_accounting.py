"""Exact key accounting for the prefill and decode attention kernels.

The other attention tests draw randn inputs and compare at rtol = atol =
3e-2, which is a third of the signal or more once a few hundred keys share
the softmax: a dropped tile, a causal horizon or length off by one, or one
stale cache row all pass.  Here every op is compared with an fp64 softmax
over an explicit allowed-key mask, on inputs where one miscounted key is
far outside the bound.

Input families (one (batch, kv-head) slab of N keys, D dims):

* uniform A / B ("counting"): q = 0 and K = 0, so every allowed key scores
  exactly 0, P = exp(0) = 1, l = n and the output is count_d / n, where V
  carries the key's identity: A: V[j, d] = [d == j % D]; B: V[j, d] =
  [d == (j // 16) % D].  Every intermediate is exact in fp32; the only
  roundings are the fp32 divide (or multiply by the reciprocal) and the
  bf16 store, so |got - want| <= 2^-7 |want| (one bf16 ulp), and exactly 0
  where count_d == 0.  Shapes keep count_d <= 32, so one key more or less
  in a column (1/n against 2^-7 * 32/n) is at least four times the bound.
* staircase: q[..., 0] = 1, K[j, 0] = s_j, scale = 1, so the scores are the
  small integers s_j = 0..7..0 over 16-key groups (period 256 keys): the
  running max moves inside a 64-key tile, across tiles, waves and decode
  splits.  V is pattern A.
* random: randn q / K / V (rounded to bf16), unequal B, S, H, Hkv, D, the
  default scale: transposes and the GQA head mapping.

Poison: every K / V row that no query of its batch row may attend (at or
past the length, past the last query's causal horizon, past the new token,
a cache batch row beyond q's batch) holds V = 64 in every dimension and
K[j, 0] = 8 -- finite, since the kernels multiply masked keys by P = 0.

Bound for staircase and random inputs.  With p the fp64 softmax weights,
    |got - want| <= 2^-8 * (sum_j p_j |v_j| + |want|).
The prefill kernel rounds P to bf16 before the PV MFMA and the output to
bf16 at the store.  A bf16 rounding moves x by at most 2^-9 |x| at the top
of a binade and 2^-8 |x| at its bottom, so the first contributes at most
2^-8 sum_j p_j |v_j| and the second at most 2^-8 |want|: the bound is the
worst case of both together (twice their sum at the top of the binades),
reached only if every term of an element sits at the bottom of its binade
and errs in one direction.  The denominator l is summed from the unrounded
fp32 P; fp32 accumulation and __expf at these arguments are 2^-20 and
below.  The decode kernels keep P in fp32 and are held to the same bound.

The CPU tests at the top prove the comparison is sensitive, on the
reference alone; the gpu-marked tests run the kernels.
"""

import functools
import math
from typing import NamedTuple

import pytest
import torch

gpu = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
POISON_V, POISON_K = 64.0, 8.0
UNIFORM = ("A", "B")
KINDS = ("A", "B", "stair", "rand")


# ---------------------------------------------------------------- harness

class Case(NamedTuple):
    kind: str
    q: torch.Tensor          # [B, Q, H, D] fp64, values exact in bf16
    k: torch.Tensor          # [B, Hkv, N, D]
    v: torch.Tensor          # [B, Hkv, N, D]
    allowed: torch.Tensor    # [B, Q, N] bool: query (b, i) attends key j
    scale: float | None      # as passed to the op (None: 1/sqrt(D))


def key_mask(B, Q, N, lens=None, causal=False, q_off=0, dh=0, dl=0):
    """allowed[b, i, j] = j < lens[b] + dl, and when causal j <= q_off[b] +
    i + dh for a query that sits inside the N rows (q_off[b] + i < N; a
    token past the cache attends nothing).  dh / dl shift the horizon / the
    length: the off-by-one mutations."""
    lens = torch.full((B,), N) if lens is None else torch.as_tensor(lens)
    q_off = torch.as_tensor(q_off).expand(B)
    j = torch.arange(N).view(1, 1, N)
    i = torch.arange(Q).view(1, Q, 1)
    ok = (j < lens.view(B, 1, 1) + dl).expand(B, Q, N)
    if causal:
        pos = q_off.view(B, 1, 1) + i
        ok = ok & (j <= pos + dh) & (pos < N)
    return ok.clone()


def pattern_v(N, D, pat):
    j = torch.arange(N)
    col = j % D if pat == "A" else (j // 16) % D
    v = torch.zeros(N, D, dtype=F64)
    v[j, col] = 1.0
    return v


def staircase(N):
    g = (torch.arange(N) // 16) % 16
    return torch.where(g < 8, g, 15 - g).to(F64)


def make_case(kind, H, Hkv, D, allowed, seed=0):
    """Inputs of one family under `allowed` [B, Q, N], poison applied."""
    B, Q, N = allowed.shape
    q = torch.zeros(B, Q, H, D, dtype=F64)
    k = torch.zeros(B, Hkv, N, D, dtype=F64)
    scale = None
    if kind in UNIFORM:
        v = pattern_v(N, D, kind).expand(B, Hkv, N, D).clone()
    elif kind == "stair":
        q[..., 0] = 1.0
        k[..., 0] = staircase(N)
        v = pattern_v(N, D, "A").expand(B, Hkv, N, D).clone()
        scale = 1.0
    else:
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(B, Q, H, D, generator=g).to(BF16).to(F64)
        k = torch.randn(B, Hkv, N, D, generator=g).to(BF16).to(F64)
        v = torch.randn(B, Hkv, N, D, generator=g).to(BF16).to(F64)
    unseen = ~allowed.any(dim=1)                      # [B, N]
    k[..., 0] = torch.where(unseen[:, None, :], POISON_K, k[..., 0])
    v = torch.where(unseen[:, None, :, None], POISON_V, v)
    return Case(kind, q, k, v, allowed, scale)


def reference(case, weight=None):
    """fp64 softmax attention over the allowed keys -> (want, mag), both
    [B, Q, H, D]; mag = sum_j p_j |v_j|.  `weight` [B, Q, N] replaces the
    0 / 1 mask (a mutation: 0 drops a key, 2 counts it twice).  A query
    with no allowed key gives zeros."""
    B, Q, H, D = case.q.shape
    rep = H // case.k.shape[1]
    w = (case.allowed if weight is None else weight).to(F64)[:, None]
    kf = case.k.repeat_interleave(rep, dim=1)         # [B, H, N, D]
    vf = case.v.repeat_interleave(rep, dim=1)
    scale = case.scale if case.scale is not None else 1.0 / math.sqrt(D)
    sc = torch.einsum("bqhd,bhnd->bhqn", case.q, kf) * scale
    sc = sc.masked_fill(w == 0, float("-inf"))
    m = sc.amax(dim=-1, keepdim=True)
    m = m.masked_fill(torch.isneginf(m), 0.0)
    e = w * torch.exp(sc - m)
    den = e.sum(dim=-1, keepdim=True)
    p = e / den.masked_fill(den == 0, 1.0)
    want, mag = p @ vf, p @ vf.abs()
    return want.permute(0, 2, 1, 3), mag.permute(0, 2, 1, 3)


def tolerance(kind, want, mag):
    if kind in UNIFORM:
        return 2.0 ** -7 * want.abs()
    return 2.0 ** -8 * (mag + want.abs())


def assert_within(got, want, tol, what=""):
    err = (got.to(F64) - want).abs()
    bad = ~(err <= tol)                               # NaN counts as bad
    if bad.any():
        over = torch.where(bad, err - tol, torch.zeros_like(err))
        idx = tuple(int(x) for x in
                    torch.unravel_index(over.argmax(), over.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside "
            f"the bound; worst at [b, i, h, d] = {idx}: got "
            f"{float(got[idx]):.6g}, want {float(want[idx]):.6g}, bound "
            f"{float(tol[idx]):.3g}")


def expected(case):
    """(want, bound) of a case."""
    want, mag = reference(case)
    return want, tolerance(case.kind, want, mag)


def check(case, got, what="", ref=None):
    want, tol = ref if ref is not None else expected(case)
    assert_within(got.reshape(want.shape), want, tol, what)


def max_count(case):
    """Largest count_d of a uniform case (the 32 of the docstring)."""
    return float((case.allowed.to(F64)[:, None] @ case.v).max())


# ---- the families, one builder per op.  The decode ones are shared by the
# split / wave settings: built once with their reference, never modified.

def attn_case(kind, D, S, H, Hkv, causal, with_lens, zero_row=False):
    """ops.attention: B = 3, kv_lens = S, a ragged middle value and 1."""
    lens = None
    if with_lens:
        lens = torch.tensor([S, 0 if zero_row else max(1, S // 2 + 1), 1])
    allowed = key_mask(3, S, S, lens, causal)
    return make_case(kind, H, Hkv, D, allowed, seed=D + S + H), lens


CACHE_SMAX, CACHE_H, CACHE_HKV = 200, 8, 2


def cache_case(kind, D, q_off, S):
    """ops.attention_cache: B = 3 of a 4-row cache of Smax = 200; kv_lens
    = q_off + S, a padded suffix (q_off + 3) and q_off + 1."""
    lens = torch.tensor([q_off + S, q_off + min(3, S), q_off + 1])
    allowed = key_mask(3, S, CACHE_SMAX, lens, True, q_off)
    return make_case(kind, CACHE_H, CACHE_HKV, D, allowed,
                     seed=D + q_off + S), lens


DEC_B, DEC_HKV, DEC_SMAX = 7, 2, 768
DEC_LENS = (1, 31, 32, 33, 257, 700, 768)
DEC_POS = (1, 31, 32, 33, 257, 700, 767)


@functools.lru_cache(maxsize=16)
def decode_case(kind, D, G):
    lens = torch.tensor(DEC_LENS)
    allowed = key_mask(DEC_B, 1, DEC_SMAX, lens)
    case = make_case(kind, G * DEC_HKV, DEC_HKV, D, allowed, seed=D + G)
    return case, lens, expected(case)


@functools.lru_cache(maxsize=16)
def step_case(kind, D, G, T):
    """The fused decode forms: T new tokens per row at positions p + t
    (T = 1: decode_attention_fused), token t attending keys 0 .. p + t.
    The case holds the caches as they are AFTER the call."""
    pos = torch.tensor(DEC_POS)
    allowed = key_mask(DEC_B, T, DEC_SMAX, None, True, pos)
    case = make_case(kind, G * DEC_HKV, DEC_HKV, D, allowed)
    return case, pos, expected(case)


def step_inputs(case, pos, T):
    """(qkv [B*T, (H+2Hkv)*D], k, v before the call): q and k segments zero
    (RoPE of zero is zero), the v segment the pattern row of key p + t (64
    for a token past the cache: it is nobody's key), cache rows from p
    upward poisoned."""
    B, _, H, D = case.q.shape
    Hkv, N = case.k.shape[1], case.k.shape[2]
    qkv = torch.zeros(B, T, H + 2 * Hkv, D, dtype=F64)
    k, v = case.k.clone(), case.v.clone()
    for b in range(B):
        p = int(pos[b])
        for t in range(T):
            qkv[b, t, H + Hkv:] = (case.v[b, :, p + t] if p + t < N
                                   else POISON_V)
        k[b, :, p:, 0] = POISON_K
        v[b, :, p:] = POISON_V
    return qkv.view(B * T, -1), k, v


# ------------------------------------------- CPU: the harness is sensitive

def _busiest(allowed):
    """(b, i) of the query with the most allowed keys."""
    n = allowed.sum(-1)
    b, i = divmod(int(n.argmax()), n.shape[1])
    return b, i


def _mut_drop_one(spec, allowed):
    b, i = _busiest(allowed)
    js = allowed[b, i].nonzero().flatten()
    w = allowed.to(F64)
    w[b, i, js[len(js) // 2]] = 0
    return w


def _mut_swap(delta):
    def mut(spec, allowed):
        b, i = _busiest(allowed)
        row = allowed[b, i]
        both = (row[:-delta] & row[delta:]).nonzero().flatten()
        if both.numel() == 0:
            return None
        j = int(both[len(both) // 2])
        w = allowed.to(F64)
        w[b, i, j], w[b, i, j + delta] = 0, 2
        return w
    return mut


def _mut_admit_poison(spec, allowed):
    unseen = ~allowed.any(dim=1)
    live = allowed.any(dim=-1)
    for b in range(allowed.shape[0]):
        if unseen[b].any() and live[b].any():
            w = allowed.to(F64)
            i = int(live[b].nonzero()[-1])
            w[b, i, int(unseen[b].nonzero()[0])] = 1
            return w
    return None


def _mut_shift(**shift):
    def mut(spec, allowed):
        if "dh" in shift and not spec.get("causal"):
            return None
        other = key_mask(**spec, **shift)
        return None if torch.equal(other, allowed) else other.to(F64)
    return mut


def _mut_drop_group(spec, allowed):
    b, i = _busiest(allowed)
    row = allowed[b, i]
    full = row[:row.numel() // 16 * 16].view(-1, 16).all(-1).nonzero()
    if full.numel() == 0:
        return None
    g = int(full.flatten()[len(full) // 2])
    w = allowed.to(F64)
    w[b, i, 16 * g:16 * g + 16] = 0
    return w


MUTATIONS = {
    "drop_one": _mut_drop_one,
    "swap_16": _mut_swap(16),
    "swap_64": _mut_swap(64),
    "admit_poison": _mut_admit_poison,
    "horizon_plus": _mut_shift(dh=1),
    "horizon_minus": _mut_shift(dh=-1),
    "len_plus": _mut_shift(dl=1),
    "len_minus": _mut_shift(dl=-1),
    "drop_group": _mut_drop_group,
}

# (H, Hkv, D, key_mask arguments): one shape per op form and edge
CPU_SHAPES = {
    "attn_full_d32": (4, 2, 32, dict(B=3, Q=200, N=200)),
    "attn_lens_d96": (6, 2, 96, dict(B=3, Q=65, N=65, lens=(65, 33, 1))),
    "attn_causal_d128": (1, 1, 128, dict(B=3, Q=129, N=129, causal=True)),
    "attn_causal_lens_d64": (4, 2, 64, dict(B=3, Q=200, N=200, causal=True,
                                            lens=(200, 101, 1))),
    "attn_tiny": (4, 2, 64, dict(B=3, Q=1, N=1, causal=True)),
    "cache_d64": (8, 2, 64, dict(B=3, Q=70, N=200, causal=True, q_off=65,
                                 lens=(135, 68, 66))),
    "cache_full_d128": (8, 2, 128, dict(B=3, Q=70, N=200, causal=True,
                                        q_off=130, lens=(200, 133, 131))),
    "decode_d64": (14, 2, 64, dict(B=7, Q=1, N=768, lens=DEC_LENS)),
    "fused_d128": (8, 2, 128, dict(B=7, Q=1, N=768, causal=True,
                                   q_off=torch.tensor(DEC_POS))),
    "verify_d64": (2, 2, 64, dict(B=7, Q=5, N=768, causal=True,
                                  q_off=torch.tensor(DEC_POS))),
}


def _rejects(case, weight):
    """Whether check() refuses the reference computed under `weight`,
    rounded to bf16 as a kernel would store it."""
    mutant, _ = reference(case, weight)
    try:
        check(case, mutant.to(BF16))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("shape", list(CPU_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_harness_accepts_rounded_reference(shape, kind):
    H, Hkv, D, spec = CPU_SHAPES[shape]
    case = make_case(kind, H, Hkv, D, key_mask(**spec), seed=5)
    want, _ = reference(case)
    assert torch.isfinite(want).all()
    check(case, want.to(BF16), shape)
    if kind in UNIFORM:
        assert max_count(case) <= 32


@pytest.mark.parametrize("shape", list(CPU_SHAPES))
def test_harness_rejects_every_mutation(shape):
    """Patterns A and B together see every mutation that applies to the
    shape (a 64-key swap is invisible to A at D = 64, visible to B)."""
    H, Hkv, D, spec = CPU_SHAPES[shape]
    allowed = key_mask(**spec)
    cases = [make_case(kind, H, Hkv, D, allowed) for kind in UNIFORM]
    applied = 0
    for name, mutate in MUTATIONS.items():
        w = mutate(spec, allowed)
        if w is None:
            continue
        applied += 1
        assert not torch.equal(w, allowed.to(F64)), name
        assert any(_rejects(c, w) for c in cases), f"{shape}: {name} passes"
    assert applied >= 2, shape


def test_every_mutation_applies_to_some_shape():
    seen = set()
    for H, Hkv, D, spec in CPU_SHAPES.values():
        allowed = key_mask(**spec)
        seen |= {n for n, m in MUTATIONS.items()
                 if m(spec, allowed) is not None}
    assert seen == set(MUTATIONS)


@pytest.mark.parametrize("shape", ["attn_causal_lens_d64", "cache_d64",
                                   "decode_d64"])
def test_harness_staircase_and_random_sensitivity(shape):
    """The derived bound still refuses an admitted poison row (score 8
    against a staircase top of 7; V = 64) and, on the staircase, a dropped
    group at the top of the stairs."""
    H, Hkv, D, spec = CPU_SHAPES[shape]
    allowed = key_mask(**spec)
    for kind in ("stair", "rand"):
        case = make_case(kind, H, Hkv, D, allowed, seed=9)
        assert _rejects(case, _mut_admit_poison(spec, allowed)), kind
    stair = make_case("stair", H, Hkv, D, allowed)
    b, i = _busiest(allowed)
    w = allowed.to(F64)
    w[b, i, 112:128] = 0                    # s_j = 7: the first top step
    assert allowed[b, i, 112:128].all() and _rejects(stair, w)


def test_staircase_shape():
    s = staircase(512)
    assert s[:16].eq(0).all() and s[112:144].eq(7).all()
    assert s[240:272].eq(0).all() and s.max() == 7
    assert torch.equal(s[:256], s[256:])
    # every 64-key tile sees its running max move
    assert all(len(s[t:t + 64].unique()) == 4 for t in range(0, 512, 64))


def test_reference_matches_torch_ref():
    """The fp64 reference and ops.torch_ref agree on what each op means."""
    from sentio_amd.ops import torch_ref as R

    case, lens = attn_case("rand", 32, 17, 6, 2, True, True)
    want, _ = reference(case)
    got = R.attention(case.q.float(), case.k.permute(0, 2, 1, 3).float(),
                      case.v.permute(0, 2, 1, 3).float(), True, None, lens)
    torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-5)

    case, lens = cache_case("rand", 64, 65, 17)
    want, _ = reference(case)
    got = R.attention_cache(case.q.float(), case.k.float(), case.v.float(),
                            lens, 65)
    torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-5)

    case, lens, (want, _) = decode_case("rand", 64, 1)
    got = R.decode_attention(case.q[:, 0].float(), case.k.float(),
                             case.v.float(), lens)
    torch.testing.assert_close(got.double(), want[:, 0], rtol=1e-4,
                               atol=1e-5)


@pytest.mark.parametrize("T", [1, 5])
def test_step_inputs_reproduce_the_case_on_the_reference_ops(T):
    """The fused-form inputs, run through torch_ref, leave the caches of
    the case behind and give its outputs: the construction is right."""
    from sentio_amd.ops import torch_ref as R

    D, G = 64, 1
    case, pos, ref = step_case("B", D, G, T)
    qkv, k, v = step_inputs(case, pos, T)
    cos, sin = R.rope_tables(DEC_SMAX, D)
    k, v, p32 = k.float(), v.float(), pos.to(torch.int32)
    if T == 1:
        got = R.decode_attention_fused(qkv.float(), k, v, cos, sin, p32)
    else:
        got = R.decode_attention_verify(qkv.float(), k, v, cos, sin, p32, T)
    check(case, got.view(DEC_B, T, G * DEC_HKV, D), ref=ref)
    assert torch.equal(k.double(), case.k) and torch.equal(v.double(), case.v)


def test_rows_without_keys_are_zero_on_the_reference():
    from sentio_amd import ops

    torch.manual_seed(0)
    B, S, H, Hkv, D = 3, 5, 4, 2, 8
    q, k, v = (torch.randn(B, S, h, D) for h in (H, Hkv, Hkv))
    lens = torch.tensor([S, 0, 1], dtype=torch.int32)
    out = ops.attention(q, k, v, causal=False, kv_lens=lens)
    assert torch.isfinite(out).all() and out[1].eq(0).all()
    assert not out[0].eq(0).any() and not out[2].eq(0).any()
    full = ops.attention(q, k, v, causal=False)
    torch.testing.assert_close(out[0], full[0])

    kc = k.permute(0, 2, 1, 3).contiguous()
    vc = v.permute(0, 2, 1, 3).contiguous()
    out = ops.attention_cache(q, kc, vc, lens, 0)
    assert torch.isfinite(out).all() and out[1].eq(0).all()
    causal = ops.attention(q, k, v, causal=True)
    torch.testing.assert_close(out[0], causal[0])


# ------------------------------------- CPU: the wrappers refuse bad calls

def _attn_args():
    B, S, H, Hkv, D = 2, 6, 4, 2, 32
    return dict(q=torch.zeros(B, S, H, D), k=torch.zeros(B, S, Hkv, D),
                v=torch.zeros(B, S, Hkv, D),
                kv_lens=torch.tensor([6, 3], dtype=torch.int32))


ATTN_BAD = {
    "q_3d": (dict(q=torch.zeros(2, 6, 128)), "q must"),
    "q_empty": (dict(q=torch.zeros(2, 0, 4, 32)), "q must"),
    "k_3d": (dict(k=torch.zeros(2, 6, 64)), "k must"),
    "kv_differ": (dict(v=torch.zeros(2, 6, 1, 32)), "k and v"),
    "kv_batch": (dict(k=torch.zeros(1, 6, 2, 32),
                      v=torch.zeros(1, 6, 2, 32)), "k and v"),
    "kv_seq": (dict(k=torch.zeros(2, 5, 2, 32),
                    v=torch.zeros(2, 5, 2, 32)), "k and v"),
    "kv_dim": (dict(k=torch.zeros(2, 6, 2, 64),
                    v=torch.zeros(2, 6, 2, 64)), "k and v"),
    "heads_indivisible": (dict(k=torch.zeros(2, 6, 3, 32),
                               v=torch.zeros(2, 6, 3, 32)), "do not divide"),
    "more_kv_heads": (dict(k=torch.zeros(2, 6, 8, 32),
                           v=torch.zeros(2, 6, 8, 32)), "do not divide"),
    "lens_short": (dict(kv_lens=torch.tensor([6], dtype=torch.int32)),
                   "kv_lens"),
    "lens_long": (dict(kv_lens=torch.tensor([6, 3, 1])), "kv_lens"),
    "lens_float": (dict(kv_lens=torch.tensor([6.0, 3.0])), "kv_lens"),
    "lens_2d": (dict(kv_lens=torch.tensor([[6, 3]])), "kv_lens"),
    "lens_list": (dict(kv_lens=[6, 3]), "kv_lens"),
}


@pytest.mark.parametrize("bad", list(ATTN_BAD))
def test_attention_rejects(bad):
    from sentio_amd import ops

    change, match = ATTN_BAD[bad]
    a = {**_attn_args(), **change}
    with pytest.raises(ValueError, match=match):
        ops.attention(a["q"], a["k"], a["v"], causal=False,
                      kv_lens=a["kv_lens"])


def _cache_args():
    B, S, H, Hkv, D, Smax = 2, 3, 4, 2, 32, 16
    return dict(q=torch.zeros(B, S, H, D), kc=torch.zeros(3, Hkv, Smax, D),
                vc=torch.zeros(3, Hkv, Smax, D),
                kv_lens=torch.tensor([8, 6], dtype=torch.int32), q_off=5)


_KC = torch.zeros(3, 2, 16, 32)

CACHE_BAD = {
    "q_3d": (dict(q=torch.zeros(2, 3, 128)), "q must"),
    "q_empty": (dict(q=torch.zeros(0, 3, 4, 32)), "q must"),
    "cache_3d": (dict(kc=torch.zeros(3, 2, 512)), "k_cache must"),
    "caches_differ": (dict(vc=torch.zeros(3, 2, 8, 32)), "caches must both"),
    "cache_rows": (dict(kc=torch.zeros(1, 2, 16, 32),
                        vc=torch.zeros(1, 2, 16, 32)), "batch rows"),
    "cache_dim": (dict(kc=torch.zeros(3, 2, 16, 64),
                       vc=torch.zeros(3, 2, 16, 64)), "caches must both"),
    "cache_strided": (dict(kc=torch.zeros(3, 2, 32, 32)[:, :, ::2]),
                      "k_cache must be a contiguous"),
    "cache_transposed": (dict(vc=torch.zeros(3, 16, 2, 32).transpose(1, 2)),
                         "v_cache must be a contiguous"),
    "cache_dtype": (dict(kc=_KC.to(torch.bfloat16),
                         vc=_KC.to(torch.bfloat16)), "k_cache must"),
    "heads_indivisible": (dict(kc=torch.zeros(3, 3, 16, 32),
                               vc=torch.zeros(3, 3, 16, 32)),
                          "do not divide"),
    "more_kv_heads": (dict(kc=torch.zeros(3, 8, 16, 32),
                           vc=torch.zeros(3, 8, 16, 32)), "do not divide"),
    "lens_short": (dict(kv_lens=torch.tensor([8], dtype=torch.int32)),
                   "kv_lens"),
    "lens_float": (dict(kv_lens=torch.tensor([8.0, 6.0])), "kv_lens"),
    "lens_none": (dict(kv_lens=None), "kv_lens"),
    "q_off_negative": (dict(q_off=-1), "q_off"),
}


@pytest.mark.parametrize("bad", list(CACHE_BAD))
def test_attention_cache_rejects(bad):
    from sentio_amd import ops

    change, match = CACHE_BAD[bad]
    a = {**_cache_args(), **change}
    with pytest.raises(ValueError, match=match):
        ops.attention_cache(a["q"], a["kc"], a["vc"], a["kv_lens"],
                            a["q_off"])


def test_wrappers_accept_the_good_calls():
    """The base arguments of the rejection tests are themselves valid, with
    int64 lengths too, a bigger cache batch and no kv_lens."""
    from sentio_amd import ops

    a = _attn_args()
    assert ops.attention(a["q"], a["k"], a["v"], causal=True).shape == \
        a["q"].shape
    ops.attention(a["q"], a["k"], a["v"], kv_lens=a["kv_lens"].long())
    c = _cache_args()
    out = ops.attention_cache(c["q"], c["kc"], c["vc"], c["kv_lens"].long(),
                              c["q_off"])
    assert out.shape == c["q"].shape


# ------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sentio_amd import ops

    assert ops.hip_available(), (
        "HIP extension must be built/loaded on a GPU box — no eager fallback")
    return "cuda:0"


def _bf(t, dev):
    return t.to(BF16).contiguous().to(dev)


ATTN_SHAPES = [(D, S, 4, 2) for D in (32, 64, 96, 128)
               for S in (1, 16, 17, 64, 65, 129, 200)]
ATTN_SHAPES += [(D, S, H, Hkv) for D in (64, 96) for S in (17, 129)
                for H, Hkv in ((1, 1), (6, 2))]
MASKS = [(False, False), (False, True), (True, False), (True, True)]


def _run_attention(case, lens, causal, dev):
    from sentio_amd import ops

    return ops.attention(
        _bf(case.q, dev), _bf(case.k.permute(0, 2, 1, 3), dev),
        _bf(case.v.permute(0, 2, 1, 3), dev), causal=causal,
        scale=case.scale,
        kv_lens=None if lens is None else lens.to(torch.int32).to(dev)).cpu()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("causal,with_lens", MASKS)
@pytest.mark.parametrize("D,S,H,Hkv", ATTN_SHAPES)
def test_attention_key_accounting(dev, D, S, H, Hkv, causal, with_lens, kind):
    """Every query row is compared, the rows past kv_lens[b] too."""
    case, lens = attn_case(kind, D, S, H, Hkv, causal, with_lens)
    got = _run_attention(case, lens, causal, dev)
    check(case, got, f"attention {kind}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,S", [(64, 65), (96, 17)])
def test_attention_row_without_keys_is_zero(dev, D, S, kind):
    case, lens = attn_case(kind, D, S, 4, 2, False, True, zero_row=True)
    assert int(lens[1]) == 0
    got = _run_attention(case, lens, False, dev)
    assert got[1].eq(0).all()
    check(case, got, f"attention {kind}, kv_lens {lens.tolist()}")


CACHE_SHAPES = [(D, q_off, S) for D in (64, 128)
                for q_off in (0, 1, 63, 64, 65, 130) for S in (1, 17, 64, 70)]


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,q_off,S", CACHE_SHAPES)
def test_attention_cache_key_accounting(dev, D, q_off, S, kind):
    """Smax = 200 (no multiple of the 64-key tile; 130 + 70 fills it), one
    poisoned cache batch row more than q has, everything at or past
    kv_lens[b] poisoned."""
    from sentio_amd import ops

    case, lens = cache_case(kind, D, q_off, S)
    assert q_off + S <= CACHE_SMAX and int(lens.max()) <= CACHE_SMAX
    extra_k = torch.zeros(1, CACHE_HKV, CACHE_SMAX, D, dtype=F64)
    extra_k[..., 0] = POISON_K
    extra_v = torch.full((1, CACHE_HKV, CACHE_SMAX, D), POISON_V, dtype=F64)
    kc = _bf(torch.cat([case.k, extra_k]), dev)
    vc = _bf(torch.cat([case.v, extra_v]), dev)
    got = ops.attention_cache(_bf(case.q, dev), kc, vc,
                              lens.to(torch.int32).to(dev), q_off,
                              scale=case.scale).cpu()
    check(case, got, f"attention_cache {kind}, kv_lens {lens.tolist()}")


@gpu
def test_attention_gpu_only_checks(dev):
    """dtype and head size are refused by the wrapper before a launch."""
    from sentio_amd import ops

    q = torch.zeros(1, 4, 2, 64, dtype=BF16, device=dev)
    lens = torch.tensor([4], dtype=torch.int32, device=dev)
    kc = torch.zeros(1, 2, 8, 64, dtype=BF16, device=dev)
    with pytest.raises(ValueError, match="bf16"):
        ops.attention(q.half(), q.half(), q.half())
    with pytest.raises(ValueError, match="bf16"):
        ops.attention(q, q, q.float())
    with pytest.raises(ValueError, match="bf16"):
        ops.attention_cache(q.float(), kc.float(), kc.float(), lens, 0)
    q48 = torch.zeros(1, 4, 2, 48, dtype=BF16, device=dev)
    kc48 = torch.zeros(1, 2, 8, 48, dtype=BF16, device=dev)
    with pytest.raises(ValueError, match="head dim"):
        ops.attention(q48, q48, q48)
    with pytest.raises(ValueError, match="head dim"):
        ops.attention_cache(q48, kc48, kc48, lens, 0)
    with pytest.raises(ValueError, match="kv_lens"):
        ops.attention(q, q, q, kv_lens=lens.cpu())


# ---- decode family

SPLITS = [None, "1", "3"]
WAVES = ["4", "8"]
HEADS = [(128, 4), (64, 7), (64, 1)]
VERIFY = [(D, G, T) for D, G in HEADS for T in (2, 5, 8) if G * T <= 32]


def _set_env(monkeypatch, splits, waves):
    if splits is None:
        monkeypatch.delenv("SENTIO_DECODE_SPLITS", raising=False)
    else:
        monkeypatch.setenv("SENTIO_DECODE_SPLITS", splits)
    monkeypatch.setenv("SENTIO_DECODE_WAVES", waves)


@gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,G", HEADS)
def test_decode_attention_key_accounting(dev, monkeypatch, D, G, kind, splits,
                                         waves):
    from sentio_amd import ops

    _set_env(monkeypatch, splits, waves)
    case, lens, ref = decode_case(kind, D, G)
    got = ops.decode_attention(_bf(case.q[:, 0], dev), _bf(case.k, dev),
                               _bf(case.v, dev),
                               lens.to(torch.int32).to(dev),
                               scale=case.scale).cpu()
    check(case, got, f"decode_attention {kind}", ref)


def _rope(D, dev):
    from sentio_amd import ops

    cos, sin = ops.torch_ref.rope_tables(DEC_SMAX, D)
    return cos.to(dev), sin.to(dev)


@gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("kind", UNIFORM)
@pytest.mark.parametrize("D,G", HEADS)
def test_decode_fused_key_accounting(dev, monkeypatch, D, G, kind, splits,
                                     waves):
    """Output count / (p + 1); afterwards the caches hold the new row at p
    and the poison everywhere above it."""
    from sentio_amd import ops

    _set_env(monkeypatch, splits, waves)
    case, pos, ref = step_case(kind, D, G, 1)
    qkv, k, v = step_inputs(case, pos, 1)
    kc, vc = _bf(k, dev), _bf(v, dev)
    got = ops.decode_attention_fused(_bf(qkv, dev), kc, vc, *_rope(D, dev),
                                     pos.to(torch.int32).to(dev)).cpu()
    check(case, got, f"decode_attention_fused {kind}", ref)
    assert torch.equal(kc.cpu().double(), case.k)
    assert torch.equal(vc.cpu().double(), case.v)


@gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("kind", UNIFORM)
@pytest.mark.parametrize("D,G", HEADS)
def test_decode_fused_fp8_key_accounting(dev, monkeypatch, D, G, kind, splits,
                                         waves):
    """All scales 1.0: 0, 1, 8 and 64 are exact in e4m3."""
    from sentio_amd import ops
    from sentio_amd.ops.torch_ref import kv_dequantize, kv_quantize

    _set_env(monkeypatch, splits, waves)
    case, pos, ref = step_case(kind, D, G, 1)
    qkv, k, v = step_inputs(case, pos, 1)
    one = torch.ones(DEC_HKV)
    kc, vc = kv_quantize(k, one).to(dev), kv_quantize(v, one).to(dev)
    one_d = one.to(dev)
    got = ops.decode_attention_fused_fp8(
        _bf(qkv, dev), kc, vc, *_rope(D, dev), pos.to(torch.int32).to(dev),
        one_d, one_d, one_d, one_d).cpu()
    check(case, got, f"decode_attention_fused_fp8 {kind}", ref)
    assert torch.equal(kv_dequantize(kc.cpu(), one).double(), case.k)
    assert torch.equal(kv_dequantize(vc.cpu(), one).double(), case.v)


@gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("kind", UNIFORM)
@pytest.mark.parametrize("D,G,T", VERIFY)
def test_decode_verify_key_accounting(dev, monkeypatch, D, G, T, kind, splits,
                                      waves):
    """Token t counts keys 0 .. p + t.  In the last row (p = 767) the
    tokens from t = 1 sit past the cache: zero output rows, nothing
    written."""
    from sentio_amd import ops

    _set_env(monkeypatch, splits, waves)
    case, pos, ref = step_case(kind, D, G, T)
    qkv, k, v = step_inputs(case, pos, T)
    kc, vc = _bf(k, dev), _bf(v, dev)
    got = ops.decode_attention_verify(_bf(qkv, dev), kc, vc, *_rope(D, dev),
                                      pos.to(torch.int32).to(dev), T).cpu()
    got = got.view(DEC_B, T, G * DEC_HKV, D)
    assert got[-1, 1:].eq(0).all()
    check(case, got, f"decode_attention_verify {kind}", ref)
    assert torch.equal(kc.cpu().double(), case.k)
    assert torch.equal(vc.cpu().double(), case.v)
