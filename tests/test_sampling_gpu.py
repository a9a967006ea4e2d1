"""Per-row top-k / top-p / seeded sampling on the MI355X: the HIP nucleus
kernel (ops.sample_support / ops.sample_filtered) against the sort-based fp64
oracle in ops.torch_ref, and the engine / continuous-batcher plumbing.

Margins.  The exact (bit-equal tau) tests state a CONDITION on their inputs,
asserted on the CPU before the kernel runs: at the boundary value group the
oracle's cumulative mass (row mass normalised to 1) is >= 1e-4 away from the
target on both sides, and the boundary logit is >= 1e-4 away from its
neighbouring distinct values.  When the boundary group is the TOP group there
is no earlier boundary (the prefix always holds one token), so only the
upper side applies.  Rows decided by count alone (top_p == 1) are integer
logic and carry no mass condition.  An fp32 cumsum of the same sorted masses
stays within 1e-5 of the fp64 one (checked), 10x inside the margin.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

VOCABS = (3, 1000, 1001, 4608, 128256, 152064)
MARGIN = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


# ---------------------------------------------------------------- inputs

def geometric_rows(B: int, V: int, seed: int) -> torch.Tensor:
    """LLM-like peaked rows: a random permutation of logit_r = -0.05*r for
    ranks r < 200, about -30 for the rest, plus 1e-3 jitter."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(B):
        r = torch.arange(V, dtype=torch.float32)
        base = torch.where(r < 200, -0.05 * r, torch.full_like(r, -30.0))
        base = base + 1e-3 * torch.randn(V, generator=g)
        rows.append(base[torch.randperm(V, generator=g)])
    return torch.stack(rows).contiguous()


def param_sets(V: int):
    """Two B=8 parameter sets; together they cover every T, top_k and top_p
    value of the issue, each filter alone and both combined."""
    a = [(0.0, 0, 1.0), (0.3, 0, 0.9), (0.7, 50, 0.9), (1.0, V + 5, 0.5),
         (2.0, 1, 1.0), (1.0, 50, 1.0), (0.7, 0, 1e-6), (2.0, 50, 0.95)]
    b = [(1.0, 0, 1.0), (0.3, 50, 0.5), (2.0, 0, 0.9), (0.7, V + 5, 0.95),
         (1.0, 1, 0.5), (0.0, 50, 0.9), (2.0, 50, 1e-6), (1.0, 50, 0.95)]
    return a, b


def _tensors(params):
    t = torch.tensor([p[0] for p in params], dtype=torch.float32)
    k = torch.tensor([p[1] for p in params], dtype=torch.int32)
    p_ = torch.tensor([p[2] for p in params], dtype=torch.float32)
    return t, k, p_


def assert_margin(row: torch.Tensor, ref: dict, what: str) -> None:
    """The input condition of the exact tests (module docstring)."""
    if ref["greedy"] or ref["target"] is None:
        return
    vals, cs, target, tau = ref["vals"], ref["cs"], ref["target"], ref["tau"]
    first = int((vals > tau).sum())            # boundary group = [first, last]
    last = int((vals >= tau).sum()) - 1
    through = float(cs[last])
    assert through - target >= MARGIN, (what, "upper", through, target)
    if first > 0:
        before = float(cs[first - 1])
        assert target - before >= MARGIN, (what, "lower", before, target)
        assert float(vals[first - 1]) - tau >= MARGIN, (what, "gap above")
    if last + 1 < vals.numel():
        assert tau - float(vals[last + 1]) >= MARGIN, (what, "gap below")
    # fp32 accumulation of the same masses stays far inside the margin
    w = torch.diff(cs, prepend=torch.zeros(1, dtype=cs.dtype))
    cs32 = torch.cumsum(w.float(), 0).double()
    assert float((cs32 - cs).abs().max()) < MARGIN / 10, what


_CASES: dict = {}


def support_case(V: int, which: int, bf16: bool):
    """(logits [8,V] cpu f32, params, oracle rows) -- computed once."""
    key = (V, which, bf16)
    if key not in _CASES:
        from sentio_amd.ops import torch_ref

        x = geometric_rows(8, V, seed=1000 + 17 * V % 9973 + which)
        if bf16:
            x = x.to(torch.bfloat16).float()
        params = param_sets(V)[which]
        refs = [torch_ref.sample_support_row(x[b], float(torch.tensor(
            params[b][0], dtype=torch.float32)), params[b][1], float(
            torch.tensor(params[b][2], dtype=torch.float32)))
            for b in range(8)]
        for b in range(8):
            assert_margin(x[b], refs[b], f"V={V} set={which} row={b}")
        _CASES[key] = (x, params, refs)
    return _CASES[key]


def check_support(dev, x, params, refs):
    from sentio_amd import ops

    t, k, p = _tensors(params)
    tau, count = ops.sample_support(x.to(dev), t, k, p)
    tau, count = tau.cpu(), count.cpu()
    for b, ref in enumerate(refs):
        want = torch.tensor(ref["tau"], dtype=torch.float32)
        assert tau[b].view(torch.int32) == want.view(torch.int32), (
            b, params[b], float(tau[b]), ref["tau"])
        if not ref["greedy"]:
            assert int(count[b]) == int((x[b] >= tau[b]).sum()), (b, params[b])


# ---------------------------------------------------------------- 1, 2

@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("V", VOCABS)
def test_support_exact_peaked(dev, V, which):
    check_support(dev, *support_case(V, which, bf16=False))


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("V", VOCABS)
def test_support_exact_ties(dev, V, which):
    """bf16-rounded logits: ties are the normal case; every token tied with
    tau is kept, so count may exceed top_k."""
    check_support(dev, *support_case(V, which, bf16=True))


def test_support_exact_ties_random_normal(dev):
    from sentio_amd.ops import torch_ref

    g = torch.Generator().manual_seed(4242)
    V = 128256
    x = torch.randn(1, V, generator=g).to(torch.bfloat16).float()
    assert torch.unique(x).numel() < V // 10          # heavily tied
    for params in ((1.0, 0, 0.9), (0.7, 50, 0.9), (1.0, 2000, 0.5),
                   (1.0, 50, 1.0)):
        ref = torch_ref.sample_support_row(x[0], params[0], params[1],
                                           float(torch.tensor(
                                               params[2],
                                               dtype=torch.float32)))
        assert_margin(x[0], ref, f"randn bf16 {params}")
        check_support(dev, x, [params], [ref])


# ---------------------------------------------------------------- 3

def test_support_wide_nucleus(dev):
    """3*randn rows keep ~11.6k tokens at top_p = 0.95 and cross the target
    within ~1e-6 of a token boundary, so the kernel's count n is bounded
    instead: cs[n-1] >= top_p - eps and cs[n-2] < top_p + eps with
    eps = V * 2^-24, the worst-case error of an fp32 sum of V non-negative
    terms totalling <= 1 in any order."""
    from sentio_amd import ops

    V, B, top_p = 128256, 4, 0.95
    g = torch.Generator().manual_seed(77)
    x = 3.0 * torch.randn(B, V, generator=g)
    tau, count = ops.sample_support(x.to(dev), 1.0, 0, top_p)
    tau, count = tau.cpu(), count.cpu()
    eps = V * 2.0 ** -24
    p32 = float(torch.tensor(top_p, dtype=torch.float32))
    for b in range(B):
        vals = torch.sort(x[b].double(), descending=True).values
        w = torch.exp(vals - vals[0])
        cs = torch.cumsum(w, 0) / w.sum()
        n = int(count[b])
        assert 9000 < n < 14000, n
        assert n == int((x[b] >= tau[b]).sum())
        assert float(cs[n - 1]) >= p32 - eps, (b, n, float(cs[n - 1]))
        assert float(cs[n - 2]) < p32 + eps, (b, n, float(cs[n - 2]))


# ---------------------------------------------------------------- 4

@pytest.mark.parametrize("V", VOCABS)
def test_tokens_inside_support(dev, V):
    from sentio_amd import ops

    for which in (0, 1):
        x, params, refs = support_case(V, which, bf16=False)
        t, k, p = _tensors(params)
        xd = x.to(dev)
        seed = torch.arange(8, dtype=torch.int64) + 100
        toks = torch.stack([
            ops.sample_filtered(xd, t, k, p, seed,
                                torch.full((8,), s, dtype=torch.int32))
            for s in range(32)]).cpu()                       # [32, 8]
        for b, ref in enumerate(refs):
            got = x[b][toks[:, b]]
            assert bool((got >= ref["tau"]).all()), (V, which, b)
            T, kk, pp = params[b]
            if T == 0.0 or kk == 1 or pp == 1e-6:
                first_max = int((x[b] == x[b].max()).nonzero()[0])
                assert bool((toks[:, b] == first_max).all()), (V, which, b)


def test_greedy_lowest_index_on_ties(dev):
    from sentio_amd import ops

    x = torch.zeros(3, 1001)
    x[0, [900, 17, 400]] = 5.0
    x[1, [1000, 999]] = 2.0
    x[2, :] = float("-inf")
    x[2, [3, 800]] = -1.0
    for T, k, p in ((0.0, 0, 1.0), (1.0, 1, 1.0)):
        # top_k = 1 keeps every token tied with the maximum: only T = 0 pins
        # the lowest index, top_k = 1 must stay inside the tie group
        tok = ops.sample_filtered(x.to(dev), T, k, p, 5, 0).cpu().tolist()
        if T == 0.0:
            assert tok == [17, 999, 3]
        else:
            assert tok[0] in (900, 17, 400) and tok[1] in (1000, 999) \
                and tok[2] in (3, 800)


# ---------------------------------------------------------------- 5

@pytest.mark.parametrize("vary", ("seed", "step"))
@pytest.mark.parametrize("top_k,top_p", ((0, 1.0), (8, 0.9)))
def test_distribution(dev, top_k, top_p, vary):
    """N fixed draws against the softmax renormalised over the oracle's
    support: max |freq - p| < 5 * 0.5 / sqrt(N) (five standard deviations of
    a binomial proportion; deterministic -- the seeds are fixed)."""
    from sentio_amd import ops
    from sentio_amd.ops import torch_ref

    V, N = 1000, 16384
    row = geometric_rows(1, V, seed=5)[0]
    ref = torch_ref.sample_support_row(row, 1.0, top_k, float(torch.tensor(
        top_p, dtype=torch.float32)))
    keep = row.double() >= ref["tau"]
    want = torch.softmax(torch.where(keep, row.double(),
                                     torch.full((V,), -math.inf,
                                                dtype=torch.float64)), 0)
    x = row.to(dev).expand(N, V).contiguous()
    ar = torch.arange(N, dtype=torch.int64)
    if vary == "seed":
        seed, step = ar, torch.zeros(N, dtype=torch.int32)
    else:
        seed, step = torch.full((N,), 1234, dtype=torch.int64), ar.int()
    tok = ops.sample_filtered(x, 1.0, top_k, top_p, seed, step).cpu()
    assert bool(keep[tok].all())                    # never outside the support
    freq = torch.bincount(tok, minlength=V).double() / N
    dev_max = float((freq - want).abs().max())
    print(f"top_k={top_k} top_p={top_p} vary={vary}: max dev {dev_max:.5f}")
    assert dev_max < 5 * 0.5 / math.sqrt(N)


# ---------------------------------------------------------------- 5b

_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def kernel_hash(seed: int, step: int, v: int) -> int:
    """The kernel's counter hash of (seed, step, v), in plain integers."""
    rk = _mix64((seed & _M64) ^ _mix64((step & 0xFFFFFFFF)
                                       + 0x9E3779B97F4A7C15))
    k0, k1, m = rk & 0xFFFFFFFF, rk >> 32, 0xFFFFFFFF
    x = (v ^ k0) & m
    x = (x * 0x9E3779B1) & m; x ^= x >> 16
    x = (x * 0x85EBCA6B) & m; x ^= x >> 13
    x ^= k1
    x = (x * 0xC2B2AE35) & m; x ^= x >> 16
    x = (x * 0x27D4EB2F) & m; x ^= x >> 15
    return x


@pytest.mark.parametrize("seed,v_top", ((548, 3121), (5581, 4575),
                                        (7490, 3877)))
def test_largest_hash_value_is_finite_noise(dev, seed, v_top):
    """(seed, step 0, v_top) hashes to the largest 24-bit value.  The
    uniform built from it must stay below 1: at u == 1 the Gumbel noise is
    +inf and v_top wins whatever its logit.  Here v_top sits 30 below every
    other token but inside the support (filters off); its noise is at most
    -log(2^-24) = 16.6, so it cannot win."""
    from sentio_amd import ops

    V = 4608
    assert kernel_hash(seed, 0, v_top) >> 8 == 0xFFFFFF
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(1, V, generator=g)
    x[0, v_top] = -30.0
    tau, _ = ops.sample_support(x.to(dev), 1.0, 0, 1.0)
    assert float(tau[0]) == -30.0                       # v_top is kept
    tok = int(ops.sample_filtered(x.to(dev), 1.0, 0, 1.0, seed, 0)[0])
    assert tok != v_top


# ---------------------------------------------------------------- 6

def test_row_and_batch_invariance(dev):
    from sentio_amd import ops

    V = 4608
    g = torch.Generator().manual_seed(9)
    row = torch.randn(V, generator=g)
    T, k, p, seed = 1.0, 0, 1.0, 11

    def run(B, pos, seed_, step0):
        x = 2.0 * torch.randn(B, V, generator=g)
        x[pos] = row
        t = torch.rand(B, generator=g) + 0.5
        kk = torch.randint(0, 100, (B,), generator=g, dtype=torch.int32)
        pp = torch.rand(B, generator=g) * 0.5 + 0.5
        sd = torch.randint(0, 1 << 40, (B,), generator=g)
        t[pos], kk[pos], pp[pos], sd[pos] = T, k, p, seed_
        xd = x.to(dev)
        out = []
        for s in range(16):
            st = torch.randint(0, 1000, (B,), generator=g, dtype=torch.int32)
            st[pos] = step0 + s
            out.append(int(ops.sample_filtered(xd, t, kk, pp, sd, st)[pos]))
        return out

    a = run(1, 0, seed, 0)
    assert a == run(8, 5, seed, 0)
    assert a == run(64, 63, seed, 0)
    assert a != run(1, 0, seed + 1, 0)          # another seed: another draw
    assert a != run(1, 0, seed, 16)             # other steps: other draws
    # a filtered row is invariant too
    T, k, p = 0.8, 50, 0.9
    b = run(1, 0, seed, 0)
    assert b == run(8, 5, seed, 0) == run(64, 63, seed, 0)


# ---------------------------------------------------------------- 7

def test_engine_seeded_generate(dev):
    from sentio_amd.engines.generator import GeneratorEngine

    eng = GeneratorEngine("tiny-decoder64", device=dev, max_seq=512)
    kw = dict(max_new_tokens=32, temperature=1.0, top_k=50, top_p=0.9,
              stop_on_eos=False)
    a = eng.generate(["seeded sampling on the MI355X"], seed=7, **kw)
    b = eng.generate(["seeded sampling on the MI355X"], seed=7, **kw)
    c = eng.generate(["seeded sampling on the MI355X"], seed=8, **kw)
    assert a[0] and a == b
    assert a != c


def test_continuous_frontend_seeded_request_reproduces(dev):
    """The serving frontend: a seeded request submitted twice, alone each
    time, gives identical non-empty text.  Sampled requests run as
    raw-engine waves beside the slot loop, which they never start."""
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.serving.batcher import ContinuousGenerator

    eng = GeneratorEngine("tiny-decoder64", device=dev, max_seq=512)
    gen = ContinuousGenerator(eng, slots=4)
    try:
        kw = dict(max_new_tokens=24, temperature=1.0, stop_on_eos=False,
                  top_k=50, top_p=0.9, seed=7)
        a = gen.generate(["the same seeded request"], **kw)[0]
        b = gen.generate(["the same seeded request"], **kw)[0]
        assert a and a == b
        s = "".join(gen.stream("the same seeded request", max_new_tokens=24,
                               temperature=1.0, top_k=50, top_p=0.9, seed=7))
        assert isinstance(s, str)
        assert gen.batcher._thread is None
    finally:
        gen.batcher.stop()
        gen.sampled_batcher.stop()


def test_continuous_frontend_mixed_default_and_top_p(dev):
    """One default request (joins the slot loop) and one top_p request (a
    raw-engine wave beside it), submitted concurrently on a 4-slot,
    max_seq-512 frontend: both complete with non-empty text.  Each path
    first serves one request alone, the order a serving start-up follows
    (decode graphs are captured serially before traffic), so the concurrent
    phase replays captured graphs.  The default request is greedy, like the
    existing continuous-batching GPU test: the slot loop's stochastic eager
    sampling is not part of this change."""
    import threading

    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.serving.batcher import ContinuousGenerator

    eng = GeneratorEngine("tiny-decoder64", device=dev, max_seq=512)
    gen = ContinuousGenerator(eng, slots=4)
    try:
        kw = dict(max_new_tokens=24, stop_on_eos=False)
        assert gen.generate(["warm the slot loop"], temperature=0.0, **kw)[0]
        assert gen.generate(["warm the sampled wave"], temperature=0.7,
                            top_p=0.9, **kw)[0]
        outs = {}

        def run(name, **extra):
            outs[name] = gen.generate(["a mixed batch of requests"],
                                      **kw, **extra)[0]

        th = [threading.Thread(target=run, args=("default",),
                               kwargs={"temperature": 0.0}),
              threading.Thread(target=run, args=("nucleus",),
                               kwargs={"temperature": 0.7, "top_p": 0.9})]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join(timeout=150)
        assert isinstance(outs.get("default"), str) and outs["default"]
        assert isinstance(outs.get("nucleus"), str) and outs["nucleus"]
        assert gen.batcher.stats["completed"] == 2
        assert gen.sampled_batcher.stats["requests"] == 2
    finally:
        gen.batcher.stop()
        gen.sampled_batcher.stop()
