"""ops.sample_constrained / ops.sample_slots_constrained on the MI355X.

Exact oracle: the constrained kernel must pick, token for token, what
ops.sample_filtered picks on logits whose disallowed entries (and every
v >= Vt) were set to -inf in torch by the sampling rule -- v is allowed iff
v < min(V, Vt), bit v of mask[state] is set and dist[next[state, v]] <=
left - 1 -- and must then store state = next[state, tok], left = left - 1.
ops.sample_filtered is pinned to the fp64 sort oracle by
tests/test_sampling_gpu.py, so no tolerance applies anywhere here.
"""

import re
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL_TOK = -7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


# ---------------------------------------------------------------- inputs

def geometric_rows(B: int, V: int, seed: int) -> torch.Tensor:
    """The peaked rows of tests/test_sampling_slots_gpu.py: a random
    permutation of logit_r = -0.05*r for ranks r < 200, about -30 for the
    rest, plus 1e-3 jitter."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(B):
        r = torch.arange(V, dtype=torch.float32)
        base = torch.where(r < 200, -0.05 * r, torch.full_like(r, -30.0))
        base = base + 1e-3 * torch.randn(V, generator=g)
        rows.append(base[torch.randperm(V, generator=g)])
    return torch.stack(rows).contiguous()


def param_sets(V: int):
    """The two S=8 parameter sets of tests/test_sampling_slots_gpu.py."""
    a = [(0.0, 0, 1.0), (0.3, 0, 0.9), (0.7, 50, 0.9), (1.0, V + 5, 0.5),
         (2.0, 1, 1.0), (1.0, 50, 1.0), (0.7, 0, 1e-6), (2.0, 50, 0.95)]
    b = [(1.0, 0, 1.0), (0.3, 50, 0.5), (2.0, 0, 0.9), (0.7, V + 5, 0.95),
         (1.0, 1, 0.5), (0.0, 50, 0.9), (2.0, 50, 1e-6), (1.0, 50, 0.95)]
    return a, b


def pack(nxt: np.ndarray) -> np.ndarray:
    """Bitset of nxt >= 0, written independently of the package."""
    N, Vt = nxt.shape
    W = (Vt + 31) // 32
    out = np.zeros((N, W), dtype=np.uint32)
    for s in range(N):
        for v in np.flatnonzero(nxt[s] >= 0):
            out[s, v >> 5] |= np.uint32(1) << np.uint32(v & 31)
    return out.view(np.int32)


def bfs_dist(nxt: np.ndarray, accepting) -> np.ndarray:
    N = nxt.shape[0]
    dist = np.full(N, 30000, dtype=np.int64)
    dist[list(accepting)] = 0
    changed = True
    while changed:
        changed = False
        for s in range(N):
            to = nxt[s][nxt[s] >= 0]
            if to.size and dist[to].min() + 1 < dist[s]:
                dist[s] = dist[to].min() + 1
                changed = True
    return dist.astype(np.int16)


def synthetic_tables():
    """N = 5, Vt = 70 (three mask words, the last partial).  State 0: many
    tokens, into states 0, 1 and 2; state 1: exactly one token (40);
    state 2: into 3 and 0; state 3 accepts; state 4 is DONE."""
    N, Vt = 5, 70
    nxt = np.full((N, Vt), -1, dtype=np.int16)
    for v in range(3, Vt):
        if v % 7:
            nxt[0, v] = v % 3
        nxt[2, v] = 3 if v % 2 else 0
    nxt[1, 40] = 2
    nxt[3, 10:21] = 3
    nxt[3, 69] = 0
    nxt[3, 2] = 4
    nxt[4, 2] = 4
    dist = bfs_dist(nxt, (3, 4))
    assert dist.tolist() == [2, 2, 1, 0, 0]
    return nxt, pack(nxt), dist


@pytest.fixture(scope="module")
def verdict_np():
    from sentio_amd.engines.bpe import get_tokenizer
    from sentio_amd.engines.grammar import VERDICT_GRAMMAR

    tb = VERDICT_GRAMMAR.token_tables(get_tokenizer())
    # inside the first string of "notes": most of the vocabulary is allowed
    inside = VERDICT_GRAMMAR.walk(
        0, b'{"verdict": "pass", "citations_ok":true, "notes": ["a')
    assert inside >= 0
    return tb.next, tb.mask, tb.dist, inside


def to_tables(nxt, mask, dist, dev):
    from sentio_amd import ops

    return ops.GrammarTables.from_numpy(nxt, mask, dist, device=dev)


def masked_logits(x, state, left, nxt, dist):
    """The sampling rule in torch, row by row, from `next` and `dist` alone
    (the mask bit is next >= 0).  Rows with state < 0 stay as they are."""
    N, Vt = nxt.shape
    V = x.shape[1]
    out = x.clone()
    nx = torch.from_numpy(nxt.astype(np.int64))
    ds = torch.from_numpy(dist.astype(np.int64))
    for b, (s, lf) in enumerate(zip(state, left)):
        if s < 0:
            continue
        ok = torch.zeros(V, dtype=torch.bool)
        Vc = min(V, Vt)
        to = nx[s, :Vc]
        ok[:Vc] = (to >= 0) & (ds[to.clamp_min(0)] <= lf - 1)
        out[b, ~ok.to(x.device)] = float("-inf")
    return out


def run_case(dev, x, params, state, left, nxt, mask, dist, tables, seed0):
    from sentio_amd import ops

    B = x.shape[0]
    t = torch.tensor([p[0] for p in params], dtype=torch.float32, device=dev)
    k = torch.tensor([p[1] for p in params], dtype=torch.int32, device=dev)
    p_ = torch.tensor([p[2] for p in params], dtype=torch.float32, device=dev)
    seed = (torch.arange(B, dtype=torch.int64) * 7919 + seed0).to(dev)
    step = (torch.arange(B, dtype=torch.int32) * 5 + 3).to(dev)
    st = torch.tensor(state, dtype=torch.int32, device=dev)
    lf = torch.tensor(left, dtype=torch.int32, device=dev)
    want = ops.sample_filtered(masked_logits(x, state, left, nxt, dist), t, k,
                               p_, seed, step).cpu().tolist()
    got = ops.sample_constrained(x, t, k, p_, seed, step, st, lf,
                                 tables).cpu().tolist()
    assert got == want, (got, want, params)
    new_state, new_left = st.cpu().tolist(), lf.cpu().tolist()
    for b in range(B):
        if state[b] < 0:
            assert (new_state[b], new_left[b]) == (state[b], left[b]), b
        else:
            assert new_state[b] == int(nxt[state[b], got[b]]), b
            assert new_state[b] >= 0, b
            assert new_left[b] == left[b] - 1, b
    return got


def all_param_rows(V):
    """Every entry of both parameter sets, five rows at a time."""
    a, b = param_sets(V)
    return [a[:5], a[3:], b[:5], b[3:]]


# ---------------------------------------------------------------- kernel

@pytest.mark.parametrize("V", (67, 70, 1001))
def test_synthetic_table_equals_masked_sample_filtered(dev, V):
    """V < Vt, V == Vt and an odd V whose rows are not 16-byte aligned.
    Rows: unconstrained, a one-token state, DONE, a row whose budget binds
    (state 0, left 2: only tokens into state 2 remain) and one where it does
    not (left - 1 above every dist: the kernel skips the dist sweep); on
    every other pass that last row binds too (state 2, left 2)."""
    nxt, mask, dist = synthetic_tables()
    tables = to_tables(nxt, mask, dist, dev)
    x = geometric_rows(5, V, seed=11 + V).to(dev)
    for i, params in enumerate(all_param_rows(V)):
        state = [-1, 1, 4, 0, 2]
        left = [9, 7, 3, 2, 50 if i % 2 == 0 else 2]
        got = run_case(dev, x, params, state, left, nxt, mask, dist, tables,
                       seed0=1000 + i)
        assert got[1] == 40 and got[2] == 2
        assert got[3] % 3 == 2          # the binding budget: into state 2


@pytest.mark.parametrize("V", (4608, 128256))
def test_verdict_tables_equal_masked_sample_filtered(dev, verdict_np, V):
    """The real tokenizer's tables (Vt = 4355) under a tiny decoder's and
    llama3-8b's vocabulary."""
    nxt, mask, dist, inside = verdict_np
    assert nxt.shape[1] == 4355 and (nxt[inside] >= 0).sum() > 1000
    tables = to_tables(nxt, mask, dist, dev)
    done = nxt.shape[0] - 1
    count = (nxt >= 0).sum(axis=1)
    single = int(np.flatnonzero(count[:done] == 1)[0])
    x = geometric_rows(5, V, seed=5 + V % 9973).to(dev)
    for i, params in enumerate(all_param_rows(V)):
        state = [-1, single, done, inside, inside]
        left = [9, int(dist[single]) + 4, 3, int(dist[inside]), 200]
        run_case(dev, x, params, state, left, nxt, mask, dist, tables,
                 seed0=2000 + i)


def test_all_non_finite_row_takes_the_lowest_allowed_index(dev):
    from sentio_amd import ops

    nxt, mask, dist = synthetic_tables()
    tables = to_tables(nxt, mask, dist, dev)
    V = 70
    x = torch.full((3, V), float("-inf"))
    x[1, ::2] = float("nan")
    x[2, :3] = 5.0                      # finite only where nothing is allowed
    x = x.to(dev)
    state = torch.tensor([0, 0, 0], dtype=torch.int32, device=dev)
    left = torch.tensor([9, 2, 9], dtype=torch.int32, device=dev)
    for T in (0.0, 0.8):
        st, lf = state.clone(), left.clone()
        tok = ops.sample_constrained(x, T, 0, 1.0, 7, 0, st, lf, tables)
        # state 0 allows v >= 3 with v % 7 != 0; with left = 2 only v % 3 == 2
        assert tok.cpu().tolist() == [3, 5, 3]
        assert st.cpu().tolist() == [0, 2, 0]
        assert lf.cpu().tolist() == [8, 1, 8]


def test_slot_form_matches_the_per_row_op(dev):
    """S = 8, R = 5 on a permuted slot list: slot 7 inactive, slot 2 never
    listed, one constrained and one unconstrained active slot among the
    rest.  Skipped slots keep tok, step, state and left; sampled ones equal
    ops.sample_constrained at their own step."""
    from sentio_amd import ops

    nxt, mask, dist = synthetic_tables()
    tables = to_tables(nxt, mask, dist, dev)
    V, S = 1001, 8
    slot = [6, 1, 7, 0, 3]
    x = geometric_rows(5, V, seed=99).to(dev)
    for which in (0, 1):
        params = param_sets(V)[which]
        t = torch.tensor([p[0] for p in params], dtype=torch.float32,
                         device=dev)
        k = torch.tensor([p[1] for p in params], dtype=torch.int32, device=dev)
        p_ = torch.tensor([p[2] for p in params], dtype=torch.float32,
                          device=dev)
        seed = (torch.arange(S, dtype=torch.int64) * 7919 + 1000).to(dev)
        step = (torch.arange(S, dtype=torch.int32) * 5 + 3).to(dev)
        tok = torch.full((S,), SENTINEL_TOK, dtype=torch.int64, device=dev)
        state0 = [0, -1, 2, 3, 1, 0, 0, 2]
        left0 = [2, 5, 6, 7, 8, 9, 40, 11]
        state = torch.tensor(state0, dtype=torch.int32, device=dev)
        left = torch.tensor(left0, dtype=torch.int32, device=dev)
        active = torch.ones(S, dtype=torch.uint8, device=dev)
        active[7] = 0
        step0 = step.cpu().tolist()
        # the per-row op on copies, rows in slot order
        idx = torch.tensor(slot, device=dev)
        st_r, lf_r = state[idx].contiguous(), left[idx].contiguous()
        want = ops.sample_constrained(x, t[idx], k[idx], p_[idx], seed[idx],
                                      step[idx], st_r, lf_r, tables)
        ops.sample_slots_constrained(x, slot, t, k, p_, seed, step, active,
                                     tok, state, left, tables)
        tok_h, step_h = tok.cpu().tolist(), step.cpu().tolist()
        state_h, left_h = state.cpu().tolist(), left.cpu().tolist()
        for r, s in enumerate(slot):
            if s == 7:
                continue
            assert tok_h[s] == int(want[r]), (r, s)
            assert step_h[s] == step0[s] + 1
            assert state_h[s] == int(st_r[r]) and left_h[s] == int(lf_r[r])
        for s in (2, 4, 5, 7):
            assert tok_h[s] == SENTINEL_TOK and step_h[s] == step0[s]
            assert state_h[s] == state0[s] and left_h[s] == left0[s]
        assert state_h[1] == -1 and left_h[1] == 5      # unconstrained slot


def test_slot_form_with_no_constrained_slot_equals_sample_slots(dev):
    """state = -1 everywhere: token for token ops.sample_slots."""
    from sentio_amd import ops

    nxt, mask, dist = synthetic_tables()
    tables = to_tables(nxt, mask, dist, dev)
    V, S = 1001, 8
    x = geometric_rows(S, V, seed=3).to(dev)
    params = param_sets(V)[0]
    t = torch.tensor([p[0] for p in params], dtype=torch.float32, device=dev)
    k = torch.tensor([p[1] for p in params], dtype=torch.int32, device=dev)
    p_ = torch.tensor([p[2] for p in params], dtype=torch.float32, device=dev)
    seed = (torch.arange(S, dtype=torch.int64) * 31 + 5).to(dev)
    outs = []
    for constrained in (False, True):
        step = torch.arange(S, dtype=torch.int32, device=dev)
        tok = torch.zeros(S, dtype=torch.int64, device=dev)
        if constrained:
            state = torch.full((S,), -1, dtype=torch.int32, device=dev)
            left = torch.zeros(S, dtype=torch.int32, device=dev)
            ops.sample_slots_constrained(x, None, t, k, p_, seed, step, None,
                                         tok, state, left, tables)
            assert state.cpu().tolist() == [-1] * S
        else:
            ops.sample_slots(x, None, t, k, p_, seed, step, None, tok)
        outs.append((tok.cpu().tolist(), step.cpu().tolist()))
    assert outs[0] == outs[1]


def test_host_validation_raises_before_any_launch(dev):
    from sentio_amd import ops

    nxt, mask, dist = synthetic_tables()
    tables = to_tables(nxt, mask, dist, dev)
    x = geometric_rows(2, 70, seed=1).to(dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    left = torch.full((2,), 5, dtype=torch.int32, device=dev)

    def call(st=state, lf=left, tb=tables, lg=x):
        return ops.sample_constrained(lg, 1.0, 0, 1.0, 1, 0, st, lf, tb)

    with pytest.raises(ValueError):
        call(st=state.long())                            # dtype
    with pytest.raises(ValueError):
        call(lf=left[:1])                                # shape
    with pytest.raises(ValueError):
        call(st=state.cpu())                             # device
    with pytest.raises(ValueError):
        call(tb=to_tables(nxt, mask, dist, "cpu"))       # tables' device
    with pytest.raises(ValueError):
        call(tb=(tables.next, tables.mask, tables.dist))  # not a holder
    with pytest.raises(ValueError):
        ops.GrammarTables(tables.next, tables.mask[:, :2].contiguous(),
                          tables.dist)                   # mask word count
    with pytest.raises(ValueError):
        ops.GrammarTables(tables.next.int(), tables.mask, tables.dist)
    tok = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.sample_slots_constrained(
            x, None, torch.ones(2, device=dev),
            torch.zeros(2, dtype=torch.int32, device=dev),
            torch.ones(2, device=dev),
            torch.zeros(2, dtype=torch.int64, device=dev),
            torch.zeros(2, dtype=torch.int32, device=dev), None, tok,
            state.long(), left, tables)
    assert state.cpu().tolist() == [0, 0] and left.cpu().tolist() == [5, 5]
    assert call().shape == (2,)                          # and the good call runs


# ---------------------------------------------------------------- engine

PATTERN = r"(yes|no), [a-c]{2,5}!"


def graphed_engine(dev, max_seq):
    """A tiny-decoder64 engine as production builds it: decode steps are
    captured hipGraphs, the constrained sampler runs next to them."""
    from sentio_amd.engines.generator import GeneratorEngine

    eng = GeneratorEngine("tiny-decoder64", device=dev, max_seq=max_seq)
    assert eng._use_graphs()
    return eng


@pytest.fixture(scope="module")
def engine(dev):
    return graphed_engine(dev, 512)


def test_engine_constrained_generate_full_matches(engine):
    from sentio_amd.engines.grammar import Grammar

    g = Grammar.from_regex(PATTERN)
    h = engine.register_grammar(g)
    prompts = ["answer yes or no", "a second prompt", "and a third one"]
    for T, extra in ((0.0, {}), (0.7, {}), (1.0, {"top_k": 20, "top_p": 0.9,
                                                  "seed": 5})):
        for budget in (h.min_tokens, h.min_tokens + 3):
            outs = engine.generate(prompts, max_new_tokens=budget,
                                   temperature=T, grammar=g, **extra)
            for o in outs:
                assert re.fullmatch(PATTERN, o), (T, budget, o)
    plain = engine.generate(prompts, max_new_tokens=h.min_tokens + 3,
                            temperature=0.0)
    assert not any(re.fullmatch(PATTERN, o) for o in plain)


def test_capture_outside_inference_mode_still_works_after_the_engine(engine):
    """The engine captures its decode graph under inference mode.  If that
    were the process's first capture, the default generator's capture state
    would be inference tensors and this plain capture would fail in
    capture_begin (engines/graphed.py: prime_capture_state)."""
    engine.generate(["capture a decode graph"], max_new_tokens=4,
                    temperature=0.0)
    assert any(s.graph is not None for s in engine._sessions.values())
    assert not torch.is_inference_mode_enabled()
    buf = torch.zeros(4, device=engine.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    assert buf.tolist() == [1.0] * 4


def test_engine_grammar_none_is_the_unused_feature(dev):
    """Greedy output with grammar=None equals the same call on an engine
    that never registered a grammar."""
    from sentio_amd.engines.grammar import Grammar

    prompts = ["the same prompt twice over", "and one more"]
    fresh = graphed_engine(dev, 256)
    want = fresh.generate(prompts, max_new_tokens=12, temperature=0.0)
    used = graphed_engine(dev, 256)
    g = Grammar.from_regex(PATTERN)
    used.generate(prompts, max_new_tokens=12, temperature=0.0, grammar=g)
    assert used.generate(prompts, max_new_tokens=12, temperature=0.0,
                         grammar=None) == want


def test_slot_loop_serves_constrained_and_plain_together(engine):
    from sentio_amd.engines.grammar import Grammar
    from sentio_amd.serving.batcher import ContinuousGenerator

    g = Grammar.from_regex(PATTERN)
    gen = ContinuousGenerator(engine, slots=4, slot_sampling=True)
    try:
        kw = dict(max_new_tokens=12, temperature=0.7)
        assert gen.generate(["warm the slot loop"], **kw)[0]
        outs = {}

        def run(name, **extra):
            outs[name] = gen.generate(["a mixed batch of requests"], **kw,
                                      **extra)[0]

        th = [threading.Thread(target=run, args=("plain",),
                               kwargs={"stop_on_eos": False}),
              threading.Thread(target=run, args=("constrained",),
                               kwargs={"grammar": g})]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join(timeout=150)
        assert re.fullmatch(PATTERN, outs.get("constrained") or ""), outs
        assert isinstance(outs.get("plain"), str) and outs["plain"]
        assert not re.fullmatch(PATTERN, outs["plain"])
        assert gen.batcher.stats["completed"] == 3
        assert gen.sampled_batcher.stats["requests"] == 0
    finally:
        gen.batcher.stop()
        gen.sampled_batcher.stop()
