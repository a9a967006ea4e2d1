"""ops.sample_slots on the MI355X: the slot-table sampler of the continuous
batcher against the project's own ops.sample_filtered, which
tests/test_sampling_gpu.py pins to the fp64 sort oracle.  Both kernels call
the same two device functions (threshold, then Gumbel-argmax), so every
comparison here is EXACT token equality, no tolerance.

The engine-level tests use tiny-decoder64, the tiny decoder whose head
dimension the GPU attention kernels accept.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

VOCABS = (3, 1000, 1001, 4608, 128256)
SENTINEL_TOK = -7


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
    """Two S=8 parameter sets: every T, top_k and top_p value of the
    sample_filtered tests, each filter alone and both combined, greedy and
    temperature-only slots among them."""
    a = [(0.0, 0, 1.0), (0.3, 0, 0.9), (0.7, 50, 0.9), (1.0, V + 5, 0.5),
         (2.0, 1, 1.0), (1.0, 50, 1.0), (0.7, 0, 1e-6), (2.0, 50, 0.95)]
    b = [(1.0, 0, 1.0), (0.3, 50, 0.5), (2.0, 0, 0.9), (0.7, V + 5, 0.95),
         (1.0, 1, 0.5), (0.0, 50, 0.9), (2.0, 50, 1e-6), (1.0, 50, 0.95)]
    return a, b


class Slots:
    """Device slot arrays for S slots: distinct seeds, distinct non-zero
    starting steps, sentinel tokens."""

    def __init__(self, params, dev, seed0=1000):
        S = len(params)
        self.S, self.dev = S, dev
        self.t = torch.tensor([p[0] for p in params], dtype=torch.float32,
                              device=dev)
        self.k = torch.tensor([p[1] for p in params], dtype=torch.int32,
                              device=dev)
        self.p = torch.tensor([p[2] for p in params], dtype=torch.float32,
                              device=dev)
        self.seed = (torch.arange(S, dtype=torch.int64) * 7919
                     + seed0).to(dev)
        self.step = (torch.arange(S, dtype=torch.int32) * 5 + 3).to(dev)
        self.tok = torch.full((S,), SENTINEL_TOK, dtype=torch.int64,
                              device=dev)

    def oracle(self, logits_row, s: int, step: int) -> int:
        """ops.sample_filtered on one row with slot s's parameters."""
        from sentio_amd import ops

        return int(ops.sample_filtered(
            logits_row.view(1, -1), self.t[s:s + 1], self.k[s:s + 1],
            self.p[s:s + 1], self.seed[s:s + 1],
            torch.tensor([step], dtype=torch.int32, device=self.dev))[0])

    def run(self, logits, slot, active):
        from sentio_amd import ops

        ops.sample_slots(logits, slot, self.t, self.k, self.p, self.seed,
                         self.step, active, self.tok)


def check(st: Slots, x, pairs, step_before, tok_before):
    """pairs: (row, slot) that must have been sampled; every other slot
    keeps tok_before / step_before."""
    tok, step = st.tok.cpu().tolist(), st.step.cpu().tolist()
    sampled = set()
    for r, s in pairs:
        want = st.oracle(x[r], s, step_before[s])
        assert tok[s] == want, (r, s, tok[s], want)
        assert step[s] == step_before[s] + 1, (r, s)
        sampled.add(s)
    for s in range(st.S):
        if s not in sampled:
            assert tok[s] == tok_before[s] and step[s] == step_before[s], s


# ---------------------------------------------------------------- kernel

@pytest.mark.parametrize("V", VOCABS)
def test_equals_sample_filtered_over_a_slot_table(dev, V):
    """S = 8, R = 5 rows on a permuted slot list, one listed slot inactive.
    Odd V and V = 3 give misaligned row starts and the head / tail path of
    the row visitor; 128256 is a full vocabulary."""
    slot = [6, 1, 7, 0, 3]
    inactive = 7
    x = geometric_rows(5, V, seed=31 + V % 9973).to(dev)
    active = torch.ones(8, dtype=torch.uint8, device=dev)
    active[inactive] = 0
    for which in (0, 1):
        st = Slots(param_sets(V)[which], dev, seed0=1000 + which)
        step0, tok0 = st.step.cpu().tolist(), st.tok.cpu().tolist()
        st.run(x, slot, active)
        check(st, x, [(r, s) for r, s in enumerate(slot) if s != inactive],
              step0, tok0)


def test_identity_addressing_and_device_step_counter(dev):
    """slot=None: row r is slot r.  A second call on the same logits draws at
    the advanced step values: the counter lives on the device."""
    V = 4608
    x = geometric_rows(8, V, seed=77).to(dev)
    mask = [1, 0, 1, 1, 0, 1, 0, 1]
    active = torch.tensor(mask, dtype=torch.uint8, device=dev)
    pairs = [(s, s) for s in range(8) if mask[s]]
    st = Slots(param_sets(V)[0], dev)
    first = None
    for call in range(2):
        step0, tok0 = st.step.cpu().tolist(), st.tok.cpu().tolist()
        st.run(x, None, active)
        check(st, x, pairs, step0, tok0)
        if call == 0:
            first = st.step.cpu().tolist()
    assert st.step.cpu().tolist() == [f + m for f, m in zip(first, mask)]


def test_all_inactive_and_out_of_range_slots_write_nothing(dev):
    """The in-kernel guard: a block whose slot is outside [0, S) or inactive
    returns before any store."""
    V = 1001
    x = geometric_rows(5, V, seed=5).to(dev)
    st = Slots(param_sets(V)[1], dev)
    step0, tok0 = st.step.cpu().tolist(), st.tok.cpu().tolist()
    st.run(x, [4, 2, 0, 1, 7], torch.zeros(8, dtype=torch.uint8, device=dev))
    check(st, x, [], step0, tok0)

    slot = torch.tensor([2, -1, 5, 8, 0], dtype=torch.int32, device=dev)
    st.run(x, slot, None)
    check(st, x, [(0, 2), (2, 5), (4, 0)], step0, tok0)


def test_slot_invariance(dev):
    """The same (row, parameters, seed, step) in slot 0 of S = 1 and in slot
    6 of S = 8 among other neighbours gives the same token."""
    from sentio_amd import ops

    V = 4608
    row = geometric_rows(1, V, seed=9).to(dev)
    others = geometric_rows(8, V, seed=10).to(dev)
    for T, k, p in ((1.0, 0, 1.0), (0.8, 50, 0.9)):
        draws = []
        for step in (0, 1, 2, 40):
            one = Slots([(T, k, p)], dev)
            one.seed[0], one.step[0] = 4242, step
            one.run(row, None, None)
            params = list(param_sets(V)[0])
            params[6] = (T, k, p)
            eight = Slots(params, dev)
            eight.seed[6], eight.step[6] = 4242, step
            x = others.clone()
            x[3] = row[0]
            eight.run(x[1:6].contiguous(), [0, 4, 6, 2, 7], None)
            assert int(one.tok[0]) == int(eight.tok[6]), (T, k, p, step)
            assert int(eight.step[6]) == step + 1
            draws.append(int(one.tok[0]))
            assert draws[-1] == int(ops.sample_filtered(row, T, k, p, 4242,
                                                        step)[0])
        assert len(set(draws)) > 1                # the step changes the draw


# ---------------------------------------------------------------- engine

def test_engine_slot_sampler_on_real_logits(dev):
    """Two prompts prefilled into rows [2, 0] of a 4-slot session, slots 1
    and 3 free: the admission draw and three decode steps equal
    ops.sample_filtered on each step's logits rows, free rows of `cur` never
    change, and the device step counters end at 4."""
    from sentio_amd import ops
    from sentio_amd.engines.generator import GeneratorEngine, SamplingParams

    eng = GeneratorEngine("tiny-decoder64", device=dev, max_seq=128)
    sess = eng.make_slot_session(4)
    rows = [2, 0]
    logits = eng.prefill_into_slots(
        sess, rows, ["the first resident request", "a second, other prompt"],
        [8, 8])
    sp = eng.make_slot_sampler(4)
    params = [SamplingParams(0.8, 50, 0.9, seed=17),
              SamplingParams(1.0, 0, 1.0, seed=23)]
    sp.admit(rows, params)
    FREE = 5
    cur = torch.full((4,), FREE, dtype=torch.int64, device=dev)

    def oracle(lg, step):
        return ops.sample_filtered(
            lg, [q.temperature for q in params], [q.top_k for q in params],
            [q.top_p for q in params], [q.seed for q in params],
            step).cpu().tolist()

    want = oracle(logits, 0)
    sp.sample(logits, cur, rows=rows)
    assert cur.cpu().tolist() == [want[1], FREE, want[0], FREE]
    for i in range(3):
        logits = eng.decode_step_session(sess, cur)
        want = oracle(logits[rows], i + 1)
        sp.sample(logits, cur)
        assert cur.cpu().tolist() == [want[1], FREE, want[0], FREE], i
    assert sp.step.cpu().tolist() == [4, 0, 4, 0]


def test_frontend_top_p_and_default_share_the_slot_loop(dev):
    """A top_p / top_k request and a default request, submitted concurrently
    with slot sampling on: both join the slot loop, none runs as a wave.  One
    request alone first, so the loop's decode graph is captured before the
    concurrent phase.  Texts are not compared with the wave path: bf16 logits
    from different batch shapes legitimately differ at near-ties."""
    import threading

    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.serving.batcher import ContinuousGenerator

    eng = GeneratorEngine("tiny-decoder64", device=dev, max_seq=512)
    gen = ContinuousGenerator(eng, slots=4, slot_sampling=True)
    try:
        kw = dict(max_new_tokens=8, stop_on_eos=False)
        assert gen.generate(["warm the slot loop"], temperature=0.7,
                            top_p=0.9, **kw)[0]
        outs = {}

        def run(name, **extra):
            outs[name] = gen.generate(["a mixed batch of requests"],
                                      **kw, **extra)[0]

        th = [threading.Thread(target=run, args=("default",),
                               kwargs={"temperature": 0.7}),
              threading.Thread(target=run, args=("nucleus",),
                               kwargs={"temperature": 0.7, "top_p": 0.9,
                                       "top_k": 50})]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join(timeout=150)
        assert isinstance(outs.get("default"), str) and outs["default"]
        assert isinstance(outs.get("nucleus"), str) and outs["nucleus"]
        assert gen.batcher.stats["completed"] == 3
        assert gen.sampled_batcher.stats["requests"] == 0
    finally:
        gen.batcher.stop()
        gen.sampled_batcher.stop()
