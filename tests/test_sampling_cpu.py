"""Per-request top-k / top-p / seeded sampling without a GPU: the fp64
oracle's semantics on hand-checkable rows, the CPU op path, that default
requests stay on the default sampling path, and the plumbing from the HTTP
API / CLI down to the generator's keyword arguments."""

import pytest
import torch

from sentio_amd import ops

NEG = float("-inf")


def support(row, T, k, p):
    tau, count = ops.sample_support(torch.tensor([row]), T, k, p)
    return float(tau[0]), int(count[0])


# ---------------------------------------------------------------- oracle

def test_top_k_one_and_tiny_top_p_give_the_argmax():
    row = [0.5, 2.0, -1.0, 1.5]
    assert support(row, 1.0, 1, 1.0) == (2.0, 1)
    assert support(row, 1.0, 0, 0.0) == (2.0, 1)
    assert support(row, 1.0, 0, -0.5) == (2.0, 1)
    assert support(row, 0.7, 3, 1e-6) == (2.0, 1)


def test_filters_off_keep_the_full_set():
    row = [0.5, 2.0, -1.0, 1.5]
    assert support(row, 1.0, 0, 1.0) == (-1.0, 4)
    assert support(row, 1.0, 4, 1.0) == (-1.0, 4)       # top_k >= V: off
    assert support(row, 1.0, 9, 1.0) == (-1.0, 4)
    assert support(row, 1.0, -3, 1.0) == (-1.0, 4)


def test_top_p_renormalises_over_the_top_k_survivors():
    # p = softmax([0,-1,-2,-3]) = .6439 .2369 .0871 .0321
    row = [0.0, -1.0, -2.0, -3.0]
    # top-p alone: .6439 < .7 <= .8808 -> two tokens
    assert support(row, 1.0, 0, 0.7) == (-1.0, 2)
    # top_k = 2 first: M_k = .8808, target .7 * .8808 = .6166 <= .6439 -> ONE
    # token (without renormalisation the answer would stay at two)
    assert support(row, 1.0, 2, 0.7) == (0.0, 1)
    # temperature rescales before the softmax: T = 2 flattens the row
    # (.4551 .2760 .1674 .1015): .7 needs two tokens, .75 needs three
    assert support(row, 2.0, 0, 0.7) == (-1.0, 2)
    assert support(row, 2.0, 0, 0.75) == (-2.0, 3)


def test_every_token_tied_with_tau_is_kept():
    row = [1.0, 3.0, 1.0, 1.0, 0.0]
    assert support(row, 1.0, 2, 1.0) == (1.0, 4)         # count > top_k
    # p = .6652 .1001 x3 .0368: .7 lands inside the tie group
    assert support(row, 1.0, 0, 0.7) == (1.0, 4)
    assert support([2.0, 2.0, 2.0], 1.0, 1, 1.0) == (2.0, 3)


def test_minus_inf_entries_are_excluded():
    row = [NEG, 1.0, NEG, 0.0]
    assert support(row, 1.0, 0, 1.0) == (0.0, 2)
    assert support(row, 1.0, 3, 1.0) == (0.0, 2)         # only 2 finite: off
    assert support(row, 1.0, 1, 1.0) == (1.0, 1)
    tok = ops.sample_filtered(torch.tensor([row] * 64), 1.0, 0, 1.0,
                              torch.arange(64), 0)
    assert set(tok.tolist()) <= {1, 3}


def test_non_positive_temperature_is_greedy():
    row = [0.5, 2.0, -1.0, 2.0]
    for T in (0.0, -1.0):
        tau, _ = ops.sample_support(torch.tensor([row]), T, 3, 0.5)
        assert float(tau[0]) == 2.0
        tok = ops.sample_filtered(torch.tensor([row]), T, 3, 0.5, 1, 0)
        assert tok.tolist() == [1]                       # lowest index of max


def test_per_row_parameters_and_scalar_broadcast():
    x = torch.tensor([[0.0, -1.0, -2.0, -3.0]] * 3)
    tau, count = ops.sample_support(x, [1.0, 1.0, 0.0], [0, 2, 0],
                                    torch.tensor([0.7, 0.7, 1.0]))
    assert tau.tolist() == [-1.0, 0.0, 0.0]
    assert count.tolist()[:2] == [2, 1]
    assert tau.dtype == torch.float32 and count.dtype == torch.int32
    with pytest.raises(ValueError):
        ops.sample_support(x, [1.0, 2.0], 0, 1.0)         # 2 entries, 3 rows


# ---------------------------------------------------------------- CPU op

def _rows(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    return 2.0 * torch.randn(B, V, generator=g)


def test_cpu_tokens_stay_inside_the_support():
    x = _rows(16, 300, 1)
    t = torch.linspace(0.0, 1.5, 16)
    k = torch.tensor([0, 1, 5, 50] * 4)
    p = torch.tensor([1.0, 0.9, 0.5, 0.05] * 4)
    tau, _ = ops.sample_support(x, t, k, p)
    for step in range(4):
        tok = ops.sample_filtered(x, t, k, p, torch.arange(16), step)
        assert tok.dtype == torch.int64
        assert bool((x.gather(1, tok[:, None])[:, 0] >= tau).all())


def test_cpu_same_seed_and_step_same_token_anywhere():
    row = _rows(1, 500, 2)[0]
    args = (0.9, 40, 0.95)

    def at(B, pos, seed, step):
        x = _rows(B, 500, 100 + B)
        x[pos] = row
        sd = torch.arange(B) + 1000
        sd[pos] = seed
        st = torch.arange(B) % 7
        st[pos] = step
        return int(ops.sample_filtered(x, *args, sd, st)[pos])

    a = [at(1, 0, 11, s) for s in range(12)]
    assert a == [at(8, 5, 11, s) for s in range(12)]
    assert a == [at(33, 32, 11, s) for s in range(12)]
    assert len(set(a)) > 1                               # steps: other draws
    assert a != [at(1, 0, 12, s) for s in range(12)]     # seeds: other draws


# ---------------------------------------------------------------- engine

class _Spy:
    def __init__(self, monkeypatch):
        self.calls = {"sample_token": 0, "sample_filtered": 0}
        for name in self.calls:
            real = getattr(ops, name)

            def wrap(*a, _real=real, _name=name, **kw):
                self.calls[_name] += 1
                return _real(*a, **kw)

            monkeypatch.setattr(ops, name, wrap)


def test_default_generate_stays_on_sample_token(monkeypatch):
    from sentio_amd.engines.generator import GeneratorEngine

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=64)
    spy = _Spy(monkeypatch)
    out = eng.generate(["hello"], max_new_tokens=4, temperature=0.7,
                       stop_on_eos=False)
    assert len(out) == 1
    assert spy.calls == {"sample_token": 4, "sample_filtered": 0}
    list(eng.stream("hello", max_new_tokens=3, temperature=0.7))
    assert spy.calls["sample_filtered"] == 0


def test_top_p_generate_uses_sample_filtered(monkeypatch):
    from sentio_amd.engines.generator import GeneratorEngine

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=64)
    spy = _Spy(monkeypatch)
    kw = dict(max_new_tokens=6, temperature=1.0, stop_on_eos=False)
    a = eng.generate(["hello"], top_p=0.9, seed=3, **kw)
    assert spy.calls == {"sample_token": 0, "sample_filtered": 6}
    assert a == eng.generate(["hello"], top_p=0.9, seed=3, **kw)
    list(eng.stream("hello", max_new_tokens=3, temperature=1.0, top_k=5))
    assert spy.calls["sample_token"] == 0


def test_sampling_params_defaults():
    from sentio_amd.engines.generator import SamplingParams

    sp = SamplingParams()
    assert (sp.top_k, sp.top_p, sp.seed) == (0, 1.0, None)
    assert not sp.filtered
    assert SamplingParams(top_p=0.9).filtered
    assert SamplingParams(top_k=5).filtered
    assert SamplingParams(seed=0).filtered


def test_sample_rows_keeps_its_signature_and_eager_code(monkeypatch):
    from sentio_amd.engines.generator import GeneratorEngine

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=64)
    spy = _Spy(monkeypatch)
    x = _rows(4, eng.cfg.vocab_size, 5)
    tok = eng.sample_rows(x, torch.tensor([0.0, 0.5, 1.0, 0.0]))
    assert spy.calls == {"sample_token": 0, "sample_filtered": 0}
    assert tok[0] == x[0].argmax() and tok[3] == x[3].argmax()


def test_continuous_frontend_routes_sampled_requests_beside_the_loop():
    """Requests with top-k / top-p / seed run as raw-engine waves; the slot
    loop is not started for them and default requests still join it."""
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.serving.batcher import ContinuousGenerator

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=64)
    gen = ContinuousGenerator(eng, slots=2)
    try:
        kw = dict(max_new_tokens=6, temperature=1.0, stop_on_eos=False,
                  top_k=20, top_p=0.9, seed=5)
        a = gen.generate(["seeded"], **kw)
        b = gen.generate(["seeded"], **kw)
        assert a == b and len(a) == 1
        s = "".join(gen.stream("seeded", max_new_tokens=6, temperature=1.0,
                               top_p=0.9, seed=5))
        assert isinstance(s, str)
        assert gen.batcher._thread is None               # loop never started
        assert gen.sampled_batcher.stats["requests"] == 3
        # filters switched off explicitly: a default request, joins the loop
        out = gen.generate(["plain"], max_new_tokens=4, temperature=0.5,
                           top_k=0, top_p=1.0, seed=None)
        assert isinstance(out[0], str)
        assert gen.batcher.stats["requests"] == 1
        assert gen.sampled_batcher.stats["requests"] == 3
    finally:
        gen.batcher.stop()
        gen.sampled_batcher.stop()


# ---------------------------------------------------------------- plumbing

class _Recorder:
    """Stub generator that records the keyword arguments it receives."""

    tokenizer = None

    def __init__(self):
        self.calls = []

    def generate(self, prompts, **kw):
        self.calls.append(kw)
        return ["recorded answer [1]"] * len(prompts)


def _client(**overrides):
    from fastapi.testclient import TestClient

    from sentio_amd.config import Settings
    from sentio_amd.serving.app import create_app
    from sentio_amd.serving.container import ServiceContainer

    s = Settings()
    s.mock_compute = True
    s.device = "cpu"
    s.use_verifier = False
    for k, v in overrides.items():
        setattr(s, k, v)
    container = ServiceContainer(s)
    rec = _Recorder()
    container._cache["generator"] = rec
    return TestClient(create_app(s, container)), rec, container


def test_chat_forwards_sampling_fields_to_the_generator():
    client, rec, container = _client()
    with client:
        r = client.post("/chat", json={
            "question": "what is nucleus sampling?", "temperature": 0.8,
            "top_p": 0.9, "sampling_top_k": 50, "seed": 1})
        assert r.status_code == 200, r.text
        assert r.json()["answer"] == "recorded answer [1]"
        kw = rec.calls[-1]
        assert (kw["top_p"], kw["top_k"], kw["seed"]) == (0.9, 50, 1)
        assert kw["temperature"] == 0.8
        # nothing set: the generator sees none of the new keywords
        r = client.post("/chat", json={"question": "a plain question"})
        assert r.status_code == 200, r.text
        assert not {"top_p", "top_k", "seed"} & set(rec.calls[-1])


@pytest.mark.parametrize("field,value", (("top_p", 0), ("top_p", 1.5),
                                         ("sampling_top_k", -1),
                                         ("seed", -1)))
def test_chat_rejects_out_of_range_sampling_fields(field, value):
    client, rec, _ = _client()
    with client:
        r = client.post("/chat", json={"question": "hello there", field: value})
        assert r.status_code == 422
        r = client.post("/chat/stream",
                        json={"question": "hello there", field: value})
        assert r.status_code == 422
    assert rec.calls == []


def test_omitted_fields_fall_back_to_service_defaults():
    client, rec, _ = _client(gen_top_p=0.8, gen_top_k=40)
    with client:
        r = client.post("/chat", json={"question": "use the defaults"})
        assert r.status_code == 200, r.text
        kw = rec.calls[-1]
        assert (kw["top_p"], kw["top_k"]) == (0.8, 40)
        assert kw["seed"] is None
        # a request's own value wins, including "off"
        r = client.post("/chat", json={"question": "override the defaults",
                                       "top_p": 1.0, "sampling_top_k": 0})
        assert r.status_code == 200, r.text
        assert not {"top_p", "top_k", "seed"} & set(rec.calls[-1])


def test_settings_read_gen_defaults_from_env(monkeypatch):
    from sentio_amd.config import Settings

    assert (Settings().gen_top_p, Settings().gen_top_k) == (1.0, 0)
    monkeypatch.setenv("GEN_TOP_P", "0.85")
    monkeypatch.setenv("GEN_TOP_K", "64")
    monkeypatch.setenv("GEN_SEED", "12")
    s = Settings.from_env()
    assert (s.gen_top_p, s.gen_top_k, s.gen_seed) == (0.85, 64, 12)
    assert Settings().gen_seed == -1


def test_generate_node_reads_sampling_metadata():
    from sentio_amd.pipeline.nodes import create_generator_node
    from sentio_amd.pipeline.state import create_initial_state

    rec = _Recorder()
    node = create_generator_node(rec, "balanced", 16)
    node(create_initial_state("q", {"top_p": 0.5, "sampling_top_k": 7,
                                    "seed": 9}))
    assert {k: rec.calls[-1][k] for k in ("top_p", "top_k", "seed")} == {
        "top_p": 0.5, "top_k": 7, "seed": 9}
    node(create_initial_state("q", {}))
    assert not {"top_p", "top_k", "seed"} & set(rec.calls[-1])


def test_mock_generator_accepts_the_new_keywords():
    from sentio_amd.engines.mock import MockGeneratorEngine

    m = MockGeneratorEngine()
    assert m.generate(["p"], top_k=5, top_p=0.9, seed=1) == m.generate(["p"])
    assert "".join(m.stream("p", top_k=5, top_p=0.9, seed=1))


def test_dynamic_batcher_key_separates_top_p():
    from sentio_amd.serving.batcher import _Item, _make_item

    base = _make_item("a", 8, 0.7, True)
    assert type(base) is _Item                           # default: unchanged
    assert base.group_key == _make_item("b", 8, 0.7, True).group_key
    assert base.group_key == (0.7, 8, True)
    p9 = _make_item("a", 8, 0.7, True, top_p=0.9)
    assert p9.group_key != base.group_key
    assert p9.group_key == _make_item("b", 8, 0.7, True, top_p=0.9).group_key
    assert p9.group_key != _make_item("b", 8, 0.7, True, top_p=0.8).group_key
    assert p9.group_key != _make_item("b", 8, 0.7, True, top_p=0.9,
                                      top_k=5).group_key
    # seeded requests never share a wave (row 0 of their own batch)
    assert _make_item("a", 8, 0.7, True, seed=1).group_key != \
        _make_item("a", 8, 0.7, True, seed=1).group_key


def test_dynamic_batcher_passes_sampling_kwargs():
    from sentio_amd.serving.batcher import BatchedGenerator

    rec = _Recorder()
    gen = BatchedGenerator(rec, max_batch=4, max_wait_ms=1.0)
    try:
        gen.generate(["x"], max_new_tokens=4, temperature=0.5, top_p=0.9,
                     seed=4)
        assert rec.calls[-1]["top_p"] == 0.9 and rec.calls[-1]["seed"] == 4
        gen.generate(["x"], max_new_tokens=4, temperature=0.5)
        assert not {"top_p", "top_k", "seed"} & set(rec.calls[-1])
    finally:
        gen.batcher.stop()


def test_cli_flags_parse(monkeypatch):
    import json

    from typer.testing import CliRunner

    from sentio_amd.cli import app, apply_sampling_defaults
    from sentio_amd.config import Settings, reload_settings
    from sentio_amd.serving.container import reset_container

    monkeypatch.setenv("MOCK_COMPUTE", "1")
    monkeypatch.setenv("SENTIO_DEVICE", "cpu")
    reload_settings()
    reset_container()
    runner = CliRunner()
    r = runner.invoke(app, ["chat", "what is top-p?", "--top-p", "0.9",
                            "--sampling-top-k", "50", "--seed", "1"])
    assert r.exit_code == 0, r.output
    assert json.loads(r.output)["answer"]
    assert runner.invoke(app, ["chat", "q", "--top-p", "1.5"]).exit_code != 0
    assert runner.invoke(app, ["chat", "q", "--top-p", "0"]).exit_code != 0
    assert runner.invoke(app, ["chat", "q", "--seed", "-1"]).exit_code != 0
    h = runner.invoke(app, ["run", "--help"])
    assert h.exit_code == 0
    for flag in ("--top-p", "--sampling-top-k", "--seed"):
        assert flag in h.output
    s = Settings()
    apply_sampling_defaults(s, 0.9, 50, 1)
    assert (s.gen_top_p, s.gen_top_k, s.gen_seed) == (0.9, 50, 1)
    reset_container()


def test_mixed_default_and_sampled_requests_concurrently_cpu():
    import threading

    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.serving.batcher import ContinuousGenerator

    eng = GeneratorEngine("tiny-decoder", device="cpu", max_seq=64)
    gen = ContinuousGenerator(eng, slots=2)
    try:
        kw = dict(max_new_tokens=8, temperature=0.7, stop_on_eos=False)
        outs = {}

        def run(name, **extra):
            outs[name] = gen.generate(["mixed"], **kw, **extra)[0]

        th = [threading.Thread(target=run, args=("default",)),
              threading.Thread(target=run, args=("nucleus",),
                               kwargs={"top_p": 0.9})]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join(timeout=60)
        assert isinstance(outs.get("default"), str)
        assert isinstance(outs.get("nucleus"), str)
        assert gen.batcher.stats["completed"] == 1
        assert gen.sampled_batcher.stats["requests"] == 1
    finally:
        gen.batcher.stop()
        gen.sampled_batcher.stop()
