"""FP8 (e4m3fn) KV cache without a GPU: the quantisation spec byte for byte,
the CPU references, the wrapper contract, and the engine running on the
references (GeneratorEngine(..., device="cpu", kv_cache_dtype="fp8"))."""

import pytest
import torch

from sentio_amd import ops
from sentio_amd.ops import torch_ref

# ties-to-even (17, 18, 19 -> 16/18/20 steps of 2), subnormals (2^-9 is the
# smallest, 2^-10 ties to zero, 1.5*2^-9 ties up to 2*2^-9), saturation
# (448 is the largest finite; 464 and above are NaN without the clamp)
TABLE_IN = [0.0, -0.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 448.0, 464.0,
            480.0, 1e9, -1e9, 17.0, 18.0, 19.0, 0.0634765625]
TABLE_BYTES = [0, 128, 1, 0, 2, 126, 126, 126, 126, 254, 88, 89, 90, 24]


def _table():
    return torch.tensor(TABLE_IN, dtype=torch.float32).view(1, 1, -1)


def test_byte_table_scale_one():
    got = torch_ref.kv_quantize(_table(), torch.ones(1))
    assert got.dtype == torch.uint8
    assert got.view(-1).tolist() == TABLE_BYTES
    back = torch_ref.kv_dequantize(got, torch.ones(1)).view(-1)
    assert back[5:10].tolist() == [448.0, 448.0, 448.0, 448.0, -448.0]
    assert back[10:13].tolist() == [16.0, 18.0, 20.0]


def test_byte_table_non_power_of_two_scale():
    scale = torch.tensor([3.0])
    inv = torch.reciprocal(scale)
    x = torch.cat([_table() * 3.0, _table(),
                   torch.randn(1, 1, 4096, generator=torch.Generator()
                               .manual_seed(5)) * 300.0], dim=-1)
    got = torch_ref.kv_quantize(x, inv)
    want = (x.float() * inv).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(got, want.view(torch.uint8))
    assert not bool(((got & 0x7F) == 0x7F).any())      # never NaN bytes
    deq = torch_ref.kv_dequantize(got, scale)
    assert torch.equal(deq, want.float() * 3.0)
    # two heads, two scales: each head uses its own reciprocal
    x2 = torch.randn(2, 5, 8, generator=torch.Generator().manual_seed(6)) * 40
    inv2 = torch.reciprocal(torch.tensor([3.0, 0.5]))
    got2 = torch_ref.kv_quantize(x2, inv2)
    for h in range(2):
        want_h = (x2[h] * inv2[h]).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(got2[h], want_h.view(torch.uint8))


# ---- reference composition

def _fp8_args(D=64, G=2, smax=16, B=2, hkv=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    k_scale = torch.tensor([0.25, 2.0])[:hkv].contiguous()
    v_scale = torch.tensor([0.5, 3.0])[:hkv].contiguous()
    k_inv, v_inv = torch.reciprocal(k_scale), torch.reciprocal(v_scale)
    kc = torch_ref.kv_quantize(torch.randn(B, hkv, smax, D, generator=g),
                               k_inv)
    vc = torch_ref.kv_quantize(torch.randn(B, hkv, smax, D, generator=g),
                               v_inv)
    qkv = torch.randn(B, (G + 2) * hkv * D, generator=g)
    cos, sin = torch_ref.rope_tables(smax, D)
    pos = torch.tensor([0, 5], dtype=torch.int32)[:B].contiguous()
    return qkv, kc, vc, cos, sin, pos, k_scale, v_scale, k_inv, v_inv


def test_fused_fp8_reference_composition():
    """= quantise-write of the prep op's rows + decode_attention over the
    dequantised cache; every row other than pos keeps its bytes."""
    qkv, kc, vc, cos, sin, pos, ks, vs, ki, vi = _fp8_args()
    kc0, vc0 = kc.clone(), vc.clone()
    got = ops.decode_attention_fused_fp8(qkv, kc, vc, cos, sin, pos, ks, vs,
                                         ki, vi)
    assert got.shape == (2, 4, 64)

    # the exact rows, from the bf16-path op on a float staging cache
    B, hkv, smax, D = kc.shape
    k_st, v_st = torch.zeros(B, hkv, smax, D), torch.zeros(B, hkv, smax, D)
    q = ops.decode_qkv_prep(qkv, k_st, v_st, cos, sin, pos)
    kc2, vc2 = kc0.clone(), vc0.clone()
    bidx, rows = torch.arange(B), pos.long()
    kc2[bidx, :, rows] = torch_ref.kv_quantize(k_st, ki)[bidx, :, rows]
    vc2[bidx, :, rows] = torch_ref.kv_quantize(v_st, vi)[bidx, :, rows]
    want = ops.decode_attention(q, torch_ref.kv_dequantize(kc2, ks),
                                torch_ref.kv_dequantize(vc2, vs), pos + 1)
    torch.testing.assert_close(got, want)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    other = torch.ones(B, smax, dtype=torch.bool)
    other[bidx, rows] = False
    assert torch.equal(kc[:, 0][other], kc0[:, 0][other])
    assert torch.equal(vc[:, 1][other], vc0[:, 1][other])
    assert not torch.equal(kc[bidx, :, rows], kc0[bidx, :, rows])
    # reciprocals default to torch.reciprocal of the scales
    got2 = ops.decode_attention_fused_fp8(qkv, kc0.clone(), vc0.clone(), cos,
                                          sin, pos, ks, vs)
    assert torch.equal(got, got2)


def test_kv_store_reference():
    g = torch.Generator().manual_seed(8)
    n, hkv, s_src, D, B, smax = 3, 2, 10, 64, 5, 12
    sk = torch.randn(n, hkv, s_src, D, generator=g) * 8
    sv = torch.randn(n, hkv, s_src, D, generator=g) * 8
    ki = torch.reciprocal(torch.tensor([0.25, 2.0]))
    vi = torch.reciprocal(torch.tensor([0.5, 3.0]))
    kc = torch.full((B, hkv, smax, D), 7, dtype=torch.uint8)
    vc = torch.full((B, hkv, smax, D), 9, dtype=torch.uint8)
    rows, S = [4, 0, 2], 7
    ops.kv_store_fp8(sk, sv, kc, vc, rows, S, ki, vi)
    for i, r in enumerate(rows):
        assert torch.equal(kc[r, :, :S], torch_ref.kv_quantize(sk[i, :, :S], ki))
        assert torch.equal(vc[r, :, :S], torch_ref.kv_quantize(sv[i, :, :S], vi))
        assert bool((kc[r, :, S:] == 7).all()) and bool((vc[r, :, S:] == 9).all())
    for r in (1, 3):
        assert bool((kc[r] == 7).all()) and bool((vc[r] == 9).all())
    # a rows TENSOR may hold out-of-range entries: skipped, as the kernel does
    kc.fill_(7)
    ops.kv_store_fp8(sk, sv, kc, vc, torch.tensor([4, 99, -1]), S, ki, vi)
    assert bool((kc[:4] == 7).all())
    assert torch.equal(kc[4, :, :S], torch_ref.kv_quantize(sk[0, :, :S], ki))


# ---- wrapper contract: one ValueError per validation, nothing written

def test_fused_fp8_wrapper_contract():
    qkv, kc, vc, cos, sin, pos, ks, vs, ki, vi = _fp8_args()
    kc0, vc0 = kc.clone(), vc.clone()
    f = ops.decode_attention_fused_fp8
    with pytest.raises(ValueError, match="uint8"):
        f(qkv, kc.float(), vc.float(), cos, sin, pos, ks, vs, ki, vi)
    with pytest.raises(ValueError, match="equal shape"):
        f(qkv, kc, vc[:, :, :-1], cos, sin, pos, ks, vs, ki, vi)
    with pytest.raises(ValueError, match="qkv width"):
        f(qkv[:, :-8], kc, vc, cos, sin, pos, ks, vs, ki, vi)
    a96 = _fp8_args(D=96)
    with pytest.raises(ValueError, match="head dim"):
        f(*a96)
    a9 = _fp8_args(G=9)
    with pytest.raises(ValueError, match="at most 8"):
        f(*a9)
    with pytest.raises(ValueError, match="seq_lens"):
        f(qkv, kc, vc, cos, sin, pos.long(), ks, vs, ki, vi)
    with pytest.raises(ValueError, match="seq_lens"):
        f(qkv, kc, vc, cos, sin, pos.repeat_interleave(2)[::2], ks, vs, ki, vi)
    with pytest.raises(ValueError, match="seq_lens"):
        f(qkv, kc, vc, cos, sin, pos[:1], ks, vs, ki, vi)
    with pytest.raises(ValueError, match="k_scale"):
        f(qkv, kc, vc, cos, sin, pos, ks.double(), vs, ki, vi)
    with pytest.raises(ValueError, match="v_scale"):
        f(qkv, kc, vc, cos, sin, pos, ks, vs[:1], ki, vi)
    with pytest.raises(ValueError, match="k_inv"):
        f(qkv, kc, vc, cos, sin, pos, ks, vs, ki.view(1, 2), vi)
    with pytest.raises(ValueError, match="v_inv"):
        f(qkv, kc, vc, cos, sin, pos, ks, vs, ki, vi.to("meta"))
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


def test_kv_store_wrapper_contract():
    n, hkv, s_src, D, B, smax = 3, 2, 10, 64, 5, 8
    sk, sv = torch.randn(n, hkv, s_src, D), torch.randn(n, hkv, s_src, D)
    ki, vi = torch.ones(hkv), torch.ones(hkv)
    kc = torch.full((B, hkv, smax, D), 7, dtype=torch.uint8)
    vc = torch.full((B, hkv, smax, D), 7, dtype=torch.uint8)
    f = ops.kv_store_fp8
    with pytest.raises(ValueError, match="uint8"):
        f(sk, sv, kc.float(), vc.float(), [0, 1, 2], 4, ki, vi)
    with pytest.raises(ValueError, match="equal shape"):
        f(sk, sv, kc, vc[:1], [0, 1, 2], 4, ki, vi)
    with pytest.raises(ValueError, match="equal shape"):
        f(sk, sv[:2], kc, vc, [0, 1, 2], 4, ki, vi)
    with pytest.raises(ValueError, match="head dim"):
        f(sk[..., :32], sv[..., :32], kc, vc, [0, 1, 2], 4, ki, vi)
    with pytest.raises(ValueError, match="exceeds"):       # S > Smax
        f(sk, sv, kc, vc, [0, 1, 2], 9, ki, vi)
    with pytest.raises(ValueError, match="exceeds"):       # S > S_src
        f(sk[:, :, :3], sv[:, :, :3], kc, vc, [0, 1, 2], 4, ki, vi)
    with pytest.raises(ValueError, match="outside"):
        f(sk, sv, kc, vc, [0, 1, 5], 4, ki, vi)
    with pytest.raises(ValueError, match="outside"):
        f(sk, sv, kc, vc, [0, -1, 2], 4, ki, vi)
    with pytest.raises(ValueError, match="duplicate"):
        f(sk, sv, kc, vc, [0, 1, 1], 4, ki, vi)
    with pytest.raises(ValueError, match="rows for"):
        f(sk, sv, kc, vc, [0, 1], 4, ki, vi)
    with pytest.raises(ValueError, match="k_inv"):
        f(sk, sv, kc, vc, [0, 1, 2], 4, ki[:1], vi)
    with pytest.raises(ValueError, match="v_inv"):
        f(sk, sv, kc, vc, [0, 1, 2], 4, ki, vi.double())
    assert bool((kc == 7).all()) and bool((vc == 7).all())
    assert "decode_attention_fused_fp8" in ops.__all__
    assert "kv_store_fp8" in ops.__all__


# ---- model and engine on the CPU references

def test_kvcache_dtypes():
    from sentio_amd.engines.configs import MODEL_CONFIGS
    from sentio_amd.engines.transformer import KVCache, Transformer

    cfg = MODEL_CONFIGS["tiny-decoder64"]
    c = KVCache(cfg, 2, 16, "cpu", torch.float32)
    assert c.kv_dtype == "bf16" and c.scales is None
    assert c.k[0].dtype == torch.float32
    c8 = KVCache(cfg, 2, 16, "cpu", torch.float32, kv_dtype="fp8")
    assert c8.k[0].dtype == torch.uint8 and c8.v[-1].dtype == torch.uint8
    assert c8.k[0].shape == c.k[0].shape
    assert len(c8.scales) == cfg.n_layers
    assert c8.scales[0].shape == (4, cfg.n_kv_heads)
    assert bool((c8.scales[0] == 1).all())
    with pytest.raises(ValueError, match="kv cache dtype"):
        KVCache(cfg, 2, 16, "cpu", torch.float32, kv_dtype="e5m2")
    with pytest.raises(ValueError, match="scales"):
        c.set_scales([], [])
    # prefill never writes an fp8 cache directly
    m = Transformer(cfg, device="cpu", seed=11)
    with pytest.raises(ValueError, match="staging"):
        m.prefill(torch.zeros(2, 4, dtype=torch.int64), c8)


def test_fp8_rejected_where_the_engine_is_built(monkeypatch):
    import dataclasses

    from sentio_amd.engines import configs
    from sentio_amd.engines.generator import GeneratorEngine
    from sentio_amd.engines.transformer import KVCache

    base = configs.MODEL_CONFIGS["tiny-decoder64"]
    with pytest.raises(ValueError, match="kv cache dtype"):
        GeneratorEngine("tiny-decoder64", device="cpu", kv_cache_dtype="int4")
    wide = dataclasses.replace(base, n_heads=base.n_kv_heads * 16,
                               dim=base.n_kv_heads * 16 * 64)
    with pytest.raises(ValueError, match="at most 8"):
        KVCache(wide, 1, 8, "cpu", torch.float32, kv_dtype="fp8")
    d96 = dataclasses.replace(base, dim=base.n_heads * 96)
    assert d96.head_dim == 96
    with pytest.raises(ValueError, match="head dim"):
        KVCache(d96, 1, 8, "cpu", torch.float32, kv_dtype="fp8")
    monkeypatch.setitem(configs.MODEL_CONFIGS, "tiny-wide-gqa", wide)
    with pytest.raises(ValueError, match="at most 8"):
        GeneratorEngine("tiny-wide-gqa", device="cpu", kv_cache_dtype="fp8")
    monkeypatch.setenv("SENTIO_DECODE_ATTN", "bmm")
    with pytest.raises(ValueError, match="bmm"):
        GeneratorEngine("tiny-decoder64", device="cpu", kv_cache_dtype="fp8")
    GeneratorEngine("tiny-decoder64", device="cpu")      # bf16 + bmm still fine


@pytest.fixture(scope="module")
def engines():
    from sentio_amd.engines.generator import GeneratorEngine

    e8 = GeneratorEngine("tiny-decoder64", device="cpu", seed=11,
                         kv_cache_dtype="fp8")
    e16 = GeneratorEngine("tiny-decoder64", device="cpu", seed=11)
    return e8, e16


def test_engine_generates_on_cpu(engines):
    e8, e16 = engines
    prompts = ["what is a kv cache?", "fp8 halves it"]
    out = e8.generate(prompts, max_new_tokens=6, temperature=0.0,
                      stop_on_eos=False)
    assert len(out) == 2 and all(isinstance(t, str) and t for t in out)
    sess = e8._sessions[(2, e8.max_seq)]
    assert all(k.dtype == torch.uint8 for k in sess.cache.k + sess.cache.v)
    assert sess.cache.scales is e8._kv_scales
    assert e16.kv_cache_dtype == "bf16"
    assert e8.kv_bytes_per_token * 2 == e16.kv_bytes_per_token
    cfg = e8.cfg
    assert e8.kv_bytes_per_token == 2 * cfg.n_layers * cfg.n_kv_heads \
        * cfg.head_dim


def test_engine_logits_gap_against_exact_cache(engines):
    """Seed 11, torch.manual_seed(7), B=2, S=24, six decode steps: the max
    logits gap of the fp8-cache session against the exact-cache one is
    real (> 0) and small (<= 0.05; measured 0.0174 at a logits std of
    0.32, deterministic on CPU, bound ~3x for torch-version differences)."""
    e8, e16 = engines
    Bm, S, steps = 2, 24, 6
    torch.manual_seed(7)
    toks = torch.randint(0, e8.cfg.vocab_size, (Bm, S + steps))
    s8 = e8._decode_session(Bm, 64)
    s16 = e16._decode_session(Bm, 64)
    with torch.inference_mode():
        l8, l16 = s8.prefill(toks[:, :S]), s16.prefill(toks[:, :S])
        # prefill ran on exact K/V in both
        torch.testing.assert_close(l8, l16, rtol=0, atol=1e-6)
        assert s8.cache.seq_lens.tolist() == [S, S]
        gap = 0.0
        for i in range(steps):
            t = toks[:, S + i:S + i + 1]
            l8, l16 = s8.decode_step(t), s16.decode_step(t)
            gap = max(gap, float((l8 - l16).abs().max()))
    assert s8.cache.seq_lens.tolist() == [S + steps] * Bm
    print(f"fp8-vs-exact max logits gap {gap:.4f}, logits std "
          f"{float(l16.std()):.3f}")
    assert 0.0 < gap <= 0.05
    # stored prompt rows are the spec's bytes of the exact rows
    sc = s8.cache.scales[0]
    assert torch.equal(s8.cache.k[0][:, :, :S],
                       torch_ref.kv_quantize(s16.cache.k[0][:, :, :S], sc[2]))
    assert float(s8.cache.k[0][:, :, S + steps:].sum()) == 0


def test_engine_prefix_and_slot_paths(engines):
    """prefill_with_prefix and integrate_admission (with an idx subset)
    splice through the same helper in both dtypes."""
    e8, e16 = engines
    ids = list(range(3, 3 + 70))
    suffix = torch.tensor([[5, 6, 7, 8], [9, 10, 11, 0]])
    lens = torch.tensor([4, 3], dtype=torch.int32)
    with torch.inference_mode():
        s8, s16 = e8._decode_session(2, 96), e16._decode_session(2, 96)
        l8 = s8.prefill_with_prefix(ids, suffix, lens)
        l16 = s16.prefill_with_prefix(ids, suffix, lens)
    torch.testing.assert_close(l8, l16, rtol=0, atol=1e-6)
    assert s8.cache.seq_lens.tolist() == s16.cache.seq_lens.tolist() == [74, 73]
    sc = s8.cache.scales[1]
    assert torch.equal(s8.cache.v[1][:, :, :74],
                       torch_ref.kv_quantize(s16.cache.v[1][:, :, :74], sc[3]))
    # the prefix store stays in the model dtype
    assert all(k.dtype == torch.float32 for k in e8._prefix_store[tuple(ids)][0])

    prompts = ["first admitted prompt", "the second one, longer than the first"]
    slot8, slot16 = e8.make_slot_session(4), e16.make_slot_session(4)
    for eng, sl in ((e8, slot8), (e16, slot16)):
        pre = eng.prefill_admission(prompts, [4, 4])
        assert pre["tmp"].k[0].dtype == torch.float32
        eng.integrate_admission(sl, [2], pre, idx=[1])
    n = int(slot16.cache.seq_lens[2])
    assert slot8.cache.seq_lens.tolist() == [0, 0, n, 0]
    assert torch.equal(
        slot8.cache.k[0][2, :, :n],
        torch_ref.kv_quantize(slot16.cache.k[0][2, :, :n], sc[2]))
    assert float(slot8.cache.k[0][[0, 1, 3]].sum()) == 0
    with pytest.raises(ValueError, match="bad cache rows"):
        e8.integrate_admission(slot8, [1, 1], pre)


def test_set_and_calibrate_kv_scales():
    from sentio_amd.engines.generator import GeneratorEngine

    e = GeneratorEngine("tiny-decoder64", device="cpu", seed=11,
                        kv_cache_dtype="fp8")
    L, hkv = e.cfg.n_layers, e.cfg.n_kv_heads
    held = e._kv_scales[0]
    e.set_kv_scales([[2.0] * hkv] * L, [torch.full((hkv,), 3.0)] * L)
    assert e._kv_scales[0] is held                      # in place
    assert held[0].tolist() == [2.0] * hkv and held[1].tolist() == [3.0] * hkv
    assert torch.equal(held[2:], torch.reciprocal(held[:2]))
    with pytest.raises(ValueError, match="per-layer"):
        e.set_kv_scales([[1.0] * hkv], [[1.0] * hkv])
    with pytest.raises(ValueError, match="per layer"):
        e.set_kv_scales([[1.0] * (hkv + 1)] * L, [[1.0] * hkv] * L)
    with pytest.raises(ValueError, match="positive"):
        e.set_kv_scales([[0.0] * hkv] * L, [[1.0] * hkv] * L)
    assert held[0].tolist() == [2.0] * hkv              # failed calls wrote nothing
    with pytest.raises(ValueError, match="fp8"):
        GeneratorEngine("tiny-decoder64", device="cpu").set_kv_scales([], [])

    # a checkpoint with outliers: layer 0's K projection x1000.  At scale 1
    # its K saturates; after calibration no stored byte is +-448.
    hd = e.cfg.head_dim
    q_end = e.cfg.n_heads * hd
    e.model.w.layers[0]["wqkv"][q_end:q_end + hkv * hd] *= 1000.0
    prompts = ["calibration prompt one", "and a second, different, prompt"]
    e.set_kv_scales([[1.0] * hkv] * L, [[1.0] * hkv] * L)
    sess = e.make_slot_session(2)
    e.prefill_into_slots(sess, [0, 1], prompts, [4, 4])
    k0 = sess.cache.k[0]
    assert bool(((k0 == 126) | (k0 == 254)).any())       # saturated

    ks, vs = e.calibrate_kv_scales(prompts, margin=2.0)
    assert len(ks) == L and ks[0].shape == (hkv,)
    assert float(ks[0].min()) > 10 * float(ks[1].max())
    assert e._kv_scales[0] is held
    e.prefill_into_slots(sess, [0, 1], prompts, [4, 4])
    n = int(sess.cache.seq_lens.max())
    for li in range(L):
        for t in (sess.cache.k[li], sess.cache.v[li]):
            assert not bool(((t == 126) | (t == 254)).any())
    # margin 2: the largest stored magnitude sits at half of 448 (byte
    # 0x76 = 224 +- one e4m3 step)
    top = int((sess.cache.k[0][:, :, :n] & 0x7F).max())
    assert 0x74 <= top <= 0x77
    # the floor: an all-zero V head still gets a usable scale
    e.model.w.layers[1]["wqkv"][q_end + hkv * hd:] = 0
    ks, vs = e.calibrate_kv_scales(prompts)
    assert vs[1].tolist() == [2.0 ** -20] * hkv


def test_settings_kv_cache_dtype(monkeypatch):
    from sentio_amd.config import Settings

    monkeypatch.delenv("KV_CACHE_DTYPE", raising=False)
    assert Settings.from_env().kv_cache_dtype == "bf16"
    monkeypatch.setenv("KV_CACHE_DTYPE", "fp8")
    assert Settings.from_env().kv_cache_dtype == "fp8"
    monkeypatch.setenv("KV_CACHE_DTYPE", "fp4")
    with pytest.raises(ValueError, match="KV_CACHE_DTYPE"):
        Settings.from_env()
