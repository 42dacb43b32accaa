"""KV cache and incremental decoding on the reference path (fp32, CPU): ``CausalLM.generate`` / ``prefill`` /
``decode_step``, ``ops.kv_cache.KVCache``, the math reference of the decode attention and the PyTorch branch of
``rope_append_``.

Bounds.  Greedy tokens are compared exactly, under a precondition on the INPUTS computed here: the smallest
top-2 logit gap of the fp64 model over all steps is >= 1e-3, a thousand times the fp32 logit error (< 1e-6),
so no argmax can flip by rounding.  Measured: 9.0e-3 (llama-tiny), 9.6e-3 (llama-tiny-gqa), 3.4e-3
(mistral-tiny) with seed 1; seeds 0 and 2 do not meet it.  Cached logits: the error against the fp64 model is
at most twice the uncached fp32 model's, measured per step in the test, plus 1e-6.  ``attn_decode_ref`` is held
to the reference bounds of ``tests/test_attention_oracles_cpu.py`` (ctx 5e-3 of the row's largest element --
the bf16 output's half ulp is 3.9e-3 --, lse 2.5e-6 (1 + A)) against the fp64 oracle.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.memory import kv_cache_bytes
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models.config import get_config
from distributed_training_and_deepspeed_amd.models.llama import to_hf_state_dict
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

from . import decode_cases as DC
from .conftest import pick_free_port

GAP = 1e-3
SIZES = {"llama-tiny": (12, 16), "llama-tiny-gqa": (12, 16), "mistral-tiny": (40, 24)}   # (S0, N): 64 > window 48
PAD_SEED = 1        # the first seed in 1..8 whose left-padded batch meets the gap precondition


def _model(name, seed=1):
    return build_model(name, impl="reference", seed=seed).eval()


def _prompt(cfg, S0, seed=1, B=2):
    return torch.randint(3, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(seed))


def _greedy_uncached(model, ids, N, attention_mask=None):
    """(tokens [B, S0 + N], smallest top-2 logit gap over the steps) by re-running the whole prefix."""
    gap = float("inf")
    mask = attention_mask
    with torch.no_grad():
        for _ in range(N):
            lg = model(ids, attention_mask=mask).logits[:, -1]
            top = lg.topk(2, -1).values
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
            ids = torch.cat([ids, lg.argmax(-1, keepdim=True)], 1)
            if mask is not None:
                mask = torch.cat([mask, mask.new_ones(mask.shape[0], 1)], 1)
    return ids, gap


def _hf_model(tf, name, model):
    cfg = model.cfg
    kw = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.ffn_size,
              num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.kv_heads,
              max_position_embeddings=cfg.max_positions, rms_norm_eps=cfg.ln_eps, rope_theta=cfg.rope_theta,
              hidden_act="silu", tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="eager",
              pad_token_id=cfg.pad_token_id, bos_token_id=None, eos_token_id=None)
    if cfg.sliding_window:
        hf = tf.MistralForCausalLM(tf.MistralConfig(sliding_window=cfg.sliding_window, **kw))
    else:
        hf = tf.LlamaForCausalLM(tf.LlamaConfig(attention_bias=False, mlp_bias=False, **kw))
    hf = hf.float().eval()
    res = hf.load_state_dict(to_hf_state_dict(model.state_dict()), strict=False)
    assert not res.unexpected_keys and all("rotary" in k for k in res.missing_keys), res
    return hf


# ------------------------------------------------------------------------------------- generation
@pytest.mark.parametrize("name", list(SIZES))
def test_greedy_tokens_equal_hf_generate(name):
    tf = pytest.importorskip("transformers")
    model = _model(name)
    S0, N = SIZES[name]
    ids = _prompt(model.cfg, S0)
    _, gap = _greedy_uncached(_model(name).double(), ids, N)
    print(f"{name}: smallest top-2 gap of the fp64 model {gap:.2e}")
    assert gap >= GAP, f"precondition on the inputs: top-2 gap {gap:.2e} < {GAP}"
    out = model.generate(ids, N)
    assert out.dtype == torch.int64 and tuple(out.shape) == (2, S0 + N)
    hf = _hf_model(tf, name, model)
    with torch.no_grad():
        ref = hf.generate(ids, attention_mask=torch.ones_like(ids), do_sample=False, max_new_tokens=N, min_new_tokens=N)
    assert torch.equal(out, ref)
    assert torch.equal(out, _greedy_uncached(model, ids, N)[0])


@pytest.mark.parametrize("name", list(SIZES))
def test_cached_logits_equal_the_uncached_models_teacher_forced(name):
    model, m64 = _model(name), _model(name).double()
    S0, N = SIZES[name]
    ids = _prompt(model.cfg, S0 + N)
    cache = KVCache.allocate(model.cfg, 2, S0 + N, "cpu", torch.float32)
    worst = 0.0
    with torch.no_grad():
        got = [model.prefill(ids[:, :S0], cache)]
        for t in range(N - 1):
            got.append(model.decode_step(ids[:, S0 + t], cache))
        for t in range(N):
            pre = ids[:, :S0 + t]
            r64 = m64(pre).logits[:, -1]
            e_unc = float((model(pre).logits[:, -1].double() - r64).abs().max())
            e_cached = float((got[t].double() - r64).abs().max())
            print(f"{name} step {t}: cached {e_cached:.2e}, uncached {e_unc:.2e}")
            assert e_cached <= 2 * e_unc + 1e-6, (t, e_cached, e_unc)
            worst = max(worst, e_cached)
    assert int(cache.overflow) == 0 and cache.filled == S0 + N - 1
    assert cache.kv_len.tolist() == [S0 + N - 1] * 2 and cache.kv_next.tolist() == [S0 + N] * 2


def _padded_batch(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randint(3, cfg.vocab_size, (1, 12), generator=g), torch.randint(3, cfg.vocab_size, (1, 7), generator=g)
    ids = torch.cat([a, torch.cat([torch.full((1, 5), cfg.pad_token_id), b], 1)], 0)
    mask = torch.ones(2, 12, dtype=torch.int64)
    mask[1, :5] = 0
    return a, b, ids, mask


@pytest.mark.parametrize("name", list(SIZES))
def test_left_padded_batch_equals_its_parts(name):
    model, N = _model(name), 16
    a, b, ids, mask = _padded_batch(model.cfg, PAD_SEED)
    m64 = _model(name).double()
    gaps = [_greedy_uncached(m64, p, N)[1] for p in (a, b)]
    print(f"{name}: top-2 gaps of the fp64 model {gaps}")
    assert min(gaps) >= GAP, f"precondition on the inputs: top-2 gap {min(gaps):.2e} < {GAP}"
    out = model.generate(ids, N, attention_mask=mask)
    assert torch.equal(out[0], model.generate(a, N)[0])
    assert torch.equal(out[1, 5:], model.generate(b, N)[0])
    assert torch.equal(out[:, :12], ids)


def test_sampling_eos_and_mode():
    model = _model("llama-tiny-gqa")
    ids = _prompt(model.cfg, 9)
    model.train()
    a = model.generate(ids, 12, do_sample=True, temperature=0.8, top_k=5, seed=3)
    assert model.training                                        # the caller's mode is restored
    model.eval()
    b = model.generate(ids, 12, do_sample=True, temperature=0.8, top_k=5, seed=3)
    assert not model.training and torch.equal(a, b)             # seeded
    assert not torch.equal(a, model.generate(ids, 12, do_sample=True, temperature=0.8, top_k=5, seed=4))
    # top_k = 1 is greedy
    greedy = model.generate(ids, 12)
    assert torch.equal(greedy, model.generate(ids, 12, do_sample=True, top_k=1, seed=9))
    # after the eos token a sequence emits the pad token; all steps run
    eos = int(greedy[0, 9 + 3])
    out = model.generate(ids, 12, eos_token_id=eos)
    first = (greedy[0, 9:] == eos).nonzero()[0, 0]
    assert torch.equal(out[0, :9 + first + 1], greedy[0, :9 + first + 1])
    assert bool((out[0, 9 + first + 1:] == model.cfg.pad_token_id).all()) and out.shape == greedy.shape
    assert tuple(model.generate(ids, 0).shape) == (2, 9)


@pytest.fixture
def gloo_world1(monkeypatch):
    from distributed_training_and_deepspeed_amd import comm
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(pick_free_port()))
    comm.init(rank=0, world_size=1, backend="gloo")
    yield
    comm.destroy()


def test_error_cases():
    model = _model("llama-tiny")
    ids = _prompt(model.cfg, 8)
    holes = torch.ones(2, 8, dtype=torch.int64)
    holes[0, 3] = 0                                             # a 0 after a 1: not left-padded
    with pytest.raises(ValueError):
        model.generate(ids, 4, attention_mask=holes)
    right = torch.ones(2, 8, dtype=torch.int64)
    right[1, 6:] = 0
    with pytest.raises(ValueError):
        model.generate(ids, 4, attention_mask=right)
    with pytest.raises(ValueError):
        model.generate(ids, 5, max_len=12)                      # S0 + N > max_len
    with pytest.raises(ValueError):
        KVCache.allocate(model.cfg, 2, model.cfg.max_positions + 1, "cpu", torch.float32)    # the rotary table
    with pytest.raises(ValueError):
        model.generate(ids, model.cfg.max_positions, max_len=None)
    cache = KVCache.allocate(model.cfg, 2, 16, "cpu", torch.float32)
    with pytest.raises(ValueError):
        model.decode_step(ids[:, 0], cache)                     # nothing prefilled
    model.prefill(ids, cache)
    with pytest.raises(ValueError):
        model.prefill(ids, cache)                               # needs an empty cache
    cache.reset()
    assert cache.filled == 0 and cache.kv_len.tolist() == [0, 0] and cache.kv_next.tolist() == [1, 1]
    model.prefill(ids, cache)
    for name in ("causal-tiny", "mixtral-tiny"):                # learned positions; mixture of experts
        other = build_model(name, impl="reference")
        with pytest.raises(NotImplementedError):
            other.generate(_prompt(other.cfg, 8), 4)


def test_a_zero_wrapped_model_is_refused(gloo_world1):
    from distributed_training_and_deepspeed_amd.parallel.zero import ZeroEngine
    model = _model("llama-tiny")
    ids = _prompt(model.cfg, 8)
    zcfg = {"optimizer": {"type": "Adam", "params": {"lr": 1e-3}}, "comms_logger": {"enabled": False},
            "zero_optimization": {"stage": 1}}
    model.generate(ids, 4)
    eng = ZeroEngine(model, zcfg, model.parameters())
    with pytest.raises(NotImplementedError):
        eng.module.generate(ids, 4)
    cache = KVCache.allocate(model.cfg, 2, 16, "cpu", torch.float32)
    with pytest.raises(NotImplementedError):
        model.prefill(ids, cache)


@pytest.mark.parametrize("name,dtype", [("llama-tiny", torch.float32), ("llama-tiny-gqa", torch.bfloat16),
                                        ("mistral-7b", torch.bfloat16)])
def test_kv_cache_bytes(name, dtype):
    cfg = get_config(name)
    B, Smax = 3, 40
    want = 2 * cfg.num_layers * B * cfg.kv_heads * Smax * cfg.head_dim * (4 if dtype == torch.float32 else 2)
    assert kv_cache_bytes(cfg, B, Smax, dtype) == want
    if cfg.num_layers <= 2:
        cache = KVCache.allocate(cfg, B, Smax, "cpu", dtype)
        assert cache.nbytes() == want == sum(t.numel() * t.element_size() for t in (cache.k, cache.v))
        k, v = cache.layer(1)
        assert tuple(k.shape) == tuple(v.shape) == (B, cfg.kv_heads, Smax, cfg.head_dim) and k.dtype == dtype
        assert cache.workspace.numel() >= A.decode_workspace_floats(B, cfg.num_heads, cfg.head_dim, cache.splits)


# ------------------------------------------------------------------------------------- attn_decode_ref
def _ref(c, kv_len=None, window=None, kv_start=None):
    return A.attn_decode_ref(c.qkv, c.k, c.v, c.kv_len if kv_len is None else kv_len, c.B, c.H, c.D, c.Hkv,
                             c.W if window is None else window, c.kv_start if kv_start is None else kv_start)


@pytest.mark.parametrize("p", DC.all_cases(), ids=DC.case_id)
def test_attn_decode_ref_against_the_oracle(p):
    c = DC.decode_case(*p)
    ctx, lse = _ref(c)
    assert ctx.dtype == torch.bfloat16 and tuple(ctx.shape) == (c.B, c.H * c.D) and lse.dtype == torch.float32
    e = DC.check_decode(c, ctx, lse, DC.REF_CTX_TOL, DC.REF_LSE_TOL, DC.case_id(p))
    print(f"{DC.case_id(p)}: ctx {e[0]:.2e} lse {e[1]:.2e} staged {c.e_staged:.2e}")
    # the routed entry point takes the reference here (CPU) and agrees with it bitwise
    c2, l2 = A.attn_decode(c.qkv, c.k, c.v, c.kv_len, c.B, c.H, c.D, c.Hkv, c.W, c.kv_start)
    assert torch.equal(c2, ctx) and torch.equal(l2, lse)
    # fp32 inputs: far inside the bf16 bound
    c3, l3 = A.attn_decode_ref(c.qkv.float(), c.k.float(), c.v.float(), c.kv_len, c.B, c.H, c.D, c.Hkv, c.W, c.kv_start)
    DC.check_decode(c, c3, l3, 5e-5, DC.REF_LSE_TOL, DC.case_id(p) + " fp32")


def _wrong_group(c):
    """Query head h reading key/value head h % Hkv instead of h // G: the cache expanded in that order."""
    idx = torch.arange(c.H) % c.Hkv
    q = c.qkv[:, :c.H * c.D]
    qkv = torch.cat([q, q, q], 1)                         # only the q block is read
    return A.attn_decode_ref(qkv, c.k[:, idx].contiguous(), c.v[:, idx].contiguous(), c.kv_len, c.B, c.H, c.D, c.H,
                             c.W, c.kv_start)


MUTANTS = {
    "kv_len + 1": lambda c: _ref(c, kv_len=c.kv_len + 1),
    "W + 1": lambda c: _ref(c, window=c.W + 1) if c.W else _ref(c),
    "kv_start - 1": lambda c: _ref(c, kv_start=c.kv_start - 1) if c.kv_start is not None else _ref(c),
    "h % Hkv": _wrong_group,
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_bound_catches_mutants(mutant):
    caught = 0
    for p in DC.all_cases():
        c = DC.decode_case(*p)
        try:
            DC.check_decode(c, *MUTANTS[mutant](c), DC.REF_CTX_TOL, DC.REF_LSE_TOL)
        except AssertionError:
            caught += 1
    print(f"mutant {mutant}: caught on {caught} of {len(DC.all_cases())} cases")
    assert caught > 0


def test_decode_splits_rule():
    assert A.DECODE_KEY_TILE == 64
    for B, Hkv, Smax in ((1, 8, 8192), (64, 32, 4096), (1, 1, 200), (8, 4, 64), (4, 2, 2048)):
        s = A.decode_splits(B, Hkv, Smax)
        tiles = -(-Smax // A.DECODE_KEY_TILE)
        assert 1 <= s <= max(1, tiles) and s == A.decode_splits(B, Hkv, Smax)
    assert A.decode_splits(64, 32, 4096) == 1                   # the grid is covered without splitting
    assert A.decode_splits(1, 8, 8192) > 1


# ------------------------------------------------------------------------------------- rope_append_
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 64), (4, 2, 64), (2, 1, 128)])
@pytest.mark.parametrize("Sq", [1, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_append_cpu_branch(H, Hkv, D, Sq, dtype):
    B, Smax, SENT = 3, 20, -77.0
    table = Fx.rope_table(64, D)
    g = torch.Generator().manual_seed(5)
    qkv0 = torch.randn(B * Sq, (H + 2 * Hkv) * D, generator=g).to(dtype)
    for kv_len, over in (((0, 5, Smax - Sq), False), ((0, Smax - Sq + 1, Smax + 3), True)):
        n = torch.tensor(kv_len, dtype=torch.int32)
        kc, vc = (torch.full((B, Hkv, Smax, D), SENT, dtype=dtype) for _ in range(2))
        flag = torch.zeros(1, dtype=torch.int32)
        qkv = qkv0.clone()
        assert Fx.rope_append_(qkv, table, kc, vc, n, B, Sq, H, D, kv_heads=Hkv, overflow=flag) is qkv
        want = Fx.rope_(qkv0.clone(), table, B, Sq, H, D, pos=n.view(B, 1) + torch.arange(Sq), kv_heads=Hkv)
        assert torch.equal(qkv, want)                           # bitwise: the same rotation
        x = want.view(B, Sq, H + 2 * Hkv, D)
        for cache, new in ((kc, x[:, :, H:H + Hkv]), (vc, x[:, :, H + Hkv:])):
            expect = torch.full_like(cache, SENT)
            for b in range(B):
                for s in range(Sq):
                    if kv_len[b] + s < Smax:
                        expect[b, :, kv_len[b] + s] = new[b, s]
            assert torch.equal(cache, expect)                   # the rows, and the sentinel everywhere else
        assert int(flag) == int(over)
        assert n.tolist() == list(kv_len)                       # not advanced
