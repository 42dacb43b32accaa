"""The FP8 KV cache on the reference path (CPU): the quantisation law ``ops.kv_cache.quantize_kv_ref``, the math
reference of the decode attention with per-row scales, and ``CausalLM.generate(kv_dtype="fp8")``.

Bounds.  The law is checked exactly where it is exact (``scale == amax / 448`` by an IEEE fp32 division, done here
by numpy) and by e4m3fn's own precision elsewhere: a normal code carries 3 mantissa bits, so round-to-nearest
leaves at most 2^-4 of the value, and below the smallest normal (2^-6 in code units) the spacing is 2^-9, so at
most 2^-10 of the scale: ``|x - deq| <= max(|x| 2^-4, scale 2^-10)``.  ``attn_decode_ref`` with scales is held to
the reference bounds of ``tests/decode_cases.py`` against the same function in fp64 on the dequantised cache
``float64(code) * float64(scale)`` -- quantisation is not an error there.  Against the UNQUANTISED fp64 oracle the
bounds are 0.12 of the row's largest element (ctx) and 0.02 (1 + A) (lse): about 1.5 times what the reference
measures on these 56 cases (0.078 and 0.011), far below the order-1 error of a dropped or swapped scale.  ``A`` is
the unquantised case's score magnitude: a property of the inputs.
"""
import numpy as np
import pytest
import torch

from distributed_training_and_deepspeed_amd.memory import kv_cache_bytes
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache, dequantize_kv, quantize_kv_ref

from . import decode_cases as DC
from .decode_fp8_cases import FP8, dequantized_oracle, quantized_case

Q_CTX_TOL, Q_LSE_TOL = 0.12, 0.02


def _ref(c, kq, vq, ks, vs, qkv=None):
    return A.attn_decode_ref(c.qkv if qkv is None else qkv, kq, vq, c.kv_len, c.B, c.H, c.D, c.Hkv, c.W, c.kv_start,
                             k_scale=ks, v_scale=vs)


# ------------------------------------------------------------------------------------- the law
@pytest.mark.parametrize("p", DC.all_cases(), ids=DC.case_id)
def test_quantisation_law(p):
    c = DC.decode_case(*p)
    for x in (c.k, c.v):
        x = x.clone()
        x[0, 0, 3] = 0                                           # a zero row: scale 1, codes 0
        x[1, 0, 5] = 0
        x[1, 0, 5, 7] = -0.375                                   # a row of a single non-zero element
        code, scale = quantize_kv_ref(x)
        assert code.dtype == FP8 and code.shape == x.shape and scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
        xf = x.float()
        amax = xf.abs().amax(-1)
        want = torch.from_numpy(amax.numpy() / np.float32(448.0))
        assert want.dtype == torch.float32
        want[amax == 0] = 1.0
        assert torch.equal(scale, want)                          # exactly amax / 448
        assert float(scale[0, 0, 3]) == 1.0 and bool((code[0, 0, 3].view(torch.uint8) & 0x7F == 0).all())
        assert float(code[1, 0, 5, 7].float()) == -448.0 and int((code[1, 0, 5].float() != 0).sum()) == 1
        cf = code.float()
        assert not bool(torch.isnan(cf).any())
        deq = dequantize_kv(code, scale)
        assert torch.equal(deq, cf * scale.unsqueeze(-1))
        bound = torch.maximum(xf.abs() * 2.0 ** -4, scale.unsqueeze(-1) * 2.0 ** -10)
        assert bool(((xf - deq).abs() <= bound).all())


def test_rounding_is_to_nearest_even():
    x = torch.tensor([17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -10, 448.0])
    assert x.to(FP8).float().tolist() == [16.0, 20.0, 0.0, 2.0 ** -9, 448.0]


# ------------------------------------------------------------------------------------- attn_decode_ref with scales
@pytest.mark.parametrize("p", DC.all_cases(), ids=DC.case_id)
def test_ref_with_scales_against_the_oracle_on_the_dequantised_cache(p):
    c = DC.decode_case(*p)
    q = quantized_case(p)
    d = dequantized_oracle(p)
    ctx, lse = _ref(c, *q)
    assert ctx.dtype == torch.bfloat16 and tuple(ctx.shape) == (c.B, c.H * c.D) and lse.dtype == torch.float32
    e = DC.check_decode(d, ctx, lse, DC.REF_CTX_TOL, DC.REF_LSE_TOL, DC.case_id(p))
    # the routed entry point takes the reference here (CPU) and agrees with it bitwise
    c2, l2 = A.attn_decode(c.qkv, q[0], q[1], c.kv_len, c.B, c.H, c.D, c.Hkv, c.W, c.kv_start, k_scale=q[2], v_scale=q[3])
    assert torch.equal(c2, ctx) and torch.equal(l2, lse)
    # fp32 activations: far inside the bf16 bound
    c3, l3 = _ref(c, *q, qkv=c.qkv.float())
    e3 = DC.check_decode(d, c3, l3, 5e-5, DC.REF_LSE_TOL, DC.case_id(p) + " fp32")
    print(f"{DC.case_id(p)}: bf16 ctx {e[0]:.2e} lse {e[1]:.2e}; fp32 ctx {e3[0]:.2e} lse {e3[1]:.2e}")


@pytest.mark.parametrize("p", DC.all_cases(), ids=DC.case_id)
def test_quantisation_effect_against_the_unquantised_oracle(p):
    c = DC.decode_case(*p)
    ctx, lse = _ref(c, *quantized_case(p))
    e = DC.check_decode(c, ctx, lse, Q_CTX_TOL, Q_LSE_TOL, DC.case_id(p))
    print(f"{DC.case_id(p)}: quantisation effect ctx {e[0]:.3e} lse {e[1]:.3e}")


def _tile_scale(s):
    j = torch.arange(s.shape[-1])
    return s[..., j // DC.KT * DC.KT]


MUTANTS = {                    # (k_scale, v_scale) -> what a faulty implementation would apply
    "K scale ignored": lambda ks, vs: (torch.ones_like(ks), vs),
    "V scale ignored": lambda ks, vs: (ks, torch.ones_like(vs)),
    "scales swapped": lambda ks, vs: (vs, ks),
    "scale of the slot's tile": lambda ks, vs: (_tile_scale(ks), _tile_scale(vs)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_bounds_catch_mutants(mutant):
    caught = 0
    for p in DC.all_cases():
        c = DC.decode_case(*p)
        kq, vq, ks, vs = quantized_case(p, poison=False)        # (finite everywhere: a mutant is caught by its error)
        d = dequantized_oracle(p)
        got = _ref(c, kq, vq, *MUTANTS[mutant](ks, vs))
        try:
            DC.check_decode(d, *got, DC.REF_CTX_TOL, DC.REF_LSE_TOL)
            DC.check_decode(c, *got, Q_CTX_TOL, Q_LSE_TOL)
        except AssertionError:
            caught += 1
    print(f"mutant {mutant}: caught on {caught} of {len(DC.all_cases())} cases")
    assert caught > 0


def test_scale_arguments_are_validated():
    p = (DC.HEADS[1], DC.LENS[0], None, 0, "gauss")
    c = DC.decode_case(*p)
    kq, vq, ks, vs = quantized_case(p)
    args = (c.kv_len, c.B, c.H, c.D, c.Hkv)
    for fn in (A.attn_decode, A.attn_decode_ref):
        with pytest.raises(ValueError):
            fn(c.qkv, kq, vq, *args)                             # FP8 caches without scales
        with pytest.raises(ValueError):
            fn(c.qkv, kq, vq, *args, k_scale=ks)
        with pytest.raises(ValueError):
            fn(c.qkv, kq, vq, *args, k_scale=ks[:, :, :-1], v_scale=vs)
        with pytest.raises(ValueError):
            fn(c.qkv, kq, vq, *args, k_scale=ks.double(), v_scale=vs)
        with pytest.raises(ValueError):
            fn(c.qkv, kq, c.v, *args, k_scale=ks, v_scale=vs)   # one cache FP8, the other not
        with pytest.raises(ValueError):
            fn(c.qkv, c.k, c.v, *args, k_scale=ks, v_scale=vs)   # scales with a bf16 cache


# ------------------------------------------------------------------------------------- rope_append_ (PyTorch branch)
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (2, 1, 128), (2, 2, 32)])
@pytest.mark.parametrize("Sq", [1, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_append_fp8_cpu_branch(H, Hkv, D, Sq, dtype):
    B, Smax = 3, 20
    table = Fx.rope_table(64, D)
    g = torch.Generator().manual_seed(5)
    qkv0 = torch.randn(B * Sq, (H + 2 * Hkv) * D, generator=g).to(dtype)
    qkv0.view(B, Sq, H + 2 * Hkv, D)[0, 0, H + Hkv] = 0         # a zero v row
    for kv_len, over in (((0, 5, Smax - Sq), False), ((0, Smax - Sq + 1, Smax + 3), True)):
        n = torch.tensor(kv_len, dtype=torch.int32)
        kc, vc = (torch.full((B, Hkv, Smax, D), 0x7F, dtype=torch.uint8).view(FP8) for _ in range(2))
        ks, vs = (torch.full((B, Hkv, Smax), -77.0) for _ in range(2))
        flag = torch.zeros(1, dtype=torch.int32)
        qkv = qkv0.clone()
        assert Fx.rope_append_(qkv, table, kc, vc, n, B, Sq, H, D, kv_heads=Hkv, overflow=flag, k_scale=ks, v_scale=vs) is qkv
        ref_k, ref_v = (torch.zeros((B, Hkv, Smax, D), dtype=dtype) for _ in range(2))
        want = Fx.rope_append_(qkv0.clone(), table, ref_k, ref_v, n, B, Sq, H, D, kv_heads=Hkv)
        assert torch.equal(qkv, want)                           # bitwise the unquantised call's qkv
        x = want.view(B, Sq, H + 2 * Hkv, D)
        for cache, sc, new in ((kc, ks, x[:, :, H:H + Hkv]), (vc, vs, x[:, :, H + Hkv:])):
            code, scale = quantize_kv_ref(new)
            e_code, e_scale = torch.full_like(cache.view(torch.uint8), 0x7F), torch.full_like(sc, -77.0)
            for b in range(B):
                for s in range(Sq):
                    if kv_len[b] + s < Smax:
                        e_code[b, :, kv_len[b] + s] = code[b, s].view(torch.uint8)
                        e_scale[b, :, kv_len[b] + s] = scale[b, s]
            assert torch.equal(cache.view(torch.uint8), e_code) and torch.equal(sc, e_scale)
        assert int(flag) == int(over) and n.tolist() == list(kv_len)
    assert float(vs[0, 0, 0]) == 1.0 and bool((vc[0, 0, 0].view(torch.uint8) == 0).all())
    with pytest.raises(ValueError):
        Fx.rope_append_(qkv0.clone(), table, kc, vc, n, B, Sq, H, D, kv_heads=Hkv)                   # no scales
    with pytest.raises(ValueError):
        Fx.rope_append_(qkv0.clone(), table, kc, vc, n, B, Sq, H, D, kv_heads=Hkv, k_scale=ks, v_scale=vs[:, :, 1:])


# ------------------------------------------------------------------------------------- cache and model
def test_allocate_and_bytes():
    cfg = build_model("llama-tiny-gqa", impl="reference").cfg
    B, Smax = 3, 40
    L, Hkv, D = cfg.num_layers, cfg.kv_heads, cfg.head_dim
    plain = kv_cache_bytes(cfg, B, Smax, torch.bfloat16)
    assert kv_cache_bytes(cfg, B, Smax, torch.bfloat16, None) == plain == kv_cache_bytes(cfg, B, Smax, torch.bfloat16, torch.bfloat16)
    want = 2 * L * B * Hkv * Smax * (D + 4)
    assert kv_cache_bytes(cfg, B, Smax, torch.bfloat16, "fp8") == want == kv_cache_bytes(cfg, B, Smax, torch.float32, FP8)
    for kv in ("fp8", FP8):
        cache = KVCache.allocate(cfg, B, Smax, "cpu", torch.float32, kv_dtype=kv)
        assert cache.quantized and cache.nbytes() == want
        assert cache.k.dtype == cache.v.dtype == FP8 and tuple(cache.k.shape) == tuple(cache.v.shape) == (L, B, Hkv, Smax, D)
        for s in (cache.k_scale, cache.v_scale):
            assert s.dtype == torch.float32 and tuple(s.shape) == (L, B, Hkv, Smax)
        ks, vs = cache.layer_scales(1)
        assert ks.data_ptr() == cache.k_scale[1].data_ptr() and tuple(vs.shape) == (B, Hkv, Smax)
        assert cache.kv_len.tolist() == [0] * B and cache.kv_next.tolist() == [1] * B
    for kv in (None, torch.float32):
        cache = KVCache.allocate(cfg, B, Smax, "cpu", torch.float32, kv_dtype=kv)
        assert not cache.quantized and cache.k.dtype == torch.float32 and cache.layer_scales(0) == (None, None)
        assert cache.nbytes() == kv_cache_bytes(cfg, B, Smax, torch.float32)
    for bad in (torch.float16, "int8", torch.float8_e5m2):
        with pytest.raises(ValueError):
            KVCache.allocate(cfg, B, Smax, "cpu", torch.float32, kv_dtype=bad)
        with pytest.raises(ValueError):
            kv_cache_bytes(cfg, B, Smax, torch.float32, bad)
    # the README's example: Llama-3-8B at B = 8, Smax = 8192
    from distributed_training_and_deepspeed_amd.models.config import get_config
    big = get_config("llama-3-8b")
    assert kv_cache_bytes(big, 8, 8192, torch.bfloat16, "fp8") == 2 * 32 * 8 * 8 * 8192 * 132


SIZES = {"llama-tiny-gqa": (12, 16), "mistral-tiny": (40, 24)}       # (S0, N): 64 > window 48


def _model(name):
    return build_model(name, impl="reference", seed=1).eval()


@pytest.mark.parametrize("name", list(SIZES))
def test_generate_with_an_fp8_cache(name):
    model = _model(name)
    cfg = model.cfg
    S0, N = SIZES[name]
    ids = torch.randint(3, cfg.vocab_size, (2, S0 + N), generator=torch.Generator().manual_seed(1))
    caches = []
    out = model.generate(ids[:, :S0], N, kv_dtype="fp8", cache_out=caches)
    assert out.dtype == torch.int64 and tuple(out.shape) == (2, S0 + N) and torch.equal(out[:, :S0], ids[:, :S0])
    cache = caches[0]
    assert cache.quantized and cache.nbytes() == kv_cache_bytes(cfg, 2, S0 + N, torch.float32, kv_dtype="fp8")
    assert int(cache.overflow) == 0 and cache.kv_len.tolist() == [S0 + N - 1] * 2
    assert torch.equal(out, model.generate(ids[:, :S0], N, kv_dtype=FP8))
    # teacher-forced per-step logits against the unquantised cache: e_q, recorded
    q8 = KVCache.allocate(cfg, 2, S0 + N, "cpu", torch.float32, kv_dtype="fp8")
    un = KVCache.allocate(cfg, 2, S0 + N, "cpu", torch.float32)
    worst = 0.0
    for t in range(N):
        a, b = ((model.prefill(ids[:, :S0], ch) if t == 0 else model.decode_step(ids[:, S0 + t - 1], ch)) for ch in (q8, un))
        e_q = float((a - b).abs().max())
        print(f"{name} step {t}: e_q {e_q:.3e} (logits up to {float(b.abs().max()):.2f})")
        assert e_q == e_q and e_q != float("inf") and (t > 0 or e_q == 0.0)     # the prompt's attention is unquantised
        worst = max(worst, e_q)
    print(f"{name}: largest e_q {worst:.3e}")
    for other in ("causal-tiny", "mixtral-tiny"):
        m = build_model(other, impl="reference")
        with pytest.raises(NotImplementedError):
            m.generate(torch.randint(3, m.cfg.vocab_size, (2, 8)), 4, kv_dtype="fp8")


@pytest.mark.parametrize("name", list(SIZES))
def test_left_padded_batch_equals_its_parts(name):
    """As ``tests/test_kv_cache_cpu.py``: greedy tokens of the batch equal those of each sequence alone, exactly."""
    model, N = _model(name), 16
    g = torch.Generator().manual_seed(1)
    cfg = model.cfg
    a, b = torch.randint(3, cfg.vocab_size, (1, 12), generator=g), torch.randint(3, cfg.vocab_size, (1, 7), generator=g)
    ids = torch.cat([a, torch.cat([torch.full((1, 5), cfg.pad_token_id), b], 1)], 0)
    mask = torch.ones(2, 12, dtype=torch.int64)
    mask[1, :5] = 0
    out = model.generate(ids, N, attention_mask=mask, kv_dtype="fp8")
    assert torch.equal(out[0], model.generate(a, N, kv_dtype="fp8")[0])
    assert torch.equal(out[1, 5:], model.generate(b, N, kv_dtype="fp8")[0])
    assert torch.equal(out[:, :12], ids)
