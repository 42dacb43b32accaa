"""The FP8 KV-cache kernels (ops/csrc/attention_decode.hip) on the GPU: ``dtd_rope_append_fp8`` bitwise against
``Fx.rope_append_`` on a bf16 cache (the qkv) and ``ops.kv_cache.quantize_kv_ref`` (codes and scales), and
``dtd_attn_decode_fp8`` against the fp64 oracle on the DEQUANTISED cache (``tests/decode_fp8_cases.py``) on the
cases of ``tests/decode_cases.py``.

Bounds: the project's bf16 ones, as for the bf16 kernel -- quantisation is not an error against this oracle: per
(sequence, head) ctx error against the row's largest element <= 2e-2, |lse error| <= 1e-5 (1 + A); ctx = 0 and
lse = -inf exactly on a row without a key.  The append has no tolerance: codes and scales are compared as bits.

Memory safety as in ``test_attention_decode_gpu.py``, without provoking anything: every buffer a kernel reads or
writes is a slice out of the middle of a larger sentinel-filled one whose guard regions -- and, for the decode
kernel, every cache and scale slot -- must be unchanged after each call; every slot outside a sequence's
[lo, hi) holds the NaN code 0x7F and a NaN scale, so a read of a slot that takes no part shows in the result.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.kv_cache import quantize_kv_ref

from . import decode_cases as DC
from .decode_cases import SENT, SENT_CODE, bits as _bits, guarded as _guarded, guards_intact as _guards_intact
from .decode_fp8_cases import FP8, dequantized_oracle, quantized_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------- dtd_rope_append_fp8
@pytest.mark.parametrize("H,Hkv,D", DC.HEADS, ids=str)
@pytest.mark.parametrize("Sq", [1, 5])
def test_rope_append_fp8(H, Hkv, D, Sq):
    B, Smax, kv_len = 3, 40, (0, 7, 38)                          # the third sequence overflows at Sq = 5
    over = Sq == 5
    table = Fx.rope_table(128, D, device=DEV)
    g = torch.Generator().manual_seed(7)
    qkv0 = torch.randn(B * Sq, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    qkv0.view(B, Sq, H + 2 * Hkv, D)[1, 0, H + Hkv] = 0          # a zero v row: scale 1, codes 0
    qkv0 = qkv0.to(DEV)
    n = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    # the bf16 cache's call: what qkv must be afterwards, bit for bit
    want = qkv0.clone()
    Fx.rope_append_(want, table, *(torch.zeros((B, Hkv, Smax, D), dtype=torch.bfloat16, device=DEV) for _ in range(2)),
                    n, B, Sq, H, D, kv_heads=Hkv)
    kb, kc = _guarded((B, Hkv, Smax, D), torch.uint8)
    vb, vc = _guarded((B, Hkv, Smax, D), torch.uint8)
    ksb, ks = _guarded((B, Hkv, Smax), torch.float32)
    vsb, vs = _guarded((B, Hkv, Smax), torch.float32)
    qb, qkv = _guarded(tuple(qkv0.shape), torch.bfloat16, qkv0)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = Fx.rope_append_(qkv, table, kc.view(FP8), vc.view(FP8), n, B, Sq, H, D, kv_heads=Hkv, overflow=flag,
                          k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert out is qkv and torch.equal(_bits(qkv), _bits(want))
    x = want.cpu().view(B, Sq, H + 2 * Hkv, D)
    for cache, sc, new in ((kc, ks, x[:, :, H:H + Hkv]), (vc, vs, x[:, :, H + Hkv:])):
        code, scale = quantize_kv_ref(new)                       # on the CPU
        e_code = torch.full((B, Hkv, Smax, D), SENT_CODE, dtype=torch.uint8)
        e_scale = torch.full((B, Hkv, Smax), SENT)
        for b in range(B):
            m = max(0, min(Sq, Smax - kv_len[b]))                # rows of sequence b that fit
            e_code[b, :, kv_len[b]:kv_len[b] + m] = code[b, :m].view(torch.uint8).transpose(0, 1)
            e_scale[b, :, kv_len[b]:kv_len[b] + m] = scale[b, :m].transpose(0, 1)
        assert torch.equal(cache.cpu(), e_code), "codes: the rows, and the sentinel in every other slot"
        assert torch.equal(_bits(sc.cpu()), _bits(e_scale)), "scales: the rows, and the sentinel in every other slot"
    assert float(vs[1, 0, kv_len[1]]) == 1.0 and bool((vc[1, 0, kv_len[1]] == 0).all())
    for buf, t in ((kb, kc), (vb, vc), (ksb, ks), (vsb, vs), (qb, qkv)):
        assert _guards_intact(buf, t.numel())
    assert int(flag) == int(over) and n.tolist() == list(kv_len)


# ------------------------------------------------------------------------------------- dtd_attn_decode_fp8
def _run(p, splits, kv_len=None, kv_start=None):
    """One guarded kernel call; asserts guards, caches and scales unchanged; returns (ctx, lse) on the CPU."""
    c = DC.decode_case(*p)
    k0, v0, ks0, vs0 = quantized_case(p)
    kb, k = _guarded(k0.shape, torch.uint8, k0.view(torch.uint8))
    vb, v = _guarded(v0.shape, torch.uint8, v0.view(torch.uint8))
    ksb, ks = _guarded(ks0.shape, torch.float32, ks0)
    vsb, vs = _guarded(vs0.shape, torch.float32, vs0)
    cb, ctx = _guarded((c.B, c.H * c.D), torch.bfloat16)
    lb, lse = _guarded((c.B, c.H), torch.float32)
    s = min(splits or A.decode_splits(c.B, c.Hkv, DC.SMAX), -(-DC.SMAX // DC.KT))
    need = A.decode_workspace_floats(c.B, c.H, c.D, s)
    wb, ws = _guarded((need,), torch.float32)
    kv_len = (c.kv_len if kv_len is None else kv_len).to(DEV)
    start = c.kv_start if kv_start is None else kv_start
    start = start.to(DEV) if start is not None else None
    qkv = c.qkv.to(DEV)
    assert A.decode_kernel_supported(qkv, c.H, c.Hkv, c.D)
    out = A.attn_decode(qkv, k.view(FP8), v.view(FP8), kv_len, c.B, c.H, c.D, c.Hkv, c.W, start, splits=splits,
                        workspace=ws, out=(ctx, lse), k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert out[0] is ctx and out[1] is lse
    for buf, n in ((kb, k.numel()), (vb, v.numel()), (ksb, ks.numel()), (vsb, vs.numel()), (cb, ctx.numel()),
                   (lb, lse.numel()), (wb, need)):
        assert _guards_intact(buf, n), "a guard region was written"
    assert torch.equal(k.cpu(), k0.view(torch.uint8)) and torch.equal(v.cpu(), v0.view(torch.uint8)), "the cache was written"
    assert torch.equal(_bits(ks.cpu()), _bits(ks0)) and torch.equal(_bits(vs.cpu()), _bits(vs0)), "the scales were written"
    return ctx.cpu().clone(), lse.cpu().clone()


@pytest.mark.parametrize("p", DC.all_cases(), ids=DC.case_id)
def test_decode_fp8_against_the_oracle_on_the_dequantised_cache(p):
    d = dequantized_oracle(p)
    for splits in DC.SPLITS:
        ctx, lse = _run(p, splits)
        e = DC.check_decode(d, ctx, lse, DC.CAP_BF16, DC.LSE_TOL, f"{DC.case_id(p)} splits={splits}")
        print(f"{DC.case_id(p)} splits={splits}: ctx {e[0]:.2e} lse {e[1]:.2e}")
        dead = torch.isinf(d.lse)
        assert bool((ctx.view(d.B, d.H, d.D)[dead] == 0).all()) and bool((lse[dead] == float("-inf")).all())


@pytest.mark.parametrize("heads", DC.HEADS, ids=str)
def test_determinism_and_clamping(heads):
    for p in ((heads, DC.LENS[0], None, 0, "spikes_up"), (heads, (DC.SMAX,) * 4, (0, 10, 100, 199), DC.KT + 7, "gauss")):
        for splits in (4, None):
            a, b = _run(p, splits), _run(p, splits)
            assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    # a kv_len beyond the cache is clamped: exactly the result of kv_len = Smax; a negative kv_start: exactly 0
    p = (heads, (1, DC.KT + 1, DC.SMAX, DC.SMAX), None, 0, "gauss")
    a = _run(p, 4)
    b = _run(p, 4, kv_len=torch.tensor([1, DC.KT + 1, DC.SMAX + 5, 2 ** 31 - 1], dtype=torch.int32),
             kv_start=torch.tensor([0, -3, -(2 ** 31), 0], dtype=torch.int32))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_routing_and_rejections():
    """G = 16 and fp32 activations are outside the kernel's domain: they take the reference, bitwise.  FP8 caches
    without their scales, or with scales of another shape or dtype, are a ValueError."""
    B, H, Hkv, D = 2, 16, 1, 64
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16).to(DEV)
    (k, ks), (v, vs) = (quantize_kv_ref(torch.randn(B, Hkv, 70, D, generator=g).to(torch.bfloat16)) for _ in range(2))
    k, ks, v, vs = (t.to(DEV) for t in (k, ks, v, vs))
    n = torch.tensor([70, 33], dtype=torch.int32, device=DEV)
    assert not A.decode_kernel_supported(qkv, H, Hkv, D)
    got = A.attn_decode(qkv, k, v, n, B, H, D, Hkv, k_scale=ks, v_scale=vs)
    ref = A.attn_decode_ref(qkv, k, v, n, B, H, D, Hkv, k_scale=ks, v_scale=vs)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    p = (DC.HEADS[1], DC.LENS[0], None, 0, "gauss")
    c, d = DC.decode_case(*p), dequantized_oracle(p)
    k, v, ks, vs = (t.to(DEV) for t in quantized_case(p))
    args = (c.kv_len.to(DEV), c.B, c.H, c.D, c.Hkv)
    got = A.attn_decode(c.qkv.float().to(DEV), k, v, *args, k_scale=ks, v_scale=vs)
    ref = A.attn_decode_ref(c.qkv.float().to(DEV), k, v, *args, k_scale=ks, v_scale=vs)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    DC.check_decode(d, got[0], got[1], 5e-5, DC.LSE_TOL, "fp32 routing")
    qkv = c.qkv.to(DEV)
    for bad in (dict(), dict(k_scale=ks), dict(v_scale=vs), dict(k_scale=ks[:, :, :-1], v_scale=vs),
                dict(k_scale=ks, v_scale=vs.view(-1)), dict(k_scale=ks.double(), v_scale=vs),
                dict(k_scale=ks.to(torch.bfloat16), v_scale=vs.to(torch.bfloat16))):
        with pytest.raises(ValueError):
            A.attn_decode(qkv, k, v, *args, **bad)
    with pytest.raises(ValueError):
        A.attn_decode(qkv, c.k.to(DEV), c.v.to(DEV), *args, k_scale=ks, v_scale=vs)      # scales with a bf16 cache


def test_launcher_rejections():
    """Null pointers -- the scales' among them -- and any D but 64 / 128 are error codes, in both entry points."""
    p = (DC.HEADS[1], DC.LENS[0], None, 0, "gauss")
    c = DC.decode_case(*p)
    k, v, ks, vs = (t.to(DEV) for t in quantized_case(p, poison=False))
    qkv, n = c.qkv.to(DEV), c.kv_len.to(DEV)
    ctx = torch.empty((c.B, c.H * c.D), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((c.B, c.H), dtype=torch.float32, device=DEV)
    ws = torch.empty(A.decode_workspace_floats(c.B, c.H, c.D, 4), dtype=torch.float32, device=DEV)
    good = dict(q=qkv.data_ptr(), ldq=qkv.stride(0), k=k.data_ptr(), v=v.data_ptr(), ks=ks.data_ptr(), vs=vs.data_ptr(),
                n=n.data_ptr(), start=None, ctx=ctx.data_ptr(), ldo=c.H * c.D, lse=lse.data_ptr(), ws=ws.data_ptr(),
                wsn=ws.numel(), B=c.B, H=c.H, Hkv=c.Hkv, D=c.D, Smax=DC.SMAX, W=0, scale=0.125, splits=4)

    def call(**kw):
        _lib.call("dtd_attn_decode_fp8", *{**good, **kw}.values(), _lib.stream())

    call()
    torch.cuda.synchronize()
    for bad in (dict(ks=None), dict(vs=None), dict(q=None), dict(k=None), dict(v=None), dict(n=None), dict(ctx=None),
                dict(lse=None), dict(ws=None), dict(Hkv=3), dict(ldq=qkv.stride(0) + 4), dict(wsn=ws.numel() - 1),
                dict(D=96), dict(D=32), dict(D=256), dict(splits=0)):
        with pytest.raises(_lib.KernelError):
            call(**bad)
    torch.cuda.synchronize()

    Sq, Smax = 1, DC.SMAX
    table = Fx.rope_table(256, c.D, device=DEV)
    kc, vc = (torch.zeros((c.B, c.Hkv, Smax, c.D), dtype=torch.uint8, device=DEV) for _ in range(2))
    s1, s2 = (torch.zeros((c.B, c.Hkv, Smax), dtype=torch.float32, device=DEV) for _ in range(2))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    zero = torch.zeros(c.B, dtype=torch.int32, device=DEV)
    q2 = qkv.clone()                                             # rotated in place by the good call
    good2 = dict(qkv=q2.data_ptr(), table=table.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(), ks=s1.data_ptr(),
                 vs=s2.data_ptr(), n=zero.data_ptr(), flag=flag.data_ptr(), B=c.B, Sq=Sq, H=c.H, Hkv=c.Hkv, D=c.D,
                 ld=qkv.stride(0), Smax=Smax, P=256)

    def append(**kw):
        _lib.call("dtd_rope_append_fp8", *{**good2, **kw}.values(), _lib.stream())

    append()
    torch.cuda.synchronize()
    for bad in (dict(ks=None), dict(vs=None), dict(qkv=None), dict(table=None), dict(kc=None), dict(vc=None), dict(n=None),
                dict(flag=None), dict(Hkv=3), dict(D=96), dict(D=32), dict(D=16), dict(ld=qkv.stride(0) + 4), dict(Smax=0)):
        with pytest.raises(_lib.KernelError):
            append(**bad)
    torch.cuda.synchronize()
    assert int(flag) == 0
