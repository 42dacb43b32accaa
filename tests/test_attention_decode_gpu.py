"""The decode-attention kernels (ops/csrc/attention_decode.hip) on the GPU: ``dtd_attn_decode`` against the
fp64 oracle on the cases of ``tests/decode_cases.py``, and ``dtd_rope_append`` bitwise against ``Fx.rope_`` + a copy.

Bound (the project's bf16 one, tests/test_attention_oracles_cpu.py): per (sequence, head) ctx error against the
row's largest element <= min(2e-2, 4 e_staged), e_staged the error of ``oracles.attention_staged`` on the
decoded rows of that very case; |lse error| <= 1e-5 (1 + A); ctx = 0 and lse = -inf exactly on a row without a
key.  Neither comes from a kernel's result.

Memory safety is checked without provoking anything: the K / V caches, ctx, lse and the workspace are slices
out of the middle of larger sentinel-filled buffers whose guard regions -- and every cache slot -- must be
unchanged after each call, and every cache slot outside a sequence's [lo, hi) holds NaN, so a read of a slot
that takes no part shows in the result.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx

from . import decode_cases as DC
from .decode_cases import SENT, bits as _bits, guarded as _guarded, guards_intact as _guards_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _poisoned(c):
    """The case's K / V with NaN in every slot outside [lo, hi) of its sequence."""
    j = torch.arange(DC.SMAX).view(1, 1, DC.SMAX, 1)
    dead = (j < c.lo.view(-1, 1, 1, 1)) | (j >= c.hi.view(-1, 1, 1, 1))
    return c.k.masked_fill(dead, float("nan")), c.v.masked_fill(dead, float("nan"))


def _run(c, splits, kv_len=None):
    """One guarded kernel call; asserts guards and caches unchanged; returns (ctx, lse) on the CPU."""
    k0, v0 = _poisoned(c)
    kb, k = _guarded(k0.shape, torch.bfloat16, k0)
    vb, v = _guarded(v0.shape, torch.bfloat16, v0)
    cb, ctx = _guarded((c.B, c.H * c.D), torch.bfloat16)
    lb, lse = _guarded((c.B, c.H), torch.float32)
    s = min(splits or A.decode_splits(c.B, c.Hkv, DC.SMAX), -(-DC.SMAX // DC.KT))
    need = A.decode_workspace_floats(c.B, c.H, c.D, s)
    wb, ws = _guarded((need,), torch.float32)
    kv_len = (c.kv_len if kv_len is None else kv_len).to(DEV)
    start = c.kv_start.to(DEV) if c.kv_start is not None else None
    assert A.decode_kernel_supported(c.qkv.to(DEV), c.H, c.Hkv, c.D)
    out = A.attn_decode(c.qkv.to(DEV), k, v, kv_len, c.B, c.H, c.D, c.Hkv, c.W, start, splits=splits,
                        workspace=ws, out=(ctx, lse))
    torch.cuda.synchronize()
    assert out[0] is ctx and out[1] is lse
    for buf, n in ((kb, k.numel()), (vb, v.numel()), (cb, ctx.numel()), (lb, lse.numel()), (wb, need)):
        assert _guards_intact(buf, n), "a guard region was written"
    assert torch.equal(_bits(k.cpu()), _bits(k0)) and torch.equal(_bits(v.cpu()), _bits(v0)), "the cache was written"
    return ctx.cpu().clone(), lse.cpu().clone()


def _check(p, splits_list):
    c = DC.decode_case(*p)
    tol = min(DC.CAP_BF16, 4 * c.e_staged)
    for splits in splits_list:
        ctx, lse = _run(c, splits)
        e = DC.check_decode(c, ctx, lse, tol, DC.LSE_TOL, f"{DC.case_id(p)} splits={splits}")
        print(f"{DC.case_id(p)} splits={splits}: ctx {e[0]:.2e} (tol {tol:.2e}) lse {e[1]:.2e}")


def test_key_tile_is_the_kernels():
    assert _lib.lib().dtd_attn_decode_key_tile() == A.DECODE_KEY_TILE == DC.KT


@pytest.mark.parametrize("p", DC.base_cases(), ids=DC.case_id)
def test_decode_against_the_oracle(p):
    _check(p, DC.SPLITS)


@pytest.mark.parametrize("p", DC.pad_cases(), ids=DC.case_id)
def test_left_padding(p):
    _check(p, (4, None))
    c = DC.decode_case(*p)
    ctx, lse = _run(c, 4)
    assert bool((ctx[-1] == 0).all()) and bool((lse[-1] == float("-inf")).all())     # kv_start == kv_len


@pytest.mark.parametrize("p", DC.window_cases(), ids=DC.case_id)
def test_window(p):
    _check(p, (1, 4, None))


@pytest.mark.parametrize("heads", DC.HEADS, ids=str)
def test_determinism_and_clamping(heads):
    for p in ((heads, DC.LENS[0], None, 0, "spikes_up"), (heads, (DC.SMAX,) * 4, (0, 10, 100, 199), DC.KT + 7, "gauss")):
        c = DC.decode_case(*p)
        for splits in (4, None):
            a, b = _run(c, splits), _run(c, splits)
            assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    # a kv_len beyond the cache is clamped: exactly the result of kv_len = Smax
    c = DC.decode_case(heads, (1, DC.KT + 1, DC.SMAX, DC.SMAX), None, 0, "gauss")
    a = _run(c, 4)
    b = _run(c, 4, kv_len=torch.tensor([1, DC.KT + 1, DC.SMAX + 5, 2 ** 31 - 1], dtype=torch.int32))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_routing_to_the_reference():
    """G = 16 and fp32 inputs are outside the kernel's domain: they take the reference, bitwise."""
    B, H, Hkv, D = 2, 16, 1, 64
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16).to(DEV)
    k, v = (torch.randn(B, Hkv, 70, D, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    n = torch.tensor([70, 33], dtype=torch.int32, device=DEV)
    assert not A.decode_kernel_supported(qkv, H, Hkv, D)
    got, ref = A.attn_decode(qkv, k, v, n, B, H, D, Hkv), A.attn_decode_ref(qkv, k, v, n, B, H, D, Hkv)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    c = DC.decode_case(DC.HEADS[1], DC.LENS[0], None, 0, "gauss")
    args = (c.qkv.float().to(DEV), c.k.float().to(DEV), c.v.float().to(DEV), c.kv_len.to(DEV), c.B, c.H, c.D, c.Hkv)
    got, ref = A.attn_decode(*args), A.attn_decode_ref(*args)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    DC.check_decode(c, got[0], got[1], 5e-5, DC.LSE_TOL, "fp32 routing")


def test_launcher_rejections():
    """Null pointers, H % Hkv, a row stride that is no multiple of 8 and a short workspace are error codes."""
    c = DC.decode_case(DC.HEADS[1], DC.LENS[0], None, 0, "gauss")
    qkv, k, v, n = c.qkv.to(DEV), c.k.to(DEV), c.v.to(DEV), c.kv_len.to(DEV)
    ctx = torch.empty((c.B, c.H * c.D), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((c.B, c.H), dtype=torch.float32, device=DEV)
    ws = torch.empty(A.decode_workspace_floats(c.B, c.H, c.D, 4), dtype=torch.float32, device=DEV)
    good = dict(q=qkv.data_ptr(), ldq=qkv.stride(0), k=k.data_ptr(), v=v.data_ptr(), n=n.data_ptr(), start=None,
                ctx=ctx.data_ptr(), ldo=c.H * c.D, lse=lse.data_ptr(), ws=ws.data_ptr(), wsn=ws.numel(), B=c.B, H=c.H,
                Hkv=c.Hkv, D=c.D, Smax=DC.SMAX, W=0, scale=0.125, splits=4)

    def call(**kw):
        a = {**good, **kw}
        _lib.call("dtd_attn_decode", *a.values(), _lib.stream())

    call()
    torch.cuda.synchronize()
    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(n=None), dict(ctx=None), dict(lse=None), dict(ws=None),
                dict(Hkv=3), dict(ldq=qkv.stride(0) + 4), dict(wsn=ws.numel() - 1), dict(D=96), dict(splits=0)):
        with pytest.raises(_lib.KernelError):
            call(**bad)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- dtd_rope_append
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 64), (4, 2, 64), (2, 1, 128)])
@pytest.mark.parametrize("Sq", [1, 70])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_rope_append(H, Hkv, D, Sq, dtype):
    B, Smax = 3, 100
    table = Fx.rope_table(128, D, device=DEV)
    g = torch.Generator().manual_seed(7)
    qkv0 = torch.randn(B * Sq, (H + 2 * Hkv) * D, generator=g).to(dtype).to(DEV)
    for kv_len, over in (((0, 5, Smax - Sq), False), ((0, Smax - Sq + 1, Smax + 3), True)):
        n = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
        kb, kc = _guarded((B, Hkv, Smax, D), dtype)
        vb, vc = _guarded((B, Hkv, Smax, D), dtype)
        qb, qkv = _guarded(tuple(qkv0.shape), dtype, qkv0)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        Fx.rope_append_(qkv, table, kc, vc, n, B, Sq, H, D, kv_heads=Hkv, overflow=flag)
        torch.cuda.synchronize()
        pos = n.view(B, 1) + torch.arange(Sq, device=DEV, dtype=torch.int32)
        want = Fx.rope_(qkv0.clone(), table, B, Sq, H, D, pos=pos, kv_heads=Hkv)
        assert torch.equal(_bits(qkv), _bits(want))             # bitwise Fx.rope_
        x = want.view(B, Sq, H + 2 * Hkv, D)
        for cache, new in ((kc, x[:, :, H:H + Hkv]), (vc, x[:, :, H + Hkv:])):
            expect = torch.full_like(cache, SENT)
            for b in range(B):
                m = max(0, min(Sq, Smax - kv_len[b]))           # rows of sequence b that fit
                expect[b, :, kv_len[b]:kv_len[b] + m] = new[b, :m].transpose(0, 1)
            assert torch.equal(_bits(cache), _bits(expect))     # the rows, and the sentinel in every other slot
        for buf, t in ((kb, kc), (vb, vc), (qb, qkv)):
            assert _guards_intact(buf, t.numel())
        assert int(flag) == int(over) and n.tolist() == list(kv_len)
