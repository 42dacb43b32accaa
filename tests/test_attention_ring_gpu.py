"""The ring KV-cache kernels (ops/csrc/attention_ring.hip) on the GPU, R = 128 slots (two key tiles).

Append: slot p mod R of the ring equals, bit for bit, what the linear ``rope_append_`` wrote at position p of a
linear cache (rows, codes and scales), qkv is rotated identically, every slot the law does not write keeps its
sentinel, and the flag is raised exactly when a position reaches the table's end.

Decode: against ``attn_decode_ref`` in float64 on the LINEAR history with the window -- code the ring does not
touch.  The ring is filled from that history by indexing, and every slot that takes no part holds NaN (bf16 NaN; code
0x7F and a NaN scale), so a read of one shows.  One batch holds every hi of interest -- before the wrap, the seam at
slot 1, inside a tile, on a tile boundary -- and so mixes wrapped and unwrapped sequences.  Bound: that of
``tests/test_attention_decode_gpu.py``, min(2e-2, 4 e_staged) and 1e-5 (1 + A), through ``decode_cases.check_decode``;
for the FP8 ring the case behind A and e_staged is the dequantised cache's (with W = 1 the bf16 case's e_staged is 0:
ctx is a bf16 row of V, while a dequantised row rounds once on its way to bf16 -- which the staged model on it shows).
Every buffer is a slice of a sentinel-filled one whose guards must be intact after each call.
"""
import functools
import types

import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.kv_cache import FP8, dequantize_kv, quantize_kv_ref

from . import decode_cases as DC
from . import oracles as O
from .decode_cases import bits as _bits, guarded as _guarded, guards_intact as _guards_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 128
HI = (1, 64, R - 1, R, R + 1, R + 63, R + 64, 2 * R + 5, 3 * R)
FMT = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": torch.bfloat16}


# ------------------------------------------------------------------------------------- dtd_rope_append_ring[_fp8]
def _caches(B, Hkv, S, D, fmt):
    """Guarded (buffer, view) pairs of a cache of S slots: K, V, and the scales of an FP8 one."""
    dt = torch.uint8 if fmt == "fp8" else FMT[fmt]
    return [_guarded((B, Hkv, S, D), dt) for _ in range(2)] + [_guarded((B, Hkv, S), torch.float32) for _ in range(2 * (fmt == "fp8"))]


def _append(qkv, table, bufs, n, B, Sq, H, Hkv, D, flag, fmt, ring):
    t = [v for _, v in bufs]
    kw = dict(k_scale=t[2], v_scale=t[3]) if fmt == "fp8" else {}
    kc, vc = (t[0].view(FP8), t[1].view(FP8)) if fmt == "fp8" else t[:2]
    Fx.rope_append_(qkv, table, kc, vc, n, B, Sq, H, D, kv_heads=Hkv, overflow=flag, ring=ring, **kw)


@pytest.mark.parametrize("H,Hkv,D", DC.HEADS, ids=str)
@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("Sq", [1, 70, R + 9])
@pytest.mark.parametrize("base", [0, R - 3, 2 * R + 5])
def test_ring_append_equals_the_linear_append(H, Hkv, D, fmt, Sq, base):
    B, P = 3, 420                                   # P table positions: only base = 2R + 5 with Sq = R + 9 passes them
    kv_len = (base, base + 7, base + 70)
    table = Fx.rope_table(P, D, device=DEV)
    n = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    qkv0 = torch.randn(B * Sq, (H + 2 * Hkv) * D, generator=torch.Generator().manual_seed(7)).to(FMT[fmt]).to(DEV)
    lin, ring = _caches(B, Hkv, P, D, fmt), _caches(B, Hkv, R, D, fmt)
    want, (qb, qkv) = qkv0.clone(), _guarded(tuple(qkv0.shape), FMT[fmt], qkv0)
    flags = torch.zeros(2, 1, dtype=torch.int32, device=DEV)
    _append(want, table, lin, n, B, Sq, H, Hkv, D, flags[0], fmt, False)
    _append(qkv, table, ring, n, B, Sq, H, Hkv, D, flags[1], fmt, True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(qkv), _bits(want))
    for (_, full), (buf, got) in zip(lin, ring):
        expect = torch.full_like(got, DC.SENT_CODE if got.dtype == torch.uint8 else DC.SENT)
        for b in range(B):
            p = torch.arange(kv_len[b] + max(0, Sq - R), min(kv_len[b] + Sq, P), device=DEV)
            expect[b, :, p % R] = full[b, :, p]
        assert torch.equal(_bits(got), _bits(expect)), "the rows at p mod R, and the sentinel in every other slot"
        assert _guards_intact(buf, got.numel())
    assert _guards_intact(qb, qkv.numel()) and n.tolist() == list(kv_len)
    assert flags[:, 0].tolist() == [int(kv_len[2] + Sq > P)] * 2


# ------------------------------------------------------------------------------------- dtd_attn_decode_ring[_fp8]
@functools.lru_cache(maxsize=None)
def _case(heads, W, start, fp8):
    """One batch over the linear history of 3R positions: the step's qkv, the ring's tensors, the fp64 oracle."""
    H, Hkv, D = heads
    B, P = len(HI), 3 * R
    qkv, dctx = O.attn_inputs("gauss", B, P, H, D, Hkv, seed=300 + H + D)
    hi = torch.tensor(HI)
    st = (hi - (W + 1) // 2).clamp(min=0) if start == "inside" else torch.full_like(hi, start)
    lo = torch.maximum(st, hi - W)
    b = torch.arange(B)
    c = types.SimpleNamespace(B=B, H=H, Hkv=Hkv, D=D, W=W, kv_len=hi.to(torch.int32), kv_start=st.to(torch.int32))
    x = qkv.double().view(B, P, H + 2 * Hkv, D).clone()
    c.qkv = x[b, hi - 1].reshape(B, -1).to(torch.bfloat16)
    lin = [x[:, :, H:H + Hkv].transpose(1, 2).to(torch.bfloat16), x[:, :, H + Hkv:].transpose(1, 2).to(torch.bfloat16)]
    if fp8:      # the case is the dequantised cache's: A and e_staged are taken on it
        (kq, ks), (vq, vs) = (quantize_kv_ref(t) for t in lin)
        lin, ref_kw = [kq.view(torch.uint8), vq.view(torch.uint8), ks, vs], dict(k_scale=ks, v_scale=vs)
        ref_kv = (kq, vq)
        x[:, :, H:H + Hkv], x[:, :, H + Hkv:] = (dequantize_kv(q8, s, torch.float64).transpose(1, 2) for q8, s in ((kq, ks), (vq, vs)))
    else:
        ref_kw, ref_kv = {}, (lin[0].double(), lin[1].double())
    kw = dict(causal=True, key_range=torch.stack([lo, hi], 1).to(torch.int32), kv_heads=Hkv)
    xs = x.view(B * P, -1)
    o, staged = O.attention(xs, dctx, B, P, H, D, **kw), O.attention_staged(xs, dctx, B, P, H, D, **kw)
    c.A = o["A"][b, :, hi - 1]
    c.e_staged = float(O.slice_errors(staged["ctx"][b, hi - 1], o["ctx"][b, hi - 1]).max())
    ctx, c.lse = A.attn_decode_ref(c.qkv.double(), *ref_kv, hi, B, H, D, Hkv, W, st, **ref_kw)
    c.ctx = ctx.view(B, H, D)
    # the ring: slot u holds position pos(u), NaN unless lo <= pos(u)
    pos = (hi - 1).view(B, 1) - torch.remainder((hi - 1).view(B, 1) - torch.arange(R), R)
    dead = (pos < lo.view(B, 1)).view(B, 1, R)
    pick = pos.clamp(min=0).view(B, 1, R).expand(B, Hkv, R)
    c.ring = []
    for t in lin:
        if t.dim() == 4:
            t, d = t.gather(2, pick.unsqueeze(-1).expand(B, Hkv, R, D)), dead.unsqueeze(-1)
            c.ring.append(t.masked_fill(d, 0x7F) if fp8 else t.masked_fill(d, float("nan")))
        else:
            c.ring.append(t.gather(2, pick).masked_fill(dead, float("nan")))
    return c


def _run(c, splits, kv_len=None, kv_start=None):
    """One guarded kernel call; asserts the guards intact and the ring unchanged; returns (ctx, lse) on the CPU."""
    fp8 = len(c.ring) == 4
    s = min(splits or A.decode_splits(c.B, c.Hkv, R), R // DC.KT)
    bufs = [_guarded(t.shape, t.dtype, t) for t in c.ring]
    bufs += [_guarded((c.B, c.H * c.D), torch.bfloat16), _guarded((c.B, c.H), torch.float32),
             _guarded((A.decode_workspace_floats(c.B, c.H, c.D, s),), torch.float32)]
    t = [v for _, v in bufs]
    k, v = (t[0].view(FP8), t[1].view(FP8)) if fp8 else t[:2]
    kw = dict(k_scale=t[2], v_scale=t[3]) if fp8 else {}
    n, st = ((c.kv_len if kv_len is None else kv_len).to(DEV), (c.kv_start if kv_start is None else kv_start).to(DEV))
    assert A.decode_kernel_supported(c.qkv.to(DEV), c.H, c.Hkv, c.D)
    A.attn_decode(c.qkv.to(DEV), k, v, n, c.B, c.H, c.D, c.Hkv, c.W, st, splits=splits, workspace=t[-1], out=(t[-3], t[-2]),
                  ring=True, **kw)
    torch.cuda.synchronize()
    assert all(_guards_intact(buf, view.numel()) for buf, view in bufs), "a guard region was written"
    assert all(torch.equal(_bits(got.cpu()), _bits(t0)) for got, t0 in zip(t, c.ring)), "the ring was written"
    return t[-3].cpu().clone(), t[-2].cpu().clone()


@pytest.mark.parametrize("heads", DC.HEADS, ids=str)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("W", [1, 65, R - 1, R])
def test_ring_decode_against_the_oracle_on_the_linear_history(heads, fp8, W):
    for start in (0, 5, "inside"):
        c = _case(heads, W, start, fp8)
        tol = min(DC.CAP_BF16, 4 * c.e_staged)
        for splits in (1, 2, None):
            ctx, lse = _run(c, splits)
            e = DC.check_decode(c, ctx, lse, tol, DC.LSE_TOL, f"W={W} start={start} splits={splits}")
            print(f"{heads} W={W} start={start} splits={splits}: ctx {e[0]:.2e} (tol {tol:.2e}) lse {e[1]:.2e}")


@pytest.mark.parametrize("heads", DC.HEADS, ids=str)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_determinism_and_garbage_counters(heads, fp8):
    c = _case(heads, 65, 5, fp8)
    for splits in (2, None):
        a, b = _run(c, splits), _run(c, splits)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    big = 2 ** 31 - 1
    _run(c, 2, kv_len=torch.tensor([-5, big, -big - 1, 0, big - 1, R, 7, big, 3], dtype=torch.int32),
         kv_start=torch.tensor([big, -big - 1, 0, -1, big - 70, big, -9, big - 1, 0], dtype=torch.int32))


def test_rejections():
    c = _case(DC.HEADS[1], 65, 0, False)
    q, k, v, n = c.qkv.to(DEV), c.ring[0].to(DEV), c.ring[1].to(DEV), c.kv_len.to(DEV)
    for window, kk, vv in ((None, k, v), (R + 1, k, v), (65, k[:, :, :100].contiguous(), v[:, :, :100].contiguous())):
        for fn in (A.attn_decode, A.attn_decode_ref):
            with pytest.raises(ValueError):
                fn(q, kk, vv, n, c.B, c.H, c.D, c.Hkv, window, ring=True)
