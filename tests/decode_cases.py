"""Shared cases of the decode-attention tests (``test_kv_cache_cpu.py`` runs the math reference on them,
``test_attention_decode_gpu.py`` the kernel): inputs, the fp64 oracle and the staged model's error of each
case, computed once and never modified.

A decoded row at ``kv_len = n`` is the last query row of a causal prefill over n tokens whose key range is
[max(start, n - W), n).  So one case is ONE call of ``oracles.attention`` over B sequences of Smax tokens,
causal, with ``key_range[b] = (lo_b, n_b)``; sequence b's decoded row is row n_b - 1 of it.  The cache holds
the K / V of all Smax tokens of that prefill, the step's qkv the rows n_b - 1.
"""
import functools
import math
import types

import torch

from distributed_training_and_deepspeed_amd.ops import attention as A

from . import oracles as O

KT = A.DECODE_KEY_TILE
SMAX = 200                      # with KT = 64: four tiles, splits=4 gives 64 keys per split and 8 in the last
HEADS = ((4, 4, 64), (4, 2, 64), (8, 1, 64), (4, 1, 128))            # (H, Hkv, D)
LENS = ((1, KT + 1, 2 * KT, SMAX), (KT - 1, KT, 3 * KT + 1, SMAX - 1))
REGIMES = ("gauss", "spikes_up", "spikes_down")
SPLITS = (1, 2, 4, None)
PAD_STARTS = (0, 5, KT, KT + 3)   # under splits=4 the first split of the last two sequences is wholly empty
WINDOWS = (1, KT, KT + 7)

CAP_BF16, LSE_TOL = 2e-2, 1e-5            # the project's bf16 bounds (tests/test_attention_oracles_cpu.py)
REF_CTX_TOL, REF_LSE_TOL = 5e-3, 2.5e-6   # ... and a quarter of them: the math reference's

GUARD = 1024          # elements on either side of a guarded slice (a multiple of 16: 16-byte alignment, of codes too)
SENT, SENT_CODE = -12345.0, 0xA5          # the sentinel of a guarded buffer: floating point, uint8 codes


# ------------------------------------------------------------------------------------- guarded buffers (GPU tests)
def guarded(shape, dtype, fill=None, device="cuda"):
    """(buffer, slice of ``shape`` out of its middle); the buffer is the sentinel everywhere else."""
    n = math.prod(shape)
    sent = SENT_CODE if dtype == torch.uint8 else SENT
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device=device)
    view = buf[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf, n):
    sent = SENT_CODE if buf.dtype == torch.uint8 else SENT
    return bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + n:] == sent).all())


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def base_cases():
    return [(h, lens, None, 0, r) for h in HEADS for lens in LENS for r in REGIMES]


def pad_cases():
    """Left padding; a fifth sequence has kv_start == kv_len: no key at all."""
    return [(h, LENS[0] + (KT,), PAD_STARTS + (KT,), 0, r) for h in HEADS for r in ("gauss", "spikes_down")]


def window_cases():
    """W at kv_len = Smax, combined with a kv_start inside the window (sequences 2 and 3)."""
    return [(h, (SMAX,) * 4, (0, 10, SMAX - W + W // 2, SMAX - 1), W, r)
            for h in HEADS for W in WINDOWS for r in ("gauss", "spikes_up")]


def all_cases():
    return base_cases() + pad_cases() + window_cases()


def case_id(p):
    (H, Hkv, D), lens, starts, W, regime = p
    return f"h{H}kv{Hkv}d{D}-n{lens[0]}_{lens[-1]}-{'pad' if starts else 'nopad'}-w{W}-{regime}"


@functools.lru_cache(maxsize=None)
def decode_case(heads, lens, starts, W, regime):
    H, Hkv, D = heads
    B = len(lens)
    qkv, dctx = O.attn_inputs(regime, B, SMAX, H, D, Hkv, seed=300 + len(regime) + H + D)
    n = torch.tensor(lens, dtype=torch.int64)
    st = torch.tensor(starts if starts else (0,) * B, dtype=torch.int64)
    lo = torch.maximum(st, n - W) if W else st
    key_range = torch.stack([lo, n], 1).to(torch.int32)
    kw = dict(causal=True, key_range=key_range, kv_heads=Hkv)
    o = O.attention(qkv, dctx, B, SMAX, H, D, **kw)
    staged = O.attention_staged(qkv, dctx, B, SMAX, H, D, **kw)
    b = torch.arange(B)
    c = types.SimpleNamespace(heads=heads, H=H, Hkv=Hkv, D=D, B=B, W=W, regime=regime, lens=lens, starts=starts)
    c.ctx = o["ctx"][b, n - 1]                    # [B, H, D] fp64
    c.lse = o["lse"][b, :, n - 1]                 # [B, H]
    c.A = o["A"][b, :, n - 1]
    c.e_staged = float(O.slice_errors(staged["ctx"][b, n - 1], c.ctx).max())
    x = qkv.view(B, SMAX, H + 2 * Hkv, D)
    c.qkv = x[b, n - 1].reshape(B, (H + 2 * Hkv) * D).contiguous()              # the step's packed projection
    c.k = x[:, :, H:H + Hkv].transpose(1, 2).contiguous()                       # [B, Hkv, Smax, D]
    c.v = x[:, :, H + Hkv:].transpose(1, 2).contiguous()
    c.kv_len = n.to(torch.int32)
    c.kv_start = st.to(torch.int32) if starts else None
    c.lo, c.hi = lo, n
    return c


def check_decode(c, ctx, lse, ctx_tol, lse_tol, what=""):
    """Per (sequence, head): ctx against the row's largest element, |lse error| <= lse_tol (1 + A), -inf and
    ctx = 0 exactly on a row without a key.  Returns the worst (ctx, lse / (1 + A)) errors."""
    got = ctx.detach().cpu().reshape(c.B, c.H, c.D)
    e_ctx = O.assert_rows_close(got, c.ctx, ctx_tol, what=f"{what} ctx")
    dead = torch.isinf(c.lse)
    assert bool((got[dead] == 0).all()), f"{what}: ctx of a row without a key is not 0"
    e_lse = O.slice_errors(lse.detach().cpu().reshape(c.B, c.H), c.lse, axis=None, scale=1.0 + c.A)
    worst = float(e_lse.max())
    assert worst <= lse_tol, f"{what} lse: error {worst:.3e} (1 + A) > {lse_tol:.1e}"
    return e_ctx, worst
