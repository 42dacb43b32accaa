"""The CPU branches of ``ops/functional.py`` and ``adam_reference_`` against the fp64 oracles of
``tests/oracles.py``, per slice, for every op x input regime x dtype.

Three jobs: it validates the oracles against an implementation that shares none of their code; it
checks the CPU branches every other GPU test trusts as truth; and it shows that each regime is
achievable -- the fp32 CPU branch must sit at <= 1/4 of the tolerance the GPU kernels are held to
(``tests/test_kernel_numerics_gpu.py`` runs these same ``check_*`` functions on the device).  Under
``-s`` the last test prints the measured error of every op x regime x dtype next to its tolerance.

Tolerances are the project's own (test_kernels_gpu.py, test_llama_ops_gpu.py), applied per slice:
normalisations / softmax / SwiGLU / RoPE 2e-2 (bf16) and 1e-4 (fp32); cross-entropy loss and lse
1e-4, dlogits 2e-2; fp32 activations 2e-6 absolute; Adam p / m / v 1e-5, its bf16 copy 1e-2.

Regimes made milder than first written, because plain fp32 arithmetic cannot meet the tolerance on
them (so they would test the number format, not the kernel):
  * LayerNorm ``offset`` has no branch input (y = None, z = r, no dropout): with one, z = r + y is
    stored rounded, and at mean 50, std 1 the bf16 rounding of z (half an ulp, 0.125) is 9 % of the std -- the block
    kernel (h > 2048 or not a wave width), which re-reads its stored z where the wave kernels keep the
    fp32 sum in registers, then differs from LN of the unrounded z by 3.4e-2 of the row's largest
    element (measured, h = 2050), and every backward works from that stored z.  In fp32 it is mean 30,
    std 0.1, not mean 1000: an fp32 value near 1000 is known to half an ulp, 3e-5, which is 3e-4 of the
    std and about 1e-4 of the largest x-hat -- the whole tolerance before any arithmetic.  Measured on
    the fp32 CPU branch, error of ``out``: 7.7e-4 (mean 1000), 1.0e-4 (mean 100), 1.2e-5 (mean 30).
  * The softmax *backward* works from the stored output y, and for a nearly one-hot row dx_k = y_k
    (dy_k - sum y dy) cancels to the size of the rounding of y: the error grows as 1 / (1 - largest
    probability).  On ``large_logits`` it therefore runs on a tenth of the forward's logits (10 randn)
    and only on rows whose largest probability is at most 1/2 (or exactly 1: one-element rows).
    Measured on the CPU branch over the GPU file's widths and row counts, worst row of dx, bf16 / fp32:
    100 randn, every row 2.3e+1 / 3.2e+0; 10 randn, every row 3.3e+0 / 1.0e+0; 3 randn, every row
    7.2e-2 / 1.5e-5; 10 randn, largest probability <= 0.9: 9.6e-2 / 9.2e-6, <= 0.75: 1.7e-2 / 9.6e-7,
    <= 0.5: 5.0e-3 / 2.3e-7 (74 of 387 rows) -- the last is the one kept.
  * Cross-entropy ``large_logits`` labels avoid the row's largest logit: there dlogit = p - 1 with p
    within an fp32 ulp of 1, i.e. the rounding of the stored fp32 lse.
"""
import collections
import functools

import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.rng import RngState
from distributed_training_and_deepspeed_amd.optim.fused_adam import adam_reference_

from . import oracles as O

BF16, F32 = torch.bfloat16, torch.float32
SEED, STEP, SID = 7, 3, 5          # dropout seed / step / stream id of every case
LN_EPS, RMS_EPS = 1e-5, 1e-5
MODES = list(range(8))             # Adam mode bits: 1 AdamW, 2 bias correction, 4 HF eps placement

# (op, regime, dtype name) -> {quantity: (worst error, tolerance)}
TABLE = collections.defaultdict(dict)


def tol(dtype):
    return 2e-2 if dtype == BF16 else 1e-4


def dname(dtype):
    return "bf16" if dtype == BF16 else "fp32"


class Errs:
    """Records the worst per-slice error of each quantity, then asserts it against its tolerance."""

    def __init__(self, op, regime, dtype, dev="cpu"):
        # the table is of the CPU branches: a run on the device asserts but is not recorded
        self.row = TABLE[(op, regime, dname(dtype))] if str(dev) == "cpu" else {}
        self.tag = f"{op}/{regime}/{dname(dtype)}"

    def cmp(self, name, got, ref, t, **kw):
        e = O.slice_errors(got, ref, **kw).reshape(-1)
        val = float(e.max()) if e.numel() else 0.0
        self.row[name] = (max(val, self.row.get(name, (0.0, t))[0]), t)
        O.assert_rows_close(got, ref, t, what=f"{self.tag} {name}", **kw)
        return val


def ln_offset(rows, width, dtype, seed):
    """``offset`` as LayerNorm takes it in fp32: mean 30, std 0.1 (see the module docstring)."""
    if dtype == BF16:
        return O.offset(rows, width, dtype, seed)
    return 30.0 + 0.1 * O.gauss(rows, width, F32, seed)


def regime_fn(name):
    return getattr(O, name)


def make_rng(dev):
    rng = RngState(SEED, device=dev)
    rng.state[1] = STEP
    return rng


def _to(dev):
    return lambda t: None if t is None else t.to(dev)


def _vec(h, seed, dtype, mean, std):
    return (mean + std * O.gauss(1, h, F32, seed)[0]).to(dtype)


# ------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def ln_case(rows, h, dtype, p, regime):
    if regime == "offset":      # no branch input: z is r itself, exactly (see the module docstring)
        y, r, p = None, ln_offset(rows, h, dtype, 12), 0.0
    else:
        y, r = regime_fn(regime)(rows, h, dtype, 11), regime_fn(regime)(rows, h, dtype, 12)
    gamma, beta = _vec(h, 13, dtype, 1.0, 0.1), _vec(h, 14, dtype, 0.0, 0.1)
    dout, dout2, dext = (O.gauss(rows, h, dtype, s) for s in (15, 16, 17))
    keep = O.keep_mask(rows * h, p, SEED, STEP, SID) if p > 0 else None
    return y, r, p, gamma, beta, dout, dout2, dext, keep, O.layernorm_fwd(y, r, gamma, beta, LN_EPS, p, keep)


def check_layernorm(dev, rows, h, dtype, p, regime, bwd_setups=(None,)):
    """ln_fwd and ln_bwd (from the stored z) against the oracle.  ``bwd_setups``: callables run
    before each repeat of the backward (the GPU test flips the row-loop form between them)."""
    y, r, p, gamma, beta, dout, dout2, dext, keep, fw = ln_case(rows, h, dtype, p, regime)
    E, t, to, rng = Errs("layernorm", regime, dtype, dev), tol(dtype), _to(dev), make_rng(dev)
    z, out, mean, rstd = Fx.ln_fwd(to(y), to(r), to(gamma), to(beta), LN_EPS, p, rng, SID)
    assert (z is None) == (y is None)
    if z is None:
        z = to(r)
    else:
        E.cmp("z", z, fw["z"], t)
    E.cmp("out", out, fw["out"], t)
    E.cmp("mean", mean, fw["mean"], t, axis=None, scale=fw["z"].abs().amax(-1))
    E.cmp("rstd", rstd, fw["rstd"], t, axis=None)
    ob = O.layernorm_bwd(z, gamma, beta, LN_EPS, dout, dout2, dext, p, keep)
    for setup in bwd_setups:
        if setup is not None:
            setup()
        dg, db, dbias = (torch.zeros(h, dtype=F32, device=dev) for _ in range(3))
        dz, dy = Fx.ln_bwd(to(dout), to(dext), z, mean, rstd, to(gamma), p, rng, SID, want_dz=True, want_dy=True,
                           dgamma=dg, dbeta=db, dbias=dbias, dout2=to(dout2))
        E.cmp("dz", dz, ob["dz"], t)
        E.cmp("dy", dy, ob["dy"], t)
        for name, got in (("dgamma", dg), ("dbeta", db), ("dbias", dbias)):
            E.cmp(name, got, ob[name], t, axis=None, scale=ob["sc_" + name])


def check_layernorm_from_output(dev, rows, h, ratio, zero_cols=(), setups=(None,), dtype=BF16):
    """The memory-efficient backward (x-hat = (out - beta) / gamma from the stored output) against the
    true gradients, with |beta| = ratio * |gamma|.  The yardstick is the loss the rounded output has
    already suffered: the fp64 evaluation of the same formula on it (``inherent``).  Per slice the
    kernel must stay within 2 x inherent + the dtype's ordinary tolerance.  Columns with gamma == 0 get x-hat 0
    and dgamma exactly 0 (the contract documented in norm.hip) and are left out of the dgamma
    comparison.  Returns (worst kernel error, worst inherent error) of dz."""
    t, to, rng = tol(dtype), _to(dev), make_rng(dev)
    y, r = O.gauss(rows, h, dtype, 21), O.gauss(rows, h, dtype, 22)
    g32 = 1.0 + 0.1 * O.gauss(1, h, F32, 23)[0]
    sign = torch.where(O.gauss(1, h, F32, 24)[0] < 0, -1.0, 1.0)
    gamma, beta = g32.to(dtype), (ratio * g32 * sign).to(dtype)
    zc = torch.tensor(list(zero_cols), dtype=torch.long)
    gamma[zc] = 0.0
    dout, dout2 = O.gauss(rows, h, dtype, 25), O.gauss(rows, h, dtype, 26)
    p = 0.1
    keep = O.keep_mask(rows * h, p, SEED, STEP, SID)
    fw = O.layernorm_fwd(y, r, gamma, beta, LN_EPS, p, keep)
    true = O.layernorm_bwd(fw["z"], gamma, beta, LN_EPS, dout, dout2, None, p, keep)
    z, out, mean, rstd = Fx.ln_fwd(to(y), to(r), to(gamma), to(beta), LN_EPS, p, rng, SID, store_z=False)
    assert z is None
    inh = O.layernorm_from_output(out, gamma, beta, rstd, dout, dout2)
    live = torch.ones(h, dtype=torch.bool)
    live[zc] = False
    inh_dz = O.slice_errors(inh["dz"], true["dz"])
    inh_dg = O.slice_errors(inh["dgamma"], true["dgamma"], axis=None, scale=true["sc_dgamma"])[live]
    worst = 0.0
    for setup in setups:
        if setup is not None:
            setup()
        dg, db, dbias = (torch.zeros(h, dtype=F32, device=dev) for _ in range(3))
        dz, dy = Fx.ln_bwd(to(dout), None, None, mean, rstd, to(gamma), p, rng, SID, want_dz=True, want_dy=True,
                           dgamma=dg, dbeta=db, dbias=dbias, dout2=to(dout2), xout=out, beta=to(beta))
        e_dz = O.slice_errors(dz, true["dz"])
        e_dy = O.slice_errors(dy, true["dy"])
        e_dg = O.slice_errors(dg, true["dgamma"], axis=None, scale=true["sc_dgamma"])[live]
        worst = max(worst, float(e_dz.max()))
        for name, e, lim in (("dz", e_dz, inh_dz), ("dy", e_dy, inh_dz), ("dgamma", e_dg, inh_dg)):
            over = e - (2 * lim + t)
            i = int(over.argmax())
            assert float(over[i]) <= 0, (f"from-output {name} ratio {ratio}: slice {i} error {float(e[i]):.3e} > 2 x "
                                         f"inherent {float(lim[i]):.3e} + {t}")
        assert bool((dg.cpu()[zc] == 0).all()), "a gamma == 0 column must get no dgamma"
        O.assert_rows_close(db, true["dbeta"], t, axis=None, scale=true["sc_dbeta"], what="from-output dbeta")
    return worst, float(inh_dz.max())


# ------------------------------------------------------------------------------------------
# RMSNorm
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def rms_case(rows, h, dtype, extras, regime):
    rf = regime_fn(regime)
    y = rf(rows, h, dtype, 31) if extras else None
    r = rf(rows, h, dtype, 32)
    gamma = _vec(h, 33, dtype, 1.0, 0.1)
    dout = O.gauss(rows, h, dtype, 34)
    dout2, dext = ((O.gauss(rows, h, dtype, 35), O.gauss(rows, h, dtype, 36)) if extras else (None, None))
    return y, r, gamma, dout, dout2, dext, O.rmsnorm_fwd(y, r, gamma, RMS_EPS)


def check_rmsnorm(dev, rows, h, dtype, extras, regime):
    y, r, gamma, dout, dout2, dext, fw = rms_case(rows, h, dtype, extras, regime)
    E, t, to = Errs("rmsnorm", regime, dtype, dev), tol(dtype), _to(dev)
    z, out, rstd = Fx.rms_fwd(to(y), to(r), to(gamma), RMS_EPS)
    assert (z is not None) == extras
    if extras:
        E.cmp("z", z, fw["z"], t)
    E.cmp("out", out, fw["out"], t)
    E.cmp("rstd", rstd, fw["rstd"], t, axis=None)
    if regime == "constant":     # the all-zero last row: rstd = eps^-1/2, to fp32 rounding
        assert abs(rstd[-1].item() * RMS_EPS ** 0.5 - 1.0) <= 1e-6
    zin = z if extras else to(r)
    ob = O.rmsnorm_bwd(zin, gamma, RMS_EPS, dout, dout2, dext)
    dg = torch.zeros(h, dtype=F32, device=dev)
    dz = Fx.rms_bwd(to(dout), to(dext), zin, rstd, to(gamma), dgamma=dg, dout2=to(dout2))
    E.cmp("dz", dz, ob["dz"], t)
    E.cmp("dgamma", dg, ob["dgamma"], t, axis=None, scale=ob["sc_dgamma"])
    # dgamma: fixed-order partial sums, bitwise equal from run to run; accumulate adds to the destination
    dg2 = torch.zeros(h, dtype=F32, device=dev)
    Fx.rms_bwd(to(dout), to(dext), zin, rstd, to(gamma), dgamma=dg2, dout2=to(dout2))
    assert torch.equal(dg, dg2)
    Fx.rms_bwd(to(dout), to(dext), zin, rstd, to(gamma), dgamma=(dg2, True), dout2=to(dout2))
    O.assert_rows_close(dg2, 2 * dg.double(), 1e-6, axis=None, scale=2 * dg.double().abs().max().expand(h),
                        what="rmsnorm dgamma accumulate")


# ------------------------------------------------------------------------------------------
# row softmax
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def softmax_case(rows, n, dtype, regime):
    """(x, dy, oracle of x, x of the backward, oracle of that, rows the backward is checked on)."""
    x, dy = regime_fn(regime)(rows, n, dtype, 41), O.gauss(rows, n, dtype, 42)
    ref = O.softmax(x, dy)
    if regime != "large_logits":
        return x, dy, ref, x, ref, torch.ones(rows, dtype=torch.bool)
    xb = (0.1 * x.float()).to(dtype)          # see the module docstring
    refb = O.softmax(xb, dy)
    pmax = refb["y"].amax(-1)
    return x, dy, ref, xb, refb, (pmax <= 0.5) | (pmax == 1.0)


def check_softmax(dev, rows, n, dtype, regime):
    x, dy, ref, xb, refb, rows_b = softmax_case(rows, n, dtype, regime)
    E, t = Errs("softmax", regime, dtype, dev), tol(dtype)
    y = Fx.softmax_fwd(x.to(dev))
    E.cmp("y", y, ref["y"], t)
    assert bool((y.cpu()[torch.isinf(x)] == 0).all()), "masked positions must be exactly 0"
    if xb is not x:
        y = Fx.softmax_fwd(xb.to(dev))
        E.cmp("y", y, refb["y"], t)
    dx = Fx.softmax_bwd(y, dy.to(dev))
    if bool(rows_b.any()):
        E.cmp("dx", dx.cpu()[rows_b], refb["dx"][rows_b], t)
    return int(rows_b.sum())


# ------------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------------
GOUT = 0.7


@functools.lru_cache(maxsize=8)
def xent_case(rows, V, dtype, regime):
    z = regime_fn(regime)(rows, V, dtype, 51)
    zl = z.float()
    if regime == "large_logits" and V > 1:     # see the module docstring
        zl = zl.masked_fill(zl == zl.amax(-1, keepdim=True), float("-inf"))
    lab = O.labels_on_finite(zl, 52)
    fin = torch.where(torch.isfinite(z.float()), z.float().abs(), torch.zeros(()))
    return z, lab, fin.amax(-1).double(), O.cross_entropy(z, lab, GOUT), O.cross_entropy(z, lab, 1.0)


def _at_offset(t, off, dev):
    """A device copy of ``t`` whose base is ``off`` elements past an allocation boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    return buf[off:].view(t.shape).copy_(t)


def check_xent(dev, rows, V, dtype, base_offset, regime):
    """xent_fwd, xent_bwd and xent_bwd(dbias=...).  lse is one number per row whose natural scale is
    the row's logits (shifting every logit by c shifts lse by c, so its own zero crossing means
    nothing): its error is taken against max(|lse|, max |finite logit|) of the row."""
    z, lab, zmax, ref, _ = xent_case(rows, V, dtype, regime)
    E = Errs("xent", regime, dtype, dev)
    zd, ld = _at_offset(z, base_offset, dev), lab.to(dev)
    valid = lab != -100
    assert bool(valid.any())
    if regime == "masked" and V >= 64:
        # a labelled row starts with -inf through its scalar head and a whole 16-byte vector at any base
        # offset: the kernel's vector body meets a chunk of nothing but -inf before anything finite
        assert bool(torch.isinf(z.float()[valid][:, :16]).all(-1).any())
    loss, lse, st = Fx.xent_fwd(zd, ld)
    E.cmp("loss", loss, ref["loss"], 1e-4, scale=torch.maximum(ref["loss"].abs(), zmax[valid].max()))
    E.cmp("lse", lse.cpu()[valid], ref["lse"][valid], 1e-4, axis=None,
          scale=torch.maximum(ref["lse"].abs(), zmax)[valid])
    assert st[1].item() == int(valid.sum()) and st[0].item() == loss.item()
    gout = torch.tensor(GOUT, device=dev)
    d = Fx.xent_bwd(zd, ld, lse, st, gout)
    E.cmp("dlogits", d, ref["dlogits"], 2e-2)
    colsum, colscale = O.column_sums(d)
    for acc in (False, True):
        db = torch.full((V,), 0.25, device=dev)
        d2 = Fx.xent_bwd(zd, ld, lse, st, gout, dbias=(db, acc))
        assert torch.equal(d2, d)
        E.cmp("dbias", db.double().cpu() - (0.25 if acc else 0.0), colsum, 1e-4, axis=None,
              scale=colscale + (0.25 if acc else 0.0))


# ------------------------------------------------------------------------------------------
# activations, SwiGLU, RoPE, dropout-add
# ------------------------------------------------------------------------------------------
def check_activation(dev, n, dtype, act, regime):
    """act_fwd, act_bwd and the backward's fused recompute.  fp32: 2e-6 absolute with dy = 1 (the
    bound of test_activation_fast_math_accuracy_fp32).  bf16: 2e-2 of the row, and -- because one
    saturated 1e30 would hide everything else in its row -- 2e-2 of |ref| + |dy| element by element
    (the outputs are rounded once, 2^-8 relative, from an fp32 value good to 2e-6 absolute)."""
    u = regime_fn(regime)(1, n, dtype, 61)[0]
    dy = torch.ones(n, dtype=dtype) if dtype == F32 else O.gauss(1, n, dtype, 62)[0]
    ref = O.activation(u, act, dy)
    E = Errs(act, regime, dtype, dev)
    a = Fx.act_fwd(u.to(dev), act)
    db = torch.zeros(n, dtype=F32, device=dev)
    du = Fx.act_bwd(dy.to(dev), u.to(dev), act, dbias=db)
    db2 = torch.zeros(n, dtype=F32, device=dev)
    du2, a2 = Fx.act_bwd(dy.to(dev), u.to(dev), act, dbias=db2, want_act=True)
    assert torch.equal(a, a2)                       # the backward's recompute is bitwise the forward
    if dtype == BF16:
        assert torch.equal(du, du2)                 # as test_activation_fwd_bwd asserts
    else:     # fp32 GELU-tanh: the two forms contract their multiply-adds differently (last bits of du)
        O.assert_rows_close(du2, ref["du"], 2e-6, absolute=True, what=f"{act} du with recompute")
    if dtype == F32:
        E.cmp("a", a, ref["a"], 2e-6, absolute=True)
        E.cmp("du", du, ref["du"], 2e-6, absolute=True)
        E.cmp("dbias", db, ref["dbias"], 2e-6, absolute=True)
        E.cmp("dbias", db2, ref["dbias"], 2e-6, absolute=True)
    else:
        E.cmp("a", a, ref["a"], 2e-2)
        E.cmp("du", du, ref["du"], 2e-2)
        E.cmp("a/elem", a, ref["a"], 2e-2, axis=None, scale=ref["a"].abs() + 1.0)
        E.cmp("du/elem", du, ref["du"], 2e-2, axis=None, scale=ref["du"].abs() + O.f64(dy).abs())
        for got in (db, db2):
            E.cmp("dbias", got, ref["dbias"], 2e-2, axis=None, scale=ref["sc_dbias"] + O.f64(dy).abs())


def check_swiglu(dev, rows, f, dtype, regime):
    """The gate takes the regime, up and the upstream gradient are ordinary.  Recompute and forward
    bitwise equal, as test_swiglu_fwd_bwd asserts."""
    gate = regime_fn(regime)(rows, f, dtype, 71)
    gu = torch.cat([gate, O.gauss(rows, f, dtype, 72)], -1)
    da = O.gauss(rows, f, dtype, 73)
    ref = O.swiglu(gu, da)
    E, t = Errs("swiglu", regime, dtype, dev), tol(dtype)
    a = Fx.swiglu_fwd(gu.to(dev))
    dgu, a2 = Fx.swiglu_bwd(da.to(dev), gu.to(dev), want_act=True)
    assert torch.equal(a2, a) and torch.equal(Fx.swiglu_bwd(da.to(dev), gu.to(dev)), dgu)
    E.cmp("a", a, ref["a"], t)
    E.cmp("dgu", dgu, ref["dgu"], t)
    # element by element too: a saturated 1e30 gate must not hide its row
    E.cmp("a/elem", a, ref["a"], t, axis=None, scale=ref["a"].abs() + 1.0)
    E.cmp("dgu/elem", dgu, ref["dgu"], t, axis=None, scale=ref["dgu"].abs() + 1.0)


def check_rope(dev, D, S, dtype, pos_mode):
    """Forward and inverse rotation against the oracle built from the same fp32 table; v untouched."""
    B, H, P = 2, 3, 256
    table = Fx.rope_table(P, D, 10000.0)
    g = torch.Generator().manual_seed(81)
    pos = None
    if pos_mode == "random":
        pos = torch.randint(0, P, (B, S), generator=g, dtype=torch.int32)
    elif pos_mode == "clamped":
        pos = torch.randint(0, 2 * P, (B, S), generator=g, dtype=torch.int32)
        pos[0, 0], pos[-1, -1] = P, 2**30
    x = O.gauss(B * S, 3 * H * D, dtype, 82)
    E, t = Errs("rope", pos_mode, dtype, dev), tol(dtype)
    for inverse in (False, True):
        got = Fx.rope_(x.clone().to(dev), table.to(dev), B, S, H, D, pos=None if pos is None else pos.to(dev),
                       inverse=inverse)
        E.cmp("inverse" if inverse else "forward", got, O.rope(x, table, B, S, H, D, pos, inverse), t)
        assert torch.equal(got.cpu()[:, 2 * H * D:], x[:, 2 * H * D:])


def check_dropout_add(dev, n, dtype, p):
    """res + keep * x / (1 - p): the bounds of test_dropout_add_fused_residual, 1e-2 (bf16) and 1e-6
    (fp32), but element by element against |res| + |x| / (1 - p).  (The fp32 scale, the product and
    the sum round once each, 3 x 2^-24, and a bf16 result once more, 2^-8 -- twice, 2^-7, where the
    dropout is rounded before the add as in the CPU branch.)"""
    x, res = O.gauss(1, n, dtype, 91)[0], O.gauss(1, n, dtype, 92)[0]
    keep = O.keep_mask(n, p, SEED, STEP, SID) if p > 0 else None
    ref = O.dropout_add(x, res, p, keep)
    got = Fx.dropout_add(x.to(dev), res.to(dev), p, make_rng(dev), SID)
    Errs("dropout_add", f"p={p}", dtype, dev).cmp("out", got, ref, 1e-2 if dtype == BF16 else 1e-6, axis=None,
                                            scale=O.f64(res).abs() + O.f64(x).abs() / (1.0 - p))
    if keep is not None and dtype == F32:
        assert torch.equal(got.cpu()[~keep], res[~keep])     # a dropped element leaves the residual untouched


# ------------------------------------------------------------------------------------------
# Adam, sq-norm, scale-cast
# ------------------------------------------------------------------------------------------
PAD, SENTINEL = 64, 7.25


def adam_case(n, gdt, step, wd, seed=101):
    """(p, m, v, g, hp): moments zero at step 1 (the real first step); every fifth gradient is 0, and
    at a later step every tenth element has g = m = v = 0 as well (0 / eps must be 0)."""
    p = O.gauss(1, n, F32, seed)[0]
    m = 0.1 * O.gauss(1, n, F32, seed + 1)[0]
    v = 0.01 * O.gauss(1, n, F32, seed + 2)[0].abs()
    g = O.gauss(1, n, F32, seed + 3)[0]
    g[::5] = 0.0
    if step == 1:
        m.zero_()
        v.zero_()
    else:
        m[::10] = 0.0
        v[::10] = 0.0
    hp = torch.tensor([1e-3, 0.9, 0.999, 1e-6, wd, float(step), 0.5, 0.0], dtype=F32)
    return p, m, v, g.to(gdt), hp


def padded(t, dev):
    """``t`` on ``dev`` with PAD sentinel elements on each side: (whole buffer, view of t)."""
    buf = torch.full((t.numel() + 2 * PAD,), SENTINEL, dtype=t.dtype, device=dev)
    buf[PAD:PAD + t.numel()] = t.to(dev)
    return buf, buf[PAD:PAD + t.numel()]


def check_adam(run, dev, n, mode, gdt, with_lowp, step, wd):
    """``run(p, m, v, g, lowp, n, hp, mode)`` updates the views in place.  p / m / v and the bf16 copy
    against the oracle, and the sentinels around every buffer bitwise untouched."""
    p, m, v, g, hp = adam_case(n, gdt, step, wd)
    rp, rm, rv = O.adam(p, m, v, g, hp, mode)
    bufs = [padded(t, dev) for t in (p, m, v, g)]
    lowp = padded(torch.zeros(n, dtype=BF16), dev) if with_lowp else (None, None)
    run(bufs[0][1], bufs[1][1], bufs[2][1], bufs[3][1], lowp[1], n, hp, mode)
    E = Errs("adam", f"step={step},wd={wd}", gdt, dev)
    for name, (buf, view), ref in (("p", bufs[0], rp), ("m", bufs[1], rm), ("v", bufs[2], rv)):
        E.cmp(name, view, ref, 1e-5)
    # On a flat buffer the metric above is the global one, and 1e-5 of max |p| is 4 % of an update of
    # size lr.  So also the update p_new - p_old, element by element: 1e-5 of the update itself plus the
    # roundings of p.  The new p is rounded to fp32 up to three times at magnitude |p| (the decay, its
    # fp32 factor, the step): 3 x 2^-24 |p|, and four times that, 2^-20 |p|, is allowed -- a tenth of
    # the smallest term that tells two modes apart here (lr * wd * |p| = 1e-5 |p|).
    upd = rp - O.f64(p)
    E.cmp("update", O.f64(bufs[0][1]) - O.f64(p), upd, 1e-5, axis=None,
          scale=upd.abs() + (2.0 ** -20 / 1e-5) * O.f64(p).abs())
    if with_lowp:
        E.cmp("lowp", lowp[1], rp, 1e-2)
    for buf, _ in bufs + ([lowp] if with_lowp else []):
        edge = torch.cat([buf[:PAD], buf[-PAD:]]).cpu()
        assert torch.equal(edge, torch.full_like(edge, SENTINEL)), "a sentinel next to the buffer changed"
    assert torch.equal(bufs[3][1].cpu(), g)     # the gradient is read only
    return [b[1] for b in bufs[:3]] + [lowp[1]]


def run_adam_reference(p, m, v, g, lowp, n, hp, mode):
    lr, b1, b2, eps, wd, step, gs = (float(t) for t in hp.double()[:7])     # the fp32 values the kernel reads
    adam_reference_(p, m, v, g, lr, b1, b2, eps, wd, int(step), mode, grad_scale=gs)
    if lowp is not None:
        lowp.copy_(p)


def check_sqnorm_scale_cast(dev, n, sdt, ddt, with_dscale):
    """sq_norm: 1e-4 (test_sqnorm_and_scale_cast).  scale_cast_: 1e-6 of each element into fp32 (the
    same test: the fp32 scale product and the multiply round once each, 2^-23), and one more bf16
    rounding, 2^-8 < 1e-2 (the bound of Adam's bf16 copy), into bf16."""
    x = O.row_scales(13, (n + 12) // 13, sdt, 111).t().reshape(-1)[:n].clone()     # neighbours 2^-6 .. 2^6 apart
    Errs("sq_norm", "row_scales", sdt, dev).cmp("sq_norm", Fx.sq_norm(x.to(dev)), O.sq_norm(x), 1e-4)
    E = Errs("scale_cast", f"from {dname(sdt)}", ddt, dev)     # listed under the dtype it writes
    dscale = torch.tensor([1.7], dtype=F32) if with_dscale else None
    dst = torch.full((n + 2 * PAD,), SENTINEL, dtype=ddt, device=dev)
    Fx.scale_cast_(x.to(dev), dst[PAD:PAD + n], 0.3, None if dscale is None else dscale.to(dev))
    E.cmp("scale_cast", dst[PAD:PAD + n], O.scale_cast(x, 0.3, dscale), 1e-6 if ddt == F32 else 1e-2, axis=None)
    edge = torch.cat([dst[:PAD], dst[-PAD:]]).cpu()
    assert torch.equal(edge, torch.full_like(edge, SENTINEL))


# ------------------------------------------------------------------------------------------
# the CPU branches: every op x regime x dtype
# ------------------------------------------------------------------------------------------
DTYPES = [BF16, F32]
ids = dict(ids=lambda v: dname(v) if isinstance(v, torch.dtype) else str(v))
LN_REGIMES = ["gauss", "row_scales", "offset", "constant", "spike"]
RMS_REGIMES = ["gauss", "row_scales", "constant", "tiny", "huge", "spike"]
LOGIT_REGIMES = ["gauss", "large_logits", "masked"]
ACTS = ["gelu", "gelu_tanh", "relu"]
ACT_REGIMES = ["gauss", "saturated"]
ROPE_POS = ["arange", "random", "clamped"]
ADAM_STEPS = [(1, 0.0), (1, 0.01), (100000, 0.0), (100000, 0.01)]


def ln_probs(regime):
    return (0.0,) if regime == "offset" else (0.0, 0.1)      # offset has no branch input, so no dropout


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("regime", LN_REGIMES)
def test_layernorm_cpu_branch(regime, dtype):
    for rows, h in ((1, 128), (5, 2050), (37, 768)):
        for p in ln_probs(regime):
            check_layernorm("cpu", rows, h, dtype, p, regime)


@pytest.mark.parametrize("ratio", [0.1, 1, 10, 100])
def test_layernorm_from_output_cpu_branch(ratio):
    k, i = check_layernorm_from_output("cpu", 37, 768, ratio)
    print(f"\nfrom-output LayerNorm, CPU branch, |beta|/|gamma| = {ratio}: dz error {k:.3e}, inherent {i:.3e}")


def test_layernorm_from_output_zero_gamma_cpu_branch():
    check_layernorm_from_output("cpu", 37, 768, 1, zero_cols=(0, 5, 767))
    check_layernorm_from_output("cpu", 5, 2050, 1, zero_cols=(0, 5, 2049), dtype=F32)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("regime", RMS_REGIMES)
def test_rmsnorm_cpu_branch(regime, dtype):
    if regime in ("tiny", "huge") and dtype == BF16:
        return     # fp32 only
    for rows, h in ((1, 8), (5, 1032), (37, 8192)):
        for extras in (True, False):
            check_rmsnorm("cpu", rows, h, dtype, extras, regime)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("regime", LOGIT_REGIMES)
def test_softmax_cpu_branch(regime, dtype):
    checked = sum(check_softmax("cpu", rows, n, dtype, regime) for rows, n in ((1, 1), (5, 7), (37, 300), (37, 2056)))
    assert checked >= 5      # rows the backward was held to


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("regime", LOGIT_REGIMES)
def test_xent_cpu_branch(regime, dtype):
    for rows, V in ((1, 1), (4, 7), (33, 13), (33, 1004), (4, 4099)):
        check_xent("cpu", rows, V, dtype, 1, regime)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("regime", ACT_REGIMES)
@pytest.mark.parametrize("act", ACTS)
def test_activation_cpu_branch(act, regime, dtype):
    for n in (1, 7, 2047, 2048 * 3 + 5):
        check_activation("cpu", n, dtype, act, regime)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("regime", ACT_REGIMES)
def test_swiglu_cpu_branch(regime, dtype):
    for rows, f in ((1, 8), (5, 392)):
        check_swiglu("cpu", rows, f, dtype, regime)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("pos_mode", ROPE_POS)
def test_rope_cpu_branch(pos_mode, dtype):
    for D, S in ((64, 1), (128, 130)):
        check_rope("cpu", D, S, dtype, pos_mode)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dropout_add_cpu_branch(p, dtype):
    for n in (1, 7, 8, 100003):
        check_dropout_add("cpu", n, dtype, p)


@pytest.mark.parametrize("gdt", DTYPES, **ids)
@pytest.mark.parametrize("step,wd", ADAM_STEPS)
def test_adam_reference(step, wd, gdt):
    for mode in MODES:
        for n in (1, 9, 4099):
            check_adam(run_adam_reference, "cpu", n, mode, gdt, True, step, wd)


@pytest.mark.parametrize("sdt", DTYPES, **ids)
@pytest.mark.parametrize("ddt", DTYPES, **ids)
def test_sqnorm_scale_cast_cpu_branch(sdt, ddt):
    for n in (1, 7, 2049, 123457):
        for with_dscale in (False, True):
            check_sqnorm_scale_cast("cpu", n, sdt, ddt, with_dscale)


def test_every_fp32_regime_is_achievable():
    """The table (``-s`` shows it), and the rule that keeps a regime: the fp32 CPU branch's worst
    per-slice error is at most a quarter of the tolerance.  Measures everything itself, so it does not
    depend on which other tests ran, or in what order."""
    TABLE.clear()
    for dt in DTYPES:
        for regime in LN_REGIMES:
            test_layernorm_cpu_branch(regime, dt)
        for regime in RMS_REGIMES:
            test_rmsnorm_cpu_branch(regime, dt)
        for regime in LOGIT_REGIMES:
            test_softmax_cpu_branch(regime, dt)
            test_xent_cpu_branch(regime, dt)
        for regime in ACT_REGIMES:
            test_swiglu_cpu_branch(regime, dt)
            for act in ACTS:
                test_activation_cpu_branch(act, regime, dt)
        for pos_mode in ROPE_POS:
            test_rope_cpu_branch(pos_mode, dt)
        for p in (0.0, 0.1):
            test_dropout_add_cpu_branch(p, dt)
        for step, wd in ADAM_STEPS:
            test_adam_reference(step, wd, dt)
        for ddt in DTYPES:
            test_sqnorm_scale_cast_cpu_branch(dt, ddt)
    lines, over = [], []
    for (op, regime, dt), row in sorted(TABLE.items()):
        if not row:
            continue
        name, (err, t) = max(row.items(), key=lambda kv: kv[1][0] / kv[1][1])
        lines.append(f"{op:18s} {regime:22s} {dt:5s} {name:10s} err {err:9.3e}  tol {t:7.1e}  ratio {err / t:6.3f}")
        if dt == "fp32" and err > t / 4:
            over.append(lines[-1])
    print("\nop                 regime                 dtype worst      CPU-branch error vs tolerance")
    print("\n".join(lines))
    assert not over, "fp32 CPU branch above 1/4 of the tolerance:\n" + "\n".join(over)
