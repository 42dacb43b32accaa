"""Float64 oracles, a per-slice error metric and named input regimes for the streaming kernels
(LayerNorm, RMSNorm, row softmax, cross-entropy, activations, SwiGLU, RoPE, dropout-add, fused Adam,
sq-norm, scale-cast).

A plain helper module: no fixtures, and nothing from the package but ``ops.rng.keep_mask`` (the
dropout keep bits are an input of the oracles, not something they re-derive).  Every oracle takes
the kernel's inputs in their storage dtype, upcasts them to fp64 (exact for bf16 and fp32), builds
the forward from torch operators and takes every gradient with ``torch.autograd.grad`` -- no
hand-derived backward formulas, so a formula error in a kernel and in the CPU branch of
``ops/functional.py`` cannot hide in the oracle too.  The one exception is ``layernorm_from_output``,
which *is* a formula by definition: the yardstick for the memory-efficient LayerNorm backward is the
fp64 evaluation of that form on the rounded output it is given.

Column sums (dgamma, dbeta, dbias) come with a per-column scale: the sum over rows of the size of
the column's summands.  Where a summand holds a computed row quantity (x-hat in dgamma, dy in dbias),
its size is taken with that quantity's row maximum, because the row metric itself only holds x-hat and
dy to the tolerance times their row's largest element (an x-hat near zero is the difference of z and
the mean and carries the rounding of both); dbeta sums stored inputs, so its scale is sum |d|.
"""
import math

import torch
import torch.nn.functional as F

from distributed_training_and_deepspeed_amd.ops.rng import keep_mask  # noqa: F401  (re-exported for the tests)

TINY = 1e-30
BF16, F32 = torch.bfloat16, torch.float32


def f64(t):
    """Exact upcast of a stored tensor (None passes through)."""
    return None if t is None else t.detach().to("cpu", torch.float64)


def _leaf(t):
    return f64(t).clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------
# metric
# ------------------------------------------------------------------------------------------
def slice_errors(got, ref64, axis=-1, scale=None, absolute=False):
    """Per-slice error max_j |got - ref| / (max_j |ref| + tiny), j running over ``axis`` (None:
    every element is its own slice -- column sums, with ``scale`` the column's own scale).  Also
    asserts that got is finite wherever ref is and equal to ref where ref is not finite."""
    g, r = f64(got), f64(ref64)
    assert g.shape == r.shape, f"shape {tuple(g.shape)} vs reference {tuple(r.shape)}"
    fin = torch.isfinite(r)
    bad = fin & ~torch.isfinite(g)
    assert not bool(bad.any()), f"non-finite result at {bad.nonzero()[0].tolist()} where the reference is finite"
    if not bool(fin.all()):
        same = torch.where(torch.isnan(r), torch.isnan(g), g == r)
        assert bool(same[~fin].all()), "result differs from a non-finite reference value"
    err = torch.where(fin, (g - r).abs(), torch.zeros_like(r))
    mag = torch.where(fin, r.abs(), torch.zeros_like(r))
    if g.dim() == 0 or axis is None:
        den = mag if scale is None else f64(scale)
    else:
        err = err.amax(axis)
        den = mag.amax(axis) if scale is None else f64(scale)
    return err if absolute else err / (den + TINY)


def assert_rows_close(got, ref64, tol, axis=-1, scale=None, absolute=False, what=""):
    """Every slice's error <= tol; the message names the worst slice.  Returns the worst error."""
    e = slice_errors(got, ref64, axis, scale, absolute).reshape(-1)
    if e.numel() == 0:
        return 0.0
    worst = int(e.argmax())
    val = float(e[worst])
    assert val <= tol, f"{what}: slice {worst} of {e.numel()} has error {val:.3e} > tol {tol:.1e}"
    return val


# ------------------------------------------------------------------------------------------
# input regimes: f(rows, width, dtype, seed) -> [rows, width] CPU tensor of dtype
# ------------------------------------------------------------------------------------------
def _randn(rows, width, seed):
    return torch.randn(rows, width, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def gauss(rows, width, dtype, seed):
    return _randn(rows, width, seed).to(dtype)


def row_scales(rows, width, dtype, seed):
    """Row i times 2^((i mod 13) - 6): small rows next to large ones."""
    e = (torch.arange(rows) % 13 - 6).float()
    return (_randn(rows, width, seed) * torch.exp2(e)[:, None]).to(dtype)


def offset(rows, width, dtype, seed):
    """mean >> std.  bf16: mean 50, std 1, so the rounded data (ulp 0.25 at 50) still varies."""
    x = _randn(rows, width, seed)
    return (50.0 + x).to(dtype) if dtype == BF16 else (1000.0 + 0.1 * x).to(dtype)


def constant(rows, width, dtype, seed):
    """Every fourth row all equal (variance 0: rstd = eps^-1/2) and the last row all zero."""
    x = _randn(rows, width, seed)
    for i in range(0, rows, 4):
        x[i] = 0.5 * (i % 7 + 1)
    x[rows - 1] = 0.0
    return x.to(dtype)


def spike(rows, width, dtype, seed):
    """Even rows: zero but for one element at 1e4."""
    x = _randn(rows, width, seed)
    for i in range(0, rows, 2):
        x[i] = 0.0
        x[i, (7 * i + 3) % width] = 1e4
    return x.to(dtype)


def tiny(rows, width, dtype, seed):
    assert dtype == F32
    return _randn(rows, width, seed) * 1e-20     # squares underflow in fp32


def huge(rows, width, dtype, seed):
    assert dtype == F32
    return _randn(rows, width, seed) * 1e15      # squares ~1e30: 8192 of them stay below fp32 overflow


SATURATING = (20.0, -20.0, 90.0, -90.0, 200.0, -200.0, 1e30)


def saturated(rows, width, dtype, seed, values=SATURATING):
    """Every fifth element takes the next of ``values`` (saturated sigmoid / erf / tanh); the rest
    are ordinary."""
    x = _randn(rows, width, seed).reshape(-1)
    idx = torch.arange(0, x.numel(), 5)
    x[idx] = torch.tensor(values, dtype=torch.float32)[(idx // 5) % len(values)]
    return x.view(rows, width).to(dtype)


def large_logits(rows, width, dtype, seed):
    return (100.0 * _randn(rows, width, seed)).to(dtype)


def masked(rows, width, dtype, seed):
    """-inf logits: a -inf prefix (length not a multiple of 8), a -inf suffix, or every third column
    -inf.  The kind of row i is (i + i // 3) mod 3, so that with every third row unlabelled
    (``labels_on_finite``) each kind keeps labelled rows.  Every row keeps a finite logit.
    Unit-scale logits: a narrow row of wider ones is nearly one-hot, where the softmax backward cancels
    (see test_oracles_cpu.py on large_logits)."""
    x = _randn(rows, width, seed)
    n = int(0.3 * width)
    if n % 8 == 0 and n + 1 < width:
        n += 1
    for i in range(rows):
        kept = x[i, 0].clone()
        kind = (i + i // 3) % 3
        if kind == 0:
            x[i, :n] = -math.inf
        elif kind == 1:
            x[i, width - n:] = -math.inf
        else:
            x[i, ::3] = -math.inf
        if width < 3:
            x[i, 0] = kept          # too narrow to mask and keep a finite logit
    return x.to(dtype)


def labels_on_finite(z, seed, ignore_every=3, ignore_index=-100):
    """One label per row pointing at a finite logit; rows 2, 5, 8, ... (every ``ignore_every``-th)
    ignored, so row 0 -- the only row of a one-row case -- is labelled."""
    g = torch.Generator().manual_seed(seed)
    score = torch.rand(z.shape, generator=g).masked_fill(~torch.isfinite(z.float()), -1.0)
    lab = score.argmax(-1)
    lab[ignore_every - 1::ignore_every] = ignore_index
    return lab


# ------------------------------------------------------------------------------------------
# normalisations
# ------------------------------------------------------------------------------------------
def _branch(y, r, p, keep):
    """(z, y-leaf): z = r + keep * y / (1 - p) in fp64."""
    yl = _leaf(y) if y is not None else None
    z = None
    if yl is not None:
        z = yl * f64(keep).view_as(yl) / (1.0 - p) if (p > 0 and keep is not None) else yl * 1.0
    if r is not None:
        z = f64(r) if z is None else z + f64(r)
    return z, yl


def _col_scale(d, rowq):
    """Scale of the column sums of d * rowq: sum_i |d_ij| * max_j |rowq_ij|."""
    return (d.abs() * rowq.abs().amax(-1, keepdim=True)).sum(0)


def layernorm_fwd(y, r, gamma, beta, eps, p=0.0, keep=None):
    """z = r + keep * y / (1 - p); out = F.layer_norm(z).  Returns dict z, out, mean, rstd."""
    z, _ = _branch(y, r, p, keep)
    z = z.detach()
    h = z.shape[-1]
    out = F.layer_norm(z, (h,), f64(gamma), f64(beta), eps)
    return dict(z=z, out=out, mean=z.mean(-1), rstd=torch.rsqrt(z.var(-1, unbiased=False) + eps))


def layernorm_bwd(z, gamma, beta, eps, dout, dout2=None, dz_extra=None, p=0.0, keep=None):
    """Gradients of sum(LN(z) * (dout + dout2)) + sum(z * dz_extra) with z = z_stored + keep * y /
    (1 - p) at y = 0: dz, dy (the branch gradient), dgamma, dbeta, dbias (column sums of dy), and the
    column scales sc_dgamma / sc_dbeta / sc_dbias."""
    zl, gl, bl = _leaf(z), _leaf(gamma), _leaf(beta)
    y0 = torch.zeros_like(zl, requires_grad=True)
    k = f64(keep).view_as(zl) / (1.0 - p) if (p > 0 and keep is not None) else torch.ones_like(zl)
    zt = zl + y0 * k
    h = zl.shape[-1]
    d = f64(dout) + (f64(dout2) if dout2 is not None else 0.0)
    loss = (F.layer_norm(zt, (h,), gl, bl, eps) * d).sum()
    if dz_extra is not None:
        loss = loss + (zt * f64(dz_extra)).sum()
    dz, dy, dg, db = torch.autograd.grad(loss, (zl, y0, gl, bl))
    xh = F.layer_norm(zl.detach(), (h,), None, None, eps)
    return dict(dz=dz, dy=dy, dgamma=dg, dbeta=db, dbias=dy.sum(0), sc_dgamma=_col_scale(d, xh),
                sc_dbeta=d.abs().sum(0), sc_dbias=_col_scale(torch.ones_like(dy), dy))


def layernorm_from_output(xout, gamma, beta, rstd, dout, dout2=None, dz_extra=None):
    """The memory-efficient backward's own formula in fp64 on the stored (rounded) output: x-hat =
    (xout - beta) / gamma with |gamma| clamped at 1e-12, dz = rstd * (g - mean g - x-hat mean(g
    x-hat)).  Not an independent oracle: it measures what the rounded output has already lost."""
    g64 = f64(gamma)
    gs = torch.where(g64.abs() < 1e-12, torch.full_like(g64, 1e-12).copysign(g64), g64)
    xh = (f64(xout) - f64(beta)) / gs
    d = f64(dout) + (f64(dout2) if dout2 is not None else 0.0)
    g = d * g64
    dz = f64(rstd)[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if dz_extra is not None:
        dz = dz + f64(dz_extra)
    return dict(dz=dz, dgamma=(d * xh).sum(0), sc_dgamma=_col_scale(d, xh))


def _rms(z, gamma, eps):
    return z * torch.rsqrt(z.pow(2).mean(-1, keepdim=True) + eps) * gamma


def rmsnorm_fwd(y, r, gamma, eps):
    z = f64(y) + f64(r) if (y is not None and r is not None) else f64(y if y is not None else r)
    return dict(z=z, out=_rms(z, f64(gamma), eps), rstd=torch.rsqrt(z.pow(2).mean(-1) + eps))


def rmsnorm_bwd(z, gamma, eps, dout, dout2=None, dz_extra=None):
    zl, gl = _leaf(z), _leaf(gamma)
    d = f64(dout) + (f64(dout2) if dout2 is not None else 0.0)
    loss = (_rms(zl, gl, eps) * d).sum()
    if dz_extra is not None:
        loss = loss + (zl * f64(dz_extra)).sum()
    dz, dg = torch.autograd.grad(loss, (zl, gl))
    xh = _rms(zl.detach(), 1.0, eps)
    return dict(dz=dz, dgamma=dg, sc_dgamma=_col_scale(d, xh))


# ------------------------------------------------------------------------------------------
# softmax and cross-entropy
# ------------------------------------------------------------------------------------------
def softmax(x, dy=None):
    xl = _leaf(x)
    y = torch.softmax(xl, -1)
    out = dict(y=y.detach())
    if dy is not None:
        (out["dx"],) = torch.autograd.grad((y * f64(dy)).sum(), xl)
    return out


def cross_entropy(logits, labels, grad_out=1.0, ignore_index=-100):
    """Mean cross-entropy over the labelled rows: loss, lse [rows], dlogits for ``grad_out``."""
    zl = _leaf(logits)
    loss = F.cross_entropy(zl, labels.cpu().long(), ignore_index=ignore_index)
    (d,) = torch.autograd.grad(loss * float(grad_out), zl)
    return dict(loss=loss.detach(), lse=torch.logsumexp(zl.detach(), -1), dlogits=d)


def column_sums(d_rounded):
    """fp64 column sums of the dlogits as stored (the bias gradient), and their scale."""
    d = f64(d_rounded)
    return d.sum(0), d.abs().sum(0)


# ------------------------------------------------------------------------------------------
# elementwise ops
# ------------------------------------------------------------------------------------------
def activation(u, act, dy=None):
    ul = _leaf(u)
    if act == "gelu":
        a = F.gelu(ul)
    elif act == "gelu_tanh":
        a = F.gelu(ul, approximate="tanh")
    elif act == "relu":
        a = F.relu(ul)
    else:
        raise ValueError(act)
    out = dict(a=a.detach())
    if dy is not None:
        (out["du"],) = torch.autograd.grad((a * f64(dy)).sum(), ul)
        out["dbias"] = out["du"].reshape(-1, u.shape[-1]).sum(0)
        out["sc_dbias"] = out["du"].reshape(-1, u.shape[-1]).abs().sum(0)
    return out


def swiglu(gu, da=None):
    gl = _leaf(gu)
    f = gu.shape[-1] // 2
    a = F.silu(gl[..., :f]) * gl[..., f:]
    out = dict(a=a.detach())
    if da is not None:
        (out["dgu"],) = torch.autograd.grad((a * f64(da)).sum(), gl)
    return out


def rope(qkv, table, B, S, H, D, pos=None, inverse=False):
    """Rotate-half rotation of the q and k slices by the fp32 table the kernel receives (its
    rounding is not the kernel's), positions clamped into the table."""
    x = f64(qkv).clone()
    idx = torch.arange(S).repeat(B) if pos is None else pos.reshape(-1).cpu().long()
    idx = idx.clamp(0, table.shape[0] - 1)
    cs = f64(table)[idx]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    if inverse:
        s = -s
    q = x[:, :2 * H * D].reshape(B * S, 2 * H, D)
    x1, x2 = q[..., :D // 2], q[..., D // 2:]
    x[:, :2 * H * D] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(B * S, 2 * H * D)
    return x


def dropout_add(x, res, p, keep):
    k = f64(keep).view_as(x) / (1.0 - p) if p > 0 else 1.0
    return f64(res) + f64(x) * k


def adam(p, m, v, g, hp, mode):
    """One Adam / AdamW step in fp64.  ``hp`` is the fp32 array the kernel reads (lr, beta1, beta2,
    eps, weight decay, step, gradient scale) and the hyper-parameters are *those fp32 values*, upcast:
    the kernel forms 1.f - beta2 from the stored fp32 beta2, which is 4.7e-5 relative away from the
    double 1 - 0.999, and an oracle built from Python doubles would charge that choice -- made when
    the caller stored fp32 hyper-parameters -- to the kernel.  Mode bits as in ops/csrc/adam.hip:
    1 decoupled weight decay, 2 bias correction, 4 HF eps placement.  Returns (p, m, v)."""
    assert hp.dtype == torch.float32
    lr, b1, b2, eps, wd, step, gs = (float(t) for t in f64(hp)[:7])
    p, m, v = f64(p).clone(), f64(m), f64(v)
    g = f64(g) * gs
    if not (mode & 1) and wd != 0:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    if mode & 1:
        p = p - lr * wd * p
    bc1 = 1 - b1 ** step if mode & 2 else 1.0
    bc2s = math.sqrt(1 - b2 ** step) if mode & 2 else 1.0
    if mode & 4:
        p = p - lr * bc2s / bc1 * m / (v.sqrt() + eps)
    else:
        p = p - lr / bc1 * m / (v.sqrt() / bc2s + eps)
    return p, m, v


def sq_norm(x):
    return f64(x).pow(2).sum()


def scale_cast(src, scale, dscale=None):
    s = float(torch.tensor(scale, dtype=torch.float32))
    if dscale is not None:
        s = s * float(f64(dscale).reshape(-1)[0])
    return f64(src) * s
