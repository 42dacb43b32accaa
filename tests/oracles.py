"""Float64 oracles, a per-slice error metric and named input regimes for the streaming kernels
(LayerNorm, RMSNorm, row softmax, cross-entropy, activations, SwiGLU, RoPE, dropout-add, fused Adam,
sq-norm, scale-cast) and for attention.

A plain helper module: no fixtures, and nothing from the package but ``ops.rng.keep_mask`` and
``ops.rng.attn_keep_mask`` (the dropout keep bits are an input of the oracles, not something they
re-derive).  Every oracle takes
the kernel's inputs in their storage dtype, upcasts them to fp64 (exact for bf16 and fp32), builds
the forward from torch operators and takes every gradient with ``torch.autograd.grad`` -- no
hand-derived backward formulas, so a formula error in a kernel and in the CPU branch of
``ops/functional.py`` cannot hide in the oracle too.  The exceptions are ``layernorm_from_output``,
which *is* a formula by definition: the yardstick for the memory-efficient LayerNorm backward is the
fp64 evaluation of that form on the rounded output it is given; and ``attention_staged``, the flash
algorithm with its bf16 rounding points, which only measures what those roundings lose (it sets how
tight a bound on a kernel can be, never what the right answer is).

Column sums (dgamma, dbeta, dbias) come with a per-column scale: the sum over rows of the size of
the column's summands.  Where a summand holds a computed row quantity (x-hat in dgamma, dy in dbias),
its size is taken with that quantity's row maximum, because the row metric itself only holds x-hat and
dy to the tolerance times their row's largest element (an x-hat near zero is the difference of z and
the mean and carries the rounding of both); dbeta sums stored inputs, so its scale is sum |d|.
"""
import math

import torch
import torch.nn.functional as F

from distributed_training_and_deepspeed_amd.ops.rng import attn_keep_mask, keep_mask  # noqa: F401  (re-exported for the tests)

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


# ------------------------------------------------------------------------------------------
# attention (ops/attention.py: qkv [B*S, (H + 2 Hkv) D], ctx [B*S, H D], lse [B, H, S])
# ------------------------------------------------------------------------------------------
def _rb(t):
    """Round an fp64 tensor to bf16 and back (the kernels' rounding points of attention_staged)."""
    return t.to(torch.bfloat16).to(torch.float64)


def _attn_allowed(B, S, causal, key_range, doc_range):
    """[B, 1, S, S] bool (query, key): True where the key takes part.  None: every key does."""
    ok = None
    j = torch.arange(S)
    if causal:
        ok = (j.view(1, S) <= j.view(S, 1)).view(1, 1, S, S).expand(B, 1, S, S)
    if key_range is not None:
        kr = key_range.detach().cpu().long().view(B, 2)
        m = ((j.view(1, S) >= kr[:, :1]) & (j.view(1, S) < kr[:, 1:])).view(B, 1, 1, S).expand(B, 1, S, S)
        ok = m if ok is None else ok & m
    if doc_range is not None:
        r = getattr(doc_range, "ranges", doc_range).detach().cpu().long().view(B, S, 2)
        m = ((j.view(1, 1, S) >= r[:, :, :1]) & (j.view(1, 1, S) < r[:, :, 1:])).view(B, 1, S, S)
        ok = m if ok is None else ok & m
    return ok


def _attn_scores(q, ke, D, S, slopes, ok):
    """(scores with -inf for the keys left out, the same with 0 in rows that have no key, dead rows)."""
    s = q @ ke.transpose(-1, -2) / math.sqrt(D)
    if slopes is not None:
        s = s + f64(slopes).view(1, -1, 1, 1) * torch.arange(S, dtype=torch.float64).view(1, 1, 1, S)
    if ok is None:
        return s, s, torch.zeros(s.shape[:-1], dtype=torch.bool)
    s = s.masked_fill(~ok, -math.inf)
    dead = ~ok.any(-1).expand(s.shape[:-1])
    return s, s.masked_fill(dead[..., None], 0.0), dead


def _attn_keep(keep, p, like):
    """Dropout as a factor on the probabilities: keep / (1 - p), or None."""
    if p <= 0 or keep is None:
        return None
    return f64(keep).view_as(like) / (1.0 - p)


def attn_split(t, B, S, H, Hkv, D):
    """A [B*S, (H + 2 Hkv) D] tensor (qkv or dqkv) as its q [B, S, H, D] and k, v [B, S, Hkv, D] views."""
    x = t.reshape(B, S, H + 2 * Hkv, D)
    return x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]


def _attn_scales(P, dP, dO, O, q, ke, scale, G):
    """Row scales of dq [B, S, H] and dk [B, S, Hkv]: the size of the summands of dS = P (dP - delta)
    times the largest element of the key / query row they multiply, with delta taken as sum_d |dO||O|
    (|delta| would miss the cancellation inside delta itself)."""
    w = P * (dP.abs() + (dO.abs() * O.abs()).sum(-1, keepdim=True))          # [B, H, S, S]
    sc_dq = scale * (w * ke.abs().amax(-1)[:, :, None, :]).sum(-1)             # [B, H, S]
    sc_dk = scale * (w * q.abs().amax(-1)[:, :, :, None]).sum(-2)              # [B, H, S] over the keys
    B, H, S = sc_dk.shape
    sc_dk = sc_dk.view(B, H // G, G, S).sum(2)
    return sc_dq.transpose(1, 2), sc_dk.transpose(1, 2)


def attention(qkv, dctx, B, S, H, D, causal=False, slopes=None, p=0.0, keep=None, key_range=None, doc_range=None,
              kv_heads=None):
    """Scaled-dot-product attention and its gradients for the loss sum(ctx * dctx), in fp64 from torch
    operators and ``torch.autograd.grad``.  ``keep``: the [B, H, S, S] keep bits of ``ops.rng.
    attn_keep_mask`` (an input).  Grouped-query attention is ``repeat_interleave`` inside the graph, so
    autograd forms the group sum.  A row without a key has lse = -inf, ctx = 0 and takes part in no
    gradient -- written as a rule (probabilities 0), not left to NaN arithmetic.

    Returns ctx and dq [B, S, H, D] (one slice of the metric per (token, head) row: a kernel's [B*S, H D]
    ctx is reshaped to it, never the other way), lse [B, H, S], dk / dv [B, S, Hkv, D], the row scales sc_dq
    [B, S, H] and sc_dk [B, S, Hkv] (``_attn_scales``) and A [B, H, S] = max_j (scale sum_d |q||k| +
    |slope j|) over the row's keys, the size of the scores behind the lse."""
    Hkv = H if kv_heads is None else int(kv_heads)
    G = H // Hkv
    xl = _leaf(qkv).view(B, S, H + 2 * Hkv, D)
    q, k, v = (t.transpose(1, 2) for t in attn_split(xl, B, S, H, Hkv, D))
    ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    ok = _attn_allowed(B, S, causal, key_range, doc_range)
    s, s0, dead = _attn_scores(q, ke, D, S, slopes, ok)
    lse = torch.logsumexp(s0, -1).masked_fill(dead, -math.inf)
    P = torch.softmax(s0, -1).masked_fill(dead[..., None], 0.0)
    kf = _attn_keep(keep, p, P)
    Pd = P if kf is None else P * kf
    ctx = Pd @ ve                                                  # [B, H, S, D]
    dO = f64(dctx).view(B, S, H, D).transpose(1, 2)
    (g,) = torch.autograd.grad((ctx * dO).sum(), xl)
    dq, dk, dv = attn_split(g, B, S, H, Hkv, D)
    with torch.no_grad():
        dP = dO @ ve.transpose(-1, -2)
        if kf is not None:
            dP = dP * kf
        scale = 1.0 / math.sqrt(D)
        sc_dq, sc_dk = _attn_scales(P, dP, dO, ctx, q, ke, scale, G)
        a = scale * (q.abs() @ ke.abs().transpose(-1, -2))
        if slopes is not None:
            a = a + (f64(slopes).view(1, -1, 1, 1) * torch.arange(S, dtype=torch.float64).view(1, 1, 1, S)).abs()
        if ok is not None:
            a = a.masked_fill(~ok, 0.0)
    return dict(ctx=ctx.detach().transpose(1, 2), lse=lse.detach(), dq=dq, dk=dk, dv=dv,
                sc_dq=sc_dq, sc_dk=sc_dk, A=a.amax(-1))


def attention_staged(qkv, dctx, B, S, H, D, causal=False, slopes=None, p=0.0, keep=None, key_range=None,
                     doc_range=None, kv_heads=None):
    """The flash kernels' algorithm in fp64 with bf16 rounding exactly where they round: P (after
    dropout) before P V and P^T dO, dS before the dq / dk products, ctx before delta, and the outputs.
    Like ``layernorm_from_output`` not an independent oracle: its distance from ``attention`` is what the
    algorithm's rounding points have already lost on a given case.  Returns ctx, dq, dk, dv in the
    oracle's [B, S, heads, D] shapes."""
    Hkv = H if kv_heads is None else int(kv_heads)
    G = H // Hkv
    q, k, v = (t.transpose(1, 2) for t in attn_split(f64(qkv), B, S, H, Hkv, D))
    ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    ok = _attn_allowed(B, S, causal, key_range, doc_range)
    s, s0, dead = _attn_scores(q, ke, D, S, slopes, ok)
    P = torch.softmax(s0, -1).masked_fill(dead[..., None], 0.0)
    kf = _attn_keep(keep, p, P)
    Pb = _rb(P if kf is None else P * kf)
    dO = f64(dctx).view(B, S, H, D).transpose(1, 2)
    ctx = _rb(Pb @ ve)
    dv = Pb.transpose(-1, -2) @ dO
    dP = dO @ ve.transpose(-1, -2)
    if kf is not None:
        dP = dP * kf
    dS = _rb(P * (dP - (dO * ctx).sum(-1, keepdim=True)))
    scale = 1.0 / math.sqrt(D)
    dq = _rb(scale * (dS @ ke))
    dk = scale * (dS.transpose(-1, -2) @ q)
    dk, dv = (_rb(t.reshape(B, Hkv, G, S, D).sum(2)) for t in (dk, dv))
    return dict(ctx=ctx.transpose(1, 2), dq=dq.transpose(1, 2), dk=dk.transpose(1, 2),
                dv=dv.transpose(1, 2))


# attention input regimes: f(B, S, H, D, Hkv, seed) -> (qkv, dctx) bf16 (so exact in fp32 too).  Positions
# that depend on S are chosen per 64-key tile.
SPIKE_MAGS = (1.0, 1.5, 2.5, 2.6)


def spike_keys(S, descending=False):
    """One spike key per 64-key tile, at a position that is not tile-aligned, with the magnitudes
    1.0 / 1.5 / 2.5 / 2.6 (+2 per four tiles) ascending -- 8 c natural score units at D 64, so the
    running maximum crosses the kernels' defer-max threshold (8 log2 units) at some tiles and stays
    under it at others -- or the same magnitudes descending, from key 1 on."""
    nt = (S + 63) // 64
    pos = [64 * t + (5 + 13 * t) % min(64, S - 64 * t) for t in range(nt)]
    mags = [SPIKE_MAGS[t % 4] + 2.0 * (t // 4) for t in range(nt)]
    if descending:
        pos[0], mags = 1, mags[::-1]
    return list(zip(pos, mags))


def _attn_randn(B, S, H, D, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, H + 2 * Hkv, D, generator=g, dtype=torch.float32),
            torch.randn(B, S, H, D, generator=g, dtype=torch.float32))


def _spiked(x, H, spikes):
    """tests/test_attention_gpu.py ``_spiked_qkv``: half-scale inputs, every query of head 0 the
    direction u = 1, and the K row c u at each spike position of key head 0 (V stays random, so a
    wrongly weighted spike key shows in ctx)."""
    x = x * 0.5
    x[:, :, 0] = 1.0
    for key, c in spikes:
        x[:, key, H] = c
    return x


def attn_inputs(regime, B, S, H, D, kv_heads=None, seed=0):
    Hkv = H if kv_heads is None else int(kv_heads)
    x, d = _attn_randn(B, S, H, D, Hkv, seed)
    i, h = torch.arange(S).view(1, S, 1, 1), torch.arange(H).view(1, 1, H, 1)
    if regime == "gauss":
        pass
    elif regime == "peaked":                  # q, k x 2: score std 4
        x[:, :, :H + Hkv] *= 2.0
    elif regime == "onehot":                  # q, k x 4: score std 16, |lse| up to about 75
        x[:, :, :H + Hkv] *= 4.0
    elif regime == "row_scales":
        # small query / dctx rows next to large ones.  The exponent is shifted per head ((i + 3h) mod 13,
        # (i + 2h) mod 7, not i alone), so that the query heads of one GQA group differ in size at the
        # same token and the dK / dV group sum adds terms up to 2^6 apart
        x[:, :, :H] *= torch.exp2((((i + 3 * h) % 13) - 6) / 2.0)
        d *= torch.exp2((((i + 2 * h) % 7) - 3).float())
    elif regime == "k_offset":                # a large common-mode score: softmax is invariant
        x[:, :, H:H + Hkv] += 4.0
    elif regime == "spikes_up":
        x = _spiked(x, H, spike_keys(S))
    elif regime == "spikes_down":
        x = _spiked(x, H, spike_keys(S, descending=True))
    elif regime == "spike_at_edges":
        x = _spiked(x, H, [(0, 2.5), (S - 1, 2.6)])
    elif regime == "zero_rows":
        x[:, 0::5, :H] = 0.0
        d[:, 0::7] = 0.0
        x[:, S // 2, H + Hkv:] = 0.0
    else:
        raise ValueError(regime)
    return (x.reshape(B * S, (H + 2 * Hkv) * D).to(torch.bfloat16), d.reshape(B * S, H * D).to(torch.bfloat16))


ATTN_REGIMES = ("gauss", "peaked", "onehot", "row_scales", "k_offset", "spikes_up", "spikes_down", "spike_at_edges",
                "zero_rows")
