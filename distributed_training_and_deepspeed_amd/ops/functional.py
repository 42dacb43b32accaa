"""Functional front-end of the fused ops.

Each function runs the gfx950 HIP kernel for CUDA(HIP) tensors and the PyTorch reference
(same semantics and dropout masks as the kernels) for CPU tensors.  Parameter-gradient outputs
are written into caller-provided destination tensors (``main_grad`` views of the flat
gradient buffers, see ``parallel/flat.py``) with overwrite-or-accumulate semantics,
which is how the framework avoids a separate gradient-accumulation pass.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from .rng import RngState, keep_mask

ACT_CODES = {"none": 0, "gelu": 1, "gelu_tanh": 2, "relu": 3}
IGNORE_INDEX = -100


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _c(t):
    return None if t is None else t.contiguous()


# --------------------------------------------------------------------------------------
# dropout
# --------------------------------------------------------------------------------------
def _ref_dropout(x: torch.Tensor, p: float, rng: RngState, sid: int) -> torch.Tensor:
    if p <= 0.0:
        return x
    seed, step = (int(v) for v in rng.state.tolist())
    keep = keep_mask(x.numel(), p, seed, step, sid, device=x.device).view_as(x)
    return (x.float() * keep / (1.0 - p)).to(x.dtype)


def dropout(x: torch.Tensor, p: float, rng: RngState, sid: int) -> torch.Tensor:
    if p <= 0.0:
        return x
    if not _on_gpu(x):
        return _ref_dropout(x, p, rng, sid)
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.call("dtd_dropout", _lib.dt(x), x.data_ptr(), None, y.data_ptr(), x.numel(), float(p),
              rng.state.data_ptr(), sid, _lib.stream())
    return y


def dropout_add(x: torch.Tensor, res: torch.Tensor, p: float, rng: RngState, sid: int) -> torch.Tensor:
    """res + dropout(x) in one pass (sum in fp32); same keep bits as ``dropout(x, p, rng, sid)``."""
    if not _on_gpu(x):
        return res + dropout(x, p, rng, sid)
    assert x.shape == res.shape and x.dtype == res.dtype
    x, res = x.contiguous(), res.contiguous()
    y = torch.empty_like(x)
    _lib.call("dtd_dropout", _lib.dt(x), x.data_ptr(), res.data_ptr(), y.data_ptr(), x.numel(), float(p),
              rng.state.data_ptr(), sid, _lib.stream())
    return y


# --------------------------------------------------------------------------------------
# residual + dropout + LayerNorm
# --------------------------------------------------------------------------------------
def ln_fwd(y, r, gamma, beta, eps: float, p: float, rng: RngState, sid: int, store_z: bool = True):
    """z = r + dropout(y); out = LN(z).  Returns (z, out, mean, rstd); z is None when it
    equals an input (no branch) or store_z is False."""
    ref = y if y is not None else r
    rows = ref.numel() // ref.shape[-1]
    h = ref.shape[-1]
    if not _on_gpu(ref):
        z = torch.zeros_like(ref, dtype=torch.float32)
        if y is not None:
            z = z + _ref_dropout(y, p, rng, sid).float()
        if r is not None:
            z = z + r.float()
        zf = z.view(rows, h)
        mean = zf.mean(-1)
        var = zf.var(-1, unbiased=False)
        rstd = torch.rsqrt(var + eps)
        out = ((zf - mean[:, None]) * rstd[:, None] * gamma.float() + beta.float()).to(ref.dtype).view_as(ref)
        zz = z.to(ref.dtype) if (store_z and y is not None) else None
        return zz, out, mean, rstd
    y, r = _c(y), _c(r)
    z = torch.empty_like(ref) if (store_z and y is not None) else None
    out = torch.empty_like(ref)
    mean = torch.empty(rows, dtype=torch.float32, device=ref.device)
    rstd = torch.empty_like(mean)
    _lib.call("dtd_ln_fwd", _lib.dt(ref), _lib.ptr(y), _lib.ptr(r), gamma.data_ptr(), beta.data_ptr(),
              _lib.ptr(z), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, h, float(eps),
              float(p if y is not None else 0.0), rng.state.data_ptr(), sid, _lib.stream())
    return z, out, mean, rstd


def _unpack(dst, acc):
    """Gradient destinations are a tensor (with the call's ``acc``) or a (tensor, acc) pair."""
    if isinstance(dst, tuple):
        return dst
    return dst, acc


def _write_grad(dst, val: torch.Tensor, acc: bool) -> None:
    if dst is None:
        return
    dst, acc = _unpack(dst, acc)
    if acc:
        dst.add_(val.to(dst.dtype))
    else:
        dst.copy_(val)


def _finalize_stream(part: torch.Tensor, defer: bool = True) -> int:
    """Stream for a column-sum finalize of gradient partials.  Inside a DDP backward window
    (``grad.defer_finalize``) the ~10 us finalize launches go to the async-gradient side stream,
    off the dgrad chain: the side stream waits for the partials' producer, the partial buffer is
    held until the join, and the reducer joins it before any collective or the optimizer reads a
    gradient (``join_async_wgrad``)."""
    from .grad import finalize_side_stream
    side = finalize_side_stream(part.device) if defer and part.is_cuda else None
    if side is None:
        return _lib.stream()
    side.wait_stream(torch.cuda.current_stream(part.device))
    from .grad import hold_until_join
    hold_until_join(part)   # freed after the reducer's join (not record_stream: ops/grad.py emit_wgrad)
    return side.cuda_stream


# Batched finalizes.  Inside an autograd backward the column-sum finalizes (bias / LayerNorm
# gradients from fp32 partials) are queued and launched together -- one kernel per batch of up to 32
# (``dtd_colsum_finalize_batch``) -- when something is about to read a gradient: the DDP / ZeRO
# reducers flush before they launch a bucket's collective, and the end of the backward flushes the
# rest (an autograd-engine callback).  The queue holds the partial buffers, so the caching
# allocator cannot hand their memory to a later kernel first.  DTD_FINALIZE_BATCH=0: launch each
# finalize where it is issued (the round-5 behaviour).
_BATCH = [os.environ.get("DTD_FINALIZE_BATCH", "1") == "1"]
_PENDING: list = []        # (stream handle, job tuple, keep-alive tensors)
_PENDING_DST: set = set()
_CB_QUEUED = [False]


class _Job(ctypes.Structure):
    _fields_ = [("part", ctypes.c_void_p), ("out", ctypes.c_void_p), ("nparts", ctypes.c_int), ("cols", ctypes.c_int),
                ("dtype", ctypes.c_int), ("acc", ctypes.c_int), ("scale", ctypes.c_float), ("pad", ctypes.c_int)]


def set_finalize_batching(on: bool) -> None:
    flush_finalizes()
    _BATCH[0] = bool(on)


def _batching(part: torch.Tensor) -> bool:
    return (_BATCH[0] and part.is_cuda and _lib.has("dtd_colsum_finalize_batch")
            and torch._C._current_graph_task_id() != -1)


def _queue(stream: int, jobs, keep) -> None:
    """Queue finalize jobs (part_ptr, out_ptr, nparts, cols, dtype, acc, scale) on ``stream``."""
    dsts = {j[1] for j in jobs}
    if dsts & _PENDING_DST:      # a second finalize into the same gradient: keep them ordered
        flush_finalizes()
    for j in jobs:
        _PENDING.append((stream, j, keep))
        _PENDING_DST.add(j[1])
    if not _CB_QUEUED[0]:
        _CB_QUEUED[0] = True
        torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)


def _end_of_backward() -> None:
    _CB_QUEUED[0] = False
    flush_finalizes()


def flush_finalizes() -> None:
    """Launch every queued finalize (on the stream it was issued on, in issue order)."""
    if not _PENDING:
        return
    pending = list(_PENDING)
    _PENDING.clear()
    _PENDING_DST.clear()
    i = 0
    while i < len(pending):
        stream = pending[i][0]
        batch = []
        while i < len(pending) and pending[i][0] == stream and len(batch) < 32:
            batch.append(pending[i][1])
            i += 1
        arr = (_Job * len(batch))(*[_Job(*j, 0) for j in batch])
        _lib.call("dtd_colsum_finalize_batch", len(batch), ctypes.addressof(arr), stream)


def _finalize(part: torch.Tensor, n: int, cols: int, dst, acc: bool, scale: float = 1.0, defer: bool = True):
    if dst is None:
        return
    dst, acc = _unpack(dst, acc)
    stream = _finalize_stream(part, defer)
    if stream == _lib.stream() and _batching(part):
        _queue(stream, [(part.data_ptr(), dst.data_ptr(), n, cols, _lib.dt(dst), int(acc), float(scale))], (part, dst))
        return
    _lib.call("dtd_colsum_finalize", part.data_ptr(), n, cols, dst.data_ptr(), _lib.dt(dst), int(acc),
              float(scale), stream)


def ln_bwd(dout, dz_extra, z, mean, rstd, gamma, p: float, rng: RngState, sid: int,
           want_dz: bool = True, want_dy: bool = False,
           dgamma=None, dbeta=None, dbias=None, acc: bool = False, dout2=None, xout=None, beta=None):
    """Backward of ``ln_fwd``.  Returns (dz, dy); writes dgamma/dbeta/dbias (bias of the
    producer of y, i.e. column sums of dy) into the destination tensors.  ``dout2``: a second
    upstream gradient summed into ``dout`` inside the kernel (residual branches).

    Memory-efficient form (``z=None``, ``xout``/``beta`` given): x-hat is recomputed from the
    forward's output, x-hat = (xout - beta) / gamma, so the forward need not store z
    (``ln_fwd(store_z=False)``); ``mean`` is then unused."""
    rows = dout.numel() // dout.shape[-1]
    h = dout.shape[-1]
    fo = z is None
    if fo and (xout is None or beta is None):
        raise ValueError("ln_bwd: z=None needs the LayerNorm output (xout) and beta")
    if not _on_gpu(dout):
        if fo:
            g32 = gamma.float()
            g32 = torch.where(g32.abs() < 1e-12, torch.full_like(g32, 1e-12).copysign(g32), g32)
            xh = (xout.float().view(rows, h) - beta.float()) / g32
        else:
            zf = z.float().view(rows, h)
            xh = (zf - mean[:, None]) * rstd[:, None]
        d = dout.float().view(rows, h)
        if dout2 is not None:
            d = d + dout2.float().view(rows, h)
        g = d * gamma.float()
        m1 = g.mean(-1, keepdim=True)
        m2 = (g * xh).mean(-1, keepdim=True)
        dz = rstd[:, None] * (g - m1 - xh * m2)
        if dz_extra is not None:
            dz = dz + dz_extra.float().view(rows, h)
        dy = None
        if want_dy:
            dy = _ref_dropout(dz.to(dout.dtype), p, rng, sid) if p > 0 else dz.to(dout.dtype)
            _write_grad(dbias, dy.float().sum(0), acc)
            dy = dy.view_as(dout)
        _write_grad(dgamma, (d * xh).sum(0), acc)
        _write_grad(dbeta, d.sum(0), acc)
        return (dz.to(dout.dtype).view_as(dout) if want_dz else None), dy
    dout, dz_extra, dout2 = _c(dout), _c(dz_extra), _c(dout2)
    dz = torch.empty_like(dout) if want_dz else None
    dy = torch.empty_like(dout) if want_dy else None
    n = _lib.lib().dtd_ln_bwd_num_partials(rows, h)
    k = int(dgamma is not None) + int(dbeta is not None) + int(dbias is not None and want_dy)
    part = torch.empty((max(k, 1), n, h), dtype=torch.float32, device=dout.device)
    slots = iter(range(k))
    pg = part[next(slots)] if dgamma is not None else None
    pb = part[next(slots)] if dbeta is not None else None
    py = part[next(slots)] if (dbias is not None and want_dy) else None
    if fo:
        xout = xout.contiguous()
        assert xout.shape == dout.shape and xout.dtype == dout.dtype
        _lib.call("dtd_ln_bwd_fo", _lib.dt(dout), dout.data_ptr(), _lib.ptr(dout2), _lib.ptr(dz_extra),
                  xout.data_ptr(), beta.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), _lib.ptr(dz), _lib.ptr(dy),
                  _lib.ptr(pg), _lib.ptr(pb), _lib.ptr(py), rows, h, float(p if want_dy else 0.0),
                  rng.state.data_ptr(), sid, _lib.stream())
    else:
        _lib.call("dtd_ln_bwd", _lib.dt(dout), dout.data_ptr(), _lib.ptr(dout2), _lib.ptr(dz_extra), z.data_ptr(),
                  mean.data_ptr(),
                  rstd.data_ptr(), gamma.data_ptr(), _lib.ptr(dz), _lib.ptr(dy), _lib.ptr(pg), _lib.ptr(pb),
                  _lib.ptr(py), rows, h, float(p if want_dy else 0.0), rng.state.data_ptr(), sid, _lib.stream())
    dsts = [d for d, on in ((dgamma, pg is not None), (dbeta, pb is not None), (dbias, py is not None)) if on]
    if dsts:
        args = []
        for d in dsts + [None] * (3 - len(dsts)):
            if d is None:
                args += [None, 0, 0]
            else:
                t, a = _unpack(d, acc)
                args += [t.data_ptr(), _lib.dt(t), int(a)]
        stream = _finalize_stream(part)
        if stream == _lib.stream() and _batching(part):
            jobs = []
            for i, d in enumerate(dsts):
                t, a = _unpack(d, acc)
                jobs.append((part.data_ptr() + i * n * h * 4, t.data_ptr(), n, h, _lib.dt(t), int(a), 1.0))
            _queue(stream, jobs, (part, [_unpack(d, acc)[0] for d in dsts]))
        else:
            _lib.call("dtd_colsum_finalize_multi", len(dsts), part.data_ptr(), n, h, *args, stream)
    return dz, dy


# --------------------------------------------------------------------------------------
# activations
# --------------------------------------------------------------------------------------
def _ref_act(u: torch.Tensor, act: str) -> torch.Tensor:
    x = u.float()
    if act == "gelu":
        y = 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    elif act == "gelu_tanh":
        y = 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    elif act == "relu":
        y = torch.clamp_min(x, 0.0)
    else:
        y = x
    return y.to(u.dtype)


def _ref_act_grad(u: torch.Tensor, act: str) -> torch.Tensor:
    x = u.float()
    if act == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))
        return cdf + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
    if act == "gelu_tanh":
        k = 0.7978845608028654
        t = torch.tanh(k * (x + 0.044715 * x ** 3))
        return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * (x * x).clamp_max(1e30))
    if act == "relu":
        return (x > 0).float()
    return torch.ones_like(x)


def act_fwd(u: torch.Tensor, act: str) -> torch.Tensor:
    if act == "none":
        return u
    if not _on_gpu(u):
        return _ref_act(u, act)
    u = u.contiguous()
    y = torch.empty_like(u)
    _lib.call("dtd_act_fwd", _lib.dt(u), u.data_ptr(), y.data_ptr(), u.numel(), ACT_CODES[act], _lib.stream())
    return y


def act_bwd(dy: torch.Tensor, u: torch.Tensor | None, act: str, dbias=None, acc: bool = False,
            want_du: bool = True, want_act: bool = False):
    """du = dy * act'(u); writes column sums of du into ``dbias``.  act='none' is a plain
    bias-gradient column sum of dy (returns dy).  ``want_act``: also return act(u), recomputed
    in the same pass -> (du, a)."""
    cols = dy.shape[-1]
    rows = dy.numel() // cols
    if want_act and act == "none":
        raise ValueError("want_act needs an activation")
    if not _on_gpu(dy):
        du = dy.float() if act == "none" else dy.float() * _ref_act_grad(u, act)
        _write_grad(dbias, du.view(rows, cols).sum(0), acc)
        du = du.to(dy.dtype) if want_du else None
        return (du, act_fwd(u, act)) if want_act else du
    dy = dy.contiguous()
    du = torch.empty_like(dy) if (want_du and act != "none") else None
    a = torch.empty_like(u) if want_act else None
    n = _lib.lib().dtd_act_bwd_num_partials(rows, cols)
    part = torch.empty((n, cols), dtype=torch.float32, device=dy.device) if dbias is not None else None
    _lib.call("dtd_act_bwd", _lib.dt(dy), dy.data_ptr(), _lib.ptr(u), _lib.ptr(du), _lib.ptr(part), _lib.ptr(a),
              rows, cols, ACT_CODES[act], _lib.stream())
    if part is not None:
        _finalize(part, n, cols, dbias, acc)
    du = dy if act == "none" else du
    return (du, a) if want_act else du


def bias_grad(dy: torch.Tensor, dbias: torch.Tensor, acc: bool = False) -> None:
    act_bwd(dy, None, "none", dbias=dbias, acc=acc, want_du=False)


# --------------------------------------------------------------------------------------
# Llama-family ops: residual + RMSNorm, rotary embedding, SwiGLU (ops/csrc/rmsnorm.hip, rope.hip,
# swiglu.hip).  Each runs its kernel for bf16 / fp32 tensors on the GPU and the same math in fp32
# PyTorch elsewhere (CPU, a shape the kernels do not take, or a library built before they existed).
# --------------------------------------------------------------------------------------
def _kernel_dtype(t: torch.Tensor) -> bool:
    return _on_gpu(t) and t.dtype in (torch.bfloat16, torch.float32)


def _rms_kernel(t: torch.Tensor, h: int) -> bool:
    return _kernel_dtype(t) and _lib.has("dtd_rms_fwd") and bool(_lib.lib().dtd_rms_supported(h))


def rms_fwd(y, r, gamma, eps: float):
    """z = r + y (either may be None); out = z * rsqrt(mean(z^2) + eps) * gamma, in fp32, rounded
    once.  Returns (z, out, rstd); z is None unless both y and r are given (it is then an input)."""
    ref = y if y is not None else r
    h = ref.shape[-1]
    rows = ref.numel() // h
    both = y is not None and r is not None
    if not _rms_kernel(ref, h):
        zf = ref.float() if not both else y.float() + r.float()
        z2 = zf.reshape(rows, h)
        rstd = torch.rsqrt(z2.pow(2).mean(-1) + eps)
        out = (z2 * rstd[:, None] * gamma.float()).to(ref.dtype).view_as(ref)
        return (zf.to(ref.dtype) if both else None), out, rstd
    y, r, gamma = _c(y), _c(r), gamma.contiguous()
    assert gamma.dtype == ref.dtype and (not both or (y.shape == r.shape and y.dtype == r.dtype))
    z = torch.empty_like(ref) if both else None
    out = torch.empty_like(ref)
    rstd = torch.empty(rows, dtype=torch.float32, device=ref.device)
    _lib.call("dtd_rms_fwd", _lib.dt(ref), _lib.ptr(y), _lib.ptr(r), gamma.data_ptr(), _lib.ptr(z), out.data_ptr(),
              rstd.data_ptr(), rows, h, float(eps), _lib.stream())
    return z, out, rstd


def rms_bwd(dout, dz_extra, z, rstd, gamma, dgamma=None, acc: bool = False, dout2=None):
    """Backward of ``rms_fwd`` for its input sum z: g = (dout + dout2) * gamma, x-hat = z * rstd,
    dz = rstd * (g - x-hat * mean(g * x-hat)) + dz_extra.  Writes the column sums of
    (dout + dout2) * x-hat into ``dgamma`` (a tensor with ``acc``, or a (tensor, acc) pair) through
    fp32 per-block partials and the deterministic column-sum finalize."""
    h = dout.shape[-1]
    rows = dout.numel() // h
    if not _rms_kernel(dout, h):
        d = dout.float().reshape(rows, h)
        if dout2 is not None:
            d = d + dout2.float().reshape(rows, h)
        xh = z.float().reshape(rows, h) * rstd[:, None]
        g = d * gamma.float()
        dz = rstd[:, None] * (g - xh * (g * xh).mean(-1, keepdim=True))
        if dz_extra is not None:
            dz = dz + dz_extra.float().reshape(rows, h)
        _write_grad(dgamma, (d * xh).sum(0), acc)
        return dz.to(dout.dtype).view_as(dout)
    dout, dz_extra, dout2, z, gamma = _c(dout), _c(dz_extra), _c(dout2), z.contiguous(), gamma.contiguous()
    assert z.dtype == dout.dtype and z.numel() == dout.numel() and gamma.dtype == dout.dtype
    dz = torch.empty_like(dout)
    part = None
    if dgamma is not None:
        n = _lib.lib().dtd_rms_bwd_num_partials(rows, h)
        part = torch.empty((n, h), dtype=torch.float32, device=dout.device)
    _lib.call("dtd_rms_bwd", _lib.dt(dout), dout.data_ptr(), _lib.ptr(dout2), _lib.ptr(dz_extra), z.data_ptr(),
              rstd.data_ptr(), gamma.data_ptr(), dz.data_ptr(), _lib.ptr(part), rows, h, _lib.stream())
    if part is not None:
        _finalize(part, n, h, dgamma, acc)
    return dz


def rope_table(max_positions: int, head_dim: int, theta: float = 10000.0, device="cpu") -> torch.Tensor:
    """(cos, sin) of p * theta^(-2j/D) for p < max_positions, j < D/2: fp32 [max_positions, D/2, 2],
    rounded once from float64 angles."""
    if head_dim % 2:
        raise ValueError("rope_table: head_dim must be even")
    j = torch.arange(head_dim // 2, dtype=torch.float64)
    inv = torch.pow(torch.tensor(float(theta), dtype=torch.float64), -2.0 * j / head_dim)
    ang = torch.arange(max_positions, dtype=torch.float64)[:, None] * inv[None]
    return torch.stack([ang.cos(), ang.sin()], -1).to(torch.float32).to(device).contiguous()


def rope_(qkv: torch.Tensor, table: torch.Tensor, B: int, S: int, H: int, D: int, pos: torch.Tensor | None = None,
          inverse: bool = False, kv_heads: int | None = None) -> torch.Tensor:
    """Rotate the q and k slices of the packed ``qkv [B*S, 3*H*D]`` IN PLACE (HF's rotate-half
    convention; v untouched) and return it.  ``table``: ``rope_table`` on qkv's device.  ``pos``:
    optional integer [B, S] position per token (default s).  ``inverse`` negates the sine: the inverse
    rotation, which is also the adjoint -- the backward is ``rope_(dqkv, ..., inverse=True)``.

    ``kv_heads`` (grouped-query attention, ops/attention.py): qkv is ``[B*S, (H + 2*Hkv)*D]`` and the
    H + Hkv heads of its q and k blocks are rotated."""
    Hkv = H if kv_heads is None else int(kv_heads)
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"rope_: kv_heads = {Hkv} must divide the {H} query heads")
    width, nrot = (H + 2 * Hkv) * D, H + Hkv
    if qkv.dim() != 2 or qkv.shape[0] != B * S or qkv.shape[1] != width or qkv.stride(1) != 1:
        raise ValueError(f"rope_: qkv must be [B*S, (H + 2*Hkv)*D] = [{B * S}, {width}], got {tuple(qkv.shape)}")
    if tuple(table.shape[1:]) != (D // 2, 2) or table.dtype != torch.float32 or table.device != qkv.device:
        raise ValueError("rope_: table must be rope_table(max_positions, D) (fp32 [P, D/2, 2]) on qkv's device")
    if pos is None and S > table.shape[0]:
        raise ValueError(f"rope_: sequence length {S} exceeds the table's {table.shape[0]} positions")
    if pos is not None and pos.numel() != B * S:
        raise ValueError("rope_: pos needs one position per token")
    if _kernel_dtype(qkv) and D % 16 == 0 and qkv.stride(0) % 8 == 0 and qkv.data_ptr() % 16 == 0 \
            and _lib.has("dtd_rope"):
        table = table.contiguous()
        p32 = pos.reshape(-1).to(device=qkv.device, dtype=torch.int32).contiguous() if pos is not None else None
        if Hkv != H:
            if not _lib.has("dtd_rope_heads"):
                raise _lib.KernelError("the kernel library has no grouped-query rope entry point (stale build)")
            _lib.call("dtd_rope_heads", _lib.dt(qkv), qkv.data_ptr(), table.data_ptr(), _lib.ptr(p32), B, S, nrot, D,
                      qkv.stride(0), table.shape[0], int(inverse), _lib.stream())
            return qkv
        _lib.call("dtd_rope", _lib.dt(qkv), qkv.data_ptr(), table.data_ptr(), _lib.ptr(p32), B, S, H, D,
                  qkv.stride(0), table.shape[0], int(inverse), _lib.stream())
        return qkv
    if pos is None:
        idx = torch.arange(S, device=qkv.device).repeat(B)
    else:
        idx = pos.reshape(-1).to(device=qkv.device, dtype=torch.int64).clamp(0, table.shape[0] - 1)
    cs = table[idx]                                    # [B*S, D/2, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    if inverse:
        s = -s
    x = qkv[:, :nrot * D].reshape(B * S, nrot, D).float()
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    qkv[:, :nrot * D] = out.reshape(B * S, nrot * D).to(qkv.dtype)
    return qkv


def rope_append_(qkv: torch.Tensor, table: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                 kv_len: torch.Tensor, B: int, Sq: int, H: int, D: int, kv_heads: int | None = None,
                 overflow: torch.Tensor | None = None, k_scale: torch.Tensor | None = None,
                 v_scale: torch.Tensor | None = None) -> torch.Tensor:
    """``rope_`` with ``pos = kv_len[b] + s`` IN PLACE on the packed ``qkv [B*Sq, (H + 2*Hkv)*D]`` (bitwise
    the same rotation), plus the KV-cache append: the rotated k row and the v row of token (b, s) go to
    slot ``kv_len[b] + s`` of ``k_cache`` / ``v_cache [B, Hkv, Smax, D]``.  ``kv_len``: device int32 [B],
    read on the device and NOT advanced (the caller adds Sq once per step, after the last layer).  A slot
    outside [0, Smax) is not written and sets ``overflow`` (an int32 tensor of one element) to 1.  Returns qkv.

    FP8 caches (``torch.float8_e4m3fn``, with ``k_scale`` / ``v_scale`` fp32 ``[B, Hkv, Smax]``): qkv is
    rotated exactly as above and each row is quantised by ``ops.kv_cache.quantize_kv_ref``'s law -- D codes and
    one scale per slot, neither written for a row that does not fit.  bf16 on the GPU with D 64 / 128 runs the
    quantising kernel (same codes and scales, bit for bit); everything else -- the CPU, fp32 activations,
    another D -- the PyTorch reference."""
    fp8 = k_cache.dtype == torch.float8_e4m3fn or v_cache.dtype == torch.float8_e4m3fn or k_scale is not None \
        or v_scale is not None
    Hkv = H if kv_heads is None else int(kv_heads)
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"rope_append_: kv_heads = {Hkv} must divide the {H} query heads")
    width = (H + 2 * Hkv) * D
    if qkv.dim() != 2 or qkv.shape[0] != B * Sq or qkv.shape[1] != width or qkv.stride(1) != 1:
        raise ValueError(f"rope_append_: qkv must be [B*Sq, (H + 2*Hkv)*D] = [{B * Sq}, {width}], got {tuple(qkv.shape)}")
    if tuple(table.shape[1:]) != (D // 2, 2) or table.dtype != torch.float32 or table.device != qkv.device:
        raise ValueError("rope_append_: table must be rope_table(max_positions, D) (fp32 [P, D/2, 2]) on qkv's device")
    want = torch.float8_e4m3fn if fp8 else qkv.dtype
    if k_cache.dim() != 4 or tuple(k_cache.shape[:2]) != (B, Hkv) or k_cache.shape[3] != D \
            or v_cache.shape != k_cache.shape or k_cache.dtype != want or v_cache.dtype != want \
            or not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError(f"rope_append_: k_cache / v_cache must both be contiguous [B, Hkv, Smax, D] = [{B}, {Hkv}, Smax, {D}] "
                         f"of {'float8_e4m3fn (an FP8 cache)' if fp8 else 'the dtype of qkv'}, got "
                         f"{tuple(k_cache.shape)} {k_cache.dtype} / {tuple(v_cache.shape)} {v_cache.dtype}")
    Smax = k_cache.shape[2]
    for name, sc in (("k_scale", k_scale), ("v_scale", v_scale)) if fp8 else ():
        if sc is None or tuple(sc.shape) != (B, Hkv, Smax) or sc.dtype != torch.float32 or not sc.is_contiguous() \
                or sc.device != k_cache.device:
            raise ValueError(f"rope_append_: an FP8 cache needs {name}, contiguous fp32 [B, Hkv, Smax] = [{B}, {Hkv}, {Smax}]")
    if kv_len.numel() != B:
        raise ValueError(f"rope_append_: kv_len must hold one length per sequence ({B})")
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=qkv.device)
    # the kernels' domains: the plain append takes both kernel dtypes and any D % 16; the quantising one bf16, D 64 / 128
    kernel = (qkv.is_cuda and qkv.dtype == torch.bfloat16 and D in (64, 128)) if fp8 else (_kernel_dtype(qkv) and D % 16 == 0)
    if kernel and qkv.stride(0) % 8 == 0 and qkv.data_ptr() % 16 == 0:
        entry = "dtd_rope_append_fp8" if fp8 else "dtd_rope_append"
        if not _lib.has(entry):
            raise _lib.KernelError(f"the kernel library has no {'FP8 ' if fp8 else ''}KV-cache append entry point (stale build)")
        table = table.contiguous()
        kv32 = kv_len.reshape(-1).to(device=qkv.device, dtype=torch.int32).contiguous()
        head = (qkv.data_ptr(), table.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr())
        head = (head + (k_scale.data_ptr(), v_scale.data_ptr())) if fp8 else ((_lib.dt(qkv),) + head)
        _lib.call(entry, *head, kv32.data_ptr(), overflow.data_ptr(), B, Sq, H, Hkv, D, qkv.stride(0), Smax,
                  table.shape[0], _lib.stream())
        return qkv
    slot = kv_len.reshape(B, 1).to(device=qkv.device, dtype=torch.int64) + torch.arange(Sq, device=qkv.device)
    rope_(qkv, table, B, Sq, H, D, pos=slot, kv_heads=Hkv)
    x = qkv.view(B, Sq, H + 2 * Hkv, D)
    pairs = ((k_cache, x[:, :, H:H + Hkv]), (v_cache, x[:, :, H + Hkv:]))
    if fp8:
        from .kv_cache import quantize_kv_ref
        (kq, ks), (vq, vs) = (quantize_kv_ref(new) for _, new in pairs)
        pairs = ((k_cache.view(torch.uint8), kq.view(torch.uint8)), (k_scale.unsqueeze(-1), ks.unsqueeze(-1)),
                 (v_cache.view(torch.uint8), vq.view(torch.uint8)), (v_scale.unsqueeze(-1), vs.unsqueeze(-1)))
    _append_rows_ref(slot, overflow, pairs)
    return qkv


def _append_rows_ref(slot: torch.Tensor, overflow: torch.Tensor, pairs) -> None:
    """The append of ``rope_append_``'s PyTorch branch: for every (cache ``[B, Hkv, Smax, W]``, new
    ``[B, Sq, Hkv, W]``) of ``pairs``, row (b, s) of new into slot ``slot[b, s]`` of cache; a slot outside
    [0, Smax) is not written and raises ``overflow``."""
    B, Sq = slot.shape
    dev = slot.device
    Hkv, Smax = pairs[0][0].shape[1:3]
    fits = (slot >= 0) & (slot < Smax)
    overflow.copy_(torch.maximum(overflow, (~fits).any().to(overflow.dtype).reshape(overflow.shape)))
    # index_copy_ with the slots clamped into the cache.  A row that does not fit lands on slot 0 or
    # Smax - 1 and carries what that slot ends up holding anyway -- the row that does belong there, if the
    # step has one, else the slot's old content -- so duplicate indices all write the same value.
    clamped = slot.clamp(0, Smax - 1)                                                   # [B, Sq]
    writer = clamped - (slot - torch.arange(Sq, device=dev))                            # the s that owns the slot
    has = ((writer >= 0) & (writer < Sq)).view(B, 1, Sq, 1)
    rows = (torch.arange(B, device=dev).view(B, 1, 1) * Hkv
            + torch.arange(Hkv, device=dev).view(1, Hkv, 1)) * Smax + clamped.view(B, 1, Sq)
    for cache, new in pairs:
        W = cache.shape[3]
        pick = writer.clamp(0, Sq - 1).view(B, 1, Sq, 1).expand(B, Hkv, Sq, W)
        flat = cache.view(B * Hkv * Smax, W)
        val = torch.where(has, new.transpose(1, 2).gather(2, pick), flat[rows.reshape(-1)].view(B, Hkv, Sq, W))
        flat.index_copy_(0, rows.reshape(-1), val.reshape(-1, W))


def _swiglu_kernel(t: torch.Tensor, f: int) -> bool:
    return _kernel_dtype(t) and f % 8 == 0 and _lib.has("dtd_swiglu_fwd")


def swiglu_fwd(gu: torch.Tensor) -> torch.Tensor:
    """a = silu(gate) * up for ``gu [rows, 2f]`` = (gate | up)."""
    f = gu.shape[-1] // 2
    if gu.shape[-1] != 2 * f:
        raise ValueError("swiglu_fwd: gu needs an even number of columns (gate | up)")
    rows = gu.numel() // (2 * f)
    if not _swiglu_kernel(gu, f):
        g, u = gu.float().split(f, -1)
        return (g * torch.sigmoid(g) * u).to(gu.dtype)
    gu = gu.contiguous()
    a = torch.empty(gu.shape[:-1] + (f,), dtype=gu.dtype, device=gu.device)
    _lib.call("dtd_swiglu_fwd", _lib.dt(gu), gu.data_ptr(), a.data_ptr(), rows, f, _lib.stream())
    return a


def swiglu_bwd(da: torch.Tensor, gu: torch.Tensor, want_act: bool = False):
    """dgu = (dgate | dup) with dgate = da * up * sig(g) * (1 + g * (1 - sig(g))) and
    dup = da * silu(g).  ``want_act``: also return a = silu(gate) * up, rewritten in the same pass
    (bitwise the forward's) -> (dgu, a)."""
    f = gu.shape[-1] // 2
    rows = gu.numel() // (2 * f)
    if not _swiglu_kernel(gu, f):
        g, u = gu.float().split(f, -1)
        sg = torch.sigmoid(g)
        d = da.float()
        dgu = torch.cat([d * u * sg * (1 + g * (1 - sg)), d * (g * sg)], -1).to(gu.dtype)
        return (dgu, swiglu_fwd(gu)) if want_act else dgu
    gu, da = gu.contiguous(), da.contiguous()
    assert da.dtype == gu.dtype and da.numel() == rows * f
    dgu = torch.empty_like(gu)
    a = torch.empty_like(da) if want_act else None
    _lib.call("dtd_swiglu_bwd", _lib.dt(gu), da.data_ptr(), gu.data_ptr(), dgu.data_ptr(), _lib.ptr(a), rows, f,
              _lib.stream())
    return (dgu, a) if want_act else dgu


# --------------------------------------------------------------------------------------
# softmax cross-entropy
# --------------------------------------------------------------------------------------
def xent_fwd(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = IGNORE_INDEX):
    """Returns (mean loss [scalar fp32 tensor], lse [N], stats [2] = (mean, count))."""
    V = logits.shape[-1]
    rows = logits.numel() // V
    labels = labels.reshape(-1)
    if not _on_gpu(logits):
        z = logits.float().view(rows, V)
        lse = torch.logsumexp(z, -1)
        valid = labels != ignore_index
        tgt = z.gather(1, labels.clamp_min(0)[:, None])[:, 0]
        loss_row = torch.where(valid, lse - tgt, torch.zeros_like(lse))
        cnt = valid.sum().float()
        mean = loss_row.sum() / cnt
        return mean, lse, torch.stack([mean, cnt])
    logits = logits.contiguous()
    labels = labels.contiguous().to(torch.int64)
    loss_row = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty_like(loss_row)
    stats = torch.empty(2, dtype=torch.float32, device=logits.device)
    _lib.call("dtd_xent_fwd", _lib.dt(logits), logits.data_ptr(), labels.data_ptr(), loss_row.data_ptr(),
              lse.data_ptr(), stats.data_ptr(), rows, V, ignore_index, _lib.stream())
    return stats[0], lse, stats


def xent_fwd_train(logits, labels, ignore_index: int = IGNORE_INDEX):
    """Training forward of the mean cross-entropy in one pass over the logits: returns
    (loss, lse, stats, dlogits, dbias) with dlogits / dbias (fp32 column sums of dlogits) for a
    loss gradient of 1 -- ``xent_grad_scale`` applies the actual one in the backward -- or None
    when the fused kernel does not cover the case (CPU, not bf16, V % 4 != 0, V > 32768)."""
    V = logits.shape[-1]
    rows = logits.numel() // V
    if (not _on_gpu(logits) or logits.dtype != torch.bfloat16 or not logits.is_contiguous() or rows <= 0
            or logits.data_ptr() % 8 != 0 or not _lib.has("dtd_xent_fwd_train")
            or not _lib.lib().dtd_xent_bwd_colsum_supported(V)):
        return None
    labels = labels.reshape(-1).contiguous().to(torch.int64)
    loss_row = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty_like(loss_row)
    stats = torch.empty(2, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits)
    n = _lib.lib().dtd_xent_bwd_colsum_parts(rows)
    part = torch.empty((n, V), dtype=torch.float32, device=logits.device)
    _lib.call("dtd_xent_fwd_train", logits.data_ptr(), labels.data_ptr(), loss_row.data_ptr(), lse.data_ptr(),
              stats.data_ptr(), d.data_ptr(), part.data_ptr(), rows, V, ignore_index, _lib.stream())
    dbias = torch.empty(V, dtype=torch.float32, device=logits.device)
    _finalize(part, n, V, dbias, False, defer=False)   # a forward result, read by the backward
    return stats[0], lse, stats, d, dbias


def xent_grad_scale_(d: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """d *= grad_out in place unless grad_out == 1 (checked on the device: no host sync)."""
    g = grad_out.reshape(1).to(torch.float32).contiguous()
    _lib.call("dtd_xent_grad_scale", d.data_ptr(), d.numel(), g.data_ptr(), _lib.stream())
    return d


def xent_bwd(logits, labels, lse, stats, grad_out, ignore_index: int = IGNORE_INDEX, dbias=None):
    """dlogits of the mean cross-entropy.  ``dbias`` = (dst, acc): also the column sums of dlogits
    (the bias gradient of the Linear that produced the logits) -- on the kernel path from the same
    pass (``dtd_xent_bwd_colsum``: no re-read of dlogits) when V % 4 == 0 and V <= 32768."""
    V = logits.shape[-1]
    rows = logits.numel() // V
    labels = labels.reshape(-1)
    if not _on_gpu(logits):
        z = logits.float().view(rows, V)
        p = torch.exp(z - lse[:, None])
        valid = labels != ignore_index
        p[torch.arange(rows), labels.clamp_min(0)] -= 1.0
        p = p * valid[:, None].float() * (grad_out.float() / stats[1])
        d = p.to(logits.dtype).view_as(logits)
        if dbias is not None:
            bias_grad(d, *dbias)
        return d
    if (dbias is not None and logits.dtype == torch.bfloat16 and logits.is_contiguous() and rows > 0
            and logits.data_ptr() % 8 == 0 and _lib.has("dtd_xent_bwd_colsum")
            and _lib.lib().dtd_xent_bwd_colsum_supported(V)):
        d = torch.empty_like(logits)
        n = _lib.lib().dtd_xent_bwd_colsum_parts(rows)
        part = torch.empty((n, V), dtype=torch.float32, device=logits.device)
        gout = grad_out.reshape(1).to(torch.float32).contiguous()
        _lib.call("dtd_xent_bwd_colsum", logits.data_ptr(), labels.contiguous().to(torch.int64).data_ptr(),
                  lse.data_ptr(), stats.data_ptr(), gout.data_ptr(), d.data_ptr(), part.data_ptr(), rows, V,
                  ignore_index, _lib.stream())
        _finalize(part, n, V, dbias, dbias[1] if isinstance(dbias, tuple) else False)
        return d
    phase = logits.data_ptr() % 16   # the kernel needs dlogits in the same 16-byte phase
    if phase:
        es = logits.element_size()
        buf = torch.empty(logits.numel() + 16 // es, dtype=logits.dtype, device=logits.device)
        d = buf[phase // es:phase // es + logits.numel()].view_as(logits)
    else:
        d = torch.empty_like(logits)
    gout = grad_out.reshape(1).to(torch.float32).contiguous()
    _lib.call("dtd_xent_bwd", _lib.dt(logits), logits.data_ptr(), labels.contiguous().to(torch.int64).data_ptr(),
              lse.data_ptr(), stats.data_ptr(), gout.data_ptr(), d.data_ptr(), rows, V, ignore_index,
              _lib.stream())
    if dbias is not None:
        bias_grad(d, *dbias)
    return d


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        loss, lse, stats = xent_fwd(logits, labels, ignore_index)
        ctx.save_for_backward(logits, labels, lse, stats)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, gloss):
        logits, labels, lse, stats = ctx.saved_tensors
        return xent_bwd(logits, labels, lse, stats, gloss, ctx.ignore_index), None, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = IGNORE_INDEX) -> torch.Tensor:
    """Mean softmax cross-entropy over rows of ``logits`` [..., V] straight from the logits' own
    dtype (bf16: no fp32 up-cast copy of the logits; the kernel accumulates in fp32) -- the
    drop-in for ``nn.CrossEntropyLoss()(logits.view(-1, V).float(), labels.view(-1))`` of
    /root/reference/model_parallel_training.py:51,73."""
    return _CrossEntropyFn.apply(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index)


class CrossEntropyLoss(torch.nn.Module):
    def __init__(self, ignore_index: int = IGNORE_INDEX):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, logits, labels):
        return cross_entropy(logits, labels, self.ignore_index)


# --------------------------------------------------------------------------------------
# LM head + cross-entropy without the logits (ops/csrc/head_xent.hip)
# --------------------------------------------------------------------------------------
HEAD_XENT_TILE = 128                 # column tile of the kernels: chunk widths are multiples of it
HEAD_XENT_MAX_BLOCK = 1 << 30        # rows x chunk width of one block (dtd_head_dlogits_max_elems)


def _row_major(t: torch.Tensor) -> bool:
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]


def head_xent_supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    """True when the gfx950 kernels take this head: bf16 row-major operands on the GPU with
    16-byte aligned rows and a hidden size the kernels cover (``dtd_head_xent_supported``)."""
    if not (_on_gpu(x) and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.device == x.device):
        return False
    if not (_row_major(x) and _row_major(w) and x.shape[1] == w.shape[1]):
        return False
    if any(t.data_ptr() % 16 or t.stride(0) % 8 for t in (x, w)):
        return False
    return bool(_lib.lib().dtd_head_xent_supported(x.shape[0], w.shape[0], x.shape[1]))


def head_xent_ranges(T: int, V: int) -> int:
    """Vocabulary ranges R of the forward kernel: its partials are ``part [T, R, 2]`` fp32."""
    return int(_lib.lib().dtd_head_lse_ranges(T, V))


def _head_cols(V: int, step: int):
    return [(v0, min(V, v0 + step)) for v0 in range(0, V, step)]


def head_xent_fwd(x: torch.Tensor, w: torch.Tensor, labels: torch.Tensor, ignore_index: int = IGNORE_INDEX,
                  part: torch.Tensor | None = None):
    """Mean cross-entropy of ``x [T, h] @ w [V, h]^T`` against ``labels [T]`` without the logits:
    returns (loss, lse [T], stats [2] = (mean, count)) as ``xent_fwd`` does.  bf16 on the GPU runs
    ``dtd_head_lse`` (``part``: optional caller-owned [T, R, 2] fp32 partials); anything else runs
    the same math in fp32 PyTorch over vocabulary chunks, so it never holds [T, V] either."""
    T, V = x.shape[0], w.shape[0]
    labels = labels.reshape(-1)
    if not head_xent_supported(x, w):
        valid = labels != ignore_index
        yl = labels.clamp_min(0)
        xf = x.float()
        m = torch.full((T,), float("-inf"), dtype=torch.float32, device=x.device)
        s = torch.zeros(T, dtype=torch.float32, device=x.device)
        tgt = torch.zeros(T, dtype=torch.float32, device=x.device)
        for v0, v1 in _head_cols(V, 8192):
            z = xf @ w[v0:v1].float().t()
            inside = (yl >= v0) & (yl < v1)
            tgt = torch.where(inside, z.gather(1, (yl - v0).clamp(0, v1 - v0 - 1)[:, None])[:, 0], tgt)
            mn = torch.maximum(m, z.max(1).values)
            s = s * torch.exp(m - mn) + torch.exp(z - mn[:, None]).sum(1)
            m = mn
        lse = m + torch.log(s)
        loss_row = torch.where(valid, lse - tgt, torch.zeros_like(lse))
        cnt = valid.sum().float()
        mean = loss_row.sum() / cnt
        return mean, lse, torch.stack([mean, cnt])
    labels = labels.contiguous().to(torch.int64)
    dev = x.device
    R = head_xent_ranges(T, V)
    if part is None:
        part = torch.empty((T, R, 2), dtype=torch.float32, device=dev)
    assert part.shape == (T, R, 2) and part.is_contiguous() and part.dtype == torch.float32
    zlab = torch.empty(T, dtype=torch.float32, device=dev)
    loss_row = torch.empty_like(zlab)
    lse = torch.empty_like(zlab)
    stats = torch.empty(2, dtype=torch.float32, device=dev)
    _lib.call("dtd_head_lse", x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), labels.data_ptr(),
              part.data_ptr(), zlab.data_ptr(), lse.data_ptr(), loss_row.data_ptr(), stats.data_ptr(), T, V,
              x.shape[1], ignore_index, _lib.stream())
    return stats[0], lse, stats


def head_xent_dlogits(x: torch.Tensor, w: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor,
                      stats: torch.Tensor, grad_out: torch.Tensor, v0: int, v1: int,
                      out: torch.Tensor | None = None, ignore_index: int = IGNORE_INDEX) -> torch.Tensor:
    """Columns [v0, v1) of dlogits = (softmax - onehot) * valid * grad_out / count, recomputed from
    x and w with the forward's ``lse``; [T, v1 - v0] in x's dtype.  ``out``: a row-major buffer with
    at least T rows and v1 - v0 columns (the chunk buffer a caller reuses); the result is its
    leading view.  grad_out and count are read on the device."""
    T = x.shape[0]
    n = v1 - v0
    labels = labels.reshape(-1)
    if out is None:
        out = torch.empty((T, n), dtype=x.dtype, device=x.device)
    d = out[:T, :n]
    if (head_xent_supported(x, w) and out.dtype == x.dtype and _row_major(out)
            and T * out.stride(0) <= HEAD_XENT_MAX_BLOCK and -(-n // HEAD_XENT_TILE) <= 65535):
        gout = grad_out.reshape(1).to(torch.float32).contiguous()
        _lib.call("dtd_head_dlogits", x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0),
                  labels.contiguous().to(torch.int64).data_ptr(), lse.data_ptr(), stats.data_ptr(), gout.data_ptr(),
                  d.data_ptr(), out.stride(0), T, w.shape[0], x.shape[1], v0, v1, ignore_index, _lib.stream())
        return d
    valid = labels != ignore_index
    p = torch.exp(x.float() @ w[v0:v1].float().t() - lse[:, None])
    inside = valid & (labels >= v0) & (labels < v1)
    p[torch.arange(T, device=x.device), (labels - v0).clamp(0, n - 1)] -= inside.float()
    p = p * (valid.float() * (grad_out.float() / stats[1]))[:, None]
    d.copy_(torch.where(valid[:, None], p, torch.zeros_like(p)))   # lse is 0 on unlabelled rows: exp may overflow
    return d


def head_xent_plan(T: int, V: int, h: int, chunks: int):
    """Blocks (r0, r1, v0, v1) of the chunked head backward, covering [0, T) x [0, V) exactly once.
    Column chunks are ``ceil(V / chunks)`` rounded up to the kernels' 128-column tile (the last one
    takes the rest); rows are split (on tile boundaries) only when rows x chunk width would pass
    ``HEAD_XENT_MAX_BLOCK``, the 32-bit addressing limit of the chunk buffer.  Row blocks are the
    outer loop: one fp32 input-gradient accumulator per row block, one reused chunk buffer."""
    if T < 1 or V < 1 or chunks < 1:
        raise ValueError("head_xent_plan: T, V and chunks must be positive")
    width = -(-(-(-V // chunks)) // HEAD_XENT_TILE) * HEAD_XENT_TILE
    rows = T
    if T * width > HEAD_XENT_MAX_BLOCK:
        rows = max(HEAD_XENT_TILE, HEAD_XENT_MAX_BLOCK // width // HEAD_XENT_TILE * HEAD_XENT_TILE)
        nrb = -(-T // rows)
        rows = -(-(-(-T // nrb)) // HEAD_XENT_TILE) * HEAD_XENT_TILE   # even row blocks
    return [(r0, min(T, r0 + rows), v0, v1) for r0 in range(0, T, rows) for v0, v1 in _head_cols(V, width)]


# --------------------------------------------------------------------------------------
# embeddings
# --------------------------------------------------------------------------------------
def embed_fwd(ids: torch.Tensor, word: torch.Tensor, pos: torch.Tensor | None, type_: torch.Tensor | None,
              seq: int, pos_offset: int = 0, type_ids: torch.Tensor | None = None,
              position_ids: torch.Tensor | None = None) -> torch.Tensor:
    """``position_ids``: optional integer positions, one per id (sequence packing: they restart at
    every document); row r then takes position-table row ``position_ids[r] + pos_offset`` instead
    of ``r % seq + pos_offset``.  The kernel clamps that row index into the table."""
    rows = ids.numel()
    h = word.shape[1]
    if position_ids is not None and (pos is None or position_ids.numel() != rows):
        raise ValueError("position_ids needs a position table and one position per id")
    if not _on_gpu(word):
        flat = ids.reshape(-1)
        out = word[flat].float()
        if pos is not None:
            if position_ids is not None:
                pidx = (position_ids.reshape(-1).to(torch.int64) + pos_offset).clamp(0, pos.shape[0] - 1)
            else:
                pidx = torch.arange(rows, device=ids.device) % seq + pos_offset
            out = out + pos[pidx].float()
        if type_ is not None:
            tid = type_ids.reshape(-1) if type_ids is not None else torch.zeros_like(flat)
            out = out + type_[tid].float()
        return out.to(word.dtype)
    out = torch.empty((rows, h), dtype=word.dtype, device=word.device)
    ids_c = ids.reshape(-1).contiguous().to(torch.int64)
    tids = type_ids.reshape(-1).contiguous().to(torch.int64) if type_ids is not None else None
    if position_ids is not None:
        if not _lib.has("dtd_embed_fwd_pos"):
            raise _lib.KernelError("the kernel library has no position-id embedding entry point (stale build)")
        pids = position_ids.reshape(-1).contiguous().to(device=word.device, dtype=torch.int64)
        _lib.call("dtd_embed_fwd_pos", _lib.dt(word), ids_c.data_ptr(), _lib.ptr(tids), pids.data_ptr(),
                  word.data_ptr(), pos.data_ptr(), _lib.ptr(type_), out.data_ptr(), rows, h, pos_offset,
                  pos.shape[0], _lib.stream())
        return out
    _lib.call("dtd_embed_fwd", _lib.dt(word), ids_c.data_ptr(), _lib.ptr(tids), word.data_ptr(), _lib.ptr(pos),
              _lib.ptr(type_), out.data_ptr(), rows, h, seq, pos_offset, _lib.stream())
    return out


def embed_ln_fwd(ids, word, pos, type_, seq: int, pos_offset: int, gamma, beta, eps: float, p: float,
                 rng: RngState, sid: int, type_ids=None, position_ids=None):
    """Embedding gather-sum + LayerNorm + dropout in one kernel: returns (out, z, mean, rstd), the
    same values as ``embed_fwd`` -> ``ln_fwd(None, z, ...)`` -> ``dropout`` (z = the LN input the
    backward needs), or None when the fused kernel does not cover the case (CPU, fp32, h other
    than 768 / 1024, or ``position_ids`` given -- the fused kernel derives positions from the row
    index only): the caller then runs the three passes."""
    h = word.shape[1]
    if (position_ids is not None or not _on_gpu(word) or word.dtype != torch.bfloat16 or h not in (768, 1024) or gamma is None
            or not _lib.has("dtd_embed_ln_fwd")
            or any(t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous())
                   for t in (word, pos, type_, gamma, beta))):
        return None
    rows = ids.numel()
    z = torch.empty((rows, h), dtype=word.dtype, device=word.device)
    out = torch.empty_like(z)
    mean = torch.empty(rows, dtype=torch.float32, device=word.device)
    rstd = torch.empty_like(mean)
    ids_c = ids.reshape(-1).contiguous().to(torch.int64)
    tids = type_ids.reshape(-1).contiguous().to(torch.int64) if type_ids is not None else None
    _lib.call("dtd_embed_ln_fwd", ids_c.data_ptr(), _lib.ptr(tids), word.data_ptr(), _lib.ptr(pos), _lib.ptr(type_),
              gamma.data_ptr(), beta.data_ptr(), z.data_ptr(), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              rows, h, seq, pos_offset, float(eps), float(p), rng.state.data_ptr(), sid,
              _lib.stream())
    return out, z, mean, rstd


def scatter_rows_supported(g: torch.Tensor) -> bool:
    return (g.is_cuda and g.dtype == torch.bfloat16 and g.dim() == 2 and g.is_contiguous() and g.shape[1] % 8 == 0
            and g.data_ptr() % 16 == 0 and _lib.has("dtd_scatter_rows"))


def scatter_rows(g: torch.Tensor, idx: torch.Tensor, count: torch.Tensor | None, cap: int, rows: int) -> torch.Tensor:
    """[rows, h] with row idx[p] = g[p] for p < n and zeros elsewhere, n = min(count, cap) (count: a
    device scalar, None -> cap); idx[0:n) ascending and unique (the backward of a row gather)."""
    out = torch.empty((rows, g.shape[1]), dtype=g.dtype, device=g.device)
    assert idx.dtype == torch.int64 and idx.is_contiguous() and cap <= idx.numel() and cap <= g.shape[0]
    _lib.call("dtd_scatter_rows", g.data_ptr(), idx.data_ptr(), _lib.ptr(count), int(cap), out.data_ptr(), rows,
              g.shape[1], _lib.stream())
    return out


def embed_word_bwd(ids: torch.Tensor, dz: torch.Tensor, grad: torch.Tensor, acc: bool, padding_idx: int = -1):
    flat = ids.reshape(-1)
    h = grad.shape[1]
    dz = dz.reshape(-1, h)
    if not _on_gpu(grad):
        g = torch.zeros(grad.shape, dtype=torch.float32, device=grad.device)
        g.index_add_(0, flat, dz.float())
        if padding_idx >= 0:
            g[padding_idx] = 0
        if acc:
            grad.add_(g.to(grad.dtype))
        else:
            grad.copy_(g)
        return
    if not acc:
        grad.zero_()
    sorted_ids, perm = torch.sort(flat.to(torch.int64), stable=True)
    lo = torch.searchsorted(sorted_ids, sorted_ids, right=False)
    hi = torch.searchsorted(sorted_ids, sorted_ids, right=True)
    dz = dz.contiguous()
    scratch = torch.empty((flat.numel(), h), dtype=torch.float32, device=dz.device)
    _lib.call("dtd_embed_word_bwd_chunked", _lib.dt(dz), _lib.dt(grad), sorted_ids.data_ptr(), perm.data_ptr(),
              lo.data_ptr(), hi.data_ptr(), scratch.data_ptr(), dz.data_ptr(), grad.data_ptr(), flat.numel(), h, 1,
              padding_idx, _lib.stream())


def embed_pos_bwd(dz: torch.Tensor, grad: torch.Tensor, batch: int, seq: int, pos_offset: int, acc: bool,
                  position_ids: torch.Tensor | None = None):
    """``position_ids`` (sequence packing): the positions repeat inside a row, so the gradient is a
    segment sum with duplicates -- the sorted, atomic-free path of the word table, keyed by the
    position-table row (clamped like the forward's)."""
    h = grad.shape[1]
    if position_ids is not None:
        rows = (position_ids.reshape(-1).to(torch.int64) + pos_offset).clamp(0, grad.shape[0] - 1)
        return embed_word_bwd(rows, dz, grad, acc)
    if not _on_gpu(grad):
        s = dz.reshape(batch, seq, h).float().sum(0)
        if not acc:
            grad.zero_()
        grad[pos_offset:pos_offset + seq].add_(s.to(grad.dtype))
        return
    if not acc:
        grad.zero_()
    dz = dz.contiguous()
    _lib.call("dtd_embed_pos_bwd", _lib.dt(dz), _lib.dt(grad), dz.data_ptr(), grad.data_ptr(), batch, seq, h,
              pos_offset, 1, _lib.stream())


# --------------------------------------------------------------------------------------
# flat-buffer utilities
# --------------------------------------------------------------------------------------
def scale_cast_(src: torch.Tensor, dst: torch.Tensor, scale: float = 1.0, dscale: torch.Tensor | None = None):
    """dst = src * scale * (dscale[0] if given), with dtype conversion (flat buffers)."""
    if not _on_gpu(src):
        v = src.float() * scale
        if dscale is not None:
            v = v * dscale[0]
        dst.copy_(v)
        return dst
    _lib.call("dtd_scale_cast", src.data_ptr(), _lib.dt(src), dst.data_ptr(), _lib.dt(dst), src.numel(),
              float(scale), _lib.ptr(dscale), _lib.stream())
    return dst


def sq_norm(x: torch.Tensor) -> torch.Tensor:
    """Sum of squares of a flat tensor as a 0-dim fp32 device tensor (no host sync)."""
    if not _on_gpu(x):
        return x.float().pow(2).sum()
    n = _lib.lib().dtd_sqnorm_num_partials(x.numel())
    part = torch.empty(n, dtype=torch.float32, device=x.device)
    _lib.call("dtd_sqnorm_partials", x.data_ptr(), _lib.dt(x), x.numel(), part.data_ptr(), _lib.stream())
    return part.sum()


# --------------------------------------------------------------------------------------
# row softmax (instrumented block)
# --------------------------------------------------------------------------------------
def softmax_fwd(x: torch.Tensor) -> torch.Tensor:
    if not _on_gpu(x) or x.dtype not in (torch.bfloat16, torch.float32):
        return torch.softmax(x.float(), dim=-1).to(x.dtype)
    x = x.contiguous()
    y = torch.empty_like(x)
    n = x.shape[-1]
    _lib.call("dtd_softmax_fwd", _lib.dt(x), x.data_ptr(), y.data_ptr(), x.numel() // n, n, _lib.stream())
    return y


def softmax_bwd(y: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    if not _on_gpu(y) or y.dtype not in (torch.bfloat16, torch.float32):
        yf, df = y.float(), dy.float()
        return (yf * (df - (yf * df).sum(-1, keepdim=True))).to(y.dtype)
    dy = dy.contiguous().to(y.dtype)
    dx = torch.empty_like(y)
    n = y.shape[-1]
    _lib.call("dtd_softmax_bwd", _lib.dt(y), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.numel() // n, n,
              _lib.stream())
    return dx


class _SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = softmax_fwd(x)
        ctx.save_for_backward(y)      # like ATen's softmax: the output is the saved activation
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return softmax_bwd(y, dy)


class Softmax(torch.nn.Module):
    """Drop-in ``nn.Softmax(dim=-1)`` backed by the HIP row-softmax kernels on the GPU."""

    def __init__(self, dim: int = -1):
        super().__init__()
        if dim not in (-1,):
            raise ValueError("row softmax over the last dim only")
        self.dim = dim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _SoftmaxFn.apply(x)
