"""FP8 (OCP e4m3fn) weight storage for the decode step's projections (``ops/csrc/gemm_skinny.hip``).

The law, per output row ``w[n, :]``:

    amax  = max |w[n, :]|
    scale = the smallest power of two s with amax / s <= 448   (1 for an all-zero row; at least 2^-100)
    code  = e4m3fn(w / scale), round to nearest even
    dequantised = float(code) * scale

It is deliberately not the KV cache's ``amax / 448``.  A code has 4 significant bits and the scale is a power of
two, so the dequantised weight is exactly representable in bf16: a quantised model is an ordinary bf16 model
whose weights lie on that grid, and every path that reads the parameters (prefill, training kernels, the
reference path, checkpoints) computes the same mathematical model as the decode steps that read the codes.
The code is itself floating point, so the power-of-two scale costs no relative precision: ``amax / scale``
lies in (224, 448], and ``|w - deq| <= |w| / 17`` wherever the code is a normal number.
"""
from __future__ import annotations

import torch

E4M3_MAX = 448.0
_MIN_EXP = -100


def quantize_weight_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``w [N, K]`` -> (codes float8_e4m3fn [N, K], scale fp32 [N]) by the law above."""
    if w.dim() != 2:
        raise ValueError(f"quantize_weight_fp8 takes a [N, K] weight, got {tuple(w.shape)}")
    wf = w.detach().float()
    amax = wf.abs().amax(1)
    # amax = m * 2^e with m in [0.5, 1) and 448 = 0.875 * 2^9: amax / 2^k <= 448 from k = e - 9 on when
    # m <= 0.875, from e - 8 on otherwise.  No division, no logarithm: exact at amax = 448 * 2^k.
    m, e = torch.frexp(amax)
    k = torch.where(m <= 0.875, e - 9, e - 8).clamp_(min=_MIN_EXP)
    k = torch.where(amax == 0, torch.zeros_like(k), k)
    scale = torch.ldexp(torch.ones_like(amax), k)
    # the division by a power of two is exact (up to fp32 underflow, far below the smallest code)
    codes = torch.ldexp(wf, -k[:, None]).to(torch.float8_e4m3fn)
    return codes, scale


def dequantize_weight(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``float(code) * scale[n]`` in ``dtype``: exact in bf16 for power-of-two scales."""
    return (codes.float() * scale.float()[:, None]).to(dtype)


# FP8 weight storage of some parameters of a module: ``<name>_codes`` / ``<name>_scale`` as
# non-persistent buffers (not in the state dict), the parameter overwritten in place with the dequantised
# values, and its ``_version`` remembered in ``versions`` -- an in-place update afterwards (an optimizer step,
# a loaded checkpoint) leaves the codes stale, which ``check_quantized`` turns into an error.
@torch.no_grad()
def quantize_params_(mod: torch.nn.Module, names, versions: dict) -> None:
    for name in names:
        p = getattr(mod, name)
        codes, scale = quantize_weight_fp8(p)
        p.copy_(dequantize_weight(codes, scale, p.dtype))
        mod.register_buffer(name + "_codes", codes, persistent=False)
        mod.register_buffer(name + "_scale", scale, persistent=False)
        versions[name] = p._version


def clear_quantized_(mod: torch.nn.Module, versions: dict) -> None:
    for name in list(versions):
        delattr(mod, name + "_codes")
        delattr(mod, name + "_scale")
    versions.clear()


def check_quantized(mod: torch.nn.Module, versions: dict) -> None:
    for name, v in versions.items():
        codes = getattr(mod, name + "_codes")
        if getattr(mod, name)._version != v or codes.dtype != torch.float8_e4m3fn:
            raise RuntimeError(f"{type(mod).__name__}.{name} changed after quantize_weights_: its FP8 codes are stale "
                               f"(call quantize_weights_ again, or clear_quantized_weights)")
