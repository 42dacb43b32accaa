"""FP8 (OCP e4m3fn) and MXFP4 (OCP MX: e2m1 elements, e8m0 block scales) weight storage for the decode step's
projections (``ops/csrc/gemm_skinny.hip``, ``ops/csrc/gemm_skinny_mx4.hip``).

The FP8 law, per output row ``w[n, :]``:

    amax  = max |w[n, :]|
    scale = the smallest power of two s with amax / s <= 448   (1 for an all-zero row; at least 2^-100)
    code  = e4m3fn(w / scale), round to nearest even
    dequantised = float(code) * scale

``quantize_act_fp8`` applies the same law to the rows of activations ``x[m, :]`` (one scale per token), for the
FP8 x FP8 product of more than 64 rows (``ops/csrc/gemm_fp8.hip``).

It is deliberately not the KV cache's ``amax / 448``.  A code has 4 significant bits and the scale is a power of
two, so the dequantised weight is exactly representable in bf16: a quantised model is an ordinary bf16 model
whose weights lie on that grid, and every path that reads the parameters (prefill, training kernels, the
reference path, checkpoints) computes the same mathematical model as the decode steps that read the codes.
The code is itself floating point, so the power-of-two scale costs no relative precision: ``amax / scale``
lies in (224, 448], and ``|w - deq| <= |w| / 17`` wherever the code is a normal number.

The MX4 law, per row n and block kb of 32 consecutive k (``quantize_weight_mx4``):

    amax  = max |w| over the block
    scale = the smallest power of two s with amax / s <= 6    (2^0 for an all-zero block; at least 2^-100)
    code  = e2m1(w / scale), round to nearest, ties to the even mantissa, never saturating
            grid +-{0, .5, 1, 1.5, 2, 3, 4, 6}; sign bit 3, exponent bits 2:1, mantissa bit 0
    byte  = scale exponent + 127 (e8m0; 255, its NaN, is never written)

Element 2 j sits in the low nibble of byte j of ``codes [N, K / 2]``, element 2 j + 1 in the high nibble (the
OCP / ``float4_e2m1fn_x2`` order); ``scales [N, K / 32]`` holds the bytes.  N K / 2 + N K / 32 bytes: 4.25 bits
per weight.  An e2m1 value times a power of two is exact in bf16, so the rule above holds here too;
``amax / scale`` lies in (3, 6] and ``|w - deq| <= max(|w| / 5, scale / 4)``: the grid's widest relative gap is
2 .. 3 (half of it is a fifth of 2.5), and below 0.5 the spacing is 0.5.
"""
from __future__ import annotations

import torch

E4M3_MAX = 448.0
_MIN_EXP = -100
MX_BLOCK = 32
FORMATS = {"fp8": torch.float8_e4m3fn, "mxfp4": torch.uint8}      # format name -> dtype of the codes
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _quantize_rows_fp8(wf: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The FP8 law on the rows of an fp32 ``[R, K]``: weights (a row per output feature) and activations alike."""
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


def quantize_weight_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``w [N, K]`` -> (codes float8_e4m3fn [N, K], scale fp32 [N]) by the law above."""
    if w.dim() != 2:
        raise ValueError(f"quantize_weight_fp8 takes a [N, K] weight, got {tuple(w.shape)}")
    return _quantize_rows_fp8(w.detach().float())


def quantize_act_fp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``x [M, K]`` -> (codes float8_e4m3fn [M, K], scale fp32 [M]): the weight law applied to the rows of
    activations (bf16 values read as fp32).  ``dequantize_weight`` is its inverse.  Finite inputs are the contract:
    the result for a row that holds a NaN or an inf is unspecified."""
    if x.dim() != 2:
        raise ValueError(f"quantize_act_fp8 takes [M, K] activations, got {tuple(x.shape)}")
    return _quantize_rows_fp8(x.detach().float())


def dequantize_weight(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``float(code) * scale[n]`` in ``dtype``: exact in bf16 for power-of-two scales."""
    return (codes.float() * scale.float()[:, None]).to(dtype)


def quantize_weight_mx4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``w [N, K]`` -> (codes uint8 [N, K / 2], scales uint8 [N, K / 32]) by the MX4 law above; K % 32 == 0."""
    if w.dim() != 2 or w.shape[1] % MX_BLOCK:
        raise ValueError(f"quantize_weight_mx4 takes a [N, K] weight with K % {MX_BLOCK} == 0, got {tuple(w.shape)}")
    N, K = w.shape
    wf = w.detach().float().view(N, K // MX_BLOCK, MX_BLOCK)
    amax = wf.abs().amax(2)
    # amax = m * 2^e with m in [0.5, 1) and 6 = 0.75 * 2^3: amax / 2^k <= 6 from k = e - 3 on when m <= 0.75,
    # from e - 2 on otherwise.  Exact at amax = 6 * 2^k.
    m, e = torch.frexp(amax)
    k = torch.where(m <= 0.75, e - 3, e - 2).clamp_(min=_MIN_EXP)
    k = torch.where(amax == 0, torch.zeros_like(k), k)
    a = torch.ldexp(wf, -k[:, :, None]).abs()
    # round to nearest on the grid: one comparison per midpoint, a tie going to the neighbour with mantissa bit 0
    idx = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    nib = (idx | (torch.signbit(wf).to(torch.uint8) << 3)).view(N, K // 2, 2)
    return nib[..., 0] | (nib[..., 1] << 4), (k + 127).to(torch.uint8)


def dequantize_weight_mx4(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Grid value times ``2^(byte - 127)`` as ``[N, K]`` in ``dtype``: exact in bf16."""
    N = codes.shape[0]
    nib = torch.stack((codes & 15, codes >> 4), -1).view(N, -1, MX_BLOCK).long()
    grid = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=codes.device)
    return torch.ldexp(grid[nib], scales.to(torch.int32)[:, :, None] - 127).view(N, -1).to(dtype)


_LAWS = {"fp8": (quantize_weight_fp8, dequantize_weight), "mxfp4": (quantize_weight_mx4, dequantize_weight_mx4)}


# Quantised weight storage of some parameters of a module: ``<name>_codes`` / ``<name>_scale`` as
# non-persistent buffers (not in the state dict), the parameter overwritten in place with the dequantised
# values, and its ``_version`` remembered in ``versions`` -- an in-place update afterwards (an optimizer step,
# a loaded checkpoint) leaves the codes stale, which ``check_quantized`` turns into an error.
@torch.no_grad()
def quantize_params_(mod: torch.nn.Module, names, versions: dict, fmt: str = "fp8") -> None:
    quantize, dequantize = _LAWS[fmt]
    for name in names:
        p = getattr(mod, name)
        codes, scale = quantize(p)
        p.copy_(dequantize(codes, scale, p.dtype))
        mod.register_buffer(name + "_codes", codes, persistent=False)
        mod.register_buffer(name + "_scale", scale, persistent=False)
        versions[name] = p._version


def clear_quantized_(mod: torch.nn.Module, versions: dict) -> None:
    for name in list(versions):
        delattr(mod, name + "_codes")
        delattr(mod, name + "_scale")
    versions.clear()


def check_quantized(mod: torch.nn.Module, versions: dict, fmt: str = "fp8") -> None:
    for name, v in versions.items():
        codes = getattr(mod, name + "_codes")
        if getattr(mod, name)._version != v or codes.dtype != FORMATS[fmt]:
            raise RuntimeError(f"{type(mod).__name__}.{name} changed after quantize_weights_: its {fmt} codes are stale "
                               f"(call quantize_weights_ again, or clear_quantized_weights)")
