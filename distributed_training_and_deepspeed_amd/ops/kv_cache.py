"""KV cache of the Llama family's incremental decoding.

Per layer one K and one V tensor ``[B, Hkv, Smax, D]`` in the model's dtype: the keys of one (sequence,
key/value head) are one contiguous stream, which is what the decode kernel reads
(ops/csrc/attention_decode.hip).  The cache is linear -- a sliding window is a bound inside the kernel,
not a ring buffer.  Its position lives in device memory and is shared by all layers:

* ``kv_len``   int32 [B]: slots written;
* ``kv_next``  int32 [B]: ``kv_len + 1``, what a decode step's attention takes as its length (the new token
  counted), kept in step with ``kv_len`` so that no layer has to form it;
* ``kv_start`` int32 [B]: first valid slot -- 0 unless the prompt was left-padded;
* ``overflow`` int32 [1]: set by an append that did not fit (it writes nothing out of bounds).

Nothing about the position is read back to the host during a step, and everything a step needs -- the
decode kernel's split workspace included -- is allocated here, up front, so a captured step allocates
nothing.  ``functional.rope_append_`` writes a layer's new rows at ``kv_len`` without moving it; the caller
advances it once per step, after the last layer (``advance``: an in-place device add).

FP8 cache (``kv_dtype="fp8"``, opt-in): K and V hold one-byte OCP ``e4m3fn`` codes, same shape, and
``k_scale`` / ``v_scale`` fp32 ``[L, B, Hkv, Smax]`` hold one scale per row -- a row being the D elements of one
(layer, sequence, key/value head, slot).  The law, ``quantize_kv_ref``: ``amax = max |x|`` over the row in
fp32, x the row as the bf16 cache would hold it (the rotated k as rounded to the model's dtype; v);
``scale = amax / 448`` (1 when amax is 0); ``code = e4m3fn(x / scale)``, both IEEE fp32 divisions, the conversion
round-to-nearest-even; the dequantised value is ``float(code) * scale``.  The quantising append kernel writes the
same codes and scales bit for bit.  Half the bytes of a bf16 cache plus 4 / D of them again for the scales.
"""
from __future__ import annotations

import torch

from ..memory.estimate import kv_cache_bytes
from . import attention as A


FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0          # the largest e4m3fn value


def quantize_kv_ref(x: torch.Tensor):
    """The FP8 cache's quantisation law (module docstring) in plain PyTorch: ``x [..., D]`` -> (codes
    ``float8_e4m3fn [..., D]``, scale fp32 ``[...]``), one scale per row.  The divisor is a tensor, so both
    divisions are element-wise IEEE divisions on every backend (none becomes a multiply by a reciprocal)."""
    xf = x.to(torch.float32)
    amax = xf.abs().amax(-1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, FP8_MAX))
    return (xf / scale.unsqueeze(-1)).to(FP8), scale


def dequantize_kv(code: torch.Tensor, scale: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``float(code) * scale`` per row, in ``dtype`` (fp32 or fp64: both hold a code exactly)."""
    return code.to(dtype) * scale.to(dtype).unsqueeze(-1)


def _kv_dtype(kv_dtype, dtype):
    """None (the model's dtype) or ``FP8`` of ``KVCache.allocate``'s ``kv_dtype``."""
    if kv_dtype is None or kv_dtype == dtype:
        return None
    if kv_dtype == FP8 or kv_dtype == "fp8":
        return FP8
    raise ValueError(f"kv_dtype must be None, the model's dtype ({dtype}), torch.float8_e4m3fn or 'fp8', got {kv_dtype!r}")


class KVCache:
    def __init__(self, k, v, kv_len, kv_next, kv_start, overflow, workspace, splits, k_scale=None, v_scale=None):
        self.k, self.v = k, v                      # [L, B, Hkv, Smax, D]
        self.k_scale, self.v_scale = k_scale, v_scale      # FP8 cache: fp32 [L, B, Hkv, Smax]; else None
        self.kv_len, self.kv_next, self.kv_start, self.overflow = kv_len, kv_next, kv_start, overflow
        self.filled = 0                            # host mirror of kv_len (every sequence advances alike)
        self.workspace, self.splits = workspace, splits
        self.num_layers, self.batch, self.kv_heads, self.max_len, self.head_dim = k.shape

    @classmethod
    def allocate(cls, cfg, batch: int, max_len: int, device, dtype, kv_dtype=None) -> "KVCache":
        """The cache of ``cfg`` for ``batch`` sequences of up to ``max_len`` positions (prompt and
        continuation), empty.  ``max_len`` beyond ``cfg.max_positions`` is a ``ValueError``: the rotary
        table ends there.  ``kv_dtype``: None or ``dtype`` -- K / V in the model's dtype; ``torch.float8_e4m3fn``
        or ``"fp8"`` -- the FP8 cache (module docstring); anything else is a ``ValueError``."""
        fp8 = _kv_dtype(kv_dtype, dtype) is not None
        if batch <= 0 or max_len <= 0:
            raise ValueError(f"KVCache: batch = {batch} and max_len = {max_len} must be positive")
        if cfg.rope_theta > 0 and max_len > cfg.max_positions:
            raise ValueError(f"KVCache: max_len = {max_len} exceeds max_positions = {cfg.max_positions} (the rotary table)")
        L, Hkv, D = cfg.num_layers, cfg.kv_heads, cfg.head_dim
        if fp8:      # (zeros through uint8: code 0 is 0.0)
            k, v = (torch.zeros((L, batch, Hkv, max_len, D), dtype=torch.uint8, device=device).view(FP8) for _ in range(2))
            k_scale, v_scale = (torch.ones((L, batch, Hkv, max_len), dtype=torch.float32, device=device) for _ in range(2))
        else:
            k = torch.zeros((L, batch, Hkv, max_len, D), dtype=dtype, device=device)
            v = torch.zeros_like(k)
            k_scale = v_scale = None
            assert (k.numel() + v.numel()) * k.element_size() == kv_cache_bytes(cfg, batch, max_len, dtype)
        splits = A.decode_splits(batch, Hkv, max_len)
        ws = torch.empty(A.decode_workspace_floats(batch, cfg.num_heads, D, splits), dtype=torch.float32, device=device)
        ints = torch.zeros((4, batch), dtype=torch.int32, device=device)
        ints[1].fill_(1)
        cache = cls(k, v, ints[0], ints[1], ints[2], ints[3, :1], ws, splits, k_scale, v_scale)
        assert cache.nbytes() == kv_cache_bytes(cfg, batch, max_len, dtype, FP8 if fp8 else None)
        return cache

    @property
    def quantized(self) -> bool:
        """Whether this is the FP8 cache (codes and per-row scales)."""
        return self.k_scale is not None

    def reset(self) -> None:
        """Empty the cache (the K / V slots keep their stale content: nothing reads past ``kv_len``)."""
        self.kv_len.zero_()
        self.kv_next.fill_(1)
        self.kv_start.zero_()
        self.overflow.zero_()
        self.filled = 0

    def advance(self, n: int) -> None:
        """``kv_len += n`` on the device, once per step after the last layer's append.  ``filled``, the
        host's count, moves with it (a graph replay of this call moves only the device's: whoever replays
        adds to ``filled`` itself)."""
        self.kv_len.add_(n)
        self.kv_next.add_(n)
        self.filled += n

    def layer(self, i: int):
        """(K, V) ``[B, Hkv, Smax, D]`` of layer i."""
        return self.k[i], self.v[i]

    def layer_scales(self, i: int):
        """(k_scale, v_scale) fp32 ``[B, Hkv, Smax]`` of layer i; (None, None) unless ``quantized``."""
        return (self.k_scale[i], self.v_scale[i]) if self.quantized else (None, None)

    def nbytes(self) -> int:
        """Bytes of K and V, the FP8 cache's scales included (``memory.kv_cache_bytes``)."""
        n = (self.k.numel() + self.v.numel()) * self.k.element_size()
        return n + 4 * (self.k_scale.numel() + self.v_scale.numel()) if self.quantized else n
