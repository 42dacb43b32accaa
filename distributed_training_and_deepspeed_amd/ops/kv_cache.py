"""KV cache of the Llama family's incremental decoding.

Per layer one K and one V tensor ``[B, Hkv, Smax, D]`` in the model's dtype: the keys of one (sequence,
key/value head) are one contiguous stream, which is what the decode kernel reads
(ops/csrc/attention_decode.hip).  By default the cache is linear -- slot = position, a sliding window being
a bound inside the kernel; the ring layout below is opt-in.  Its position lives in device memory and is
shared by all layers:

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

Ring cache (``ring=True``, opt-in, sliding-window models; ops/csrc/attention_ring.hip): K / V are ``[L, B, Hkv, R,
D]`` (scales ``[L, B, Hkv, R]``) and position j of a sequence lives in slot ``j mod R``.  R, ``cache.slots``, is a
multiple of the decode kernel's 64-key tile and at least the window W (default: W rounded up to the tile).  The
counters above stay ABSOLUTE positions -- they are the rotary positions too -- and advance as in the linear cache;
``max_len`` stays the bound on positions.  One law for the kernels and the PyTorch reference:

* append of Sq rows at the positions ``p = kv_len[b] + s``: every q and k row is rotated; row s is stored in slot
  ``p mod R`` only if it is among the last R rows of the call (no slot is written twice); a position outside
  [0, rotary table) stores nothing and raises ``overflow``;
* decode with ``hi = kv_len[b]`` (the new token counted) attends ``lo <= j < hi``, ``lo = max(kv_start[b], 0, hi - W,
  hi - R)``: slot u holds the position ``(hi - 1) - ((hi - 1 - u) mod R)`` and takes part iff that is ``>= lo``.

The cache's bytes, the decode kernel's splits and its workspace follow R, not the number of positions: memory
and the time of a step stop growing once a sequence is longer than the window.  Multi-token steps on a ring
(``attn_extend``, chunked prefill) are not implemented; ``ring_slots`` leaves room for them (R >= W + T - 1).
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
    def __init__(self, k, v, kv_len, kv_next, kv_start, overflow, workspace, splits, k_scale=None, v_scale=None,
                 num_heads=None, ring=False, max_len=None):
        self.k, self.v = k, v                      # [L, B, Hkv, Smax, D] (a ring: [L, B, Hkv, R, D])
        self.k_scale, self.v_scale = k_scale, v_scale      # FP8 cache: fp32 [L, B, Hkv, Smax]; else None
        self.kv_len, self.kv_next, self.kv_start, self.overflow = kv_len, kv_next, kv_start, overflow
        self.filled = 0                            # host mirror of kv_len (every sequence advances alike)
        self.workspace, self.splits = workspace, splits
        self._extend_ws, self._extend_t = None, 0  # the extend kernel's split workspace: see extend_workspace
        self.num_layers, self.batch, self.kv_heads, self.slots, self.head_dim = k.shape
        self.ring = bool(ring)                     # position j in slot j mod slots
        self.max_len = self.slots if max_len is None else max_len     # the bound on positions
        self.num_heads = num_heads or self.kv_heads        # query heads (the extend workspace's size)

    @classmethod
    def allocate(cls, cfg, batch: int, max_len: int, device, dtype, kv_dtype=None, ring: bool = False,
                 ring_slots: int | None = None) -> "KVCache":
        """The cache of ``cfg`` for ``batch`` sequences of up to ``max_len`` positions (prompt and
        continuation), empty.  ``max_len`` beyond ``cfg.max_positions`` is a ``ValueError``: the rotary
        table ends there.  ``kv_dtype``: None or ``dtype`` -- K / V in the model's dtype; ``torch.float8_e4m3fn``
        or ``"fp8"`` -- the FP8 cache (module docstring); anything else is a ``ValueError``.

        ``ring=True`` (a config with ``sliding_window`` = W, else a ``ValueError``): the ring layout of R slots
        (module docstring), R = ``ring_slots`` or W rounded up to the key tile; ``ring_slots`` must be a multiple of
        the tile and at least W (a later chunk of T tokens per step needs W + T - 1).  ``max_len`` still bounds the
        positions; the bytes, the splits and the workspace follow R."""
        fp8 = _kv_dtype(kv_dtype, dtype) is not None
        if batch <= 0 or max_len <= 0:
            raise ValueError(f"KVCache: batch = {batch} and max_len = {max_len} must be positive")
        if cfg.rope_theta > 0 and max_len > cfg.max_positions:
            raise ValueError(f"KVCache: max_len = {max_len} exceeds max_positions = {cfg.max_positions} (the rotary table)")
        L, Hkv, D = cfg.num_layers, cfg.kv_heads, cfg.head_dim
        slots = max_len
        if ring:
            W, T = cfg.sliding_window or 0, A.DECODE_KEY_TILE
            if not W:
                raise ValueError("KVCache: ring=True needs a model with a sliding window")
            slots = -(-W // T) * T if ring_slots is None else int(ring_slots)
            if slots < W or slots % T:
                raise ValueError(f"KVCache: ring_slots = {ring_slots} must be a multiple of {T} and at least the window {W}")
        elif ring_slots is not None:
            raise ValueError("KVCache: ring_slots goes with ring=True")
        if fp8:      # (zeros through uint8: code 0 is 0.0)
            k, v = (torch.zeros((L, batch, Hkv, slots, D), dtype=torch.uint8, device=device).view(FP8) for _ in range(2))
            k_scale, v_scale = (torch.ones((L, batch, Hkv, slots), dtype=torch.float32, device=device) for _ in range(2))
        else:
            k = torch.zeros((L, batch, Hkv, slots, D), dtype=dtype, device=device)
            v = torch.zeros_like(k)
            k_scale = v_scale = None
            assert (k.numel() + v.numel()) * k.element_size() == kv_cache_bytes(cfg, batch, slots, dtype)
        splits = A.decode_splits(batch, Hkv, slots)
        ws = torch.empty(A.decode_workspace_floats(batch, cfg.num_heads, D, splits), dtype=torch.float32, device=device)
        ints = torch.zeros((4, batch), dtype=torch.int32, device=device)
        ints[1].fill_(1)
        cache = cls(k, v, ints[0], ints[1], ints[2], ints[3, :1], ws, splits, k_scale, v_scale, cfg.num_heads, ring, max_len)
        assert cache.nbytes() == kv_cache_bytes(cfg, batch, slots, dtype, FP8 if fp8 else None)
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

    def extend_workspace(self, T: int):
        """(splits, workspace) of ``ops.attention.attn_extend`` for chunks of T tokens per sequence.  The workspace is
        allocated on first use, for the largest T seen, and kept (None while no T seen needs one: a single split
        writes its output itself).  A captured step calls this once before the capture, so the capture allocates
        nothing."""
        if self.ring:
            raise NotImplementedError("multi-token cached attention (attn_extend) on a ring cache is not implemented")
        H = self.num_heads
        splits = A.extend_splits(self.batch, self.kv_heads, self.max_len, T, H // self.kv_heads)
        if T > self._extend_t:
            # the largest need of any chunk length up to T: splits fall as T grows, the rows rise
            need = max(A.extend_workspace_floats(self.batch, t, H, self.head_dim, A.extend_splits(
                self.batch, self.kv_heads, self.max_len, t, H // self.kv_heads)) for t in range(1, T + 1))
            if need and (self._extend_ws is None or self._extend_ws.numel() < need):
                self._extend_ws = torch.empty(need, dtype=torch.float32, device=self.k.device)
            self._extend_t = T
        return splits, self._extend_ws

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
