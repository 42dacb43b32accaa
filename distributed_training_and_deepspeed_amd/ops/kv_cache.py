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
"""
from __future__ import annotations

import torch

from ..memory.estimate import kv_cache_bytes
from . import attention as A


class KVCache:
    def __init__(self, k, v, kv_len, kv_next, kv_start, overflow, workspace, splits):
        self.k, self.v = k, v                      # [L, B, Hkv, Smax, D]
        self.kv_len, self.kv_next, self.kv_start, self.overflow = kv_len, kv_next, kv_start, overflow
        self.filled = 0                            # host mirror of kv_len (every sequence advances alike)
        self.workspace, self.splits = workspace, splits
        self.num_layers, self.batch, self.kv_heads, self.max_len, self.head_dim = k.shape

    @classmethod
    def allocate(cls, cfg, batch: int, max_len: int, device, dtype) -> "KVCache":
        """The cache of ``cfg`` for ``batch`` sequences of up to ``max_len`` positions (prompt and
        continuation), empty.  ``max_len`` beyond ``cfg.max_positions`` is a ``ValueError``: the rotary
        table ends there."""
        if batch <= 0 or max_len <= 0:
            raise ValueError(f"KVCache: batch = {batch} and max_len = {max_len} must be positive")
        if cfg.rope_theta > 0 and max_len > cfg.max_positions:
            raise ValueError(f"KVCache: max_len = {max_len} exceeds max_positions = {cfg.max_positions} (the rotary table)")
        L, Hkv, D = cfg.num_layers, cfg.kv_heads, cfg.head_dim
        k = torch.zeros((L, batch, Hkv, max_len, D), dtype=dtype, device=device)
        v = torch.zeros_like(k)
        assert (k.numel() + v.numel()) * k.element_size() == kv_cache_bytes(cfg, batch, max_len, dtype)
        splits = A.decode_splits(batch, Hkv, max_len)
        ws = torch.empty(A.decode_workspace_floats(batch, cfg.num_heads, D, splits), dtype=torch.float32, device=device)
        ints = torch.zeros((4, batch), dtype=torch.int32, device=device)
        ints[1].fill_(1)
        return cls(k, v, ints[0], ints[1], ints[2], ints[3, :1], ws, splits)

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

    def nbytes(self) -> int:
        return (self.k.numel() + self.v.numel()) * self.k.element_size()
