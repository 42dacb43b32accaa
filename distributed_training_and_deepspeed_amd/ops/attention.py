"""Scaled-dot-product attention core: flash-style HIP kernels (gfx950 MFMA) + math reference.

Layout contract (shared by kernels, reference and models): the fused projection output
``qkv`` is ``[B*S, 3*H*D]`` viewed as ``[B, S, 3, H, D]`` (q, k, v blocks), the context
output ``ctx`` is ``[B*S, H*D]`` and the log-sum-exp ``lse`` is ``[B, H, S]`` fp32 (natural
log of sum(exp(score)), score = q.k * scale + bias).  Supported score modifiers: causal mask,
ALiBi (BLOOM: bias = slope_h * key_position, which equals BLOOM's relative form up to a
per-row constant that softmax cancels) and dropout on the probabilities with the counter RNG
(mask element index = ((b*H + h)*S + i)*S + j, regenerated in backward), and a per-sequence key
range ``key_range`` (int32 ``[B, 2]`` = (lo, hi), the key-padding mask of a left- or right-padded
batch, ``key_range_from_mask``): key j of sequence b takes part iff lo <= j < hi, before and
independently of the causal mask and ALiBi.  Padded *query* rows are computed like any other (they
attend to the valid keys, as in HF models).  A row left without a key -- lo >= hi, or causal with
q < lo -- has ctx = 0, lse = -inf and contributes nothing to any gradient.  Dropout keep bits stay
indexed by the absolute (b, h, q, key), so a range does not change which bits a pair draws.

Sequence packing: ``doc_range`` (``DocRange``, from ``doc_range_from_segment_ids``) gives every
position the half-open span (lo, hi) of its document, int32 ``[B, S, 2]``, (0, 0) for a pad.  Query i
attends key j iff lo_i <= j < hi_i (and j <= i when causal) -- block-diagonal attention over the
documents of a row; the relation is symmetric.  Everything else is as for a key range (which it
excludes: padding is an empty span here): the mask comes before ALiBi, whose bias stays slope *
absolute key position, the keep bits stay absolutely indexed, and a row without a key -- a pad -- has
ctx = 0, lse = -inf, dq = 0 and contributes to no gradient; pad keys get dk = dv = 0.

Grouped-query attention: ``kv_heads = Hkv`` (``H % Hkv == 0``, G = H / Hkv) gives the key/value
projections Hkv heads; query head h reads key/value head h // G (HF's ``repeat_kv`` order).  The
packed projection output is then ``qkv [B*S, (H + 2*Hkv)*D]``: the q block (H*D columns), then k
(Hkv*D), then v (Hkv*D); ``dqkv`` has the same layout, its dK / dV the sums over each group's query
heads (formed in fp32 inside the dK/dV kernel, rounded once).  ``ctx``, ``lse`` and ``delta`` stay
per query head.  The causal mask, ``key_range`` and ``doc_range`` apply as above; dropout and ALiBi
are not supported together with ``Hkv != H`` (``ValueError``).  ``kv_heads`` None or H is the
multi-head layout above, on its own code paths.

Sliding window: ``window = W`` (an integer > 0, ``causal=True`` only) lets query i attend key j iff
i - W < j <= i -- W keys including the query's own, HF Mistral's ``sliding_window``.  It composes by
intersection with ``key_range`` (additionally lo <= j < hi) and ``doc_range`` (additionally j inside
i's document); a row left without a key -- e.g. i >= hi + W - 1 under a right-padded range (0, hi) --
follows the empty-row rule above, and keys no query sees get dk = dv = 0.  Neither dropout nor ALiBi
(``ValueError``).  The bf16 kernels are windowed instantiations of the grouped-query family, which
visit only the O(S W) band of key tiles; the multi-head layout runs through them with one query head
per group (its q | k | v blocks are that layout).  ``window`` None, 0 or >= S is the call without
the argument, on its code paths and bit for bit.

Incremental decoding (``attn_decode``, at the end of this module): one new query per sequence against a
KV cache ``[B, Hkv, Smax, D]`` whose fill level lives in device memory (ops/kv_cache.py).

Reference semantics: HF BertSelfAttention eager path (matmul, softmax, dropout, matmul --
SURVEY.md K2, reference model/transformer.py:80-86); the reference never passes an
attention mask for BERT (data_parallel_training.py:53), so by default (no ``key_range``) padding
is attended to.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import torch

from . import _lib
from .rng import RngState, attn_keep_mask


def alibi_slopes(num_heads: int) -> torch.Tensor:
    """BLOOM/ALiBi head slopes (geometric sequence, with the interleaved extension for
    non-power-of-two head counts)."""
    def pow2(n):
        start = 2 ** (-(2 ** -(math.log2(n) - 3)))
        return [start * (start ** i) for i in range(n)]
    if math.log2(num_heads).is_integer():
        s = pow2(num_heads)
    else:
        c = 2 ** math.floor(math.log2(num_heads))
        s = pow2(c) + pow2(2 * c)[0::2][: num_heads - c]
    return torch.tensor(s, dtype=torch.float32)


def _split(qkv, B, S, H, D):
    x = qkv.view(B, S, 3, H, D)
    return x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)


def _kv_heads(kv_heads, H: int) -> int:
    """Hkv of a call: ``kv_heads`` (None = H), which must divide H."""
    Hkv = H if kv_heads is None else int(kv_heads)
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"kv_heads = {Hkv} must be positive and divide the {H} query heads")
    return Hkv


def _check_gqa(qkv, B, S, H, Hkv, D, p, slopes):
    """The grouped-query layout and what it excludes (module docstring)."""
    if p > 0 or slopes is not None:
        raise ValueError("grouped-query attention (kv_heads != H) supports neither dropout nor ALiBi")
    if qkv.numel() != B * S * (H + 2 * Hkv) * D:
        raise ValueError(f"qkv must be [B*S, (H + 2*Hkv)*D] = [{B * S}, {(H + 2 * Hkv) * D}], got {tuple(qkv.shape)}")


def _split_gqa(qkv, B, S, H, Hkv, D):
    """q [B, H, S, D] and the k, v [B, Hkv, S, D] of a grouped-query qkv."""
    x = qkv.reshape(B, S, H + 2 * Hkv, D)
    return (x[:, :, :H].transpose(1, 2), x[:, :, H:H + Hkv].transpose(1, 2), x[:, :, H + Hkv:].transpose(1, 2))


def _window(window, S: int, causal, p, slopes) -> int:
    """The effective window of a call: 0 = none (None, 0, or >= S, where the band is the whole causal
    triangle); otherwise validated (module docstring)."""
    if window is None:
        return 0
    if isinstance(window, bool) or int(window) != window or window < 0:
        raise ValueError(f"window must be a positive integer (or None / 0 for no window), got {window!r}")
    window = int(window)
    if window == 0:
        return 0
    if not causal:
        raise ValueError("a sliding window needs causal=True (a symmetric local window is not supported)")
    if p > 0 or slopes is not None:
        raise ValueError("a sliding window supports neither dropout nor ALiBi")
    return 0 if window >= S else window


def _cdt(t: torch.Tensor) -> torch.dtype:
    """Compute dtype of the math reference: fp64 for fp64 inputs (kernel tests), else fp32."""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def key_range_from_mask(attention_mask: torch.Tensor, check: bool = False) -> torch.Tensor:
    """(lo, hi) key ranges, int32 ``[B, 2]`` on the mask's device, of a 0/1 ``[B, S]`` attention
    mask: lo = first kept position, hi = last kept position + 1 -- left padding, right padding or
    both; a row of zeros gives (0, 0).  Runs on the device with no host synchronisation, so a
    captured step can call it on its static mask input.

    Only contiguous masks are supported: a mask with holes inside [lo, hi) is treated as if the
    holes were kept.  ``check=True`` synchronises and raises ``ValueError`` for such a mask."""
    if attention_mask.dim() != 2:
        raise ValueError(f"attention_mask must be [B, S], got {tuple(attention_mask.shape)}")
    B, S = attention_mask.shape
    if S == 0:
        return torch.zeros((B, 2), dtype=torch.int32, device=attention_mask.device)
    keep = attention_mask != 0
    idx = torch.arange(S, device=keep.device, dtype=torch.int32)
    hi = torch.where(keep, idx + 1, torch.zeros_like(idx)).amax(1)
    lo = torch.minimum(torch.where(keep, idx, torch.full_like(idx, S)).amin(1), hi)
    if check and bool((keep.sum(1) != hi - lo).any()):
        raise ValueError("attention_mask has holes inside its kept range: only contiguous "
                         "(left- / right-padded) masks map to a key range")
    return torch.stack([lo, hi], 1).contiguous()


class DocRange(NamedTuple):
    """Document spans of a packed batch.  ``ranges``: int32 [B, S, 2], (lo, hi) of each position's
    document, (0, 0) for a pad.  ``blocks``: int32 [B, ceil(S / 128), 2], (min lo, max hi) over each
    128-position block's non-empty rows, (0, 0) for a block without one -- the tile range of the
    workgroup that owns the block.  Both are views of ``flat``, the kernels' one argument."""
    ranges: torch.Tensor
    blocks: torch.Tensor
    flat: torch.Tensor


_DOC_BLOCK = 128     # positions per workgroup of the attention kernels


def _doc_pack(ranges: torch.Tensor) -> DocRange:
    """DocRange of int [B, S, 2] spans: the block bounds are derived on the device, no sync."""
    B, S = ranges.shape[:2]
    nb = (S + _DOC_BLOCK - 1) // _DOC_BLOCK
    r = ranges.to(torch.int32)
    lo, hi = r[..., 0], r[..., 1]
    live = hi > lo
    pad = nb * _DOC_BLOCK - S
    blo = torch.nn.functional.pad(torch.where(live, lo, torch.full_like(lo, S)), (0, pad), value=S)
    bhi = torch.nn.functional.pad(torch.where(live, hi, torch.zeros_like(hi)), (0, pad), value=0)
    bhi = bhi.view(B, nb, _DOC_BLOCK).amax(2) if S else bhi.view(B, nb)
    blo = torch.minimum(blo.view(B, nb, _DOC_BLOCK).amin(2), bhi) if S else blo.view(B, nb)
    flat = torch.cat([r.reshape(-1), torch.stack([blo, bhi], 2).reshape(-1)])
    n = B * S * 2
    return DocRange(flat[:n].view(B, S, 2), flat[n:].view(B, nb, 2), flat)


def doc_range_from_segment_ids(segment_ids: torch.Tensor, check: bool = False) -> DocRange:
    """Document spans (``DocRange``) of integer ``[B, S]`` segment ids: 0 marks padding, each
    document is a contiguous run of one non-zero id, and an id does not come back in a row after a
    different id; pads may sit at the front, at the end or between documents.  Runs on the ids'
    device with no host synchronisation, so a captured step can call it on its static input.

    Ids that break the rule are not detected: every run counts as a document of its own.
    ``check=True`` synchronises and raises ``ValueError`` for an id that reappears in a row."""
    if segment_ids.dim() != 2:
        raise ValueError(f"segment_ids must be [B, S], got {tuple(segment_ids.shape)}")
    if segment_ids.dtype.is_floating_point or segment_ids.dtype == torch.bool:
        raise ValueError(f"segment_ids must be an integer tensor, got {segment_ids.dtype}")
    B, S = segment_ids.shape
    dev = segment_ids.device
    if S == 0:
        return _doc_pack(torch.zeros((B, 0, 2), dtype=torch.int32, device=dev))
    seg = segment_ids
    live = seg != 0
    edge = seg[:, 1:] != seg[:, :-1]
    one = torch.ones((B, 1), dtype=torch.bool, device=dev)
    first = live & torch.cat([one, edge], 1)          # first token of a run
    last = live & torch.cat([edge, one], 1)           # last token of a run
    idx = torch.arange(S, device=dev, dtype=torch.int64).expand(B, S)
    # lo = the latest run start at or before i; hi = the earliest run end at or after i, + 1
    lo = torch.where(first, idx, torch.zeros_like(idx)).cummax(1).values
    hi = torch.where(last, idx + 1, torch.full_like(idx, S)).flip(1).cummin(1).values.flip(1)
    zero = torch.zeros_like(idx)
    if check:
        ids, rows = seg[first], idx.new_tensor(range(B)).view(B, 1).expand(B, S)[first]
        pairs = torch.stack([rows, ids.to(torch.int64)], 1)
        if pairs.shape[0] != torch.unique(pairs, dim=0).shape[0]:
            raise ValueError("segment_ids: an id reappears in a row after a different id or a pad -- "
                             "only contiguous documents map to document spans")
    return _doc_pack(torch.stack([torch.where(live, lo, zero), torch.where(live, hi, zero)], 2))


def doc_position_ids(doc_range: DocRange | torch.Tensor) -> torch.Tensor:
    """Position of every token inside its document, int64 [B, S]: i - lo_i, 0 for a pad."""
    r = doc_range.ranges if isinstance(doc_range, DocRange) else doc_range
    S = r.shape[1]
    i = torch.arange(S, device=r.device, dtype=torch.int64).view(1, S)
    lo, hi = r[..., 0].to(torch.int64), r[..., 1].to(torch.int64)
    return torch.where(hi > lo, i - lo, torch.zeros_like(lo))


def _doc_ranges(doc_range, B, S) -> torch.Tensor:
    r = doc_range.ranges if isinstance(doc_range, DocRange) else doc_range
    if tuple(r.shape) != (B, S, 2):
        raise ValueError(f"doc_range must be [B, S, 2] = [{B}, {S}, 2], got {tuple(r.shape)}")
    return r


def _doc_mask(doc_range, B, S, device):
    """[B, 1, S, S] bool, True where key j lies OUTSIDE query i's document span."""
    r = _doc_ranges(doc_range, B, S).to(device=device, dtype=torch.int64)
    j = torch.arange(S, device=device).view(1, 1, S)
    return ((j < r[:, :, :1]) | (j >= r[:, :, 1:])).view(B, 1, S, S)


def _exclusive(key_range, doc_range):
    if key_range is not None and doc_range is not None:
        raise ValueError("key_range and doc_range are mutually exclusive (padding is an empty span of doc_range)")


def _range_mask(key_range, B, S, device):
    """[B, 1, 1, S] bool, True where the key is OUTSIDE its sequence's range."""
    kr = key_range.to(device=device, dtype=torch.int64).view(B, 2)
    j = torch.arange(S, device=device).view(1, S)
    return ((j < kr[:, :1]) | (j >= kr[:, 1:])).view(B, 1, 1, S)


def _probs(s, lse):
    """exp(s - lse) with the empty-row rule: a row without a key has lse = -inf (and s = -inf
    throughout), where exp(s - lse) would be NaN -- its probabilities are 0."""
    lse = lse[..., None].to(s.dtype)
    return torch.exp(s - lse.masked_fill(lse == float("-inf"), 0.0))


def _scores(q, k, scale, causal, slopes, key_range=None, doc_range=None, window: int = 0):
    _exclusive(key_range, doc_range)
    c = _cdt(q)
    s = torch.matmul(q.to(c), k.to(c).transpose(-1, -2)) * scale
    S = q.shape[2]
    if slopes is not None:
        s = s + slopes.to(s.device).view(1, -1, 1, 1) * torch.arange(S, device=s.device, dtype=s.dtype).view(1, 1, 1, S)
    if causal:
        m = torch.ones(S, S, dtype=torch.bool, device=s.device).triu(1)
        s = s.masked_fill(m, float("-inf"))
    if window:       # the band: key j <= i - window lies behind query i's window
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=s.device).tril(-window), float("-inf"))
    if key_range is not None:
        s = s.masked_fill(_range_mask(key_range, q.shape[0], S, s.device), float("-inf"))
    if doc_range is not None:
        s = s.masked_fill(_doc_mask(doc_range, q.shape[0], S, s.device), float("-inf"))
    return s


def _drop_mask(B, H, S, p, rng, sid, device):
    seed, step = (int(v) for v in rng.state.tolist())
    return attn_keep_mask(B, H, S, p, seed, step, sid, device=device)


def attn_fwd_ref(qkv, B, S, H, D, causal=False, slopes=None, p=0.0, rng: RngState | None = None, sid=0,
                 scale=None, key_range=None, doc_range=None, kv_heads: int | None = None, window: int | None = None):
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    Hkv = _kv_heads(kv_heads, H)
    window = _window(window, S, causal, p, slopes)
    if Hkv != H:     # K / V expanded to the H query heads (repeat_kv order)
        _check_gqa(qkv, B, S, H, Hkv, D, p, slopes)
        q, k, v = _split_gqa(qkv, B, S, H, Hkv, D)
        k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    else:
        q, k, v = _split(qkv, B, S, H, D)
    s = _scores(q, k, scale, causal, slopes, key_range, doc_range, window)
    lse = torch.logsumexp(s, -1)       # -inf for a row without a key
    prob = _probs(s, lse)
    if p > 0:
        prob = prob * _drop_mask(B, H, S, p, rng, sid, qkv.device) / (1.0 - p)
    ctx = torch.matmul(prob, v.to(prob.dtype))  # [B,H,S,D]
    return ctx.transpose(1, 2).reshape(B * S, H * D).to(qkv.dtype), lse


def attn_bwd_ref(dctx, qkv, ctx, lse, B, S, H, D, causal=False, slopes=None, p=0.0, rng=None, sid=0, scale=None,
                 key_range=None, doc_range=None, kv_heads: int | None = None, window: int | None = None):
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    Hkv = _kv_heads(kv_heads, H)
    window = _window(window, S, causal, p, slopes)
    if Hkv != H:
        _check_gqa(qkv, B, S, H, Hkv, D, p, slopes)
        q, k, v = _split_gqa(qkv, B, S, H, Hkv, D)
        k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    else:
        q, k, v = _split(qkv, B, S, H, D)
    s = _scores(q, k, scale, causal, slopes, key_range, doc_range, window)
    prob = _probs(s, lse)
    c = s.dtype
    do = dctx.view(B, S, H, D).transpose(1, 2).to(c)
    o = ctx.view(B, S, H, D).transpose(1, 2).to(c)
    if p > 0:
        keep = _drop_mask(B, H, S, p, rng, sid, qkv.device).to(c) / (1.0 - p)
        pd = prob * keep
    else:
        keep, pd = None, prob
    dv = torch.matmul(pd.transpose(-1, -2), do)
    dpd = torch.matmul(do, v.to(c).transpose(-1, -2))
    dp = dpd * keep if keep is not None else dpd
    delta = (do * o).sum(-1, keepdim=True)
    ds = prob * (dp - delta)
    dq = torch.matmul(ds, k.to(c)) * scale
    dk = torch.matmul(ds.transpose(-1, -2), q.to(c)) * scale
    if Hkv != H:     # dK / dV: the sum over each group's query heads
        dk, dv = (t.reshape(B, Hkv, H // Hkv, S, D).sum(2) for t in (dk, dv))
        dqkv = torch.cat([dq, dk, dv], dim=1)   # [B, H + 2 Hkv, S, D]
        return dqkv.permute(0, 2, 1, 3).reshape(B * S, (H + 2 * Hkv) * D).to(qkv.dtype)
    dqkv = torch.stack([dq, dk, dv], dim=2)  # [B,H,3,S,D]
    return dqkv.permute(0, 3, 2, 1, 4).reshape(B * S, 3 * H * D).to(qkv.dtype)


_WARNED = []


def _warn_once():
    if not _WARNED:
        import warnings
        warnings.warn("HIP flash-attention kernel not built: using the math reference on GPU")
        _WARNED.append(1)


_BWD_FORMS = ("split", "fused", "fused4")


def set_bwd_form(form: str) -> str:
    """'fused': one-kernel backward (one workgroup per (batch, head), dQ summed in LDS) where it
    applies -- head_dim 64, no causal mask / ALiBi, S % 128 == 0, S <= 512; 8 waves (two per SIMD)
    at S = 512, else 4.  'fused4': the 4-wave form at every S.  'split': the dQ + dK/dV
    kernel pair.  Returns the previous form.  Without an experimental build every form runs the
    split kernels."""
    old = _lib.lib().dtd_attn_set_bwd_form(_BWD_FORMS.index(form))
    return _BWD_FORMS[old]


def set_bwd_kernels(dq: bool = True, dkdv: bool = True) -> tuple[bool, bool]:
    """Timing hook (scripts/bench_attn.py): run only the dQ or only the dK/dV kernel of the split
    backward, to price them separately.  Anything but (True, True) leaves part of dqkv unwritten.
    Returns the previous setting."""
    old = _lib.lib().dtd_attn_set_bwd_kernels(int(dq) | (int(dkdv) << 1))
    return bool(old & 1), bool(old & 2)


def fused_bwd_built() -> bool:
    """The one-kernel backward forms are compiled only into experimental builds
    (DTD_BUILD_EXPERIMENTAL=1): they measured no faster than the split kernels."""
    return _lib.has("dtd_attn_fused_bwd_built") and bool(_lib.lib().dtd_attn_fused_bwd_built())


def fused_bwd_applies(S: int, D: int, causal: bool, slopes, key_range=None, doc_range=None, window=None) -> bool:
    """Whether ``attn_bwd`` may take a one-kernel form; never with a key range, document spans or a
    sliding window (split pair only)."""
    return (not window and key_range is None and doc_range is None and D == 64 and not causal and slopes is None and S % 128 == 0 and S <= 512
            and fused_bwd_built())


def _require(name: str, what: str) -> str:
    """Entry point ``name`` of the kernel library; one built before it existed is an error, not a fallback."""
    if not _lib.has(name):
        raise _lib.KernelError(f"the kernel library has no {what} attention entry points (stale build)")
    return name


def _range_arg(key_range: torch.Tensor, B: int, device) -> torch.Tensor:
    """The kernels' kv_range argument: int32 [B, 2], contiguous, on the activations' device."""
    if tuple(key_range.shape) != (B, 2):
        raise ValueError(f"key_range must be [B, 2] = [{B}, 2], got {tuple(key_range.shape)}")
    _require("dtd_attn_fwd_range", "ranged")
    return key_range.to(device=device, dtype=torch.int32).contiguous()


def _doc_arg(doc_range, B: int, S: int, device) -> torch.Tensor:
    """The kernels' doc argument: int32, the [B, S, 2] spans then the [B, ceil(S/128), 2] block
    bounds, contiguous, on the activations' device.  Bare [B, S, 2] spans get their bounds here."""
    _doc_ranges(doc_range, B, S)
    _require("dtd_attn_fwd_doc", "document-masked")
    if not isinstance(doc_range, DocRange):
        doc_range = _doc_pack(doc_range.to(device))
    flat = doc_range.flat.to(device=device, dtype=torch.int32).contiguous()
    nb = (S + _DOC_BLOCK - 1) // _DOC_BLOCK
    if flat.numel() != 2 * B * (S + nb):
        raise ValueError(f"doc_range.flat must hold 2 * B * (S + ceil(S/128)) = {2 * B * (S + nb)} ints, got {flat.numel()}")
    return flat


def kernel_supported(qkv: torch.Tensor, D: int) -> bool:
    return qkv.is_cuda and qkv.dtype == torch.bfloat16 and D in (64, 128) and _lib.has("dtd_attn_fwd")


def f32_kernel_supported(qkv: torch.Tensor, D: int) -> bool:
    """The reference-precision kernels (ops/csrc/attention_f32.hip: exact f32 MFMA products)."""
    return (qkv.is_cuda and qkv.dtype == torch.float32 and D in (64, 128) and _lib.has("dtd_attn_fwd_f32")
            and _lib.has("dtd_attn_masks"))


def _masks_now(B, S, H, p, rng, sid, device) -> torch.Tensor:
    """Dropout keep bits generated on the current stream (the fp32 path)."""
    masks = alloc_masks(B, H, S, device)
    _lib.call("dtd_attn_masks", masks.data_ptr(), B, S, H, float(p), rng.state.data_ptr(), sid, _lib.stream())
    return masks


_SIDE = {}


def _side_stream(device) -> torch.cuda.Stream:
    s = _SIDE.get(device)
    if s is None:
        s = _SIDE[device] = torch.cuda.Stream(device)
    return s


def mask_words(B: int, H: int, S: int) -> int:
    """Words per keep-bit layout of one attention call: [B*H][W][32 W], W = ceil(S / 32)."""
    W = (S + 31) // 32
    return B * H * W * 32 * W


def alloc_masks(B: int, H: int, S: int, device) -> torch.Tensor:
    """[2, mask_words] int32 keep-bit buffer (both layouts back to back), exactly sized: every keep
    word the attention kernels read lies inside it (their scalar-load addresses are clamped into
    the (batch, head) plane and the row, ops/csrc/attention.hip keep_off; the vector prefetches go
    through bounded buffer resources)."""
    n = mask_words(B, H, S)
    return torch.empty((2, n), dtype=torch.int32, device=device)


def _lm_pos(n: int) -> torch.Tensor:
    """Word position of each of n positions inside its [32 W] row (ops/csrc/attention.hip lm_pos:
    within a 32-group, c = 8a + 4b + j sits at 8a + 2j + b)."""
    x = torch.arange(n)
    c = x & 31
    return (x & ~31) | (c & 24) | ((c & 3) << 1) | ((c >> 2) & 1)


def decode_masks(masks: torch.Tensor, B: int, H: int, S: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The two generated keep-bit layouts as [B*H, S, S] 0/1 int64 tensors (query, key): A (key
    bits per query word) and B (query bits per key word) -- both must equal attn_keep_mask."""
    W = (S + 31) // 32
    m = masks.cpu().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    pos = _lm_pos(S)
    bits = torch.arange(32, dtype=torch.int64)
    out = []
    for li in range(2):
        words = m[li].view(B * H, W, 32 * W)[:, :, pos]          # [bh][w][position]
        d = ((words.unsqueeze(-1) >> bits) & 1).permute(0, 2, 1, 3).reshape(B * H, S, W * 32)[..., :S]
        out.append(d if li == 0 else d.transpose(1, 2))            # B: [bh][key][q] -> [bh][q][key]
    return out[0], out[1]


class PendingMasks:
    """Dropout keep-bit masks being generated on a side stream (see ``attn_masks_async``)."""

    def __init__(self, masks: torch.Tensor, event: torch.cuda.Event):
        self.masks, self.event = masks, event


_MASK_REPEAT = max(1, int(os.environ.get("DTD_ATTN_MASK_REPEAT", "1")))


def attn_masks_async(B, S, H, D, p, rng: RngState, sid, device) -> PendingMasks | None:
    """Start generating the attention-dropout keep bits on a side stream.  The kernel is pure
    VALU (counter-RNG hashing) and independent of the activations, so issued before the QKV
    projection it runs concurrently with that MFMA-bound GEMM; ``attn_fwd(masks=...)`` joins
    it.  Returns None when the kernel path is not used (CPU / reference)."""
    if p <= 0 or not torch.cuda.is_available() or torch.device(device).type != "cuda" or D not in (64, 128) \
            or not _lib.has("dtd_attn_masks"):
        return None
    cur = torch.cuda.current_stream(device)
    masks = alloc_masks(B, H, S, device)
    side = _side_stream(torch.device(device))
    side.wait_stream(cur)                      # the rng step / previous users of the buffer
    with torch.cuda.stream(side):
        for _ in range(_MASK_REPEAT):   # (diagnostic: DTD_ATTN_MASK_REPEAT > 1 prices the generator)
            _lib.call("dtd_attn_masks", masks.data_ptr(), B, S, H, float(p), rng.state.data_ptr(), sid,
                      side.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(side)
    return PendingMasks(masks, ev)


class _Route(NamedTuple):
    """Where a call runs: the math ``reference``, or a kernel family -- ``f32`` (reference-precision),
    ``mha`` (bf16 multi-head), ``gqa``, ``win`` -- with the validated Hkv and effective window."""
    family: str
    Hkv: int
    window: int


# (forward, backward) entry points of the kernel families; mha by key_range / doc_range
_ENTRY = {
    "f32": ("dtd_attn_fwd_f32", "dtd_attn_bwd_f32"),
    "mha": ("dtd_attn_fwd", "dtd_attn_bwd"),
    "mha_range": ("dtd_attn_fwd_range", "dtd_attn_bwd_range"),
    "mha_doc": ("dtd_attn_fwd_doc", "dtd_attn_bwd_doc"),
    "gqa": ("dtd_attn_fwd_gqa", "dtd_attn_bwd_gqa"),
    "win": ("dtd_attn_fwd_win", "dtd_attn_bwd_win"),
}


def _route(qkv, B, S, H, D, causal, slopes, p, key_range, doc_range, kv_heads, window, backward: bool,
           masks=None) -> _Route:
    """The one routing rule of ``attn_fwd`` and ``attn_bwd`` (``backward``), so that a backward takes
    its forward's family.  A window, then grouped-query heads: bf16 on the GPU with D 64 / 128 runs
    their kernels (a library without them is an error, not a fallback), everything else the math
    reference.  Multi-head: fp32 with a range or spans takes the reference (the fp32 kernels know
    neither), other fp32 the fp32 kernels (a backward with dropout only given the keep bits), bf16 the
    bf16 kernels; a GPU build without them warns once and falls back."""
    _exclusive(key_range, doc_range)
    Hkv = _kv_heads(kv_heads, H)
    window = _window(window, S, causal, p, slopes)
    family = "reference"
    if window or Hkv != H:
        _check_gqa(qkv, B, S, H, Hkv, D, p, slopes)     # (a window: p = 0 and no slopes here -- the width)
        if qkv.is_cuda and qkv.dtype == torch.bfloat16 and D in (64, 128):
            family = "win" if window else "gqa"
            _require(_ENTRY[family][backward], "sliding-window" if window else "grouped-query")
    elif qkv.dtype == torch.float32 and (key_range is not None or doc_range is not None):
        pass
    elif f32_kernel_supported(qkv, D) and (not backward or p <= 0 or masks is not None):
        family = "f32"
    elif kernel_supported(qkv, D):
        family = "mha"
    elif not backward and qkv.is_cuda and qkv.dtype == torch.bfloat16 and _lib.has("dtd_attn_fwd") is False:
        _warn_once()
    return _Route(family, Hkv, window)


def _views(t: torch.Tensor, H: int, Hkv: int, D: int):
    """(q, k, v, ld): the addresses of the q | k | v blocks (H, Hkv and Hkv heads of D columns) inside
    the first row of a packed qkv / dqkv, and its row stride in elements.  Hkv = H is [.., 3, H, D]."""
    base, es = t.data_ptr(), t.element_size()
    return base, base + H * D * es, base + (H + Hkv) * D * es, (H + 2 * Hkv) * D


def _range_ptrs(r: _Route, key_range, doc_range, B, S, device, backward: bool):
    """(entry point, its key-range / document arguments, the tensors to keep alive) of a bf16 call:
    the grouped families take both pointers, either may be null; the multi-head entries are one per
    kind of masking and take their own."""
    kr = _range_arg(key_range, B, device) if key_range is not None else None
    doc = _doc_arg(doc_range, B, S, device) if doc_range is not None else None
    if r.family != "mha":
        return _ENTRY[r.family][backward], (_lib.ptr(kr), _lib.ptr(doc)), (kr, doc)
    if doc is not None:
        return _ENTRY["mha_doc"][backward], (doc.data_ptr(),), doc
    if kr is not None:
        return _ENTRY["mha_range"][backward], (kr.data_ptr(),), kr
    return _ENTRY["mha"][backward], (), None


def attn_fwd(qkv, B, S, H, D, causal=False, slopes=None, p=0.0, rng: RngState | None = None, sid=0,
             masks: PendingMasks | None = None, key_range: torch.Tensor | None = None,
             doc_range: DocRange | torch.Tensor | None = None, kv_heads: int | None = None,
             window: int | None = None):
    """Returns (ctx [B*S, H*D], lse [B, H, S] fp32, masks).  ``masks`` holds the dropout keep
    bits for the backward ([2, B*H*S*ceil(S/32)] int32 on the kernel path, None otherwise);
    pass the ``attn_masks_async`` result to reuse masks generated ahead on a side stream.

    ``key_range``: optional int32 [B, 2] per-sequence key ranges (module docstring).  The bf16
    kernels skip the key tiles outside a range.  fp32 inputs with a range take the math reference
    (the reference-precision fp32 kernels know no range).

    ``doc_range``: optional document spans of a packed batch (``DocRange``, or the bare int [B, S, 2]
    spans), exclusive with ``key_range``.  The bf16 kernels visit only the key tiles between each
    128-query block's bounds; fp32 inputs take the math reference, as with a key range.

    ``kv_heads``: grouped-query attention (module docstring): qkv is ``[B*S, (H + 2*Hkv)*D]``.  The
    bf16 kernels read each query head's K/V tiles from its group's head; fp32 inputs take the math
    reference.  None or H: the multi-head path, exactly as without the argument.

    ``window``: causal sliding window of that many keys per query (module docstring).  The bf16
    kernels visit only the band's key tiles; fp32 and CPU inputs take the math reference.  None, 0 or
    >= S: exactly the call without the argument."""
    r = _route(qkv, B, S, H, D, causal, slopes, p, key_range, doc_range, kv_heads, window, False)
    if r.family == "reference":
        if masks is not None:    # keep bits generated ahead for the fp32 kernels: unused, but join
            torch.cuda.current_stream(qkv.device).wait_event(masks.event)   # before their buffer is freed
        ctx, lse = attn_fwd_ref(qkv, B, S, H, D, causal, slopes, p, rng, sid, key_range=key_range, doc_range=doc_range,
                                kv_heads=r.Hkv, window=r.window)
        return ctx, lse, None
    qkv = qkv.contiguous()
    ctx = torch.empty((B * S, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    q, k, v, ld = _views(qkv, H, r.Hkv, D)
    scale = 1.0 / math.sqrt(D)
    if r.family in ("gqa", "win"):       # (no dropout, so no keep bits; causal = 1 under a window)
        name, ranges, _keep = _range_ptrs(r, key_range, doc_range, B, S, qkv.device, False)
        win = (1, scale, r.window) if r.window else (int(causal), scale)
        _lib.call(name, q, k, v, ctx.data_ptr(), lse.data_ptr(), B, S, H, r.Hkv, D, ld, H * D, *win, *ranges, _lib.stream())
        return ctx, lse, None
    rng_ptr = rng.state.data_ptr() if rng is not None else None
    if p > 0 and masks is not None:
        torch.cuda.current_stream(qkv.device).wait_event(masks.event)
        masks, rng_ptr = masks.masks, None     # generated already
    elif p > 0 and r.family == "f32":
        masks = _masks_now(B, S, H, p, rng, sid, qkv.device)
    elif p > 0:
        masks = alloc_masks(B, H, S, qkv.device)   # the forward kernel call generates them
    else:
        masks = None
    sl = slopes.to(device=qkv.device, dtype=torch.float32).contiguous() if slopes is not None else None
    args = (q, k, v, ctx.data_ptr(), lse.data_ptr(), _lib.ptr(sl), _lib.ptr(masks), B, S, H, D, ld, H * D, int(causal),
            scale, float(p))
    if r.family == "f32":
        _lib.call(_ENTRY["f32"][0], *args, _lib.stream())
    else:
        name, ranges, _keep = _range_ptrs(r, key_range, doc_range, B, S, qkv.device, False)
        _lib.call(name, *args, rng_ptr, sid, *ranges, _lib.stream())
    return ctx, lse, masks


def attn_bwd(dctx, qkv, ctx, lse, B, S, H, D, causal=False, slopes=None, p=0.0, rng=None, sid=0, masks=None,
             dbias=None, key_range: torch.Tensor | None = None,
             doc_range: DocRange | torch.Tensor | None = None, kv_heads: int | None = None,
             window: int | None = None):
    """Returns dqkv [B*S, 3*H*D] in the qkv layout.  ``dbias`` = (dst, acc): also writes the
    column sums of dqkv (the qkv projection's bias gradient) -- on the multi-head bf16 kernel path at
    D = 64 as per-wave partials from the dQ / dK,dV epilogues (no extra pass over dqkv), everywhere
    else in a pass of its own (``bias_grad``).

    ``key_range``: the forward's ranges.  Keys outside a range get zero dK / dV; the bf16 path
    runs the split dQ + dK/dV kernels (never a one-kernel form) and skips the key tiles / key
    blocks outside the range.  fp32 inputs with a range take the math reference.

    ``doc_range``: the forward's document spans.  Pad keys get zero dK / dV and pad queries zero dQ;
    the split kernels visit only the key tiles (dQ) / query tiles (dK/dV) between each block's bounds.

    ``kv_heads``: the forward's (grouped-query attention): dqkv is ``[B*S, (H + 2*Hkv)*D]``; one
    dK/dV workgroup per (key block, key/value head) sums its group's query heads in registers.

    ``window``: the forward's sliding window: the split kernels of the windowed family, whose dK/dV
    workgroups stop at the last query that sees one of their keys."""
    from . import functional as Fx
    r = _route(qkv, B, S, H, D, causal, slopes, p, key_range, doc_range, kv_heads, window, True, masks)
    part = None
    if r.family == "reference":
        dqkv = attn_bwd_ref(dctx, qkv, ctx, lse, B, S, H, D, causal, slopes, p, rng, sid, key_range=key_range,
                            doc_range=doc_range, kv_heads=r.Hkv, window=r.window)
    else:
        dctx = dctx.contiguous()
        dqkv = torch.empty_like(qkv)
        delta = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
        q, k, v, ld = _views(qkv, H, r.Hkv, D)
        dq, dk, dv, _ = _views(dqkv, H, r.Hkv, D)
        scale = 1.0 / math.sqrt(D)
        head = (q, k, v, ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), delta.data_ptr())
        if r.family == "f32":
            name, ranges = _ENTRY["f32"][1], ()
        else:
            name, ranges, _keep = _range_ptrs(r, key_range, doc_range, B, S, qkv.device, True)
        if r.family in ("gqa", "win"):
            win = (1, scale, r.window) if r.window else (int(causal), scale)
            _lib.call(name, *head, dq, dk, dv, B, S, H, r.Hkv, D, ld, H * D, *win, *ranges, _lib.stream())
        else:
            sl = slopes.to(device=qkv.device, dtype=torch.float32).contiguous() if slopes is not None else None
            if r.family == "mha" and dbias is not None and D == 64:
                # one row per (batch, 32-row block of a 128-row workgroup tile); every entry is written
                part = torch.empty((B * 4 * ((S + 127) // 128), ld), dtype=torch.float32, device=qkv.device)
            tail = (_lib.ptr(part),) if r.family == "mha" else ()
            _lib.call(name, *head, _lib.ptr(masks if p > 0 else None), dq, dk, dv, _lib.ptr(sl), B, S, H, D, ld, H * D,
                      int(causal), scale, float(p), *tail, *ranges, _lib.stream())
    if dbias is not None and part is not None:
        dst, acc = dbias
        Fx._finalize(part, part.shape[0], ld, (dst, acc), acc)
    elif dbias is not None:
        Fx.bias_grad(dqkv, *dbias)
    return dqkv


# ---------------------------------------------------------------------------------- incremental decoding
# One new query token per sequence against a KV cache (ops/kv_cache.py, ops/csrc/attention_decode.hip).
# Cache layout, per layer: K, V [B, Hkv, Smax, D]; ``kv_len`` / ``kv_start`` are device int32 [B] (slots
# written, counting the new token; first valid slot, 0 unless the prompt was left-padded).  Sequence b
# attends the slots max(kv_start[b], hi - W) <= j < hi with hi = min(kv_len[b], Smax) -- a kv_len beyond
# the cache is clamped, not trusted, before the window is applied; an empty range gives ctx = 0,
# lse = -inf (the empty-row rule above).  An FP8 cache holds e4m3fn codes in K / V and one fp32 scale per row in
# ``k_scale`` / ``v_scale [B, Hkv, Smax]``; its value is float(code) * scale (ops/kv_cache.py).
DECODE_KEY_TILE = 64         # keys per tile of the decode kernel: split boundaries are its multiples
_DECODE_MAX_GROUP = 8         # query heads per key/value head the kernel keeps in registers
_DECODE_WORKGROUPS = 512      # two workgroups for each of the 256 CUs


def decode_splits(B: int, Hkv: int, Smax: int) -> int:
    """Key splits of a decode call: a function of (B, Hkv, Smax) only -- never of the cache position --
    so the launch sequence of a step is static and can be captured.  Enough (sequence, key/value head,
    split) workgroups to cover the CUs twice, but no split shorter than two key tiles."""
    tiles = (Smax + DECODE_KEY_TILE - 1) // DECODE_KEY_TILE
    want = (_DECODE_WORKGROUPS + B * Hkv - 1) // max(1, B * Hkv)
    return max(1, min(want, tiles // 2))


def decode_workspace_floats(B: int, H: int, D: int, splits: int) -> int:
    """fp32 elements of the decode kernel's split workspace: (m, l, o[D]) per (split, sequence, head)."""
    return splits * B * H * (D + 2)


def _decode_bounds(kv_len, kv_start, window, Smax):
    """(lo, hi) int64 [B] of a decode call (see above)."""
    hi = kv_len.to(torch.int64).clamp(max=Smax)
    lo = torch.zeros_like(hi) if kv_start is None else kv_start.to(device=hi.device, dtype=torch.int64).clamp(min=0)
    if window:
        lo = torch.maximum(lo, hi - int(window))
    return lo, hi


def _decode_window(window) -> int:
    if window is None:
        return 0
    if isinstance(window, bool) or int(window) != window or window < 0:
        raise ValueError(f"window must be a positive integer (or None / 0 for no window), got {window!r}")
    return int(window)


_FP8 = torch.float8_e4m3fn


def _check_decode(qkv, k_cache, v_cache, kv_len, B, H, Hkv, D, k_scale=None, v_scale=None) -> bool:
    """Validates a decode call; returns whether the caches are FP8 (e4m3fn codes with per-row scales)."""
    if qkv.dim() != 2 or tuple(qkv.shape) != (B, (H + 2 * Hkv) * D) or qkv.stride(1) != 1:
        raise ValueError(f"qkv must be [B, (H + 2*Hkv)*D] = [{B}, {(H + 2 * Hkv) * D}], got {tuple(qkv.shape)}")
    if k_cache.dim() != 4 or tuple(k_cache.shape[:2]) != (B, Hkv) or k_cache.shape[3] != D \
            or v_cache.shape != k_cache.shape:
        raise ValueError(f"k_cache / v_cache must be [B, Hkv, Smax, D] = [{B}, {Hkv}, Smax, {D}], got "
                         f"{tuple(k_cache.shape)} / {tuple(v_cache.shape)}")
    fp8 = k_cache.dtype == _FP8 or v_cache.dtype == _FP8
    if fp8:
        if k_cache.dtype != v_cache.dtype:
            raise ValueError("k_cache and v_cache must both be float8_e4m3fn")
        want = tuple(k_cache.shape[:3])
        for name, sc in (("k_scale", k_scale), ("v_scale", v_scale)):
            if sc is None or tuple(sc.shape) != want or sc.dtype != torch.float32 or sc.device != k_cache.device:
                raise ValueError(f"an FP8 cache needs {name}: fp32 [B, Hkv, Smax] = {list(want)} on the cache's device, got "
                                 f"{None if sc is None else (tuple(sc.shape), sc.dtype)}")
    elif k_scale is not None or v_scale is not None:
        raise ValueError("k_scale / v_scale go with an FP8 (float8_e4m3fn) cache only")
    elif k_cache.dtype != qkv.dtype or v_cache.dtype != qkv.dtype:
        raise ValueError("the cache must have the activations' dtype")
    if kv_len.numel() != B:
        raise ValueError(f"kv_len must hold one length per sequence ({B}), got {tuple(kv_len.shape)}")
    return fp8


def attn_decode_ref(qkv, k_cache, v_cache, kv_len, B, H, D, kv_heads=None, window=None, kv_start=None, scale=None,
                    k_scale=None, v_scale=None):
    """Math reference of ``attn_decode``: plain PyTorch over the whole cache with the slots outside
    [lo, hi) masked, softmax in fp32 (fp64 for fp64 inputs), the rounding points of ``attn_fwd_ref``
    (ctx rounded once, at the end).  An FP8 cache (``k_scale`` / ``v_scale``) is dequantised first --
    ``float(code) * scale`` in the compute dtype -- and then takes the same math.
    Returns (ctx [B, H*D], lse [B, H] fp32)."""
    Hkv = _kv_heads(kv_heads, H)
    fp8 = _check_decode(qkv, k_cache, v_cache, kv_len, B, H, Hkv, D, k_scale, v_scale)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    Smax = k_cache.shape[2]
    c = _cdt(qkv)
    q = qkv[:, :H * D].reshape(B, H, 1, D).to(c)
    G = H // Hkv
    if fp8:
        k_cache, v_cache = k_cache.to(c) * k_scale.to(c).unsqueeze(-1), v_cache.to(c) * v_scale.to(c).unsqueeze(-1)
    k, v = k_cache.to(c).repeat_interleave(G, 1), v_cache.to(c).repeat_interleave(G, 1)     # [B, H, Smax, D]
    s = torch.matmul(q, k.transpose(-1, -2)) * scale                                       # [B, H, 1, Smax]
    lo, hi = _decode_bounds(kv_len.to(qkv.device), kv_start, _decode_window(window), Smax)
    j = torch.arange(Smax, device=qkv.device).view(1, Smax)
    outside = ((j < lo.view(B, 1)) | (j >= hi.view(B, 1))).view(B, 1, 1, Smax)
    s = s.masked_fill(outside, float("-inf"))
    lse = torch.logsumexp(s, -1)
    prob = _probs(s, lse)
    # (0 * a masked slot's V: a never-written slot may hold anything, NaN included -- it takes no part)
    v = v.masked_fill(outside.transpose(-1, -2), 0.0)
    ctx = torch.matmul(prob, v)                                                            # [B, H, 1, D]
    return ctx.reshape(B, H * D).to(qkv.dtype), lse.reshape(B, H).to(torch.float32)


def decode_kernel_supported(qkv: torch.Tensor, H: int, Hkv: int, D: int) -> bool:
    """The decode kernel's domain: bf16 on the GPU, D 64 / 128, at most 8 query heads per key/value head."""
    return qkv.is_cuda and qkv.dtype == torch.bfloat16 and D in (64, 128) and H // Hkv <= _DECODE_MAX_GROUP


def attn_decode(qkv, k_cache, v_cache, kv_len, B, H, D, kv_heads=None, window=None, kv_start=None, splits=None,
                workspace: torch.Tensor | None = None, out: tuple | None = None, k_scale: torch.Tensor | None = None,
                v_scale: torch.Tensor | None = None):
    """Attention of one new token per sequence against the cache: ``qkv [B, (H + 2*Hkv)*D]`` is the step's
    packed projection output (only its q block is read; its k / v rows are already in the cache,
    ``functional.rope_append_``), ``k_cache`` / ``v_cache [B, Hkv, Smax, D]``, ``kv_len`` / ``kv_start``
    device int32 [B] as above.  Returns (ctx [B, H*D], lse [B, H] fp32).

    One routing rule: bf16 on the GPU with D 64 / 128 and H / Hkv <= 8 runs the split-KV kernel -- in its FP8
    format when the caches are ``float8_e4m3fn`` codes with their ``k_scale`` / ``v_scale`` (fp32
    ``[B, Hkv, Smax]``, ops/kv_cache.py) -- and a library without it is an error, not a fallback; everything
    else -- larger groups, fp32, the CPU -- the math reference.  FP8 caches without scales, or scales of another
    shape or dtype, are a ``ValueError``.  ``splits``: override of ``decode_splits`` (tests, benchmarks).  ``workspace``: fp32 buffer of
    at least ``decode_workspace_floats`` elements (``KVCache`` holds one, so a captured step allocates
    nothing for it); allocated here when None.  ``out``: (ctx, lse) tensors to write, of the returned
    shapes and dtypes, ctx with unit column stride."""
    Hkv = _kv_heads(kv_heads, H)
    window = _decode_window(window)
    fp8 = _check_decode(qkv, k_cache, v_cache, kv_len, B, H, Hkv, D, k_scale, v_scale)
    if not decode_kernel_supported(qkv, H, Hkv, D):
        ctx, lse = attn_decode_ref(qkv, k_cache, v_cache, kv_len, B, H, D, Hkv, window, kv_start, k_scale=k_scale,
                                   v_scale=v_scale)
        if out is not None:
            out[0].copy_(ctx)
            out[1].copy_(lse)
            return out[0], out[1]
        return ctx, lse
    entry = "dtd_attn_decode_fp8" if fp8 else "dtd_attn_decode"
    _require(entry, "FP8 decode" if fp8 else "decode")
    Smax = k_cache.shape[2]
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("k_cache / v_cache must be contiguous [B, Hkv, Smax, D]")
    if fp8 and not (k_scale.is_contiguous() and v_scale.is_contiguous()):
        raise ValueError("k_scale / v_scale must be contiguous [B, Hkv, Smax]")
    tiles = (Smax + DECODE_KEY_TILE - 1) // DECODE_KEY_TILE
    splits = decode_splits(B, Hkv, Smax) if splits is None else int(splits)
    if splits < 1:
        raise ValueError(f"splits must be >= 1, got {splits}")
    splits = min(splits, tiles)
    need = decode_workspace_floats(B, H, D, splits)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=qkv.device)
    elif workspace.dtype != torch.float32 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous fp32 tensor of at least {need} elements")
    dev = qkv.device
    kv_len = kv_len.to(device=dev, dtype=torch.int32).contiguous()
    kv_start = kv_start.to(device=dev, dtype=torch.int32).contiguous() if kv_start is not None else None
    if out is None:
        ctx = torch.empty((B, H * D), dtype=qkv.dtype, device=dev)
        lse = torch.empty((B, H), dtype=torch.float32, device=dev)
    else:
        ctx, lse = out
        if tuple(ctx.shape) != (B, H * D) or ctx.dtype != qkv.dtype or ctx.stride(1) != 1 or ctx.device != dev \
                or tuple(lse.shape) != (B, H) or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.device != dev:
            raise ValueError(f"out must be (ctx [{B}, {H * D}] {qkv.dtype}, lse [{B}, {H}] fp32, contiguous) on {dev}")
    scales = (k_scale.data_ptr(), v_scale.data_ptr()) if fp8 else ()
    _lib.call(entry, qkv.data_ptr(), qkv.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), *scales,
              kv_len.data_ptr(), _lib.ptr(kv_start), ctx.data_ptr(), ctx.stride(0), lse.data_ptr(), workspace.data_ptr(),
              workspace.numel(), B, H, Hkv, D, Smax, window, 1.0 / math.sqrt(D), splits, _lib.stream())
    return ctx, lse
