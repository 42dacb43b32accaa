"""Mixture-of-experts decoder layer (HF ``MixtralDecoderLayer``): the Llama layer's attention half with a
routed expert FFN in place of the dense SwiGLU MLP.

    z1 = x + attention(RMS1(x));  f_in = RMS2(z1);  logits = f_in gate_w^T            [T, E]
    the k largest logits of a token select its experts e_0 .. e_{k-1} (a tie to the lower index),
    w_r = exp(l_{e_r} - m) / sum_{r' < k} exp(l_{e_r'} - m)   (fp32; HF's softmax, top-k, renormalise)
    out = z1 + sum_r w_r (silu(f_in gate_{e_r}^T) * (f_in up_{e_r}^T)) down_{e_r}^T

Layout: ``gate_w [E, h]`` (the router), ``gu_w [E, 2f, h]`` (per expert: gate rows, then up rows, as the dense
``gu_w``), ``down_w [E, h, f]`` -- HF 5's ``mlp.gate.weight``, ``mlp.experts.gate_up_proj`` and
``mlp.experts.down_proj`` one to one.  The experts run as strided-batch GEMMs over a fixed-capacity
``[E, C, .]`` layout: expert e's C slots are taken by the (token, rank) pairs that chose it, by rank first and
then token index, so no token's second choice displaces another token's first; pairs past C are dropped (they
add nothing to the output and their weights are not renormalised).  ``C = T`` when ``cfg.moe_capacity_factor``
is 0 -- dropless, exactly HF Mixtral, at the cost of E / k times the active FLOPs -- else
``min(T, 8 ceil(cf T k / (8 E)))`` (DeepSpeed's capacity factor).  C is a function of the shapes only and nothing
reads a count back to the host.

Load-balancing loss of layer l: ``aux_l = E sum_{r, e} f_l[r, e] P_l[e]`` with f_l[r, e] the share of the T
tokens whose rank-r choice is e (counted before drops, no gradient) and ``P_l = mean_t softmax(logits_l)``.
The model's ``aux_loss`` is the mean of aux_l over the layers.  For one layer that is exactly HF's
``load_balancing_loss_func``; for more, HF multiplies the layer-averaged f and P, which adds cross-layer terms
this definition does not have.  Limit: all T positions count, pads included -- HF's behaviour without
``attention_mask``.

Only the ``reference`` implementation exists: differentiable PyTorch, on the CPU or the GPU.  There is no fused
path (gfx950 routing kernels and a hand-written backward) yet, and asking for one -- ``impl='fused'``, or
``impl='auto'`` on a GPU -- is an error, not a fall-back: build the model with ``impl='reference'``.  Expert
parallelism (all-to-all) is not implemented either.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from ..ops import attention as A
from .config import TransformerConfig
from .layers import ref_rms_norm
from .llama import LlamaLayer, _ref_rope, rope_table_for
from .transformer import Runtime, init_linear_, ref_attn_dropout


def capacity(T: int, E: int, k: int, capacity_factor: float) -> int:
    """Slots per expert: T when ``capacity_factor`` is 0 (dropless: an expert can take every token once),
    else DeepSpeed's ``min(T, 8 * ceil(cf * T * k / (8 * E)))``."""
    if capacity_factor < 0:
        raise ValueError("capacity_factor must be >= 0 (0 = dropless)")
    if capacity_factor == 0:
        return T
    return max(1, min(T, 8 * math.ceil(capacity_factor * T * k / (8 * E))))


def select_topk(logits: torch.Tensor, k: int) -> torch.Tensor:
    """[T, k] int64 expert indices: the k largest stored logits, rank 0 the largest, ties to the lower index (a
    stable sort).  Exact comparison of stored values: fp32 softmax rounding cannot change a choice."""
    if not 1 <= k <= logits.shape[-1]:
        raise ValueError(f"select_topk: k = {k} must be in [1, E = {logits.shape[-1]}]")
    return torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]


def assign_slots(idx: torch.Tensor, E: int, C: int):
    """(token_slot [T, k], slot_src [E * C]) int64 for the choices ``idx [T, k]``: token_slot is the pair's flat
    slot ``e * C + pos`` or -1 when dropped, slot_src the slot's flat pair ``t * k + r`` or -1 when empty;
    positions inside an expert go by rank, then token.  Indexing ops with static shapes (one-hot + cumsum), so
    nothing is read back to the host."""
    T, k = idx.shape
    flat = idx.t().reshape(-1)                                         # pair order: rank-major
    onehot = F.one_hot(flat, E)
    pos = (onehot.cumsum(0) - onehot).gather(1, flat[:, None])[:, 0]   # earlier pairs of the same expert
    keep = pos < C
    slot = torch.where(keep, flat * C + pos, torch.full_like(pos, -1))
    pair = (torch.arange(T, device=idx.device)[None, :] * k + torch.arange(k, device=idx.device)[:, None]).reshape(-1)
    buf = torch.full((E * C + 1,), -1, dtype=torch.int64, device=idx.device)
    buf.scatter_(0, torch.where(keep, slot, torch.full_like(slot, E * C)), pair)   # drops land in the spare element
    return slot.view(k, T).t().contiguous(), buf[:E * C].contiguous()


def ref_moe_ffn(f_in: torch.Tensor, z1: torch.Tensor | None, logits: torch.Tensor, gu_w, down_w, k: int, C: int):
    """The routed FFN in differentiable PyTorch on ``[T, h]`` rows for given router ``logits [T, E]``: returns
    (out = z1 + sum_r w_r FFN_{e_r}(f_in), aux_l).  Selection and slots are integer functions of the detached
    logits; the weights, the gathers and the load-balancing loss are differentiable.  The sum over the kept
    pairs runs in rank order in fp32 and is rounded once."""
    T, h = f_in.shape
    E, f2, _ = gu_w.shape
    idx = select_topk(logits.detach(), k)
    w = torch.softmax(logits.float().gather(1, idx), -1)
    token_slot, slot_src = assign_slots(idx, E, C)
    zero = torch.zeros((), dtype=f_in.dtype, device=f_in.device)
    xe = torch.where((slot_src >= 0)[:, None], f_in[slot_src.clamp_min(0) // k], zero)      # empty slots: zero rows
    g, u = torch.bmm(xe.view(E, C, h), gu_w.transpose(1, 2)).split(f2 // 2, -1)
    ye = torch.bmm(F.silu(g) * u, down_w.transpose(1, 2)).view(E * C, h)
    acc = torch.zeros((T, h), dtype=torch.float32, device=f_in.device) if z1 is None else z1.float()
    for r in range(k):
        s = token_slot[:, r]
        acc = acc + torch.where((s >= 0)[:, None], w[:, r, None] * ye[s.clamp_min(0)].float(), zero.float())
    frac = (F.one_hot(idx, E).sum(0).double() / T).float()                # [k, E], no gradient
    aux = float(E) * (frac.sum(0) * torch.softmax(logits.float(), -1).mean(0)).sum()
    return acc.to(f_in.dtype), aux


class MoeLlamaLayer(LlamaLayer):
    """``LlamaLayer`` with ``cfg.num_experts`` routed experts.  After a forward ``aux_loss`` holds the layer's
    load-balancing loss (a graph-connected fp32 scalar) and ``router_logits`` its [T, E] logits (detached)."""

    def __init__(self, cfg: TransformerConfig, rt: Runtime):
        if cfg.num_experts <= 0:
            raise ValueError("MoeLlamaLayer needs num_experts > 0")
        super().__init__(cfg, rt)
        h, f, E = cfg.hidden_size, cfg.ffn_size, cfg.num_experts
        del self.gu_w, self.down_w                                 # the dense MLP's
        self.gate_w = nn.Parameter(torch.empty(E, h))              # router
        self.gu_w = nn.Parameter(torch.empty(E, 2 * f, h))         # per expert: gate rows, then up
        self.down_w = nn.Parameter(torch.empty(E, h, f))
        for w in (self.gate_w, self.gu_w, self.down_w):
            init_linear_(w, None)
        self.aux_loss = self.router_logits = None

    def params(self):
        return (self.qkv_w, self.o_w, self.n1_g, self.gate_w, self.gu_w, self.down_w, self.n2_g)

    def dgrad_weights(self, nt: bool):
        """Nothing to transpose ahead: there is no hand-written backward here."""
        return ()

    def forward(self, x: torch.Tensor, key_range: torch.Tensor | None = None, doc_range=None,
                position_ids: torch.Tensor | None = None) -> torch.Tensor:
        if key_range is not None and doc_range is not None:
            raise ValueError("key_range and doc_range are mutually exclusive")
        S = x.shape[1]
        if S > self.cfg.max_positions:
            raise ValueError(f"sequence length {S} exceeds max_positions {self.cfg.max_positions} of the rotary table")
        if self.rt.use_fused(x):
            raise NotImplementedError("the mixture-of-experts layer has no fused path (no routing kernels yet): "
                                      "build the model with impl='reference'")
        self._dtd_weightless_bwd = False
        table = rope_table_for(self.rt, self.cfg, x.device)
        out, aux, logits = self._reference(x, key_range, doc_range, position_ids, table)
        self.aux_loss, self.router_logits = aux, logits.detach()
        return out

    def _reference(self, x, key_range, doc_range, position_ids, table):
        """``LlamaLayer._reference``'s attention half, then the routed FFN."""
        c, rt = self.cfg, self.rt
        B, S, h = x.shape
        H, D, Hkv = c.num_heads, c.head_dim, c.kv_heads
        tr = self.training
        if position_ids is None:
            cs = table[:S][None]
        else:
            cs = table[position_ids.to(device=x.device, dtype=torch.int64).clamp(0, table.shape[0] - 1)]
        a_in = ref_rms_norm(x, self.n1_g, c.ln_eps)
        qkv = F.linear(a_in, self.qkv_w).view(B, S, H + 2 * Hkv, D)
        q = _ref_rope(qkv[:, :, :H], cs).transpose(1, 2)
        k = _ref_rope(qkv[:, :, H:H + Hkv], cs).transpose(1, 2).repeat_interleave(H // Hkv, 1)
        v = qkv[:, :, H + Hkv:].transpose(1, 2).repeat_interleave(H // Hkv, 1)
        s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
        if c.causal:
            s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
        if c.sliding_window:
            s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=s.device).tril(-c.sliding_window), float("-inf"))
        if key_range is not None or doc_range is not None:
            outside = A._range_mask(key_range, B, S, s.device) if key_range is not None \
                else A._doc_mask(doc_range, B, S, s.device)
            s = s.masked_fill(outside, float("-inf"))
            dead = (s == float("-inf")).all(-1, keepdim=True)       # a row without a key attends to nothing
            prob = torch.softmax(s.float().masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0).to(s.dtype)
        else:
            prob = torch.softmax(s.float(), -1).to(s.dtype)
        prob = ref_attn_dropout(prob, c.attn_dropout if tr else 0.0, tr, rt, rt.rng.sid(self.sid_attn))
        ctx = torch.matmul(prob, v).transpose(1, 2).reshape(B, S, h)
        z1 = x + F.linear(ctx, self.o_w)
        f_in = ref_rms_norm(z1, self.n2_g, c.ln_eps).reshape(B * S, h)
        logits = F.linear(f_in, self.gate_w)
        C = capacity(B * S, c.num_experts, c.experts_per_token, c.moe_capacity_factor)
        out, aux = ref_moe_ffn(f_in, z1.reshape(B * S, h), logits, self.gu_w, self.down_w, c.experts_per_token, C)
        return out.view(B, S, h), aux, logits
