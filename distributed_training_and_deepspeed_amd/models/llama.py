"""Llama-family decoder layer (HF ``LlamaDecoderLayer``, multi-head or grouped-query attention) and HF
weight conversion.

    a_in = RMS1(x);  qkv = a_in qkv_w^T;  rotary(q, k);  ctx = causal attention;  o = ctx o_w^T
    z1 = x + o;  f_in = RMS2(z1);  gu = f_in gu_w^T;  a = silu(gate) * up;  out = z1 + a down_w^T

Two interchangeable implementations, as ``TransformerLayer``:

* ``fused``: one autograd node per layer with a hand-written backward over the gfx950 kernels -- residual +
  RMSNorm (ops/csrc/rmsnorm.hip), rotary embedding in place on the packed qkv (rope.hip), flash attention,
  SwiGLU (swiglu.hip) -- and the GEMMs of ops/gemm.py, writing weight gradients straight into the flat
  gradient buckets.  Saved per layer: x, a_in, the rotated qkv, ctx + LSE, z1, f_in, gu, the two rstd
  vectors and (``rt.keep_ffn_act``) a.  No cos / sin, no attention scores.  The rotation is orthogonal, so
  the backward applies the inverse rotation to the attention backward's dqkv before the qkv projection's
  weight and input gradients.
* ``reference``: the same math in plain differentiable PyTorch.

Weight layout: ``qkv_w [(H + 2 Hkv) D, h]`` (``[3h, h]`` for multi-head attention) is HF's q_proj, k_proj,
v_proj rows concatenated, ``gu_w [2f, h]`` its gate_proj then up_proj rows, so HF checkpoints convert by
``torch.cat`` (``from_hf_state_dict`` / ``to_hf_state_dict``; they only rename, concatenate and split --
nothing here reaches a hub).

Grouped-query attention (``cfg.num_kv_heads`` = Hkv < H = ``cfg.num_heads``): the k and v projections have
Hkv heads and query head i reads key/value head i // (H / Hkv) (HF's ``repeat_kv``).  The fused path never
expands K / V: the rotary kernel rotates the H + Hkv heads of the q and k blocks and the attention kernels
address K / V by group (ops/attention.py, ``kv_heads``).

Sliding window (``cfg.sliding_window`` = W > 0, Mistral): query i attends the W keys i - W < j <= i,
intersected with the key range / document span.  The fused path hands W to the attention kernels
(ops/attention.py, ``window``), which visit only the band's tiles; the reference masks the band.

Incremental decoding (``forward_cached``): the layer with a KV cache ``[B, Hkv, Smax, D]`` per layer
(ops/kv_cache.py) -- the prompt through the training forward's attention, then one token per step through
the split-KV decode kernel (ops/csrc/attention_decode.hip); ``CausalLM.generate`` drives it.

Rotary scaling is not implemented.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from ..ops import attention as A
from ..ops import functional as Fx
from ..ops import gemm as G
from ..ops.grad import emit_wgrad, grad_done, grad_dst, note_use
from .config import TransformerConfig
from .layers import ref_rms_norm
from .transformer import Runtime, init_linear_, ref_attn_dropout


def rope_table_for(rt: Runtime, cfg: TransformerConfig, device) -> torch.Tensor:
    """The model's (cos, sin) table on ``device``: built once (float64 angles, fp32 [max_positions,
    D/2, 2]) and kept on the Runtime -- not a buffer, so it stays off the state dict and
    ``model.to(bfloat16)`` does not round it.  It must exist before a hipGraph capture (the eager
    warm-up steps build it): building it inside one would tie its memory to the graph's pool."""
    tables = rt.rope_tables
    key = (str(torch.device(device)), cfg.head_dim, float(cfg.rope_theta), cfg.max_positions)
    t = tables.get(key)
    if t is None:
        if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the rotary table must be built before a graph capture (run one eager step first)")
        t = tables[key] = Fx.rope_table(cfg.max_positions, cfg.head_dim, cfg.rope_theta, device=device)
    return t


def _ref_rope(x: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    """Differentiable rotate-half rotary embedding: x [B, S, H, D], cs [B or 1, S, D/2, 2] fp32."""
    half = x.shape[-1] // 2
    c, s = cs[..., 0][:, :, None], cs[..., 1][:, :, None]
    x1, x2 = x[..., :half].float(), x[..., half:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)


class LlamaLayer(nn.Module):
    def __init__(self, cfg: TransformerConfig, rt: Runtime):
        super().__init__()
        if not cfg.llama_style:
            raise ValueError("LlamaLayer needs norm='rms', rope_theta > 0 and activation='swiglu'")
        h, f = cfg.hidden_size, cfg.ffn_size
        self.cfg, self.rt = cfg, rt
        # q rows, then k, then v: [3h, h], or [(H + 2 Hkv) D, h] with grouped-query attention
        self.qkv_w = nn.Parameter(torch.empty((cfg.num_heads + 2 * cfg.kv_heads) * cfg.head_dim, h))
        self.o_w = nn.Parameter(torch.empty(h, h))
        self.n1_g = nn.Parameter(torch.ones(h))               # input_layernorm
        self.gu_w = nn.Parameter(torch.empty(2 * f, h))       # gate rows, then up
        self.down_w = nn.Parameter(torch.empty(h, f))
        self.n2_g = nn.Parameter(torch.ones(h))               # post_attention_layernorm
        for w in (self.qkv_w, self.o_w, self.gu_w, self.down_w):
            init_linear_(w, None)
        self.sid_attn = rt.new_sid()

    def params(self):
        return (self.qkv_w, self.o_w, self.n1_g, self.gu_w, self.down_w, self.n2_g)

    def dgrad_weights(self, nt: bool):
        """See ``TransformerLayer.dgrad_weights``: the four projections in the NT form; there is no
        fused FFN-backward GEMM here, so nothing otherwise."""
        return (self.qkv_w, self.o_w, self.gu_w, self.down_w) if nt else ()

    def prefetch_attention_masks(self, B: int, S: int, device) -> None:
        """No side-stream mask prefetch: attention dropout (0 in every Llama preset) draws its keep
        bits inside the attention call."""

    def forward(self, x: torch.Tensor, key_range: torch.Tensor | None = None, doc_range=None,
                position_ids: torch.Tensor | None = None) -> torch.Tensor:
        """x: [B, S, h] -> [B, S, h].  ``key_range`` / ``doc_range`` as ``TransformerLayer.forward``.
        ``position_ids``: optional integer [B, S] rotary position per token (a packed batch restarts
        them at each document); default s."""
        if key_range is not None and doc_range is not None:
            raise ValueError("key_range and doc_range are mutually exclusive")
        S = x.shape[1]
        if S > self.cfg.max_positions:
            raise ValueError(f"sequence length {S} exceeds max_positions {self.cfg.max_positions} of the rotary table")
        table = rope_table_for(self.rt, self.cfg, x.device)
        # the fused backward reads the parameters at backward time: see TransformerLayer.forward
        self._dtd_weightless_bwd = self.rt.use_fused(x)
        if self._dtd_weightless_bwd:
            note_use(self.params())
            return _FusedLlamaLayerFn.apply(x, self, key_range, doc_range, position_ids, table, *self.params())
        return self._reference(x, key_range, doc_range, position_ids, table)

    # ------------------------------------------------------------------ incremental decoding
    @torch.no_grad()
    def forward_cached(self, x: torch.Tensor, cache, i: int, prefill: bool,
                       key_range: torch.Tensor | None = None) -> torch.Tensor:
        """x [B, Sq, h] -> [B, Sq, h] with the KV cache (ops/kv_cache.py) as layer ``i``; no autograd node.
        The new tokens sit at the slots ``cache.kv_len[b] + s``, which are also their rotary positions; the
        rotated k rows and the v rows are appended there (``Fx.rope_append_``) and ``cache.kv_len`` is left
        alone -- the caller advances it after the last layer.  ``prefill``: the prompt into an empty cache,
        attention being the training forward's over the prompt itself (``key_range`` for a left-padded
        one).  Otherwise one token per sequence (Sq = 1) against the cache (``A.attn_decode``).  The fused
        path runs the kernels of the training forward around it; the reference path the same cache in
        plain PyTorch.

        An FP8 cache (``cache.quantized``): the append quantises each row (``ops.kv_cache.quantize_kv_ref``'s law,
        by the quantising kernel on the fused path) and the decode attention reads codes and scales.  The prefill
        appends the prompt's rows the same way, but the prompt's own attention runs on the unquantised qkv: only
        the decode steps see quantised keys and values."""
        c, rt = self.cfg, self.rt
        B, Sq, h = x.shape
        H, D, Hkv = c.num_heads, c.head_dim, c.kv_heads
        if not prefill and Sq != 1:
            raise ValueError(f"a decode step takes one token per sequence, got {Sq}")
        table = rope_table_for(rt, c, x.device)
        kc, vc = cache.layer(i)
        fused = rt.use_fused(x)
        eps, window = c.ln_eps, c.sliding_window or None
        x2d = x.reshape(B * Sq, h)
        if fused:
            _, a_in, _ = Fx.rms_fwd(None, x2d, self.n1_g, eps)
            qkv = _linear(a_in, self.qkv_w)
        else:
            qkv = F.linear(ref_rms_norm(x2d, self.n1_g, eps), self.qkv_w)
        ks, vs = cache.layer_scales(i)      # (None, None) unless the cache is FP8
        Fx.rope_append_(qkv, table, kc, vc, cache.kv_len, B, Sq, H, D, kv_heads=Hkv, overflow=cache.overflow,
                        k_scale=ks, v_scale=vs)
        if prefill:      # (also with an FP8 cache: the prompt attends its own unquantised k / v)
            attn = A.attn_fwd if fused else A.attn_fwd_ref
            actx = attn(qkv, B, Sq, H, D, c.causal, key_range=key_range, kv_heads=Hkv if Hkv != H else None,
                        window=window)[0]
        elif fused:
            actx, _ = A.attn_decode(qkv, kc, vc, cache.kv_next, B, H, D, Hkv, window, cache.kv_start,
                                    splits=cache.splits, workspace=cache.workspace, k_scale=ks, v_scale=vs)
        else:
            actx, _ = A.attn_decode_ref(qkv, kc, vc, cache.kv_next, B, H, D, Hkv, window, cache.kv_start,
                                        k_scale=ks, v_scale=vs)
        if fused:
            o = _linear(actx, self.o_w)
            z1, f_in, _ = Fx.rms_fwd(o, x2d, self.n2_g, eps)
            a = Fx.swiglu_fwd(_linear(f_in, self.gu_w))
            out = Fx.dropout_add(_linear(a, self.down_w), z1, 0.0, rt.rng, 0)
        else:
            z1 = x2d + F.linear(actx, self.o_w)
            g, u = F.linear(ref_rms_norm(z1, self.n2_g, eps), self.gu_w).split(c.ffn_size, -1)
            out = z1 + F.linear(F.silu(g) * u, self.down_w)
        return out.view(B, Sq, h)

    # ------------------------------------------------------------------ reference path
    def _reference(self, x, key_range, doc_range, position_ids, table):
        c, rt = self.cfg, self.rt
        B, S, h = x.shape
        H, D = c.num_heads, c.head_dim
        tr = self.training
        p_a = c.attn_dropout if tr else 0.0
        if position_ids is None:
            cs = table[:S][None]
        else:
            cs = table[position_ids.to(device=x.device, dtype=torch.int64).clamp(0, table.shape[0] - 1)]
        a_in = ref_rms_norm(x, self.n1_g, c.ln_eps)
        Hkv = c.kv_heads
        if Hkv == H:
            qkv = F.linear(a_in, self.qkv_w).view(B, S, 3, H, D)
            q = _ref_rope(qkv[:, :, 0], cs).transpose(1, 2)
            k = _ref_rope(qkv[:, :, 1], cs).transpose(1, 2)
            v = qkv[:, :, 2].transpose(1, 2)
        else:    # grouped-query: K / V expanded to the query heads (HF repeat_kv)
            qkv = F.linear(a_in, self.qkv_w).view(B, S, H + 2 * Hkv, D)
            q = _ref_rope(qkv[:, :, :H], cs).transpose(1, 2)
            k = _ref_rope(qkv[:, :, H:H + Hkv], cs).transpose(1, 2).repeat_interleave(H // Hkv, 1)
            v = qkv[:, :, H + Hkv:].transpose(1, 2).repeat_interleave(H // Hkv, 1)
        s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
        if c.causal:
            s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
        if c.sliding_window:     # key j <= i - W lies behind query i's window
            s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=s.device).tril(-c.sliding_window), float("-inf"))
        if key_range is not None or doc_range is not None:
            outside = A._range_mask(key_range, B, S, s.device) if key_range is not None \
                else A._doc_mask(doc_range, B, S, s.device)
            s = s.masked_fill(outside, float("-inf"))
            # a row without a key (all -inf, softmax NaN) attends to nothing: probabilities 0
            dead = (s == float("-inf")).all(-1, keepdim=True)
            prob = torch.softmax(s.float().masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0).to(s.dtype)
        else:
            prob = torch.softmax(s.float(), -1).to(s.dtype)
        prob = ref_attn_dropout(prob, p_a, tr, rt, rt.rng.sid(self.sid_attn))
        ctx = torch.matmul(prob, v).transpose(1, 2).reshape(B, S, h)
        z1 = x + F.linear(ctx, self.o_w)
        f_in = ref_rms_norm(z1, self.n2_g, c.ln_eps)
        g, u = F.linear(f_in, self.gu_w).split(c.ffn_size, -1)
        return z1 + F.linear(F.silu(g) * u, self.down_w)


_dgrad = G.dgrad


def _linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Bias-free projection: the GEMM dispatch of ops/gemm.py on the GPU, F.linear on the CPU."""
    return G.linear_any(x, w) if x.is_cuda else F.linear(x, w)


def fused_attn_half_fwd(ctx, x, layer, key_range, doc_range, position_ids, table, qkv_w, o_w, g1, g2):
    """The attention half of the fused forward, apart from the FFN so that a layer with another FFN on the same
    attention half (the mixture-of-experts layer of models/moe.py, which has no fused path yet) can share it:
    x [B, S, h] -> (z1, f_in) with z1 = x + attention(RMS1(x)) and f_in = RMS2(z1), both [T, h], and the tensors
    its backward reads, which the caller saves in this order in front of its own.  The non-tensor state goes onto
    ``ctx``."""
    c, rt = layer.cfg, layer.rt
    B, S, h = x.shape
    H, D = c.num_heads, c.head_dim
    Hkv = c.kv_heads if c.kv_heads != H else None      # None: the multi-head kernels and layout
    T = B * S
    p_a = c.attn_dropout if layer.training else 0.0
    rng = rt.rng
    sa = rng.sid(layer.sid_attn)
    x2d = x.reshape(T, h)
    eps = c.ln_eps
    _, a_in, r1 = Fx.rms_fwd(None, x2d, g1, eps)
    qkv = _linear(a_in, qkv_w)
    Fx.rope_(qkv, table, B, S, H, D, pos=position_ids, kv_heads=Hkv)   # in place: the rotated qkv is what is kept
    actx, lse, amask = A.attn_fwd(qkv, B, S, H, D, c.causal, None, p_a, rng, sa,
                                  key_range=key_range, doc_range=doc_range, kv_heads=Hkv,
                                  window=c.sliding_window or None)
    o = _linear(actx, o_w)
    z1, f_in, r2 = Fx.rms_fwd(o, x2d, g2, eps)             # z1 = x + o and RMS2(z1) in one pass
    ctx.layer = layer
    ctx.amask = amask
    ctx.key_range, ctx.doc_range, ctx.position_ids, ctx.table = key_range, doc_range, position_ids, table
    ctx.rng = rng
    ctx.meta = (B, S, h, H, D, p_a, sa)
    ctx.kv_heads = Hkv
    return z1, f_in, (x2d, a_in, qkv, actx, lse, z1, f_in, r1, r2)


ATTN_HALF_SAVED = 9     # tensors fused_attn_half_fwd hands back for save_for_backward


def fused_bwd_begin(ctx, dout):
    """Start of a fused layer's backward: the step's batched weight transposes (first layer backward only) and
    dout as contiguous [T, h] rows."""
    layer = ctx.layer
    B, S, h = ctx.meta[:3]
    pend, layer.rt.pending_wt = layer.rt.pending_wt, None
    if pend:   # first layer backward of the step: every layer's W^T in one launch
        G.prepare_transposes(pend)
    return dout.reshape(B * S, h).contiguous()


def fused_attn_half_bwd(ctx, saved, dfin, dout, qkv_w, o_w, g1, g2):
    """The attention half of the fused backward: from dfin (f_in's gradient) and dout (z1 is also out's
    residual) down to dx [B, S, h]; ``saved`` as ``fused_attn_half_fwd`` returned it."""
    c, rng = ctx.layer.cfg, ctx.rng
    B, S, h, H, D, p_a, sa = ctx.meta
    x2d, a_in, qkv, actx, lse, z1, f_in, r1, r2 = saved
    # f_in = RMS2(z1) and z1 is also out's residual: dz1 = RMS2'(dfin) + dout; z1 = x + o, so dz1
    # is both o's gradient and the residual term of dx
    dz1 = Fx.rms_bwd(dfin, dout, z1, r2, g2, dgamma=grad_dst(g2))
    grad_done(g2)
    emit_wgrad(o_w, dz1, actx, async_ok=True)
    dctx = _dgrad(dz1, o_w)
    dqkv = A.attn_bwd(dctx, qkv, actx, lse, B, S, H, D, c.causal, None, p_a, rng, sa, ctx.amask,
                      key_range=ctx.key_range, doc_range=ctx.doc_range, kv_heads=ctx.kv_heads,
                      window=c.sliding_window or None)
    # the rotation's adjoint is its inverse: dqkv back in front of the rotary embedding
    Fx.rope_(dqkv, ctx.table, B, S, H, D, pos=ctx.position_ids, inverse=True, kv_heads=ctx.kv_heads)
    emit_wgrad(qkv_w, dqkv, a_in, async_ok=True)
    dain = _dgrad(dqkv, qkv_w)
    dx = Fx.rms_bwd(dain, dz1, x2d, r1, g1, dgamma=grad_dst(g1))
    grad_done(g1)
    return dx.view(B, S, h)


class _FusedLlamaLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layer: LlamaLayer, key_range, doc_range, position_ids, table, *params):
        rt = layer.rt
        (qkv_w, o_w, g1, gu_w, down_w, g2) = params
        B, S, h = x.shape
        z1, f_in, attn_saved = fused_attn_half_fwd(ctx, x, layer, key_range, doc_range, position_ids, table,
                                                   qkv_w, o_w, g1, g2)
        gu = _linear(f_in, gu_w)
        a = Fx.swiglu_fwd(gu)
        y = _linear(a, down_w)
        out = Fx.dropout_add(y, z1, 0.0, ctx.rng, 0)
        ctx.save_for_backward(*attn_saved, gu, a if rt.keep_ffn_act else None)
        return out.view(B, S, h)

    @staticmethod
    def backward(ctx, dout):
        (qkv_w, o_w, g1, gu_w, down_w, g2) = ctx.layer.params()
        dout = fused_bwd_begin(ctx, dout)
        saved = ctx.saved_tensors
        attn_saved, (gu, a) = saved[:ATTN_HALF_SAVED], saved[ATTN_HALF_SAVED:]
        f_in = attn_saved[6]
        # out = z1 + a down_w^T
        da = _dgrad(dout, down_w)
        if a is None:    # a = silu(gate) * up rewritten inside the SwiGLU backward pass
            dgu, a = Fx.swiglu_bwd(da, gu, want_act=True)
        else:
            dgu = Fx.swiglu_bwd(da, gu)
        del da
        emit_wgrad(down_w, dout, a, async_ok=True)
        del a
        emit_wgrad(gu_w, dgu, f_in, async_ok=True)
        dfin = _dgrad(dgu, gu_w)
        dx = fused_attn_half_bwd(ctx, attn_saved, dfin, dout, qkv_w, o_w, g1, g2)
        return (dx, None, None, None, None, None) + (None,) * 6


# ---------------------------------------------------------------------------------- HF weight conversion
_HF_LAYER = "model.layers.{i}."


def from_hf_state_dict(sd: dict) -> dict:
    """HF ``LlamaForCausalLM`` state dict -> ``CausalLM`` (Llama family) state dict: keys renamed,
    q/k/v and gate/up concatenated along the output rows -- a grouped-query checkpoint's k_proj / v_proj
    simply have fewer rows.  ``rotary_emb.inv_freq`` buffers of older checkpoints are dropped; a tied
    checkpoint (no ``lm_head.weight``) gets the embedding table.  An HF ``MistralForCausalLM`` state dict
    converts unchanged, here and in ``to_hf_state_dict``: its tensor names are Llama's, and the sliding
    window is a matter of the config (``sliding_window``), not of the weights.

    An HF ``MixtralForCausalLM`` state dict (models/moe.py) converts too: ``mlp.gate.weight [E, h]``,
    ``mlp.experts.gate_up_proj [E, 2f, h]`` and ``mlp.experts.down_proj [E, h, f]`` map one to one onto gate_w,
    gu_w and down_w; the older per-expert names ``block_sparse_moe.gate.weight`` and
    ``block_sparse_moe.experts.J.w1 / w3 / w2.weight`` (gate / up / down) are stacked into the same tensors."""
    out = {"embeddings.word": sd["model.embed_tokens.weight"],
           "final_ln.weight": sd["model.norm.weight"],
           "head.own_weight": sd["lm_head.weight"] if "lm_head.weight" in sd else sd["model.embed_tokens.weight"]}
    i = 0
    while _HF_LAYER.format(i=i) + "input_layernorm.weight" in sd:
        p, q = _HF_LAYER.format(i=i), f"layers.{i}."
        att, mlp = p + "self_attn.", p + "mlp."
        out[q + "qkv_w"] = torch.cat([sd[att + "q_proj.weight"], sd[att + "k_proj.weight"], sd[att + "v_proj.weight"]], 0)
        out[q + "o_w"] = sd[att + "o_proj.weight"]
        out[q + "n1_g"] = sd[p + "input_layernorm.weight"]
        old = p + "block_sparse_moe."
        if mlp + "experts.gate_up_proj" in sd:         # Mixtral, fused expert tensors
            out[q + "gate_w"] = sd[mlp + "gate.weight"]
            out[q + "gu_w"] = sd[mlp + "experts.gate_up_proj"]
            out[q + "down_w"] = sd[mlp + "experts.down_proj"]
        elif old + "gate.weight" in sd:                # Mixtral, one w1 (gate) / w3 (up) / w2 (down) per expert
            out[q + "gate_w"] = sd[old + "gate.weight"]
            ex = [old + f"experts.{j}." for j in range(out[q + "gate_w"].shape[0])]
            out[q + "gu_w"] = torch.stack([torch.cat([sd[e + "w1.weight"], sd[e + "w3.weight"]], 0) for e in ex])
            out[q + "down_w"] = torch.stack([sd[e + "w2.weight"] for e in ex])
        else:
            out[q + "gu_w"] = torch.cat([sd[mlp + "gate_proj.weight"], sd[mlp + "up_proj.weight"]], 0)
            out[q + "down_w"] = sd[mlp + "down_proj.weight"]
        out[q + "n2_g"] = sd[p + "post_attention_layernorm.weight"]
        if sd[att + "q_proj.weight"].shape[0] != out[q + "o_w"].shape[0] \
                or sd[att + "k_proj.weight"].shape[0] != sd[att + "v_proj.weight"].shape[0]:
            raise ValueError("q_proj must have as many rows as o_proj, and k_proj as many as v_proj")
        i += 1
    if i == 0:
        raise ValueError("not a Llama state dict: no model.layers.0.input_layernorm.weight")
    return out


def to_hf_state_dict(sd: dict) -> dict:
    """The inverse of ``from_hf_state_dict``: split qkv_w into q/k/v and gu_w into gate/up.  The split
    goes by sizes, so no config is needed: the q rows are as many as ``o_w``'s, the rest halves into k
    and v (fewer rows than q with grouped-query attention).  A mixture-of-experts layer (it has a ``gate_w``)
    is written under HF 5's fused Mixtral names."""
    out = {"model.embed_tokens.weight": sd["embeddings.word"], "model.norm.weight": sd["final_ln.weight"],
           "lm_head.weight": sd["head.own_weight"]}
    i = 0
    while f"layers.{i}.qkv_w" in sd:
        p, q = _HF_LAYER.format(i=i), f"layers.{i}."
        att, mlp = p + "self_attn.", p + "mlp."
        nq = sd[q + "o_w"].shape[0]
        nkv = (sd[q + "qkv_w"].shape[0] - nq) // 2
        qw, kw, vw = sd[q + "qkv_w"].split([nq, nkv, nkv], 0)
        if q + "gate_w" in sd:
            out[mlp + "gate.weight"] = sd[q + "gate_w"]
            out[mlp + "experts.gate_up_proj"], out[mlp + "experts.down_proj"] = sd[q + "gu_w"], sd[q + "down_w"]
        else:
            gw, uw = sd[q + "gu_w"].chunk(2, 0)
            out[mlp + "gate_proj.weight"], out[mlp + "up_proj.weight"] = gw, uw
            out[mlp + "down_proj.weight"] = sd[q + "down_w"]
        out[att + "q_proj.weight"], out[att + "k_proj.weight"], out[att + "v_proj.weight"] = qw, kw, vw
        out[att + "o_proj.weight"] = sd[q + "o_w"]
        out[p + "input_layernorm.weight"] = sd[q + "n1_g"]
        out[p + "post_attention_layernorm.weight"] = sd[q + "n2_g"]
        i += 1
    return out
