"""Decoder-only causal LMs (HF ``AutoModelForCausalLM`` equivalents, random init).

Reference usage: ``AutoModelForCausalLM.from_pretrained('bigscience/bloom-560m')`` with
``model(input_ids, labels=labels).loss`` (zero_dp_training.py:24,85); the multi-node script
intends ``facebook/opt-125m`` (scripts/launch-multinode.sh:5) and BASELINE.json names
gpt2-medium.  SURVEY.md D17:
  * BLOOM: word embeddings -> embedding LN, pre-LN blocks with fused QKV, ALiBi, tanh-GELU,
    final LN, tied LM head, vocab 250,880 (559,214,592 parameters for bloom-560m);
  * OPT: word + learned positions (offset 2), pre-LN, ReLU, final LN, tied head;
  * GPT-2: wte + wpe, pre-LN, tanh-GELU, final LN, tied head;
  * Llama (models/llama.py): word embeddings only, RMSNorm blocks with rotary q / k and a SwiGLU MLP, no
    biases, final RMSNorm, untied head.  Rotary positions are arange(S), also under ``attention_mask``
    (as HF's; rotary attention depends only on position differences), and restart at each document
    with ``segment_ids``;
  * Mixtral (models/moe.py, ``cfg.num_experts > 0``): the Llama layer with a routed mixture-of-experts FFN.
    ``loss`` then includes ``cfg.router_aux_loss_coef * aux_loss``, ``aux_loss`` being the mean over the layers
    of their load-balancing losses (every position counts, pads included); ``output_router_logits=True`` also
    returns each layer's [T, E] router logits (HF's name).
Loss: shifted next-token cross entropy (labels = input_ids, ignore_index -100).

``forward(..., attention_mask=...)`` takes HF's 0/1 ``[B, S]`` key-padding mask (contiguous: left-
or right-padded, ``ops.attention.key_range_from_mask``); without it pads are attended to, as in the
reference.  Position ids stay ``arange(S)``: equal to HF's for right-padded batches, and for BLOOM
(ALiBi, no position table) under either padding side.  For a LEFT-padded OPT or GPT-2 batch HF
derives the positions from the mask (first real token = position 0); here they are not shifted.

``forward(..., segment_ids=...)`` takes a packed batch instead (integer ``[B, S]``, 0 = padding, one
non-zero id per contiguous document, ``ops.attention.doc_range_from_segment_ids``): attention is
causal inside each document, the learned positions of OPT / GPT-2 restart at each document (BLOOM's
ALiBi keeps absolute key positions: a per-row constant the softmax cancels), and it excludes
``attention_mask``.  The loss does not cross a boundary when the labels of every document's first
token are -100 (data/synthetic.py, data/text.py write them so): the head's shift then leaves no
position predicting the next document.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from .config import BLOOM_560M, TransformerConfig, get_config
from .layers import Embeddings, LayerNorm, LMHead, RMSNorm
from .llama import LlamaLayer
from .moe import MoeLlamaLayer
from ..ops.attention import doc_position_ids, doc_range_from_segment_ids, key_range_from_mask
from .transformer import Runtime, TransformerLayer, prefetch_masks, stage_dgrad_transposes


@dataclass
class CausalLMOutput:
    loss: torch.Tensor | None = None
    logits: torch.Tensor | None = None
    aux_loss: torch.Tensor | None = None          # mixture-of-experts models: mean load-balancing loss of the layers
    router_logits: tuple | None = None            # with output_router_logits: one [T, E] tensor per layer


class CausalLM(nn.Module):
    def __init__(self, cfg: TransformerConfig = BLOOM_560M, rt: Runtime | None = None):
        super().__init__()
        self.config = self.cfg = cfg
        self.rt = rt or Runtime()
        self.embeddings = Embeddings(cfg, self.rt)
        layer_cls = (MoeLlamaLayer if cfg.num_experts else LlamaLayer) if cfg.llama_style else TransformerLayer
        norm_cls = RMSNorm if cfg.norm == "rms" else LayerNorm
        self.layers = nn.ModuleList([layer_cls(cfg, self.rt) for _ in range(cfg.num_layers)])
        self.final_ln = norm_cls(cfg.hidden_size, cfg.ln_eps, self.rt) if cfg.final_ln else None
        self.head = LMHead(cfg, self.rt, self.embeddings.word)

    @classmethod
    def from_config(cls, name: str, **kw) -> "CausalLM":
        return cls(get_config(name), **kw)

    def zero3_units(self):
        """Parameter-gathering units for ZeRO-3, in forward order."""
        return [self.embeddings, *self.layers] + ([self.final_ln] if self.final_ln is not None else [])

    def zero3_persistent(self):
        """Parameters outside the gathered units: the word embeddings the tied LM head shares, or the
        untied head's own weight (Llama family) -- replicated, with stage-2 treatment of its gradient."""
        return [self.embeddings.word] if self.head.own_weight is None else [self.head.own_weight]

    def encode(self, input_ids: torch.Tensor, attention_mask: torch.Tensor | None = None,
               segment_ids: torch.Tensor | None = None) -> torch.Tensor:
        if attention_mask is not None and segment_ids is not None:
            raise ValueError("attention_mask and segment_ids are mutually exclusive (segment id 0 marks padding)")
        if input_ids.is_cuda and self.training:
            prefetch_masks(self.layers, input_ids)
        # one conversion per forward (on the device, no host sync); every layer gets the ranges
        key_range = key_range_from_mask(attention_mask) if attention_mask is not None else None
        doc_range = position_ids = None
        if segment_ids is not None:
            if segment_ids.shape != input_ids.shape:
                raise ValueError(f"segment_ids must be {tuple(input_ids.shape)}, got {tuple(segment_ids.shape)}")
            doc_range = doc_range_from_segment_ids(segment_ids)
            position_ids = doc_position_ids(doc_range)      # restart at every document; pads take 0
        if self.cfg.rope_theta > 0 and input_ids.shape[1] > self.cfg.max_positions:
            raise ValueError(f"sequence length {input_ids.shape[1]} exceeds max_positions {self.cfg.max_positions} "
                             f"(the rotary table)")
        x = self.embeddings(input_ids) if position_ids is None else self.embeddings(input_ids, position_ids=position_ids)
        # rotary positions restart at each document (one int32 copy serves every layer); arange(S)
        # otherwise, also under a key-padding mask: rotary attention sees only position differences
        rope_pos = position_ids.to(torch.int32) if self.cfg.rope_theta > 0 and doc_range is not None else None
        for layer in self.layers:
            if rope_pos is not None:
                x = layer(x, doc_range=doc_range, position_ids=rope_pos)
            elif doc_range is not None:
                x = layer(x, doc_range=doc_range)
            else:
                x = layer(x) if key_range is None else layer(x, key_range=key_range)
        stage_dgrad_transposes(self.layers, x)
        if self.final_ln is not None:
            x = self.final_ln(x)
        return x

    def forward(self, input_ids: torch.Tensor, labels: torch.Tensor | None = None,
                return_logits: bool = False, attention_mask: torch.Tensor | None = None,
                segment_ids: torch.Tensor | None = None, output_router_logits: bool = False) -> CausalLMOutput:
        x = self.encode(input_ids, attention_mask, segment_ids)
        out = CausalLMOutput()
        if labels is not None:
            out.loss = self.head(x, labels)
        if self.cfg.num_experts:
            out.aux_loss = torch.stack([layer.aux_loss for layer in self.layers]).mean()
            if out.loss is not None and self.cfg.router_aux_loss_coef:
                out.loss = out.loss + self.cfg.router_aux_loss_coef * out.aux_loss
            if output_router_logits:
                out.router_logits = tuple(layer.router_logits for layer in self.layers)
        if labels is None or return_logits:
            out.logits = self.head.logits(x)
        return out
