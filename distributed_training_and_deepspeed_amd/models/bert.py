"""BERT for masked-LM pre-training (HF ``BertForMaskedLM`` equivalent, random init).

Reference usage: ``BertForMaskedLM.from_pretrained('bert-base-cased'|'bert-large-cased')`` and
``model(input_ids, labels=...).loss`` (data_parallel_training.py:30-31,53-54).  Architecture
per SURVEY.md D15: word+position+token-type embeddings -> LN(1e-12) -> dropout 0.1;
N post-LN encoder layers (fused q/k/v projection: identical parameter count to HF's three
Linears); MLM head dense -> GELU(erf) -> LN -> decoder tied to the word embeddings + bias;
cross entropy with ignore_index -100 over all labelled positions.  By default no attention mask
is applied (the reference never passes one, so pads are attended to); ``forward(...,
attention_mask=...)`` takes HF's 0/1 ``[B, S]`` key-padding mask of a left- or right-padded batch
(contiguous masks only, ``ops.attention.key_range_from_mask``).  Position ids stay ``arange(S)``,
which equals HF's for right-padded batches.  ``forward(..., segment_ids=...)`` takes a packed
batch instead (integer ``[B, S]``, 0 = padding, one non-zero id per contiguous document,
``ops.attention.doc_range_from_segment_ids``): attention stays inside each document and the learned
positions restart at each one; it excludes ``attention_mask``.  There is no pooler (add_pooling_layer=False).
Parameter count for bert-base-cased: 108,340,804.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from .config import BERT_BASE, TransformerConfig, get_config
from .layers import Embeddings, MLMHead
from ..ops.attention import doc_position_ids, doc_range_from_segment_ids, key_range_from_mask
from .transformer import Runtime, TransformerLayer, prefetch_masks, stage_dgrad_transposes


@dataclass
class MaskedLMOutput:
    loss: torch.Tensor | None = None
    logits: torch.Tensor | None = None


class BertForMaskedLM(nn.Module):
    def __init__(self, cfg: TransformerConfig = BERT_BASE, rt: Runtime | None = None, sparse_mlm_head: bool = True):
        super().__init__()
        self.config = self.cfg = cfg
        self.rt = rt or Runtime()
        self.embeddings = Embeddings(cfg, self.rt)
        self.layers = nn.ModuleList([TransformerLayer(cfg, self.rt) for _ in range(cfg.num_layers)])
        self.head = MLMHead(cfg, self.rt, self.embeddings.word, sparse=sparse_mlm_head)

    @classmethod
    def from_config(cls, name: str, **kw) -> "BertForMaskedLM":
        return cls(get_config(name), **kw)

    def zero3_units(self):
        """Parameter-gathering units for ZeRO-3, in forward order."""
        return [self.embeddings, *self.layers, self.head]

    def zero3_persistent(self):
        """Parameters shared between units (tied decoder / word embeddings)."""
        return [self.embeddings.word] if self.head.decoder_w is None else []

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
        x = self.embeddings(input_ids) if position_ids is None else self.embeddings(input_ids, position_ids=position_ids)
        for layer in self.layers:
            if doc_range is not None:
                x = layer(x, doc_range=doc_range)
            else:
                x = layer(x) if key_range is None else layer(x, key_range=key_range)
        stage_dgrad_transposes(self.layers, x)
        return x

    def forward(self, input_ids: torch.Tensor, labels: torch.Tensor | None = None,
                return_logits: bool = False, attention_mask: torch.Tensor | None = None,
                segment_ids: torch.Tensor | None = None) -> MaskedLMOutput:
        x = self.encode(input_ids, attention_mask, segment_ids)
        out = MaskedLMOutput()
        if labels is not None:
            out.loss = self.head(x, labels)
        if labels is None or return_logits:
            out.logits = self.head(x)   # module call: ZeRO-3 / staged-optimizer hooks fire
        return out
