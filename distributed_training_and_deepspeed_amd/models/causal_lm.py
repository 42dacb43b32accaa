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

Generation (Llama family, dense FFN): ``generate`` / ``prefill`` / ``decode_step`` run the layers with a KV cache
(ops/kv_cache.py) -- the prompt once, then one token per step at a cost linear in the cache's fill.  Greedy or
temperature / top-k sampling; a left-padded batch through ``attention_mask``; optionally the step as a HIP graph.

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
from ..ops.kv_cache import KVCache
from ..utils.graphs import CAPTURE_ERROR_MODE
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

    # ------------------------------------------------------------------ incremental decoding (Llama family)
    def _check_generation(self) -> None:
        c = self.cfg
        if not c.llama_style or c.rope_theta <= 0:
            raise NotImplementedError(f"generation with a KV cache is implemented for the Llama family only, not "
                                      f"{c.family!r} (ALiBi and learned positions are out of scope)")
        if c.num_experts:
            raise NotImplementedError("generation with a KV cache does not cover mixture-of-experts models")
        # a ZeRO engine leaves its gradient-ready hook (a bound method of the engine) on every parameter
        for p in self.parameters():
            owner = getattr(getattr(p, "_dtd_ready_hook", None), "__self__", None)
            if type(owner).__name__ == "ZeroEngine":
                raise NotImplementedError("generation needs the whole weights: a ZeRO-wrapped model is not supported")

    @torch.no_grad()
    def prefill(self, input_ids: torch.Tensor, cache: KVCache, attention_mask: torch.Tensor | None = None) -> torch.Tensor:
        """The prompt ``input_ids [B, S0]`` into the EMPTY ``cache``; returns the logits ``[B, V]`` of the last
        position only (the head runs on B rows).  ``attention_mask``: HF's 0/1 mask of a LEFT-padded batch
        (a 0 after a 1 is a ``ValueError``; checked here, once, on the host); ``cache.kv_start`` becomes each
        sequence's first real position.  Rotary positions are the slots, arange(S0), as in ``forward``.
        Advances the cache by S0."""
        self._check_generation()
        B, S0 = input_ids.shape
        if cache.filled != 0:
            raise ValueError(f"prefill needs an empty cache, this one holds {cache.filled} positions (reset() it)")
        if B != cache.batch or S0 > cache.max_len or S0 == 0:
            raise ValueError(f"prefill: a [{B}, {S0}] prompt does not fit a cache of {cache.batch} sequences x "
                             f"{cache.max_len} positions")
        key_range = None
        if attention_mask is not None:
            if attention_mask.shape != input_ids.shape:
                raise ValueError(f"attention_mask must be {tuple(input_ids.shape)}, got {tuple(attention_mask.shape)}")
            keep = attention_mask != 0
            if bool((keep[:, :-1] & ~keep[:, 1:]).any()):
                raise ValueError("generation takes a left-padded attention_mask: a 0 follows a 1")
            key_range = key_range_from_mask(attention_mask)
            cache.kv_start.copy_(key_range[:, 0])
        x = self.embeddings(input_ids)
        for i, layer in enumerate(self.layers):
            x = layer.forward_cached(x, cache, i, True, key_range)
        cache.advance(S0)
        return self._last_logits(x[:, -1])

    @torch.no_grad()
    def decode_step(self, tokens: torch.Tensor, cache: KVCache) -> torch.Tensor:
        """One new token per sequence, ``tokens [B]``, on top of a prefilled ``cache``: the logits ``[B, V]`` of
        the next position.  Advances the cache by one.  No host synchronisation: the position is the
        cache's device counters, so the launch sequence is the same at every step."""
        if cache.filled == 0:      # (what generation supports was checked by the prefill that filled it)
            raise ValueError("decode_step needs a prefilled cache")
        if cache.filled + 1 > cache.max_len:
            raise ValueError(f"the cache is full ({cache.max_len} positions)")
        x = self.embeddings(tokens.view(cache.batch, 1))
        for i, layer in enumerate(self.layers):
            x = layer.forward_cached(x, cache, i, False)
        cache.advance(1)
        return self._last_logits(x[:, 0])

    def _last_logits(self, x: torch.Tensor) -> torch.Tensor:
        if self.final_ln is not None:
            x = self.final_ln(x)
        return self.head.logits(x)

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int, attention_mask: torch.Tensor | None = None,
                 do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, eos_token_id: int | None = None,
                 seed: int = 0, max_len: int | None = None, graph: bool = False,
                 logits_out: list | None = None, kv_dtype=None, cache_out: list | None = None) -> torch.Tensor:
        """``input_ids [B, S0]`` continued by ``max_new_tokens`` = N tokens: int64 ``[B, S0 + N]``.  Greedy by
        default; ``do_sample``: temperature, then top-k (0 = the whole vocabulary), drawn with a
        ``torch.Generator`` seeded with ``seed``.  ``attention_mask``: a LEFT-padded batch (``prefill``).  After
        a sequence emits ``eos_token_id`` it emits ``cfg.pad_token_id``; all N steps always run, so no step
        waits for the host.  ``max_len``: cache positions (default S0 + N; at most ``cfg.max_positions``).  The
        model is put in eval mode for the call and its mode is restored.

        ``graph=True`` (GPU): after two eager steps ``decode_step`` is captured once into a HIP graph -- one
        stream, the token a static input -- and replayed; the token selection stays outside the graph.
        ``logits_out``: a list that receives each step's ``[B, V]`` logits (tests).

        ``kv_dtype``: ``"fp8"`` (or ``torch.float8_e4m3fn``) keeps the cache as e4m3fn codes with one fp32 scale per
        row (``KVCache.allocate``): half the bytes and half the decode kernel's traffic, at the quantisation's
        error -- a greedy token may differ from the unquantised cache's.  None: the cache in the model's dtype.
        ``cache_out``: a list that receives the call's ``KVCache`` (tests)."""
        self._check_generation()
        B, S0 = input_ids.shape
        N = int(max_new_tokens)
        max_len = S0 + N if max_len is None else int(max_len)
        if N < 0 or S0 + N > max_len:
            raise ValueError(f"generate: prompt {S0} + {N} new tokens exceed max_len = {max_len}")
        if do_sample and temperature <= 0:
            raise ValueError(f"temperature must be positive, got {temperature}")
        w = self.head.weight
        dev = w.device
        input_ids = input_ids.to(dev)
        if attention_mask is not None:
            attention_mask = attention_mask.to(dev)
        cache = KVCache.allocate(self.cfg, B, max_len, dev, w.dtype, kv_dtype=kv_dtype)
        if cache_out is not None:
            cache_out.append(cache)
        gen = torch.Generator(device=dev).manual_seed(seed) if do_sample else None
        graph = bool(graph) and dev.type == "cuda"
        was_training = self.training
        self.eval()
        try:
            out = [input_ids.to(torch.int64)]
            done = torch.zeros(B, dtype=torch.bool, device=dev)
            logits = self.prefill(input_ids, cache, attention_mask) if N > 0 else None
            captured = static_tok = None
            for t in range(N):
                if logits_out is not None:
                    logits_out.append(logits.clone())
                tok = self._select(logits, do_sample, temperature, top_k, gen)
                if eos_token_id is not None:
                    tok = torch.where(done, torch.full_like(tok, self.cfg.pad_token_id), tok)
                    done = done | (tok == eos_token_id)
                out.append(tok.view(B, 1))
                if t == N - 1:
                    break
                if graph and t >= 2:
                    if captured is None:
                        static_tok = tok.clone()
                        torch.cuda.synchronize()
                        captured = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(captured, capture_error_mode=CAPTURE_ERROR_MODE):
                            static_logits = self.decode_step(static_tok, cache)
                        cache.filled -= 1          # the capture computed nothing: only replays advance
                    static_tok.copy_(tok)
                    captured.replay()
                    cache.filled += 1
                    logits = static_logits
                else:
                    logits = self.decode_step(tok, cache)
            if captured is not None:
                torch.cuda.synchronize()
                captured.reset()
            return torch.cat(out, 1)
        finally:
            self.train(was_training)

    @staticmethod
    def _select(logits, do_sample, temperature, top_k, gen) -> torch.Tensor:
        if not do_sample:
            return logits.argmax(-1)
        z = logits.float() / temperature
        if top_k and top_k < z.shape[-1]:
            z = z.masked_fill(z < z.topk(top_k, -1).values[:, -1:], float("-inf"))
        return torch.multinomial(torch.softmax(z, -1), 1, generator=gen).view(-1)
