"""Synthetic token datasets with the reference's schema and masking law.

The reference tokenizes wikitext-2 (util.py:38-60): rows padded/truncated to 512 tokens, then
either *static* MLM masking via HF DataCollatorForLanguageModeling.torch_mask_tokens
(p = 0.15 over non-special tokens; of those 80% -> [MASK], 10% -> random token, 10% kept;
unmasked labels -100 -- SURVEY.md D19) or causal labels = input_ids (pads included).
There is no network on the MI355X boxes, so rows here are random token ids with the same
shape, framing ([CLS] ... [SEP] for BERT) and the same masking law, generated
deterministically from a seed.  ``pad_fraction`` optionally right-pads rows with the pad id
to mimic short wikitext lines; ``return_attention_mask=True`` adds the matching 0/1
``attention_mask`` column (ones over each row's drawn length), which the models turn into key
ranges so the pads are not attended to.  ``max_docs > 0`` packs rows instead: each row is cut into
1 to ``max_docs`` documents of random lengths (each framed [CLS] ... [SEP] for BERT) and a
``segment_ids`` column (0 = padding, 1, 2, ... per document) is added -- data/packing.py.
"""
from __future__ import annotations

import torch
from torch.utils.data import Dataset

from ..models.config import TransformerConfig
from .packing import packed_causal_labels

IGNORE_INDEX = -100


def mlm_mask_tokens(input_ids: torch.Tensor, special_mask: torch.Tensor, vocab_size: int, mask_token_id: int,
                    generator: torch.Generator, mlm_probability: float = 0.15):
    """HF ``torch_mask_tokens`` law.  Returns (masked inputs, labels)."""
    labels = input_ids.clone()
    prob = torch.full(labels.shape, mlm_probability)
    prob.masked_fill_(special_mask, 0.0)
    masked = torch.bernoulli(prob, generator=generator).bool()
    labels[~masked] = IGNORE_INDEX
    inputs = input_ids.clone()
    replaced = torch.bernoulli(torch.full(labels.shape, 0.8), generator=generator).bool() & masked
    inputs[replaced] = mask_token_id
    rnd = torch.bernoulli(torch.full(labels.shape, 0.5), generator=generator).bool() & masked & ~replaced
    inputs[rnd] = torch.randint(vocab_size, labels.shape, dtype=inputs.dtype, generator=generator)[rnd]
    return inputs, labels


def synthetic_token_rows(n: int, seq_len: int, cfg: TransformerConfig, generator: torch.Generator,
                         pad_fraction: float = 0.0):
    """Random rows (+ special-token mask).  BERT rows are framed [CLS] x ... x [SEP]."""
    ids, special, _ = synthetic_token_rows_lengths(n, seq_len, cfg, generator, pad_fraction)
    return ids, special


def synthetic_token_rows_lengths(n: int, seq_len: int, cfg: TransformerConfig, generator: torch.Generator,
                                 pad_fraction: float = 0.0):
    """``synthetic_token_rows`` plus each row's length before padding ([n] int64; ``seq_len`` for
    an unpadded row).  Same draws from ``generator``, so the rows are the same."""
    row_len = torch.full((n,), seq_len, dtype=torch.int64)
    specials = set(cfg.special_token_ids)
    lo = max(specials) + 1 if cfg.family == "bert" and specials else 0
    lo = min(lo, cfg.vocab_size - 1)
    ids = torch.randint(lo, cfg.vocab_size, (n, seq_len), generator=generator, dtype=torch.int64)
    if cfg.family == "bert":
        ids[:, 0] = 101
        ids[:, -1] = 102
    if pad_fraction > 0:
        lengths = torch.randint(2, seq_len + 1, (n,), generator=generator)
        padded = torch.rand(n, generator=generator) < pad_fraction
        for i in torch.nonzero(padded).flatten().tolist():
            L = int(lengths[i])
            row_len[i] = L
            if cfg.family == "bert":
                ids[i, L - 1] = 102
            # (a shrunken-vocabulary preset may keep its family's pad id: stay inside the table)
            ids[i, L:] = cfg.pad_token_id if cfg.pad_token_id < cfg.vocab_size else 0
    special = torch.zeros_like(ids, dtype=torch.bool)
    for s in specials:
        special |= ids == s
    return ids, special, row_len


def cut_into_documents(ids: torch.Tensor, row_len: torch.Tensor, cfg: TransformerConfig, max_docs: int,
                       generator: torch.Generator) -> torch.Tensor:
    """Cut the first ``row_len[i]`` tokens of every row into 1 to ``max_docs`` documents of random
    lengths (at least 2 tokens each) and frame each as [CLS] ... [SEP] for BERT, in place.  Returns
    the ``segment_ids`` ([n, seq_len] int64: 1, 2, ... per document, 0 over the padded tail)."""
    n, S = ids.shape
    seg = torch.zeros((n, S), dtype=torch.int64)
    want = torch.randint(1, max_docs + 1, (n,), generator=generator)
    for i in range(n):
        L = int(row_len[i])
        # distinct random cut points, kept when they leave 2 tokens on either side
        cand = (torch.randperm(max(L - 3, 0), generator=generator)[: int(want[i]) - 1] + 2).sort().values.tolist()
        cuts = [0]
        for c in cand:
            if c - cuts[-1] >= 2 and L - c >= 2:
                cuts.append(c)
        cuts.append(L)
        for d, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            seg[i, lo:hi] = d + 1
            if cfg.family == "bert":
                ids[i, lo] = 101
                ids[i, hi - 1] = 102
    return seg


class SyntheticLMDataset(Dataset):
    """Map-style dataset of {'input_ids', 'labels'} rows, statically masked like util.py.
    ``return_attention_mask=True`` adds an 'attention_mask' column: a prefix of ones of each row's
    drawn length (not ``ids != pad``: a random token can equal the pad id)."""

    attention_mask = None   # [n, seq_len] int64 0/1 when requested
    segment_ids = None      # [n, seq_len] int64 document ids of packed rows (max_docs > 0)

    def __init__(self, cfg: TransformerConfig, num_samples: int, seq_len: int = 512, mlm: bool | None = None,
                 seed: int = 0, pad_fraction: float = 0.0, return_attention_mask: bool = False, max_docs: int = 0):
        """``max_docs > 0``: packed rows (module docstring) with a 'segment_ids' column.  Causal
        labels are then -100 on every document's first token and on pads, so that after the head's
        shift no position predicts across a boundary; MLM labels follow the unchanged masking law,
        every document's [CLS] / [SEP] exempt.  ``max_docs = 0`` draws exactly the rows it always did."""
        self.cfg = cfg
        self.mlm = (cfg.family == "bert") if mlm is None else mlm
        g = torch.Generator().manual_seed(seed)
        ids, special, row_len = synthetic_token_rows_lengths(num_samples, seq_len, cfg, g, pad_fraction)
        if return_attention_mask:
            self.attention_mask = (torch.arange(seq_len).view(1, -1) < row_len.view(-1, 1)).to(torch.int64)
        if max_docs > 0:
            self.segment_ids = cut_into_documents(ids, row_len, cfg, max_docs, g)
            special = torch.zeros_like(ids, dtype=torch.bool)
            for s in set(cfg.special_token_ids):
                special |= ids == s
        if self.mlm:
            self.input_ids, self.labels = mlm_mask_tokens(ids, special, cfg.vocab_size, cfg.mask_token_id, g)
        elif max_docs > 0:
            self.input_ids, self.labels = ids, packed_causal_labels(ids, self.segment_ids)
        else:
            self.input_ids, self.labels = ids, ids.clone()  # util.py:54-58: pads included

    def __len__(self):
        return self.input_ids.shape[0]

    def __getitem__(self, i):
        row = {"input_ids": self.input_ids[i], "labels": self.labels[i]}
        if self.attention_mask is not None:
            row["attention_mask"] = self.attention_mask[i]
        if self.segment_ids is not None:
            row["segment_ids"] = self.segment_ids[i]
        return row

    def select(self, indices) -> "SyntheticLMDataset":
        """HF ``Dataset.select`` parity (data_parallel_training.py:36)."""
        idx = torch.as_tensor(list(indices), dtype=torch.int64)
        out = object.__new__(SyntheticLMDataset)
        out.cfg, out.mlm = self.cfg, self.mlm
        out.input_ids, out.labels = self.input_ids[idx], self.labels[idx]
        out.attention_mask = None if self.attention_mask is None else self.attention_mask[idx]
        out.segment_ids = None if self.segment_ids is None else self.segment_ids[idx]
        return out


def load_synthetic(cfg: TransformerConfig, num_samples: int, seq_len: int = 512, mlm: bool | None = None,
                   seed: int = 0, pad_fraction: float = 0.0, return_attention_mask: bool = False,
                   max_docs: int = 0) -> SyntheticLMDataset:
    """Stand-in for ``util.load_wikitext`` (same columns, same masking law)."""
    return SyntheticLMDataset(cfg, num_samples, seq_len, mlm=mlm, seed=seed, pad_fraction=pad_fraction,
                              return_attention_mask=return_attention_mask, max_docs=max_docs)


class NativeSyntheticLM:
    """On-demand synthetic rows (no materialised dataset): row ``i`` of the stream ``seed`` is
    generated by the native worker pool (``runtime/csrc/loader.cpp``) with the same schema and
    masking law as ``SyntheticLMDataset`` -- [CLS] x ... x [SEP] BERT framing, HF static MLM
    masking (15 % of non-special tokens; 80 % [MASK], 10 % random, 10 % kept; labels -100
    elsewhere) or causal labels = ids -- from a counter-based hash of (seed, row, position), so
    any rank / worker / resume point reproduces the same row.  Works with ``DistributedSampler``
    and ``DeviceBatchLoader`` (which calls ``fill_rows`` into its pinned slots)."""

    keys = ("input_ids", "labels")

    def __init__(self, cfg: TransformerConfig, num_samples: int, seq_len: int = 512, mlm: bool | None = None,
                 seed: int = 0):
        self.cfg, self.num_samples, self.seq_len, self.seed = cfg, int(num_samples), int(seq_len), int(seed)
        self.mlm = (cfg.family == "bert") if mlm is None else mlm
        self._producer = None

    def __len__(self):
        return self.num_samples

    def row_shape(self, key):
        return (self.seq_len,)

    def row_dtype(self, key):
        return torch.int64

    def _pool(self):
        if self._producer is None:
            from ..runtime import BatchProducer
            self._producer = BatchProducer()
        return self._producer

    def fill_rows(self, idx: torch.Tensor, out: dict, producer=None) -> None:
        """Generate rows ``idx`` into out['input_ids'] / out['labels'] ([n, seq] int64, CPU)."""
        producer = producer or self._pool()
        idx = torch.as_tensor(idx, dtype=torch.int64).flatten()
        ids, lab = out["input_ids"], out["labels"]
        n = idx.numel()
        if n == 0:
            return
        # consecutive runs are generated in place; scattered indices row by row
        runs, start = [], 0
        for i in range(1, n + 1):
            if i == n or int(idx[i]) != int(idx[i - 1]) + 1:
                runs.append((start, i))
                start = i
        jobs = [producer.synthesize(self.cfg, self.seed, int(idx[a]), ids[a:b], lab[a:b], mlm=self.mlm, wait=False)
                for a, b in runs]
        for j in jobs:
            producer.wait(j)

    def __getitem__(self, i):
        ids = torch.empty((1, self.seq_len), dtype=torch.int64)
        lab = torch.empty_like(ids)
        self.fill_rows(torch.tensor([i]), {"input_ids": ids, "labels": lab})
        return {"input_ids": ids[0], "labels": lab[0]}

    def batch(self, row0: int, n: int):
        ids = torch.empty((n, self.seq_len), dtype=torch.int64)
        lab = torch.empty_like(ids)
        self.fill_rows(torch.arange(row0, row0 + n), {"input_ids": ids, "labels": lab})
        return ids, lab
