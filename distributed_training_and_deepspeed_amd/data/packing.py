"""Sequence packing: several documents share a row instead of each being padded to the row length.

``pack_documents`` lays token lists out into ``[rows, seq_len]`` ids plus the matching
``segment_ids`` (0 = padding, documents numbered 1, 2, ... inside their row) that the models'
``segment_ids=`` argument takes: attention stays inside each document, learned positions restart at
each one, and -- with ``packed_causal_labels`` -- no position predicts across a boundary.
"""
from __future__ import annotations

import torch

IGNORE_INDEX = -100


def pack_documents(docs, seq_len: int, pad_id: int):
    """Greedy first-fit packing, in order: every document goes into the first row that still has
    room for all of it, or opens a new row; a document longer than ``seq_len`` is truncated to it.
    Empty documents are dropped.  Returns ``(input_ids, segment_ids)``, int64 ``[rows, seq_len]``.
    The layout depends on the documents' lengths only."""
    if seq_len <= 0:
        raise ValueError("seq_len must be positive")
    rows: list[list] = []       # per row: its (document, start) pairs
    used: list[int] = []
    for d in docs:
        d = list(d)[:seq_len]
        if not d:
            continue
        for r, u in enumerate(used):
            if u + len(d) <= seq_len:
                break
        else:
            r = len(used)
            used.append(0)
            rows.append([])
        rows[r].append((d, used[r]))
        used[r] += len(d)
    ids = torch.full((len(rows), seq_len), int(pad_id), dtype=torch.int64)
    seg = torch.zeros((len(rows), seq_len), dtype=torch.int64)
    for r, row in enumerate(rows):
        for n, (d, start) in enumerate(row):
            ids[r, start:start + len(d)] = torch.as_tensor(d, dtype=torch.int64)
            seg[r, start:start + len(d)] = n + 1
    return ids, seg


def document_starts(segment_ids: torch.Tensor) -> torch.Tensor:
    """[B, S] bool: the first token of every document."""
    prev = torch.nn.functional.pad(segment_ids[:, :-1], (1, 0), value=0)
    return (segment_ids != 0) & (segment_ids != prev)


def packed_causal_labels(input_ids: torch.Tensor, segment_ids: torch.Tensor) -> torch.Tensor:
    """Next-token labels of a packed batch: the ids, with -100 on every document's first token and
    on pads.  The LM head shifts the labels by one, so the last token of a document (and a pad)
    predicts nothing, and no position predicts the first token of the following document."""
    labels = input_ids.clone()
    labels[document_starts(segment_ids) | (segment_ids == 0)] = IGNORE_INDEX
    return labels
