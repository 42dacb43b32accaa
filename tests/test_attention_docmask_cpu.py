"""Sequence packing, the CPU side: ``doc_range_from_segment_ids``, the math reference with
document spans against a brute-force fp64 ``same_doc & causal`` mask, ``pack_documents``, the
packed dataset columns and label rules, ``load_wikitext(pack=True)``, the reference-path models on
a packed batch against the same documents run as separate sequences, and the scripts' ``--pack-docs``."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_and_deepspeed_amd.data import (SyntheticLMDataset, load_wikitext, pack_documents,
                                                          packed_causal_labels)
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops.rng import RngState, attn_keep_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ doc_range_from_segment_ids
def test_doc_range_from_segment_ids_hand_written_rows():
    seg = torch.tensor([
        [0, 0, 3, 3, 3, 7, 0, 2, 2, 0],      # front, middle and tail pads; a one-token document
        [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],      # all pads
        [5, 5, 5, 5, 5, 5, 5, 5, 5, 5],      # one document
        [1, 2, 2, 4, 4, 4, 4, 4, 4, 9],      # back to back, one-token documents at both ends
    ])
    d = A.doc_range_from_segment_ids(seg, check=True)
    assert d.ranges.dtype == torch.int32 and d.ranges.shape == (4, 10, 2) and d.blocks.shape == (4, 1, 2)
    assert d.flat.is_contiguous() and d.flat.numel() == 2 * 4 * (10 + 1)
    Z = [0, 0]
    assert d.ranges.tolist() == [
        [Z, Z, [2, 5], [2, 5], [2, 5], [5, 6], Z, [7, 9], [7, 9], Z],
        [Z] * 10,
        [[0, 10]] * 10,
        [[0, 1], [1, 3], [1, 3]] + [[3, 9]] * 6 + [[9, 10]],
    ]
    assert d.blocks.tolist() == [[[2, 9]], [[0, 0]], [[0, 10]], [[0, 10]]]
    assert A.doc_position_ids(d).tolist() == [
        [0, 0, 0, 1, 2, 0, 0, 0, 1, 0], [0] * 10, list(range(10)), [0, 0, 1, 0, 1, 2, 3, 4, 5, 0]]
    # int32 ids give the same spans; the views alias the flat buffer the kernels read
    assert torch.equal(A.doc_range_from_segment_ids(seg.to(torch.int32)).flat, d.flat)
    assert d.ranges.data_ptr() == d.flat.data_ptr()


def test_doc_block_bounds_per_128_positions():
    S = 300
    seg = torch.zeros(2, S, dtype=torch.int64)
    seg[0, 10:140] = 1
    seg[0, 140:200] = 2          # block 1 holds the end of document 1 and all of 2; block 2 is all pads
    seg[1, 260:300] = 4          # blocks 0 and 1 all pads
    d = A.doc_range_from_segment_ids(seg)
    assert d.blocks.tolist() == [[[10, 140], [10, 200], [0, 0]], [[0, 0], [0, 0], [260, 300]]]
    # bare spans get the same bounds
    assert torch.equal(A._doc_pack(d.ranges.clone()).flat, d.flat)


def test_doc_range_check_raises_on_a_reappearing_id():
    seg = torch.tensor([[1, 1, 2, 2, 1, 1, 0, 0]])
    assert A.doc_range_from_segment_ids(seg).ranges[0, 4].tolist() == [4, 6]     # unchecked: a run of its own
    with pytest.raises(ValueError):
        A.doc_range_from_segment_ids(seg, check=True)
    with pytest.raises(ValueError):                                              # ... also after a pad
        A.doc_range_from_segment_ids(torch.tensor([[3, 3, 0, 3]]), check=True)
    with pytest.raises(ValueError):
        A.doc_range_from_segment_ids(torch.ones(2, 4))                           # float ids
    A.doc_range_from_segment_ids(torch.tensor([[1, 1, 2, 2], [2, 2, 1, 1]]), check=True)   # per row, fine


def test_key_range_and_doc_range_are_exclusive():
    B, S, H, D = 1, 8, 1, 8
    qkv = torch.randn(B * S, 3 * H * D)
    kr = torch.tensor([[0, S]], dtype=torch.int32)
    dr = A.doc_range_from_segment_ids(torch.ones(B, S, dtype=torch.int64))
    with pytest.raises(ValueError):
        A.attn_fwd(qkv, B, S, H, D, key_range=kr, doc_range=dr)
    with pytest.raises(ValueError):
        A.attn_fwd_ref(qkv, B, S, H, D, key_range=kr, doc_range=dr)
    ctx, lse, _ = A.attn_fwd(qkv, B, S, H, D, doc_range=dr)
    with pytest.raises(ValueError):
        A.attn_bwd(torch.randn(B * S, H * D), qkv, ctx, lse, B, S, H, D, key_range=kr, doc_range=dr)
    with pytest.raises(ValueError):
        A.attn_fwd_ref(qkv, B, S, H, D, doc_range=dr.ranges[:, :4])             # wrong shape
    assert A.fused_bwd_applies(512, 64, False, None, doc_range=dr) is False
    layer = build_model("tiny", impl="reference", seed=0).layers[0]
    with pytest.raises(ValueError):
        layer(torch.randn(B, S, layer.cfg.hidden_size), key_range=kr, doc_range=dr)


# ------------------------------------------------------------------ math reference vs brute force
def _oracle(qkv, dctx, B, S, H, D, causal, slopes, p, seed, sid, seg):
    """Dense ``same_doc & causal`` mask in fp64, torch.softmax, autograd for the gradients.  Rows
    without a key are zeroed after the softmax (their softmax is NaN)."""
    x = qkv.double().clone().requires_grad_(True)
    v5 = x.view(B, S, 3, H, D)
    q, k, v = (v5[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    j = torch.arange(S)
    if slopes is not None:
        s = s + slopes.double().view(1, H, 1, 1) * j.double().view(1, 1, 1, S)
    allowed = (seg.view(B, S, 1) == seg.view(B, 1, S)) & (seg != 0).view(B, S, 1)
    if causal:
        allowed = allowed & (j.view(1, S) <= j.view(S, 1))
    allowed = allowed.view(B, 1, S, S).expand(B, H, S, S)
    s = s.masked_fill(~allowed, float("-inf"))
    dead = ~allowed.any(-1, keepdim=True)
    prob = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    lse = torch.logsumexp(s, -1)
    if p > 0:
        prob = prob * attn_keep_mask(B, H, S, p, seed, 0, sid).double() / (1.0 - p)
    ctx = (prob @ v).transpose(1, 2).reshape(B * S, H * D)
    ctx.backward(dctx.double())
    return ctx.detach(), lse.detach(), x.grad


@pytest.mark.parametrize("causal,alibi,p", [(False, False, 0.0), (True, True, 0.0), (True, False, 0.2),
                                            (False, True, 0.2)])
def test_reference_with_doc_range_matches_fp64_dense_mask(causal, alibi, p):
    B, S, H, D = 3, 40, 2, 8
    seg = torch.zeros(B, S, dtype=torch.int64)
    seg[0, :13], seg[0, 13:14], seg[0, 14:33] = 1, 2, 3          # a one-token document, a padded tail
    seg[1, 5:40] = 9                                             # left pad
    #  row 2: all pads
    torch.manual_seed(0)
    qkv = torch.randn(B * S, 3 * H * D, dtype=torch.float64)
    dctx = torch.randn(B * S, H * D, dtype=torch.float64)
    slopes = A.alibi_slopes(H) if alibi else None
    dr = A.doc_range_from_segment_ids(seg, check=True)
    rng = RngState(7, device="cpu")
    ctx, lse = A.attn_fwd_ref(qkv, B, S, H, D, causal, slopes, p, rng, 4, doc_range=dr)
    dqkv = A.attn_bwd_ref(dctx, qkv, ctx, lse, B, S, H, D, causal, slopes, p, rng, 4, doc_range=dr)
    ctx_o, lse_o, dqkv_o = _oracle(qkv, dctx, B, S, H, D, causal, slopes, p, 7, 4, seg)
    assert torch.allclose(ctx, ctx_o, atol=1e-10) and torch.allclose(dqkv, dqkv_o, atol=1e-10)
    pad = seg == 0
    assert torch.equal(lse == float("-inf"), pad.view(B, 1, S).expand(B, H, S))
    assert torch.allclose(lse[~torch.isinf(lse)], lse_o[~torch.isinf(lse_o)], atol=1e-10)
    # empty rows: ctx 0, dq 0; pad keys: dk = dv = 0 -- exactly
    assert (ctx.view(B, S, -1)[pad] == 0).all() and (dqkv.view(B, S, -1)[pad] == 0).all()
    # bare [B, S, 2] spans are accepted too
    assert torch.equal(A.attn_fwd_ref(qkv, B, S, H, D, causal, slopes, p, rng, 4, doc_range=dr.ranges)[0], ctx)


# ------------------------------------------------------------------ pack_documents
def test_pack_documents_properties():
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, 40, (60,), generator=g).tolist() + [64, 100, 0]
    docs = [[1000 * n + t for t in range(L)] for n, L in enumerate(lens)]      # every token is unique
    S = 64
    ids, seg = pack_documents(docs, S, pad_id=-7)
    assert ids.shape == seg.shape and ids.shape[1] == S and ids.dtype == seg.dtype == torch.int64
    assert ((ids == -7) == (seg == 0)).all()                                   # pads, and only pads, take id 0
    A.doc_range_from_segment_ids(seg, check=True)                              # contiguous, no id comes back
    flat = ids[seg != 0].tolist()
    assert len(flat) == len(set(flat))                                         # every token at most once
    for n, d in enumerate(docs):
        want = d[:S]                                                           # truncated to the row length
        if not want:
            continue
        r, c = (ids == want[0]).nonzero()[0].tolist()
        assert ids[r, c:c + len(want)].tolist() == want, n                     # once, contiguously, in one row
        assert seg[r, c:c + len(want)].unique().numel() == 1
        assert (c == 0 or seg[r, c - 1] != seg[r, c]) and (c + len(want) == S or seg[r, c + len(want)] != seg[r, c])
    assert len(flat) == sum(min(L, S) for L in lens)
    # first fit, in order: a document never sits in a later row than an earlier row could have held it
    free = (seg == 0).sum(1)
    first = {int(ids[r, c]): r for r in range(ids.shape[0]) for c in range(S) if seg[r, c] and (c == 0 or seg[r, c - 1] != seg[r, c])}
    assert first[docs[0][0]] == 0
    assert free.min() >= 0 and (seg.max(1).values >= 1).all()                  # no row over-full, none empty
    assert ids.shape[0] < len([L for L in lens if L])                          # it packs
    # segment ids number the documents of a row 1, 2, ...
    for r in range(ids.shape[0]):
        u = seg[r][seg[r] != 0].unique_consecutive().tolist()
        assert u == list(range(1, len(u) + 1))
    e_ids, e_seg = pack_documents([], 8, 0)
    assert e_ids.shape == (0, 8) and e_seg.shape == (0, 8)


# ------------------------------------------------------------------ dataset columns and label rules
@pytest.mark.parametrize("name", ["tiny", "causal-tiny"])
def test_packed_synthetic_dataset_columns_and_labels(name):
    cfg = build_model(name, device="meta").cfg
    S = 48
    ds = SyntheticLMDataset(cfg, 64, seq_len=S, seed=4, pad_fraction=0.5, max_docs=4)
    seg, ids, lab = ds.segment_ids, ds.input_ids, ds.labels
    assert seg.shape == (64, S) and seg.dtype == torch.int64
    dr = A.doc_range_from_segment_ids(seg, check=True)
    ndocs = seg.max(1).values
    assert ndocs.min() >= 1 and ndocs.max() <= 4 and (ndocs > 1).any()
    assert (seg == 0).any() and ((seg != 0).sum(1) == S).any()                 # padded tails and full rows
    lo, hi = dr.ranges[..., 0].long(), dr.ranges[..., 1].long()
    live = seg != 0
    assert ((hi - lo)[live] >= 2).all()
    pos = torch.arange(S).expand(64, S)
    first, last = live & (pos == lo), live & (pos == hi - 1)
    pad_id = cfg.pad_token_id if cfg.pad_token_id < cfg.vocab_size else 0
    assert (ids[~live] == pad_id).all() and (lab[~live] == -100).all()
    if cfg.family == "bert":
        assert (ids[first] == 101).all() and (ids[last] == 102).all()          # every document is framed
        assert (lab[first | last] == -100).all()                               # ... and its specials exempt
        labelled = lab != -100
        assert 0.08 < labelled[live & ~first & ~last].float().mean() < 0.25    # the 15 % law on the rest
    else:
        assert torch.equal(lab, packed_causal_labels(ids, seg))
        assert (lab[first] == -100).all() and torch.equal(lab[live & ~first], ids[live & ~first])
    row = ds[3]
    assert set(row) == {"input_ids", "labels", "segment_ids"} and torch.equal(row["segment_ids"], seg[3])
    sub = ds.select([5, 1])
    assert torch.equal(sub.segment_ids, seg[[5, 1]]) and set(sub[0]) == set(row)


@pytest.mark.parametrize("name", ["tiny", "causal-tiny"])
def test_draws_without_max_docs_are_unchanged(name):
    """max_docs = 0 draws what the dataset drew before the argument existed: the unpacked rows are
    a pure function of the generator's first draws, which this re-derives by hand."""
    from distributed_training_and_deepspeed_amd.data.synthetic import mlm_mask_tokens, synthetic_token_rows_lengths
    cfg = build_model(name, device="meta").cfg
    ds = SyntheticLMDataset(cfg, 16, seq_len=32, seed=9, pad_fraction=0.5)
    g = torch.Generator().manual_seed(9)
    ids, special, _ = synthetic_token_rows_lengths(16, 32, cfg, g, 0.5)
    if ds.mlm:
        ids, lab = mlm_mask_tokens(ids, special, cfg.vocab_size, cfg.mask_token_id, g)
    else:
        lab = ids.clone()
    assert torch.equal(ds.input_ids, ids) and torch.equal(ds.labels, lab)
    assert ds.segment_ids is None and set(ds[0]) == {"input_ids", "labels"}
    assert torch.equal(SyntheticLMDataset(cfg, 16, seq_len=32, seed=9, pad_fraction=0.5, max_docs=0).input_ids, ids)


class _Tok:
    """Minimal stand-in for an HF tokenizer: one token per character, [CLS] ... [SEP] framing."""
    pad_token_id, mask_token_id, cls, sep = 0, 4, 2, 3

    def __len__(self):
        return 300

    def __call__(self, lines, padding, truncation, max_length, return_special_tokens_mask, **kw):
        assert padding is False and truncation
        ids = [([self.cls] + [10 + ord(c) for c in ln] + [self.sep])[:max_length] for ln in lines]
        return {"input_ids": ids, "special_tokens_mask": [[int(t in (self.cls, self.sep)) for t in r] for r in ids]}


@pytest.mark.parametrize("mlm", [False, True])
def test_load_wikitext_pack(tmp_path, mlm):
    lines = ["abc", "defghij", "k", "lmnopqrstuvwxyzabcdefghijklmnopqrstuvwxyz", "no", "pq rs"]
    f = tmp_path / "wiki.train.raw"
    f.write_text("\n".join(lines) + "\n")
    S = 16
    ds = load_wikitext(_Tok(), max_length=S, path=str(f), mlm=mlm, seed=1, pack=True)
    seg, ids, lab = ds.segment_ids, ds.input_ids, ds.labels
    assert ids.shape == seg.shape == lab.shape and ids.shape[1] == S and ids.shape[0] < len(lines)
    A.doc_range_from_segment_ids(seg, check=True)
    assert set(ds[0]) == {"input_ids", "labels", "segment_ids"}
    want_ids, want_seg = pack_documents(_Tok()(lines, False, True, S, True)["input_ids"], S, 0)
    assert torch.equal(seg, want_seg)
    assert (lab[seg == 0] == -100).all()
    if mlm:
        special = (want_ids == 2) | (want_ids == 3) | (want_seg == 0)
        assert (lab[special] == -100).all() and torch.equal(ids[special], want_ids[special])
        assert torch.equal(lab[lab != -100], want_ids[lab != -100])
    else:
        assert torch.equal(ids, want_ids) and torch.equal(lab, packed_causal_labels(ids, seg))
        assert (lab[ids == 2] == -100).all()                    # every document starts with [CLS]
    with pytest.raises(ValueError):
        load_wikitext(_Tok(), max_length=S, path=str(f), mlm=mlm, pack=True, return_attention_mask=True)


# ------------------------------------------------------------------ the model-level proof
def _models():
    # a BLOOM-style tiny: ALiBi, no position table
    C.PRESETS["_dm_bloom"] = C.BLOOM_560M.with_(name="_dm_bloom", vocab_size=1024, hidden_size=128, num_layers=2,
                                                num_heads=2, ffn_size=512)
    return ["causal-tiny", "_dm_bloom", "tiny"]


def _labelled_mean(model, rows):
    """Labelled-token-weighted mean of the losses of ``rows`` = [(ids [1, L], labels [1, L])], each
    run as a sequence of its own."""
    tot, cnt = 0.0, 0
    for ids, lab in rows:
        shifted = lab[:, 1:] if model.cfg.causal else lab
        n = int((shifted != -100).sum())
        if n:
            tot += model(ids, labels=lab).loss.double().item() * n
            cnt += n
    return tot / cnt


@pytest.mark.parametrize("which", [0, 1, 2], ids=["causal-learned-positions", "bloom-alibi", "bert"])
def test_packed_loss_equals_the_documents_run_separately(which):
    """fp32 CPU reference path, dropout off: the loss of a packed batch with segment_ids equals the
    labelled-token-weighted mean of the losses of its documents run as separate unpadded sequences
    (block-diagonal attention, positions that restart, no label across a boundary) -- and differs
    from the loss of the same batch without segment_ids."""
    name = _models()[which]
    model = build_model(name, impl="reference", seed=3)
    model.eval()
    cfg = model.cfg
    if which == 1:
        assert model.embeddings.pos is None and model.layers[0].alibi is not None
    else:
        assert model.embeddings.pos is not None
    ds = SyntheticLMDataset(cfg, 6, seq_len=40, seed=2, pad_fraction=0.5, max_docs=3)
    ids, lab, seg = ds.input_ids, ds.labels, ds.segment_ids
    assert int(seg.max()) > 1 and (seg == 0).any()
    dr = A.doc_range_from_segment_ids(seg, check=True)
    rows = []
    for b in range(ids.shape[0]):
        for lo, hi in sorted({tuple(r) for r in dr.ranges[b].tolist() if r[1] > r[0]}):
            rows.append((ids[b:b + 1, lo:hi], lab[b:b + 1, lo:hi]))
    with torch.no_grad():
        packed = model(ids, labels=lab, segment_ids=seg).loss.double().item()
        separate = _labelled_mean(model, rows)
        plain = model(ids, labels=lab).loss.double().item()
    print(f"{name}: packed {packed:.7f} separate {separate:.7f} without segment_ids {plain:.7f}")
    assert abs(packed - separate) <= 1e-5 * abs(separate)
    assert abs(plain - separate) > 1e-5 * abs(separate)       # (randomly initialised: the leak is small, not absent)
    with pytest.raises(ValueError):
        model(ids, labels=lab, segment_ids=seg, attention_mask=(seg != 0).long())


# ------------------------------------------------------------------ scripts
def _script(args):
    return subprocess.run([sys.executable, *args], cwd=ROOT, capture_output=True, text=True, timeout=120,
                          env={**os.environ, "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""})


@pytest.mark.parametrize("script,model", [("data_parallel_training.py", ["--model", "tiny", "--device-count", "1"]),
                                          ("zero_dp_training.py", ["--model-name", "causal-tiny", "--no-memstats"])])
def test_scripts_pack_docs_two_cpu_steps(script, model):
    common = [script, *model, "--batch-size", "2", "--training-steps", "2", "--seq-len", "32", "--backend", "gloo",
              "--dtype", "fp32", "--quiet", "--pad-fraction", "0.5"]
    r = _script(common + ["--pack-docs", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{") and "tokens_per_s" in ln][-1])
    assert rec["final_loss"] == rec["final_loss"] and 0 < rec["labelled_tokens_per_s"] < rec["tokens_per_s"]
    bad = _script(common + ["--pack-docs", "3", "--attention-mask"])
    assert bad.returncode != 0 and "mutually exclusive" in bad.stderr
