"""Sliding-window attention without a GPU: the math reference (``attn_fwd_ref`` / ``attn_bwd_ref`` with
``window=``) against the fp64 oracle of ``tests/oracles.py``, the argument's validation and dispatch
rules, and the Mistral models (``TransformerConfig.sliding_window``) against ``transformers`` and against
per-document / per-sequence runs.  ``tests/test_attention_window_gpu.py`` runs the same cases on the
windowed HIP kernels.

The oracle needs no band of its own: under ``causal`` a window of W keys is a span per query, and
``oracles.attention`` / ``attention_staged`` take plain ``[B, S, 2]`` spans as ``doc_range``.  Query i of
a case gets ``(max(lo_i, i - W + 1), max(hi_i, that))``, with ``(lo_i, hi_i)`` = (0, S), its sequence's
key range or its document's span.  Metric and bounds are ``check_attention``'s of
``tests/test_attention_oracles_cpu.py``, unchanged: per (token, head) row, the reference at a quarter
of the bf16 cap.

Cases (``CASES``; shapes of that file's ``SHAPES``), chosen for what the kernels cross:
  inside-wave      g200 Hkv 2, W 20: band narrower than a wave's 32 rows, every diagonal tile masked
  tile-aligned     g200 Hkv 1, W 64: the band edge on a 64-key tile boundary -- the off-by-one cases
  across-tiles     g200 Hkv 2, W 100: first tile > 0 in block 1; waves of a block start at different tiles
  self-only        g200 Hkv 2, W 1: one key per row (P = 1)
  d128-*           g160, W 70 / 64: head_dim 128, dK/dV with 64-row query tiles
  multi-head       m512 Hkv = H, W 128: one query head per group; dK/dV's last query tile cut at every block
  group-walk-*     m512 Hkv 2, W 130 / 300: 1-3 query tiles per key block, the same count for each head
  key-range-*      g200 Hkv 2, W 40, ``make_mask("pad")`` / ``("empty")``: intersection, dead rows
  documents        g200 Hkv 2, W 40, ``make_mask("doc")``: the window folded into the spans
"""
import functools
import importlib.util
import os
import types

import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model, count_parameters, get_config
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.models.llama import from_hf_state_dict, to_hf_state_dict
from distributed_training_and_deepspeed_amd.ops import attention as A

from . import oracles as O
from .test_attention_oracles_cpu import BF16, F32, OUTPUTS, SHAPES, _worst, check_attention, make_mask, run_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = ("gauss", "peaked", "row_scales", "spikes_up")

# name -> (shape, kv_heads (None = multi-head), window, mask kind)
CASES = {
    "inside-wave": ("g200", 2, 20, None),
    "tile-aligned": ("g200", 1, 64, None),
    "across-tiles": ("g200", 2, 100, None),
    "self-only": ("g200", 2, 1, None),
    "d128-mqa": ("g160", 1, 70, None),
    "d128-gqa": ("g160", 2, 64, None),
    "multi-head": ("m512", None, 128, None),
    "group-walk-130": ("m512", 2, 130, None),
    "group-walk-300": ("m512", 2, 300, None),
    "key-range-pad": ("g200", 2, 40, "pad"),
    "key-range-empty": ("g200", 2, 40, "empty"),
    "documents": ("g200", 2, 40, "doc"),
}
# rows without a key in the oracle ([B, H, S] entries): the 37 causal rows in front of sequence 0's left
# padding, times 4 heads; with "empty" also every row of sequence 1
DEAD_ROWS = {"key-range-pad": 148, "key-range-empty": 948}


def window_spans(B, S, W, key_range=None, doc_range=None):
    """[B, S, 2] int64: query i's keys under a causal window of W, intersected with the mask."""
    i = torch.arange(S).view(1, S).expand(B, S)
    if doc_range is not None:
        lo, hi = doc_range.ranges[..., 0].long(), doc_range.ranges[..., 1].long()
    elif key_range is not None:
        lo, hi = (key_range[:, k].long().view(B, 1).expand(B, S) for k in (0, 1))
    else:
        lo, hi = torch.zeros(B, S, dtype=torch.int64), torch.full((B, S), S, dtype=torch.int64)
    lo = torch.maximum(lo, i - W + 1)
    return torch.stack([lo, torch.maximum(hi, lo)], 2)


@functools.lru_cache(maxsize=None)
def win_case(regime, name):
    """Inputs, oracle and staged-model errors of one windowed case -- the namespace of ``attn_case``,
    plus ``window``; computed once, shared, never modified."""
    shape, kv_heads, W, mask = CASES[name]
    B, S, H, D = SHAPES[shape]
    qkv, dctx = O.attn_inputs(regime, B, S, H, D, kv_heads, seed=100 + len(regime) + S)
    key_range, doc_range = make_mask(mask, B, S)
    kw = dict(causal=True, doc_range=window_spans(B, S, W, key_range, doc_range), kv_heads=kv_heads)
    c = types.SimpleNamespace(regime=regime, shape=shape, B=B, S=S, H=H, D=D, Hkv=kv_heads or H, mode="causal",
                              causal=True, slopes=None, p=0.0, keep=None, mask=mask, key_range=key_range,
                              doc_range=doc_range, kv_heads=kv_heads, qkv=qkv, dctx=dctx, window=W, name=name)
    c.tag = f"{regime}/{name}/{shape}/W{W}"
    c.oracle = O.attention(qkv, dctx, B, S, H, D, **kw)
    st = O.attention_staged(qkv, dctx, B, S, H, D, **kw)
    c.e_staged = {n: _worst(st[n], c.oracle, n) for n in OUTPUTS}
    c.e_ref32 = None
    return c


def all_cases(regimes=REGIMES):
    return [(r, n) for n in CASES for r in regimes]


def case_id(case):
    return f"{case[1]}-{case[0]}"


# ------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("case", all_cases(), ids=case_id)
def test_reference_meets_a_quarter_of_the_tolerance(case):
    c = win_case(*case)
    o = c.oracle
    assert all(torch.isfinite(o[n]).all() for n in OUTPUTS) and not torch.isnan(o["lse"]).any()
    assert int((o["lse"] == float("-inf")).sum()) == DEAD_ROWS.get(c.name, int((o["lse"] == float("-inf")).sum()))
    if c.mask is None:
        assert not (o["lse"] == float("-inf")).any()
    check_attention(c, *run_ref(c, BF16, window=c.window), "ref", "ref bf16 window")
    check_attention(c, *run_ref(c, F32, window=c.window), "ref32", "ref fp32 window")


def test_rows_die_when_the_window_lies_behind_a_right_padded_range():
    """Range (0, hi): every query i >= hi + W - 1 has its whole window behind the range."""
    B, S, H, Hkv, D, W, hi = 1, 96, 2, 1, 64, 8, 50
    qkv, dctx = O.attn_inputs("gauss", B, S, H, D, Hkv, seed=7)
    kr = torch.tensor([[0, hi]], dtype=torch.int32)
    ctx, lse = A.attn_fwd_ref(qkv, B, S, H, D, True, key_range=kr, kv_heads=Hkv, window=W)
    dead = torch.arange(S) >= hi + W - 1
    assert torch.equal(lse == float("-inf"), dead.view(1, 1, S).expand(B, H, S))
    assert (ctx.view(B, S, H, D)[:, dead] == 0).all()
    dq, dk, dv = O.attn_split(A.attn_bwd_ref(dctx, qkv, ctx, lse, B, S, H, D, True, key_range=kr, kv_heads=Hkv, window=W),
                              B, S, H, Hkv, D)
    assert torch.isfinite(dq).all() and (dq[:, dead] == 0).all()
    assert (dk[:, hi:] == 0).all() and (dv[:, hi:] == 0).all() and (dv[:, :hi] != 0).any()


@pytest.mark.parametrize("name", ["across-tiles", "multi-head", "key-range-pad", "documents"])
def test_no_window_and_a_window_of_the_whole_sequence_are_the_plain_call(name):
    c = win_case("gauss", name)
    base = run_ref(c)
    for w in (None, 0, c.S, c.S + 1000):
        got = run_ref(c, window=w)
        assert all(torch.equal(a, b) for a, b in zip(base, got)), w
    assert not torch.equal(base[0], run_ref(c, window=c.window)[0])


def test_rejections():
    c = win_case("gauss", "inside-wave")
    mh = win_case("gauss", "multi-head")
    from distributed_training_and_deepspeed_amd.ops.rng import RngState
    rng = RngState(1, device="cpu")
    for fwd in (A.attn_fwd, A.attn_fwd_ref):
        with pytest.raises(ValueError):          # a window needs causal
            fwd(c.qkv, c.B, c.S, c.H, c.D, False, kv_heads=c.kv_heads, window=20)
        with pytest.raises(ValueError):
            fwd(c.qkv, c.B, c.S, c.H, c.D, True, kv_heads=c.kv_heads, window=-3)
        with pytest.raises(ValueError):          # no dropout, no ALiBi
            fwd(mh.qkv, mh.B, mh.S, mh.H, mh.D, True, None, 0.1, rng, 0, window=20)
        with pytest.raises(ValueError):
            fwd(mh.qkv, mh.B, mh.S, mh.H, mh.D, True, A.alibi_slopes(mh.H), window=20)
    ctx, lse, _ = A.attn_fwd(mh.qkv, mh.B, mh.S, mh.H, mh.D, True, window=20)
    for bwd in (A.attn_bwd, A.attn_bwd_ref):
        with pytest.raises(ValueError):
            bwd(mh.dctx, mh.qkv, ctx, lse, mh.B, mh.S, mh.H, mh.D, False, window=20)
        with pytest.raises(ValueError):
            bwd(mh.dctx, mh.qkv, ctx, lse, mh.B, mh.S, mh.H, mh.D, True, None, 0.1, rng, 0, window=20)
        with pytest.raises(ValueError):
            bwd(mh.dctx, mh.qkv, ctx, lse, mh.B, mh.S, mh.H, mh.D, True, A.alibi_slopes(mh.H), window=20)
    # window >= S is dropped before dispatch, but not before it is validated
    with pytest.raises(ValueError):
        A.attn_fwd(mh.qkv, mh.B, mh.S, mh.H, mh.D, False, window=mh.S + 5)
    assert not A.fused_bwd_applies(512, 64, False, None, window=64)
    assert A.fused_bwd_applies(512, 64, False, None, window=None) == A.fused_bwd_applies(512, 64, False, None)


def test_cpu_and_fp32_inputs_take_the_reference_and_dbias_the_column_sums():
    c = win_case("gauss", "inside-wave")
    kw = dict(kv_heads=c.kv_heads, window=c.window)
    for dtype in (BF16, F32):
        qkv, dctx = c.qkv.to(dtype), c.dctx.to(dtype)
        ctx, lse, masks = A.attn_fwd(qkv, c.B, c.S, c.H, c.D, True, **kw)
        rc, rl = A.attn_fwd_ref(qkv, c.B, c.S, c.H, c.D, True, **kw)
        assert masks is None and torch.equal(ctx, rc) and torch.equal(lse, rl)
        db = torch.full((qkv.shape[1],), 0.25, dtype=F32)
        dqkv = A.attn_bwd(dctx, qkv, ctx, lse, c.B, c.S, c.H, c.D, True, dbias=(db, True), **kw)
        assert torch.equal(dqkv, A.attn_bwd_ref(dctx, qkv, ctx, lse, c.B, c.S, c.H, c.D, True, **kw))
        ref = dqkv.float().sum(0)
        assert ((db - 0.25) - ref).abs().max().item() <= 1e-3 * (ref.abs().max().item() + 1.0)


@pytest.mark.parametrize("name", ["inside-wave", "tile-aligned", "multi-head", "key-range-pad", "documents"])
def test_mutants_window_off_by_one_and_window_ignored(name):
    """The chosen inputs see the band's edge: one key too many per row fails the check, and so does the
    plain causal call."""
    c = win_case("gauss", name)
    check_attention(c, *run_ref(c, window=c.window), "ref", "ref bf16 window")
    for w in (c.window + 1, None):
        with pytest.raises(AssertionError, match="above its bound"):
            check_attention(c, *run_ref(c, window=w), "ref", f"mutant W={w}")


# ------------------------------------------------------------------------------------------ models
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4     # tests/test_llama_cpu.py's, relative
MS = 128


def _batch(cfg, B=2, S=MS, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.vocab_size, (B, S), generator=g)
    labels = ids.clone()
    labels[torch.rand(B, S, generator=g) < 0.2] = -100
    return ids, labels


def test_presets():
    cfg = get_config("mistralai/Mistral-7B-v0.1")
    assert get_config("mistral-7b") is cfg
    assert (cfg.vocab_size, cfg.hidden_size, cfg.num_layers, cfg.num_heads, cfg.kv_heads, cfg.ffn_size) == \
        (32000, 4096, 32, 32, 8, 14336)
    assert (cfg.max_positions, cfg.ln_eps, cfg.rope_theta, cfg.sliding_window, cfg.head_dim) == (32768, 1e-5, 10000.0, 4096, 128)
    assert cfg.family == "llama" and cfg.llama_style and cfg.causal and not cfg.tie_word_embeddings
    V, h, L, f, kv = cfg.vocab_size, cfg.hidden_size, cfg.num_layers, cfg.ffn_size, cfg.kv_heads * cfg.head_dim
    assert 2 * V * h + L * (2 * h * h + 2 * h * kv + 3 * h * f + 2 * h) + h == 7_241_732_096
    tiny = get_config("mistral-tiny")
    assert tiny == get_config("llama-tiny-gqa").with_(name="mistral-tiny", sliding_window=48)
    assert count_parameters(build_model("mistral-tiny")) == count_parameters(build_model("llama-tiny-gqa"))
    assert all(c.sliding_window == 0 for n, c in C.PRESETS.items() if "istral" not in n)


@pytest.mark.parametrize("bad", [dict(sliding_window=-1), dict(sliding_window=8, causal=False),
                                 dict(sliding_window=8, attn_dropout=0.1)])
def test_config_rejections(bad):
    with pytest.raises(ValueError):
        get_config("llama-tiny").with_(**bad)
    with pytest.raises(ValueError):
        get_config("causal-tiny").with_(sliding_window=8)


def test_cli_flag_needs_a_llama_family_model():
    spec = importlib.util.spec_from_file_location("_zero_dp_training", os.path.join(ROOT, "zero_dp_training.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError):
        mod.window_config("facebook/opt-125m", 64)
    with pytest.raises(ValueError):
        mod.window_config("tiny", 64)
    assert mod.window_config("facebook/opt-125m", 0) == "facebook/opt-125m"
    assert mod.window_config("mistral-tiny", 0) == "mistral-tiny"
    cfg = mod.window_config("llama-tiny-gqa", 48)
    assert cfg == get_config("llama-tiny-gqa").with_(sliding_window=48) and get_config(cfg) is cfg


def test_reference_matches_hf_mistral():
    tf = pytest.importorskip("transformers")
    cfg = get_config("mistral-tiny")
    torch.manual_seed(1)
    hf = tf.MistralForCausalLM(tf.MistralConfig(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.ffn_size,
        num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.kv_heads,
        head_dim=cfg.head_dim, max_position_embeddings=cfg.max_positions, rms_norm_eps=cfg.ln_eps,
        rope_theta=cfg.rope_theta, hidden_act="silu", tie_word_embeddings=False, attention_dropout=0.0,
        sliding_window=cfg.sliding_window, attn_implementation="eager")).float()
    hf.train()
    with torch.no_grad():      # HF initialises the norms to 1: give them something to get wrong
        for n, p in hf.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    model = build_model("mistral-tiny", impl="reference")
    missing = model.load_state_dict(from_hf_state_dict(hf.state_dict()), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.train()
    ids, labels = _batch(cfg)
    hf_loss = hf(input_ids=ids, labels=labels).loss
    hf_loss.backward()
    model.zero_grad(set_to_none=True)
    loss = model(ids, labels=labels).loss
    loss.backward()
    assert abs(loss.item() - hf_loss.item()) <= LOSS_TOL * abs(hf_loss.item()), (loss.item(), hf_loss.item())
    ours_hf = to_hf_state_dict({n: p.grad for n, p in model.named_parameters()})     # our gradients in HF's layout
    for n, p in hf.named_parameters():
        err = (ours_hf[n] - p.grad).norm().item() / (p.grad.norm().item() + 1e-30)
        assert err <= GRAD_TOL, (n, err)
    # the window bites at this length: the same weights without it give another loss
    plain = build_model("llama-tiny-gqa", impl="reference")
    plain.load_state_dict(model.state_dict())
    assert abs(plain(ids, labels=labels).loss.item() - loss.item()) > 10 * LOSS_TOL * abs(loss.item())


@pytest.mark.parametrize("impl", ["reference", "fused"])
def test_fused_cpu_path_and_reference_agree(impl):
    """The fused layer on the CPU (the math reference behind ``attn_fwd(window=)``) against the plain
    PyTorch reference layer, in the three mask modes."""
    cfg = get_config("mistral-tiny")
    ref = build_model("mistral-tiny", impl="reference", seed=5)
    got = build_model("mistral-tiny", impl=impl, seed=5)
    got.load_state_dict(ref.state_dict())
    ids, labels = _batch(cfg, seed=4)
    for kw in ({}, {"attention_mask": _padding_mask()}, {"segment_ids": _segments()}):
        outs = []
        for m in (ref, got):
            m.zero_grad(set_to_none=True)
            loss = m(ids, labels=labels, **kw).loss
            loss.backward()
            outs.append((loss.item(), {n: p.grad.clone() for n, p in m.named_parameters()}))
        (l1, g1), (l2, g2) = outs
        assert abs(l1 - l2) <= LOSS_TOL * abs(l1), (list(kw), l1, l2)
        for n in g1:
            err = (g1[n] - g2[n]).norm().item() / (g1[n].norm().item() + 1e-30)
            assert err <= GRAD_TOL, (list(kw), n, err)


def _segments(B=2, S=MS):
    """Documents longer than the window of 48, a short one, pads between and behind."""
    seg = torch.zeros(B, S, dtype=torch.int64)
    seg[0, :70], seg[0, 70:MS - 9] = 1, 2
    seg[1, :5], seg[1, 8:90], seg[1, 90:] = 1, 2, 3
    return seg


def _padding_mask(B=2, S=MS):
    m = torch.ones(B, S, dtype=torch.int64)
    m[0, S - 29:] = 0            # right-padded
    m[1, :41] = 0                # left-padded (rotary embeddings are relative: the shift does not show)
    return m


def _weighted_mean(model, rows):
    tot, cnt = 0.0, 0
    for ids, lab in rows:
        n = int((lab[:, 1:] != -100).sum())
        if n:
            tot += model(ids, labels=lab).loss.double().item() * n
            cnt += n
    return tot / cnt


def test_packed_and_padded_losses_equal_the_parts_run_alone():
    """mistral-tiny, fp32 reference: under ``segment_ids`` the loss is the labelled-token-weighted mean of
    the documents run alone (each windowed, from position 0), under ``attention_mask`` that of the
    unpadded sequences -- the window intersects the span / the range."""
    from distributed_training_and_deepspeed_amd.data.packing import packed_causal_labels
    cfg = get_config("mistral-tiny")
    model = build_model("mistral-tiny", impl="reference", seed=3)
    model.eval()
    ids, _ = _batch(cfg, seed=2)
    with torch.no_grad():
        seg = _segments()
        lab = packed_causal_labels(ids, seg)
        dr = A.doc_range_from_segment_ids(seg, check=True)
        rows = [(ids[b:b + 1, lo:hi], lab[b:b + 1, lo:hi]) for b in range(ids.shape[0])
                for lo, hi in sorted({tuple(r) for r in dr.ranges[b].tolist() if r[1] > r[0]})]
        assert max(r[0].shape[1] for r in rows) > cfg.sliding_window
        packed = model(ids, labels=lab, segment_ids=seg).loss.double().item()
        separate = _weighted_mean(model, rows)
        assert abs(packed - separate) <= 1e-5 * abs(separate), (packed, separate)
        m = _padding_mask()
        lab = ids.masked_fill(m == 0, -100)
        kr = A.key_range_from_mask(m)
        for b, (lo, _) in enumerate(kr.tolist()):     # a sequence's first token is predicted by nothing of it
            lab[b, lo] = -100
        rows =[(ids[b:b + 1, lo:hi], lab[b:b + 1, lo:hi]) for b, (lo, hi) in enumerate(kr.tolist())]
        padded = model(ids, labels=lab, attention_mask=m).loss.double().item()
        separate = _weighted_mean(model, rows)
        assert abs(padded - separate) <= 1e-5 * abs(separate), (padded, separate)
        unwindowed = build_model("llama-tiny-gqa", impl="reference", seed=3)
        unwindowed.load_state_dict(model.state_dict())
        other = unwindowed(ids, labels=lab, attention_mask=m).loss.double().item()
        assert abs(other - padded) > 1e-5 * abs(padded)
