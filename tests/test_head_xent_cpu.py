"""Logit-free LM-head loss (Runtime.head_loss = "fused"): the block plan and the chunked autograd
function on the CPU (fp32 math path) against torch autograd on F.cross_entropy(F.linear(...))."""
import pytest
import torch
import torch.nn.functional as F

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.models import layers as L
from distributed_training_and_deepspeed_amd.ops import functional as Fx


@pytest.mark.parametrize("T,V,h,chunks", [(130, 549, 128, 3), (512, 50257, 1024, 8), (131072, 250880, 1024, 8)])
def test_plan_covers_the_rectangle_once(T, V, h, chunks):
    plan = Fx.head_xent_plan(T, V, h, chunks)
    area = 0
    for r0, r1, v0, v1 in plan:
        assert 0 <= r0 < r1 <= T and 0 <= v0 < v1 <= V
        assert (r1 - r0) * (v1 - v0) <= Fx.HEAD_XENT_MAX_BLOCK      # the chunk buffer's addressing limit
        assert v1 == V or (v1 - v0) % Fx.HEAD_XENT_TILE == 0        # whole column tiles except the last
        assert v0 % Fx.HEAD_XENT_TILE == 0
        area += (r1 - r0) * (v1 - v0)
    assert area == T * V
    # equal total area + pairwise disjoint = exactly once
    rows = sorted({(r0, r1) for r0, r1, _, _ in plan})
    cols = sorted({(v0, v1) for _, _, v0, v1 in plan})
    assert len(plan) == len(rows) * len(cols) == len(set(plan))
    for spans, end in ((rows, T), (cols, V)):
        assert spans[0][0] == 0 and spans[-1][1] == end
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert len(cols) <= chunks


def test_plan_splits_rows_only_past_the_limit():
    assert len({(r0, r1) for r0, r1, _, _ in Fx.head_xent_plan(512, 50257, 1024, 8)}) == 1
    assert len({(r0, r1) for r0, r1, _, _ in Fx.head_xent_plan(131072, 250880, 1024, 8)}) > 1


def _model(chunks=3):
    C.PRESETS["_hx"] = C.get_config("causal-tiny").with_(vocab_size=1000)
    m = build_model("_hx", impl="fused", seed=4)
    m.rt.head_loss, m.rt.head_chunks = "fused", chunks
    return m


def _inputs(m, B=3, S=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, m.cfg.hidden_size, generator=g, requires_grad=True)
    lab = torch.randint(0, m.cfg.vocab_size, (B, S), generator=g)
    lab[0, 1] = 0
    lab[0, 2] = m.cfg.vocab_size - 1
    lab[1, 3:6] = -100
    lab[2, 1] = -100
    return x, lab


def _reference(x, w, lab):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    h = x.shape[-1]
    loss = F.cross_entropy(F.linear(x[:, :-1].reshape(-1, h), w), lab[:, 1:].reshape(-1), ignore_index=-100)
    loss.backward()
    return loss.detach(), x.grad, w.grad


@pytest.mark.parametrize("slot", ["grad", "main_grad"])
def test_lm_head_fused_loss_matches_autograd(slot, monkeypatch):
    m = _model()
    head, w = m.head, m.embeddings.word
    x, lab = _inputs(m)
    calls = []
    fwd = Fx.head_xent_fwd
    monkeypatch.setattr(Fx, "head_xent_fwd", lambda *a, **k: calls.append(1) or fwd(*a, **k))
    # the embedding's share of the tied weight's gradient is already in the slot
    prior = torch.randn(w.shape, generator=torch.Generator().manual_seed(9))
    if slot == "main_grad":
        w.main_grad = prior.clone()
        w._dtd_touched = True
    else:
        w.grad = prior.clone()
    loss = head(x, lab)
    loss.backward()
    assert calls == [1]                      # the logit-free path ran
    ref_loss, ref_dx, ref_dw = _reference(x, w, lab)
    got_dw = (w.main_grad if slot == "main_grad" else w.grad) - prior
    assert abs(loss.item() - ref_loss.item()) <= 1e-5
    assert (x.grad - ref_dx).abs().max().item() <= 1e-5
    assert (got_dw - ref_dw).abs().max().item() <= 1e-5
    assert ref_dw.abs().max().item() > 1e-3   # the comparison is not vacuous
    # each sequence's last position and the positions whose next token is -100: exactly zero
    assert torch.equal(x.grad[:, -1], torch.zeros_like(x.grad[:, -1]))
    assert torch.equal(x.grad[1, 2:5], torch.zeros_like(x.grad[1, 2:5]))


def test_first_contribution_overwrites_the_slot():
    """Without an earlier contribution (acc = False) every block overwrites: stale values in a fresh
    main_grad must not survive in any row range."""
    m = _model()
    w = m.embeddings.word
    x, lab = _inputs(m)
    w.main_grad = torch.full(w.shape, 7.0)
    w._dtd_touched = False
    m.head(x, lab).backward()
    _, _, ref_dw = _reference(x, w, lab)
    assert (w.main_grad - ref_dw).abs().max().item() <= 1e-5
    assert w._dtd_touched


def test_default_path_is_unchanged(monkeypatch):
    m = _model()
    m.rt.head_loss = "logits"
    monkeypatch.setattr(Fx, "head_xent_fwd", lambda *a, **k: pytest.fail("fused head ran without the flag"))
    x, lab = _inputs(m)
    m.head(x, lab).backward()
    from distributed_training_and_deepspeed_amd.models.transformer import Runtime
    assert Runtime().head_loss == "logits" and Runtime().head_chunks == 8


def test_one_grad_done_per_backward(monkeypatch):
    """The reducer protocol of the tied weight: one expected use noted in the forward, one ready
    call in the backward, however many blocks the gradient was written in."""
    m = _model(chunks=3)
    w = m.embeddings.word
    noted, done, blocks = [], [], []
    w._dtd_expect = lambda p: noted.append(p)
    w._dtd_ready_hook = lambda p: done.append(p)
    rows = L.wgrad_rows_into
    monkeypatch.setattr(L, "wgrad_rows_into", lambda *a, **k: blocks.append(a[2:4]) or rows(*a, **k))
    x, lab = _inputs(m)
    loss = m.head(x, lab)
    assert len(noted) == 1 and not done
    loss.backward()
    assert len(done) == 1 and done[0] is w
    assert len(blocks) == 3 and blocks[0][0] == 0 and blocks[-1][1] == 1000


def test_transient_bytes_estimate():
    from distributed_training_and_deepspeed_amd.memory import lm_head_transient_bytes
    T, V = 512, 250880
    assert lm_head_transient_bytes(T, V) == 2 * T * V * 2                  # logits + dlogits, bf16
    assert lm_head_transient_bytes(T, V, dtype_bytes=4) == 2 * T * V * 4
    assert lm_head_transient_bytes(T, V, fused=True) == T * (V // 8) * 2  # 31360 = 245 column tiles
    assert lm_head_transient_bytes(T, 50257, fused=True, chunks=3) == T * 16768 * 2
    # past the chunk buffer's addressing limit the rows are split, and the buffer stops growing
    assert lm_head_transient_bytes(131072, V, fused=True) <= Fx.HEAD_XENT_MAX_BLOCK * 2


def test_functional_chunks_match_dense_reference():
    """head_xent_fwd / head_xent_dlogits (math path) against dense fp64, and the chunk buffer view."""
    g = torch.Generator().manual_seed(1)
    T, V, h = 37, 301, 16
    x, w = torch.randn(T, h, generator=g), torch.randn(V, h, generator=g)
    lab = torch.randint(0, V, (T,), generator=g)
    lab[::5] = -100
    loss, lse, stats = Fx.head_xent_fwd(x, w, lab)
    z = x.double() @ w.double().t()
    assert (lse.double() - torch.logsumexp(z, 1)).abs().max().item() <= 1e-5
    assert abs(loss.item() - F.cross_entropy(z, lab, ignore_index=-100).item()) <= 1e-5
    assert stats[1].item() == (lab != -100).sum().item()
    zr = z.clone().requires_grad_(True)
    (F.cross_entropy(zr, lab, ignore_index=-100) * 0.5).backward()
    buf = torch.full((T + 3, 160), -5.0)
    for v0, v1 in ((0, 128), (128, 256), (256, 301)):
        d = Fx.head_xent_dlogits(x, w, lab, lse, stats, torch.tensor(0.5), v0, v1, out=buf)
        assert d.shape == (T, v1 - v0) and d.data_ptr() == buf.data_ptr()
        assert (d.double() - zr.grad[:, v0:v1]).abs().max().item() <= 1e-6
        assert torch.equal(d[::5], torch.zeros_like(d[::5]))
    assert torch.equal(buf[T:], torch.full_like(buf[T:], -5.0))
