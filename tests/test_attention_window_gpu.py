"""The sliding-window flash-attention kernels (``attn_fwd_win_kernel``, ``attn_bwd_dq_win_kernel``,
``attn_bwd_dkdv_win_kernel`` of ops/csrc/attention.hip) against the fp64 oracle, per (token, head) row:
the cases, the oracle and the bounds of ``tests/test_attention_window_cpu.py`` (``check_attention`` of
``tests/test_attention_oracles_cpu.py``, kind ``"kernel"``: min(2e-2, 4 e_staged), lse 1e-5 (1 + A)), none
of them taken from a kernel's result.  Then the dispatch rules (a window of the whole sequence is the
unwindowed call bit for bit), determinism, the rejections, and ``mistral-tiny`` end to end.

W = 1 (``self-only``) is degenerate: every row has one key, so the staged model's error -- and with it
4 e_staged -- is exactly 0 for ctx, dq and dk.  Checked there instead: ctx equals the V row of the
query's key/value head bit for bit (P = 1), lse and dv hold their usual bounds, and dq and dk lie within
2e-2, the project's bf16 cap, of their row scales (dS = P (dP - delta) cancels exactly in fp32 and only
nearly in bf16).
"""
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_and_deepspeed_amd.data import SyntheticLMDataset
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A

from . import oracles as O
from .test_attention_oracles_cpu import CAP_BF16, attention_errors, bounds, print_worst
from .test_attention_oracles_cpu import check_attention as _check
from .test_attention_window_cpu import CASES, DEAD_ROWS, all_cases, case_id, win_case

pytestmark = pytest.mark.gpu

GPU_TITLE = "sliding-window HIP kernels"
BF16, F32 = torch.bfloat16, torch.float32
REGIMES = ("gauss", "spikes_up")
FORM_ENV = ("DTD_ATTN_FWD", "DTD_ATTN_FWD_PK", "DTD_ATTN_OCC", "DTD_ATTN_TILE", "DTD_ATTN_DKDV_BM", "DTD_ATTN_RESCALE_THR",
            "DTD_ATTN_BWD")


@pytest.fixture(autouse=True)
def default_forms(monkeypatch):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)


def run_kernels(c, window="case"):
    """attn_fwd, then attn_bwd on what it returned, on the GPU; ``window`` defaults to the case's."""
    w = c.window if window == "case" else window
    qkv, dctx = c.qkv.cuda(), c.dctx.cuda()
    assert A.kernel_supported(qkv, c.D) and _lib.has("dtd_attn_fwd_win") and _lib.has("dtd_attn_bwd_win")
    kw = dict(key_range=c.key_range, doc_range=c.doc_range, kv_heads=c.kv_heads, window=w)
    ctx, lse, mk = A.attn_fwd(qkv, c.B, c.S, c.H, c.D, True, **kw)
    dqkv = A.attn_bwd(dctx, qkv, ctx, lse, c.B, c.S, c.H, c.D, True, **kw)
    torch.cuda.synchronize()
    assert mk is None and ctx.dtype == BF16 and dqkv.dtype == BF16 and lse.dtype == F32
    return ctx.cpu(), lse.cpu(), dqkv.cpu()


@pytest.mark.parametrize("case", [k for k in all_cases(REGIMES) if k[1] != "self-only"], ids=case_id)
def test_kernels_against_the_oracle(case):
    c = win_case(*case)
    ctx, lse, dqkv = run_kernels(c)
    _check(c, ctx, lse, dqkv, "kernel", "window", title=GPU_TITLE)
    o = c.oracle
    dead = o["lse"] == float("-inf")                     # [B, H, S]
    assert torch.equal(lse == float("-inf"), dead)       # the kernel's -inf set is the oracle's, exactly
    if c.name in DEAD_ROWS:
        assert int(dead.sum()) == DEAD_ROWS[c.name]
    if dead.any():
        rows = dead.permute(0, 2, 1)                     # [B, S, H]
        dq, dk, dv = O.attn_split(dqkv, c.B, c.S, c.H, c.Hkv, c.D)
        assert (ctx.view(c.B, c.S, c.H, c.D)[rows] == 0).all() and (dq[rows] == 0).all()
        unseen = (o["dv"] == 0).all(-1) & (o["dk"] == 0).all(-1)       # keys no query sees: exact zeros
        assert unseen.any() and (dk[unseen] == 0).all() and (dv[unseen] == 0).all()


@pytest.mark.parametrize("regime", REGIMES)
def test_window_of_one_key(regime):
    c = win_case(regime, "self-only")
    ctx, lse, dqkv = run_kernels(c)
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    v = O.attn_split(c.qkv, B, S, H, Hkv, D)[2]          # [B, S, Hkv, D]
    assert torch.equal(ctx.view(B, S, H, D), v.repeat_interleave(H // Hkv, 2))
    err, b = attention_errors(c, ctx, lse, dqkv), bounds(c, "kernel")
    print(f"{c.tag}: " + "  ".join(f"{n} {err[n]:.1e}" for n in err) + f"   bounds lse {b['lse']:.1e} dv {b['dv']:.1e}")
    assert c.e_staged["ctx"] == 0 and c.e_staged["dq"] == 0 and c.e_staged["dk"] == 0
    assert err["lse"] <= b["lse"] and err["dv"] <= b["dv"], (err, b)
    assert err["dq"] <= CAP_BF16 and err["dk"] <= CAP_BF16, err


@pytest.mark.parametrize("name", ["across-tiles", "d128-gqa", "multi-head", "key-range-pad", "documents"])
def test_a_window_of_the_whole_sequence_is_the_unwindowed_call(name):
    """``window >= S`` is dropped before dispatch: the grouped-query path for Hkv < H, the multi-head
    path for Hkv = H, bit for bit."""
    c = win_case("gauss", name)
    base = run_kernels(c, None)
    for w in (0, c.S, c.S + 1000):
        assert all(torch.equal(a, b) for a, b in zip(base, run_kernels(c, w))), w
    assert not torch.equal(base[0], run_kernels(c)[0])


@pytest.mark.parametrize("name", ["across-tiles", "d128-mqa", "group-walk-300", "documents"])
def test_two_calls_are_bitwise_equal(name):
    c = win_case("gauss", name)
    assert all(torch.equal(a, b) for a, b in zip(run_kernels(c), run_kernels(c)))


def test_rejections():
    from distributed_training_and_deepspeed_amd.ops.rng import RngState
    B, S, H, Hkv, D = 1, 64, 4, 2, 64
    qkv = torch.randn(B * S, (H + 2 * Hkv) * D).to(BF16).cuda()
    mh = torch.randn(B * S, 3 * H * D).to(BF16).cuda()
    ctx, lse, _ = A.attn_fwd(mh, B, S, H, D, True, window=16)
    rng = RngState(1, device="cuda")
    with pytest.raises(ValueError):
        A.attn_fwd(qkv, B, S, H, D, False, kv_heads=Hkv, window=16)
    with pytest.raises(ValueError):
        A.attn_fwd(mh, B, S, H, D, False, window=16)
    with pytest.raises(ValueError):
        A.attn_fwd(mh, B, S, H, D, True, p=0.1, rng=rng, window=16)
    with pytest.raises(ValueError):
        A.attn_fwd(mh, B, S, H, D, True, slopes=A.alibi_slopes(H), window=16)
    with pytest.raises(ValueError):
        A.attn_fwd(mh, B, S, H, D, True, window=-1)
    with pytest.raises(ValueError):
        A.attn_bwd(ctx, mh, ctx, lse, B, S, H, D, False, window=16)
    with pytest.raises(ValueError):
        A.attn_bwd(ctx, mh, ctx, lse, B, S, H, D, True, p=0.1, rng=rng, window=16)
    with pytest.raises(ValueError):
        A.attn_bwd(ctx, mh, ctx, lse, B, S, H, D, True, slopes=A.alibi_slopes(H), window=16)
    with pytest.raises(ValueError):
        A.attn_fwd(qkv[:, :3 * Hkv * D].contiguous(), B, S, H, D, True, kv_heads=Hkv, window=16)     # a wrong width
    # the C entry points decline what the Python layer never sends them
    p, st = mh.data_ptr(), _lib.stream()
    fwd = lambda hkv, d, causal, w, kr=None, doc=None: _lib.lib().dtd_attn_fwd_win(   # noqa: E731
        p, p, p, ctx.data_ptr(), lse.data_ptr(), B, S, H, hkv, d, 3 * H * D, H * D, causal, 0.125, w, kr, doc, st)
    for args in ((H, D, 1, 0), (H, D, 0, 16), (3, D, 1, 16), (H + 1, D, 1, 16), (H, 32, 1, 16), (H, D, 1, 16, p, p)):
        assert fwd(*args) != 0, args
    torch.cuda.synchronize()


def test_dbias_falls_back_to_the_column_sums():
    c = win_case("gauss", "group-walk-130")
    q = c.qkv.cuda()
    kw = dict(kv_heads=c.kv_heads, window=c.window)
    ctx, lse, _ = A.attn_fwd(q, c.B, c.S, c.H, c.D, True, **kw)
    db = torch.full((q.shape[1],), 0.25, device="cuda", dtype=F32)
    dqkv = A.attn_bwd(c.dctx.cuda(), q, ctx, lse, c.B, c.S, c.H, c.D, True, dbias=(db, True), **kw)
    ref = dqkv.float().sum(0)
    assert ((db - 0.25) - ref).abs().max().item() <= 1e-3 * (ref.abs().max().item() + 1.0)


# ------------------------------------------------------------------ model
MB, MS = 4, 128


def _spread_norm_weights(model):
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("_g") or n == "final_ln.weight":
                p.mul_(1 + 0.1 * torch.sin(torch.arange(p.numel(), dtype=torch.float32, device=p.device)))


def _inputs(cfg, mode):
    ds = SyntheticLMDataset(cfg, MB, seq_len=MS, seed=5)
    ids, lab = ds.input_ids, ds.labels
    kw = {}
    if mode == "key_padding":
        m = torch.ones(MB, MS, dtype=torch.int64)
        m[0, MS - 29:] = 0           # right-padded
        m[1, :41] = 0                # left-padded
        kw["attention_mask"] = m
    elif mode == "segments":
        from distributed_training_and_deepspeed_amd.data.packing import packed_causal_labels
        seg = torch.zeros(MB, MS, dtype=torch.int64)
        seg[0, :50], seg[0, 50:MS - 11] = 1, 2
        seg[1, :3], seg[1, 3:77], seg[1, 77:] = 1, 2, 3
        seg[2, :] = 1
        seg[3, :64], seg[3, 64:] = 1, 2
        kw["segment_ids"] = seg
        lab = packed_causal_labels(ids, seg)
    return ids, lab, kw


@pytest.mark.parametrize("mode", ["plain", "key_padding", "segments"])
def test_fused_model_matches_reference(mode):
    """mistral-tiny (window 48 at S = 128), bf16 fused on the GPU against the fp32 CPU reference path: the
    bounds of tests/test_attention_gqa_gpu.py::test_fused_model_matches_reference (loss 3e-2, every
    gradient 0.15 in relative L2)."""
    cfg = C.get_config("mistral-tiny")
    ref = build_model("mistral-tiny", impl="reference", seed=3)
    _spread_norm_weights(ref)
    ids, lab, kw = _inputs(cfg, mode)
    l1 = ref(ids, labels=lab, **kw).loss
    l1.backward()
    fus = build_model("mistral-tiny", impl="fused", seed=3, device="cuda")
    fus.load_state_dict(ref.state_dict())
    fus.to(torch.bfloat16)
    l2 = fus(ids.cuda(), labels=lab.cuda(), **{k: v.cuda() for k, v in kw.items()}).loss
    l2.backward()
    assert abs(l1.item() - l2.item()) <= 3e-2 * abs(l1.item()), (l1.item(), l2.item())
    for (n, p1), (_, p2) in zip(ref.named_parameters(), fus.named_parameters()):
        a, b = p1.grad.float(), p2.grad.float().cpu()
        err = (a - b).norm().item() / (a.norm().item() + 1e-12)
        assert err < 0.15, f"{n}: rel err {err}"


def test_captured_step_matches_eager():
    """CapturedStep on mistral-tiny: the replays give the eager steps' losses and parameters.  In a fresh
    child process, as tests/test_attention_gqa_gpu.py::test_captured_step_matches_eager and for the reason
    it gives: the streams and the graph this case creates would shift which hardware queues the later
    captured RCCL cases of the suite's process get."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "import tests.test_attention_window_gpu as t; t._captured_case()"],
                       cwd=root, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "WINDOW_CAPTURE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def _captured_case():
    from distributed_training_and_deepspeed_amd.optim import hf_adamw
    from distributed_training_and_deepspeed_amd.parallel import DistributedDataParallel
    from distributed_training_and_deepspeed_amd.utils.graphs import CapturedStep

    def setup():
        model = build_model("mistral-tiny", dtype=torch.bfloat16, device="cuda", seed=3)
        ddp = DistributedDataParallel(model)
        opt = hf_adamw(ddp.parameters(), lr=1e-3)

        def step(input_ids, labels):
            out = ddp(input_ids, labels=labels)
            out.loss.backward()
            opt.step()
            model.rt.rng.advance()
            return out.loss.detach()
        return model, step

    n = 4
    ds = SyntheticLMDataset(C.get_config("mistral-tiny"), MB * n, seq_len=MS, seed=5)
    ids, lab = ds.input_ids.view(n, MB, MS).cuda(), ds.labels.view(n, MB, MS).cuda()
    ma, sa = setup()
    mb, sb = setup()
    cap = CapturedStep(sb, {"input_ids": ids[0], "labels": lab[0]}, warmup=3, runtime=mb.rt)
    la = [sa(ids[0], lab[0]) for _ in range(3)]
    la += [sa(ids[i], lab[i]) for i in range(1, n)]
    lb = [cap(input_ids=ids[i], labels=lab[i]).clone() for i in range(1, n)]
    torch.cuda.synchronize()
    cap.check()
    assert torch.equal(torch.stack(la[3:]), torch.stack(lb)), (la[3:], lb)
    for (name, p), q in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(p, q), name
    print("WINDOW_CAPTURE_OK", flush=True)


def test_print_worst_ratios():
    assert set(CASES) >= {"self-only"}
    print_worst(GPU_TITLE)
