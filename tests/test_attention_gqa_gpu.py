"""Grouped-query flash attention on the GPU: the GQA forward / dQ / dK,dV kernels against the CPU math
reference (a head seam at every tile step, a ragged last block, MQA, varying tile counts per key
block, both ``xcd_tile`` branches, head_dim 128, key ranges with a whole key block outside, document
spans with pads), the unchanged multi-head path, the rejections, the rotary kernel with ``kv_heads``,
and ``llama-tiny-gqa`` fused against its reference, eager and captured.

Tolerances are those of tests/test_attention_docmask_gpu.py (ctx rel 1e-2, lse abs 2e-2, dq / dk / dv
rel 2e-2): the dK/dV sum over a group is accumulated in fp32 and rounded once, like one head's."""
import functools

import pytest
import torch

from distributed_training_and_deepspeed_amd.data import SyntheticLMDataset
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx

from .test_gqa_cpu import angles_f64, rope_f64

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _segments(spans, S):
    seg = torch.zeros(len(spans), S, dtype=torch.int64)
    for b, row in enumerate(spans):
        for n, (lo, hi) in enumerate(row):
            seg[b, lo:hi] = n + 1
    return seg


DOC_SPANS = [[(0, 100), (100, 256)], [(150, 256)], []]
CASES = {
    # B, S, H, Hkv, D, causal, key ranges, document spans
    # one query tile per head: every tile step of dK/dV is a head seam; grids 3*4 / 3*2: xcd_tile's identity branch
    "seam-every-tile": (3, 96, 4, 2, 64, False, None, None),
    "ragged-mqa": (2, 200, 4, 1, 64, True, None, None),
    # 3, 2 and 1 query tiles per key block; dK/dV grid 3*4 (identity), forward / dQ grid 3*16 (remapped)
    "tiles-3-2-1": (2, 384, 8, 2, 64, True, None, None),
    "dkdv-grid-8": (2, 256, 4, 2, 64, True, None, None),           # dK/dV grid 2*4 = 8: remapped as well
    "D128": (2, 160, 2, 1, 128, True, None, None),
    # sequence 0 left-padded (key block 0 wholly outside), sequence 1 right-padded (key block 1 wholly outside)
    "key-range": (2, 200, 4, 1, 64, True, [[140, 200], [0, 100]], None),
    "doc-range": (3, 256, 4, 2, 64, True, None, DOC_SPANS),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the CPU math reference of a case -- computed once, shared, never modified."""
    B, S, H, Hkv, D, causal, kr, spans = CASES[name]
    torch.manual_seed(sorted(CASES).index(name))
    qkv = torch.randn(B * S, (H + 2 * Hkv) * D).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D).to(torch.bfloat16)
    kw = {}
    if kr is not None:
        kw["key_range"] = torch.tensor(kr, dtype=torch.int32)
    if spans is not None:
        kw["doc_range"] = A.doc_range_from_segment_ids(_segments(spans, S), check=True)
    ctx_r, lse_r = A.attn_fwd_ref(qkv, B, S, H, D, causal, kv_heads=Hkv, **kw)
    dq_r = A.attn_bwd_ref(dctx, qkv, ctx_r, lse_r, B, S, H, D, causal, kv_heads=Hkv, **kw)
    assert torch.isfinite(ctx_r.float()).all() and torch.isfinite(dq_r.float()).all() and not torch.isnan(lse_r).any()
    return qkv, dctx, kw, ctx_r, lse_r, dq_r


def _run(name):
    B, S, H, Hkv, D, causal, _, _ = CASES[name]
    qkv, dctx, kw, *_ = _case(name)
    q = qkv.cuda()
    assert A.kernel_supported(q, D) and _lib.has("dtd_attn_fwd_gqa") and _lib.has("dtd_attn_bwd_gqa")
    kwg = {}
    if "key_range" in kw:
        kwg["key_range"] = kw["key_range"].cuda()
    if "doc_range" in kw:
        kwg["doc_range"] = A.DocRange(*(t.cuda() for t in kw["doc_range"]))
    ctx, lse, mk = A.attn_fwd(q, B, S, H, D, causal, kv_heads=Hkv, **kwg)
    assert mk is None
    dqkv = A.attn_bwd(dctx.cuda(), q, ctx, lse, B, S, H, D, causal, kv_heads=Hkv, **kwg)
    torch.cuda.synchronize()
    assert tuple(ctx.shape) == (B * S, H * D) and tuple(lse.shape) == (B, H, S) and dqkv.shape == q.shape
    return ctx.cpu(), lse.float().cpu(), dqkv.cpu()


def _check(name, got):
    B, S, H, Hkv, D = CASES[name][:5]
    _, _, _, ctx_r, lse_r, dq_r = _case(name)
    ctx_g, lse_g, dq_g = got
    assert torch.isfinite(ctx_g.float()).all() and torch.isfinite(dq_g.float()).all() and not torch.isnan(lse_g).any()
    lse_r = lse_r.float()
    dead = lse_r == float("-inf")
    e_ctx = rel(ctx_g, ctx_r)
    e_lse = (lse_g[~dead] - lse_r[~dead]).abs().max().item()
    g, r = dq_g.view(B * S, H + 2 * Hkv, D), dq_r.view(B * S, H + 2 * Hkv, D)
    parts = {"q": slice(0, H), "k": slice(H, H + Hkv), "v": slice(H + Hkv, H + 2 * Hkv)}
    errs = {n: rel(g[:, s], r[:, s]) for n, s in parts.items()}
    print(f"{name}: ctx rel {e_ctx:.3e}  lse abs {e_lse:.3e}  dq/dk/dv rel {errs}")
    assert e_ctx < 1e-2, e_ctx
    assert torch.equal(lse_g == float("-inf"), dead)              # exactly -inf where the reference is
    assert e_lse < 2e-2, e_lse
    for n, e in errs.items():
        assert e < 2e-2, f"d{n} rel err {e}"
    # every key/value head on its own: a group summed into the wrong head's columns averages out above
    for hk in range(Hkv):
        for n in "kv":
            s = parts[n].start + hk
            assert rel(g[:, s], r[:, s]) < 2e-2, (n, hk)
    # exact zeros where masking puts them: a row without a key has ctx = 0 and dq = 0 (the keys outside a
    # range and the pads are checked by the ranged tests).  Not every zero of the reference: causal
    # query 0 sees one key, so its dS = P (dP - delta) cancels exactly in fp32 and only nearly in bf16.
    dead_rows = dead.transpose(1, 2).reshape(B * S, H)               # [B, H, S] -> [B*S, H]
    assert (ctx_r.view(B * S, H, D)[dead_rows] == 0).all() and (r[:, :H][dead_rows] == 0).all()
    assert (ctx_g.view(B * S, H, D)[dead_rows] == 0).all() and (g[:, :H][dead_rows] == 0).all()
    return dead


@pytest.mark.parametrize("name", ["seam-every-tile", "ragged-mqa", "tiles-3-2-1", "dkdv-grid-8", "D128"])
def test_gqa_kernels_match_reference(name):
    _check(name, _run(name))


def test_gqa_kernels_with_key_range():
    name = "key-range"
    B, S, H, Hkv, D, _, kr, _ = CASES[name]
    got = _run(name)
    dead = _check(name, got)
    ctx_g, _, dq_g = got
    # causal and left-padded: the queries in front of the range have no key
    want_dead = torch.zeros(B, H, S, dtype=torch.bool)
    want_dead[0, :, :140] = True
    assert torch.equal(dead, want_dead)
    assert (ctx_g.view(B, S, H * D)[0, :140] == 0).all()
    g = dq_g.view(B, S, H + 2 * Hkv, D)
    assert (g[0, :140, :H] == 0).all()                               # dq of the rows without a key
    for b, (lo, hi) in enumerate(kr):                                # dk = dv = 0 outside the range: the whole
        out = torch.ones(S, dtype=torch.bool)                        # key block 0 of sequence 0, 1 of sequence 1
        out[lo:hi] = False
        assert (g[b, out, H:] == 0).all(), b
        assert (g[b, ~out, H:] != 0).any(), b


def test_gqa_kernels_with_doc_range():
    name = "doc-range"
    B, S, H, Hkv, D = CASES[name][:5]
    got = _run(name)
    dead = _check(name, got)
    ctx_g, _, dq_g = got
    live = _segments(DOC_SPANS, S) != 0
    assert torch.equal(dead, ~live.view(B, 1, S).expand(B, H, S))    # the dead rows are the pads
    assert (ctx_g.view(B, S, H * D)[~live] == 0).all()
    assert (dq_g.view(B, S, (H + 2 * Hkv) * D)[~live] == 0).all()    # dq = dk = dv = 0 exactly


def test_results_are_reproducible():
    a, b = _run("tiles-3-2-1"), _run("tiles-3-2-1")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_multi_head_path_is_unchanged():
    """kv_heads = H and kv_heads = None are the call without the argument, bitwise."""
    B, S, H, D = 2, 200, 2, 64
    torch.manual_seed(3)
    qkv = torch.randn(B * S, 3 * H * D).to(torch.bfloat16).cuda()
    dctx = torch.randn(B * S, H * D).to(torch.bfloat16).cuda()
    kr = torch.tensor([[0, 150], [30, 200]], dtype=torch.int32).cuda()

    def run(**kw):
        ctx, lse, _ = A.attn_fwd(qkv, B, S, H, D, True, **kw)
        return ctx, lse, A.attn_bwd(dctx, qkv, ctx, lse, B, S, H, D, True, **kw)

    for extra in ({}, {"key_range": kr}):
        base = run(**extra)
        for kvh in (H, None):
            got = run(kv_heads=kvh, **extra)
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(base, got)), (kvh, list(extra))


def test_rejections():
    B, S, H, Hkv, D = 1, 64, 4, 2, 64
    qkv = torch.randn(B * S, (H + 2 * Hkv) * D).to(torch.bfloat16).cuda()
    ctx, lse, _ = A.attn_fwd(qkv, B, S, H, D, True, kv_heads=Hkv)
    from distributed_training_and_deepspeed_amd.ops.rng import RngState
    rng = RngState(1, device="cuda")
    with pytest.raises(ValueError):
        A.attn_fwd(qkv, B, S, H, D, True, p=0.1, rng=rng, kv_heads=Hkv)
    with pytest.raises(ValueError):
        A.attn_fwd(qkv, B, S, H, D, True, slopes=A.alibi_slopes(H), kv_heads=Hkv)
    with pytest.raises(ValueError):
        A.attn_bwd(ctx, qkv, ctx, lse, B, S, H, D, True, p=0.1, rng=rng, kv_heads=Hkv)
    with pytest.raises(ValueError):
        A.attn_bwd(ctx, qkv, ctx, lse, B, S, H, D, True, slopes=A.alibi_slopes(H), kv_heads=Hkv)
    with pytest.raises(ValueError):
        A.attn_fwd(qkv[:, :3 * Hkv * D].contiguous(), B, S, H, D, True, kv_heads=Hkv)     # a wrong width


def test_dbias_falls_back_to_the_column_sums():
    name = "seam-every-tile"
    B, S, H, Hkv, D, causal, _, _ = CASES[name]
    qkv, dctx, *_ = _case(name)
    q = qkv.cuda()
    ctx, lse, _ = A.attn_fwd(q, B, S, H, D, causal, kv_heads=Hkv)
    db = torch.full(((H + 2 * Hkv) * D,), 0.25, device="cuda", dtype=torch.float32)
    dqkv = A.attn_bwd(dctx.cuda(), q, ctx, lse, B, S, H, D, causal, kv_heads=Hkv, dbias=(db, True))
    ref = dqkv.float().sum(0)
    assert ((db - 0.25) - ref).abs().max().item() <= 1e-3 * (ref.abs().max().item() + 1.0)


# ------------------------------------------------------------------ rotary embedding
@pytest.mark.parametrize("B,S,H,Hkv,D", [(2, 96, 4, 2, 64), (1, 130, 2, 1, 128)])
@pytest.mark.parametrize("with_pos", [False, True], ids=["arange", "random_pos"])
def test_rope_with_kv_heads(B, S, H, Hkv, D, with_pos):
    assert _lib.has("dtd_rope_heads")
    torch.manual_seed(1)
    table = Fx.rope_table(4096, D, 10000.0)
    pos = torch.randint(0, 4096, (B, S), dtype=torch.int32) if with_pos else None
    x = torch.randn(B * S, (H + 2 * Hkv) * D).to(torch.bfloat16)
    nrot = H + Hkv
    flat = torch.arange(S).repeat(B) if pos is None else pos.reshape(-1)
    xg = x.cuda()
    for inverse in (False, True):
        want = rope_f64(x, angles_f64(flat, D) * (-1.0 if inverse else 1.0), nrot, D)
        got = Fx.rope_(xg.clone(), table.cuda(), B, S, H, D, pos=pos.cuda() if with_pos else None, inverse=inverse,
                       kv_heads=Hkv)
        torch.cuda.synchronize()
        # tests/test_llama_ops_gpu.py's close() at its bf16 bound: max error <= 2e-2 of the reference's max
        err = (got.double().cpu() - want).abs().max().item()
        assert err <= 2e-2 * (want.abs().max().item() + 1e-6), err
        assert torch.equal(got[:, nrot * D:], xg[:, nrot * D:])            # v: bitwise untouched
        assert not torch.equal(got[:, H * D:nrot * D], xg[:, H * D:nrot * D])   # the k block was rotated


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
    """llama-tiny-gqa, bf16 fused on the GPU against the fp32 CPU reference path: the bf16 bounds of
    tests/test_llama_model_gpu.py (loss 3e-2, every gradient 0.15 in relative L2)."""
    cfg = C.get_config("llama-tiny-gqa")
    ref = build_model("llama-tiny-gqa", impl="reference", seed=3)
    _spread_norm_weights(ref)
    ids, lab, kw = _inputs(cfg, mode)
    l1 = ref(ids, labels=lab, **kw).loss
    l1.backward()
    fus = build_model("llama-tiny-gqa", impl="fused", seed=3, device="cuda")
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
    """CapturedStep on llama-tiny-gqa: the replays give the eager steps' losses (and parameters), as
    tests/test_llama_model_gpu.py::test_captured_step_matches_eager.

    The case runs in a fresh child process.  It draws streams (the optimizers' and the capture's side
    streams) and instantiates a graph with a parallel branch; which hardware queues the streams of
    later graphs share depends on how many were created before them in the process, and
    tests/test_graph_gpu.py's captured RCCL cases, which run in the suite's process after this file,
    are sensitive to exactly that (README, "hipGraph replay").  A child leaves that sequence as it was."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "import tests.test_attention_gqa_gpu as t; t._captured_case()"],
                       cwd=root, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "GQA_CAPTURE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def _captured_case():
    from distributed_training_and_deepspeed_amd.optim import hf_adamw
    from distributed_training_and_deepspeed_amd.parallel import DistributedDataParallel
    from distributed_training_and_deepspeed_amd.utils.graphs import CapturedStep

    def setup():
        model = build_model("llama-tiny-gqa", dtype=torch.bfloat16, device="cuda", seed=3)
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
    ds = SyntheticLMDataset(C.get_config("llama-tiny-gqa"), MB * n, seq_len=MS, seed=5)
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
    print("GQA_CAPTURE_OK", flush=True)
