"""Flash-attention HIP kernels with per-position document spans (sequence packing) vs the math
reference: span edges inside 32 / 64 / 128-tiles, a pad gap that empties a wave, one-token
documents, left pads and all-pad sequences, head_dim 128, tile skipping with the keep-word ring;
no leak between the documents of a row; a packed row against its documents run alone; the
bias-gradient partials; the position-id embedding kernels; and the models' ``segment_ids`` on the
fused path, eager and captured.

Structure, helpers and tolerances are those of tests/test_attention_keyrange_gpu.py."""
import functools

import pytest
import torch

from distributed_training_and_deepspeed_amd.data import SyntheticLMDataset
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.rng import RngState

pytestmark = pytest.mark.gpu

SEED, SID = 11, 9


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


CASES = [
    # B, S, H, D, causal, alibi, p, spans per sequence (the remaining positions are pads)
    (3, 200, 2, 64, False, False, 0.0, [[(0, 200)], [(0, 37), (37, 133), (133, 170)], [(0, 50), (140, 200)]]),
    (2, 256, 2, 64, False, False, 0.1, [[(0, 128), (128, 256)], [(0, 64), (64, 65), (65, 256)]]),
    (3, 256, 2, 64, True, True, 0.0, [[(0, 100), (100, 256)], [(150, 256)], []]),
    (2, 160, 2, 128, True, False, 0.1, [[(0, 160)], [(0, 130), (130, 131), (131, 160)]]),
    (2, 512, 2, 64, False, False, 0.1, [[(0, 128), (128, 256), (256, 384), (384, 512)], [(0, 384), (384, 512)]]),
]
IDS = ["edges-S200-padgap", "S256-onetoken-drop", "causal-alibi-leftpad-empty", "D128", "S512-tile-skip"]


def _segments(spans, S):
    seg = torch.zeros(len(spans), S, dtype=torch.int64)
    for b, row in enumerate(spans):
        for n, (lo, hi) in enumerate(row):
            seg[b, lo:hi] = n + 1
    return seg


def _live(spans, S):
    return _segments(spans, S) != 0


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the CPU math reference of case i -- computed once, shared, never modified."""
    B, S, H, D, causal, alibi, p, spans = CASES[i]
    torch.manual_seed(i)
    qkv = torch.randn(B * S, 3 * H * D).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D).to(torch.bfloat16)
    slopes = A.alibi_slopes(H) if alibi else None
    dr = A.doc_range_from_segment_ids(_segments(spans, S), check=True)
    for b, row in enumerate(spans):                    # the conversion gives the table's spans
        for lo, hi in row:
            assert dr.ranges[b, lo:hi].tolist() == [[lo, hi]] * (hi - lo)
    rc = RngState(SEED, device="cpu")
    ctx_r, lse_r = A.attn_fwd_ref(qkv, B, S, H, D, causal, slopes, p, rc, SID, doc_range=dr)
    dq_r = A.attn_bwd_ref(dctx, qkv, ctx_r, lse_r, B, S, H, D, causal, slopes, p, rc, SID, doc_range=dr)
    assert torch.isfinite(ctx_r.float()).all() and torch.isfinite(dq_r.float()).all() and not torch.isnan(lse_r).any()
    return qkv, dctx, slopes, dr, ctx_r, lse_r, dq_r


def _run(qkv, dctx, case, dr, dbias=None):
    B, S, H, D, causal, alibi, p, _ = case
    slopes = A.alibi_slopes(H) if alibi else None
    rg = RngState(SEED, device="cuda")
    q = qkv.cuda()
    assert A.kernel_supported(q, D) and _lib.has("dtd_attn_fwd_doc") and _lib.has("dtd_attn_bwd_doc")
    drg = A.DocRange(*(t.cuda() for t in dr)) if dr is not None else None
    ctx, lse, mk = A.attn_fwd(q, B, S, H, D, causal, slopes, p, rg, SID, doc_range=drg)
    dqkv = A.attn_bwd(dctx.cuda(), q, ctx, lse, B, S, H, D, causal, slopes, p, rg, SID, mk, dbias=dbias,
                      doc_range=drg)
    torch.cuda.synchronize()
    return ctx, lse, dqkv


def _check_against(case, got, ref, rows=None):
    """``rows``: optional [B, S] bool -- compare these positions only."""
    B, S, H, D = case[:4]
    (ctx_g, lse_g, dq_g), (ctx_r, lse_r, dq_r) = got, ref
    assert torch.isfinite(ctx_g.float()).all() and torch.isfinite(dq_g.float()).all()
    lse_g, lse_r = lse_g.float().cpu(), lse_r.float().cpu()
    assert not torch.isnan(lse_g).any()
    rows = torch.ones(B, S, dtype=torch.bool) if rows is None else rows
    e_ctx = rel(ctx_g.view(B, S, -1).cpu()[rows], ctx_r.view(B, S, -1).cpu()[rows])
    lg, lr = lse_g.transpose(1, 2)[rows], lse_r.transpose(1, 2)[rows]
    dead = lr == float("-inf")
    e_lse = (lg[~dead] - lr[~dead]).abs().max().item()
    g, r = dq_g.view(B, S, 3, H, D).cpu()[rows], dq_r.view(B, S, 3, H, D).cpu()[rows]
    errs = [rel(g[:, i], r[:, i]) for i in range(3)]
    print(f"ctx rel {e_ctx:.3e}  lse abs {e_lse:.3e}  dq/dk/dv rel {errs}")
    assert e_ctx < 1e-2, e_ctx
    assert torch.equal(lg == float("-inf"), dead)              # exactly -inf where the reference is
    assert e_lse < 2e-2, e_lse
    for name, e in zip("qkv", errs):
        assert e < 2e-2, f"d{name} rel err {e}"
    return lse_r == float("-inf")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_doc_kernels_match_reference(i):
    case = CASES[i]
    B, S, H, D, causal, alibi, p, spans = case
    qkv, dctx, slopes, dr, ctx_r, lse_r, dq_r = _case(i)
    got = _run(qkv, dctx, case, dr)
    dead = _check_against(case, got, (ctx_r, lse_r, dq_r))
    ctx_g, _, dq_g = got
    # the dead rows are the pads; their ctx and dq are exactly 0, and pad keys get dk = dv = 0
    live = _live(spans, S)
    assert torch.equal(dead, ~live.view(B, 1, S).expand(B, H, S))
    assert (ctx_g.view(B, S, H * D).cpu()[~live] == 0).all()
    g = dq_g.view(B, S, 3 * H * D).cpu()
    assert (g[~live] == 0).all()


def _refill_others(qkv, case, keep, gen_seed):
    """q, k and v rows of every position outside document ``keep`` = (sequence, lo, hi) of that
    sequence -- its other documents and its pads -- replaced by finite values up to 1e4."""
    B, S, H, D = case[:4]
    b, lo, hi = keep
    x = qkv.clone().view(B, S, 3 * H * D)
    g = torch.Generator().manual_seed(gen_seed)
    out = torch.ones(S, dtype=torch.bool)
    out[lo:hi] = False
    x[b, out] = ((torch.rand(int(out.sum()), 3 * H * D, generator=g) * 2 - 1) * 1e4).to(torch.bfloat16)
    return x.view(B * S, 3 * H * D)


@pytest.mark.parametrize("i,keep", [(0, (1, 37, 133)), (0, (2, 140, 200)), (4, (0, 256, 384)), (4, (1, 384, 512))],
                         ids=["S200-middle-doc", "S200-doc-after-gap", "S512-third-doc", "S512-late-doc"])
def test_no_cross_document_leak(i, keep):
    case = CASES[i]
    B, S, H, D = case[:4]
    qkv, dctx, _, dr, *_ = _case(i)
    b, lo, hi = keep
    a = _run(_refill_others(qkv, case, keep, 1), dctx, case, dr)
    c = _run(_refill_others(qkv, case, keep, 2), dctx, case, dr)
    assert torch.equal(a[0].view(B, S, -1)[b, lo:hi], c[0].view(B, S, -1)[b, lo:hi]), "ctx"
    assert torch.equal(a[1][b, :, lo:hi], c[1][b, :, lo:hi]), "lse"
    assert torch.equal(a[2].view(B, S, -1)[b, lo:hi], c[2].view(B, S, -1)[b, lo:hi]), "dq / dk / dv"
    # and the other rows did not leak into the document: still the reference of the original input
    rows = torch.zeros(B, S, dtype=torch.bool)
    rows[b, lo:hi] = True
    _check_against(case, a, _case(i)[4:], rows)


@pytest.mark.parametrize("causal_alibi", [False, True], ids=["plain", "causal-alibi"])
def test_packed_equals_separate(causal_alibi):
    """Each document of case 1's sequence 1, run alone through the unranged kernel (B = 1, S = its
    length), agrees with its rows of the packed run.  Not bitwise: the tiles differ, and with ALiBi
    the absolute key positions (a per-row constant the softmax cancels)."""
    B, S, H, D, _, _, _, spans = CASES[0]
    qkv, dctx, _, dr, *_ = _case(0)
    case = (B, S, H, D, causal_alibi, causal_alibi, 0.0, spans)
    ctx_p, lse_p, dq_p = _run(qkv, dctx, case, dr)
    for lo, hi in spans[1]:
        n = hi - lo
        one = (1, n, H, D, causal_alibi, causal_alibi, 0.0, None)
        q1 = qkv.view(B, S, -1)[1, lo:hi].contiguous()
        d1 = dctx.view(B, S, -1)[1, lo:hi].contiguous()
        ctx_s, lse_s, dq_s = _run(q1, d1, one, None)
        lse_s = lse_s.float().cpu()
        if causal_alibi:     # the packed rows carry slope * lo more bias on every key: lse shifts by it
            lse_s = lse_s + (A.alibi_slopes(H) * lo).view(1, H, 1)
        packed = (ctx_p.view(B, S, -1)[1:2, lo:hi].reshape(n, -1), lse_p[1:2, :, lo:hi],
                  dq_p.view(B, S, -1)[1:2, lo:hi].reshape(n, -1))
        _check_against(one, packed, (ctx_s.cpu(), lse_s, dq_s.cpu()))


@pytest.mark.parametrize("i", [0, 1, 2, 4], ids=[IDS[0], IDS[1], IDS[2], IDS[4]])
def test_bias_partials_with_doc_range_are_the_column_sums(i):
    """Every bias_part row is written (all-pad dK/dV blocks write zeros): the finalized qkv bias
    gradient equals the column sums of the returned dqkv."""
    case = CASES[i]
    H, D = case[2], case[3]
    qkv, dctx, _, dr, *_ = _case(i)
    db = torch.full((3 * H * D,), 0.25, device="cuda", dtype=torch.float32)
    # attn_bwd takes its partials buffer from torch.empty: leave NaNs in a freed block of that size,
    # so a partial row that a skipped block failed to write would most likely show up in the sum
    B, S = case[0], case[1]
    junk = torch.full((B * 4 * ((S + 127) // 128), 3 * H * D), float("nan"), device="cuda", dtype=torch.float32)
    del junk
    _, _, dq_b = _run(qkv, dctx, case, dr, dbias=(db, True))
    _, _, dq_g = _run(qkv, dctx, case, dr)
    assert torch.equal(dq_b, dq_g)
    ref_db = dq_g.float().sum(0)
    assert ((db - 0.25) - ref_db).abs().max().item() <= 1e-3 * (ref_db.abs().max().item() + 1.0)


@pytest.mark.parametrize("i", [1, 2], ids=[IDS[1], IDS[2]])
def test_one_span_per_row_agrees_with_no_range(i):
    case = CASES[i]
    B, S = case[0], case[1]
    qkv, dctx, *_ = _case(i)
    full = A.doc_range_from_segment_ids(torch.ones(B, S, dtype=torch.int64))
    assert full.ranges.tolist() == [[[0, S]] * S] * B
    _check_against(case, _run(qkv, dctx, case, full), tuple(t.cpu() for t in _run(qkv, dctx, case, None)))


# ------------------------------------------------------------------ embedding with position ids
def test_embedding_with_position_ids_matches_cpu_branch():
    """dtd_embed_fwd_pos and the sorted position-table gradient vs the CPU branch: rows = 2 x 96,
    h = 64, positions that restart twice per row.  The bf16 forward is exact (the same fp32 sum,
    rounded once); the gradient is compared with fp32 index_add_."""
    assert _lib.has("dtd_embed_fwd_pos")
    B, S, h, V, P, off = 2, 96, 64, 50, 100, 2
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, V, (B, S), generator=g)
    tids = torch.randint(0, 2, (B, S), generator=g)
    pos_ids = torch.cat([torch.arange(30), torch.arange(35), torch.arange(31)]).repeat(B, 1)   # restarts twice
    pos_ids[1] = torch.cat([torch.arange(10), torch.arange(38), torch.zeros(10, dtype=torch.int64), torch.arange(38)])
    word, pos, typ = (torch.randn(n, h, generator=g).to(torch.bfloat16) for n in (V, P + off, 2))
    want = Fx.embed_fwd(ids, word, pos, typ, S, off, type_ids=tids, position_ids=pos_ids)
    got = Fx.embed_fwd(ids.cuda(), word.cuda(), pos.cuda(), typ.cuda(), S, off, type_ids=tids.cuda(),
                       position_ids=pos_ids.cuda())
    assert torch.equal(got.cpu(), want)
    # and it is not the positions of the row index
    assert not torch.equal(want, Fx.embed_fwd(ids, word, pos, typ, S, off, type_ids=tids))
    dz = torch.randn(B * S, h, generator=g).to(torch.bfloat16)
    ref = torch.zeros(P + off, h).index_add_(0, pos_ids.reshape(-1) + off, dz.float())
    for acc in (False, True):
        grad = torch.full((P + off, h), 0.5, device="cuda")
        Fx.embed_pos_bwd(dz.cuda(), grad, B, S, off, acc, position_ids=pos_ids.cuda())
        torch.cuda.synchronize()
        assert rel(grad.cpu() - (0.5 if acc else 0.0), ref) < 1e-2
        gc = torch.full((P + off, h), 0.5)
        Fx.embed_pos_bwd(dz, gc, B, S, off, acc, position_ids=pos_ids)
        assert rel(gc - (0.5 if acc else 0.0), ref) < 1e-2


# ------------------------------------------------------------------ models
def _pair(name):
    # (the causal preset keeps GPT-2's pad id, which lies outside the tiny vocabulary)
    cfg = C.get_config(name).with_(pad_token_id=0)
    C.PRESETS["_dm"] = cfg
    ref = build_model("_dm", impl="reference", seed=3)
    fus = build_model("_dm", impl="fused", seed=3, device="cuda")
    fus.load_state_dict(ref.state_dict())
    fus.to(torch.bfloat16)
    return cfg, ref, fus


@pytest.mark.parametrize("name", ["tiny", "causal-tiny"])
def test_fused_model_with_segment_ids_matches_reference(name):
    """bf16 fused path vs the fp32 CPU reference path on a packed batch with segment_ids: loss and
    parameter gradients, with test_model_gpu.py's fused-vs-reference bf16 tolerances."""
    cfg, ref, fus = _pair(name)
    ds = SyntheticLMDataset(cfg, 4, seq_len=128, seed=5, pad_fraction=0.75, max_docs=3)
    ids, lab, seg = ds.input_ids, ds.labels, ds.segment_ids
    assert int(seg.max()) > 1 and int((seg == 0).sum()) > 0            # several documents, some padding
    l1 = ref(ids, labels=lab, segment_ids=seg).loss
    l1.backward()
    l2 = fus(ids.cuda(), labels=lab.cuda(), segment_ids=seg.cuda()).loss
    l2.backward()
    l0 = ref(ids, labels=lab).loss.item()
    print(f"loss reference {l1.item():.5f} fused {l2.item():.5f} (no segment ids: {l0:.5f})")
    assert abs(l1.item() - l2.item()) <= 3e-2 * abs(l1.item())
    for (n, p1), (_, p2) in zip(ref.named_parameters(), fus.named_parameters()):
        g1, g2 = p1.grad.float(), p2.grad.float().cpu()
        err = (g1 - g2).norm().item() / (g1.norm().item() + 1e-12)
        assert err < 0.15, f"{n}: rel err {err}"


def test_captured_step_with_segment_ids_replays_to_the_eager_loss():
    """The segment ids are a third static input of the captured step (doc_range_from_segment_ids and
    the position ids run inside the graph, no host sync): replays equal the same steps run eagerly."""
    from distributed_training_and_deepspeed_amd.optim import hf_adamw
    from distributed_training_and_deepspeed_amd.parallel import DistributedDataParallel
    from distributed_training_and_deepspeed_amd.utils.graphs import CapturedStep, mlm_capacity

    def setup():
        model = build_model("tiny", dtype=torch.bfloat16, device="cuda", seed=3)
        model.rt.mlm_capacity = mlm_capacity(4 * 128)
        model.rt.mlm_overflow = torch.zeros((), dtype=torch.bool, device="cuda")
        ddp = DistributedDataParallel(model)
        opt = hf_adamw(ddp.parameters(), lr=1e-3)

        def step(input_ids, labels, segment_ids):
            out = ddp(input_ids, labels=labels, segment_ids=segment_ids)
            out.loss.backward()
            opt.step()
            model.rt.rng.advance()
            return out.loss.detach()
        return model, step

    n = 4
    ds = SyntheticLMDataset(build_model("tiny").cfg, 4 * n, seq_len=128, seed=5, pad_fraction=0.75, max_docs=3)
    ids, lab, seg = (t.view(n, 4, 128).cuda() for t in (ds.input_ids, ds.labels, ds.segment_ids))
    ma, sa = setup()
    mb, sb = setup()
    cap = CapturedStep(sb, {"input_ids": ids[0], "labels": lab[0], "segment_ids": seg[0]}, warmup=3, runtime=mb.rt)
    la = [sa(ids[0], lab[0], seg[0]) for _ in range(3)]
    la += [sa(ids[i], lab[i], seg[i]) for i in range(1, n)]
    lb = [cap(input_ids=ids[i], labels=lab[i], segment_ids=seg[i]).clone() for i in range(1, n)]
    torch.cuda.synchronize()
    cap.check()
    assert torch.equal(torch.stack(la[3:]), torch.stack(lb))
    for (name, p), q in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(p, q), name
