"""Flash-attention HIP kernels with per-sequence key ranges (key-padding masks) vs the math
reference: tile skipping at range edges inside / between tiles, the masked dK/dV dispatch at
S % 128 == 0, rows and sequences without any key, dropout keep words of a range that starts at a
late tile, head_dim 128; independence from the masked K / V rows; the bias-gradient partials of
skipped blocks; and the models' ``attention_mask`` on the fused path, eager and captured.

Tolerances are those of tests/test_attention_gpu.py and tests/test_model_gpu.py."""
import functools

import pytest
import torch

from distributed_training_and_deepspeed_amd.data import SyntheticLMDataset
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops.rng import RngState

pytestmark = pytest.mark.gpu

SEED, SID = 11, 9


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


CASES = [
    # B, S, H, D, causal, alibi, p, ranges
    (3, 200, 2, 64, False, False, 0.0, [(0, 200), (0, 70), (37, 133)]),     # edges inside 32/64/128 tiles, odd S
    (2, 256, 2, 64, False, False, 0.1, [(0, 256), (0, 96)]),                # MASK=false dK/dV + fast softmax dispatch
    (3, 256, 2, 64, True, True, 0.0, [(0, 256), (150, 256), (0, 0)]),       # left pad: rows q < lo; an empty sequence
    (2, 160, 2, 128, True, False, 0.1, [(0, 160), (130, 131)]),             # D = 128, one key in the last tile
    (2, 512, 2, 64, False, False, 0.1, [(0, 512), (384, 512)]),             # range from a late tile: ring, keep words
]
IDS = ["edges-S200", "S256-drop", "causal-alibi-leftpad-empty", "D128-onekey", "S512-late-tile"]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the CPU math reference of case i -- computed once, shared, never modified."""
    B, S, H, D, causal, alibi, p, ranges = CASES[i]
    torch.manual_seed(i)
    qkv = torch.randn(B * S, 3 * H * D).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D).to(torch.bfloat16)
    slopes = A.alibi_slopes(H) if alibi else None
    kr = torch.tensor(ranges, dtype=torch.int32)
    rc = RngState(SEED, device="cpu")
    ctx_r, lse_r = A.attn_fwd_ref(qkv, B, S, H, D, causal, slopes, p, rc, SID, key_range=kr)
    dq_r = A.attn_bwd_ref(dctx, qkv, ctx_r, lse_r, B, S, H, D, causal, slopes, p, rc, SID, key_range=kr)
    assert torch.isfinite(ctx_r.float()).all() and torch.isfinite(dq_r.float()).all() and not torch.isnan(lse_r).any()
    return qkv, dctx, slopes, kr, ctx_r, lse_r, dq_r


def _run(qkv, dctx, case, kr, dbias=None):
    B, S, H, D, causal, alibi, p, _ = case
    slopes = A.alibi_slopes(H) if alibi else None
    rg = RngState(SEED, device="cuda")
    q = qkv.cuda()
    assert A.kernel_supported(q, D) and _lib.has("dtd_attn_fwd_range") and _lib.has("dtd_attn_bwd_range")
    krg = kr.cuda() if kr is not None else None
    ctx, lse, mk = A.attn_fwd(q, B, S, H, D, causal, slopes, p, rg, SID, key_range=krg)
    dqkv = A.attn_bwd(dctx.cuda(), q, ctx, lse, B, S, H, D, causal, slopes, p, rg, SID, mk, dbias=dbias,
                      key_range=krg)
    torch.cuda.synchronize()
    return ctx, lse, dqkv


def _check_against(case, got, ref):
    B, S, H, D = case[:4]
    (ctx_g, lse_g, dq_g), (ctx_r, lse_r, dq_r) = got, ref
    assert torch.isfinite(ctx_g.float()).all() and torch.isfinite(dq_g.float()).all()
    lse_g, lse_r = lse_g.float().cpu(), lse_r.float().cpu()
    assert not torch.isnan(lse_g).any()
    e_ctx = rel(ctx_g, ctx_r)
    dead = lse_r == float("-inf")
    e_lse = (lse_g[~dead] - lse_r[~dead]).abs().max().item()
    g, r = dq_g.view(B, S, 3, H, D).cpu(), dq_r.view(B, S, 3, H, D).cpu()
    errs = [rel(g[:, :, i], r[:, :, i]) for i in range(3)]
    print(f"ctx rel {e_ctx:.3e}  lse abs {e_lse:.3e}  dq/dk/dv rel {errs}")
    assert e_ctx < 1e-2, e_ctx
    assert torch.equal(lse_g == float("-inf"), dead)           # exactly -inf where the reference is
    assert e_lse < 2e-2, e_lse
    for name, e in zip("qkv", errs):
        assert e < 2e-2, f"d{name} rel err {e}"
    return dead


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_ranged_kernels_match_reference(i):
    case = CASES[i]
    B, S, H, D, causal, alibi, p, ranges = case
    qkv, dctx, slopes, kr, ctx_r, lse_r, dq_r = _case(i)
    got = _run(qkv, dctx, case, kr)
    dead = _check_against(case, got, (ctx_r, lse_r, dq_r))
    ctx_g, _, dq_g = got
    # rows without a key: ctx and dq exactly 0; keys outside a range: dk, dv exactly 0
    assert dead.any().item() == any(lo >= hi or (causal and lo > 0) for lo, hi in ranges)
    dead_rows = dead.transpose(1, 2)                                         # [B, S, H]
    assert (ctx_g.view(B, S, H, D).cpu()[dead_rows] == 0).all()
    g = dq_g.view(B, S, 3, H, D).cpu()
    assert (g[:, :, 0][dead_rows] == 0).all()
    for b, (lo, hi) in enumerate(ranges):
        assert (g[b, :lo, 1:] == 0).all() and (g[b, hi:, 1:] == 0).all(), b


def _refill_outside(qkv, case, gen_seed):
    """K and V rows outside each sequence's range replaced by finite values up to 1e4 in magnitude."""
    B, S, H, D, *_, ranges = case
    x = qkv.clone().view(B, S, 3, H, D)
    g = torch.Generator().manual_seed(gen_seed)
    for b, (lo, hi) in enumerate(ranges):
        out = torch.ones(S, dtype=torch.bool)
        out[lo:hi] = False
        n = int(out.sum())
        if n:
            x[b, out, 1:] = ((torch.rand(n, 2, H, D, generator=g) * 2 - 1) * 1e4).to(torch.bfloat16)
    return x.view(B * S, 3 * H * D)


@pytest.mark.parametrize("i", [0, len(CASES) - 1], ids=[IDS[0], IDS[-1]])
def test_result_is_independent_of_masked_keys(i):
    case = CASES[i]
    B, S, H, D, *_, ranges = case
    qkv, dctx, _, kr, *_ = _case(i)
    a = _run(_refill_outside(qkv, case, 1), dctx, case, kr)
    b = _run(_refill_outside(qkv, case, 2), dctx, case, kr)
    assert torch.equal(a[0], b[0]), "ctx"
    assert torch.equal(a[1], b[1]), "lse"
    ga, gb = (t[2].view(B, S, 3, H, D).cpu() for t in (a, b))
    assert torch.equal(ga[:, :, 0], gb[:, :, 0]), "dq"
    for s, (lo, hi) in enumerate(ranges):
        assert torch.equal(ga[s, lo:hi, 1:], gb[s, lo:hi, 1:]), f"dk/dv inside the range, sequence {s}"
        for t in (ga, gb):
            assert (t[s, :lo, 1:] == 0).all() and (t[s, hi:, 1:] == 0).all(), f"dk/dv outside, sequence {s}"
    # and the masked rows did not leak into the result: still the reference of the original input
    _check_against(case, a, _case(i)[4:])


@pytest.mark.parametrize("i", [0, 1, 2, 4], ids=[IDS[0], IDS[1], IDS[2], IDS[4]])
def test_bias_partials_with_range_are_the_column_sums(i):
    """Every bias_part row is written (skipped dK/dV blocks write zeros): the finalized qkv bias
    gradient equals the column sums of the returned dqkv."""
    case = CASES[i]
    H, D = case[2], case[3]
    qkv, dctx, _, kr, *_ = _case(i)
    db = torch.full((3 * H * D,), 0.25, device="cuda", dtype=torch.float32)
    # attn_bwd takes its partials buffer from torch.empty: leave NaNs in a freed block of that size,
    # so a partial row that a skipped block failed to write would most likely show up in the sum
    B, S = case[0], case[1]
    junk = torch.full((B * 4 * ((S + 127) // 128), 3 * H * D), float("nan"), device="cuda", dtype=torch.float32)
    del junk
    _, _, dq_b = _run(qkv, dctx, case, kr, dbias=(db, True))
    _, _, dq_g = _run(qkv, dctx, case, kr)
    assert torch.equal(dq_b, dq_g)
    ref_db = dq_g.float().sum(0)
    assert ((db - 0.25) - ref_db).abs().max().item() <= 1e-3 * (ref_db.abs().max().item() + 1.0)


@pytest.mark.parametrize("i", [1, 2], ids=[IDS[1], IDS[2]])
def test_full_range_agrees_with_no_range(i):
    case = CASES[i]
    B, S = case[0], case[1]
    qkv, dctx, *_ = _case(i)
    full = torch.tensor([[0, S]] * B, dtype=torch.int32)
    _check_against(case, _run(qkv, dctx, case, full), tuple(t.cpu() for t in _run(qkv, dctx, case, None)))


# ------------------------------------------------------------------ models
def _pair(name):
    # (the causal preset keeps GPT-2's pad id, which lies outside the tiny vocabulary)
    cfg = C.get_config(name).with_(pad_token_id=0)
    C.PRESETS["_kr"] = cfg
    ref = build_model("_kr", impl="reference", seed=3)
    fus = build_model("_kr", impl="fused", seed=3, device="cuda")
    fus.load_state_dict(ref.state_dict())
    fus.to(torch.bfloat16)
    return cfg, ref, fus


@pytest.mark.parametrize("name", ["tiny", "causal-tiny"])
def test_fused_model_with_attention_mask_matches_reference(name):
    """bf16 fused path vs the fp32 CPU reference path on a right-padded batch with attention_mask:
    loss and parameter gradients, with test_model_gpu.py's fused-vs-reference bf16 tolerances."""
    cfg, ref, fus = _pair(name)
    ds = SyntheticLMDataset(cfg, 4, seq_len=128, seed=5, pad_fraction=0.75, return_attention_mask=True)
    ids, lab, am = ds.input_ids, ds.labels, ds.attention_mask
    assert 0 < int((am.sum(1) < 128).sum())                    # some rows are padded
    l1 = ref(ids, labels=lab, attention_mask=am).loss
    l1.backward()
    l2 = fus(ids.cuda(), labels=lab.cuda(), attention_mask=am.cuda()).loss
    l2.backward()
    l0 = ref(ids, labels=lab).loss.item()
    print(f"loss reference {l1.item():.5f} fused {l2.item():.5f} (no mask: {l0:.5f})")
    assert abs(l1.item() - l2.item()) <= 3e-2 * abs(l1.item())
    for (n, p1), (_, p2) in zip(ref.named_parameters(), fus.named_parameters()):
        g1, g2 = p1.grad.float(), p2.grad.float().cpu()
        err = (g1 - g2).norm().item() / (g1.norm().item() + 1e-12)
        assert err < 0.15, f"{n}: rel err {err}"


def test_captured_step_with_attention_mask_replays_to_the_eager_loss():
    """The mask is a third static input of the captured step (key_range_from_mask runs inside the
    graph, no host sync): replays equal the same steps run eagerly."""
    from distributed_training_and_deepspeed_amd.optim import hf_adamw
    from distributed_training_and_deepspeed_amd.parallel import DistributedDataParallel
    from distributed_training_and_deepspeed_amd.utils.graphs import CapturedStep, mlm_capacity

    def setup():
        model = build_model("tiny", dtype=torch.bfloat16, device="cuda", seed=3)
        model.rt.mlm_capacity = mlm_capacity(4 * 128)
        model.rt.mlm_overflow = torch.zeros((), dtype=torch.bool, device="cuda")
        ddp = DistributedDataParallel(model)
        opt = hf_adamw(ddp.parameters(), lr=1e-3)

        def step(input_ids, labels, attention_mask):
            out = ddp(input_ids, labels=labels, attention_mask=attention_mask)
            out.loss.backward()
            opt.step()
            model.rt.rng.advance()
            return out.loss.detach()
        return model, step

    n = 4
    ds = SyntheticLMDataset(build_model("tiny").cfg, 4 * n, seq_len=128, seed=5, pad_fraction=0.75,
                            return_attention_mask=True)
    ids, lab, am = (t.view(n, 4, 128).cuda() for t in (ds.input_ids, ds.labels, ds.attention_mask))
    ma, sa = setup()
    mb, sb = setup()
    cap = CapturedStep(sb, {"input_ids": ids[0], "labels": lab[0], "attention_mask": am[0]}, warmup=3, runtime=mb.rt)
    la = [sa(ids[0], lab[0], am[0]) for _ in range(3)]
    la += [sa(ids[i], lab[i], am[i]) for i in range(1, n)]
    lb = [cap(input_ids=ids[i], labels=lab[i], attention_mask=am[i]).clone() for i in range(1, n)]
    torch.cuda.synchronize()
    cap.check()
    assert torch.equal(torch.stack(la[3:]), torch.stack(lb))
    for (name, p), q in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(p, q), name
