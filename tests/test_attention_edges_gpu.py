"""Flash-attention HIP kernels at the edges of their prologues and epilogues: the branch-free
fragment and row-statistic loads (rows past S read 0 through a bounded buffer resource) and the
16-byte epilogue stores (v_permlane32_swap pairs), at the smallest shapes where they can go wrong:

  S = 33          one lane of the second wave is valid: loads and stores at a row edge
  S = 100, 130    a partly-valid second 128-row block
  S = 200         the second dK/dV query tile has 72 valid statistic rows
  S = 512         four 128-row blocks (the benchmark's shape)
  S = 160, D=128  the head_dim 128 instantiations

Each case is checked against the fp32 math reference with the thresholds of
tests/test_attention_gpu.py, run twice (bit-equal), and run once more through the C entry points
on sentinel-filled output buffers that are wider (one spare head slot per row) and longer (one
spare 128-row block) than the result: everything outside the result must keep the sentinel, and
the result must equal the plain call's bit for bit -- a wrong half-wave offset of a widened
store lands in a neighbouring head or slot."""
import functools
import math

import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops.rng import RngState

pytestmark = pytest.mark.gpu

SEED, SID = 11, 9
SENTINEL = -1234.0        # exactly representable in bf16; no kernel output of these cases equals it
PAD_ROWS = 128            # spare rows behind the last sequence: one whole workgroup tile


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


CASES = [
    # B, S, H, D, causal, alibi, p, ranges
    (2, 33, 3, 64, False, False, 0.1, None),
    (2, 33, 2, 64, True, False, 0.0, None),
    (2, 100, 3, 64, False, False, 0.1, None),
    (1, 100, 2, 64, True, False, 0.0, None),
    (2, 130, 2, 64, False, False, 0.0, None),
    (1, 130, 3, 64, True, True, 0.1, None),
    (2, 200, 3, 64, False, False, 0.1, None),
    (1, 200, 2, 64, True, False, 0.0, None),
    (1, 512, 3, 64, False, False, 0.1, None),
    (1, 512, 2, 64, True, False, 0.0, None),
    (2, 160, 3, 128, False, False, 0.1, None),
    (1, 160, 2, 128, True, False, 0.0, None),
    # left-padded sequence (rows q < lo have no key under the causal mask) and an empty range:
    # rows with lse = -inf go through the row-statistic transform of the dK/dV kernel
    (2, 200, 3, 64, True, False, 0.1, [(37, 200), (50, 50)]),
]
IDS = [f"S{c[1]}-B{c[0]}H{c[2]}D{c[3]}{'-causal' if c[4] else ''}{'-alibi' if c[5] else ''}-p{c[6]}"
       f"{'-range' if c[7] else ''}" for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the CPU math reference of case i -- computed once, shared, never modified."""
    B, S, H, D, causal, alibi, p, ranges = CASES[i]
    torch.manual_seed(100 + i)
    qkv = torch.randn(B * S, 3 * H * D).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D).to(torch.bfloat16)
    slopes = A.alibi_slopes(H) if alibi else None
    kr = torch.tensor(ranges, dtype=torch.int32) if ranges else None
    rc = RngState(SEED, device="cpu")
    ctx_r, lse_r = A.attn_fwd_ref(qkv, B, S, H, D, causal, slopes, p, rc, SID, key_range=kr)
    dq_r = A.attn_bwd_ref(dctx, qkv, ctx_r, lse_r, B, S, H, D, causal, slopes, p, rc, SID, key_range=kr)
    assert torch.isfinite(ctx_r.float()).all() and torch.isfinite(dq_r.float()).all() and not torch.isnan(lse_r).any()
    return qkv, dctx, slopes, kr, ctx_r, lse_r, dq_r


def _run(i, dbias=None):
    B, S, H, D, causal, alibi, p, _ = CASES[i]
    qkv, dctx, slopes, kr, *_ = _case(i)
    rg = RngState(SEED, device="cuda")
    q = qkv.cuda()
    assert A.kernel_supported(q, D)
    krg = kr.cuda() if kr is not None else None
    ctx, lse, mk = A.attn_fwd(q, B, S, H, D, causal, slopes, p, rg, SID, key_range=krg)
    dqkv = A.attn_bwd(dctx.cuda(), q, ctx, lse, B, S, H, D, causal, slopes, p, rg, SID, mk, dbias=dbias,
                      key_range=krg)
    torch.cuda.synchronize()
    return ctx, lse, dqkv, mk


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_edge_shapes_match_reference_and_repeat(i):
    B, S, H, D, causal, alibi, p, ranges = CASES[i]
    *_, ctx_r, lse_r, dq_r = _case(i)
    ctx_g, lse_g, dq_g, _ = _run(i)
    assert torch.isfinite(ctx_g.float()).all() and torch.isfinite(dq_g.float()).all()
    lse_c, lse_r = lse_g.float().cpu(), lse_r.float().cpu()
    assert not torch.isnan(lse_c).any()
    dead = lse_r == float("-inf")
    assert dead.any().item() == bool(ranges)
    assert torch.equal(lse_c == float("-inf"), dead)
    e_ctx = rel(ctx_g, ctx_r)
    e_lse = (lse_c[~dead] - lse_r[~dead]).abs().max().item()
    g, r = dq_g.view(B, S, 3, H, D).cpu(), dq_r.view(B, S, 3, H, D).cpu()
    errs = [rel(g[:, :, k], r[:, :, k]) for k in range(3)]
    print(f"ctx rel {e_ctx:.3e}  lse abs {e_lse:.3e}  dq/dk/dv rel {errs}")
    assert e_ctx < 1e-2, e_ctx
    assert e_lse < 2e-2, e_lse
    for name, e in zip("qkv", errs):
        assert e < 2e-2, f"d{name} rel err {e}"
    if ranges:   # rows without a key: ctx and dq exactly 0; keys outside a range: dk, dv exactly 0
        dead_rows = dead.transpose(1, 2)
        assert (ctx_g.view(B, S, H, D).cpu()[dead_rows] == 0).all()
        assert (g[:, :, 0][dead_rows] == 0).all()
        for b, (lo, hi) in enumerate(ranges):
            assert (g[b, :lo, 1:] == 0).all() and (g[b, hi:, 1:] == 0).all(), b
    # qkv bias gradient from the backward epilogues == column sums of dqkv (as in test_attention_gpu.py)
    db = torch.full((3 * H * D,), 0.25, device="cuda", dtype=torch.float32)
    ctx_2, lse_2, dq_b, _ = _run(i, dbias=(db, True))
    ref_db = dq_g.float().sum(0)
    assert ((db - 0.25) - ref_db).abs().max().item() <= 1e-3 * (ref_db.abs().max().item() + 1.0)
    # the second run is the first, bit for bit
    assert torch.equal(ctx_2, ctx_g) and torch.equal(lse_2, lse_g) and torch.equal(dq_b, dq_g)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_stores_stay_inside_their_rows_and_head(i):
    """The C entry points on wider and longer sentinel-filled buffers: qkv / dqkv rows of 3 H D + D
    columns and ctx rows of H D + D (a spare head slot behind each row), PAD_ROWS spare rows behind
    the last sequence.  The spare columns and rows keep the sentinel; the rest equals the plain call."""
    B, S, H, D, causal, alibi, p, ranges = CASES[i]
    qkv, dctx, slopes, kr, *_ = _case(i)
    ctx_p, lse_p, dq_p, mk = _run(i)
    dev = torch.device("cuda")
    HD, es = H * D, 2
    ld, ldo, rows = 3 * HD + D, HD + D, B * S + PAD_ROWS
    # precondition of the 16-byte stores: every row of every (slice, head) starts 16-byte aligned
    assert (ld * es) % 16 == 0 and (ldo * es) % 16 == 0 and (HD * es) % 16 == 0 and (D * es) % 16 == 0
    assert (3 * HD * es) % 16 == 0   # ... and in the packed layout of the plain call too
    qkv_w = torch.zeros(rows, ld, dtype=torch.bfloat16, device=dev)
    qkv_w[:B * S, :3 * HD] = qkv.cuda()
    ctx_w = torch.full((rows, ldo), SENTINEL, dtype=torch.bfloat16, device=dev)
    dqkv_w = torch.full((rows, ld), SENTINEL, dtype=torch.bfloat16, device=dev)
    lse_w = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    delta = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    sl = slopes.to(device=dev, dtype=torch.float32).contiguous() if slopes is not None else None
    krg = kr.to(device=dev, dtype=torch.int32).contiguous() if kr is not None else None
    for t in (qkv_w, ctx_w, dqkv_w):
        assert t.data_ptr() % 16 == 0
    qb, gb, scale = qkv_w.data_ptr(), dqkv_w.data_ptr(), 1.0 / math.sqrt(D)
    # forward (keep bits of the plain call: generated already, so no rng state)
    fargs = (qb, qb + HD * es, qb + 2 * HD * es, ctx_w.data_ptr(), lse_w.data_ptr(), _lib.ptr(sl), _lib.ptr(mk),
             B, S, H, D, ld, ldo, int(causal), scale, float(p), None, SID)
    if krg is None:
        _lib.call("dtd_attn_fwd", *fargs, _lib.stream())
    else:
        _lib.call("dtd_attn_fwd_range", *fargs, krg.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(ctx_w[:B * S, :HD], ctx_p), "ctx differs from the plain call"
    assert torch.equal(lse_w, lse_p)
    assert (ctx_w[:B * S, HD:] == SENTINEL).all(), "a ctx store left its head"
    assert (ctx_w[B * S:] == SENTINEL).all(), "a ctx row past S was written"
    # backward: ctx / dctx in the same wide row layout (they share the row stride ldo)
    dctx_w = torch.zeros(rows, ldo, dtype=torch.bfloat16, device=dev)
    dctx_w[:B * S, :HD] = dctx.cuda()
    ctx_in = torch.zeros(rows, ldo, dtype=torch.bfloat16, device=dev)
    ctx_in[:B * S, :HD] = ctx_p
    bargs = (qb, qb + HD * es, qb + 2 * HD * es, ctx_in.data_ptr(), dctx_w.data_ptr(), lse_p.data_ptr(),
             delta.data_ptr(), _lib.ptr(mk), gb, gb + HD * es, gb + 2 * HD * es, _lib.ptr(sl),
             B, S, H, D, ld, ldo, int(causal), scale, float(p), None)
    if krg is None:
        _lib.call("dtd_attn_bwd", *bargs, _lib.stream())
    else:
        _lib.call("dtd_attn_bwd_range", *bargs, krg.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(dqkv_w[:B * S, :3 * HD], dq_p), "dqkv differs from the plain call"
    assert (dqkv_w[:B * S, 3 * HD:] == SENTINEL).all(), "a dq / dk / dv store left its slice"
    assert (dqkv_w[B * S:] == SENTINEL).all(), "a dq / dk / dv row past S was written"
