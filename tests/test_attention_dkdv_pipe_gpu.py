"""attn_bwd_dkdv_pipe_kernel (ops/csrc/attention_bwd_dkdv_pipe_body.h): the dK/dV kernel of the unmasked
D = 64 call with its Q / dO tiles delivered by LDS-DMA and the S / dP MFMAs issued one query sub-block
ahead.  It changes how operands arrive and the order instructions issue in, not the arithmetic or its
order, so its gradients must equal attn_bwd_dkdv_kernel's bit for bit (DTD_ATTN_DKDV=old / dma / pipe
selects the kernel at launch), on every tile count the double buffer distinguishes:

  S = 128  one query tile: prologue only, no DMA inside the loop
  S = 256  one seam, the DMA lands in buffer 1
  S = 384  three tiles: both buffer parities, an odd count
  S = 512  the benchmark's four tiles

each with and without dropout and with and without the bias-gradient epilogue.  A wrong DMA address or
a wrong wait shows as wrong numbers (or as two runs that differ), never as a fault: the DMA writes LDS.
Shapes outside the kernel's scope (S % 128 != 0, causal) must still be right: they keep the old kernel."""
import functools

import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops.rng import RngState

pytestmark = pytest.mark.gpu

D = 64
SHAPES = [(128, 2, 3), (256, 2, 3), (384, 1, 3), (512, 1, 2)]   # S, B, H
ARMS = ("old", "dma", "pipe")


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(S, B, H, p, causal=False):
    """Inputs, the forward's outputs and the fp32 reference gradient of one shape, computed once."""
    torch.manual_seed(S + int(p * 100))
    qkv = torch.randn(B * S, 3 * H * D).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D).to(torch.bfloat16)
    rg, rc = RngState(7, device="cuda"), RngState(7, device="cpu")
    ctx, lse, mk = A.attn_fwd(qkv.cuda(), B, S, H, D, causal, None, p, rg, 5)
    ctx_r, lse_r = A.attn_fwd_ref(qkv, B, S, H, D, causal, None, p, rc, 5)
    ref = A.attn_bwd_ref(dctx, qkv, ctx_r, lse_r, B, S, H, D, causal, None, p, rc, 5).view(B, S, 3, H, D)
    return {"qkv": qkv.cuda(), "dctx": dctx.cuda(), "ctx": ctx, "lse": lse, "mk": mk, "rg": rg, "ref": ref}


def _bwd(c, S, B, H, p, arm, monkeypatch, dbias, causal=False):
    monkeypatch.setenv("DTD_ATTN_DKDV", arm)
    db = torch.full((3 * H * D,), 0.25, device="cuda", dtype=torch.float32) if dbias else None
    g = A.attn_bwd(c["dctx"], c["qkv"], c["ctx"], c["lse"], B, S, H, D, causal, None, p, c["rg"], 5, c["mk"],
                   dbias=(db, True) if dbias else None)
    torch.cuda.synchronize()
    return g, db


@pytest.mark.parametrize("dbias", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.0])
@pytest.mark.parametrize("S,B,H", SHAPES)
def test_bit_equal_to_the_register_staged_kernel(S, B, H, p, dbias, monkeypatch):
    c = _case(S, B, H, p)
    out = {arm: _bwd(c, S, B, H, p, arm, monkeypatch, dbias) for arm in ARMS}
    again = _bwd(c, S, B, H, p, "pipe", monkeypatch, dbias)
    for arm in ("dma", "pipe"):
        assert torch.equal(out[arm][0], out["old"][0]), f"{arm}: dqkv differs from the old kernel's"
        if dbias:
            assert torch.equal(out[arm][1], out["old"][1]), f"{arm}: bias gradient differs from the old kernel's"
    assert torch.equal(again[0], out["pipe"][0]), "two runs differ"
    if dbias:
        assert torch.equal(again[1], out["pipe"][1]), "two runs differ (bias gradient)"


@pytest.mark.parametrize("arm", ["dma", "pipe"])
@pytest.mark.parametrize("p", [0.1, 0.0])
@pytest.mark.parametrize("S,B,H", SHAPES)
def test_matches_reference(S, B, H, p, arm, monkeypatch):
    """The thresholds of tests/test_attention_gpu.py."""
    c = _case(S, B, H, p)
    g, db = _bwd(c, S, B, H, p, arm, monkeypatch, True)
    gv = g.view(B, S, 3, H, D).cpu()
    for i, name in enumerate("qkv"):
        e = rel(gv[:, :, i], c["ref"][:, :, i])
        assert e < 2e-2, f"d{name} rel err {e}"
    ref_db = g.float().sum(0)
    assert ((db - 0.25) - ref_db).abs().max().item() <= 1e-3 * (ref_db.abs().max().item() + 1.0)


@pytest.mark.parametrize("S,B,H,causal", [(200, 2, 3, False), (256, 2, 3, True)])
def test_uncovered_shapes_keep_the_old_kernel(S, B, H, causal, monkeypatch):
    """The new kernel has no mask: had one of these taken it, the result would be wrong."""
    p = 0.1
    c = _case(S, B, H, p, causal)
    out = {arm: _bwd(c, S, B, H, p, arm, monkeypatch, True, causal) for arm in ARMS}
    for arm in ("dma", "pipe"):
        assert torch.equal(out[arm][0], out["old"][0]) and torch.equal(out[arm][1], out["old"][1])
    gv = out["pipe"][0].view(B, S, 3, H, D).cpu()
    for i, name in enumerate("qkv"):
        e = rel(gv[:, :, i], c["ref"][:, :, i])
        assert e < 2e-2, f"d{name} rel err {e}"
