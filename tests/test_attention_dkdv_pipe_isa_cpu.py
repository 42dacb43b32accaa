"""ISA checks of attn_bwd_dkdv_pipe_kernel (ops/csrc/attention_bwd_dkdv_pipe_body.h, compiled for gfx950;
CPU-only), in the style of test_attention_isa_cpu.py.  What the kernel is for is visible in its listing,
and a compiler update or an edit that quietly undoes it shows up here:

  * no scratch, 2 waves per SIMD (the second score accumulator pair fits the 256 registers);
  * the Q / dO tiles arrive by LDS-DMA: eight `buffer_load_dwordx4 ... lds` in the prologue and eight per
    query tile in the loop, and no 16-byte LDS write anywhere;
  * the DMA is hidden from the compiler, so the kernel waits for it itself: an `s_waitcnt vmcnt(0)`
    stands between the loop's last MFMA and its barrier -- and NO vmcnt wait stands between the loop's
    DMA pieces and that last MFMA (vmcnt retires in order: a counted wait for an older compiler-visible
    load there would drain the prefetch at the head of every tile);
  * PIPE: per query tile the MFMAs and exponentials come as S/dP(0) | S/dP(1) exp(0) dV/dK(0) |
    S/dP(2) exp(1) dV/dK(1) | S/dP(3) exp(2) dV/dK(2) | exp(3) dV/dK(3): eight score MFMAs stand
    between a steady-state sub-block's start and its first v_exp_f32;
  * the epilogue stores 16 bytes per lane: 8 dwordx4, no dwordx2."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "diag"))
SRC = os.path.join(ROOT, "distributed_training_and_deepspeed_amd", "ops", "csrc", "attention.hip")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None,
                                reason="hipcc not available")

# attn_bwd_dkdv_pipe_kernel<DROP, PIPE> (template arguments, mangled)
KERNELS = {
    "drop_pipe": "attn_bwd_dkdv_pipe_kernelILb1ELb1EE",
    "drop_dma": "attn_bwd_dkdv_pipe_kernelILb1ELb0EE",
    "pipe": "attn_bwd_dkdv_pipe_kernelILb0ELb1EE",
    "dma": "attn_bwd_dkdv_pipe_kernelILb0ELb0EE",
}


@pytest.fixture(scope="module")
def listing():
    from audit_fused_bwd_asm import build_asm
    return build_asm(SRC, ())


def _kernel(text, key):
    """(instructions of the kernel in listing order, its resource footer)"""
    m = re.search(r"^(_Z\S*" + KERNELS[key] + r"\S*):", text, re.M)
    assert m, f"{KERNELS[key]} not in the listing"
    end = text.index(".Lfunc_end", m.end())
    lines = [ln.strip() for ln in text[m.end():end].split("\n")[1:]]
    ins = [ln for ln in lines if ln and not ln.startswith((";", ".")) or ln.startswith(".LBB")]   # (labels kept)
    nxt = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, end + 1)   # the resource comments follow the end label
    return ins, text[end:nxt.start() if nxt else len(text)]


def _vmcnt(ins):
    m = re.search(r"vmcnt\((\d+)\)", ins) if ins.startswith("s_waitcnt") else None
    return int(m.group(1)) if m else None


def _is_dma(ins):
    return ins.startswith("buffer_load_dwordx4") and ins.endswith(" lds")


def _loop(ins):
    """(prologue, rest): split at the first barrier.  The listing need not keep the loop's blocks in
    program order (its latch, with the second barrier, may stand ahead of its body), so the loop's
    pieces are found by what they are: the DMA pieces after the prologue's, the MFMAs, the second barrier."""
    bars = [i for i, s in enumerate(ins) if s.startswith("s_barrier")]
    assert len(bars) == 2, bars
    return ins[:bars[0]], ins[bars[0] + 1:]


def _block_before(ins, i):
    """The straight-line code that ends at instruction i: back to the nearest label or branch."""
    j = i
    while j > 0 and not ins[j - 1].startswith((".LBB", "s_cbranch", "s_branch")):
        j -= 1
    return ins[j:i]


@pytest.mark.parametrize("key", list(KERNELS))
def test_resources(listing, key):
    ins, foot = _kernel(listing, key)
    assert int(re.search(r"; ScratchSize: (\d+)", foot).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", foot).group(1)) == 2
    assert not [s for s in ins if s.startswith("v_accvgpr")]


@pytest.mark.parametrize("key", list(KERNELS))
def test_tiles_arrive_by_lds_dma(listing, key):
    ins, _ = _kernel(listing, key)
    pro, loop = _loop(ins)
    assert len([s for s in pro if _is_dma(s)]) == 8
    assert len([s for s in loop if _is_dma(s)]) == 8
    assert len([s for s in ins if _is_dma(s)]) == 16
    assert not [s for s in ins if s.startswith(("ds_write_b128", "ds_write2_b64", "ds_write2st64_b64"))]
    # the K / V fragments (8) are the only 16-byte loads into registers
    assert len([s for s in ins if s.startswith("buffer_load_dwordx4") and not _is_dma(s)]) == 8


@pytest.mark.parametrize("key", list(KERNELS))
def test_loop_waits_for_its_dma_at_the_barrier_and_nowhere_else(listing, key):
    ins, _ = _kernel(listing, key)
    pro, loop = _loop(ins)
    last_dma = max(i for i, s in enumerate(loop) if _is_dma(s))
    last_mfma = max(i for i, s in enumerate(loop) if s.startswith("v_mfma"))
    assert last_dma < last_mfma
    mid = [s for s in loop[last_dma:last_mfma] if _vmcnt(s) is not None]
    assert not mid, f"vmcnt waits between the DMA pieces and the tile's last MFMA: {mid}"
    bar = next(i for i, s in enumerate(loop) if s.startswith("s_barrier"))
    assert [s for s in _block_before(loop, bar) if _vmcnt(s) == 0], "no vmcnt(0) before the loop's barrier"
    # the prologue's DMA is waited for before the first barrier too
    first_dma = min(i for i, s in enumerate(pro) if _is_dma(s))
    assert [s for s in pro[first_dma:] if _vmcnt(s) == 0]


@pytest.mark.parametrize("key", ["drop_pipe", "pipe"])
def test_score_mfmas_run_one_sub_block_ahead(listing, key):
    ins, _ = _kernel(listing, key)
    _, loop = _loop(ins)
    ev = [(s.split()[0][:6], s) for s in loop if s.startswith(("v_mfma", "v_exp_f32"))]
    kinds = [k for k, _ in ev]
    assert kinds.count("v_mfma") == 64 and kinds.count("v_exp_") == 64, (kinds.count("v_mfma"), kinds.count("v_exp_"))
    dst = lambda s: s.split(None, 1)[1].split(",")[0]   # noqa: E731
    fresh = lambda s: s.endswith(", 0")                 # noqa: E731  (C = 0: the first MFMA of a score chain)
    mfmas = [s for k, s in ev if k == "v_mfma"]
    score = {dst(s) for s in mfmas if fresh(s)}          # S / dP accumulators (two pairs)
    grads = {dst(s) for s in mfmas} - score              # dV / dK accumulators (2 each)
    assert len(grads) == 4 and len([s for s in mfmas if dst(s) in grads]) == 32
    # the first exponential of sub-block qb is the 16 qb-th of the tile
    exps = [i for i, k in enumerate(kinds) if k == "v_exp_"]
    first = [exps[16 * qb] for qb in range(4)]
    # sub-block 0: its own score MFMAs and sub-block 1's stand ahead of it
    assert first[0] == 16 and kinds[:16] == ["v_mfma"] * 16
    ahead = [ev[0:8]] + [ev[first[qb] - 8:first[qb]] for qb in range(3)]
    # sub-blocks 0, 1, 2 (1 and 2 are the steady state): the eight MFMAs ahead of the sub-block's first
    # exponential are the whole S / dP chains of the NEXT sub-block -- two accumulators, each started from
    # zero, neither a gradient accumulator, and not the pair the softmax behind them works on
    for a in ahead:
        assert [k for k, _ in a] == ["v_mfma"] * 8, a
        assert len({dst(s) for _, s in a}) == 2 and {dst(s) for _, s in a} <= score, a
        assert len([s for _, s in a if fresh(s)]) == 2, a
    for a, b in zip(ahead, ahead[1:]):
        assert not {dst(s) for _, s in a} & {dst(s) for _, s in b}, (a, b)
    # the last sub-block has no scores to issue ahead
    assert all(dst(s) in grads for k, s in ev[first[3]:] if k == "v_mfma")


@pytest.mark.parametrize("key", list(KERNELS))
def test_epilogue_stores_are_16_bytes(listing, key):
    ins, _ = _kernel(listing, key)
    ops = [i.split()[0] for i in ins]
    assert not [o for o in ops if o.endswith("_store_dwordx2")]
    assert len([o for o in ops if o.endswith("_store_dwordx4")]) == 8
    assert "v_permlane32_swap_b32_e32" in ops
