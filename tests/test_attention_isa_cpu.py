"""ISA checks of the flash-attention kernels the benchmark launches (ops/csrc/attention.hip,
compiled for gfx950; CPU-only): resources, and the placement of memory waits and the width of the
epilogue stores outside the tile loops -- a compiler update that quietly puts a drained prefetch, a
serialized prologue or 8-byte store pairs back shows up here, not as a slower step weeks later.

  * no scratch; 3 / 3 / 2 waves per SIMD (forward / dQ / dK,dV);
  * dK/dV: between the eight Q / dO tile loads at the head of a query tile and the tile's first
    MFMA nothing waits for them (vmcnt retires in order: a wait below 8 drains the prefetch);
  * dQ: the K/V tile loads are issued before the kernel's first vmcnt wait, and at most one
    vmcnt(0) stands before the first barrier (one memory round trip in the prologue);
  * the dQ / dK / dV epilogues store 16 bytes per lane: 4 / 8 dwordx4, no dwordx2.  (The forward's
    ctx store keeps its 8-byte form: widened, the kernel did not clear the noise margin of the
    interleaved kernel benchmark -- docs/PERFORMANCE.md, Attention, "Prologues and epilogues".)"""
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

# the instantiations of the default launch at D = 64 with dropout (template arguments, mangled)
KERNELS = {
    "fwd": "attn_fwd_kernelILi64ELi3ELi64ELi1ELb0ELb0EE",
    "dq": "attn_bwd_dq_kernelILi64ELi3ELi64ELi1ELb0ELb0EE",
    "dkdv": "attn_bwd_dkdv_kernelILi64ELi2ELi128ELb1ELb0ELb0ELb0EE",
}
OCCUPANCY = {"fwd": 3, "dq": 3, "dkdv": 2}
STORES_X4 = {"dq": 4, "dkdv": 8}


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
    ins = [ln for ln in lines if ln and not ln.startswith((";", ".")) and not ln.endswith(":")]
    nxt = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, end + 1)   # the resource comments follow the end label
    return ins, text[end:nxt.start() if nxt else len(text)]


def _vmcnt(ins):
    m = re.search(r"vmcnt\((\d+)\)", ins) if ins.startswith("s_waitcnt") else None
    return int(m.group(1)) if m else None


def _first(ins, pred, start=0):
    return next(i for i in range(start, len(ins)) if pred(ins[i]))


@pytest.mark.parametrize("key", list(KERNELS))
def test_resources(listing, key):
    _, foot = _kernel(listing, key)
    assert int(re.search(r"; ScratchSize: (\d+)", foot).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", foot).group(1)) == OCCUPANCY[key]


@pytest.mark.parametrize("key", list(STORES_X4))
def test_epilogue_stores_are_16_bytes(listing, key):
    ins, _ = _kernel(listing, key)
    ops = [i.split()[0] for i in ins]
    assert not [o for o in ops if o.endswith("_store_dwordx2")]
    assert len([o for o in ops if o.endswith("_store_dwordx4")]) == STORES_X4[key]
    assert "v_permlane32_swap_b32_e32" in ops


def test_dkdv_tile_head_does_not_drain_its_prefetch(listing):
    ins, _ = _kernel(listing, "dkdv")
    mfma = _first(ins, lambda s: s.startswith("v_mfma"))
    loads = [i for i in range(mfma) if ins[i].startswith("buffer_load_dwordx4")]
    # prologue: K / V fragments (8) and the first Q / dO tile (8); then the loop head's eight
    assert len(loads) == 24, len(loads)
    head = loads[-8:]
    between = ins[head[0]:mfma]
    assert not [s for s in between if s.startswith("s_barrier")], "not the loop-head loads"
    assert [s for s in ins[loads[-9]:head[0]] if s.startswith("s_barrier")], "not the loop-head loads"
    waits = [_vmcnt(s) for s in between if _vmcnt(s) is not None]
    assert all(n >= 8 for n in waits), waits
    # the row statistics ride behind the tile loads, nothing consumes them here
    assert len([s for s in between if s.startswith("buffer_load_dword ")]) >= 2


def test_dq_prologue_is_one_round_trip(listing):
    ins, _ = _kernel(listing, "dq")
    first_wait = _first(ins, lambda s: _vmcnt(s) is not None)
    first_load = _first(ins, lambda s: s.startswith("buffer_load_dwordx4"))
    assert first_load < first_wait
    # K/V tiles t0 and t0 + 1 (8 loads) and the Q / dO / O fragments (12) are all in flight by then
    assert len([s for s in ins[:first_wait] if s.startswith("buffer_load_dwordx4")]) == 20
    barrier = _first(ins, lambda s: s.startswith("s_barrier"))
    assert first_wait < barrier
    assert len([s for s in ins[:barrier] if _vmcnt(s) == 0]) <= 1
    assert not [s for s in ins[:barrier] if s.startswith("global_load")]
