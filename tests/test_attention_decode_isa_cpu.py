"""Resource checks of the 16 ``decode_split_kernel<D, GP, FP8>`` instantiations (ops/csrc/attention_decode.hip,
compiled for gfx950; CPU-only).  The two cache formats share one kernel text, so an edit made for one of them
can cost the other registers or a wave without any test of results noticing; the figures below are those of the
two kernels the template was folded from (profiles/attn_decode_resources.md):

  * no scratch;
  * the LDS of the final reduction, exactly (it is a function of D, GP and the format alone);
  * VGPRs + AGPRs and waves per SIMD no worse.

Only the resource footers are read; scripts/diag/compare_kernel_asm.py compares the instructions of two builds."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "diag"))
SRC = os.path.join(ROOT, "distributed_training_and_deepspeed_amd", "ops", "csrc", "attention_decode.hip")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None,
                                reason="hipcc not available")

# (D, GP, FP8): (VGPRs + AGPRs, waves per SIMD, LDS bytes)
EXPECTED = {
    (64, 1, False): (64, 8, 8448), (64, 2, False): (84, 5, 16896),
    (64, 4, False): (116, 4, 33792), (64, 8, False): (246, 2, 33792),
    (128, 1, False): (90, 5, 8320), (128, 2, False): (130, 3, 16640),
    (128, 4, False): (152, 3, 33280), (128, 8, False): (236, 2, 33280),
    (64, 1, True): (81, 5, 16896), (64, 2, True): (126, 4, 33792),
    (64, 4, True): (178, 2, 33792), (64, 8, True): (256 + 3, 1, 33792),
    (128, 1, True): (79, 6, 16640), (128, 2, True): (141, 3, 33280),
    (128, 4, True): (230, 2, 33280), (128, 8, True): (256 + 34, 1, 33280),
}


@pytest.fixture(scope="module")
def figures():
    """{(D, GP, FP8): resource figures} of every decode_split_kernel in one compile of the file."""
    from audit_fused_bwd_asm import build_asm
    from compare_kernel_asm import kernels
    found = kernels(build_asm(SRC, ()))
    out = {}
    for (D, GP, fp8) in EXPECTED:
        tag = f"decode_split_kernelILi{D}ELi{GP}ELb{int(fp8)}EE"
        hits = [fig for name, (_, fig) in found.items() if tag in name]
        assert len(hits) == 1, f"{tag}: {len(hits)} kernels in the listing"
        out[(D, GP, fp8)] = hits[0]
    assert len([n for n in found if "decode_split" in n]) == len(EXPECTED), "a split kernel the table does not know"
    return out


@pytest.mark.parametrize("key", list(EXPECTED), ids=lambda k: f"D{k[0]}-GP{k[1]}-{'fp8' if k[2] else 'bf16'}")
def test_split_kernel_resources(figures, key):
    regs, waves, lds = EXPECTED[key]
    fig = figures[key]
    assert fig["ScratchSize"] == 0
    assert fig["LDSByteSize"] == lds
    assert fig["NumVgprs"] + fig["NumAgprs"] <= regs, fig
    assert fig["Occupancy"] >= waves, fig
