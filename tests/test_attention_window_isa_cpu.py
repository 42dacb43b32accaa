"""Resources of the sliding-window flash-attention kernels (ops/csrc/attention.hip compiled for gfx950;
CPU-only, the listing is built as in tests/test_attention_isa_cpu.py): each of the 18 windowed
instantiations -- plain, key range, document spans x head_dim 64, 128 x forward, dQ, dK/dV -- has no
scratch, and at D = 64 runs at the waves per SIMD of the grouped-query instantiation it derives from:
3 (forward), 3 (dQ), 2 (dK/dV)."""
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

MODES = {"plain": 0, "key_range": 1, "doc_range": 2}
# template arguments (mangled) in front of the MODE argument, per head_dim
KERNELS = {
    "fwd": {64: "attn_fwd_win_kernelILi64ELi3ELi64ELi1E", 128: "attn_fwd_win_kernelILi128ELi1ELi64ELi2E"},
    "dq": {64: "attn_bwd_dq_win_kernelILi64ELi3ELi64ELi1E", 128: "attn_bwd_dq_win_kernelILi128ELi1ELi64ELi2E"},
    "dkdv": {64: "attn_bwd_dkdv_win_kernelILi64ELi2ELi128E", 128: "attn_bwd_dkdv_win_kernelILi128ELi1ELi64E"},
}
OCCUPANCY_D64 = {"fwd": 3, "dq": 3, "dkdv": 2}


@pytest.fixture(scope="module")
def listing():
    from audit_fused_bwd_asm import build_asm
    return build_asm(SRC, ())


def _footer(text, name):
    """The resource comments behind the kernel whose symbol contains ``name``."""
    m = re.search(r"^(_Z\S*" + re.escape(name) + r"\S*):", text, re.M)
    assert m, f"{name} not in the listing"
    end = text.index(".Lfunc_end", m.end())
    nxt = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, end + 1)
    return text[end:nxt.start() if nxt else len(text)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("key", list(KERNELS))
def test_resources(listing, key, D, mode):
    foot = _footer(listing, f"{KERNELS[key][D]}Li{MODES[mode]}EE")
    assert int(re.search(r"; ScratchSize: (\d+)", foot).group(1)) == 0
    if D == 64:
        assert int(re.search(r"; Occupancy: (\d+)", foot).group(1)) == OCCUPANCY_D64[key]
