"""The flash-attention HIP kernels (ops/csrc/attention.hip and its three body headers, attention_f32.hip)
against the fp64 autograd oracle of ``tests/oracles.py``, per (token, head) row, in every input regime
of ``oracles.attn_inputs`` -- the device run of the ``check_attention`` that
``tests/test_attention_oracles_cpu.py`` runs on the math reference (metric, bounds and their
derivation: that file's docstring).  The bounds came from that derivation and from CPU measurements of
the reference and the staged model, none from a kernel's result.

Covered here and nowhere else: the instantiations that only ``scripts/ab.py`` and
``scripts/bench_attn.py`` select -- forward ``<64,2,64,2>`` / ``<64,1,64,2>`` and dQ ``<64,2,64,2>`` /
``<64,1,64,2>`` (DTD_ATTN_OCC), the 128-key-tile dQ ``<64,2,128,2>`` (DTD_ATTN_TILE), dK/dV ``<64,1,128>``,
``<64,2,64>`` and ``<64,1,64>`` (DTD_ATTN_OCC, DTD_ATTN_DKDV_BM).  A variant that differs from the
default form only in how its tiles are loaded (same keys per tile / query rows per tile) must equal it
bit for bit.

Shapes (``SHAPES`` of the CPU file) are the smallest that cross the structures: S 200 (four 64-key
tiles, a partial second 128-row block, 72 valid rows in the second dK/dV tile), S 512 (the no-mask
dK/dV path), S 160 at head_dim 128, S 33 for the regimes that sit at the sequence edges.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops.rng import RngState

from . import oracles as O
from .test_attention_oracles_cpu import MODES, SEED, SID, attn_case, print_worst
from .test_attention_oracles_cpu import check_attention as _check

pytestmark = pytest.mark.gpu

GPU_TITLE = "attention HIP kernels"       # this file's own table of worst ratios
BF16, F32 = torch.bfloat16, torch.float32
FORM_ENV = ("DTD_ATTN_FWD", "DTD_ATTN_FWD_PK", "DTD_ATTN_OCC", "DTD_ATTN_TILE", "DTD_ATTN_DKDV_BM", "DTD_ATTN_RESCALE_THR",
            "DTD_ATTN_BWD")


@pytest.fixture(autouse=True)
def default_forms(monkeypatch):
    """Every test starts from the shipped forms; the launchers read their overrides on every call."""
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)


def check_attention(c, ctx, lse, dqkv, kind, form):
    return _check(c, ctx, lse, dqkv, kind, form, title=GPU_TITLE)


def run_kernels(c, monkeypatch, env=None, dtype=BF16):
    """attn_fwd, then attn_bwd on what it returned, under the form overrides ``env``."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    qkv, dctx = c.qkv.to(dtype).cuda(), c.dctx.to(dtype).cuda()
    assert A.kernel_supported(qkv, c.D) if dtype == BF16 else A.f32_kernel_supported(qkv, c.D)
    rg = RngState(SEED, device="cuda")
    kw = dict(key_range=c.key_range, doc_range=c.doc_range, kv_heads=c.kv_heads)
    ctx, lse, mk = A.attn_fwd(qkv, c.B, c.S, c.H, c.D, c.causal, c.slopes, c.p, rg, SID, **kw)
    dqkv = A.attn_bwd(dctx, qkv, ctx, lse, c.B, c.S, c.H, c.D, c.causal, c.slopes, c.p, rg, SID, mk, **kw)
    torch.cuda.synchronize()
    for k in (env or {}):
        monkeypatch.delenv(k)
    assert ctx.dtype == dtype and dqkv.dtype == dtype and lse.dtype == F32
    return ctx.cpu(), lse.cpu(), dqkv.cpu()


def _ids(cases):
    return ["-".join(str(v) for v in case if v is not None) for case in cases]


# ------------------------------------------------------------------------------------------
# default forms: every regime x {plain, causal, causal + ALiBi} x p in {0, 0.1}
# ------------------------------------------------------------------------------------------
DEFAULT = [(r, s, m, p) for r in O.ATTN_REGIMES for s in ("s200", "s512", "d128") for m in MODES for p in (0.0, 0.1)]
DEFAULT += [(r, "s33", m, p) for r in ("zero_rows", "spike_at_edges") for m in MODES for p in (0.0, 0.1)]


@pytest.mark.parametrize("case", DEFAULT, ids=_ids(DEFAULT))
def test_default_forms(case, monkeypatch):
    c = attn_case(*case)
    check_attention(c, *run_kernels(c, monkeypatch), "kernel", "default")
    if c.regime.startswith("spikes"):    # textbook online softmax (rescale on every growth), and never rescaling
        for thr in ("0", "1000"):
            check_attention(c, *run_kernels(c, monkeypatch, {"DTD_ATTN_RESCALE_THR": thr}), "kernel", f"thr {thr}")


# ------------------------------------------------------------------------------------------
# the pipelined forward, and the packed-fp32 softmax forms of the forward and dQ (head_dim 64)
# ------------------------------------------------------------------------------------------
FORMS = {"pipe": {"DTD_ATTN_FWD": "pipe"}, "pk": {"DTD_ATTN_FWD_PK": "1"}}
FORM_CASES = [(f, r, s, m, p) for f in FORMS for r in ("gauss", "onehot", "spikes_up") for s in ("s200", "s512")
              for m, p in (("plain", 0.0), ("causal", 0.1), ("alibi", 0.1))]


@pytest.mark.parametrize("case", FORM_CASES, ids=_ids(FORM_CASES))
def test_pipe_and_packed_forms(case, monkeypatch):
    c = attn_case(*case[1:])
    check_attention(c, *run_kernels(c, monkeypatch, FORMS[case[0]]), "kernel", case[0])


# ------------------------------------------------------------------------------------------
# instantiations no other test launches
# ------------------------------------------------------------------------------------------
# name -> (overrides, outputs that must equal the form `base` bit for bit, base).  The 128-key dQ tile
# and the 64-row dK/dV tile change the tile size itself: their dq / dk, dv are held to the oracle only.
VARIANTS = {
    "occ222": ({"DTD_ATTN_OCC": "2,2,2"}, ("ctx", "lse", "dq", "dk", "dv"), "default"),     # fwd, dQ <64,2,64,2>
    "occ111": ({"DTD_ATTN_OCC": "1,1,1"}, ("ctx", "lse", "dq", "dk", "dv"), "default"),     # <64,1,64,2>, dK/dV <64,1,128>
    "tile128": ({"DTD_ATTN_TILE": "64,128"}, ("ctx", "lse", "dk", "dv"), "default"),          # dQ <64,2,128,2>
    "bm64kv2": ({"DTD_ATTN_DKDV_BM": "64"}, ("ctx", "lse", "dq"), "default"),                 # dK/dV <64,2,64>
    "bm64kv1": ({"DTD_ATTN_DKDV_BM": "64", "DTD_ATTN_OCC": "3,1,3"}, ("ctx", "lse", "dq", "dk", "dv"), "bm64kv2"),  # <64,1,64>
}
# causal + dropout: the masked form of every variant, with keep words in flight through the tile ring, at
# a partial last tile (S 200) and at four full blocks (S 512); plain + dropout at S 512 is the one shape
# that takes the variants' no-mask dK/dV forms
VARIANT_CASES = [(r, s, "causal", 0.1) for r in ("gauss", "onehot", "spikes_up") for s in ("s200", "s512")]
VARIANT_CASES += [("gauss", "s512", "plain", 0.1)]
_RESULTS = {}


def _parts(c, out):
    ctx, lse, dqkv = out
    return dict(zip(("ctx", "lse", "dq", "dk", "dv"), (ctx, lse) + O.attn_split(dqkv, c.B, c.S, c.H, c.Hkv, c.D)))


def _variant_result(c, name, monkeypatch):
    """The kernels' result under a variant (or 'default'), computed once per case."""
    if (c.tag, name) not in _RESULTS:
        _RESULTS[(c.tag, name)] = run_kernels(c, monkeypatch, VARIANTS[name][0] if name != "default" else None)
    return _RESULTS[(c.tag, name)]


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("case", VARIANT_CASES, ids=_ids(VARIANT_CASES))
def test_unlaunched_instantiations(case, name, monkeypatch):
    c = attn_case(*case)
    _, same, base = VARIANTS[name]
    out = _variant_result(c, name, monkeypatch)
    check_attention(c, *out, "kernel", name)
    got, ref = _parts(c, out), _parts(c, _variant_result(c, base, monkeypatch))
    differ = [n for n in same if not torch.equal(got[n], ref[n])]
    assert not differ, f"{name} {c.tag}: {differ} differ from the {base} form's, which runs the same arithmetic"


# ------------------------------------------------------------------------------------------
# key ranges, document spans, grouped-query attention
# ------------------------------------------------------------------------------------------
MASK_REGIMES = ("gauss", "onehot", "spikes_up", "zero_rows")
MASKED = [(r, s, m, p, k) for r in MASK_REGIMES for k in ("pad", "empty", "doc")
          for s, m, p in (("s200", "causal", 0.1), ("s200", "plain", 0.0), ("d128", "plain", 0.1), ("d128", "alibi", 0.0))]


@pytest.mark.parametrize("case", MASKED, ids=_ids(MASKED))
def test_key_range_and_doc_range(case, monkeypatch):
    """Left and right padding, an empty range, and three documents with their seams inside 64-key tiles
    and a pad tail.  Rows without a key: lse = -inf, ctx = dq = 0 exactly; keys outside every range: dk =
    dv = 0 exactly (their oracle rows and row scales are exactly 0, so the metric demands it)."""
    c = attn_case(*case)
    check_attention(c, *run_kernels(c, monkeypatch), "kernel", c.mask)


GQA_REGIMES = ("gauss", "peaked", "row_scales", "spikes_up")
GQA = [(r, s, m, 0.0, k, kv) for r in GQA_REGIMES for s in ("g200", "g160") for kv in (2, 1)
       for k, m in ((None, "plain"), (None, "causal"), ("pad", "causal"), ("empty", "plain"), ("doc", "plain"), ("doc", "causal"))]


@pytest.mark.parametrize("case", GQA, ids=_ids(GQA))
def test_grouped_query(case, monkeypatch):
    """G = 2 and 4 at head_dim 64 and 128.  ``row_scales`` puts query heads whose rows differ by up to
    2^6 in size into one dK / dV group sum."""
    c = attn_case(*case)
    check_attention(c, *run_kernels(c, monkeypatch), "kernel", f"gqa G{c.H // c.Hkv}")


# ------------------------------------------------------------------------------------------
# reference-precision fp32 kernels
# ------------------------------------------------------------------------------------------
F32_CASES = [(r, s, m, p) for r in ("gauss", "onehot", "row_scales", "spikes_up") for s in ("s200", "d128")
             for m, p in (("plain", 0.0), ("causal", 0.0), ("plain", 0.1), ("alibi", 0.1))]


@pytest.mark.parametrize("case", F32_CASES, ids=_ids(F32_CASES))
def test_f32_kernels(case, monkeypatch):
    c = attn_case(*case)
    check_attention(c, *run_kernels(c, monkeypatch, dtype=F32), "f32", "fp32")


# ------------------------------------------------------------------------------------------
# the experimental one-kernel backward
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fused", "fused4"])
@pytest.mark.parametrize("regime,p", [("gauss", 0.1), ("onehot", 0.0), ("row_scales", 0.1)])
def test_fused_backward(regime, p, form, monkeypatch):
    if not A.fused_bwd_built():
        pytest.skip("the one-kernel backward is compiled only into experimental builds (DTD_BUILD_EXPERIMENTAL=1)")
    c = attn_case(regime, "s512", "plain", p)
    assert A.fused_bwd_applies(c.S, c.D, c.causal, c.slopes)
    prev = A.set_bwd_form(form)
    try:
        out = run_kernels(c, monkeypatch)
    finally:
        A.set_bwd_form(prev)
    check_attention(c, *out, "kernel", form)


def test_print_worst_ratios():
    print_worst(GPU_TITLE)
