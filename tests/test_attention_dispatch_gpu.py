"""Which ``dtd_attn_*`` entry point ``attn_fwd`` / ``attn_bwd`` launch for a call, and with which arguments.

``_lib.call`` is wrapped by a recorder that forwards to the real function, and every case asserts the
entry-point name and the whole argument tuple of its forward and backward launch.  The expected tuples
are written out here from the layout rules of the ``ops/attention.py`` module docstring (q | k | v
blocks of ``H*D`` / ``Hkv*D`` columns inside one row of ``ld`` elements, ``ctx`` rows of ``H*D``), not
taken from the module: q/k/v and dq/dk/dv as byte offsets from ``qkv.data_ptr()`` / ``dqkv.data_ptr()``,
the sizes, ``causal``, ``scale``, ``p``, the window, which of the key-range / document pointers are
null, and the stream last.  ``delta`` is scratch the call allocates: only required to be non-null.

A backward runs the family its forward ran (``dtd_attn_fwd_X`` <-> ``dtd_attn_bwd_X``) -- or launches
nothing where the call takes the math reference.

All cases: B = 2, S = 160 (two 128-query blocks, the second partial), H = 4.
"""
import ctypes
from typing import NamedTuple

import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.rng import RngState

pytestmark = pytest.mark.gpu

B, S, H = 2, 160, 4
SID = 3
BF16, F32 = torch.bfloat16, torch.float32
FORM_ENV = ("DTD_ATTN_FWD", "DTD_ATTN_FWD_PK", "DTD_ATTN_OCC", "DTD_ATTN_TILE", "DTD_ATTN_DKDV_BM", "DTD_ATTN_RESCALE_THR",
            "DTD_ATTN_BWD")


class Anything:
    """Matches a non-null pointer the test cannot name (scratch allocated inside the call)."""

    def __eq__(self, other):
        return isinstance(other, int) and other != 0

    def __repr__(self):
        return "<non-null>"


ANY = Anything()


class Case(NamedTuple):
    name: str
    fwd: str | None              # expected entry points (None: no launch, the math reference)
    bwd: str | None
    D: int = 64
    dtype: torch.dtype = BF16
    mask: str = "plain"          # plain | range | doc
    kv_heads: int | None = None
    window: int | None = None
    causal: bool = False
    p: float = 0.0
    alibi: bool = False
    premask: bool = False        # keep bits from attn_masks_async
    dbias: bool = False
    bwd_masks: bool = True       # hand the forward's keep bits to the backward


def _mha(D, mask):
    sfx = {"plain": "", "range": "_range", "doc": "_doc"}[mask]
    return Case(f"mha-d{D}-{mask}", "dtd_attn_fwd" + sfx, "dtd_attn_bwd" + sfx, D=D, mask=mask)


CASES = (
    [_mha(D, m) for D in (64, 128) for m in ("plain", "range", "doc")]
    + [Case("mha-dropout-alibi-causal", "dtd_attn_fwd", "dtd_attn_bwd", causal=True, p=0.1, alibi=True),
       Case("mha-masks-ahead", "dtd_attn_fwd", "dtd_attn_bwd", p=0.1, premask=True),
       Case("mha-dbias-d64", "dtd_attn_fwd", "dtd_attn_bwd", D=64, dbias=True),
       Case("mha-dbias-d128", "dtd_attn_fwd", "dtd_attn_bwd", D=128, dbias=True)]
    + [Case(f"gqa-{m}{'-dbias' if db else ''}", "dtd_attn_fwd_gqa", "dtd_attn_bwd_gqa", mask=m, kv_heads=2, causal=True, dbias=db)
       for m in ("plain", "range", "doc") for db in (False, True)]
    + [Case(f"win-hkv{kv}-{m}", "dtd_attn_fwd_win", "dtd_attn_bwd_win", mask=m, kv_heads=kv, window=70, causal=True)
       for kv in (None, 2) for m in ("plain", "range", "doc")]
    + [Case("win-whole-sequence-mha", "dtd_attn_fwd", "dtd_attn_bwd", window=160, causal=True),
       Case("win-whole-sequence-gqa", "dtd_attn_fwd_gqa", "dtd_attn_bwd_gqa", kv_heads=2, window=160, causal=True),
       Case("f32-plain", "dtd_attn_fwd_f32", "dtd_attn_bwd_f32", dtype=F32, causal=True),
       Case("f32-range", None, None, dtype=F32, mask="range"),
       Case("f32-dropout-bwd-without-masks", "dtd_attn_fwd_f32", None, dtype=F32, p=0.1, bwd_masks=False)]
)


class Run(NamedTuple):
    calls: list                  # (entry, args) of every dtd_attn_fwd* / dtd_attn_bwd* launch, in order
    epilogue: list               # ("finalize", part) / ("bias_grad",): how dbias was formed
    t: dict                      # the tensors of the call


def run_case(c: Case, monkeypatch) -> Run:
    """attn_fwd, then attn_bwd on its results, with ``_lib.call`` and the two dbias epilogues recorded."""
    calls, epilogue = [], []
    real_call, real_fin, real_bg = _lib.call, Fx._finalize, Fx.bias_grad

    def call(name, *args):
        if name.startswith(("dtd_attn_fwd", "dtd_attn_bwd")):
            calls.append((name, args))
        return real_call(name, *args)

    def finalize(part, *args, **kw):
        epilogue.append(("finalize", part))
        return real_fin(part, *args, **kw)

    def bias_grad(*args, **kw):
        epilogue.append(("bias_grad",))
        return real_bg(*args, **kw)

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(Fx, "_finalize", finalize)
    monkeypatch.setattr(Fx, "bias_grad", bias_grad)

    D, Hkv = c.D, c.kv_heads or H
    g = torch.Generator().manual_seed(1234)
    qkv = torch.randn(B * S, (H + 2 * Hkv) * D, generator=g).to(c.dtype).cuda()
    dctx = torch.randn(B * S, H * D, generator=g).to(c.dtype).cuda()
    kw = {}
    key_range = doc = None
    if c.mask == "range":
        key_range = kw["key_range"] = torch.tensor([[0, 100], [30, 160]], dtype=torch.int32, device="cuda")
    elif c.mask == "doc":
        seg = torch.zeros(B, S, dtype=torch.int64)
        seg[0, :50], seg[0, 50:150] = 1, 2                 # two documents, ten pads
        seg[1, 5:135], seg[1, 135:] = 1, 2                 # a document across the block seam
        doc = kw["doc_range"] = A.doc_range_from_segment_ids(seg.cuda())
    if c.kv_heads is not None:
        kw["kv_heads"] = c.kv_heads
    if c.window is not None:
        kw["window"] = c.window
    slopes = A.alibi_slopes(H).cuda() if c.alibi else None
    rng = RngState(7, device="cuda") if c.p > 0 else None
    pending = A.attn_masks_async(B, S, H, D, c.p, rng, SID, "cuda") if c.premask else None
    ctx, lse, masks = A.attn_fwd(qkv, B, S, H, D, c.causal, slopes, c.p, rng, SID, masks=pending, **kw)
    db = torch.zeros(qkv.shape[1], dtype=F32, device="cuda") if c.dbias else None
    dqkv = A.attn_bwd(dctx, qkv, ctx, lse, B, S, H, D, c.causal, slopes, c.p, rng, SID,
                      masks=masks if c.bwd_masks else None, dbias=(db, False) if c.dbias else None, **kw)
    Fx.flush_finalizes()
    torch.cuda.synchronize()
    t = dict(qkv=qkv, dctx=dctx, ctx=ctx, lse=lse, masks=masks, dqkv=dqkv, dbias=db, key_range=key_range,
             doc=doc.flat if doc is not None else None, slopes=slopes, rng=rng, pending=pending)
    return Run(calls, epilogue, t)


def expected(c: Case, t: dict):
    """The (entry, args) pair of the forward and of the backward launch, from the layout rules."""
    D, es = c.D, 2 if c.dtype == BF16 else 4
    Hkv = c.kv_heads or H
    scale = {64: 0.125, 128: 128 ** -0.5}[D]
    qb, gb, st = t["qkv"].data_ptr(), t["dqkv"].data_ptr(), _lib.stream()
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    kr, doc = ptr(t["key_range"]), ptr(t["doc"])
    grouped = c.fwd in ("dtd_attn_fwd_gqa", "dtd_attn_fwd_win")
    if grouped:      # q block of H heads, then k and v of Hkv heads each
        ld, ko, vo = (H + 2 * Hkv) * D, H * D * es, (H + Hkv) * D * es
        win = (c.window,) if c.fwd == "dtd_attn_fwd_win" else ()
        tail = (B, S, H, Hkv, D, ld, H * D, int(c.causal), scale, *win, kr, doc, st)
        fwd = (qb, qb + ko, qb + vo, ptr(t["ctx"]), ptr(t["lse"]), *tail)
        bwd = (qb, qb + ko, qb + vo, ptr(t["ctx"]), ptr(t["dctx"]), ptr(t["lse"]), ANY, gb, gb + ko, gb + vo, *tail)
        return (c.fwd, fwd), (c.bwd, bwd)
    # [B, S, 3, H, D]: three blocks of H heads
    ld, ko, vo = 3 * H * D, H * D * es, 2 * H * D * es
    sizes = (B, S, H, D, ld, H * D, int(c.causal), scale, c.p)
    masks = ptr(t["masks"]) if c.p > 0 else None
    fwd = (qb, qb + ko, qb + vo, ptr(t["ctx"]), ptr(t["lse"]), ptr(t["slopes"]), masks, *sizes)
    bwd = (qb, qb + ko, qb + vo, ptr(t["ctx"]), ptr(t["dctx"]), ptr(t["lse"]), ANY, masks, gb, gb + ko, gb + vo,
           ptr(t["slopes"]), *sizes)
    if c.dtype == F32:
        return (c.fwd, (*fwd, st)), (c.bwd, (*bwd, st))
    # bf16: the rng state (null when the keep bits were generated ahead) and the stream id; the backward
    # takes the bias-gradient partials, one fp32 row per 32-row block: at D = 64 only
    rng = ptr(t["rng"].state) if c.p > 0 and not c.premask else None
    part = ANY if c.dbias and D == 64 else None
    rd = tuple(x for x in (kr, doc) if x is not None)      # the _range / _doc forms take theirs, non-null
    return (c.fwd, (*fwd, rng, SID, *rd, st)), (c.bwd, (*bwd, part, *rd, st))


def _as_passed(args):
    """Floats as the C ABI receives them (``float``), so 1 / sqrt(D) compares in fp32."""
    return tuple(ctypes.c_float(a).value if isinstance(a, float) else a for a in args)


@pytest.fixture(autouse=True)
def default_forms(monkeypatch):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_entry_points_and_arguments(case, monkeypatch):
    c = case
    run = run_case(c, monkeypatch)
    t = run.t
    assert A.kernel_supported(t["qkv"], c.D) or c.dtype == F32
    want = [w for w in expected(c, t) if w[0] is not None]
    assert [n for n, _ in run.calls] == [n for n, _ in want]
    for (name, got), (_, exp) in zip(run.calls, want):
        assert len(got) == len(exp) == len(_lib._SIGS[name][1]), name
        got, exp = _as_passed(got), _as_passed(exp)
        assert got == exp, (name, [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if not g == e])
    # the backward runs the forward's family, or nothing
    names = [n for n, _ in run.calls]
    fwd = next((n for n in names if n.startswith("dtd_attn_fwd")), None)
    bwd = next((n for n in names if n.startswith("dtd_attn_bwd")), None)
    assert bwd in (None, fwd.replace("_fwd", "_bwd") if fwd else None)
    assert bwd is not None or c.bwd is None
    # results in the documented layouts, whichever path produced them
    assert t["ctx"].shape == (B * S, H * c.D) and t["lse"].shape == (B, H, S) and t["dqkv"].shape == t["qkv"].shape
    if c.premask:
        assert t["masks"] is t["pending"].masks
    if c.dbias:
        if c.bwd == "dtd_attn_bwd" and c.D == 64:       # per-wave partials from the kernels' epilogues
            (kind, part), = run.epilogue
            ld = 3 * H * c.D
            assert kind == "finalize" and part.shape == (B * 4 * 2, ld) and part.dtype == F32
            assert part.data_ptr() == run.calls[-1][1][21]
        else:                                           # a pass of its own over dqkv (which finalizes its own partials)
            assert run.epilogue[0] == ("bias_grad",)
        # dqkv is the fp32 gradient rounded to bf16 once (relative error <= 2^-9 an element): its column
        # sums lie within 2^-9 sum |dqkv| of the partials'; 2^-8 leaves room for the fp32 summation orders
        g = t["dqkv"].float()
        assert ((t["dbias"] - g.sum(0)).abs() <= 2.0 ** -8 * g.abs().sum(0) + 1e-6).all()
    else:
        assert run.epilogue == []
