"""The hand-written GEMM family -- ``ops/csrc/gemm.hip`` (every epilogue, both kernel forms, both tile
orders), ``gemm_w4.hip``, ``wgrad.hip`` and ``gemm_f32.hip`` -- against the fp64 product, element by element,
with the cases and checkers of ``tests/gemm_cases.py``: the exact regime (``torch.equal``: one stale 16-byte
chunk, wrong row or missing bias anywhere fails), the rounded regime (a per-element bound and the share of
outputs that are not the correctly rounded result: truncation and low-precision accumulators), split-K
partials one by one, column views of wider buffers with a canary around every output, and non-finite inputs.
``tests/test_gemm_cases_cpu.py`` shows that a correct stand-in passes all of it and what each check rejects.

What the first run on an MI355X found:

  * ``EPI_GELU_TANH_BWD`` (``gelu_bwd_gemm(act="gelu_tanh")``): du up to 70 % off where the derivative is small.
    ``gelu_tanh_grad`` formed 1 + t and 1 - t^2 from t = tanh(y), which cancel in the negative tail (u about -5:
    derivative ~1e-6, absolute error of the same size -- inside the activation's own fp32 bound, which is why
    ``test_activation_fast_math_accuracy_fp32`` never saw it), and the epilogue multiplies that by dA: got
    7.54e-6 for 4.46e-6, -1.14e-5 for -6.76e-6, at every shape and in both kernel forms, 2 to 559 elements
    per case beyond one ulp + 2e-6.  The derivative now comes from q = e^{-2|y|} and 1 / (1 + q) with no
    cancelling difference (``ops/csrc/gemm.hip``; same v_exp and v_rcp, same registers, no scratch; 99.3 -
    99.9 us against the old form's 100.7 at 16384 x 3072 x 768, alternating runs; on Gaussian data 2.3 % of
    du change, by one bf16 ulp); the
    ``gelu_tanh_bwd`` cases of ``test_gemm_epilogue_exact`` and ``..._one_tile_form`` are the regression test.
    The stored-derivative epilogue ``EPI_BIAS_GELU_TANH_G`` keeps the old form: its g is held to the same bound
    and passes (the cancellation stays under the 2e-6 floor when nothing multiplies it).
  * Nothing else: every exact comparison held on the first run -- all eleven epilogues in both tile orders
    and both kernel forms, the tile seam, ``gemm_w4``, every split-K partial of the four ``wgrad_tn`` variants
    (the default spread-DMA form on ranges shorter than its ring and on empty ranges included), the two
    ``gemm_f32`` forms -- and so did every canary and both non-finite rows.

Worst error of the transcendental epilogues in bf16 ulps of the fp64 value, over all shapes (the bound is 1;
a correctly rounded result has at most 0.5, and the exact grid holds only the 513 multiples of 1/16 in [-16, 16]):

    linear_gelu gelu a 0.491, gelu_tanh a 0.533        gelu_bwd_gemm gelu du 0.504, gelu_tanh du 0.500 (after the fix)
    linear_act_grad gelu g 0.499, a 0.491              linear_act_grad gelu_tanh g 0.507, a 0.533

Rounded regime, worst error / bound and misrounded share (cap 1e-2) at (512, 768, 768) | (256, 256, 128):

    gemm_bt + bias    gauss 0.84, 1.5e-4 | 0.97, 7.6e-5   row_scales 0.89, 1.3e-4 | 0.98, 7.6e-5   cancel 0.25, 2.4e-3 | 0.87, 3.7e-4
    matmul_nt_add_    gauss 0.84, 1.2e-4 | 0.97, 3.1e-5   row_scales 0.84, 1.2e-4 | 0.97, 3.1e-5   cancel 0.25, 2.3e-3 | 0.86, 3.8e-4
    linear_gelu u     gauss 0.84, 1.5e-4 | 0.97, 7.6e-5
    gemm_w4 + bias    gauss 0.84, 1.5e-4                  row_scales 0.89, 1.3e-4                  cancel 0.25, 2.4e-3
    gemm_w4 out=      gauss 0.84, 1.2e-4                  row_scales 0.84, 1.2e-4                  cancel 0.25, 2.3e-3
    wgrad_tn          gauss, T = 1024 in 32 partials: 0.027 of the fp32 bound (no share test on fp32 outputs)

(The worst error / bound is the final bf16 rounding, close to 1 wherever an output sits just above a power of
two; the stand-in of ``test_gemm_cases_cpu.py`` gives the same figures.)
"""
import contextlib
import functools
import types

import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import gemm as G
from distributed_training_and_deepspeed_amd.ops.grad import splitk_reduce

from . import gemm_cases as GC
from . import oracles as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
WORST_ULP: dict = {}          # epilogue output -> worst error in bf16 ulps seen in this run (printed)


def dev(t):
    return None if t is None else t.to(DEV)


def note_ulp(key, val):
    WORST_ULP[key] = max(WORST_ULP.get(key, 0.0), val)
    print(f"\nworst error of {key}: {WORST_ULP[key]:.3f} bf16 ulp")


@contextlib.contextmanager
def tile_order(mode):
    prev = G._SCHED[0]
    G.set_sched(mode)
    try:
        yield
    finally:
        G.set_sched(prev)


@contextlib.contextmanager
def one_tile_form():
    """gemm.hip's one-tile-per-workgroup kernel instead of the persistent one."""
    prev = _lib.lib().dtd_gemm_set_variant(0)
    try:
        yield
    finally:
        _lib.lib().dtd_gemm_set_variant(prev)


# ------------------------------------------------------------------------------------------
# cases and oracles, computed once per shape and never modified
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact(shape):
    """The exact case of a shape with its device operands and the fp64 product."""
    case = GC.exact_operands(*shape)
    case.d = types.SimpleNamespace(**{k: dev(getattr(case, k)) for k in ("a", "b", "bias", "c0", "u", "g")})
    case.prod = GC.product(case)
    return case


@functools.lru_cache(maxsize=None)
def fwd_oracle(shape, act, bias):
    """u = x W^T (+ b) (exact) and fp64 act(u), act'(u)."""
    case = exact(shape)
    u = case.prod + O.f64(case.bias) if bias else case.prod
    r = O.activation(u.to(BF16), act, dy=torch.ones_like(u))
    return types.SimpleNamespace(u=u, a=r["a"], g=r["du"])


@functools.lru_cache(maxsize=None)
def bwd_oracle(shape, act):
    """du = (dy w_t^T) act'(u) in fp64 for the case's stored u; act None: times the stored derivative g."""
    case = exact(shape)
    if act is None:
        return case.prod * O.f64(case.g)
    return O.activation(case.u, act, dy=case.prod)["du"]


def seam(K):
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    shape = GC.seam_shape(cus, K)
    assert (shape[0] // 256) * (shape[1] // 256) > cus // 8 * 8       # some workgroup takes a second tile
    return shape


# ------------------------------------------------------------------------------------------
# gemm.hip: the 11 epilogues, exact regime
# ------------------------------------------------------------------------------------------
def run_store(shape, bias):
    case = exact(shape)
    assert G.supported(*shape, case.d.a, case.d.b)
    c = G.gemm_bt(case.d.a, case.d.b, case.d.bias if bias else None)
    GC.assert_equal(c, case.prod + O.f64(case.bias) if bias else case.prod, f"gemm_bt bias={bias}")


def run_add(shape, bias):
    case = exact(shape)
    c = case.d.c0.clone()
    assert G.supported(*shape, case.d.a, case.d.b, c)
    G.matmul_nt_add_(c, case.d.a, case.d.b)
    GC.assert_equal(c, case.prod + O.f64(case.c0), "matmul_nt_add_")


def run_linear_gelu(act, shape, bias):
    case, ref = exact(shape), fwd_oracle(shape, act, bias)
    assert G.supported(*shape, case.d.a, case.d.b)
    u, a = G.linear_gelu(case.d.a, case.d.b, case.d.bias if bias else None, act)
    GC.assert_equal(u, ref.u, f"linear_gelu {act} u bias={bias}")
    if act == "relu":
        GC.assert_equal(a, ref.a, "linear_gelu relu a")
    else:
        note_ulp(f"linear_gelu {act} a", GC.assert_within_ulp(a, ref.a, f"linear_gelu {act} a bias={bias}"))
    return a


def run_linear_act_grad(act, shape, bias):
    case, ref = exact(shape), fwd_oracle(shape, act, bias)
    assert G.supported(*shape, case.d.a, case.d.b)
    b = case.d.bias if bias else None
    g, a = G.linear_act_grad(case.d.a, case.d.b, b, act)
    note_ulp(f"linear_act_grad {act} g", GC.assert_within_ulp(g, ref.g, f"linear_act_grad {act} g bias={bias}"))
    note_ulp(f"linear_act_grad {act} a", GC.assert_within_ulp(a, ref.a, f"linear_act_grad {act} a bias={bias}"))
    _, a_u = G.linear_gelu(case.d.a, case.d.b, b, act)
    assert torch.equal(a, a_u)                  # the same activation values as the u-storing epilogue, bit for bit


def run_bwd(act, shape, bias):
    """gelu_bwd_gemm (act) / mul_bwd_gemm (act None): du, and dbias written and accumulated.  ``bias`` unused:
    the backward epilogues take none."""
    case, du64 = exact(shape), bwd_oracle(shape, act)
    second = case.d.g if act is None else case.d.u
    assert G.supported(*shape, case.d.a, case.d.b, second)
    exact_du = act in (None, "relu")
    name = "mul_bwd_gemm" if act is None else f"gelu_bwd_gemm {act}"
    for acc in (False, True):
        dst = dev(case.dst).clone()
        if act is None:
            du = G.mul_bwd_gemm(case.d.a, case.d.b, second, dbias=(dst, acc))
        else:
            du = G.gelu_bwd_gemm(case.d.a, case.d.b, second, dbias=(dst, acc), act=act)
        base = case.dst if acc else None
        if exact_du:
            GC.assert_equal(du, du64, f"{name} du")
            GC.assert_equal(dst, du64.sum(0) + (O.f64(base) if acc else 0.0), f"{name} dbias acc={acc}")
        else:
            note_ulp(f"{name} du", GC.assert_within_ulp(du, du64, f"{name} du"))
            GC.assert_colsum_close(dst, du64, f"{name} dbias acc={acc}", base=base)
    du_only = (G.mul_bwd_gemm(case.d.a, case.d.b, second) if act is None
               else G.gelu_bwd_gemm(case.d.a, case.d.b, second, act=act))
    assert torch.equal(du_only, du)             # without a dbias destination: the same du


EPILOGUES = {
    "store": (G.EPI_STORE, run_store),
    "add": (G.EPI_ADD, run_add),
    "gelu": (G.EPI_BIAS_GELU, functools.partial(run_linear_gelu, "gelu")),
    "gelu_tanh": (G.EPI_BIAS_GELU_TANH, functools.partial(run_linear_gelu, "gelu_tanh")),
    "relu": (G.EPI_BIAS_RELU, functools.partial(run_linear_gelu, "relu")),
    "gelu_g": (G.EPI_BIAS_GELU_G, functools.partial(run_linear_act_grad, "gelu")),
    "gelu_tanh_g": (G.EPI_BIAS_GELU_TANH_G, functools.partial(run_linear_act_grad, "gelu_tanh")),
    "gelu_bwd": (G.EPI_GELU_BWD, functools.partial(run_bwd, "gelu")),
    "gelu_tanh_bwd": (G.EPI_GELU_TANH_BWD, functools.partial(run_bwd, "gelu_tanh")),
    "relu_bwd": (G.EPI_RELU_BWD, functools.partial(run_bwd, "relu")),
    "mul_bwd": (G.EPI_MUL_BWD, functools.partial(run_bwd, None)),
}
HAS_BIAS = ("store", "gelu", "gelu_tanh", "relu", "gelu_g", "gelu_tanh_g")
# an epilogue that always takes the static tile order runs once
EPI_ORDERS = [(name, order) for name, (code, _) in EPILOGUES.items() for order in ("static", "dynamic")
              if not (order == "dynamic" and code in G._STATIC_EPIS)]


def run_epilogue(name, shape):
    for bias in ((True, False) if name in HAS_BIAS else (False,)):
        EPILOGUES[name][1](shape, bias)


def test_all_eleven_epilogues_are_covered():
    assert sorted(code for code, _ in EPILOGUES.values()) == list(range(11))
    assert len(EPI_ORDERS) == 2 * 11 - len(G._STATIC_EPIS)


@pytest.mark.parametrize("shape", GC.GEMM_SHAPES, ids=str)
@pytest.mark.parametrize("name,order", EPI_ORDERS)
def test_gemm_epilogue_exact(name, order, shape):
    with tile_order(order):
        run_epilogue(name, shape)


@pytest.mark.parametrize("name", list(EPILOGUES))
def test_gemm_epilogue_exact_one_tile_form(name):
    with one_tile_form():
        run_epilogue(name, (512, 768, 320))


# ------------------------------------------------------------------------------------------
# gemm.hip: the tile seam of the persistent form (a workgroup's second tile: the cross-tile prefetch, the
# claim of the dynamic queue; K = 64 is the single-K-step claim path)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["static", "dynamic"])
@pytest.mark.parametrize("K", GC.SEAM_K)
def test_gemm_tile_seam_exact(K, order):
    shape = seam(K)
    with tile_order(order):
        run_store(shape, True)
        run_linear_act_grad("gelu", shape, True)
        run_bwd(None, shape, False)


# ------------------------------------------------------------------------------------------
# layout: operands and outputs as column views of wider buffers, a canary around every output
# ------------------------------------------------------------------------------------------
def wider(t, left=8, right=24):
    """(buffer, view): ``t`` on the device as a column view of a canary-filled buffer whose rows are
    left + right elements longer (row stride and view offset stay multiples of 8 elements)."""
    rows, cols = t.shape
    buf = torch.full((rows, left + cols + right), GC.CANARY, dtype=t.dtype, device=DEV)
    view = buf[:, left:left + cols]
    view.copy_(t)
    return buf, view


def assert_outside_intact(buf, view, what):
    left = view.storage_offset() % buf.stride(0)
    cols = view.shape[1]
    assert bool((buf[:, :left] == GC.CANARY).all()) and bool((buf[:, left + cols:] == GC.CANARY).all()), \
        f"{what}: written outside the view"


def guarded(shape, dtype=F32, pad=1024):
    """(buffer, contiguous view of ``shape`` out of its middle), canary everywhere."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad,), GC.CANARY, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n].view(shape)


def assert_guards_intact(buf, view, what, pad=1024):
    assert bool((buf[:pad] == GC.CANARY).all()) and bool((buf[pad + view.numel():] == GC.CANARY).all()), \
        f"{what}: written outside the destination"


@pytest.mark.parametrize("order", ["static", "dynamic"])
def test_gemm_strided_views_and_canaries(order):
    shape = (512, 768, 320)
    M, N, K = shape
    case = exact(shape)
    (_, a), (_, b) = wider(case.a), wider(case.b, 16, 48)
    (_, u), (_, g) = wider(case.u, 24, 8), wider(case.g, 8, 56)
    canary = torch.full((M, N), GC.CANARY, dtype=BF16)
    with tile_order(order):
        # store with bias
        cb, c = wider(canary)
        assert G.supported(M, N, K, a, b, c) and a.stride(0) > K and c.stride(0) > N
        G._call(G.EPI_STORE, a, b, c, bias=case.d.bias)
        GC.assert_equal(c, case.prod + O.f64(case.bias), "strided store")
        assert_outside_intact(cb, c, "store")
        # residual add in place
        cb, c = wider(case.c0, 16, 16)
        G._call(G.EPI_ADD, a, b, c)
        GC.assert_equal(c, case.prod + O.f64(case.c0), "strided add")
        assert_outside_intact(cb, c, "add")
        # forward activation epilogues: two outputs of one stride
        for act in ("gelu", "relu"):
            ref = fwd_oracle(shape, act, True)
            (cb, c), (c2b, c2) = wider(canary, 8, 24), wider(canary, 24, 8)
            G._call(G._ACT_EPI[act][0], a, b, c, c2=c2, bias=case.d.bias)
            GC.assert_equal(c, ref.u, f"strided {act} u")
            if act == "relu":
                GC.assert_equal(c2, ref.a, "strided relu a")
            else:
                GC.assert_within_ulp(c2, ref.a, "strided gelu a")
            assert_outside_intact(cb, c, f"{act} u")
            assert_outside_intact(c2b, c2, f"{act} a")
        ref = fwd_oracle(shape, "gelu_tanh", True)
        (cb, c), (c2b, c2) = wider(canary, 8, 24), wider(canary, 24, 8)
        G._call(G.EPI_BIAS_GELU_TANH_G, a, b, c, c2=c2, bias=case.d.bias)
        GC.assert_within_ulp(c, ref.g, "strided gelu_tanh g")
        GC.assert_within_ulp(c2, ref.a, "strided gelu_tanh a")
        assert_outside_intact(cb, c, "g")
        assert_outside_intact(c2b, c2, "a")
        # backward epilogues: u / g strided, the fp32 column partials between guards
        rows = _lib.lib().dtd_gemm_bt_part_rows(M)
        for epi, second, du64 in ((G.EPI_MUL_BWD, g, bwd_oracle(shape, None)),
                                  (G.EPI_RELU_BWD, u, bwd_oracle(shape, "relu"))):
            cb, c = wider(canary, 16, 16)
            pb, part = guarded((rows, N))
            assert G.supported(M, N, K, a, b, c, second) and second.stride(0) > N
            G._call(epi, a, b, c, u=second, part=part)
            GC.assert_equal(c, du64, f"strided du (epilogue {epi})")
            GC.assert_equal(part, du64.view(rows, M // rows, N).sum(1), f"column partials (epilogue {epi})")
            assert_outside_intact(cb, c, "du")
            assert_guards_intact(pb, part, "column partials")
        # the finalized bias gradient between guards
        db, dst = guarded((N,))
        dst.copy_(dev(case.dst))
        G.mul_bwd_gemm(a, b, g, dbias=(dst, True))
        GC.assert_equal(dst, bwd_oracle(shape, None).sum(0) + O.f64(case.dst), "dbias")
        assert_guards_intact(db, dst, "dbias")


# ------------------------------------------------------------------------------------------
# gemm.hip: rounded regime
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounded(regime, shape):
    case = GC.rounded_operands(regime, *shape)
    case.d = types.SimpleNamespace(**{k: dev(getattr(case, k)) for k in ("a", "b", "bias", "c0")})
    case.rb_bias, case.rb_add = GC.rounded_bound(case, bias=True), GC.rounded_bound(case, c0=True)
    return case


def report(kernel, regime, shape, res):
    print(f"\n{kernel} {regime} {shape}: worst error / bound {res[0]:.2f}, misrounded share {res[1]:.1e}")


@pytest.mark.parametrize("shape", GC.ROUNDED_SHAPES, ids=str)
@pytest.mark.parametrize("regime", GC.ROUNDED_REGIMES)
def test_gemm_rounded(regime, shape):
    case = rounded(regime, shape)
    assert G.supported(*shape, case.d.a, case.d.b)
    c = G.gemm_bt(case.d.a, case.d.b, case.d.bias)
    report("gemm_bt", regime, shape, GC.check_rounded(c, case, ref_bound=case.rb_bias, what="gemm_bt"))
    c = case.d.c0.clone()
    G.matmul_nt_add_(c, case.d.a, case.d.b)
    report("matmul_nt_add_", regime, shape, GC.check_rounded(c, case, ref_bound=case.rb_add, what="matmul_nt_add_"))
    if regime == "cancel":          # the bare product: the bound alone (gemm_cases.rounded_operands)
        GC.check_rounded(G.gemm_bt(case.d.a, case.d.b), case, what="bare product", share=False)
    if regime == "gauss":
        u, _ = G.linear_gelu(case.d.a, case.d.b, case.d.bias)
        report("linear_gelu u", regime, shape, GC.check_rounded(u, case, ref_bound=case.rb_bias, what="linear_gelu u"))


# ------------------------------------------------------------------------------------------
# gemm.hip: non-finite inputs stay in their rows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["static", "dynamic"])
def test_gemm_nonfinite_rows(order):
    """+inf and NaN in two rows of A: those rows are non-finite exactly where the fp64 product is (inf times a
    zero of B is NaN), every other row is finite and exact."""
    shape = (256, 256, 128)
    case = exact(shape)
    a = case.a.clone()
    a[3, 5], a[200, 77] = float("inf"), float("nan")
    ref = O.f64(a) @ O.f64(case.b).t() + O.f64(case.bias)
    assert bool(torch.isnan(ref[3]).any()) and bool(torch.isinf(ref[3]).any()) and bool(torch.isnan(ref[200]).all())
    with tile_order(order):
        ad = dev(a)
        assert G.supported(*shape, ad, case.d.b)
        c = G.gemm_bt(ad, case.d.b, case.d.bias)
    err = O.slice_errors(c, ref)                   # asserts finite where ref is, equal where it is not
    assert float(err.max()) == 0.0
    keep = torch.ones(256, dtype=torch.bool)
    keep[[3, 200]] = False
    assert bool(torch.isfinite(c.cpu()[keep].float()).all())
    GC.assert_equal(c.cpu()[keep], (case.prod + O.f64(case.bias))[keep], "the finite rows")


# ------------------------------------------------------------------------------------------
# gemm_w4.hip
# ------------------------------------------------------------------------------------------
def run_w4(shape):
    case = exact(shape)
    assert G.w4_supported(*shape, case.d.a, case.d.b)
    GC.assert_equal(G.gemm_w4(case.d.a, case.d.b, case.d.bias), case.prod + O.f64(case.bias), "gemm_w4 bias")
    GC.assert_equal(G.gemm_w4(case.d.a, case.d.b), case.prod, "gemm_w4")
    c = case.d.c0.clone()
    assert G.w4_supported(*shape, case.d.a, case.d.b, c)
    G.gemm_w4(case.d.a, case.d.b, out=c)
    GC.assert_equal(c, case.prod + O.f64(case.c0), "gemm_w4 out=")


@pytest.mark.parametrize("shape", GC.W4_SHAPES, ids=str)
def test_w4_exact(shape):
    run_w4(shape)


def test_w4_tile_seam_exact():
    run_w4(seam(GC.W4_SEAM_K))


@pytest.mark.parametrize("regime", GC.ROUNDED_REGIMES)
def test_w4_rounded(regime):
    shape = (512, 768, 768)
    case = rounded(regime, shape)
    assert G.w4_supported(*shape, case.d.a, case.d.b)
    c = G.gemm_w4(case.d.a, case.d.b, case.d.bias)
    report("gemm_w4", regime, shape, GC.check_rounded(c, case, ref_bound=case.rb_bias, what="gemm_w4"))
    c = case.d.c0.clone()
    G.gemm_w4(case.d.a, case.d.b, out=c)
    report("gemm_w4 out=", regime, shape, GC.check_rounded(c, case, ref_bound=case.rb_add, what="gemm_w4 out="))
    if regime == "cancel":
        GC.check_rounded(G.gemm_w4(case.d.a, case.d.b), case, what="bare product", share=False)


def test_w4_strided_views_and_canaries():
    shape = (512, 768, 320)
    M, N, K = shape
    case = exact(shape)
    (_, a), (_, b) = wider(case.a, 16, 8), wider(case.b, 8, 40)
    cb, c = wider(torch.full((M, N), GC.CANARY, dtype=BF16))
    assert G.w4_supported(M, N, K, a, b, c) and a.stride(0) > K and b.stride(0) > K and c.stride(0) > N
    _lib.call("dtd_gemm_w4", G.EPI_STORE, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
              c.stride(0), case.d.bias.data_ptr(), M, N, K, _lib.stream())
    GC.assert_equal(c, case.prod + O.f64(case.bias), "strided gemm_w4")
    assert_outside_intact(cb, c, "gemm_w4")
    cb, c = wider(case.c0, 24, 16)
    G.gemm_w4(a, b, out=c)
    GC.assert_equal(c, case.prod + O.f64(case.c0), "strided gemm_w4 out=")
    assert_outside_intact(cb, c, "gemm_w4 out=")


# ------------------------------------------------------------------------------------------
# wgrad.hip: every split-K partial on its own
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_case(T, o, i):
    """dy [T, o], x [T, i]: integers in [-3, 3] (every partial sum is exact in fp32)."""
    case = GC.exact_operands(o, i, T, bk=GC.WGRAD_BK, integers=True)
    case.dy, case.x = case.a.t().contiguous(), case.b.t().contiguous()
    case.d = types.SimpleNamespace(dy=dev(case.dy), x=dev(case.x))
    return case


@functools.lru_cache(maxsize=None)
def wgrad_partials(T, o, i, splits):
    case = wgrad_case(T, o, i)
    return GC.partials(case.dy, case.x, GC.token_ranges(T, splits, GC.WGRAD_BK))


def wgrad_splits(T, o, i, splits):
    return int(_lib.lib().dtd_wgrad_tn_splits(o, i, T)) if splits is None else splits


@pytest.mark.parametrize("variant", GC.WGRAD_VARIANTS)
@pytest.mark.parametrize("T,o,i,splits", GC.WGRAD_CASES)
def test_wgrad_partials_exact(T, o, i, splits, variant):
    case = wgrad_case(T, o, i)
    assert G.wgrad_supported(case.d.dy, case.d.x)
    part = G.wgrad_tn(case.d.dy, case.d.x, splits, variant=variant)
    n = wgrad_splits(T, o, i, splits)
    assert part.shape == (n, o, i)
    ref = wgrad_partials(T, o, i, n)
    for r in range(n):
        GC.assert_equal(part[r], ref[r], f"partial {r} of {n}")


@pytest.mark.parametrize("acc", [False, True])
def test_wgrad_splitk_reduce_exact(acc):
    T, o, i, splits = 4128, 512, 256, 7
    case = wgrad_case(T, o, i)
    assert G.wgrad_supported(case.d.dy, case.d.x)
    part = G.wgrad_tn(case.d.dy, case.d.x, splits)
    dst0 = torch.randint(-50, 51, (o, i), generator=torch.Generator().manual_seed(3)).float()
    db, dst = guarded((o, i))
    dst.copy_(dev(dst0))
    splitk_reduce(part, dst, acc)
    GC.assert_equal(dst, wgrad_partials(T, o, i, splits).sum(0) + (O.f64(dst0) if acc else 0.0), f"acc={acc}")
    assert_guards_intact(db, dst, "splitk_reduce")


@pytest.mark.parametrize("variant", GC.WGRAD_VARIANTS)
def test_wgrad_strided_views_and_canaries(variant):
    T, o, i, splits = 160, 256, 256, 2
    case = wgrad_case(T, o, i)
    (_, dy), (_, x) = wider(case.dy, 8, 56), wider(case.x, 24, 8)
    assert G.wgrad_supported(dy, x) and dy.stride(0) > o and x.stride(0) > i
    pb, part = guarded((splits, o, i))
    _lib.call("dtd_wgrad_tn", variant, dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), part.data_ptr(), o, i,
              T, splits, _lib.stream())
    GC.assert_equal(part, wgrad_partials(T, o, i, splits), "strided partials")
    assert_guards_intact(pb, part, "wgrad partials")


def test_wgrad_rounded_gauss():
    """Per partial: 2 K 2^-24 |dy|^T |x| over the partial's own K tokens, plus the fp32 output's rounding."""
    T, o, i = 1024, 512, 256
    g = GC.rounded_operands("gauss", o, i, T)
    dy, x = g.a.t().contiguous(), g.b.t().contiguous()
    dyd, xd = dev(dy), dev(x)
    assert G.wgrad_supported(dyd, xd)
    part = G.wgrad_tn(dyd, xd)
    ranges = GC.token_ranges(T, part.shape[0], GC.WGRAD_BK)
    worst = 0.0
    for r, (lo, hi) in enumerate(ranges):
        sub = types.SimpleNamespace(a=dy[lo:hi].t(), b=x[lo:hi].t(), K=hi - lo)
        worst = max(worst, GC.check_rounded(part[r], sub, what=f"partial {r}")[0])
    print(f"\nwgrad_tn gauss T = {T}, {len(ranges)} partials: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------
# gemm_f32.hip
# ------------------------------------------------------------------------------------------
@pytest.fixture(params=["reg", "lds"])
def f32_form(request):
    """Every case runs on both hand-written forms (the register-direct and the LDS-staged kernel)."""
    prev = (G._F32[0], G._F32_WGRAD[0], G._F32_DG[0])
    G.set_f32(True)
    G.set_f32_kernel(request.param)
    try:
        yield request.param
    finally:
        G.set_f32_kernel("auto")
        G._F32[0], G._F32_WGRAD[0], G._F32_DG[0] = prev


@functools.lru_cache(maxsize=None)
def f32_case(shape):
    case = GC.exact_operands(*shape, bk=32, integers=True, dtype=F32)
    case.d = types.SimpleNamespace(**{k: dev(getattr(case, k)) for k in ("a", "b", "bias", "c0")})
    case.prod = GC.product(case)
    return case


@pytest.mark.parametrize("shape", GC.F32_SHAPES, ids=str)
def test_gemm_f32_nt_exact(f32_form, shape):
    case = f32_case(shape)
    assert G.f32_supported(*shape, case.d.a, case.d.b)
    GC.assert_equal(G.gemm_f32_nt(case.d.a, case.d.b, case.d.bias), case.prod + O.f64(case.bias), "nt bias")
    GC.assert_equal(G.gemm_f32_nt(case.d.a, case.d.b), case.prod, "nt")
    for bias in (None, case.d.bias):
        out = case.d.c0.clone()
        assert G.f32_supported(*shape, case.d.a, case.d.b, out)
        G.gemm_f32_nt(case.d.a, case.d.b, bias, out=out)
        GC.assert_equal(out, GC.product(case, bias is not None, True), "nt out=")


@pytest.mark.parametrize("shape", GC.F32_SHAPES, ids=str)
def test_gemm_f32_nn_exact(f32_form, shape):
    case = f32_case(shape)
    b_kn = case.d.b.t().contiguous()
    assert G.f32_supported(*shape, case.d.a, b_kn)
    GC.assert_equal(G.gemm_f32_nn(case.d.a, b_kn), case.prod, "nn")
    out = case.d.c0.clone()
    G.gemm_f32_nn(case.d.a, b_kn, out=out)
    GC.assert_equal(out, GC.product(case, c0=True), "nn out=")


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("shape", GC.F32_SHAPES, ids=str)
def test_gemm_f32_tn_partials_exact(f32_form, shape, splits):
    """a^T b per partial.  The register form splits K into even counts of 16-deep steps, the LDS form into
    32-deep steps."""
    M, N, K = shape
    case = f32_case(shape)
    a_km, b_kn = case.d.a.t().contiguous(), case.d.b.t().contiguous()
    assert G.f32_supported(M, N, K, a_km, b_kn, wgrad=True)
    part = G.gemm_f32_tn(a_km, b_kn, splits)
    ranges = GC.token_ranges(K, splits, 16, even=True) if f32_form == "reg" else GC.token_ranges(K, splits, 32)
    ref = GC.partials(case.a.t(), case.b.t(), ranges)
    assert part.shape == ref.shape
    for r in range(splits):
        GC.assert_equal(part[r], ref[r], f"partial {r} of {splits} ({f32_form} form, tokens {ranges[r]})")
