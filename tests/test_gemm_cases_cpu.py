"""Self-test of ``tests/gemm_cases.py`` without a GPU: a CPU stand-in of the kernels (fp32 matmul, one
rounding to the output type) passes every check in every regime, every mutant of it is rejected by at least
one checker, and the exact builder keeps its promises at every shape the GPU file uses.

``test_old_metric_on_mutants`` records what the existing GPU tests' global relative norm makes of the same
mutants at their own recipe (Gaussian bf16 operands, M, N, K = 4096, 3072, 768, bound 1e-2).  Measured:

    stand-in 1.66e-3 | two swapped 16-byte chunks 2.44e-3 | stale 2 x 256 segment 8.57e-3 | truncation 3.31e-3 |
    bf16 accumulators 4.53e-3 | bias missing on 8 columns of a tile 1.71e-3 | bias shifted by 8 columns in a
    tile 3.95e-3 | one element one ulp off 1.66e-3 | every output times 1 + 2^-7 7.85e-3

-- all accepted; it rejects two whole swapped rows (3.08e-2) and a K-step dropped from a whole tile (2.07e-2).
A split-K boundary moved by one K-step leaves the sum of the partials, which is all the wgrad tests compare,
unchanged (3.7e-8).  The stand-in against the rounded regime's checks (worst error / bound, misrounded share)
at (512, 768, 768): gauss 0.84, 1.8e-4; row_scales 0.89, 1.3e-4; cancel 0.25, 3.0e-3; at (256, 256, 128):
0.97, 1.1e-4; 0.98, 1.1e-4; 0.87, 5.0e-4.  Truncation misrounds 0.50 of the elements at every K, bf16
accumulators 0.26 (K = 128) and 0.59 (K = 768), 0.98 in the cancel regime.
"""
import functools

import pytest
import torch

from . import gemm_cases as GC
from . import oracles as O

BF16, F32 = torch.bfloat16, torch.float32
EXACT_AT = (512, 768, 320)
ROUNDED_AT = (512, 768, 768)


@functools.lru_cache(maxsize=None)
def exact_case(shape=EXACT_AT, bk=64):
    return GC.exact_operands(*shape, bk=bk)


@functools.lru_cache(maxsize=None)
def rounded_case(regime="gauss", shape=ROUNDED_AT):
    return GC.rounded_operands(regime, *shape)


def rejected(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------
# the builder
# ------------------------------------------------------------------------------------------
ALL_SHAPES = (GC.GEMM_SHAPES + GC.ROUNDED_SHAPES + GC.W4_SHAPES + tuple(GC.seam_shape(256, k) for k in GC.SEAM_K)
              + (GC.seam_shape(256, GC.W4_SEAM_K), GC.seam_shape(304, 64)))


@pytest.mark.parametrize("shape", sorted(set(ALL_SHAPES)), ids=str)
def test_exact_builder_invariants(shape):
    GC.check_exact_invariants(GC.exact_operands(*shape))


@pytest.mark.parametrize("T,o,i,splits", GC.WGRAD_CASES)
def test_exact_builder_invariants_wgrad(T, o, i, splits):
    """dy^T x: the operands are [T, o] and [T, i], so the 'A' of the builder is dy^T."""
    case = GC.exact_operands(o, i, T, bk=GC.WGRAD_BK, integers=True)
    GC.check_exact_invariants(case)
    ranges = GC.token_ranges(T, splits or 5, GC.WGRAD_BK)
    part = GC.partials(case.a.t(), case.b.t(), ranges)
    assert torch.equal(part.sum(0), GC.product(case)) and float(part.abs().max()) < 2 ** 24
    assert all(hi - lo == 0 or (hi - lo) % GC.WGRAD_BK == 0 for lo, hi in ranges) and ranges[-1][1] == T
    if (T, splits) == (96, 8):
        assert [hi - lo for lo, hi in ranges] == [32, 32, 32, 0, 0, 0, 0, 0] and not bool(part[3:].any())
    if (T, splits) == (160, 2):
        assert ranges == [(0, 96), (96, 160)]


@pytest.mark.parametrize("shape", GC.F32_SHAPES, ids=str)
def test_exact_builder_invariants_f32(shape):
    GC.check_exact_invariants(GC.exact_operands(*shape, bk=32, integers=True, dtype=F32))
    K = shape[2]
    assert GC.token_ranges(K, 3, 32)[-1][1] == K and GC.token_ranges(K, 3, 16, even=True)[-1][1] == K


def test_builder_refuses_too_many_ksteps():
    with pytest.raises(AssertionError):
        GC.exact_operands(256, 256, 64 * 193)


# ------------------------------------------------------------------------------------------
# the stand-in passes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GC.GEMM_SHAPES, ids=str)
def test_standin_passes_exact(shape):
    case = exact_case(shape)
    for bias in (False, True):
        GC.assert_equal(GC.standin(case, bias), GC.product(case, bias), "store")
    GC.assert_equal(GC.standin(case, c0=True), GC.product(case, c0=True), "add")
    da = GC.product(case)
    du = (GC.standin(case).float() * case.g.float())
    GC.assert_equal(du.to(BF16), da * O.f64(case.g), "mul_bwd du")
    GC.assert_equal(du.sum(0) + case.dst, (da * O.f64(case.g)).sum(0) + O.f64(case.dst), "mul_bwd dbias")


def test_standin_passes_exact_fp32_outputs():
    T, o, i = 160, 256, 256
    case = GC.exact_operands(o, i, T, bk=32, integers=True)
    ranges = GC.token_ranges(T, 2, 32)
    got = torch.stack([case.a.t()[lo:hi].float().t() @ case.b.t()[lo:hi].float() for lo, hi in ranges])
    GC.assert_equal(got, GC.partials(case.a.t(), case.b.t(), ranges), "partials")
    c32 = GC.exact_operands(256, 384, 96, bk=32, integers=True, dtype=F32)
    GC.assert_equal(GC.standin(c32, True, True, F32), GC.product(c32, True, True), "fp32 nt")


@pytest.mark.parametrize("shape", GC.ROUNDED_SHAPES, ids=str)
@pytest.mark.parametrize("regime", GC.ROUNDED_REGIMES)
def test_standin_passes_rounded(regime, shape):
    case = rounded_case(regime, shape)
    w, s = GC.check_rounded(GC.standin(case, bias=True), case, bias=True, what="store")
    print(f"\nstand-in {regime} {shape}: worst error / bound {w:.2f}, misrounded share {s:.1e}")
    GC.check_rounded(GC.standin(case, c0=True), case, c0=True, what="add")
    GC.check_rounded(GC.standin(case, out_dtype=F32), case, what="fp32 output")
    if regime == "cancel":
        ref = GC.product(case)
        mag = O.f64(case.a).abs() @ O.f64(case.b).abs().t()
        assert float(ref.abs().mean() / mag.mean()) < 2e-3          # the product really cancels (1.2e-3 at K = 128)
        GC.check_rounded(GC.standin(case), case, what="bare product", share=False)


@pytest.mark.parametrize("act", ["gelu", "gelu_tanh"])
def test_standin_activation_within_one_ulp(act):
    """fp32 torch activations of the exact grid (every multiple of 1/16 in [-16, 16], shuffled per row),
    rounded once; the upstream gradient in {0, +-1/2, +-1}, so that du carries the activation's own bound."""
    g = torch.Generator().manual_seed(5)
    grid = torch.arange(-256, 257).float() / 16
    u = torch.stack([grid[torch.randperm(513, generator=g)] for _ in range(64)]).to(BF16)
    dy = GC.exact_operands(256, 768, 64).g[:64, :513]
    ref = O.activation(u, act, dy=dy)
    ul = u.float().requires_grad_(True)
    a = torch.nn.functional.gelu(ul, approximate="tanh" if act == "gelu_tanh" else "none")
    (du,) = torch.autograd.grad((a * dy.float()).sum(), ul)
    worst = GC.assert_within_ulp(a.detach().to(BF16), ref["a"], "a")
    assert 0 < worst <= 1.0
    GC.assert_within_ulp(du.to(BF16), ref["du"], "du")
    assert rejected(GC.assert_within_ulp, GC.mutant_one_ulp(GC.mutant_one_ulp(a.detach().to(BF16), 1, 300), 1, 300),
                    ref["a"])
    GC.assert_colsum_close(du.sum(0), ref["du"], "dbias")


# ------------------------------------------------------------------------------------------
# every mutant is rejected
# ------------------------------------------------------------------------------------------
def _output_mutants(case, bias=True):
    """name -> mutated stand-in output of ``case`` (store with bias)."""
    out = GC.standin(case, bias)
    return {
        "dropped_kstep": GC.mutant_dropped_kstep(case, bias),
        "swapped_rows": GC.mutant_swapped_rows(out),
        "swapped_chunk": GC.mutant_swapped_chunk(out),
        "shifted_bias": GC.mutant_shifted_bias(case),
        "missing_bias_chunk": GC.mutant_missing_bias_chunk(case),
        "stale_segment": GC.mutant_stale_segment(out),
        "one_ulp": GC.mutant_one_ulp(out),
        "scaled": GC.mutant_scaled(out),
        "truncation": GC.standin_truncating(case, bias),
        "bf16_accumulator": GC.standin_bf16_accumulator(case, bias),
    }


LAYOUT_MUTANTS = ("dropped_kstep", "swapped_rows", "swapped_chunk", "shifted_bias", "missing_bias_chunk",
                  "stale_segment", "one_ulp", "scaled")
ROUNDING_MUTANTS = ("truncation", "bf16_accumulator")


@pytest.mark.parametrize("shape", [EXACT_AT, (256, 512, 192), (1024, 768, 64)], ids=str)
def test_exact_regime_rejects_layout_mutants(shape):
    """... and cannot see the two rounding mutants: every value on the way is exact in bf16."""
    case = exact_case(shape)
    ref = GC.product(case, True)
    muts = _output_mutants(case)
    for name in LAYOUT_MUTANTS:
        assert rejected(GC.assert_equal, muts[name], ref, name), name
    for name in ROUNDING_MUTANTS:
        GC.assert_equal(muts[name], ref, name)


@pytest.mark.parametrize("regime", GC.ROUNDED_REGIMES)
def test_rounded_regime_rejects_rounding_mutants(regime):
    case = rounded_case(regime)
    muts = _output_mutants(case)
    rb = GC.rounded_bound(case, bias=True)
    for name in ROUNDING_MUTANTS + ("scaled", "dropped_kstep", "stale_segment"):
        assert rejected(GC.check_rounded, muts[name], case, bias=True, ref_bound=rb), (regime, name)
    for K in (128, 768):
        c = GC.rounded_operands(regime, 256, 256, K, seed=3)
        ref = GC.product(c).to(BF16)
        t = float((GC.standin_truncating(c) != ref).double().mean())
        b = float((GC.standin_bf16_accumulator(c) != ref).double().mean())
        print(f"\n{regime} K = {K}: misrounded share truncation {t:.2f}, bf16 accumulators {b:.2f}")
        assert t > 0.3 and b > 0.1


def test_every_listed_mutant_is_rejected_by_a_checker():
    exact, rnd = exact_case(), rounded_case()
    me, mr = _output_mutants(exact), _output_mutants(rnd)
    ref, rb = GC.product(exact, True), GC.rounded_bound(rnd, bias=True)
    for name in me:
        assert (rejected(GC.assert_equal, me[name], ref, name)
                or rejected(GC.check_rounded, mr[name], rnd, bias=True, ref_bound=rb)), name


def test_moved_split_boundary_is_rejected_per_partial_only():
    T, o, i = 160, 256, 256
    case = GC.exact_operands(o, i, T, bk=32, integers=True)
    dy, x = case.a.t(), case.b.t()
    ranges = GC.token_ranges(T, 2, 32)
    ref = GC.partials(dy, x, ranges)
    mut = GC.mutant_moved_split(dy, x, ranges, 32)
    assert torch.equal(mut.sum(0).double(), ref.sum(0))             # what the existing tests compare
    assert rejected(GC.assert_equal, mut, ref)
    g = GC.rounded_operands("gauss", o, i, T)
    gr = GC.token_ranges(T, 2, 32)
    mutg = GC.mutant_moved_split(g.a.t(), g.b.t(), gr, 32)
    refg = GC.partials(g.a.t(), g.b.t(), gr)
    print(f"\nmoved split boundary: rel of the sum {GC.rel(mutg.sum(0), refg.sum(0)):.1e}")
    assert GC.rel(mutg.sum(0), refg.sum(0)) < 2e-3


def test_dbias_missing_a_wave_is_rejected():
    case = exact_case()
    du = GC.product(case) * O.f64(case.g)
    ref = du.sum(0)
    GC.assert_equal(du.sum(0).float(), ref, "dbias")
    mut = GC.mutant_dbias_missing_wave(du)
    assert rejected(GC.assert_equal, mut, ref)
    # the transcendental epilogues' column check sees it too: 32 of 512 rows are 6 % of a column's scale
    assert rejected(GC.assert_colsum_close, mut, du)
    print(f"\ndbias without one wave's rows: rel {GC.rel(mut, ref):.1e} (the existing bound is 2e-2)")


# ------------------------------------------------------------------------------------------
# what the old metric made of them
# ------------------------------------------------------------------------------------------
OLD_REL = {}


def test_old_metric_on_mutants():
    M, N, K = 4096, 3072, 768
    g = torch.Generator().manual_seed(0)
    case = GC.rounded_operands("gauss", M, N, K)
    case.a, case.b, case.bias = (torch.randn(s, generator=g).to(BF16) for s in ((M, K), (N, K), (N,)))
    ref = case.a.float() @ case.b.float().t() + case.bias.float()      # the existing tests' reference
    OLD_REL["stand-in"] = GC.rel(GC.standin(case, True), ref)
    for name, out in _output_mutants(case).items():
        OLD_REL[name] = GC.rel(out, ref)
    print("\nold metric (rel < 1e-2 passes): " + " | ".join(f"{k} {v:.2e}" for k, v in OLD_REL.items()))
    for name in ("swapped_chunk", "stale_segment", "truncation", "bf16_accumulator"):
        assert OLD_REL[name] < 1e-2, (name, OLD_REL[name])
