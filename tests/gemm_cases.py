"""Cases and checkers of the hand-written GEMM tests (``test_gemm_cases_cpu.py`` drives them with a CPU
stand-in and with mutants of it, ``test_gemm_numerics_gpu.py`` with the kernels of ``ops/csrc/gemm.hip``,
``gemm_w4.hip``, ``wgrad.hip`` and ``gemm_f32.hip``).  A plain helper module: no fixtures, and nothing from
the package but what ``tests/oracles.py`` brings.  Every reference is the fp64 product of the stored operands
(``oracles.f64``).

Two regimes, because a global relative norm on Gaussian data cannot see a few stale 16-byte chunks, two
wrong rows in one tile of hundreds, a truncating conversion or a low-precision accumulator:

* exact (``exact_operands``): operands built so that the true result -- and every partial sum on the way
  to it, in any order -- is exactly representable in the output type.  A in {-1, 0, +1} with the same
  number of non-zeros (at least one, at most 192 per row in all) in every K-step, B in {-1, 0, +1} / 16,
  bias and residual multiples of 1/16 within [-4, 4]: every output is a multiple of 1/16 of magnitude at
  most 16, exact in bf16 (16 |u| <= 256 fits the 8-bit significand) and in fp32.  The assertion is
  ``torch.equal``; one wrong element anywhere fails it.  For fp32 outputs the entries are integers in
  [-3, 3].  The transcendental epilogues are one bf16 rounding of an fp32 evaluation at an exactly known
  argument: ``assert_within_ulp``.

* rounded (``rounded_operands`` / ``check_rounded``): ordinary bf16 data, where exactness cannot see how
  the fp32 accumulator is kept and rounded.  Per element |got - ref| <= 2^-8 |ref| + 2 K 2^-24 (|A| |B|^T
  + |bias| + |c0|): bf16's unit roundoff, plus the recursive-summation bound K u sum |a||b| of fp32 (u =
  2^-24) doubled for an adder that truncates -- derived, not measured.  And the share of elements that
  differ from the correctly rounded fp64 result is at most 1e-2: a round-to-nearest conversion of an fp32
  accumulator misses the correct rounding only where the fp32 sum's error (~1e-7 relative) straddles a
  rounding boundary (measured with the stand-in: 1e-4 .. 2e-4 of the elements, 3e-3 in the cancel regime),
  truncation misses it for half of them, bf16 accumulators for 0.26 .. 0.98.
"""
import math
import types

import torch

from . import oracles as O

BF16, F32 = torch.bfloat16, torch.float32
TILE = 256                     # output tile of gemm.hip, gemm_w4.hip (2 x 2 waves of 128) and wgrad.hip
MAX_NNZ = 192                  # non-zeros per row of A: 192 / 16 + 4 = 16, the largest magnitude that is exact
U24 = 2.0 ** -24               # fp32 unit roundoff
MISROUND_CAP = 1e-2
ACT_FLOOR = 2e-6               # the project's fp32 activation bound (test_activation_fast_math_accuracy_fp32)
DBIAS_TOL = 2e-2               # check_activation's column-sum tolerance (tests/test_oracles_cpu.py)
CANARY = -12345.0              # exactly representable in bf16 and fp32


# shapes of the GPU file (M, N, K): one, two, an odd number of and many K-steps; 1, 6 and 12 tiles
GEMM_SHAPES = ((256, 256, 64), (256, 256, 128), (256, 512, 192), (512, 768, 320), (256, 256, 3072), (1024, 768, 64))
ROUNDED_SHAPES = ((512, 768, 768), (256, 256, 128))
W4_SHAPES = ((256, 256, 128), (256, 512, 192), (512, 768, 320))
SEAM_K, W4_SEAM_K = (64, 192), 128
# wgrad.hip (T, o, i, splits): a single K-step; ranges shorter than the ring and empty ranges; 3 + 2 steps
# around ring depths 4 and 5; uneven ranges; the library's own split count
WGRAD_CASES = ((32, 256, 256, 1), (96, 256, 512, 8), (160, 256, 256, 2), (4128, 512, 256, 7), (1024, 512, 256, None))
WGRAD_VARIANTS = (0, 4, 5, 44)
WGRAD_BK = 32
F32_SHAPES = ((128, 128, 32), (128, 128, 64), (256, 384, 96), (512, 768, 160))


def seam_shape(cus, K):
    """More tiles than CUs, so a persistent workgroup takes a second tile: 8 (cus // 8 + 1) tiles."""
    return TILE * (cus // 8 + 1), 2048, K


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tern(shape, g):
    return torch.randint(-1, 2, shape, generator=g).float()


def _sixteenths(shape, g, bound=4):
    """Multiples of 1/16 within [-bound, bound]."""
    return torch.randint(-16 * bound, 16 * bound + 1, shape, generator=g).float() / 16.0


# ------------------------------------------------------------------------------------------
# exact regime
# ------------------------------------------------------------------------------------------
def nnz_per_kstep(K, bk):
    nk = K // bk
    per = min(bk, MAX_NNZ // nk)
    assert K % bk == 0 and per >= 1, \
        f"K = {K}: {nk} K-steps of {bk} cannot each hold a non-zero within {MAX_NNZ} per row"
    return per


def exact_operands(M, N, K, bk=64, seed=0, integers=False, dtype=BF16):
    """CPU operands of C[M, N] = A[M, K] . B[N, K]^T whose result is exact (module docstring).

    Default: a (A), b (B), bias [N], c0 [M, N] (the residual of EPI_ADD), u [M, N] (a pre-activation for the
    backward epilogues: multiples of 1/16 within [-6, 6]), g [M, N] (a stored derivative in {0, +-1/2, +-1})
    and dst [N] fp32 (a column-sum destination: multiples of 1/32).  ``integers``: a, b, bias, c0 integers
    in [-3, 3] (fp32 outputs; a dense)."""
    gen = _gen(1000 * seed + 17)
    if integers:
        a = torch.randint(-3, 4, (M, K), generator=gen).float()
        b = torch.randint(-3, 4, (N, K), generator=gen).float()
        bias = torch.randint(-3, 4, (N,), generator=gen).float()
        c0 = torch.randint(-3, 4, (M, N), generator=gen).float()
        return types.SimpleNamespace(M=M, N=N, K=K, bk=bk, integers=True, a=a.to(dtype), b=b.to(dtype),
                                     bias=bias.to(dtype), c0=c0.to(dtype))
    per, nk = nnz_per_kstep(K, bk), K // bk
    # per non-zeros at random places of every K-step of every row, random signs
    place = torch.rand(M, nk, bk, generator=gen).argsort(-1) < per
    sign = torch.randint(0, 2, (M, nk, bk), generator=gen).float() * 2 - 1
    a = (place.float() * sign).view(M, K)
    b = _tern((N, K), gen) / 16.0
    halves = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0])
    case = types.SimpleNamespace(
        M=M, N=N, K=K, bk=bk, integers=False, a=a.to(dtype), b=b.to(dtype), bias=_sixteenths((N,), gen).to(dtype),
        c0=_sixteenths((M, N), gen).to(dtype), u=_sixteenths((M, N), gen, 6).to(dtype),
        g=halves[torch.randint(0, 5, (M, N), generator=gen)].to(dtype),
        dst=torch.randint(-64, 65, (N,), generator=gen).float() / 32.0)
    return case


def product(case, bias=False, c0=False):
    """fp64 A . B^T (+ bias) (+ c0)."""
    r = O.f64(case.a) @ O.f64(case.b).t()
    if bias:
        r = r + O.f64(case.bias)
    if c0:
        r = r + O.f64(case.c0)
    return r


def check_exact_invariants(case):
    """The builder's promises: value sets, non-zeros per K-step, and the reference (with bias, and with the
    residual) exactly representable and bounded."""
    a, b = O.f64(case.a), O.f64(case.b)
    M, N, K, bk = case.M, case.N, case.K, case.bk
    if case.integers:
        for t in (a, b, O.f64(case.bias), O.f64(case.c0)):
            assert bool((t == t.round()).all()) and float(t.abs().max()) <= 3
        r = product(case, True, True)
        assert float(r.abs().max()) <= 9 * K + 6 < 2 ** 24
        assert torch.equal(r.float().double(), r)
        return
    per = nnz_per_kstep(K, bk)
    assert bool(((a == 0) | (a.abs() == 1)).all())
    cnt = (a != 0).view(M, K // bk, bk).sum(-1)
    assert bool((cnt == per).all()) and 1 <= per and per * (K // bk) <= MAX_NNZ
    assert bool((((b * 16) == 0) | ((b * 16).abs() == 1)).all())
    for t, bound in ((case.bias, 4), (case.c0, 4), (case.u, 6)):
        t = O.f64(t)
        assert bool((t * 16 == (t * 16).round()).all()) and float(t.abs().max()) <= bound
    assert bool(torch.isin(O.f64(case.g), torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0], dtype=torch.float64)).all())
    assert bool((O.f64(case.dst) * 32 == (O.f64(case.dst) * 32).round()).all())
    for r in (product(case), product(case, bias=True), product(case, c0=True)):
        assert bool((r * 16 == (r * 16).round()).all()) and float(r.abs().max()) <= 16
        assert torch.equal(r.to(BF16).double(), r) and torch.equal(r.float().double(), r)
    assert float((product(case, bias=True) == 0).double().mean()) < 1e-2


def token_ranges(T, splits, bk, even=False):
    """[lo, hi) token ranges of the split-K partials: range r covers K-steps [r ks, (r + 1) ks) with ks =
    ceil(nk / splits) (``even``: rounded up to an even count, gemm_f32.hip's register form); ranges past the
    end are empty."""
    nk = T // bk
    ks = -(-nk // splits)
    if even:
        ks = (ks + 1) & ~1
    return [(min(r * ks, nk) * bk, min((r + 1) * ks, nk) * bk) for r in range(splits)]


def partials(a_t, b_t, ranges):
    """fp64 [len(ranges), o, i]: a_t[lo:hi]^T b_t[lo:hi] per range (zero for an empty one)."""
    a, b = O.f64(a_t), O.f64(b_t)
    return torch.stack([a[lo:hi].t() @ b[lo:hi] for lo, hi in ranges])


def assert_equal(got, ref64, what=""):
    """``torch.equal`` against the fp64 reference cast to got's dtype; the message names the first wrong
    element and counts them."""
    g = got.detach().cpu()
    r = ref64.to(g.dtype)
    assert torch.equal(r.double(), ref64), f"{what}: the reference is not representable in {g.dtype}"
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    if not torch.equal(g, r):
        bad = (g != r) | (torch.isnan(g) != torch.isnan(r))
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ, first at {first}: "
                             f"got {float(g[tuple(first)])}, reference {float(r[tuple(first)])}")


def bf16_ulp(ref64):
    """One bf16 ulp at the reference's magnitude: 2^-7 2^floor(log2 |ref|) (0 at 0)."""
    r = ref64.abs()
    e = torch.floor(torch.log2(torch.where(r > 0, r, torch.ones_like(r))))
    return torch.where(r > 0, torch.exp2(e - 7), torch.zeros_like(r))


def assert_within_ulp(got, ref64, what="", floor=ACT_FLOOR):
    """One bf16 rounding of an fp32 evaluation: |got - ref| <= one bf16 ulp of ref + ``floor`` (the fp32
    evaluation's own absolute bound, which is all that is left where ref underflows towards 0).  Returns the
    worst error in ulps over the elements whose ulp exceeds the floor."""
    g, r = O.f64(got), ref64
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), what
    err, ulp = (g - r).abs(), bf16_ulp(r)
    over = err > ulp + floor
    if bool(over.any()):
        i = tuple(int(v) for v in torch.unravel_index((err - ulp - floor).argmax(), err.shape))
        raise AssertionError(f"{what}: {int(over.sum())} elements beyond one bf16 ulp, worst at {list(i)}: "
                             f"got {float(g[i])!r}, reference {float(r[i])!r}, ulp {float(ulp[i]):.3e}")
    big = ulp > floor
    return float((err[big] / ulp[big]).max()) if bool(big.any()) else 0.0


def assert_colsum_close(got, summands64, what="", base=None):
    """Column sums of ``summands64`` (+ ``base``) to DBIAS_TOL of the column's own scale sum |summand|."""
    ref = summands64.sum(0) + (0.0 if base is None else O.f64(base))
    return O.assert_rows_close(got, ref, DBIAS_TOL, axis=None, scale=summands64.abs().sum(0), what=what)


# ------------------------------------------------------------------------------------------
# rounded regime
# ------------------------------------------------------------------------------------------
ROUNDED_REGIMES = ("gauss", "row_scales", "cancel")


def rounded_operands(regime, M, N, K, seed=0, dtype=BF16):
    """a [M, K], b [N, K], bias [N], c0 [M, N] in ``dtype``.  gauss: the existing tests' recipe (standard
    normal everything).  row_scales: row i of a and of c0 times 2^((i mod 13) - 6).  cancel: the second half
    of K repeats the first with b negated and off by 2^-6 of itself (rounded to ``dtype``: one to three ulps
    of every mirrored b, the last column included), so the product is about 5e-4 of sum |a||b| at K = 768
    (1.2e-3 at 128) and the accumulator ends near 0 after passing through partial sums of size sqrt(K / 2).  bias and c0 keep
    their unit scale: an accumulator that adds the K-steps in order carries an absolute error of about 2^-24
    sqrt(K / 2) per step, some 5e-6 at K = 768, and the misrounding share is a condition on the conversion
    only where that is small against the output's bf16 spacing (2^-8 at unit size: a share of a few 1e-3);
    on the bare product, 0.25 in size, a correct fp32 kernel may misround one element in a hundred.  The bare
    product is still held to the bound (``check_rounded(share=False)``)."""
    assert K % 2 == 0
    a = O.gauss(M, K, F32, 4 * seed + 1)
    b = O.gauss(N, K, F32, 4 * seed + 2)
    bias = O.gauss(1, N, F32, 4 * seed + 3)[0]
    c0 = O.gauss(M, N, F32, 4 * seed + 4)
    if regime == "row_scales":
        s = torch.exp2((torch.arange(M) % 13 - 6).float())[:, None]
        a, c0 = a * s, c0 * s
    elif regime == "cancel":
        a, b = a.to(dtype).float(), b.to(dtype).float()        # mirror the stored values
        a[:, K // 2:] = a[:, :K // 2]
        b[:, K // 2:] = -b[:, :K // 2] * (1 + 2.0 ** -6)
    else:
        assert regime == "gauss", regime
    return types.SimpleNamespace(M=M, N=N, K=K, a=a.to(dtype), b=b.to(dtype), bias=bias.to(dtype), c0=c0.to(dtype))


def rounded_bound(case, bias=False, c0=False, K=None, out_dtype=BF16):
    """(ref, bound) of the module docstring, fp64.  ``K``: the length of the reduction behind the output
    (default: the operands').  fp32 outputs: the summation term plus the output's own rounding 2^-24 |ref|."""
    ref = product(case, bias, c0)
    mag = O.f64(case.a).abs() @ O.f64(case.b).abs().t()
    if bias:
        mag = mag + O.f64(case.bias).abs()
    if c0:
        mag = mag + O.f64(case.c0).abs()
    k = case.K if K is None else K
    lead = 2.0 ** -8 if out_dtype == BF16 else U24
    return ref, lead * ref.abs() + 2.0 * k * U24 * mag


def check_rounded(got, case, bias=False, c0=False, K=None, what="", ref_bound=None, share=True):
    """Both assertions of the rounded regime on ``got`` (bf16: the bound and the misrounding share; fp32: the
    bound).  ``share=False``: the bound alone (the bare product of the cancel regime, see ``rounded_operands``).
    Returns (worst error / bound, share)."""
    g = got.detach().cpu()
    ref, bound = rounded_bound(case, bias, c0, K, g.dtype) if ref_bound is None else ref_bound
    assert g.shape == ref.shape and bool(torch.isfinite(g).all()), what
    ratio = (g.double() - ref).abs() / (bound + O.TINY)
    worst = int(ratio.argmax())
    val = float(ratio.flatten()[worst])
    assert val <= 1.0, (f"{what}: element {[int(v) for v in torch.unravel_index(torch.tensor(worst), ratio.shape)]} "
                        f"is {val:.3f} of its bound (got {float(g.flatten()[worst])!r}, "
                        f"reference {float(ref.flatten()[worst])!r})")
    frac = 0.0
    if g.dtype == BF16:
        frac = float((g != ref.to(BF16)).double().mean())
        assert not share or frac <= MISROUND_CAP, f"{what}: {frac:.3e} of the elements are not the correctly rounded result"
    return val, frac


# ------------------------------------------------------------------------------------------
# CPU stand-in of a kernel (fp32 accumulate, one rounding to the output type) and its mutants
# ------------------------------------------------------------------------------------------
def standin(case, bias=False, c0=False, out_dtype=BF16):
    acc = case.a.float() @ case.b.float().t()
    if bias:
        acc = acc + case.bias.float()
    if c0:
        acc = acc + case.c0.float()
    return acc.to(out_dtype)


def truncate_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits."""
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def standin_truncating(case, bias=False):
    acc = case.a.float() @ case.b.float().t()
    return truncate_bf16(acc + case.bias.float() if bias else acc)


def standin_bf16_accumulator(case, bias=False, bk=64):
    """The accumulator rounded to bf16 after every K-step."""
    acc = torch.zeros(case.M, case.N)
    for k in range(0, case.K, bk):
        acc = (acc + case.a[:, k:k + bk].float() @ case.b[:, k:k + bk].float().t()).to(BF16).float()
    return (acc + case.bias.float() if bias else acc).to(BF16)


def _tile(t, i, j):
    return t[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE]


def mutant_dropped_kstep(case, bias=False, bk=64):
    """The last tile misses its last K-step."""
    out = standin(case, bias)
    i, j = case.M // TILE - 1, case.N // TILE - 1
    a = case.a[i * TILE:(i + 1) * TILE, :case.K - bk].float()
    b = case.b[j * TILE:(j + 1) * TILE, :case.K - bk].float()
    acc = a @ b.t() if case.K > bk else torch.zeros(TILE, TILE)
    _tile(out, i, j).copy_((acc + case.bias[j * TILE:(j + 1) * TILE].float() if bias else acc).to(out.dtype))
    return out


def mutant_swapped_rows(out, r=37):
    out = out.clone()
    out[[r, r + 1]] = out[[r + 1, r]]
    return out


def mutant_swapped_chunk(out, r=101, c=24):
    """Two neighbouring 16-byte chunks (8 bf16 columns each) of one row change places."""
    out = out.clone()
    out[r, c:c + 16] = torch.cat([out[r, c + 8:c + 16], out[r, c:c + 8]])
    return out


def mutant_shifted_bias(case):
    """The last tile adds its bias 8 columns off."""
    out = standin(case, True)
    i, j = case.M // TILE - 1, case.N // TILE - 1
    acc = _tile(case.a.float() @ case.b.float().t(), i, j)
    _tile(out, i, j).copy_((acc + case.bias[j * TILE:(j + 1) * TILE].float().roll(8)).to(out.dtype))
    return out


def mutant_missing_bias_chunk(case):
    """8 columns of the last tile get no bias."""
    out = standin(case, True)
    i, j = case.M // TILE - 1, case.N // TILE - 1
    acc = case.a.float() @ case.b.float().t()
    rows, cols = slice(i * TILE, (i + 1) * TILE), slice(j * TILE + 40, j * TILE + 48)
    out[rows, cols] = acc[rows, cols].to(out.dtype)
    return out


def mutant_stale_segment(out, r=66):
    """Two rows x 256 columns of a tile keep the values of the tile before it (the previous tile row when
    there is only one tile column)."""
    out = out.clone()
    if out.shape[1] >= 2 * TILE:
        out[r:r + 2, TILE:2 * TILE] = out[r:r + 2, :TILE]
    else:
        assert out.shape[0] >= 2 * TILE
        out[TILE + r:TILE + r + 2, :TILE] = out[r:r + 2, :TILE]
    return out


def mutant_one_ulp(out, r=5, c=9):
    """One element one ulp (of the output type) up."""
    out = out.clone()
    v = float(out[r, c])
    if out.dtype == BF16:
        out[r, c] = v + float(bf16_ulp(torch.tensor(v if v != 0 else 2.0 ** -126, dtype=torch.float64)))
    else:
        out[r, c] = torch.nextafter(out[r, c], torch.tensor(math.inf))
    return out


def mutant_scaled(out):
    """Every output times 1 + 2^-7."""
    return (out.float() * (1 + 2.0 ** -7)).to(out.dtype)


def mutant_moved_split(a_t, b_t, ranges, bk):
    """Range 0 takes the first K-step of range 1: the partials' sum does not change."""
    (l0, h0), (l1, h1) = ranges[0], ranges[1]
    assert h0 == l1 and h1 - l1 >= bk
    moved = [(l0, h0 + bk), (l1 + bk, h1)] + list(ranges[2:])
    return partials(a_t, b_t, moved).float()


def mutant_dbias_missing_wave(du64, wave=3):
    """The column sums without the 32 rows one wave of the epilogue owns."""
    keep = torch.ones(du64.shape[0], dtype=torch.bool)
    keep[wave * 32:(wave + 1) * 32] = False
    return du64[keep].sum(0).float()


def rel(a, b):
    """The existing tests' metric: global relative Frobenius norm."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-12))
