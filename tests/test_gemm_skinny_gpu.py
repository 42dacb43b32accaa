"""The skinny GEMM (``ops/csrc/gemm_skinny.hip``, ``ops.gemm.linear_skinny``): Y = X . W^T for 1 <= M <= 64 rows,
bf16 weights or FP8 codes with one scale per output row, against the fp64 product of the stored operands.

Shapes: M on both sides of every bucket edge (16 / 32 / 64 columns); (N, K) with one slab and one K-step,
three of each, five K-steps (uneven over the four waves: one wave gets two), Llama-2's longest reduction, and
-- the workgroups carry 2 or 4 slabs once every CU has one -- two shapes with 2 CUs + 1 and 4 CUs + 1 slabs,
whose last workgroup has a single live slab.

Exact regime (``gemm_cases.exact_operands``): every sum is exact in fp32, so the result is the reference bit
for bit; the weights 0, +-1/16 are FP8 codes exactly (the law gives them the scale 2^-12).  Rounded regime:
Gaussian x, weights of std 0.05, bound 2^-8 |ref| + 2 K 2^-24 |x| |W|^T (``gemm_cases``' derived bound; W
the dequantised weight).  The FP8 scales there are positive, not powers of two and distinct per row.

Every operand is a guarded slice whose guards must be intact; x's rows at and above M hold NaN.
"""
import pytest
import torch
import torch.nn.functional as F

from distributed_training_and_deepspeed_amd.ops import gemm as G
from distributed_training_and_deepspeed_amd.ops.quant import quantize_weight_fp8

from . import decode_cases as C
from . import gemm_cases as GC
from . import oracles as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (1, 7, 16, 17, 33, 64)


def _shapes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    small = [(M, N, K) for (N, K) in ((16, 128), (48, 384), (80, 640)) for M in MS]
    big = [(M, N, K) for (N, K) in ((64, 11008), (16 * (2 * cus + 1), 256), (16 * (4 * cus + 1), 128))
           for M in (7, 17, 64)]
    return small + big


def _run(x, w, scale):
    """linear_skinny on guarded copies of x [M, K] (bf16), w (bf16 values, or FP8 codes with ``scale``): the
    result on the CPU, after checking the guards and that a second call is bitwise equal."""
    M, K = x.shape
    N = w.shape[0]
    nan_rows = torch.full((64, K), float("nan"), dtype=torch.bfloat16)
    nan_rows[:M] = x
    xb, xv = C.guarded((64, K), torch.bfloat16, nan_rows)
    if scale is None:
        wb, wv = C.guarded((N, K), torch.bfloat16, w)
        sb = sv = None
    else:
        wb, wv = C.guarded((N, K), torch.uint8, w.view(torch.uint8))
        wv = wv.view(torch.float8_e4m3fn)
        sb, sv = C.guarded((N,), torch.float32, scale)
    yb, yv = C.guarded((M, N), torch.bfloat16)
    assert G.skinny_supported(M, N, K, xv[:M], wv, yv)
    G.linear_skinny(xv[:M], wv, sv, out=yv)
    first = yv.clone()
    G.linear_skinny(xv[:M], wv, sv, out=yv)
    torch.cuda.synchronize()
    assert torch.equal(C.bits(first), C.bits(yv)), "two calls differ"
    assert C.guards_intact(yb, M * N) and C.guards_intact(xb, 64 * K) and C.guards_intact(wb, N * K)
    assert sb is None or C.guards_intact(sb, N)
    return yv.cpu()


@pytest.mark.parametrize("fmt", ("bf16", "fp8"))
@pytest.mark.parametrize("M,N,K", _shapes())
def test_exact(fmt, M, N, K):
    case = GC.exact_operands(M, N, K, bk=128)
    if fmt == "fp8":
        codes, scale = quantize_weight_fp8(case.b)
        assert torch.equal(codes.float() * scale[:, None], case.b.float())
        got = _run(case.a, codes, scale)
    else:
        got = _run(case.a, case.b, None)
    GC.assert_equal(got, GC.product(case), f"{fmt} {M}x{N}x{K}")


@pytest.mark.parametrize("fmt", ("bf16", "fp8"))
@pytest.mark.parametrize("M,N,K", _shapes())
def test_rounded(fmt, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = torch.randn(N, K, generator=g) * 0.05
    if fmt == "fp8":
        codes, s = quantize_weight_fp8(w)
        scale = s * (1.0 + (torch.arange(N) + 1.0) / (N + 3.0))       # in (s, 2 s): no power of two, all distinct
        got = _run(x, codes, scale)
        w64 = codes.double() * scale.double()[:, None]
    else:
        w = w.bfloat16()
        got = _run(x, w, None)
        w64 = O.f64(w)
    ref = O.f64(x) @ w64.t()
    bound = 2.0 ** -8 * ref.abs() + 2.0 * K * 2.0 ** -24 * (O.f64(x).abs() @ w64.abs().t())
    val, frac = GC.check_rounded(got, None, what=f"{fmt} {M}x{N}x{K}", ref_bound=(ref, bound))
    print(f"{fmt} {M}x{N}x{K}: worst error {val:.3f} of the bound, misrounded share {frac:.2e}")


def test_unsupported_shapes_and_the_switch():
    x = torch.randn(8, 256, device=DEV).bfloat16()
    w = torch.randn(32, 256, device=DEV).bfloat16()
    assert G.skinny_supported(8, 32, 256, x, w)
    assert not G.skinny_supported(8, 32, 192, x[:, :192], w[:, :192])
    assert not G.skinny_supported(8, 24, 256, x, w[:24])
    assert not G.skinny_supported(65, 32, 256, x, w)
    with pytest.raises(ValueError):
        G.linear_skinny(x, w[:24])
    assert not G.skinny_enabled()                 # off by default: linear_any is the library's product
    assert torch.equal(C.bits(G.linear_any(x, w)), C.bits(F.linear(x, w)))
    G.set_skinny(True)
    try:
        assert torch.equal(C.bits(G.linear_any(x, w)), C.bits(G.linear_skinny(x, w)))
    finally:
        G.set_skinny(False)
