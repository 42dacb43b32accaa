"""The MXFP4 skinny GEMM (``ops/csrc/gemm_skinny_mx4.hip``, ``ops.gemm.linear_skinny_mx4``): Y = X . deq(W)^T for
1 <= M <= 64 rows against the fp64 product of the stored operands, on guarded slices; x's rows from M on hold NaN.
Shapes: M on both sides of every bucket edge; one slab and one K-step, three of each, five K-steps; Llama-2's longest
reduction (22 chunks, the last with two K-steps); 8 CUs + 1 slabs, whose last workgroup has one live slab at every
slab count.  Exact regime: integer x in [-3, 3], weights a random e2m1 code times 2^(s - 4), s per block in -2 .. 2,
each block's first element 6 (the law then reproduces codes and scale bytes).  Every term is a multiple of 2^-7 and
|sum| <= 4.5 K < 2^17, so the fp32 sum is exact in any order: the output is the fp64 product rounded once to bf16.
Rounded regime: Gaussian x, weights of std 0.05 by the law, bound 2^-8 |ref| + 2 K 2^-24 |x| |W|^T (``gemm_cases``).
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import gemm as G
from distributed_training_and_deepspeed_amd.ops.quant import dequantize_weight_mx4, quantize_weight_mx4

from . import decode_cases as C
from . import gemm_cases as GC
from . import oracles as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _shapes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    small = [(M, N, K) for (N, K) in ((16, 128), (48, 384), (80, 640)) for M in (1, 7, 16, 17, 33, 64)]
    big = [(M, N, K) for (N, K) in ((64, 11008), (16 * (G.SKINNY_MX4_MAX_SLABS * cus + 1), 256)) for M in (7, 17, 64)]
    return small + big


def _run(x, codes, scales):
    M, K = x.shape
    N = codes.shape[0]
    nan_rows = torch.full((64, K), float("nan"), dtype=torch.bfloat16)
    nan_rows[:M] = x
    xb, xv = C.guarded((64, K), torch.bfloat16, nan_rows)
    cb, cv = C.guarded((N, K // 2), torch.uint8, codes)
    sb, sv = C.guarded((N, K // 32), torch.uint8, scales)
    yb, yv = C.guarded((M, N), torch.bfloat16)
    assert G.skinny_mx4_supported(M, N, K, xv[:M], cv, yv)
    G.linear_skinny_mx4(xv[:M], cv, sv, out=yv)
    first = yv.clone()
    G.linear_skinny_mx4(xv[:M], cv, sv, out=yv)
    torch.cuda.synchronize()
    assert torch.equal(C.bits(first), C.bits(yv)), "two calls differ"
    assert C.guards_intact(yb, M * N) and C.guards_intact(xb, 64 * K)
    assert C.guards_intact(cb, N * K // 2) and C.guards_intact(sb, N * K // 32)
    return yv.cpu()


@pytest.mark.parametrize("M,N,K", _shapes())
def test_exact(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randint(-3, 4, (M, K), generator=g).bfloat16()
    nib = torch.randint(0, 16, (N, K // 32, 32), generator=g)
    nib[:, :, 0] = 7
    exps = torch.randint(-2, 3, (N, K // 32), generator=g) - 4
    w = torch.ldexp(torch.where(nib >= 8, -GRID[nib & 7], GRID[nib & 7]), exps[:, :, None]).view(N, K)
    codes, scales = quantize_weight_mx4(w)
    flat = nib.view(N, K // 2, 2)
    assert torch.equal(codes, (flat[..., 0] | (flat[..., 1] << 4)).to(torch.uint8))
    assert torch.equal(scales, (exps + 127).to(torch.uint8))
    ref = O.f64(x) @ O.f64(w).t()
    got = _run(x, codes, scales)
    assert torch.equal(got, ref.float().bfloat16())        # (ref is exact in fp32: this is one rounding)


@pytest.mark.parametrize("M,N,K", _shapes())
def test_rounded(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    codes, scales = quantize_weight_mx4(torch.randn(N, K, generator=g) * 0.05)
    w64 = dequantize_weight_mx4(codes, scales, torch.float64)
    ref = O.f64(x) @ w64.t()
    bound = 2.0 ** -8 * ref.abs() + 2.0 * K * 2.0 ** -24 * (O.f64(x).abs() @ w64.abs().t())
    GC.check_rounded(_run(x, codes, scales), None, what=f"mx4 {M}x{N}x{K}", ref_bound=(ref, bound))


def test_unsupported_shapes():
    x = torch.randn(8, 256, device=DEV).bfloat16()
    codes = torch.zeros(32, 128, dtype=torch.uint8, device=DEV)
    scales = torch.full((32, 8), 127, dtype=torch.uint8, device=DEV)
    assert G.skinny_mx4_supported(8, 32, 256, x, codes)
    assert not G.skinny_mx4_supported(8, 32, 192, x[:, :192], codes[:, :96])
    assert not G.skinny_mx4_supported(8, 24, 256, x, codes[:24])
    assert not G.skinny_mx4_supported(65, 32, 256, x, codes)
    assert not bool(G.linear_skinny_mx4(x, codes, scales).any())
    for bad in ((x, codes[:24], scales[:24]), (x[:, :192], codes[:, :96], scales[:, :6]), (x.float(), codes, scales),
                (x, codes.view(torch.int8), scales), (x, codes, scales.float()), (x, codes, scales.t().contiguous().t()),
                (x, codes, scales[:, :4])):
        with pytest.raises(ValueError):
            G.linear_skinny_mx4(*bad)
