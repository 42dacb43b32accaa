"""The FP8 x FP8 GEMM and the activation quantiser (``ops/csrc/gemm_fp8.hip``; ``ops.gemm.linear_fp8``,
``ops.functional.act_quant_fp8``).

Quantiser: codes and scales bit for bit the law's (``ops.quant.quantize_act_fp8``), the hand-made rows of
``test_quant_act_cpu.py`` included.

GEMM: every tile of the kernel (``ops.gemm.fp8_tile_ms()``, forced) at M = 1, 64, 65 and one below, at and above its own
M edge; N of one 16-column slab, one full tile plus a slab, and 16 (2 CUs + 1); K of one MFMA, 3 and 5 K-steps (odd
against the ring of 3) and Llama-2's 11008 (at the smallest M and N); and two shapes on the tile the shape picks itself.
Exact regime: codes in {0, +-1, +-2} (at most 128 non-zeros a row, some in every K-step) times {0, +-1/16}, scales 1:
every sum is a multiple of 1/16 of magnitude at most 16, exact in fp32 and in bf16 -- the result is the fp64 product bit
for bit.  Rounded regime: random codes, scales positive, distinct and no powers of two; the bound of ``gemm_cases``,
2^-8 |ref| + 2 K 2^-24 sx sw |xc| |wc|^T, against the fp64 product of the dequantised operands.

Every operand is a guarded slice whose guards must be intact; x's rows at and above M hold NaN codes.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops import gemm as G
from distributed_training_and_deepspeed_amd.ops.quant import quantize_act_fp8

from . import decode_cases as C
from . import gemm_cases as GC
from .test_quant_act_cpu import hand_rows

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
TILES = (64, 128, 256)            # checked against the kernel's getter in test_unsupported


def _shapes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    out = []
    for T in TILES:
        n1 = (64 if T == 64 else 128) + 16
        out += [(T, M, n1, 384) for M in sorted({1, 64, 65, T - 1, T, T + 1})]
        out += [(T, T + 1, n1, K) for K in (128, 640)] + [(T, 1, 16, 11008)]
        out += [(T, 65, N, 128) for N in (16, 16 * (2 * cus + 1))]
    return out + [(0, 96, 144, 384), (0, 300, 16 * (2 * cus + 1), 128)]


@pytest.mark.parametrize("M", (1, 65, 130))
@pytest.mark.parametrize("K", (128, 384, 11008))
def test_quantiser(M, K):
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)) * torch.logspace(-6, 6, M, base=2.0)[:, None]
    x = x.bfloat16()
    x[:min(M, 4)] = hand_rows(K)[:min(M, 4)]
    poisoned = torch.full((M + 3, K), float("nan"), dtype=torch.bfloat16)
    poisoned[:M] = x
    xb, xv = C.guarded((M + 3, K), torch.bfloat16, poisoned)
    cb, cv = C.guarded((M + 3, K), torch.uint8)
    sb, sv = C.guarded((M + 3,), torch.float32)
    Fx.act_quant_fp8(xv[:M], cv[:M].view(F8), sv[:M])
    torch.cuda.synchronize()
    codes, scale = quantize_act_fp8(x)
    assert torch.equal(sv[:M].cpu(), scale)
    assert torch.equal(cv[:M].cpu(), codes.view(torch.uint8))
    assert bool((cv[M:] == C.SENT_CODE).all()) and bool((sv[M:] == C.SENT).all())       # rows at and above M
    assert C.guards_intact(xb, (M + 3) * K) and C.guards_intact(cb, (M + 3) * K) and C.guards_intact(sb, M + 3)


def _run(tile, xc, sx, wc, sw):
    """linear_fp8 on guarded copies (codes as CPU float8 tensors): the result on the CPU, after checking the guards and
    that a second call is bitwise equal."""
    M, K = xc.shape
    N = wc.shape[0]
    rows = torch.full((M + 2, K), 0x7F, dtype=torch.uint8)              # 0x7f: e4m3fn's NaN
    rows[:M] = xc.view(torch.uint8)
    xb, xv = C.guarded((M + 2, K), torch.uint8, rows)
    wb, wv = C.guarded((N, K), torch.uint8, wc.view(torch.uint8))
    sxb, sxv = C.guarded((M,), torch.float32, sx)
    swb, swv = C.guarded((N,), torch.float32, sw)
    yb, yv = C.guarded((M, N), torch.bfloat16)
    xq, wq = xv[:M].view(F8), wv.view(F8)
    assert G.fp8_supported(M, N, K, xq, wq, yv)
    G.linear_fp8(xq, sxv, wq, swv, out=yv, tile=tile)
    first = yv.clone()
    G.linear_fp8(xq, sxv, wq, swv, out=yv, tile=tile)
    torch.cuda.synchronize()
    assert torch.equal(C.bits(first), C.bits(yv)), "two calls differ"
    assert C.guards_intact(yb, M * N) and C.guards_intact(xb, (M + 2) * K) and C.guards_intact(wb, N * K)
    assert C.guards_intact(sxb, M) and C.guards_intact(swb, N)
    return yv.cpu()


@pytest.mark.parametrize("tile,M,N,K", _shapes())
def test_exact(tile, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    nk = K // 128
    place = torch.rand(M, nk, 128, generator=g).argsort(-1) < max(1, 128 // nk)
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (M, nk, 128), generator=g)]
    x = (place * vals).view(M, K)
    w = torch.randint(-1, 2, (N, K), generator=g).float() / 16.0
    got = _run(tile, x.to(F8), torch.ones(M), w.to(F8), torch.ones(N))
    GC.assert_equal(got, x.double() @ w.double().t(), f"tile {tile} {M}x{N}x{K}")


@pytest.mark.parametrize("tile,M,N,K", _shapes())
def test_rounded(tile, M, N, K):
    g = torch.Generator().manual_seed(M + N + K + 1)
    xc = (torch.randn(M, K, generator=g) * 40.0).to(F8)
    wc = (torch.randn(N, K, generator=g) * 10.0).to(F8)
    sx = 2.0 ** -6 * (1.0 + (torch.arange(M) + 1.0) / (M + 3.0))       # in (s, 2 s): no power of two, all distinct
    sw = 2.0 ** -9 * (1.0 + (torch.arange(N) + 1.0) / (N + 3.0))
    got = _run(tile, xc, sx, wc, sw)
    x64, w64 = xc.double() * sx.double()[:, None], wc.double() * sw.double()[:, None]
    ref = x64 @ w64.t()
    bound = 2.0 ** -8 * ref.abs() + 2.0 * K * 2.0 ** -24 * (x64.abs() @ w64.abs().t())
    val, frac = GC.check_rounded(got, None, what=f"tile {tile} {M}x{N}x{K}", ref_bound=(ref, bound), share=False)
    print(f"tile {tile} {M}x{N}x{K}: worst error {val:.3f} of the bound, misrounded share {frac:.2e}")


def test_unsupported():
    assert G.fp8_tile_ms() == TILES
    xc = torch.zeros(80, 256, device="cuda").to(F8)
    wc = torch.zeros(32, 256, device="cuda").to(F8)
    sx, sw = torch.ones(80, device="cuda"), torch.ones(32, device="cuda")
    assert G.fp8_supported(80, 32, 256, xc, wc)
    assert not G.fp8_supported(80, 24, 256, xc, wc[:24])
    assert not G.fp8_supported(80, 32, 192, xc[:, :192], wc[:, :192])
    for bad in ((xc, sx, wc[:24], sw[:24]), (xc.bfloat16(), sx, wc, sw), (xc, sx[:8], wc, sw)):
        with pytest.raises(ValueError):
            G.linear_fp8(*bad)
    with pytest.raises(ValueError):
        Fx.act_quant_fp8(torch.zeros(8, 192, device="cuda", dtype=torch.bfloat16))
