"""The streaming HIP kernels -- LayerNorm, RMSNorm, row softmax, cross-entropy, activations, SwiGLU,
RoPE, dropout-add, fused Adam, sq-norm, scale-cast -- against the fp64 oracles of ``tests/oracles.py``
with the per-slice metric, on the hard input regimes, at the smallest shapes that reach each code path.

The ``check_*`` functions, tolerances and regimes are those of ``tests/test_oracles_cpu.py`` (which
holds the CPU branches to a quarter of the same tolerances, and explains the regimes that had to be
made milder); here they run on the device.  What the first run of this file found:

  * ``xent_fwd_kernel`` gave a NaN loss and ``softmax_fwd_kernel``'s wide-row path NaN rows whenever a
    thread / lane met a -inf input before its first finite one (exp(-inf - -inf)).  Both running
    maxima now start at -FLT_MAX; ``test_finite_inputs_bitwise_as_before_the_inf_fix`` pins the
    finite-input results to the values the kernels gave before.
  * The GELU-tanh derivative was NaN for |x| >~ 1.8e19 (x^2 overflowed: 0 * inf), in the kernel and
    the CPU branch alike; both now cap x^2 at 1e30 and the ``saturated`` regime's 1e30 passes.  In fp32
    its du differs in the last bits between act_bwd with and without the fused recompute (the two
    forms contract their multiply-adds differently); the bitwise assertion stays where
    test_kernels_gpu.py has it, on bf16.
  * The block-form LayerNorm forward (h > 2048 or not a wave width) normalises its stored, rounded z,
    the wave kernels the fp32 sum: at mean / std = 35 in bf16 the two differ by 3.4e-2 of the row's
    largest element.  A limit of the stored z, which every backward reads anyway; the ``offset``
    regime therefore runs without a branch input (test_oracles_cpu.py has the numbers).
  * The memory-efficient LayerNorm backward: see ``test_layernorm_bwd_from_output``.
"""
import hashlib

import pytest
import torch

from distributed_training_and_deepspeed_amd.ops import _lib
from distributed_training_and_deepspeed_amd.ops import functional as Fx

from . import oracles as O
from . import test_oracles_cpu as C
from .test_oracles_cpu import BF16, F32, MODES, dname

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [BF16, F32]
ids = dict(ids=lambda v: dname(v) if isinstance(v, torch.dtype) else str(v))


def each(fn, combos):
    """Run ``fn`` on every combination; a failure names the combination."""
    for c in combos:
        try:
            fn(*c)
        except AssertionError as e:
            raise AssertionError(f"{fn.__name__}{c}: {e}") from e


def prefetch_setups(monkeypatch):
    return tuple((lambda v=v: monkeypatch.setenv("DTD_LN_BWD_PREFETCH", v)) for v in ("0", "1"))


# ------------------------------------------------------------------------------------------
# LayerNorm: every wave kernel (128 .. 2048), the block kernel just past them (2050, 2304); fewer
# rows than a block holds, an odd count for the two-rows-per-wave forwards, several blocks
# ------------------------------------------------------------------------------------------
LN_WIDTHS = [128, 256, 512, 768, 1024, 1280, 1536, 2048, 2050, 2304]


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("h", LN_WIDTHS)
def test_layernorm_fwd_bwd(h, dtype, monkeypatch):
    setups = prefetch_setups(monkeypatch)
    each(lambda rows, p, regime: C.check_layernorm(DEV, rows, h, dtype, p, regime, setups),
         [(rows, p, regime) for regime in C.LN_REGIMES for rows in (1, 3, 5, 37) for p in C.ln_probs(regime)])


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("h", LN_WIDTHS)
def test_layernorm_bwd_from_output(h, dtype, monkeypatch):
    """x-hat = (out - beta) / gamma from the stored output loses information as |beta| / |gamma| grows.
    No fixed tolerance: per slice, the kernel's error against the true gradients must stay within
    twice the error of the fp64 evaluation of the same formula on the same rounded output (what the
    stored data has already lost) plus the dtype's ordinary tolerance.  Both errors are printed per
    ratio.  Measured on an MI355X, bf16, 37 rows, worst row of dz, kernel / inherent:

        |beta|/|gamma|   h = 128            h = 768            h = 1024           h = 2304
        0.1              3.2e-3 / 7.3e-4    2.7e-3 / 2.3e-4    3.1e-3 / 2.6e-4    3.8e-3 / 1.4e-4
        1                3.2e-3 / 7.8e-4    2.8e-3 / 3.2e-4    3.1e-3 / 3.2e-4    3.8e-3 / 1.7e-4
        10               5.3e-3 / 4.7e-3    3.7e-3 / 2.0e-3    3.1e-3 / 1.4e-3    3.8e-3 / 7.0e-4
        100              4.1e-2 / 4.1e-2    1.4e-2 / 1.4e-2    1.3e-2 / 1.4e-2    6.7e-3 / 6.7e-3

    (fp32: 2.2e-7 .. 2.7e-7 / 1.2e-7 .. 2.2e-7 at every ratio.)  Up to a ratio of 10 the kernel's error
    is the bf16 rounding of dz itself; from there the loss in the stored output takes over and grows
    with the ratio: at 100 it is 70 % of the 2e-2 bf16 tolerance for h >= 768 and twice the tolerance
    at h = 128.  The models initialise gamma = 1, beta = 0 (ratio 0) and are 768 wide or more, so
    ``store_z=False`` is safe unless training drives |beta| to about a hundred times |gamma|."""
    setups = prefetch_setups(monkeypatch)
    for rows in (1, 3, 5):
        C.check_layernorm_from_output(DEV, rows, h, 1, setups=setups, dtype=dtype)
    for ratio in (0.1, 1, 10, 100):
        k, i = C.check_layernorm_from_output(DEV, 37, h, ratio, setups=setups, dtype=dtype)
        print(f"\nfrom-output LayerNorm {dname(dtype)} h={h} |beta|/|gamma|={ratio}: dz error {k:.3e}, inherent {i:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("h", [768, 2050])
def test_layernorm_bwd_from_output_zero_gamma(h, dtype, monkeypatch):
    """gamma == 0 columns: x-hat 0, no dgamma (norm.hip's documented limit of the form)."""
    C.check_layernorm_from_output(DEV, 5, h, 1, zero_cols=(0, 5, h - 1), setups=prefetch_setups(monkeypatch),
                                  dtype=dtype)


# ------------------------------------------------------------------------------------------
# RMSNorm: both sides of every switch of form (512, 1024, 2048, 4096), the smallest and the two
# largest widths the kernel takes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("h", [8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8184, 8192])
def test_rmsnorm_fwd_bwd(h, dtype):
    assert _lib.lib().dtd_rms_supported(h)
    regimes = ["gauss", "row_scales", "constant", "spike"] + (["tiny", "huge"] if dtype == F32 else [])
    each(lambda rows, extras, regime: C.check_rmsnorm(DEV, rows, h, dtype, extras, regime),
         [(rows, extras, regime) for regime in regimes for rows in (1, 5, 37) for extras in (True, False)])


# ------------------------------------------------------------------------------------------
# row softmax: n = 300 / 2049 the VEC = 1 wide path, 2048 the register-resident limit, 2056 the
# VEC = 8 wide path
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("n", [1, 7, 8, 100, 256, 300, 2048, 2056, 2049])
def test_softmax_fwd_bwd(n, dtype):
    each(lambda rows, regime: C.check_softmax(DEV, rows, n, dtype, regime),
         [(rows, regime) for regime in ("gauss", "large_logits", "masked") for rows in (1, 5, 37)])
    # the large_logits backward is held on the rows that are not nearly one-hot: some at every width
    assert sum(int(C.softmax_case(rows, n, dtype, "large_logits")[5].sum()) for rows in (1, 5, 37)) >= 1


# ------------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("V", [1, 7, 13, 1000, 1004, 4099])
def test_xent_fwd_bwd(V, dtype):
    each(lambda rows, off, regime: C.check_xent(DEV, rows, V, dtype, off, regime),
         [(rows, off, regime) for regime in ("gauss", "large_logits", "masked") for rows in (1, 4, 33)
          for off in (0, 1, 3)])


@pytest.mark.parametrize("regime", ["gauss", "large_logits", "masked"])
@pytest.mark.parametrize("V", [4, 1000, 1004, 4100])
def test_xent_fwd_train(V, regime):
    """The one-pass training forward (bf16, V % 4 == 0): loss, lse, dlogits for a loss gradient of 1 and
    -- through xent_grad_scale_ -- of 0.7, and the bias gradient, all against the oracle."""
    for rows in (4, 33):
        z, lab, zmax, ref07, ref1 = C.xent_case(rows, V, BF16, regime)
        E = C.Errs("xent_fwd_train", regime, BF16)
        valid = lab != -100
        res = Fx.xent_fwd_train(z.to(DEV), lab.to(DEV))
        assert res is not None, "the fused training forward must take this case"
        loss, lse, st, d, dbias = res
        E.cmp("loss", loss, ref1["loss"], 1e-4, scale=torch.maximum(ref1["loss"].abs(), zmax[valid].max()))
        E.cmp("lse", lse.cpu()[valid], ref1["lse"][valid], 1e-4, axis=None,
              scale=torch.maximum(ref1["lse"].abs(), zmax)[valid])
        assert torch.equal(lse.cpu()[~valid], torch.zeros(int((~valid).sum())))
        assert st[1].item() == int(valid.sum()) and st[0].item() == loss.item()
        E.cmp("dlogits", d, ref1["dlogits"], 2e-2)
        colsum, colscale = O.column_sums(d)
        E.cmp("dbias", dbias, colsum, 1e-4, axis=None, scale=colscale)
        one = Fx.xent_grad_scale_(d.clone(), torch.tensor(1.0, device=DEV))
        assert torch.equal(one, d)                                    # a loss gradient of 1 leaves it alone
        E.cmp("dlogits*0.7", Fx.xent_grad_scale_(d.clone(), torch.tensor(C.GOUT, device=DEV)), ref07["dlogits"], 2e-2)


# ------------------------------------------------------------------------------------------
# the -inf fix leaves finite inputs alone
# ------------------------------------------------------------------------------------------
def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def finite_input_digests():
    """Digests of xent_fwd's (loss, lse) and the wide-row softmax output on the ``gauss`` regime."""
    out = {}
    for dtype in DTYPES:
        for V in (1000, 1004, 4099):
            z, lab, *_ = C.xent_case(33, V, dtype, "gauss")
            res = []
            for off in (0, 1, 3):
                loss, lse, _ = Fx.xent_fwd(C._at_offset(z, off, DEV), lab.to(DEV))
                res += [loss.reshape(1), lse]
            out[f"xent/{dname(dtype)}/{V}"] = _digest(*res)
        for n in (300, 2049, 2056):
            x = C.softmax_case(37, n, dtype, "gauss")[0]
            out[f"softmax/{dname(dtype)}/{n}"] = _digest(Fx.softmax_fwd(x.to(DEV)))
    return out


# Recorded from the kernels as they were before the running maxima started at -FLT_MAX (the parent
# commit's library, run on the same inputs on an MI355X).
DIGESTS_BEFORE_THE_FIX = {
    "xent/bf16/1000": "872432633ebe3f56",
    "xent/bf16/1004": "b5a6e453f5520407",
    "xent/bf16/4099": "84df89b4754ee7c3",
    "softmax/bf16/300": "ea78cf91728bfc19",
    "softmax/bf16/2049": "7faf2f3899e44420",
    "softmax/bf16/2056": "48c26af90d32d1b8",
    "xent/fp32/1000": "5deb1973fcb8a148",
    "xent/fp32/1004": "211a513f16734b3c",
    "xent/fp32/4099": "d747e568e5522ce8",
    "softmax/fp32/300": "e2365cc910bebf5f",
    "softmax/fp32/2049": "8451a0627055befa",
    "softmax/fp32/2056": "fcfc4e62804faa59",
}


def test_finite_inputs_bitwise_as_before_the_inf_fix():
    got = finite_input_digests()
    print(got)
    assert got == DIGESTS_BEFORE_THE_FIX


# ------------------------------------------------------------------------------------------
# activations, SwiGLU, RoPE, dropout-add
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("act", ["gelu", "gelu_tanh", "relu"])
def test_activation_fwd_bwd(act, dtype):
    each(lambda n, regime: C.check_activation(DEV, n, dtype, act, regime),
         [(n, regime) for regime in ("gauss", "saturated") for n in (1, 7, 8, 2047, 2048 * 3 + 5)])


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("f", [8, 384, 392])
def test_swiglu_fwd_bwd(f, dtype):
    each(lambda rows, regime: C.check_swiglu(DEV, rows, f, dtype, regime),
         [(rows, regime) for regime in ("gauss", "saturated") for rows in (1, 5, 37)])


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("pos_mode", ["arange", "random", "clamped"])
def test_rope(pos_mode, dtype):
    each(lambda D, S: C.check_rope(DEV, D, S, dtype, pos_mode), [(D, S) for D in (64, 128) for S in (1, 130)])


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dropout_add(p, dtype):
    each(lambda n: C.check_dropout_add(DEV, n, dtype, p), [(n,) for n in (1, 7, 8, 100003)])


# ------------------------------------------------------------------------------------------
# fused Adam
# ------------------------------------------------------------------------------------------
ADAM_N = (1, 7, 8, 9, 2048, 2055, 4096 + 3)


def adam_launch(p, m, v, g, lowp, n, hp, mode, start=0):
    """dtd_adam_step on elements [start, start + n) of the views, at pointer offsets as
    FusedAdam.step_range launches it."""
    hp = hp if hp.is_cuda else hp.to(DEV)
    _lib.call("dtd_adam_step", p.data_ptr() + 4 * start, m.data_ptr() + 4 * start, v.data_ptr() + 4 * start,
              g.data_ptr() + g.element_size() * start, _lib.dt(g), None if lowp is None else lowp.data_ptr() + 2 * start,
              n, hp.data_ptr(), mode, _lib.stream())
    torch.cuda.synchronize()     # hp may be a temporary


@pytest.mark.parametrize("gdt", DTYPES, **ids)
@pytest.mark.parametrize("with_lowp", [True, False], ids=["lowp", "no_lowp"])
@pytest.mark.parametrize("step,wd", [(1, 0.0), (1, 0.01), (100000, 0.0), (100000, 0.01)])
def test_fused_adam_matches_oracle(step, wd, with_lowp, gdt):
    each(lambda n, mode: C.check_adam(adam_launch, DEV, n, mode, gdt, with_lowp, step, wd),
         [(n, mode) for n in ADAM_N for mode in MODES])


def _adam_state(n, gdt, step, wd):
    p, m, v, g, hp = C.adam_case(n, gdt, step, wd)
    bufs = [C.padded(t, DEV) for t in (p, m, v, g)] + [C.padded(torch.zeros(n, dtype=BF16), DEV)]
    return bufs, hp.to(DEV)


def _assert_same_buffers(a, b, what):
    for (ba, _), (bb, _), name in zip(a, b, ("p", "m", "v", "g", "lowp")):
        assert torch.equal(ba, bb), f"{what}: {name} differs (sentinels included)"


@pytest.mark.parametrize("gdt", DTYPES, **ids)
def test_fused_adam_forms_bitwise_identical(gdt, monkeypatch):
    """DTD_ADAM_FORM: one or two 8-element groups per thread, cached or non-temporal loads -- the same
    p / m / v / bf16 copy bit for bit, sentinels untouched."""
    for n in ADAM_N:
        for mode in (0, 3, 7):
            monkeypatch.delenv("DTD_ADAM_FORM", raising=False)
            ref, hp = _adam_state(n, gdt, 100000, 0.01)
            adam_launch(*(v for _, v in ref), n, hp, mode)
            for form in ("1", "2", "1c", "2c"):
                monkeypatch.setenv("DTD_ADAM_FORM", form)
                got, _ = _adam_state(n, gdt, 100000, 0.01)
                adam_launch(*(v for _, v in got), n, hp, mode)
                _assert_same_buffers(got, ref, f"n={n} mode={mode} form={form}")


@pytest.mark.parametrize("gdt", DTYPES, **ids)
@pytest.mark.parametrize("form", [None, "2c"])
def test_fused_adam_spans_bitwise_identical(form, gdt, monkeypatch):
    """A whole-buffer launch equals launches over [0, a) and [a, n) at pointer offsets (a: multiples of
    FlatLayout's 64-element alignment), as FusedAdam._step_staged / step_range split the buffer: an
    element is a vector element in one launch and a tail element in the other."""
    if form is None:
        monkeypatch.delenv("DTD_ADAM_FORM", raising=False)
    else:
        monkeypatch.setenv("DTD_ADAM_FORM", form)
    for n in (2055, 4096 + 3):
        for a in (64, 2048 + 64):
            if a >= n:
                continue
            for mode in (0, 3, 7):
                whole, hp = _adam_state(n, gdt, 100000, 0.01)
                adam_launch(*(v for _, v in whole), n, hp, mode)
                parts, _ = _adam_state(n, gdt, 100000, 0.01)
                views = [v for _, v in parts]
                adam_launch(*views, a, hp, mode, start=0)
                adam_launch(*views, n - a, hp, mode, start=a)
                _assert_same_buffers(parts, whole, f"n={n} a={a} mode={mode}")


# ------------------------------------------------------------------------------------------
# sq-norm and scale-cast
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", DTYPES, **ids)
@pytest.mark.parametrize("ddt", DTYPES, **ids)
def test_sqnorm_and_scale_cast(ddt, sdt):
    each(lambda n, ds: C.check_sqnorm_scale_cast(DEV, n, sdt, ddt, ds),
         [(n, ds) for n in (1, 7, 8, 2049, 123457) for ds in (False, True)])
