"""The FP8 activation law (``ops.quant.quantize_act_fp8``: the weight law on the rows of activations) and the model
contract of ``CausalLM.set_fp8_activations`` on the CPU (fp32, reference path).

``hand_rows`` are the law's edge cases, shared with ``test_gemm_fp8_gpu.py``: an all-zero row, amax exactly 448 * 2^3,
amax one bf16 step above it, and tiny values whose exponent hits the clamp at -100.
"""
import pytest
import torch
import torch.nn.functional as F

from distributed_training_and_deepspeed_amd.models import build_model, llama
from distributed_training_and_deepspeed_amd.ops import gemm as G
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache
from distributed_training_and_deepspeed_amd.ops.quant import dequantize_weight, quantize_act_fp8

HAND_SCALES = (1.0, 8.0, 16.0, 2.0 ** -100)


def hand_rows(K):
    """bf16 [4, K]; their scales are HAND_SCALES."""
    x = torch.randn(4, K, generator=torch.Generator().manual_seed(K)).clamp_(-3, 3)
    x[0] = 0.0
    x[1] *= 100.0
    x[1, K // 2] = -3584.0                # 448 * 2^3 exactly: scale 2^3
    x[2] *= 100.0
    x[2, 1] = 3600.0                      # the next bf16 above it: scale 2^4, amax / scale = 225
    x[3] *= 2.0 ** -106                   # amax about 3 * 2^-106: the law's exponent would be -113
    return x.bfloat16()


def test_law():
    x = torch.randn(40, 384, generator=torch.Generator().manual_seed(5)) * torch.logspace(-8, 8, 40, base=2.0)[:, None]
    x = torch.cat([hand_rows(384).float(), x]).bfloat16()
    codes, scale = quantize_act_fp8(x)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == x.shape and scale.dtype == torch.float32
    assert torch.equal(scale[:4], torch.tensor(HAND_SCALES))
    assert not bool(codes[0].float().any()) and float(codes[1].float().abs().max()) == 448.0
    assert torch.equal(torch.exp2(torch.log2(scale).round()), scale)          # powers of two
    xf = x.float()
    ratio = xf.abs().amax(1) / scale
    assert bool(((ratio > 224) & (ratio <= 448))[[1, 2] + list(range(4, 44))].all())
    deq = dequantize_weight(codes, scale, torch.float32)
    normal = xf.abs() / scale[:, None] >= 2.0 ** -6
    assert bool(normal[3].any()) and bool(((xf - deq).abs()[normal] <= xf.abs()[normal] / 17).all())


class _EmulatedF:
    """``models/llama.py``'s ``F`` with the law written out in front of every product of more than 64 rows."""
    silu = staticmethod(F.silu)

    @staticmethod
    def linear(x, w):
        if x.dim() == 2 and x.shape[0] > 64:
            codes, scale = quantize_act_fp8(x)
            x = codes.float() * scale[:, None]
        return F.linear(x, w)


def _prefill(model, ids):
    cache = KVCache.allocate(model.cfg, ids.shape[0], ids.shape[1], "cpu", torch.float32)
    return model.prefill(ids, cache)


def test_model_contract(monkeypatch):
    model = build_model("llama-tiny", impl="reference", seed=1).eval()
    with pytest.raises(ValueError):
        model.set_fp8_activations(True)
    with pytest.raises(ValueError):
        model.quantize_weights_("mxfp4").set_fp8_activations(True)
    model.quantize_weights_("fp8")
    g = torch.Generator().manual_seed(0)
    long, short = (torch.randint(3, model.cfg.vocab_size, (2, s), generator=g) for s in (40, 24))
    off_long, off_short = _prefill(model, long), _prefill(model, short)
    with monkeypatch.context() as mp:
        mp.setattr(llama, "F", _EmulatedF)
        emulated = _prefill(model, long)
    assert model.set_fp8_activations(True) is model and model.fp8_activations
    assert torch.equal(_prefill(model, long), off_long)          # (products this small stay on the parameters)
    with G.fp8_at_any_size():
        on_long = _prefill(model, long)
        assert torch.equal(on_long, emulated) and not torch.equal(on_long, off_long)      # 80 rows
        assert torch.equal(_prefill(model, short), off_short)                              # 48 rows
    model.clear_quantized_weights()
    assert not model.fp8_activations
