"""The FP8 weight law (``ops/quant.py``) and ``CausalLM.quantize_weights_`` on the CPU (fp32, reference path).

"Normal codes" in the |w| / 17 bound: weights whose scaled value |w| / scale is at least 2^-6, e4m3fn's
smallest normal number.  There the code has 4 significant bits, so |w - deq| <= 2^-4 2^e for |w| / scale in
[2^e, 2^(e+1)), and the rounding error reaches 2^-4 2^e only from 2^e (1 + 1/16) on: at most |w| / 17.
"""
import math

import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models.llama import LlamaLayer
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache
from distributed_training_and_deepspeed_amd.ops.quant import dequantize_weight, quantize_weight_fp8


@pytest.mark.parametrize("std", (0.02, 1.0, 1e-6, 300.0))
def test_law(std):
    w = torch.randn(48, 640, generator=torch.Generator().manual_seed(3)) * std
    w[5] = 0.0
    e7 = math.frexp(std)[1] - 8
    w[7].clamp_(-100.0 * 2.0 ** e7, 100.0 * 2.0 ** e7)
    w[7, 11] = -448.0 * 2.0 ** e7                                     # amax exactly 448 * 2^e: scale 2^e
    codes, scale = quantize_weight_fp8(w)
    assert codes.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and scale.shape == (48,)
    deq = dequantize_weight(codes, scale, torch.float32)
    assert torch.equal(deq.bfloat16().float(), deq)                  # on the bf16 grid, bit for bit
    assert torch.equal(dequantize_weight(codes, scale, torch.bfloat16).float(), deq)
    live = torch.arange(48) != 5
    ratio = w.abs().amax(1) / scale
    assert bool(((ratio > 224) & (ratio <= 448))[live].all())
    assert torch.equal(torch.exp2(torch.log2(scale).round()), scale)  # powers of two
    assert float(scale[5]) == 1.0 and not bool(codes[5].float().any())
    assert float(scale[7]) == 2.0 ** e7 and float(ratio[7]) == 448.0
    normal = w.abs() / scale[:, None] >= 2.0 ** -6
    assert bool(((w - deq).abs()[normal] <= w.abs()[normal] / 17).all())


def test_model_quantize_weights():
    model = build_model("llama-tiny-gqa", impl="reference", seed=1).eval()
    keys = list(model.state_dict())
    assert model.quantize_weights_("fp8", head=True) is model
    assert list(model.state_dict()) == keys
    mods = [(layer, name) for layer in model.layers for name in LlamaLayer.W8_NAMES] + [(model.head, "own_weight")]
    for mod, name in mods:
        codes, scale = getattr(mod, name + "_codes"), getattr(mod, name + "_scale")
        assert torch.equal(getattr(mod, name), dequantize_weight(codes, scale, torch.float32)), name
    ids = torch.randint(3, model.cfg.vocab_size, (2, 8), generator=torch.Generator().manual_seed(0))
    cache = KVCache.allocate(model.cfg, 2, 16, "cpu", torch.float32)
    model.prefill(ids, cache)
    model.decode_step(ids[:, 0], cache)
    with torch.no_grad():
        model.layers[1].down_w.add_(1.0)          # what an optimizer step does
    with pytest.raises(RuntimeError, match="stale"):
        model.decode_step(ids[:, 1], cache)
    model.clear_quantized_weights()
    assert not [n for n, _ in model.named_buffers() if n.endswith(("_codes", "_scale"))]
    model.decode_step(ids[:, 1], cache)
    with pytest.raises(NotImplementedError):
        build_model("mixtral-tiny", impl="reference").quantize_weights_("fp8")
