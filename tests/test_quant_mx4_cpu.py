"""The MX4 weight law (``ops/quant.py``) and ``CausalLM.quantize_weights_("mxfp4")`` on the CPU (fp32, reference path)."""
import math

import pytest
import torch

from distributed_training_and_deepspeed_amd.memory.estimate import weight_bytes_mx4
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.models.llama import LlamaLayer
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache
from distributed_training_and_deepspeed_amd.ops.quant import dequantize_weight_mx4, quantize_weight_mx4


@pytest.mark.parametrize("std", (0.02, 1.0, 1e-6, 300.0))
def test_law(std):
    w = torch.randn(48, 640, generator=torch.Generator().manual_seed(3)) * std
    w[5] = 0.0
    e7 = math.frexp(std)[1] - 2
    w[7, 64:96].clamp_(-5.0 * 2.0 ** e7, 5.0 * 2.0 ** e7)
    w[7, 75] = -6.0 * 2.0 ** e7                                       # block 2 of row 7: amax exactly 6 * 2^e
    codes, scales = quantize_weight_mx4(w)
    assert codes.dtype == scales.dtype == torch.uint8 and codes.shape == (48, 320) and scales.shape == (48, 20)
    deq = dequantize_weight_mx4(codes, scales, torch.float32)
    assert deq.shape == w.shape and torch.equal(deq.bfloat16().float(), deq)      # on the bf16 grid, bit for bit
    assert torch.equal(dequantize_weight_mx4(codes, scales, torch.bfloat16).float(), deq)
    scale = torch.ldexp(torch.ones(48, 20), scales.int() - 127)
    ratio = w.view(48, 20, 32).abs().amax(2) / scale
    live = torch.arange(48) != 5
    assert bool(((ratio > 3) & (ratio <= 6))[live].all())
    assert bool((scales[5] == 127).all()) and not bool(codes[5].any())
    assert float(scale[7, 2]) == 2.0 ** e7 and float(ratio[7, 2]) == 6.0
    s = scale.repeat_interleave(32, 1)
    assert bool(((w - deq).abs() <= torch.maximum(w.abs() / 5, s / 4)).all())


def test_packing():
    vals = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
    block = torch.tensor(vals + tuple(-v for v in vals) + (6.0,) * 16) * 0.25      # -0.0 is code 8
    codes, scales = quantize_weight_mx4(block[None])
    assert scales.tolist() == [[125]]
    assert codes.tolist() == [[0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE] + [0x77] * 8]
    assert torch.equal(dequantize_weight_mx4(codes, scales, torch.float32), block[None])


def test_model_quantize_weights():
    model = build_model("llama-tiny-gqa", impl="reference", seed=1).eval()
    keys = list(model.state_dict())
    assert model.quantize_weights_("mxfp4", head=True) is model
    assert list(model.state_dict()) == keys
    mods = [(layer, name) for layer in model.layers for name in LlamaLayer.W8_NAMES] + [(model.head, "own_weight")]
    nbytes = 0
    for mod, name in mods:
        codes, scale = getattr(mod, name + "_codes"), getattr(mod, name + "_scale")
        assert torch.equal(getattr(mod, name), dequantize_weight_mx4(codes, scale, torch.float32)), name
        nbytes += codes.numel() + scale.numel()
    assert nbytes == weight_bytes_mx4(model.cfg, head=True)
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
    with pytest.raises(ValueError):
        model.quantize_weights_("int4")
