"""FP8 activations (``CausalLM.set_fp8_activations``) on the GPU: a prefill of 96 rows and an ``extend`` of 80 rows of
``llama-tiny-gqa`` in bf16 with FP8 weights (head included), whose projections run on the FP8 GEMM.

Oracle: the same quantised model in fp64 on the reference path, the activation law emulated.  Metric: e = max |logits -
oracle|.  Bound: e_fused <= 2 e_ref, e_ref being the PyTorch reference path in bf16 on the GPU, computed here.  The
bound is measured against the reference, not derived: a bf16-level difference between two paths can move an activation
across a rounding tie of the e4m3 grid, a step of 2^-3 relative on that element; the reference path suffers the same
flips against fp64, and the factor 2 lets the two paths flip different elements.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops import gemm as G
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

pytestmark = pytest.mark.gpu
NAME, B, S0, T = "llama-tiny-gqa", 2, 48, 40


def _like(model, impl, dtype, device):
    """The quantised ``model`` on another path: the same weights, with codes made again from them (a weight on the grid
    is its own dequantised value)."""
    m = build_model(NAME, impl=impl, seed=1).eval()
    m.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    m = m.to(device=device, dtype=dtype)
    m.quantize_weights_("fp8", head=True).set_fp8_activations(True)
    assert torch.equal(m.head.weight.double().cpu(), model.head.weight.double().cpu())
    return m


def _logits(model, ids, dtype):
    """(the prefill's last-position logits [B, V], the extend's [B, T, V]) in fp64 on the CPU."""
    cache = KVCache.allocate(model.cfg, B, S0 + T, ids.device, dtype)
    with torch.no_grad():
        out = model.prefill(ids[:, :S0], cache), model.extend(ids[:, S0:], cache)
    assert int(cache.overflow) == 0
    return [o.double().cpu() for o in out]


def test_prefill_and_extend_against_the_fp64_oracle():
    fused = build_model(NAME, impl="fused", dtype=torch.bfloat16, device="cuda", seed=1).eval()
    fused.quantize_weights_("fp8", head=True).set_fp8_activations(True)
    ids = torch.randint(3, fused.cfg.vocab_size, (B, S0 + T), generator=torch.Generator().manual_seed(1))
    with G.fp8_at_any_size():           # (the dispatch leaves products as small as this model's on the parameters)
        oracle = _logits(_like(fused, "reference", torch.float64, "cpu"), ids, torch.float64)
        ref = _logits(_like(fused, "reference", torch.bfloat16, "cuda"), ids.cuda(), torch.bfloat16)
        got = _logits(fused, ids.cuda(), torch.bfloat16)
        plain = fused.set_fp8_activations(False).prefill(ids[:, :S0].cuda(), KVCache.allocate(fused.cfg, B, S0, "cuda", torch.bfloat16))
    assert not torch.equal(plain.double().cpu(), got[0])          # the FP8 GEMM did run
    for what, o, r, g in zip(("prefill, 96 rows", "extend, 80 rows"), oracle, ref, got):
        e_ref, e_fused = float((r - o).abs().max()), float((g - o).abs().max())
        print(f"{what}: e_ref {e_ref:.3e}, e_fused {e_fused:.3e}")
        assert e_fused <= 2 * e_ref, (what, e_fused, e_ref)
