"""Decoding with FP8 weights (``CausalLM.quantize_weights_("fp8", head=True)``) on the GPU: the decode steps read
the codes through ``ops.gemm.linear_skinny``, everything else the parameters, which hold the same values.

The reference is the fp32 reference-path model loaded from the QUANTISED model's state dict: the weights are
identical on both sides, so quantisation is no error here and ``test_generate_gpu.py``'s bound holds as it is:
per step, e_cached <= 2 e_uncached + 1e-3, e_uncached being the same quantised model's uncached fused forward.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S0, N = 3, 40, 24
ABS = 1e-3


def _model(name):
    model = build_model(name, impl="fused", dtype=torch.bfloat16, device=DEV, seed=1).eval()
    model.quantize_weights_("fp8", head=True)
    assert model.layers[0].qkv_w_codes.dtype == torch.float8_e4m3fn and model.head.own_weight_codes.is_cuda
    return model


@pytest.mark.parametrize("name", ("llama-tiny-gqa", "mistral-tiny"))
def test_cached_logits_of_the_quantised_model(name):
    model = _model(name)
    ref = build_model(name, impl="reference", seed=1).eval()
    ref.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    ids = torch.randint(3, model.cfg.vocab_size, (B, S0 + N), generator=torch.Generator().manual_seed(1))
    d = ids.to(DEV)
    cache = KVCache.allocate(model.cfg, B, S0 + N, DEV, torch.bfloat16)
    got = [model.prefill(d[:, :S0], cache)] + [model.decode_step(d[:, S0 + t], cache) for t in range(N - 1)]
    got = torch.stack(got).float().cpu()
    assert int(cache.overflow) == 0
    with torch.no_grad():
        unc = model(d).logits.float().cpu()
        r32 = ref(ids).logits
    for t in range(N):
        p = S0 - 1 + t
        e_unc = float((unc[:, p] - r32[:, p]).abs().max())
        e_cached = float((got[t] - r32[:, p]).abs().max())
        print(f"{name} step {t}: cached {e_cached:.3e}, uncached {e_unc:.3e}")
        assert e_cached <= 2 * e_unc + ABS, (t, e_cached, e_unc)


@pytest.mark.parametrize("name", ("llama-tiny-gqa", "mistral-tiny"))
def test_graph_replay_equals_eager(name):
    model = _model(name)
    ids = torch.randint(3, model.cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(1)).to(DEV)
    le, lg = [], []
    eager = model.generate(ids, N, logits_out=le)
    graph = model.generate(ids, N, graph=True, logits_out=lg)
    assert torch.equal(eager, graph) and len(le) == len(lg) == N
    for t, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"step {t}: replayed logits differ"
