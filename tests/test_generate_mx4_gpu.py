"""Decoding with MXFP4 weights (``quantize_weights_("mxfp4", head=True)``) on the GPU against the fp32 reference model
loaded from the QUANTISED state dict: ``test_generate_w8_gpu.py``'s criterion, e_cached <= 2 e_uncached + 1e-3."""
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
    model.quantize_weights_("mxfp4", head=True)
    qkv, head = model.layers[0].qkv_w_codes, model.head.own_weight_codes
    assert qkv.dtype == torch.uint8 and qkv.shape[1] * 2 == model.cfg.hidden_size and head.is_cuda
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
        e_unc = float((unc[:, S0 - 1 + t] - r32[:, S0 - 1 + t]).abs().max())
        e_cached = float((got[t] - r32[:, S0 - 1 + t]).abs().max())
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
