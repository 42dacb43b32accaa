"""Generation with the ring KV cache on the GPU (bf16, fused path; ops/csrc/attention_ring.hip): ``mistral-tiny``
(window 48, R = 64), prompts of 40 and of 100 tokens (longer than the ring), 80 more tokens so the ring wraps more
than once, B = 3 with left padding, both cache formats.

Bound of the logits, teacher-forced: the reference is the fp32 reference-path model on a LINEAR cache of the same
format.  ``e_lin`` is the linear fused path's worst error against it over the decode steps (the prefill's own logits
come from the same code in both and are left out) -- the parent's code, measured here -- and the ring's worst error must be <= 2 e_lin: the two fused paths read the same keys and differ only in the
summation order and the split boundaries, so a factor of two is slack for rounding, not for a wrong key.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME, B, N, R = "mistral-tiny", 3, 80, 64


def _models():
    model = build_model(NAME, impl="fused", dtype=torch.bfloat16, device=DEV, seed=1).eval()
    ref = build_model(NAME, impl="reference", seed=1).eval()
    ref.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    return model, ref


def _batch(cfg, length):
    ids = torch.randint(3, cfg.vocab_size, (B, length), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(B, length, dtype=torch.int64)
    for b, pad in ((1, 5), (2, 17)):
        ids[b, :pad], mask[b, :pad] = cfg.pad_token_id, 0
    return ids, mask


def _steps(model, ids, mask, S0, dev, dtype, kv_dtype, ring):
    """Teacher-forced cached logits [N, B, V]: the prompt ids[:, :S0], then one given token per step."""
    cache = KVCache.allocate(model.cfg, B, ids.shape[1], dev, dtype, kv_dtype=kv_dtype, ring=ring)
    d = ids.to(dev)
    out = [model.prefill(d[:, :S0], cache, mask[:, :S0].to(dev))]
    for t in range(N - 1):
        out.append(model.decode_step(d[:, S0 + t], cache))
    assert int(cache.overflow) == 0 and cache.kv_len.tolist() == [S0 + N - 1] * B and cache.slots == (R if ring else S0 + N)
    return torch.stack(out).float().cpu()


@pytest.mark.parametrize("kv_dtype", [None, "fp8"], ids=["bf16", "fp8"])
@pytest.mark.parametrize("S0", [40, 100])
def test_ring_logits_against_the_reference_on_the_linear_cache(S0, kv_dtype):
    model, ref = _models()
    ids, mask = _batch(model.cfg, S0 + N)
    r = _steps(ref, ids, mask, S0, "cpu", torch.float32, kv_dtype, False)
    e_lin = float((_steps(model, ids, mask, S0, DEV, torch.bfloat16, kv_dtype, False) - r)[1:].abs().max())
    e_ring = float((_steps(model, ids, mask, S0, DEV, torch.bfloat16, kv_dtype, True) - r)[1:].abs().max())
    print(f"S0 = {S0}, {kv_dtype or 'bf16'} cache: e_ring {e_ring:.3e}, e_lin {e_lin:.3e}")
    assert e_ring <= 2 * e_lin, (e_ring, e_lin)


@pytest.mark.parametrize("kv_dtype", [None, "fp8"], ids=["bf16", "fp8"])
def test_graph_replay_equals_the_eager_ring_run(kv_dtype):
    model, _ = _models()
    ids, mask = _batch(model.cfg, 100)
    kw = dict(attention_mask=mask.to(DEV), kv_dtype=kv_dtype, kv_ring=True)
    caches = []
    eager = model.generate(ids.to(DEV), N, **kw)
    graph = model.generate(ids.to(DEV), N, graph=True, cache_out=caches, **kw)
    torch.cuda.synchronize()
    assert torch.equal(eager, graph) and tuple(eager.shape) == (B, 100 + N)
    assert caches[0].ring and caches[0].slots == R and int(caches[0].overflow) == 0
