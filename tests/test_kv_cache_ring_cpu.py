"""The ring KV cache on the reference path (fp32, CPU; ops/kv_cache.py): ``generate(kv_ring=True)`` against the
linear cache on ``mistral-tiny`` (window 48, so R = 64).  Both caches hold the same keys and the reference path
attends them with the same operators, so the per-step logits agree within 1e-5 -- the project's bound for fp32
reference-path equalities -- and the greedy tokens are equal (teacher-forced by construction: the linear run's
tokens are what both runs emit when the logits agree to 1e-5 and the top-2 gap is larger, which is asserted).
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.memory import kv_cache_bytes
from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

NAME, R, N = "mistral-tiny", 64, 80          # 80 new tokens: the ring wraps more than once


def _batch(cfg, S0, B=3):
    """B prompts of S0 tokens, sequences 1 and 2 left-padded by 5 and 17."""
    ids = torch.randint(3, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(B, S0, dtype=torch.int64)
    for b, pad in ((1, 5), (2, 17)):
        ids[b, :pad], mask[b, :pad] = cfg.pad_token_id, 0
    return ids, mask


@pytest.mark.parametrize("S0", [40, 100], ids=["prompt40", "prompt100_longer_than_the_ring"])
def test_generate_on_the_ring_equals_the_linear_cache(S0):
    model = build_model(NAME, impl="reference", seed=1).eval()
    ids, mask = _batch(model.cfg, S0)
    lin, ring, caches = [], [], []
    want = model.generate(ids, N, attention_mask=mask, logits_out=lin)
    got = model.generate(ids, N, attention_mask=mask, logits_out=ring, kv_ring=True, cache_out=caches)
    cache = caches[0]
    assert cache.ring and cache.slots == R and cache.max_len == S0 + N and tuple(cache.k.shape[3:]) == (R, model.cfg.head_dim)
    assert cache.nbytes() == kv_cache_bytes(model.cfg, 3, R, torch.float32)
    assert int(cache.overflow) == 0 and cache.kv_len.tolist() == [S0 + N - 1] * 3
    worst = max(float((a - b).abs().max()) for a, b in zip(lin, ring))
    gap = min(float((t[:, 0] - t[:, 1]).min()) for t in (lg.topk(2, -1).values for lg in lin))
    print(f"S0 = {S0}: worst logit difference {worst:.2e}, smallest top-2 gap {gap:.2e}")
    assert len(ring) == N and worst <= 1e-5
    assert gap > 2e-5, "precondition on the inputs: a top-2 gap within the bound"
    assert torch.equal(got, want)


def test_what_the_ring_does_not_do():
    model = build_model(NAME, impl="reference", seed=1).eval()
    ids, _ = _batch(model.cfg, 40)
    with pytest.raises(ValueError):
        model.generate(ids, 4, kv_ring=True, prefill_chunk=16)
    with pytest.raises(ValueError):          # no window
        build_model("llama-tiny-gqa", impl="reference", seed=1).eval().generate(ids, 4, kv_ring=True)
    for bad in (32, 100):                    # below the window; no multiple of the tile
        with pytest.raises(ValueError):
            KVCache.allocate(model.cfg, 3, 64, "cpu", torch.float32, ring=True, ring_slots=bad)
    cache = KVCache.allocate(model.cfg, 3, 64, "cpu", torch.float32, ring=True, ring_slots=128, kv_dtype="fp8")
    assert cache.slots == 128 and cache.nbytes() == kv_cache_bytes(model.cfg, 3, 128, torch.float32, torch.float8_e4m3fn)
    model.prefill(ids, cache)
    with pytest.raises(NotImplementedError):
        model.extend(ids[:, :4], cache)
    with pytest.raises(NotImplementedError):
        cache.extend_workspace(4)
