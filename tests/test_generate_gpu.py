"""Incremental decoding on the GPU (bf16, fused path): ``prefill`` / ``decode_step`` / ``generate`` of the tiny
Llama-family presets against the uncached fused forward and the fp32 reference-path model on the CPU.

Bound: per step, the cached logits' largest error against the fp32 reference is at most twice the uncached
fused model's error against it -- measured here, on the same prefix -- plus 1e-3 absolute: a quarter of a bf16
ulp at logits of size 1, which is what the head's output rounding alone can move.  The uncached fused forward
and the reference run once over the whole teacher-forced sequence: a causal model's logits at position p are
those of the prefix ending there.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRESETS = ("llama-tiny", "llama-tiny-gqa", "mistral-tiny")
B, S0, N = 3, 40, 24
ABS = 1e-3


def _models(name):
    model = build_model(name, impl="fused", dtype=torch.bfloat16, device=DEV, seed=1).eval()
    ref = build_model(name, impl="reference", seed=1).eval()
    ref.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    return model, ref


def _ids(cfg, rows, length, seed=1):
    return torch.randint(3, cfg.vocab_size, (rows, length), generator=torch.Generator().manual_seed(seed))


def _steps(model, ids, attention_mask=None, max_len=None):
    """Teacher-forced cached logits [N, B, V]: the prompt ids[:, :S0], then one given token per step."""
    rows, total = ids.shape
    cache = KVCache.allocate(model.cfg, rows, max_len or total, DEV, torch.bfloat16)
    d = ids.to(DEV)
    out = [model.prefill(d[:, :S0], cache, attention_mask.to(DEV) if attention_mask is not None else None)]
    for t in range(total - S0 - 1):
        out.append(model.decode_step(d[:, S0 + t], cache))
    torch.cuda.synchronize()
    assert int(cache.overflow) == 0
    assert cache.kv_len.tolist() == [total - 1] * rows == [cache.filled] * rows
    return torch.stack(out).float().cpu()


@pytest.mark.parametrize("name", PRESETS)
def test_cached_logits_against_the_uncached_model(name):
    model, ref = _models(name)
    ids = _ids(model.cfg, B, S0 + N)
    got = _steps(model, ids)
    with torch.no_grad():
        unc = model(ids.to(DEV)).logits.float().cpu()
        r32 = ref(ids).logits
    for t in range(N):
        p = S0 - 1 + t
        e_unc = float((unc[:, p] - r32[:, p]).abs().max())
        e_cached = float((got[t] - r32[:, p]).abs().max())
        print(f"{name} step {t}: cached {e_cached:.3e}, uncached {e_unc:.3e}")
        assert e_cached <= 2 * e_unc + ABS, (t, e_cached, e_unc)


@pytest.mark.parametrize("name", PRESETS)
def test_graph_replay_equals_eager(name):
    model, _ = _models(name)
    ids = _ids(model.cfg, B, S0).to(DEV)
    le, lg = [], []
    eager = model.generate(ids, N, logits_out=le)
    graph = model.generate(ids, N, graph=True, logits_out=lg)
    assert torch.equal(eager, graph) and tuple(eager.shape) == (B, S0 + N) and eager.dtype == torch.int64
    assert len(le) == len(lg) == N
    for t, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"step {t}: replayed logits differ"
    # the sampled path too: the same seeded draws from the same logits
    s1 = model.generate(ids, N, do_sample=True, temperature=0.8, top_k=50, seed=5)
    s2 = model.generate(ids, N, do_sample=True, temperature=0.8, top_k=50, seed=5, graph=True)
    assert torch.equal(s1, s2)


@pytest.mark.parametrize("name", PRESETS)
def test_left_padded_batch_equals_its_parts(name):
    model, ref = _models(name)
    lens = (S0, 33, 21)
    ids = _ids(model.cfg, B, S0 + N, seed=2)
    mask = torch.ones(B, S0, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids[b, :S0 - n] = model.cfg.pad_token_id
        mask[b, :S0 - n] = 0
    got = _steps(model, ids, mask)                               # [N, B, V]
    for b, n in enumerate(lens):
        part = ids[b:b + 1, S0 - n:]
        with torch.no_grad():
            unc = model(part.to(DEV)).logits.float().cpu()[0]
            r32 = ref(part).logits[0]
        alone = _steps_alone(model, part, n)
        for t in range(N):
            p = n - 1 + t
            e_unc = float((unc[p] - r32[p]).abs().max())
            for what, x in (("batch", got[t, b]), ("alone", alone[t, 0])):
                e = float((x - r32[p]).abs().max())
                assert e <= 2 * e_unc + ABS, (what, b, t, e, e_unc)


def _steps_alone(model, part, n):
    cache = KVCache.allocate(model.cfg, 1, part.shape[1], DEV, torch.bfloat16)
    d = part.to(DEV)
    out = [model.prefill(d[:, :n], cache)]
    for t in range(part.shape[1] - n - 1):
        out.append(model.decode_step(d[:, n + t], cache))
    assert int(cache.overflow) == 0
    return torch.stack(out).float().cpu()


def test_overflow_flag_and_no_out_of_bounds_append():
    """A step past the cache's end is refused on the host; the device-side guard is the append's own: it
    writes nothing and raises the flag (tests/test_attention_decode_gpu.py checks the slots)."""
    model, _ = _models("llama-tiny-gqa")
    ids = _ids(model.cfg, 2, 8).to(DEV)
    cache = KVCache.allocate(model.cfg, 2, 9, DEV, torch.bfloat16)
    model.prefill(ids, cache)
    model.decode_step(ids[:, 0], cache)
    with pytest.raises(ValueError):
        model.decode_step(ids[:, 0], cache)
    assert int(cache.overflow) == 0
