"""``CausalLM.extend`` and the chunked prefill on the GPU (bf16, fused path) against the fp32 reference-path model.

Bound: tests/test_generate_gpu.py's -- at every position the cached logits' largest error against the fp32
reference is at most twice the uncached fused model's error, measured here on the same prefix, plus 1e-3 absolute.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache
from distributed_training_and_deepspeed_amd.utils.graphs import CAPTURE_ERROR_MODE

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRESETS = ("llama-tiny", "llama-tiny-gqa", "mistral-tiny")
ABS = 1e-3


def _models(name):
    model = build_model(name, impl="fused", dtype=torch.bfloat16, device=DEV, seed=1).eval()
    ref = build_model(name, impl="reference", seed=1).eval()
    ref.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    return model, ref


def _ids(cfg, rows, length, seed=1):
    return torch.randint(3, cfg.vocab_size, (rows, length), generator=torch.Generator().manual_seed(seed))


def _assert_rule(got, unc, r32, what):
    e_unc, e = float((unc - r32).abs().max()), float((got.float().cpu() - r32).abs().max())
    print(f"{what}: cached {e:.3e}, uncached {e_unc:.3e}")
    assert e <= 2 * e_unc + ABS, (what, e, e_unc)


@pytest.mark.parametrize("name", PRESETS)
def test_extend_logits_against_the_uncached_model(name):
    """prefill 13, extend 20, extend 7, three decode steps."""
    model, ref = _models(name)
    S = 13 + 20 + 7 + 3
    ids = _ids(model.cfg, 3, S)
    d = ids.to(DEV)
    cache = KVCache.allocate(model.cfg, 3, S, DEV, torch.bfloat16)
    got = {12: model.prefill(d[:, :13], cache)}
    got.update((13 + t, lg) for t, lg in enumerate(model.extend(d[:, 13:33], cache).unbind(1)))
    got[39] = model.extend(d[:, 33:40], cache, last_only=True)
    for t in range(40, S):
        got[t] = model.decode_step(d[:, t], cache)
    torch.cuda.synchronize()
    assert int(cache.overflow) == 0 and cache.kv_len.tolist() == [S] * 3 == [cache.filled] * 3
    with torch.no_grad():
        unc, r32 = model(d).logits.float().cpu(), ref(ids).logits
    for t, lg in got.items():
        _assert_rule(lg, unc[:, t], r32[:, t], f"{name} position {t}")


@pytest.mark.parametrize("name", PRESETS)
def test_chunked_prefill_of_a_left_padded_batch(name):
    model, ref = _models(name)
    S0, N, lens = 40, 4, (40, 33, 14)          # the last sequence is padded beyond the first chunk
    ids = _ids(model.cfg, 3, S0, seed=2)
    mask = torch.ones(3, S0, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids[b, :S0 - n] = model.cfg.pad_token_id
        mask[b, :S0 - n] = 0
    logits = []
    out = model.generate(ids.to(DEV), N, attention_mask=mask.to(DEV), prefill_chunk=16, logits_out=logits).cpu()
    assert tuple(out.shape) == (3, S0 + N) and len(logits) == N
    for b, n in enumerate(lens):
        part = out[b:b + 1, S0 - n:]
        with torch.no_grad():
            unc, r32 = model(part.to(DEV)).logits.float().cpu()[0], ref(part).logits[0]
        for t in range(N):
            _assert_rule(logits[t][b], unc[n - 1 + t], r32[n - 1 + t], f"{name} sequence {b} step {t}")


def test_a_captured_extend_replays_bitwise():
    model, _ = _models("llama-tiny-gqa")
    d = _ids(model.cfg, 2, 24).to(DEV)
    cache = KVCache.allocate(model.cfg, 2, 64, DEV, torch.bfloat16)
    cache.extend_workspace(4)
    model.prefill(d[:, :12], cache)
    want = [model.extend(d[:, s:s + 4], cache).clone() for s in (12, 16, 20)]
    cache.reset()
    model.prefill(d[:, :12], cache)
    tok = d[:, 12:16].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_ERROR_MODE):
        logits = model.extend(tok, cache)
    cache.filled -= 4                          # the capture computed nothing: only replays advance
    for i, s in enumerate((12, 16, 20)):
        tok.copy_(d[:, s:s + 4])
        graph.replay()
        cache.filled += 4
        assert torch.equal(logits.view(torch.int16), want[i].view(torch.int16)), f"replay {i} differs from the eager call"
    torch.cuda.synchronize()
    graph.reset()
