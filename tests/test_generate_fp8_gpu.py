"""Generation with the FP8 KV cache on the GPU (bf16, fused path): ``generate(kv_dtype="fp8")`` of llama-tiny-gqa and
of mistral-tiny past its window -- graph replay against eager, the cache's counters, and the per-step logits
against the fp32 reference-path model with an FP8 cache of its own (``quantize_kv_ref`` on the CPU).

Bound of the logits: per step ``e <= 2 e_unc + e_q + ABS``.  ``e_unc`` and ``ABS`` = 1e-3 are those of
``tests/test_generate_gpu.py``: the uncached bf16 fused model's error against the uncached fp32 reference on the same
prefix, and a quarter of a bf16 ulp at logits of size 1.  ``e_q`` is the reference's own difference between its FP8
and its unquantised cache at that step: the two models quantise rows that differ by bf16 roundings, so their codes
differ in places by one step -- an error of the quantisation's own size, not of the kernels.  All three come from
code other than the kernels under test.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRESETS = ("llama-tiny-gqa", "mistral-tiny")
B, S0, N = 3, 40, 24          # 64 positions: past mistral-tiny's window of 48
ABS = 1e-3


def _models(name):
    model = build_model(name, impl="fused", dtype=torch.bfloat16, device=DEV, seed=1).eval()
    ref = build_model(name, impl="reference", seed=1).eval()
    ref.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    return model, ref


def _ids(cfg, rows, length, seed=1):
    return torch.randint(3, cfg.vocab_size, (rows, length), generator=torch.Generator().manual_seed(seed))


def _steps(model, ids, dev, dtype, kv_dtype):
    """Teacher-forced cached logits [N, B, V] and the cache: the prompt ids[:, :S0], then one given token per step."""
    rows, total = ids.shape
    cache = KVCache.allocate(model.cfg, rows, total, dev, dtype, kv_dtype=kv_dtype)
    d = ids.to(dev)
    out = [model.prefill(d[:, :S0], cache)]
    for t in range(total - S0 - 1):
        out.append(model.decode_step(d[:, S0 + t], cache))
    return torch.stack(out).float().cpu(), cache


@pytest.mark.parametrize("name", PRESETS)
def test_graph_replay_equals_eager_and_the_counters(name):
    model, _ = _models(name)
    ids = _ids(model.cfg, B, S0).to(DEV)
    le, lg, ce, cg = [], [], [], []
    eager = model.generate(ids, N, logits_out=le, kv_dtype="fp8", cache_out=ce)
    graph = model.generate(ids, N, graph=True, logits_out=lg, kv_dtype="fp8", cache_out=cg)
    torch.cuda.synchronize()
    assert torch.equal(eager, graph) and tuple(eager.shape) == (B, S0 + N) and eager.dtype == torch.int64
    assert len(le) == len(lg) == N
    for t, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"step {t}: replayed logits differ"
    for cache in (ce[0], cg[0]):
        assert cache.quantized and cache.k.dtype == torch.float8_e4m3fn
        assert int(cache.overflow) == 0
        assert cache.kv_len.tolist() == [S0 + N - 1] * B == [cache.filled] * B
        assert cache.kv_next.tolist() == [S0 + N] * B
    for a, b in ((ce[0].k, cg[0].k), (ce[0].v, cg[0].v), (ce[0].k_scale, cg[0].k_scale), (ce[0].v_scale, cg[0].v_scale)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))         # the replays appended the same codes and scales


@pytest.mark.parametrize("name", PRESETS)
def test_cached_logits_against_the_reference_with_an_fp8_cache(name):
    model, ref = _models(name)
    ids = _ids(model.cfg, B, S0 + N)
    got, cache = _steps(model, ids, DEV, torch.bfloat16, "fp8")
    torch.cuda.synchronize()
    assert int(cache.overflow) == 0 and cache.kv_len.tolist() == [S0 + N - 1] * B == [cache.filled] * B
    with torch.no_grad():
        unc = model(ids.to(DEV)).logits.float().cpu()
        r32 = ref(ids).logits
    r8, _ = _steps(ref, ids, "cpu", torch.float32, "fp8")
    ru, _ = _steps(ref, ids, "cpu", torch.float32, None)
    for t in range(N):
        p = S0 - 1 + t
        e_unc = float((unc[:, p] - r32[:, p]).abs().max())
        e_q = float((r8[t] - ru[t]).abs().max())
        e = float((got[t] - r8[t]).abs().max())
        print(f"{name} step {t}: e {e:.3e}, e_unc {e_unc:.3e}, e_q {e_q:.3e}")
        assert e <= 2 * e_unc + e_q + ABS, (t, e, e_unc, e_q)
