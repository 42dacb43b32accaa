"""Multi-token cached attention on the CPU: ``attn_extend_ref`` against the fp64 oracle, and ``CausalLM.extend`` /
``generate(prefill_chunk=)`` of the reference-path models against the uncached model.

The rows of a chunk of T tokens on top of n earlier ones are the rows n .. n + T - 1 of a causal prefill over
n + T tokens with ``key_range = (start, n + T)`` -- ``decode_cases.py``'s construction with T rows instead of one.
"""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops import attention as A
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache

from . import oracles as O
from .decode_cases import REF_CTX_TOL, REF_LSE_TOL, SMAX

NAMES = ("llama-tiny", "llama-tiny-gqa", "mistral-tiny")


@pytest.mark.parametrize("G", (1, 8))
@pytest.mark.parametrize("T", (1, 5, 70))
def test_attn_extend_ref_against_the_oracle(T, G):
    B, Hkv, D = 3, 1, 64
    H = G * Hkv
    qkv, dctx = O.attn_inputs("gauss", B, SMAX, H, D, Hkv, seed=40 + T + G)
    n = torch.tensor([0, 63, SMAX - T])
    start = torch.tensor([0, 5, 64])
    key_range = torch.stack([start, n + T], 1).to(torch.int32)
    o = O.attention(qkv, dctx, B, SMAX, H, D, causal=True, key_range=key_range, kv_heads=Hkv)
    x = qkv.view(B, SMAX, H + 2 * Hkv, D).double()
    rows = torch.stack([torch.arange(int(n[b]), int(n[b]) + T) for b in range(B)])          # [B, T]
    bi = torch.arange(B).view(B, 1)
    k = x[:, :, H:H + Hkv].transpose(1, 2).contiguous()
    v = x[:, :, H + Hkv:].transpose(1, 2).contiguous()
    ctx, lse = A.attn_extend_ref(x[bi, rows].reshape(B * T, -1), k, v, n.to(torch.int32), B, T, H, D, Hkv,
                                 kv_start=start.to(torch.int32))
    assert tuple(ctx.shape) == (B * T, H * D) and tuple(lse.shape) == (B * T, H) and lse.dtype == torch.float32
    O.assert_rows_close(ctx.view(B, T, H, D), o["ctx"][bi, rows], REF_CTX_TOL, what="ctx")
    want, scale = o["lse"].transpose(1, 2)[bi, rows], 1.0 + o["A"].transpose(1, 2)[bi, rows]
    assert float(O.slice_errors(lse.view(B, T, H), want, axis=None, scale=scale).max()) <= REF_LSE_TOL


@pytest.mark.parametrize("name", NAMES)
def test_extend_logits_equal_the_uncached_models(name):
    """prefill 13, extend 20, extend 7, three decode steps: every position's logits against the fp64 uncached model,
    under test_kv_cache_cpu.py's bound for cached-against-uncached fp32 logits."""
    model, m64 = (build_model(name, impl="reference", seed=1).eval() for _ in range(2))
    m64 = m64.double()
    S = 13 + 20 + 7 + 3
    ids = torch.randint(3, model.cfg.vocab_size, (2, S), generator=torch.Generator().manual_seed(1))
    cache = KVCache.allocate(model.cfg, 2, S, "cpu", torch.float32)
    with torch.no_grad():
        got = {12: model.prefill(ids[:, :13], cache)}
        got.update((13 + t, lg) for t, lg in enumerate(model.extend(ids[:, 13:33], cache).unbind(1)))
        got[39] = model.extend(ids[:, 33:40], cache, last_only=True)
        for t in range(40, S):
            got[t] = model.decode_step(ids[:, t], cache)
        r64, unc = m64(ids).logits, model(ids).logits.double()
    assert cache.filled == S and int(cache.overflow) == 0 and cache.kv_len.tolist() == [S, S]
    for t, lg in got.items():
        e_unc = float((unc[:, t] - r64[:, t]).abs().max())
        e_cached = float((lg.double() - r64[:, t]).abs().max())
        print(f"{name} position {t}: cached {e_cached:.2e}, uncached {e_unc:.2e}")
        assert e_cached <= 2 * e_unc + 1e-6, (t, e_cached, e_unc)


@pytest.mark.parametrize("name", NAMES)
def test_chunked_prefill_generates_the_same_tokens(name):
    """A left-padded batch, one sequence padded beyond the first chunk."""
    model = build_model(name, impl="reference", seed=1).eval()
    ids = torch.randint(3, model.cfg.vocab_size, (2, 40), generator=torch.Generator().manual_seed(2))
    mask = torch.ones_like(ids)
    mask[1, :21] = 0
    ids[1, :21] = model.cfg.pad_token_id
    want = model.generate(ids, 6, attention_mask=mask)
    assert torch.equal(model.generate(ids, 6, attention_mask=mask, prefill_chunk=16), want)
    assert torch.equal(model.generate(ids, 6, attention_mask=mask, prefill_chunk=64), want)      # one piece


def test_extend_errors():
    model = build_model("llama-tiny", impl="reference", seed=1).eval()
    ids = torch.randint(3, model.cfg.vocab_size, (2, 12), generator=torch.Generator().manual_seed(3))
    cache = KVCache.allocate(model.cfg, 2, 16, "cpu", torch.float32)
    with pytest.raises(ValueError, match="prefilled"):
        model.extend(ids[:, :4], cache)
    model.prefill(ids[:, :8], cache)
    with pytest.raises(ValueError, match="do not fit"):
        model.extend(ids[:, :9], cache)
    assert tuple(model.extend(ids[:, 8:], cache).shape) == (2, 4, model.cfg.vocab_size) and cache.filled == 12
    with pytest.raises(ValueError):
        model.generate(ids, 2, prefill_chunk=0)
