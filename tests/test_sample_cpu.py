"""The sampling law (``ops.functional.sample_tokens_ref`` / ``sample_keep_ref``) against an fp64 implementation
written out here with a sort and a cumulative sum, and ``generate(top_p=...)`` on the CPU."""
import pytest
import torch

from distributed_training_and_deepspeed_amd.models import build_model
from distributed_training_and_deepspeed_amd.ops.functional import sample_keep_ref, sample_tokens_ref, sample_uniform24

V = 200


def _logits(kind):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, V, generator=g)
    if kind == "ties":
        x = (x * 2).round() / 2              # about ten distinct values: ties at every threshold
    if kind == "inf":
        x[:, ::3] = float("-inf")
        x[1, 5:] = float("-inf")
    return x


def _kept_fp64(x, temperature, top_k, top_p):
    """Row by row: (value descending, index ascending) order, top-k, softmax, the shortest prefix reaching top_p."""
    z = (x.float() * float(torch.tensor(1.0 / temperature, dtype=torch.float32))).double()
    keep = torch.zeros_like(x, dtype=torch.bool)
    for b in range(x.shape[0]):
        idx = sorted((i for i in range(V) if z[b, i] > float("-inf")), key=lambda i: (-float(z[b, i]), i))
        if 0 < top_k < V:
            idx = idx[:top_k]
        p = torch.softmax(z[b, idx], 0).cumsum(0)
        n = len(idx) if top_p == 1.0 else int((p < top_p).sum()) + 1
        keep[b, idx[:n]] = True
    return keep


@pytest.mark.parametrize("kind", ["gauss", "ties", "inf"])
@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (7, 1.0), (0, 0.1), (0, 0.9), (30, 0.9), (1, 1.0), (0, 1e-6)])
def test_kept_set_and_draws(kind, top_k, top_p):
    x = _logits(kind)
    keep, _, _ = sample_keep_ref(x, 0.7, top_k, top_p)
    want = _kept_fp64(x, 0.7, top_k, top_p)
    assert torch.equal(keep, want)
    toks = torch.stack([sample_tokens_ref(x, 0.7, top_k, top_p, 11, step, check=True) for step in range(64)])
    assert bool(want.gather(1, toks.t()).all()), "a token outside the kept set was drawn"
    if top_k == 1 or top_p == 1e-6:      # argmax, the lowest index of a tie
        assert torch.equal(toks[0], torch.where(x == x.max(-1, keepdim=True).values, 1, 0).argmax(-1))
    else:
        assert len(toks.unique()) > 4


def test_draw_follows_the_cdf_in_index_order():
    x = torch.tensor([[0.0, 1.0, float("-inf"), 2.0, 1.0]]).log_softmax(-1)
    cdf = x.double().exp().cumsum(-1)
    for step in range(200):
        tok, margin = sample_tokens_ref(x, 1.0, 0, 1.0, 5, step, return_margin=True)
        u = float(sample_uniform24(5, step, 1)[0]) / 2 ** 24
        assert int(tok) == int((cdf[0] <= u).sum()) and int(tok) != 2
        assert abs(float(margin) - float((cdf[0] - u).abs().min()) / float(x.exp().max())) < 1e-6


def test_rows_without_a_finite_logit_and_eos():
    x = torch.full((2, 9), float("-inf"))
    x[1, 4] = 0.5
    assert sample_tokens_ref(x, 1.0, 0, 0.9, 0, 0).tolist() == [0, 4]
    with pytest.raises(ValueError):
        sample_tokens_ref(x, 1.0, 0, 0.9, 0, 0, check=True)
    done = torch.tensor([1, 0], dtype=torch.uint8)
    assert sample_tokens_ref(x, 1.0, 0, 1.0, 0, 0, done, eos=4, pad=7).tolist() == [7, 4] and done.tolist() == [1, 1]


def test_generate_top_p_is_seeded():
    model = build_model("llama-tiny", seed=1).eval()
    ids = torch.randint(3, model.cfg.vocab_size, (2, 8), generator=torch.Generator().manual_seed(1))
    a, b, c = (model.generate(ids, 8, do_sample=True, top_p=0.9, seed=s) for s in (3, 3, 4))
    assert torch.equal(a, b) and not torch.equal(a, c) and tuple(a.shape) == (2, 16)
    assert torch.equal(model.generate(ids, 8, do_sample=True, top_k=1, sampler="device"), model.generate(ids, 8))
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError):
            model.generate(ids, 2, do_sample=True, top_p=bad)
    with pytest.raises(ValueError):
        model.generate(ids, 2, sampler="host")
