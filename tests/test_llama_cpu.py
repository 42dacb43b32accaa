"""Llama family on the CPU: presets, the reference path against HF's LlamaForCausalLM, the fused
path's CPU branches (functional ops + the hand-written layer backward) against the reference,
sequence packing, the rotary embedding's properties, config rejections, the HF weight conversion and
the ZeRO stages over gloo."""
import pytest
import torch
import torch.multiprocessing as mp

from distributed_training_and_deepspeed_amd.models import build_model, count_parameters, get_config
from distributed_training_and_deepspeed_amd.models import config as C
from distributed_training_and_deepspeed_amd.models.causal_lm import CausalLM
from distributed_training_and_deepspeed_amd.models.llama import from_hf_state_dict, to_hf_state_dict
from distributed_training_and_deepspeed_amd.ops import functional as Fx

from . import dist_workers as W
from .conftest import pick_free_port

LOSS_TOL, GRAD_TOL = 1e-5, 1e-4     # relative; the project's own fp32 model bounds are 1e-4 / 1e-3


def _llama_params(c) -> int:
    V, h, L, f = c.vocab_size, c.hidden_size, c.num_layers, c.ffn_size
    return 2 * V * h + L * (4 * h * h + 3 * h * f + 2 * h) + h


# ------------------------------------------------------------------------------------- presets
@pytest.mark.parametrize("name,alias,expected", [
    ("JackFram/llama-160m", "llama-160m", 162_417_408),
    ("princeton-nlp/Sheared-LLaMA-1.3B", "sheared-llama-1.3b", 1_345_423_360),
    ("meta-llama/Llama-2-7b-hf", "llama-2-7b", 6_738_415_616),
])
def test_preset_parameter_counts(name, alias, expected):
    cfg = get_config(name)
    assert get_config(alias) is cfg
    assert cfg.family == "llama" and cfg.norm == "rms" and cfg.rope_theta == 10000.0 and cfg.activation == "swiglu"
    assert not cfg.bias and cfg.pre_ln and cfg.causal and cfg.final_ln and not cfg.tie_word_embeddings
    assert cfg.hidden_dropout == 0.0 and cfg.attn_dropout == 0.0 and not cfg.embedding_ln
    assert _llama_params(cfg) == expected
    with torch.device("meta"):          # nothing is allocated
        model = CausalLM(cfg)
    assert count_parameters(model) == expected
    assert model.embeddings.pos is None


def test_tiny_parameter_count_and_state_dict():
    model = build_model("llama-tiny")
    assert count_parameters(model) == _llama_params(model.cfg)
    # the rotary table is not a parameter or a buffer
    assert not any("rope" in k or "table" in k for k in model.state_dict())
    assert "head.own_weight" in model.state_dict()


def test_defaults_leave_the_other_families_alone():
    for name in ("bert-tiny", "causal-tiny", "bigscience/bloom-560m", "facebook/opt-125m"):
        c = get_config(name)
        assert c.norm == "layer" and c.rope_theta == 0.0 and c.tie_word_embeddings and not c.llama_style
    model = build_model("causal-tiny")
    assert model.head.own_weight is None and model.head.weight is model.embeddings.word
    assert model.zero3_persistent() == [model.embeddings.word]
    llama = build_model("llama-tiny")
    assert llama.zero3_persistent() == [llama.head.own_weight]
    assert len(llama.zero3_units()) == 1 + llama.cfg.num_layers + 1


def test_dgrad_weights_of_the_existing_layers_are_unchanged():
    layer = build_model("causal-tiny").layers[0]
    assert [id(w) for w in layer.dgrad_weights(True)] == [id(getattr(layer, n)) for n in ("qkv_w", "o_w", "fc1_w", "fc2_w")]
    assert [id(w) for w in layer.dgrad_weights(False)] == [id(layer.fc2_w)]
    layer.rt.keep_ffn_act = False
    assert layer.dgrad_weights(False) == ()
    ll = build_model("llama-tiny").layers[0]
    assert [id(w) for w in ll.dgrad_weights(True)] == [id(w) for w in (ll.qkv_w, ll.o_w, ll.gu_w, ll.down_w)]


@pytest.mark.parametrize("bad", [
    dict(hidden_dropout=0.1),      # norm="rms" with hidden dropout
    dict(alibi=True),              # rope with ALiBi
    dict(num_heads=4),             # rope at head_dim 32
    dict(bias=True),               # swiglu with biases
])
def test_config_rejections(bad):
    with pytest.raises(ValueError):
        get_config("llama-tiny").with_(**bad)


# ------------------------------------------------------------------------------------- model helpers
def _tiny(heads: int):
    cfg = get_config("llama-tiny").with_(num_heads=heads)
    C.PRESETS["_llama_t"] = cfg
    return cfg


def _batch(cfg, B=2, S=96, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.vocab_size, (B, S), generator=g)
    labels = ids.clone()
    labels[torch.rand(B, S, generator=g) < 0.2] = -100
    return ids, labels


def _run(model, ids, labels, **kw):
    model.zero_grad(set_to_none=True)
    loss = model(ids, labels=labels, **kw).loss
    loss.backward()
    return loss.item(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _assert_close(l1, g1, l2, g2):
    assert abs(l1 - l2) <= LOSS_TOL * abs(l1), (l1, l2)
    assert g1.keys() == g2.keys()
    for n in g1:
        err = (g1[n] - g2[n]).norm().item() / (g1[n].norm().item() + 1e-30)
        assert err <= GRAD_TOL, (n, err)


# ------------------------------------------------------------------------------------- against HF
@pytest.mark.parametrize("heads", [2, 1], ids=["D64", "D128"])
def test_reference_matches_hf_llama(heads):
    tf = pytest.importorskip("transformers")
    cfg = _tiny(heads)
    torch.manual_seed(1)
    hf = tf.LlamaForCausalLM(tf.LlamaConfig(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.ffn_size,
        num_hidden_layers=cfg.num_layers, num_attention_heads=heads, num_key_value_heads=heads,
        max_position_embeddings=cfg.max_positions, rms_norm_eps=cfg.ln_eps, rope_theta=cfg.rope_theta,
        hidden_act="silu", attention_bias=False, mlp_bias=False, tie_word_embeddings=False,
        attention_dropout=0.0, attn_implementation="eager")).float()
    hf.train()
    with torch.no_grad():      # HF initialises the norms to 1: give them something to get wrong
        for n, p in hf.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    model = build_model("_llama_t", impl="reference")
    missing = model.load_state_dict(from_hf_state_dict(hf.state_dict()), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.train()
    ids, labels = _batch(cfg)
    hf_loss = hf(input_ids=ids, labels=labels).loss
    hf_loss.backward()
    loss, grads = _run(model, ids, labels)
    assert abs(loss - hf_loss.item()) <= LOSS_TOL * abs(hf_loss.item()), (loss, hf_loss.item())
    ours_hf = to_hf_state_dict(grads)     # our gradients in HF's layout
    for n, p in hf.named_parameters():
        g = p.grad
        err = (ours_hf[n] - g).norm().item() / (g.norm().item() + 1e-30)
        assert err <= GRAD_TOL, (n, err)


# ------------------------------------------------------------------------------------- fused on the CPU
def _masks(B, S):
    right = torch.ones(B, S, dtype=torch.int64)
    right[0, S - 17:] = 0
    left = torch.ones(B, S, dtype=torch.int64)
    left[1, :23] = 0
    return {"right": right, "left": left}


def _segments(B, S):
    seg = torch.zeros(B, S, dtype=torch.int64)
    seg[0, :40], seg[0, 40:S - 9] = 1, 2                # two documents and 9 pads
    seg[1, :5], seg[1, 5:61], seg[1, 61:] = 1, 2, 3     # three documents, no pad
    return seg


@pytest.mark.parametrize("heads", [2, 1], ids=["D64", "D128"])
@pytest.mark.parametrize("mode", ["plain", "right", "left", "segments"])
def test_fused_cpu_matches_reference(heads, mode):
    cfg = _tiny(heads)
    ref = build_model("_llama_t", impl="reference", seed=3)
    fus = build_model("_llama_t", impl="fused", seed=3)
    fus.load_state_dict(ref.state_dict())
    with torch.no_grad():
        for m in (ref, fus):
            for n, p in m.named_parameters():
                if n.endswith("_g") or n == "final_ln.weight":
                    p.mul_(1 + 0.1 * torch.sin(torch.arange(p.numel(), dtype=torch.float32)))
    ids, labels = _batch(cfg, seed=2)
    kw = {}
    if mode in ("right", "left"):
        kw["attention_mask"] = _masks(*ids.shape)[mode]
    elif mode == "segments":
        kw["segment_ids"] = _segments(*ids.shape)
    _assert_close(*_run(ref, ids, labels, **kw), *_run(fus, ids, labels, **kw))


@pytest.mark.parametrize("impl", ["reference", "fused"])
def test_packed_loss_is_the_weighted_mean_of_its_documents(impl):
    """Rotary positions restart at each document: a packed row's loss equals the labelled-token
    weighted mean of its documents run on their own (each from position 0)."""
    from distributed_training_and_deepspeed_amd.data.packing import packed_causal_labels
    cfg = get_config("llama-tiny")
    model = build_model("llama-tiny", impl=impl, seed=5)
    model.eval()
    ids, _ = _batch(cfg, seed=4)
    seg = _segments(*ids.shape)
    labels = packed_causal_labels(ids, seg)
    with torch.no_grad():
        packed = model(ids, labels=labels, segment_ids=seg).loss.item()
        tot, cnt = 0.0, 0
        for b in range(ids.shape[0]):
            for d in seg[b].unique().tolist():
                if d == 0:
                    continue
                sel = seg[b] == d
                di, dl = ids[b][sel][None], labels[b][sel][None]
                n = int((dl[:, 1:] != -100).sum())
                if n == 0:
                    continue
                tot += model(di, labels=dl).loss.item() * n
                cnt += n
    assert abs(packed - tot / cnt) <= 1e-5 * abs(packed), (packed, tot / cnt)


# ------------------------------------------------------------------------------------- rotary embedding
@pytest.mark.parametrize("D", [64, 128])
def test_rope_properties_cpu(D):
    B, S, H = 2, 50, 3
    g = torch.Generator().manual_seed(0)
    table = Fx.rope_table(64, D, 10000.0)
    assert table.shape == (64, D // 2, 2) and table.dtype == torch.float32
    x = torch.randn(B * S, 3 * H * D, generator=g)
    y = torch.randn(B * S, 3 * H * D, generator=g)
    pos = torch.randint(0, 64, (B, S), generator=g, dtype=torch.int32)
    for p in (None, pos):
        rx = Fx.rope_(x.clone(), table, B, S, H, D, pos=p)
        assert torch.equal(rx[:, 2 * H * D:], x[:, 2 * H * D:])          # v untouched
        assert not torch.equal(rx[:, :2 * H * D], x[:, :2 * H * D])
        back = Fx.rope_(rx.clone(), table, B, S, H, D, pos=p, inverse=True)
        assert torch.allclose(back, x, rtol=1e-6, atol=1e-6)
        # the inverse is the adjoint: <rope(x), y> == <x, rope^-1(y)>
        lhs = (rx.double() * y.double()).sum().item()
        rhs = (x.double() * Fx.rope_(y.clone(), table, B, S, H, D, pos=p, inverse=True).double()).sum().item()
        assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs), 1.0)
    # HF's convention on one vector: position 1, pair (j, j + D/2) turns by theta^(-2j/D)
    one = torch.zeros(2, 3 * D)
    one[1, 3] = 1.0
    out = Fx.rope_(one, table, 1, 2, 1, D)
    ang = 10000.0 ** (-2 * 3 / D)
    assert abs(out[1, 3].item() - torch.cos(torch.tensor(ang)).item()) < 1e-6
    assert abs(out[1, 3 + D // 2].item() - torch.sin(torch.tensor(ang)).item()) < 1e-6
    with pytest.raises(ValueError):
        Fx.rope_(torch.zeros(65, 3 * D), table, 1, 65, 1, D)             # S > max_positions


def test_model_rejects_sequences_past_max_positions():
    cfg = get_config("llama-tiny").with_(max_positions=32)
    C.PRESETS["_llama_short"] = cfg
    for impl in ("reference", "fused"):
        model = build_model("_llama_short", impl=impl)
        with pytest.raises(ValueError):
            model(torch.zeros(1, 33, dtype=torch.int64))


# ------------------------------------------------------------------------------------- ops, CPU branch
def test_rms_and_swiglu_cpu_branches_match_autograd():
    torch.manual_seed(0)
    rows, h, f = 37, 48, 40
    y, r = torch.randn(rows, h), torch.randn(rows, h)
    gamma = 1 + 0.1 * torch.randn(h)
    dout, dout2, dext = torch.randn(rows, h), torch.randn(rows, h), torch.randn(rows, h)
    z, out, rstd = Fx.rms_fwd(y, r, gamma, 1e-6)
    zz = (y + r).requires_grad_()
    gg = gamma.clone().requires_grad_()
    ref = zz * torch.rsqrt(zz.pow(2).mean(-1, keepdim=True) + 1e-6) * gg
    assert torch.allclose(out, ref, atol=1e-6) and torch.equal(z, y + r)
    ref.backward(dout + dout2)
    dg = torch.zeros(h)
    dz = Fx.rms_bwd(dout, dext, z, rstd, gamma, dgamma=dg, dout2=dout2)
    assert torch.allclose(dz, zz.grad + dext, atol=1e-5) and torch.allclose(dg, gg.grad, atol=1e-5)
    assert Fx.rms_fwd(None, r, gamma, 1e-6)[0] is None
    gu = torch.randn(rows, 2 * f, requires_grad=True)
    a = Fx.swiglu_fwd(gu.detach())
    ref = torch.nn.functional.silu(gu[:, :f]) * gu[:, f:]
    assert torch.allclose(a, ref, atol=1e-6)
    da = torch.randn(rows, f)
    ref.backward(da)
    dgu, a2 = Fx.swiglu_bwd(da, gu.detach(), want_act=True)
    assert torch.allclose(dgu, gu.grad, atol=1e-5) and torch.equal(a, a2)


# ------------------------------------------------------------------------------------- HF conversion
def test_hf_state_dict_round_trip_is_exact():
    model = build_model("llama-tiny", seed=9)
    sd = model.state_dict()
    hf = to_hf_state_dict(sd)
    assert "model.layers.1.self_attn.k_proj.weight" in hf and "model.layers.0.mlp.up_proj.weight" in hf
    assert hf["model.layers.0.self_attn.q_proj.weight"].shape == (128, 128)
    assert hf["model.layers.0.mlp.gate_proj.weight"].shape == (384, 128)
    back = from_hf_state_dict(hf)
    assert back.keys() == sd.keys()
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    again = to_hf_state_dict(back)
    assert again.keys() == hf.keys() and all(torch.equal(again[k], hf[k]) for k in hf)


# ------------------------------------------------------------------------------------- ZeRO over gloo
def _param_vector(res, world):
    vals = []
    for unit, numel, chunk, off, shapes in res["layout"]:
        full = torch.cat([res["shards"][r][off:off + chunk] for r in range(world)])
        o = 0
        for shp in shapes:
            n = 1
            for d in shp:
                n *= d
            vals.append((tuple(shp), full[o:o + n].clone()))
            o += -(-n // 64) * 64
    vals.sort(key=lambda t: (t[0], t[1].sum().item()))
    return vals


@pytest.mark.parametrize("head_loss", ["logits", "fused"])
def test_zero_stages_agree_llama(tmp_path, monkeypatch, head_loss):
    """tests/test_distributed_cpu.py::test_zero_stages_agree for the Llama family (untied head as a
    replicated persistent parameter): stages 0-3 at world 2 leave the same parameters after two
    steps as each other and as one process that accumulates the two ranks' micro-batches."""
    monkeypatch.setenv("DTD_HEAD_XENT", "1" if head_loss == "fused" else "0")   # read by the workers' Runtime
    world, steps = 2, 2
    results = {}
    for stage in (0, 1, 2, 3):
        mp.spawn(W.zero_worker, args=(world, pick_free_port(), str(tmp_path), "llama-tiny", stage, steps, 1),
                 nprocs=world, join=True)
        results[stage] = _param_vector(torch.load(tmp_path / f"zero{stage}.pt", weights_only=True),
                                       1 if stage == 0 else world)
    # one process, stage 0, two accumulated micro-batches per step: the same samples in the same order
    mp.spawn(W.zero_worker, args=(1, pick_free_port(), str(tmp_path), "llama-tiny", 0, steps, 2, 0.0, "_single"),
             nprocs=1, join=True)
    results["single"] = _param_vector(torch.load(tmp_path / "zero0_single.pt", weights_only=True), 1)
    ref = results[0]
    assert sum(v.numel() for _, v in ref) == count_parameters(build_model("llama-tiny"))
    for key in (1, 2, 3, "single"):
        got = results[key]
        assert len(got) == len(ref)
        for (s1, a), (s2, b) in zip(ref, got):
            assert s1 == s2
            assert torch.allclose(a, b, atol=3e-5, rtol=1e-4), (key, s1, (a - b).abs().max().item())
