"""Float64 oracles and input regimes for the mixture-of-experts FFN (models/moe.py), by the rules of
tests/oracles.py: inputs are upcast exactly to fp64, the forward is built from torch / numpy operators with the
selection, tie and slot rules written here as sorts (nothing shared with models/moe.py), and every gradient
comes from ``torch.autograd.grad``.

Rules: the k largest stored logits are selected, rank 0 the largest, a tie to the lower expert index; expert e's
slots are taken by its (token, rank) pairs in order of rank first, then token index; pairs past the capacity C
are dropped.  ``higher_tie`` and ``token_major`` build the two wrong variants the tests must be able to tell
from the right one.
"""
import numpy as np
import torch
import torch.nn.functional as F

from .oracles import BF16, F32, _leaf, _randn, f64, saturated

__all__ = ["BF16", "F32", "REGIMES", "logits_for", "route", "moe_ffn", "capacity"]


def capacity(T, E, k, cf):
    """C = T when cf == 0, else min(T, 8 ceil(cf T k / (8 E)))."""
    if cf == 0:
        return T
    return max(1, min(T, 8 * int(np.ceil(cf * T * k / (8 * E)))))


# ------------------------------------------------------------------------------------------ regimes
def gauss(T, E, dtype, seed):
    return _randn(T, E, seed).to(dtype)


def ties(T, E, dtype, seed):
    """Eight distinct bf16 values: every row of more than 8 experts has ties, most rows of fewer do."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.0])
    return vals[torch.randint(0, 8, (T, E), generator=g)].to(BF16).to(dtype)


def overflow(T, E, dtype, seed):
    """Every token prefers expert 0: it is the first choice of the even tokens and the second choice of the odd
    ones (another expert, cycling with the token, lies above it), so expert 0 is asked for by T pairs of both
    ranks -- which pairs it keeps depends on the order in which its slots are filled."""
    x = _randn(T, E, seed)
    x[:, 0] = x.abs().amax(-1) + 1.0 + x[:, 0].abs()
    if E > 1:
        odd = torch.arange(1, T, 2)
        x[odd, 1 + odd % (E - 1)] = x[odd, 0] + 1.0
    return x.to(dtype)


def saturating(T, E, dtype, seed):
    """+-20, +-90, +-200 and 1e30 among ordinary logits (tests/oracles.py::saturated)."""
    return saturated(T, E, dtype, seed)


REGIMES = {"gauss": gauss, "ties": ties, "overflow": overflow, "saturating": saturating}


def logits_for(regime, T, E, dtype, seed=0):
    return REGIMES[regime](T, E, dtype, seed)


# ------------------------------------------------------------------------------------------ routing
def _select(l64, k, higher_tie=False):
    T, E = l64.shape
    a = l64.numpy()
    col = np.broadcast_to(np.arange(E), (T, E))
    # last key is the primary one: value descending, then expert index (ascending: the rule)
    order = np.lexsort((-col if higher_tie else col, -a), axis=-1)
    return torch.from_numpy(np.ascontiguousarray(order[:, :k])).long()


def _slots(idx, E, C, token_major=False):
    T, k = idx.shape
    t = np.repeat(np.arange(T), k)
    r = np.tile(np.arange(k), T)
    e = idx.numpy().reshape(-1)
    # pairs sorted by expert, then rank, then token (the rule) -- or expert, token, rank (the wrong variant)
    order = np.lexsort((r, t, e)) if token_major else np.lexsort((t, r, e))
    es = e[order]
    start = np.searchsorted(es, np.arange(E), side="left")
    pos = np.arange(T * k) - start[es]
    token_slot = np.full(T * k, -1, dtype=np.int64)
    slot_src = np.full(E * C, -1, dtype=np.int64)
    keep = pos < C
    pair = (t * k + r)[order]
    token_slot[pair[keep]] = es[keep] * C + pos[keep]
    slot_src[es[keep] * C + pos[keep]] = pair[keep]
    return torch.from_numpy(token_slot).view(T, k), torch.from_numpy(slot_src)


def route(logits, k, C, higher_tie=False, token_major=False):
    """dict topk_idx [T, k], token_slot [T, k], slot_src [E C] (int64), topk_w [T, k], frac [k, E],
    prob_mean [E] (fp64), aux = E sum frac * prob_mean."""
    l = f64(logits)
    T, E = l.shape
    idx = _select(l, k, higher_tie)
    token_slot, slot_src = _slots(idx, E, C, token_major)
    w = torch.softmax(l.gather(1, idx), -1)
    frac = F.one_hot(idx, E).sum(0).to(torch.float64) / T
    pm = torch.softmax(l, -1).mean(0)
    return dict(topk_idx=idx, token_slot=token_slot, slot_src=slot_src, topk_w=w, frac=frac, prob_mean=pm,
                aux=E * (frac * pm[None]).sum())


# ------------------------------------------------------------------------------------ the whole block
def _valid(i, n):
    i = i.detach().cpu().long()
    return (i >= 0) & (i < n), i.clamp(0, max(n - 1, 0))


def _gather64(x64, slot_src, k):
    ok, p = _valid(slot_src, x64.shape[0] * k)
    return x64[p // k] * ok[:, None].to(x64.dtype)


def _combine64(rows64, token_slot, w64, res64):
    T, k = token_slot.shape
    out = torch.zeros((T, rows64.shape[1]), dtype=torch.float64) if res64 is None else res64
    for r in range(k):
        ok, s = _valid(token_slot[:, r], rows64.shape[0])
        out = out + rows64[s] * ok[:, None].to(torch.float64) * w64[:, r, None]
    return out


def moe_ffn(x, logits, gu_w, down_w, k, C, dout, aux_scale=0.0, res=None):
    """out = res + sum_r w_r FFN_{e_r}(x), aux, and the gradients of sum(out * dout) + aux_scale * aux for x,
    logits, gu_w [E, 2f, h] and down_w [E, h, f]; sc_dgu_w / sc_ddown_w: each weight-gradient element's sum of
    the sizes of its summands.  sc_dlogits [T]: a row of dlogits is a difference that can cancel altogether
    (dlogits[t, e_r] = w_r (dw_r - sum_r' w_r' dw_r') with dw_r a dot product of size S_r = sum |dout| |ye|, plus
    p_e (g_e - sum p g) with g_e = aux_scale E sum_r frac[r, e] / T, nearly constant under a balanced router),
    so its scale is the size of the summands: max_r w_r (S_r + sum w S) + max_e p_e (|g_e| + sum p |g|)."""
    xl, ll, gl, dl = _leaf(x), _leaf(logits), _leaf(gu_w), _leaf(down_w)
    T, E = ll.shape
    f = dl.shape[2]
    rt = route(logits, k, C)
    idx = rt["topk_idx"]
    w = torch.softmax(ll.gather(1, idx), -1)
    xe = _gather64(xl, rt["slot_src"], k).view(E, C, -1)
    gu = torch.bmm(xe, gl.transpose(1, 2))
    a = F.silu(gu[..., :f]) * gu[..., f:]
    ye = torch.bmm(a, dl.transpose(1, 2))
    out = _combine64(ye.reshape(E * C, -1), rt["token_slot"], w, f64(res))
    aux = E * (rt["frac"] * torch.softmax(ll, -1).mean(0)[None]).sum()
    d64 = f64(dout)
    dx, dlog, dgw, ddw, dgu, dye = torch.autograd.grad((out * d64).sum() + float(aux_scale) * aux,
                                                       (xl, ll, gl, dl, gu, ye))
    with torch.no_grad():
        sc_g = torch.bmm(dgu.abs().transpose(1, 2), xe.abs())
        sc_d = torch.bmm(dye.abs().transpose(1, 2), a.abs())
        yf = ye.reshape(E * C, -1).abs()
        S = []
        for r in range(k):
            ok, s = _valid(rt["token_slot"][:, r], E * C)
            S.append((d64.abs() * yf[s]).sum(-1) * ok.to(torch.float64))
        S = torch.stack(S, -1)
        p = torch.softmax(ll, -1)
        g = (float(aux_scale) * E / T * rt["frac"].sum(0)).abs()[None]
        sc_l = (w * (S + (w * S).sum(-1, keepdim=True))).amax(-1) + (p * (g + (p * g).sum(-1, keepdim=True))).amax(-1)
    return dict(out=out.detach(), aux=aux.detach(), dx=dx, dlogits=dlog, dgu_w=dgw, ddown_w=ddw, sc_dgu_w=sc_g,
                sc_ddown_w=sc_d, sc_dlogits=sc_l, routing=rt)
