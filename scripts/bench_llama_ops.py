"""Timings of the Llama-family kernels (ops/csrc/rmsnorm.hip, rope.hip, swiglu.hip), each interleaved
in the same process with the existing kernel that moves the same [T, h] tensors:

  rms fwd   z = r + y, out = RMS(z)        vs  ln_fwd(y, r, p = 0, store_z)      read 2, write 2
  rms bwd   dz from dout, z (+ dgamma)     vs  ln_bwd(dout, z; dgamma, dbeta)    read 2, write 1
  rope      q, k of [T, 3*H*D] in place                                          read + write 2/3 of qkv
  swiglu    fwd gu [T, 2f] -> a [T, f]     vs  act_fwd over [T, 2f]              (gelu_tanh moves 4 T f)
            bwd da, gu -> dgu              vs  act_bwd over [T, 2f]

Every pair is run A B A B: the two repeats of the existing kernel give the run's own spread.  The bar for
RMSNorm is LayerNorm's mean time at the shape plus that spread (RMSNorm moves the same tensors minus
beta and the mean); each line records both kernels' times, the spread and ``meets_bar``.

Prints one JSON line per case (us per call, effective TB/s from the tensors read + written) and, with
--out, appends them to a file.  Usage: python scripts/bench_llama_ops.py [--iters K] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_training_and_deepspeed_amd.ops import functional as Fx
from distributed_training_and_deepspeed_amd.ops.rng import RngState


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def abab(new, old, iters):
    """old, new, old, new -> (new mean us, old mean us, spread of the two old repeats)."""
    o1 = timeit(old, iters)
    n1 = timeit(new, iters)
    o2 = timeit(old, iters)
    n2 = timeit(new, iters)
    return (n1 + n2) / 2, (o1 + o2) / 2, abs(o1 - o2), (n1, n2), (o1, o2)


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def pair_record(case, shape, new_name, old_name, res, new_bytes, old_bytes, bar: bool):
    n, o, spread, ns, os_ = res
    rec = {"case": case, "shape": shape, f"{new_name}_us": round(n, 1), f"{new_name}_runs_us": [round(v, 1) for v in ns],
           f"{new_name}_tb_s": round(new_bytes / n / 1e6, 2), f"{old_name}_us": round(o, 1),
           f"{old_name}_runs_us": [round(v, 1) for v in os_], f"{old_name}_tb_s": round(old_bytes / o / 1e6, 2),
           f"{old_name}_spread_us": round(spread, 1)}
    if bar:
        rec["bar_us"] = round(o + spread, 1)
        rec["meets_bar"] = bool(n <= o + spread)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_llama_ops.py needs a GPU")
    dev, dt = "cuda", torch.bfloat16
    torch.manual_seed(0)
    rng = RngState(seed=1, device=dev)
    it = args.iters

    for R, h in ((131072, 768), (16384, 4096)):
        y, r, dout = (torch.randn(R, h, device=dev, dtype=dt) for _ in range(3))
        gamma = (1 + 0.1 * torch.randn(h, device=dev)).to(dt)
        beta = (0.1 * torch.randn(h, device=dev)).to(dt)
        tb = R * h * 2
        res = abab(lambda: Fx.rms_fwd(y, r, gamma, 1e-5),
                   lambda: Fx.ln_fwd(y, r, gamma, beta, 1e-5, 0.0, rng, 5, store_z=True), it)
        emit(args.out, pair_record("rms_fwd", [R, h], "rms", "ln", res, 4 * tb, 4 * tb, True))
        z, _, rs = Fx.rms_fwd(y, r, gamma, 1e-5)
        zl, _, m, rl = Fx.ln_fwd(y, r, gamma, beta, 1e-5, 0.0, rng, 5, store_z=True)
        dg, db = torch.zeros(h, device=dev), torch.zeros(h, device=dev)
        res = abab(lambda: Fx.rms_bwd(dout, None, z, rs, gamma, dgamma=dg),
                   lambda: Fx.ln_bwd(dout, None, zl, m, rl, gamma, 0.0, rng, 5, want_dz=True, want_dy=False,
                                     dgamma=dg, dbeta=db), it)
        emit(args.out, pair_record("rms_bwd", [R, h], "rms", "ln", res, 3 * tb, 3 * tb, True))
        del y, r, dout, z, zl

    B, S, H, D = 8, 2048, 32, 128
    qkv = torch.randn(B * S, 3 * H * D, device=dev, dtype=dt)
    table = Fx.rope_table(4096, D, 10000.0, device=dev)
    us = timeit(lambda: Fx.rope_(qkv, table, B, S, H, D), it)
    us2 = timeit(lambda: Fx.rope_(qkv, table, B, S, H, D), it)
    nbytes = 2 * (B * S * 2 * H * D * 2)      # q and k read and written
    emit(args.out, {"case": "rope", "shape": [B * S, H, D], "us": round((us + us2) / 2, 1),
                    "runs_us": [round(us, 1), round(us2, 1)], "tb_s": round(nbytes / ((us + us2) / 2) / 1e6, 2)})
    del qkv

    R, f = 16384, 11008
    gu = torch.randn(R, 2 * f, device=dev, dtype=dt)
    da = torch.randn(R, f, device=dev, dtype=dt)
    dgu_like = torch.randn(R, 2 * f, device=dev, dtype=dt)
    tf = R * f * 2
    res = abab(lambda: Fx.swiglu_fwd(gu), lambda: Fx.act_fwd(gu, "gelu_tanh"), it)
    emit(args.out, pair_record("swiglu_fwd", [R, f], "swiglu", "act", res, 3 * tf, 4 * tf, False))
    res = abab(lambda: Fx.swiglu_bwd(da, gu), lambda: Fx.act_bwd(dgu_like, gu, "gelu_tanh"), it)
    emit(args.out, pair_record("swiglu_bwd", [R, f], "swiglu", "act", res, 5 * tf, 6 * tf, False))
    res = abab(lambda: Fx.swiglu_bwd(da, gu, want_act=True),
               lambda: Fx.act_bwd(dgu_like, gu, "gelu_tanh", want_act=True), it)
    emit(args.out, pair_record("swiglu_bwd_recompute", [R, f], "swiglu", "act", res, 6 * tf, 8 * tf, False))


if __name__ == "__main__":
    main()
