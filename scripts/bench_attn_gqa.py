"""Timings of the grouped-query flash-attention kernels (ops/csrc/attention.hip, the *_gqa_kernel forms)
against what a model without them has to do: expand K / V to the H query heads in memory, run the
multi-head kernels at the same H, and sum dK / dV over each group afterwards.

Per shape (causal, bf16, B * S = 16384 tokens) and per pass -- forward, dQ, dK/dV (the two backward
kernels priced separately through ``set_bwd_kernels``) -- three timings, interleaved b a c a in one process:

  (a) the GQA kernels on qkv [T, (H + 2 Hkv) D];
  (b) the multi-head kernels on the pre-expanded qkv [T, 3 H D];
  (c) (b) a second time: |b - c| is the run's own noise floor.

The expansion (qkv -> the multi-head layout) and the dK / dV group sum are timed on their own: they are
what (b) costs on top in a real step.  One JSON line per (shape, pass), appended to --out.

Usage: python scripts/bench_attn_gqa.py [--iters K] [--out profiles/attn_gqa.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_training_and_deepspeed_amd.ops import attention as A

SHAPES = (
    # name, H, Hkv, D, S
    ("TinyLlama", 32, 4, 64, 2048),
    ("Llama-3-8B", 32, 8, 128, 4096),
)
TOKENS = 16384


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


def baca(gqa, mha, iters):
    """mha, gqa, mha, gqa -> (a runs, b, c)."""
    b = timeit(mha, iters)
    a1 = timeit(gqa, iters)
    c = timeit(mha, iters)
    a2 = timeit(gqa, iters)
    return (a1, a2), b, c


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def expand(qkv, T, H, Hkv, D):
    x = qkv.view(T, H + 2 * Hkv, D)
    G = H // Hkv
    return torch.cat([x[:, :H], x[:, H:H + Hkv].repeat_interleave(G, 1), x[:, H + Hkv:].repeat_interleave(G, 1)],
                     1).reshape(T, 3 * H * D)


def group_sum(dqkv, T, H, Hkv, D):
    x = dqkv.view(T, 3, H, D)
    G = H // Hkv
    return torch.cat([x[:, 0], x[:, 1].reshape(T, Hkv, G, D).float().sum(2).to(x.dtype),
                      x[:, 2].reshape(T, Hkv, G, D).float().sum(2).to(x.dtype)], 1).reshape(T, (H + 2 * Hkv) * D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_gqa.py needs a GPU")
    dev, dt, it = "cuda", torch.bfloat16, args.iters
    torch.manual_seed(0)
    for name, H, Hkv, D, S in SHAPES:
        B = TOKENS // S
        T = B * S
        shape = {"model": name, "B": B, "S": S, "H": H, "Hkv": Hkv, "D": D, "causal": True}
        qkv = torch.randn(T, (H + 2 * Hkv) * D, device=dev, dtype=dt)
        big = expand(qkv, T, H, Hkv, D)
        dctx = torch.randn(T, H * D, device=dev, dtype=dt)
        ctx_g, lse_g, _ = A.attn_fwd(qkv, B, S, H, D, True, kv_heads=Hkv)
        ctx_m, lse_m, _ = A.attn_fwd(big, B, S, H, D, True)
        dbig = A.attn_bwd(dctx, big, ctx_m, lse_m, B, S, H, D, True)      # (also leaves delta behind)
        A.attn_bwd(dctx, qkv, ctx_g, lse_g, B, S, H, D, True, kv_heads=Hkv)

        def rec(pass_, res):
            (a1, a2), b, c = res
            a = (a1 + a2) / 2
            emit(args.out, {"case": "attn_gqa", **shape, "pass": pass_, "gqa_us": round(a, 1),
                            "gqa_runs_us": [round(a1, 1), round(a2, 1)], "mha_expanded_us": round(b, 1),
                            "mha_expanded_again_us": round(c, 1), "noise_us": round(abs(b - c), 1),
                            "gqa_over_mha": round(a / ((b + c) / 2), 3)})

        rec("fwd", baca(lambda: A.attn_fwd(qkv, B, S, H, D, True, kv_heads=Hkv),
                        lambda: A.attn_fwd(big, B, S, H, D, True), it))
        for pass_, sel in (("dq", (True, False)), ("dkdv", (False, True))):
            old = A.set_bwd_kernels(*sel)
            try:
                rec(pass_, baca(lambda: A.attn_bwd(dctx, qkv, ctx_g, lse_g, B, S, H, D, True, kv_heads=Hkv),
                                lambda: A.attn_bwd(dctx, big, ctx_m, lse_m, B, S, H, D, True), it))
            finally:
                A.set_bwd_kernels(*old)
        e1, e2 = timeit(lambda: expand(qkv, T, H, Hkv, D), it), timeit(lambda: expand(qkv, T, H, Hkv, D), it)
        s1, s2 = timeit(lambda: group_sum(dbig, T, H, Hkv, D), it), timeit(lambda: group_sum(dbig, T, H, Hkv, D), it)
        emit(args.out, {"case": "attn_gqa_extras", **shape, "expand_kv_us": round((e1 + e2) / 2, 1),
                        "expand_kv_runs_us": [round(e1, 1), round(e2, 1)], "group_sum_us": round((s1 + s2) / 2, 1),
                        "group_sum_runs_us": [round(s1, 1), round(s2, 1)]})
        del qkv, big, dctx, dbig, ctx_g, ctx_m


if __name__ == "__main__":
    main()
