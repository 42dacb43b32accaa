"""Timings of the sliding-window flash-attention kernels (ops/csrc/attention.hip, the *_win_kernel forms)
against the unwindowed grouped-query kernels on the same tensors.

Per shape (causal, bf16) and window, and per pass -- forward, dQ, dK/dV (the two backward kernels priced
separately through ``set_bwd_kernels``) -- the windowed call (a) and the unwindowed call (b), interleaved
b a b a in one process; |b1 - b2| is the run's own noise floor.  Next to the time ratio stands the share
of (query block, key tile) pairs -- (key block, query tile) pairs for dK/dV -- that the windowed kernel
visits, computed from its loop bounds: what the ratio would be if a tile cost the same in both.

Where ``--gqa-record`` (default profiles/attn_gqa.jsonl) holds the unwindowed kernels' times for a
shape, they are reported beside this run's: the unwindowed kernels' code does not depend on the window,
so the two should agree within that file's own run-to-run spread.

One JSON line per (shape, window, pass), appended to --out.

Usage: python scripts/bench_attn_window.py [--iters K] [--out profiles/attn_window.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_training_and_deepspeed_amd.ops import attention as A  # noqa: E402

SHAPES = (
    # name, H, Hkv, D, B, S, windows
    ("Mistral-7B", 32, 8, 128, 2, 8192, (4096, 1024)),
    ("TinyLlama", 32, 4, 64, 8, 2048, (512,)),
)
BN = 64                               # keys per tile of the forward and dQ


def tile_share(S: int, W: int, D: int) -> dict:
    """Tiles visited with the window over tiles visited without, per pass (the kernels' loop bounds)."""
    def fwd(w):
        n = 0
        for qblk in range(0, S, 128):
            t0 = max(qblk - w + 1, 0) // BN if w else 0
            n += -(-min(S, qblk + 128) // BN) - t0
        return n
    bm = 128 if D == 64 else 64       # query rows per tile of dK/dV

    def dkdv(w):
        n = 0
        for kblk in range(0, S, 128):
            qstart = (kblk // bm) * bm
            qend = min(S, kblk + 127 + w) if w else S
            n += -(-(qend - qstart) // bm)
        return n
    f = fwd(W) / fwd(0)
    return {"fwd": round(f, 4), "dq": round(f, 4), "dkdv": round(dkdv(W) / dkdv(0), 4)}


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


def baba(win, full, iters):
    b1 = timeit(full, iters)
    a1 = timeit(win, iters)
    b2 = timeit(full, iters)
    a2 = timeit(win, iters)
    return (a1, a2), (b1, b2)


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def gqa_record(path):
    """{(B, S, H, Hkv, D, pass): record} of the grouped-query benchmark's file, if it is there."""
    out = {}
    if path and os.path.exists(path):
        with open(path) as f:
            for line in f:
                r = json.loads(line)
                if r.get("case") == "attn_gqa":
                    out[(r["B"], r["S"], r["H"], r["Hkv"], r["D"], r["pass"])] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--gqa-record", type=str, default=os.path.join(ROOT, "profiles", "attn_gqa.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_window.py needs a GPU")
    dev, dt, it = "cuda", torch.bfloat16, args.iters
    before = gqa_record(args.gqa_record)
    torch.manual_seed(0)
    for name, H, Hkv, D, B, S, windows in SHAPES:
        T = B * S
        qkv = torch.randn(T, (H + 2 * Hkv) * D, device=dev, dtype=dt)
        dctx = torch.randn(T, H * D, device=dev, dtype=dt)
        ctx_f, lse_f, _ = A.attn_fwd(qkv, B, S, H, D, True, kv_heads=Hkv)
        A.attn_bwd(dctx, qkv, ctx_f, lse_f, B, S, H, D, True, kv_heads=Hkv)      # (also leaves delta behind)
        for W in windows:
            shape = {"model": name, "B": B, "S": S, "H": H, "Hkv": Hkv, "D": D, "causal": True, "window": W}
            share = tile_share(S, W, D)
            ctx_w, lse_w, _ = A.attn_fwd(qkv, B, S, H, D, True, kv_heads=Hkv, window=W)
            A.attn_bwd(dctx, qkv, ctx_w, lse_w, B, S, H, D, True, kv_heads=Hkv, window=W)

            def rec(pass_, res):
                (a1, a2), (b1, b2) = res
                a, b = (a1 + a2) / 2, (b1 + b2) / 2
                r = {"case": "attn_window", **shape, "pass": pass_, "window_us": round(a, 1),
                     "window_runs_us": [round(a1, 1), round(a2, 1)], "full_us": round(b, 1),
                     "full_runs_us": [round(b1, 1), round(b2, 1)], "noise_us": round(abs(b1 - b2), 1),
                     "window_over_full": round(a / b, 3), "tile_share": share[pass_]}
                old = before.get((B, S, H, Hkv, D, pass_))
                if old is not None:
                    r["full_us_gqa_record"] = old["gqa_us"]
                    r["full_runs_us_gqa_record"] = old["gqa_runs_us"]
                emit(args.out, r)

            rec("fwd", baba(lambda: A.attn_fwd(qkv, B, S, H, D, True, kv_heads=Hkv, window=W),
                            lambda: A.attn_fwd(qkv, B, S, H, D, True, kv_heads=Hkv), it))
            for pass_, sel in (("dq", (True, False)), ("dkdv", (False, True))):
                old = A.set_bwd_kernels(*sel)
                try:
                    rec(pass_, baba(lambda: A.attn_bwd(dctx, qkv, ctx_w, lse_w, B, S, H, D, True, kv_heads=Hkv, window=W),
                                    lambda: A.attn_bwd(dctx, qkv, ctx_f, lse_f, B, S, H, D, True, kv_heads=Hkv), it))
                finally:
                    A.set_bwd_kernels(*old)
        del qkv, dctx, ctx_f, ctx_w


if __name__ == "__main__":
    main()
