"""The decode step's projections, M in {1, 8, 64} rows: ``F.linear`` on bf16 (the library; what the dispatch runs
with the skinny kernel off) against ``ops.gemm.linear_skinny`` on bf16 weights and on FP8 codes, and ``ops.gemm.linear_skinny_mx4`` on MXFP4 codes.

Shapes: the four projections and the LM head of llama-160m, TinyLlama-1.1B and Llama-2-7B, the four
projections of Llama-3-8B.  The four arms alternate in one process, two repeats each; a repeat is ``--iters``
calls between two device events after ``--warmup`` calls, each call on the next of several copies of the
weight -- enough copies to exceed 512 MiB, so no call finds its weight in the L2 / MALL that the call before
left (the MXFP4 arm has twice the copies: its weight is half the size) -- which is what a decode step sees, with 12.9 GB of other weights between two uses of one.  Reported
per arm: us per call (mean of the two repeats, and both) and TB/s of weight bytes (2 N K, N K + 4 N, or N K / 2 + N K / 32).
"Faster" needs more than the spread of the yardstick's two repeats: ``beats_library``, and for MXFP4 against the
FP8 arm ``skinny_mx4_beats_fp8``.

One JSON line per (product, M), appended to --out.

Usage: python scripts/bench_gemm_skinny.py [--out profiles/gemm_skinny.jsonl] [--models llama-160m,...]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_training_and_deepspeed_amd.models.config import get_config  # noqa: E402
from distributed_training_and_deepspeed_amd.ops import gemm as G  # noqa: E402
from distributed_training_and_deepspeed_amd.ops.quant import quantize_weight_fp8, quantize_weight_mx4  # noqa: E402

MODELS = ("llama-160m", "tinyllama-1.1b", "llama-2-7b", "llama-3-8b")
FLUSH_BYTES = 512 << 20


def products(cfg, head):
    h, f = cfg.hidden_size, cfg.ffn_size
    out = [("qkv_w", (cfg.num_heads + 2 * cfg.kv_heads) * cfg.head_dim, h), ("o_w", h, h), ("gu_w", 2 * f, h),
           ("down_w", h, f)]
    return out + [("head", cfg.vocab_size, h)] if head else out


def timed(fn, copies, warmup, iters):
    for i in range(warmup):
        fn(i % copies)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i % copies)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--models", type=str, default=",".join(MODELS))
    ap.add_argument("--rows", type=str, default="1,8,64")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_skinny.py needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in args.models.split(","):
        cfg = get_config(name)
        for what, N, K in products(cfg, head=cfg.vocab_size <= 65536):
            copies = max(2, -(-FLUSH_BYTES // (N * K)))        # the FP8 copies alone exceed the flush size
            w1 = torch.randn(N, K, device="cuda", generator=g) * 0.02
            codes1, scale = quantize_weight_fp8(w1)
            mx1, mxs1 = quantize_weight_mx4(w1)
            w = [w1.bfloat16().clone() for _ in range(copies)]
            codes = [codes1.clone() for _ in range(copies)]
            mx = [(mx1.clone(), mxs1.clone()) for _ in range(2 * copies)]
            del w1, codes1, mx1, mxs1
            for M in (int(m) for m in args.rows.split(",")):
                x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
                y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
                arms = {"library_bf16": lambda i: F.linear(x, w[i]),
                        "skinny_bf16": lambda i: G.linear_skinny(x, w[i], out=y),
                        "skinny_fp8": lambda i: G.linear_skinny(x, codes[i], scale, out=y),
                        "skinny_mx4": lambda i: G.linear_skinny_mx4(x, *mx[i], out=y)}
                ncopies = {k: 2 * copies if k == "skinny_mx4" else copies for k in arms}
                err = float((G.linear_skinny(x, w[0]).float() - F.linear(x, w[0]).float()).abs().max())
                runs = {k: [] for k in arms}
                for _ in range(2):
                    for k, fn in arms.items():
                        runs[k].append(timed(fn, ncopies[k], args.warmup, args.iters))
                rec = {"case": "gemm_skinny", "model": cfg.name, "product": what, "M": M, "N": N, "K": K,
                       "weight_copies": copies, "iters": args.iters, "max_abs_diff_skinny_vs_library_bf16": err}
                for k, r in runs.items():
                    us = sum(r) / 2
                    nbytes = {"skinny_fp8": N * K + 4 * N, "skinny_mx4": N * K // 2 + N * K // 32}.get(k, 2 * N * K)
                    rec[f"{k}_us"] = round(us, 2)
                    rec[f"{k}_runs_us"] = [round(v, 2) for v in r]
                    rec[f"{k}_weight_TBps"] = round(nbytes / us * 1e-6, 3)
                lib = runs["library_bf16"]
                spread = abs(lib[0] - lib[1])
                for k in ("skinny_bf16", "skinny_fp8", "skinny_mx4"):
                    rec[f"{k}_beats_library"] = bool(max(runs[k]) < min(lib) - spread)
                fp8 = runs["skinny_fp8"]
                rec["skinny_mx4_beats_fp8"] = bool(max(runs["skinny_mx4"]) < min(fp8) - abs(fp8[0] - fp8[1]))
                line = json.dumps(rec)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")
            del w, codes, mx
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
