"""The projections of a prompt pass, M in {96, 128, 512, 2048, 8192} rows: ``ops.gemm.linear_any`` on the bf16 parameter
(what a quantised model ran before FP8 activations, and still runs with them off) against ``ops.gemm.linear_w8a8`` on the
FP8 codes -- timed once whole (the quantising kernel, then the FP8 GEMM) and once without its quantiser
(``ops.gemm.linear_fp8`` on codes made beforehand).

Shapes: the four projections of TinyLlama-1.1B, Llama-2-7B and Llama-3-8B.  The three arms alternate in one process, two
repeats each; a repeat is ``--iters`` calls between two device events after ``--warmup`` calls, each call on the next of
several copies of the weight (enough to exceed 256 MiB in codes, so no call finds its weight where the call before left
it).  Reported per arm: us per call (mean of the two repeats, and both) and TFLOP/s (2 M N K over the time); per FP8
arm the ratio library time / arm time, and ``*_beats_library``: faster by more than the spread of the library's two
repeats.  ``max_abs_diff`` is the FP8 path against the library's product: the activation quantisation, not an error of
the kernel (tests/test_gemm_fp8_gpu.py bounds that).

One JSON line per (product, M), appended to --out.

Usage: python scripts/bench_gemm_fp8.py [--out profiles/gemm_fp8.jsonl] [--models tinyllama-1.1b,...] [--rows 96,...]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_training_and_deepspeed_amd.models.config import get_config  # noqa: E402
from distributed_training_and_deepspeed_amd.ops import functional as Fx  # noqa: E402
from distributed_training_and_deepspeed_amd.ops import gemm as G  # noqa: E402
from distributed_training_and_deepspeed_amd.ops.quant import dequantize_weight, quantize_weight_fp8  # noqa: E402

MODELS = ("tinyllama-1.1b", "llama-2-7b", "llama-3-8b")
FLUSH_BYTES = 256 << 20


def products(cfg):
    h, f = cfg.hidden_size, cfg.ffn_size
    return [("qkv_w", (cfg.num_heads + 2 * cfg.kv_heads) * cfg.head_dim, h), ("o_w", h, h), ("gu_w", 2 * f, h),
            ("down_w", h, f)]


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
    ap.add_argument("--rows", type=str, default="96,128,512,2048,8192")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_fp8.py needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in args.models.split(","):
        cfg = get_config(name)
        for what, N, K in products(cfg):
            copies = max(2, -(-FLUSH_BYTES // (N * K)))
            codes1, scale = quantize_weight_fp8(torch.randn(N, K, device="cuda", generator=g) * 0.02)
            w = [dequantize_weight(codes1, scale) for _ in range(copies)]      # the parameter of a quantised model
            codes = [codes1.clone() for _ in range(copies)]
            del codes1
            for M in (int(m) for m in args.rows.split(",")):
                x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
                y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
                xc, xs = Fx.act_quant_fp8(x)
                arms = {"library_bf16": lambda i: G.linear_any(x, w[i]),
                        "w8a8": lambda i: G.linear_w8a8(x, codes[i], scale, out=y),
                        "fp8_gemm": lambda i: G.linear_fp8(xc, xs, codes[i], scale, out=y)}
                ref = G.linear_any(x, w[0]).float()
                err = float((G.linear_w8a8(x, codes[0], scale).float() - ref).abs().max())
                runs = {k: [] for k in arms}
                for _ in range(2):
                    for k, fn in arms.items():
                        runs[k].append(timed(fn, copies, args.warmup, args.iters))
                rec = {"case": "gemm_fp8", "model": cfg.name, "product": what, "M": M, "N": N, "K": K,
                       "weight_copies": copies, "iters": args.iters, "max_abs_diff": err, "max_abs_ref": float(ref.abs().max())}
                lib = runs["library_bf16"]
                spread = abs(lib[0] - lib[1])
                for k, r in runs.items():
                    us = sum(r) / 2
                    rec[f"{k}_us"] = round(us, 2)
                    rec[f"{k}_runs_us"] = [round(v, 2) for v in r]
                    rec[f"{k}_TFLOPs"] = round(2.0 * M * N * K / us * 1e-6, 1)
                    if k != "library_bf16":
                        rec[f"{k}_speedup"] = round(sum(lib) / sum(r), 3)
                        rec[f"{k}_beats_library"] = bool(max(r) < min(lib) - spread)
                line = json.dumps(rec)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")
            del w, codes
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
