"""Timings of the decode-attention kernel (ops/csrc/attention_decode.hip) against two yardsticks in the same
process, on the same cache:

  (a) ``F.scaled_dot_product_attention`` with one query per sequence -- grouped heads natively
      (``enable_gqa=True``) where this torch supports it, otherwise on K / V expanded to the query heads
      beforehand, the expansion timed separately and reported (``expand_us``); a windowed shape hands it the
      window's slice of the cache;
  (b) a device-to-device copy of as many bytes as the valid K / V rows hold: the bandwidth bound of the box
      the run landed on (the copy also writes them; its rate counts the bytes once, as the kernels' does).

Shapes (H / Hkv / D): Llama-2-7B 32/32/128, Llama-3-8B 32/8/128, TinyLlama 32/4/64, Mistral 32/8/128 with a
window of 4096; B in {1, 8, 64}, kv_len in {512, 4096, 8192} (the cache is exactly that long and full), and
Mistral also at 32768, where the window cuts 7/8 of the keys.  The three are interleaved, two repeats each;
the difference between the repeats is the run's own noise.  ``slower_than_sdpa`` marks a shape where the kernel
is slower than (a) by more than that spread.  Small caches sit in L2 / MALL for all three alike.

One JSON line per shape, appended to --out: microseconds, and TB/s of valid K / V bytes.

``--fp8`` is another arm on the same table of shapes: the kernel on an FP8 cache (e4m3fn codes with one fp32 scale
per row, ops/kv_cache.py) against the bf16 kernel on the bf16 cache of the same values, alternating in one process,
two repeats each.  One JSON line per shape: microseconds and TB/s of valid bytes (the FP8 arm's include its scales);
``fp8_faster`` marks a gain beyond the bf16 arm's own difference between its repeats.

Usage: python scripts/bench_attn_decode.py [--iters K] [--budget-s SECONDS] [--out profiles/attn_decode.jsonl]
       python scripts/bench_attn_decode.py --fp8 [--iters K] [--out profiles/attn_decode_fp8.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_training_and_deepspeed_amd.ops import attention as A  # noqa: E402
from distributed_training_and_deepspeed_amd.ops.kv_cache import FP8, quantize_kv_ref  # noqa: E402

MODELS = (
    # name, H, Hkv, D, window, extra kv_len
    ("Llama-2-7B", 32, 32, 128, 0, ()),
    ("Llama-3-8B", 32, 8, 128, 0, ()),
    ("TinyLlama", 32, 4, 64, 0, ()),
    ("Mistral-7B", 32, 8, 128, 4096, (32768,)),
)
BATCHES = (1, 8, 64)
KV_LENS = (512, 4096, 8192)


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


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def sdpa_native_gqa(dev) -> bool:
    try:
        q = torch.randn(1, 4, 1, 64, device=dev, dtype=torch.bfloat16)
        k = torch.randn(1, 2, 8, 64, device=dev, dtype=torch.bfloat16)
        F.scaled_dot_product_attention(q, k, k, enable_gqa=True)
        return True
    except (TypeError, RuntimeError):
        return False


def quantized(x):
    """(codes, scales, how) of a bf16 cache [B, Hkv, n, D] by the FP8 cache's law, one sequence at a time (the fp32
    intermediates stay small); a torch without device-side e4m3fn conversion gets random finite codes and the
    scale 1 / 448 instead -- the timing does not depend on the values."""
    try:
        parts = [quantize_kv_ref(x[b]) for b in range(x.shape[0])]
        return torch.stack([p[0].view(torch.uint8) for p in parts]).view(FP8), torch.stack([p[1] for p in parts]), "quantize_kv_ref"
    except RuntimeError:
        code = torch.randint(0, 0x7F, x.shape, device=x.device, dtype=torch.uint8)
        code |= torch.randint(0, 2, x.shape, device=x.device, dtype=torch.uint8) << 7
        return code.view(FP8), torch.full(x.shape[:-1], 1.0 / 448.0, device=x.device), "random codes"


def fp8_arm(args):
    """The FP8 cache's kernel against the bf16 kernel on the same shapes, in one process: the two alternate, two
    repeats each; the bf16 arm's difference between its repeats is the run's own noise.  TB/s counts the valid
    bytes a call has to read: K and V rows, and for FP8 their scales."""
    dev, dt = "cuda", torch.bfloat16
    t_start = time.perf_counter()
    torch.manual_seed(0)
    for name, H, Hkv, D, W, extra in MODELS:
        for B in BATCHES:
            for n in KV_LENS + extra:
                shape = {"case": "attn_decode_fp8", "model": name, "B": B, "H": H, "Hkv": Hkv, "D": D, "kv_len": n, "window": W}
                if args.budget_s and time.perf_counter() - t_start > args.budget_s:
                    emit(args.out, {**shape, "status": "not measured (time budget of the run)"})
                    continue
                valid = min(n, W) if W else n
                bytes16 = 2 * B * Hkv * valid * D * 2
                bytes8 = 2 * B * Hkv * valid * (D + 4)
                iters = args.iters if bytes16 < (1 << 30) else max(5, args.iters // 4)
                qkv = torch.randn(B, (H + 2 * Hkv) * D, device=dev, dtype=dt)
                k = torch.randn(B, Hkv, n, D, device=dev, dtype=dt)
                v = torch.randn(B, Hkv, n, D, device=dev, dtype=dt)
                k8, ks, how = quantized(k)
                v8, vs, _ = quantized(v)
                kv_len = torch.full((B,), n, dtype=torch.int32, device=dev)
                splits = A.decode_splits(B, Hkv, n)
                ws = torch.empty(A.decode_workspace_floats(B, H, D, splits), dtype=torch.float32, device=dev)
                out = (torch.empty(B, H * D, device=dev, dtype=dt), torch.empty(B, H, device=dev, dtype=torch.float32))
                out8 = (torch.empty_like(out[0]), torch.empty_like(out[1]))

                def bf16():
                    return A.attn_decode(qkv, k, v, kv_len, B, H, D, Hkv, W, splits=splits, workspace=ws, out=out)

                def fp8():
                    return A.attn_decode(qkv, k8, v8, kv_len, B, H, D, Hkv, W, splits=splits, workspace=ws, out=out8,
                                         k_scale=ks, v_scale=vs)

                diff = float((bf16()[0].float() - fp8()[0].float()).abs().max())
                runs = {"bf16": [], "fp8": []}
                for _ in range(2):
                    for key, fn in (("bf16", bf16), ("fp8", fp8)):
                        runs[key].append(timeit(fn, iters))
                mean = {key: sum(r) / 2 for key, r in runs.items()}
                noise = abs(runs["bf16"][0] - runs["bf16"][1])
                rec = {**shape, "splits": splits, "bf16_bytes": bytes16, "fp8_bytes": bytes8, "iters": iters, "fp8_data": how,
                       "max_abs_diff_fp8_vs_bf16": round(diff, 5)}
                for key, nbytes in (("bf16", bytes16), ("fp8", bytes8)):
                    rec[f"{key}_us"] = round(mean[key], 1)
                    rec[f"{key}_runs_us"] = [round(x, 1) for x in runs[key]]
                    rec[f"{key}_tbps"] = round(nbytes / mean[key] / 1e6, 3)
                rec["fp8_over_bf16"] = round(mean["fp8"] / mean["bf16"], 3)
                rec["bf16_noise_us"] = round(noise, 1)
                rec["fp8_faster"] = bool(mean["bf16"] - mean["fp8"] > noise)
                emit(args.out, rec)
                del qkv, k, v, k8, v8, ks, vs, ws
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--budget-s", type=float, default=0.0, help="stop starting new shapes after this many seconds")
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--fp8", action="store_true", help="the FP8 arm: the FP8 cache's kernel against the bf16 kernel "
                                                       "(profiles/attn_decode_fp8.jsonl)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_decode.py needs a GPU")
    if args.fp8:
        return fp8_arm(args)
    dev, dt = "cuda", torch.bfloat16
    native = sdpa_native_gqa(dev)
    t_start = time.perf_counter()
    torch.manual_seed(0)
    for name, H, Hkv, D, W, extra in MODELS:
        G = H // Hkv
        for B in BATCHES:
            for n in KV_LENS + extra:
                shape = {"case": "attn_decode", "model": name, "B": B, "H": H, "Hkv": Hkv, "D": D, "kv_len": n, "window": W}
                if args.budget_s and time.perf_counter() - t_start > args.budget_s:
                    emit(args.out, {**shape, "status": "not measured (time budget of the run)"})
                    continue
                valid = min(n, W) if W else n
                kv_bytes = 2 * B * Hkv * valid * D * 2
                iters = args.iters if kv_bytes < (1 << 30) else max(5, args.iters // 4)
                qkv = torch.randn(B, (H + 2 * Hkv) * D, device=dev, dtype=dt)
                k = torch.randn(B, Hkv, n, D, device=dev, dtype=dt)
                v = torch.randn(B, Hkv, n, D, device=dev, dtype=dt)
                kv_len = torch.full((B,), n, dtype=torch.int32, device=dev)
                splits = A.decode_splits(B, Hkv, n)
                ws = torch.empty(A.decode_workspace_floats(B, H, D, splits), dtype=torch.float32, device=dev)
                out = (torch.empty(B, H * D, device=dev, dtype=dt), torch.empty(B, H, device=dev, dtype=torch.float32))

                def decode():
                    return A.attn_decode(qkv, k, v, kv_len, B, H, D, Hkv, W, splits=splits, workspace=ws, out=out)

                q4 = qkv[:, :H * D].view(B, H, 1, D)
                ks, vs = (k[:, :, n - valid:], v[:, :, n - valid:]) if W else (k, v)
                expand_us = None
                if G > 1 and not native:
                    expand_us = timeit(lambda: (ks.repeat_interleave(G, 1), vs.repeat_interleave(G, 1)), max(3, iters // 4))
                    ke, ve = ks.repeat_interleave(G, 1), vs.repeat_interleave(G, 1)

                    def sdpa():
                        return F.scaled_dot_product_attention(q4, ke, ve)
                elif G > 1:
                    def sdpa():
                        return F.scaled_dot_product_attention(q4, ks, vs, enable_gqa=True)
                else:
                    def sdpa():
                        return F.scaled_dot_product_attention(q4, ks, vs)

                src = torch.empty(kv_bytes // 2, device=dev, dtype=dt)
                dst = torch.empty_like(src)

                def copy():
                    return dst.copy_(src)

                diff = float((decode()[0].float().view(B, H, D) - sdpa().float().view(B, H, D)).abs().max())
                runs = {"decode": [], "sdpa": [], "copy": []}
                for _ in range(2):
                    for key, fn in (("decode", decode), ("sdpa", sdpa), ("copy", copy)):
                        runs[key].append(timeit(fn, iters))
                mean = {key: sum(r) / 2 for key, r in runs.items()}
                spread = max(abs(r[0] - r[1]) for r in (runs["decode"], runs["sdpa"]))
                rec = {**shape, "splits": splits, "kv_bytes": kv_bytes, "iters": iters,
                       "sdpa_form": "none" if G == 1 else ("enable_gqa" if native else "expanded"),
                       "expand_us": None if expand_us is None else round(expand_us, 1),
                       "max_abs_diff_vs_sdpa": round(diff, 5)}
                for key in runs:
                    rec[f"{key}_us"] = round(mean[key], 1)
                    rec[f"{key}_runs_us"] = [round(x, 1) for x in runs[key]]
                    rec[f"{key}_tbps"] = round(kv_bytes / mean[key] / 1e6, 3)
                rec["decode_over_sdpa"] = round(mean["decode"] / mean["sdpa"], 3)
                rec["decode_over_copy"] = round(mean["decode"] / mean["copy"], 3)
                rec["spread_us"] = round(spread, 1)
                rec["slower_than_sdpa"] = bool(mean["decode"] - mean["sdpa"] > spread)
                emit(args.out, rec)
                del qkv, k, v, ks, vs, src, dst, ws
                if expand_us is not None:
                    del ke, ve
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
