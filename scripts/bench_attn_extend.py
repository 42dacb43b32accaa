"""Timings of the multi-token cached-attention kernel (ops/csrc/attention_extend.hip) against what else could
serve the same T tokens, in one process on the same cache, arms alternating, two repeats each:

  * ``extend``      the kernel on the bf16 cache;
  * ``extend_fp8``  the kernel on the FP8 cache of the same values;
  * ``decode_x_T``  T successive ``attn_decode`` calls (token t at kv_len + t + 1): what there was before the kernel;
  * ``sdpa``        ``F.scaled_dot_product_attention`` with an explicit [B, 1, T, Smax] mask, K / V expanded to the
                    query heads beforehand (the expansion is not timed: in the yardstick's favour).

Shapes (H / Hkv / D): Llama-2-7B 32/32/128, Llama-3-8B 32/8/128, TinyLlama 32/4/64; T in {4, 16, 128, 512}; kv_len in
{512, 4096, 8192} slots before the chunk (the cache is kv_len + T long); B in {1, 8}.  Each timing is a device-event
window of at least ``--window-ms`` of work after a warm-up of the same call.  A difference counts only where it
exceeds the spread between an arm's two repeats: ``slower_than_decode`` / ``slower_than_sdpa`` mark a shape whose
faster ``extend`` repeat is slower than the yardstick's slower one.

One JSON line per shape, appended to --out.  Usage:
    python scripts/bench_attn_extend.py [--window-ms 30] [--budget-s SECONDS] [--out profiles/attn_extend.jsonl]
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
from distributed_training_and_deepspeed_amd.ops.kv_cache import quantize_kv_ref  # noqa: E402

MODELS = (("Llama-2-7B", 32, 32, 128), ("Llama-3-8B", 32, 8, 128), ("TinyLlama", 32, 4, 64))
TS = (4, 16, 128, 512)
KV_LENS = (512, 4096, 8192)
BATCHES = (1, 8)


def timeit(fn, window_ms):
    """Microseconds per call over a window of at least ``window_ms`` (3 to 200 calls), after a warm-up."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    iters = max(3, min(200, int(window_ms / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def shape_row(name, H, Hkv, D, T, n, B, window_ms):
    dev, G, Smax = "cuda", H // Hkv, n + T
    g = torch.Generator(device=dev).manual_seed(H + D + T + n + B)
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D, generator=g, device=dev).to(torch.bfloat16)
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g, device=dev).to(torch.bfloat16) for _ in range(2))
    (k8, ks), (v8, vs) = quantize_kv_ref(k), quantize_kv_ref(v)
    kv_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    splits = A.extend_splits(B, Hkv, Smax, T, G)
    ws = torch.empty(max(1, A.extend_workspace_floats(B, T, H, D, splits)), dtype=torch.float32, device=dev)
    out = (torch.empty(B * T, H * D, dtype=torch.bfloat16, device=dev), torch.empty(B * T, H, dtype=torch.float32, device=dev))
    # T decode calls
    steps = [kv_len + t + 1 for t in range(T)]
    rows = qkv.view(B, T, -1)
    dsplits = A.decode_splits(B, Hkv, Smax)
    dws = torch.empty(A.decode_workspace_floats(B, H, D, dsplits), dtype=torch.float32, device=dev)
    dout = (torch.empty(B, H * D, dtype=torch.bfloat16, device=dev), torch.empty(B, H, dtype=torch.float32, device=dev))
    # SDPA
    q = rows[:, :, :H * D].reshape(B, T, H, D).transpose(1, 2)
    ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    mask = (torch.arange(Smax, device=dev).view(1, 1, 1, Smax) <= (n + torch.arange(T, device=dev)).view(1, 1, T, 1))

    def decode_x_t():
        for t in range(T):
            A.attn_decode(rows[:, t], k, v, steps[t], B, H, D, Hkv, splits=dsplits, workspace=dws, out=dout)

    arms = {
        "extend": lambda: A.attn_extend(qkv, k, v, kv_len, B, T, H, D, Hkv, splits=splits, workspace=ws, out=out),
        "extend_fp8": lambda: A.attn_extend(qkv, k8, v8, kv_len, B, T, H, D, Hkv, splits=splits, workspace=ws, out=out,
                                            k_scale=ks, v_scale=vs),
        "decode_x_T": decode_x_t,
        "sdpa": lambda: F.scaled_dot_product_attention(q, ke, ve, attn_mask=mask),
    }
    us = {a: [] for a in arms}
    for _ in range(2):
        for a, fn in arms.items():
            us[a].append(round(timeit(fn, window_ms), 2))
    # the same answer: the kernel against the T decode calls' last token
    ctx = A.attn_extend(qkv, k, v, kv_len, B, T, H, D, Hkv)[0].view(B, T, -1)[:, -1].float()
    last = A.attn_decode(rows[:, T - 1], k, v, steps[-1], B, H, D, Hkv)[0].float()
    row = dict(model=name, H=H, Hkv=Hkv, D=D, T=T, kv_len=n, B=B, splits=splits, us=us,
               max_abs_diff_vs_decode=round(float((ctx - last).abs().max()), 5),
               speedup_vs_decode=round(min(us["decode_x_T"]) / min(us["extend"]), 2),
               speedup_vs_sdpa=round(min(us["sdpa"]) / min(us["extend"]), 2),
               slower_than_decode=min(us["extend"]) > max(us["decode_x_T"]),
               slower_than_sdpa=min(us["extend"]) > max(us["sdpa"]))
    return row


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--budget-s", type=float, default=0.0, help="stop starting new shapes after this long (0: no limit)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_extend.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_extend.py needs the GPU: nothing is measured without one")
    t0 = time.time()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for name, H, Hkv, D in MODELS:
            for B in BATCHES:
                for n in KV_LENS:
                    for T in TS:
                        if args.budget_s and time.time() - t0 > args.budget_s:
                            print(f"budget of {args.budget_s:.0f} s spent: stopping before {name} B={B} kv_len={n} T={T}")
                            return 0
                        row = shape_row(name, H, Hkv, D, T, n, B, args.window_ms)
                        f.write(json.dumps(row) + "\n")
                        f.flush()
                        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
