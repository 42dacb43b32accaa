#!/usr/bin/env python
"""Time the flash-attention kernels at the BERT-base training shape for several occupancy
variants (DTD_ATTN_OCC="fwd,dkdv,dq" waves/SIMD).  Prints one JSON line per variant.

fwd_us: forward kernel with the dropout keep bits generated ahead (as in the model, where the
mask kernel runs on a side stream under the forward GEMMs); mask_us: the mask generator alone;
bwd_us: dK/dV + dQ, or the one-kernel fused backward for a variant named "fused" (or "fused:<occ>").
Env: B, H, P, CAUSAL=1 (model FLOPs are quoted for the full square), ALIBI=1 (ALiBi slopes, with
``--valid-frac`` / ``--docs``).

``--valid-frac F [F ...]``: the key-range (key-padding mask) kernels instead -- every row gets the
right-padded range (0, round(F * S)).  One JSON line per fraction with the forward, dQ, dK/dV and
whole-backward times (dq_us / dkdv_us: each kernel alone, ops.attention.set_bwd_kernels), plus a
line ``"valid_frac": null`` for the call without a range.  The configurations are timed
interleaved, ``--rounds`` times over; each figure is the median of its rounds (the spread is in
``*_minmax``).  ``--out FILE`` appends the lines to a jsonl file, ``--tag`` labels them.

``--docs N [N ...]``: the document-mask (sequence packing) kernels -- every row holds N equal
documents (S // N tokens each, the last takes the remainder).  Same records, with ``"docs": N``;
interleaved with the call without a range like ``--valid-frac`` (both flags may be given).

``--dkdv-arms``: the three dK/dV kernels of the unmasked call (DTD_ATTN_DKDV=old / dma / pipe: register-
staged tiles, LDS-DMA tiles, LDS-DMA tiles with the score MFMAs one sub-block ahead) at S = 512, H = 12,
p = P, B = 256 and 1024 (``--dkdv-batches``).  Same protocol: the arms alternate inside every round,
medians over ``--rounds``, one JSON line per (B, arm) with dkdv_us (the kernel alone) and bwd_us."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_training_and_deepspeed_amd.ops import _lib  # noqa: E402
from distributed_training_and_deepspeed_amd.ops import attention as A  # noqa: E402
from distributed_training_and_deepspeed_amd.ops.rng import RngState  # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def equal_docs(B, S, n):
    """DocRange of B rows of n equal documents."""
    seg = torch.clamp(torch.arange(S, device="cuda") // max(S // n, 1), max=n - 1) + 1
    return A.doc_range_from_segment_ids(seg.view(1, S).expand(B, S).contiguous())


def ranged(args, B, S, H, D, p, causal, qkv, dctx, rng, slopes=None):
    """Forward / dQ / dK/dV times per valid fraction / document count (None = no range),
    interleaved over rounds.
    With a kernel library from before the key ranges (DTD_KERNELS_SO=<older build>, the yardstick
    of an A/B) only the call without a range is timed, forward and whole backward."""
    has_range = _lib.has("dtd_attn_fwd_range") and _lib.has("dtd_attn_set_bwd_kernels")
    configs = [None] + ([("valid_frac", f) for f in args.valid_frac or []] if has_range else []) \
        + [("docs", n) for n in args.docs or []]
    pend = A.attn_masks_async(B, S, H, D, p, rng, 3, qkv.device) if p > 0 else None
    torch.cuda.synchronize()
    state = {}
    for f in configs:
        kr = {}
        if f is not None and f[0] == "valid_frac":
            kr = {"key_range": torch.tensor([[0, int(round(f[1] * S))]] * B, dtype=torch.int32, device="cuda")}
        elif f is not None:
            kr = {"doc_range": equal_docs(B, S, f[1])}
        ctx, lse, mk = A.attn_fwd(qkv, B, S, H, D, causal, slopes, p, rng, 3, masks=pend, **kr)
        state[f] = (kr, ctx, lse, mk)
    times = {f: {"fwd_us": [], "dq_us": [], "dkdv_us": [], "bwd_us": []} for f in configs}
    for _ in range(args.rounds):
        for f in configs:
            kr, ctx, lse, mk = state[f]
            t = times[f]
            t["fwd_us"].append(timeit(lambda: A.attn_fwd(qkv, B, S, H, D, causal, slopes, p, rng, 3, masks=pend, **kr)))
            bwd = lambda: A.attn_bwd(dctx, qkv, ctx, lse, B, S, H, D, causal, slopes, p, rng, 3, mk, **kr)  # noqa: E731
            t["bwd_us"].append(timeit(bwd))
            if not has_range:
                continue
            try:     # (dK/dV alone reads an unwritten delta: wrong values, same work)
                A.set_bwd_kernels(dq=True, dkdv=False)
                t["dq_us"].append(timeit(bwd))
                A.set_bwd_kernels(dq=False, dkdv=True)
                t["dkdv_us"].append(timeit(bwd))
            finally:
                A.set_bwd_kernels(True, True)
    for f in configs:
        rec = {"tag": args.tag, "valid_frac": f[1] if f and f[0] == "valid_frac" else None, "B": B, "S": S, "H": H,
               "D": D, "causal": causal, "p": p, "rounds": args.rounds}
        if args.docs:
            rec["docs"] = f[1] if f and f[0] == "docs" else None
            rec["alibi"] = slopes is not None
        for k, v in times[f].items():
            if not v:
                continue
            rec[k] = round(statistics.median(v), 1)
            rec[k + "_minmax"] = [round(min(v), 1), round(max(v), 1)]
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


DKDV_ARMS = ("old", "dma", "pipe")


def dkdv_arms(args, S, H, D, p):
    """dK/dV alone and the whole backward per arm of DTD_ATTN_DKDV (read at every launch), the arms
    interleaved over rounds, at B * H = 3072 and 12288.  One JSON line per (B, arm)."""
    for B in args.dkdv_batches:
        qkv = torch.randn(B * S, 3 * H * D, device="cuda").to(torch.bfloat16)
        dctx = torch.randn(B * S, H * D, device="cuda").to(torch.bfloat16)
        rng = RngState(1, device="cuda")
        for _ in range(20):   # clock / cache warm-up
            A.attn_fwd(qkv, B, S, H, D, False, None, p, rng, 3)
        ctx, lse, mk = A.attn_fwd(qkv, B, S, H, D, False, None, p, rng, 3)
        torch.cuda.synchronize()
        bwd = lambda: A.attn_bwd(dctx, qkv, ctx, lse, B, S, H, D, False, None, p, rng, 3, mk)  # noqa: E731
        times = {arm: {"dkdv_us": [], "bwd_us": []} for arm in DKDV_ARMS}
        try:
            for _ in range(args.rounds):
                for arm in DKDV_ARMS:
                    os.environ["DTD_ATTN_DKDV"] = arm
                    times[arm]["bwd_us"].append(timeit(bwd))
                    try:     # (dK/dV alone reads an unwritten delta: wrong values, same work)
                        A.set_bwd_kernels(dq=False, dkdv=True)
                        times[arm]["dkdv_us"].append(timeit(bwd))
                    finally:
                        A.set_bwd_kernels(True, True)
        finally:
            os.environ.pop("DTD_ATTN_DKDV", None)
        for arm in DKDV_ARMS:
            rec = {"tag": args.tag, "dkdv_arm": arm, "B": B, "S": S, "H": H, "D": D, "p": p, "rounds": args.rounds}
            for k, v in times[arm].items():
                rec[k] = round(statistics.median(v), 1)
                rec[k + "_minmax"] = [round(min(v), 1), round(max(v), 1)]
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
        del qkv, dctx, ctx, lse, mk


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dkdv-arms", action="store_true",
                    help="time the dK/dV arms old / dma / pipe (DTD_ATTN_DKDV) interleaved, S = 512, H = 12, D = 64")
    ap.add_argument("--dkdv-batches", type=int, nargs="+", default=[256, 1024],
                    help="--dkdv-arms: batch sizes (B * 12 heads = 3072 and 12288 by default)")
    ap.add_argument("occ", nargs="*", help='occupancy variants "fwd,dkdv,dq", "fused" or "fused:<occ>"')
    ap.add_argument("--valid-frac", type=float, nargs="+", default=None,
                    help="time the key-range kernels at these valid fractions of S (right-padded rows)")
    ap.add_argument("--docs", type=int, nargs="+", default=None,
                    help="time the document-mask kernels with this many equal documents per row")
    ap.add_argument("--rounds", type=int, default=5, help="--valid-frac: interleaved rounds per configuration")
    ap.add_argument("--out", default="", help="--valid-frac: append the JSON lines to this file")
    ap.add_argument("--tag", default="", help="--valid-frac: label of the records")
    args = ap.parse_args()
    B, S, H, D = int(os.environ.get("B", 32)), int(os.environ.get("S", 512)), int(os.environ.get("H", 12)), 64
    p = float(os.environ.get("P", 0.1))
    causal = os.environ.get("CAUSAL", "0") == "1"
    if args.dkdv_arms:
        dkdv_arms(args, 512, 12, D, p)
        return
    qkv = torch.randn(B * S, 3 * H * D, device="cuda").to(torch.bfloat16)
    dctx = torch.randn(B * S, H * D, device="cuda").to(torch.bfloat16)
    rng = RngState(1, device="cuda")
    flops_f = 4 * B * H * S * S * D
    # clock / cache warm-up: the first timed configuration otherwise reads ~20 % slow
    for _ in range(50):
        A.attn_fwd(qkv, B, S, H, D, causal, None, p, rng, 3)
    torch.cuda.synchronize()
    if args.valid_frac is not None or args.docs is not None:
        slopes = A.alibi_slopes(H) if os.environ.get("ALIBI", "0") == "1" else None
        ranged(args, B, S, H, D, p, causal, qkv, dctx, rng, slopes)
        return
    for occ in args.occ or ["1,1,1", "2,2,2", "3,2,2", "3,2,3"]:
        form = occ.split(":", 1)[0] if occ.startswith("fused") else "split"
        A.set_bwd_form(form)
        occ = occ.split(":", 1)[1] if ":" in occ else ("3,2,3" if form != "split" else occ)
        os.environ["DTD_ATTN_OCC"] = occ
        pend = A.attn_masks_async(B, S, H, D, p, rng, 3, qkv.device) if p > 0 else None
        torch.cuda.synchronize()
        ctx, lse, mk = A.attn_fwd(qkv, B, S, H, D, causal, None, p, rng, 3, masks=pend)
        tf = timeit(lambda: A.attn_fwd(qkv, B, S, H, D, causal, None, p, rng, 3, masks=pend))
        cur = torch.cuda.current_stream()
        tm = timeit(lambda: cur.wait_event(A.attn_masks_async(B, S, H, D, p, rng, 3, qkv.device).event)) \
            if p > 0 else 0.0
        tb = timeit(lambda: A.attn_bwd(dctx, qkv, ctx, lse, B, S, H, D, causal, None, p, rng, 3, mk))
        print(json.dumps({"occ": occ, "bwd_form": form, "B": B, "S": S, "H": H, "causal": causal, "p": p, "fwd_us": round(tf, 1), "mask_us": round(tm, 1),
                          "bwd_us": round(tb, 1), "fwd_TFs": round(flops_f / tf / 1e6, 1),
                          "bwd_TFs": round(2.5 * flops_f / tb / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
