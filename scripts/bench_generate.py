"""Decode rate of ``CausalLM.generate`` -- eager and with ``graph=True`` -- against the only way to continue a
prompt without the KV cache: running the whole prefix through the model again for every token.

Models llama-160m and TinyLlama-1.1B (random init, bf16, fused path), B in {1, 8}, prompt 128, 128 new
tokens, greedy.  The steady-state step time of ``generate`` is the difference of two timed calls, 128 and 16
new tokens, over their 112 extra steps: both pay the prefill, the two eager steps and (``graph=True``) the
capture once.  The baseline runs ``model(prefix)`` for the same 112 steps (prefix lengths 144 .. 255) and takes
the argmax of the last position.  Each arm is timed twice, interleaved; the whole 128-token call is reported too.

``--kv-cache-dtype fp8`` runs both ``generate`` arms with the FP8 KV cache (``kv_dtype="fp8"``); the row says so.

One JSON line per (model, B), appended to --out.

Usage: python scripts/bench_generate.py [--out profiles/generate.jsonl] [--models llama-160m,tinyllama-1.1b]
                                        [--kv-cache-dtype auto|fp8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_training_and_deepspeed_amd.models import build_model  # noqa: E402

PROMPT, NEW, SHORT = 128, 128, 16


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


@torch.no_grad()
def recompute(model, ids, first, steps):
    """``steps`` greedy tokens, each from a full forward of the prefix; starts from a prefix of ``first`` tokens."""
    cur = ids[:, :first]
    for _ in range(steps):
        nxt = model(cur).logits[:, -1].argmax(-1, keepdim=True)
        cur = torch.cat([cur, nxt], 1)
    return cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--models", type=str, default="llama-160m,tinyllama-1.1b")
    ap.add_argument("--batches", type=str, default="1,8")
    ap.add_argument("--kv-cache-dtype", default="auto", choices=("auto", "fp8"), help="auto: the model's dtype")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate.py needs a GPU")
    steps = NEW - SHORT
    kv_dtype = None if args.kv_cache_dtype == "auto" else args.kv_cache_dtype
    for name in args.models.split(","):
        model = build_model(name, impl="fused", dtype=torch.bfloat16, device="cuda", seed=0).eval()
        for B in (int(b) for b in args.batches.split(",")):
            g = torch.Generator().manual_seed(B)
            ids = torch.randint(3, model.cfg.vocab_size, (B, PROMPT + NEW), generator=g).cuda()
            prompt = ids[:, :PROMPT]
            arms = {
                "eager": lambda n: model.generate(prompt, n, kv_dtype=kv_dtype),
                "graph": lambda n: model.generate(prompt, n, graph=True, kv_dtype=kv_dtype),
            }
            for fn in arms.values():                      # warm-up of every shape the timed calls use
                fn(SHORT)
            recompute(model, ids, PROMPT + SHORT, 4)
            same = bool(torch.equal(arms["eager"](NEW), arms["graph"](NEW)))
            runs = {"eager": [], "graph": [], "recompute": []}
            totals = {"eager": [], "graph": []}
            for _ in range(2):
                for key, fn in arms.items():
                    _, t_long = wall(lambda: fn(NEW))
                    _, t_short = wall(lambda: fn(SHORT))
                    runs[key].append((t_long - t_short) / steps)
                    totals[key].append(t_long)
                _, t = wall(lambda: recompute(model, ids, PROMPT + SHORT, steps))
                runs["recompute"].append(t / steps)
            rec = {"case": "generate", "model": model.cfg.name, "B": B, "prompt": PROMPT, "new_tokens": NEW,
                   "kv_cache_dtype": args.kv_cache_dtype, "steps_timed": steps, "graph_tokens_equal_eager": same}
            for key, r in runs.items():
                ms = sum(r) / 2 * 1e3
                rec[f"{key}_ms_per_step"] = round(ms, 4)
                rec[f"{key}_runs_ms_per_step"] = [round(x * 1e3, 4) for x in r]
                rec[f"{key}_tokens_per_s"] = round(B / (ms * 1e-3), 1)
            for key, r in totals.items():
                rec[f"{key}_call_ms"] = round(sum(r) / 2 * 1e3, 2)
            rec["eager_over_recompute"] = round(rec["recompute_ms_per_step"] / rec["eager_ms_per_step"], 2)
            rec["graph_over_eager"] = round(rec["eager_ms_per_step"] / rec["graph_ms_per_step"], 2)
            emit(args.out, rec)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
