"""Decode rate of ``CausalLM.generate`` -- eager and with ``graph=True`` -- against the only way to continue a
prompt without the KV cache: running the whole prefix through the model again for every token.

Models llama-160m and TinyLlama-1.1B (random init, bf16, fused path), B in {1, 8}, prompt 128, 128 new
tokens, greedy.  The steady-state step time of ``generate`` is the difference of two timed calls, 128 and 16
new tokens, over their 112 extra steps: both pay the prefill, the two eager steps and (``graph=True``) the
capture once.  The baseline runs ``model(prefix)`` for the same 112 steps (prefix lengths 144 .. 255) and takes
the argmax of the last position.  Each arm is timed twice, interleaved; the whole 128-token call is reported too.

``--kv-cache-dtype fp8`` runs both ``generate`` arms with the FP8 KV cache (``kv_dtype="fp8"``); the row says so.
``--weight-dtype fp8`` / ``mxfp4`` quantises the projections first (``quantize_weights_``: the decode steps stream the codes),
``--skinny-gemm`` sends the bf16 products of at most 64 rows to ``gemm_skinny.hip``.

``--sampler`` times the sampled step instead (``do_sample``, ``top_k=50``, ``graph=True``): ``sampler="torch"``
(eager ``topk`` / ``softmax`` / ``multinomial`` between replays) against ``sampler="device"`` (``sample.hip`` inside the
graph), the arms alternating, two repeats; then the selection alone at V = 32000 and 128256, the kernel against the
torch sequence, in ms per call of a 200-call loop.  Default --out then: profiles/generate_sampler.jsonl.

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
from distributed_training_and_deepspeed_amd.ops import gemm as G  # noqa: E402

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


@torch.no_grad()
def prompt_pass(model, args, iters=10):
    """ms per ``prefill`` of ``--prompt-pass`` tokens: two repeats of ``iters`` calls per arm, the arms alternating."""
    from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache
    S0 = args.prompt_pass
    arms = {"bf16_act": False, "fp8_act": True} if args.act_dtype == "fp8" else {"bf16_act": False}
    for B in (int(b) for b in args.batches.split(",")):
        ids = torch.randint(3, model.cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(B)).cuda()
        cache = KVCache.allocate(model.cfg, B, S0, "cuda", torch.bfloat16)

        def run(on, n):
            if args.act_dtype == "fp8":
                model.set_fp8_activations(on)
            for _ in range(n):
                cache.reset()
                logits = model.prefill(ids, cache)
            return logits

        logits = {k: run(on, 2).float() for k, on in arms.items()}      # warm-up of both arms
        runs = {k: [] for k in arms}
        for _ in range(2):
            for k, on in arms.items():
                runs[k].append(wall(lambda: run(on, iters))[1] / iters * 1e3)
        rec = {"case": "prompt_pass", "model": model.cfg.name, "B": B, "prompt": S0, "weight_dtype": args.weight_dtype,
               "iters": iters}
        for k, r in runs.items():
            rec[f"{k}_ms"] = round(sum(r) / 2, 3)
            rec[f"{k}_runs_ms"] = [round(v, 3) for v in r]
        if "fp8_act" in runs:
            rec["fp8_act_speedup"] = round(sum(runs["bf16_act"]) / sum(runs["fp8_act"]), 3)
            rec["max_abs_logit_diff"] = float((logits["fp8_act"] - logits["bf16_act"]).abs().max())
            rec["max_abs_logit"] = float(logits["bf16_act"].abs().max())
        emit(args.out, rec)


@torch.no_grad()
def sampler_steps(model, args):
    """ms per sampled step, torch sampler against device sampler, both with ``graph=True``."""
    steps = NEW - SHORT
    for B in (int(b) for b in args.batches.split(",")):
        prompt = torch.randint(3, model.cfg.vocab_size, (B, PROMPT), generator=torch.Generator().manual_seed(B)).cuda()
        arms = {s: (lambda n, s=s: model.generate(prompt, n, do_sample=True, temperature=0.8, top_k=50, seed=1, graph=True,
                                                  sampler=s)) for s in ("torch", "device")}
        for fn in arms.values():
            fn(SHORT)
        runs = {k: [] for k in arms}
        for _ in range(2):
            for key, fn in arms.items():
                t_long, t_short = wall(lambda: fn(NEW))[1], wall(lambda: fn(SHORT))[1]
                runs[key].append((t_long - t_short) / steps * 1e3)
        rec = {"case": "sampled_step", "model": model.cfg.name, "B": B, "V": model.cfg.vocab_size, "prompt": PROMPT,
               "new_tokens": NEW, "top_k": 50, "graph": True, "steps_timed": steps}
        for key, r in runs.items():
            rec[f"{key}_ms_per_step"] = round(sum(r) / 2, 4)
            rec[f"{key}_runs_ms_per_step"] = [round(x, 4) for x in r]
        rec["torch_over_device"] = round(rec["torch_ms_per_step"] / rec["device_ms_per_step"], 3)
        emit(args.out, rec)


@torch.no_grad()
def sampler_alone(args, calls=200):
    """The selection alone, eager launches from Python: the kernel against ``CausalLM._select``'s torch sequence."""
    from distributed_training_and_deepspeed_amd.models.causal_lm import CausalLM
    from distributed_training_and_deepspeed_amd.ops.functional import sample_tokens
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    for V in (32000, 128256):
        for B in (int(b) for b in args.batches.split(",")):
            logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(V)) * 3).bfloat16().cuda()
            for top_k, top_p in ((50, 1.0), (50, 0.9), (0, 0.9), (0, 1.0)):
                arms = {"device": lambda: sample_tokens(logits, 0.8, top_k, top_p, 1, step)}
                if top_p == 1.0:
                    arms["torch"] = lambda: CausalLM._select(logits, True, 0.8, top_k, gen)
                runs = {k: [] for k in arms}
                for fn in arms.values():
                    fn()
                for _ in range(2):
                    for key, fn in arms.items():
                        runs[key].append(wall(lambda: [fn() for _ in range(calls)])[1] / calls * 1e3)
                rec = {"case": "selection_alone", "V": V, "B": B, "dtype": "bfloat16", "top_k": top_k, "top_p": top_p,
                       "calls": calls}
                for key, r in runs.items():
                    rec[f"{key}_ms"] = round(sum(r) / 2, 4)
                    rec[f"{key}_runs_ms"] = [round(x, 4) for x in r]
                emit(args.out, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--models", type=str, default="llama-160m,tinyllama-1.1b")
    ap.add_argument("--batches", type=str, default="1,8")
    ap.add_argument("--kv-cache-dtype", default="auto", choices=("auto", "fp8"), help="auto: the model's dtype")
    ap.add_argument("--weight-dtype", default="auto", choices=("auto", "fp8", "mxfp4"),
                    help="fp8 / mxfp4: quantize_weights_ -- the decode steps stream FP8 or MXFP4 codes of the projections")
    ap.add_argument("--act-dtype", default="auto", choices=("auto", "fp8"),
                    help="fp8 (with --weight-dtype fp8): set_fp8_activations -- products of more than 64 rows on the FP8 GEMM")
    ap.add_argument("--prompt-pass", type=int, default=0, metavar="S0",
                    help="time the prompt pass alone (prefill of S0 tokens) instead of the decode steps; with --act-dtype fp8 "
                         "the arms with and without FP8 activations alternate in one process")
    ap.add_argument("--skinny-gemm", action="store_true", help="bf16 products of at most 64 rows on gemm_skinny.hip")
    ap.add_argument("--skip-recompute", action="store_true", help="leave the no-cache baseline out")
    ap.add_argument("--sampler", action="store_true",
                    help="time the sampled step, torch sampler against device sampler, and the selection alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate.py needs a GPU")
    if args.sampler and args.prompt_pass:
        raise SystemExit("--sampler and --prompt-pass are separate measurements: give one")
    if args.sampler and not args.out:
        args.out = os.path.join(ROOT, "profiles", "generate_sampler.jsonl")
    steps = NEW - SHORT
    kv_dtype = None if args.kv_cache_dtype == "auto" else args.kv_cache_dtype
    for name in args.models.split(","):
        model = build_model(name, impl="fused", dtype=torch.bfloat16, device="cuda", seed=0).eval()
        if args.weight_dtype != "auto":
            model.quantize_weights_(args.weight_dtype)
        G.set_skinny(args.skinny_gemm)
        if args.sampler:
            sampler_steps(model, args)
        elif args.prompt_pass:
            prompt_pass(model, args)
        if args.sampler or args.prompt_pass:
            del model
            torch.cuda.empty_cache()
            continue
        if args.act_dtype == "fp8":
            model.set_fp8_activations(True)
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
            if not args.skip_recompute:
                recompute(model, ids, PROMPT + SHORT, 4)
            same = bool(torch.equal(arms["eager"](NEW), arms["graph"](NEW)))
            runs = {"eager": [], "graph": []} if args.skip_recompute else {"eager": [], "graph": [], "recompute": []}
            totals = {"eager": [], "graph": []}
            for _ in range(2):
                for key, fn in arms.items():
                    _, t_long = wall(lambda: fn(NEW))
                    _, t_short = wall(lambda: fn(SHORT))
                    runs[key].append((t_long - t_short) / steps)
                    totals[key].append(t_long)
                if not args.skip_recompute:
                    _, t = wall(lambda: recompute(model, ids, PROMPT + SHORT, steps))
                    runs["recompute"].append(t / steps)
            rec = {"case": "generate", "model": model.cfg.name, "B": B, "prompt": PROMPT, "new_tokens": NEW,
                   "kv_cache_dtype": args.kv_cache_dtype, "weight_dtype": args.weight_dtype,
                   "skinny_gemm": args.skinny_gemm, "steps_timed": steps, "graph_tokens_equal_eager": same}
            for key, r in runs.items():
                ms = sum(r) / 2 * 1e3
                rec[f"{key}_ms_per_step"] = round(ms, 4)
                rec[f"{key}_runs_ms_per_step"] = [round(x * 1e3, 4) for x in r]
                rec[f"{key}_tokens_per_s"] = round(B / (ms * 1e-3), 1)
            for key, r in totals.items():
                rec[f"{key}_call_ms"] = round(sum(r) / 2 * 1e3, 2)
            if not args.skip_recompute:
                rec["eager_over_recompute"] = round(rec["recompute_ms_per_step"] / rec["eager_ms_per_step"], 2)
            rec["graph_over_eager"] = round(rec["eager_ms_per_step"] / rec["graph_ms_per_step"], 2)
            emit(args.out, rec)
        del model
        torch.cuda.empty_cache()
    if args.sampler:
        sampler_alone(args)


if __name__ == "__main__":
    main()
