"""Text generation with a KV cache for the Llama family (random-init weights, synthetic prompts).

    python generate_text.py --model-name llama-tiny-gqa --batch-size 4 --prompt-len 64 --max-new-tokens 64 \
        [--graph] [--impl auto|fused|reference] [--sample --top-k 50 --temperature 0.8] [--metrics-json F] \
        [--kv-cache-dtype auto|fp8]

Prints the token ids of row 0, the prefill time and the decode rate.  The prompt goes through the model once
(``CausalLM.prefill``); every further token costs one ``decode_step`` against the cache, whose attention is the
split-KV decode kernel on the GPU.  ``--graph`` replays the step as a HIP graph.  ``--kv-cache-dtype fp8`` keeps the
cache as e4m3fn codes with one fp32 scale per row: half the bytes, at the quantisation's error.  Timings: the run is repeated
after a warm-up run; prefill is the time of a one-token ``generate``, the decode rate is
batch x (N - 1) tokens over the rest.
"""
from __future__ import annotations

import argparse
import json
import time

import torch

from distributed_training_and_deepspeed_amd.models import build_model


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-name", default="llama-tiny-gqa")
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--max-new-tokens", type=int, default=64)
    ap.add_argument("--graph", action="store_true", help="replay the decode step as a HIP graph (GPU)")
    ap.add_argument("--impl", default="auto", choices=("auto", "fused", "reference"))
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is a GPU, else cpu")
    ap.add_argument("--dtype", default=None, choices=("bfloat16", "float32"), help="default: bfloat16 on the GPU")
    ap.add_argument("--kv-cache-dtype", default="auto", choices=("auto", "fp8"),
                    help="auto: the cache in the model's dtype; fp8: e4m3fn codes with per-row scales")
    ap.add_argument("--metrics-json", default="")
    args = ap.parse_args(argv)

    dev = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    dtype = getattr(torch, args.dtype) if args.dtype else (torch.bfloat16 if dev.type == "cuda" else torch.float32)
    model = build_model(args.model_name, impl=args.impl, dtype=dtype, device=dev, seed=args.seed).eval()
    cfg = model.cfg
    B, S0, N = args.batch_size, args.prompt_len, args.max_new_tokens
    ids = torch.randint(3, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(args.seed)).to(dev)
    kw = dict(do_sample=args.sample, temperature=args.temperature, top_k=args.top_k, seed=args.seed, graph=args.graph,
              kv_dtype=None if args.kv_cache_dtype == "auto" else args.kv_cache_dtype)

    def timed(n):
        _sync(dev)
        t0 = time.perf_counter()
        out = model.generate(ids, n, **kw)
        _sync(dev)
        return out, time.perf_counter() - t0

    timed(min(N, 4))                       # warm-up: kernels loaded, GEMM algorithms picked, the rotary table built
    _, t_prefill = timed(1)
    out, t_all = timed(N)
    decode_s = max(t_all - t_prefill, 1e-9)
    rate = B * max(N - 1, 0) / decode_s
    print("tokens[0]:", out[0].tolist())
    print(f"{cfg.name}: batch {B}, prompt {S0}, {N} new tokens, {dtype}, impl {args.impl}"
          f"{', fp8 kv cache' if args.kv_cache_dtype == 'fp8' else ''}"
          f"{', graph' if args.graph and dev.type == 'cuda' else ''}")
    print(f"prefill {t_prefill * 1e3:.2f} ms, decode {rate:.1f} tokens/s ({decode_s / max(N - 1, 1) * 1e3:.3f} ms/step)")
    if args.metrics_json:
        with open(args.metrics_json, "w") as f:
            json.dump({"model": cfg.name, "batch": B, "prompt_len": S0, "new_tokens": N, "dtype": str(dtype),
                       "impl": args.impl, "graph": bool(args.graph and dev.type == "cuda"), "sample": args.sample,
                       "kv_cache_dtype": args.kv_cache_dtype,
                       "prefill_ms": t_prefill * 1e3, "decode_tokens_per_s": rate, "tokens_row0": out[0].tolist()}, f)
    return out


if __name__ == "__main__":
    main()
