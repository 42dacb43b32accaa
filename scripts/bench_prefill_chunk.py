"""Whole-model cost of the chunked prefill (``generate(prefill_chunk=C)``: ``prefill`` then ``extend``, the MFMA
extend kernel of ops/csrc/attention_extend.hip) against the one-piece prefill, in scripts/bench_generate.py's
style: the bf16 fused model, one process, the two arms alternating, two repeats each.  Per arm: the wall time
of the prompt pass into one pre-allocated cache -- ``prefill`` of the whole prompt, or ``prefill`` of the first C
tokens and ``extend(last_only=True)`` of each further chunk -- and the greedy first token, ending in a device
synchronise, and ``torch.cuda.max_memory_allocated`` over the pass with the counter reset before it (weights and
cache included).

Usage: python scripts/bench_prefill_chunk.py [--model tinyllama-1.1b] [--prompt 2048] [--chunk 256] [--batch 1]
       [--out profiles/attn_extend.jsonl]
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
from distributed_training_and_deepspeed_amd.ops.kv_cache import KVCache  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="tinyllama-1.1b")
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefill_chunk.py needs a GPU")
    model = build_model(args.model, impl="fused", dtype=torch.bfloat16, device="cuda", seed=0).eval()
    g = torch.Generator().manual_seed(args.batch)
    prompt = torch.randint(3, model.cfg.vocab_size, (args.batch, args.prompt), generator=g).cuda()
    cache = KVCache.allocate(model.cfg, args.batch, args.prompt, "cuda", torch.bfloat16)
    arms = {"one_piece": args.prompt, "chunked": args.chunk}

    @torch.no_grad()
    def prompt_pass(c):
        """The prompt c tokens at a time (the head on B rows per chunk); the first token."""
        cache.reset()
        logits = model.prefill(prompt[:, :c], cache)
        for s in range(c, args.prompt, c):
            logits = model.extend(prompt[:, s:s + c], cache, last_only=True)
        return logits.argmax(-1)

    ms, mib, tokens = {a: [] for a in arms}, {a: [] for a in arms}, {}
    for c in arms.values():        # warm-up: kernels loaded, GEMM algorithms picked for both arms' shapes
        prompt_pass(c)
    for _ in range(2):
        for a, c in arms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            tokens[a] = prompt_pass(c)
            torch.cuda.synchronize()
            ms[a].append(round(1e3 * (time.perf_counter() - t0), 2))
            mib[a].append(round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
    rec = dict(bench="prefill_chunk", model=args.model, B=args.batch, prompt=args.prompt, chunk=args.chunk, ms=ms,
               peak_mib=mib, same_first_token=bool(torch.equal(tokens["one_piece"], tokens["chunked"])))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
