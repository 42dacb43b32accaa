#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device listings (`hipcc --cuda-device-only -S` output): the acceptance
check of a refactor that must not move the generated code.

    compare_kernel_asm.py OLD.s NEW.s [--map old_substr=new_substr ...] [--any-sgpr]

Each listing is split into its kernels; a kernel is its instructions and basic-block labels, comments and
assembler directives dropped.  Labels (.LBB<function>_<block>) are renumbered in order of appearance and the
--map substitutions are applied, in the order given, to OLD's symbol names, so that a renamed kernel or
template argument pairs with its successor.  Per kernel: IDENTICAL, or a unified diff, the mnemonics whose
counts differ, and the resource figures of both sides.  --any-sgpr blanks the numbers of the scalar registers
(s7 -> s, s[8:15] -> s[8]: the width stays), for a change that only moves kernel arguments: their loads stay in
the diff, the renumbering that follows from them does not.  Exit status 1 if any kernel differs or has no
partner."""
import argparse
import collections
import difflib
import re
import sys

FIGURES = ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def _any_sgpr(ln: str) -> str:
    ln = re.sub(r"\bs\[(\d+):(\d+)\]", lambda m: f"s[{int(m.group(2)) - int(m.group(1)) + 1}]", ln)
    return re.sub(r"\bs\d+\b", "s", ln)


def kernels(text: str, maps=(), any_sgpr=False) -> dict:
    """{mangled name: (instruction and label lines, {figure: value})} of a listing, in listing order."""
    for old, new in maps:
        text = text.replace(old, new)
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=^\t\.section\t\.text|\Z)", text, re.M | re.S):
        name, body, foot = m.groups()
        if ".amdhsa_kernel" not in body:
            continue                                   # a device function that was not inlined
        labels, lines = {}, []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or (ln.startswith(".") and not ln.endswith(":")):
                continue
            ln = re.sub(r"\.LBB\d+_\d+", lambda b: labels.setdefault(b.group(0), f".L{len(labels)}"), ln)
            lines.append(re.sub(r"\s+", " ", _any_sgpr(ln) if any_sgpr else ln))
        lines = lines[:lines.index("s_endpgm") + 1] if "s_endpgm" in lines else lines   # (padding s_nop / s_code_end follow)
        out[name] = (lines, {k: int(re.search(rf"; {k}: (\d+)", foot).group(1)) for k in FIGURES})
    return out


def mnemonic_counts(lines) -> collections.Counter:
    return collections.Counter(ln.split()[0] for ln in lines if not ln.endswith(":"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW",
                    help="substring of OLD's symbol names and its replacement (repeatable, applied in order)")
    ap.add_argument("--any-sgpr", action="store_true", help="compare with the scalar register numbers blanked")
    ap.add_argument("--context", type=int, default=2, help="context lines of the diffs")
    args = ap.parse_args()
    maps = [tuple(m.split("=", 1)) for m in args.map]
    with open(args.old) as f:
        old = kernels(f.read(), maps, args.any_sgpr)
    with open(args.new) as f:
        new = kernels(f.read(), (), args.any_sgpr)
    bad = 0
    for name in list(old) + [n for n in new if n not in old]:
        if name not in old or name not in new:
            print(f"{name}: ONLY IN {'OLD' if name in old else 'NEW'}")
            bad += 1
            continue
        (a, fa), (b, fb) = old[name], new[name]
        if a == b and fa == fb:
            print(f"{name}: IDENTICAL ({len(a)} lines)")
            continue
        bad += 1
        print(f"{name}: DIFFERENT")
        print("  figures old " + ", ".join(f"{k} {v}" for k, v in fa.items()))
        print("  figures new " + ", ".join(f"{k} {v}" for k, v in fb.items()))
        ca, cb = mnemonic_counts(a), mnemonic_counts(b)
        for op in sorted(set(ca) | set(cb)):
            if ca[op] != cb[op]:
                print(f"  count {op}: {ca[op]} -> {cb[op]}")
        for ln in difflib.unified_diff(a, b, "old", "new", n=args.context, lineterm=""):
            print("  " + ln)
    print(f"{len(old)} / {len(new)} kernels, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
