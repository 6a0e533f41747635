#!/usr/bin/env python
"""Compare the gfx950 device code of two revisions of a translation unit, kernel by kernel.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S old/conv_igemm.hip -o parent.s
    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S conv_igemm.hip -o head_a.s      (likewise head_b.s for conv_wgrad.hip)
    python tools/device_code_diff.py --parent parent.s --head head_a.s head_b.s

A refactor that moves kernels between files or touches only host code must leave every kernel as it was.  Per kernel symbol the
instruction text (comments stripped; the numbers in .LBB<n>_<m> and .Lfunc_end<n> follow the function's position in the file and
are dropped) and the .amdhsa_ descriptor block (registers, LDS, private segment) must be equal, and both sides must define the
same set of kernels.  Prints a summary, exits 1 on any difference."""
import argparse
import re
import sys

LABEL_NUMBERS = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1")]


def _normalise(line):
    line = line.split(";", 1)[0].rstrip()
    for pattern, to in LABEL_NUMBERS:
        line = pattern.sub(to, line)
    return line


def kernels(path):
    """{kernel symbol: (instruction lines, descriptor lines)} of one assembly file.  A function runs from its label to
    .Lfunc_end<n>; the .amdhsa_kernel block sits inside that span, and the .set <symbol>.num_vgpr ... lines that follow it hold the
    register counts where the block refers to them by name."""
    with open(path) as fh:
        lines = fh.read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        start = next(k for k in range(i, len(lines)) if lines[k].startswith(sym + ":"))
        end = next(k for k in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
        body = lines[start + 1:end]
        d0 = next((k for k, l in enumerate(body) if l.strip().startswith(".amdhsa_kernel ")), None)
        if d0 is not None:          # device functions that are no kernels have no descriptor and are not compared
            d1 = next(k for k in range(d0, len(body)) if body[k].strip() == ".end_amdhsa_kernel")
            text = [t for t in (_normalise(l) for l in body[:d0] + body[d1 + 1:]) if t.strip()]
            desc = [" ".join(_normalise(l).split()) for l in body[d0 + 1:d1]]
            k = end + 1
            while k < len(lines) and not re.match(r"\s*\.type\s", lines[k]):
                if lines[k].strip().startswith(f".set {sym}."):
                    desc.append(" ".join(_normalise(lines[k]).split()))
                k += 1
            out[sym] = (text, desc)
        i = end + 1
    return out


def collect(paths):
    out, twice = {}, []
    for p in paths:
        for sym, k in kernels(p).items():
            if sym in out and out[sym] != k:        # an internal-linkage kernel of a shared header may repeat, as the same code
                twice.append(sym)
            out[sym] = k
    return out, twice


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--head", nargs="+", required=True)
    a = ap.parse_args()
    (old, old_twice), (new, new_twice) = collect(a.parent), collect(a.head)
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    text_differs = sorted(s for s in set(old) & set(new) if old[s][0] != new[s][0])
    desc_differs = sorted(s for s in set(old) & set(new) if old[s][1] != new[s][1])
    instructions = sum(len(k[0]) for k in old.values())
    print(f"parent: {' '.join(a.parent)}: {len(old)} kernel symbols, {instructions} instruction and label lines")
    print(f"head:   {' '.join(a.head)}: {len(new)} kernel symbols, {sum(len(k[0]) for k in new.values())} instruction and label lines")
    for what, syms in (("only in the parent", gone), ("only in the head", added), ("defined twice in the head, differently", new_twice),
                       ("instruction text differs", text_differs), ("descriptor block differs", desc_differs)):
        for s in syms:
            print(f"{what}: {s}")
    bad = bool(gone or added or new_twice or text_differs or desc_differs)
    print("DIFFERENT" if bad else "identical: the same kernel symbols, instruction text and .amdhsa_ descriptor blocks")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
