#!/usr/bin/env python3
"""
Compare the device code of two builds symbol by symbol.
    hipcc <the Makefile's flags> --cuda-device-only -S unit.hip -o unit.s      (for every unit, both builds)
    python tools/isa_symbols.py old/*.s -- new/*.s
For every kernel and every non-inlined device function it prints the SHA-256 of the symbol's assembly text (code, resource
`.set`s, the compiler's resource comments, `.amdhsa_kernel` block) and of its `amdhsa.kernels` metadata entry on either side,
with the unit each was found in.  Functions may move between units.  Two things are taken out before hashing: lines naming
`__hip_cuid_` (a random symbol per compilation) and the function's ordinal in its unit inside local labels (`.LBB12_3`,
`.Lfunc_end12`, `BB12_3` in loop comments: a function that moves, or whose predecessor does, is renumbered; the padding in front of a
comment follows the label's width).  Exit status 1 if a symbol of the old build
is missing or differs in the new one, or the new one has a symbol the old one lacks.
"""
import hashlib
import os
import re
import sys

LABEL = re.compile(r"(\.L(?:BB|func_begin|func_end|JTI|CPI|tmp)|(?<![\w.])BB)\d+")
BEGIN = re.compile(r"-- Begin function (\S+)")


def symbols(path):
    """{(kind, symbol): sha256} of one assembly file; kind is 'text' or 'meta'"""
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    chunks, cur, pending = {}, None, []
    for l in lines:
        m = BEGIN.search(l)
        if m:
            cur = ("text", m.group(1))
            chunks[cur] = pending if pending and pending[-1].startswith("\t.section\t.text.") else []
        elif ".AMDGPU.gpr_maximums" in l or l.startswith("amdhsa.kernels:"):
            cur = None
        if cur:
            chunks[cur].append(re.sub(r"\s+;", " ;", LABEL.sub(r"\1#", l)))
        pending = [l]
    if "amdhsa.kernels:" in lines:
        entry = []
        for l in lines[lines.index("amdhsa.kernels:") + 1:] + ["x"]:
            if l.startswith("  - ") or not l.startswith("  "):
                name = [e.split()[-1] for e in entry if e.startswith("    .name:")]
                if name:
                    chunks[("meta", name[0])] = entry
                entry = []
                if not l.startswith("  "):
                    break
            entry.append(l)
    for v in chunks.values():                   # (a chunk ends where the next function's section is switched to)
        while v and (v[-1] == "\t.text" or v[-1].startswith("\t.section\t.text.")):
            v.pop()
    return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in chunks.items()}


def side(paths):
    out = {}
    for p in paths:
        unit = os.path.basename(p)
        for k, h in symbols(p).items():
            out.setdefault(k, []).append((unit, h))
    return out


def main():
    cut = sys.argv.index("--")
    old, new = side(sys.argv[1:cut]), side(sys.argv[cut + 1:])
    bad = 0
    for key in sorted(set(old) | set(new)):
        o, n = old.get(key, []), new.get(key, [])
        # a static function that several units use is emitted in each: every copy must match a copy of the other side
        same = bool(o) and bool(n) and {h for _, h in o} == {h for _, h in n}
        bad += not same
        print("%-9s %s %s" % ("same" if same else "DIFFERENT" if o and n else "MISSING" if o else "NEW", key[0], key[1]))
        for tag, rows in (("old", o), ("new", n)):
            for unit, h in rows:
                print("    %s %s  %s" % (tag, h, unit))
    print("%d symbols, %d not identical" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
