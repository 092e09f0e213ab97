#!/usr/bin/env python3
"""Compare the device functions of two gfx950 assembly files (the `make asm` output) one by one.

    tools/asm_kernels_equal.py before.s after.s

For every function: the instruction stream and, for a kernel, its .amdhsa_ descriptor block, with
comments dropped and compiler-local labels (.LBB12_3, .Lfunc_end12, .Ltmp4, ...) renamed in order
of first appearance, so that a function that only moved inside the file compares equal.  Prints
one line per function -- equal / DIFFERENT (first differing line) / only in one file -- and exits
0 only if every function of either file is in both and equal.  A refactor that must not change
a kernel by an instruction is checked with this and `make resource-usage`.

Not compared: the .amdgpu_metadata section (each kernel's argument layout and kernarg preload
count, as the runtime reads them) and the data sections (.rodata tables, LDS symbols).  A change
that touches a kernel's argument list or a device table needs those looked at separately, e.g.
by diffing the two files' metadata sections with the kernel entries sorted by name.
"""
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_$]*\d+(?:_\d+)?")


def functions(path):
    """name -> (is_kernel, [normalised lines])"""
    out, kernels = {}, set()
    name, body, typed = None, None, set()
    desc = None
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            typed.add(m.group(1))
            continue
        if name is None and line.endswith(":") and line[:-1] in typed:
            name, body = line[:-1], []
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            desc = m.group(1)
            kernels.add(desc)
            continue
        if desc is not None:
            if line == ".end_amdhsa_kernel":
                desc = None
            elif desc == name:          # the descriptor stands inside its function's text
                body.append(line)
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if line.startswith((".section", ".p2align", ".loc", ".file", ".cfi_")):
            continue
        body.append(line)
    res = {}
    for fn, lines in out.items():
        names = {}
        res[fn] = (fn in kernels,
                   [LOCAL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), x)
                    for x in lines])
    return res


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for fn in sorted(set(a) | set(b)):
        kind = "kernel  " if (a.get(fn) or b.get(fn))[0] else "function"
        if fn not in a or fn not in b:
            bad += 1
            print(f"{kind} ONLY IN {'first' if fn in a else 'second'}  {fn}")
            continue
        la, lb = a[fn][1], b[fn][1]
        if la == lb:
            print(f"{kind} equal      {len(la):6d} lines  {fn}")
            continue
        bad += 1
        i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        print(f"{kind} DIFFERENT  {len(la):6d} / {len(lb):6d} lines, first at {i}  {fn}")
        print(f"    < {la[i] if i < len(la) else '(end)'}")
        print(f"    > {lb[i] if i < len(lb) else '(end)'}")
    n_k = sum(1 for v in b.values() if v[0])
    print(f"{len(b)} functions ({n_k} kernels) in the second file; {bad} differ or are missing")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
