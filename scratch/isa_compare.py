#!/usr/bin/env python3
"""Compare two device-only assembly listings kernel by kernel: isa_compare.py [--kernarg-size] [--pair OLD=NEW ...] parent.s branch.s [more.s ...]

For every .amdhsa_kernel of the first two files: the text from the kernel's label to the end of the function (every s_endpgm) and the
.amdhsa_* descriptor block (registers, LDS, scratch) must be the same text.  Emission order is ignored.  Every further
file must hold no kernel at all (host-only units).  Exit status 1 on any difference.  --pair OLD=NEW compares the parent's kernel
OLD with the branch's kernel NEW (a kernel that was renamed, or became a template's instantiation): NEW's text is read with the name
OLD in it.  A name that holds OLD or NEW as a substring is enough, as long as it fits one kernel.  --kernarg-size (first): the
.amdhsa_kernarg_size line is left out of the comparison -- an argument struct that grew at its END moves no load of the fields in front.

The listings come from
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include --cuda-device-only -S UNIT.hip -o UNIT.s
run in imageclust_amd/csrc.
"""
import re
import sys


KERNARG_SIZE = False


def kernels(path):
    lines = open(path).read().split("\n")
    if KERNARG_SIZE:
        lines = [ln for ln in lines if not ln.strip().startswith(".amdhsa_kernarg_size")]
    out = {}
    label = {ln.split(";")[0].strip(): i for i, ln in enumerate(lines) if ln[:1] not in (" ", "\t", "")}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        j = i
        while not lines[j].strip().startswith(".end_amdhsa_kernel"):
            j += 1
        desc = "\n".join(x.strip() for x in lines[i:j + 1])
        a = label[name + ":"]
        b = a
        while not lines[b].startswith(".Lfunc_end"):  # past the last s_endpgm of the function
            b += 1
        # block labels carry the function's emission index (.LBB<index>_<block>), and so do the loop comments that name them (BB<index>_<block>):
        # drop the index, keep everything else
        lines[a] = re.sub(r":\s+;", ": ;", lines[a])  # (the comment behind the label is aligned to a column: a longer name moves it)
        # (... and the comment behind a block label is aligned to a column too: an index of two digits moves it)
        text = re.sub(r"(?m)^(\.LBB_\d+:)\s+;", r"\1 ;", re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(lines[a:b])))
        out[name] = (re.sub(r"\bBB\d+_", "BB_", text), desc)
    return out


def main():
    global KERNARG_SIZE
    argv, pairs = sys.argv[1:], []
    if argv and argv[0] == "--kernarg-size":
        KERNARG_SIZE, argv = True, argv[1:]
    while argv and argv[0] == "--pair":
        pairs.append(argv[1].split("="))
        argv = argv[2:]
    pa, pb, rest = argv[0], argv[1], argv[2:]
    A, B = kernels(pa), kernels(pb)
    for old, new in pairs:
        (old,), (new,) = [n for n in A if old in n], [n for n in B if new in n]
        # (an instantiation has a section of its own; the directive that returns to it behind the descriptor is no code: read it as .text)
        B[old] = tuple(re.sub(r"(?m)^\t\.section\t\.text\.%s,.*$" % re.escape(old), "\t.text", t.replace(new, old)) for t in B.pop(new))
        print("paired: %s (parent) with %s" % (old, new))
    bad = 0
    print("%s: %d kernels, %s: %d kernels, same names: %s" % (pa, len(A), pb, len(B), sorted(A) == sorted(B)))
    for name in sorted(set(A) | set(B)):
        if name not in A or name not in B:
            verdict = "only in " + (pa if name in A else pb)
        else:
            verdict = "identical" if A[name] == B[name] else "differs (%s)" % ("code" if A[name][0] != B[name][0] else "descriptor")
        bad += verdict != "identical"
        print("  %-9s %s" % (verdict, name))
    for p in rest:
        n = len(kernels(p))
        bad += n != 0
        print("%s: %d kernels (host-only unit: expected 0)" % (p, n))
    print("ALL IDENTICAL" if not bad else "%d DIFFERENCES" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
