#!/usr/bin/env python3
"""Compare two device assembly listings of one source file kernel by kernel (`hipcc --offload-arch=gfx950 <the Makefile's flags>
--offload-device-only -S file.hip -o file.s` on two trees).  Kernels are found by their `.amdhsa_kernel` descriptors; a kernel's text is
everything between its label and its `.Lfunc_end`, comments stripped and block labels renumbered in order of appearance.  Prints the
two symbol sets' differences, then for every kernel whose text differs the mnemonics whose counts differ (parent -> change), then
how many kernels were compared and how many are identical.  It classifies nothing: which differences matter is for the reader.
usage: isa_diff.py PARENT.s CHANGE.s [--desc]      (--desc: also compare the .amdhsa_ descriptor lines)"""
import collections
import re
import subprocess
import sys


def kernels(path):
    """-> {symbol: (instruction lines, descriptor lines)}"""
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        labels, text = {}, []
        for ln in lines[start + 1:end]:
            ln = re.sub(r"\s*(;|//).*$", "", ln).strip()
            if ln and not ln.startswith("."):
                text.append(ln)
            elif ln.endswith(":"):
                text.append(ln)
        for ln in text:          # block labels: .LBB12_3 -> L0, L1, ... in order of definition
            if ln.endswith(":"):
                labels.setdefault(ln[:-1], f"L{len(labels)}")
        pat = re.compile(r"\.L[A-Za-z_]*\d+_\d+")
        text = [pat.sub(lambda m: labels.get(m.group(0), m.group(0)), ln) for ln in text]
        d0 = next(i for i, ln in enumerate(lines) if ln.strip() == ".amdhsa_kernel " + name)
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        out[name] = (text, [ln.strip() for ln in lines[d0 + 1:d1]])
    return out


def demangle(names):
    for tool in ("llvm-cxxfilt", "c++filt"):
        try:
            res = subprocess.run([tool] + names, capture_output=True, text=True).stdout.split("\n")
            return {n: (r.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0] or n) for n, r in zip(names, res)}
        except OSError:
            continue
    return {n: n for n in names}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = kernels(args[0]), kernels(args[1])
    short = demangle(sorted(set(a) | set(b)))
    for n in sorted(set(a) - set(b)):
        print(f"only in parent: {short[n]}")
    for n in sorted(set(b) - set(a)):
        print(f"only in change: {short[n]}")
    same = lines = 0
    for n in sorted(set(a) & set(b)):
        (ta, da), (tb, db) = a[n], b[n]
        lines += len(ta)
        if ta == tb and (da == db or "--desc" not in sys.argv):
            same += 1
            continue
        ca = collections.Counter(ln.split()[0] for ln in ta if not ln.endswith(":"))
        cb = collections.Counter(ln.split()[0] for ln in tb if not ln.endswith(":"))
        diff = [f"{m} {ca[m]} -> {cb[m]}" for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]]
        print(f"{short[n]}: {len(ta)} -> {len(tb)} lines; " + ("; ".join(diff) if diff else "same mnemonic counts (order or operands differ)"))
        if "--desc" in sys.argv:
            for x, y in zip(da, db):
                if x != y:
                    print(f"    descriptor: {x} -> {y}")
    both = len(set(a) & set(b))
    print(f"{len(a)} kernels in parent, {len(b)} in change, {both} in both, {same} identical, {both - same} differ; {lines} parent lines compared")


if __name__ == "__main__":
    main()
