"""Compare two sets of AMDGPU assembly files (`hipcc --save-temps`: *-gfx950.s) kernel by kernel.

Per kernel symbol: the four resource figures of its `.amdhsa_kernel` block (next_free_vgpr, next_free_sgpr,
group_segment_fixed_size, private_segment_fixed_size) and the histogram of its opcodes.  Two kernels MATCH if the figures
are equal and the opcode multisets are equal once scalar-ALU and branch instructions (`s_*` other than `s_waitcnt` and
`s_barrier`) are set aside: those follow from how the compiler lays out control flow and address arithmetic, not from what
the vector units, LDS and memory are asked to do.  Kernels whose name matches --free are reported but not held to it.
Exit status 1 if a held kernel differs or exists on one side only.

    python tools/isa_compare.py OLD.s[,OLD2.s,...] NEW.s[,NEW2.s,...] [--free REGEX] [--verbose]

Either side may be several files, separated by commas: a kernel meets its counterpart by name, whichever file holds it (code
that moved between translation units).  A kernel defined in two files of one side is an error.
"""
import argparse
import collections
import re
import subprocess
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
KEPT_SCALAR = ("s_waitcnt", "s_barrier")


def parse(path):
    """{kernel name: (figures dict, Counter of opcodes, instruction text)}; the name is the demangled symbol without its
    parameter list, so a kernel whose signature changed still meets its counterpart"""
    text = open(path).read().split("\n")
    kernels, figures = {}, {}
    sym, body = None, []
    for line in text:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            figures[m.group(1)] = cur = {}
            continue
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", line)
        if m and m.group(1) in FIGURES:
            cur[m.group(1)] = m.group(2)
            continue
        m = re.match(r"(\w+):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            sym, body = m.group(1), []
            continue
        if sym and re.match(r"\.Lfunc_end\d+:", line):
            kernels[sym] = body
            sym = None
            continue
        if sym:
            code = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())      # (labels carry the function's number)
            if code and not code.startswith(".") and not code.endswith(":"):
                body.append(code)
    out = {}
    pretty = demangle(sorted(figures))
    for s, f in figures.items():
        ops = collections.Counter(c.split()[0] for c in kernels.get(s, []))
        out[re.sub(r"^void ", "", pretty[s]).split("(")[0]] = (f, ops, "\n".join(kernels.get(s, [])))
    return out


def parse_all(paths):
    """parse() over a comma-separated list of files, merged; a kernel name may come from one of them only"""
    out = {}
    for path in paths.split(","):
        one = parse(path)
        twice = sorted(set(one) & set(out))
        if twice:
            sys.exit(f"{path}: kernels already defined in an earlier file of the same side: {', '.join(twice)}")
        out.update(one)
    return out


def held(ops):
    return collections.Counter({o: c for o, c in ops.items() if not o.startswith("s_") or o in KEPT_SCALAR})


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old", help="assembly file, or several separated by commas")
    ap.add_argument("new", help="assembly file, or several separated by commas")
    ap.add_argument("--free", default=None, help="regex on the demangled name: kernels reported but not held to the condition")
    ap.add_argument("--verbose", action="store_true", help="print the full opcode histogram of every kernel")
    a = ap.parse_args()
    A, B = parse_all(a.old), parse_all(a.new)
    names = sorted(set(A) | set(B))
    nsame = nmatch = 0
    bad, free_diff = [], []
    for name in names:
        free = bool(a.free and re.search(a.free, name))
        if name not in A or name not in B:
            print(f"{name}: only in {'old' if name in A else 'new'}{' (free)' if free else ''}")
            (free_diff if free else bad).append(name)
            continue
        (fa, oa, ta), (fb, ob, tb) = A[name], B[name]
        fig = " ".join(f"{k}={fa.get(k)}" + ("" if fa.get(k) == fb.get(k) else f"->{fb.get(k)}") for k in FIGURES)
        if ta == tb and fa == fb:
            verdict = "identical"
            nsame += 1
        elif fa == fb and held(oa) == held(ob):
            verdict = "match"
            nmatch += 1
        else:
            verdict = "DIFFERS (free)" if free else "DIFFERS"
            (free_diff if free else bad).append(name)
        print(f"{name}: {verdict}  {fig}  instructions={sum(oa.values())}->{sum(ob.values())}")
        if verdict != "identical":
            for o in sorted(set(oa) | set(ob)):
                if oa[o] != ob[o]:
                    mark = "" if o.startswith("s_") and o not in KEPT_SCALAR else "  <-- held"
                    print(f"    {o}: {oa[o]} -> {ob[o]}{mark}")
        if a.verbose:
            print("    " + " ".join(f"{o}:{c}" for o, c in sorted(ob.items())))
    print(f"SUMMARY kernels={len(names)} identical={nsame} match={nmatch} differ_free={len(free_diff)} differ_held={len(bad)}")
    for n in bad:
        print(f"HELD KERNEL DIFFERS: {n}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
