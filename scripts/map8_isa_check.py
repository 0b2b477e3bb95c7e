#!/usr/bin/env python3
"""Do the fp16 instantiations of attn_self_kernel compile to the same code as in another revision of csrc/attn_self.hip?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffast-math -fno-finite-math-only -S --cuda-device-only \\
          -Rpass-analysis=kernel-resource-usage fatezero_amd/csrc/attn_self.hip -o new.s 2> new.rpt      (same for the other revision -> old.s)
    python scripts/map8_isa_check.py old.s new.s new.rpt

Prints, per kernel of old.s, whether new.s holds the same instruction stream (comments, directives and branch-label numbers
removed), then the compiler's resource report of every D = 40 / 64 / 80 / 160 instantiation of new.s.

Any other kernel template, by the prefix of its mangled name (e.g. igemm_kernel of csrc/igemm.hip):

    python scripts/map8_isa_check.py --prefix _Z12igemm_kernel [--dropped-arg N] old.s new.s [old.rpt new.rpt]

Prints, per kernel of NEW.s, whether old.s holds the same instruction stream, then the kernels of old.s that new.s no longer has; with the
two resource reports, per kernel of new.s whether VGPRs / AGPRs / scratch / LDS / occupancy are equal, and the instruction-count difference.
--dropped-arg N: new.s was compiled after the template lost its N-th parameter (0-based) -- a kernel of old.s is matched with that
argument taken out of its name, and the value it had there is shown for the kernels that disappeared."""
import re
import sys

MODES = {0: "FLASH", 1: "CAPTURE", 2: "INJECT", 3: "CAPTURE8", 4: "INJECT8", 5: "CAPTURE8U", 6: "INJECT8U"}


def kernels(path, prefix="_Z16attn_self_kernel"):
    out = {}
    for m in re.finditer(r"^(%s\w+):.*?\n(.*?)^\s*s_endpgm" % re.escape(prefix), open(path).read(), re.S | re.M):
        lines = [ln.split(";")[0].rstrip() for ln in m.group(2).split("\n") if not ln.strip().startswith((";", "."))]
        out[m.group(1)] = [re.sub(r"\.LBB\d+_", ".LBBn_", ln) for ln in lines if ln.strip()]
    return out


def ident(name):
    m = re.match(r"_Z16attn_self_kernelILi(\d+)ELi(\d)ELi0E", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


RES = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def resources(path):
    out, cur = {}, None
    for m in re.finditer(r"remark: (.*?) \[-Rpass", open(path).read()):
        k, _, v = m.group(1).strip().partition(":")
        if k == "Function Name":
            cur = out.setdefault(v.strip(), {})
        elif cur is not None:
            cur[k.strip()] = v.strip()
    return out


def drop_arg(name, prefix, n):
    """(name without its n-th template argument, that argument)"""
    args = re.findall(r"L[a-z]n?\d+E", name[len(prefix):])
    if n >= len(args):
        return name, None
    return name.replace("".join(args), "".join(args[:n] + args[n + 1:]), 1), args[n]


def main_prefix(argv):
    prefix, dropped = argv[argv.index("--prefix") + 1], None
    if "--dropped-arg" in argv:
        dropped = int(argv[argv.index("--dropped-arg") + 1])
    files = [a for i, a in enumerate(argv) if not a.startswith("--") and argv[i - 1] not in ("--prefix", "--dropped-arg")]
    old, new = kernels(files[0], prefix), kernels(files[1], prefix)
    old_name = {(drop_arg(k, prefix, dropped)[0] if dropped is not None else k): k for k in old
                if dropped is None or drop_arg(k, prefix, dropped)[0] in new}
    same = 0
    for name in sorted(new):
        o = old.get(old_name.get(name))
        same += o == new[name]
        print("%-100s %5d instructions  %s" % (name[len(prefix):], len(new[name]), "missing in old" if o is None else "identical" if o == new[name] else "DIFFERENT"))
    print("identical: %d of %d kernels of %s" % (same, len(new), files[1]))
    gone = sorted(set(old) - set(old_name.values()))
    print("kernels of %s that %s no longer has: %d" % (files[0], files[1], len(gone)))
    for name in gone:
        print("    %s%s" % (name[len(prefix):], "" if dropped is None else "   (argument %d = %s)" % (dropped, drop_arg(name, prefix, dropped)[1])))
    ok = same == len(new)
    if len(files) > 3:
        ro, rn = resources(files[2]), resources(files[3])
        print("\n%-100s %s  instructions" % ("kernel", "  ".join(RES)))
        for name in sorted(new):
            a, b = ro.get(old_name.get(name), {}), rn[name]
            eq = all(a.get(k) == b[k] for k in RES)
            ok = ok and eq
            print("%-100s %s  %s  %+d" % (name[len(prefix):], "  ".join(b[k] for k in RES), "equal" if eq else "DIFFERENT from %s" % [a.get(k) for k in RES],
                                         len(new[name]) - len(old.get(old_name.get(name), []))))
    return 0 if ok else 1


def main():
    if "--prefix" in sys.argv:
        return main_prefix(sys.argv[1:])
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = 0
    for name in sorted(old, key=ident):
        d, mode = ident(name)
        eq = name in new and old[name] == new[name]
        same += eq
        print("D=%-3d %-8s %5d instructions  %s" % (d, MODES[mode], len(old[name]), "identical" if eq else "DIFFERENT"))
    print("identical: %d of %d kernels of %s" % (same, len(old), sys.argv[1]))
    if len(sys.argv) > 3:
        rows, cur = [], None
        for m in re.finditer(r"remark: (.*?) \[-Rpass", open(sys.argv[3]).read()):
            t = m.group(1).strip()
            if t.startswith("Function Name:"):
                cur = ident(t.split(":", 1)[1].strip())
                if cur:
                    rows.append([cur, {}])
            elif cur and ":" in t:
                k, v = t.split(":", 1)
                rows[-1][1][k.strip()] = v.strip()
        print("\n%-5s %-9s %6s %6s %6s %8s %10s %10s" % ("D", "mode", "VGPRs", "AGPRs", "SGPRs", "scratch", "waves/SIMD", "LDS bytes"))
        for (d, mode), r in sorted(rows):
            if d in (40, 64, 80, 160):
                print("%-5d %-9s %6s %6s %6s %8s %10s %10s" % (d, MODES[mode], r["VGPRs"], r["AGPRs"], r["TotalSGPRs"], r["ScratchSize [bytes/lane]"],
                                                               r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]))
    return 0 if same == len(old) else 1


if __name__ == "__main__":
    sys.exit(main())
