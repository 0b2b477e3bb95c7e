#!/usr/bin/env python3
"""Do the fp16 instantiations of attn_self_kernel compile to the same code as in another revision of csrc/attn_self.hip?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffast-math -fno-finite-math-only -S --cuda-device-only \\
          -Rpass-analysis=kernel-resource-usage fatezero_amd/csrc/attn_self.hip -o new.s 2> new.rpt      (same for the other revision -> old.s)
    python scripts/map8_isa_check.py old.s new.s new.rpt

Prints, per kernel of old.s, whether new.s holds the same instruction stream (comments, directives and branch-label numbers
removed), then the compiler's resource report of every D = 40 / 64 / 80 / 160 instantiation of new.s."""
import re
import sys

MODES = {0: "FLASH", 1: "CAPTURE", 2: "INJECT", 3: "CAPTURE8", 4: "INJECT8"}


def kernels(path):
    out = {}
    for m in re.finditer(r"^(_Z16attn_self_kernel\w+):.*?\n(.*?)^\s*s_endpgm", open(path).read(), re.S | re.M):
        lines = [ln.split(";")[0].rstrip() for ln in m.group(2).split("\n") if not ln.strip().startswith((";", "."))]
        out[m.group(1)] = [re.sub(r"\.LBB\d+_", ".LBBn_", ln) for ln in lines if ln.strip()]
    return out


def ident(name):
    m = re.match(r"_Z16attn_self_kernelILi(\d+)ELi(\d)ELi0E", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


def main():
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
