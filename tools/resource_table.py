"""Kernel resources of two builds of one translation unit side by side, as a markdown table.

    hipcc ... -Rpass-analysis=kernel-resource-usage --save-temps=obj -c fg_kernels_fast.hip -o DIR/fast.o 2> DIR/resources.txt
    python tools/resource_table.py PARENT_DIR THIS_DIR [name filter] > profiles/<change>_resources.md

Per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane, LDS bytes per block, occupancy, and the instruction count of its ISA
(the lines of the kernel's body in the saved .s that are neither labels, directives nor comments).  Exit status 1 if a row
differs in anything but the instruction count."""
import glob
import os
import re
import subprocess
import sys

KEYS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
        ("LDS", "LDS Size [bytes/block]"), ("occ", "Occupancy [waves/SIMD]")]


def resources(d):
    out, cur = {}, None
    for ln in open(os.path.join(d, "resources.txt")):
        m = re.search(r"remark: \S+ +(.*?): (\S+) \[-Rpass", ln)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k] = v
    return out


def instructions(d):
    (asm,) = glob.glob(os.path.join(d, "*amdgcn*.s"))
    out, cur = {}, None
    for ln in open(asm):
        s = ln.strip()
        m = re.match(r"^(\w+):", s)
        if m and not s.startswith("."):
            cur = m.group(1)
            out[cur] = 0
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif cur and s and not s.startswith((".", ";")) and not re.match(r"^\.?\w+:", s):
            out[cur] += 1
    return out


def main():
    pd, td = sys.argv[1], sys.argv[2]
    want = sys.argv[3] if len(sys.argv) > 3 else ""
    pr, tr, pi, ti = resources(pd), resources(td), instructions(pd), instructions(td)
    names = sorted(n for n in set(pr) | set(tr) if want in n)
    short = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    print("| kernel | " + " | ".join(k for k, _ in KEYS) + " | instructions | same |")
    print("|---|" + "---|" * (len(KEYS) + 2))
    bad = 0
    for n, s in zip(names, short):
        s = s.replace("(anonymous namespace)::", "").replace("fg::", "").replace("void ", "")
        s = re.sub(r">\(.*", ">", s)   # the kernel and its template arguments, without the parameter list
        a, b = pr.get(n, {}), tr.get(n, {})
        cells = ["%s / %s" % (a.get(key, "-"), b.get(key, "-")) for _, key in KEYS]
        same = all(a.get(key) == b.get(key) and key in a for _, key in KEYS)
        bad += not same
        print("| `%s` | %s | %s / %s | %s |" % (s, " | ".join(cells), pi.get(n, "-"), ti.get(n, "-"),
                                               ("yes" if pi.get(n) == ti.get(n) else "resources") if same else "NO"))
    print("\n%d kernels, %d rows differ (parent / this build in every cell)" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
