"""Compiler resource usage of every kernel instantiation in csrc/*.hip files, as one text table: VGPRs, AGPRs, SGPRs, scratch
bytes per lane, LDS bytes and waves per SIMD, from hipcc's -Rpass-analysis=kernel-resource-usage remarks (no GPU needed).

    python tools/resource_table.py [--csrc DIR] [--label TEXT] xattn.hip attention.hip hsattn.hip f32_ops.hip > table.txt
    python tools/resource_table.py --diff before.txt after.txt     # fails when a kernel gained scratch or lost occupancy
    python tools/resource_table.py --diff both.txt both.txt --sections "parent commit" "this commit"   # two labelled tables in one file
    python tools/resource_table.py --diff before.txt after.txt --defaulted-false   # a kernel template gained a trailing `bool = false` parameter:
                                                                                    # its <..., false> instantiation is compared with the old name

Two tables of two commits compare line by line: the kernels are sorted by their mangled name."""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
        ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "waves"))


def flags_for(src):
    base = ["--offload-arch=gfx950", "-O3", "-std=c++17"]
    if src == "mlp.hip":
        return base + ["-mllvm", "-amdgpu-use-amdgpu-trackers=1"]
    if src in ("mlp3.hip", "geglu3.hip"):
        return base
    return base + ["-mllvm", "-amdgpu-mfma-vgpr-form"]


def remarks(csrc, src):
    r = subprocess.run(["/opt/rocm/bin/hipcc", *flags_for(src), "-S", "--cuda-device-only", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?)(\s*\[-Rpass.*)?$", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = rows.setdefault(t.split(":", 1)[1].strip(), {})
            continue
        for text, key in KEYS:
            if cur is not None and t.startswith(text + ":"):
                cur[key] = int(t.rsplit(":", 1)[1])
    return rows


def parse(path, section=None):
    """the rows of a table file; ``section``: only those under the "# <section>" label line (a file holding several tables)"""
    out, on = {}, section is None
    for line in open(path):
        if section is not None and line.startswith("# ") and len(line.split()) <= 4 and "file" not in line:
            on = line[2:].strip() == section
        if not on:
            continue
        f = line.split()
        if len(f) == 8 and f[0].endswith(".hip"):
            out[(f[0], f[7])] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "lds", "waves"), map(int, f[1:7])))
    return out


def under_old_names(a, b):
    """``b`` with every kernel whose template gained a trailing ``bool = false`` parameter since ``a`` filed under its name in ``a`` (Itanium
    mangling: the template argument list ends "...ELb0EEEv" where it ended "...EEEv"); its <..., true> instantiations stay new kernels"""
    b = dict(b)
    for src, name in [k for k in b if k not in a]:
        old = (src, name.replace("ELb0EEEv", "EEEv", 1))
        if old == (src, name):
            continue
        if old not in a:
            # the flag also selects the kernel's parameter type (attn_kernel's AttnArg<MULTI>::type): the parameter list is then mangled as a
            # dependent type, so match on the template argument list alone when exactly one old kernel carries it
            head = old[1].split("EEEv", 1)[0] + "EEEv"
            same = [k for k in a if k[0] == src and k[1].startswith(head) and k not in b]
            if len(same) != 1:
                continue
            old = same[0]
        if old not in b:
            b[old] = b.pop((src, name))
    return b


def diff(before, after, sections=(None, None), defaulted_false=False):
    a, b = parse(before, sections[0]), parse(after, sections[1])
    if defaulted_false:
        b = under_old_names(a, b)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("only in %s: %s %s" % ("after" if k in b else "before", *k))
            bad += k not in b
            continue
        if a[k] != b[k]:
            worse = b[k]["scratch"] > a[k]["scratch"] or b[k]["waves"] < a[k]["waves"]
            bad += worse
            print("%s %s %s: %s -> %s" % ("WORSE" if worse else "moved", *k, a[k], b[k]))
    print("%d kernels before, %d after, %d gained scratch or lost occupancy" % (len(a), len(b), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ap-adapter_amd", "csrc"))
    ap.add_argument("--label", default="")
    ap.add_argument("--diff", nargs=2)
    ap.add_argument("--sections", nargs=2, default=(None, None))
    ap.add_argument("--defaulted-false", action="store_true")
    ap.add_argument("srcs", nargs="*")
    a = ap.parse_args()
    if a.diff:
        sys.exit(diff(*a.diff, sections=tuple(a.sections), defaulted_false=a.defaulted_false))
    with ThreadPoolExecutor(4) as ex:
        tabs = list(ex.map(lambda s: remarks(a.csrc, s), a.srcs))
    if a.label:
        print("# " + a.label)
    print("# %-11s %5s %5s %5s %7s %6s %5s  %s" % ("file", "VGPR", "AGPR", "SGPR", "scratch", "LDS", "waves", "kernel"))
    for src, rows in zip(a.srcs, tabs):
        for name in sorted(rows):
            r = rows[name]
            print("%-13s %5d %5d %5d %7d %6d %5d  %s" % (src, r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"], r["waves"], name))


if __name__ == "__main__":
    main()
