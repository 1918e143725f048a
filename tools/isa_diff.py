#!/usr/bin/env python3
"""Compare the gfx950 code of csrc files between two checkouts, kernel by kernel (no GPU needed).

    tools/isa_diff.py OLD NEW gemm_x3.hip                                   same file on both sides
    tools/isa_diff.py OLD NEW gemm.hip --new-files gemm.hip gemm_tn.hip     a file that was split

OLD / NEW are repository roots.  Every file is compiled to device assembly with the flags of
epn_pointcloud_amd/build.py plus `-S --cuda-device-only` (as tools/kres.sh runs hipcc), the output is cut into kernels
(identity = demangled name; the kernels of all files of a side are pooled) and for every kernel on both sides two things
are compared: the instruction stream -- comments, debug / alignment directives dropped, local labels renumbered in order of
appearance -- and the `.amdhsa_` descriptor lines (VGPRs, AGPRs, SGPRs, scratch, LDS, ...).  Exit status 1 on any difference.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]   # build.py FLAGS
LOCAL = re.compile(r"\.L[A-Za-z_]+[0-9_]*")
SKIP = (".loc", ".file", ".cfi_", ".p2align", ".section", ".text", ".globl", ".protected", ".hidden", ".type", ".size", ".weak")


def assemble(root, name, extra, out_dir, tag):
    src = os.path.join(root, "epn_pointcloud_amd", "csrc", name)
    out = os.path.join(out_dir, f"{tag}_{name}.s")
    subprocess.check_call([HIPCC] + FLAGS + extra + ["-S", "--cuda-device-only", src, "-o", out],
                          stderr=subprocess.DEVNULL)
    return out


def kernels_of(path):
    """{mangled name: (instruction lines, descriptor lines)} of one assembly file"""
    body, desc, cur, in_desc = {}, {}, None, None
    for raw in open(path):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if in_desc is not None:
            if line == ".end_amdhsa_kernel":
                in_desc = None
            else:
                desc[in_desc].append(" ".join(line.split()))
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            in_desc = m.group(1)
            desc[in_desc] = []
            continue
        m = re.match(r"([A-Za-z_][\w$.]*):$", line)
        if m and not line.startswith(".L"):
            cur = m.group(1)
            body[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None and not line.startswith(SKIP):
            body[cur].append(" ".join(line.split()))
    out = {}
    for k in desc:
        names = {}
        lines = [LOCAL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), l) for l in body.get(k, [])]
        out[k] = (lines, desc[k])
    return out


def side(root, files, extra, out_dir, tag):
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        paths = list(ex.map(lambda f: assemble(root, f, extra, out_dir, tag), files))
    pool = {}
    for p in paths:
        pool.update(kernels_of(p))
    names = list(pool)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d: pool[n] for n, d in zip(names, dem)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("file", help="csrc file name, e.g. gemm.hip")
    ap.add_argument("--old-files", nargs="+", help="files of OLD whose kernels are pooled (default: FILE)")
    ap.add_argument("--new-files", nargs="+", help="files of NEW whose kernels are pooled (default: FILE)")
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides, e.g. -DEPN_TUNING")
    ap.add_argument("--keep", help="directory to keep the .s files in")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    os.makedirs(tmp, exist_ok=True)
    extra = a.flags.split()
    old = side(a.old, a.old_files or [a.file], extra, tmp, "old")
    new = side(a.new, a.new_files or [a.file], extra, tmp, "new")
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    both = sorted(set(old) & set(new))
    bad_isa = [k for k in both if old[k][0] != new[k][0]]
    bad_res = [k for k in both if old[k][1] != new[k][1]]
    for title, rows in (("only in OLD", only_old), ("only in NEW", only_new), ("instruction stream differs", bad_isa),
                        ("resource lines differ", bad_res)):
        for k in rows:
            print(f"{title}: {k}")
    for k in bad_isa:
        o, n = old[k][0], new[k][0]
        first = next((i for i, (x, y) in enumerate(zip(o, n)) if x != y), min(len(o), len(n)))
        print(f"  {k[:90]}: {len(o)} -> {len(n)} lines, first difference at line {first}")
    print(f"{a.file}: {len(old)} kernels old, {len(new)} new, {len(both)} on both sides; only old {len(only_old)}, "
          f"only new {len(only_new)}; instruction streams equal {len(both) - len(bad_isa)}/{len(both)}, "
          f"resource lines equal {len(both) - len(bad_res)}/{len(both)}")
    return 1 if only_old or only_new or bad_isa or bad_res else 0


if __name__ == "__main__":
    sys.exit(main())
