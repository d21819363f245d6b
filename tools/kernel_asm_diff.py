"""Kernel-by-kernel text diff of two sets of gfx950 device assembly listings.

A refactor of the device sources must leave every kernel's code unchanged.  Build both
trees' listings with the Makefile's flags plus `--cuda-device-only -S`, one .s per .hip:

  for f in modular_rl_amd/csrc/*.hip; do
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Iinclude \
      --cuda-device-only -S $f -o OUT/$(basename $f .hip).s; done

  python tools/kernel_asm_diff.py BASE_DIR NEW_DIR [--rename 'REGEX=REPLACEMENT' ...]

Kernels are matched by demangled name over all listings of a directory (a kernel may move
between units).  Compared per kernel: the text between its entry label and its end label,
and its .amdhsa_kernel descriptor block.  Block labels carry the function's index in its
unit and a kernel's own mangled name appears in its LDS symbols; both are normalised.
--rename rewrites demangled BASE names before matching (a dropped template argument).
Exit status 0: every NEW kernel equals its BASE kernel; the kernels only in BASE are listed.
"""
import argparse
import glob
import os
import re
import subprocess
import sys


def kernels(directory):
    """{mangled name: (body lines, descriptor lines)} over every .s of the directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
        for name in names:
            start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
            d0 = next(i for i, ln in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"$", ln))
            d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])

            def norm(ls):
                ls = [re.sub(r"BB\d+_(?=\d)", "BB_", ln.replace(name, "KERNEL")) for ln in ls]
                # a label's trailing comment is aligned to a column: collapse the padding
                return [re.sub(r"^(\.LBB_\d+:)\s+;", r"\1 ;", ln) for ln in ls]

            out[name] = (norm(lines[start + 1:end]), norm(lines[d0 + 1:d1]))
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.split("\n")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[])
    args = ap.parse_args()
    base, new = kernels(args.base), kernels(args.new)
    bn, nn = demangle(list(base)), demangle(list(new))
    for rule in args.rename:
        pat, rep = rule.split("=", 1)
        bn = {k: re.sub(pat, rep, v) for k, v in bn.items()}
    base_by = {bn[k]: base[k] for k in base}
    new_by = {nn[k]: new[k] for k in new}
    assert len(base_by) == len(base) and len(new_by) == len(new), "demangled names collide"
    bad = 0
    for name in sorted(new_by):
        if name not in base_by:
            print("ONLY IN NEW:", name)
            bad += 1
        elif new_by[name] != base_by[name]:
            print("DIFFERS:", name)
            bad += 1
    gone = sorted(set(base_by) - set(new_by))
    for name in gone:
        print("only in base:", name)
    print(f"{len(new_by)} kernels in new, {len(base_by)} in base, {len(new_by) - bad} identical, "
          f"{bad} differing or new, {len(gone)} only in base")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
