#!/usr/bin/env python3
"""Same machine code, parent against change: compare the device code of two trees unit by unit.  CPU only, no GPU.

    python tools/device_code_diff.py PARENT_TREE THIS_TREE [--jobs N] [--keep DIR [--reuse-parent]]

Each unit of `tscode_amd.build.SOURCES` (the list of THIS_TREE; a unit only one tree has is reported as such) is compiled in both trees
with the library's CFLAGS plus `--cuda-device-only -S`, and once more with `--cuda-host-only -c` for the host object whose
`__device_stub__` symbols name the kernels the unit launches.  Per function symbol the instruction stream -- and for a kernel its
`.amdhsa_*` descriptor block -- is compared after removing `;` comments and the function index of `.LBB<n>_<m>` labels.  Printed per unit:
kernels in the device code (parent -> this), kernels launched, launched kernels differing, other functions and how many of them differ;
then the totals and the number of distinct kernels.  The exit status is 1 when a launched kernel differs.  (MEASURED.md sections 34, 35.)
"""

import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(tree))), os.path.join(tree, "tscode_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_unit(build, tree, unit, out, reuse=False):
    """unit -> (assembly text, set of launched kernel symbols)"""
    src = os.path.join("tscode_amd", "csrc", unit)
    asm, obj = os.path.join(out, unit + ".s"), os.path.join(out, unit + ".host.o")
    cc = [build._hipcc()] + build.CFLAGS
    if not (reuse and os.path.exists(asm) and os.path.exists(obj)):
        subprocess.run(cc + ["--cuda-device-only", "-S", "-o", asm, src], check=True, cwd=tree)
        subprocess.run(cc + ["--cuda-host-only", "-c", "-o", obj, src], check=True, cwd=tree)
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    if nm:
        syms = subprocess.run([nm, obj], check=True, capture_output=True, text=True).stdout
    else:
        syms = subprocess.run([shutil.which("llvm-objdump") or "/opt/rocm/llvm/bin/llvm-objdump", "-t", obj], check=True, capture_output=True, text=True).stdout
    # the host stub of kernel <len><name> is mangled <len + 15>__device_stub__<name>, inside whatever namespace the kernel is in
    launched = set()
    for word in syms.split():
        m = re.search(r"(\d+)__device_stub__", word)
        if m:
            launched.add(word[:m.start()] + str(int(m.group(1)) - len("__device_stub__")) + word[m.end():])
    return open(asm).read(), launched


def short(symbol):
    """k_name out of a mangled kernel symbol (<length>k_name...), template arguments dropped"""
    for m in re.finditer(r"\d+(?=k_)", symbol):
        for i in range(len(m.group())):              # (_GLOBAL__N_111k_xchg_push: the length is 11)
            name = symbol[m.end():m.end() + int(m.group()[i:])]
            if re.fullmatch(r"k_[a-z0-9_]+", name) and len(name) == int(m.group()[i:]):
                return name
    return symbol


LABEL = re.compile(r"\.LBB\d+_(\d+)")


def functions(asm):
    """assembly text -> ({symbol: normalised instruction stream}, {kernel symbol: normalised descriptor block})"""
    bodies, descriptors = {}, {}
    name, lines, kernel = None, None, None
    for raw in asm.splitlines():
        line = LABEL.sub(r".LBB_\1", raw.split(";", 1)[0]).strip()
        if kernel is not None:
            if line.startswith(".end_amdhsa_kernel"):
                kernel = None
            elif line:
                descriptors[kernel].append(line)
            continue
        if line.startswith(".amdhsa_kernel"):
            kernel = line.split()[1]
            descriptors[kernel] = []
            continue
        if name is None:
            m = re.fullmatch(r"\.type\s+([^,\s]+),@function", line)
            if m:
                name, lines = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            bodies[name] = "\n".join(lines)
            name = None
        elif line and line != name + ":":
            lines.append(line)
    return bodies, {k: "\n".join(v) for k, v in descriptors.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_tree")
    ap.add_argument("this_tree")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="keep the .s files and host objects in this directory")
    ap.add_argument("--reuse-parent", action="store_true", help="with --keep: take the parent's files from an earlier run of this tool")
    args = ap.parse_args()
    trees = [os.path.abspath(args.parent_tree), os.path.abspath(args.this_tree)]
    builds = [load_build(t) for t in trees]
    units = list(builds[1].SOURCES) + [u for u in builds[0].SOURCES if u not in builds[1].SOURCES]
    work = args.keep or tempfile.mkdtemp(prefix="device_code_diff_")
    outs = [os.path.join(work, side) for side in ("parent", "this")]
    for o in outs:
        os.makedirs(o, exist_ok=True)
    jobs = [(side, u) for u in units for side in (0, 1) if u in builds[side].SOURCES]
    with ThreadPoolExecutor(args.jobs) as pool:
        results = dict(zip(jobs, pool.map(lambda j: compile_unit(builds[j[0]], trees[j[0]], j[1], outs[j[0]], args.reuse_parent and j[0] == 0), jobs)))

    total = dict(parent=0, this=0, launched=0, differing=0, excess=0, others=0, others_differing=0)
    distinct, bad = set(), []
    print(f"{'unit':<20}{'parent':>8}{'this':>8}{'launched':>10}{'differing':>11}{'unlaunched':>12}{'other fns':>11}{'differing':>11}")
    for u in units:
        if (0, u) not in results or (1, u) not in results:
            print(f"{u:<20} only in the {'parent' if (0, u) in results else 'change'}")
            continue
        (pb, pd), (tb, td) = functions(results[0, u][0]), functions(results[1, u][0])
        launched = results[1, u][1]
        assert launched == results[0, u][1], f"{u}: the two trees launch different kernels: {sorted(launched ^ results[0, u][1])}"
        assert launched <= set(td) and launched <= set(pd), f"{u}: a launched kernel is missing from the device code"
        differing = sorted(k for k in launched if pb[k] != tb[k] or pd[k] != td[k])
        others = sorted(set(tb) - launched)
        others_differing = [f for f in others if f not in pb or pb[f] != tb[f] or pd.get(f) != td.get(f)]
        unlaunched = sorted(set(td) - launched)
        print(f"{u:<20}{len(pd):>8}{len(td):>8}{len(launched):>10}{len(differing):>11}{len(unlaunched):>12}{len(others):>11}{len(others_differing):>11}"
              + ("   unlaunched: " + " ".join(short(k) for k in unlaunched) if unlaunched else ""))
        bad += [(u, k) for k in differing]
        distinct |= set(td)
        for key, n in (("parent", len(pd)), ("this", len(td)), ("launched", len(launched)), ("differing", len(differing)),
                       ("excess", len(unlaunched)), ("others", len(others)), ("others_differing", len(others_differing))):
            total[key] += n
    print(f"{'total':<20}{total['parent']:>8}{total['this']:>8}{total['launched']:>10}{total['differing']:>11}{total['excess']:>12}{total['others']:>11}{total['others_differing']:>11}")
    print(f"launched (unit, kernel) pairs: {total['launched']} compared, {total['differing']} differing; "
          f"kernel bodies {total['parent']} -> {total['this']} for {len(distinct)} distinct kernels; files under {work}")
    for u, k in bad:
        print(f"DIFFERS: {u} {k}")
    if not args.keep:
        shutil.rmtree(work)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
