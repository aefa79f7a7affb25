"""The sizing functions of csrc/cross_plan.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/cross_plan_check.py [--keep DIR]

Builds tools/probe/cross_plan_check.cpp (a stand-alone program with its own main that includes only cross_plan.hpp; hipcc, host code with
-fsanitize=address,undefined) and runs it: the padded atom counts and the path they select, the segment width and count and the grid of a
cross-set RMSD call at both extremes (one query against 10^6, 10^5 queries against a few hundred), at the test shapes and at 2^31 - 1
structures a side, the rows a launch may take under a byte budget, and a replay of the work items' indexing on host arrays of the sizes the
library allocates.  Needs no GPU."""

import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscode_amd.build import _hipcc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="directory for the program (default: a temporary one)")
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="cross_plan_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "cross_plan_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "cross_plan_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"cross_plan_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
