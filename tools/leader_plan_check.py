"""The sizing functions of csrc/leader_plan.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/leader_plan_check.py [--keep DIR]

Builds tools/probe/leader_plan_check.cpp (a stand-alone program with its own main that includes only leader_plan.hpp and, through it,
cross_plan.hpp; hipcc, host code with -fsanitize=address,undefined) and runs it: the blocks of an energy-ordered RMSD prune, the rows of the
last block, the capacity and leading dimension of the growing library pack and the grid of the in-block bits at N = 1, B - 1, B, B + 1 and
2^31 - 1 (B = LEADER_BLOCK), the launches and read-backs of a run, and a replay of a whole run's indexing -- bit words written and read,
rows, columns and norms appended, the library walk's column loads -- on host arrays of the sizes the library allocates.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="leader_plan_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "leader_plan_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "leader_plan_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"leader_plan_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
