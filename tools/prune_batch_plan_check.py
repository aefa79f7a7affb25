"""The tables of csrc/prune_batch_plan.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/prune_batch_plan_check.py [--keep DIR]

Builds tools/probe/prune_batch_plan_check.cpp (a stand-alone program with its own main that includes only prune_batch_plan.hpp; hipcc, host code
with -fsanitize=address,undefined) and runs it: what the many-ensembles RMSD prune (tsc_prune_rmsd_batch, tsc_prune_rmsd_team and their _dev
forms) hands its kernels -- the segments' offsets at 0 .. 129 structures, an empty batch, every refusal with its message, the schedule, its gate
and the slot lists, both launch orders on a batch with ties -- and a replay of the team route's bit-array indexing on host arrays of exactly
the planned size.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="prune_batch_plan_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "prune_batch_plan_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "prune_batch_plan_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"prune_batch_plan_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
