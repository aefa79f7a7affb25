"""The sizing functions of csrc/pass_plan.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/pass_plan_check.py [--keep DIR]

Builds tools/probe/pass_plan_check.cpp (a stand-alone program with its own main that includes only pass_plan.hpp; hipcc, host code with
-fsanitize=address,undefined) and runs it: which shape a prune pass takes (chunk-local, culled, walked) and every grid of each, at shapes
worked out by hand -- the walked pass at 57 046 structures and at the limits of its segment and workgroup choices, on several ranks and
with the rows the host has learnt; the chunk-local pass whole and partitioned, at both sides of its chunk limit; the culled pass on one
rank and on five, in both kernel forms.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="pass_plan_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "pass_plan_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "pass_plan_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"pass_plan_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
