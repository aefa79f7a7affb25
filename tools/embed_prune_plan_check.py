"""The sizing functions of csrc/embed_prune_plan.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/embed_prune_plan_check.py [--keep DIR]

Builds tools/probe/embed_prune_plan_check.cpp (a stand-alone program with its own main that includes only embed_prune_plan.hpp; host code with
-fsanitize=address,undefined) and runs it: how the device buffers of an embed-and-prune run (tsc_embed_prune_*) grow as slabs append their kept
poses -- at 0 rows, 1, an exact power of two, one above, config 5's 500 000 and the end of the prune's range --, where a slab's rows start, and
a replay of whole runs on host arrays sized exactly as the plan says.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="embed_prune_plan_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "embed_prune_plan_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "embed_prune_plan_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"embed_prune_plan_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
