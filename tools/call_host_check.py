"""The argument checks and the width dispatch of csrc/call.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/call_host_check.py [--keep DIR]

Builds tools/probe/call_host_check.cpp (a stand-alone program with its own main that includes only call.hpp; hipcc, host code with
-fsanitize=address,undefined) and runs it: valid class tables of one and of sixteen classes, shared and per-structure index lists on
512 atoms with the indices -1, 0 and 511, every refusal with its message, the word counts of 1 .. 512 atoms.  Every array lives in a
heap block of exactly its documented size.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="call_host_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "call_host_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "call_host_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"call_host_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
