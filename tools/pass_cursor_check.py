"""The host's bookkeeping of a stepped prune run (csrc/pass_cursor.hpp) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/pass_cursor_check.py [--keep DIR]

Builds tools/probe/pass_cursor_check.cpp (a stand-alone program with its own main that includes only pass_cursor.hpp; hipcc, host code with
-fsanitize=address,undefined) and runs it: the run's layout numbers against values worked out by hand, and the cursor driven through every
sequence of pass kinds at 1, 20, 21, 41 and 450 structures and through written-out mixed sequences at 450, 57 046 and 10 000 001, against a
model of the device that counts how often each schedule slot is opened and closed -- each runnable slot once and once, never opened before
the slot in front of it is closed or named as the one its opener closes, nothing left open after the export -- with every entry point's
answer checked at every point of every run.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="pass_cursor_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "pass_cursor_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "pass_cursor_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"pass_cursor_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
