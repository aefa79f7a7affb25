"""The ownership rule of csrc/owned.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/owned_check.py [--keep DIR]

Builds tools/probe/owned_check.cpp (a stand-alone program with its own main that includes only common.hpp, and with it owned.hpp; hipcc,
host code with -fsanitize=address,undefined) and runs it on contexts that never saw a device: destroy-all deletes every listed object
once, newest first, and not the one destroyed by hand before; objects that disown themselves while it runs; unknown pointers; the empty
list of a context whose creation failed; blocks that come out of the context's cache and go back to it; two threads that adopt and disown
1000 objects each.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="owned_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "owned_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "owned_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"owned_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
