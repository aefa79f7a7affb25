"""The option table of csrc/options.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

    python tools/options_check.py [--keep DIR]

Builds tools/probe/options_check.cpp (a stand-alone program with its own main that includes only options.hpp; hipcc, host code with
-fsanitize=address,undefined) and runs it: for every option the default set and read back, one other accepted value, the values just
outside its rule refused by name with the stored value left alone; unknown names; the walk of tsc_option_info; and what the rules keep
as it always was -- fractions cut off, the clamp of "open_lds_blocks", "non-zero means 1", the unchecked options.  Needs no GPU."""

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
    work = args.keep or tempfile.mkdtemp(prefix="options_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "options_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "options_check.cpp")], check=True, cwd=ROOT)
    subprocess.run([exe], check=True)
    print(f"options_check: clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
