"""The ownership rule of the objects created from a context (csrc/owned.hpp: the base they derive from, the list their context keeps) on the
CPU: tools/owned_check.py builds the stand-alone program tools/probe/owned_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and
runs it.  Needs no GPU."""

import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_list_destroys_each_object_once_newest_first(tmp_path):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "owned_check.py"), "--keep", str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"owned_check: \d+ checks passed", run.stdout), run.stdout + run.stderr
    assert "clean under ASan and UBSan" in run.stdout
