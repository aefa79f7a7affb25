"""The host's bookkeeping of a stepped prune run (csrc/pass_cursor.hpp: which kernel closes a pass on the device and opens the next, the
call order of the stepping entry points, the run's layout numbers) on the CPU: tools/pass_cursor_check.py builds the stand-alone program
tools/probe/pass_cursor_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and runs it.  Needs no GPU."""

import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_slot_is_opened_once_and_closed_once_in_every_call_order(tmp_path):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pass_cursor_check.py"), "--keep", str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"pass_cursor_check: \d+ checks passed", run.stdout), run.stdout + run.stderr
    assert "clean under ASan and UBSan" in run.stdout
