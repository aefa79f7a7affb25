"""The tables of the many-ensembles RMSD prune (csrc/prune_batch_plan.hpp) on the CPU: tools/prune_batch_plan_check.py builds the stand-alone
program tools/probe/prune_batch_plan_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and runs it at sizes worked out by hand.
Needs no GPU."""

import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segments_refusals_orders_and_team_indexing_at_hand_worked_sizes(tmp_path):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prune_batch_plan_check.py"), "--keep", str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"prune_batch_plan_check: \d+ checks passed", run.stdout), run.stdout + run.stderr
    assert "clean under ASan and UBSan" in run.stdout
