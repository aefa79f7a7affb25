"""Cross-set RMSD without a GPU: the grid arithmetic of csrc/cross_plan.hpp on the CPU (tools/cross_plan_check.py builds the stand-alone
program tools/probe/cross_plan_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and runs it at sizes worked out by hand), the
argument errors of tscode_amd/rmsd_cross.py, which come before an engine exists, and the package's exports."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_at_hand_worked_sizes(tmp_path):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cross_plan_check.py"), "--keep", str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"cross_plan_check: \d+ checks passed", run.stdout), run.stdout + run.stderr
    assert "clean under ASan and UBSan" in run.stdout


def test_package_exports_the_five_calls():
    import tscode_amd
    from tscode_amd import rmsd_cross
    names = ("rmsd_matrix", "rmsd_similarity_mask", "nearest_structures", "prune_conformers_rmsd_against", "assign_to_kept")
    for name in names:
        assert getattr(tscode_amd, name) is getattr(rmsd_cross, name) and name in rmsd_cross.__all__
    assert rmsd_cross.CROSS_MATRIX_BYTES == 1 << 30


@pytest.fixture
def no_engine(monkeypatch):
    """every way from rmsd_cross.py to the device fails the test: the errors below are raised before an engine is asked for"""
    from tscode_amd import rmsd_cross

    def refuse(*_a, **_k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(rmsd_cross, "get_engine", refuse)


def calls(queries, library, atomnos):
    import tscode_amd
    return (lambda: tscode_amd.rmsd_matrix(queries, library, atomnos),
            lambda: tscode_amd.rmsd_similarity_mask(queries, library, atomnos),
            lambda: tscode_amd.nearest_structures(queries, library, atomnos),
            lambda: tscode_amd.prune_conformers_rmsd_against(queries, library, atomnos))


def test_argument_errors_come_without_an_engine(no_engine):
    import tscode_amd
    x, y = np.zeros((4, 5, 3)), np.ones((6, 5, 3))
    for bad in (np.zeros((5, 3)), np.zeros((4, 5, 2)), np.zeros((4, 5, 3, 1))):            # wrong rank or last extent
        for call in calls(bad, y, None) + calls(x, bad, None):
            with pytest.raises(ValueError, match=r"must be \(N, n_atoms, 3\)"):
                call()
    for call in calls(x, np.ones((6, 4, 3)), None):                                       # unequal atom counts
        with pytest.raises(ValueError, match="5 atoms, library has 4"):
            call()
    for atomnos in (np.full(4, 6), np.full(6, 6), np.full((5, 1), 6)):                      # atomnos of the wrong length
        for call in calls(x, y, atomnos):
            with pytest.raises(ValueError, match="atomnos must be"):
                call()
    for call in calls(x, y, np.ones(5, dtype=int)):                                       # no compared atom
        with pytest.raises(ZeroDivisionError):
            call()
    for value in (np.nan, np.inf):
        q, lib = x.copy(), y.copy()
        q[2, 3, 1] = value
        lib[5, 0, 2] = value
        for call in calls(q, y, None) + calls(x, lib, None):                              # a coordinate that is not finite
            with pytest.raises(ValueError, match="not finite"):
                call()
    with pytest.raises(ValueError, match="library is empty"):                             # nothing can be nearest in an empty library
        tscode_amd.nearest_structures(x, np.zeros((0, 5, 3)))
    with pytest.raises(ValueError, match="mask must be bool"):
        tscode_amd.assign_to_kept(x, np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="none kept"):
        tscode_amd.assign_to_kept(x, np.zeros(4, dtype=bool))


def test_empty_sets_return_empty_outputs_without_an_engine(no_engine):
    import tscode_amd
    none, lib = np.zeros((0, 5, 3)), np.ones((6, 5, 3))
    r, m = tscode_amd.rmsd_matrix(none, lib)
    assert r.shape == m.shape == (0, 6) and r.dtype == np.float64
    r, m = tscode_amd.rmsd_matrix(lib, none)
    assert r.shape == m.shape == (6, 0)
    assert tscode_amd.rmsd_matrix(none)[0].shape == (0, 0)
    similar, first = tscode_amd.rmsd_similarity_mask(none, lib)
    assert similar.shape == first.shape == (0,) and similar.dtype == bool and first.dtype == np.int32
    similar, first = tscode_amd.rmsd_similarity_mask(lib, none)                            # an empty library covers nothing
    assert not similar.any() and (first == -1).all() and first.dtype == np.int32
    index, r, m = tscode_amd.nearest_structures(none, lib)
    assert index.shape == r.shape == m.shape == (0,) and index.dtype == np.int32
    novel, mask = tscode_amd.prune_conformers_rmsd_against(lib, none, np.full(5, 6))
    assert mask.all() and np.array_equal(novel, lib)
    rep, population = tscode_amd.assign_to_kept(lib, np.ones(6, dtype=bool))               # nothing removed: nothing to look up
    assert np.array_equal(rep, np.arange(6)) and rep.dtype == np.int32 and np.array_equal(population, np.ones(6)) and population.dtype == np.int64
