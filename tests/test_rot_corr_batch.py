"""prune_rmsd_rot_corr_arrays_batch: the symmetry-corrected RMSD prune of many ensembles per call (tscode_amd/csrc/rot_corr.hpp,
refine_batch.hpp, refine_batch.hip, tscode_amd/rot_corr.py).  The yardstick is always the reference's recorded run (G19), the single-ensemble call on the
same segment or the numpy restatement of test_rot_corr_sweep.py, never the batch code itself."""

import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_rot_corr import case as g19_case, centred
from test_rot_corr_sweep import THR, Setup, molecule, pass_restated, raw_ensemble, small_molecule

SYMBOLS = ("tsc_rot_corr_batch_begin", "tsc_rot_corr_batch_pass", "tsc_rot_corr_batch_end", "tsc_rot_corr_batch_destroy",
           "tsc_inertia_moments_batch", "tsc_moi_first_similar_batch")
NO_TORSIONS = dict(torsions=[], angles=[], move_masks=[], sub_nodes=[])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def g19_batch(names):
    cases = [g19_case(n) for n in names]
    return (cases, [c.structures for c in cases], [c.atomnos for c in cases], [c.setup if c.meta["n_torsions"] else NO_TORSIONS for c in cases],
            [c.meta["max_rmsd"] for c in cases])


# ------------------------------------------------------------------------------------------------------- CPU
def test_host_driver_with_the_restatement_gives_the_recorded_g19_runs(monkeypatch):
    """G19 n40 and n160a as ONE batch with their own thresholds through the product's host driver, the device run replaced by the numpy
    restatement answering every slot segment by segment: the reference's masks, its (n_active, pairs evaluated) per slot and its
    structures.  The two cases are not open in the same slots, and a slot with no open segment never reaches the pair search."""
    pytest.importorskip("networkx")
    import tscode_amd
    import tscode_amd.rot_corr as rc
    cases, ens, atomnos, setups, thr = g19_batch(["n40", "n160a"])
    restated = [Setup(c.atomnos, **c.setup) for c in cases]
    slots = []

    class RestatedRun:
        def __init__(self, engine, ensembles, device_setups):
            assert engine is None and len(ensembles) == 2
            self.S = [np.array(e) for e in ensembles]
            self.cache = [set() for _ in ensembles]
            self.off = np.concatenate(([0], np.cumsum([len(e) for e in ensembles])))

        def run_slot(self, open_segs, d, k, num_active, max_rmsd):
            first = np.full(self.off[-1], -1, dtype=np.int32)
            ev = []
            for q, s in enumerate(open_segs.tolist()):
                f, e = pass_restated(self.S[s], self.cache[s], restated[s], int(d[q]), int(k), int(num_active[q]), float(max_rmsd[q]))
                first[self.off[s]:self.off[s + 1]] = f
                ev.append(e)
            slots.append((int(k), open_segs.tolist()))
            return first, np.array(ev, dtype=np.int64)

        def end(self):
            return self.S

        def close(self):
            pass

    monkeypatch.setattr(rc, "_BatchRun", RestatedRun)
    monkeypatch.setattr(rc, "get_engine", lambda: None)
    got = tscode_amd.prune_rmsd_rot_corr_arrays_batch(ens, atomnos, setups, max_rmsd=thr)
    stats = tscode_amd.last_rot_corr_batch_stats()
    assert all(segs for _, segs in slots), "a slot without an open segment reached the pair search"
    assert {tuple(segs) for _, segs in slots} >= {(0, 1), (1,)}, slots            # n160a opens at k = 20, n40 at k = 5
    assert [k for k, _ in slots] == sorted({k for k, _ in slots}, reverse=True)
    for s, (c, (kept, mask), st) in enumerate(zip(cases, got, stats)):
        assert np.array_equal(mask, c.mask), (c.meta["name"], int(mask.sum()), int(c.mask.sum()))
        assert [x["n_active"] for x in st] == c.passes[:, 0].tolist()
        assert [x["pairs_evaluated"] for x in st] == c.passes[:, 1].tolist()
        assert [int(x["k"]) for x in st if x["ran"]] == [k for k, segs in slots if s in segs]
        assert kept.shape == c.out.shape and np.abs(kept - c.out).max() < 1e-10


def test_argument_checks_raise_valueerror_before_the_library_is_entered(monkeypatch):
    import tscode_amd
    import tscode_amd.rot_corr as rc

    def no_device(*a, **k):
        raise AssertionError("the library was entered")
    monkeypatch.setattr(rc, "get_engine", no_device)
    monkeypatch.setattr(rc, "_BatchRun", no_device)
    c = g19_case("n40")
    s, n = c.setup, c.structures.shape[1]
    a, b = c.structures[:6], c.structures[:4]
    batch = tscode_amd.prune_rmsd_rot_corr_arrays_batch

    def changed(**kw):
        return {**s, **kw}
    for bad in (lambda: batch([a, b], c.atomnos, [s]),                                            # one set-up for two ensembles
                lambda: batch([a, b], c.atomnos, [s, s, s]),
                lambda: batch([a, b], [c.atomnos], s),                                            # one atomnos array in a list for two
                lambda: batch([a, b], [c.atomnos] * 3, s),
                lambda: batch([a, b], c.atomnos[:-1], s),                                         # an atom short
                lambda: batch([a, b], c.atomnos, s, max_rmsd=[0.25]),
                lambda: batch([a, b], c.atomnos, s, max_rmsd=[0.25, 0.5, 0.1]),
                lambda: batch([a, b[0]], c.atomnos, s),                                           # not (N, n, 3)
                lambda: batch([a, b[:, :, :2]], c.atomnos, s),
                lambda: batch([a, b], c.atomnos, [s, changed(torsions=np.array([[0, 1, 2, n], s["torsions"][1]]))]),     # atom n of n
                lambda: batch([a, b], c.atomnos, [s, changed(torsions=np.array([[0, -1, 2, 3], s["torsions"][1]]))]),
                lambda: batch([a, b], c.atomnos, [changed(sub_nodes=[[0, n], s["sub_nodes"][1]]), s]),
                lambda: batch([a, b], c.atomnos, [s, changed(sub_nodes=[[], s["sub_nodes"][1]])]),
                lambda: batch([a, b], c.atomnos, [s, {k: [v[0]] * 17 for k, v in s.items()}]),                             # 17 torsions
                lambda: batch([np.zeros((3, 513, 3)), b], [np.full(513, 6), c.atomnos],
                              [dict(torsions=[[0, 1, 2, 3]], angles=[[0, 180]], move_masks=np.zeros((1, 513), bool), sub_nodes=[[0, 1]]), s]),
                lambda: batch([a, b], c.atomnos, [s, changed(angles=[[], s["angles"][1]])]),                              # a table of 0 entries
                lambda: batch([a, b], c.atomnos, [s, changed(angles=[np.arange(7.0), s["angles"][1]])]),                  # ... of 7
                lambda: batch([a, b], c.atomnos, [s, {k: v for k, v in s.items() if k != "angles"}])):
        with pytest.raises(ValueError):
            bad()
    assert batch([], c.atomnos, s) == [] and tscode_amd.last_rot_corr_batch_stats() == []
    # ensembles that take no part never reach the library either: centred, full masks
    got = batch([a, b[:1], b[:0]], c.atomnos, [NO_TORSIONS, s, s])
    assert [m.tolist() for _, m in got] == [[True] * 6, [True], []]
    assert got[0][0].tobytes() == centred(a).tobytes() and got[1][0].tobytes() == centred(b[:1]).tobytes() and got[2][0].shape == (0, n, 3)
    assert tscode_amd.last_rot_corr_batch_stats() == [[], [], []]
    # ... also where the list holds one ensemble: nothing goes to the single call
    monkeypatch.setattr(rc, "prune_rmsd_rot_corr_arrays", no_device)
    for e, st in ((b[:1], s), (b[:0], s), (a, NO_TORSIONS)):
        (kept, mask), = batch([e], c.atomnos, st)
        assert mask.all() and len(mask) == len(e) and kept.tobytes() == centred(e).tobytes() and kept.shape == e.shape
        assert tscode_amd.last_rot_corr_batch_stats() == [[]]


def test_the_symbols_are_in_the_header_and_the_prototype_table():
    from tscode_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "tscode_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"^int " + s + r"\(", header, re.M), f"{s} is not declared in include/tscode_hip.h"
        assert s in _lib.EXPORTED_SYMBOLS
    assert "refine_batch.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "tscode_amd", "csrc", "refine_batch.hip")).read()
    bodies = re.split(r'extern "C"', src)[1:]
    assert len(bodies) == len(SYMBOLS)
    for body in bodies:
        assert re.search(r"\)\s*\{\s*TSC_API_GUARD_BEGIN", body), "an entry point does not start with TSC_API_GUARD_BEGIN"


# ------------------------------------------------------------------------------------------------------- GPU
_SINGLE = {}


def single(key, structures, atomnos, setup, max_rmsd):
    """prune_rmsd_rot_corr_arrays on one segment and its stats, computed once per key and left unchanged."""
    if key not in _SINGLE:
        import tscode_amd
        kept, mask = tscode_amd.prune_rmsd_rot_corr_arrays(structures, atomnos, **setup, max_rmsd=max_rmsd)
        ran = len(setup["torsions"]) > 0 and len(structures) <= 750
        _SINGLE[key] = (kept, mask, tscode_amd.last_rot_corr_stats() if ran else [])
    return _SINGLE[key]


def assert_equals_single(key, got, stats, structures, atomnos, setup, max_rmsd):
    kept, mask, st = single(key, structures, atomnos, setup, max_rmsd)
    assert got[1].dtype == np.bool_ and np.array_equal(got[1], mask), (key, int(got[1].sum()), int(mask.sum()))
    assert got[0].shape == kept.shape and np.array_equal(bits(got[0]), bits(kept)), key
    if len(structures) >= 2:
        assert stats == st, key
    else:
        assert stats == [], key


@pytest.mark.gpu
def test_g19_cases_as_one_batch():
    pytest.importorskip("networkx")
    import tscode_amd
    names = ["n40", "n150", "n160a", "notors", "n760"]
    cases, ens, atomnos, setups, thr = g19_batch(names)
    assert [(c.structures.shape[1], c.meta["n_torsions"]) for c in cases[:3]] == [(23, 2), (40, 6), (23, 2)]
    got = tscode_amd.prune_rmsd_rot_corr_arrays_batch(ens, atomnos, setups, max_rmsd=thr)
    stats = tscode_amd.last_rot_corr_batch_stats()
    assert len(got) == len(stats) == 5
    for name, c, (kept, mask), st, setup in zip(names, cases, got, stats, setups):
        assert np.array_equal(mask, c.mask), (name, int(mask.sum()), int(c.mask.sum()))
        if name in ("notors", "n760"):
            assert mask.all() and kept.tobytes() == centred(c.structures).tobytes() and st == []
            continue
        assert [x["n_active"] for x in st] == c.passes[:, 0].tolist(), name
        assert [x["pairs_evaluated"] for x in st] == c.passes[:, 1].tolist(), name
        assert kept.shape == c.out.shape
        err = np.abs(kept - c.out).max()
        assert err < 1e-10, (name, err)
        assert_equals_single(("g19", name), (kept, mask), st, c.structures, c.atomnos, setup, c.meta["max_rmsd"])
    first_open = [next(int(x["k"]) for x in st if x["ran"]) for st in stats[:3]]
    assert first_open == [5, 20, 20], first_open


EDGE_SIZES = (0, 1, 2, 8, 9, 17, 26, 27)


def edge_ensembles():
    """Ensembles of the small rotor molecule with EDGE_SIZES structures: clusters of three symmetry turns, shuffled, cut to size."""
    mol = small_molecule()
    return mol, [raw_ensemble(mol, 9, 3, seed=6100 + N)[:N] for N in EDGE_SIZES]


@pytest.mark.gpu
def test_segment_sizes_around_the_kernels_edges_in_any_order():
    """A chunk shorter than, equal to and one past the batch of eight wavefronts; 17: k = 2 opens and its last chunk [8, 17) is longer
    than d; 26: the first size at which the k = 5 gate (5 k < active) opens, last chunk [20, 26)."""
    pytest.importorskip("networkx")
    import tscode_amd
    mol, ens = edge_ensembles()
    order = list(range(len(ens)))
    pruned = 0
    for perm in (order, order[::-1], order[2:5] + [0] + order[5:] + [1]):           # as listed, reversed, an empty ensemble in the middle
        got = tscode_amd.prune_rmsd_rot_corr_arrays_batch([ens[s] for s in perm], mol.atomnos, mol.setup(), max_rmsd=THR)
        stats = tscode_amd.last_rot_corr_batch_stats()
        for q, s in enumerate(perm):
            assert_equals_single(("edge", s), got[q], stats[q], ens[s], mol.atomnos, mol.setup(), THR)
            pruned += int((~got[q][1]).sum())
    ran = {N: [int(x["k"]) for x in single(("edge", s), ens[s], mol.atomnos, mol.setup(), THR)[2] if x["ran"]] for s, N in enumerate(EDGE_SIZES)}
    assert {N: k[0] for N, k in ran.items() if N >= 2} == {2: 1, 8: 1, 9: 1, 17: 2, 26: 5, 27: 5}, ran       # the first open slot of every size
    assert pruned > 0, "nothing was pruned: the commit rule was not exercised"


@pytest.mark.gpu
def test_a_small_and_a_large_footprint_in_one_launch():
    """65 atoms x 2 torsions beside 512 atoms x 16 torsions: the small segment's workgroups lay out their lists and wave blocks inside
    the dynamic LDS sized for the large one."""
    pytest.importorskip("networkx")
    import tscode_amd
    mols = [molecule("65x2"), molecule("512x16", "shuffle")]
    ens = [raw_ensemble(m, 4, 3, seed=6200 + q) for q, m in enumerate(mols)]
    got = tscode_amd.prune_rmsd_rot_corr_arrays_batch(ens, [m.atomnos for m in mols], [m.setup() for m in mols], max_rmsd=THR)
    stats = tscode_amd.last_rot_corr_batch_stats()
    for q, m in enumerate(mols):
        assert_equals_single(("mixed", q), got[q], stats[q], ens[q], m.atomnos, m.setup(), THR)


@pytest.mark.gpu
def test_a_list_beyond_the_byte_budget_goes_in_slices_with_the_same_results(monkeypatch):
    pytest.importorskip("networkx")
    import tscode_amd
    import tscode_amd.rot_corr as rc
    mol, ens = edge_ensembles()
    three = [ens[EDGE_SIZES.index(N)] for N in (17, 26, 27)]
    whole = tscode_amd.prune_rmsd_rot_corr_arrays_batch(three, mol.atomnos, mol.setup(), max_rmsd=THR)
    whole_stats = tscode_amd.last_rot_corr_batch_stats()
    uploads = []
    real = rc._rot_corr_batch_upload
    monkeypatch.setattr(rc, "_rot_corr_batch_upload", lambda e, s, t, v=False: (uploads.append(len(e)), real(e, s, t, v))[1])
    cost = [e.nbytes + (len(e) ** 2 + 7) // 8 for e in three]
    monkeypatch.setattr(rc, "ROT_CORR_BATCH_BYTES", cost[0] + cost[1])             # the third ensemble no longer fits beside the first two
    sliced = tscode_amd.prune_rmsd_rot_corr_arrays_batch(three, mol.atomnos, mol.setup(), max_rmsd=THR)
    assert uploads == [2, 1], uploads
    assert tscode_amd.last_rot_corr_batch_stats() == whole_stats
    for a, b in zip(sliced, whole):
        assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    for q, N in enumerate((17, 26, 27)):
        assert_equals_single(("edge", EDGE_SIZES.index(N)), sliced[q], whole_stats[q], three[q], mol.atomnos, mol.setup(), THR)


@pytest.mark.gpu
def test_a_run_outlives_its_engine_without_harm():
    """The context destroys the batch runs it still lists; a run closed or collected after its engine skips the destroy call."""
    pytest.importorskip("networkx")
    import tscode_amd.rot_corr as rc
    from tscode_amd.engine import Engine
    mol, ens = edge_ensembles()
    two = [centred(ens[EDGE_SIZES.index(N)]) for N in (9, 17)]
    setups = [rc._Setup(mol.coords.shape[0], mol.atomnos, **mol.setup())] * 2
    for listed in (True, False):
        e = Engine(0)
        run = rc._BatchRun(e, two, setups)
        first, ev = run.run_slot(np.array([0, 1]), np.array([9, 17]), 1, np.array([9, 17]), np.array([THR, THR]))
        assert first.shape == (26,) and ev.shape == (2,) and ev.min() > 0
        if not listed:
            e._runs.discard(run)                 # the engine no longer knows the run: tsc_ctx_destroy frees it
        e.close()
        run.close()
        del run
    fresh = Engine(0)
    try:
        run = rc._BatchRun(fresh, two, setups)
        assert [x.shape for x in run.end()] == [x.shape for x in two]
        run.close()
    finally:
        fresh.close()
