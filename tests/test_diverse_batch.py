"""diverse_select_batch / most_diverse_conformers_batch: alignment, k-means and the pick of many ensembles per call.  The yardstick is
always the existing per-ensemble call on the same segment (diverse_select, most_diverse_conformers), a recorded fixture (G20) or the
NumPy restatement of tests/test_diverse.py that G20 pins on the CPU -- never the batch code itself."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_diverse import COORD_TOL, MARGIN_BAND, g20, kabsch_align_numpy, lloyd_restated, moved

SYMBOL = "tsc_diverse_select_batch"


# ------------------------------------------------------------------------------------------------------- CPU
def _no_device(monkeypatch):
    from tscode_amd import hypermolecule_class, kmeans, numba_functions, torsion_module

    def no_device(*a, **k):
        raise AssertionError("the library was entered")
    for mod in (hypermolecule_class, kmeans, numba_functions, torsion_module):
        monkeypatch.setattr(mod, "get_engine", no_device)


def test_argument_checks_raise_valueerror_before_the_library_is_entered(monkeypatch):
    import tscode_amd
    _no_device(monkeypatch)
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(8, 5, 3)), rng.normal(size=(6, 4, 3))
    rows = [[0, 1], [2, 3]]
    for kw in (dict(k=[2], init_rows=rows), dict(k=[2, 2, 2], init_rows=rows), dict(k=2, init_rows=[[0, 1]]), dict(k=2, seeds=[1]),
               dict(k=2, seeds=[1, 2, 3]), dict(k=2, init_rows=rows, energies=[np.zeros(8)])):      # ragged list lengths
        with pytest.raises(ValueError):
            tscode_amd.diverse_select_batch([a, b], **kw)
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b], [2, 7], init_rows=[[0, 1], list(range(7))])         # k_s > N_s
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b], [2, 0], init_rows=[[0, 1], []])
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b], 2, init_rows=[[0, 1], [2, 6]])                      # row 6 of 6
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b], 2, init_rows=[[0, 1], [2, -1]])
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b], 2, init_rows=[[0, 1], [2]])
    e = np.zeros(6)
    e[4] = np.nan
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b], 2, init_rows=rows, energies=[None, e])              # NaN energies
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b], 2, init_rows=rows, energies=[np.zeros(7), None])    # 7 energies for 8 structures
    for bad in (np.nan, np.inf, -np.inf):                                                           # non-finite coordinates
        bb = b.copy()
        bb[3, 2, 1] = bad
        with pytest.raises(ValueError):
            tscode_amd.diverse_select_batch([a, bb], 2, init_rows=rows)
        with pytest.raises(ValueError):
            tscode_amd.diverse_select_batch([a, bb], 2, seeds=[0, 1])
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, b[0]], 2, init_rows=rows)                               # not (N, n_atoms, 3)
    with pytest.raises(ValueError):
        tscode_amd.diverse_select_batch([a, np.zeros((4, 513, 3))], 2, init_rows=rows)              # 513 atoms
    assert tscode_amd.diverse_select_batch([], 2) == []
    # most_diverse_conformers_batch: ragged lists, before anything is pruned
    q = np.array([[0, 1, 2, 3]], dtype=np.int32)
    for kw in (dict(n=[2]), dict(n=2, seeds=[1]), dict(n=2, init_rows=[None]), dict(n=2, energies=[None, None, None])):
        with pytest.raises(ValueError):
            tscode_amd.most_diverse_conformers_batch(kw.pop("n"), [a, b], q, **kw)
    with pytest.raises(ValueError):
        tscode_amd.most_diverse_conformers_batch(2, [a, b], [q])


def test_the_symbol_is_in_the_header_and_the_prototype_table():
    from tscode_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "tscode_hip.h")).read()
    assert re.search(r"^int " + SYMBOL + r"\(", header, re.M), f"{SYMBOL} is not declared in include/tscode_hip.h"
    assert SYMBOL in _lib.EXPORTED_SYMBOLS
    assert "select_batch.hip" in build.SOURCES and "diverse_batch.hpp" in build.HEADERS


def test_every_kernel_of_diverse_hpp_is_a_wrapper_of_a_device_function_the_batch_calls_too():
    """The promise of the same bits rests on the single and the segmented kernel calling ONE function."""
    csrc = os.path.join(ROOT, "tscode_amd", "csrc")
    single = open(os.path.join(csrc, "diverse.hpp")).read()
    # (the wrapper kernels: diverse_kernels.hpp, which diverse.hip alone includes, and k_align_structures in diverse_align_kernel.hpp)
    wrappers = open(os.path.join(csrc, "diverse_kernels.hpp")).read() + open(os.path.join(csrc, "diverse_align_kernel.hpp")).read()
    batch = open(os.path.join(csrc, "diverse_batch.hpp")).read()
    for body in ("dv_align_structures", "dv_col_partial", "dv_col_finish", "dv_sum_fixed", "dv_row_norms", "dv_kmeans_assign", "dv_label_count",
                 "dv_label_bucket", "dv_own_d2", "dv_kmeans_relocate", "dv_kmeans_update", "dv_kmeans_control", "dv_kmeans_seed_update",
                 "dv_kmeans_seed_pick", "dv_diverse_pick"):
        assert len(re.findall(r"__device__ inline void " + body + r"\(", single)) == 1, body
        assert re.search(r"\n    " + body + r"(<NT>)?\(", wrappers), f"{body}: no wrapper kernel in diverse_kernels.hpp"
        assert re.search(r"\b" + body + r"(<NT>)?\(", batch), f"{body}: not called by diverse_batch.hpp"


def test_batch_makes_the_np_random_draws_of_the_loop_in_the_same_order(monkeypatch):
    """With stubs in place of the device calls: a batch that mixes n > 300, both early returns, seeded, row-initialised and unseeded
    clustered segments draws from np.random what the loop over most_diverse_conformers draws, in the same order."""
    import tscode_amd
    from tscode_amd import numba_functions, torsion_module
    _no_device(monkeypatch)
    rng = np.random.default_rng(5)
    sizes = (5, 400, 50, 60, 70, 500, 80, 90, 45)
    ns = (10, 301, 10, 10, 10, 320, 10, 10, 10)
    ens = [rng.normal(size=(N, 4, 3)) for N in sizes]
    seeds = [None, None, None, None, 123, None, None, None, None]
    rows = [None] * 6 + [np.arange(10)] + [None] * 2
    energies = [None, None, None, rng.normal(size=60), None, None, None, None, rng.normal(size=45)]
    q = np.array([[0, 1, 2, 3]], dtype=np.int32)
    seen = []

    def prune_one(structures, quadruplets, thresh=10, verbose=False):
        mask = np.zeros(len(structures), dtype=bool)
        mask[:8 if len(structures) == 50 else len(structures) // 2 + 11] = True      # 50 -> 8 <= n: the early return after the prune
        return structures[mask], mask

    def select_one(structures, k, init_rows=None, seed=None, energies=None, max_iter=300, tol=1e-4):
        seen.append((len(structures), k, seed, None if init_rows is None else tuple(init_rows), None if energies is None else energies.tobytes()))
        return structures + 1.0, np.zeros(len(structures), np.int32), np.arange(k, dtype=np.int32), np.arange(k, dtype=np.int32), 1
    monkeypatch.setattr(numba_functions, "prune_conformers_tfd", prune_one)
    monkeypatch.setattr(numba_functions, "prune_conformers_tfd_batch", lambda es, qs, thresh=10: [prune_one(e, None) for e in es])
    monkeypatch.setattr(torsion_module, "diverse_select", select_one)
    monkeypatch.setattr(torsion_module, "diverse_select_batch",
                        lambda es, k, init_rows=None, seeds=None, energies=None, **kw: [select_one(e, kk, r, sd, en)
                                                                                        for e, kk, r, sd, en in zip(es, k, init_rows, seeds, energies)])
    for s0 in (3, 4):
        np.random.seed(s0)
        seen.clear()
        want = [tscode_amd.most_diverse_conformers(ns[s], ens[s], q, energies[s], seed=seeds[s], init_rows=rows[s]) for s in range(len(ens))]
        want_seen, want_state = list(seen), np.random.get_state()[1].copy()
        np.random.seed(s0)
        seen.clear()
        got = tscode_amd.most_diverse_conformers_batch(list(ns), ens, q, energies, seeds=list(seeds), init_rows=rows)
        assert seen == want_seen and len(seen) == 5, "the clustered segments got other seeds, rows or energies"
        assert np.array_equal(np.random.get_state()[1], want_state), "np.random was left in another state"
        for s in range(len(ens)):
            assert np.array_equal(got[s], want[s]), s
        assert got[0] is ens[0] and len(got[1]) == 301 and len(got[2]) == 8 and len(got[5]) == 320
    assert {t[2] for t in seen if t[0] == 70 // 2 + 11} == {123}


# ------------------------------------------------------------------------------------------------------- GPU
_SEGMENTS = {}


def segments():
    """The segment shapes of the sweep, built once: [(structures, k, init_rows | None, seed | None, energies | None)].
    N: k, k + 1, 63, 64, 65, 255, 256, 512, 600, 1100 (a row tile of 64, the column-statistics chunks from N = 512 on, one and two pieces
    per thread of the 1024-thread kernels); atoms: 1, 10, 11, 21, 22, 40 (D = 3 .. 120 crosses 32 and 64); k: 1, 2, 16, 17, 20, 129 (the
    template widths 1, 2 and 5 of the assignment); the 65-row segment directly in front of the 63-row one."""
    if not _SEGMENTS:
        from tscode_amd.synthetic import make_ensemble
        rng = np.random.default_rng(77)

        def clustered(N, n, seed):
            return moved(make_ensemble(N, (n // 2, n - n // 2), seed=seed, children=7).poses(), seed)

        def loose(N, n):                       # no structure to find: Lloyd takes tens of iterations
            return rng.normal(size=(N, n, 3))
        segs = [
            (clustered(20, 10, 1), 20, rng.permutation(20)[:20], None, None),                 # N == k
            (clustered(21, 11, 2), 20, None, 11, None),                                       # N == k + 1
            (clustered(65, 21, 3), 16, None, 12, rng.normal(size=65)),
            (clustered(63, 22, 4), 17, rng.choice(63, 17, replace=False), None, None),
            (loose(64, 1), 2, None, 13, None),                                                # one atom: every centred feature is zero
            (clustered(255, 40, 5), 20, rng.choice(255, 20, replace=False), None, rng.normal(size=255)),
            (clustered(256, 10, 6), 1, None, 14, None),
            (clustered(512, 11, 7), 129, None, 15, None),
            (loose(600, 21), 20, rng.choice(600, 20, replace=False), None, None),
            (loose(1100, 22), 17, None, 16, rng.normal(size=1100)),
        ]
        _SEGMENTS["v"] = [(np.ascontiguousarray(x), k, None if r is None else r.astype(np.int32), sd, e) for x, k, r, sd, e in segs]
    return _SEGMENTS["v"]


def run_both(segs, **kw):
    import tscode_amd
    got = tscode_amd.diverse_select_batch([s[0] for s in segs], [s[1] for s in segs], init_rows=[s[2] for s in segs], seeds=[s[3] for s in segs],
                                          energies=[s[4] for s in segs], **kw)
    want = [tscode_amd.diverse_select(x, k, init_rows=r, seed=sd, energies=e, **kw) for x, k, r, sd, e in segs]
    return got, want


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g[0].shape == w[0].shape and np.array_equal(g[0].view(np.uint64), w[0].view(np.uint64)), f"{what} segment {s}: aligned differs in its bits"
        assert g[4] == w[4], f"{what} segment {s}: n_iter {g[4]}, alone {w[4]}"
        for name, a, b in (("labels", g[1], w[1]), ("picked", g[2], w[2]), ("init_rows", g[3], w[3])):
            assert a.dtype == np.int32 and np.array_equal(a, b), f"{what} segment {s}: {name} differ at {int((a != b).sum())} places"


@pytest.mark.gpu
def test_batch_equals_diverse_select_on_each_segment_alone():
    segs = segments()
    got, want = run_both(segs)
    iters = [w[4] for w in want]
    print("n_iter per segment:", iters)
    assert_same(got, want)
    assert iters[0] <= 2 and max(iters) >= 10, "no segment with N == k beside one that runs tens of iterations"
    assert len(set(iters)) >= 3, "the segments do not finish at different iterations"
    again, _ = run_both(segs)
    assert_same(again, got, "second call:")                                  # the same batch twice returns the same bits
    # another order, and a batch of two: a segment's result does not depend on its neighbours
    order = [9, 0, 4, 7, 2, 3]
    got2, _ = run_both([segs[s] for s in order])
    assert_same(got2, [want[s] for s in order], "reordered:")


@pytest.mark.gpu
def test_batch_with_max_iter_3_leaves_by_the_cap_where_the_single_call_does():
    segs = segments()
    got, want = run_both(segs, max_iter=3)
    iters = [w[4] for w in want]
    print("n_iter per segment at max_iter = 3:", iters)
    assert_same(got, want, "max_iter = 3:")
    assert iters.count(3) >= 2 and min(iters) < 3, "some segments leave by the cap, others before it"
    full = [w[4] for w in run_both(segs[8:], max_iter=300)[1]]
    assert min(full) > 3, "the capped segments would have gone on: they needed the extra assignment"


@pytest.mark.gpu
def test_g20_kmeans_cases_as_one_batch():
    """small, mdc and wide against their recorded labels and n_iter.  The recorded run of `empty` starts from centres that are no rows of
    its X, which diverse_select cannot be given; the relocation of an empty cluster is reached through rows instead: structure
    init_rows[3] becomes an exact copy of structure init_rows[1], the two centres coincide, every tie goes to the lower one and the
    upper cluster is empty in the first iteration.  Its yardstick is the restatement that G20 pins on the CPU (and diverse_select)."""
    import tscode_amd
    small, empty, mdc, wide = (g20(c) for c in ("small", "empty", "mdc", "wide"))
    dup = empty.structures.copy()
    dup[empty.init_rows[3]] = dup[empty.init_rows[1]]
    Xd = kabsch_align_numpy(dup).reshape(len(dup), -1)
    lab_d, _, _, it_d, margin_d, max_empty_d = lloyd_restated(Xd, Xd[empty.init_rows])
    assert max_empty_d == 1, "the case with a forced empty cluster has lost it"
    Xe = empty.aligned.reshape(len(empty.aligned), -1)
    lab_e, _, _, it_e, margin_e, _ = lloyd_restated(Xe, Xe[empty.init_rows])
    assert margin_e >= MARGIN_BAND
    ens = [small.structures, empty.structures, dup, mdc.structures[mdc.tfd_mask], wide.X.reshape(1200, 20, 3)]
    rows = [small.init_rows, empty.init_rows, empty.init_rows, mdc.init_rows, wide.init_rows]
    got = tscode_amd.diverse_select_batch(ens, [len(r) for r in rows], init_rows=rows)
    for name, g, labels, n_iter in (("small", got[0], small.labels, int(small.n_iter)), ("empty from rows", got[1], lab_e, it_e),
                                    ("empty cluster", got[2], lab_d, it_d), ("mdc", got[3], mdc.labels, int(mdc.n_iter)),
                                    ("wide", got[4], wide.labels, int(wide.n_iter))):
        print(f"{name}: n_iter {g[4]} (want {n_iter}), labels differing {int((g[1] != labels).sum())}")
        assert np.array_equal(g[1], labels) and g[4] == n_iter, name
    assert np.abs(got[0][0] - small.aligned).max() <= COORD_TOL and np.abs(got[1][0] - empty.aligned).max() <= COORD_TOL
    assert_same(got, [tscode_amd.diverse_select(e, len(r), init_rows=r) for e, r in zip(ens, rows)], "G20:")


@pytest.mark.gpu
def test_most_diverse_conformers_batch_matches_the_reference_in_both_modes_beside_other_segments():
    pytest.importorskip("networkx")
    import tscode_amd
    c = g20("mdc")
    n = int(c.n)
    segs = segments()
    others = [segs[2][0], segs[5][0], segs[0][0]]                      # 65 x 21, 255 x 40, and 20 structures: the early return at len <= n
    q_others = [np.array([[0, 5, 11, 17], [1, 2, 12, 13]], np.int32), np.array([[0, 1, 20, 21]], np.int32), np.zeros((0, 4), np.int32)]
    ens = [others[0], c.structures.copy(), others[1], c.structures.copy(), others[2]]
    quads = [q_others[0], c.quadruplets, q_others[1], c.quadruplets, q_others[2]]
    out = tscode_amd.most_diverse_conformers_batch([10, n, 12, n, 20], ens, quads, [None, c.energies, None, None, None], seeds=[1, None, 2, None, None],
                                                   init_rows=[None, c.init_rows, None, c.init_rows, None])
    for name, got, want in (("energies", out[1], c.out_energies), ("diverse", out[3], c.out_diverse)):
        assert got.shape == want.shape, name
        print(f"most_diverse_conformers_batch ({name}): |out - reference| = {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= COORD_TOL, name
    assert out[4] is ens[4]
    for s, (k, sd) in ((0, (10, 1)), (2, (12, 2))):
        assert np.array_equal(out[s], tscode_amd.most_diverse_conformers(k, ens[s], quads[s], seed=sd)), s
    # one torsion array and one n for all; a batch in which a single segment reaches the clustering goes to the single calls
    same = tscode_amd.most_diverse_conformers_batch(n, [c.structures.copy(), c.structures[:15]], c.quadruplets, init_rows=[c.init_rows, None])
    assert np.abs(same[0] - c.out_diverse).max() <= COORD_TOL and len(same[1]) == 15


@pytest.mark.gpu
def test_library_refuses_an_invalid_segment_before_any_launch_and_names_it():
    from tscode_amd import _lib
    from tscode_amd.engine import get_engine
    eng = get_engine()
    x = np.random.default_rng(1).normal(size=(2 * 8 * 4 * 3))
    offsets = np.array([0, 96, 192], dtype=np.int64)
    N, n, flags = np.array([8, 8], np.int32), np.array([4, 4], np.int32), np.zeros(2, np.uint8)
    al, lab, pk, it = np.full(192, 7.0), np.zeros(16, np.int32), np.full(5, -7, np.int32), np.zeros(2, np.int32)

    def call(k, rows, structures=x, fl=flags, u=None):
        return eng.lib.tsc_diverse_select_batch(eng._h, _lib.ptr(structures), _lib.ptr(offsets), _lib.ptr(N), _lib.ptr(n), _lib.ptr(np.array(k, np.int32)),
                                                C.c_int64(2), _lib.ptr(np.array(rows, np.int32)), None if u is None else _lib.ptr(u), None, _lib.ptr(fl),
                                                C.c_int(300), C.c_double(1e-4), _lib.ptr(al), _lib.ptr(lab), _lib.ptr(pk), _lib.ptr(it))
    assert call([2, 9], [0, 1] + list(range(9))) != 0 and "segment 1" in eng.lib.tsc_last_error().decode()          # k > N
    assert call([2, 3], [0, 1, 0, 8, 2]) != 0 and "segment 1" in eng.lib.tsc_last_error().decode()                  # row 8 of 8
    bad = x.copy()
    bad[50] = np.nan
    assert call([2, 3], [0, 1, 0, 1, 2], structures=bad) != 0 and "segment 0" in eng.lib.tsc_last_error().decode()
    assert call([2, 3], [0, 1, 0, 1, 2], fl=np.array([0, 2], np.uint8), u=np.array([0, 0, 0.5, 1.0, 0.2])) != 0     # u = 1.0
    assert "segment 1" in eng.lib.tsc_last_error().decode()
    assert (al == 7.0).all() and (pk == -7).all(), "a refused call has written to the caller's arrays"
    assert call([2, 3], [0, 1, 0, 1, 2]) == 0 and not (al == 7.0).any()


@pytest.mark.gpu
def test_a_list_beyond_the_device_limit_goes_in_slices_with_the_same_results(monkeypatch):
    from tscode_amd import torsion_module
    segs = segments()[:8]
    whole, _ = run_both(segs)
    calls = []
    real = torsion_module._diverse_select_slice
    monkeypatch.setattr(torsion_module, "_diverse_select_slice", lambda s, *a: (calls.append(len(s)), real(s, *a))[1])
    monkeypatch.setattr(torsion_module, "DIVERSE_BATCH_BYTES", 3 * 24 * 70 * 22 * 2)     # two 65 x 22 ensembles: 255 x 40 and 512 x 11 go alone
    sliced, _ = run_both(segs)
    assert len(calls) >= 2 and sum(calls) < len(segs), calls                            # slices of several ensembles, and single calls
    assert_same(sliced, whole, "sliced:")
