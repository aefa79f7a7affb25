"""prune_by_moment_of_inertia_batch: the moment-of-inertia prune of many ensembles per call (tscode_amd/csrc/moi.hpp, refine_batch.hpp, refine_batch.hip,
tscode_amd/optimization_methods.py).  The yardstick is the single-ensemble path on the same segment (Engine.inertia_moments,
Engine.moi_first_similar, prune_by_moment_of_inertia) or the reference's recorded results (G9), never the batch code itself."""

import numpy as np
import pytest

from conftest import load_golden

SIZES = (1, 2, 64, 65, 129)                  # one wavefront looks at 64 columns per step
ATOMS = (5, 9, 3, 12, 7)
Z = np.array([6, 7, 8, 9, 16, 17])


# ------------------------------------------------------------------------------------------------------- CPU
def test_argument_checks_raise_valueerror_before_the_library_is_entered(monkeypatch):
    import tscode_amd
    from tscode_amd import optimization_methods as om

    def no_device(*a, **k):
        raise AssertionError("the library was entered")
    monkeypatch.setattr(om, "get_engine", no_device)
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(6, 5, 3)), rng.normal(size=(4, 7, 3))
    za, zb = np.array([6, 1, 8, 6, 1]), np.array([6, 6, 1, 7, 8, 1, 1])
    batch = tscode_amd.prune_by_moment_of_inertia_batch
    for bad in (lambda: batch([a, b], [za]),                                           # one atomnos array in a list for two ensembles
                lambda: batch([a, b], [za, zb, zb]),
                lambda: batch([a, b], za),                                             # five entries for ensemble 1's seven atoms
                lambda: batch([a, b], [za, zb[:-1]]),
                lambda: batch([a, b[0]], [za, zb]),                                    # not (N, n, 3)
                lambda: batch([a, b], [za, zb], max_deviation=[1e-2]),
                lambda: batch([a, b], [za, zb], max_deviation=[1e-2, 1e-3, 1e-4]),
                lambda: batch([a, b], [za, zb], masses=[np.ones(5)]),
                lambda: batch([a, b], [za, zb], masses=[np.ones(5), np.ones(6)]),
                lambda: batch([a, b], [za, np.ones(7, dtype=int)]),                    # hydrogens only
                lambda: batch([a, b], [za, np.array([6, 6, 1, 7, 8, 1, 92])])):        # no built-in mass for Z = 92
        with pytest.raises(ValueError):
            bad()
    assert batch([], za) == []


def test_engine_refuses_a_short_masses_list_before_it_looks_at_the_pairs():
    from tscode_amd.engine import Engine
    eng = Engine.__new__(Engine)                       # no context: the check comes before the library is entered
    with pytest.raises(ValueError, match="1 mass arrays for 2 ensembles"):
        eng.inertia_moments_batch([np.zeros((2, 3, 3)), np.zeros((2, 4, 3))], [np.ones(3)])


# ------------------------------------------------------------------------------------------------------- GPU
_BATCH = {}


def edge_batch():
    """Segments of SIZES structures of different molecules (atoms, elements, masses), built once: a few base geometries per
    segment repeated in turn with noise far below max_deviation, so that rows match, in the longest segment beyond the first 64 columns."""
    if not _BATCH:
        rng = np.random.default_rng(515)
        ens, atomnos, masses = [], [], []
        for N, n in zip(SIZES, ATOMS):
            n_base = 70 if N == 129 else 5                           # 129 rows over 70 geometries: row i first matches row i + 70
            base = rng.normal(scale=2.0, size=(n_base, n, 3))
            pick = np.arange(N) % n_base
            ens.append(base[pick] + rng.normal(scale=1e-7, size=(N, n, 3)))
            z = rng.choice(Z, size=n)
            z[rng.integers(n)] = 1                                   # one hydrogen each: dropped before the moments (:335-336)
            z[(np.flatnonzero(z == 1)[0] + 1) % n] = 6
            atomnos.append(z)
            masses.append(rng.uniform(1.0, 40.0, size=n))
        _BATCH["v"] = (ens, atomnos, masses)
    return _BATCH["v"]


@pytest.mark.gpu
def test_moments_and_first_equal_the_single_kernels_per_segment():
    import tscode_amd
    eng = tscode_amd.get_engine(0)
    ens, atomnos, masses = edge_batch()
    heavy = [e[:, z != 1] for e, z in zip(ens, atomnos)]
    hm = [m[z != 1] for m, z in zip(masses, atomnos)]
    mo = eng.inertia_moments_batch(heavy, hm)
    dev = np.array([1e-2, 1e-3, 1e-2, 5e-2, 1e-2])
    first = eng.moi_first_similar_batch(mo, dev)
    far = 0
    for s, (h, m) in enumerate(zip(heavy, hm)):
        alone = eng.inertia_moments(h, m)
        assert mo[s].shape == alone.shape and np.array_equal(mo[s].view(np.uint64), alone.view(np.uint64)), s
        want = eng.moi_first_similar(alone, float(dev[s]))
        assert first[s].dtype == np.int32 and np.array_equal(first[s], want), s
        far += int(((want - np.arange(len(want)) > 64) & (want >= 0)).sum())
    assert far > 0, "no row found its match beyond the first 64 columns"
    # empty segments in front, in the middle and at the end; a batch of one
    empty = [heavy[2][:0], heavy[3], heavy[0][:0], heavy[4], heavy[1][:0]]
    mo2 = eng.inertia_moments_batch(empty, [hm[2], hm[3], hm[0], hm[4], hm[1]])
    assert [x.shape for x in mo2] == [(0, 3), (65, 3), (0, 3), (129, 3), (0, 3)]
    assert np.array_equal(mo2[1].view(np.uint64), mo[3].view(np.uint64)) and np.array_equal(mo2[3].view(np.uint64), mo[4].view(np.uint64))
    f2 = eng.moi_first_similar_batch(mo2, np.array([1e-2, 5e-2, 1e-2, 1e-2, 1e-2]))
    assert np.array_equal(f2[1], first[3]) and np.array_equal(f2[3], first[4]) and len(f2[0]) == len(f2[2]) == len(f2[4]) == 0
    one = eng.moi_first_similar_batch(eng.inertia_moments_batch(heavy[4:], hm[4:]), dev[4:])
    assert np.array_equal(one[0], first[4])
    # a NaN max_deviation is taken as the single entry point takes it (no comparison holds: no match), for its segment alone
    nan = eng.moi_first_similar_batch(mo, np.array([1e-2, 1e-3, np.nan, 5e-2, 1e-2]))
    assert np.array_equal(nan[2], eng.moi_first_similar(mo[2], float("nan"))) and (nan[2] == -1).all()
    assert np.array_equal(nan[3], first[3]) and np.array_equal(nan[4], first[4])


@pytest.mark.gpu
def test_batch_prune_equals_the_single_call_per_ensemble():
    pytest.importorskip("networkx")
    import tscode_amd
    ens, atomnos, masses = edge_batch()
    dev = [1e-2, 1e-3, 1e-2, 5e-2, 1e-2]
    got = tscode_amd.prune_by_moment_of_inertia_batch(ens, atomnos, max_deviation=dev, masses=masses)
    pruned = 0
    for s, (e, z, m) in enumerate(zip(ens, atomnos, masses)):
        kept, mask = tscode_amd.prune_by_moment_of_inertia(e, z, max_deviation=dev[s], masses=m)
        assert got[s][1].dtype == np.bool_ and np.array_equal(got[s][1], mask), (s, int(got[s][1].sum()), int(mask.sum()))
        assert np.array_equal(got[s][0], kept), s
        pruned += int((~mask).sum())
    assert pruned > 100, "the clustered segments lost nothing: the prune was not exercised"
    # one atomnos array, one masses array and one max_deviation for all; the built-in table where no masses are given
    same = [ens[3], ens[3][:40], ens[3][::-1]]
    got = tscode_amd.prune_by_moment_of_inertia_batch(same, atomnos[3], masses=masses[3])
    table = tscode_amd.prune_by_moment_of_inertia_batch(same, atomnos[3])
    for e, g, t in zip(same, got, table):
        assert np.array_equal(g[1], tscode_amd.prune_by_moment_of_inertia(e, atomnos[3], masses=masses[3])[1])
        assert np.array_equal(t[1], tscode_amd.prune_by_moment_of_inertia(e, atomnos[3])[1])


@pytest.mark.gpu
def test_the_masses_warning_is_given_once_per_call():
    pytest.importorskip("networkx")
    import warnings

    import tscode_amd
    import tscode_amd.optimization_methods as om
    ens, atomnos, _ = edge_batch()
    om._WARNED_MASSES = False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        tscode_amd.prune_by_moment_of_inertia_batch(ens, atomnos)
    assert len([w for w in seen if "built-in table of standard atomic weights" in str(w.message)]) == 1


@pytest.mark.gpu
def test_g9_cases_as_one_batch_give_the_recorded_masks():
    """What test_moi_and_scores_golden asserts for the recorded cases one by one, for all of them in one call."""
    pytest.importorskip("networkx")
    import tscode_amd
    g = load_golden("G9_moi_scores")
    cases = list(range(int(g["n_cases"]))) + ["h"]
    structures = [g[f"structures{c}"] if c != "h" else g["h_structures"] for c in cases]
    atomnos = [g[f"atomnos{c}"] if c != "h" else g["h_atomnos"] for c in cases]
    masses = [g[f"masses{c}"] if c != "h" else g["h_masses"] for c in cases]
    want = [g[f"mask{c}"] if c != "h" else g["h_mask"] for c in cases]
    got = tscode_amd.prune_by_moment_of_inertia_batch(structures, atomnos, max_deviation=1e-2, masses=masses)
    for c, s, (kept, mask), w in zip(cases, structures, got, want):
        assert np.array_equal(mask, w), c
        assert np.array_equal(kept, s[w]), c
    eng = tscode_amd.get_engine(0)
    mo = eng.inertia_moments_batch(structures[:-1], masses[:-1])
    first = eng.moi_first_similar_batch(mo, np.full(len(mo), 1e-2))
    for c, m, f in zip(cases[:-1], mo, first):
        assert (np.abs(m - g[f"moments{c}"]) / np.abs(g[f"moments{c}"])).max() < 1e-12
        assert [(int(i), int(f[i])) for i in np.flatnonzero(f >= 0)] == [tuple(x) for x in g[f"matches{c}"].tolist()]
