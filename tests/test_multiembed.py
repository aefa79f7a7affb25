"""tsc_cyclical_embed_groups, multiembed_batch and the multiembed drop-ins.  The yardstick is always the recorded fixture (G27: the reference's
own functions driven in run_child_embedder's order; G12 / G18 for the embed itself), an EXISTING entry point on the same input
(tsc_cyclical_embed on the expanded rows; cyclical_embed_batch -> fitness_mask -> similarity_refining_batch per arrangement) or the
reference's loops restated in this file -- never the new code."""

import json
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

VAL_TOL = 1e-9          # the project's asserted value-parity tolerance (tests/test_gpu_parity.py:15)
SYMBOL = "tsc_cyclical_embed_groups"
_cache = {}


def g27():
    if "g27" not in _cache:
        _cache["g27"] = load_golden("G27_multiembed")
    return _cache["g27"]


def cases(g):
    return [str(k) for k in g["cases"]]


def sites():
    with open(os.path.join(GOLDEN, "G27_multiembed.json")) as f:
        return json.load(f)["sites"]


def arrs_of(g, key):
    return g[f"arrangements_{key}"]


def recorded_molecule(g, key, a, m):
    """What cyclical_embed_batch reads from molecule m of arrangement a, as the reference built it."""
    coords = g[f"coords{m}_{key}"]
    return dict(coords=coords, reactive_indices=g[f"reactive_indices{m}_{key}_{a}"],
                pivots=[(g[f"pivot_vec{m}_{c}_{key}_{a}"], g[f"pivot_mean{m}_{c}_{key}_{a}"], g[f"pivot_cumnums{m}_{c}_{key}_{a}"]) for c in range(len(coords))])


def by_ordered_pair(g, key):
    """({(ix, iy): molecule}, {(ix, iy): lobes}) per side, collected from the arrangements that use the pair."""
    mols, lobes = [{}, {}], [{}, {}]
    for a, ((ix_1, ix_2), (iy_1, iy_2)) in enumerate(arrs_of(g, key).tolist()):
        for m, pair in enumerate(((ix_1, iy_1), (ix_2, iy_2))):
            mols[m].setdefault(pair, recorded_molecule(g, key, a, m))
            lobes[m].setdefault(pair, [g[f"lobes{m}_{j}_{key}_{a}"] for j in range(2)])
            assert tuple(mols[m][pair]["reactive_indices"].tolist()) == pair
    return mols, lobes


def used_groups(g, key, a):
    """The groups the reference's loop entered (its _get_cyclical_reactive_indices is also called for the orientation the pairings skip)."""
    group_of = g[f"group_of_{key}_{a}"]
    used = np.unique(group_of)
    assert np.array_equal(group_of, np.repeat(used, len(g[f"angles_{key}"])))          # in order, A candidates each
    return used


def restated_records(g, key, a):
    """The rigid shortcut's loops (tscode/embeds.py:741-783) restated plainly on the recorded pivots: conformer pairs and pivot pairs in
    cartesian_product's order, pairs of pivots more than 5 apart skipped, and of the two polygon orientations the one whose facing atoms are
    the child's pairings (x with x, y with y: orientation 0)."""
    from tscode_amd.utils import cartesian_product
    mols = [recorded_molecule(g, key, a, m) for m in range(2)]
    direction = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    recs, ids = [], []
    for conf in cartesian_product(*[np.arange(len(m["coords"])) for m in mols]):
        for pi in cartesian_product(*[np.arange(len(m["pivots"][c][0])) for m, c in zip(mols, conf)]):
            pv = [m["pivots"][c][0][i] for m, c, i in zip(mols, conf, pi)]
            norms = np.linalg.norm(np.array(pv), axis=1)                                 # :759, as written there (the axis form sums in another order than norm(v))
            if abs(norms[0] - norms[1]) > 5:
                continue
            rec = np.zeros((2, 23))
            for m in range(2):
                r = mols[m]["coords"][conf[m]][mols[m]["reactive_indices"]]
                rec[m, 0], rec[m, 3] = -norms[m] / 2, norms[m] / 2
                rec[m, 6:9], rec[m, 9:12], rec[m, 12:15] = direction[m], pv[m], mols[m]["pivots"][conf[m]][1][pi[m]]
                rec[m, 15:18], rec[m, 18:21], rec[m, 21], rec[m, 22] = r[0], r[1], 2, conf[m]
            c0, c1 = (mols[m]["pivots"][conf[m]][2][pi[m]] for m in range(2))
            recs.append(rec), ids.append([[c0[0], c1[0]], [c0[1], c1[1]]])
    return np.array(recs).reshape(-1, 2, 23), np.array(ids, dtype=np.int64).reshape(-1, 2, 2)


def _no_device(monkeypatch):
    from tscode_amd import graph_manipulations, multiembed, numba_functions, optimization_methods, reactive_atoms

    def no_device(*a, **k):
        raise AssertionError("the library was entered")
    for mod in (graph_manipulations, multiembed, numba_functions, optimization_methods, reactive_atoms):
        monkeypatch.setattr(mod, "get_engine", no_device)


# ------------------------------------------------------------------------------------------------------- CPU
def test_arrangements_in_the_reference_order():
    from tscode_amd.multiembed import arrangements
    g = g27()
    for key in ("a", "b"):
        got = arrangements(g[f"reactive0_{key}"], g[f"reactive1_{key}"])
        assert got.dtype == np.int64 and np.array_equal(got, arrs_of(g, key)), key
    assert len(arrs_of(g, "a")) == 4 and len(arrs_of(g, "b")) == 12
    for r1, r2, n in (([4, 9], [1, 2], 4), ([5, 0, 7], [2, 6], 12), ([0, 1, 2, 3], [7, 5, 3, 1], 144)):
        got = arrangements(r1, r2)
        assert got.shape == (n, 2, 2) and len({tuple(x.ravel()) for x in got}) == n
        assert (got[:, 0, 0] != got[:, 1, 0]).all() and (got[:, 0, 1] != got[:, 1, 1]).all()       # distinct atoms on both sides
        assert set(got[:, :, 0].ravel()) == set(r1) and set(got[:, :, 1].ravel()) == set(r2)
        seen = {tuple(map(tuple, x)) for x in got.tolist()}
        assert {(x[1], x[0]) for x in seen} == seen                                                  # both orders occur


def test_group_records_and_facing_atoms_against_the_fixture(monkeypatch):
    from tscode_amd.multiembed import group_records
    _no_device(monkeypatch)
    g = g27()
    for key in ("a", "b", "c"):
        mols, _ = by_ordered_pair(g, key)
        arrs = arrs_of(g, key)
        n1 = int(g[f"ids_{key}"][0])
        rec, ids, per = group_records(mols[0], mols[1], arrs, n1)
        assert rec.shape == (per.sum(), 2, 23) and ids.shape == (per.sum(), 2, 2) and len(per) == len(arrs)
        at = 0
        for a in range(len(arrs)):
            used = used_groups(g, key, a)
            assert per[a] == len(used), (key, a)
            assert np.array_equal(ids[at:at + per[a]], g[f"group_ids_{key}_{a}"][used]), (key, a)       # the reference's facing atoms, group by group
            want_rec, want_ids = restated_records(g, key, a)
            assert np.array_equal(want_ids, ids[at:at + per[a]])
            assert np.array_equal(rec[at:at + per[a]], want_rec), (key, a)
            at += per[a]


def test_quadruplets_and_fitness_targets_against_the_fixture(monkeypatch):
    from tscode_amd.multiembed import arrangement_quadruplets, fitness_targets, orbital_lengths
    _no_device(monkeypatch)
    g = g27()
    for key in ("a", "b", "c"):
        arrs = arrs_of(g, key)
        n1, n2 = (int(x) for x in g[f"ids_{key}"])
        quads = arrangement_quadruplets(g[f"edges0_{key}"], g[f"edges1_{key}"], n1, n2, arrs)
        _, lobes = by_ordered_pair(g, key)
        lengths = [{pair: orbital_lengths(lb, g[f"coords{m}_{key}"][0], pair) for pair, lb in lobes[m].items()} for m in range(2)]
        targets = fitness_targets(arrs, lengths[0], lengths[1])
        for a in range(len(arrs)):
            assert np.array_equal(quads[a], g[f"quadruplets_{key}_{a}"]), (key, a)
            assert len(quads[a]) > 0
            assert np.abs(targets[a] - g[f"targets_{key}_{a}"]).max() < 1e-12, (key, a, targets[a], g[f"targets_{key}_{a}"])
        assert not bool(g[f"is_single_molecule_{key}_0"]) and not bool(g[f"ref_tfd_entered_{key}_0"]) and bool(g[f"tfd_tfd_entered_{key}_0"])


def test_argument_errors_are_raised_before_the_library_is_entered(monkeypatch):
    import tscode_amd
    from tscode_amd import multiembed as M
    from tscode_amd.embeds import MAX_GROUP_POSES
    from tscode_amd.reactive_atoms import MAX_ATOMS
    _no_device(monkeypatch)
    g = g27()
    mol = lambda m, **kw: {**dict(coords=g[f"coords{m}_b"], atomnos=g[f"atomnos{m}_b"], reactive_indices=g[f"reactive{m}_b"], bonds=g[f"edges{m}_b"]), **kw}
    n2 = len(g["atomnos1_b"])
    bad_coords = g["coords1_b"].copy()
    bad_coords[0, 2, 1] = np.nan
    inf_coords = g["coords0_b"].copy()
    inf_coords[0, 0, 0] = np.inf
    for m1, m2, kw in ((mol(0, reactive_indices=[3]), mol(1), {}),                       # fewer than two reactive atoms on a side
                       (mol(0), mol(1, reactive_indices=[]), {}),
                       (mol(0), mol(1, reactive_indices=[1, n2]), {}),                   # out of range
                       (mol(0, reactive_indices=[-1, 3]), mol(1), {}),
                       (mol(0), mol(1, reactive_indices=[1, 3, 1]), {}),                 # a duplicate
                       (mol(0), mol(1), dict(systematic_angles=np.zeros((MAX_GROUP_POSES + 1, 2)))),
                       (mol(0), mol(1), dict(systematic_angles=np.zeros((0, 2)))),
                       (mol(0), mol(1), dict(systematic_angles=np.zeros((4, 3)))),
                       (mol(0), mol(1, coords=bad_coords), {}),                          # non-finite coordinates
                       (mol(0, coords=inf_coords), mol(1), {}),
                       (mol(0), mol(1), dict(max_poses_per_call=0)),
                       (mol(0, atomnos=g["atomnos0_b"][:-1]), mol(1), {})):              # atoms and atomic numbers disagree
        with pytest.raises(ValueError):
            tscode_amd.multiembed_batch(m1, m2, **kw)
    big = MAX_ATOMS + 1                                                                   # over the limit orbitals_batch states
    with pytest.raises(ValueError, match=str(MAX_ATOMS)):
        M.check_args(dict(coords=np.zeros((1, big, 3)), atomnos=np.ones(big, dtype=np.int64), reactive_indices=[0, 1]), mol(1))


def _fake_modules():
    names = sorted({m for mods in sites().values() for m in mods} | {"tscode.embeds", "tscode.operators"})
    mods = {}
    for n in names:
        m = types.ModuleType(n)
        m.multiembed_dispatcher = lambda embedder: ("the reference's dispatcher", len(embedder.objects))
        m.multiembed_bifunctional = lambda embedder: ("the reference's bifunctional", len(embedder.objects))
        mods[n] = m
    return mods


def test_install_multiembed_sites():
    """install(multiembed=True) patches exactly the sites recorded from the reference's import lines; install() alone none; uninstall() restores."""
    import tscode_amd
    from tscode_amd import multiembed as M
    recorded = sites()
    assert sorted(recorded) == ["multiembed_bifunctional", "multiembed_dispatcher"]
    mods = _fake_modules()
    before = {(n, attr): getattr(m, attr) for n, m in mods.items() for attr in recorded}
    try:
        done = tscode_amd.install(modules=mods)
        assert not [d for d in done if d[1] in recorded]
        assert all(getattr(mods[n], attr) is fn for (n, attr), fn in before.items())
        tscode_amd.uninstall(modules=mods)
        done = tscode_amd.install(modules=mods, multiembed=True)
        want = sorted((m, attr) for attr, where in recorded.items() for m in where)
        assert sorted(d for d in done if d[1] in recorded) == want
        for n, m in mods.items():
            for attr in recorded:
                assert (getattr(m, attr) is getattr(M, attr)) == (n in recorded[attr]), (n, attr)
        assert M._originals == {attr: before[("tscode.multiembed", attr)] for attr in recorded}
    finally:
        tscode_amd.uninstall(modules=mods)
    assert all(getattr(mods[n], attr) is fn for (n, attr), fn in before.items())
    assert M._originals == {}


def test_runs_the_dropin_does_not_cover_reach_the_recorded_originals():
    """Three objects through the dispatcher, and shrink / simpleorbitals / debug children, go to the reference's own functions."""
    import tscode_amd
    from tscode_amd import multiembed as M
    mods = _fake_modules()
    opts = lambda **kw: types.SimpleNamespace(**{**dict(shrink=False, simpleorbitals=False, debug=False), **kw})
    three = types.SimpleNamespace(objects=[object()] * 3, options=opts())
    with pytest.raises(RuntimeError, match="install"):
        M.multiembed_dispatcher(three)                                       # nothing recorded to hand it to
    try:
        tscode_amd.install(modules=mods, multiembed=True)
        assert mods["tscode.embedder"].multiembed_dispatcher is M.multiembed_dispatcher
        assert mods["tscode.embedder"].multiembed_dispatcher(three) == ("the reference's dispatcher", 3)
        for kw in (dict(shrink=True), dict(simpleorbitals=True), dict(debug=True)):
            two = types.SimpleNamespace(objects=[object()] * 2, options=opts(**kw))
            assert M.multiembed_dispatcher(two) == ("the reference's bifunctional", 2)
    finally:
        tscode_amd.uninstall(modules=mods)


def test_header_and_symbol_table_declare_the_grouped_entry_point():
    from tscode_amd import _lib
    with open(os.path.join(ROOT, "include", "tscode_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", header)
    assert SYMBOL in _lib.EXPORTED_SYMBOLS
    assert "multiembed.py:26-82" in header and "embeds.py:657-717" in header


# ------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def rows_and_groups(eng, coords, blocks, angles, thresh, max_clashes=0):
    """The same records through tsc_cyclical_embed on the expanded rows (the existing entry point, expanded as _run_cyclical_groups does) and
    through tsc_cyclical_embed_groups.  Verdicts must be identical, poses within VAL_TOL.  Returns the grouped result and whether the poses
    were bit-equal."""
    import tscode_amd
    n_mols = len(coords)
    angles = np.asarray(angles, dtype=np.float64).reshape(-1, n_mols)
    G, A = len(blocks), len(angles)
    frags = tscode_amd.FragmentSet(coords)
    expand = lambda lo, hi, dtype=np.float64: np.repeat(np.ascontiguousarray(blocks[:, :, lo:hi], dtype=dtype), A, axis=0).reshape(-1, hi - lo)
    ok_r, kept_r, poses_r = eng.cyclical_embed(frags, *[expand(lo, lo + 3) for lo in range(0, 21, 3)], expand(21, 22, np.int32).reshape(-1),
                                               np.tile(angles, (G, 1)).reshape(-1), expand(22, 23, np.int32).reshape(-1),
                                               np.arange(G + 1, dtype=np.int32) * A, thresh, max_clashes)
    cut = lambda lo, hi, dtype=np.float64: np.ascontiguousarray(blocks[:, :, lo:hi], dtype=dtype)
    ok_g, kept_g, poses_g = eng.cyclical_embed_groups(frags, *[cut(lo, lo + 3) for lo in range(0, 21, 3)], cut(21, 22, np.int32), cut(22, 23, np.int32),
                                                      angles, thresh, max_clashes)
    assert ok_g.shape == (G * A,) and np.array_equal(ok_g, ok_r), (int(ok_g.sum()), int(ok_r.sum()))       # clash_ok and n_pass
    assert np.array_equal(kept_g, kept_r), (int(kept_g.sum()), int(kept_r.sum()))                             # kept and n_kept
    assert poses_g.shape == poses_r.shape == (int(kept_r.sum()), sum(c.shape[1] for c in coords), 3)
    assert len(poses_g) == 0 or np.abs(poses_g - poses_r).max() < VAL_TOL
    return ok_g, kept_g, poses_g, np.array_equal(poses_g, poses_r)


def g12_records(k):
    from tscode_amd.embeds import _bimolecular_groups
    g = load_golden("G12_cyclical_embed")
    coords = [np.ascontiguousarray(g[f"coords{m}_{k}"]) for m in range(2)]
    pivots = [[(g[f"pivot_vec{m}_{c}_{k}"], g[f"pivot_mean{m}_{c}_{k}"], g[f"pivot_cumnums{m}_{c}_{k}"]) for c in range(len(coords[m]))] for m in range(2)]
    blocks, ids, _ = _bimolecular_groups(coords, [g[f"reactive_indices{m}_{k}"] for m in range(2)], pivots, rigid_shortcut=bool(g[f"rigid_{k}"]))
    return g, coords, blocks, ids


@pytest.mark.gpu
def test_grouped_entry_point_equals_the_row_entry_point_on_g12_and_g18(eng):
    from tscode_amd.embeds import _trimolecular_groups
    bit_equal = []
    for k in range(4):
        g, coords, blocks, ids = g12_records(k)
        ok, kept, poses, same = rows_and_groups(eng, coords, blocks, g[f"angles_{k}"], float(g[f"clash_thresh_{k}"]))
        bit_equal.append(same)
        assert np.array_equal(ok, g[f"clash_ok_{k}"]) and np.array_equal(kept, g[f"kept_{k}"]), k
        assert poses.shape == g[f"poses_{k}"].shape and np.abs(poses - g[f"poses_{k}"]).max() < VAL_TOL
        A = len(g[f"angles_{k}"])
        assert np.array_equal(ids[np.repeat(np.arange(len(blocks)), A)[kept]], g[f"constrained_indices_{k}"])
    g = load_golden("G18_cyclical_embed_trimolecular")
    for k in range(int(g["n_cases"])):
        coords = [np.ascontiguousarray(g[f"coords{m}_{k}"]) for m in range(3)]
        pivots = [[(g[f"pivot_vec{m}_{c}_{k}"], g[f"pivot_mean{m}_{c}_{k}"], g[f"pivot_cumnums{m}_{c}_{k}"]) for c in range(len(coords[m]))] for m in range(3)]
        blocks, ids, _ = _trimolecular_groups(coords, [g[f"reactive_indices{m}_{k}"] for m in range(3)], pivots,
                                              [g[f"reactive_cumnums{m}_{k}"] for m in range(3)], None, ())
        ok, kept, poses, same = rows_and_groups(eng, coords, blocks, g[f"angles_{k}"], float(g[f"clash_thresh_{k}"]))
        bit_equal.append(same)
        assert np.array_equal(ok, g[f"clash_ok_{k}"]) and np.array_equal(kept, g[f"kept_{k}"]), k
        assert poses.shape == g[f"poses_{k}"].shape and np.abs(poses - g[f"poses_{k}"]).max() < VAL_TOL
        if k == 0:                                                           # three molecules: a wavefront takes 21 groups (63 records)
            for n_groups in (20, 22, 43, 85):
                rows_and_groups(eng, coords, np.tile(blocks, (-(-n_groups // len(blocks)), 1, 1))[:n_groups], g[f"angles_{k}"], float(g[f"clash_thresh_{k}"]))
    print(f"poses bit-equal between the two entry points, G12 cases then G18 cases: {bit_equal}")


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 36, 63, 64, 65, 1369])
def test_grouped_entry_point_angle_counts(eng, A):
    """Fewer angle sets than lanes, exactly 64, one more, and STEPS = 36 (1369: the group filter's large-group path), on G12 case 0's molecules."""
    from tscode_amd.utils import cartesian_product
    g, coords, blocks, _ = g12_records(0)
    if A == 1369:
        steps = np.linspace(-40.0, 40.0, 37)
        angles = cartesian_product(steps, steps)
    else:
        angles = np.random.default_rng(A).uniform(-45.0, 45.0, size=(A, 2))
    ok, kept, _, _ = rows_and_groups(eng, coords, blocks, angles, float(g["clash_thresh_0"]))
    assert ok.any() and kept.any()


@pytest.mark.gpu
def test_grouped_entry_point_one_group_many_groups_and_mixed_reactive_counts(eng):
    g, coords, blocks, _ = g12_records(0)
    angles, thresh = g["angles_0"], float(g["clash_thresh_0"])
    for one in (0, len(blocks) - 1):                                         # G = 1
        rows_and_groups(eng, coords, blocks[one:one + 1], angles, thresh)
    for n_groups in (31, 33, 65, 129):                                       # around the 32 groups a wavefront takes, and past a workgroup's four
        rows_and_groups(eng, coords, np.tile(blocks, (-(-n_groups // len(blocks)), 1, 1))[:n_groups], angles, thresh)
    # 3 000 groups x 36 poses; and, with two angle sets, 100 000 groups: the parameter kernel gives a wavefront 32 groups and launches at most
    # 768 workgroups of four wavefronts, so past 98 304 groups its grid wraps
    for n_groups, table in ((3000, angles), (100_000, angles[[0, 17]])):
        reps = -(-n_groups // len(blocks))
        many = np.tile(blocks, (reps, 1, 1))
        assert len(many) >= n_groups and (n_groups > 3000 or len(many) * len(table) >= 3000 * 36)
        ok, kept, _, _ = rows_and_groups(eng, coords, many, table, thresh)
        assert np.array_equal(ok.reshape(reps, -1), np.tile(ok[:len(blocks) * len(table)], (reps, 1)))    # every repeat of a group gives the same verdicts
        assert np.array_equal(kept.reshape(reps, -1), np.tile(kept[:len(blocks) * len(table)], (reps, 1)))
    # records of one and of two reactive atoms in one call (one: the pivot is the axis and r1 is not read)
    mixed = blocks.copy()
    mixed[::2, 0, 21] = 1
    mixed[1::3, 1, 21] = 1
    mixed[::2, 0, 18:21] = 1e6                                              # r1 of a one-atom record must not matter
    assert {1.0, 2.0} == set(mixed[:, :, 21].ravel())
    rows_and_groups(eng, coords, mixed, angles, thresh)


@pytest.mark.gpu
def test_grouped_entry_point_refuses_bad_arguments_naming_the_group(eng):
    import tscode_amd
    g, coords, blocks, _ = g12_records(0)
    frags = tscode_amd.FragmentSet(coords)
    cut = lambda b, lo, hi, dtype=np.float64: np.ascontiguousarray(b[:, :, lo:hi], dtype=dtype)
    call = lambda b, angles: eng.cyclical_embed_groups(frags, *[cut(b, lo, lo + 3) for lo in range(0, 21, 3)], cut(b, 21, 22, np.int32),
                                                       cut(b, 22, 23, np.int32), angles, 1.5, 0)
    bad = blocks.copy()
    bad[5, 1, 21] = 3
    with pytest.raises(Exception, match="group 5"):
        call(bad, g["angles_0"])
    bad = blocks.copy()
    bad[7, 0, 22] = len(coords[0])
    with pytest.raises(Exception, match="group 7"):
        call(bad, g["angles_0"])
    with pytest.raises(Exception):
        call(blocks, np.zeros((8193, 2)))
    with pytest.raises(Exception):
        call(blocks, np.zeros((0, 2)))


def packed_molecules(g, key):
    return [dict(coords=g[f"coords{m}_{key}"], atomnos=g[f"atomnos{m}_{key}"], reactive_indices=g[f"reactive{m}_{key}"], bonds=g[f"edges{m}_{key}"])
            for m in range(2)]


def batch_result(g, key, tfd):
    """multiembed_batch on a case of the fixture, computed once per (case, chain) and shared."""
    import tscode_amd
    if ("out", key, tfd) not in _cache:
        mols = packed_molecules(g, key)
        _cache[("out", key, tfd)] = tscode_amd.multiembed_batch(mols[0], mols[1], fitness_threshold=float(g[f"fitness_threshold_{key}"]), tfd=tfd)
    return _cache[("out", key, tfd)]


@pytest.mark.gpu
@pytest.mark.parametrize("tfd", [False, True])
def test_multiembed_batch_against_the_fixture(eng, tfd):
    """All cases, both chains: "ref" = what the reference's child does (its TFD gate is never open for two separate molecules), "tfd" = the
    same with the TFD stage entered, the reference's own prune_conformers_tfd on the recorded quadruplets."""
    g = g27()
    chain = "tfd" if tfd else "ref"
    for key in cases(g):
        out = batch_result(g, key, tfd)
        arrs = arrs_of(g, key)
        assert np.array_equal(out.arrangements, arrs)
        want_counts = np.array([g[f"{chain}_counts_{key}_{a}"] for a in range(len(arrs))])
        assert np.array_equal(out.counts, want_counts), (key, chain, out.counts.tolist(), want_counts.tolist())
        assert np.abs(out.targets - np.array([g[f"targets_{key}_{a}"] for a in range(len(arrs))])).max() < 1e-9
        at = np.zeros(4, dtype=np.int64)             # rows consumed of: kept poses, fit, after TFD, final
        structures, constrained, arr_of = [], [], []
        for a in range(len(arrs)):
            lo, hi = out.candidate_off[a], out.candidate_off[a + 1]
            assert np.array_equal(out.clash_ok[lo:hi], g[f"clash_ok_{key}_{a}"]), (key, a)
            assert np.array_equal(out.kept[lo:hi], g[f"kept_{key}_{a}"]), (key, a)
            c = want_counts[a]
            fit, m_tfd, m_moi = (g[f"{chain}_{s}_mask_{key}_{a}"] for s in ("fitness", "tfd", "moi"))
            assert np.array_equal(out.masks["fitness"][at[0]:at[0] + c[2]], fit), (key, a)
            assert np.array_equal(out.masks["tfd"][at[1]:at[1] + c[3]], m_tfd), (key, a)
            assert np.array_equal(out.masks["moi"][at[2]:at[2] + c[4]], m_moi), (key, a)
            at += c[2:6]
            left = g[f"poses_{key}_{a}"][fit][m_tfd][m_moi]                      # the embed's own coordinates of what the child keeps
            structures.append(left), arr_of.append(np.full(len(left), a))
            constrained.append(g[f"constrained_indices_{key}_{a}"][fit][m_tfd][m_moi])
            assert np.array_equal(constrained[-1], g[f"{chain}_final_constrained_{key}_{a}"])
            centred = left - left.mean(axis=1, keepdims=True)
            assert np.abs(centred - g[f"{chain}_final_{key}_{a}"]).max() < VAL_TOL      # (what the fixture says the child hands back)
        assert np.array_equal(out.arrangement_of, np.concatenate(arr_of))
        assert np.array_equal(out.constrained_indices, np.concatenate(constrained))
        want = np.concatenate(structures)
        assert out.structures.shape == want.shape and np.abs(out.structures - want).max() < VAL_TOL, (key, chain)
    if tfd:
        assert any((g[f"tfd_counts_{key}_{a}"][3] > g[f"tfd_counts_{key}_{a}"][4]) for key in cases(g) for a in range(len(arrs_of(g, key))))


def existing_calls(g, key, a, tfd, clash_thresh=1.5):
    """One arrangement alone through the calls that exist without this feature: reactive_molecule, cyclical_embed_batch (tsc_cyclical_embed),
    fitness_mask, similarity_refining_batch(rmsd=False).  The targets and quadruplets are the fixture's."""
    import tscode_amd
    (ix_1, ix_2), (iy_1, iy_2) = arrs_of(g, key)[a].tolist()
    mols = packed_molecules(g, key)
    n1 = len(mols[0]["atomnos"])
    rms = [tscode_amd.reactive_molecule(m["coords"], m["atomnos"], list(pair), m["bonds"], cumnum_offset=off)
           for m, pair, off in zip(mols, ((ix_1, iy_1), (ix_2, iy_2)), (0, n1))]
    poses, cons = tscode_amd.cyclical_embed_batch(rms, g[f"angles_{key}"], clash_thresh=clash_thresh, rigid_shortcut=True, max_norm_delta=5,
                                                  pairings=[[ix_1, ix_2 + n1], [iy_1, iy_2 + n1]])
    if not len(poses):
        return poses, cons, (None, None)
    fit = tscode_amd.fitness_mask(poses, cons, np.tile(g[f"targets_{key}_{a}"], (len(poses), 1)), float(g[f"fitness_threshold_{key}"]))
    if not fit.any():
        return poses[fit], cons[fit], (fit, None)
    atomnos = np.concatenate([m["atomnos"] for m in mols])
    (left, mask), = tscode_amd.similarity_refining_batch([poses[fit]], atomnos, quadruplets=[g[f"quadruplets_{key}_{a}"]] if tfd else None, rmsd=False)
    return left, cons[fit][mask], (fit, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("tfd", [False, True])
def test_multiembed_batch_against_the_existing_calls_per_arrangement(eng, tfd):
    g = g27()
    for key in ("b", "c"):
        out = batch_result(g, key, tfd)
        fit_at = 0
        for a in range(len(arrs_of(g, key))):
            left, cons, (fit, mask) = existing_calls(g, key, a, tfd)
            mine = out.arrangement_of == a
            n_kept, n_fit = out.counts[a, 2], out.counts[a, 3]
            assert np.array_equal(out.masks["fitness"][fit_at:fit_at + n_kept], fit), (key, a)
            fit_at += n_kept
            lo = out.counts[:a, 3].sum()
            both = out.masks["tfd"][lo:lo + n_fit].copy()
            t_lo = out.counts[:a, 4].sum()
            both[both] = out.masks["moi"][t_lo:t_lo + out.counts[a, 4]]
            assert np.array_equal(both, mask), (key, a)
            assert np.array_equal(out.constrained_indices[mine], cons)
            assert out.structures[mine].shape == left.shape and np.abs(out.structures[mine] - left).max() < VAL_TOL, (key, a)


@pytest.mark.gpu
def test_slab_size_does_not_change_the_result(eng):
    import tscode_amd
    g = g27()
    for key, per_call in (("a", 36), ("c", 36 * 100 + 7)):       # one group per call; slabs that end inside an arrangement
        mols = packed_molecules(g, key)
        whole = batch_result(g, key, True)
        slabbed = tscode_amd.multiembed_batch(mols[0], mols[1], fitness_threshold=float(g[f"fitness_threshold_{key}"]), tfd=True, max_poses_per_call=per_call)
        for name in ("structures", "constrained_indices", "arrangement_of", "counts", "clash_ok", "kept"):
            assert np.array_equal(getattr(whole, name), getattr(slabbed, name)), (key, name)
        for name in ("fitness", "tfd", "moi"):
            assert np.array_equal(whole.masks[name], slabbed.masks[name]), (key, name)


EMPTYING_THRESH = 1.6     # case b: four arrangements lose every pose to the clash check here and eight do not (asserted below); the nearest clash
                          # distance of a candidate lies 4e-5 from it (the CPU oracle on the recorded pivots)


@pytest.mark.gpu
def test_arrangements_that_end_empty_drop_out(eng):
    import tscode_amd
    g = g27()
    mols = packed_molecules(g, "b")
    out = tscode_amd.multiembed_batch(mols[0], mols[1], clash_thresh=EMPTYING_THRESH)
    empty = out.counts[:, 1] == 0
    assert empty.any() and not empty.all(), out.counts[:, :3].tolist()
    assert not np.isin(out.arrangement_of, np.flatnonzero(empty)).any()
    assert (out.counts[empty, 1:] == 0).all() and (out.counts[:, 0] == g["ref_counts_b_0"][0]).all()
    for a in range(len(empty)):                                  # the rest: what each gives alone through the existing calls
        left, cons, _ = existing_calls(g, "b", a, False, clash_thresh=EMPTYING_THRESH)
        mine = out.arrangement_of == a
        assert mine.sum() == len(left) == out.counts[a, 5], a
        if len(left):
            assert np.abs(out.structures[mine] - left).max() < VAL_TOL and np.array_equal(out.constrained_indices[mine], cons)
    nothing = tscode_amd.multiembed_batch(mols[0], mols[1], clash_thresh=9.0)       # every arrangement empty: the empty arrays
    assert nothing.structures.shape == (0, 11, 3) and nothing.constrained_indices.shape == (0, 2, 2) and len(nothing.arrangement_of) == 0
    assert not nothing.counts[:, 1:].any()


def duck_embedder(g, key, logs, **options):
    import networkx as nx
    objects = []
    for m in range(2):
        graph = nx.Graph()
        graph.add_nodes_from(range(len(g[f"atomnos{m}_{key}"])))
        graph.add_edges_from(g[f"edges{m}_{key}"].tolist())
        objects.append(types.SimpleNamespace(atomcoords=g[f"coords{m}_{key}"], atomnos=g[f"atomnos{m}_{key}"], reactive_indices=g[f"reactive{m}_{key}"],
                                             graph=graph, name=f"mol{m}.xyz"))
    opts = dict(shrink=False, simpleorbitals=False, debug=False, let=False, clash_thresh=1.5, max_clashes=0)
    opts.update(options)
    return types.SimpleNamespace(objects=objects, options=types.SimpleNamespace(**opts), avail_cpus=4, log=lambda *a, **k: logs.append(a))


@pytest.mark.gpu
def test_dropin_returns_what_the_children_hand_back(eng):
    """multiembed_bifunctional(embedder) on duck-typed molecules carrying the fixture's arrays: the centred structures the reference's children
    leave behind, concatenated in arrangement order, and embedder.constrained_indices."""
    from tscode_amd import multiembed as M
    g = g27()
    for key in ("a", "b", "c"):
        logs = []
        emb = duck_embedder(g, key, logs)
        got = M.multiembed_dispatcher(emb)
        n_arr = len(arrs_of(g, key))
        want = np.concatenate([g[f"ref_final_{key}_{a}"] for a in range(n_arr)])
        assert got.shape == want.shape and np.abs(got - want).max() < VAL_TOL, key
        assert np.array_equal(emb.constrained_indices, np.concatenate([g[f"ref_final_constrained_{key}_{a}"] for a in range(n_arr)]))
        assert np.abs(got.mean(axis=1)).max() < 1e-12                                   # centred, as write_structures leaves them
        text = " ".join(str(x) for line in logs for x in line)
        assert f"running {n_arr} embeds" in text and f"generated {len(want)} candidates" in text
