"""The clustered conformational search of a whole ensemble (csrc/torsions.hpp: k_torsion_groups; tscode_amd.torsion_module:
group_torsions_batch, clustered_csearch_batch, csearch_batch and the install(csearch=True) drop-ins): fixture G26
(tests/golden/gen_clustered_csearch.py: the reference's own _group_torsions_dbscan and its whole clustered_csearch, mode 1) and a
sweep of the grouping kernel against a NumPy yardstick written here from the definition at tsc_torsion_groups in
include/tscode_hip.h."""

import json
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

COORD_TOL = 1e-9               # Angstrom (tests/test_diverse.py): the structures pass through an alignment
DIST_BAND = 1e-6               # every pair distance of the centres stays this far from every level (G20's band)
LEVELS = np.arange(10, 1.5, -0.5)
T_LIST = (1, 8, 9, 10, 63, 64, 65, 130, 512)
TSC_ERR_INVALID = -1
NEW_SYMBOLS = ("tsc_torsion_groups", "tsc_torsion_groups_dev", "tsc_torsion_groups_timings")


# ------------------------------------------------------------------------------------------------------- fixture
_g26 = {}


def g26():
    if not _g26:
        g = load_golden("G26_clustered_csearch")
        _g26["g"] = g
        _g26["meta"] = json.loads(g["meta_json"].tobytes().decode())
    return _g26["g"], _g26["meta"]


def sites():
    with open(os.path.join(GOLDEN, "G26_clustered_csearch_sites.json")) as f:
        return json.load(f)["sites"]


# ------------------------------------------------------------------------------------------------------- yardstick
def yard_groups(coords, torsions, max_size=5, min_torsions=9):
    """(group_of i32[T], n_groups, eps_index, oversize, margin) from the definition of tsc_torsion_groups.  margin: the smallest
    distance of a pair of centres from a level."""
    torsions = np.asarray(torsions).reshape(-1, 4)
    T = len(torsions)
    if T < min_torsions or T == 0:
        return np.zeros(T, np.int32), 1 if T else 0, -1, 0, np.inf
    c = (coords[torsions[:, 1]] + coords[torsions[:, 2]]) / 2
    d = c[:, None, :] - c[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    off = np.sqrt(d2[np.triu_indices(T, 1)])
    margin = float(np.abs(off[:, None] - LEVELS[None, :]).min()) if len(off) else np.inf
    for level, eps in enumerate(LEVELS):
        linked = d2 <= eps * eps
        first = np.arange(T)                                                # the smallest member of every torsion's component
        while True:
            new = np.where(linked, first[None, :], T).min(axis=1)
            new = new[new]
            if np.array_equal(new, first):
                break
            first = new
        roots, label, sizes = np.unique(first, return_inverse=True, return_counts=True)   # labels by smallest member
        if sizes.max() <= max_size:
            break
    order = np.argsort(sizes, kind="stable")                                # sorted(output, key=len)
    place = np.empty(len(order), np.int32)
    place[order] = np.arange(len(order))
    return place[label].astype(np.int32), len(roots), level, int(sizes.max() > max_size), margin


def test_fixture_loads():
    g, meta = g26()
    assert len(meta["part_a"]) >= 14 * 1 and len(meta["part_b"]) == 3
    assert {c["T"] for c in meta["part_a"]} == {8, 9, 10, 33, 64, 65, 130} and {c["max_size"] for c in meta["part_a"]} == {5, 3}
    assert meta["levels"] == LEVELS.tolist() and len(LEVELS) == 17
    assert all(c["margin"] >= DIST_BAND for c in meta["part_a"])
    kept = {c["eps_index"] for c in meta["part_a"] if not c["oversize"]}
    assert 0 in kept and 16 in kept and any(0 < e < 16 for e in kept)       # level 10.0, level 2.0, an interior one
    assert any(c["oversize"] and c["design"] == "line" and c["n_groups"] == 1 for c in meta["part_a"])
    assert any(len(set(c["sizes"])) < len(c["sizes"]) for c in meta["part_a"])           # groups of equal size: the stable order
    for p in meta["part_b"]:
        assert p["n_groups"] >= 2 and p["calls"] == p["n_groups"]
        assert all(built > meta["n"] for built, _ in p["round_sizes"][:-1]) and p["round_sizes"][-1][0] > meta["n_out"]
        assert g[f"b{p['index']}_out"].shape == (p["n_final"], 40, 3)
    assert os.path.getsize(os.path.join(GOLDEN, "G26_clustered_csearch.npz")) < 1 << 20


def test_yardstick_reproduces_the_reference_grouping():
    g, meta = g26()
    for c in meta["part_a"]:
        k = c["index"]
        group_of, n_groups, eps_index, oversize, margin = yard_groups(g[f"a{k}_coords"], g[f"a{k}_torsions"], c["max_size"], min_torsions=0)
        assert np.array_equal(group_of, g[f"a{k}_group_of"]), c
        assert (n_groups, eps_index, oversize) == (c["n_groups"], c["eps_index"], c["oversize"]), c
        assert margin >= DIST_BAND
        if c["T"] < 9:                                                      # clustered_csearch does not call the function there (:689)
            assert yard_groups(g[f"a{k}_coords"], g[f"a{k}_torsions"], c["max_size"])[:4][1:] == (1, -1, 0)


def test_new_symbols_are_exported():
    from tscode_amd import _lib
    from tscode_amd.build import build
    build()
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED_SYMBOLS, s


def test_argument_checks_come_before_the_library(monkeypatch):
    import tscode_amd
    from tscode_amd import torsion_module as tm

    def no_engine():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(tm, "get_engine", no_engine)
    x = np.zeros((2, 6, 3))
    quads = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.int32)
    bad = [dict(structures=np.zeros((2, 6, 2))), dict(structures=np.zeros((2, 0, 3))), dict(structures=np.full((2, 6, 3), np.nan)),
           dict(max_size=0), dict(max_size=2.5), dict(torsion_sets=[quads, quads, quads]), dict(set_of_structure=[0, 1]),
           dict(set_of_structure=[0]), dict(set_of_structure=[0, -2]), dict(torsion_sets=[np.array([[0, 1, 2, 6]])]),
           dict(torsion_sets=[np.array([[0, -1, 2, 3]])]), dict(torsion_sets=[np.zeros((513, 4), np.int32)])]
    for kw in bad:
        a = dict(structures=x, torsion_sets=[quads], set_of_structure=None, max_size=5)
        a.update(kw)
        with pytest.raises(ValueError):
            tm.group_torsions_batch(**a)
    z = np.array([6, 6, 1, 1, 1, 1])
    for kw in (dict(n=0), dict(n=2.5), dict(n_out=0), dict(max_size=0), dict(init_rows=[1, 2]), dict(structures=np.zeros((2, 5, 3))),
               dict(atomnos=z.astype(float)), dict(constrained_indices=[[0, 9]])):
        a = dict(structures=x, atomnos=z)
        a.update(kw)
        with pytest.raises(ValueError):
            tscode_amd.clustered_csearch_batch(**a)
    with pytest.raises(ValueError, match="optimiser"):
        tscode_amd.csearch_batch(x, z, mode=0)
    with pytest.raises(ValueError):
        tscode_amd.csearch_batch(x, z, mode=3)
    with pytest.raises(RuntimeError, match="install"):                      # nothing recorded to hand ff_opt to
        tm.clustered_csearch(x[0], z, [], None, ff_opt=True)


def _fake_modules():
    names = sorted({m for mods in sites().values() for m in mods} | {"tscode.embedder", "tscode.operators"})
    original = object()
    mods = {}
    for n in names:
        m = types.ModuleType(n)
        m.clustered_csearch = m._group_torsions_dbscan = original
        mods[n] = m
    return mods, original


def test_install_csearch_sites():
    """install(csearch=True) patches exactly the sites recorded from the reference's import lines; uninstall() restores them."""
    import tscode_amd
    from tscode_amd import torsion_module as tm
    recorded = sites()
    assert sorted(recorded) == ["_group_torsions_dbscan", "clustered_csearch"]
    mods, original = _fake_modules()
    try:
        done = tscode_amd.install(modules=mods, csearch=True)
        want = sorted((m, attr) for attr, where in recorded.items() for m in where)
        assert sorted(d for d in done if d[1] in recorded) == want
        for n, m in mods.items():
            for attr in recorded:
                assert (getattr(m, attr) is getattr(tm, attr)) == (n in recorded[attr]), (n, attr)
        assert tm._csearch_originals == {"clustered_csearch": original, "_group_torsions_dbscan": original}
    finally:
        tscode_amd.uninstall(modules=mods)
    assert all(m.clustered_csearch is original and m._group_torsions_dbscan is original for m in mods.values())
    assert tm._csearch_originals == {}


def test_default_install_patches_nothing_new():
    import tscode_amd
    from tscode_amd.install import _PATCHES, _WHOLE_ENSEMBLE
    mods, original = _fake_modules()
    try:
        for kw in ({}, dict(per_item=True), dict(rot_corr=True, diverse=True, topology=True, nci=True)):
            assert tscode_amd.install(modules=mods, **kw) == []
            assert all(m.clustered_csearch is original and m._group_torsions_dbscan is original for m in mods.values())
    finally:
        tscode_amd.uninstall(modules=mods)
    assert not {"clustered_csearch", "_group_torsions_dbscan"} & (set(_PATCHES) | set(_WHOLE_ENSEMBLE))


# ------------------------------------------------------------------------------------------------------- GPU: the grouping kernel
def groups_dev(eng, coords, flat, set_off, max_size, min_torsions):
    """tsc_torsion_groups_dev on uploaded copies of the host form's arrays."""
    S, n = coords.shape[:2]
    held = [eng.dev_upload(np.ascontiguousarray(coords)), eng.dev_upload(np.ascontiguousarray(flat, dtype=np.int32)), eng.dev_alloc(max(len(flat), 1) * 4),
            eng.dev_alloc(S * 4), eng.dev_alloc(S * 4), eng.dev_alloc(S)]
    try:
        eng.torsion_groups_dev(held[0], S, n, held[1], set_off, max_size, min_torsions, *held[2:])
        return (eng.dev_download(held[2], np.empty(len(flat), np.int32)), eng.dev_download(held[3], np.empty(S, np.int32)),
                eng.dev_download(held[4], np.empty(S, np.int32)), eng.dev_download(held[5], np.empty(S, np.uint8)))
    finally:
        for a in held:
            eng.dev_free(a)


@pytest.mark.gpu
def test_torsion_groups_equal_the_reference():
    from tscode_amd.engine import get_engine
    eng = get_engine()
    g, meta = g26()
    for c in meta["part_a"]:
        k = c["index"]
        coords, quads = g[f"a{k}_coords"][None], g[f"a{k}_torsions"]
        set_off = np.array([0, len(quads)], np.int32)
        for min_torsions in (0, 9):
            if c["T"] >= 9 or min_torsions == 0:
                want = (g[f"a{k}_group_of"], c["n_groups"], c["eps_index"], c["oversize"])
            else:
                want = (np.zeros(c["T"], np.int32), 1, -1, 0)               # the caller's single group (:689)
            for got in (eng.torsion_groups(coords, quads, set_off, c["max_size"], min_torsions),
                        groups_dev(eng, coords, quads, set_off, c["max_size"], min_torsions)):
                assert np.array_equal(got[0], want[0]), c
                assert (int(got[1][0]), int(got[2][0]), int(got[3][0])) == want[1:], c


def sweep_structure(rng, n, T, max_size):
    """Coordinates of n atoms and T torsions whose centres are midpoints of atom pairs: a box whose density (drawn) decides the
    level, or a line 1.9 A apart that every level links.  Drawn again while a pair distance lies inside the guard band."""
    while True:
        quads = rng.integers(0, n, size=(T, 4)).astype(np.int32)
        design = rng.choice(["box", "box", "box", "line"]) if 2 * T <= n else "box"
        coords = rng.uniform(0.0, rng.choice([1.5, 4.0, 8.0, 14.0]) * T ** (1.0 / 3.0) + 4.0, size=(n, 3))
        if design == "line":                                               # torsion t owns atoms 2t and 2t + 1, its place on the line is drawn
            place = rng.permutation(T)
            quads[:, 1], quads[:, 2] = 2 * np.arange(T), 2 * np.arange(T) + 1
            coords[quads[:, 1]] = np.stack([1.9 * place, np.zeros(T), np.zeros(T)], axis=1) + rng.uniform(-0.01, 0.01, size=(T, 3))
            coords[quads[:, 2]] = coords[quads[:, 1]] + rng.uniform(-0.01, 0.01, size=(T, 3))
        want = yard_groups(coords, quads, max_size)
        if want[4] >= DIST_BAND:
            return coords, quads, want


@pytest.mark.gpu
@pytest.mark.parametrize("n_structs", (1, 3, 67))
def test_torsion_groups_sweep(n_structs):
    from tscode_amd.engine import get_engine
    eng = get_engine()
    rng = np.random.default_rng(2600 + n_structs)
    plans = [[T] for T in T_LIST] if n_structs == 1 else [list(rng.choice(T_LIST, size=n_structs)) for _ in range(2)]
    if n_structs == 3:
        plans.append([512, 1, 65])
    seen_levels, seen_over = set(), set()
    for p, plan in enumerate(plans):
        n = (512, 300, 131)[p % 3] if max(plan) <= 65 else 512
        max_size = (5, 3)[p % 2]
        parts = [sweep_structure(rng, n, int(T), max_size) for T in plan]
        coords = np.array([q[0] for q in parts])
        flat = np.concatenate([q[1] for q in parts])
        set_off = np.concatenate([[0], np.cumsum(plan)]).astype(np.int32)
        want_group = np.concatenate([q[2][0] for q in parts])
        want = [np.array([q[2][k] for q in parts]) for k in (1, 2, 3)]
        for got in (eng.torsion_groups(coords, flat, set_off, max_size, 9), groups_dev(eng, coords, flat, set_off, max_size, 9)):
            assert np.array_equal(got[0], want_group), (plan, np.flatnonzero(got[0] != want_group)[:5])
            for a, b, name in zip(got[1:], want, ("n_groups", "eps_index", "oversize")):
                assert np.array_equal(a, b), (name, plan, a, b)
        seen_levels |= set(want[1].tolist())
        seen_over |= set(want[2].tolist())
    if n_structs == 67:                                                     # (what the draws cover: unclustered, many levels, oversize or not)
        assert -1 in seen_levels and 16 in seen_levels and len(seen_levels) >= 6 and seen_over == {0, 1}


@pytest.mark.gpu
def test_torsion_groups_refusals():
    import ctypes as C

    from tscode_amd._lib import ptr
    from tscode_amd.engine import get_engine
    eng = get_engine()
    lib, h = eng.lib, eng._h
    n, S = 6, 2
    x = np.zeros((S, n, 3))
    tors = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5]], np.int32)
    set_off = np.array([0, 2, 3], np.int32)
    outs = dict(group_of=np.full(3, -7, np.int32), n_groups=np.full(S, -7, np.int32), eps_index=np.full(S, -7, np.int32), oversize=np.full(S, 7, np.uint8))

    def groups(fn=lib.tsc_torsion_groups, **kw):
        a = dict(coords=x, n_structs=S, n_atoms=n, torsions=tors, set_off=set_off, max_size=5, min_torsions=9, **outs)
        a.update(kw)
        return fn(h, ptr(a["coords"]), C.c_int(a["n_structs"]), C.c_int(a["n_atoms"]), ptr(a["torsions"]), ptr(a["set_off"]), C.c_int(a["max_size"]),
                  C.c_int(a["min_torsions"]), ptr(a["group_of"]), ptr(a["n_groups"]), ptr(a["eps_index"]), ptr(a["oversize"]))

    def t(row, k, v):
        out = tors.copy()
        out[row, k] = v
        return out
    many = np.zeros((513, 4), np.int32)
    refused = [dict(coords=None), dict(torsions=None), dict(set_off=None), dict(group_of=None), dict(n_groups=None), dict(eps_index=None),
               dict(oversize=None), dict(n_atoms=0), dict(n_atoms=513), dict(n_structs=-1), dict(max_size=0), dict(max_size=-3),
               dict(set_off=np.array([1, 2, 3], np.int32)), dict(set_off=np.array([0, 2, 1], np.int32)),
               dict(torsions=many, set_off=np.array([0, 513, 513], np.int32), group_of=np.full(513, -7, np.int32)),
               dict(torsions=t(0, 1, -1)), dict(torsions=t(2, 2, n)), dict(torsions=t(1, 0, n)), dict(torsions=t(1, 3, -2))]
    for kw in refused:
        assert groups(**kw) == TSC_ERR_INVALID, kw
    for kw in refused[:15]:                                                 # (the _dev form cannot look at the indices)
        assert groups(fn=lib.tsc_torsion_groups_dev, **kw) == TSC_ERR_INVALID, kw
    untouched = lambda: all((v == (7 if k == "oversize" else -7)).all() for k, v in outs.items())
    assert untouched()                                                      # nothing was launched: nothing was written
    for fn in (lib.tsc_torsion_groups, lib.tsc_torsion_groups_dev):
        assert groups(fn=fn, n_structs=0) == 0 and groups(fn=fn, set_off=np.array([0, 0, 0], np.int32)) == 0
    assert untouched()


# ------------------------------------------------------------------------------------------------------- GPU: the search
_batch = {}


def part_b_inputs():
    g, meta = g26()
    poses = np.array([g[f"b{p['index']}_coords"] for p in meta["part_b"]])
    init_rows = {(p["index"], c): g[f"b{p['index']}_init_rows{c}"] for p in meta["part_b"] for c in range(p["calls"])}
    return poses, g["b_atomnos"].astype(np.int64), init_rows


def batch_run():
    """clustered_csearch_batch on the three poses in one call with the recorded init rows: computed once, never changed."""
    if not _batch:
        import tscode_amd
        _, meta = g26()
        poses, atomnos, init_rows = part_b_inputs()
        info = {}
        out, start = tscode_amd.clustered_csearch_batch(poses, atomnos, n=meta["n"], n_out=meta["n_out"], init_rows=init_rows, info=info)
        _batch.update(out=out, start=start, info=info)
    return _batch["out"], _batch["start"], _batch["info"]


@pytest.mark.gpu
def test_clustered_csearch_batch_equals_the_reference():
    g, meta = g26()
    out, start, info = batch_run()
    assert not info["segmented"].any() and not info["oversize"].any()
    for p in meta["part_b"]:
        k = p["index"]
        assert np.array_equal(info["torsions"][k], g[f"b{k}_torsions"]) and np.array_equal(info["n_folds"][k], g[f"b{k}_n_folds"])
        group_of = np.zeros(len(g[f"b{k}_torsions"]), np.int32)
        for j, idx in enumerate(info["groups"][k]):
            group_of[idx] = j
        assert np.array_equal(group_of, g[f"b{k}_group_of"]) and len(info["groups"][k]) == p["n_groups"]
        assert [list(r) for r in info["round_sizes"][k]] == p["round_sizes"]
        mine, want = out[start == k], g[f"b{k}_out"]
        assert len(mine) == p["n_final"] == len(want)
        worst = float(np.abs(mine - want).max())
        print(f"pose {k}: {len(mine)} structures, largest coordinate difference {worst:.3e} A")
        assert worst <= COORD_TOL                                           # (row by row: the order is the reference's)
    assert np.array_equal(start, np.repeat(np.arange(3), [p["n_final"] for p in meta["part_b"]]))


@pytest.mark.gpu
def test_each_pose_alone_gives_the_rows_of_the_batch():
    import tscode_amd
    _, meta = g26()
    out, start, _ = batch_run()
    poses, atomnos, init_rows = part_b_inputs()
    for p in meta["part_b"]:
        k = p["index"]
        rows = {(0, c): init_rows[(k, c)] for c in range(p["calls"])}
        alone, s0 = tscode_amd.csearch_batch(poses[k], atomnos, mode=1, n=meta["n"], n_out=meta["n_out"], init_rows=rows)
        assert np.array_equal(alone, out[start == k]) and not s0.any()


@pytest.mark.gpu
def test_seeded_search_is_reproducible_however_the_ensemble_is_sliced(monkeypatch):
    import tscode_amd
    from tscode_amd import torsion_module as tm
    _, meta = g26()
    poses, atomnos, _ = part_b_inputs()
    kw = dict(n=meta["n"], n_out=meta["n_out"], seed=77)
    first = tscode_amd.clustered_csearch_batch(poses, atomnos, **kw)
    again = tscode_amd.clustered_csearch_batch(poses, atomnos, **kw)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and len(first[0]) > 3
    head, tail = tscode_amd.clustered_csearch_batch(poses[:1], atomnos, **kw), tscode_amd.clustered_csearch_batch(poses[1:], atomnos, **kw)
    assert np.array_equal(np.concatenate([head[0], tail[0]]), first[0])
    assert np.array_equal(np.concatenate([head[1], tail[1] + 1]), first[1])
    monkeypatch.setattr(tm, "MULTI_SCRATCH_BYTES", 200 * 40 * 24)           # a round no longer fits one call: one call per structure
    sliced = tscode_amd.clustered_csearch_batch(poses, atomnos, **kw)
    assert np.array_equal(sliced[0], first[0]) and np.array_equal(sliced[1], first[1])
    other = tscode_amd.clustered_csearch_batch(poses, atomnos, n=meta["n"], n_out=meta["n_out"], seed=78)
    assert other[0].shape[1:] == first[0].shape[1:]


def ethane(split):
    """C2H6, staggered; with ``split`` the second methyl 30 A away: two pieces and no N / O to bridge them."""
    x = [[0.0, 0.0, 0.765], [0.0, 0.0, -0.765]]
    for k in range(3):
        a = np.deg2rad(120.0 * k)
        x.append([1.02 * np.cos(a), 1.02 * np.sin(a), 0.765 + 0.39])
        x.append([1.02 * np.cos(a + np.pi / 3), 1.02 * np.sin(a + np.pi / 3), -0.765 - 0.39])
    x = np.array(x)
    if split:
        x[[1, 3, 5, 7]] += (0.0, 0.0, -30.0)
    return x


@pytest.mark.gpu
def test_segmented_pose_and_pose_without_torsions():
    import tscode_amd
    atomnos = np.array([6, 6, 1, 1, 1, 1, 1, 1])
    x = np.array([ethane(True), ethane(False), ethane(True)])
    for mode in (1, 2):
        info = {}
        kw = dict(info=info) if mode == 1 else {}
        out, start = tscode_amd.csearch_batch(x, atomnos, mode=mode, n=6, n_out=8, **kw)
        assert start.tolist() == [1] and np.array_equal(out, x[1:2])        # nothing for the pieces, the molecule itself (:619-621)
        if mode == 1:
            assert info["segmented"].tolist() == [True, False, True] and info["groups"] == [[], [], []]


@pytest.mark.gpu
def test_dropin_equals_the_batch():
    import networkx as nx

    from tscode_amd import torsion_module as tm
    g, meta = g26()
    out, start, info = batch_run()
    poses, atomnos, init_rows = part_b_inputs()
    k = meta["part_b"][1]["index"]
    torsions = [types.SimpleNamespace(torsion=tuple(int(i) for i in q), n_fold=int(f)) for q, f in zip(info["torsions"][k], info["n_folds"][k])]
    graph = nx.Graph()
    graph.add_nodes_from(range(len(atomnos)))
    graph.add_edges_from((i, i) for i in range(len(atomnos)))               # graphize's self loops
    graph.add_edges_from((int(a), int(b)) for a, b in g["b_bonds"])
    lines = []
    rows = {(0, c): init_rows[(k, c)] for c in range(meta["part_b"][1]["calls"])}
    got = tm.clustered_csearch(poses[k].copy(), atomnos, torsions, graph, constrained_indices=np.array([]), n=meta["n"], n_out=meta["n_out"],
                               mode=1, title="pose", logfunction=lines.append, interactive_print=False, init_rows=rows)
    assert np.array_equal(got, out[start == k])
    text = "\n".join(lines)
    assert str([len(idx) for idx in info["groups"][k]]) in text and f"{len(torsions)} torsions in {len(info['groups'][k])} groups" in text
    assert f"most diverse {len(got)} conformers" in text and f"kept the most diverse {meta['n']}" in text
    grouped = tm._group_torsions_dbscan(poses[k], torsions, max_size=5)
    assert [[torsions.index(t) for t in grp] for grp in grouped] == [idx.tolist() for idx in info["groups"][k]]
    with pytest.raises(RuntimeError, match="install"):
        tm.clustered_csearch(poses[k], atomnos, torsions, graph, mode=0, ff_opt=True)
