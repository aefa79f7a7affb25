"""Symmetry-corrected RMSD pruning (tscode_amd.rot_corr) against G19 (tests/golden/gen_rot_corr.py): the reference's own
prune_conformers_rmsd_rot_corr (tscode/torsion_module.py:953-1161), case by case."""

import json
import os
import sys
import types

import networkx as nx
import numpy as np
import pytest

from conftest import GOLDEN

_G19 = {}

# Torsion.get_angles (tscode/torsion_module.py:113-119): the angle table of each fold
FOLD_ANGLES = {2: (0, 180), 3: (0, 120, 240), 4: (0, 90, 180, 270), 6: (0, 60, 120, 180, 240, 300)}
SYMBOLS = {1: "H", 6: "C", 7: "N", 8: "O", 9: "F"}


def g19():
    if not _G19:
        a = np.load(os.path.join(GOLDEN, "G19a_rot_corr.npz"), allow_pickle=False)
        b = np.load(os.path.join(GOLDEN, "G19b_rot_corr.npz"), allow_pickle=False)
        _G19["meta"] = json.loads(a["meta_json"].tobytes().decode())
        _G19["data"] = {**{k: a[k] for k in a.files}, **{k: b[k] for k in b.files}}
    return _G19["meta"], _G19["data"]


def case(name):
    meta, data = g19()
    c = next(c for c in meta["cases"] if c["name"] == name)
    p = name + "_"
    mol = c["molecule"]
    structures = data[p + "structures"] if p + "structures" in data else data["n160a_structures"][data[p + "from_n160a"]]
    setup_from = name if p + "torsions" in data else ("n160a" if mol == "A" else None)
    setup = None
    if setup_from is not None:
        q = setup_from + "_"
        ptr_ = data[q + "sub_ptr"]
        setup = dict(torsions=data[q + "torsions"],
                     angles=[data[q + "angles"][t, :data[q + "n_angles"][t]] for t in range(len(data[q + "torsions"]))],
                     move_masks=data[q + "move_masks"],
                     sub_nodes=[data[q + "sub_idx"][ptr_[t]:ptr_[t + 1]] for t in range(len(ptr_) - 1)])
    return types.SimpleNamespace(meta=c, structures=structures, atomnos=data[f"mol{mol}_atomnos"], setup=setup,
                                 mask=data[p + "mask"], out=data.get(p + "out"), passes=data.get(p + "passes"), edges=data[p + "edges"],
                                 data=data, p=p)


def centred(structures):
    return np.array([s - s.mean(axis=0) for s in structures])


def graph_of(c):
    g = nx.Graph()
    g.add_nodes_from(range(len(c.atomnos)))
    g.add_edges_from(map(tuple, c.edges.tolist()))
    return g


def edge_set(g):
    return sorted(tuple(sorted(e)) for e in g.edges)


class _Torsion:
    """What _get_torsions hands back (tscode/torsion_module.py:40-119), rebuilt from G19's record."""

    def __init__(self, torsion, n_fold):
        self.i1, self.i2, self.i3, self.i4 = torsion
        self.torsion = tuple(torsion)
        self.n_fold = n_fold

    def get_angles(self):
        return FOLD_ANGLES[self.n_fold]


def fake_torsion_module(c):
    """A stand-in for a live tscode.torsion_module that serves the helper results G19 recorded for this case."""
    h = c.meta["helpers"]
    tm = types.ModuleType("tscode.torsion_module")
    hb_calls = iter(h["hydrogen_bonds"])
    tm._get_hydrogen_bonds = lambda coords, atomnos, graph, **kw: [tuple(p) for p in next(hb_calls)]
    tm.get_double_bonds_indices = lambda coords, atomnos: [tuple(p) for p in h["double_bonds"][0]]
    tm._get_torsions = lambda graph, hydrogen_bonds, double_bonds, keepdummy=False: [_Torsion(t, f) for t, f in h["torsions"]]
    nondummy = {(a, b): v for a, b, v in h["is_nondummy"]}
    tm._is_nondummy = lambda i, root, graph: nondummy[(int(i), int(root))]
    n = h["n_atoms"]

    def rotation_mask(graph, torsion):
        m = np.zeros(n, dtype=bool)
        m[h["rotation_masks"][json.dumps([int(i) for i in torsion])]] = True
        return m

    tm._get_rotation_mask = rotation_mask
    tm.pt = {z: types.SimpleNamespace(symbol=s) for z, s in SYMBOLS.items()}
    return tm


@pytest.fixture
def live_module(monkeypatch):
    def install(c):
        monkeypatch.setitem(sys.modules, "tscode.torsion_module", fake_torsion_module(c))
    return install


# ----------------------------------------------------------------------------------------------------------- CPU
def test_g19_loads():
    meta, data = g19()
    names = [c["name"] for c in meta["cases"]]
    assert names == ["n40", "n150", "n400", "n160a", "n760", "notors"]
    for name in names:
        c = case(name)
        assert c.structures.ndim == 3 and c.structures.shape[1:] == (len(c.atomnos), 3)
        assert len(c.mask) == len(c.structures) == c.meta["n"]
        if c.meta["n_torsions"]:
            assert c.out.shape == (int(c.mask.sum()),) + c.structures.shape[1:] and c.passes.shape == (18, 2)
    assert case("n760").mask.all() and case("notors").mask.all() and case("notors").meta["n_torsions"] == 0
    assert {case(n).meta["max_rmsd"] for n in names} == {0.25, 0.5}


@pytest.mark.parametrize("name", ["n40", "n150", "n400"])
def test_dropin_setup_from_live_module(name, live_module, monkeypatch):
    """The drop-in derives the reference's set-up (:1023-1049) from the live module's helpers and hands the caller's graph back
    unchanged."""
    import tscode_amd.rot_corr as rc
    c = case(name)
    live_module(c)
    seen = {}

    def arrays(structures, atomnos, torsions, angles, move_masks, sub_nodes, max_rmsd, max_structures, verbose):
        seen.update(torsions=torsions, angles=angles, masks=move_masks, subs=sub_nodes, max_rmsd=max_rmsd, max_structures=max_structures)
        return structures, np.ones(len(structures), dtype=bool)

    monkeypatch.setattr(rc, "prune_rmsd_rot_corr_arrays", arrays)
    g = graph_of(c)
    before = edge_set(g)
    lines = []
    rc.prune_conformers_rmsd_rot_corr(c.structures, c.atomnos, g, max_rmsd=c.meta["max_rmsd"], logfunction=lines.append)
    assert edge_set(g) == before
    s = c.setup
    assert [list(map(int, t)) for t in seen["torsions"]] == s["torsions"].tolist()
    assert [list(a) for a in seen["angles"]] == [list(a) for a in s["angles"]]
    assert np.array_equal(np.array(seen["masks"]), s["move_masks"])
    assert [list(x) for x in seen["subs"]] == [sorted(x.tolist()) for x in s["sub_nodes"]]
    assert seen["max_rmsd"] == c.meta["max_rmsd"] and seen["max_structures"] == 750
    assert lines[0] == "\n >> Dihedrals considered for subsymmetry corrections:" and len(lines) == len(s["torsions"]) + 2


def test_dropin_without_live_tscode(monkeypatch):
    import tscode_amd
    monkeypatch.delitem(sys.modules, "tscode.torsion_module", raising=False)
    c = case("n40")
    with pytest.raises(RuntimeError, match="prune_rmsd_rot_corr_arrays"):
        tscode_amd.prune_conformers_rmsd_rot_corr(c.structures, c.atomnos, graph_of(c))


def test_install_rot_corr_sites():
    """install(rot_corr=True) patches exactly the three binding sites; install() alone patches none of them."""
    import tscode_amd
    from tscode_amd.install import _PATCHES, _WHOLE_ENSEMBLE
    names = ("tscode.torsion_module", "tscode.embedder", "tscode.operators", "tscode.rmsd_pruning")
    original = object()
    mods = {}
    for n in names:
        m = types.ModuleType(n)
        m.prune_conformers_rmsd_rot_corr = original
        mods[n] = m
    try:
        assert tscode_amd.install(modules=mods) == []
        assert all(m.prune_conformers_rmsd_rot_corr is original for m in mods.values())
        done = tscode_amd.install(modules=mods, rot_corr=True)
        assert sorted(done) == sorted((n, "prune_conformers_rmsd_rot_corr") for n in names[:3])
        for n in names[:3]:
            assert mods[n].prune_conformers_rmsd_rot_corr is tscode_amd.prune_conformers_rmsd_rot_corr
        assert mods["tscode.rmsd_pruning"].prune_conformers_rmsd_rot_corr is original
    finally:
        tscode_amd.uninstall(modules=mods)
    assert all(m.prune_conformers_rmsd_rot_corr is original for m in mods.values())
    assert "prune_conformers_rmsd_rot_corr" not in _PATCHES and "prune_conformers_rmsd_rot_corr" not in _WHOLE_ENSEMBLE


def test_limits_refused_before_the_device():
    """Set-ups beyond the engine's limits are refused on the host (ValueError), never by a launch."""
    import tscode_amd
    c = case("n40")
    s = c.setup
    with pytest.raises(ValueError):
        tscode_amd.prune_rmsd_rot_corr_arrays(c.structures, c.atomnos, [s["torsions"][0]] * 17, [s["angles"][0]] * 17,
                                              [s["move_masks"][0]] * 17, [s["sub_nodes"][0]] * 17)
    with pytest.raises(ValueError):
        tscode_amd.prune_rmsd_rot_corr_arrays(c.structures, c.atomnos, s["torsions"][:1], [np.arange(7.0)], s["move_masks"][:1],
                                              s["sub_nodes"][:1])


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n40", "n150", "n400", "n160a"])
def test_arrays_match_reference(name):
    import tscode_amd
    c = case(name)
    kept, mask = tscode_amd.prune_rmsd_rot_corr_arrays(c.structures, c.atomnos, **c.setup, max_rmsd=c.meta["max_rmsd"])
    assert np.array_equal(mask, c.mask), (int(mask.sum()), int(c.mask.sum()))
    stats = tscode_amd.last_rot_corr_stats()
    assert [s["n_active"] for s in stats] == c.passes[:, 0].tolist()
    assert [s["pairs_evaluated"] for s in stats] == c.passes[:, 1].tolist()
    assert kept.shape == c.out.shape
    err = np.abs(kept - c.out).max()
    assert err < 1e-10, err


@pytest.mark.gpu
def test_early_returns():
    import tscode_amd
    for name, setup in (("n760", case("n760").setup), ("notors", dict(torsions=[], angles=[], move_masks=[], sub_nodes=[]))):
        c = case(name)
        kept, mask = tscode_amd.prune_rmsd_rot_corr_arrays(c.structures, c.atomnos, **setup, max_rmsd=c.meta["max_rmsd"])
        assert np.array_equal(mask, c.mask) and mask.all()
        assert kept.tobytes() == centred(c.structures).tobytes()


@pytest.mark.gpu
def test_pair_trace():
    """Every pair the reference evaluated in the N = 40 case, in its order, through the value-level form on the structures as
    the earlier pairs left them (the recorded best angles applied in place, rotate_dihedral's arithmetic)."""
    import tscode_amd
    from tscode_amd.algebra import rot_mat_from_pointer
    c = case("n40")
    s = c.setup
    pairs, best, rmsd = (c.data[c.p + k] for k in ("trace_pairs", "trace_best", "trace_rmsd"))
    state = centred(c.structures)
    got_r, got_b = [], []
    for (i, j), b in zip(pairs.tolist(), best):
        r, a = tscode_amd.rot_corr_pairs(state, c.atomnos, **s, pairs=[(i, j)])
        got_r.append(r[0])
        got_b.append(a[0])
        x = state[j]
        for t, ang in zip(s["torsions"], b):
            i2, i3 = int(t[1]), int(t[2])
            m = s["move_masks"][list(s["torsions"].tolist()).index(t.tolist())]
            R = rot_mat_from_pointer(x[i2] - x[i3], ang)
            x[m] = (R @ (x[m] - x[i3]).T).T + x[i3]
    assert np.array_equal(np.array(got_b), best)
    err = np.abs(np.array(got_r) - rmsd).max()
    assert err < 1e-9, err


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n40", "n150"])
def test_dropin_end_to_end(name, live_module):
    import tscode_amd
    c = case(name)
    live_module(c)
    g = graph_of(c)
    before = edge_set(g)
    kept, mask = tscode_amd.prune_conformers_rmsd_rot_corr(c.structures, c.atomnos, g, max_rmsd=c.meta["max_rmsd"])
    assert edge_set(g) == before
    assert np.array_equal(mask, c.mask)
    assert np.abs(kept - c.out).max() < 1e-10


def expected_mask_by_label(labels):
    """The schedule, the cache and the graph step of :1076-1152 with `similar` = same label."""
    from tscode_amd.numba_functions import _pass_schedule
    n = len(labels)
    cache = set()

    def first_similar(d, k, num_active):
        first = np.full(n, -1, dtype=np.int32)
        for step in range(k):
            lo, hi = d * step, (num_active if step == k - 1 else d * (step + 1))
            for i in range(lo, hi):
                for j in range(i + 1, hi):
                    if (i, j) in cache:
                        continue
                    if labels[i] == labels[j]:
                        first[i] = j
                        break
                    cache.add((i, j))
        return first

    return _pass_schedule(n, False, first_similar)


@pytest.mark.gpu
def test_uncapped_clustered_ensemble():
    """max_structures=None on 1 500 structures in 150 clusters of molecule A: members differ by exact symmetry turns of the CF3
    rotor plus <= 0.01 A of noise, clusters lie far apart (the reference's rot-corr RMSD on such an ensemble: <= 0.011 inside a
    cluster, >= 0.58 between the closest clusters) -- the mask is the schedule's with `similar` = same label.
    The CF3 torsion is the only one searched: a second torsion whose turns move the first one's local subgraph (molecule A's tBu
    bond turns the CH2-CF3 end) lets an evaluation against ANOTHER cluster leave a structure turned in a way its cluster-mates'
    CF3 search, run before that turn is undone, no longer recognises -- the reference's semantics, but no longer `same label`."""
    import tscode_amd
    from tscode_amd.synthetic import make_rot_corr_ensemble
    meta, data = g19()
    s = {k: v[:1] for k, v in case("n160a").setup.items()}         # the CF3 torsion alone (see below)
    S, labels = make_rot_corr_ensemble(data["molA_coords"], s["torsions"], s["angles"], s["move_masks"], 150, 10, seed=1500)
    kept, mask = tscode_amd.prune_rmsd_rot_corr_arrays(S, data["molA_atomnos"], **s, max_rmsd=0.25, max_structures=None)
    expected = expected_mask_by_label(labels)
    assert np.array_equal(mask, expected), (int(mask.sum()), int(expected.sum()))
