"""The batched non-covalent-interaction finder (tscode_amd.nci, csrc/nci.hpp) against G22 (tests/golden/gen_nci.py): the
reference's own get_nci, _get_aromatic_centers and is_phenyl.  The yardstick of the shapes G22 does not hold is the NumPy
restatement below, which takes nothing from the module under test and is itself pinned to G22 on the CPU.

Centres are compared at 1e-12 A absolute (six additions of |x| <= 100 round to below 1e-13); everything else exactly.

"Verdict family" here and in the generator: for each of the five interaction types, and for "the structure has a ring", the
verdict of a structure is whether it has one; an ensemble that can show a family at all shows it in 20 % to 80 % of its structures.
"""

import importlib
import json
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

GUARD = 1e-9
SYMBOLS = ("tsc_nci", "tsc_nci_dev", "tsc_nci_timings")
CASES = ("trimol", "bimol", "edges_a", "edges_b", "edges_c")
TYPES = ("HO", "HN", "FF", "HPh", "PhPh")
NCI = {"HO": (2.2, "O-H hydrogen bond"), "HN": (2.2, "N-H hydrogen bond"), "HPh": (2.8, "H-Ar non-conventional hydrogen bond"),
       "PhPh": (3.8, "pi-stacking interaction"), "FF": (3.5, "F-F interaction")}            # tscode/parameters.py:56-78, typed in again
SYM = {1: "H", 6: "C", 7: "N", 8: "O", 9: "F"}
SLOTS = 64
_G22 = {}


def g22(case):
    if not _G22:
        _G22["meta"] = json.load(open(os.path.join(GOLDEN, "G22_nci.json")))
        _G22["files"] = {}
    meta = _G22["meta"]["cases"][case]
    fn = meta["file"]
    if fn not in _G22["files"]:
        _G22["files"][fn] = np.load(os.path.join(GOLDEN, fn), allow_pickle=False)
    z = _G22["files"][fn]
    d = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}
    return types.SimpleNamespace(meta=meta, **d)


def split(flat, off):
    return [flat[off[s]:off[s + 1]] for s in range(len(off) - 1)]


# ------------------------------------------------------------------------------------------------------- the restatement
def dihedral(p):
    """tscode/algebra.py:24-56, restated."""
    b0 = -1.0 * (p[1] - p[0])
    b1 = p[2] - p[1]
    b2 = p[3] - p[2]
    b1 = b1 / np.sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2])
    v = b0 - np.dot(b0, b1) * b1
    w = b2 - np.dot(b2, b1) * b1
    return np.degrees(np.arctan2(np.dot(np.cross(b1, v), w), np.dot(v, w)))


_THR = {}


def pair_thresholds(atomnos):
    """f64[n, n]: the threshold of every pair of atoms by its elements (0: none)."""
    key = np.asarray(atomnos, dtype=np.int64).tobytes()
    if key not in _THR:
        sym = [SYM.get(int(z), "X") for z in atomnos]
        _THR[key] = np.array([[NCI.get("".join(sorted([a, b])), (0.0,))[0] for b in sym] for a in sym])
    return _THR[key]


def cliques6(near):
    """The 6-subsets of 0 .. k-1 that are cliques of the boolean matrix ``near``, in lexicographic order."""
    k = len(near)
    nb = [set(np.nonzero(near[a])[0].tolist()) for a in range(k)]
    out = []

    def grow(members, allowed):
        if len(members) == 6:
            out.append(tuple(members))
            return
        for v in sorted(allowed):
            grow(members + [v], {u for u in allowed if u > v and u in nb[v]})

    for a in range(k):
        grow([a], {u for u in nb[a] if u > a})
    return out


def restate_one(x, atomnos, ids, constrained, rule="reference"):
    """Sections 1 - 4 of the contract (include/tscode_hip.h) for one structure, in NumPy.  Returns a namespace: pairs [(i1, i2)],
    rings [(owner, atoms int[6], centre f64[3])] (all of them), ring_atom [(r, i)] and ring_ring [(r, s)] over the first 64 rings,
    margin (the smallest |distance - threshold| over every distance tested), flat_margin, flat_only (6-cliques that are not flat)."""
    n = len(atomnos)
    with np.errstate(invalid="ignore", divide="ignore"):
        sym = [SYM.get(int(z), "X") for z in atomnos]
        mol = np.repeat(np.arange(len(ids)), ids)
        d = x[:, None, :] - x[None, :, :]
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        thr = pair_thresholds(atomnos)
        free = ~np.isin(np.arange(n), np.asarray(constrained).ravel())
        tested = (mol[None, :] > mol[:, None]) & free[:, None] & free[None, :] & (thr > 0)
        margin = float(np.abs(dist - thr)[tested].min()) if tested.any() else np.inf
        pairs = [(int(a), int(b)) for a, b in zip(*np.nonzero(tested & (dist < thr)))]
        rings, flat_margin, flat_only = [], np.inf, 0
        bound = 1 - np.cos(10 * np.pi / 180)
        for m in range(len(ids)):
            cand = np.array([i for i in np.nonzero(mol == m)[0] if sym[i] in ("C", "N")], dtype=np.int64)
            if len(cand) <= 5:
                continue
            dc = dist[np.ix_(cand, cand)]
            margin = min(margin, float(np.abs(dc[np.triu_indices(len(cand), 1)] - 3).min()))
            for clique in cliques6(~(dc > 3)):
                atoms = cand[list(clique)]
                flat = 1 - np.abs(np.cos(dihedral(x[atoms[:4]]) * np.pi / 180))
                if not np.isnan(flat):
                    flat_margin = min(flat_margin, float(abs(flat - bound)))
                if flat < bound:
                    rings.append((m, atoms, np.mean(x[atoms], axis=0)))
                else:
                    flat_only += 1
        ring_atom, ring_ring = [], []
        hyd = np.nonzero(np.asarray(atomnos) == 1)[0]
        listed = rings[:SLOTS]
        for r, (owner, _, c) in enumerate(listed):
            v = c[None, :] - x[hyd]
            dh = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
            if len(hyd):
                margin = min(margin, float(np.abs(dh - NCI["HPh"][0]).min()))
            open_to = (mol[hyd] != owner) if rule == "intermolecular" else np.full(len(hyd), owner != 0)
            ring_atom += [(r, int(i)) for i in hyd[open_to & (dh < NCI["HPh"][0])]]
        for r in range(len(listed)):
            for s in range(r + 1, len(listed)):
                if listed[r][0] != listed[s][0]:
                    v = listed[r][2] - listed[s][2]
                    dr = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
                    margin = min(margin, float(abs(dr - NCI["PhPh"][0])))
                    if dr < NCI["PhPh"][0]:
                        ring_ring.append((r, s))
    return types.SimpleNamespace(pairs=pairs, rings=rings, ring_atom=ring_atom, ring_ring=ring_ring, margin=margin, flat_margin=flat_margin,
                                 flat_only=flat_only)


def constrained_rows(constrained, n_structs):
    if constrained is None:
        return [np.zeros(0, dtype=np.int64)] * n_structs
    c = np.asarray(constrained)
    return [c.ravel()] * n_structs if c.ndim == 1 else [c[s].ravel() for s in range(n_structs)]


_RESTATED = {}


def restate(key, structures, atomnos, ids, constrained, rule="reference"):
    """restate_one of every structure, computed once per (input, rule) and shared by the tests that need it."""
    if (key, rule) not in _RESTATED:
        rows = constrained_rows(constrained, len(structures))
        _RESTATED[(key, rule)] = [restate_one(structures[s], atomnos, ids, rows[s], rule) for s in range(len(structures))]
    return _RESTATED[(key, rule)]


def nci_tuples(r, atomnos):
    """get_nci's tuples from a restated structure."""
    sym = [SYM.get(int(z), "X") for z in atomnos]
    return ([(NCI["".join(sorted([sym[a], sym[b]]))][1], a, b) for a, b in r.pairs] + [(NCI["HPh"][1], i, "ring") for _, i in r.ring_atom] +
            [(NCI["PhPh"][1], "ring", "ring")] * len(r.ring_ring))


def expected_arrays(per, n):
    """The arrays of tsc_nci from restated structures, packed here bit by bit."""
    N, w = len(per), (n + 63) // 64
    e = types.SimpleNamespace(counts=np.zeros((N, 4), np.int32), overflow=np.zeros(N, bool), pair_bits=np.zeros((N, n, w), np.uint64),
                              ring_atoms=np.zeros((N, SLOTS, 6), np.uint16), ring_owner=np.zeros((N, SLOTS), np.uint8),
                              ring_center=np.zeros((N, SLOTS, 3)), ring_atom_bits=np.zeros((N, SLOTS, w), np.uint64),
                              ring_ring_bits=np.zeros((N, SLOTS), np.uint64))
    for s, r in enumerate(per):
        e.counts[s] = (len(r.pairs), len(r.rings), len(r.ring_atom), len(r.ring_ring))
        e.overflow[s] = len(r.rings) > SLOTS
        for a, b in r.pairs:
            e.pair_bits[s, a, b >> 6] |= np.uint64(1 << (b & 63))
        for k, (owner, atoms, c) in enumerate(r.rings[:SLOTS]):
            e.ring_atoms[s, k], e.ring_owner[s, k], e.ring_center[s, k] = atoms, owner, c
        for k, i in r.ring_atom:
            e.ring_atom_bits[s, k, i >> 6] |= np.uint64(1 << (i & 63))
        for k, j in r.ring_ring:
            e.ring_ring_bits[s, k] |= np.uint64(1 << j)
    return e


def assert_equal_arrays(res, e, want=None):
    assert (res["counts"] == e.counts).all(), (res["counts"][(res["counts"] != e.counts).any(1)][:4], e.counts[(res["counts"] != e.counts).any(1)][:4])
    assert (res["overflow"] == e.overflow).all()
    for name in ("pair_bits", "ring_atoms", "ring_owner", "ring_atom_bits", "ring_ring_bits") if want is None else want:
        if name == "ring_center":
            continue
        assert (res[name] == getattr(e, name)).all(), name
    if want is None or "ring_center" in want:
        assert np.abs(res["ring_center"] - e.ring_center).max() <= 1e-12


def family_shares(per, atomnos):
    sym = [SYM.get(int(z), "X") for z in atomnos]
    has = {t: [] for t in TYPES + ("ring",)}            # ("ring": judged only where an input shows none of the five types)
    for r in per:
        tags = {"".join(sorted([sym[a], sym[b]])) for a, b in r.pairs}
        for t in ("HO", "HN", "FF"):
            has[t].append(t in tags)
        has["HPh"].append(bool(r.ring_atom))
        has["PhPh"].append(bool(r.ring_ring))
        has["ring"].append(bool(r.rings))
    return {t: float(np.mean(v)) for t, v in has.items()}


# ------------------------------------------------------------------------------------------------------- sweep inputs
Z = 3.5
SWEEP_SIGMAS = (0.0, 0.05, 0.1, 0.15)            # (a ring of a later molecule reports its own hydrogens: half the structures keep theirs)


def unit(k, last):
    """Molecule k of a stack: a pyridine, a fluorine, an oxygen and two hydrogens that reach for the nitrogen and the oxygen of
    molecule k + 1 -- every contact at its threshold, so that moving the molecules as a whole opens and closes it."""
    z = k * Z
    mol = [("pyridine", (0, 0, z)), ("F", (0, -3.8, z - (0.05 if k % 2 else 0.0))), ("O", (0, 5, z))]
    if not last:
        mol += [("H", (1.39 + 2.2, 0, z + Z)), ("H", (0, 5 - 2.2, z + Z))]
    return mol


def fillers(count, row):
    """Oxygens far from everything (and 3 A from one another): atoms that only fill the structure up."""
    return [("O", (40.0 + 3.0 * (q % 12), 40.0 + 3.0 * (q // 12), 30.0 + 3.0 * row)) for q in range(count)]


def sweep_input(name):
    """(structures, atomnos, ids, constrained) of a sweep input, by name; deterministic."""
    from tscode_amd.synthetic import make_aromatic_ensemble as make
    kind, _, arg = name.partition(":")
    con = None
    if kind == "atoms":
        n = int(arg)
        if n == 6:
            mols, N = [[("hexagon", (0, 0, 0))]], 24
        else:
            # the two molecules of a stack in the middle of the structure, filled up at both ends; the first and the last atom
            # are an oxygen and a hydrogen at their threshold: row 0 against the last column
            fill = n - 15 - 13 - 2
            a = [("O", (20, 20, 20))] + fillers(fill // 2, 0) + unit(0, False)
            b = unit(1, True) + fillers(fill - fill // 2, 1) + [("H", (20, 20, 22.2))]
            mols, N = [a, b], 24
        out = make(mols, N, 3100 + n, SWEEP_SIGMAS, rigid=0.25)
    elif kind == "mols":
        m = int(arg)
        if m == 1:
            mols = [[("benzene", (0, 0, 0)), ("chair", (4.3, 0, 0))]]
        else:
            # the contacts lie between molecules 0 and 1; the others are bare rings far away, the last one with a fluorine that
            # reaches for molecule 0's
            mols = [unit(0, False), unit(1, True)] + [[("hexagon", (12.0 * (k - 1), 20, 0))] for k in range(2, m)]
            if m > 2:
                mols[-1].append(("F", (0, -3.8 - 3.6, 0)))
        out = make(mols, 24, 3200 + m, SWEEP_SIGMAS, rigid=0.25)
    elif kind == "cand":
        k = int(arg)
        ring = {5: [("pyranyl", (0, 0, Z))], 6: [("benzene", (0, 0, Z))], 7: [("benzene", (0, 0, Z)), ("C", (2.89, 0, Z))],
                64: [("hexagon", (5.5 * q, 0, Z)) for q in range(10)] + [("C", (5.5 * q + 2.75, 3.5, Z)) for q in range(4)],
                65: [("hexagon", (5.5 * q, 0, Z)) for q in range(10)] + [("C", (5.5 * q + 2.75, 3.5, Z)) for q in range(5)]}[k]
        out = make([unit(0, False), ring + [("F", (0, -3.8, Z)), ("O", (0, 5, Z))]], 24, 3300 + k, SWEEP_SIGMAS, rigid=0.25)
    elif kind == "con":
        out = make([unit(0, False), unit(1, True)], 24, 3410, SWEEP_SIGMAS, rigid=0.25)
        n = len(out[2])
        hot = [11, 12, 13, 14, 15, 26, 27]               # F, O, H, H of molecule 0; N, F, O of molecule 1
        rng = np.random.default_rng(3411)
        if arg == "shared":
            con = np.array([13, 26])
        elif arg == "per":
            con = np.full((24, 3), -1)
            for s in range(24):
                k = int(rng.integers(0, 6)) % 4                          # (0, 0, 1, 1, 2 or 3 atoms: rows of all -1 occur)
                con[s, :k] = rng.choice(hot, size=k, replace=False)
        elif arg == "16":
            con = np.array([12, 27] + [i for i in range(n) if i not in hot][:14])
    elif kind == "size":
        N = int(arg)
        out = list(make([unit(0, False), unit(1, True)], min(N, 250), 3500 + min(N, 250), SWEEP_SIGMAS, rigid=0.25))
        if N > 250:                                     # 250 distinct structures, repeated
            out[1] = np.ascontiguousarray(np.tile(out[1], (N // 250, 1, 1)))
    elif kind == "rings70":
        mols = [[("hexagon", (6.0 * q, 0, Z * m)) for q in range(10)] for m in range(7)]
        out = make(mols, 2, 3600, sigmas=(0.0,), rigid=0.0)
    else:
        raise KeyError(name)
    return out[1], out[2], out[3], con


SWEEPS = (["atoms:%d" % n for n in (6, 63, 64, 65, 129, 512)] + ["mols:%d" % m for m in (1, 2, 3, 8)] + ["cand:%d" % k for k in (5, 6, 7, 64)] +
          ["con:none", "con:shared", "con:per", "con:16"] + ["size:%d" % N for N in (1, 3, 4, 5, 10000)] + ["rings70"])
_INPUTS = {}


def sweep(name):
    if name not in _INPUTS:
        x, z, ids, con = sweep_input(name)
        distinct = x[:250] if name == "size:10000" else x
        per = restate(name, distinct, z, ids, None if con is None else (con if np.ndim(con) == 1 else con[:len(distinct)]))
        _INPUTS[name] = (x, z, ids, con, per)
    return _INPUTS[name]


# ------------------------------------------------------------------------------------------------------- CPU: the fixtures
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    g = g22(case)
    per = restate(case, g.structures, g.atomnos, g.ids, g.constrained)
    for s, r in enumerate(per):
        assert r.pairs == [tuple(p) for p in split(g.pairs, g.pair_off)[s].tolist()]
        lo, hi = g.ring_off[s], g.ring_off[s + 1]
        assert [q[0] for q in r.rings] == g.ring_owner[lo:hi].tolist()
        assert [q[1].tolist() for q in r.rings] == g.ring_atoms[lo:hi].tolist()
        assert hi == lo or np.abs(np.array([q[2] for q in r.rings]) - g.ring_center[lo:hi]).max() <= 1e-12
        assert r.ring_atom == [tuple(p) for p in split(g.ring_atom, g.ring_atom_off)[s].tolist()]
        assert r.ring_ring == [tuple(p) for p in split(g.ring_ring, g.ring_ring_off)[s].tolist()]
        assert len(nci_tuples(r, g.atomnos)) == len(g.meta["print_lists"][s])


@pytest.mark.parametrize("case", CASES)
def test_fixture_conditions(case):
    """What the generator asserts, asserted again on the files."""
    g = g22(case)
    per = restate(case, g.structures, g.atomnos, g.ids, g.constrained)
    assert min(r.margin for r in per) > GUARD and min(r.flat_margin for r in per) > GUARD
    assert os.path.getsize(os.path.join(GOLDEN, g.meta["file"])) < 700000
    shares = family_shares(per, g.atomnos)
    if case in ("trimol", "bimol"):
        for t in TYPES:
            assert 0.2 <= shares[t] <= 0.8, (case, t, shares[t])
        assert len({len(r.rings) for r in per}) >= 3
        assert sum(r.flat_only for r in per) > 0
        assert set(np.unique(g.sigma).tolist()) == {0.0, 0.03, 0.08, 0.15}
    if case == "trimol":
        assert len(g.ids) == 3 and 40 <= len(g.atomnos) <= 50 and (g.constrained >= 0).any() and (g.constrained == -1).all(1).any()
        assert max(int(np.isin(g.atomnos[lo:hi], (6, 7)).sum()) for lo, hi in zip(np.cumsum(g.ids) - g.ids, np.cumsum(g.ids))) == 12
    if case == "edges_a":
        cands = [int(np.isin(g.atomnos[lo:hi], (6, 7)).sum()) for lo, hi in zip(np.cumsum(g.ids) - g.ids, np.cumsum(g.ids))]
        assert cands == [5, 6, 10] and all(q[0] != 0 for r in per for q in r.rings)
        assert any(sum(q[0] == 2 for q in r.rings) >= 2 for r in per) and any(q[0] == 1 for r in per for q in r.rings)
    if case == "edges_b":
        rod = list(range(12, 18))
        assert all(q[0] == 0 for r in per for q in r.rings) and not any(r.ring_atom for r in per)
        assert any(q[1].tolist() == rod for r, sg in zip(per, g.sigma) if sg == 0 for q in r.rings)          # atan2(0, 0) = 0 counts as flat
        other = restate(case, g.structures, g.atomnos, g.ids, g.constrained, "intermolecular")
        assert any(r.ring_atom for r in other), "the hydrogens of molecule 1 are inside the rings' 2.8 A"
    if case == "edges_c":
        assert (g.constrained[:, 0] == 0).all() and np.mean([any(i == 0 for _, i in r.ring_atom) for r in per]) >= 0.2
        assert not any(0 in p for r in per for p in r.pairs)
        free = [restate_one(x, g.atomnos, g.ids, []) for x in g.structures]
        assert any(0 in p for r in free for p in r.pairs), "without the constraint the hydrogen pairs with the oxygen"


def test_threshold_table_equals_the_recorded_nci_dict():
    from tscode_amd.nci import NCI_DICT, nci_tables
    recorded = {k: (v[0], v[1]) for k, v in json.load(open(os.path.join(GOLDEN, "G22_nci.json")))["nci_dict"].items()}
    assert NCI_DICT == recorded == NCI
    classes, thr, ring_thr, cand = nci_tables(np.array([1, 6, 7, 8, 9, 16]))
    assert classes.tolist() == [1, 0, 2, 3, 4, 0] and cand.tolist() == [0, 1, 1, 0, 0, 0]
    want = np.zeros((5, 5))
    want[1, 3] = want[3, 1] = want[1, 2] = want[2, 1] = 2.2
    want[4, 4] = 3.5
    assert (thr == want).all() and ring_thr.tolist() == [0, 2.8, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------- CPU: ABI, install, refusals
def test_header_and_prototype_table_declare_the_entry_points():
    import tscode_amd
    from tscode_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tscode_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"{s} not declared in include/tscode_hip.h"
        assert s in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["tsc_nci"] == _lib._SIGNATURES["tsc_nci_dev"]
    assert "nci.hip" in build.SOURCES and "nci.hpp" in build.HEADERS
    for name in ("get_nci", "nci_batch", "differential_nci"):
        assert callable(getattr(tscode_amd, name))
    assert callable(tscode_amd.Engine.nci) and callable(tscode_amd.Engine.nci_dev)


def test_nci_patch_table_equals_the_recorded_sites():
    inst = importlib.import_module("tscode_amd.install")
    g = json.load(open(os.path.join(GOLDEN, "G22_nci_sites.json")))
    assert not g["modules_not_importable_here"] and len(g["modules_imported"]) >= 25
    assert {k: sorted(v[1]) for k, v in inst._NCI_PATCHES.items()} == {k: v["bound_in"] for k, v in g["sites"].items()}
    assert all(v["defined_in"] in v["bound_in"] for v in g["sites"].values())
    others = set(inst._PATCHES) | set(inst._ROT_CORR_PATCHES) | set(inst._DIVERSE_PATCHES) | set(inst._TOPOLOGY_PATCHES)
    assert not set(inst._NCI_PATCHES) & others and inst._NCI_PATCHES in inst._OPT_IN


def test_install_nci_is_opt_in_and_uninstall_restores():
    import tscode_amd
    inst = importlib.import_module("tscode_amd.install")
    fake, originals = {}, {}
    for name in inst._NCI_PATCHES["get_nci"][1]:
        fake[name] = types.ModuleType(name)
        originals[name] = (lambda *a, _k=name, **kw: _k)
        fake[name].get_nci = originals[name]
    try:
        done = tscode_amd.install(modules=fake, per_item=True, rot_corr=True, diverse=True, topology=True)
        assert not [d for d in done if d[1] == "get_nci"], "install() without nci=True must not patch get_nci"
        assert all(fake[n].get_nci is fn for n, fn in originals.items())
        done = tscode_amd.install(modules=fake, nci=True)
        assert sorted(d for d in done if d[1] == "get_nci") == sorted((n, "get_nci") for n in originals)
        assert all(fake[n].get_nci is tscode_amd.get_nci for n in originals)
    finally:
        tscode_amd.uninstall(modules=fake)
    assert all(fake[n].get_nci is fn for n, fn in originals.items())


def test_refusals_raise_value_error_before_the_library_is_loaded():
    import tscode_amd as ta
    z = np.array([6, 6, 8, 1])
    x = np.zeros((2, 4, 3)) + np.arange(4)[None, :, None]
    ids = np.array([2, 2])
    from tscode_amd.nci import check_nci_args
    check_nci_args(x, z, np.array([[0, -1], [-1, -1]]), ids, "intermolecular", ("pair_bits",))          # (a valid call)
    bad = x.copy()
    bad[1, 2, 0] = np.inf
    x65, z65, ids65, _ = sweep_input("cand:65")
    refusals = [
        lambda: ta.nci_batch(bad, z, None, ids),                                          # non-finite coordinates
        lambda: ta.nci_batch(x[:, :3], z, None, ids),                                     # shape mismatch
        lambda: ta.nci_batch(np.zeros((2, 4, 2)), z, None, ids),
        lambda: ta.nci_batch(np.zeros((1, 513, 3)), np.full(513, 8), None, [513]),        # n_atoms > 512
        lambda: ta.nci_batch(np.zeros((1, 0, 3)), np.zeros(0, int), None, [0]),           # n_atoms < 1
        lambda: ta.nci_batch(x, z.astype(float), None, ids),                              # atomic numbers that are no integers
        lambda: ta.nci_batch(x, z, None, [2, 1]),                                         # ids do not add up
        lambda: ta.nci_batch(x, z, None, [4, 0]),                                         # an empty molecule
        lambda: ta.nci_batch(x, z, None, []),                                             # no molecule
        lambda: ta.nci_batch(np.zeros((1, 9, 3)), np.full(9, 8), None, [1] * 9),          # 9 molecules
        lambda: ta.nci_batch(x65, z65, None, ids65),                                      # 65 candidates in a molecule
        lambda: ta.nci_batch(x, z, np.arange(17) % 4, ids),                               # 17 constrained atoms
        lambda: ta.nci_batch(x, z, np.array([4]), ids),                                   # constrained index >= n_atoms
        lambda: ta.nci_batch(x, z, np.array([-2]), ids),                                  # constrained index < -1
        lambda: ta.nci_batch(x, z, np.zeros((3, 2), int), ids),                           # rows != structures
        lambda: ta.nci_batch(x, z, np.array([0.5]), ids),                                 # constrained indices that are no integers
        lambda: ta.nci_batch(x, z, None, ids, owner_rule="mine"),                         # an unknown owner rule
        lambda: ta.nci_batch(x, z, None, ids, want=("pairs",)),                           # an unknown output
        lambda: ta.get_nci(bad[1], z, np.array([]), ids),
        lambda: ta.differential_nci({"counts": np.zeros((1, 4), np.int32)}),              # a counts-only result
    ]
    for k, call in enumerate(refusals):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} did not raise")


def test_c_abi_refuses_every_limit_before_any_launch():
    """tsc_nci with zero structures: the arguments are checked, nothing is launched and the context is not touched (a block of
    zeroed memory stands in for it), so the refusals of include/tscode_hip.h can be asked for without a GPU."""
    import ctypes as C
    from tscode_amd import _lib
    from tscode_amd.build import build
    build()
    lib = _lib.load()
    ctx = C.create_string_buffer(4096)
    n = 130
    base = dict(n=n, cls=np.zeros(n, np.uint8), thr=np.ones((2, 2)), T=2, mol=np.repeat([0, 1], 65).astype(np.uint8), M=2,
                cand=(np.arange(n) % 65 < 64).astype(np.uint8), rthr=np.ones(2), rr=3.8, con=np.array([0, -1, n - 1], np.int32), E=3, per=0, rule=0)

    def call(**kw):
        a = dict(base, **kw)
        counts, overflow = np.zeros((1, 4), np.int32), np.zeros(1, np.uint8)
        return lib.tsc_nci(C.cast(ctx, C.c_void_p), _lib.ptr(np.zeros((1, a["n"], 3))), 0, a["n"], _lib.ptr(a["cls"]), _lib.ptr(a["thr"]), a["T"],
                           _lib.ptr(a["mol"]), a["M"], _lib.ptr(a["cand"]), _lib.ptr(a["rthr"]), a["rr"], _lib.ptr(a["con"]), a["E"], a["per"],
                           a["rule"], _lib.ptr(counts), _lib.ptr(overflow), *[None] * 8)

    assert call() == 0, lib.tsc_last_error()                                               # 64 candidates in each molecule
    refused = [dict(n=0), dict(n=513), dict(T=0), dict(T=9, thr=np.ones((9, 9)), rthr=np.ones(9)), dict(M=0), dict(M=9), dict(E=17), dict(E=-1),
               dict(rule=2), dict(cls=np.full(n, 2, np.uint8)), dict(cand=np.ones(n, np.uint8)),                       # 65 candidates
               dict(mol=np.repeat([1, 0], 65).astype(np.uint8)), dict(mol=np.repeat([0, 2], 65).astype(np.uint8)), dict(M=3),
               dict(thr=np.array([[1.0, -1.0], [1.0, 1.0]])), dict(thr=np.array([[1.0, np.nan], [1.0, 1.0]])), dict(rthr=np.array([np.inf, 1.0])),
               dict(rr=-1.0), dict(con=np.array([n, 0, 0], np.int32)), dict(con=np.array([-2, 0, 0], np.int32))]
    for kw in refused:
        assert call(**kw) == -1, (sorted(kw), lib.tsc_last_error())                        # TSC_ERR_INVALID
        assert lib.tsc_last_error()


def test_sweep_inputs_keep_their_margins_and_shares():
    """Every sweep input below, regenerated and judged by the restatement alone: no distance within 1e-9 A of its threshold, no
    flatness value within 1e-9 of its bound, and every verdict family that the input shows at all shows in 20 % to 80 % of its
    structures (ensembles of 20 structures and more)."""
    shown = set()
    for name in SWEEPS:
        x, z, ids, con, per = sweep(name)
        assert min(r.margin for r in per) > GUARD and min(r.flat_margin for r in per) > GUARD, name
        shares = family_shares(per, z)
        shown |= {t for t, v in shares.items() if v > 0}
        if any(shares[t] > 0 for t in TYPES):
            del shares["ring"]
        if len(per) >= 20:
            assert any(v > 0 for v in shares.values()), name
            for t, v in shares.items():
                assert v == 0 or 0.2 <= v <= 0.8, (name, t, v)
    assert shown == set(TYPES) | {"ring"}
    n = {name: sweep(name)[0].shape[1] for name in SWEEPS if name.startswith("atoms")}
    assert n == {"atoms:%d" % k: k for k in (6, 63, 64, 65, 129, 512)}
    assert [len(sweep("mols:%d" % m)[2]) for m in (1, 2, 3, 8)] == [1, 2, 3, 8]
    for k in (5, 6, 7, 64):
        x, z, ids, _, _ = sweep("cand:%d" % k)
        assert int(np.isin(z[ids[0]:], (6, 7)).sum()) == k
    per70 = sweep("rings70")[4]
    assert sweep("rings70")[0].shape[1] == 420 and all(len(r.rings) == 70 and r.ring_ring for r in per70)
    assert any(p[0] == 0 and p[1] == 511 for r in sweep("atoms:512")[4] for p in r.pairs), "row 0 never meets the last column"


# ------------------------------------------------------------------------------------------------------- GPU
def batch(x, z, con, ids, **kw):
    import tscode_amd
    return tscode_amd.nci_batch(x, z, con, ids, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["reference", "intermolecular"])
@pytest.mark.parametrize("case", CASES)
def test_g22_through_nci_batch(case, rule):
    """Every G22 case under both owner rules: the reference's recorded lists (rule "reference") and the restatement."""
    g = g22(case)
    per = restate(case, g.structures, g.atomnos, g.ids, g.constrained, rule)
    res = batch(g.structures, g.atomnos, g.constrained, g.ids, owner_rule=rule)
    assert_equal_arrays(res, expected_arrays(per, len(g.atomnos)))
    if rule == "reference":
        assert (res["counts"][:, 0] == np.diff(g.pair_off)).all() and (res["counts"][:, 1] == np.diff(g.ring_off)).all()
        assert (res["counts"][:, 2] == np.diff(g.ring_atom_off)).all() and (res["counts"][:, 3] == np.diff(g.ring_ring_off)).all()
        for s in range(len(g.structures)):
            k = int(res["counts"][s, 1])
            assert (res["ring_atoms"][s, :k] == g.ring_atoms[g.ring_off[s]:g.ring_off[s + 1]]).all()
            assert k == 0 or np.abs(res["ring_center"][s, :k] - g.ring_center[g.ring_off[s]:g.ring_off[s + 1]]).max() <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_drop_in_returns_the_recorded_tuples_and_strings(case):
    import tscode_amd
    g = g22(case)
    per = restate(case, g.structures, g.atomnos, g.ids, g.constrained)
    for s in range(len(g.structures)):
        nci, print_list = tscode_amd.get_nci(g.structures[s], g.atomnos, g.constrained[s].reshape(-1, 2), g.ids)
        assert nci == nci_tuples(per[s], g.atomnos)
        assert print_list == g.meta["print_lists"][s]


@pytest.mark.gpu
def test_differential_nci_on_trimol():
    import tscode_amd
    g = g22("trimol")
    per = restate("trimol", g.structures, g.atomnos, g.ids, g.constrained)
    lists = [nci_tuples(r, g.atomnos) for r in per]
    expect = []
    for lst in lists:                                                                    # tscode/embedder.py:2076-2096
        for nci in lst:
            if nci not in [e[0] for e in expect] and not all(nci in other for other in lists):
                expect.append((nci, [j for j, other in enumerate(lists) if nci in other]))
    res = batch(g.structures, g.atomnos, g.constrained, g.ids)
    assert [tscode_amd.interactions_of(res, s) for s in range(len(lists))] == lists
    got = tscode_amd.differential_nci(res)
    assert got == expect and len(expect) >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s for s in SWEEPS if s != "rings70"])
def test_sweeps_equal_the_restatement(name):
    """Atom counts 6 .. 512, 1 .. 8 molecules, 5 .. 64 candidates, every form of the constrained list, ensembles of 1 .. 10 000."""
    x, z, ids, con, per = sweep(name)
    res = batch(x, z, con, ids)
    if name == "size:10000":
        per = per * (len(x) // len(per))
    assert_equal_arrays(res, expected_arrays(per, len(z)))


@pytest.mark.gpu
def test_seventy_rings_overflow_the_list_and_keep_the_count():
    x, z, ids, con, per = sweep("rings70")
    res = batch(x, z, con, ids)
    assert res["overflow"].all() and (res["counts"][:, 1] == 70).all()
    assert_equal_arrays(res, expected_arrays(per, len(z)))
    import tscode_amd
    with pytest.raises(ValueError):
        tscode_amd.get_nci(x[0], z, np.array([]), ids)


@pytest.mark.gpu
def test_counts_only_equals_the_popcounts_of_the_full_output():
    g = g22("trimol")
    full = batch(g.structures, g.atomnos, g.constrained, g.ids)
    lean = batch(g.structures, g.atomnos, g.constrained, g.ids, want=())
    assert set(lean) == {"counts", "overflow", "atomnos", "ids", "owner_rule"}
    assert (lean["counts"] == full["counts"]).all() and (lean["overflow"] == full["overflow"]).all()

    def pop(a):
        return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1), axis=1).sum(1)

    assert (pop(full["pair_bits"]) == lean["counts"][:, 0]).all() and (pop(full["ring_atom_bits"]) == lean["counts"][:, 2]).all()
    assert (pop(full["ring_ring_bits"]) == lean["counts"][:, 3]).all()
    assert ((full["ring_atoms"].astype(int).sum(2) > 0).sum(1) == lean["counts"][:, 1]).all()
    assert lean["counts"][:, 0].any() and lean["counts"][:, 2].any() and lean["counts"][:, 3].any()


@pytest.mark.gpu
def test_device_entry_equals_the_host_entry():
    """tsc_nci_dev on torch buffers against tsc_nci on the same arrays, per-structure constrained atoms included; and zero
    structures succeed and write nothing."""
    import torch
    import tscode_amd
    from tscode_amd.nci import NCI_DICT, check_nci_args, nci_tables
    g = g22("trimol")
    x, z, ids, atom_mol, con, rule, _ = check_nci_args(g.structures, g.atomnos, g.constrained, g.ids)
    classes, thr, ring_thr, cand = nci_tables(z)
    eng = tscode_amd.get_engine()
    host = eng.nci(x, classes, thr, atom_mol, len(ids), cand, ring_thr, NCI_DICT["PhPh"][0], con, rule, tscode_amd.nci.WANT_ALL)
    N, n = x.shape[:2]
    w = (n + 63) // 64
    dev = torch.device("cuda", eng.device)
    shapes = {"counts": ((N, 4), torch.int32), "overflow": ((N,), torch.uint8), "pair_bits": ((N, n, w), torch.int64),
              "ring_atoms": ((N, 64, 6), torch.int16), "ring_owner": ((N, 64), torch.uint8), "ring_center": ((N, 64, 3), torch.float64),
              "ring_atom_bits": ((N, 64, w), torch.int64), "ring_ring_bits": ((N, 64), torch.int64)}
    out = {k: torch.full(s, 7, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    d_x, d_con = torch.from_numpy(x).to(dev), torch.from_numpy(con).to(dev)
    torch.cuda.synchronize()
    eng.nci_dev(d_x, 0, n, classes, thr, atom_mol, len(ids), cand, ring_thr, NCI_DICT["PhPh"][0], d_con, True, rule, *out.values())
    eng.synchronize()
    assert all((v.cpu() == 7).all() for v in out.values()), "zero structures wrote something"
    eng.nci_dev(d_x, N, n, classes, thr, atom_mol, len(ids), cand, ring_thr, NCI_DICT["PhPh"][0], d_con, True, rule, *out.values())
    eng.synchronize()
    for k, v in out.items():
        got = v.cpu().numpy()
        assert (got.view(host[k].dtype if k != "overflow" else np.uint8) == host[k]).all(), k
    empty = eng.nci(np.zeros((0, n, 3)), classes, thr, atom_mol, len(ids), cand, ring_thr, 3.8, None, 0, ("pair_bits",))
    assert empty["counts"].shape == (0, 4) and empty["pair_bits"].shape == (0, n, w)


@pytest.mark.gpu
def test_kernel_time_is_taken_only_under_pass_timing_and_per_thread():
    """tsc_nci_timings on 3 structures of the smallest fixture molecule: -1 without the option, a positive time with it through both
    entries, -1 after zero structures, -1 again once the option is off, -1 in a thread that never called."""
    import math
    import threading
    import torch
    import tscode_amd
    from tscode_amd.nci import NCI_DICT, check_nci_args, nci_tables
    g = g22(min(CASES, key=lambda case: len(g22(case).atomnos)))
    x, z, ids, atom_mol, con, rule, _ = check_nci_args(g.structures[:3], g.atomnos, g.constrained[:3], g.ids)
    classes, thr, ring_thr, cand = nci_tables(z)
    eng = tscode_amd.get_engine()
    N, n = x.shape[:2]
    assert N == 3
    dev = torch.device("cuda", eng.device)
    counts = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    overflow = torch.zeros((N,), dtype=torch.uint8, device=dev)
    d_x, d_con = torch.from_numpy(x).to(dev), torch.from_numpy(con).to(dev)
    torch.cuda.synchronize()

    def host(rows=N):
        return eng.nci(x[:rows], classes, thr, atom_mol, len(ids), cand, ring_thr, NCI_DICT["PhPh"][0], con[:rows], rule, ())

    def device():
        eng.nci_dev(d_x, N, n, classes, thr, atom_mol, len(ids), cand, ring_thr, NCI_DICT["PhPh"][0], d_con, True, rule, counts, overflow)
        eng.synchronize()

    def in_a_fresh_thread():
        got = []
        t = threading.Thread(target=lambda: got.append(eng.nci_kernel_ms()))
        t.start()
        t.join()
        return got[0]

    with eng.options(pass_timing=0):
        want = host()
        assert eng.nci_kernel_ms() == -1.0
        device()
        assert eng.nci_kernel_ms() == -1.0
        with eng.options(pass_timing=1):
            timed = host()
            assert math.isfinite(eng.nci_kernel_ms()) and eng.nci_kernel_ms() > 0.0
            assert (timed["counts"] == want["counts"]).all()
            assert in_a_fresh_thread() == -1.0
            device()
            assert math.isfinite(eng.nci_kernel_ms()) and eng.nci_kernel_ms() > 0.0
            assert (counts.cpu().numpy() == want["counts"]).all()
            host(0)
            assert eng.nci_kernel_ms() == -1.0
            host()
            assert eng.nci_kernel_ms() > 0.0
        host()
        assert eng.nci_kernel_ms() == -1.0
