"""Reactive-atom orbitals and pivots per conformer (tscode_amd.reactive_atoms, csrc/orbitals.hpp) against G23
(tests/golden/gen_orbitals.py): the reference's own compute_orbitals, reactive-atom classes and Embedder._set_pivots.  The yardstick of
the shapes G23 does not hold is the NumPy restatement below, which takes nothing from the module under test and is itself pinned to G23
on the CPU.

Coordinates (centres, orbital vectors, pivots, mean points) are compared at VAL_TOL = 1e-9 A, the project's tolerance for
reference-recorded coordinates; kinds, lobe counts, sigmatropic flags, pivot counts and lobe indices exactly.  The guards keep the
discrete outputs exact: no angle within 1e-6 degrees of 175, no reactive-pair distance within 1e-9 A of 3 A, a gap of at least 1e-6 A
between the 2nd and 3rd shortest of four pivots, no pivot length between 1e-6 and 1e-4 A above the shortest, and every vector that is
normalised at least 1e-3 of the product of its operands' lengths: that bounds the amplification of rounding differences at 1e3 times a
few hundred ulp of |x| <= 20 A, about 1e-11 A.
"""

import json
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

VAL_TOL = 1e-9
SYMBOLS = ("tsc_orbitals", "tsc_orbitals_dev", "tsc_orbitals_timings")
CASES = ("ch3cl_ch", "ch3cl_c", "ch3cl_cl", "hcooh_co", "hcooh_oh", "c2h4", "allene", "acetonitrile", "diimine", "ketene", "alkoxide", "enolate",
         "propenal", "propenal50")
GUARD_ANGLE, GUARD_DIST, GUARD_GAP, GUARD_BAND, GUARD_COND = 1e-6, 1e-9, 1e-6, (1e-6, 1e-4), 1e-3
SYM = {1: "H", 3: "Li", 6: "C", 7: "N", 8: "O", 17: "Cl"}
# tscode/parameters.py:19-53, typed in again
ORB_DIM = {"H Single Bond": 0.85, "C Single Bond": 1, "O Single Bond": 1, "N Single Bond": 1, "F Single Bond": 1, "Cl Single Bond": 1.5,
           "Br Single Bond": 1.5, "I Single Bond": 2, "C sp": 1, "N sp": 1, "B sp2": 0.8, "C sp2": 1.1, "N sp2": 1, "B sp3": 1, "C sp3": 1,
           "Br sp3": 1, "O Ether": 1, "S Ether": 1, "O Ketone": 0.85, "S Ketone": 1, "N Imine": 1, "C bent carbene": 1, "Metal": 2.5, "Fallback": 1}
# tscode/reactive_atoms_classes.py:579-643, the entries the fixtures' elements can reach
TYPE_OF = {"H1": "Single", "C1": "Single", "C2": "Sp_or_carbene", "C3": "Sp2", "C4": "Sp3", "N1": "Single", "N2": "Imine", "N3": "Sp2", "N4": "Sp3",
           "O1": "Ketone", "O2": "Ether", "Cl1": "Single", **{"Li%d" % b: "Metal" for b in range(1, 9)}}
NAME_OF = {"Single": "Single Bond", "Sp2": "sp2", "Sp3": "sp3", "Ether": "Ether", "Ketone": "Ketone", "Imine": "Imine", "Metal": "Metal"}
KINDS = ("Single Bond", "sp2", "sp3", "Ether", "Ketone (p+p)", "Ketone (sp2)", "Ketone (p)", "Ketone (trilobe)", "Imine", "sp", "bent carbene", "Metal")
_G23 = {}


def g23(case):
    if not _G23:
        _G23["meta"] = json.load(open(os.path.join(GOLDEN, "G23_orbitals.json")))
        _G23["files"] = {}
    meta = _G23["meta"]["cases"][case]
    fn = meta["file"]
    if fn not in _G23["files"]:
        _G23["files"][fn] = np.load(os.path.join(GOLDEN, fn), allow_pickle=False)
    z = _G23["files"][fn]
    d = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}
    return types.SimpleNamespace(meta=meta, **d)


# ------------------------------------------------------------------------------------------------------- the restatement
class Margins:
    """The smallest distance of every decision of a conformer from its threshold, and the worst conditioning of a normalisation."""

    def __init__(self):
        self.angle = self.dist = self.gap = self.cond = np.inf
        self.band = False

    def ok(self):
        return self.angle > GUARD_ANGLE and self.dist > GUARD_DIST and self.gap >= GUARD_GAP and not self.band and self.cond >= GUARD_COND


def length(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def unit(v, m=None, scale=1.0):
    """v / |v|; ``scale`` = the product of the lengths of the operands v was formed from."""
    n = length(v)
    if m is not None:
        m.cond = min(m.cond, n / scale if scale > 0 else 0.0)
    return v / n


def rot(pointer, degrees):
    """The rotation about ``pointer`` by ``degrees`` as a unit quaternion's matrix (tscode/algebra.py:285-344), restated."""
    p = unit(pointer)
    a = degrees * (np.pi / 180)
    s, c = np.sin(a / 2), np.cos(a / 2)
    q0, q1, q2, q3 = c, s * p[0], s * p[1], s * p[2]
    return np.array([[2 * (q0 * q0 + q1 * q1) - 1, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), 2 * (q0 * q0 + q2 * q2) - 1, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), 2 * (q0 * q0 + q3 * q3) - 1]])


def cross_unit(a, b, m):
    return unit(np.cross(a, b), m, length(a) * length(b))


def reject(v, axis, m):
    """v minus its component along the unit vector ``axis``; conditioning judged when the result is normalised later."""
    out = v - (v @ axis) * axis
    m.cond = min(m.cond, length(out) / length(v))
    return out


def neighbours_from_edges(edges, n):
    sets = [set() for _ in range(n)]
    for a, b in np.asarray(edges).reshape(-1, 2).tolist():
        if a != b:
            sets[a].add(b), sets[b].add(a)
    return [sorted(s) for s in sets]


def graph_part(atomnos, edges, reactive, overrides=None, orb_dim=None, leaving_group=None, sigmatropic=None):
    """Everything that is read from the bond graph of conformer 0, once: per reactive atom a plain dict."""
    n = len(atomnos)
    nbs = neighbours_from_edges(edges, n)
    sym = [SYM[int(z)] for z in atomnos]
    reactive = [int(i) for i in reactive]
    classes = [(overrides or {}).get(i) or TYPE_OF[sym[i] + str(len(nbs[i]))] for i in reactive]
    vicinal = len(reactive) == 2 and all(c in ("Sp3", "Single") for c in classes) and reactive[0] in nbs[reactive[1]]
    path = False
    if len(reactive) == 2 and all(c in ("Sp2", "Imine", "Sp_or_carbene") for c in classes):
        def walk(node, seen):                                 # every simple path, as the reference enumerates them
            for v in nbs[node]:
                if v == reactive[1]:
                    return True
                if v not in seen and len(nbs[v]) - 2 <= 1 and walk(v, seen | {v}):
                    return True
            return False
        path = walk(reactive[0], {reactive[0]})
    atoms = []
    for i, cls in zip(reactive, classes):
        nb = nbs[i]
        a = dict(cls=cls, atom=i, nb=nb, symbol=sym[i], sigmastar=vicinal)
        if cls in ("Single", "Sp3") and vicinal:
            a["partner"] = [j for j in reactive if j != i and j in nb][0]
            a["third"] = [v for v in (nbs[a["partner"]] if cls == "Single" else nb) if v not in (i, a["partner"])][0]
        elif cls == "Sp3":
            s = [sym[v] for v in nb]
            if len([t for t in s if t in ("O", "N", "Cl", "Br", "I")]) == 1:
                a["leaving"] = nb[s.index([t for t in s if t in ("O", "Cl", "Br", "I")][0])]
            elif len([t for t in s if t != "H"]) == 1:
                a["leaving"] = nb[s.index([t for t in s if t != "H"][0])]
            else:
                a["leaving"] = leaving_group[i]
        elif cls == "Ketone":
            a["non"] = [v for v in nbs[nb[0]] if v != i]
            if len(a["non"]) == 1:
                a["sub"] = [v for v in nbs[a["non"][0]] if v != nb[0]][0]
        elif cls == "Sp_or_carbene":
            s = [sym[v] for v in nb]
            sides = [[v for v in nbs[nb[0]] if v != i], [v for v in nbs[nb[1]] if v != i]]
            a["ref"] = None
            if all(t == "C" for t in s):
                a["ref"] = (sides[0][0], nb[0])
            elif sorted(s) in (["C", "O"], ["C", "S"]):
                if len(sides[0]) == 2:
                    a["ref"] = (sides[0][0], nb[0])
                elif len(sides[1]) == 2:
                    a["ref"] = (sides[1][0], nb[1])
        elif cls == "Metal":
            a["second"] = nbs[nb[0]][0]
        a["orb_dim"] = None if orb_dim is None else orb_dim.get(i)
        atoms.append(a)
    mode = ("distance" if path else "never") if sigmatropic is None else ("always" if sigmatropic else "never")
    return dict(atoms=atoms, classes=classes, sigmastar=vicinal, path=path, mode=mode, neighbours=[nbs[i] for i in reactive], reactive=reactive)


def dim_of(a, name):
    if a["orb_dim"] is not None:
        return a["orb_dim"]
    if a["cls"] == "Metal":
        return ORB_DIM["Metal"]
    return ORB_DIM.get(a["symbol"] + " " + name, None if a["cls"] == "Single" else ORB_DIM["Fallback"])


def lobes_of(x, a, sigmatropic, seed, m):
    """(centres, orbital vectors, name) of one reactive atom of one conformer."""
    cls, coord, nb = a["cls"], x[a["atom"]], a["nb"]
    if cls in ("Single", "Sp3"):
        name = NAME_OF[cls]
        d = dim_of(a, name)
        if cls == "Single" and d is None:
            d = length(coord - x[nb[0]])
        if not a["sigmastar"]:
            if cls == "Single":
                vecs = [unit(coord - x[nb[0]], m)]
                return [d * vecs[0] + coord], vecs, name
            vecs = [coord - x[a["leaving"]]]
            return [d * unit(vecs[0], m) + coord], vecs, name
        partner = x[a["partner"]]
        pivot = unit(partner - coord, m)
        v = reject(unit(x[a["third"]] - (partner if cls == "Single" else coord), m), pivot, m)
        vecs = [rot(pivot, angle + 60) @ v for angle in (0, 120, 240)]
        return [d * (w if cls == "Single" else unit(w)) + coord for w in vecs], vecs, name
    if cls == "Sp2":
        d = dim_of(a, "sp2")
        n0, n1, n2 = (unit(x[j] - coord, m) for j in nb[:3])
        v = unit((np.cross(n0, n1) + np.cross(n1, n2) + np.cross(n2, n0)) / 3, m)
        return [v * d + coord, -v * d + coord], [v, -v], "sp2"
    if cls == "Ether":
        d = dim_of(a, "Ether")
        v = [d * unit(x[j] - coord, m) for j in nb[:2]]
        m.cond = min(m.cond, length(v[0] + v[1]) / (2 * d), length(np.cross(v[0], v[1])) / (d * d))
        mat = rot((v[0] + v[1]) / 2, 90) @ rot(np.cross(v[0], v[1]), 180)
        vecs = [mat @ w for w in v]
        return [w + coord for w in vecs], vecs, "Ether"
    if cls == "Ketone":
        d = dim_of(a, "Ketone")
        vector = unit(x[nb[0]] - coord, m) * d
        non = a["non"]
        if len(non) == 1:
            v = x[a["sub"]] - x[non[0]]
            pointer = v - (v @ unit(vector)) * vector
            pointer = unit(pointer, m, length(v)) * d
            centres, name = [rot(vector, 90 * k) @ pointer for k in range(4)], "Ketone (p+p)"
        elif len(non) == 2:
            pivot = cross_unit(x[non[0]] - coord, x[non[1]] - coord, m)
            if sigmatropic:
                centres, name = [pivot * d, -pivot * d], "Ketone (p)"
            else:
                centres, name = [rot(pivot, angle) @ vector for angle in (120, 240)], "Ketone (sp2)"
        else:
            v = [unit(x[j] - coord, m) * d for j in non]
            pivot = cross_unit(vector, v[0], m)
            centres, name = [rot(pivot, 180) @ w for w in v], "Ketone (trilobe)"
        return [c + coord for c in centres], [unit(c) for c in centres], name
    if cls == "Imine":
        d = dim_of(a, "Imine")
        v0, v1 = x[nb[0]] - coord, x[nb[1]] - coord
        if sigmatropic:
            p = cross_unit(v0, v1, m) * d
            vecs = [p, -p]
        else:
            vecs = [-unit((unit(v0, m) + unit(v1, m)) / 2, m) * d]
        return [w + coord for w in vecs], vecs, "Imine"
    if cls == "Sp_or_carbene":
        v0, v1 = x[nb[0]] - coord, x[nb[1]] - coord
        n0, n1 = unit(v0, m), unit(v1, m)
        angle = np.arccos(min(1.0, max(-1.0, unit(n0) @ unit(n1)))) * 180 / np.pi
        m.angle = min(m.angle, abs(angle - 175))
        if abs(angle - 180) < 5:
            d = dim_of(a, "sp")
            if a["ref"] is not None:
                axis = unit(x[nb[0]] - x[nb[1]], m)
                pivot1 = reject(x[a["ref"][0]] - x[a["ref"][1]], axis, m)
            else:
                v = np.asarray(seed, dtype=np.float64)
                pivot1 = v - (v @ n0) * v0
                m.cond = min(m.cond, length(pivot1) / length(v))
            pivot2 = cross_unit(pivot1, v0, m)
            vecs = [rot(pivot2, 90) @ rot(pivot1, angle) @ n0 * d for angle in (0, 90, 180, 270)]
            return [w + coord for w in vecs], vecs, "sp"
        d = dim_of(a, "bent carbene")
        p = cross_unit(n0, n1, m)
        vecs = [-unit((n0 + n1) / 2, m) * d, p * d, -p * d]
        return [w + coord for w in vecs], vecs, "bent carbene"
    d = dim_of(a, "Metal")
    v1, v2 = x[nb[0]] - coord, x[a["second"]] - coord
    m.cond = min(m.cond, length(np.cross(v1, v2)) / (length(v1) * length(v2)))
    v = unit(rot(np.cross(v1, v2), 120) @ v1, m, length(v1))
    vecs = [rot(v1, 90 * k) @ v for k in range(4)]
    return [w * d + coord for w in vecs], vecs, "Metal"


def pivots_of(centres, suprafacial, sigmastar, m):
    """[(pivot, mean point, (i, j))] of one conformer: the lobe pairs with the first index fastest (one reactive atom: i < j), the
    suprafacial filter where there are exactly four, the sigma-star filter."""
    if len(centres) == 2:
        pairs = [(i, j) for j in range(len(centres[1])) for i in range(len(centres[0]))]
        second = centres[1]
    elif len(centres) == 1:
        pairs = [(i, j) for j in range(len(centres[0])) for i in range(len(centres[0])) if i < j]
        second = centres[0]
    else:
        return []
    out = [(second[j] - centres[0][i], (centres[0][i] + second[j]) / 2, (i, j)) for i, j in pairs]
    if len(out) == 4:
        norms = sorted(length(p[0]) for p in out)
        m.gap = min(m.gap, norms[2] - norms[1])
    if suprafacial and len(out) == 4:
        norms = [length(p[0]) for p in out]
        for sample in norms:
            if sum(sample >= v for v in norms) == 2:
                out = [p for p, v in zip(out, norms) if v <= sample]
                break
    if sigmastar and out:
        lengths = [length(p[0]) for p in out]
        m.band = m.band or any(GUARD_BAND[0] <= v - min(lengths) <= GUARD_BAND[1] for v in lengths)
        out = [p for p, v in zip(out, lengths) if v - min(lengths) < 1e-5]
    return out


def restate(coords, atomnos, edges, reactive, seed=(1.0, 0.0, 0.0), suprafacial=False, **graph_options):
    """Every output of tsc_orbitals for coords f64[C, n, 3], in NumPy, plus the margins of every conformer."""
    g = graph_part(atomnos, edges, reactive, **graph_options)
    C, R = len(coords), len(g["atoms"])
    e = types.SimpleNamespace(centers=np.zeros((C, R, 4, 3)), orb_vecs=np.zeros((C, R, 4, 3)), n_lobes=np.zeros((C, R), np.uint8),
                              kind=np.zeros((C, R), np.uint8), sigmatropic=np.zeros(C, bool), pivot=np.zeros((C, 16, 3)),
                              meanpoint=np.zeros((C, 16, 3)), lobe_index=np.full((C, 16, 2), -1, np.int8), n_pivots=np.zeros(C, np.uint8),
                              margins=[], graph=g)
    for c, x in enumerate(coords):
        m = Margins()
        sig = g["mode"] == "always"
        if len(g["reactive"]) == 2 and g["path"]:
            d = length(x[g["reactive"][0]] - x[g["reactive"][1]])
            m.dist = abs(d - 3)
            if g["mode"] == "distance":
                sig = d < 3
        e.sigmatropic[c] = sig
        centres = []
        for r, a in enumerate(g["atoms"]):
            cen, vec, name = lobes_of(x, a, sig, seed, m)
            e.centers[c, r, :len(cen)], e.orb_vecs[c, r, :len(vec)] = cen, vec
            e.n_lobes[c, r], e.kind[c, r] = len(cen), KINDS.index(name)
            centres.append(cen)
        piv = pivots_of(centres, suprafacial, g["sigmastar"], m)
        for k, (p, mean, ij) in enumerate(piv):
            e.pivot[c, k], e.meanpoint[c, k], e.lobe_index[c, k] = p, mean, ij
        e.n_pivots[c] = len(piv)
        e.margins.append(m)
    return e


def case_options(g):
    """The arguments a recorded case was run with, for the restatement and for the product (atom -> value mappings)."""
    o = g.meta["options"]
    return dict(orb_dim={int(k): v for k, v in o["orb_dim"].items()} if o.get("orb_dim") else None,
                leaving_group={int(k): v for k, v in o["leaving_group"].items()} if o.get("leaving_group") else None)


_RESTATED = {}


def restated(case, suprafacial=False):
    if (case, suprafacial) not in _RESTATED:
        g = g23(case)
        _RESTATED[(case, suprafacial)] = restate(g.coords, g.atomnos, g.edges, g.reactive, seed=g.seed, suprafacial=suprafacial, **case_options(g))
    return _RESTATED[(case, suprafacial)]


def assert_equal_outputs(res, e, pivots=True):
    for name in ("kind", "n_lobes", "sigmatropic"):
        assert (np.asarray(res[name]) == getattr(e, name)).all(), name
    for name in ("centers", "orb_vecs"):
        assert np.abs(res[name] - getattr(e, name)).max() <= VAL_TOL, (name, np.abs(res[name] - getattr(e, name)).max())
    if pivots:
        assert (res["n_pivots"] == e.n_pivots).all(), (res["n_pivots"][:8], e.n_pivots[:8])
        assert (res["lobe_index"] == e.lobe_index).all()
        for name in ("pivot", "meanpoint"):
            assert np.abs(res[name] - getattr(e, name)).max() <= VAL_TOL, name


# ------------------------------------------------------------------------------------------------------- CPU: the fixtures
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    g = g23(case)
    for supra, tag in ((False, "off"), (True, "on")):
        e = restated(case, supra)
        assert e.graph["classes"] == g.meta["classes"] and e.graph["neighbours"] == g.meta["neighbors"]
        assert e.graph["sigmastar"] == g.meta["sp3_sigmastar"] and e.graph["path"] == g.meta["sigmatropic_path"]
        assert [[KINDS[k] for k in row] for row in e.kind] == g.meta["names"]
        assert (e.n_lobes == g.n_lobes).all() and (e.sigmatropic == g.sigmatropic).all()
        assert np.abs(e.centers - g.centers).max() <= VAL_TOL and np.abs(e.orb_vecs - g.orb_vecs).max() <= VAL_TOL
        assert (e.n_pivots == getattr(g, "n_pivots_" + tag)).all() and (e.lobe_index == getattr(g, "lobe_index_" + tag)).all()
        assert np.abs(e.pivot - getattr(g, "pivot_" + tag)).max() <= VAL_TOL
        assert np.abs(e.meanpoint - getattr(g, "meanpoint_" + tag)).max() <= VAL_TOL


@pytest.mark.parametrize("case", CASES)
def test_fixture_conditions(case):
    """What the generator asserts, asserted again on the files."""
    g = g23(case)
    e = restated(case)
    assert all(m.ok() for m in e.margins), [vars(m) for m in e.margins if not m.ok()][:3]
    for name in ("centers", "orb_vecs", "pivot_off", "meanpoint_off", "pivot_on", "meanpoint_on", "coords"):
        assert np.isfinite(getattr(g, name)).all(), name
    assert os.path.getsize(os.path.join(GOLDEN, g.meta["file"])) < 700000
    if case == "allene":
        share = float(np.mean(e.kind[:, 0] == KINDS.index("sp")))
        assert 0.2 <= share <= 0.8 and set(e.n_lobes[:, 0].tolist()) == {3, 4} and set(e.n_pivots.tolist()) == {3, 6}
    if case == "diimine":
        assert 0.2 <= float(np.mean(e.sigmatropic)) <= 0.8 and set(map(tuple, e.n_lobes.tolist())) == {(1, 1), (2, 2)}
    if case == "ch3cl_ch":
        assert g.meta["sp3_sigmastar"] and (e.n_lobes == 3).all() and (e.n_pivots == 3).all()
    if case == "c2h4":
        assert e.sigmatropic.all() and (e.n_pivots == 4).all() and (restated(case, True).n_pivots == 2).all()
    if case == "acetonitrile":
        assert (e.kind == KINDS.index("sp")).all() and not np.allclose(g.seed, (1, 0, 0))
    if case == "ketene":
        assert (e.kind == KINDS.index("Ketone (p+p)")).all()
    if case == "alkoxide":
        assert (e.kind == KINDS.index("Ketone (trilobe)")).all()
    if case == "enolate":
        assert g.meta["classes"][-1] == "Metal" and int(g.atomnos[-1]) == 3
    if case == "propenal50":
        assert len(g.atomnos) == 50


def test_orb_dim_dict_equals_the_recorded_dict():
    from tscode_amd.reactive_atoms import ORB_DIM_DICT
    recorded = json.load(open(os.path.join(GOLDEN, "G23_orbitals.json")))["orb_dim_dict"]
    assert ORB_DIM_DICT == recorded == ORB_DIM


@pytest.mark.parametrize("case", CASES)
def test_recipes_equal_the_recorded_graph_facts(case):
    """orbital_recipes / atom_type / is_vicinal / the sigmatropic path flag against what the reference's graph gave, without the library."""
    from tscode_amd import reactive_atoms as ra
    g = g23(case)
    opts = case_options(g)
    host = ra.orbital_recipes(g.atomnos, g.reactive, g.edges, orb_dim=opts["orb_dim"], leaving_group=opts["leaving_group"], sp_seed=g.seed)
    assert host["classes"] == g.meta["classes"] and host["neighbors"] == g.meta["neighbors"]
    assert host["sp3_sigmastar"] == g.meta["sp3_sigmastar"] and host["sigmatropic_path"] == g.meta["sigmatropic_path"]
    assert [ra.atom_type(g.edges, g.atomnos, int(i)) for i in g.reactive] == g.meta["classes"]
    nbs = ra.neighbor_lists(g.edges, len(g.atomnos))
    assert ra.is_vicinal(nbs, g.reactive, host["classes"]) == g.meta["sp3_sigmastar"]
    assert ra.sigmatropic_path(nbs, g.reactive, host["classes"]) == g.meta["sigmatropic_path"]
    # the same graph as packed bits and as a graph object
    from tscode_amd.graph_manipulations import pack_edges
    assert ra.neighbor_lists(pack_edges(g.edges, len(g.atomnos)), len(g.atomnos)) == nbs
    graph = types.SimpleNamespace(nodes=list(range(len(g.atomnos))), edges=[tuple(e) for e in g.edges.tolist()] + [(0, 0)])
    assert ra.neighbor_lists(graph, len(g.atomnos)) == nbs
    rec = host["recipes"]
    assert rec.dtype.itemsize == 88 and (rec["atom"] == g.reactive).all()
    assert ra.atom_type(g.edges, g.atomnos, 0, override="Single") == "Single"


def test_header_and_prototype_table_declare_the_entry_points():
    import tscode_amd
    from tscode_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tscode_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"{s} not declared in include/tscode_hip.h"
        assert s in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["tsc_orbitals"] == _lib._SIGNATURES["tsc_orbitals_dev"]
    assert "orbitals.hip" in build.SOURCES and "orbitals.hpp" in build.HEADERS
    for name in ("orbitals_batch", "orbital_recipes", "reactive_molecule", "atom_type"):
        assert callable(getattr(tscode_amd, name))
    assert callable(tscode_amd.Engine.orbitals) and callable(tscode_amd.Engine.orbitals_dev)


def test_refusals_raise_value_error_before_the_library_is_loaded(monkeypatch):
    import tscode_amd as ta
    from tscode_amd import reactive_atoms as ra

    def no_library(*a, **k):
        raise AssertionError("the library was asked for before the arguments were refused")
    monkeypatch.setattr(ra, "get_engine", no_library)
    g = g23("ch3cl_c")
    x, z, e = g.coords, g.atomnos, g.edges
    # nine reactive atoms on a chain of ten carbons
    chain = np.array([(i, i + 1) for i in range(9)])
    # a carbon with two chlorines and two carbons: the leaving group cannot be inferred;  a carbon with one nitrogen and three carbons
    z_amb, e_amb = np.array([6, 17, 17, 6, 6]), np.array([(0, 1), (0, 2), (0, 3), (0, 4)])
    z_n, e_n = np.array([6, 7, 6, 6, 6]), e_amb
    mixed = ra.ReactiveMolecule(np.zeros((2, 3, 3)), [0], {"n_lobes": np.array([[4], [3]], np.uint8), "centers": np.zeros((2, 1, 4, 3)),
                                                          "orb_vecs": np.zeros((2, 1, 4, 3)), "n_pivots": np.zeros(2, np.uint8),
                                                          "pivot": np.zeros((2, 16, 3)), "meanpoint": np.zeros((2, 16, 3))}, 0)
    bad = x.copy()
    bad[0, 0, 0] = np.nan
    refusals = [
        lambda: ta.orbitals_batch(x[:, :4], z, [0], e),                                   # atoms per conformer != atomic numbers
        lambda: ta.orbitals_batch(np.zeros((2, 5, 2)), z, [0], e),                        # wrong shape
        lambda: ta.orbitals_batch(bad, z, [0], e),                                        # non-finite coordinates
        lambda: ta.orbitals_batch(x, z.astype(float), [0], e),                            # atomic numbers that are no integers
        lambda: ta.orbitals_batch(np.zeros((1, 10, 3)), np.full(10, 6), list(range(9)), chain),   # R > 8
        lambda: ta.orbitals_batch(x, z, [], e),                                           # no reactive atom
        lambda: ta.orbitals_batch(x, z, [5], e),                                          # index out of range
        lambda: ta.orbitals_batch(x, z, [-1], e),
        lambda: ta.orbitals_batch(x, z, [0, 0], e),                                       # a repeated atom
        lambda: ta.orbitals_batch(x, z, [7]),                                             # (bonds=None: the index checks still come first)
        lambda: ta.orbitals_batch(x, z, [0], np.array([(0, 9)])),                         # a bond index out of range
        lambda: ta.orbitals_batch(x, z, [0], np.zeros((3, 3), int)),                      # an edge list that is none
        lambda: ta.orbitals_batch(x, z, [0], e, overrides="Sp4"),                         # an unknown class name
        lambda: ta.orbitals_batch(x, z, [0], e, orb_dim=np.inf),
        lambda: ta.orbitals_batch(x, z, [0], e, orb_dim={3: 1.0}),                        # an orb_dim for an atom that is not reactive
        lambda: ta.orbitals_batch(x, z, [0], e, sp_seed=(1, 2)),
        lambda: ta.orbitals_batch(x, z, [0], e, sigmatropic="yes"),
        lambda: ta.orbitals_batch(np.zeros((1, 5, 3)), z_amb, [0], e_amb),                # uninferable leaving group
        lambda: ta.orbitals_batch(np.zeros((1, 5, 3)), z_amb, [0], e_amb, leaving_group=7),   # ... and one that is not bonded
        lambda: ta.orbitals_batch(np.zeros((1, 5, 3)), z_n, [0], e_n),                    # the lone nitrogen
        lambda: ta.orbitals_batch(x, z, [1], e, overrides="Sp2"),                         # a class that reads more neighbours than the atom has
        lambda: ta.orbitals_batch(np.zeros((1, 2, 3)), np.array([8, 8]), [0], np.array([(0, 1)])),   # a Ketone whose neighbour has no other neighbour
        lambda: ta.reactive_molecule(x, z, [0, 1, 2], e),                                 # the embed drivers take one or two
        lambda: ta.reactive_molecule(x, z, [0], e, cumnum_offset=-1),
        lambda: ta.atom_type(e, z, 9),
        lambda: ta.atom_type(e, np.array([6, 1, 1, 1, 79]), 4),                           # an element / bond count without a class
        mixed.string_inputs,                                                              # mixed lobe counts
    ]
    for k, call in enumerate(refusals):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} did not raise")
    with pytest.raises(ValueError, match="nitrogen"):
        ra.orbital_recipes(z_n, [0], e_n)
    before = (x.copy(), z.copy(), e.copy())
    ra.orbital_recipes(z, [0, 1], e)
    assert (x == before[0]).all() and (z == before[1]).all() and (e == before[2]).all()


def test_c_abi_refuses_every_limit_before_any_launch():
    """tsc_orbitals with zero conformers: the arguments are checked, nothing is launched and the context is not touched (a block of zeroed
    memory stands in for it), so the refusals of include/tscode_hip.h can be asked for without a GPU."""
    import ctypes as C
    from tscode_amd import _lib
    from tscode_amd.build import build
    from tscode_amd.reactive_atoms import RECIPE_DTYPE
    build()
    lib = _lib.load()
    ctx = C.create_string_buffer(4096)
    n = 6

    def recipe(**kw):
        r = np.zeros(1, RECIPE_DTYPE)
        r["cls"], r["atom"], r["nb"], r["ex"], r["orb_dim"], r["orb_dim_bent"], r["seed"] = 1, 0, (1, 2, 3, -1), -1, 1.0, 1.0, (1, 0, 0)
        for k, v in kw.items():
            r[k] = v
        return r

    def call(rec, n_atoms=n, mode=0, outs=9, R=None):
        bufs = [np.zeros(64) for _ in range(9)]
        ptrs = [_lib.ptr(b) for b in bufs[:outs]] + [None] * (9 - outs)
        return lib.tsc_orbitals(C.cast(ctx, C.c_void_p), _lib.ptr(np.zeros((1, n_atoms, 3))), 0, n_atoms, _lib.ptr(rec), len(rec) if R is None else R,
                                mode, 0, *ptrs)

    assert call(recipe()) == 0, lib.tsc_last_error()
    assert call(recipe(), outs=5) == 0, lib.tsc_last_error()                               # (without the pivot arrays)
    two = np.concatenate([recipe(), recipe(atom=3, nb=(0, 4, 5, -1))])
    assert call(two, mode=1) == 0, lib.tsc_last_error()
    assert call(np.concatenate([two, recipe(atom=1, nb=(0, 2, 3, -1))]), outs=5) == 0, lib.tsc_last_error()      # three reactive atoms, no pivot arrays
    refused = [lambda: call(recipe(), n_atoms=0), lambda: call(recipe(), n_atoms=65537), lambda: call(recipe(), R=0), lambda: call(recipe(), R=9),
               lambda: call(recipe(cls=8)), lambda: call(recipe(cls=-1)), lambda: call(recipe(flags=64)), lambda: call(recipe(atom=n)),
               lambda: call(recipe(atom=-1)), lambda: call(recipe(nb=(1, 2, n, -1))), lambda: call(recipe(nb=(1, -1, 3, -1))),
               lambda: call(recipe(cls=4)),                                                 # a Ketone without a subtype
               lambda: call(recipe(cls=4, flags=48, ex=(1, 2, -1, -1))),                    # a trilobe that names two atoms
               lambda: call(recipe(cls=7, ex=(n, -1, -1, -1))), lambda: call(recipe(cls=2)),   # Sp3 without its leaving group
               lambda: call(recipe(orb_dim=np.nan)), lambda: call(recipe(seed=(np.inf, 0, 0))), lambda: call(recipe(), mode=3),
               lambda: call(recipe(), mode=1),                                              # by distance with one reactive atom
               lambda: call(np.concatenate([recipe(cls=0, flags=1, ex=(3, 4, -1, -1)), recipe(atom=3)])),   # disagree on sigma-star
               lambda: call(recipe(), outs=7), lambda: call(recipe(), outs=4),
               lambda: call(np.concatenate([recipe(), recipe(atom=3, nb=(0, 4, 5, -1)), recipe(atom=1, nb=(0, 2, 3, -1))]))]   # pivot arrays with R = 3
    for k, f in enumerate(refused):
        assert f() == -1, (k, lib.tsc_last_error())                                         # TSC_ERR_INVALID
        assert lib.tsc_last_error()


# ------------------------------------------------------------------------------------------------------- sweep inputs
PAD_SPACING = 4.0
SWEEP_C = (1, 63, 64, 65, 257, 4097)
SWEEP_N = (5, 64, 200)
DISTINCT = 257
# molecule of a sweep -> (G23 case whose atoms it takes, the reactive atoms of that case moved to the first / last index, noise sigma)
SWEEP_MOLS = {5: ("ch3cl_ch", "ch3cl_c"), 64: ("allene", "diimine", "ch3cl_ch"), 200: ("allene", "diimine", "ch3cl_ch")}
_SWEEP = {}


def sweep_core(case):
    """(atomnos, edges, reactive, conformers f64[DISTINCT, k, 3], seed) of a sweep molecule: the atoms of a G23 case reordered so that its
    reactive atoms are the first and the last (one reactive atom: the last), with seeded noise of the case's sigma, every conformer
    redrawn (seed + 1000 * attempt) until it keeps the guards."""
    if case not in _SWEEP:
        g = g23(case)
        k = len(g.atomnos)
        r = [int(i) for i in g.reactive]
        rest = [i for i in range(k) if i not in r]
        order = ([r[0]] + rest + [r[1]]) if len(r) == 2 else (rest + r)
        new_of = {old: new for new, old in enumerate(order)}
        z = g.atomnos[order]
        edges = np.array([(new_of[a], new_of[b]) for a, b in g.edges.tolist()], dtype=np.int64).reshape(-1, 2)
        reactive = [new_of[i] for i in r]
        base, sigma = g.base[order], float(g.meta["sigma"])
        out = np.zeros((DISTINCT, k, 3))
        for c in range(DISTINCT):
            for attempt in range(50):
                x = base + np.random.default_rng(230000 + 7 * c + 1000 * attempt).normal(size=base.shape) * sigma
                both = [restate(x[None], z, edges, reactive, seed=g.seed, suprafacial=s) for s in (False, True)]
                if all(e.margins[0].ok() and np.isfinite(e.centers).all() for e in both):
                    break
            else:
                raise AssertionError(f"{case}: conformer {c} never keeps the guards")
            out[c] = x
        _SWEEP[case] = dict(z=z, edges=edges, reactive=reactive, coords=out, seed=g.seed, expect={})
    return _SWEEP[case]


def sweep_input(case, n, C, suprafacial):
    """(coords f64[C, n, 3], atomnos, edges, reactive, expected) -- the core molecule with isolated hydrogens on a far grid between its first
    and last atom, the DISTINCT conformers repeated up to C."""
    core = sweep_core(case)
    k = len(core["z"])
    pad = n - k
    assert pad >= 0
    keep = list(range(k - 1)) + [n - 1]                                                   # where the core's atoms go
    z = np.ones(n, dtype=np.int64)
    z[keep] = core["z"]
    grid = np.array([(30.0 + PAD_SPACING * (q % 8), 30.0 + PAD_SPACING * ((q // 8) % 8), 30.0 + PAD_SPACING * (q // 64)) for q in range(pad)]).reshape(-1, 3)
    move = {old: new for old, new in enumerate(keep)}
    edges = np.array([(move[a], move[b]) for a, b in core["edges"].tolist()], dtype=np.int64).reshape(-1, 2)
    reactive = [move[i] for i in core["reactive"]]
    x = np.zeros((DISTINCT, n, 3))
    x[:, keep] = core["coords"]
    x[:, k - 1:n - 1] = grid
    if (n, suprafacial) not in core["expect"]:
        core["expect"][(n, suprafacial)] = restate(x, z, edges, reactive, seed=core["seed"], suprafacial=suprafacial)
    reps = -(-C // DISTINCT)
    return np.ascontiguousarray(np.tile(x, (reps, 1, 1))[:C]), z, edges, reactive, core["expect"][(n, suprafacial)], reps


def tiled(e, reps, C):
    out = types.SimpleNamespace()
    for name in ("centers", "orb_vecs", "n_lobes", "kind", "sigmatropic", "pivot", "meanpoint", "lobe_index", "n_pivots"):
        a = getattr(e, name)
        setattr(out, name, np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:C])
    return out


def test_sweep_inputs_hold_both_outcomes_in_every_wavefront():
    """The allene and diimine sweeps mix their two outcomes inside every run of 64 conformers, so lanes of a wavefront diverge."""
    for case, column in (("allene", lambda e: e.kind[:, 0] == KINDS.index("sp")), ("diimine", lambda e: e.sigmatropic)):
        _, _, _, _, e, _ = sweep_input(case, 64, DISTINCT, False)
        v = column(e)
        assert 0.2 <= float(v.mean()) <= 0.8
        for lo in range(0, 256, 64):
            assert 0 < int(v[lo:lo + 64].sum()) < 64, (case, lo)
        assert all(m.ok() for m in e.margins)


# ------------------------------------------------------------------------------------------------------- branches G23 does not reach
TET = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]) / np.sqrt(3)
F_BOND_LENGTH, F_KETENE = 2, 8                                                            # TSC_ORB_F_* of include/tscode_hip.h
_EXTRA = {}
EXTRAS = ("ketene_carbon_first_side", "ketene_carbon_second_side", "single_without_parameter", "given_leaving_group", "override_one_atom")


def extra_case(name):
    """A molecule, the arguments for the product and for the restatement, and what the recipe must hold -- for the host's choices that no
    recorded case makes: the ketene bookkeeping of an 'sp' carbon on either side, Single's fall-back to the conformer's bond length, a
    leaving group that has to be given, a class override for one atom of two.  12 conformers, each redrawn until it keeps the guards."""
    if name in _EXTRA:
        return _EXTRA[name]
    product, want = {}, {}
    if name.startswith("ketene_carbon"):
        g = g23("ketene")                                                                  # C0(H2)=C1=O2, H3, H4
        order = [0, 1, 2, 3, 4] if name.endswith("first_side") else [2, 1, 0, 3, 4]        # ... or O first: then nb[1] is the side with two
        new_of = {old: new for new, old in enumerate(order)}
        z, base = g.atomnos[order], g.base[order]
        edges = np.array([(new_of[a], new_of[b]) for a, b in g.edges.tolist()])
        reactive, sigma = [1], 0.01
        want = dict(flags=F_KETENE, ex=[3, new_of[0]], kinds={"sp"})
    elif name == "single_without_parameter":
        g = g23("enolate")
        z, base, edges, reactive, sigma = g.atomnos, g.base, g.edges, [6], 0.03
        product = dict(overrides={6: "Single"})                                           # there is no 'Li Single Bond' in orb_dim_dict
        want = dict(flags=F_BOND_LENGTH, ex=[], kinds={"Single Bond"})
    elif name == "given_leaving_group":
        z = np.array([6, 17, 17, 1, 6, 1, 1, 1])                                           # CHCl2-CH3
        c4 = 1.53 * TET[3]
        base = np.array([(0, 0, 0), *(1.77 * TET[:2]), 1.09 * TET[2], c4, *(c4 - 1.09 * TET[:3])], dtype=np.float64)
        edges = np.array([(0, 1), (0, 2), (0, 3), (0, 4), (4, 5), (4, 6), (4, 7)])
        reactive, sigma = [0], 0.03
        product = dict(leaving_group={0: 2})
        want = dict(flags=0, ex=[2], kinds={"sp3"})
    else:
        g = g23("hcooh_co")
        z, base, edges, reactive, sigma = g.atomnos, g.base, g.edges, [1, 3], 0.03
        product = dict(overrides={3: "Single"})                                           # the hydroxyl oxygen as a Single Bond beside a Ketone
        want = dict(flags=None, ex=None, kinds={"Ketone (sp2)", "Single Bond"})
    coords = np.zeros((12,) + base.shape)
    for c in range(12):
        for attempt in range(50):
            x = base + np.random.default_rng(231000 + 7 * c + 1000 * attempt).normal(size=base.shape) * sigma
            e = restate(x[None], z, edges, reactive, **product)
            if e.margins[0].ok() and np.isfinite(e.centers).all():
                break
        else:
            raise AssertionError(f"{name}: conformer {c} never keeps the guards")
        coords[c] = x
    _EXTRA[name] = dict(z=z, edges=edges, reactive=reactive, coords=coords, product=product, want=want, expect=restate(coords, z, edges, reactive, **product))
    return _EXTRA[name]


@pytest.mark.parametrize("name", EXTRAS)
def test_recipes_of_the_branches_no_fixture_reaches(name):
    from tscode_amd import reactive_atoms as ra
    x = extra_case(name)
    host = ra.orbital_recipes(x["z"], x["reactive"], x["edges"], **x["product"])
    e, want = x["expect"], x["want"]
    assert host["classes"] == e.graph["classes"] and host["neighbors"] == e.graph["neighbours"]
    assert {KINDS[k] for k in e.kind.ravel()} == want["kinds"]
    rec = host["recipes"]
    if want["flags"] is not None:
        assert int(rec[0]["flags"]) == want["flags"] and [int(v) for v in rec[0]["ex"] if v >= 0] == want["ex"]
    if name == "single_without_parameter":
        bond = np.linalg.norm(x["coords"][:, 6] - x["coords"][:, 2], axis=1)               # the lobe sits one bond length from the lithium
        assert np.abs(np.linalg.norm(e.centers[:, 0, 0] - x["coords"][:, 6], axis=1) - bond).max() < 1e-12 and bond.std() > 1e-3
        assert ra.orbital_recipes(x["z"], x["reactive"], x["edges"], overrides={6: "Single"}, orb_dim=1.0)["recipes"][0]["flags"] == 0
    if name == "override_one_atom":
        assert host["classes"] == ["Ketone", "Single"] and not host["sp3_sigmastar"]


def test_an_edge_list_given_as_a_list_of_lists_is_an_edge_list():
    """A molecule with one ring has as many bonds as atoms: cyclopentadiene's eleven edges as a plain list of lists are edges, whatever
    their count, and give what the same edges give as an array."""
    from tscode_amd import reactive_atoms as ra
    z = np.array([6] * 5 + [1] * 6)
    edges = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 0], [0, 5], [1, 6], [2, 7], [3, 8], [4, 9], [4, 10]]
    assert len(edges) == len(z)
    a, b = ra.orbital_recipes(z, [0, 3], np.array(edges)), ra.orbital_recipes(z, [0, 3], edges)
    assert a["classes"] == b["classes"] == ["Sp2", "Sp2"] and a["neighbors"] == b["neighbors"] == [[1, 4, 5], [2, 4, 8]]
    assert (a["recipes"] == b["recipes"]).all() and b["sigmatropic_path"]
    assert ra.atom_type(edges, z, 4) == "Sp3" and ra.atom_type([tuple(e) for e in edges], z, 0) == "Sp2"
    nbs = ra.neighbor_lists(edges, len(z))
    assert isinstance(nbs, ra.NeighborLists) and ra.orbital_recipes(z, [0, 3], nbs)["neighbors"] == a["neighbors"]
    with pytest.raises(ValueError):
        ra.orbital_recipes(z, [0, 3], [list(v) for v in nbs])                             # plain lists of neighbours are no edge list


# ------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_g23_through_orbitals_batch(case):
    """Every G23 case, suprafacial off and on: the reference's recorded arrays and the restatement."""
    import tscode_amd
    g = g23(case)
    opts = case_options(g)
    for supra, tag in ((False, "off"), (True, "on")):
        res = tscode_amd.orbitals_batch(g.coords, g.atomnos, g.reactive, g.edges, orb_dim=opts["orb_dim"], leaving_group=opts["leaving_group"],
                                        sp_seed=g.seed, suprafacial=supra)
        assert res["names"] == g.meta["names"] and res["sp3_sigmastar"] == g.meta["sp3_sigmastar"]
        assert (res["n_lobes"] == g.n_lobes).all() and (res["sigmatropic"] == g.sigmatropic).all()
        assert (res["n_pivots"] == getattr(g, "n_pivots_" + tag)).all() and (res["lobe_index"] == getattr(g, "lobe_index_" + tag)).all()
        assert np.abs(res["centers"] - g.centers).max() <= VAL_TOL and np.abs(res["orb_vecs"] - g.orb_vecs).max() <= VAL_TOL
        assert np.abs(res["pivot"] - getattr(g, "pivot_" + tag)).max() <= VAL_TOL
        assert np.abs(res["meanpoint"] - getattr(g, "meanpoint_" + tag)).max() <= VAL_TOL
        assert_equal_outputs(res, restated(case, supra))


@pytest.mark.gpu
def test_bond_graph_from_coordinates_gives_the_recorded_graph():
    """bonds=None: this package's graphize of conformer 0 (elements of its built-in radius table only)."""
    import tscode_amd
    for case in ("hcooh_co", "c2h4", "propenal50"):
        g = g23(case)
        res = tscode_amd.orbitals_batch(g.coords, g.atomnos, g.reactive, sp_seed=g.seed)
        assert res["neighbors"] == g.meta["neighbors"] and res["classes"] == g.meta["classes"]
        assert_equal_outputs(res, restated(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_device_entry_equals_the_recorded_arrays(case):
    """tsc_orbitals_dev on torch buffers; zero conformers write nothing."""
    import torch
    import tscode_amd
    from tscode_amd.reactive_atoms import orbital_recipes
    g = g23(case)
    opts = case_options(g)
    host = orbital_recipes(g.atomnos, g.reactive, g.edges, orb_dim=opts["orb_dim"], leaving_group=opts["leaving_group"], sp_seed=g.seed)
    eng = tscode_amd.get_engine()
    dev = torch.device("cuda", eng.device)
    C, n, R = g.coords.shape[0], g.coords.shape[1], len(g.reactive)
    shapes = {"centers": ((C, R, 4, 3), torch.float64), "orb_vecs": ((C, R, 4, 3), torch.float64), "n_lobes": ((C, R), torch.uint8),
              "kind": ((C, R), torch.uint8), "sigmatropic": ((C,), torch.uint8), "pivot": ((C, 16, 3), torch.float64),
              "meanpoint": ((C, 16, 3), torch.float64), "lobe_index": ((C, 16, 2), torch.int8), "n_pivots": ((C,), torch.uint8)}
    out = {k: torch.full(s, 7, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    d_x = torch.from_numpy(np.ascontiguousarray(g.coords)).to(dev)
    torch.cuda.synchronize()
    eng.orbitals_dev(d_x, 0, n, host["recipes"], host["sigmatropic_mode"], True, *out.values())
    eng.synchronize()
    assert all((v.cpu() == 7).all() for v in out.values()), "zero conformers wrote something"
    eng.orbitals_dev(d_x, C, n, host["recipes"], host["sigmatropic_mode"], True, *out.values())
    eng.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["sigmatropic"] = res["sigmatropic"].astype(bool)
    assert_equal_outputs(res, restated(case, True))
    assert [[KINDS[k] for k in row] for row in res["kind"]] == g.meta["names"]
    assert np.abs(res["pivot"] - g.pivot_on).max() <= VAL_TOL and (res["n_pivots"] == g.n_pivots_on).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SWEEP_N)
@pytest.mark.parametrize("C", SWEEP_C)
def test_sweeps_equal_the_restatement(C, n):
    """1 .. 4097 conformers (around one wavefront, more than one block, a grid of several blocks), molecules of 5, 64 and 200 atoms with the
    reactive atoms at the first and the last index, one and two reactive atoms, suprafacial off and on."""
    import tscode_amd
    for case in SWEEP_MOLS[n]:
        for supra in (False, True):
            x, z, edges, reactive, e, reps = sweep_input(case, n, C, supra)
            assert x.shape == (C, n, 3) and reactive[-1] == n - 1 and (len(reactive) == 1 or reactive[0] == 0)
            res = tscode_amd.orbitals_batch(x, z, reactive, edges, sp_seed=sweep_core(case)["seed"], suprafacial=supra)
            assert_equal_outputs(res, tiled(e, reps, C))


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXTRAS)
def test_branches_no_fixture_reaches_equal_the_restatement(name):
    import tscode_amd
    x = extra_case(name)
    res = tscode_amd.orbitals_batch(x["coords"], x["z"], x["reactive"], x["edges"], **x["product"])
    assert_equal_outputs(res, x["expect"])


@pytest.mark.gpu
def test_more_than_two_reactive_atoms_give_orbitals_and_no_pivots():
    import tscode_amd
    g = g23("propenal")
    reactive = [0, 1, 2, 3]
    res = tscode_amd.orbitals_batch(g.coords, g.atomnos, reactive, g.edges)
    e = restate(g.coords, g.atomnos, g.edges, reactive)
    assert "pivot" not in res and res["centers"].shape == (len(g.coords), 4, 4, 3)
    assert_equal_outputs(res, e, pivots=False)


@pytest.mark.gpu
def test_sigmatropic_override_reaches_the_ketone_p_lobes():
    import tscode_amd
    g = g23("propenal")
    res = tscode_amd.orbitals_batch(g.coords, g.atomnos, g.reactive, g.edges, sigmatropic=True)
    e = restate(g.coords, g.atomnos, g.edges, g.reactive, sigmatropic=True)
    assert all(row[1] == "Ketone (p)" for row in res["names"]) and res["sigmatropic"].all()
    assert_equal_outputs(res, e)
    off = tscode_amd.orbitals_batch(g23("c2h4").coords, g23("c2h4").atomnos, g23("c2h4").reactive, g23("c2h4").edges, sigmatropic=False)
    assert not off["sigmatropic"].any()


@pytest.mark.gpu
def test_chain_from_coordinates_to_the_recorded_cyclical_poses():
    """Coordinates -> reactive_molecule -> cyclical_embed_batch equals the reference's own cyclical_embed on the same two ensembles."""
    import tscode_amd
    g = g23("chain")
    mols, offset = [], 0
    for k in range(2):
        x, z = getattr(g, f"coords{k}"), getattr(g, f"atomnos{k}")
        mols.append(tscode_amd.reactive_molecule(x, z, getattr(g, f"reactive{k}"), getattr(g, f"edges{k}"), orb_dim=float(g.meta["dist"]) / 2,
                                                 cumnum_offset=offset))
        offset += len(z)
        for c in range(len(x)):
            assert np.abs(mols[k].pivots[c][0] - getattr(g, f"pivot_vec{k}_{c}")).max() <= VAL_TOL
            assert (mols[k].pivots[c][2] == getattr(g, f"pivot_cumnums{k}_{c}")).all()
    poses, cons = tscode_amd.cyclical_embed_batch(mols, g.angles, clash_thresh=float(g.meta["clash_thresh"]), rigid_shortcut=True)
    assert poses.shape == g.poses.shape and np.abs(poses - g.poses).max() < VAL_TOL
    assert np.array_equal(cons, g.constrained_indices)


@pytest.mark.gpu
def test_string_inputs_feed_string_embed_to_the_recorded_poses():
    """CH3Cl + HCOOH of G11 (cases 0 - 2: conformer ensembles included): string_inputs() in place of the recorded centres and vectors."""
    import tscode_amd
    from tscode_amd.reactive_atoms import neighbor_lists
    g = np.load(os.path.join(GOLDEN, "G11_string_embed.npz"), allow_pickle=False)
    edges = {5: {17: g23("ch3cl_c").edges, 8: g23("hcooh_oh").edges}}
    for k in range(3):
        dist = {0: 2.5, 1: None, 2: 2.2}[k]
        ins = []
        for m in range(2):
            x, z = g[f"coords{m}_{k}"], g[f"atomnos{m}_{k}"]
            e = edges[5][17 if 17 in z else 8]
            mol = tscode_amd.reactive_molecule(x, z, [int(g[f"reactive_index{m}_{k}"])], e, orb_dim=None if dist is None else dist / 2)
            centers, vecs = mol.string_inputs()
            assert np.abs(centers - g[f"centers{m}_{k}"]).max() <= VAL_TOL and np.abs(vecs - g[f"orb_vecs{m}_{k}"]).max() <= VAL_TOL
            ins += [centers, vecs]
        poses = tscode_amd.string_embed_batch(g[f"coords0_{k}"], g[f"coords1_{k}"], ins[0], ins[1], ins[2], ins[3], g[f"angles_{k}"],
                                              clash_thresh=float(g[f"clash_thresh_{k}"]), quadruplets=g[f"quadruplets_{k}"])
        assert poses.shape == g[f"poses_{k}"].shape and np.abs(poses - g[f"poses_{k}"]).max() < VAL_TOL
    assert neighbor_lists(edges[5][17], 5)[0] == [1, 2, 3, 4]


@pytest.mark.gpu
def test_kernel_time_is_taken_only_under_pass_timing_and_per_thread():
    """tsc_orbitals_timings on 2 conformers of the smallest fixture: -1 without the option, a positive time with it through both
    entries, -1 after zero conformers, -1 again once the option is off, -1 in a thread that never called."""
    import math
    import threading
    import torch
    import tscode_amd
    from tscode_amd.reactive_atoms import orbital_recipes
    g = g23(min(CASES, key=lambda case: g23(case).coords.shape[1]))
    opts = case_options(g)
    rec = orbital_recipes(g.atomnos, g.reactive, g.edges, orb_dim=opts["orb_dim"], leaving_group=opts["leaving_group"], sp_seed=g.seed)
    x = np.ascontiguousarray(g.coords[:2], dtype=np.float64)
    C, n, R = x.shape[0], x.shape[1], len(g.reactive)
    assert C == 2
    eng = tscode_amd.get_engine()
    dev = torch.device("cuda", eng.device)
    shapes = {"centers": ((C, R, 4, 3), torch.float64), "orb_vecs": ((C, R, 4, 3), torch.float64), "n_lobes": ((C, R), torch.uint8),
              "kind": ((C, R), torch.uint8), "sigmatropic": ((C,), torch.uint8)}
    out = {k: torch.zeros(s, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    d_x = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize()

    def host(rows=C):
        return eng.orbitals(x[:rows], rec["recipes"], rec["sigmatropic_mode"], False, want_pivots=False)

    def device():
        eng.orbitals_dev(d_x, C, n, rec["recipes"], rec["sigmatropic_mode"], False, *out.values())
        eng.synchronize()

    def in_a_fresh_thread():
        got = []
        t = threading.Thread(target=lambda: got.append(eng.orbitals_kernel_ms()))
        t.start()
        t.join()
        return got[0]

    with eng.options(pass_timing=0):
        want = host()
        assert eng.orbitals_kernel_ms() == -1.0
        device()
        assert eng.orbitals_kernel_ms() == -1.0
        with eng.options(pass_timing=1):
            timed = host()
            assert math.isfinite(eng.orbitals_kernel_ms()) and eng.orbitals_kernel_ms() > 0.0
            assert timed["centers"].tobytes() == want["centers"].tobytes()
            assert in_a_fresh_thread() == -1.0
            device()
            assert math.isfinite(eng.orbitals_kernel_ms()) and eng.orbitals_kernel_ms() > 0.0
            assert out["centers"].cpu().numpy().tobytes() == want["centers"].tobytes()
            host(0)
            assert eng.orbitals_kernel_ms() == -1.0
            host()
            assert eng.orbitals_kernel_ms() > 0.0
        host()
        assert eng.orbitals_kernel_ms() == -1.0
