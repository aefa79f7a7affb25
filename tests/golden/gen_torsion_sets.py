"""G25 generator: what the reference's csearch sets up per structure -- hydrogen bonds, the segmentation verdict, torsions, folds,
rotation masks -- and what its csearch_augmentation loop returns.  Runs ONLY in the build container, never where the GPU tests
run; it imports the reference's Python through tests/golden/_reference.py and records what the reference computed -- none of its
text -- in tests/golden/G25_torsion_sets.npz.

Every record comes from a real ``csearch(..., mode=2)`` call (tscode/torsion_module.py:523-653).  Note-taking wrappers installed in
the imported module record what ``_get_hydrogen_bonds``, ``get_double_bonds_indices`` and ``_get_torsions`` returned and what
``random_csearch`` was handed (the torsions after ``sort_torsion``, the graph); for Parts A/B ``random_csearch`` is replaced by
one that records and returns nothing, for Part C the real one runs.

Molecules are built here by hand (internal coordinates, ideal angles) from H, C, N, O and bonded by the reference's own graphize:
  a  4-hydroxybutanal: extended, folded so that O-H...O closes a ring, and two more folds
  b  acetic acid + methanol: held by a hydrogen bond, pulled apart, connected only through a constraint pair; both modes
  c  N-methylacetamide, N,N-dimethylacetamide, methyl acetate in two numberings (atom 1 next to the ester oxygen, and not)
  d  two waters: first candidate hydrogen fails and the second passes; both pass; a hydrogen that is a neighbour only through a
     constraint pair
  e  HO-(CH2)20-CHO + water, 68 atoms (two words per row), numbered along the chain
  f  molecule a and complex b with constraint lists that reach one and two entries from i2
  g  ethane (no rotatable bond)

Guard band: a pose is drawn again (random poses; the seed is recorded) or refused (hand-made poses) when a pair distance lies
within 1e-9 of d_min, d_max, a bond threshold or a double-bond threshold, when the two projections or the two lengths compared
for a candidate hydrogen lie within 1e-9 of each other, or an alfa within 1e-6 degrees of max_angle; Part C uses the margin rule
of gen_csearch_multi.py at the clash threshold.

Usage:  python -B tests/golden/gen_torsion_sets.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _reference as R                      # noqa: E402

R.install_standins(full=True)
import networkx as nx                       # noqa: E402

if not hasattr(nx, "from_numpy_matrix"):    # networkx 3.x renamed it; the reference was written for 2.x
    nx.from_numpy_matrix = nx.from_numpy_array

import tscode.torsion_module as ref_tm      # noqa: E402
from tscode.algebra import all_dists        # noqa: E402
from tscode.errors import SegmentedGraphError   # noqa: E402
from tscode.graph_manipulations import d_min_bond, graphize   # noqa: E402

OUT = os.path.join(HERE, "G25_torsion_sets.npz")
QUIET = dict(logfunction=lambda *a, **k: None, interactive_print=False)
D_MIN, D_MAX, MAX_ANGLE = 2.5, 3.3, 45.0
DIST_BAND, ANGLE_BAND = 1e-9, 1e-6


# ------------------------------------------------------------------------------------------------------- geometry
def _unit(v):
    return v / np.linalg.norm(v)


def place(pa, pb, pc, r, theta, phi):
    """A point at distance r from pa, angle theta (deg) to pb, dihedral phi (deg) about pa-pb with respect to pc."""
    th, ph = np.radians(theta), np.radians(phi)
    bc = _unit(pa - pb)
    nv = _unit(np.cross(pb - pc, bc))
    m = np.array([bc, np.cross(nv, bc), nv])
    d = np.array([-r * np.cos(th), r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph)])
    return pa + d @ m


class Mol:
    def __init__(self):
        self.z, self.x, self.bonds = [], [], []

    def add(self, z, pos, to=None):
        self.z.append(z), self.x.append(np.asarray(pos, dtype=float))
        if to is not None:
            self.bonds.append((to, len(self.z) - 1))
        return len(self.z) - 1

    def chain(self, z, a, b, c, r, theta, phi):
        return self.add(z, place(self.x[a], self.x[b], self.x[c], r, theta, phi), a)

    def hydrogens(self, at, count, r=1.09):
        """Fill atom `at` up to a tetrahedron (or, with count == 1 on two neighbours in a plane, a trigonal site)."""
        nb = [b if a == at else a for a, b in self.bonds if at in (a, b)]
        u = [_unit(self.x[j] - self.x[at]) for j in nb]
        out = []
        if len(u) == 3 or (len(u) == 2 and count == 1):
            out.append(-_unit(np.sum(u, axis=0)))
        elif len(u) == 2:
            mid, side = -_unit(u[0] + u[1]), _unit(np.cross(u[0], u[1]))
            out += [np.cos(np.radians(54.75)) * mid + s * np.sin(np.radians(54.75)) * side for s in (1.0, -1.0)]
        else:
            w = u[0]
            e1 = _unit(np.cross(w, [0.3, 0.5, 0.8]))
            e2 = np.cross(w, e1)
            th = np.radians(109.47)
            out += [np.cos(th) * w + np.sin(th) * (np.cos(p) * e1 + np.sin(p) * e2) for p in np.radians([30.0, 150.0, 270.0])[:count]]
        return [self.add(1, self.x[at] + r * d, at) for d in out]

    def arrays(self, order=None):
        z, x = np.array(self.z), np.array(self.x)
        if order is not None:
            z, x = z[order], x[order]
        return z, x


def hydroxybutanal(t):
    """HO-CH2-CH2-CH2-CHO, torsions t[0..3] (deg).  Atoms: O0 H1 C2 C3 C4 C5 O6 H7, then the CH2 hydrogens."""
    m = Mol()
    o = m.add(8, [0.0, 0.0, 0.0])
    h = m.add(1, [0.96, 0.0, 0.0], o)
    c1 = m.add(6, place(m.x[o], m.x[h], np.array([0.0, 1.0, 0.0]), 1.43, 108.0, 0.0), o)
    c2 = m.chain(6, c1, o, h, 1.53, 109.5, t[0])
    c3 = m.chain(6, c2, c1, o, 1.53, 109.5, t[1])
    c4 = m.chain(6, c3, c2, c1, 1.51, 109.5, t[2])
    m.chain(8, c4, c3, c2, 1.21, 124.0, t[3])
    m.chain(1, c4, c3, c2, 1.10, 116.0, t[3] + 180.0)
    for c in (c1, c2, c3):
        m.hydrogens(c, 2)
    return m.arrays()


def long_chain(n_ch2=20):
    """HO-(CH2)n-CHO, all anti, numbered along the chain (O H, then C H H per methylene, then C O H), plus a water whose oxygen
    accepts the hydroxyl's hydrogen."""
    m = Mol()
    o = m.add(8, [0.0, 0.0, 0.0])
    h = m.add(1, [0.96, 0.0, 0.0], o)
    c = m.add(6, place(m.x[o], m.x[h], np.array([0.0, 1.0, 0.0]), 1.43, 108.0, 0.0), o)
    back = [c, o, h]
    carbons = [c]
    for _ in range(n_ch2 - 1):
        c = m.chain(6, back[0], back[1], back[2], 1.53, 111.0, 180.0)
        back = [c, back[0], back[1]]
        carbons.append(c)
    cho = m.chain(6, back[0], back[1], back[2], 1.51, 111.0, 180.0)
    oc = m.chain(8, cho, back[0], back[1], 1.21, 124.0, 0.0)
    hc = m.chain(1, cho, back[0], back[1], 1.10, 116.0, 180.0)
    hs = {c: m.hydrogens(c, 2) for c in carbons}
    order = [o, h]
    for c in carbons:
        order += [c] + hs[c]
    order += [cho, oc, hc]
    z, x = m.arrays(order)
    # water: O at 2.8 A along the hydroxyl O-H, its hydrogens pointing away
    ow = x[0] + 2.8 * _unit(x[1] - x[0]) + np.array([0.0, 0.05, 0.08])
    away = _unit(ow - x[0])
    e1 = _unit(np.cross(away, [0.0, 0.0, 1.0]))
    hw = [ow + 0.96 * (np.cos(np.radians(52.0)) * away + s * np.sin(np.radians(52.0)) * e1) for s in (1.0, -1.0)]
    return np.concatenate([z, [8, 1, 1]]), np.concatenate([x, [ow], hw])


def acetic_acid():
    """CH3-COOH.  Atoms: C0(methyl) C1 O2(=O) O3 H4(acid), methyl hydrogens 5 6 7."""
    m = Mol()
    c0 = m.add(6, [0.0, 0.0, 0.0])
    c1 = m.add(6, [1.50, 0.0, 0.0], c0)
    m.add(8, place(m.x[c1], m.x[c0], np.array([0.0, 0.0, 1.0]), 1.21, 125.0, 0.0), c1)
    o3 = m.add(8, place(m.x[c1], m.x[c0], np.array([0.0, 0.0, 1.0]), 1.35, 112.0, 180.0), c1)
    m.chain(1, o3, c1, c0, 0.97, 107.0, 180.0)
    m.hydrogens(c0, 3)
    return m.arrays()


def methanol():
    """CH3-OH.  Atoms: C0 O1 H2(hydroxyl), methyl hydrogens 3 4 5."""
    m = Mol()
    c = m.add(6, [0.0, 0.0, 0.0])
    o = m.add(8, [1.43, 0.0, 0.0], c)
    m.add(1, place(m.x[o], m.x[c], np.array([0.0, 0.0, 1.0]), 0.96, 108.0, 60.0), o)
    m.hydrogens(c, 3)
    return m.arrays()


def _rand_rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, a, b, c = q
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                     [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                     [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]])


def complex_pose(rng, distance):
    """Acetic acid + methanol: the methanol oxygen `distance` A from the acid's hydroxyl oxygen, along its O-H, turned at random."""
    za, xa = acetic_acid()
    zm, xm = methanol()
    target = xa[3] + distance * _unit(xa[4] - xa[3])
    xm = (xm - xm[1]) @ _rand_rot(rng).T + target
    return np.concatenate([za, zm]), np.concatenate([xa, xm])


def amide(tertiary):
    """CH3-CO-NH-CH3 or CH3-CO-N(CH3)2.  Atoms: C0 C1 O2 N3 C4 [C5 | H5], then the methyl hydrogens."""
    m = Mol()
    c0 = m.add(6, [0.0, 0.0, 0.0])
    c1 = m.add(6, [1.51, 0.0, 0.0], c0)
    m.add(8, place(m.x[c1], m.x[c0], np.array([0.0, 0.0, 1.0]), 1.23, 121.0, 0.0), c1)
    n3 = m.add(7, place(m.x[c1], m.x[c0], np.array([0.0, 0.0, 1.0]), 1.35, 116.0, 180.0), c1)
    c4 = m.chain(6, n3, c1, c0, 1.45, 122.0, 180.0)
    if tertiary:
        c5 = m.chain(6, n3, c1, c0, 1.45, 119.0, 0.0)
    else:
        m.chain(1, n3, c1, c0, 1.01, 119.0, 0.0)
    for c in (c0, c4) + ((c5,) if tertiary else ()):
        m.hydrogens(c, 3)
    return m.arrays()


def methyl_acetate(order):
    """CH3-CO-O-CH3.  Built as C0 C1 O2(=O) O3(ester) C4, methyl hydrogens 5 .. 10; `order` renumbers."""
    m = Mol()
    c0 = m.add(6, [0.0, 0.0, 0.0])
    c1 = m.add(6, [1.50, 0.0, 0.0], c0)
    m.add(8, place(m.x[c1], m.x[c0], np.array([0.0, 0.0, 1.0]), 1.21, 125.0, 0.0), c1)
    o3 = m.add(8, place(m.x[c1], m.x[c0], np.array([0.0, 0.0, 1.0]), 1.35, 111.0, 180.0), c1)
    c4 = m.chain(6, o3, c1, c0, 1.44, 115.0, 180.0)
    for c in (c0, c4):
        m.hydrogens(c, 3)
    return m.arrays(order)


def water_pair(a_deg, first_away, b_deg):
    """O0 H1 H2, O3 H4 H5 in a plane, the oxygens 2.8 A apart.  One hydrogen of O0 lies a_deg off the O...O axis (H2 when
    first_away, else H1), the other 104.5 deg further; H4 of O3 lies b_deg off the axis back towards O0, on the other side."""
    o0, o3 = np.zeros(3), np.array([2.8, 0.0, 0.0])

    def h(origin, sign, deg):
        t = np.radians(deg)
        return origin + 0.96 * np.array([sign * np.cos(t), np.sin(t), 0.0])
    near, far = h(o0, 1.0, a_deg), h(o0, 1.0, a_deg + 104.5)
    h1, h2 = (far, near) if first_away else (near, far)
    h4, h5 = h(o3, -1.0, -b_deg), h(o3, -1.0, -b_deg - 104.5)
    return np.array([8, 1, 1, 8, 1, 1]), np.array([o0, h1, h2, o3, h4, h5])


def ethane():
    m = Mol()
    c0 = m.add(6, [0.0, 0.0, 0.0])
    c1 = m.add(6, [1.53, 0.0, 0.0], c0)
    m.hydrogens(c0, 3), m.hydrogens(c1, 3)
    return m.arrays()


# ------------------------------------------------------------------------------------------------------- guard band
def guard_ok(z, x, pairs):
    """True when no quantity the reference (or the kernels) compares lies inside the guard band of the module docstring.  Every
    hetero pair in range is looked at with EVERY hydrogen of the structure: a superset of the candidates any neighbour list holds."""
    n = len(z)
    d = all_dists(x, x)
    for i in range(n):
        for j in range(i + 1, n):
            bounds = [d_min_bond(z[i], z[j])]
            if {z[i], z[j]} <= {7, 8}:
                bounds += [D_MIN, D_MAX]
            if (z[i], z[j]) == (6, 6):
                bounds.append(1.4)
            if sorted((z[i], z[j])) == [6, 7]:
                bounds.append(1.3)
            if min(abs(d[i, j] - b) for b in bounds) < DIST_BAND:
                return False
    het = [i for i in range(n) if z[i] in (7, 8)]
    for a, i1 in enumerate(het):
        for i2 in het[a + 1:]:
            if not D_MIN < d[i1, i2] < D_MAX:
                continue
            u = _unit(x[i2] - x[i1])
            for h in np.flatnonzero(z == 1):
                v1, v2 = x[h] - x[i1], x[h] - x[i2]
                l1, l2 = v1 @ u, v2 @ -u
                alfa = np.degrees(np.arccos(np.clip(_unit(v1) @ u if l1 < l2 else _unit(v2) @ -u, -1.0, 1.0)))
                if abs(l1 - l2) < DIST_BAND or abs(d[i1, h] - d[i2, h]) < DIST_BAND or abs(alfa - MAX_ANGLE) < ANGLE_BAND:
                    return False
    return True


# ------------------------------------------------------------------------------------------------------- reference runs
def edges_of(graph):
    return sorted((int(min(a, b)), int(max(a, b))) for a, b in graph.edges if a != b)


class Notes:
    """Wrappers around the helpers csearch calls, installed in the imported module; ``run_search`` False replaces random_csearch
    by a recorder that returns nothing (and draws no random number)."""

    NAMES = ("_get_hydrogen_bonds", "get_double_bonds_indices", "_get_torsions", "random_csearch", "rotate_dihedral", "torsion_comp_check")

    def __init__(self, run_search):
        self.run_search = run_search
        self.real = {k: getattr(ref_tm, k) for k in self.NAMES}
        self.margin = np.inf
        self.reset()

    def reset(self):
        self.hb, self.double, self.torsions, self.folds, self.masks, self.n_torsions_found = [], None, [], [], [], None

    def __enter__(self):
        real = self.real

        def hbonds(*a, **k):
            out = real["_get_hydrogen_bonds"](*a, **k)
            self.hb += [[int(p), int(q)] for p, q in out]
            return out

        def double(*a, **k):
            out = real["get_double_bonds_indices"](*a, **k)
            self.double = [[int(p), int(q)] for p, q in out]
            return out

        def torsions(*a, **k):
            out = real["_get_torsions"](*a, **k)
            self.n_torsions_found = len(out)
            return out

        def search(coords, atomnos, tors, graph, **k):
            self.torsions = [[int(i) for i in t.torsion] for t in tors]          # after sort_torsion (:614-615)
            self.folds = [int(t.n_fold) for t in tors]
            self.masks = [np.array(ref_tm._get_rotation_mask(graph, t.torsion)) for t in tors]
            if self.run_search:
                return real["random_csearch"](coords, atomnos, tors, graph, **k)
            return np.zeros((0, len(coords), 3))

        def rd(coords, dihedral, angle, mask=None, indices_to_be_moved=None):
            return real["rotate_dihedral"](coords, dihedral, angle, mask=mask, indices_to_be_moved=indices_to_be_moved)

        def cc(coords, torsion, mask, thresh=1.5, max_clashes=0):
            anti = ~mask
            anti[torsion[1]] = anti[torsion[2]] = False
            if mask.any() and anti.any():
                self.margin = min(self.margin, float(np.abs(all_dists(coords[anti], coords[mask]) - thresh).min()))
            return real["torsion_comp_check"](coords, torsion=torsion, mask=mask, thresh=thresh, max_clashes=max_clashes)

        for name, f in zip(self.NAMES, (hbonds, double, torsions, search, rd, cc)):
            setattr(ref_tm, name, f)
        return self

    def __exit__(self, *exc):
        for k, f in self.real.items():
            setattr(ref_tm, k, f)


def call_csearch(x, z, pairs, keep_hb, n_out):
    ci = np.array(pairs, dtype=int).reshape(-1, 2) if len(pairs) else None
    return ref_tm.csearch(x.copy(), z, constrained_indices=ci, keep_hb=keep_hb, mode=2, n_out=n_out, title="g25", **QUIET)


def record(name, z, x, pairs, keep_hb):
    """One structure through the reference's csearch set-up; returns its record (JSON-able) and its masks."""
    assert guard_ok(z, x, pairs), f"{name}: inside the guard band"
    bonds = edges_of(graphize(x, z))
    with Notes(run_search=False) as notes:
        try:
            call_csearch(x, z, pairs, keep_hb, 1)
            segmented = False
        except SegmentedGraphError:
            segmented = True
    rec = {"name": name, "keep_hb": bool(keep_hb), "pairs": [[int(a), int(b)] for a, b in pairs], "bonds": bonds, "segmented": segmented,
           "hydrogen_bonds": notes.hb, "double_bonds": notes.double if notes.double is not None else [],
           "torsions": notes.torsions, "n_folds": notes.folds}
    masks = np.array(notes.masks, dtype=bool).reshape(len(notes.torsions), len(z))
    print(f"  {name:28s} keep_hb={int(keep_hb)} pairs={rec['pairs']} hb={notes.hb} segmented={segmented} "
          f"torsions={[(t, f) for t, f in zip(notes.torsions, notes.folds)]}")
    return rec, masks


def reach_counts(z, x, rec):
    """Per recorded torsion, how many entries of the flattened constraint list its ORIGINAL i2 reaches with i2-i3 cut (generator's
    own check that case f holds a flip and a flip back)."""
    g = nx.Graph(rec["bonds"] + rec["pairs"] + rec["hydrogen_bonds"])
    g.add_nodes_from(range(len(z)))
    flat = [i for p in rec["pairs"] for i in p]
    out = []
    for t in rec["torsions"]:
        h = g.copy()
        h.remove_edge(t[1], t[2])
        c = [sum(nx.has_path(h, end, d) for d in flat) for end in (t[1], t[2])]
        out.append(c)
    return out


def main():
    print("G25 torsion sets: the reference's csearch set-up and augmentation loop")
    structures = []                  # (case, z, x, pairs, keep_hb)
    meta = {"cases": {}, "seeds": {}}

    # ---- a: 4-hydroxybutanal
    ext = hydroxybutanal([180.0, 180.0, 180.0, 180.0])
    bonds_ext = edges_of(graphize(ext[1], ext[0]))
    a_poses = [("a_extended", ext[1])]
    seed, folded = 2500, None
    while len(a_poses) < 4:
        rng = np.random.default_rng(seed)
        z, x = hydroxybutanal(rng.uniform(0.0, 360.0, size=4))
        seed += 1
        if edges_of(graphize(x, z)) != bonds_ext or not guard_ok(z, x, []) or np.min(all_dists(x, x) + 10 * np.eye(len(z))) < 0.9:
            continue
        hb = ref_tm._get_hydrogen_bonds(x, z, graphize(x, z))
        if folded is None and not hb:
            continue                                                            # the first random pose has to be the folded one
        folded = True
        a_poses.append((f"a_fold_seed{seed - 1}", x))
    for name, x in a_poses:
        structures.append(("a", name, ext[0], x, [], True))
    structures.append(("a", "a_extended_link", ext[0], ext[1], [], False))

    # ---- b: acid + alcohol
    for tag, dist, seed0 in (("hb", 2.75, 2510), ("apart", 8.0, 2520), ("hb2", 2.9, 2530)):
        seed = seed0
        while True:
            z, x = complex_pose(np.random.default_rng(seed), dist)
            za = len(acetic_acid()[0])
            inter = all_dists(x[:za], x[za:])
            if guard_ok(z, x, []) and np.sum(inter < 2.2) <= (1 if dist < 4 else 0) and len(edges_of(graphize(x, z))) == 12:
                break
            seed += 1
        meta["seeds"][f"b_{tag}"] = seed
        for keep_hb in (True, False):
            structures.append(("b", f"b_{tag}", z, x, [], keep_hb))
        if tag == "apart":
            for keep_hb in (True, False):
                structures.append(("b", "b_apart_constrained", z, x, [(1, 9)], keep_hb))       # acid C1 - methanol O
    # ---- c: amides and the ester in two numberings
    for name, (z, x) in (("c_sec_amide", amide(False)), ("c_tert_amide", amide(True)),
                         ("c_ester_o_next_to_1", methyl_acetate([3, 1, 0, 2, 4, 5, 6, 7, 8, 9, 10])),
                         ("c_ester_plain", methyl_acetate([0, 5, 1, 2, 3, 4, 6, 7, 8, 9, 10]))):
        structures.append(("c", name, z, x, [], True))
    # ---- d: two candidate hydrogens
    z, x = water_pair(12.0, True, 75.0)
    structures.append(("d", "d_second_passes", z, x, [], True))
    z, x = water_pair(12.0, False, 20.0)
    structures.append(("d", "d_both_pass", z, x, [], True))
    z, x = water_pair(60.0, False, 20.0)
    structures.append(("d", "d_constraint_h_first", z, x, [(0, 4)], True))      # H4 joins O0's list through the constraint pair
    structures.append(("d", "d_constraint_h_last", z, x, [(3, 1)], True))
    # ---- e: more than 64 atoms
    z, x = long_chain()
    assert len(z) > 64
    structures.append(("e", "e_long_chain", z, x, [], True))
    structures.append(("e", "e_long_chain_constrained", z, x, [(62, 64), (5, 2)], True))
    # ---- f: constraint lists that reach one and two entries
    z, x = ext
    structures.append(("f", "f_one_entry", z, x, [(2, 3)], True))
    structures.append(("f", "f_two_entries", z, x, [(0, 1), (1, 0)], True))
    structures.append(("f", "f_far_pair", z, x, [(6, 7)], True))
    # ---- g: no rotatable bond
    z, x = ethane()
    structures.append(("g", "g_ethane", z, x, [], True))

    data, records = {}, []
    for k, (case, name, z, x, pairs, keep_hb) in enumerate(structures):
        rec, masks = record(name, z, x, pairs, keep_hb)
        rec["case"], rec["index"] = case, k
        if case == "f" or name.endswith("constrained"):
            rec["reach_counts"] = reach_counts(z, x, rec)
            print(f"      entries reached from (i2, i3): {rec['reach_counts']}")
        records.append(rec)
        data[f"s{k}_atomnos"], data[f"s{k}_coords"], data[f"s{k}_masks"] = z.astype(np.int32), x, masks
    by = {r["name"] + str(int(r["keep_hb"])): r for r in records}
    assert by["a_extended1"]["hydrogen_bonds"] == [] and len(by[a_poses[1][0] + "1"]["hydrogen_bonds"]) >= 1
    assert len(by[a_poses[1][0] + "1"]["torsions"]) < len(by["a_extended1"]["torsions"])
    assert by["b_apart1"]["segmented"] and by["b_apart0"]["segmented"] and not by["b_hb0"]["segmented"] and not by["b_apart_constrained1"]["segmented"]
    assert by["d_second_passes1"]["hydrogen_bonds"] == [[2, 3]] and by["d_both_pass1"]["hydrogen_bonds"] == [[1, 3]]
    assert by["g_ethane1"]["torsions"] == [] and not by["g_ethane1"]["segmented"]
    assert any(max(t) >= 64 and min(t) < 64 for t in by["e_long_chain1"]["torsions"]) and by["e_long_chain1"]["hydrogen_bonds"]

    # ---- Part C: the augmentation loop, one np.random.seed per case
    part_c = []
    for cname, names, n_out, seed0 in (("c_a", [p[0] for p in a_poses], 6, 25100),
                                       ("c_b", ["b_hb", "b_apart", "b_apart_constrained", "b_hb2"], 4, 25200),
                                       ("c_mixed", ["g_ethane", "c_sec_amide", "c_ester_plain"], 5, 25300)):
        members = [by[nm + "1"] for nm in names]
        for seed in range(seed0, seed0 + 50):
            outs = []
            with Notes(run_search=True) as notes:
                np.random.seed(seed)
                for r in members:
                    k = r["index"]
                    try:
                        outs.append(np.asarray(call_csearch(data[f"s{k}_coords"], data[f"s{k}_atomnos"], r["pairs"], True, n_out), dtype=np.float64))
                    except SegmentedGraphError:
                        outs.append(np.zeros((0, len(data[f"s{k}_atomnos"]), 3)))
            if notes.margin > 1e-9:
                break
        else:
            raise SystemExit(f"{cname}: no seed outside the clash margin")
        sizes = {len(data[f"s{r['index']}_atomnos"]) for r in members}
        entry = {"name": cname, "members": [r["index"] for r in members], "n_out": n_out, "seed": seed, "counts": [len(o) for o in outs],
                 "margin": notes.margin, "same_atoms": len(sizes) == 1}
        for j, o in enumerate(outs):
            data[f"{cname}_out{j}"] = o.reshape(len(o), len(data[f"s{members[j]['index']}_atomnos"]), 3)
        part_c.append(entry)
        print(f"  part C {cname}: seed {seed}, kept {entry['counts']}, margin {notes.margin:.3e}")
    meta["structures"], meta["part_c"] = records, part_c
    meta["thresholds"] = {"d_min": D_MIN, "d_max": D_MAX, "max_angle": MAX_ANGLE}
    data["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **data)
    print(f"  wrote {OUT}  ({os.path.getsize(OUT) / 1024:.1f} KiB)")
    assert os.path.getsize(OUT) < 1024 * 1024


if __name__ == "__main__":
    main()
