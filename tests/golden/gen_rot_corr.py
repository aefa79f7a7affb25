"""G19: the reference's prune_conformers_rmsd_rot_corr (tscode/torsion_module.py:953-1161), case by case.

BUILD CONTAINER ONLY (imports the reference through tests/golden/_reference.py).  Two molecules built here and bonded by the
reference's own graphize carry heavy-atom dummy rotors of different fold (molecule A: tBu-CH2-CH2-CF3, 3-fold tBu and CF3;
molecule B: Ph-C6H4-CH2-CH2-C(CF3)3, the 2-fold biphenyl flip, a Car-Csp3 rotor and the nested C(CF3)3) and one real torsion
(the CH2-CH2 bond) whose values make the clusters; molecule C (n-butane) has no heavy dummy rotor (the early return).

ASSUMPTION, not pinned by anything in this image: the reference calls rmsd.kabsch_rmsd (the `rmsd` package, setup.py pins
rmsd==1.4), which is not installed here.  It is restated below from that release: C = P^T Q, SVD, the sign of V[:, -1] flipped
when det(V) det(W) < 0, P rotated by V W, sqrt(sum d^2 / n), no translation (translate=False).

Ensembles: the clusters' real torsion values, every dummy rotor turned by a random multiple of its 360/fold plus a Gaussian
jitter, a random rigid rotation, Gaussian noise, shuffled.  While the reference runs, note-taking wrappers around its helpers
record what the drop-in's set-up gets from them (tscode_amd.rot_corr reads the same helpers of a live TSCoDe), and wrappers
around kabsch_rmsd / rotate_dihedral / rotationally_corrected_rmsd record every evaluated pair.  Guard band: a case is drawn
again (the seed recorded) when an evaluated pair's rmsd lies within 1e-7 of max_rmsd or two angles of a torsion search lie
within 1e-9 of each other without being equal (equal values come from bit-identical inputs -- a rotor whose moving heavy atoms
lie outside its local subgraph -- and the first angle wins in any implementation).

Usage:  python -B tests/golden/gen_rot_corr.py
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _reference as R  # noqa: E402

R.install_standins(full=True)
import networkx as nx  # noqa: E402
if not hasattr(nx, "from_numpy_matrix"):
    nx.from_numpy_matrix = nx.from_numpy_array


def kabsch_rmsd(P, Q, W=None, translate=False):
    """rmsd 1.4 kabsch_rmsd(P, Q) with translate=False: P rotated onto Q (see the module docstring)."""
    C = P.T @ Q
    V, S, Wt = np.linalg.svd(C)
    if (np.linalg.det(V) * np.linalg.det(Wt)) < 0.0:
        S[-1] = -S[-1]
        V[:, -1] = -V[:, -1]
    U = V @ Wt
    d = P @ U - Q
    return np.sqrt((d * d).sum() / P.shape[0])


sys.modules["rmsd"].kabsch_rmsd = kabsch_rmsd
import tscode.torsion_module as tm  # noqa: E402
from tscode.graph_manipulations import graphize  # noqa: E402

OUT = {"a": os.path.join(HERE, "G19a_rot_corr.npz"), "b": os.path.join(HERE, "G19b_rot_corr.npz")}    # (each under 1 MiB)
RMSD_BAND, ANGLE_BAND = 1e-7, 1e-9


# ------------------------------------------------------------------------------------------------------- geometry
def _unit(v):
    return v / np.linalg.norm(v)


def _perp(w):
    a = np.array([1.0, 0.0, 0.0]) if abs(w[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = _unit(np.cross(w, a))
    return e1, np.cross(w, e1)


def _tetra(p, back, length, m, phi0=0.0):
    """m substituent positions on atom p, 109.47 deg from the bond to `back`, 120 deg apart about it."""
    w = _unit(back - p)
    e1, e2 = _perp(w)
    th = np.radians(109.47)
    out = []
    for s in range(m):
        phi = np.radians(phi0 + 120.0 * s)
        out.append(p + length * (np.cos(th) * w + np.sin(th) * (np.cos(phi) * e1 + np.sin(phi) * e2)))
    return out


class Builder:
    def __init__(self):
        self.z, self.x, self.bonds = [], [], []

    def add(self, z, pos, bonded_to=None):
        self.z.append(z)
        self.x.append(np.asarray(pos, dtype=float))
        if bonded_to is not None:
            self.bonds.append((bonded_to, len(self.z) - 1))
        return len(self.z) - 1

    def ring(self, centre, radius_dir, normal, first_bonded=None):
        """Six aromatic C on a hexagon (1.39 A) in the plane normal to `normal`, atom 0 along radius_dir."""
        e1 = _unit(radius_dir)
        e2 = np.cross(_unit(normal), e1)
        ids = []
        for s in range(6):
            a = np.radians(60.0 * s)
            ids.append(self.add(6, centre + 1.39 * (np.cos(a) * e1 + np.sin(a) * e2)))
        for s in range(6):
            self.bonds.append((ids[s], ids[(s + 1) % 6]))
        if first_bonded is not None:
            self.bonds.append((first_bonded, ids[0]))
        return ids

    def finish(self):
        """Heavy atoms first, hydrogens last (the reference's quadruplet search then starts its paths on heavy atoms)."""
        order = sorted(range(len(self.z)), key=lambda i: (self.z[i] == 1, i))
        new = {o: k for k, o in enumerate(order)}
        z = np.array([self.z[o] for o in order])
        x = np.array([self.x[o] for o in order])
        bonds = sorted(tuple(sorted((new[a], new[b]))) for a, b in self.bonds)
        return z, x, bonds


def mol_a():
    """tBu-CH2-CH2-CF3."""
    b = Builder()
    c1 = b.add(6, [0.0, 0.0, 0.0])
    c2 = b.add(6, [1.54, 0.0, 0.0], c1)
    subs1 = _tetra(b.x[c1], b.x[c2], 1.54, 3, 0.0)
    cq = b.add(6, subs1[0], c1)
    for p in subs1[1:]:
        b.add(1, _unit(p - b.x[c1]) * 1.09 + b.x[c1], c1)
    subs2 = _tetra(b.x[c2], b.x[c1], 1.52, 3, 0.0)              # (anti to the tBu)
    cf = b.add(6, subs2[0], c2)
    for p in subs2[1:]:
        b.add(1, _unit(p - b.x[c2]) * 1.09 + b.x[c2], c2)
    for p in _tetra(b.x[cf], b.x[c2], 1.35, 3, 30.0):
        b.add(9, p, cf)
    for p in _tetra(b.x[cq], b.x[c1], 1.54, 3, 60.0):
        cm = b.add(6, p, cq)
        for h in _tetra(b.x[cm], b.x[cq], 1.09, 3, 0.0):
            b.add(1, h, cm)
    return b.finish()


def mol_b():
    """Ph-C6H4-CH2-CH2-C(CF3)3."""
    b = Builder()
    x = np.array([1.0, 0.0, 0.0])
    r2 = b.ring(np.zeros(3), -x, x * 0 + np.array([0.0, 0.0, 1.0]))             # C6H4: atom 0 ipso (-x), atom 3 para (+x)
    tw = np.radians(40.0)
    r1 = b.ring(-x * (1.39 + 1.48 + 1.39), x, np.array([0.0, -np.sin(tw), np.cos(tw)]), first_bonded=r2[0])
    for ring, skip in ((r2, (0, 3)), (r1, (0,))):
        c = np.mean([b.x[i] for i in ring], axis=0)
        for s, i in enumerate(ring):
            if s not in skip:
                b.add(1, b.x[i] + 1.08 * _unit(b.x[i] - c), i)
    ca = b.add(6, b.x[r2[3]] + 1.51 * x, r2[3])
    sa = _tetra(b.x[ca], b.x[r2[3]], 1.54, 3, 90.0)
    cb = b.add(6, sa[0], ca)
    for p in sa[1:]:
        b.add(1, _unit(p - b.x[ca]) * 1.09 + b.x[ca], ca)
    sb = _tetra(b.x[cb], b.x[ca], 1.54, 3, 0.0)
    cq = b.add(6, sb[0], cb)
    for p in sb[1:]:
        b.add(1, _unit(p - b.x[cb]) * 1.09 + b.x[cb], cb)
    for p in _tetra(b.x[cq], b.x[cb], 1.56, 3, 60.0):
        cf = b.add(6, p, cq)
        for f in _tetra(b.x[cf], b.x[cq], 1.35, 3, 0.0):
            b.add(9, f, cf)
    return b.finish()


def mol_c():
    """n-butane: its only rotors are methyls (quadruplets with H: no heavy dummy torsion)."""
    b = Builder()
    c1 = b.add(6, [0.0, 0.0, 0.0])
    c2 = b.add(6, [1.54, 0.0, 0.0], c1)
    s1 = _tetra(b.x[c1], b.x[c2], 1.54, 3, 0.0)
    c0 = b.add(6, s1[0], c1)
    for p in s1[1:]:
        b.add(1, p * 0 + _unit(p - b.x[c1]) * 1.09 + b.x[c1], c1)
    s2 = _tetra(b.x[c2], b.x[c1], 1.54, 3, 180.0)
    c3 = b.add(6, s2[0], c2)
    for p in s2[1:]:
        b.add(1, _unit(p - b.x[c2]) * 1.09 + b.x[c2], c2)
    for cm, back in ((c0, c1), (c3, c2)):
        for h in _tetra(b.x[cm], b.x[back], 1.09, 3, 60.0):
            b.add(1, h, cm)
    return b.finish()


def _side(bonds, n, a, b):
    """bool[n]: the atoms on b's side of the a-b bond."""
    g = nx.Graph(bonds)
    g.add_nodes_from(range(n))
    g.remove_edge(a, b)
    m = np.zeros(n, bool)
    m[list(nx.node_connected_component(g, b))] = True
    return m


def _turn(x, mask, a, b, deg):
    """x with the masked atoms turned by deg about the a -> b axis through b (plain NumPy, no reference code)."""
    k = _unit(x[b] - x[a])
    t = np.radians(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    y = x.copy()
    y[mask] = (x[mask] - x[b]) @ Rm.T + x[b]
    return y


def _rand_rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, a, b, c = q
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                     [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                     [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]])


def ensemble(rng, z, x0, bonds, real_bond, rotors, n, n_clusters, jitter=6.0, noise=0.02):
    """rotors: [(a, b, fold)] turned by random multiples of 360/fold + N(0, jitter) deg; clusters: the real bond at
    n_clusters evenly spaced values (+ N(0, 3) deg)."""
    nat = len(z)
    real_mask = _side(bonds, nat, *real_bond)
    rotor_masks = [_side(bonds, nat, a, b) for a, b, _ in rotors]
    out, labels = [], []
    for s in range(n):
        c = s % n_clusters
        x = _turn(x0, real_mask, *real_bond, 360.0 * c / n_clusters + rng.normal(0, 3.0))
        for (a, b, fold), m in zip(rotors, rotor_masks):
            x = _turn(x, m, a, b, 360.0 / fold * rng.integers(fold) + rng.normal(0, jitter))
        x = x @ _rand_rot(rng).T + rng.normal(0, 1.0, size=3)
        out.append(x + rng.normal(0, noise, size=x.shape))
        labels.append(c)
    perm = rng.permutation(n)
    return np.array(out)[perm], np.array(labels)[perm]


# ------------------------------------------------------------------------------------------------------- reference run
class Recorder:
    """Note-taking wrappers around the reference's helpers, installed in tscode.torsion_module's namespace."""

    HELPERS = ("_get_hydrogen_bonds", "_get_torsions", "_is_nondummy", "get_double_bonds_indices", "_get_rotation_mask")

    def __init__(self, trace=False):
        self.trace_on = trace
        self.calls = {h: [] for h in self.HELPERS}
        self.pairs = []              # (i, j, best angles, rmsd)
        self.local = []              # local values of the current pair
        self.rd_angles = []
        self.passes = []             # (active count, pairs evaluated before the next count)
        self.min_gap = np.inf
        self.min_thr_gap = np.inf
        self.setup = None

    def install(self, thr):
        self.thr = thr
        self.orig = {h: getattr(tm, h) for h in self.HELPERS + ("rotationally_corrected_rmsd", "kabsch_rmsd", "rotate_dihedral", "np")}
        for h in self.HELPERS:
            setattr(tm, h, self._wrap(h, self.orig[h]))
        rec = self

        def rcr(ref, coord, atomnos, torsions, graph, angles):
            base = ref.base if ref.base is not None else ref
            i = (ref.ctypes.data - base.ctypes.data) // base.strides[0]
            j = (coord.ctypes.data - base.ctypes.data) // base.strides[0]
            if rec.setup is None:
                rec.setup = {"torsions": [list(map(int, t)) for t in torsions], "angles": [list(a) for a in angles],
                             "masks": [np.array(rec.orig["_get_rotation_mask"](graph, t)) for t in torsions],
                             "subs": [rec._sub_nodes(graph, torsions, t, atomnos) for t in torsions]}
            rec.local, rec.rd_angles = [], []
            r = rec.orig["rotationally_corrected_rmsd"](ref, coord, atomnos, torsions, graph, angles)
            k, best = 0, []
            for t, a in enumerate(angles):
                vals = rec.local[k:k + len(a)]
                k += len(a)
                bi = int(np.argmin(vals))
                best.append(a[bi])
                for v in vals:
                    if v != vals[bi]:
                        rec.min_gap = min(rec.min_gap, abs(v - vals[bi]))
            assert best == rec.rd_angles[-len(torsions):], (best, rec.rd_angles[-len(torsions):])
            rec.min_thr_gap = min(rec.min_thr_gap, abs(r - rec.thr))
            rec.pairs.append((int(i), int(j), [float(b) for b in best], float(r)) if rec.trace_on else (int(i), int(j)))
            return r

        def kr(P, Q):
            v = kabsch_rmsd(P, Q)
            rec.local.append(v)
            return v

        def rd(coords, dihedral, angle, mask=None, indices_to_be_moved=None):
            rec.rd_angles.append(angle)
            return rec.orig["rotate_dihedral"](coords, dihedral, angle, mask=mask, indices_to_be_moved=indices_to_be_moved)

        class NpProxy:
            def __getattr__(self, name):
                if name == "count_nonzero":
                    def cnz(a, *args, **kw):
                        v = np.count_nonzero(a, *args, **kw)
                        if sys._getframe(1).f_code.co_name == "prune_conformers_rmsd_rot_corr":     # the gate's count (:1081)
                            rec.passes.append([int(v), len(rec.pairs)])
                        return v
                    return cnz
                return getattr(np, name)

        tm.rotationally_corrected_rmsd, tm.kabsch_rmsd, tm.rotate_dihedral, tm.np = rcr, kr, rd, NpProxy()

    def uninstall(self):
        for h, f in self.orig.items():
            setattr(tm, h, f)

    def _wrap(self, name, fn):
        def w(*args, **kw):
            out = fn(*args, **kw)
            self.calls[name].append((args, out))
            return out
        return w

    @staticmethod
    def _sub_nodes(graph, torsions, torsion, atomnos):
        g = graph.copy()
        for o in torsions:
            if o is not torsion:
                g.remove_edge(o[1], o[2])
        comp = [s for s in nx.connected_components(g) if torsion[1] in s][0]
        return [int(i) for i in comp if atomnos[i] != 1]


def run_reference(structures, atomnos, graph, thr, trace):
    rec = Recorder(trace)
    rec.install(thr)
    edges_before = sorted(map(tuple, map(sorted, graph.edges)))
    t0 = time.perf_counter()
    try:
        out, mask = tm.prune_conformers_rmsd_rot_corr(structures.copy(), atomnos, graph, max_rmsd=thr)
    finally:
        rec.uninstall()
    wall = time.perf_counter() - t0
    assert sorted(map(tuple, map(sorted, graph.edges))) == edges_before
    return rec, out, mask, wall


def helper_record(rec, n):
    """What the drop-in asks the live module, and what the reference answered (JSON)."""
    c = rec.calls
    hb = [[list(map(int, p)) for p in out] for _, out in c["_get_hydrogen_bonds"]]
    db = [[list(map(int, p)) for p in out] for _, out in c["get_double_bonds_indices"]]
    tors = [[list(map(int, t.torsion)), int(t.n_fold)] for t in c["_get_torsions"][0][1]]
    nd = [[int(a[0]), int(a[1]), bool(out)] for a, out in c["_is_nondummy"]]
    masks = {json.dumps(list(map(int, a[1]))): np.flatnonzero(out).tolist() for a, out in c["_get_rotation_mask"]}
    return {"hydrogen_bonds": hb, "double_bonds": db, "torsions": tors, "is_nondummy": nd, "rotation_masks": masks, "n_atoms": n}


def main():
    t_start = time.perf_counter()
    mols = {"A": mol_a(), "B": mol_b(), "C": mol_c()}
    data, meta, graphs = {}, {"cases": [], "molecules": {}}, {}
    for name, (z, x, bonds) in mols.items():
        g = graphize(x, z)                                             # the molecule's graph, as TSCoDe passes it
        edges = sorted(tuple(sorted(map(int, e))) for e in g.edges if e[0] != e[1])
        assert edges == bonds, (name, set(edges) ^ set(bonds))
        graphs[name] = g
        meta["molecules"][name] = {"n_atoms": len(z)}
        data[f"mol{name}_atomnos"] = z
        data[f"mol{name}_coords"] = x
    # real bond and rotors per molecule (atom indices after Builder.finish: heavy atoms in insertion order)
    spec = {"A": dict(real=(0, 1), rotors=[(0, 2, 3), (1, 3, 3)]),
            "B": dict(real=(12, 13), rotors=[(0, 6, 2), (3, 12, 3), (13, 14, 3), (14, 15, 3), (14, 19, 3), (14, 23, 3)]),
            "C": dict(real=(0, 1), rotors=[])}
    # (case, molecule, N, clusters, max_rmsd, seed, per-pair trace, file); n760 re-uses n160a's structures (index table below)
    cases = [("n40", "A", 40, 6, 0.25, 1940, True, "a"), ("n150", "B", 150, 10, 0.5, 19150, False, "a"),
             ("n400", "B", 400, 12, 0.25, 19400, False, "b"), ("n160a", "A", 160, 8, 0.5, 19160, False, "a"),
             ("n760", "A", 760, 0, 0.25, 19760, False, "a"), ("notors", "C", 60, 5, 0.25, 19060, False, "a")]
    files = {"a": data, "b": {}}
    for cname, mname, n, ncl, thr, seed, trace, fkey in cases:
        z, x0, bonds = mols[mname]
        sp = spec[mname]
        out_data = files[fkey]
        for attempt in range(20):
            rng = np.random.default_rng(seed + 1000 * attempt)
            if cname == "n760":
                src = rng.integers(0, 160, size=n)
                S, labels = data["n160a_structures"][src], data["n160a_labels"][src].astype(np.int64)
            else:
                S, labels = ensemble(rng, z, x0, bonds, sp["real"], sp["rotors"], n, ncl)
            graph = graphs[mname]
            edge_list = [tuple(map(int, e)) for e in graph.edges]
            rec, out, mask, wall = run_reference(S, z, graph, thr, trace)
            ok = rec.min_gap >= ANGLE_BAND and rec.min_thr_gap >= RMSD_BAND
            print(f"{cname}: seed {seed + 1000 * attempt}, {int(mask.sum())}/{n} kept, {len(rec.pairs)} pairs, {wall:.1f} s, "
                  f"min angle gap {rec.min_gap:.2e}, min |rmsd - thr| {rec.min_thr_gap:.2e}{'' if ok else '  -> redraw'}")
            if ok:
                break
        else:
            raise SystemExit(f"{cname}: no draw outside the guard band")
        p = f"{cname}_"
        data = out_data
        if cname == "n760":
            data[p + "from_n160a"] = src.astype(np.int16)
        else:
            data[p + "structures"] = S
        data[p + "labels"] = labels.astype(np.int16)
        data[p + "edges"] = np.array(edge_list, dtype=np.int32)
        data[p + "mask"] = mask
        centred = np.array([s_ - s_.mean(axis=0) for s_ in S])
        if rec.setup is None:                                          # early return: the centred input, bit for bit
            assert out.tobytes() == centred.tobytes()
        else:
            data[p + "out"] = out
        # per schedule slot k = 5e5 ... 1: the active count the gate saw and the pairs evaluated in that pass (0: gated off)
        before = np.array([b for _, b in rec.passes] + [len(rec.pairs)], dtype=np.int64)
        data[p + "passes"] = np.stack([np.array([a for a, _ in rec.passes], dtype=np.int64), np.diff(before)], axis=1)
        su = rec.setup
        if su is None:                                                  # early return: the helpers' answers only
            T = 0
        else:
            T = len(su["torsions"])
            data[p + "torsions"] = np.array(su["torsions"], dtype=np.int32)
            data[p + "angles"] = np.array([list(a) + [0] * (6 - len(a)) for a in su["angles"]], dtype=np.float64)
            data[p + "n_angles"] = np.array([len(a) for a in su["angles"]], dtype=np.int32)
            data[p + "move_masks"] = np.array(su["masks"], dtype=bool)
            data[p + "sub_ptr"] = np.concatenate(([0], np.cumsum([len(s) for s in su["subs"]]))).astype(np.int32)
            data[p + "sub_idx"] = np.concatenate([np.array(s, dtype=np.int32) for s in su["subs"]])
        if trace:
            data[p + "trace_pairs"] = np.array([(i, j) for i, j, _, _ in rec.pairs], dtype=np.int32)
            data[p + "trace_best"] = np.array([b for _, _, b, _ in rec.pairs], dtype=np.float64)
            data[p + "trace_rmsd"] = np.array([r for _, _, _, r in rec.pairs], dtype=np.float64)
        data = files["a"]
        meta["cases"].append({"name": cname, "file": fkey, "molecule": mname, "n": n, "clusters": ncl, "max_rmsd": thr,
                              "seed": seed + 1000 * attempt, "n_torsions": T, "reference_wall_s": round(wall, 3),
                              "helpers": helper_record(rec, len(z))})
    data["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    for key, path in OUT.items():
        np.savez_compressed(path, **files[key])
        print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")
    print(f"in {time.perf_counter() - t_start:.0f} s")


if __name__ == "__main__":
    main()
