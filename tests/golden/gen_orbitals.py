"""G23: the reference's own Hypermolecule.compute_orbitals (tscode/hypermolecule_class.py:195-217), the eight classes of
tscode/reactive_atoms_classes.py, is_sigmatropic / is_vicinal (tscode/graph_manipulations.py:231-298), Embedder._get_pivots / _set_pivots
(tscode/embedder.py:542-621) and orb_dim_dict (tscode/parameters.py:19-53), case by case; and one chain: two conformer ensembles given as
coordinates, through the reference's cyclical_embed.

BUILD CONTAINER ONLY (imports the reference through tests/golden/_reference.py, which exists only there).  No test imports it.

Molecules: the reference's tscode/tests/CH3Cl.xyz, HCOOH.xyz and C2H4.xyz, read as data, and small hand-built ones (MOLECULES below).
Conformer 0 of a case is the molecule as built (its bond graph is the graph of the case: hypermolecule_class.py:185); the others add
Gaussian noise of the case's sigma to every coordinate.  Coordinates are handed to the classes as they are: a Hypermolecule is assembled
from arrays here, without the centroid shift of its file constructor (:179-184).  The loop of compute_orbitals (:212-214) is walked here
with NumPy's generator re-seeded before every init(update=True), so that the one random draw of the 'sp' class (:495) is the same recorded
vector in every conformer.

Every array of a case is stored as "<case>/<name>" in G23a_orbitals.npz (the chain: G23b); G23_orbitals.json is the index and also holds
the class names per conformer, the neighbour lists, orb_dim_dict and the reference's seconds per conformer (a measurement: the one field a
rerun may write differently; every other byte is the same).

Conditions asserted here (tests/test_orbitals.py asserts them again on the files), judged by the NumPy restatement of that test file, which
is first checked against the reference's arrays: no NaN; no angle within 1e-6 degrees of 175; no reactive-pair distance within 1e-9 A of
3 A; at least 1e-6 A between the 2nd and 3rd shortest of four pivots; no pivot length between 1e-6 and 1e-4 A above the shortest under
sigma-star; every normalised vector at least 1e-3 of the product of its operands' lengths; in the allene and diimine cases each of the two
outcomes in 20 % to 80 % of the conformers.  A case that misses a condition is drawn again with seed + 1000 * attempt.

Usage:  python -B tests/golden/gen_orbitals.py
"""
import io
import json
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _reference as R  # noqa: E402

R.ELEMENTS.update({3: ("Li", 1.28, 6.941)})          # (Cordero 2008 / IUPAC 2005, typed in as the others)
import gen_golden_embeds as G  # noqa: E402  (install_standins, the networkx alias, _embedder, _conformers; nothing is generated on import)

import tscode.graph_manipulations as gm  # noqa: E402
import tscode.parameters as ref_par  # noqa: E402

import test_orbitals as T  # noqa: E402  (the restatement: NumPy only)

ref_hc, ref_embedder, ref_embeds, ref_utils = G.ref_hc, G.ref_embedder, G.ref_embeds, G.ref_utils
DRAW_SEED = 2323
TOL = 1e-9


def xyz(name):
    z, frames = R.read_xyz_data(os.path.join(G.TESTS, name))
    return np.asarray(z), frames[0]


def hand(rows):
    return np.array([r[0] for r in rows]), np.array([r[1:] for r in rows], dtype=np.float64)


C60, S60 = 0.5, 0.8660254037844386
MOLECULES = {
    "CH3Cl": xyz("CH3Cl.xyz"), "HCOOH": xyz("HCOOH.xyz"), "C2H4": xyz("C2H4.xyz"),
    # H2C=C=CH2: the two CH2 planes at right angles
    "allene": hand([(6, -1.31, 0, 0), (6, 0, 0, 0), (6, 1.31, 0, 0), (1, -1.86, 0.93, 0), (1, -1.86, -0.93, 0), (1, 1.86, 0, 0.93), (1, 1.86, 0, -0.93)]),
    "acetonitrile": hand([(6, 0, 0, 0), (6, 1.46, 0, 0), (7, 2.62, 0, 0), (1, -0.36, 1.03, 0), (1, -0.36, -0.51, 0.89), (1, -0.36, -0.51, -0.89)]),
    # s-cis HN=CH-CH=NH, the N=C-C angles opened until the nitrogens are 2.98 A apart
    "diimine": hand([(7, -1.49, 1.046, 0), (6, -0.735, 0, 0), (6, 0.735, 0, 0), (7, 1.49, 1.046, 0), (1, -1.28, -0.944, 0), (1, 1.28, -0.944, 0),
                     (1, -2.449, 1.393, 0), (1, 2.449, 1.393, 0)]),
    "ketene": hand([(6, 0, 0, 0), (6, 1.31, 0, 0), (8, 2.47, 0, 0), (1, -0.54, 0.93, 0), (1, -0.54, -0.93, 0)]),
    "alkoxide": hand([(6, 0, 0, 0), (8, 1.40, 0, 0), (1, -0.36, 1.03, 0), (1, -0.36, -0.51, 0.89), (1, -0.36, -0.51, -0.89)]),
    # CH2=CH-O-Li, the lithium LAST: neighbors(graph, O)[0] is then the carbon (reactive_atoms_classes.py:561)
    "enolate": hand([(6, 0, 0, 0), (6, 1.36, 0, 0), (8, 1.36 + 1.30 * C60, 1.30 * S60, 0), (1, -0.54, 0.93, 0), (1, -0.54, -0.93, 0),
                     (1, 1.36 + 1.09 * C60, -1.09 * S60, 0), (3, 1.36 + 1.30 * C60 + 1.75, 1.30 * S60, 0)]),
    "propenal": hand([(6, 0, 0, 0), (6, 1.34, 0, 0), (6, 1.34 + 1.47 * C60, 1.47 * S60, 0), (8, 1.34 + 1.47 * C60 + 1.22, 1.47 * S60, 0), (1, -0.54, 0.93, 0),
                      (1, -0.54, -0.93, 0), (1, 1.34 + 1.09 * C60, -1.09 * S60, 0), (1, 1.34 + 1.47 * C60 - 1.09 * C60, 1.47 * S60 + 1.09 * S60, 0)]),
}
z8, x8 = MOLECULES["propenal"]
MOLECULES["propenal50"] = (np.concatenate([z8, np.ones(42, dtype=z8.dtype)]),
                           np.concatenate([x8, [(25.0 + 4.0 * (q % 7), 25.0 + 4.0 * (q // 7), 25.0) for q in range(42)]]))

CASES = {
    "ch3cl_ch": dict(mol="CH3Cl", reactive=[0, 1], n=24, sigma=0.04, seed=2301),
    "ch3cl_c": dict(mol="CH3Cl", reactive=[0], n=24, sigma=0.04, seed=2302),
    "ch3cl_cl": dict(mol="CH3Cl", reactive=[4], n=24, sigma=0.04, seed=2303),
    "hcooh_co": dict(mol="HCOOH", reactive=[0, 1], n=24, sigma=0.04, seed=2304),
    "hcooh_oh": dict(mol="HCOOH", reactive=[3, 4], n=24, sigma=0.04, seed=2305, orb_dim={3: 1.25, 4: 1.25}),      # DIST 2.5
    "c2h4": dict(mol="C2H4", reactive=[0, 3], n=24, sigma=0.04, seed=2306),
    "allene": dict(mol="allene", reactive=[1], n=64, sigma=0.04, seed=2307, share="sp"),
    "acetonitrile": dict(mol="acetonitrile", reactive=[1], n=24, sigma=0.01, seed=2308),
    "diimine": dict(mol="diimine", reactive=[0, 3], n=64, sigma=0.06, seed=2309, share="sigmatropic"),
    "ketene": dict(mol="ketene", reactive=[2], n=24, sigma=0.03, seed=2310),
    "alkoxide": dict(mol="alkoxide", reactive=[1], n=24, sigma=0.03, seed=2311),
    "enolate": dict(mol="enolate", reactive=[0, 6], n=24, sigma=0.03, seed=2312),
    "propenal": dict(mol="propenal", reactive=[0, 3], n=24, sigma=0.04, seed=2313),
    "propenal50": dict(mol="propenal50", reactive=[0, 3], n=24, sigma=0.04, seed=2314),
}


class Redraw(Exception):
    pass


def need(cond, what):
    if not cond:
        raise Redraw(what)


def molecule(coords, atomnos, reactive):
    """A reference Hypermolecule from arrays: the attributes its file constructor sets (hypermolecule_class.py:154-188), coordinates as given."""
    mol = ref_hc.Hypermolecule.__new__(ref_hc.Hypermolecule)
    mol.rootname = mol.name = "molecule"
    mol.debug = False
    mol.reactive_indices = np.array(reactive)
    mol.atomnos = np.asarray(atomnos)
    mol.atomcoords = np.array(coords, dtype=np.float64)
    mol.position, mol.rotation = np.zeros(3), np.identity(3)
    mol.graph = gm.graphize(mol.atomcoords[0], mol.atomnos)
    mol.atoms = mol.atomcoords.reshape(-1, 3)
    return mol


def compute_orbitals(mol, orb_dim=None):
    """hypermolecule_class.py:203-214 walked step by step, the generator re-seeded before every init(update=True); then the DIST keyword
    (tscode/embedder.py:527-535) for the atoms of ``orb_dim``."""
    mol.sp3_sigmastar, mol.sigmatropic = None, None
    mol._inspect_reactive_atoms(override=None)
    mol.sigmatropic = [gm.is_sigmatropic(mol, c) for c, _ in enumerate(mol.atomcoords)]
    mol.sp3_sigmastar = gm.is_vicinal(mol)
    for c, _ in enumerate(mol.atomcoords):
        for index, r_atom in mol.reactive_atoms_classes_dict[c].items():
            np.random.seed(DRAW_SEED)
            r_atom.init(mol, index, update=True, conf=c)
            if orb_dim and int(index) in orb_dim:
                np.random.seed(DRAW_SEED)
                r_atom.init(mol, index, update=True, orb_dim=orb_dim[int(index)], conf=c)


def set_pivots(mol, suprafacial):
    e = G._embedder([mol], "cyclical", suprafacial=suprafacial)
    ref_embedder.Embedder._set_pivots(e, mol)
    return mol.pivots


def pad(rows, slots, width, fill, dtype):
    out = np.full((slots, width), fill, dtype=dtype)
    if len(rows):
        out[:len(rows)] = np.asarray(rows).reshape(len(rows), width)
    return out


def record(mol):
    """The arrays of a computed molecule, laid out as tsc_orbitals lays them out."""
    C, Rn = len(mol.atomcoords), len(mol.reactive_indices)
    d = dict(centers=np.zeros((C, Rn, 4, 3)), orb_vecs=np.zeros((C, Rn, 4, 3)), n_lobes=np.zeros((C, Rn), np.uint8), sigmatropic=np.array(mol.sigmatropic, bool))
    names = []
    for c in range(C):
        atoms = mol.get_r_atoms(c)
        names.append([str(a) for a in atoms])
        for r, a in enumerate(atoms):
            k = len(a.center)
            assert len(a.orb_vecs) == k
            d["centers"][c, r, :k], d["orb_vecs"][c, r, :k], d["n_lobes"][c, r] = a.center, a.orb_vecs, k
    for supra, tag in ((False, "off"), (True, "on")):
        pivots = set_pivots(mol, supra) if Rn <= 2 else [[] for _ in range(C)]
        d["pivot_" + tag] = np.array([pad([p.pivot for p in pv], 16, 3, 0.0, np.float64) for pv in pivots])
        d["meanpoint_" + tag] = np.array([pad([p.meanpoint for p in pv], 16, 3, 0.0, np.float64) for pv in pivots])
        d["lobe_index_" + tag] = np.array([pad([p.index for p in pv], 16, 2, -1, np.int8) for pv in pivots])
        d["n_pivots_" + tag] = np.array([len(pv) for pv in pivots], dtype=np.uint8)
    return d, names


def edges_of(graph):
    return np.array(sorted((int(min(a, b)), int(max(a, b))) for a, b in graph.edges if a != b), dtype=np.int32).reshape(-1, 2)


def case(name, spec, seed):
    z, base = MOLECULES[spec["mol"]]
    rng = np.random.default_rng(seed)
    coords = base[None] + rng.normal(size=(spec["n"],) + base.shape) * spec["sigma"]
    coords[0] = base
    mol = molecule(coords, z, spec["reactive"])
    compute_orbitals(mol, spec.get("orb_dim"))
    d, names = record(mol)
    np.random.seed(DRAW_SEED)
    drawn = np.random.rand(3)
    edges = edges_of(mol.graph)
    nbs = [[int(v) for v in gm.neighbors(mol.graph, int(i))] for i in spec["reactive"]]
    assert all(v == sorted(v) for v in nbs)
    need(all(np.isfinite(d[k]).all() for k in d if d[k].dtype == np.float64), f"{name}: NaN")
    classes = [type(a).__name__ for a in mol.get_r_atoms(0)]
    for supra, tag in ((False, "off"), (True, "on")):
        e = T.restate(coords, z, edges, spec["reactive"], seed=drawn, suprafacial=supra, orb_dim=spec.get("orb_dim"))
        need(all(m.ok() for m in e.margins), f"{name}: a guard band is violated: {[vars(m) for m in e.margins if not m.ok()][:1]}")
        # the restatement that judges the guards reproduces what the reference computed
        assert e.graph["classes"] == classes and e.graph["neighbours"] == nbs and e.graph["sigmastar"] == bool(mol.sp3_sigmastar), name
        assert [[T.KINDS[k] for k in row] for row in e.kind] == names, (name, names[:2])
        assert (e.n_lobes == d["n_lobes"]).all() and (e.sigmatropic == d["sigmatropic"]).all(), name
        assert np.abs(e.centers - d["centers"]).max() <= TOL and np.abs(e.orb_vecs - d["orb_vecs"]).max() <= TOL, name
        assert (e.n_pivots == d["n_pivots_" + tag]).all() and (e.lobe_index == d["lobe_index_" + tag]).all(), (name, tag)
        assert np.abs(e.pivot - d["pivot_" + tag]).max() <= TOL and np.abs(e.meanpoint - d["meanpoint_" + tag]).max() <= TOL, (name, tag)
    path = e.graph["path"]
    if spec.get("share") == "sp":
        share = float(np.mean([row[0] == "sp" for row in names]))
        need(0.2 <= share <= 0.8, f"{name}: 'sp' in {share:.2f} of the conformers")
    elif spec.get("share") == "sigmatropic":
        share = float(np.mean(d["sigmatropic"]))
        need(0.2 <= share <= 0.8, f"{name}: sigmatropic in {share:.2f} of the conformers")
    else:
        share = None
    arrays = dict(d, coords=coords, base=base, atomnos=z.astype(np.int32), reactive=np.array(spec["reactive"], dtype=np.int32), edges=edges, seed=drawn)
    stats = {"seed": seed, "sigma": spec["sigma"], "n_conformers": int(spec["n"]), "n_atoms": int(len(z)), "classes": classes, "neighbors": nbs,
             "names": names, "sp3_sigmastar": bool(mol.sp3_sigmastar), "sigmatropic_path": bool(path), "share": share,
             "options": {"orb_dim": {str(k): v for k, v in spec["orb_dim"].items()} if spec.get("orb_dim") else None, "leaving_group": None}}
    return arrays, stats


def drawn_case(name, spec):
    for attempt in range(50):
        try:
            return case(name, spec, spec["seed"] + 1000 * attempt)
        except Redraw as why:
            print(f"  {name} seed {spec['seed'] + 1000 * attempt}: {why} -- drawn again")
    raise SystemExit(f"{name}: no seed satisfies the conditions")


def chain():
    """Two conformer ensembles as coordinates only -> orbitals -> pivots -> the reference's cyclical_embed (rigid shortcut), as G12 records it."""
    rng = np.random.default_rng(2390)
    zc, xc = MOLECULES["C2H4"]
    zh, xh = MOLECULES["HCOOH"]
    frames = [G._conformers(zc, xc, rng, 2, (0, 3), [1, 2], jitter=0.03, jitter_first=True), G._conformers(zh, xh, rng, 3, (0, 3), [4])]
    reactive, dist, steps, rot_range, thresh = [[0, 3], [1, 3]], 2.1, 2, 40, 1.45
    mols = []
    for (z, x, r) in ((zc, frames[0], reactive[0]), (zh, frames[1], reactive[1])):
        mol = molecule(x, z, r)
        compute_orbitals(mol, {i: dist / 2 for i in r})
        mols.append(mol)
    e = G._embedder(mols, "cyclical", clash_thresh=thresh, rigid=True)
    for m in mols:
        ref_embedder.Embedder._set_pivots(e, m)
    e.systematic_angles = ref_utils.cartesian_product(*[range(steps + 1) for _ in mols]) * 2 * rot_range / steps - rot_range
    inp = G._cyclical_inputs(e)
    poses = ref_embeds.cyclical_embed(e)
    arrays = {"poses": np.asarray(poses), "constrained_indices": np.asarray(e.constrained_indices), "angles": inp["angles"]}
    for k, m in enumerate(mols):
        arrays.update({f"coords{k}": m.atomcoords, f"atomnos{k}": np.asarray(m.atomnos, dtype=np.int32), f"reactive{k}": np.array(reactive[k], dtype=np.int32),
                       f"edges{k}": edges_of(m.graph)})
        for c in range(len(m.atomcoords)):
            arrays[f"pivot_vec{k}_{c}"], arrays[f"pivot_cumnums{k}_{c}"] = inp[f"pivot_vec{k}_{c}"], inp[f"pivot_cumnums{k}_{c}"]
    assert len(poses) > 0 and np.isfinite(arrays["poses"]).all()
    stats = {"dist": dist, "clash_thresh": thresh, "steps": steps, "rot_range": rot_range, "n_poses": int(len(poses)), "file": "G23b_orbitals.npz"}
    return arrays, stats


def reference_seconds():
    """The reference's own seconds per conformer on propenal, two reactive atoms, 2 000 conformers: compute_orbitals and _set_pivots."""
    z, base = MOLECULES["propenal"]
    coords = base[None] + np.random.default_rng(2399).normal(size=(2000,) + base.shape) * 0.04
    mol = molecule(coords, z, [0, 3])
    t0 = time.perf_counter()
    mol.compute_orbitals()
    t1 = time.perf_counter()
    set_pivots(mol, False)
    t2 = time.perf_counter()
    return {"orbitals": float(f"{(t1 - t0) / 2000:.2g}"), "pivots": float(f"{(t2 - t1) / 2000:.2g}"), "molecule": "propenal", "n_conformers": 2000}


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")
    assert os.path.getsize(path) < 700000


def main():
    meta = {"numpy": np.__version__, "draw_seed": DRAW_SEED, "orb_dim_dict": dict(ref_par.orb_dim_dict), "cases": {}}
    files = {}
    for name, spec in CASES.items():
        arrays, stats = drawn_case(name, spec)
        for k, v in arrays.items():
            files[f"{name}/{k}"] = v
        meta["cases"][name] = dict(stats, file="G23a_orbitals.npz")
        print(f"  {name}: seed {stats['seed']}, classes {stats['classes']}, sigma-star {stats['sp3_sigmastar']}, path {stats['sigmatropic_path']}, "
              f"share {stats['share']}, names {sorted({tuple(n) for n in stats['names']})}")
    save_npz(os.path.join(HERE, "G23a_orbitals.npz"), files)
    arrays, stats = chain()
    meta["cases"]["chain"] = stats
    save_npz(os.path.join(HERE, "G23b_orbitals.npz"), {f"chain/{k}": v for k, v in arrays.items()})
    print(f"  chain: {stats['n_poses']} poses kept")
    meta["reference_seconds_per_conformer"] = reference_seconds()
    print("  reference:", meta["reference_seconds_per_conformer"])
    json.dump(meta, open(os.path.join(HERE, "G23_orbitals.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
