"""G21: the reference's own graphize (tscode/graph_manipulations.py:33-55), molecule_check, scramble_check and
get_double_bonds_indices (tscode/utils.py:293-387), case by case, and the modules of the reference that bind those four names.

BUILD CONTAINER ONLY (imports the reference through tests/golden/_reference.py, which exists only there).  No test imports it.

Cases (every array of a case is stored as "<case>/<name>" in the case's file; G21_topology.json is the index):
  chain50    400 structures of 50 atoms: tscode_amd.synthetic.make_chain_ensemble (a self-avoiding walk with 1.5 A steps, all other
             pairs >= 2.0 A apart, elements cycling C, C, O, N, C; the base plus Gaussian noise, sigma per structure from
             {0.02, 0.05, 0.08, 0.12} A).  The expected graph is the reference's graphize of the base.  Recorded: graphize's edges of
             every structure, scramble_check's and molecule_check's verdicts for max_newbonds in {0, 1, 3}, formed / broken counts.
  chain200   150 structures of 200 atoms, the same.
  masked50   the chain50 ensemble with a random graphize mask (edges recorded), and scramble_check with excluded atoms shared by all
             structures and with excluded atoms per structure (rows padded with -1).
  bimol      the reference's tests/CH3Cl.xyz and tests/HCOOH.xyz (data, read by _reference.read_xyz_data): the second molecule turned
             by a random rotation and put with its centroid 1.5 to 4 A from the first one's, in a random direction, everything
             jittered (sigma per structure from BIMOL_SIGMAS); mols_graphs are the two molecules' own graphs,
             excluded_atoms a reactive pair (the chlorine of CH3Cl, a hydrogen of HCOOH).
  double     a 24-atom chain with 1.35 A steps of C, C, N, C, O, H, jittered: get_double_bonds_indices of every structure.

Conditions asserted here (tests/test_topology.py asserts them again on the files): every verdict array has at least 20 % True and
at least 20 % False; every family has a structure with formed > 0 and one with broken > 0; no pair of any structure lies within
1e-10 A of its threshold.  A case that misses one is drawn again with seed + 1000 * attempt, the seed used is recorded.  A rerun
writes the same bytes.

Usage:  python -B tests/golden/gen_topology.py
"""
import importlib
import io
import json
import os
import pkgutil
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _reference as R  # noqa: E402

R.install_standins(full=True)
import networkx as nx  # noqa: E402
if not hasattr(nx, "from_numpy_matrix"):
    nx.from_numpy_matrix = nx.from_numpy_array

import tscode  # noqa: E402
import tscode.graph_manipulations as gm  # noqa: E402
import tscode.utils as ut  # noqa: E402

from tscode_amd.synthetic import make_chain_ensemble, quat_to_mat  # noqa: E402  (NumPy only)

GUARD = 1e-10
# Two five-atom molecules whose reactive pair is excluded change few bonds however they are placed: the jitter has to reach the
# X-H bonds' 0.2 A margin for a fifth of the structures to fail at max_newbonds = 3
BIMOL_SIGMAS = (0.03, 0.06, 0.45, 0.6)
MAX_NEWBONDS = (0, 1, 3)
NAMES = ("graphize", "molecule_check", "scramble_check", "get_double_bonds_indices")


class Redraw(Exception):
    pass


def need(cond, what):
    if not cond:
        raise Redraw(what)


# ------------------------------------------------------------------------------------------------------- helpers
def ref_edges(coords, atomnos, mask=None):
    """The reference's graphize: its edges without the self loops, i < j, sorted."""
    g = gm.graphize(coords, atomnos, mask) if mask is not None else gm.graphize(coords, atomnos)
    return sorted({(min(a, b), max(a, b)) for a, b in g.edges if a != b})


def flat_edges(per_structure):
    """A list of edge lists -> (edges int16[E_total, 2], offsets int32[N + 1])."""
    off = np.cumsum([0] + [len(e) for e in per_structure]).astype(np.int32)
    flat = np.array([p for e in per_structure for p in e], dtype=np.int16).reshape(-1, 2)
    return flat, off


def radii_and_thr(atomnos):
    elements = sorted(set(int(z) for z in atomnos))
    radii = np.array([gm.pt[z].covalent_radius for z in elements])
    thr = np.array([[gm.d_min_bond(a, b) for b in elements] for a in elements])
    return np.array(elements), radii, thr


def guard_distance(structures, thr_of_pair):
    """Smallest | d(i, j) - threshold(i, j) | over all structures and pairs with a threshold."""
    iu = np.triu_indices(structures.shape[1], 1)
    t = thr_of_pair[iu]
    worst = np.inf
    for x in structures:
        d = x[iu[0]] - x[iu[1]]
        dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        worst = min(worst, float(np.abs(dist - t)[t > 0].min()))
    return worst


def pair_thresholds(atomnos):
    return np.array([[gm.d_min_bond(a, b) for b in atomnos] for a in atomnos])


def delta_counts(edges, expected, excluded):
    new, old = set(edges), set(expected)
    ex = set(int(a) for a in excluded if a >= 0)
    formed = sum(1 for b in new - old if b[0] not in ex and b[1] not in ex)
    broken = sum(1 for b in old - new if b[0] not in ex and b[1] not in ex)
    return formed, broken


def scramble_case(structures, atomnos, graphs, expected, excluded_rows, edges):
    """scramble_check of every structure for every max_newbonds; excluded_rows: one list per structure (-1 entries dropped)."""
    log = []
    verdicts = np.zeros((len(MAX_NEWBONDS), len(structures)), dtype=bool)
    formed = np.zeros(len(structures), dtype=np.int32)
    broken = np.zeros(len(structures), dtype=np.int32)
    for s, x in enumerate(structures):
        ex = [int(a) for a in excluded_rows[s] if a >= 0]
        formed[s], broken[s] = delta_counts(edges[s], expected, ex)
        for m, mnb in enumerate(MAX_NEWBONDS):
            verdicts[m, s] = ut.scramble_check(x, atomnos, ex, graphs, max_newbonds=mnb, logfunction=log.append, title="t")
            assert verdicts[m, s] == (formed[s] + broken[s] <= mnb), "scramble_check disagrees with the sets of its own graphize"
    return verdicts, formed, broken


def precheck(edges, expected, excluded_rows, what):
    """The conditions, from the edges the reference's graphize gave: asked before the slow scramble_check runs."""
    fb = np.array([delta_counts(e, expected, ex) for e, ex in zip(edges, excluded_rows)])
    check_verdicts([fb.sum(1) <= m for m in MAX_NEWBONDS], fb[:, 0], fb[:, 1], what)


def check_verdicts(verdicts, formed, broken, what):
    for m, v in zip(MAX_NEWBONDS, verdicts):
        share = float(np.mean(v))
        need(0.2 <= share <= 0.8, f"{what}: max_newbonds = {m}: {share:.2f} True")
    need((formed > 0).any() and (broken > 0).any(), f"{what}: formed {int(formed.sum())}, broken {int(broken.sum())}")


# ------------------------------------------------------------------------------------------------------- cases
def chain_case(n_structs, n_atoms, with_masked, seed):
    base, structures, atomnos, sigma = make_chain_ensemble(n_structs, n_atoms, seed)
    need(guard_distance(np.concatenate([base[None], structures]), pair_thresholds(atomnos)) > GUARD, "a pair on its threshold")
    elements, radii, thr = radii_and_thr(atomnos)
    base_graph = gm.graphize(base, atomnos)
    expected = ref_edges(base, atomnos)
    assert expected == [(i, i + 1) for i in range(n_atoms - 1)], "the base is not a chain"
    edges = [ref_edges(x, atomnos) for x in structures]
    none = [[] for _ in structures]
    precheck(edges, expected, none, f"chain{n_atoms}")
    shared = per = None
    if with_masked:
        rng = np.random.default_rng(seed + 17)
        mask = rng.random(n_atoms) < 0.8
        shared = np.sort(rng.choice(n_atoms, size=3, replace=False)).astype(np.int32)
        per = np.full((n_structs, 4), -1, dtype=np.int32)
        for s in range(n_structs):
            k = int(rng.integers(0, 5))                      # 0 .. 4 atoms: rows of all -1 occur
            per[s, :k] = rng.choice(n_atoms, size=k, replace=False)
        need((per == -1).all(axis=1).any(), "no row of all -1")
        precheck(edges, expected, [shared] * n_structs, "masked50 shared")
        precheck(edges, expected, per, "masked50 per structure")
    verdicts, formed, broken = scramble_case(structures, atomnos, [base_graph], expected, none, edges)
    check_verdicts(verdicts, formed, broken, f"chain{n_atoms}")
    mol = np.array([[ut.molecule_check(base, x, atomnos, max_newbonds=m) for x in structures] for m in MAX_NEWBONDS])
    assert (mol == verdicts).all()
    fe, fo = flat_edges(edges)
    out = {"base": base, "structures": structures, "atomnos": atomnos.astype(np.int32), "sigma": sigma, "elements": elements.astype(np.int32),
           "radii": radii, "thr": thr, "expected_edges": np.array(expected, dtype=np.int16), "edges": fe, "edge_off": fo,
           "max_newbonds": np.array(MAX_NEWBONDS), "scramble_verdicts": verdicts, "molecule_verdicts": mol, "formed": formed, "broken": broken}
    stats = {"seed": seed, "true_share": [float(v.mean()) for v in verdicts], "unchanged_by_sigma":
             {str(sg): float(((formed + broken) == 0)[sigma == sg].mean()) for sg in sorted(set(sigma.tolist()))}}
    masked = None
    if with_masked:
        medges = [ref_edges(x, atomnos, mask) for x in structures]
        v_sh, f_sh, b_sh = scramble_case(structures, atomnos, [base_graph], expected, [shared] * n_structs, edges)
        v_pe, f_pe, b_pe = scramble_case(structures, atomnos, [base_graph], expected, per, edges)
        check_verdicts(v_sh, f_sh, b_sh, "masked50 shared")
        check_verdicts(v_pe, f_pe, b_pe, "masked50 per structure")
        me, mo = flat_edges(medges)
        masked = {"mask": mask, "mask_edges": me, "mask_edge_off": mo, "excluded_shared": shared, "excluded_per": per,
                  "shared_verdicts": v_sh, "shared_formed": f_sh, "shared_broken": b_sh,
                  "per_verdicts": v_pe, "per_formed": f_pe, "per_broken": b_pe}
    return out, stats, masked


def bimol_case(n_structs, seed):
    root = os.path.join(R.REFERENCE, "tscode", "tests")
    z1, c1 = R.read_xyz_data(os.path.join(root, "CH3Cl.xyz"))
    z2, c2 = R.read_xyz_data(os.path.join(root, "HCOOH.xyz"))
    m1, m2 = c1[0], c2[0]
    atomnos = np.concatenate([z1, z2])
    g1, g2 = gm.graphize(m1, z1), gm.graphize(m2, z2)
    e1, e2 = ref_edges(m1, z1), ref_edges(m2, z2)
    expected = sorted(e1 + [(a + len(z1), b + len(z1)) for a, b in e2])
    ra, rb = int(np.nonzero(z1 == 17)[0][0]), int(np.nonzero(z2 == 1)[0][0])             # the leaving chlorine, a hydrogen of the acid
    excluded = [ra, rb + len(z1)]
    rng = np.random.default_rng(seed)
    rot = quat_to_mat(rng.normal(size=(n_structs, 4)))
    direction = rng.normal(size=(n_structs, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    dist = rng.uniform(1.5, 4.0, size=n_structs)
    second = np.einsum("nij,aj->nai", rot, m2 - m2.mean(0))                               # its centroid at the origin
    second += (m1.mean(0) + direction * dist[:, None])[:, None, :]
    structures = np.concatenate([np.broadcast_to(m1, (n_structs,) + m1.shape), second], axis=1)
    sigma = np.array(BIMOL_SIGMAS)[rng.integers(0, len(BIMOL_SIGMAS), size=n_structs)]
    structures = np.ascontiguousarray(structures + rng.normal(size=structures.shape) * sigma[:, None, None])
    need(guard_distance(structures, pair_thresholds(atomnos)) > GUARD, "a pair on its threshold")
    elements, radii, thr = radii_and_thr(atomnos)
    edges = [ref_edges(x, atomnos) for x in structures]
    precheck(edges, expected, [excluded] * n_structs, "bimol")
    verdicts, formed, broken = scramble_case(structures, atomnos, [g1, g2], expected, [excluded] * n_structs, edges)
    check_verdicts(verdicts, formed, broken, "bimol")
    fe, fo = flat_edges(edges)
    out = {"structures": structures, "atomnos": atomnos.astype(np.int32), "elements": elements.astype(np.int32), "radii": radii, "thr": thr,
           "mol_sizes": np.array([len(z1), len(z2)], dtype=np.int32), "mol1_edges": np.array(e1, dtype=np.int16),
           "mol2_edges": np.array(e2, dtype=np.int16), "expected_edges": np.array(expected, dtype=np.int16), "excluded": np.array(excluded, dtype=np.int32),
           "edges": fe, "edge_off": fo, "max_newbonds": np.array(MAX_NEWBONDS), "scramble_verdicts": verdicts, "formed": formed, "broken": broken,
           "centroid_distance": dist, "sigma": sigma}
    return out, {"seed": seed, "true_share": [float(v.mean()) for v in verdicts]}


def double_case(n_structs, seed):
    rng = np.random.default_rng(seed)
    cycle = (6, 6, 7, 6, 8, 1)
    n = 24
    atomnos = np.array([cycle[i % len(cycle)] for i in range(n)])
    from tscode_amd.synthetic import make_chain
    base = make_chain(rng, n, step=1.35, min_dist=1.9)
    structures = np.ascontiguousarray(base[None] + rng.normal(size=(n_structs, n, 3)) * 0.06)
    table = {(6, 6): 1.4, (6, 7): 1.3, (7, 6): 1.3}
    thr_pair = np.array([[table.get((int(a), int(b)), 0.0) for b in atomnos] for a in atomnos])
    need(guard_distance(structures, thr_pair) > GUARD, "a pair on its threshold")
    edges = [[(int(a), int(b)) for a, b in ut.get_double_bonds_indices(x, atomnos)] for x in structures]
    assert all(e == sorted(e) for e in edges), "the reference's list is not ordered by i then j"
    kinds = {tuple(sorted((int(atomnos[a]), int(atomnos[b])))) for e in edges for a, b in e}
    need(kinds == {(6, 6), (6, 7)}, f"double: hits of kinds {kinds}")
    need(len({tuple(e) for e in edges}) >= 10, "double: the structures hardly differ")
    fe, fo = flat_edges(edges)
    return ({"structures": structures, "atomnos": atomnos.astype(np.int32), "edges": fe, "edge_off": fo},
            {"seed": seed, "distinct_edge_lists": len({tuple(e) for e in edges})})


def drawn(fn, seed, *args):
    for attempt in range(50):
        try:
            return fn(*args, seed + 1000 * attempt)
        except Redraw as why:
            print(f"  {fn.__name__} seed {seed + 1000 * attempt}: {why} -- drawn again")
    raise SystemExit(f"{fn.__name__}: no seed satisfies the conditions")


# ------------------------------------------------------------------------------------------------------- binding sites
def binding_sites():
    imported, failed = {}, {}
    for info in pkgutil.iter_modules(tscode.__path__):
        name = f"tscode.{info.name}"
        if info.name in ("__main__", "tests", "run_tests"):    # (entry points: importing them runs the program)
            continue
        try:
            imported[name] = importlib.import_module(name)
        except BaseException as e:  # noqa: BLE001
            failed[name] = f"{type(e).__name__}: {e}"[:200]
    for info in pkgutil.iter_modules(importlib.import_module("tscode.calculators").__path__):
        name = f"tscode.calculators.{info.name}"
        try:
            imported[name] = importlib.import_module(name)
        except BaseException as e:  # noqa: BLE001
            failed[name] = f"{type(e).__name__}: {e}"[:200]
    sites = {}
    for attr in NAMES:
        owners = [m for m in imported.values() if getattr(getattr(m, attr, None), "__module__", None) == m.__name__]
        obj = getattr(owners[0], attr)
        sites[attr] = {"defined_in": owners[0].__name__, "bound_in": sorted(n for n, m in imported.items() if getattr(m, attr, None) is obj)}
    return {"modules_imported": sorted(imported), "modules_not_importable_here": failed, "sites": sites}


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
    assert os.path.getsize(path) < 1000000


def main():
    sites = binding_sites()
    json.dump(sites, open(os.path.join(HERE, "G21_topology_sites.json"), "w"), indent=1, sort_keys=True)
    for a, s in sites["sites"].items():
        print(f"  {a:26s} defined in {s['defined_in']}; bound in {s['bound_in']}")
    print("  not importable here:", sites["modules_not_importable_here"])

    meta = {"numpy": np.__version__, "guard": GUARD, "max_newbonds": list(MAX_NEWBONDS), "cases": {}}
    c50, s50, masked = drawn(chain_case, 2101, 400, 50, True)
    c200, s200, _ = drawn(chain_case, 2102, 150, 200, False)
    bim, sbim = drawn(bimol_case, 2103, 200)
    dbl, sdbl = drawn(double_case, 2104, 120)
    files = {"a": {}, "b": {}, "c": {}}
    for key, case, arrays, stats in (("a", "chain50", c50, s50), ("a", "masked50", masked, {"seed": s50["seed"], "of": "chain50"}),
                                     ("b", "chain200", c200, s200), ("c", "bimol", bim, sbim), ("c", "double", dbl, sdbl)):
        for name, arr in arrays.items():
            files[key][f"{case}/{name}"] = arr
        meta["cases"][case] = dict(stats, file=f"G21{key}_topology.npz", n_structs=int(len(arrays.get("structures", c50["structures"]))),
                                   n_atoms=int(len(arrays.get("atomnos", c50["atomnos"]))))
    for key, arrays in files.items():
        save_npz(os.path.join(HERE, f"G21{key}_topology.npz"), arrays)
    json.dump(meta, open(os.path.join(HERE, "G21_topology.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
