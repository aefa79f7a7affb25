"""Shape sweep of the symmetry-corrected RMSD prune (tscode_amd/csrc/rot_corr.hpp, rot_corr.hip, tscode_amd/rot_corr.py) at the sizes
and edges the G19 fixtures do not reach: more than one wavefront of atoms, dynamic LDS above 64 KiB, heavy atoms that are no prefix,
angle tables of 1, 4 and 6 entries, the commit rule of the pass kernel (chunk lengths about the batch of 8, cache words past the first,
a second pass over cached pairs), the grid stride of the value-level kernel and the Jacobi fallback on a one-atom subgraph.

The reference is a plain numpy fp64 restatement written here (rot_corr_rmsd, pass_restated, prune_restated); the unmarked tests of
section 2 show that it reproduces the reference's own run recorded in G19.  Every input comes from tscode_amd.synthetic under a
committed seed; the unmarked guard of section 3 regenerates all of them and checks, with the restatement alone, the conditions the GPU
tests lean on (no value near a threshold, no near-tie between the angles of a torsion search, the intent of each case).  The comparisons
take the implementation as an argument (compare_values / compare_passes / compare_prune): the GPU tests hand them the engine.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from test_rot_corr import case as g19_case, centred

RMSD_TOL = 1e-9          # test_pair_trace's bound on rmsd values
COORD_TOL = 1e-10        # test_arrays_match_reference's bound on coordinates
RMSD_BAND = 1e-7         # G19's guard bands (tests/golden/gen_rot_corr.py)
ANGLE_BAND = 1e-9
BATCH = 8                # wavefronts per workgroup of k_rot_corr_pass (RC_WAVES): the j of a row are taken 8 at a time
THR = 0.25


# ===================================================================================================== 1. the restatement
def kabsch_rmsd(P, Q):
    """tests/golden/gen_rot_corr.py::kabsch_rmsd (rmsd 1.4, translate=False): P rotated onto Q."""
    Cm = P.T @ Q
    V, S, Wt = np.linalg.svd(Cm)
    if (np.linalg.det(V) * np.linalg.det(Wt)) < 0.0:
        V[:, -1] = -V[:, -1]
    d = P @ (V @ Wt) - Q
    return np.sqrt((d * d).sum() / P.shape[0])


class Setup:
    """The set-up arrays of prune_rmsd_rot_corr_arrays, as the restatement walks them."""

    def __init__(self, atomnos, torsions, angles, move_masks, sub_nodes):
        self.atomnos = np.asarray(atomnos)
        self.heavy = np.flatnonzero(self.atomnos != 1)
        self.torsions = np.asarray(torsions, dtype=np.int64).reshape(-1, 4)
        self.angles = [tuple(float(a) for a in angs) for angs in angles]
        self.masks = np.asarray(move_masks, dtype=bool).reshape(len(self.torsions), -1)
        self.subs = [np.asarray(s, dtype=np.int64) for s in sub_nodes]
        self.sub_moves = [bool(self.masks[t][s].any()) for t, s in enumerate(self.subs)]     # does torsion t turn an atom of its subgraph?
        self.long = [t for t in range(len(self.torsions)) if self.masks[t].sum() > 64]         # torsions whose moved list passes one wavefront

    def kwargs(self):
        return dict(atomnos=self.atomnos, torsions=self.torsions.astype(np.int32), angles=self.angles, move_masks=self.masks, sub_nodes=self.subs)


def turn(x, i2, i3, mask, angle):
    """rotate_dihedral (tscode/utils.py:389-414) in place, as test_pair_trace states it."""
    from tscode_amd.algebra import rot_mat_from_pointer
    R = rot_mat_from_pointer(x[i2] - x[i3], angle)
    x[mask] = (R @ (x[mask] - x[i3]).T).T + x[i3]


def rot_corr_rmsd(ref, coord, s, searches=None):
    """rotationally_corrected_rmsd (tscode/torsion_module.py:953-1011): coord is turned in place.  Returns (rmsd, best angles);
    ``searches``, a list, receives (torsion, the value of every angle) per torsion search."""
    best = []
    for t, tor in enumerate(s.torsions):
        i2, i3 = int(tor[1]), int(tor[2])
        best_rmsd, best_angle, values = 1e10, 0.0, []
        for angle in s.angles[t]:
            turn(coord, i2, i3, s.masks[t], angle)
            r = kabsch_rmsd(ref[s.subs[t]], coord[s.subs[t]])
            values.append(r)
            if r < best_rmsd:
                best_rmsd, best_angle = r, angle
            turn(coord, i2, i3, s.masks[t], -angle)
        best.append(best_angle)
        if searches is not None:
            searches.append((t, values))
    for tor, mask, angle in zip(s.torsions, s.masks, best):
        turn(coord, int(tor[1]), int(tor[2]), mask, angle)
    return kabsch_rmsd(ref[s.heavy], coord[s.heavy]), best


def chunk_bounds(d, k, num_active, step):
    return d * step, (num_active if step == k - 1 else d * (step + 1))


def pass_restated(S, cache, s, d, k, num_active, thr, on_pair=None, on_hit=None, on_skip=None):
    """One pass of tscode/torsion_module.py:1091-1125 without the graph step: S is turned in place, cache (a set of (i, j)) grows.
    Returns (first, pairs evaluated).  on_pair(i, j, rmsd, searches) sees every evaluated pair, on_hit(i, j, hi) every row's match,
    on_skip(i, j) every cached pair the pass walks past."""
    first = np.full(len(S), -1, dtype=np.int32)
    evaluated = 0
    for step in range(k):
        lo, hi = chunk_bounds(d, k, num_active, step)
        for i in range(lo, hi):
            for j in range(i + 1, hi):
                if (i, j) in cache:
                    if on_skip is not None:
                        on_skip(i, j)
                    continue
                searches = [] if on_pair is not None else None
                r, _ = rot_corr_rmsd(S[i], S[j], s, searches)
                evaluated += 1
                if on_pair is not None:
                    on_pair(i, j, r, searches)
                if r < thr:
                    first[i] = j
                    if on_hit is not None:
                        on_hit(i, j, hi)
                    break
                cache.add((i, j))
    return first, evaluated


def prune_restated(structures, s, thr, on_pair=None):
    """prune_rmsd_rot_corr_arrays with max_structures=None: pass_restated under the schedule.  Returns (kept, mask, stats as
    last_rot_corr_stats gives them)."""
    from tscode_amd.numba_functions import TFD_KS, _pass_schedule
    S = centred(structures)
    cache = set()
    stats = {int(k): {"k": k, "n_active": None, "ran": False, "pairs_evaluated": 0} for k in TFD_KS}

    def first_similar(d, k, num_active):
        first, ev = pass_restated(S, cache, s, d, k, num_active, thr, on_pair)
        stats[k].update(n_active=num_active, ran=True, pairs_evaluated=ev)
        return first

    def gate_seen(k, num_active):
        stats[int(k)]["n_active"] = num_active

    mask = _pass_schedule(len(S), False, first_similar, on_slot=gate_seen)
    return S[mask], mask, [stats[int(k)] for k in TFD_KS]


# ===================================================================================================== 2. the restatement against G19
def g19_setup(name):
    c = g19_case(name)
    return c, Setup(c.atomnos, **c.setup)


def test_restatement_reproduces_the_traced_pairs():
    """All 438 pairs the reference evaluated in the N = 40 case, in its order, each on the structures as the earlier ones left them."""
    c, s = g19_setup("n40")
    pairs, best, rmsd = (c.data[c.p + k] for k in ("trace_pairs", "trace_best", "trace_rmsd"))
    assert len(pairs) == 438
    S = centred(c.structures)
    got = [rot_corr_rmsd(S[i], S[j], s) for i, j in pairs.tolist()]
    assert np.array_equal(np.array([b for _, b in got]), best)
    err = np.abs(np.array([r for r, _ in got]) - rmsd).max()
    assert err < RMSD_TOL, err


@pytest.mark.parametrize("name", ["n40", "n160a"])
def test_restatement_reproduces_the_full_prune(name):
    c, s = g19_setup(name)
    kept, mask, stats = prune_restated(c.structures, s, c.meta["max_rmsd"])
    assert np.array_equal(mask, c.mask), (int(mask.sum()), int(c.mask.sum()))
    assert [st["n_active"] for st in stats] == c.passes[:, 0].tolist()
    assert [st["pairs_evaluated"] for st in stats] == c.passes[:, 1].tolist()
    assert kept.shape == c.out.shape
    err = np.abs(kept - c.out).max()
    assert err < COORD_TOL, err


# ===================================================================================================== 3. the sweep's inputs
# atoms x torsions -> the rotor groups of make_rotor_molecule; "far" turns the long side of the bond (a moved list of over 64 atoms)
SHAPES = {"65x2": [(3, "far"), 2],                      # one atom past a wavefront
          "130x5": [(2, "far"), (3, 3)],                # h and the first subgraphs over 64; moved lists of 126 and of 3
          "330x2": [(4, "far"), 6],                     # 67 072 bytes of dynamic LDS
          "512x16": [(4, 3), (3, 2), 6, (2, "far"), 3, 4, 6, 2, 3]}     # the limits; folds 2, 3, 4 and 6
SHAPE_SEEDS = {"65x2": 65, "130x5": 130, "330x2": 330, "512x16": 512}
LONG_MOVED = {"130x5", "330x2", "512x16"}


def lds_bytes(T, n, waves=BATCH):
    """rot_corr_lds_bytes (csrc/rot_corr.hpp) restated."""
    lists = (T * n * 2 * 2 + T * 4 * 4 + 15) & ~15
    return lists + waves * (n * 3 + 16) * 8 + 16


@functools.lru_cache(maxsize=None)
def molecule(shape, order=None):
    from tscode_amd.synthetic import make_rotor_molecule
    return make_rotor_molecule(int(shape.split("x")[0]), SHAPES[shape], seed=SHAPE_SEEDS[shape], order=order)


@pytest.mark.parametrize("shape,order", [("65x2", None), ("130x5", "shuffle"), ("512x16", None), ("512x16", "shuffle")])
def test_rotor_molecule_is_what_its_set_up_says(shape, order):
    """A tree; masks and subgraphs as networkx finds them on its bonds (the subgraphs by the drop-in's own helper); every rotor turned
    by its 360 / k is the same molecule with the rotor's atoms permuted among atoms of their element."""
    import networkx as nx
    from tscode_amd.rot_corr import _local_heavy_subgraph
    mol = molecule(shape, order)
    n, T = map(int, shape.split("x"))
    assert mol.coords.shape == (n, 3) and len(mol.atomnos) == n and mol.torsions.shape == (T, 4) and mol.move_masks.shape == (T, n)
    g = nx.Graph(mol.bonds)
    assert len(mol.bonds) == n - 1 and g.number_of_nodes() == n and nx.is_connected(g)
    tors = [list(map(int, t)) for t in mol.torsions]
    far = 0
    for t, (i1, i2, i3, i4) in enumerate(tors):
        assert g.has_edge(i1, i2) and g.has_edge(i2, i3) and g.has_edge(i3, i4) and not (mol.atomnos[[i1, i2, i3, i4]] == 1).any()
        assert mol.angles[t] == tuple(360.0 / mol.folds[t] * q for q in range(mol.folds[t]))
        cut = g.copy()
        cut.remove_edge(i2, i3)
        sides = [nx.node_connected_component(cut, a) - {i2, i3} for a in (i3, i2)]
        moved = set(np.flatnonzero(mol.move_masks[t]).tolist())
        assert moved in sides
        far += moved == sides[1]
        assert mol.sub_nodes[t] == _local_heavy_subgraph(g, tors, tors[t], mol.atomnos)
        if moved == sides[0]:
            x = mol.coords.copy()
            turn(x, i2, i3, mol.move_masks[t], mol.angles[t][1])
            idx = sorted(moved)
            d = np.sqrt(((x[idx][:, None] - mol.coords[idx][None]) ** 2).sum(axis=2))
            image = d.argmin(axis=1)
            assert d.min(axis=1).max() < 1e-12 and sorted(image.tolist()) == list(range(len(idx))) and (image != np.arange(len(idx))).all()
            assert np.array_equal(mol.atomnos[idx][image], mol.atomnos[idx])
    assert far == 1
    heavy = np.flatnonzero(mol.atomnos != 1)
    assert np.array_equal(heavy, np.arange(len(heavy))) == (order is None)
    if order is not None:                                    # the same molecule as the heavy-first one, atom for atom
        plain = molecule(shape)
        d = np.sqrt(((mol.coords[:, None] - plain.coords[None]) ** 2).sum(axis=2))
        assert (d.min(axis=1) == 0).all() and np.array_equal(plain.atomnos[d.argmin(axis=1)], mol.atomnos)


def test_rotor_molecule_options():
    from tscode_amd.synthetic import make_rotor_molecule
    a = make_rotor_molecule(30, [3, (2, 4)], seed=3)
    order = np.arange(30)[::-1]
    b = make_rotor_molecule(30, [3, (2, 4)], seed=3, order=order, table={1: (0, 10.5)})
    assert np.array_equal(b.coords, a.coords[order]) and np.array_equal(b.atomnos, a.atomnos[order]) and b.folds == a.folds == [3, 2, 4, 4]
    assert np.array_equal(b.torsions, 29 - a.torsions) and np.array_equal(b.move_masks, a.move_masks[:, order])
    assert b.sub_nodes == [sorted(29 - np.array(s)) for s in a.sub_nodes]
    assert b.angles[1] == (0.0, 10.5) and b.angles[2] == a.angles[2] == (0.0, 90.0, 180.0, 270.0)
    for bad in ([5], [(3, 3, 3)], [], [(3, "near")]):
        with pytest.raises(ValueError):
            make_rotor_molecule(30, bad if bad else [6] * 5, seed=3)


def raw_ensemble(mol, n_clusters, per_cluster, seed):
    """Clusters of exact symmetry turns plus noise (make_rot_corr_ensemble).  The torsions that turn the long side of their bond are
    left out there (the atoms they would keep from the clusters' spread are nearly all); every member then turns the long side of each
    of them by an entry of its table, so that the searches of these torsions -- the moved lists of more than 64 entries -- have
    a turn to find and the winning angle, the value and the turned coordinates depend on every entry of the list."""
    from tscode_amd.synthetic import make_rot_corr_ensemble
    few = mol.move_masks.sum(axis=1) <= mol.move_masks.shape[1] // 2
    S, _ = make_rot_corr_ensemble(mol.coords, mol.torsions, mol.angles, mol.move_masks, n_clusters, per_cluster, turn=few.tolist(), seed=seed)
    rng = np.random.default_rng([seed, 1])
    for x in S:
        for t in np.flatnonzero(~few):
            turn(x, int(mol.torsions[t][1]), int(mol.torsions[t][2]), mol.move_masks[t], mol.angles[t][rng.integers(len(mol.angles[t]))])
    return S


def ensemble(mol, n_clusters, per_cluster, seed):
    """raw_ensemble, placed for the entry points that do not centre (rot_corr_pairs, the passes of a run).  The Kabsch step takes no
    translation, so a turn of the long side about a bond far from the origin moves nearly the whole structure away and never wins a
    search.  A molecule with such a torsion is therefore placed with that torsion's i3 at the origin: its turns are rotations about the
    origin, and the search finds them.  The others are centred on their mean, as the prune centres its input."""
    S = raw_ensemble(mol, n_clusters, per_cluster, seed)
    far = np.flatnonzero(mol.move_masks.sum(axis=1) > mol.move_masks.shape[1] // 2)
    return S - S[:, int(mol.torsions[far[0]][2])][:, None, :] if len(far) else centred(S)


def best_of(s, searches):
    """The winning angle of every search of one pair (the first strictly smaller value wins)."""
    return [s.angles[t][int(np.argmin(values))] for t, values in searches]


def long_list_turns(s, all_searches):
    """In how many of the pairs a torsion with a moved list of over 64 entries wins with an angle other than 0."""
    return sum(any(b != 0 for t, b in enumerate(best_of(s, se)) if t in s.long) for se in all_searches)


VALUE_CASES = [f"{shape}-{order}" for shape in SHAPES for order in ("sorted", "shuffled")] + ["tables", "one-atom", "grid-stride", "pair-forms"]
SMALL = (40, (3, 2))               # the 40-atom, two-torsion molecule of the table, one-atom and pass cases


@functools.lru_cache(maxsize=None)
def small_molecule(order=None, table=None):
    from tscode_amd.synthetic import make_rotor_molecule
    return make_rotor_molecule(SMALL[0], list(SMALL[1]), seed=40, order=order, table=dict(table) if table else None)


@functools.lru_cache(maxsize=None)
def value_input(name):
    """(structures, Setup, pairs int32[P, 2]) of a value-level case."""
    rng = np.random.default_rng(VALUE_CASES.index(name) + 7000)
    if name.split("-")[0] in SHAPES:
        shape, order = name.split("-")
        mol = molecule(shape, "shuffle" if order == "shuffled" else None)
        S = ensemble(mol, 5, 4, seed=rng.integers(1 << 30))
        every = np.array([(i, j) for i in range(len(S)) for j in range(len(S)) if i != j], dtype=np.int32)
        return S, Setup(mol.atomnos, **mol.setup()), every[rng.choice(len(every), size=200, replace=False)]
    if name == "tables":                                  # one torsion with the single angle 0, one with a table that is no symmetry
        mol = small_molecule("shuffle", ((0, (0,)), (1, (0, 37.5, 190))))
        S = ensemble(mol, 4, 4, seed=rng.integers(1 << 30))
        return S, Setup(mol.atomnos, **mol.setup()), np.array([(i, j) for i in range(16) for j in range(16) if i != j], dtype=np.int32)
    if name == "one-atom":
        # torsion 0's subgraph is one of the atoms it turns, and that atom is the molecule's only "heavy" one: S = p q^T has rank one,
        # the top eigenvalue of Horn's matrix is double, and every value of the search and the pair's value is | |p| - |q| |
        mol = small_molecule()
        atom = int(mol.torsions[0][3])
        assert mol.move_masks[0][atom] and not mol.move_masks[1][atom]
        atomnos = np.ones_like(mol.atomnos)
        atomnos[atom] = 9
        S = ensemble(mol, 4, 4, seed=rng.integers(1 << 30))
        # (off the origin: the prune's centring is not part of the value-level form, and |p| = |q| would make every value vanish)
        S = S + np.array([0.7, -1.1, 0.4])
        return S, Setup(atomnos, mol.torsions, mol.angles, mol.move_masks, [[atom], mol.sub_nodes[1]]), \
            np.array([(i, j) for i in range(16) for j in range(16) if i != j], dtype=np.int32)
    if name == "grid-stride":                             # 9 000 draws from the ordered pairs of 80 structures of G19's molecule A
        c, s = g19_setup("n160a")
        return centred(c.structures[:80]), s, rng.integers(0, 80, size=(9000, 2)).astype(np.int32)
    assert name == "pair-forms"                           # repeated, reversed and (i, i) entries
    mol = molecule("65x2")
    S = ensemble(mol, 3, 3, seed=rng.integers(1 << 30))
    pairs = [(0, 1), (1, 0), (0, 1), (4, 4), (0, 0), (8, 2), (2, 8), (8, 2), (8, 8), (3, 5), (0, 1)]
    return S, Setup(mol.atomnos, **mol.setup()), np.array(pairs, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def value_expected(name):
    """The restatement on every distinct pair of the case, each on a private copy: (rmsd f64[P], best f64[P, T], searches per pair)."""
    S, s, pairs = value_input(name)
    done = {}
    for i, j in map(tuple, pairs.tolist()):
        if (i, j) not in done:
            searches = []
            done[(i, j)] = (*rot_corr_rmsd(S[i], S[j].copy(), s, searches), searches)
    rows = [done[p] for p in map(tuple, pairs.tolist())]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]).reshape(len(rows), len(s.torsions)), [r[2] for r in rows]


# name -> (molecule, clusters, members per cluster, the passes (d, k, num_active) of ONE run, in order).  A case's seed is its place in
# its table (here and in VALUE_CASES): new cases go to the end.
PASS_CASES = {
    "len-1-and-17": ("small", 4, 10, [(1, 24, 40)]),             # 23 chunks of one row, the last one [23, 40): longer than d
    "len-2": ("small", 4, 10, [(2, 16, 40)]),                    # 15 chunks of 2, then [30, 40)
    "len-8": ("small", 4, 10, [(8, 5, 40)]),                     # a row's j fill one batch at most
    "len-9": ("small", 4, 10, [(9, 4, 40)]),                     # one j past a batch; the last chunk is [27, 40)
    "len-17": ("small", 4, 10, [(17, 2, 40)]),                   # two batches and one j; the last chunk is [17, 40)
    "active-below-n": ("small", 4, 10, [(8, 5, 35)]),            # the last chunk is [32, 35)
    # d k < N and an empty last chunk [20, 15), while the middle chunk [10, 20) walks rows past num_active: a probe of the entry point's
    # own geometry rule -- _pass_schedule never asks for it (its d k reaches N, and num_active lies in or past the last chunk's start)
    "active-below-last-chunk": ("small", 4, 10, [(10, 3, 15)]),
    "k-1-of-100": ("small", 10, 10, [(100, 1, 100)]),            # cache words 1, 2 and 3
    "two-similar-in-a-batch": ("small", 2, 12, [(24, 1, 24)]),
    "two-passes": ("small", 4, 10, [(8, 5, 40), (40, 1, 40)]),   # the second pass skips what the first one cached
    "130x5": ("130x5", 4, 6, [(24, 1, 24)]),
    "512x16": ("512x16", 4, 6, [(12, 2, 24)]),
    # a table that is no symmetry of its rotor: a turn that the kernel must drop (a similar j past the row's match, evaluated in the same
    # batch) does not come out again when a later row turns that j, as the exact symmetry turns of the other cases do
    "table-two-similar-in-a-batch": ("table", 2, 12, [(24, 1, 24)]),
    "table-len-9": ("table", 4, 10, [(9, 4, 40)]),
}
FAR_CACHE_WORDS = {"k-1-of-100"}
TWO_IN_A_BATCH = {"two-similar-in-a-batch", "table-two-similar-in-a-batch", "table-len-9"}
TABLE = ((0, (0, 37.5, 190)), (1, (0, 120, 275, 190)))


@functools.lru_cache(maxsize=None)
def pass_input(name):
    which, n_clusters, per, passes = PASS_CASES[name]
    mol = small_molecule("shuffle") if which == "small" else small_molecule("shuffle", TABLE) if which == "table" else molecule(which, "shuffle")
    S = ensemble(mol, n_clusters, per, seed=8000 + list(PASS_CASES).index(name))
    return S, Setup(mol.atomnos, **mol.setup()), passes


@functools.lru_cache(maxsize=None)
def pass_expected(name):
    """Per pass of the run: (first, pairs evaluated, the structures after it, the structures no pair of it turned, cached pairs it
    skipped), and what the guard reads: every evaluated pair's (i, j, rmsd, searches), the cache at the end, and per match the similar
    j of its batch it left out."""
    S, s, passes = pass_input(name)
    S = S.copy()
    cache, out, seen, left_out = set(), [], [], []

    def on_hit(i, j, hi):
        # the other j of the batch of 8 that holds j: the kernel evaluates them on the structures as they are now and drops the turns
        jb = i + 1 + (j - i - 1) // BATCH * BATCH
        later = [q for q in range(j + 1, min(jb + BATCH, hi)) if (i, q) not in cache]
        left_out.append((i, j, [q for q in later if rot_corr_rmsd(S[i], S[q].copy(), s)[0] < THR]))

    for d, k, num_active in passes:
        turned, skipped = set(), []
        first, ev = pass_restated(S, cache, s, d, k, num_active, THR, on_pair=lambda i, j, r, se: (turned.add(j), seen.append((i, j, r, se))), on_hit=on_hit,
                                  on_skip=lambda i, j: skipped.append((i, j)))
        out.append((first, ev, S.copy(), sorted(set(range(len(S))) - turned), len(skipped)))
    return out, seen, cache, left_out


PRUNE_SHAPE, PRUNE_CLUSTERS, PRUNE_PER, PRUNE_SEED = "130x5", 8, 15, 9000


@functools.lru_cache(maxsize=None)
def prune_input():
    mol = molecule(PRUNE_SHAPE, "shuffle")
    return raw_ensemble(mol, PRUNE_CLUSTERS, PRUNE_PER, PRUNE_SEED), Setup(mol.atomnos, **mol.setup())           # (not centred: the prune does that)


@functools.lru_cache(maxsize=None)
def prune_expected():
    S, s = prune_input()
    seen = []
    return (*prune_restated(S, s, THR, on_pair=lambda i, j, r, se: seen.append((i, j, r, se))), seen)


def assert_searches_decided(s, searches, what):
    """Either the torsion turns no atom of its subgraph (every angle then sees bit-identical inputs and angle 0 wins in any
    implementation), or the winning value is more than ANGLE_BAND below every other one."""
    for t, values in searches:
        if not s.sub_moves[t]:
            assert len(set(values)) == 1, (what, t, values)
            continue
        order = np.sort(values)
        assert len(values) == 1 or order[1] - order[0] > ANGLE_BAND, (what, t, values)


GUARDS = [f"value:{n}" for n in VALUE_CASES] + [f"pass:{n}" for n in PASS_CASES] + ["prune"]


@pytest.mark.parametrize("what", GUARDS)
def test_sweep_inputs_meet_the_conditions_the_gpu_tests_lean_on(what):
    """With the restatement alone, on the first draw of every committed seed, for every pair the case evaluates."""
    kind, _, name = what.partition(":")
    if kind == "value":
        S, s, pairs = value_input(name)
        rmsd, best, searches = value_expected(name)
        for p, se in zip(pairs.tolist(), searches):
            assert_searches_decided(s, se, (what, p))
        assert np.isfinite(rmsd).all()
        n, T = S.shape[1], len(s.torsions)
        shape = name.split("-")[0]
        if shape in SHAPES:
            assert (n, T) == tuple(map(int, shape.split("x"))) and len(pairs) == 200
            assert (lds_bytes(T, n) > 64 * 1024) == (shape in ("330x2", "512x16"))
            assert shape != "330x2" or lds_bytes(T, n) == 67_072
            assert shape != "512x16" or lds_bytes(T, n) > 128 * 1024
            moved = s.masks.sum(axis=1)
            assert (moved.max() > 64) == (shape in LONG_MOVED) == bool(s.long) and moved.min() < 64
            if s.long:                                        # ... and its search has a turn to find in a good share of the pairs
                assert long_list_turns(s, searches) > 50, long_list_turns(s, searches)
            assert n > 64 and (shape == "65x2" or len(s.heavy) > 64)
            if shape in ("130x5", "512x16"):
                assert max(map(len, s.subs)) > 64 and min(map(len, s.subs)) < 64
            prefix = np.array_equal(s.heavy, np.arange(len(s.heavy)))
            assert prefix == name.endswith("sorted")
            if not prefix:                                    # heavy atoms and hydrogens interleave; the subgraphs sit scattered but are listed sorted
                assert all((np.diff(sub) > 0).all() for sub in s.subs)
            if shape == "512x16":
                assert {len(a) for a in s.angles} == {2, 3, 4, 6}
            # both outcomes of a search: torsions left as they are and torsions that need a turn
            assert (best != 0).any(axis=1).sum() > 20 and (best == 0).any()
        elif name == "tables":
            assert s.angles == [(0.0,), (0.0, 37.5, 190.0)] and not best[:, 0].any() and {0.0, 37.5, 190.0} == set(best[:, 1].tolist())
        elif name == "one-atom":
            assert len(s.heavy) == 1 and len(s.subs[0]) == 1 and s.sub_moves[0]
            a = s.heavy[0]
            for (i, j), r, b in zip(pairs.tolist(), rmsd, best):          # the value in closed form, after the best turns
                q = S[j].copy()
                for tor, mask, angle in zip(s.torsions, s.masks, b):
                    turn(q, int(tor[1]), int(tor[2]), mask, angle)
                assert abs(r - abs(np.linalg.norm(S[i][a]) - np.linalg.norm(q[a]))) < 1e-13
            assert rmsd.min() > 1e-6 and len(set(best[:, 0].tolist())) == 3
        elif name == "grid-stride":
            assert len(pairs) == 9000 > 1024 * BATCH and (pairs[:, 0] == pairs[:, 1]).any()
            late = set(map(tuple, pairs[1024 * BATCH:].tolist()))
            assert len(late - set(map(tuple, pairs[:1024 * BATCH].tolist()))) > 50        # pairs that occur past the first sweep of the grid only
        else:
            assert name == "pair-forms"
            assert rmsd[0] == rmsd[2] == rmsd[10] and rmsd[0] != rmsd[1] and rmsd[5] == rmsd[7]
            assert np.abs(rmsd[[3, 4, 8]]).max() < 1e-6            # (i, i): a structure against itself
        return
    if kind == "pass":
        S, s, passes = pass_input(name)
        out, seen, cache, left_out = pass_expected(name)
        assert 24 <= len(S) <= 100
    else:
        S, s = prune_input()
        kept, mask, stats, seen = prune_expected()
        assert len(S) == 120 and S.shape[1] == 130 and len(s.torsions) == 5
        ran = [st for st in stats if st["ran"]]
        assert len(ran) >= 3 and ran[0]["k"] == 20 and sum(st["pairs_evaluated"] > 0 for st in ran) >= 3 and 2 <= mask.sum() < len(S)
    assert seen
    for i, j, r, se in seen:
        assert abs(r - THR) > RMSD_BAND, (what, i, j, r)
        assert_searches_decided(s, se, (what, i, j))
    similar = sum(r < THR for _, _, r, _ in seen)
    assert 0 < similar < len(seen), (what, similar, len(seen))              # both outcomes
    if name in FAR_CACHE_WORDS:
        assert {j >> 5 for _, j in cache} == {0, 1, 2, 3} and any(j >= 64 for _, j in cache)
    if name in TWO_IN_A_BATCH:
        assert any(len(more) >= 1 for _, _, more in left_out), left_out
    if name == "two-passes":
        (_, ev1, _, _, skipped1), (_, ev2, _, _, skipped2) = out
        assert ev1 > 0 and skipped1 == 0 and ev2 > 0 and skipped2 > 20
    if name in ("130x5", "512x16"):
        assert (S.shape[1], len(s.torsions)) == tuple(map(int, name.split("x"))) and len(S) == 24
    if name in ("130x5", "512x16"):                           # the moved list of over 64 entries wins with a turn in a good share of the pairs
        assert s.long and long_list_turns(s, [se for _, _, _, se in seen]) > len(seen) // 5, long_list_turns(s, [se for _, _, _, se in seen])


# ===================================================================================================== 4. the comparisons
def compare_values(name, rot_corr_pairs):
    """rot_corr_pairs(structures, atomnos, torsions, angles, move_masks, sub_nodes, pairs) -> (rmsd, best) against the restatement."""
    S, s, pairs = value_input(name)
    rmsd, best, _ = value_expected(name)
    before = S.tobytes()
    got_r, got_b = rot_corr_pairs(S, **s.kwargs(), pairs=pairs)
    assert S.tobytes() == before, "structures changed"
    assert got_r.shape == rmsd.shape and got_b.shape == best.shape
    wrong = np.flatnonzero((got_b != best).any(axis=1))
    assert len(wrong) == 0, (name, len(wrong), "pairs with another best angle; the first:", pairs[wrong[0]].tolist(), got_b[wrong[0]].tolist(),
                             best[wrong[0]].tolist())
    err = np.abs(got_r - rmsd)
    print(f"\nrot_corr_pairs {name}: {len(pairs)} pairs, max |rmsd - restated| {err.max():.3e}")
    assert err.max() < RMSD_TOL, (name, float(err.max()), int(err.argmax()))


def compare_passes(name, make_run):
    """make_run(structures, Setup) -> an object with run_pass(d, k, num_active, thr) -> (first, pairs evaluated), end() -> structures."""
    S, s, passes = pass_input(name)
    out, _, _, _ = pass_expected(name)
    run = make_run(S.copy(), s)
    try:
        before = S
        for (d, k, num_active), (first, ev, after, untouched, _) in zip(passes, out):
            got_first, got_ev = run.run_pass(d, k, num_active, THR)
            got = run.end()
            assert np.array_equal(got_first, first), (name, (d, k, num_active), got_first.tolist(), first.tolist())
            assert got_ev == ev, (name, (d, k, num_active), got_ev, ev)
            assert got[untouched].tobytes() == before[untouched].tobytes(), (name, (d, k, num_active), "a structure no evaluated pair turns has changed")
            err = np.abs(got - after).max()
            print(f"\nrot_corr pass {name} {(d, k, num_active)}: {ev} pairs, max |coordinate - restated| {err:.3e}")
            assert err < COORD_TOL, (name, (d, k, num_active), float(err))
            before = got
    finally:
        run.close()


def compare_prune(prune, last_stats):
    S, s = prune_input()
    kept, mask, stats, _ = prune_expected()
    got_kept, got_mask = prune(S, **s.kwargs(), max_rmsd=THR, max_structures=None)
    assert np.array_equal(got_mask, mask), (int(got_mask.sum()), int(mask.sum()))
    assert last_stats() == stats
    err = np.abs(got_kept - kept).max()
    print(f"\nprune_rmsd_rot_corr_arrays: {int(mask.sum())} of {len(S)} kept, max |coordinate - restated| {err:.3e}")
    assert err < COORD_TOL, err


# ===================================================================================================== 5. on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", VALUE_CASES)
def test_rot_corr_pairs_against_the_restatement(name):
    import tscode_amd
    compare_values(name, tscode_amd.rot_corr_pairs)


def engine_run(structures, s):
    import tscode_amd
    from tscode_amd.rot_corr import _Run, _Setup
    k = s.kwargs()
    return _Run(tscode_amd.get_engine(), structures, _Setup(structures.shape[1], k["atomnos"], k["torsions"], k["angles"], k["move_masks"], k["sub_nodes"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PASS_CASES))
def test_rot_corr_pass_against_the_restatement(name):
    compare_passes(name, engine_run)


@pytest.mark.gpu
def test_whole_prune_against_the_restatement():
    import tscode_amd
    compare_prune(tscode_amd.prune_rmsd_rot_corr_arrays, tscode_amd.last_rot_corr_stats)


def abi_pairs(structures, n_atoms, heavy, torsions, angles, n_angles, masks, sub_ptr, sub_idx, pairs):
    """tsc_rot_corr_pairs on raw host arrays; returns the call's status."""
    import tscode_amd
    from tscode_amd._lib import ptr
    eng = tscode_amd.get_engine()
    arrays = [np.ascontiguousarray(a, dtype=t) for a, t in ((structures, np.float64), (heavy, np.int32), (torsions, np.int32), (angles, np.float64),
                                                            (n_angles, np.int32), (masks, np.uint8), (sub_ptr, np.int32), (sub_idx, np.int32),
                                                            (pairs, np.int32))]
    st, hv, to, an, na, ma, sp, si, pa = arrays
    rmsd, best = np.empty(len(pa)), np.empty((len(pa), len(to)))
    return eng.lib.tsc_rot_corr_pairs(eng._h, ptr(st), C.c_int64(len(st)), C.c_int(n_atoms), ptr(hv), C.c_int(len(hv)), ptr(to), C.c_int(len(to)),
                                      ptr(an), ptr(na), ptr(ma), ptr(sp), ptr(si), ptr(pa), C.c_int64(len(pa)), ptr(rmsd), ptr(best))


@pytest.mark.gpu
def test_refusals_come_before_any_launch():
    """Every call here returns TSC_ERR_INVALID from the host-side checks; the last one is the empty call."""
    import tscode_amd
    from tscode_amd._lib import TscodeHipError
    # 513 atoms through the C ABI, every array sized for them
    n = 513
    args = dict(structures=np.zeros((2, n, 3)), n_atoms=n, heavy=np.arange(n), torsions=[[0, 1, 2, 3]], angles=np.zeros((1, 6)), n_angles=[1],
                masks=np.zeros((1, n)), sub_ptr=[0, 2], sub_idx=[1, 2], pairs=[[0, 1]])
    assert abi_pairs(**args) == -1
    assert abi_pairs(**{**args, "structures": np.zeros((2, 512, 3)), "n_atoms": 512, "heavy": np.arange(512), "masks": np.zeros((1, 512)),
                        "sub_idx": [1, 512]}) == -1
    S, s, pairs = value_input("pair-forms")
    k = s.kwargs()
    for bad in ([len(k["atomnos"])], [-1]):                       # a subgraph index out of range
        with pytest.raises(TscodeHipError) as e:
            tscode_amd.rot_corr_pairs(S, **{**k, "sub_nodes": [k["sub_nodes"][0], bad]}, pairs=pairs)
        assert e.value.code == -1
    for bad in ([(0, len(S))], [(-1, 0)]):                        # a pair index out of range
        with pytest.raises(TscodeHipError) as e:
            tscode_amd.rot_corr_pairs(S, **k, pairs=bad)
        assert e.value.code == -1
    run = engine_run(S.copy(), s)
    try:
        N = len(S)
        for d, kk, na, thr in ((N // 2 + 1, 2, N, THR), (0, 1, N, THR), (N, 1, N, np.nan), (N, 1, N, np.inf)):
            with pytest.raises(TscodeHipError) as e:
                run.run_pass(d, kk, na, thr)
            assert e.value.code == -1
        assert run.end().tobytes() == S.tobytes()                 # nothing ran
    finally:
        run.close()
    r, b = tscode_amd.rot_corr_pairs(S, **k, pairs=np.zeros((0, 2), dtype=np.int32))
    assert r.shape == (0,) and b.shape == (0, len(s.torsions))
