"""G24 generator: the reference's own conformational-search loops over MANY start structures.  Runs ONLY in the build
container, never where the GPU tests run; it imports the reference's Python through tests/golden/_reference.py and records arrays the
reference produced -- none of its text -- in tests/golden/G24_csearch_multi.npz.

Part A: ``clustered_csearch`` (tscode/torsion_module.py:655-847) on a 40-atom diene, CH3-(CH2)2-CH=CH-(CH2)3-CH=CH-(CH2)3-CH3,
folded by seeded random rotations about its own torsions.  The graph is the reference's ``graphize``, the torsions its
``_get_torsions`` (9 of them), the groups its ``_group_torsions_dbscan`` (the two double bonds are what separates them in space).
The reference picks the starting points of the next group with ``most_diverse_conformers``, whose k-means is unseeded
(scikit-learn's default initialisation) and has no reproducible result: in the imported module that name is replaced by a
recorder that returns ``structures[:n]``, and ``prune_conformers_tfd`` by a recorder that runs the real function.  What is pinned
is therefore the candidate loop (:734-783) of every group for the starting points it was given -- not the pick between groups.

Part B: ``random_csearch`` (:399-521), once per start, on three conformers of that molecule.  Every start has its own torsion
list (a subset, another order, one torsion reversed) and its own seeded, shuffled table.  Two runs: one that stops on ``n_out``,
and one with a large ``n_out`` and a ``max_tries`` that is a kept row of start 1's table and the all-zero (dropped) row of start
2's table, which therefore does not stop there (:505-511).

Usage:  python -B tests/golden/gen_csearch_multi.py
"""

from __future__ import annotations

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
import tscode.utils as ref_utils            # noqa: E402
from tscode.algebra import all_dists        # noqa: E402
from tscode.graph_manipulations import graphize   # noqa: E402

QUIET = dict(logfunction=lambda *a, **k: None, interactive_print=False)
THRESH = 1.5                                # the reference's only value (:485, :759)
N_KEEP = 3                                  # clustered_csearch's n: starting points handed to the next group


def _unit(v):
    return v / np.linalg.norm(v)


def build_diene():
    """Planar zig-zag backbone of 14 carbons (double bonds C3=C4 and C8=C9, trans), hydrogens at ideal angles."""
    double = {(3, 4), (8, 9)}
    n_c = 14
    c = [np.zeros(3)]
    for i in range(1, n_c):
        length = 1.34 if (i - 1, i) in double else 1.52
        ang = np.deg2rad(28.0 if i % 2 else -28.0)
        c.append(c[-1] + length * np.array([np.cos(ang), np.sin(ang), 0.0]))
    c = np.array(c)
    sp2 = {a for b in double for a in b}
    coords, atomnos = list(c), [6] * n_c
    z = np.array([0.0, 0.0, 1.0])
    for i in range(n_c):
        if i in (0, n_c - 1):                                     # CH3: staggered about the bond
            d = _unit(c[i] - c[1 if i == 0 else n_c - 2])
            p = _unit(np.cross(d, z))
            for k in range(3):
                w = np.deg2rad(90.0 + 120.0 * k)
                coords.append(c[i] + 1.09 * (np.cos(np.deg2rad(70.5)) * d + np.sin(np.deg2rad(70.5)) * (np.cos(w) * p + np.sin(w) * z)))
                atomnos.append(1)
            continue
        out = _unit(2 * c[i] - c[i - 1] - c[i + 1])
        if i in sp2:
            coords.append(c[i] + 1.08 * out)
            atomnos.append(1)
        else:
            for sgn in (1.0, -1.0):
                coords.append(c[i] + 1.09 * (np.cos(np.deg2rad(54.75)) * out + sgn * np.sin(np.deg2rad(54.75)) * z))
                atomnos.append(1)
    return np.array(coords), np.array(atomnos)


def edges_of(graph):
    return sorted((min(a, b), max(a, b)) for a, b in graph.edges if a != b)


class Notes:
    """Note-taking wrappers around the reference's rotate_dihedral / torsion_comp_check (installed in the imported module)."""

    def __init__(self):
        self.real_rd, self.real_cc = ref_tm.rotate_dihedral, ref_tm.torsion_comp_check
        self.walkbacks_ok, self.margin, self.last_rot = 0, np.inf, None

    def rd(self, coords, dihedral, angle, mask=None, indices_to_be_moved=None):
        self.last_rot = angle
        return self.real_rd(coords, dihedral, angle, mask=mask, indices_to_be_moved=indices_to_be_moved)

    def cc(self, coords, torsion, mask, thresh=1.5, max_clashes=0):
        ok = self.real_cc(coords, torsion=torsion, mask=mask, thresh=thresh, max_clashes=max_clashes)
        anti = ~mask
        anti[torsion[1]] = anti[torsion[2]] = False
        if mask.any() and anti.any():
            self.margin = min(self.margin, float(np.abs(all_dists(coords[anti], coords[mask]) - thresh).min()))
        if ok and self.last_rot == -5:
            self.walkbacks_ok += 1
        return ok

    def __enter__(self):
        ref_tm.rotate_dihedral, ref_tm.torsion_comp_check = self.rd, self.cc
        return self

    def __exit__(self, *exc):
        ref_tm.rotate_dihedral, ref_tm.torsion_comp_check = self.real_rd, self.real_cc


def segments(array, starts):
    """Rows of ``array`` per starting point: every segment begins with the start itself (:741), bit for bit."""
    heads = []
    at = 0
    for sp in starts:
        while not np.array_equal(array[at], sp):
            at += 1
        heads.append(at)
        at += 1
    return np.diff(heads + [len(array)]) - 1


def part_a(seed):
    base, atomnos = build_diene()
    graph = graphize(base, atomnos)
    bonds = edges_of(graph)
    torsions = ref_tm._get_torsions(graph, [], ref_utils.get_double_bonds_indices(base, atomnos))
    for t in torsions:
        t.sort_torsion(graph, np.array([]))
    assert len(torsions) >= 9, len(torsions)
    rng = np.random.default_rng(seed)
    coords = base.copy()
    for t in torsions:                                               # fold: a random turn about every rotatable bond
        coords = ref_tm.rotate_dihedral(coords, t.torsion, float(rng.uniform(0.0, 360.0)), mask=ref_tm._get_rotation_mask(graph, t.torsion))
    if edges_of(graphize(coords, atomnos)) != bonds:                 # the fold made or broke a bond: not this molecule any more
        return None
    groups = ref_tm._group_torsions_dbscan(coords, torsions, max_size=5)
    if len(groups) < 2:
        return None
    picks, tfd_in = [], []
    real_mdc, real_tfd = ref_tm.most_diverse_conformers, ref_tm.prune_conformers_tfd

    def mdc(n, structures, torsion_array, energies=None, interactive_print=False):
        picks.append((np.array(structures), np.array(structures[:n])))
        return np.array(structures[:n])

    def tfd(structures, torsion_array, *a, **k):
        tfd_in.append(np.array(structures))
        return real_tfd(structures, torsion_array, *a, **k)

    ref_tm.most_diverse_conformers, ref_tm.prune_conformers_tfd = mdc, tfd
    try:
        with Notes() as notes:
            out = ref_tm.clustered_csearch(coords.copy(), atomnos, torsions, graph, constrained_indices=np.array([]), n=N_KEEP, n_out=10**6,
                                           mode=1, **QUIET)
    finally:
        ref_tm.most_diverse_conformers, ref_tm.prune_conformers_tfd = real_mdc, real_tfd
    if len(picks) != len(groups) - 1:                                # a group that built no more than n structures: no cut
        return None
    starts = [coords[None]] + [p[1] for p in picks]
    tail = tfd_in[-1][sum(len(p[1]) for p in picks):]               # the last group's array: what :823 appended after the cuts
    cands = [p[0] for p in picks] + [tail]
    rec = {"a_seed": seed, "a_n_groups": len(groups), "a_atomnos": atomnos, "a_bonds": np.array(bonds), "a_n_keep": N_KEEP,
           "a_n_final": len(out)}
    differing = False
    for g, group in enumerate(groups):
        angles = ref_utils.cartesian_product(*[t.get_angles() for t in group])
        kept = segments(cands[g], starts[g])
        if len(starts[g]) < (1 if g == 0 else 3) or kept.sum() + len(starts[g]) != len(cands[g]):
            return None
        differing |= len(set(kept.tolist())) > 1
        dropped = len(starts[g]) * len(angles) - kept.sum()
        rec.update({f"a_starts{g}": starts[g], f"a_torsions{g}": np.array([t.torsion for t in group], dtype=np.int32),
                    f"a_masks{g}": np.array([ref_tm._get_rotation_mask(graph, t.torsion) for t in group]),
                    f"a_nfolds{g}": np.array([t.n_fold for t in group]), f"a_angles{g}": angles.astype(np.int32), f"a_out{g}": cands[g],
                    f"a_kept_per_start{g}": kept})
        print(f"  part A seed {seed} group {g}: {len(group)} torsions {[t.n_fold for t in group]}-fold, {len(starts[g])} starts x {len(angles)} rows, "
              f"kept per start {kept.tolist()}, {dropped} dropped")
    print(f"  part A seed {seed}: {notes.walkbacks_ok} walk-backs succeeded, margin {notes.margin:.3e}, starts keep different numbers: {differing}")
    if not (differing and notes.walkbacks_ok >= 1 and notes.margin > 1e-9):
        return None
    rec["a_walkbacks_ok"], rec["a_margin"] = notes.walkbacks_ok, notes.margin
    return rec, (coords, atomnos, graph, torsions, cands)


def run_random(coords, atomnos, graph, tors, seed, n_out, max_tries):
    np.random.seed(seed)
    return ref_tm.random_csearch(coords.copy(), atomnos, tors, graph, n_out=n_out, max_tries=max_tries, **QUIET)


def part_b(ctx, seed0):
    coords0, atomnos, graph, torsions, cands = ctx
    starts = np.array([coords0, cands[0][-1], cands[-1][-1]])        # conformers of the one molecule: the fold and two of part A's
    quads = [t.torsion for t in torsions]
    lists = [[quads[0], quads[2], quads[3], quads[5]],                                   # a subset
             [quads[6], quads[1], quads[4], quads[0]],                                   # another subset in another order
             [quads[2], tuple(reversed(quads[7])), quads[5], quads[8]]]                  # one torsion reversed
    folds = {q: t.n_fold for q, t in zip(quads, torsions)}
    tors = []
    for lst in lists:
        row = []
        for q in lst:
            t = ref_tm.Torsion(*[int(i) for i in q])
            t.n_fold = folds[q if q in folds else tuple(reversed(q))]
            row.append(t)
        tors.append(row)
    big = 10**6
    for seed in range(seed0, seed0 + 200):
        seeds = [seed, seed + 1000, seed + 2000]
        tables = []
        for s in range(3):
            tab = ref_utils.cartesian_product(*[t.get_angles() for t in tors[s]])
            np.random.seed(seeds[s])
            np.random.shuffle(tab)                                   # the table random_csearch will walk (same seed, same call)
            tables.append(tab)
        m = int(np.flatnonzero(~tables[2].any(axis=1))[0])           # start 2: row max_tries is the all-zero row, dropped
        if not 5 <= m < len(tables[2]) - 10:
            continue
        with Notes() as notes:
            full = [run_random(starts[s], atomnos, graph, tors[s], seeds[s], big, big) for s in range(3)]
            n_out = 7
            run0 = [run_random(starts[s], atomnos, graph, tors[s], seeds[s], n_out, 10000) for s in range(3)]
            run1 = [run_random(starts[s], atomnos, graph, tors[s], seeds[s], big, m) for s in range(3)]
        # start 1: row m is kept, so the walk stops there; start 2: it is not, so the walk goes to the end of the table
        if not (len(run1[1]) < len(full[1]) and len(run1[2]) == len(full[2]) and tables[1][m].any() and notes.margin > 1e-9):
            continue
        assert all(len(r) == n_out for r in run0)
        rec = {"b_n_starts": 3, "b_starts": starts, "b_seeds": np.array(seeds), "b_n_out0": n_out, "b_max_tries0": 10000, "b_n_out1": big,
               "b_max_tries1": m, "b_margin": notes.margin, "b_walkbacks_ok": notes.walkbacks_ok}
        for s in range(3):
            rec[f"b_torsions{s}"] = np.array([t.torsion for t in tors[s]], dtype=np.int32)
            rec[f"b_masks{s}"] = np.array([ref_tm._get_rotation_mask(graph, t.torsion) for t in tors[s]])
            rec[f"b_angles{s}"] = tables[s].astype(np.int32)
            rec[f"b_full_count{s}"] = len(full[s])
        for r, run in enumerate((run0, run1)):
            rec[f"b_out{r}"] = np.concatenate(run)
            rec[f"b_counts{r}"] = np.array([len(x) for x in run])
        print(f"  part B seeds {seeds}: tables of {[len(t) for t in tables]} rows, kept in full {[len(f) for f in full]}; n_out {n_out}: "
              f"{rec['b_counts0'].tolist()}; max_tries {m}: {rec['b_counts1'].tolist()}; {notes.walkbacks_ok} walk-backs succeeded, "
              f"margin {notes.margin:.3e}")
        return rec
    raise SystemExit("part B: no seed met the conditions")


def main():
    print("G24 csearch over many starts: the reference's clustered_csearch and random_csearch")
    for seed in range(9124, 9124 + 400):
        got = part_a(seed)
        if got is not None:
            break
    else:
        raise SystemExit("part A: no seed met the conditions")
    rec, ctx = got
    rec.update(part_b(ctx, 24))
    dropped_nonzero = any((rec[f"a_kept_per_start{g}"] < len(rec[f"a_angles{g}"]) - 1).any() for g in range(rec["a_n_groups"]))
    assert dropped_nonzero, "no candidate with a non-zero angle was dropped"
    path = os.path.join(HERE, "G24_csearch_multi.npz")
    np.savez_compressed(path, **rec)
    print(f"  wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
