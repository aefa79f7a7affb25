"""G26 generator: the reference's torsion grouping and its whole clustered conformational search, mode 1.  Runs ONLY in the build
container, never where the GPU tests run; it imports the reference's Python through tests/golden/_reference.py (and scikit-learn)
and records arrays the reference produced -- none of its text -- in tests/golden/G26_clustered_csearch.npz, and the modules that
bind ``clustered_csearch`` / ``_group_torsions_dbscan`` by name, read off the reference's import lines, in
tests/golden/G26_clustered_csearch_sites.json.

Part A: ``_group_torsions_dbscan`` (tscode/torsion_module.py:373-397) itself, on torsion lists over synthetic coordinates:
T = 8, 9, 10, 33, 64, 65 and 130 torsions with ``max_size`` 5 and 3, centres drawn at random in a box, plus designed cases -- blobs
25 A apart (level 10.0 is kept; blob sizes repeat, which pins the stable order of equal groups), pairs 6.2 A apart (an interior
level), a chain 2.2 A apart (level 2.0), and a line of centres 1.9 A apart, which every level links: the fall-through of the
reference's loop and a component that closes only by transitivity.  While the reference runs, ``tm.dbscan`` is a wrapper that
notes the level of every call; the last one is the level kept.  The function has no ``len(torsions) < 9`` branch: that is its
caller's (:689), so for T = 8 the fixture holds what the function returns and the test derives the caller's single group.
Guard band, enforced by drawing again with the next seed (the seed recorded): every pair distance of the centres is at least
1e-6 A away from all seventeen levels.  No case is left out.

Part B: ``clustered_csearch`` (:655-847), mode 1, n = 6, n_out = 8, on the 40-atom diene of G24 from three folded poses, so that
the trim between groups and the final pick both run.  While it runs, ``tm.KMeans`` is gen_diverse.py's recording wrapper (init
rows drawn from a recorded seed, scikit-learn's Lloyd from ``X[init_rows]``); the rows are kept per (pose, call), the call being
the number of the ``most_diverse_conformers`` call of that pose.  Guard bands, enforced the same way (a pose is folded again with
the next seed):
  * G20's bands at every k-means call: label margin >= 1e-6 A^2 at every Lloyd iteration and no empty cluster, best and
    second-best cumdist of a cluster >= 1e-6 apart, Horn's top eigenvalue separated by >= 1e-3 relative;
  * every distance torsion_comp_check compares with 1.5 A is >= 1e-6 A away from it;
  * every sum that tfd_similarity compares with its threshold is >= 1e-3 degrees away from it (G8's generator enforces no band;
    the fingerprints are float32, nine of them summed: 1e-3 is ten times their rounding).
Recorded per pose: the coordinates, the reference's torsions, folds and groups, the size of every round's ``new_structures``
before and after the trim, the init rows and the final structures.

Usage:  python -B tests/golden/gen_clustered_csearch.py
"""

from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_diverse as GD                    # noqa: E402  (installs the stand-ins, restates rmsd.kabsch, imports the reference)
import gen_csearch_multi as GM              # noqa: E402  (the diene, the note-taking wrappers)

import sklearn                              # noqa: E402
import tscode.numba_functions as ref_nf     # noqa: E402
import tscode.torsion_module as ref_tm      # noqa: E402
import tscode.utils as ref_utils            # noqa: E402
from tscode.graph_manipulations import graphize   # noqa: E402

LEVELS = np.arange(10, 1.5, -0.5)
DIST_BAND, COMP_BAND, TFD_BAND = 1e-6, 1e-6, 1e-3
N_KEEP, N_OUT = 6, 8
QUIET = dict(logfunction=lambda *a, **k: None, interactive_print=False)


# ------------------------------------------------------------------------------------------------------- part A
def centres_for(design, T, rng):
    if design == "box":                                     # uniform in a box whose side grows with T: the level depends on the draw
        return rng.uniform(0.0, 4.0 * T ** (1.0 / 3.0) + 4.0, size=(T, 3))
    if design == "blobs":                                   # blobs of 1 .. 3 centres, 25 A apart, sizes repeating
        sizes, out = [3, 2, 2, 1, 3, 1, 2], []
        b = 0
        while len(out) < T:
            k = min(sizes[b % len(sizes)], T - len(out))
            origin = np.array([25.0 * (b % 4), 25.0 * (b // 4 % 4), 25.0 * (b // 16)])
            out += list(origin + rng.uniform(-1.0, 1.0, size=(k, 3)))
            b += 1
        return np.array(out)[rng.permutation(T)]
    if design == "pairs":                                   # pairs 1 A wide, 6.2 A apart along a line: joined down to 5.5, apart from 5.0 on
        x = np.array([6.2 * (t // 2) + 1.0 * (t % 2) for t in range(T)])
        return np.stack([x, np.zeros(T), np.zeros(T)], axis=1) + rng.uniform(-0.01, 0.01, size=(T, 3))
    if design in ("chain", "line"):                         # 2.2 A apart: single at 2.0; 1.9 A apart: one cluster at every level
        step = 2.2 if design == "chain" else 1.9
        order = rng.permutation(T) if design == "line" else np.arange(T)     # (neighbours in space are not neighbours in the list)
        return np.stack([step * order, np.zeros(T), np.zeros(T)], axis=1) + rng.uniform(-0.01, 0.01, size=(T, 3))
    raise ValueError(design)


def make_case(design, T, max_size, seed):
    """Atoms placed so that the torsions' centres are the drawn ones; None when a pair distance is inside the guard band."""
    rng = np.random.default_rng(seed)
    centres = centres_for(design, T, rng)
    n = 2 * T + 3
    place = rng.permutation(n)
    coords = rng.uniform(-5.0, 5.0, size=(n, 3))
    quads = np.zeros((T, 4), dtype=np.int32)
    for t in range(T):
        half = rng.normal(size=3)
        half *= 0.76 / np.linalg.norm(half)
        i2, i3 = place[2 * t], place[2 * t + 1]
        coords[i2], coords[i3] = centres[t] + half, centres[t] - half
        others = [int(a) for a in rng.choice(n, size=4, replace=False) if a not in (i2, i3)][:2]
        quads[t] = (others[0], i2, i3, others[1])
    real = np.array([np.mean((coords[i2], coords[i3]), axis=0) for _, i2, i3, _ in quads])
    d = np.linalg.norm(real[:, None] - real[None], axis=-1)[np.triu_indices(T, 1)]
    margin = float(np.abs(d[:, None] - LEVELS[None]).min()) if len(d) else np.inf
    if margin < DIST_BAND:
        return None
    torsions = [types.SimpleNamespace(torsion=tuple(int(i) for i in q), index=t) for t, q in enumerate(quads)]
    seen = []
    real_dbscan = ref_tm.dbscan

    def noting(X, eps=0.5, min_samples=5, **kw):
        got = real_dbscan(X, eps=eps, min_samples=min_samples, **kw)
        seen.append((float(eps), int(np.bincount(got[1]).max())))
        return got

    ref_tm.dbscan = noting
    try:
        groups = ref_tm._group_torsions_dbscan(coords, torsions, max_size=max_size)
    finally:
        ref_tm.dbscan = real_dbscan
    group_of = np.full(T, -1, dtype=np.int32)
    for g, members in enumerate(groups):
        idx = [t.index for t in members]
        assert idx == sorted(idx)
        group_of[idx] = g
    assert (group_of >= 0).all()
    eps, biggest = seen[-1]
    return dict(coords=coords, torsions=quads, group_of=group_of, n_groups=len(groups), eps_index=int(np.flatnonzero(LEVELS == eps)[0]),
                oversize=int(biggest > max_size), margin=margin, sizes=[len(g) for g in groups])


def part_a():
    plan = [("box", T, ms) for T in (8, 9, 10, 33, 64, 65, 130) for ms in (5, 3)]
    plan += [("blobs", 10, 5), ("blobs", 10, 3), ("blobs", 65, 3), ("pairs", 33, 5), ("pairs", 130, 3), ("chain", 9, 5), ("chain", 64, 3),
             ("line", 10, 5), ("line", 65, 3), ("line", 130, 5)]
    arrays, cases = {}, []
    for k, (design, T, ms) in enumerate(plan):
        for attempt in range(50):
            seed = 26000 + 100 * k + attempt
            got = make_case(design, T, ms, seed)
            if got is not None:
                break
            print(f"  part A case {k} ({design}, T = {T}): seed {seed} violates the guard band, drawn again")
        else:
            raise SystemExit(f"part A case {k}: no admissible draw")
        for name in ("coords", "torsions", "group_of"):
            arrays[f"a{k}_{name}"] = got[name]
        cases.append(dict(index=k, design=design, T=T, max_size=ms, seed=seed, n_groups=got["n_groups"], eps_index=got["eps_index"],
                          oversize=got["oversize"], margin=got["margin"], sizes=got["sizes"]))
        print(f"  part A case {k}: {design:5s} T = {T:3d} max_size {ms}: level {LEVELS[got['eps_index']]:4.1f}, oversize {got['oversize']}, "
              f"{got['n_groups']} groups, sizes {got['sizes'][:12]}{' ...' if len(got['sizes']) > 12 else ''}, margin {got['margin']:.2e}")
    by = lambda f: [c for c in cases if f(c)]
    assert by(lambda c: c["eps_index"] == 0) and by(lambda c: c["eps_index"] == 16 and not c["oversize"]) and by(lambda c: c["oversize"])
    assert by(lambda c: 0 < c["eps_index"] < 16)
    assert by(lambda c: len(set(c["sizes"])) < len(c["sizes"]) and c["n_groups"] > 1)
    return arrays, cases


# ------------------------------------------------------------------------------------------------------- part B
class Search:
    """One run of the reference's clustered_csearch with every recorder in place."""

    def __init__(self, pose, seed):
        self.pose, self.seed = pose, seed
        self.calls, self.init_rows, self.guards = 0, {}, dict(label=np.inf, pick=np.inf, horn=np.inf, tfd=np.inf, empty=0)
        self.rounds, self.kmeans_calls, self.in_mdc, self.output_len = [], 0, False, None

    def mdc(self, n, structures, torsion_array, energies=None, interactive_print=False):
        call = self.calls
        self.calls += 1
        structures = np.array(structures)
        GD.RecordingKMeans.seed, GD.RecordingKMeans.last = self.seed * 100 + call, None
        self.in_mdc = True
        try:
            out = self.real_mdc(n, structures.copy(), torsion_array, energies=energies, interactive_print=interactive_print)
        finally:
            self.in_mdc = False
        rec = GD.RecordingKMeans.last
        if rec is not None:                                  # the k-means ran: its rows and its guard values
            self.kmeans_calls += 1
            self.init_rows[call] = rec["init_rows"]
            pruned, _ = self.real_tfd(structures.copy(), torsion_array)
            _, _, gap = GD.reference_align(np.ascontiguousarray(pruned), None)
            _, _, _, _, margin, max_empty = GD.lloyd_restated(rec["X"], rec["X"][rec["init_rows"]])
            aligned = rec["X"].reshape(len(rec["X"]), -1, 3)
            pgap, _ = GD.pick_guard(aligned, rec["labels"], rec["centers"], np.arange(len(aligned), dtype=float))
            g = self.guards
            g["label"], g["pick"], g["horn"], g["empty"] = min(g["label"], margin), min(g["pick"], pgap), min(g["horn"], gap), max(g["empty"], max_empty)
        self.rounds.append((len(structures), len(out)))
        return out

    def tfd(self, structures, torsion_array, *a, **k):
        if not self.in_mdc:                                  # :827: the whole output, every round's structures one after the other
            self.output_len = len(structures)
        return self.real_tfd(structures, torsion_array, *a, **k)

    def tfd_sim(self, tfp1, tfp2, thresh=10):
        deltas = np.abs(tfp1 - tfp2)
        deltas = np.abs(deltas - (deltas > 180) * 360)
        self.guards["tfd"] = min(self.guards["tfd"], abs(float(np.sum(deltas)) - thresh))
        return self.real_sim(tfp1, tfp2, thresh=thresh)

    def run(self, coords, atomnos, torsions, graph):
        self.real_mdc, self.real_tfd, self.real_sim, real_km = ref_tm.most_diverse_conformers, ref_tm.prune_conformers_tfd, ref_nf.tfd_similarity, ref_tm.KMeans
        ref_tm.most_diverse_conformers, ref_nf.tfd_similarity, ref_tm.KMeans = self.mdc, self.tfd_sim, GD.RecordingKMeans
        ref_tm.prune_conformers_tfd = self.tfd
        try:
            with GM.Notes() as notes:
                out = ref_tm.clustered_csearch(coords.copy(), atomnos, torsions, graph, constrained_indices=np.array([]), n=N_KEEP, n_out=N_OUT,
                                               mode=1, **QUIET)
        finally:
            ref_tm.most_diverse_conformers, ref_nf.tfd_similarity, ref_tm.KMeans = self.real_mdc, self.real_sim, real_km
            ref_tm.prune_conformers_tfd = self.real_tfd
        self.guards["comp"] = notes.margin
        return np.array(out)


def fold(seed):
    """The diene folded by seeded random turns about its own torsions (gen_csearch_multi.py part A); None when the fold made or broke
    a bond or leaves fewer than two groups."""
    base, atomnos = GM.build_diene()
    graph = graphize(base, atomnos)
    bonds = GM.edges_of(graph)
    torsions = ref_tm._get_torsions(graph, [], ref_utils.get_double_bonds_indices(base, atomnos))
    for t in torsions:
        t.sort_torsion(graph, np.array([]))
    rng = np.random.default_rng(seed)
    coords = base.copy()
    for t in torsions:
        coords = ref_tm.rotate_dihedral(coords, t.torsion, float(rng.uniform(0.0, 360.0)), mask=ref_tm._get_rotation_mask(graph, t.torsion))
    if GM.edges_of(graphize(coords, atomnos)) != bonds:
        return None
    # the graph and the torsions of THIS pose, as csearch makes them (:559-615)
    graph = graphize(coords, atomnos)
    torsions = ref_tm._get_torsions(graph, [], ref_utils.get_double_bonds_indices(coords, atomnos))
    for t in torsions:
        t.sort_torsion(graph, np.array([]))
    if len(torsions) < 9:
        return None
    groups = ref_tm._group_torsions_dbscan(coords, torsions, max_size=5)
    if len(groups) < 2:
        return None
    return coords, atomnos, graph, torsions, groups


def part_b():
    arrays, poses = {}, []
    seed = 26500
    while len(poses) < 3:
        seed += 1
        if seed > 26500 + 300:
            raise SystemExit("part B: no admissible pose")
        got = fold(seed)
        if got is None:
            continue
        coords, atomnos, graph, torsions, groups = got
        run = Search(len(poses), seed)
        out = run.run(coords, atomnos, torsions, graph)
        g = run.guards
        # the trims between groups and the final pick all ran their k-means
        ok = (run.calls == len(groups) and run.kmeans_calls == run.calls and g["label"] >= GD.MARGIN_BAND and g["pick"] >= GD.PICK_BAND and
              g["horn"] >= GD.HORN_BAND and g["empty"] == 0 and g["comp"] >= COMP_BAND and g["tfd"] >= TFD_BAND)
        print(f"  part B seed {seed}: groups {[len(x) for x in groups]}, mdc calls (in, out) {run.rounds}, {len(out)} final, guards "
              f"{ {k: (float(f'{v:.3g}') if isinstance(v, float) else v) for k, v in g.items()} }: {'kept' if ok else 'drawn again'}")
        if not ok:
            continue
        p = len(poses)
        index = {t.torsion: k for k, t in enumerate(torsions)}
        group_of = np.zeros(len(torsions), dtype=np.int32)
        for k, members in enumerate(groups):
            group_of[[index[t.torsion] for t in members]] = k
        arrays.update({f"b{p}_coords": coords, f"b{p}_torsions": np.array([t.torsion for t in torsions], dtype=np.int32),
                       f"b{p}_n_folds": np.array([t.n_fold for t in torsions], dtype=np.int32), f"b{p}_group_of": group_of,
                       f"b{p}_masks": np.array([ref_tm._get_rotation_mask(graph, t.torsion) for t in torsions]), f"b{p}_out": out})
        for call, rows in run.init_rows.items():
            arrays[f"b{p}_init_rows{call}"] = rows
        # run.rounds: what every most_diverse_conformers call took and gave; the last one is the final pick on the pruned output.  The
        # last group's new_structures is what the output holds on top of the rows the trims kept.
        last = run.output_len - sum(r[1] for r in run.rounds[:-1])
        poses.append(dict(index=p, seed=seed, n_groups=len(groups), round_sizes=[list(r) for r in run.rounds[:-1]] + [[last, last]],
                          final_pick=list(run.rounds[-1]),
                          n_final=len(out), calls=run.calls, guards={k: float(v) for k, v in g.items()}))
        arrays["b_atomnos"], arrays["b_bonds"] = atomnos, np.array(GM.edges_of(graph))
    return arrays, poses


def main():
    print("G26 the reference's _group_torsions_dbscan and clustered_csearch, mode 1")
    arrays, cases = part_a()
    b_arrays, poses = part_b()
    arrays.update(b_arrays)
    meta = {"sklearn": sklearn.__version__, "numpy": np.__version__, "levels": LEVELS.tolist(), "n": N_KEEP, "n_out": N_OUT,
            "bands": {"distance": DIST_BAND, "comp": COMP_BAND, "tfd": TFD_BAND, "label": GD.MARGIN_BAND, "pick": GD.PICK_BAND, "horn": GD.HORN_BAND},
            "part_a": cases, "part_b": poses}
    arrays["meta_json"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    GD.save_npz(os.path.join(HERE, "G26_clustered_csearch.npz"), arrays)
    with open(os.path.join(HERE, "G26_clustered_csearch_sites.json"), "w") as f:
        json.dump({"sites": GD.binding_sites(["clustered_csearch", "_group_torsions_dbscan"])}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
