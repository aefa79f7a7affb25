"""The clustered conformational search of an ensemble (tscode_amd.clustered_csearch_batch) stage by stage, beside the same searches
as a loop over the structures with the per-structure functions: clustered_csearch_step per group, most_diverse_conformers between
groups and at the end, the groups made on the host in NumPy.

    python tools/clustered_csearch_profile.py [--out profiles/clustered_csearch_profile.json] [--repeats 3] [--sizes 1,16,128]

Poses: the 40-atom diene of fixture G26 (9 torsions in groups of 2, 3 and 4), its three recorded poses turned by random angles about
their own torsions; a draw that makes or breaks a bond is left out.  n = n_out = 20, one seed for every k-means, so both sides
build the same structures (the largest difference is recorded).  The set-up (torsion_sets_batch) is shared by both sides and timed on its own.  Per ensemble
size: milliseconds of the grouping (host wall and kernel), of every round's rotations and trims, and of the final prune and pick;
the loop's total; medians of --repeats after one warm-up run, with the smallest and largest value."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_KEEP = N_OUT = 20
SEED = 2626
LEVELS = np.arange(10, 1.5, -0.5)


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def host_groups(coords, torsions, max_size=5, min_torsions=9):
    """The groups of one structure in NumPy, from the definition at tsc_torsion_groups (include/tscode_hip.h)."""
    T = len(torsions)
    if T < min_torsions:
        return [np.arange(T)]
    c = (coords[torsions[:, 1]] + coords[torsions[:, 2]]) / 2
    d = c[:, None, :] - c[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    for eps in LEVELS:
        linked = d2 <= eps * eps
        first = np.arange(T)
        while True:
            new = np.where(linked, first[None, :], T).min(axis=1)
            new = new[new]
            if np.array_equal(new, first):
                break
            first = new
        _, label, sizes = np.unique(first, return_inverse=True, return_counts=True)
        if sizes.max() <= max_size:
            break
    return [np.flatnonzero(label == k) for k in np.argsort(sizes, kind="stable")]


def make_poses(count, rng):
    import tscode_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "G26_clustered_csearch.npz"))
    atomnos = g["b_atomnos"].astype(np.int64)
    want = tscode_amd.bond_graph_batch(g["b0_coords"][None], atomnos)[0]
    poses = []
    while len(poses) < count:
        drawn = []
        for k in range(2 * (count - len(poses)) + 4):
            p = k % 3
            x = g[f"b{p}_coords"].copy()
            for t, m in zip(g[f"b{p}_torsions"], g[f"b{p}_masks"]):
                x = tscode_amd.rotate_dihedral(x, t, float(rng.uniform(0.0, 360.0)), mask=m.astype(bool))
            drawn.append(x)
        bits = tscode_amd.bond_graph_batch(np.array(drawn), atomnos)
        poses += [x for x, b in zip(drawn, bits) if np.array_equal(b, want)]
    return np.array(poses[:count]), atomnos


def loop_search(x, ts):
    """Structure after structure, with what there was before the batched search."""
    import tscode_amd
    from tscode_amd.torsion_module import _trim_seed
    out = []
    for s in range(len(x)):
        tors, masks, folds = ts.sets[ts.set_of_structure[s]]
        groups = host_groups(x[s], tors)
        starts, output, call = x[s][None], [], 0
        for g, idx in enumerate(groups):
            new = tscode_amd.clustered_csearch_step(starts, tors[idx], masks[idx], n_folds=folds[idx])
            if g + 1 != len(groups) and len(new) > N_KEEP:
                new = tscode_amd.most_diverse_conformers(N_KEEP, new, tors, seed=_trim_seed(SEED, x[s], call))
                call += 1
            output.append(new)
            starts = new
        final, _ = tscode_amd.prune_conformers_tfd(np.concatenate(output), tors)
        if len(new) > N_OUT:
            final = tscode_amd.most_diverse_conformers(N_OUT, final, tors, seed=_trim_seed(SEED, x[s], call))
        out.append(final)
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clustered_csearch_profile.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="1,16,128")
    args = ap.parse_args()

    import tscode_amd
    from tscode_amd import build

    eng = tscode_amd.get_engine()
    rng = np.random.default_rng(SEED)
    rows = []
    for S in (int(v) for v in args.sizes.split(",")):
        x, atomnos = make_poses(S, rng)
        ts = tscode_amd.torsion_sets_batch(x, atomnos, None, False)
        batch, loop, stages = [], [], []
        for it in range(args.repeats + 1):
            tm, info = {}, {}
            eng.set_option("pass_timing", 1 if it == 0 else 0)       # the warm-up run times the kernels (and waits for each); the others do not
            t0 = time.perf_counter()
            got, _ = tscode_amd.clustered_csearch_batch(x, atomnos, n=N_KEEP, n_out=N_OUT, seed=SEED, info=info, timings=tm)
            t1 = time.perf_counter()
            want = loop_search(x, ts)
            t2 = time.perf_counter()
            if it == 0:
                kernel_ms = tm["groups_kernel_ms"]
                difference = float(np.abs(got - want).max()) if got.shape == want.shape else None
                if difference is None or difference > 1e-9:
                    print(f"WARNING: the batched search and the loop disagree at S = {S}: {got.shape} vs {want.shape}, {difference}", flush=True)
            else:
                batch.append(1e3 * (t1 - t0) - tm["setup_ms"]), loop.append(1e3 * (t2 - t1)), stages.append(tm)
        n_rounds = len(stages[0]["rotation_ms"])
        row = {"n_poses": S, "n_atoms": int(x.shape[1]), "n": N_KEEP, "n_out": N_OUT, "groups_of_pose_0": [len(g) for g in info["groups"][0]],
               "structures_built_per_round_pose_0": [r[0] for r in info["round_sizes"][0]], "structures_out": int(len(got)),
               "setup_ms": stats([t["setup_ms"] for t in stages]), "grouping_ms": stats([t["groups_ms"] for t in stages]),
               "grouping_kernel_ms": kernel_ms, "largest_difference_batched_vs_loop": difference,
               "rotation_ms_per_round": [stats([t["rotation_ms"][r] for t in stages]) for r in range(n_rounds)],
               "trim_ms_per_round": [stats([t["trim_ms"][r] for t in stages]) for r in range(n_rounds)],
               "final_prune_and_pick_ms": stats([t["final_ms"] for t in stages]),
               "batched_search_ms_without_setup": stats(batch), "per_structure_loop_ms_without_setup": stats(loop),
               "loop_over_batched": float(np.median(loop) / np.median(batch))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    import torch
    out = {"tool": "tools/clustered_csearch_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": build.csrc_digest(),
           "repeats": args.repeats, "seed": SEED, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
