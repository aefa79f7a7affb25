"""Many small ensembles pruned by TFD and trimmed to their most diverse conformers in one call each (tscode_amd.prune_conformers_tfd_batch,
diverse_select_batch, most_diverse_conformers_batch) beside loops of the existing single calls over the same ensembles (unchanged by
the batch kernels).

    python tools/diverse_batch_profile.py [--out profiles/diverse_batch_profile.json] [--repeats 3] [--counts 16,128] [--sizes 243,1649]

Ensembles: the 40-atom diene of fixture G26 with its 9 torsions; every structure is pose 0 with each torsion turned by a multiple of its
n-fold step plus a few degrees of noise (rotate_dihedral_batch), a seed per ensemble.  243 structures is what one round of the clustered
search hands to its trim, 1649 what its final prune and pick see (MEASURED.md section 19).  k = 20, every k-means seeded.

Per shape three pairs: the TFD prune, the selection (alignment, seeding, k-means, pick) on the pruned ensembles, and
most_diverse_conformers, which is the two in a row as the search calls them.  Times are host wall time around the whole Python call,
uploads and the final synchronisation included (every call returns host arrays, so every call ends in one); no kernel events are taken.
Every pair is run once first (warm-up) and its results are compared -- masks equal, aligned coordinates bit for bit, labels, picks,
rows and iteration counts equal -- before any time is taken; then the batch call and the loop alternate, --repeats times each; median,
smallest and largest are recorded."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 20
SEED = 2020


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def ensembles_of(count, n, seed):
    import tscode_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "G26_clustered_csearch.npz"))
    torsions, masks, folds = g["b0_torsions"], g["b0_masks"].astype(bool), g["b0_n_folds"]
    out = []
    for e in range(count):
        rng = np.random.default_rng([seed, n, e])
        x = np.repeat(g["b0_coords"][None], n, axis=0)
        for t, m, f in zip(torsions, masks, folds):
            x = tscode_amd.rotate_dihedral_batch(x, t, rng.integers(0, int(f), size=n) * (360.0 / int(f)) + rng.normal(0.0, 4.0, size=n), m)
        out.append(np.ascontiguousarray(x))
    return out, torsions.astype(np.int32)


def alternate(batch, loop, same, repeats):
    """ms of (the batch call, the loop of single calls); ``same(a, b)`` raises unless their results agree."""
    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r
    (_, rb), (_, rl) = timed(batch), timed(loop)
    same(rb, rl)
    tb, tl = [], []
    for _ in range(repeats):
        tb.append(timed(batch)[0])
        tl.append(timed(loop)[0])
    return stats(tb), stats(tl), rb


def same_masks(a, b):
    assert all(np.array_equal(p[1], q[1]) for p, q in zip(a, b)), "the TFD prunes disagree"


def same_selection(a, b):
    for p, q in zip(a, b):
        assert np.array_equal(p[0].view(np.uint64), q[0].view(np.uint64)), "aligned coordinates differ in their bits"
        assert all(np.array_equal(p[j], q[j]) for j in (1, 2, 3)) and p[4] == q[4], "labels, picks, rows or iteration counts differ"


def same_arrays(a, b):
    assert all(np.array_equal(p, q) for p, q in zip(a, b)), "most_diverse_conformers disagrees"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_batch_profile.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--counts", default="16,128")
    ap.add_argument("--sizes", default="243,1649")
    args = ap.parse_args()

    import tscode_amd
    from tscode_amd import build

    eng = tscode_amd.get_engine()
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        for count in (int(v) for v in args.counts.split(",")):
            ens, quads = ensembles_of(count, n, SEED)
            seeds = list(range(count))
            t_pb, t_pl, pruned = alternate(lambda: tscode_amd.prune_conformers_tfd_batch(ens, quads),
                                           lambda: [tscode_amd.prune_conformers_tfd(e, quads) for e in ens], same_masks, args.repeats)
            kept = [p for p, _ in pruned]
            t_sb, t_sl, sel = alternate(lambda: tscode_amd.diverse_select_batch(kept, K, seeds=seeds),
                                        lambda: [tscode_amd.diverse_select(e, K, seed=s) for e, s in zip(kept, seeds)], same_selection, args.repeats)
            t_mb, t_ml, _ = alternate(lambda: tscode_amd.most_diverse_conformers_batch(K, ens, quads, seeds=seeds),
                                      lambda: [tscode_amd.most_diverse_conformers(K, e, quads, seed=s) for e, s in zip(ens, seeds)], same_arrays,
                                      args.repeats)
            iters = [s[4] for s in sel]
            row = {"ensembles": count, "structures_per_ensemble": n, "atoms": int(ens[0].shape[1]), "torsions": int(len(quads)), "k": K,
                   "structures_after_tfd_prune": stats([len(e) for e in kept]), "lloyd_iterations": stats(iters),
                   "tfd_prune_ms": {"batch_call": t_pb, "loop_of_single_calls": t_pl, "loop_over_batch": t_pl["median"] / t_pb["median"]},
                   "diverse_select_ms": {"batch_call": t_sb, "loop_of_single_calls": t_sl, "loop_over_batch": t_sl["median"] / t_sb["median"]},
                   "most_diverse_conformers_ms": {"batch_call": t_mb, "loop_of_single_calls": t_ml, "loop_over_batch": t_ml["median"] / t_mb["median"]}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    import torch
    out = {"tool": "tools/diverse_batch_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(), "repeats": args.repeats, "seed": SEED, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
