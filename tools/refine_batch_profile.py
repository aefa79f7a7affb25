"""Many ensembles pruned by symmetry-corrected RMSD and by moments of inertia in one call each (tscode_amd.prune_rmsd_rot_corr_arrays_batch,
prune_by_moment_of_inertia_batch) beside loops of the existing single calls over the same ensembles (unchanged by the batch kernels).

    python tools/refine_batch_profile.py [--out profiles/refine_batch_profile.json] [--repeats 3] [--counts 1,16,128] [--size 200]

Ensembles: molecule B of fixture G19 (40 atoms) with its six torsions, 200 structures each from make_rot_corr_ensemble (20 clusters of
10: symmetry turns of every rotor plus noise, shuffled), a seed per ensemble; max_rmsd 0.25, max_deviation 1e-2.

Times are host wall time around the whole Python call, uploads, the host's graph steps and every synchronisation included (every
schedule slot returns host arrays, so every slot ends in one); no kernel events are taken.  Every pair is run once first (warm-up) and
its results are compared -- masks equal, kept structures bit for bit, the slots' pair counts equal -- before any time is taken; then
the batch call and the loop alternate, --repeats times each; median, smallest and largest are recorded.  The tool ends with status 1 if,
at the largest count, the rot-corr batch's median does not lie below the loop's smallest time."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 1900
MAX_RMSD, MAX_DEVIATION = 0.25, 1e-2


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def molecule_b():
    """(coords, atomnos, set-up dict) of G19's molecule B, as tests/test_rot_corr.py::case("n150") reads them."""
    a = np.load(os.path.join(ROOT, "tests", "golden", "G19a_rot_corr.npz"), allow_pickle=False)
    b = np.load(os.path.join(ROOT, "tests", "golden", "G19b_rot_corr.npz"), allow_pickle=False)
    d = {**{k: a[k] for k in a.files}, **{k: b[k] for k in b.files}}
    ptr = d["n150_sub_ptr"]
    T = len(d["n150_torsions"])
    setup = dict(torsions=d["n150_torsions"], angles=[d["n150_angles"][t, :d["n150_n_angles"][t]] for t in range(T)],
                 move_masks=d["n150_move_masks"], sub_nodes=[d["n150_sub_idx"][ptr[t]:ptr[t + 1]] for t in range(T)])
    return d["molB_coords"], d["molB_atomnos"], setup


def ensembles_of(count, size, coords, setup):
    from tscode_amd.synthetic import make_rot_corr_ensemble
    per = 10
    return [make_rot_corr_ensemble(coords, setup["torsions"], setup["angles"], setup["move_masks"], size // per, per, seed=SEED + e)[0]
            for e in range(count)]


def alternate(name, batch, loop, same, repeats):
    """ms of (the batch call, the loop of single calls); ``same(a, b)`` raises unless their results agree."""
    def timed(what, f):
        t0 = time.perf_counter()
        r = f()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"  {name} {what}: {ms:.1f} ms", flush=True)
        return ms, r
    (_, rb), (_, rl) = timed("batch (warm-up)", batch), timed("loop (warm-up)", loop)
    same(rb, rl)
    tb, tl = [], []
    for _ in range(repeats):
        tb.append(timed("batch", batch)[0])
        tl.append(timed("loop", loop)[0])
    return stats(tb), stats(tl), rb


def same_prunes(a, b):
    for p, q in zip(a, b):
        assert np.array_equal(p[1], q[1]), "the masks disagree"
        assert np.array_equal(np.ascontiguousarray(p[0]).view(np.uint64), np.ascontiguousarray(q[0]).view(np.uint64)), "kept structures differ in their bits"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_batch_profile.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--counts", default="1,16,128")
    ap.add_argument("--size", type=int, default=200)
    args = ap.parse_args()

    import tscode_amd
    from tscode_amd import build
    from tscode_amd.optimization_methods import _MASS

    eng = tscode_amd.get_engine()
    coords, atomnos, setup = molecule_b()
    masses = np.array([_MASS[int(z)] for z in atomnos])
    rows = []
    for count in (int(v) for v in args.counts.split(",")):
        ens = ensembles_of(count, args.size, coords, setup)
        print(f"{count} ensembles of {args.size}", flush=True)
        loop_stats = []

        def rot_corr_loop():
            out = []
            loop_stats.clear()
            for e in ens:
                out.append(tscode_amd.prune_rmsd_rot_corr_arrays(e, atomnos, **setup, max_rmsd=MAX_RMSD))
                loop_stats.append(tscode_amd.last_rot_corr_stats())
            return out

        t_rb, t_rl, pruned = alternate("rot-corr", lambda: tscode_amd.prune_rmsd_rot_corr_arrays_batch(ens, atomnos, setup, max_rmsd=MAX_RMSD),
                                       rot_corr_loop, same_prunes, args.repeats)
        batch_stats = tscode_amd.last_rot_corr_batch_stats() if count > 1 else loop_stats
        assert batch_stats == loop_stats, "the slots' active counts or pair counts disagree"
        t_mb, t_ml, moi = alternate("moi", lambda: tscode_amd.prune_by_moment_of_inertia_batch(ens, atomnos, MAX_DEVIATION, masses=masses),
                                    lambda: [tscode_amd.prune_by_moment_of_inertia(e, atomnos, MAX_DEVIATION, masses=masses) for e in ens],
                                    same_prunes, args.repeats)
        slots = sorted({int(x["k"]) for st in batch_stats for x in st if x["ran"]}, reverse=True)
        row = {"ensembles": count, "structures_per_ensemble": args.size, "atoms": int(coords.shape[0]), "torsions": int(len(setup["torsions"])),
               "slots_run": slots, "pairs_evaluated": int(sum(x["pairs_evaluated"] for st in batch_stats for x in st)),
               "structures_after_rot_corr": stats([int(m.sum()) for _, m in pruned]),
               "structures_after_moi": stats([int(m.sum()) for _, m in moi]),
               "rot_corr_ms": {"batch_call": t_rb, "loop_of_single_calls": t_rl, "batch_median_below_loop_min": t_rb["median"] < t_rl["min"]},
               "moi_ms": {"batch_call": t_mb, "loop_of_single_calls": t_ml, "batch_median_below_loop_min": t_mb["median"] < t_ml["min"]}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    import torch
    out = {"tool": "tools/refine_batch_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(), "repeats": args.repeats, "seed": SEED, "max_rmsd": MAX_RMSD, "max_deviation": MAX_DEVIATION,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    last = rows[-1]
    if last["ensembles"] > 1 and not last["rot_corr_ms"]["batch_median_below_loop_min"]:
        print("the rot-corr batch's median does not lie below the loop's smallest time")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
