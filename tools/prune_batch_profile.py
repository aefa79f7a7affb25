"""Many small ensembles pruned in one launch (tscode_amd.prune_conformers_rmsd_batch -> tsc_prune_rmsd_batch) beside a loop of
tscode_amd.prune_conformers_rmsd over the same ensembles (the single-ensemble path, unchanged by the batch kernel).

    python tools/prune_batch_profile.py [--out profiles/prune_batch_profile.json] [--repeats 3]

Workloads: 2 000 ensembles x 300 structures x 50 atoms (30 heavy) and 200 x 2 000 x 50, every ensemble a seeded
tscode_amd.synthetic.make_ensemble of two 25-atom fragments (the shape of BASELINE's C3), threshold 0.5, reference-exact mode.
Then one ensemble alone at N = 256 .. 8192 through both routes, the batch kernel forced by "prune_batch_max_n" = 8192: where the
one-workgroup kernel stops paying is where the option's default belongs.

Times are host wall time around the whole Python call, heavy-atom gather, uploads and the final synchronisation included (both calls
return host arrays, so both end in one).  Every shape is run once through both routes first (warm-up, and the masks are compared);
then the two routes alternate, --repeats times each; median, smallest and largest are recorded."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THR = 0.5
SEED = 2700


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def ensembles_of(count, n, seed):
    from tscode_amd.synthetic import make_ensemble
    made = [make_ensemble(n, (25, 25), seed + s) for s in range(count)]
    return [e.poses() for e in made], made[0].atomnos


def both_routes(structures, atomnos, repeats):
    """ms of (the batch call, the loop of single calls) on one list of ensembles, and what they kept (identical, or this raises)."""
    import tscode_amd

    def batch():
        t0 = time.perf_counter()
        out = tscode_amd.prune_conformers_rmsd_batch(structures, atomnos, THR)
        return (time.perf_counter() - t0) * 1e3, [m for _, m in out]

    def loop():
        t0 = time.perf_counter()
        out = [tscode_amd.prune_conformers_rmsd(s, atomnos, THR) for s in structures]
        return (time.perf_counter() - t0) * 1e3, [m for _, m in out]

    (_, mb), (_, ml) = batch(), loop()
    assert all(np.array_equal(a, b) for a, b in zip(mb, ml)), "the two routes disagree"
    tb, tl = [], []
    for _ in range(repeats):
        tb.append(batch()[0])
        tl.append(loop()[0])
    return stats(tb), stats(tl), int(sum(m.sum() for m in mb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_batch_profile.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shrink", type=int, default=1, help="divide the number of ensembles by this (trial runs of the tool itself)")
    args = ap.parse_args()

    import tscode_amd
    from tscode_amd import build

    eng = tscode_amd.get_engine()
    default_max_n = eng.prune_batch_max_n
    rows = []
    for count, n in ((2000, 300), (200, 2000)):
        count = max(1, count // args.shrink)
        structures, atomnos = ensembles_of(count, n, SEED)
        with eng.options(prune_batch_max_n=max(default_max_n, n)):      # (the kernel takes every ensemble of the workload)
            t_batch, t_loop, kept = both_routes(structures, atomnos, args.repeats)
        row = {"workload": f"{count}x{n}x50", "ensembles": count, "structures_per_ensemble": n, "atoms": 50, "heavy_atoms": int((atomnos != 1).sum()),
               "structures_kept": kept, "ms_batch_call": t_batch, "ms_loop_of_single_calls": t_loop, "loop_over_batch": t_loop["median"] / t_batch["median"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    single = []
    with eng.options(prune_batch_max_n=8192):
        for n in (256, 512, 1024, 2048, 4096, 8192):
            structures, atomnos = ensembles_of(1, n, SEED + 5000)
            t_batch, t_loop, kept = both_routes(structures, atomnos, args.repeats)
            row = {"structures": n, "structures_kept": kept, "ms_batch_kernel_one_workgroup": t_batch, "ms_single_call": t_loop,
                   "single_over_batch": t_loop["median"] / t_batch["median"]}
            single.append(row)
            print(json.dumps(row), flush=True)
    import torch
    out = {"tool": "tools/prune_batch_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(), "repeats": args.repeats, "threshold": THR, "mode": 0, "prune_batch_max_n_default": default_max_n,
           "batches": rows, "one_ensemble": single}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
