"""Many mid-size ensembles pruned per call: tscode_amd.prune_conformers_rmsd_batch with the team route open to its cap
(team_max_n = TSC_PRUNE_TEAM_MAX_N -> tsc_prune_rmsd_team, a team of workgroups per ensemble) beside the same call with team_max_n = 0,
the routing before the team route existed: k_prune_batch up to "prune_batch_max_n" structures, a single-ensemble call for every longer one.

    python tools/prune_team_profile.py [--out profiles/prune_team_profile.json] [--repeats 3]

Workloads: ensembles x structures of 50 atoms (30 heavy), every ensemble a seeded tscode_amd.synthetic.make_ensemble of two 25-atom
fragments (as tools/prune_batch_profile.py), threshold 0.5, reference-exact mode: 200 x 2000, 16 x 2000, 16 x 4096, 64 x 4096, 16 x 8192,
4 x 16384, 1 x 4096 under the default "prune_batch_max_n" (2048: the 2000-structure rows take k_prune_batch on both sides and are the
control), then 200 x 2000 and 16 x 2000 with the option lowered to 256, so that the team route takes them instead of k_prune_batch.

Times are host wall time around the whole Python call, heavy-atom gather, uploads and the final synchronisation included.  Every shape is
run once through both routings first (warm-up, and the masks and per-pass statistics are compared); then the two alternate, --repeats
times each; median, smallest and largest are recorded.  The shapes under the default option are then timed once more with the heavy atoms
resident on the device -- tsc_prune_rmsd_team_dev on all ensembles beside a loop of tsc_prune_rmsd_dev, no gather, no packing, no upload --,
which is what the two routes cost without the host's share."""

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
SHAPES = ((200, 2000, None), (16, 2000, None), (16, 4096, None), (64, 4096, None), (16, 8192, None), (4, 16384, None), (1, 4096, None),
          (200, 2000, 256), (16, 2000, 256))           # (ensembles, structures, "prune_batch_max_n" or None for the default)


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def ensembles_of(count, n, seed):
    from tscode_amd.synthetic import make_ensemble
    made = [make_ensemble(n, (25, 25), seed + s) for s in range(count)]
    return [e.poses() for e in made], made[0].atomnos


def both_routings(structures, atomnos, cap, repeats):
    """ms of the batch call under (team_max_n = cap, team_max_n = 0) on one list of ensembles, and what they kept (identical masks and
    statistics, or this raises)."""
    import tscode_amd

    def call(team_max_n):
        t0 = time.perf_counter()
        out = tscode_amd.prune_conformers_rmsd_batch(structures, atomnos, THR, team_max_n=team_max_n)
        return (time.perf_counter() - t0) * 1e3, [m for _, m in out], tscode_amd.last_prune_batch_stats()

    (_, mt, st), (_, mb, sb) = call(cap), call(0)
    assert all(np.array_equal(a, b) for a, b in zip(mt, mb)), "the two routings disagree on a mask"
    assert st == sb, "the two routings disagree on the per-pass statistics"
    tt, tb = [], []
    for _ in range(repeats):
        tt.append(call(cap)[0])
        tb.append(call(0)[0])
    return stats(tt), stats(tb), int(sum(m.sum() for m in mt)), [p["k"] for p in st[0]]


def resident(eng, structures, atomnos, repeats):
    """The same comparison without the host's share: the heavy atoms already on the device, tsc_prune_rmsd_team_dev on all ensembles
    beside a loop of tsc_prune_rmsd_dev over them (both synchronise; host wall time around the calls), masks compared first."""
    import torch
    from tscode_amd import pack_heavy_batch
    flat, offsets, n, h = pack_heavy_batch([np.ascontiguousarray(s[:, atomnos != 1]) for s in structures])
    dev = torch.device("cuda", eng.device)
    d_heavy = torch.from_numpy(flat).to(dev)
    d_team, d_loop = (torch.zeros(int(n.sum()), dtype=torch.uint8, device=dev) for _ in range(2))
    row_off = np.concatenate([[0], np.cumsum(n)]).tolist()
    torch.cuda.synchronize(dev)

    def team():
        t0 = time.perf_counter()
        eng.prune_heavy_team_dev(d_heavy, offsets, n, h, THR, 0, d_team)
        return (time.perf_counter() - t0) * 1e3

    def loop():
        t0 = time.perf_counter()
        for s in range(len(n)):
            eng.prune_heavy_dev(d_heavy[offsets[s]:offsets[s + 1]], int(n[s]), int(h[s]), THR, 0, d_loop[row_off[s]:row_off[s + 1]])
        return (time.perf_counter() - t0) * 1e3

    team(), loop()
    assert torch.equal(d_team, d_loop), "the two routes disagree on a mask"
    tt, tl = [], []
    for _ in range(repeats):
        tt.append(team())
        tl.append(loop())
    return stats(tt), stats(tl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_team_profile.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shrink", type=int, default=1, help="divide the structures per ensemble by this (trial runs of the tool itself)")
    args = ap.parse_args()

    import tscode_amd
    from tscode_amd import build
    from tscode_amd._lib import TSC_PRUNE_TEAM_MAX_N

    eng = tscode_amd.get_engine()
    default_max_n = eng.prune_batch_max_n
    rows = []
    for count, n, max_n in SHAPES:
        n = max(2, n // args.shrink)
        structures, atomnos = ensembles_of(count, n, SEED)
        with eng.options(prune_batch_max_n=default_max_n if max_n is None else max(1, max_n // args.shrink)):
            routed_to_team = n > eng.prune_batch_max_n
            t_team, t_base, kept, ks = both_routings(structures, atomnos, TSC_PRUNE_TEAM_MAX_N, args.repeats)
        r_team, r_loop = resident(eng, structures, atomnos, args.repeats) if max_n is None else (None, None)
        row = {"workload": f"{count}x{n}x50", "ensembles": count, "structures_per_ensemble": n, "atoms": 50, "heavy_atoms": int((atomnos != 1).sum()),
               "prune_batch_max_n": default_max_n if max_n is None else max_n, "team_route_taken": routed_to_team,
               "baseline_route": "single-ensemble calls" if routed_to_team else "k_prune_batch", "passes_of_first_ensemble": ks,
               "structures_kept": kept, "ms_team_max_n_cap": t_team, "ms_team_max_n_0": t_base, "baseline_over_team": t_base["median"] / t_team["median"]}
        if r_team is not None:
            row.update(ms_resident_team_dev=r_team, ms_resident_loop_of_single_dev=r_loop, resident_loop_over_team=r_loop["median"] / r_team["median"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del structures
    import torch
    out = {"tool": "tools/prune_team_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(), "repeats": args.repeats, "threshold": THR, "mode": 0, "prune_batch_max_n_default": default_max_n,
           "team_max_n_cap": TSC_PRUNE_TEAM_MAX_N, "shrink": args.shrink, "batches": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
