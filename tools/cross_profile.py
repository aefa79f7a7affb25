"""Cross-set RMSD (tscode_amd/rmsd_cross.py, csrc/cross.hpp) timed beside what the library offered for the same work before it.

    python tools/cross_profile.py [--out profiles/rmsd_cross_profile.json] [--repeats 5] [--step-limit 240]

Structures: fixed-seed tscode_amd.synthetic.make_config("C2") poses, 30 atoms, all of them compared (atomnos=None), threshold 0.5.

    values    4096 x 4096        rmsd_matrix                 beside  Engine.rmsd_pairs over the explicit list of the same 16.8 M pairs
    first     64 x 100 000       rmsd_similarity_mask        beside  the loop of _rmsd_similarity over the queries
    first     100 000 x 1 000    rmsd_similarity_mask        (alone: the loop would take minutes)
    nearest   1 x 1 000 000      nearest_structures          (alone)

One process.  Every step is warmed up once (results compared where there is a yardstick), then timed --repeats times: host wall time around
the whole Python call, argument checks, uploads and the final synchronisation included ("ms_host").  Every new call is timed once more with
its arrays resident on the device -- the _dev form and a synchronise, as many calls per window as make it a quarter of a second
("ms_resident", per call) -- and the pair evaluations per second are those of that figure.  A step that passes --step-limit seconds ends the
run there: nothing more is started on the device."""

import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THR = 0.5
STEPS = (("values", 4096, 4096), ("first", 64, 100_000), ("first", 100_000, 1_000), ("nearest", 1, 1_000_000))


class StepTimeout(Exception):
    pass


def _alarm(_sig, _frame):
    raise StepTimeout()


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def resident(eng, kind, queries, library, repeats):
    """ms per call of the _dev form on device-resident arrays (a window of `inner` calls and one synchronise)"""
    import torch
    dev = torch.device("cuda", eng.device)
    nq, nl, n = len(queries), len(library), queries.shape[1]
    d_q, d_l = torch.from_numpy(queries).to(dev), torch.from_numpy(library).to(dev)
    if kind == "values":
        d_r, d_m = (torch.empty((nq, nl), dtype=torch.float64, device=dev) for _ in range(2))
        call = lambda: eng.rmsd_cross_dev(d_q, nq, d_l, nl, n, None, 0, False, d_r, d_m, nq * nl)                # noqa: E731
    elif kind == "first":
        d_f = torch.empty(nq, dtype=torch.int32, device=dev)
        call = lambda: eng.rmsd_cross_first_dev(d_q, nq, d_l, nl, n, None, 0, False, THR, d_f)                  # noqa: E731
    else:
        d_i, d_r, d_m = torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.float64, device=dev), torch.empty(nq, dtype=torch.float64, device=dev)
        call = lambda: eng.rmsd_cross_nearest_dev(d_q, nq, d_l, nl, n, None, 0, False, d_i, d_r, d_m)           # noqa: E731
    torch.cuda.synchronize(dev)

    def window(inner):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner

    window(1)
    inner = int(min(50, max(1, np.ceil(250.0 / max(window(1), 1e-3)))))
    return stats([window(inner) for _ in range(repeats)]), inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmsd_cross_profile.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240, help="seconds a step may take before the run ends")
    ap.add_argument("--shrink", type=int, default=1, help="divide both sides of every shape by this (trial runs of the tool itself)")
    args = ap.parse_args()

    import torch
    import tscode_amd
    from tscode_amd import build
    from tscode_amd.synthetic import make_config

    eng = tscode_amd.get_engine()
    signal.signal(signal.SIGALRM, _alarm)
    rows, ended = [], None
    for kind, nq, nl in STEPS:
        nq, nl = max(1, nq // args.shrink), max(1, nl // args.shrink)
        poses = np.ascontiguousarray(make_config("C2", nq + nl).poses())
        queries, library = poses[:nq], poses[nq:]
        row = {"step": kind, "queries": nq, "library": nl, "atoms": int(poses.shape[1]), "pairs": nq * nl}
        signal.alarm(args.step_limit)
        try:
            if kind == "values":
                r, m = tscode_amd.rmsd_matrix(queries, library)
                pairs = np.stack([np.repeat(np.arange(nq, dtype=np.int32), nl), nq + np.tile(np.arange(nl, dtype=np.int32), nq)], axis=1)
                rp, mp = eng.rmsd_pairs(poses, pairs)
                row["max_abs_difference_from_rmsd_pairs"] = [float(np.abs(r.ravel() - rp).max()), float(np.abs(m.ravel() - mp).max())]
                t_new, t_old = [], []
                for _ in range(args.repeats):                   # (the two alternate: the host's memory and its other tenants move both alike)
                    t_new.append(timed(lambda: tscode_amd.rmsd_matrix(queries, library), 1)["median"])
                    t_old.append(timed(lambda: eng.rmsd_pairs(poses, pairs), 1)["median"])
                row["ms_host"], row["ms_host_rmsd_pairs"] = stats(t_new), stats(t_old)
                row["ms_host_building_the_pair_list"] = timed(lambda: np.stack([np.repeat(np.arange(nq, dtype=np.int32), nl), nq + np.tile(np.arange(nl, dtype=np.int32), nq)], axis=1), 3)
                dev = torch.device("cuda", eng.device)
                d_p, d_pairs = torch.from_numpy(poses).to(dev), torch.from_numpy(pairs).to(dev)
                d_r, d_m = (torch.empty(len(pairs), dtype=torch.float64, device=dev) for _ in range(2))
                torch.cuda.synchronize(dev)

                def pairs_dev():
                    tscode_amd._lib.check(eng.lib.tsc_rmsd_pairs_dev(eng._h, tscode_amd._lib.ptr(d_p), len(poses), poses.shape[1], tscode_amd._lib.ptr(d_pairs), len(pairs),
                                                                    tscode_amd._lib.ptr(d_r), tscode_amd._lib.ptr(d_m)))
                    eng.synchronize()
                pairs_dev()
                row["ms_resident_rmsd_pairs"] = timed(pairs_dev, args.repeats)
                del d_p, d_pairs, d_r, d_m, pairs, rp, mp, r, m
            elif kind == "first":
                similar, first = tscode_amd.rmsd_similarity_mask(queries, library, None, THR)
                row["similar_queries"] = int(similar.sum())
                if nq <= 64:
                    loop = lambda: np.array([tscode_amd._rmsd_similarity(q, library, THR) for q in queries])     # noqa: E731
                    assert np.array_equal(loop(), similar), "rmsd_similarity_mask and the loop of _rmsd_similarity disagree"
                    row["ms_host_loop_of_rmsd_similarity"] = timed(loop, args.repeats)
                row["ms_host"] = timed(lambda: tscode_amd.rmsd_similarity_mask(queries, library, None, THR), args.repeats)
            else:
                index, r, _m = tscode_amd.nearest_structures(queries, library)
                row["nearest_index"], row["nearest_rmsd"] = int(index[0]), float(r[0])
                row["ms_host"] = timed(lambda: tscode_amd.nearest_structures(queries, library), args.repeats)
            row["ms_resident"], row["resident_calls_per_window"] = resident(eng, kind, queries, library, args.repeats)
            row["pairs_per_second_resident"] = row["pairs"] / (row["ms_resident"]["median"] * 1e-3)
        except StepTimeout:
            ended = f"step {kind} {nq} x {nl} passed {args.step_limit} s: the run ends here"
            row["timed_out"] = True
        finally:
            signal.alarm(0)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if ended:
            break
        del poses, queries, library
    out = {"tool": "tools/cross_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(), "repeats": args.repeats, "threshold": THR, "structures": "make_config('C2', Nq + Nl).poses(), queries first",
           "shrink": args.shrink, "ended_early": ended, "steps": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    return 1 if ended else 0


if __name__ == "__main__":
    sys.exit(main())
