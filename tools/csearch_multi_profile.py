"""The csearch candidates of many starts: one multi launch (tsc_csearch_rotate_multi_dev) beside a loop of the single-start entry
point per start (tsc_csearch_rotate_dev, unchanged by the multi kernel), and the host drivers built on them.

    python tools/csearch_multi_profile.py [--out profiles/csearch_multi_profile.json] [--repeats 5]

Workloads: (i) clustered_csearch's starting-point loop (tscode/torsion_module.py:736-780), 100 starts x 243 angle sets x 5
torsions at 50 and 200 atoms, one torsion set; (ii) csearch_augmentation (tscode/embedder.py:1907-1939), 1000 starts of 100
atoms, each with its own 6 torsions and its own shuffled table of 729 rows, n_out = 100.  Per workload: HIP-event time on
resident buffers of the loop and of the one launch (for (ii): the first round, 256 rows of every start), and host wall time,
copies included, of a loop of csearch_candidates against csearch_candidates_multi.  Medians of --repeats after one warm-up run,
with the smallest and largest value.  The molecules are self-avoiding walks of 1.5 A steps (tscode_amd.synthetic), threshold 1.4."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESH = 1.4


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def torsion_set(rng, n, n_tors):
    centres = rng.choice(np.arange(1, n - 3), size=n_tors, replace=False)
    torsions = np.array([(c - 1, c, c + 1, c + 2) for c in centres], dtype=np.int32)
    masks = np.zeros((n_tors, n), dtype=np.uint8)
    for t, c in enumerate(centres):
        masks[t, c + 1:min(n, c + 1 + n // 3)] = 1
    return torsions, masks


def workload(rng, n, n_starts, n_tors, own_sets):
    from tscode_amd.synthetic import make_fragment, quat_to_mat
    from tscode_amd.utils import cartesian_product
    base = make_fragment(rng, n, min_dist=1.45)        # nothing closer than the threshold in the start: rotations can pass
    starts = np.array([base @ quat_to_mat(rng.normal(size=4)).T + rng.normal(size=3) for _ in range(n_starts)])
    table = cartesian_product(*[(0, 120, 240)] * n_tors).astype(np.int32)
    sets = []
    for _ in range(n_starts if own_sets else 1):
        tab = table.copy()
        if own_sets:
            rng.shuffle(tab)
        sets.append(torsion_set(rng, n, n_tors) + (tab,))
    return starts, sets


def device_times(eng, starts, sets, rows_per_start, repeats):
    """HIP-event ms of (a loop of tsc_csearch_rotate_dev per start, one tsc_csearch_rotate_multi_dev) over the first rows_per_start
    rows of every start's table, everything resident."""
    from tscode_amd.torsion_module import _pack_sets
    p = _pack_sets(starts, sets, None)
    rows = np.minimum(rows_per_start, p.table_len[p.start_set])
    cand_start = np.repeat(np.arange(p.S, dtype=np.int32), rows)
    seg = np.concatenate([[0], np.cumsum(rows)])
    cand_row = (np.arange(seg[-1]) - np.repeat(seg[:-1], rows) + np.repeat(p.row_base[p.start_set], rows)).astype(np.int32)
    items = eng.csearch_multi_plan(cand_start, p.start_set, p.set_off, p.n)
    n_cand = int(seg[-1])
    bufs = {k: eng.dev_upload(v) for k, v in dict(starts=p.starts, tors=p.torsions, masks=p.masks, angles=p.angles, cs=cand_start, cr=cand_row,
                                                  items=items).items()}
    # the single-start entry point wants a table as wide as the set: every set of a workload has the widest width here
    assert all(len(s[0]) == p.t_max for s in sets)
    bufs["out"], bufs["rb"] = eng.dev_alloc(n_cand * p.n * 24), eng.dev_alloc(n_cand * 4)
    loop, multi = [], []
    try:
        for it in range(repeats + 1):
            eng.timer_begin()
            for s in range(p.S):
                k = p.start_set[s]
                eng.csearch_rotate_dev(bufs["starts"] + s * p.n * 24, p.n, bufs["tors"] + int(p.set_off[k]) * 16, bufs["masks"] + int(p.set_off[k]) * p.n,
                                       p.t_max, bufs["angles"] + int(p.row_base[k]) * p.t_max * 4, int(rows[s]), THRESH, 0,
                                       bufs["out"] + int(seg[s]) * p.n * 24, bufs["rb"] + int(seg[s]) * 4)
            t_loop = eng.timer_end()
            eng.timer_begin()
            eng.csearch_rotate_multi_dev(bufs["starts"], p.n, bufs["tors"], bufs["masks"], p.set_off, bufs["angles"], p.t_max, bufs["cs"], bufs["cr"],
                                         n_cand, bufs["items"], len(items), THRESH, 0, bufs["out"], bufs["rb"])
            t_multi = eng.timer_end()
            if it:
                loop.append(t_loop), multi.append(t_multi)
    finally:
        for b in bufs.values():
            eng.dev_free(b)
    return n_cand, len(items), stats(loop), stats(multi)


def host_times(starts, sets, n_out, repeats):
    import tscode_amd
    loop, multi, kept = [], [], 0
    single = dict(n_out=10**9, max_tries=-1) if n_out is None else dict(n_out=n_out)
    for it in range(repeats + 1):
        t0 = time.perf_counter()
        ref = [tscode_amd.csearch_candidates(starts[s], *sets[s if len(sets) > 1 else 0], thresh=THRESH, **single) for s in range(len(starts))]
        t1 = time.perf_counter()
        got, _ = tscode_amd.csearch_candidates_multi(starts, sets, n_out=n_out, thresh=THRESH)
        t2 = time.perf_counter()
        if it == 0:
            want = np.concatenate(ref)
            assert len(got) and got.shape == want.shape and np.abs(got - want).max() < 1e-9, "the two drivers disagree"
            kept = len(got)
        else:
            loop.append((t1 - t0) * 1e3), multi.append((t2 - t1) * 1e3)
    return kept, stats(loop), stats(multi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csearch_multi_profile.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shrink", type=int, default=1, help="divide the number of starts by this (trial runs of the tool itself)")
    args = ap.parse_args()

    import tscode_amd
    from tscode_amd import build

    eng = tscode_amd.get_engine()
    rng = np.random.default_rng(2424)
    rows = []
    for name, n, n_starts, n_tors, own, n_out, first_round in (("clustered_50", 50, 100, 5, False, None, 243), ("clustered_200", 200, 100, 5, False, None, 243),
                                                               ("augmentation_100", 100, 1000, 6, True, 100, 256)):
        n_starts = max(1, n_starts // args.shrink)
        starts, sets = workload(rng, n, n_starts, n_tors, own)
        n_cand, n_items, dev_loop, dev_multi = device_times(eng, starts, sets, first_round, args.repeats)
        kept, host_loop, host_multi = host_times(starts, sets, n_out, args.repeats)
        table_rows = len(sets[0][2])
        row = {"workload": name, "n_atoms": n, "n_starts": n_starts, "n_torsions": n_tors, "table_rows_per_start": table_rows, "n_out": n_out,
               "device_candidates": n_cand, "device_work_items": n_items, "device_ms_loop_of_rotate_dev": dev_loop, "device_ms_one_multi_launch": dev_multi,
               "device_speedup": dev_loop["median"] / dev_multi["median"], "structures_kept": kept,
               "host_ms_loop_of_csearch_candidates": host_loop, "host_ms_csearch_candidates_multi": host_multi,
               "host_speedup": host_loop["median"] / host_multi["median"],
               # from the shapes: the loop downloads every candidate of every block it rotates (the whole table: block 8192 > table) and its
               # rotated_bonds; the multi driver the kept rows and 3 int32 counters per start and round
               "bytes_to_host_loop": n_starts * table_rows * (n * 24 + 4),
               "bytes_to_host_multi_kept_rows": kept * n * 24, "bytes_to_host_multi_counters_per_round": 12 * n_starts}
        rows.append(row)
        print(json.dumps(row), flush=True)
    import torch
    out = {"tool": "tools/csearch_multi_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": build.csrc_digest(),
           "repeats": args.repeats, "threshold": THRESH, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
