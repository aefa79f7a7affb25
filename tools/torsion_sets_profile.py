"""From coordinates to torsion sets: what the set-up in front of csearch_candidates_multi costs (tscode_amd.torsion_sets_batch,
csrc/torsions.hpp), beside the candidate generation it feeds.

    python tools/torsion_sets_profile.py [--out profiles/torsion_sets_profile.json] [--repeats 5]

Workloads: the augmentation_100 shape of tools/csearch_multi_profile.py -- 1000 structures x 100 atoms -- and 400 x 200 atoms.
The molecule is a hydroxy ketone with an alkyl tail (HO-(CH2)3-CO-(CH2)28-CHO: 100 atoms; HO-(CH2)3-CO-(CH2)61-CH3: 200 atoms),
every structure its own draw of torsions: in about a third the hydroxyl is folded onto the ketone oxygen (O-H...O closes a ring),
so the ensemble falls into several topology classes.
Per shape: HIP-event time of each kernel on resident buffers (context option "pass_timing"), the number of classes, host
milliseconds split into grouping, quadruplets, chemistry (cold: the class cache emptied before every run; warm: kept) and the
angle tables (at the 6 three-fold torsions per structure of the committed workload); bytes moved.  Medians of --repeats after
one warm-up run.  The committed device_ms_one_multi_launch of augmentation_100 (profiles/csearch_multi_profile.json) is printed
beside them."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def _unit(v):
    return v / np.linalg.norm(v)


def place(pa, pb, pc, r, theta, phi):
    """A point at distance r from pa, angle theta (deg) to pb, dihedral phi (deg) about pa-pb with respect to pc."""
    th, ph = np.radians(theta), np.radians(phi)
    bc = _unit(pa - pb)
    nv = _unit(np.cross(pb - pc, bc))
    m = np.array([bc, np.cross(nv, bc), nv])
    return pa + np.array([-r * np.cos(th), r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph)]) @ m


def hydroxy_ketone(m, end, torsions):
    """HO-(CH2)3-CO-(CH2)m-CHO (end "CHO") or ...-CH3 (end "CH3") from its m + 5 backbone torsions (deg); heavy atoms and the
    hydroxyl hydrogen first, then the hydrogens on carbon.  The first four torsions decide whether O-H...O=C closes a ring."""
    z, x = [8, 1], [np.zeros(3), np.array([0.96, 0.0, 0.0])]
    x.append(place(x[0], x[1], np.array([0.0, 1.0, 0.0]), 1.43, 108.0, 0.0))
    z.append(6)
    back = [2, 0, 1]
    backbone = [0, 2]
    for k in range(m + 3 + (1 if end == "CH3" else 0)):
        sp2 = k == 2                                                   # the carbonyl carbon
        x.append(place(x[back[0]], x[back[1]], x[back[2]], 1.52, 117.0 if back[0] == 5 else 111.0, torsions[k]))
        z.append(6)
        back = [len(z) - 1, back[0], back[1]]
        backbone.append(back[0])
        if sp2:
            ketone = back[:]
    if end == "CHO":
        x.append(place(x[back[0]], x[back[1]], x[back[2]], 1.51, 111.0, torsions[m + 3]))
        z.append(6)
        c = len(z) - 1
        backbone.append(c)
        x.append(place(x[c], x[back[0]], x[back[1]], 1.21, 124.0, torsions[m + 4]))
        z.append(8)
        x.append(place(x[c], x[back[0]], x[back[1]], 1.10, 116.0, torsions[m + 4] + 180.0))
        z.append(1)
    carbonyl = ketone[0]
    nxt = backbone[backbone.index(carbonyl) + 1]
    # the ketone oxygen: in the plane of its carbon's two neighbours, opposite their bisector
    x.append(x[carbonyl] - 1.22 * _unit(_unit(x[ketone[1]] - x[carbonyl]) + _unit(x[nxt] - x[carbonyl])))
    z.append(8)
    last = backbone[-1]
    for k in range(1, len(backbone)):
        c = backbone[k]
        if c == carbonyl or (end == "CHO" and c == last):
            continue
        u0 = _unit(x[backbone[k - 1]] - x[c])
        if c == last:                                                  # the methyl
            e1 = _unit(np.cross(u0, [0.3, 0.5, 0.8]))
            e2 = np.cross(u0, e1)
            for p in np.radians([30.0, 150.0, 270.0]):
                x.append(x[c] + 1.09 * (np.cos(np.radians(109.47)) * u0 + np.sin(np.radians(109.47)) * (np.cos(p) * e1 + np.sin(p) * e2)))
                z.append(1)
            continue
        u1 = _unit(x[backbone[k + 1]] - x[c])
        mid, side = -_unit(u0 + u1), _unit(np.cross(u0, u1))
        for s in (1.0, -1.0):
            x.append(x[c] + 1.09 * (np.cos(np.radians(54.75)) * mid + s * np.sin(np.radians(54.75)) * side))
            z.append(1)
    return np.array(z), np.array(x)


def ensemble(rng, n_structs, m, end, folded=0.3):
    """n_structs poses.  The tail: every torsion anti, or gauche with probability 0.1, +- 10 deg.  The head (four torsions): drawn
    uniformly, or -- for the fraction `folded` -- a pose found here in which the hydroxyl points at the ketone oxygen from 2.5 to
    3.3 A, +- 3 deg.  Poses with two atoms closer than 1.6 A that are more than two bonds apart are drawn again."""
    n_t = m + 5
    _, anti = hydroxy_ketone(m, end, np.full(n_t, 180.0))
    bonded = np.linalg.norm(anti[:, None] - anti[None], axis=2) < 1.7          # (the extended pose: bonded pairs only)
    within2 = (bonded.astype(np.int32) @ bonded.astype(np.int32)) > 0
    z, _ = hydroxy_ketone(m, end, np.full(n_t, 180.0))
    o_ketone = int(np.flatnonzero(z == 8)[-1])

    def ok(x):
        return not ((np.linalg.norm(x[:, None] - x[None], axis=2) < 1.6) & ~within2).any()

    template = None
    while template is None:                                             # a folded head: O...O in range, O-H within 30 deg of O...O
        head = rng.uniform(0.0, 360.0, size=4)
        _, x = hydroxy_ketone(m, end, np.concatenate([head, np.full(n_t - 4, 180.0)]))
        oo = x[o_ketone] - x[0]
        if 2.6 < np.linalg.norm(oo) < 3.1 and _unit(oo) @ _unit(x[1] - x[0]) > np.cos(np.radians(30.0)) and ok(x):
            template = head
    out = []
    while len(out) < n_structs:
        tail = rng.choice([180.0, 60.0, -60.0], size=n_t - 4, p=[0.9, 0.05, 0.05]) + rng.normal(0.0, 10.0, size=n_t - 4)
        head = template + rng.normal(0.0, 3.0, size=4) if rng.random() < folded else rng.uniform(0.0, 360.0, size=4)
        _, x = hydroxy_ketone(m, end, np.concatenate([head, tail]))
        if ok(x):
            out.append(x)
    return z, np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "torsion_sets_profile.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shrink", type=int, default=1, help="divide the number of structures by this (trial runs of the tool itself)")
    args = ap.parse_args()

    import tscode_amd
    from tscode_amd import build
    from tscode_amd import torsion_module as tm
    from tscode_amd.utils import cartesian_product

    eng = tscode_amd.get_engine()
    eng.set_option("pass_timing", 1)
    rng = np.random.default_rng(2525)
    committed = json.load(open(os.path.join(ROOT, "profiles", "csearch_multi_profile.json")))
    multi = next(r for r in committed["rows"] if r["workload"] == "augmentation_100")
    rows = []
    for name, n_structs, m, end in (("augmentation_100", 1000, 28, "CHO"), ("augmentation_200", 400, 61, "CH3")):
        n_structs = max(1, n_structs // args.shrink)
        z, x = ensemble(rng, n_structs, m, end)
        keys = ("bond_delta_ms", "hbonds_ms", "reach_ms", "grouping_ms", "quadruplets_ms", "chemistry_ms")
        cold, warm, wall_cold, wall_warm = {k: [] for k in keys}, {k: [] for k in keys}, [], []
        info = {}
        for it in range(args.repeats + 1):
            for bucket, wall, keep in ((cold, wall_cold, False), (warm, wall_warm, True)):
                if not keep:
                    tm._CLASS_CACHE.clear()
                t = {}
                t0 = time.perf_counter()
                ts = tscode_amd.torsion_sets_batch(x, z, None, keep_hb=True, timings=t)
                dt = 1e3 * (time.perf_counter() - t0)
                if it:
                    wall.append(dt)
                    for k in keys:
                        bucket[k].append(t[k])
                info = {"n_classes": t["n_classes"], "bytes_to_device": t["bytes_up"], "bytes_to_host": t["bytes_down"],
                        "structures_with_hydrogen_bonds": int(sum(len(h) > 0 for h in ts.hydrogen_bonds)),
                        "segmented": int(ts.segmented.sum()), "torsions_per_class": [len(s[0]) for s in ts.sets][:16]}
        # the angle tables of an augmentation at the committed workload's width: 6 three-fold torsions (729 rows) per structure, one
        # shuffle each (a chain of this length has some 30 rotatable bonds: 3^30 rows, which neither this code nor the reference builds)
        tables = []
        for it in range(args.repeats + 1):
            t0 = time.perf_counter()
            for _ in range(n_structs):
                tab = cartesian_product(*[tm.N_FOLD_ANGLES[3]] * 6)
                np.random.shuffle(tab)
            if it:
                tables.append(1e3 * (time.perf_counter() - t0))
        row = {"workload": name, "n_atoms": int(len(z)), "n_structs": n_structs, **info,
               "device_ms_bond_delta": stats(cold["bond_delta_ms"]), "device_ms_hbonds": stats(cold["hbonds_ms"]),
               "device_ms_torsion_reach": stats(cold["reach_ms"]),
               "host_ms_grouping": stats(cold["grouping_ms"]), "host_ms_quadruplets_cold": stats(cold["quadruplets_ms"]),
               "host_ms_chemistry_cold": stats(cold["chemistry_ms"]), "host_ms_quadruplets_warm": stats(warm["quadruplets_ms"]),
               "host_ms_chemistry_warm": stats(warm["chemistry_ms"]), "wall_ms_torsion_sets_batch_cold": stats(wall_cold),
               "wall_ms_torsion_sets_batch_warm": stats(wall_warm),
               "host_ms_tables_6_torsions_per_structure": stats(tables),
               "committed_device_ms_one_multi_launch_augmentation_100": multi["device_ms_one_multi_launch"]["median"],
               "committed_host_ms_csearch_candidates_multi_augmentation_100": multi["host_ms_csearch_candidates_multi"]["median"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        print(f"{name}: hbonds {row['device_ms_hbonds']['median']:.3f} ms + reach {row['device_ms_torsion_reach']['median']:.3f} ms on the device, "
              f"{row['wall_ms_torsion_sets_batch_cold']['median']:.1f} ms wall (cold) for {info['n_classes']} classes -- beside "
              f"{multi['device_ms_one_multi_launch']['median']:.1f} ms device / {multi['host_ms_csearch_candidates_multi']['median']:.1f} ms wall of the "
              f"committed augmentation_100 candidate generation", flush=True)
    import torch
    out = {"tool": "tools/torsion_sets_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": build.csrc_digest(),
           "repeats": args.repeats, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
