"""A three-molecule cyclical embed whose kept poses are pruned by RMSD on the device (tscode_amd.cyclical_embed_prune_batch -> tsc_embed_prune_*)
beside the two calls it stands for: cyclical_embed_batch, which fetches every kept pose, then prune_conformers_rmsd, which uploads them again.

    python tools/embed_prune_profile.py [--out profiles/embed_prune_profile.json] [--targets 50000 500000] [--repeats 5] [--clash-thresh 0.15]

Workload (the shape of BASELINE config 5, fed by the real embed): three synthetic molecules of 70 / 70 / 60 atoms, 60 % of them heavy
(atomnos = 6 where index % 5 < 3, else 1), random coordinates of 2 A spread; the conformers after the first are copies with 0.01 A of noise and
share their one pivot (2 .. 3 A), so the poses of different conformer triples are near duplicates: the embed keeps them, the prune removes them.
27 angle sets (-40, 0, 40 degrees per molecule), 8 orientations per pivot triple.  Atoms drawn at random lie closer than bonded ones: the clash
threshold is 0.15 A (at the product's 1.5 A no pose of 200 random atoms passes).  The number of conformers per molecule is chosen from a small
calibration run, and re-chosen from what the size itself keeps until that is within a tenth of --targets; the record states what came out.

Per size, the two routes once first (warm-up; and the results are compared BEFORE any time is taken: both flags per candidate, the prune's verdicts
and pass statistics, the constrained indices equal, the surviving poses equal to the last bit), then alternating --repeats times.  Host wall time
around the Python calls, group building and every transfer included: median, smallest, largest.
  composition_ms      cyclical_embed_batch(...) then prune_conformers_rmsd(poses, atomnos, 0.5)
  new_ms              cyclical_embed_prune_batch(...)
  bytes               what each route moves to and from the host, from the shapes (flags, poses, masks, fragments, records)

Exit status 1 if, at the larger size, the new route's median is not below the composition's smallest time."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMS, SEED, RMSD_THR = (70, 70, 60), 5, 0.5


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def noisy_mols(seed, n_atoms, n_conf, n_pivots, lengths, sigma=0.01):
    """Molecules whose conformers after the first are noisy copies with the first one's pivots (as tests/test_embed_prune.py builds them)."""
    rng = np.random.default_rng(seed)
    mols, off = [], 0
    for m, n in enumerate(n_atoms):
        base = rng.normal(size=(n, 3)) * 2.0
        coords = np.stack([base + (0 if c == 0 else rng.normal(size=(n, 3)) * sigma) for c in range(n_conf[m])])
        reactive = np.sort(rng.choice(n, size=2, replace=False))
        vec = rng.normal(size=(n_pivots[m], 3))
        vec *= (rng.uniform(*lengths, size=n_pivots[m]) / np.linalg.norm(vec, axis=1))[:, None]
        mean = base[reactive].mean(axis=0) + rng.normal(size=(n_pivots[m], 3))
        ends = np.array([[reactive[0], reactive[1]] if q % 2 == 0 else [reactive[1], reactive[0]] for q in range(n_pivots[m])])
        mols.append(dict(coords=coords, reactive_indices=reactive, pivots=[(vec.copy(), mean.copy(), ends + off)] * n_conf[m],
                         reactive_cumnums=np.array([[i, i + off] for i in reactive], dtype=np.int64)))
        off += n
    return mols


def conformers_for(target, kept_per_triple):
    """(a, b, c) near a cube whose product times kept_per_triple comes closest to target."""
    want = max(1.0, target / max(kept_per_triple, 1e-9))
    n = max(1, int(round(want ** (1.0 / 3.0))))
    options = [(n + i, n + j, n + k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if n + i >= 1 and n + j >= 1 and n + k >= 1 and i >= j >= k]
    return min(options, key=lambda t: abs(t[0] * t[1] * t[2] - want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_prune_profile.json"))
    ap.add_argument("--targets", type=int, nargs="+", default=[50000, 500000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clash-thresh", type=float, default=0.15)
    args = ap.parse_args()

    import torch
    import tscode_amd
    from tscode_amd import build
    from tscode_amd import embeds as E
    from tscode_amd.utils import cartesian_product

    steps = np.array([-40.0, 0.0, 40.0])
    angles = cartesian_product(steps, steps, steps)
    n_total = sum(ATOMS)
    atomnos = np.where(np.arange(n_total) % 5 < 3, 6, 1)
    n_heavy = int((atomnos != 1).sum())
    eng = tscode_amd.get_engine()
    kw = dict(clash_thresh=args.clash_thresh)

    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return (time.perf_counter() - t0) * 1e3, out

    def composition(mols):
        p, c, tr = tscode_amd.cyclical_embed_batch(mols, angles, return_trace=True, **kw)
        out, mask = tscode_amd.prune_conformers_rmsd(p, atomnos, RMSD_THR)
        return out, c[mask], tr, mask, tscode_amd.last_prune_stats()

    def new(mols):
        out, c, tr = tscode_amd.cyclical_embed_prune_batch(mols, angles, atomnos, RMSD_THR, return_trace=True, **kw)
        return out, c, tr, tr.survived, tr.prune_stats

    passes = lambda st: [(s["k"], s["n_active_before"], s["n_active_after"], s["pairs_evaluated"]) for s in st]
    calib = new(noisy_mols(SEED, ATOMS, (2, 2, 2), (1, 1, 1), (2.0, 3.0)))
    kept_per_triple = calib[2].kept.sum() / 8.0
    sizes = []
    for target in args.targets:
        per_triple = kept_per_triple
        for _ in range(3):      # (the share of poses that pass drifts with the conformers drawn: re-sized from what the size itself keeps)
            n_conf = conformers_for(target, per_triple)
            mols = noisy_mols(SEED, ATOMS, n_conf, (1, 1, 1), (2.0, 3.0))
            _, new_res = timed(lambda: new(mols))
            kept_here = int(new_res[2].kept.sum())
            if abs(kept_here - target) <= 0.1 * target:
                break
            per_triple = kept_here / float(np.prod(n_conf))
        _, old_res = timed(lambda: composition(mols))
        (po, co, tro, mo, so), (pn, cn, trn, mn, sn) = old_res, new_res
        assert np.array_equal(tro.clash_ok, trn.clash_ok) and np.array_equal(tro.kept, trn.kept) and np.array_equal(tro.group_of, trn.group_of), "flags differ"
        assert np.array_equal(mo, mn) and np.array_equal(co, cn) and passes(so) == passes(sn), "the prune's verdicts or statistics differ"
        assert po.shape == pn.shape and np.ascontiguousarray(po).tobytes() == pn.tobytes(), "the surviving poses differ"
        N, K, S, G = len(trn.kept), int(trn.kept.sum()), int(mn.sum()), len(trn.groups)
        del old_res, new_res, po, pn
        t = {"composition_ms": [], "new_ms": []}
        for _ in range(args.repeats):
            t["composition_ms"].append(timed(lambda: composition(mols))[0])
            t["new_ms"].append(timed(lambda: new(mols))[0])
        frag_bytes = sum(c * a for c, a in zip(n_conf, ATOMS)) * 24
        slabs = len(E._slabs(G, len(angles), E.DEFAULT_MAX_POSES_PER_CALL))
        records = G * 3 * (7 * 24 + 8) + angles.size * 8
        pose_bytes = n_total * 24
        prune_upload = K * pose_bytes if K >= 2048 else K * n_heavy * 24          # (prune_conformers_rmsd gathers small inputs on the host)
        rec = {"conformers": list(n_conf), "groups": G, "candidates": N, "clash_ok": int(trn.clash_ok.sum()), "kept": K, "survived": S,
               "prune_passes": len(sn), "results_identical": True,
               "bytes": {"composition_to_host": 2 * N + K * pose_bytes + K, "composition_to_device": slabs * frag_bytes + records + prune_upload,
                         "new_to_host": 2 * N + K + S * pose_bytes, "new_to_device": frag_bytes + records,
                         "device_rows_of_the_run": K * (24 * n_heavy + 100 * 3)}}
        rec.update({k: stats(v) for k, v in t.items()})
        rec["speedup_median"] = rec["composition_ms"]["median"] / rec["new_ms"]["median"]
        sizes.append(rec)
        print(json.dumps(rec, sort_keys=True), flush=True)
    out = {"tool": "tools/embed_prune_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(), "repeats": args.repeats,
           "workload": {"atoms": list(ATOMS), "heavy_atoms": n_heavy, "angle_sets": int(len(angles)), "clash_thresh": args.clash_thresh, "rmsd_thr": RMSD_THR,
                        "conformer_noise": 0.01, "seed": SEED, "kept_per_conformer_triple_at_calibration": float(kept_per_triple)},
           "sizes": sizes}
    last = sizes[-1]
    out["bar"] = {"rule": "at the larger size the new route's median is below the composition's smallest time",
                  "new_median_ms": last["new_ms"]["median"], "composition_min_ms": last["composition_ms"]["min"],
                  "met": bool(last["new_ms"]["median"] < last["composition_ms"]["min"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["bar"], sort_keys=True))
    return 0 if out["bar"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
