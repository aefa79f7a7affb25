"""The groups of a three-molecule cyclical embed built on the device (tscode_amd.trimolecular_groups_batch -> tsc_trimolecular_groups, then
tsc_cyclical_embed_groups on the records as they are) beside the way the same embed ran before: the host loop _trimolecular_groups, group by
group, and _run_cyclical_groups on rows expanded to one per (pose, molecule).

    python tools/trimolecular_profile.py [--out profiles/trimolecular_groups_profile.json] [--repeats 3]

Workload (the size of BASELINE config 5): three tree-shaped molecules of 66 / 67 / 66 atoms (tscode_amd.synthetic.make_rotor_molecule, seeds 21 ..
23), two jittered conformers each, the two outermost atoms of each as reactive atoms, pivots of 2 .. 3.5 A (4 x 3 x 3 per conformer triple):
8 x 36 = 288 pivot triples, every triangle closes, 2 304 groups; 6^3 = 216 angle sets of -60 .. 60 degrees: 497 664 candidate poses.

Timed, host wall time around the Python calls (uploads and the last synchronisation included), each way once first (warm-up, and the results are
compared: verdicts identical, poses within 1e-9), then alternating --repeats times; median, smallest and largest:
  old_route_ms        _trimolecular_groups + _run_cyclical_groups        (cyclical_embed_batch(..., groups_on="host"))
  old_groups_ms         of which the host loop over the groups
  new_route_ms        cyclical_embed_batch(...)                           (the default)
  new_groups_ms         of which trimolecular_groups_batch: prologue_ms on the host + one tsc_trimolecular_groups call
  kernel_ms           k_trimolecular_groups by HIP events (tsc_trimolecular_groups_timings under "pass_timing" = 1): median of 20 after 5 warm-ups"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMS, SEEDS, CONFORMERS, PIVOTS = (66, 67, 66), (21, 22, 23), (2, 2, 2), (4, 3, 3)


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def molecules():
    from tscode_amd.synthetic import make_rotor_molecule
    mols, offset = [], 0
    for n, seed, n_conf, n_piv in zip(ATOMS, SEEDS, CONFORMERS, PIVOTS):
        base = np.asarray(make_rotor_molecule(n, [3], seed=seed).coords, dtype=np.float64)
        rng = np.random.default_rng(seed)
        coords = np.stack([base + rng.normal(size=base.shape) * (0.03 if c else 0.0) for c in range(n_conf)])
        coords -= coords.mean(axis=(0, 1))
        reactive = np.sort(np.argsort(np.linalg.norm(coords[0], axis=1))[-2:])
        pivots = []
        for c in range(n_conf):
            vec = rng.normal(size=(n_piv, 3))
            vec *= (rng.uniform(2.0, 3.5, size=n_piv) / np.linalg.norm(vec, axis=1))[:, None]
            centre = coords[c][reactive].mean(axis=0)
            mean = centre + centre / np.linalg.norm(centre) * 1.5 + rng.normal(size=(n_piv, 3)) * 0.2       # outwards of the reactive atoms
            ends = np.array([[reactive[0], reactive[1]] if q % 2 == 0 else [reactive[1], reactive[0]] for q in range(n_piv)])
            pivots.append((vec, mean, ends + offset))
        mols.append(dict(coords=coords, reactive_indices=reactive, reactive_cumnums=np.array([[int(i), int(i) + offset] for i in reactive]), pivots=pivots))
        offset += n
    return mols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trimolecular_groups_profile.json"))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    import tscode_amd
    from tscode_amd import build
    from tscode_amd import embeds as E
    from tscode_amd.utils import cartesian_product

    mols = molecules()
    steps = np.linspace(-60.0, 60.0, 6)
    angles = cartesian_product(steps, steps, steps)
    coords = [m["coords"] for m in mols]
    reactive = [m["reactive_indices"] for m in mols]
    pivots = [m["pivots"] for m in mols]
    cumnums = [m["reactive_cumnums"] for m in mols]
    eng = tscode_amd.get_engine()

    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return (time.perf_counter() - t0) * 1e3, out

    old = lambda: tscode_amd.cyclical_embed_batch(mols, angles, return_trace=True, groups_on="host")
    new = lambda: tscode_amd.cyclical_embed_batch(mols, angles, return_trace=True)
    old_groups = lambda: E._trimolecular_groups(coords, reactive, pivots, cumnums, None, ())
    new_groups = lambda: tscode_amd.trimolecular_groups_batch(mols)
    prologue = lambda: E._trimolecular_prologue(coords, reactive, pivots, cumnums, None, ())

    _, (poses_o, cons_o, tr_o) = timed(old)
    _, (poses_n, cons_n, tr_n) = timed(new)
    assert np.array_equal(tr_o.clash_ok, tr_n.clash_ok) and np.array_equal(tr_o.kept, tr_n.kept) and np.array_equal(cons_o, cons_n), "the two routes disagree"
    assert tr_o.groups == tr_n.groups and poses_o.shape == poses_n.shape and (not len(poses_o) or np.abs(poses_o - poses_n).max() < 1e-9)
    t = {k: [] for k in ("old_route_ms", "new_route_ms", "old_groups_ms", "new_groups_ms", "prologue_ms")}
    for _ in range(args.repeats):
        t["old_route_ms"].append(timed(old)[0]), t["new_route_ms"].append(timed(new)[0])
        t["old_groups_ms"].append(timed(old_groups)[0]), t["new_groups_ms"].append(timed(new_groups)[0]), t["prologue_ms"].append(timed(prologue)[0])
    kernel = []
    with eng.options(pass_timing=1):
        for q in range(25):
            new_groups()
            if q >= 5:
                kernel.append(eng.trimolecular_groups_kernel_ms())
    pro = prologue()
    G, A = len(tr_n.groups), len(angles)
    rec = {"tool": "tools/trimolecular_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(),
           "workload": {"atoms": list(ATOMS), "conformers": list(CONFORMERS), "pivots_per_conformer": list(PIVOTS), "pivot_triples": int(len(pro.conf)),
                        "groups": int(G), "angle_sets": int(A), "poses": int(G * A), "clash_ok": int(tr_n.clash_ok.sum()), "kept": int(tr_n.kept.sum())},
           "repeats": args.repeats, "results_identical": True, "kernel_ms": stats(kernel), "kernel_runs": len(kernel),
           "host_row_arrays_bytes_old_route": int(G * A * 3 * 23 * 8), "record_bytes_new_route": int(G * 3 * 23 * 8)}
    rec.update({k: stats(v) for k, v in t.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
