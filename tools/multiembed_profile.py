"""A whole multiembed in one pass (tscode_amd.multiembed_batch -> tsc_cyclical_embed_groups) beside the way the same result was reached before:
a Python loop over the arrangements of cyclical_embed_batch (tsc_cyclical_embed on host-expanded rows) + fitness_mask +
similarity_refining_batch(rmsd=False).

    python tools/multiembed_profile.py [--out profiles/multiembed_profile.json] [--repeats 5] [--conformers 8] [--reactive 4]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/multiembed_profile.py --kernels-only
    python tools/multiembed_profile.py --merge-kernel-stats DIR [--out ...]

Workload: two synthetic molecules of 40 atoms (tscode_amd.synthetic.make_rotor_molecule, seeds 11 and 12), four sp2 carbons of each as reactive
atoms (144 arrangements), 8 jittered conformers each, the child's default 36 angle sets, the child's thresholds.

Timed: host wall time around the whole Python call, reactive molecules, uploads and the last synchronisation included (both ways return host
arrays, so both end in the library's wait).  Both ways are run once first (warm-up, and the results are compared: masks identical, structures
within 1e-9); then they alternate, --repeats times each; median, smallest and largest are recorded.  The loop builds each ordered reactive
pair's molecule once, as multiembed_batch does, so the difference is the embed and the stages behind it.

--kernels-only runs ONE grouped call and ONE row call on the same records and nothing else, for a kernel trace of its own: the parameter
kernels k_cyclical_embed_group_params / k_cyclical_embed_params side by side.  --merge-kernel-stats reads that trace's kernel_stats.csv into the
record.  The bytes each entry point uploads for its records are computed from the shapes."""

import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REACTIVE = ([1, 3, 6, 11, 13, 15], [3, 5, 8, 12, 13, 18])      # sp2 carbons of the two molecules (three neighbours each)
KERNELS = ("k_cyclical_embed_group_params", "k_cyclical_embed_params")


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def molecules(n_conf, n_reactive):
    from tscode_amd.synthetic import make_rotor_molecule
    out = []
    for seed, reactive in zip((11, 12), REACTIVE):
        m = make_rotor_molecule(40, [3], seed=seed)
        rng = np.random.default_rng(seed)
        coords = np.stack([m.coords + rng.normal(size=m.coords.shape) * (0.03 if c else 0.0) for c in range(n_conf)])
        coords -= coords.mean(axis=(0, 1))                       # the ensemble's centroid, as Hypermolecule subtracts it
        out.append(dict(coords=coords, atomnos=np.asarray(m.atomnos), reactive_indices=np.array(reactive[:n_reactive]), bonds=np.array(m.bonds)))
    return out


def loop_of_existing_calls(mols, arrs, angles, targets, quads=None):
    """Per arrangement: cyclical_embed_batch -> fitness_mask -> similarity_refining_batch(rmsd=False); what each leaves, in arrangement order."""
    import tscode_amd
    n1 = len(mols[0]["atomnos"])
    atomnos = np.concatenate([m["atomnos"] for m in mols])
    made = [{}, {}]
    structures, constrained, arr_of = [], [], []
    for a, ((ix_1, ix_2), (iy_1, iy_2)) in enumerate(arrs.tolist()):
        rms = []
        for side, (pair, off) in enumerate((((ix_1, iy_1), 0), ((ix_2, iy_2), n1))):
            if pair not in made[side]:
                m = mols[side]
                made[side][pair] = tscode_amd.reactive_molecule(m["coords"], m["atomnos"], list(pair), m["bonds"], cumnum_offset=off)
            rms.append(made[side][pair])
        poses, cons = tscode_amd.cyclical_embed_batch(rms, angles, rigid_shortcut=True, max_norm_delta=5, pairings=[[ix_1, ix_2 + n1], [iy_1, iy_2 + n1]])
        if not len(poses):
            continue
        fit = tscode_amd.fitness_mask(poses, cons, np.tile(targets[a], (len(poses), 1)), 5)
        if not fit.any():
            continue
        (left, mask), = tscode_amd.similarity_refining_batch([poses[fit]], atomnos, quadruplets=None if quads is None else [quads[a]], rmsd=False)
        structures.append(left), constrained.append(cons[fit][mask]), arr_of.append(np.full(len(left), a))
    n = len(atomnos)
    if not structures:
        return np.zeros((0, n, 3)), np.zeros((0, 2, 2), dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(structures), np.concatenate(constrained), np.concatenate(arr_of)


def record_bytes(G, A, n_mols=2):
    """Bytes of group records each entry point uploads (fragments aside): seven vectors, n_reactive, conf_idx, and the angles / group offsets."""
    rows = G * A * n_mols
    return {"tsc_cyclical_embed": rows * (7 * 24 + 4 + 4 + 8) + (G + 1) * 4,
            "tsc_cyclical_embed_groups": G * n_mols * (7 * 24 + 4 + 4) + A * n_mols * 8}


def the_records(mols):
    """The group records of the whole multiembed, as multiembed_batch builds them."""
    import tscode_amd
    from tscode_amd import multiembed as M
    m1, m2, angles = M.check_args(mols[0], mols[1])
    arrs = M.arrangements(m1["reactive_indices"], m2["reactive_indices"])
    n1 = len(m1["atomnos"])
    made = [{}, {}]
    for side, (m, off) in enumerate(((m1, 0), (m2, n1))):
        for pair in sorted({(int(a[0][side]), int(a[1][side])) for a in arrs.tolist()}):
            made[side][pair] = tscode_amd.reactive_molecule(m["coords"], m["atomnos"], list(pair), m["bonds"], cumnum_offset=off)
    blocks, _, per = M.group_records(made[0], made[1], arrs, n1)
    return blocks, per, angles, arrs


def kernels_only(mols):
    import tscode_amd
    blocks, per, angles, _ = the_records(mols)
    eng = tscode_amd.get_engine()
    frags = tscode_amd.FragmentSet([m["coords"] for m in mols])
    G, A = len(blocks), len(angles)
    cut = lambda lo, hi, dtype=np.float64: np.ascontiguousarray(blocks[:, :, lo:hi], dtype=dtype)
    expand = lambda lo, hi, dtype=np.float64: np.repeat(cut(lo, hi, dtype), A, axis=0).reshape(-1, hi - lo)
    ok_g, kept_g, _ = eng.cyclical_embed_groups(frags, *[cut(lo, lo + 3) for lo in range(0, 21, 3)], cut(21, 22, np.int32), cut(22, 23, np.int32), angles, 1.5, 0,
                                                want_poses=False)
    ok_r, kept_r, _ = eng.cyclical_embed(frags, *[expand(lo, lo + 3) for lo in range(0, 21, 3)], expand(21, 22, np.int32).reshape(-1),
                                         np.tile(angles, (G, 1)).reshape(-1), expand(22, 23, np.int32).reshape(-1), np.arange(G + 1, dtype=np.int32) * A, 1.5, 0,
                                         want_poses=False)
    assert np.array_equal(ok_g, ok_r) and np.array_equal(kept_g, kept_r), "the two entry points disagree"
    print(json.dumps({"groups": G, "angle_sets": A, "poses": G * A, "clash_ok": int(ok_g.sum()), "kept": int(kept_g.sum())}))


def merge_kernel_stats(path, out):
    f = max(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    rows = list(csv.DictReader(open(f)))
    rec = json.load(open(out)) if os.path.exists(out) else {}
    rec["parameter_kernels"] = {}
    for name in KERNELS:
        hit = [r for r in rows if r["Name"].split("(")[0].split("<")[0].endswith(name)]
        for r in hit:
            rec["parameter_kernels"][name] = {"calls": int(r["Calls"]), "total_us": int(r["TotalDurationNs"]) / 1e3, "average_us": float(r["AverageNs"]) / 1e3}
    rec["all_kernels_us"] = {r["Name"].split("(")[0]: int(r["TotalDurationNs"]) / 1e3 for r in rows}
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(rec["parameter_kernels"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiembed_profile.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--conformers", type=int, default=8)
    ap.add_argument("--reactive", type=int, default=4, help="reactive atoms per molecule (2 .. 6)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-kernel-stats", default=None)
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)
    mols = molecules(args.conformers, args.reactive)
    if args.kernels_only:
        return kernels_only(mols)

    import tscode_amd
    from tscode_amd import build

    def batch():
        t0 = time.perf_counter()
        out = tscode_amd.multiembed_batch(mols[0], mols[1])
        return (time.perf_counter() - t0) * 1e3, out

    _, out = batch()
    angles = tscode_amd.multiembed.child_angles()

    def loop():
        t0 = time.perf_counter()
        res = loop_of_existing_calls(mols, out.arrangements, angles, out.targets)
        return (time.perf_counter() - t0) * 1e3, res

    _, (structures, constrained, arr_of) = loop()
    assert np.array_equal(arr_of, out.arrangement_of) and np.array_equal(constrained, out.constrained_indices), "the two ways keep different structures"
    assert structures.shape == out.structures.shape and (not len(structures) or np.abs(structures - out.structures).max() < 1e-9)
    tb, tl = [], []
    for _ in range(args.repeats):
        tb.append(batch()[0])
        tl.append(loop()[0])
    blocks, per, _, _ = the_records(mols)
    G, A = len(blocks), len(angles)
    import torch
    eng = tscode_amd.get_engine()
    rec = {"tool": "tools/multiembed_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(),
           "workload": {"atoms": [int(len(m["atomnos"])) for m in mols], "conformers": args.conformers, "reactive_atoms": args.reactive,
                        "arrangements": int(len(out.arrangements)), "groups": int(G), "angle_sets": int(A), "poses": int(G * A)},
           "counts_summed": dict(zip(("candidates", "clash_ok", "kept", "fit", "after_tfd", "after_moi"), out.counts.sum(axis=0).tolist())),
           "repeats": args.repeats, "multiembed_batch_ms": stats(tb), "loop_of_existing_calls_ms": stats(tl),
           "results_identical": True, "record_bytes_uploaded": record_bytes(G, A)}
    if os.path.exists(args.out):
        old = json.load(open(args.out))
        for k in ("parameter_kernels", "all_kernels_us"):
            if k in old:
                rec[k] = old[k]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))
    print(f"multiembed_batch {rec['multiembed_batch_ms']}\nloop             {rec['loop_of_existing_calls_ms']}")


if __name__ == "__main__":
    main()
