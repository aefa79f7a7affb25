"""Kernel time of the batched non-covalent-interaction finder (tsc_nci_dev, csrc/nci.hpp) on device-resident ensembles, beside the
bond-graph check of the same arrays (tsc_bond_delta_dev: the same read stream and the same pair loop over ALL pairs, the scale).

    python tools/nci_profile.py [--out profiles/nci_profile.json] [--warmup 5] [--repeats 20]

Shapes: 500 000 x 200 atoms (three molecules of a naphthalene, a benzene and a pyridine each -- 22 C / N atoms per molecule --
stacked 3.6 A apart, filled up with water-like atoms) and 1 000 000 x 50 atoms (two molecules), built from
tscode_amd.synthetic.aromatic_block; Gaussian noise per structure, sigma from AROMATIC_SIGMAS.  Times are HIP-event times of the
kernel alone (tsc_nci_timings / tsc_topology_timings under the context option "pass_timing"), the median of --repeats launches
after --warmup, for the counts-only form and for the form that writes every list."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def system(n_atoms):
    """(molecules for make_aromatic_ensemble) of exactly n_atoms atoms: 200 -> three molecules, otherwise two."""
    n_mols = 3 if n_atoms >= 150 else 2
    per = [n_atoms // n_mols + (1 if m < n_atoms % n_mols else 0) for m in range(n_mols)]
    mols = []
    for m, size in enumerate(per):
        z = 3.6 * m
        mol = [("benzene", (0, 0, z)), ("pyridine", (7, 0, z))]
        if n_mols == 3:
            mol.append(("naphthalene", (-8, 0, z)))
        used = 12 + 11 + (18 if n_mols == 3 else 0)
        for q in range(size - used):       # fillers: O, H, H, ... on a grid beside the rings, 2.4 A apart
            mol.append((("O", "H", "H")[q % 3], (2.4 * (q % 8) - 8, 6 + 2.4 * (q // 8), z)))
        mols.append(mol)
    return mols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nci_profile.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shapes", default="500000x200,1000000x50")
    args = ap.parse_args()

    import torch

    import tscode_amd
    from tscode_amd import build
    from tscode_amd.graph_manipulations import bond_tables
    from tscode_amd.nci import NCI_DICT, check_nci_args, nci_tables
    from tscode_amd.synthetic import AROMATIC_SIGMAS, make_aromatic_ensemble

    eng = tscode_amd.get_engine()
    dev = torch.device("cuda", eng.device)
    rows = []
    for shape in args.shapes.split(","):
        N, n = (int(v) for v in shape.split("x"))
        base, _, atomnos, ids, _ = make_aromatic_ensemble(system(n), 1, 2200 + n, sigmas=(0.0,))
        assert len(atomnos) == n
        _, z, ids, atom_mol, _, rule, _ = check_nci_args(base[None], atomnos, None, ids)
        classes, thr, ring_thr, cand = nci_tables(z)
        gen = torch.Generator(device=dev)
        gen.manual_seed(2200 + n)
        sigma = torch.tensor(AROMATIC_SIGMAS, dtype=torch.float64, device=dev)[torch.randint(0, len(AROMATIC_SIGMAS), (N,), device=dev, generator=gen)]
        coords = (torch.from_numpy(base).to(dev)[None] + torch.randn((N, n, 3), dtype=torch.float64, device=dev, generator=gen) * sigma[:, None, None]).contiguous()
        w = (n + 63) // 64
        counts = torch.zeros((N, 4), dtype=torch.int32, device=dev)
        overflow = torch.zeros(N, dtype=torch.uint8, device=dev)
        lists = dict(pair_bits=torch.zeros((N, n, w), dtype=torch.int64, device=dev), ring_atoms=torch.zeros((N, 64, 6), dtype=torch.int16, device=dev),
                     ring_owner=torch.zeros((N, 64), dtype=torch.uint8, device=dev), ring_center=torch.zeros((N, 64, 3), dtype=torch.float64, device=dev),
                     ring_atom_bits=torch.zeros((N, 64, w), dtype=torch.int64, device=dev), ring_ring_bits=torch.zeros((N, 64), dtype=torch.int64, device=dev))
        mask = torch.zeros(N, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        row = {"n_structs": N, "n_atoms": n, "molecules": [int(v) for v in ids],
               "candidates_per_molecule": [int(cand[atom_mol == m].sum()) for m in range(len(ids))]}
        with eng.options(pass_timing=1):
            for name, kw in (("counts_only", {}), ("every_list", lists)):
                times = []
                for it in range(args.warmup + args.repeats):
                    eng.nci_dev(coords, N, n, classes, thr, atom_mol, len(ids), cand, ring_thr, NCI_DICT["PhPh"][0], None, False, rule, counts, overflow, **kw)
                    if it >= args.warmup:
                        times.append(eng.nci_kernel_ms())
                row[name + "_ms"] = float(np.median(times))
                row[name + "_ms_min_max"] = [float(min(times)), float(max(times))]
            b_classes, b_thr = bond_tables(atomnos)
            times = []
            for it in range(args.warmup + args.repeats):
                eng.bond_delta_dev(coords, N, n, b_classes, b_thr, None, None, None, False, 0, mask)
                if it >= args.warmup:
                    times.append(eng.topology_kernel_ms())
        row["bond_delta_ms"] = float(np.median(times))
        row["ratio_to_bond_delta"] = row["counts_only_ms"] / row["bond_delta_ms"]
        row["structures_per_s"] = N / (row["counts_only_ms"] * 1e-3)
        row["microseconds_per_structure"] = row["counts_only_ms"] * 1e3 / N
        row["bytes_per_s"] = (N * n * 24 + N * 17) / (row["counts_only_ms"] * 1e-3)
        c = counts.cpu().numpy()
        row["mean_counts"] = [float(v) for v in c.mean(0)]
        row["overflowed"] = int(overflow.sum().item())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del coords, lists
    out = {"tool": "tools/nci_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": build.csrc_digest(),
           "warmup": args.warmup, "repeats": args.repeats, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
