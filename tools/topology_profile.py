"""Kernel time of the batched bond-graph check (tsc_bond_delta_dev, csrc/topology.hpp) on device-resident ensembles, beside the
clash mask of the same arrays (tsc_clash_mask_dev: the same read stream, the natural yardstick).

    python tools/topology_profile.py [--out profiles/topology_profile.json] [--warmup 5] [--repeats 20]

Shapes: 1 000 000 x 50 atoms and 500 000 x 200 atoms, chains as the G21 fixtures draw them (one base, Gaussian noise per
structure).  Times are HIP-event times of the kernel alone (tsc_topology_timings under the context option "pass_timing"), the
median of --repeats launches after --warmup; the clash mask is timed with the context's event timer around the call.
Derived: bytes/s for N n 24 + N bytes against the HBM figures of DESIGN.md section 3 (8 TB/s specified, 6.3 achievable), pair
compares per second against the fp64 vector peak."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12       # MI355X specification ("Peaks")
HBM_ACHIEVABLE_BYTES_PER_S = 6.3e12 # ... and what a copy achieves (the same line; k_transform's stores reach 3.9 - 4.6e12, MEASURED.md section 9)
FP64_VECTOR_FLOPS = 78.6e12         # MI355X vector fp64 peak
FLOPS_PER_PAIR = 8                  # three differences, three products, two sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topology_profile.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shapes", default="1000000x50,500000x200")
    args = ap.parse_args()

    import torch

    import tscode_amd
    from tscode_amd import build
    from tscode_amd.graph_manipulations import bond_tables, pack_edges
    from tscode_amd.synthetic import CHAIN_ELEMENTS, CHAIN_SIGMAS, make_chain

    eng = tscode_amd.get_engine()
    dev = torch.device("cuda", eng.device)
    rows = []
    for shape in args.shapes.split(","):
        N, n = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(2100 + n)
        base = torch.from_numpy(make_chain(rng, n)).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(2100 + n)
        sigma = torch.tensor(CHAIN_SIGMAS, dtype=torch.float64, device=dev)[torch.randint(0, len(CHAIN_SIGMAS), (N,), device=dev, generator=gen)]
        coords = (base[None] + torch.randn((N, n, 3), dtype=torch.float64, device=dev, generator=gen) * sigma[:, None, None]).contiguous()
        atomnos = np.array([CHAIN_ELEMENTS[i % len(CHAIN_ELEMENTS)] for i in range(n)])
        classes, thr = bond_tables(atomnos)
        ref = pack_edges(np.array([(i, i + 1) for i in range(n - 1)]), n)
        mask = torch.zeros(N, dtype=torch.uint8, device=dev)
        formed = torch.zeros(N, dtype=torch.int32, device=dev)
        broken = torch.zeros(N, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        row = {"n_structs": N, "n_atoms": n}
        with eng.options(pass_timing=1):
            for name, kw in (("verdict_only", {}), ("with_counts", {"formed": formed, "broken": broken})):
                times = []
                for it in range(args.warmup + args.repeats):
                    eng.bond_delta_dev(coords, N, n, classes, thr, None, ref, None, False, 0, mask, **kw)
                    if it >= args.warmup:
                        times.append(eng.topology_kernel_ms())
                row[name + "_ms"] = float(np.median(times))
                row[name + "_ms_min_max"] = [float(min(times)), float(max(times))]
        row["unchanged_share"] = float(mask.float().mean().item())
        times = []
        for it in range(args.warmup + args.repeats):
            eng.timer_begin()
            eng.clash_mask_dev(coords, N, n, None, 1.5, 0, mask)
            ms = eng.timer_end()
            if it >= args.warmup:
                times.append(ms)
        row["clash_mask_ms"] = float(np.median(times))
        t = row["verdict_only_ms"] * 1e-3
        pairs = N * n * (n - 1) / 2
        row["ratio_to_clash_mask"] = row["verdict_only_ms"] / row["clash_mask_ms"]
        row["bytes_per_s"] = (N * n * 24 + N) / t
        row["share_of_hbm_peak"] = row["bytes_per_s"] / HBM_PEAK_BYTES_PER_S
        row["share_of_hbm_achievable"] = row["bytes_per_s"] / HBM_ACHIEVABLE_BYTES_PER_S
        row["pair_compares_per_s"] = pairs / t
        row["share_of_fp64_vector_peak"] = pairs * FLOPS_PER_PAIR / t / FP64_VECTOR_FLOPS
        rows.append(row)
        print(json.dumps(row), flush=True)
        del coords
    out = {"tool": "tools/topology_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": build.csrc_digest(),
           "warmup": args.warmup, "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE_BYTES_PER_S, "fp64_vector_flops": FP64_VECTOR_FLOPS, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
