"""Kernel time of the reactive-atom orbitals and pivots (tsc_orbitals_dev, csrc/orbitals.hpp) on device-resident conformer ensembles,
the host call with its copies (tsc_orbitals), and one launch of the embed kernel (k_transform through tsc_transform_batch_dev; its fused
sibling k_transform_describe runs inside tsc_pipeline_dev only) at the same number of rows for scale.

    python tools/orbitals_profile.py [--out profiles/orbitals_profile.json] [--warmup 5] [--repeats 20] [--sizes 20000,500000]

The molecule: propenal (CH2=CH-CH=O, reactive atoms C0 and O3: sp2 + Ketone, four pivots) padded to 50 atoms with far hydrogens --
the molecule of G23's propenal50 -- with Gaussian noise of 0.04 A per conformer.  Kernel times are HIP-event times of the kernel alone
(tsc_orbitals_timings under the context option "pass_timing"), the median of --repeats launches after --warmup.  Algorithmic bytes per
conformer = the atoms the recipes touch (24 bytes each, counted once per recipe slot) + every output written."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def propenal50():
    c60, s60 = 0.5, 0.8660254037844386
    rows = [(6, 0, 0, 0), (6, 1.34, 0, 0), (6, 1.34 + 1.47 * c60, 1.47 * s60, 0), (8, 1.34 + 1.47 * c60 + 1.22, 1.47 * s60, 0), (1, -0.54, 0.93, 0),
            (1, -0.54, -0.93, 0), (1, 1.34 + 1.09 * c60, -1.09 * s60, 0), (1, 1.34 + 1.47 * c60 - 1.09 * c60, 1.47 * s60 + 1.09 * s60, 0)]
    rows += [(1, 25.0 + 4.0 * (q % 7), 25.0 + 4.0 * (q // 7), 25.0) for q in range(42)]
    edges = [(0, 1), (0, 4), (0, 5), (1, 2), (1, 6), (2, 3), (2, 7)]
    return np.array([r[0] for r in rows]), np.array([r[1:] for r in rows], dtype=np.float64), np.array(edges)


def algorithmic_bytes(recipes):
    touched = sum(1 + int((r["nb"] >= 0).sum()) + int((r["ex"] >= 0).sum()) for r in recipes)
    R = len(recipes)
    written = R * (2 * 4 * 24 + 2) + 1 + 16 * (24 + 24 + 2) + 1
    return touched * 24, written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbitals_profile.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sizes", default="20000,500000")
    args = ap.parse_args()

    import torch

    import tscode_amd
    from tscode_amd import build
    from tscode_amd.reactive_atoms import orbital_recipes

    eng = tscode_amd.get_engine()
    dev = torch.device("cuda", eng.device)
    z, base, edges = propenal50()
    n = len(z)
    host = orbital_recipes(z, [0, 3], edges)
    rec, mode = host["recipes"], host["sigmatropic_mode"]
    bytes_in, bytes_out = algorithmic_bytes(rec)
    golden = os.path.join(ROOT, "tests", "golden", "G23_orbitals.json")
    reference = json.load(open(golden))["reference_seconds_per_conformer"] if os.path.exists(golden) else None
    rows = []
    for C in (int(v) for v in args.sizes.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(2300 + C)
        coords = (torch.from_numpy(base).to(dev)[None] + torch.randn((C, n, 3), dtype=torch.float64, device=dev, generator=gen) * 0.04).contiguous()
        out = [torch.zeros((C, 2, 4, 3), dtype=torch.float64, device=dev), torch.zeros((C, 2, 4, 3), dtype=torch.float64, device=dev),
               torch.zeros((C, 2), dtype=torch.uint8, device=dev), torch.zeros((C, 2), dtype=torch.uint8, device=dev),
               torch.zeros(C, dtype=torch.uint8, device=dev), torch.zeros((C, 16, 3), dtype=torch.float64, device=dev),
               torch.zeros((C, 16, 3), dtype=torch.float64, device=dev), torch.zeros((C, 16, 2), dtype=torch.int8, device=dev),
               torch.zeros(C, dtype=torch.uint8, device=dev)]
        torch.cuda.synchronize()
        with eng.options(pass_timing=1):
            times = []
            for it in range(args.warmup + args.repeats):
                eng.orbitals_dev(coords, C, n, rec, mode, False, *out)
                if it >= args.warmup:
                    times.append(eng.orbitals_kernel_ms())
        eng.synchronize()
        kernel_ms = float(np.median(times))
        x_host = coords.cpu().numpy()
        calls = []
        for it in range(3):
            t0 = time.perf_counter()
            res = eng.orbitals(x_host, rec, mode, False)
            calls.append((time.perf_counter() - t0) * 1e3)
        # one launch of the embed kernel on C rows of the same molecule (identity placement)
        frags = tscode_amd.FragmentSet([x_host[:min(C, 1000)]])
        conf_idx = torch.from_numpy((np.arange(C) % min(C, 1000)).astype(np.int32).reshape(C, 1)).to(dev)
        rot = torch.eye(3, dtype=torch.float64, device=dev).repeat(C, 1, 1, 1).contiguous()               # [C, 1, 3, 3]
        pos = torch.zeros((C, 1, 3), dtype=torch.float64, device=dev)
        d_frags = torch.from_numpy(frags.flat).to(dev)
        poses = torch.zeros((C, n, 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t = []
        for it in range(args.warmup + args.repeats):
            eng.timer_begin()
            eng.transform_batch_dev(frags, d_frags, conf_idx, rot, pos, C, poses)
            ms = eng.timer_end()
            if it >= args.warmup:
                t.append(ms)
        embed_ms = float(np.median(t))
        del poses
        row = {"n_conformers": C, "n_atoms": n, "n_reactive": 2, "classes": host["classes"], "kernel_ms": kernel_ms,
               "kernel_ms_min_max": [float(min(times)), float(max(times))], "host_call_ms_with_copies": float(np.median(calls)),
               "algorithmic_bytes_per_conformer": {"read": bytes_in, "written": bytes_out},
               "algorithmic_bytes_per_s": (bytes_in + bytes_out) * C / (kernel_ms * 1e-3),
               "nanoseconds_per_conformer": kernel_ms * 1e6 / C, "embed_launch_ms_same_rows": embed_ms,
               "mean_pivots": float(res["n_pivots"].mean()), "reference_seconds_per_conformer": reference}
        if reference:
            row["reference_seconds_total"] = (reference["orbitals"] + reference["pivots"]) * C
        rows.append(row)
        print(json.dumps(row), flush=True)
        del coords, out
    result = {"tool": "tools/orbitals_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": build.csrc_digest(),
              "warmup": args.warmup, "repeats": args.repeats, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
