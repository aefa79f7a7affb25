"""The 16-row matrix-core pair kernel's item shape, pass by pass: every segment length is run in ONE process, alternating, several rounds,
so that drift between processes cancels (tools/sweep.py does the same for whole steps).

    [TSCODE_AMD_LIB=tscode_amd/ab_libs/NAME.so] python tools/sweep_items.py CONFIG [--segs 0,256,512,...] [--rounds 3] [--heavy N,H]

The items per workgroup are a build's (-DTSC_MM16_ITEMS=2 / 4 through tools/build_variant.py; 0, the default: the rule of pass_plan.hpp; one item
per workgroup was swept with a third instantiation of the kernel that did not pay and is not in the tree: MEASURED.md 33), the segment length the
option "seg_cols" (0: the rule; halved like the rule's own below four segments a row -- -DTSC_MM16_SEG=cols gives a build one length unhalved).  Per candidate and round: 100 steps with the library's events off (ms per step), then 5 steps with
all of them on, of which every pass's median `gpu_ms` is taken (the detail steps of bench.py --full, more of them).  Printed: per pass, the
median over the rounds and the spread, in us.  --heavy N,H times whole eng.prune_heavy calls instead (median of 5 after 3 warm-up calls)."""
import argparse
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("config", nargs="?", default="C3")
ap.add_argument("--segs", default="0,256,512,1024,2048,4096")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--heavy", default=None)
args = ap.parse_args()
segs = [int(x) for x in args.segs.split(",")]

if args.heavy:
    from tscode_amd import get_engine
    N, h = (int(x) for x in args.heavy.split(","))
    eng = get_engine(0)
    rng = np.random.default_rng(5)
    base = rng.normal(size=(N // 6 + 1, h, 3)) * 3
    heavy = np.ascontiguousarray((base[:, None] + rng.normal(size=(N // 6 + 1, 6, h, 3)) * 0.03).reshape(-1, h, 3)[rng.permutation((N // 6 + 1) * 6)][:N])
    for seg in segs:
        with eng.options(seg_cols=seg):
            for _ in range(3):
                mask, st = eng.prune_heavy(heavy, 0.5, 0)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                mask, st = eng.prune_heavy(heavy, 0.5, 0)
                ts.append((time.perf_counter() - t0) * 1e3)
        print(f"prune_heavy {N} x {h}  seg_cols {seg:5d}: median {statistics.median(ts):.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})  {int(mask.sum())} survivors", flush=True)
    sys.exit(0)

from tscode_amd.pipeline import DevicePipeline
from tscode_amd.synthetic import make_config

pipe = DevicePipeline(make_config(args.config), device_index=0, mode=0)
for _ in range(10):
    pipe.step()
step_ms = {s: [] for s in segs}
pass_us = {s: [] for s in segs}   # per round: {k: us}
ref = None
for rnd in range(args.rounds):
    for seg in segs:
        pipe.set_option("seg_cols", seg)
        pipe.set_option("pass_timing", 0)
        for _ in range(3):
            pipe.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            r = pipe.step()
        torch.cuda.synchronize()
        step_ms[seg].append((time.perf_counter() - t0) / args.steps * 1e3)
        pipe.set_option("pass_timing", 2)
        per = {}
        for _ in range(5):
            r = pipe.step()
            torch.cuda.synchronize()
            for s in r["stats"]:
                per.setdefault(int(s["k"]), []).append(s["gpu_ms"] * 1e3)
        pass_us[seg].append({k: statistics.median(v) for k, v in per.items()})
        if ref is None:
            ref = (r["n_pass"], r["n_keep"])
        assert (r["n_pass"], r["n_keep"]) == ref, (seg, r["n_pass"], r["n_keep"], ref)
pipe.set_option("seg_cols", 0)
ks = list(pass_us[segs[0]][0].keys())
print(f"{args.config}: n_pass {ref[0]}, n_keep {ref[1]}; per pass: median over {args.rounds} rounds (min-max), us")
print("seg_cols " + " ".join(f"{'k=' + str(k):>17s}" for k in ks) + "   ms/step (events off)")
for seg in segs:
    cells = []
    for k in ks:
        v = [rd[k] for rd in pass_us[seg]]
        cells.append(f"{statistics.median(v):6.1f} ({min(v):4.1f}-{max(v):4.1f})")
    print(f"{seg:8d} " + " ".join(f"{c:>17s}" for c in cells) + "   " + " ".join(f"{x:.4f}" for x in step_ms[seg]), flush=True)
