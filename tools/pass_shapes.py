"""Small prunes that between them take every branch of the pass launcher (csrc/prune.hip: pass_launch; csrc/pass_plan.hpp), to be run
under a kernel trace of one build and of another, and the comparison of the two traces.

    rocprofv3 --kernel-trace --output-format csv -d OUT_A -- python tools/pass_shapes.py       (TSCODE_AMD_LIB selects the build)
    python tools/pass_shapes.py --compare OUT_A OUT_B

The runs, on one context: 9 000 structures with cull = 2 and cull_min_pairs = 5e6 (chunk-local passes at k = 200, 100, 50, walked at 20 and
10, culled at 5, 2, 1) with the 16-row matrix-core kernel, the 64-row ones (sieve_mm = 2), the packed-fp32 ones (sieve_mm = sieve_mm16 = 0)
and the register-tiled kernel (prune_algo = 1); passes partitioned over 5 emulated ranks on 700 structures; culled passes dealt by row tiles
to 5 emulated ranks (cull_tile_block = 16, both kernel forms); every pass dealt to 3 ranks by one run (tsc_prune_pass_local for rank 0,
tsc_prune_pass_rows for the others).  Prints one line per run with the digest of its mask.  --compare: the ordered lists of (kernel,
grid, workgroup, LDS bytes) of the project's kernels in the two traces; exit status 1 where they differ."""

import argparse
import csv
import glob
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def dispatches(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"{out_dir}: {len(files)} kernel traces")
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    ours = re.compile(r"(^|[\s:\d])k_[a-z]")       # the library's kernels (k_open_rows, void tsc::k_rmsd_sieve<...>, mangled: _ZN3tsc15k_rmsd_...), not torch's
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["LDS_Block_Size"]))
            for r in rows if ours.search(r["Kernel_Name"])]


def compare(a_dir, b_dir):
    a, b = dispatches(a_dir), dispatches(b_dir)
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            print(f"dispatch {i} differs:\n  {x}\n  {y}")
            return 1
    if len(a) != len(b):
        print(f"{len(a)} dispatches against {len(b)}")
        return 1
    print(f"{len(a)} dispatches of {len(set(x[0] for x in a))} kernels: same kernel, grid, workgroup size and LDS bytes, in the same order")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))

    import numpy as np
    import torch

    import tscode_amd
    from tscode_amd.engine import PruneStepper
    from tscode_amd.synthetic import make_config

    eng = tscode_amd.get_engine(0)
    dev = torch.device("cuda:0")

    def heavy_of(n):
        ens = make_config("C2", n)
        return np.ascontiguousarray(ens.poses()[:, ens.atomnos != 1])

    def report(name, mask):
        print(f"{name}: {int(mask.sum())} kept, digest {hashlib.sha256(np.packbits(mask.astype(bool)).tobytes()).hexdigest()[:16]}", flush=True)

    def with_options(opts, f):
        with eng.options(**opts):
            return f()

    def mask_of(st, n):
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        st.copy_mask(keep)
        eng.synchronize()
        return keep.cpu().numpy()

    heavy = heavy_of(9_000)
    n, h = heavy.shape[0], heavy.shape[1]
    cull = {"cull": 2, "cull_min_pairs": 5e6}
    for name, opts in [("16-row matrix-core", {}), ("64-row matrix-core", {"sieve_mm": 2}), ("packed fp32", {"sieve_mm": 0, "sieve_mm16": 0}),
                       ("register-tiled", {"prune_algo": 1})]:
        report(name, with_options({**cull, **opts}, lambda: eng.prune_heavy(heavy, 0.5, 0)[0]))

    def partitioned(world, min_chunks, heavy):
        n, h = heavy.shape[0], heavy.shape[1]
        d_heavy = torch.from_numpy(heavy).to(dev)
        words = PruneStepper.exchange_words(eng.lib, n, 0)
        sts, exch = [], []
        for r in range(world):
            sts.append(eng.prune_stepper(d_heavy, n, h, 0.5, 0))
            exch.append(torch.zeros(words, dtype=torch.int64, device=dev))
            sts[-1].set_partition(r, world, min_chunks, exch[-1])

        def all_reduce(lo, hi):
            eng.synchronize()
            total = torch.stack([e[lo:hi] for e in exch]).sum(0)
            for e in exch:
                e[lo:hi].copy_(total)
            torch.cuda.synchronize()

        while True:
            k = {st.next_pass() for st in sts}.pop()
            if k == 0:
                break
            if k >= min_chunks * world:
                for st in sts:
                    st.pass_range()
                all_reduce(0, n // 64 + 48)
                for st in sts:
                    st.pass_merge()
                continue
            off, w = sts[0].views_range()
            if w:
                all_reduce(off, off + w)
            for st in sts:
                st.views_merged()
                st.pass_local(0, 1)
                st.pass_finish()
        m = mask_of(sts[0], n)
        for st in sts:
            st.close()
        return m

    report("partitioned over 5 ranks", partitioned(5, 2, heavy_of(700)))

    def tiles_to_ranks(world):
        d_heavy = torch.from_numpy(heavy).to(dev)
        sts = [eng.prune_stepper(d_heavy, n, h, 0.5, 0) for _ in range(world)]
        bests = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(world)]
        for s, b in zip(sts, bests):
            s.use_best_buffer(b)
        while {s.next_pass() for s in sts}.pop() != 0:
            for r, s in enumerate(sts):
                s.pass_local(r, world)
            eng.synchronize()
            merged = torch.stack(bests).amin(0)
            for b in bests:
                b.copy_(merged)
            torch.cuda.synchronize()
            for s in sts:
                s.pass_finish()
        m = mask_of(sts[0], n)
        for s in sts:
            s.close()
        return m

    for mm in (1, 2):
        report(f"culled row tiles to 5 ranks, sieve_mm {mm}",
               with_options({"cull": 2, "cull_min_pairs": 0, "local_pass": 0, "cull_tile_block": 16, "deterministic_basis": 1, "sieve_mm": mm}, lambda: tiles_to_ranks(5)))

    def rows_of_other_ranks():
        d_heavy = torch.from_numpy(heavy).to(dev)
        s = eng.prune_stepper(d_heavy, n, h, 0.5, 0)
        while s.next_pass() != 0:
            s.pass_local(0, 3)
            s.pass_rows(1, 3)
            s.pass_rows(2, 3)
            s.pass_finish()
        m = mask_of(s, n)
        s.close()
        return m

    report("3 ranks' row tiles by one run", rows_of_other_ranks())


if __name__ == "__main__":
    main()
