"""The energy-ordered RMSD prune (tscode_amd/rmsd_ordered.py, csrc/leader.hpp) timed beside the only other implementation of its rule.

    python tools/ordered_prune_profile.py [--out profiles/ordered_prune_profile.json] [--repeats 7] [--step-limit 240] [--shrink 1]

    bar       make_ensemble(8192, (25, 25), seed=1001).poses(), all 50 atoms: prune_conformers_rmsd_ordered beside filter_angular_groups on
              the same array as ONE group (one wavefront walks the poses; 8192 is the largest group it takes).  The masks must be equal;
              "holds": the new route's median does not exceed the baseline's median by more than the baseline's own spread (max - min) in
              this run.
    c3        make_ensemble(100000, (25, 25), seed=1003), heavy atoms: the host-array call and the call on device-resident arrays; blocks,
              launches and read-backs from the shapes (csrc/leader_plan.hpp: leader_counts); the kept count; prune_conformers_rmsd mode 0 on
              the same input as context only (another rule, another result).
    all_kept  20 000 random structures of 30 atoms, no two similar: the kept set is the whole input, every row is screened against all
              rows before it -- the worst case for the growing library.

One process.  Every shape is warmed up once, then timed --repeats times with a host clock around the whole call (argument checks, uploads
and the final synchronisation included); the resident call synchronises inside.  Where two routes are compared they alternate.  A step that
passes --step-limit seconds ends the run there: nothing more is started on the device."""

import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THR = 0.5


class StepTimeout(Exception):
    pass


def _alarm(_sig, _frame):
    raise StepTimeout()


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)), "spread": float(max(values) - min(values))}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def counts(n, n_library, ordered, h):
    """leader_counts of csrc/leader_plan.hpp"""
    from tscode_amd.rmsd_ordered import LEADER_BLOCK
    blocks = -(-n // LEADER_BLOCK)
    walks = blocks if n_library else max(blocks - 1, 0)
    launches = int(ordered) + 1 + int(n_library > 0) + 2 + int(h <= 32) + walks + 2 * blocks + max(blocks - 1, 0)
    return {"blocks": blocks, "launches": launches, "readbacks": blocks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordered_prune_profile.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-limit", type=int, default=240, help="seconds a step may take before the run ends")
    ap.add_argument("--shrink", type=int, default=1, help="divide every size by this (trial runs of the tool itself)")
    args = ap.parse_args()

    import torch
    import tscode_amd
    from tscode_amd import build
    from tscode_amd.synthetic import make_ensemble

    eng = tscode_amd.get_engine()
    dev = torch.device("cuda", eng.device)
    signal.signal(signal.SIGALRM, _alarm)
    rows, ended = [], None

    def step(name, fn):
        nonlocal ended
        if ended:
            return
        row = {"step": name}
        signal.alarm(args.step_limit)
        try:
            fn(row)
        except StepTimeout:
            ended = f"step {name} passed {args.step_limit} s: the run ends here"
            row["timed_out"] = True
        finally:
            signal.alarm(0)
        rows.append(row)
        print(json.dumps(row), flush=True)

    def bar(row):
        n = 8192 // args.shrink
        x = np.ascontiguousarray(make_ensemble(n, (25, 25), seed=1001).poses())
        new = lambda: tscode_amd.prune_conformers_rmsd_ordered(x, None, THR)[1]          # noqa: E731
        old = lambda: tscode_amd.filter_angular_groups(x, [n], THR)                      # noqa: E731
        m_new, m_old = new(), old()                                                      # (warm-up)
        row.update(n=n, atoms=int(x.shape[1]), compared="all", kept=int(m_new.sum()), masks_equal=bool(np.array_equal(m_new, m_old)), **counts(n, 0, False, x.shape[1]))
        t_new, t_old = [], []
        for _ in range(args.repeats):                                                    # (the two alternate)
            t_new.append(clock(new)[0])
            t_old.append(clock(old)[0])
        row["ms_ordered"], row["ms_group_filter"] = stats(t_new), stats(t_old)
        row["holds"] = bool(row["masks_equal"] and row["ms_ordered"]["median"] <= row["ms_group_filter"]["median"] + row["ms_group_filter"]["spread"])

    def resident(x, idx):
        n, n_atoms = x.shape[0], x.shape[1]
        d_x = torch.from_numpy(x).to(dev)
        d_idx = None if idx is None else torch.from_numpy(idx).to(dev)
        d_mask = torch.empty(n, dtype=torch.uint8, device=dev)
        d_rep, d_lib = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        call = lambda: eng.prune_rmsd_ordered_dev(d_x, n, None, 0, n_atoms, d_idx, 0 if idx is None else len(idx), False, None, THR, d_mask, d_rep, d_lib)   # noqa: E731
        kept = call()
        times = [clock(call)[0] for _ in range(args.repeats)]
        return stats(times), kept, d_mask.cpu().numpy().astype(bool)

    def c3(row):
        n = 100_000 // args.shrink
        ens = make_ensemble(n, (25, 25), seed=1003)
        x, atomnos = np.ascontiguousarray(ens.poses()), ens.atomnos
        idx = np.flatnonzero(atomnos != 1).astype(np.int32)
        host = lambda: tscode_amd.prune_conformers_rmsd_ordered(x, atomnos, THR)[1]      # noqa: E731
        mask = host()
        row.update(n=n, atoms=int(x.shape[1]), compared=int(len(idx)), kept=int(mask.sum()), **counts(n, 0, False, len(idx)))
        row["ms_host"] = stats([clock(host)[0] for _ in range(args.repeats)])
        row["ms_resident"], kept, mask_dev = resident(x, idx)
        row["resident_equals_host"] = bool(kept == mask.sum() and np.array_equal(mask_dev, mask))
        ref = lambda: tscode_amd.prune_conformers_rmsd(x, atomnos, THR)[1]               # noqa: E731
        m_ref = ref()
        row["context_prune_conformers_rmsd_mode0"] = {"kept": int(m_ref.sum()), "ms_host": stats([clock(ref)[0] for _ in range(max(3, args.repeats // 2))])}

    def all_kept(row):
        n = 20_000 // args.shrink
        x = np.random.default_rng(1005).normal(scale=3.0, size=(n, 30, 3))
        host = lambda: tscode_amd.prune_conformers_rmsd_ordered(x, None, THR)[1]         # noqa: E731
        mask = host()
        row.update(n=n, atoms=30, compared="all", kept=int(mask.sum()), pairs_screened=n * (n - 1) // 2, **counts(n, 0, False, 30))
        row["ms_host"] = stats([clock(host)[0] for _ in range(args.repeats)])
        row["ms_resident"], kept, _ = resident(x, None)
        row["pairs_per_second_resident"] = row["pairs_screened"] / (row["ms_resident"]["median"] * 1e-3)

    step("bar", bar)
    step("c3", c3)
    step("all_kept", all_kept)
    out = {"tool": "tools/ordered_prune_profile.py", "device": torch.cuda.get_device_name(eng.device), "build_digest": eng.lib.tsc_build_digest().decode(),
           "sources_digest": build.csrc_digest(), "repeats": args.repeats, "threshold": THR, "leader_block": eng.lib.tsc_leader_block(), "shrink": args.shrink,
           "ended_early": ended, "steps": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    return 1 if ended else 0


if __name__ == "__main__":
    sys.exit(main())
