"""What the prune's known prefix (csrc/rmsd.hpp: known[], cbeg[]) is worth, pass by pass, modelled on the CPU from the oracle's trace of a run.

    python tools/known_prefix_model.py [CONFIG] [--mode 0|1] [--local-max-chunk L] [--n-poses N]

A row i that survives a pass had every column that was active between it and its stop position (the first active cached column, else its
chunk's end) found dissimilar; a pair's verdict depends on its two structures alone and the mask only shrinks, so a later pass need not look
at the active columns before known[i] = the furthest such stop position again.  Per pass the table counts the pairs inside the rows' ranges
(what a pass walks today: sum of cend - r - 1), the same with each row's known prefix taken out (sum of cend - max(cbeg, r + 1)), and the
ratio.  Pair counts, not times.  --local-max-chunk L: passes whose longest chunk has at most L structures neither read nor raise known[]
(the chunk-local kernel's, csrc/local_pass.hpp); default 0: every pass records its prefix.

model() is what tests/test_known_prefix.py holds tsc_pass_stats.pairs_known against."""
import argparse
import sys

import numpy as np


def model(n, mode, passes, keys, walked=lambda k, longest: True, rows=False):
    """passes: [(k, mask entering the pass as bool[n], new_keys of the pass)] in schedule order, only the passes that ran; keys: i64[*, 2], the
    cache keys (a, b) of the whole run in the order the passes appended them.  walked(k, longest chunk) -> does the pass read and raise known[].
    Returns one dict per pass: k, today, skipped (= today - known), known; rows=True adds, for the walked passes, the rows' cbeg and cend (by rank), their structures (pos) and known[] as the pass found it (known_pos)."""
    known = np.arange(1, n + 1, dtype=np.int64)
    out, k0 = [], 0
    for k, mask, new_keys in passes:
        cache = keys[:k0]
        k0 += int(new_keys)
        cs = n // k
        pos = np.flatnonzero(mask)                      # structure of every row, ascending: row r = its rank
        chunk = np.minimum(pos // cs, k - 1)
        first = chunk * cs
        last = np.where(chunk == k - 1, n, first + cs)  # rmsd_pruning.py:140-144
        found = last.copy()
        if mode == 0 and len(cache):
            starts = cache[:, 0]
            for a in np.unique(starts[(starts % cs == 0) & (starts // cs < k)]):
                rr = np.flatnonzero(first == a)                 # the rows of the chunk that starts at a
                if not len(rr):
                    continue
                d = np.unique(cache[starts == a, 1] - a)      # key (first, first + (j - i)): the row stops at column j = i + d (:65-67)
                d = d[d >= 1]
                j = pos[rr, None] + d[None, :]
                ok = (j < last[rr, None]) & mask[np.minimum(j, n - 1)]
                j = np.where(ok, j, np.iinfo(np.int64).max)
                found[rr] = np.minimum(found[rr], j.min(axis=1))
        r = np.arange(len(pos))
        cend = np.searchsorted(pos, found)              # active structures before the stop position
        today = int(np.maximum(cend - r - 1, 0).sum())
        longest = n - (k - 1) * cs
        if walked(k, longest):
            known_before = known[pos].copy()
            cbeg = np.searchsorted(pos, known_before)   # rank of the first active position >= known[i]; >= r + 1
            left = int(np.maximum(cend - np.maximum(cbeg, r + 1), 0).sum())
            known[pos] = np.maximum(known[pos], found)  # (also for the rows this pass removes: they are never rows again)
        else:
            left = today
        out.append({"k": int(k), "today": today, "skipped": left, "known": today - left})
        if rows and walked(k, longest):
            out[-1]["cbeg"], out[-1]["cend"], out[-1]["pos"], out[-1]["known_pos"] = cbeg, cend, pos, known_before
    return out


def passes_of_trace(ref):
    """(k, mask entering the pass, new_keys) of every pass of an oracle.prune_heavy(..., trace=True) result."""
    n = len(ref["mask"])
    before = np.ones(n, dtype=bool)
    out = []
    for s, after in zip(ref["stats"], ref["pass_masks"]):
        out.append((int(s["k"]), before, int(s["new_keys"])))
        before = after
    return out


def main():
    sys.path.insert(0, ".")
    import oracle
    from tscode_amd.synthetic import make_config
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C3")
    ap.add_argument("--mode", type=int, default=None)
    ap.add_argument("--local-max-chunk", type=int, default=0)
    ap.add_argument("--n-poses", type=int, default=None)
    args = ap.parse_args()
    ens = make_config(args.config, args.n_poses) if args.n_poses else make_config(args.config)
    poses = ens.poses()
    poses = poses[oracle.compenetration_mask(poses, ens.ids, 1.5, 0)]
    heavy = np.ascontiguousarray(poses[:, ens.atomnos != 1])
    n = len(heavy)
    print(f"{args.config}: {n} structures pass the clash check")
    for mode in ([args.mode] if args.mode is not None else [0, 1]):
        ref = oracle.prune_heavy(heavy, 0.5, mode=mode, row_parallel=True, trace=True)
        rows = model(n, mode, passes_of_trace(ref), ref["keys"], lambda k, longest: longest > args.local_max_chunk)
        print(f"mode {mode}\n| pass k | today | with skip | left |\n|---|---|---|---|")
        for row in rows:
            print(f"| {row['k']} | {row['today']:,} | {row['skipped']:,} | {row['skipped'] / max(row['today'], 1):.3g} |".replace(",", " "))


if __name__ == "__main__":
    main()
