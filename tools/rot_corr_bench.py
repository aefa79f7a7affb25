"""Time of prune_rmsd_rot_corr_arrays (the symmetry-corrected prune, tscode_amd.rot_corr) on the MI355X: HIP events around the
whole call (upload, every pass, the host graph steps, download) for G19's N = 400 case and for a 1 500-structure ensemble of 150
clusters (tscode_amd.synthetic.make_rot_corr_ensemble, max_structures=None), next to the reference's wall time that G19 recorded
for its case on the CPU.  Prints one JSON line.

    python tools/rot_corr_bench.py [--repeat R]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tscode_amd  # noqa: E402
from tscode_amd.synthetic import make_rot_corr_ensemble  # noqa: E402
from test_rot_corr import case, g19  # noqa: E402


def timed(fn, repeat):
    eng = tscode_amd.get_engine()
    fn()                                      # warm-up: module load, first launch
    ms = []
    for _ in range(repeat):
        eng.timer_begin()
        fn()
        ms.append(eng.timer_end())
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    meta, data = g19()
    out = {}
    c = case("n400")
    run = lambda: tscode_amd.prune_rmsd_rot_corr_arrays(c.structures, c.atomnos, **c.setup, max_rmsd=c.meta["max_rmsd"])  # noqa: E731
    med, best = timed(run, args.repeat)
    out["n400"] = {"ms_median": med, "ms_min": best, "pairs": int(c.passes[:, 1].sum()), "torsions": c.meta["n_torsions"],
                   "reference_cpu_s": c.meta["reference_wall_s"]}
    s = {k: v[:1] for k, v in case("n160a").setup.items()}         # the ensemble of test_uncapped_clustered_ensemble
    S, _ = make_rot_corr_ensemble(data["molA_coords"], s["torsions"], s["angles"], s["move_masks"], 150, 10, seed=1500)
    run = lambda: tscode_amd.prune_rmsd_rot_corr_arrays(S, data["molA_atomnos"], **s, max_rmsd=0.25, max_structures=None)  # noqa: E731
    med, best = timed(run, args.repeat)
    st = tscode_amd.last_rot_corr_stats()
    out["n1500_150clusters"] = {"ms_median": med, "ms_min": best, "pairs": int(sum(x["pairs_evaluated"] for x in st)),
                                "torsions": len(s["torsions"]),
                                "passes": [[x["k"], x["n_active"], x["pairs_evaluated"]] for x in st if x["ran"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
