"""Times of the diverse-conformer selection (csrc/diverse.hpp) on one MI355X, by HIP events inside the library (context option
"pass_timing" = 1, read back through tsc_diverse_timings): the alignment, ONE k_kmeans_assign launch (the kernel alone: the centres'
norms and the counter reset in front of it are outside the events), ONE k_kmeans_update launch and the whole device part of
tsc_diverse_select, with algorithmic flops (2 N k D per assignment) and bytes; beside them the same Lloyd iteration on the host -- scikit-learn's KMeans(init=..., n_init=1) on 16 threads where it imports, else a NumPy restatement, labelled as which.

    python tools/diverse_profile.py [--out profiles/diverse_profile.json] [--reps 3] [--no-host]

Cases: 20 000 x 50 atoms (make_ensemble(20000, (25, 25), seed=2020, children=10), the scale case of tests/test_diverse.py) and
20 000 x 100 atoms ((50, 50)), k = 100 from np.random.default_rng(2020).choice(N, 100, replace=False).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tscode_amd  # noqa: E402
from tscode_amd import _lib  # noqa: E402
from tscode_amd.synthetic import make_ensemble  # noqa: E402


def moved(x, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(len(x), 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    rot = np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                    [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                    [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]]).transpose(2, 0, 1)
    cen = x.mean(axis=1, keepdims=True)
    return np.ascontiguousarray(np.einsum("nij,naj->nai", rot, x - cen) + cen + rng.uniform(-5, 5, size=(len(x), 1, 3)))


def host_lloyd(X, init):
    """(label of the method, seconds, n_iter, labels)"""
    try:
        from sklearn.cluster import KMeans
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=16):
            t = time.perf_counter()
            km = KMeans(n_clusters=len(init), init=init, n_init=1, algorithm="lloyd").fit(X)
            return "scikit-learn KMeans(init=..., n_init=1), 16 threads", time.perf_counter() - t, int(km.n_iter_), km.labels_
    except ImportError:
        pass
    t = time.perf_counter()
    mean = X.mean(0)
    Xc, Cc = X - mean, init - mean
    tol_abs = np.mean(np.var(Xc, axis=0)) * 1e-4
    xn, old = (Xc * Xc).sum(1), None
    for it in range(300):
        labels = (xn[:, None] - 2.0 * (Xc @ Cc.T) + (Cc * Cc).sum(1)[None, :]).argmin(1)
        onehot = np.zeros((len(Cc), len(Xc)))
        onehot[labels, np.arange(len(Xc))] = 1.0
        counts = onehot.sum(1)
        new = np.where(counts[:, None] > 0, (onehot @ Xc) / np.maximum(counts, 1)[:, None], Cc)     # (no empty cluster on these inputs)
        shift = ((new - Cc) ** 2).sum()
        Cc = new
        if old is not None and np.array_equal(labels, old) or shift <= tol_abs:
            break
        old = labels
    return "NumPy restatement (matmul form; scikit-learn does not import here)", time.perf_counter() - t, it + 1, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "diverse_profile.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    eng = tscode_amd.get_engine(0)
    result = {"build_digest": eng.lib.tsc_build_digest().decode(), "assign_form": "v_mfma_f64_16x16x4_f64, 64 rows x 16 NT centres per workgroup", "cases": []}
    for atoms in ((25, 25), (50, 50)):
        s = moved(make_ensemble(20000, atoms, seed=2020, children=10).poses(), 2020)
        N, n = s.shape[:2]
        D, k = 3 * n, 100
        rows = np.random.default_rng(2020).choice(N, k, replace=False).astype(np.int32)
        tscode_amd.diverse_select(s, k, init_rows=rows)                       # warm-up: allocations, code objects
        best = None
        with eng.options(pass_timing=1):
            for _ in range(args.reps):
                t = time.perf_counter()
                aligned, labels, picked, _, n_iter = tscode_amd.diverse_select(s, k, init_rows=rows)
                wall = time.perf_counter() - t
                ms = (C.c_float * 4)()
                _lib.check(eng.lib.tsc_diverse_timings(eng._h, ms))
                got = dict(align_ms=ms[0], assign_ms=ms[1], update_ms=ms[2], select_device_ms=ms[3], select_wall_ms=1e3 * wall)
                best = got if best is None else {f: min(best[f], got[f]) for f in got}
        t = time.perf_counter()
        tscode_amd.diverse_select(s, k, init_rows=rows)
        untimed_wall = time.perf_counter() - t
        flops = 2.0 * N * k * D
        case = dict(N=N, n_atoms=n, D=D, k=k, n_iter=n_iter, **best, select_wall_untimed_ms=1e3 * untimed_wall,
                    assign_flops=flops, assign_tflops=flops / (best["assign_ms"] * 1e-3) / 1e12,
                    assign_bytes=8.0 * (N * D + k * D + 2 * N), update_bytes=8.0 * (N * D + 2 * k * D),
                    update_gbs=8.0 * (N * D + 2 * k * D) / (best["update_ms"] * 1e-3) / 1e9,
                    align_bytes=8.0 * 2 * N * D, align_gbs=8.0 * 2 * N * D / (best["align_ms"] * 1e-3) / 1e9)
        if not args.no_host:
            X = aligned.reshape(N, D)
            what, sec, host_iter, host_labels = host_lloyd(X, X[rows])
            case.update(host=what, host_lloyd_ms=1e3 * sec, host_n_iter=host_iter, host_labels_equal=bool(np.array_equal(host_labels, labels)))
        result["cases"].append(case)
        print(json.dumps(case))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
