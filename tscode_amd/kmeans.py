"""Lloyd's k-means and k-means++ seeding on the MI355X engine (csrc/diverse.hpp): what scikit-learn's KMeans computes for
tscode/torsion_module.py:889-890, restated in include/tscode_hip.h (tsc_kmeans_lloyd, tsc_kmeans_seed)."""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, ptr
from .engine import get_engine

__all__ = ["kmeans_lloyd", "kmeans_plusplus_rows"]

MAX_K, MAX_D = 300, 3 * 512          # csrc/diverse.hpp: DV_MAX_K, 3 * DV_MAX_ATOMS


def _check_k(N, D, k):
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{k} clusters: the engine takes 1 .. {MAX_K}")
    if k > N:
        raise ValueError(f"{k} clusters for {N} rows")
    if not 1 <= D <= MAX_D:
        raise ValueError(f"{D} columns: the engine takes 1 .. {MAX_D} ({MAX_D // 3} atoms)")


def _features(X):
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or len(X) == 0:
        raise ValueError(f"X of shape {X.shape}: expected (n_rows >= 1, n_columns)")
    if not np.isfinite(X).all():
        raise ValueError("X contains NaN or infinity")           # (as scikit-learn refuses it)
    return X


def kmeans_lloyd(X, init, max_iter=300, tol=1e-4):
    """KMeans(n_clusters=len(init), init=init, n_init=1, algorithm="lloyd", max_iter=max_iter, tol=tol).fit(X) of scikit-learn:
    returns (labels i32[N], centers f64[k, D], inertia, n_iter).  Ties go to the lowest centre; an empty cluster takes the row
    farthest from its own centre."""
    X = _features(X)
    init = np.ascontiguousarray(init, dtype=np.float64)
    if init.ndim != 2 or init.shape[1] != X.shape[1]:
        raise ValueError(f"init of shape {init.shape} for X of shape {X.shape}: expected (k, {X.shape[1]})")
    N, D = X.shape
    k = len(init)
    _check_k(N, D, k)
    if not np.isfinite(init).all():
        raise ValueError("init contains NaN or infinity")
    if max_iter < 1 or not np.isfinite(tol) or tol < 0:
        raise ValueError(f"max_iter = {max_iter}, tol = {tol}")
    labels = np.empty(N, dtype=np.int32)
    centers = np.empty((k, D), dtype=np.float64)
    inertia, n_iter, max_empty = C.c_double(), C.c_int(), C.c_int()
    eng = get_engine()
    check(eng.lib.tsc_kmeans_lloyd(eng._h, ptr(X), C.c_int64(N), C.c_int64(D), ptr(init), C.c_int(k), C.c_int(int(max_iter)), C.c_double(float(tol)),
                                   ptr(labels), ptr(centers), C.byref(inertia), C.byref(n_iter), C.byref(max_empty)))
    return labels, centers, inertia.value, n_iter.value


def seed_uniforms(k, seed):
    """The k uniforms in [0, 1) that choose the seeds: np.random.default_rng(seed).random(k)."""
    return np.ascontiguousarray(np.random.default_rng(seed).random(k), dtype=np.float64)


def kmeans_plusplus_rows(X, k, seed):
    """k-means++ seeding without local trials: row floor(u_0 N) first, then k - 1 times the first row whose running sum (row
    order) of the squared distance to the nearest seed so far exceeds u_j * total; u = np.random.default_rng(seed).random(k).
    Returns the k row indices (i32), in the order chosen."""
    X = _features(X)
    k = int(k)
    _check_k(len(X), X.shape[1], k)
    u = seed_uniforms(k, seed)
    rows = np.empty(k, dtype=np.int32)
    eng = get_engine()
    check(eng.lib.tsc_kmeans_seed(eng._h, ptr(X), C.c_int64(len(X)), C.c_int64(X.shape[1]), C.c_int(k), ptr(u), ptr(rows)))
    return rows
