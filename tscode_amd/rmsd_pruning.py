"""Drop-in mirror of tscode/rmsd_pruning.py on the MI355X engine.

Same names, arguments and return values as the reference; the arithmetic runs in
libtscode_hip (hand-written gfx950 kernels) through the C ABI.  No CPU fallback.
"""

from __future__ import annotations

import numpy as np

from .engine import check_team_max_n, get_engine, pack_heavy_batch  # noqa: F401  (pack_heavy_batch: the arrays tsc_prune_rmsd_batch takes)
from .segments import one_or_each, scalar_or_each

__all__ = ["prune_conformers_rmsd", "prune_conformers_rmsd_batch", "rmsd_and_max_numba", "_rmsd_similarity", "last_prune_stats",
           "last_prune_batch_stats", "pack_heavy_batch"]

_last_stats = []
_last_batch_stats = []


def last_prune_stats():
    """Per-pass statistics (k, active before/after, pair evaluations ...) of the latest prune call."""
    return list(_last_stats)


def prune_conformers_rmsd(structures, atomnos, rmsd_thr=0.5, mode=0, **_ignored):
    """tscode/rmsd_pruning.py:164-206.  Returns (structures[mask], mask).

    ``mode=0`` reproduces the reference bit for bit, including its pair-cache behaviour
    (SURVEY.md F5); ``mode=1`` is the cache-free variant.  Extra keyword arguments are accepted
    and ignored: tscode/atropisomer_module.py:499 passes ``verbose=False``.
    """
    global _last_stats
    structures = np.asarray(structures)
    atomnos = np.asarray(atomnos)
    if structures.ndim != 3 or structures.shape[1] != atomnos.shape[0]:
        raise ValueError("structures must be (N, n_atoms, 3) with len(atomnos) == n_atoms")
    n = structures.shape[0]
    if n == 0:
        return structures[:0], np.zeros(0, dtype=bool)
    heavy_idx = np.flatnonzero(atomnos != 1)                                        # :178
    if len(heavy_idx) == 0:
        raise ZeroDivisionError("no non-hydrogen atoms: the reference divides by zero (rmsd_pruning.py:35)")
    if structures.dtype == np.float64 and structures.flags.c_contiguous and n >= 2048:
        # the gather structures[:, heavy] (:179) on the device: as a strided host copy it is most of a large call's time
        mask, _last_stats = get_engine().prune_structures(structures, heavy_idx, float(rmsd_thr), int(mode))
    else:
        heavy = np.ascontiguousarray(structures[:, heavy_idx], dtype=np.float64)    # :179
        mask, _last_stats = get_engine().prune_heavy(heavy, float(rmsd_thr), int(mode))
    if n > 1 and _last_stats and _last_stats[0].get("nonfinite_input"):
        # the reference's np.linalg.svd (rmsd_pruning.py:19) raises on such a structure as soon as a pair with it is evaluated; the
        # library itself defines the verdict (similar to nothing, kept) and only reports that it met one
        raise np.linalg.LinAlgError("Array must not contain infs or NaNs")
    return structures[mask], mask                                                   # :206


def last_prune_batch_stats():
    """Per ensemble, the per-pass statistics (k, active before/after, pair evaluations, new keys) of the latest batch call."""
    return [list(passes) for passes in _last_batch_stats]


def _check_batch(ensembles, atomnos, rmsd_thr):
    """The arguments of prune_conformers_rmsd_batch as (structures, heavy indices, thresholds) per ensemble; raises before anything
    is uploaded."""
    ensembles = [np.asarray(e) for e in ensembles]       # (no ensemble_list: the shapes are checked below, together with atomnos)
    S = len(ensembles)
    atomnos = [np.asarray(a) for a in one_or_each(atomnos, S, "atomnos arrays", 1, exact=True, object_rows=True)]
    thr = scalar_or_each(rmsd_thr, S, "thresholds")
    heavy_idx = []
    for s, (e, a) in enumerate(zip(ensembles, atomnos)):
        if e.ndim != 3 or e.shape[2] != 3 or a.ndim != 1 or e.shape[1] != a.shape[0]:
            raise ValueError(f"ensemble {s}: structures must be (N, n_atoms, 3) with len(atomnos) == n_atoms, got {e.shape} and {a.shape}")
        heavy_idx.append(np.flatnonzero(a != 1))                                     # :178
    for s, idx in enumerate(heavy_idx):
        if len(idx) == 0:
            raise ZeroDivisionError(f"ensemble {s}: no non-hydrogen atoms: the reference divides by zero (rmsd_pruning.py:35)")
    return ensembles, heavy_idx, thr


def prune_conformers_rmsd_batch(ensembles, atomnos, rmsd_thr=0.5, mode=0, team_max_n=None):
    """tscode/rmsd_pruning.py:164-206 on many ensembles at once: [prune_conformers_rmsd(e, a, thr, mode) for every ensemble], by three
    routes (Engine.prune_heavy_batch): one launch for the ensembles of at most "prune_batch_max_n" structures, a workgroup each; one
    call for the longer ones of at most ``team_max_n`` structures, a team of workgroups each; a call of its own for every still
    longer one.  The results do not depend on the route.

    ``ensembles``: a sequence of (N_s, n_s, 3) arrays; ``atomnos``: one array shared by all, or a list with one per ensemble;
    ``rmsd_thr``: a scalar or one per ensemble; ``team_max_n``: None for engine.PRUNE_TEAM_MAX_N, 0 for no team route, at most
    TSC_PRUNE_TEAM_MAX_N.  Returns the list of (structures_s[mask_s], mask_s)."""
    global _last_batch_stats
    team_max_n = check_team_max_n(team_max_n)
    ensembles, heavy_idx, thr = _check_batch(ensembles, atomnos, rmsd_thr)
    if not ensembles:
        _last_batch_stats = []
        return []
    heavies = [np.ascontiguousarray(e[:, idx], dtype=np.float64) for e, idx in zip(ensembles, heavy_idx)]    # :179
    masks, _last_batch_stats, nonfinite = get_engine().prune_heavy_batch(heavies, thr, int(mode), team_max_n=team_max_n)
    for s, e in enumerate(ensembles):
        if nonfinite[s] and len(e) > 1:
            # (as prune_conformers_rmsd: the reference's np.linalg.svd raises on such a structure, rmsd_pruning.py:19)
            raise np.linalg.LinAlgError(f"ensemble {s}: Array must not contain infs or NaNs")
    return [(e[m], m) for e, m in zip(ensembles, masks)]                            # :206


def rmsd_and_max_numba(p, q):
    """tscode/rmsd_pruning.py:6-41: (rmsd, max deviation) after the optimal rotation of p onto q, no centring."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if p.shape != q.shape or p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("p and q must both be (n, 3)")
    r, m = get_engine().rmsd_pairs(np.stack([p, q]), np.array([[0, 1]], dtype=np.int32))
    return float(r[0]), float(m[0])


def _rmsd_similarity(ref, structures, rmsd_thr=0.5):
    """tscode/rmsd_pruning.py:208-224: True if ref is similar to any of structures (all atoms, no cache)."""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    if len(structures) == 0:
        return False
    stack = np.concatenate([ref[None], np.ascontiguousarray(structures, dtype=np.float64).reshape(-1, *ref.shape)])
    pairs = np.stack([np.zeros(len(stack) - 1, dtype=np.int32), np.arange(1, len(stack), dtype=np.int32)], axis=1)
    r, m = get_engine().rmsd_pairs(stack, pairs)
    return bool(np.any((r < rmsd_thr) & (m < 2 * rmsd_thr)))
