"""Cross-set RMSD: a batch of structures held against a library of structures (csrc/cross.hpp).

Every pair (query, library member) is the reference's ``rmsd_and_max_numba(query, member)`` (tscode/rmsd_pruning.py:6-41: optimal proper
rotation of the query onto the member, no centring) and "similar" is its ``rmsd < thr and maxdev < 2 * thr`` (:75, :208-224).  The
reference itself has no such call -- it only ever compares inside one set -- so nothing here is installed over it (no install() entry).

``atomnos`` given: only the atoms with ``atomnos != 1`` are compared (:178-179); ``None``: all atoms, as the embeds call
``_rmsd_similarity``.  ``center=True`` subtracts from every structure, queries and library alike, the mean of its compared atoms before
any pair is formed: structures from different runs share no frame and the reference's metric counts translation as deviation
(SURVEY.md F2).  The caller's arrays are never modified.  A coordinate that is not finite is a ValueError, raised before anything is uploaded.
"""

from __future__ import annotations

import numpy as np

from .engine import get_engine

__all__ = ["rmsd_matrix", "rmsd_similarity_mask", "nearest_structures", "prune_conformers_rmsd_against", "assign_to_kept", "CROSS_MATRIX_BYTES"]

CROSS_MATRIX_BYTES = 1 << 30     # device bytes of the two outputs of one rmsd_matrix launch; larger matrices are walked in row blocks
_INT32_MAX = np.iinfo(np.int32).max


def _structures(a, name):
    a = np.asarray(a)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{name} must be (N, n_atoms, 3), got {a.shape}")
    if a.shape[0] > _INT32_MAX:
        raise ValueError(f"{name}: {a.shape[0]} structures, at most 2^31 - 1")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: a coordinate is not finite")
    return a


def _check(queries, library, atomnos):
    """(queries, library or None, compared-atom indices or None) as the engine takes them; raises before the engine is touched."""
    queries = _structures(queries, "queries")
    if library is not None:
        library = _structures(library, "library")
        if library.shape[1] != queries.shape[1]:
            raise ValueError(f"queries have {queries.shape[1]} atoms, library has {library.shape[1]}")
    if queries.shape[1] == 0:
        raise ZeroDivisionError("no atoms: the reference divides by zero (rmsd_pruning.py:35)")
    idx = None
    if atomnos is not None:
        atomnos = np.asarray(atomnos)
        if atomnos.ndim != 1 or len(atomnos) != queries.shape[1]:
            raise ValueError(f"atomnos must be ({queries.shape[1]},), got {atomnos.shape}")
        idx = np.flatnonzero(atomnos != 1).astype(np.int32)                          # :178
        if len(idx) == 0:
            raise ZeroDivisionError("no non-hydrogen atoms: the reference divides by zero (rmsd_pruning.py:35)")
    return queries, library, idx


def rmsd_matrix(queries, library=None, atomnos=None, center=False):
    """(rmsd, maxdev), two f64[Nq, Nl] arrays: rmsd_and_max_numba(queries[q], library[l]) (rmsd_pruning.py:6-41) for every pair.
    ``library=None``: the queries against themselves, the full square with its diagonal.  The queries are walked in row blocks so that the
    device never holds more than CROSS_MATRIX_BYTES of output; the result does not depend on that constant."""
    queries, library, idx = _check(queries, library, atomnos)
    n_q, n_l = len(queries), len(queries) if library is None else len(library)
    if n_q == 0 or n_l == 0:
        return np.empty((n_q, n_l)), np.empty((n_q, n_l))
    eng = get_engine()
    rows = eng.rmsd_cross_rows(n_l, int(CROSS_MATRIX_BYTES))
    if rows >= n_q:
        return eng.rmsd_cross(queries, library, idx, center)
    lib = queries if library is None else library
    r, m = np.empty((n_q, n_l)), np.empty((n_q, n_l))
    for lo in range(0, n_q, rows):
        r[lo:lo + rows], m[lo:lo + rows] = eng.rmsd_cross(queries[lo:lo + rows], lib, idx, center)
    return r, m


def rmsd_similarity_mask(queries, library, atomnos=None, rmsd_thr=0.5, center=False):
    """(similar bool[Nq], first i32[Nq]): whether a query is similar (rmsd_pruning.py:75: rmsd < thr and maxdev < 2 thr) to any library
    member, and the lowest index of such a member or -1.  With ``atomnos=None``, similar[q] is
    ``_rmsd_similarity(queries[q], library, rmsd_thr)`` (:208-224)."""
    if library is None:
        raise ValueError("rmsd_similarity_mask: no library")
    queries, library, idx = _check(queries, library, atomnos)
    if len(queries) == 0 or len(library) == 0:
        return np.zeros(len(queries), dtype=bool), np.full(len(queries), -1, dtype=np.int32)
    first = get_engine().rmsd_cross_first(queries, library, idx, float(rmsd_thr), center)
    similar = first != _INT32_MAX
    first[~similar] = -1
    return similar, first


def nearest_structures(queries, library, atomnos=None, center=False):
    """(index i32[Nq], rmsd f64[Nq], maxdev f64[Nq]): the library member of the smallest rmsd_and_max_numba(query, member) rmsd for every
    query (ties: the lowest index) and the two values there.  An empty library is a ValueError.  Two calls return identical bits."""
    if library is None:
        raise ValueError("nearest_structures: no library")
    queries, library, idx = _check(queries, library, atomnos)
    if len(library) == 0:
        raise ValueError("nearest_structures: the library is empty")
    if len(queries) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0)
    return get_engine().rmsd_cross_nearest(queries, library, idx, center)


def prune_conformers_rmsd_against(new, library, atomnos, rmsd_thr=0.5, center=False):
    """(new[mask], mask): the new structures that no library member already covers, mask = ~similar of rmsd_similarity_mask.  The library is
    never altered.
    Unlike prune_conformers_rmsd on the concatenation, which keeps the LAST member of a duplicate cluster, works chunk by chunk and
    reproduces the reference's pair cache -- and so drops library members for new ones, or keeps both."""
    similar, _first = rmsd_similarity_mask(new, library, atomnos, rmsd_thr, center)
    mask = ~similar
    return np.asarray(new)[mask], mask


def assign_to_kept(structures, mask, atomnos=None, center=False):
    """(rep i32[N], population i64[N]) for the ``mask`` a prune returned on ``structures``: rep indexes the ORIGINAL array -- a kept
    structure represents itself, a removed one is represented by the kept structure NEAREST to it (nearest_structures of removed against
    kept; not necessarily the structure whose comparison removed it in the reference's schedule).  population counts, per kept structure,
    what it represents, itself included, and is 0 on removed rows: population.sum() == N."""
    structures = np.asarray(structures)
    mask = np.asarray(mask)
    if structures.ndim != 3 or structures.shape[2] != 3:
        raise ValueError(f"structures must be (N, n_atoms, 3), got {structures.shape}")
    if mask.dtype != bool or mask.shape != (structures.shape[0],):
        raise ValueError(f"mask must be bool ({structures.shape[0]},), got {mask.dtype} {mask.shape}")
    n = len(structures)
    kept, removed = np.flatnonzero(mask), np.flatnonzero(~mask)
    rep = np.arange(n, dtype=np.int32)
    if len(removed):
        if len(kept) == 0:
            raise ValueError("assign_to_kept: structures were removed and none kept")
        index, _r, _m = nearest_structures(structures[removed], structures[kept], atomnos, center)
        rep[removed] = kept[index]
    else:
        _check(structures, None, atomnos)
    population = np.bincount(rep, minlength=n).astype(np.int64)
    return rep, population
