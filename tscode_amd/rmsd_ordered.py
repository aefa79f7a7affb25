"""Energy-ordered RMSD prune: one representative per cluster, the first in the order, every cluster collapsed (csrc/leader.hpp).

The rule is the greedy filter of the reference's embed loops (tscode/embeds.py:715, :843), for a whole ensemble:

    order = 0 .. N-1, or np.argsort(energies, kind="stable")
    kept  = the library's rows, in index order            # optional; never removed
    for s in order:
        for k in kept:                                    # library rows first, then this call's kept rows in the order they were kept
            rmsd, maxdev = rmsd_and_max_numba(X[s][compared], k[compared])      # rmsd_pruning.py:6-41: s turned onto k, no centring
            if rmsd < thr and maxdev < 2 * thr:           # :75, :208-224
                s is removed, represented by k; break
        else:
            s is kept

A removed row never covers anything.  ``prune_conformers_rmsd`` is a different rule: it keeps the LAST member of a duplicate cluster, works
chunk by chunk and reproduces the reference's pair cache, which leaves clusters uncollapsed -- bit for bit what the
reference does, and so what is installed over it.  This one changes results by design and has no install() entry; the three places where
TSCoDe sorts by energy and then prunes (embedder.py:1542-1564, :1785, :2037) are where a maintainer would call it.

``atomnos`` given: only the atoms with ``atomnos != 1`` are compared (:178-179); ``None``: all atoms.  ``center=True`` subtracts from every
structure, library included, the mean of its compared atoms first.  The caller's arrays are never modified; a coordinate that is not finite
or a NaN energy is a ValueError, raised before anything is uploaded.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .engine import get_engine
from .rmsd_cross import _check

__all__ = ["prune_conformers_rmsd_ordered", "leader_clusters", "LEADER_BLOCK"]



def __getattr__(name):
    """LEADER_BLOCK: rows of the order decided per round, read from the library (tsc_leader_block: csrc/leader_plan.hpp); no GPU is touched"""
    if name == "LEADER_BLOCK":
        from . import _lib
        return int(_lib.load().tsc_leader_block())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _order(energies, n):
    """i32[n] the stable ascending order of ``energies``, or None (the rows as they lie)"""
    if energies is None:
        return None
    e = np.asarray(energies, dtype=np.float64)
    if e.shape != (n,):
        raise ValueError(f"energies must be ({n},), got {e.shape}")
    if np.isnan(e).any():
        raise ValueError("energies: NaN has no place in an order")
    return np.argsort(e, kind="stable").astype(np.int32)


def leader_clusters(structures, atomnos=None, rmsd_thr=0.5, energies=None, library=None, center=False):
    """The rule above as a namespace of

        mask                bool[N]   kept
        rep                 i32[N]    a kept row: itself; a removed row: the kept row of this call that the rule stopped at; -1 where a
                                      library row covered it
        library_rep         i32[N]    that library row, else -1
        population          i64[N]    rows each kept row stands for, itself included; 0 on removed rows
        library_population  i64[n_library]   rows of this call each library row covers

    so that population.sum() + library_population.sum() == N.  ``rep`` is the LEADER the sequential rule stops at -- the first kept
    structure in the order that is similar -- not the nearest kept structure; ``assign_to_kept`` gives the nearest."""
    structures, library, idx = _check(structures, library, atomnos)
    n, n_l = len(structures), 0 if library is None else len(library)
    if n + n_l > np.iinfo(np.int32).max:
        raise ValueError(f"{n} structures and {n_l} library structures: at most 2^31 - 1 together")
    order = _order(energies, n)
    thr = float(rmsd_thr)
    if not np.isfinite(thr):
        raise ValueError("rmsd_thr is not finite")
    if n == 0:
        mask, rep, lib_rep = np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    else:
        mask, rep, lib_rep, n_kept = get_engine().prune_rmsd_ordered(structures, library if n_l else None, idx, order, thr, center)
        mask = mask.astype(bool)
        assert n_kept == int(mask.sum())
    population = np.bincount(rep[rep >= 0], minlength=n).astype(np.int64)
    library_population = np.bincount(lib_rep[lib_rep >= 0], minlength=n_l).astype(np.int64)
    return SimpleNamespace(mask=mask, rep=rep, library_rep=lib_rep, population=population, library_population=library_population)


def prune_conformers_rmsd_ordered(structures, atomnos, rmsd_thr=0.5, energies=None, library=None, center=False):
    """(structures[mask], mask) of the rule above, in the caller's row order, as prune_conformers_rmsd returns it: with ``energies`` the
    lowest-energy member of every cluster survives (ties: the lowest index), without them the first."""
    mask = leader_clusters(structures, atomnos, rmsd_thr, energies, library, center).mask
    return np.asarray(structures)[mask], mask
