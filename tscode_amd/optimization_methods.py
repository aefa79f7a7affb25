"""Drop-in names of the moment-of-inertia pruning and the embed-fitness checks.

Reference: ``tscode/algebra.py:165-213`` (get_inertia_moments, get_moi_similarity_matches, diagonalize),
``tscode/optimization_methods.py:327-358`` (prune_by_moment_of_inertia), ``:544-557`` (fitness_check),
``tscode/numba_functions.py:273-288`` (_score_embed_poses).
"""

from __future__ import annotations

import numpy as np

from .engine import get_engine
from .segments import ensemble_list, one_or_each, scalar_or_each

__all__ = ["get_inertia_moments", "get_moi_similarity_matches", "prune_by_moment_of_inertia", "prune_by_moment_of_inertia_batch",
           "similarity_refining_batch", "fitness_check", "fitness_mask", "_score_embed_poses"]

# Standard atomic weights as the `periodictable` package tabulates them (tscode/pt.py builds `pt` from it; the package is
# not installed in the build image, so the table could not be checked against it) for the elements TSCoDe systems are
# usually made of; pass `masses=` for anything else or to be independent of the table
_MASS = {1: 1.00794, 3: 6.941, 5: 10.811, 6: 12.0107, 7: 14.0067, 8: 15.9994, 9: 18.9984032, 11: 22.98976928, 12: 24.305,
         13: 26.9815386, 14: 28.0855, 15: 30.973762, 16: 32.065, 17: 35.453, 19: 39.0983, 20: 40.078, 29: 63.546, 30: 65.409,
         34: 78.96, 35: 79.904, 46: 106.42, 53: 126.90447}


_WARNED_MASSES = False


def get_inertia_moments(coords, masses):
    """tscode/algebra.py:165-186 for one structure: (3,) moments, ordered by absolute value (the input is not shifted)."""
    return get_engine().inertia_moments(np.asarray(coords, dtype=np.float64)[None], masses)[0]


def _moi_first_similar(structures, masses, max_deviation):
    eng = get_engine()
    return eng.moi_first_similar(eng.inertia_moments(structures, masses), max_deviation)


def get_moi_similarity_matches(structures, masses, max_deviation=1e-2):
    """tscode/algebra.py:188-205: [(i, j)] with j the first structure after i whose moments all lie within max_deviation."""
    first = _moi_first_similar(structures, masses, max_deviation)
    return [(int(i), int(first[i])) for i in np.flatnonzero(first >= 0)]


def _heavy_masses(atomnos, heavy, masses):
    """The masses of the heavy atoms: the caller's (per atom, hydrogens included) or the built-in table's, with its warning once.
    Called from the body of the public function itself (no comprehension, no helper in between), so that the warning names that
    function's caller."""
    if masses is None:
        global _WARNED_MASSES
        if not _WARNED_MASSES:                                           # said once, loudly: the table is this package's, not periodictable's
            import warnings
            warnings.warn("prune_by_moment_of_inertia: masses= not given; using tscode_amd's built-in table of standard atomic weights, "
                          "which has not been checked against the `periodictable` package the reference reads its masses from "
                          "(tscode/pt.py).  Pass masses=[pt[z].mass for z in atomnos] to use the reference's own values.", stacklevel=3)
            _WARNED_MASSES = True
        try:
            return np.array([_MASS[int(a)] for a in atomnos[heavy]])
        except KeyError as exc:
            raise ValueError(f"no built-in mass for element Z = {exc.args[0]}; pass masses=") from None
    return np.asarray(masses, dtype=np.float64)[heavy]


def prune_by_moment_of_inertia(structures, atomnos, max_deviation=1e-2, masses=None):
    """tscode/optimization_methods.py:327-358.  ``masses`` (per atom, hydrogens included) overrides the built-in table of
    periodictable values.  The member of a cluster that survives is ``tuple(graph.nodes)[0]`` of a networkx subgraph view,
    as in the reference (and, like there, decided by CPython's set order): the graph step builds the same objects."""
    import networkx as nx
    structures = np.asarray(structures)
    atomnos = np.asarray(atomnos)
    heavy = atomnos != 1
    heavy_masses = _heavy_masses(atomnos, heavy, masses)
    heavy_structures = np.ascontiguousarray(structures[:, heavy], dtype=np.float64)
    matches = get_moi_similarity_matches(heavy_structures, heavy_masses, max_deviation=max_deviation)
    G = nx.Graph(matches)                                                # :341
    from .numba_functions import _cluster_heads
    mask = np.ones(structures.shape[0], dtype=bool)
    for members, head in _cluster_heads(G):                              # :342-346: tuple(subgraph.nodes)[0] survives
        for i in members:
            if i != head:
                mask[i] = False
    return structures[mask], mask


# ---- the same for many ensembles per call --------------------------------------------------------------------------------------
def _atom_arrays(ens, atomnos, masses, need_heavy):
    """([atomnos_s], [masses_s or None]) of the ensembles ``ens``, each one array for all or one per ensemble, one entry per atom.
    ``need_heavy``: an ensemble without a heavy atom is refused (the moments are taken over the heavy atoms)."""
    S = len(ens)
    nos = [np.asarray(a).reshape(-1) for a in one_or_each(atomnos, S, "atomnos arrays", 1, exact=True)]
    ms = [None] * S if masses is None else [np.asarray(m, dtype=np.float64).reshape(-1) for m in one_or_each(masses, S, "masses arrays", 1, exact=True)]
    for s, (e, a, m) in enumerate(zip(ens, nos, ms)):
        if len(a) != e.shape[1] or (m is not None and len(m) != e.shape[1]):
            raise ValueError(f"ensemble {s}: atomnos and masses must have one entry per atom ({e.shape[1]})")
        if need_heavy and not (a != 1).any():
            raise ValueError(f"ensemble {s}: no heavy atom")
    return nos, ms


def prune_by_moment_of_inertia_batch(ensembles, atomnos, max_deviation=1e-2, masses=None):
    """prune_by_moment_of_inertia (tscode/optimization_methods.py:327-358) for many ensembles per call:
    ``[(structures_s[mask_s], mask_s)]``, each entry exactly what ``prune_by_moment_of_inertia(ensembles[s], atomnos_s,
    max_deviation_s, masses_s)`` returns.

    ``ensembles`` is a list of [N_s, n_s, 3] arrays; ``atomnos`` and ``masses`` one array for all or one per ensemble (``masses``
    as the single call takes it; None: the built-in table, whose warning is given once per call at most); ``max_deviation`` a scalar
    or one value per ensemble.  The moments of all ensembles are one launch and their pair searches another -- the same
    per-structure and per-row device code as the single call's kernels (csrc/moi.hpp); a row only looks at columns of its own
    ensemble.  The graph step (:341-358) stays on the host, per ensemble."""
    import networkx as nx
    from .numba_functions import _cluster_heads
    ens = ensemble_list(ensembles)
    nos, ms = _atom_arrays(ens, atomnos, masses, need_heavy=True)
    dev = scalar_or_each(max_deviation, len(ens), "max_deviation values")
    if not ens:
        return []
    heavy = [a != 1 for a in nos]
    heavy_masses = []
    for a, h, m in zip(nos, heavy, ms):                  # (a plain loop: _heavy_masses' warning counts frames)
        heavy_masses.append(_heavy_masses(a, h, m))
    eng = get_engine()
    moments = eng.inertia_moments_batch([np.ascontiguousarray(e[:, h], dtype=np.float64) for e, h in zip(ens, heavy)], heavy_masses)
    firsts = eng.moi_first_similar_batch(moments, dev)
    out = []
    for e, first in zip(ens, firsts):
        G = nx.Graph([(int(i), int(first[i])) for i in np.flatnonzero(first >= 0)])      # :341
        mask = np.ones(e.shape[0], dtype=bool)
        for members, head in _cluster_heads(G):                                           # :342-346: tuple(subgraph.nodes)[0] survives
            for i in members:
                if i != head:
                    mask[i] = False
        out.append((e[mask], mask))
    return out


def similarity_refining_batch(ensembles, atomnos, quadruplets=None, rot_corr=None, rmsd_thr=0.5, tfd=True, moi=True, rmsd=True, masses=None,
                              tfd_thresh=10, max_deviation=1e-2):
    """The similarity stages of Embedder.similarity_refining (tscode/embedder.py:1310-1388) on a list of ensembles, each stage ONE
    batched call over the ensembles that take it: ``[(structures_s, mask_s)]`` with ``mask_s`` over the input rows of ensemble s.

    Stages, order and size gates are the reference's (:1322-1382), each gate taken on the ensemble's current count:
      TFD      (prune_conformers_tfd_batch, ``tfd_thresh``) where ``tfd`` and ``quadruplets[s]`` is a non-empty array;
      MOI      (prune_by_moment_of_inertia_batch, ``max_deviation``) where ``moi`` and at most 500 structures are left (:1342);
      RMSD     (prune_conformers_rmsd_batch, ``rmsd_thr``) where ``rmsd`` and at most 1e5 are left (:1356);
      rot-corr (prune_rmsd_rot_corr_arrays_batch, ``max_rmsd = rmsd_thr`` as :1377 passes it) after the RMSD stage, where at most 500
               are left (:1372) and ``rot_corr[s]`` -- a set-up dict with the keys ``torsions``, ``angles``, ``move_masks``,
               ``sub_nodes`` -- is given.
    ``atomnos`` and ``masses`` are one array for all or one per ensemble; ``quadruplets`` and ``rot_corr`` None, one (T, 4)
    array / one set-up dict for all, or a list with one entry (or None) per ensemble; ``rmsd_thr`` a scalar or one value per
    ensemble.  An ensemble that went through rot-corr comes back centred and turned, because the reference replaces
    ``self.structures`` with that stage's result.  The reference's method leaves its TFD
    ``mask`` undefined when the quadruplets are empty (:1333-1335); here an empty array simply skips the stage."""
    from .numba_functions import prune_conformers_tfd_batch
    from .rmsd_pruning import prune_conformers_rmsd_batch
    from .rot_corr import _batch_setup, prune_rmsd_rot_corr_arrays_batch
    ens = ensemble_list(ensembles)
    nos, ms = _atom_arrays(ens, atomnos, masses, need_heavy=False)       # (each stage keeps its own rule on hydrogen-only ensembles)
    S = len(ens)
    thr = scalar_or_each(rmsd_thr, S, "rmsd_thr values")
    # one (T, 4) array of quadruplets (or a list of 4-tuples) and one set-up dict stand for all ensembles, as in the stages' own calls
    quads = one_or_each(quadruplets, S, "quadruplet arrays", 2, allow_none=True, exact=True, count=False)
    setups = one_or_each(rot_corr, S, "rot-corr set-ups", None, allow_none=True, count=False)
    if len(quads) != S or len(setups) != S:
        raise ValueError(f"{len(quads)} quadruplet arrays and {len(setups)} rot-corr set-ups for {S} ensembles")
    quads = [None if q is None else np.asarray(q, dtype=np.int32).reshape(-1, 4) for q in quads]
    for s, (e, q) in enumerate(zip(ens, quads)):
        if q is not None and len(q) and (q.min() < 0 or q.max() >= e.shape[1]):
            raise ValueError(f"ensemble {s}: quadruplet atom index out of range")
    for at, s in enumerate(s for s in range(S) if setups[s] is not None):
        _batch_setup(at, ens[s].shape[1], nos[s], setups[s])         # (ValueError here, not mid-way; it counts the ensembles that have a set-up)
    if S == 0:
        return []
    cur = list(ens)
    rows = [np.arange(len(e)) for e in ens]             # the input rows still alive

    def stage(which, call):
        if which:
            for s, (kept, mask) in zip(which, call(which)):
                cur[s], rows[s] = kept, rows[s][mask]

    if tfd:
        stage([s for s in range(S) if quads[s] is not None and len(quads[s])],
              lambda w: prune_conformers_tfd_batch([cur[s] for s in w], [quads[s] for s in w], thresh=tfd_thresh))
    if moi:
        stage([s for s in range(S) if len(cur[s]) <= 500],
              lambda w: prune_by_moment_of_inertia_batch([cur[s] for s in w], [nos[s] for s in w], max_deviation=max_deviation,
                                                         masses=None if masses is None else [ms[s] for s in w]))
    if rmsd:
        stage([s for s in range(S) if len(cur[s]) <= 1e5],
              lambda w: prune_conformers_rmsd_batch([cur[s] for s in w], [nos[s] for s in w], rmsd_thr=thr[w]))
        stage([s for s in range(S) if len(cur[s]) <= 1e5 and len(cur[s]) <= 500 and setups[s] is not None],
              lambda w: prune_rmsd_rot_corr_arrays_batch([cur[s] for s in w], [nos[s] for s in w], [setups[s] for s in w], max_rmsd=thr[w]))
    out = []
    for s in range(S):
        mask = np.zeros(len(ens[s]), dtype=bool)
        mask[rows[s]] = True
        out.append((cur[s], mask))
    return out


def _score_embed_poses(structures, constrained_indices, constrained_distances):
    """tscode/numba_functions.py:273-288: float32 [N] sums of |distance - target| over each pose's constraints."""
    return get_engine().embed_scores(structures, constrained_indices, constrained_distances)[0]


def fitness_mask(structures, constrained_indices, constrained_distances, threshold):
    """The loop of tscode/embedder.py:1283-1290 in one launch: fitness_check for every structure (targets of None -> NaN)."""
    dist = np.array([[np.nan if t is None else t for t in row] for row in constrained_distances], dtype=np.float64)
    return get_engine().embed_scores(structures, constrained_indices, dist)[1] < threshold


def fitness_check(coords, constraints, targets, threshold) -> bool:
    """tscode/optimization_methods.py:544-557: the SIGNED deviations from the target distances sum to less than threshold."""
    return bool(fitness_mask(np.asarray(coords, dtype=np.float64)[None], np.asarray(constraints)[None], [list(targets)], threshold)[0])
