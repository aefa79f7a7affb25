"""Drop-in names of the conformational-search rotations and their batched form.

Reference: ``tscode/utils.py:389-414`` (rotate_dihedral), ``tscode/numba_functions.py:26-47`` (torsion_comp_check),
``tscode/torsion_module.py:463-509`` (the loop over angle sets of random_csearch / csearch).  The rotation masks
(``_get_rotation_mask``, a graph walk) and the shuffled angle table stay with the caller; everything per candidate
runs on the GPU, one wavefront per candidate.
"""

from __future__ import annotations

import numpy as np

from .algebra import rot_mat_from_pointer
from .engine import get_engine

__all__ = ["rotate_dihedral", "rotate_dihedral_batch", "torsion_comp_check", "csearch_rotate", "csearch_candidates",
           "most_diverse_conformers", "diverse_select"]


def csearch_rotate(coords, torsions, masks, angles, thresh=1.5, max_clashes=0):
    """All candidates at once: ``(new_coords [M, n, 3], rotated_bonds [M])`` for ``angles [M, n_torsions]`` (degrees, ints)."""
    return get_engine().csearch_rotate(coords, torsions, masks, angles, thresh, max_clashes)


def csearch_candidates(coords, torsions, masks, angles, n_out=100, max_tries=10000, thresh=1.5, block=8192):
    """The ``new_structures`` array of tscode/torsion_module.py:463-509: candidates in the order of ``angles`` (shuffle it
    first, :459), kept iff at least one bond really rotated (:505), until ``n_out`` are kept or row ``max_tries`` is reached.
    The angle table is walked in blocks of ``block`` rows and the walk stops where the reference's loop stops: a
    cartesian-product table (3^12 rows x 100 atoms ...) is never rotated, stored or downloaded as a whole."""
    angles = np.asarray(angles)
    coords = np.asarray(coords, dtype=np.float64)
    out, n_kept = [], 0
    for lo in range(0, len(angles), block):
        new_coords, rotated = csearch_rotate(coords, torsions, masks, angles[lo:lo + block], thresh)
        kept, done = [], False
        for a in np.flatnonzero(rotated != 0):
            kept.append(a)
            n_kept += 1
            if n_kept == n_out or lo + a == max_tries:          # :510 (tested only when a structure has just been kept)
                done = True
                break
        out.append(new_coords[kept])
        if done:
            break
    return np.concatenate(out) if out else np.zeros((0,) + coords.shape)


def rotate_dihedral_batch(coords, dihedral, angles, mask):
    """Structures f64[M, n, 3] sharing torsion and mask, structure s turned by ``angles[s]`` degrees (floats): what a search over
    correction angles (tscode/torsion_module.py:984-1005: rotate, look, rotate back, per angle) becomes as ONE call -- rotate M copies."""
    return get_engine().rotate_dihedral_batch(coords, [int(i) for i in dihedral], mask, angles)


def rotate_dihedral(coords, dihedral, angle, mask=None, indices_to_be_moved=None):
    """tscode/utils.py:389-414.  Like the reference it changes ``coords`` in place and returns it."""
    coords_arr = np.asarray(coords)
    n = len(coords_arr)
    if indices_to_be_moved is not None:
        mask = np.array([i in indices_to_be_moved for i in range(n)])
    if mask is None:
        m = np.zeros(n, dtype=bool)
        m[dihedral[0]] = True
        mask = m
    mask = np.asarray(mask, dtype=bool)
    if float(angle) == 0.0:
        return coords                                    # (the identity; the candidate loop never rotates by zero, :482)
    # ONE structure, one rotation: on the host, like the other single 3x3 helpers of the path (algebra.py) -- the
    # reference's search loops call this once per torsion and candidate and once per 5-degree walk-back step
    # (tscode/torsion_module.py:482-489, :756-763), and a GPU call per molecule-sized rotation (three uploads, a launch, a download, a
    # synchronisation: 50 us and more) would slow them down.  Whole tables of rotations belong on rotate_dihedral_batch / csearch_rotate.
    _, i2, i3, _ = (int(i) for i in dihedral)
    mat = rot_mat_from_pointer(coords_arr[i2] - coords_arr[i3], float(angle))
    center = coords_arr[i3].copy()
    coords_arr[mask] = (mat @ (coords_arr[mask] - center).T).T + center
    return coords


def torsion_comp_check(coords, torsion, mask, thresh=1.5, max_clashes=0) -> int:
    """tscode/numba_functions.py:26-47: 1 if at most ``max_clashes`` distances between the moved side and the rest (the bond
    atoms aside) are below ``thresh``, else 0."""
    coords = np.asarray(coords, dtype=np.float64)
    return int(get_engine().torsion_comp_check(coords[None], torsion, mask, thresh, max_clashes)[0])


def diverse_select(structures, k, init_rows=None, seed=None, energies=None, max_iter=300, tol=1e-4):
    """tscode/torsion_module.py:882-922 in one library call (tsc_diverse_select): align onto the first structure, Lloyd's
    k-means on the flattened aligned coordinates from the rows ``init_rows`` (or, when None, from k-means++ seeds drawn with
    ``np.random.default_rng(seed)`` on the aligned features), one pick per cluster.  Returns (aligned f64[N, n, 3], labels
    i32[N], picked i32[k] with -1 for an empty cluster, init_rows i32[k], n_iter)."""
    import ctypes as C

    from ._lib import check, ptr
    from .hypermolecule_class import _check_structures
    from .kmeans import _check_k, seed_uniforms

    structures = np.ascontiguousarray(structures, dtype=np.float64)
    _check_structures(structures)
    N, n = structures.shape[:2]
    k = int(k)
    _check_k(N, 3 * n, k)
    u = None
    if init_rows is None:
        u = seed_uniforms(k, seed)
        rows = np.empty(k, dtype=np.int32)
    else:
        rows = np.ascontiguousarray(np.asarray(init_rows).ravel(), dtype=np.int32)
        if len(rows) != k or rows.min() < 0 or rows.max() >= N:
            raise ValueError(f"init_rows: expected {k} row indices in [0, {N})")
    if energies is not None:
        energies = np.ascontiguousarray(energies, dtype=np.float64).ravel()
        if len(energies) != N:
            raise ValueError(f"{len(energies)} energies for {N} structures")
        if np.isnan(energies).any():
            raise ValueError("energies contain NaN")
    aligned = np.empty_like(structures)
    labels = np.empty(N, dtype=np.int32)
    picked = np.empty(k, dtype=np.int32)
    n_iter = C.c_int()
    eng = get_engine()
    check(eng.lib.tsc_diverse_select(eng._h, ptr(structures), C.c_int64(N), C.c_int(n), ptr(rows), ptr(u), C.c_int(k), ptr(energies),
                                     C.c_int(int(max_iter)), C.c_double(float(tol)), ptr(aligned), ptr(labels), ptr(picked), C.byref(n_iter)))
    return aligned, labels, picked, rows, n_iter.value


def most_diverse_conformers(n, structures, torsion_array, energies=None, interactive_print=False, *, seed=None, init_rows=None):
    """Drop-in for tscode.torsion_module.most_diverse_conformers (:849-924): the n most diverse structures of the set.
    TFD prune (prune_conformers_tfd), alignment onto the first structure, k-means with n clusters on the flattened aligned
    coordinates, one structure per cluster, in cluster order; the returned coordinates are the ALIGNED ones, as in the reference.

    * ``len(structures) <= n`` (before or after the TFD prune) returns the structures as they are (:859, :875); ``n > 300``
      returns ``structures[np.sort(np.random.choice(len(structures), size=n))]`` -- that very call, so a caller who seeds
      ``np.random`` gets the reference's rows (:863-865).
    * With ``energies``: the lowest-energy member of each cluster, the first on a tie.  Structure i AFTER the TFD prune is paired
      with ``energies[i]`` of the UNPRUNED list, because that is what ``zip(structures, energies, labels)`` does at :896 once
      :872 has replaced ``structures``; reproduced as it is.  (An empty cluster makes the reference raise at :901; here it is
      left out.)
    * Without: from each non-empty cluster the member with the largest cumdist, the first on a tie, where the member at position
      p of its cluster's list sums |centre_c - member| over the atoms and over the centres c != p (:919: the reference's ``c``
      is the position from ``enumerate(cluster)``; reproduced as it is).
    * Initial centres: the aligned rows ``init_rows`` if given, else k-means++ seeds (kmeans.kmeans_plusplus_rows' rule) drawn
      with ``np.random.default_rng(seed)``; ``seed=None`` draws a seed from ``np.random``.  The reference's own initialisation
      is scikit-learn's unseeded default and has no reproducible result; this one is reproducible for a seed and equals
      scikit-learn's Lloyd iteration for a given ``init``."""
    from .numba_functions import prune_conformers_tfd

    if len(structures) <= n:                                                            # :859
        return structures
    if n > 300:                                                                         # :863-865
        indices = np.sort(np.random.choice(len(structures), size=n))
        return structures[indices]
    if interactive_print:
        print(f'Removing similar structures...{" "*10}', end='\r')
    structures, _ = prune_conformers_tfd(structures, torsion_array)                     # :872
    if len(structures) <= n:                                                            # :875
        return structures
    if interactive_print:
        print(f'Aligning structures and performing KMeans clustering...{" "*10}', end='\r')
    if init_rows is None and seed is None:
        seed = int(np.random.randint(0, 2**31 - 1))
    if energies is not None:
        energies = np.asarray(energies, dtype=np.float64).ravel()[:len(structures)]     # :896 (zip stops at the shorter)
        if len(energies) < len(structures):
            raise ValueError(f"{len(energies)} energies for {len(structures)} structures")
    aligned, _, picked, _, _ = diverse_select(structures, n, init_rows=init_rows, seed=seed, energies=energies)
    return aligned[picked[picked >= 0]]
