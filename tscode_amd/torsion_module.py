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
           "csearch_rotate_multi", "csearch_candidates_multi", "clustered_csearch_step", "most_diverse_conformers", "diverse_select"]


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


# ---- many starts, many torsion sets (tscode/torsion_module.py:736-780, tscode/embedder.py:1907-1939) ----------------------------------
LDS_STAGING_BYTES = 150 * 1024          # csearch_args (csrc/adjacent.hip): torsion lists of one set + one wavefront's structure
MULTI_SCRATCH_BYTES = 1 << 30           # device bytes one launch of csearch_candidates_multi may fill with candidates (n_out=None)
N_FOLD_ANGLES = {2: (0, 180), 3: (0, 120, 240), 4: (0, 90, 180, 270), 6: (0, 60, 120, 180, 240, 300)}   # Torsion.get_angles, :112-118


def _kept_rows(rotated, n_out, max_tries):
    """The rows of one start's table that tscode/torsion_module.py:505-511 appends, given ``rotated_bonds`` of every row: a row is
    kept iff it is non-zero, and only just after a row was kept is ``len(new_structures) == n_out or a == max_tries`` tested -- so a
    dropped row ``max_tries`` does not end the walk.  ``n_out=None``: no stop on the count (:779).  Returns (rows, consumed):
    the kept row indices in order and how many rows the loop walked.  Pure host code: what the device selection is compared with."""
    rotated = np.asarray(rotated).ravel()
    flags = rotated != 0
    rank = np.cumsum(flags)                                             # len(new_structures) just after each row
    stop = flags & (np.arange(len(flags)) == max_tries)
    if n_out is not None:
        stop |= flags & (rank == n_out)
    hits = np.flatnonzero(stop)
    consumed = int(hits[0]) + 1 if len(hits) else len(flags)
    return np.flatnonzero(flags[:consumed]), consumed


def _lds_bytes(n_tors, n):
    lists = (n_tors * n * 2 * 2 + n_tors * 4 * 4 + 15) & ~15            # torsion_lists_bytes (csrc/csearch.hpp)
    return lists + n * 3 * 8 + 3 * ((n + 2) & ~1) * 4 + 12 * 8          # + csearch_wave_bytes


def _pack_sets(starts, sets, set_of_start):
    """Argument checks (ValueError, before the library is loaded) and the arrays of tsc_csearch_rotate_multi: the sets back to back,
    every table zero-padded to the widest set and stacked into one (row_base[k] = first row of set k's table)."""
    starts = np.asarray(starts, dtype=np.float64)
    if starts.ndim == 2:
        starts = starts[None]
    if starts.ndim != 3 or starts.shape[2] != 3 or starts.shape[1] == 0:
        raise ValueError("starts must be (n_starts, n_atoms, 3): every start needs the same number of atoms")
    starts = np.ascontiguousarray(starts)
    S, n = starts.shape[:2]
    sets = list(sets)
    if not sets:
        raise ValueError("at least one torsion set is needed")
    if set_of_start is None:
        if len(sets) == 1:
            set_of_start = np.zeros(S, dtype=np.int32)
        elif len(sets) == S:
            set_of_start = np.arange(S, dtype=np.int32)
        else:
            raise ValueError(f"{len(sets)} torsion sets for {S} starts: set_of_start is needed")
    set_of_start = np.ascontiguousarray(np.asarray(set_of_start).ravel(), dtype=np.int32)
    if len(set_of_start) != S or (S and (set_of_start.min() < 0 or set_of_start.max() >= len(sets))):
        raise ValueError(f"set_of_start: expected {S} set indices in [0, {len(sets)})")
    tors, masks, tables = [], [], []
    for k, (t, m, a) in enumerate(sets):
        t = np.asarray(t, dtype=np.int32).reshape(-1, 4)
        m = np.asarray(m)
        if m.size != len(t) * n:
            raise ValueError(f"torsion set {k}: masks must be ({len(t)}, {n}): the set's atoms differ from the starts'")
        if len(t) and (t.min() < 0 or t.max() >= n):
            raise ValueError(f"torsion set {k}: atom index out of range")
        a = np.asarray(a)
        if a.ndim != 2 and a.size == 0:
            a = np.zeros((0, len(t)), dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != len(t):
            raise ValueError(f"torsion set {k}: the angle table is {a.shape[-1] if a.ndim else 0} wide for {len(t)} torsions")
        if n > 65535 or _lds_bytes(len(t), n) > LDS_STAGING_BYTES:
            raise ValueError(f"torsion set {k}: {n} atoms x {len(t)} torsions exceed the LDS staging of the csearch kernels")
        tors.append(t), masks.append(m.reshape(len(t), n).astype(np.uint8)), tables.append(a.astype(np.int32))
    t_max = max(len(t) for t in tors)
    set_off = np.concatenate([[0], np.cumsum([len(t) for t in tors])]).astype(np.int32)
    table_len = np.array([len(a) for a in tables], dtype=np.int64)
    row_base = np.concatenate([[0], np.cumsum(table_len)[:-1]]).astype(np.int64)
    if table_len.sum() >= 2**31:
        raise ValueError("the angle tables have 2^31 rows or more")
    angles = np.zeros((int(table_len.sum()), t_max), dtype=np.int32)
    for k, a in enumerate(tables):
        angles[row_base[k]:row_base[k] + len(a), :a.shape[1]] = a
    import types
    return types.SimpleNamespace(starts=starts, S=S, n=n, torsions=np.ascontiguousarray(np.concatenate(tors)), masks=np.ascontiguousarray(np.concatenate(masks)),
                                 set_off=set_off, start_set=set_of_start, angles=angles, t_max=t_max, table_len=table_len, row_base=row_base)


def csearch_rotate_multi(starts, sets, set_of_start=None, rows=None, thresh=1.5, max_clashes=0):
    """Every candidate of many starts in ONE launch (tsc_csearch_rotate_multi): ``starts [S, n, 3]``; ``sets`` a list of
    ``(torsions [T_k, 4], masks [T_k, n], angles [A_k, T_k])``; start s uses set ``set_of_start[s]`` (default: the only set, or
    set s when there are S of them).  ``rows``: per start, the rows of its set's table to rotate (default: all, in table order).
    Returns ``(new_coords [K, n, 3], rotated_bonds [K], start_index [K], row_index [K])``, start after start."""
    p = _pack_sets(starts, sets, set_of_start)
    if rows is None:
        rows = [np.arange(p.table_len[k]) for k in p.start_set]
    if len(rows) != p.S:
        raise ValueError(f"rows: expected {p.S} index lists, one per start")
    rows = [np.asarray(r, dtype=np.int64).ravel() for r in rows]
    for s, r in enumerate(rows):
        if len(r) and (r.min() < 0 or r.max() >= p.table_len[p.start_set[s]]):
            raise ValueError(f"rows[{s}]: row index out of range")
    start_index = np.repeat(np.arange(p.S, dtype=np.int32), [len(r) for r in rows])
    row_index = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    if len(start_index) >= 2**31:
        raise ValueError("2^31 candidates or more in one call")
    cand_row = (row_index + p.row_base[p.start_set[start_index]]).astype(np.int32)
    out, rb = get_engine().csearch_rotate_multi(p.starts, p.torsions, p.masks, p.set_off, p.start_set, p.angles, start_index, cand_row, thresh,
                                                max_clashes)
    return out, rb, start_index, row_index


def csearch_candidates_multi(starts, sets, set_of_start=None, n_out=100, max_tries=10000, thresh=1.5, block=None, include_start=False):
    """``csearch_candidates`` for many starts at once: ``(structures [K, n, 3], start_index [K])`` where the rows of start s are what
    ``csearch_candidates(starts[s], *sets[set_of_start[s]], n_out, max_tries, thresh)`` returns, start after start.

    The tables are walked in rounds.  A round rotates the next ``block`` rows of every start that is not finished in one launch
    (tsc_csearch_rotate_multi_dev), applies the stop rule of tscode/torsion_module.py:505-511 per start and compacts the rows it
    keeps on the device (tsc_csearch_select_dev); the host downloads those rows and three counters per start, never the
    candidates.  ``block`` defaults to ``2 * n_out`` rounded up to a multiple of 64; the result does not depend on it.
    ``n_out=None`` keeps every rotated row (the rule of clustered_csearch, :779; ``max_tries`` is then ignored) and a round takes
    whole tables; the starts of one launch are then limited so that its candidates fill at most ``MULTI_SCRATCH_BYTES`` (1 GiB)
    of device memory -- always at least one start.  ``include_start=True`` puts each start itself in front of its candidates (:741)."""
    p = _pack_sets(starts, sets, set_of_start)
    if n_out is not None and int(n_out) != n_out:
        raise ValueError("n_out must be an integer or None")
    if n_out is None:
        max_tries = -1
        block = int(p.table_len.max()) if block is None else int(block)
    elif block is None:
        block = -(-2 * max(int(n_out), 1) // 64) * 64
    block = max(int(block), 1)
    row_bytes = p.n * 24
    per_launch = max(1, MULTI_SCRATCH_BYTES // (row_bytes * block))      # starts per launch
    eng = get_engine()
    held = []

    def up(a):
        held.append(eng.dev_upload(a))
        return held[-1]

    pieces = [[starts_row[None]] if include_start else [] for starts_row in p.starts]
    try:
        d_starts, d_tors, d_masks, d_angles = up(p.starts), up(p.torsions), up(p.masks), up(p.angles)
        kept_count, done, consumed = np.zeros(p.S, np.int32), np.zeros(p.S, np.int32), np.zeros(p.S, np.int32)
        d_state = [up(kept_count), up(done), up(consumed)]
        next_row = np.zeros(p.S, dtype=np.int64)
        tlen = p.table_len[p.start_set]
        cap_rows = 0
        d_cand = d_rb = d_kept = None
        while True:
            live = np.flatnonzero((done == 0) & (next_row < tlen))[:per_launch]
            if not len(live):
                break
            seg_len = np.minimum(block, tlen[live] - next_row[live])
            seg_off = np.concatenate([[0], np.cumsum(seg_len)]).astype(np.int32)
            n_cand = int(seg_off[-1])
            cand_start = np.repeat(live.astype(np.int32), seg_len)
            local = np.arange(n_cand, dtype=np.int64) - np.repeat(seg_off[:-1].astype(np.int64), seg_len) + np.repeat(next_row[live], seg_len)
            cand_row = (local + p.row_base[p.start_set[cand_start]]).astype(np.int32)
            items = eng.csearch_multi_plan(cand_start, p.start_set, p.set_off, p.n)
            if n_cand > cap_rows:                                            # the candidates and the rows kept of one round
                for a in (d_cand, d_rb, d_kept):
                    if a is not None:
                        eng.dev_free(a), held.remove(a)
                cap_rows = n_cand
                d_cand, d_rb, d_kept = eng.dev_alloc(cap_rows * row_bytes), eng.dev_alloc(cap_rows * 4), eng.dev_alloc(cap_rows * row_bytes)
                held.extend((d_cand, d_rb, d_kept))
            small = [eng.dev_upload(a) for a in (cand_start, cand_row, items, seg_off, live.astype(np.int32), next_row[live].astype(np.int32))]
            held.extend(small)
            eng.csearch_rotate_multi_dev(d_starts, p.n, d_tors, d_masks, p.set_off, d_angles, p.t_max, small[0], small[1], n_cand, small[2],
                                         len(items), thresh, 0, d_cand, d_rb)
            n_kept = eng.csearch_select_dev(d_cand, d_rb, p.n, small[3], small[4], small[5], len(live), n_out, max_tries, *d_state, d_kept, cap_rows)
            before = kept_count.copy()
            eng.dev_download(d_state[0], kept_count), eng.dev_download(d_state[1], done), eng.dev_download(d_state[2], consumed)
            rows = eng.dev_download(d_kept, np.empty((n_kept, p.n, 3)))
            for a in small:
                eng.dev_free(a), held.remove(a)
            took = (kept_count - before)[live]
            assert int(took.sum()) == n_kept
            at = 0
            for s, k in zip(live, took):
                if k:
                    pieces[s].append(rows[at:at + k])
                at += k
            next_row[live] += seg_len
    finally:
        for a in held:
            eng.dev_free(a)
    counts = [sum(len(x) for x in pc) for pc in pieces]
    flat = [x for pc in pieces for x in pc]
    structures = np.concatenate(flat) if flat else np.zeros((0, p.n, 3))
    return structures, np.repeat(np.arange(p.S, dtype=np.int32), counts)


def clustered_csearch_step(starting_points, torsions_group, masks, angles=None, thresh=1.5, n_folds=None):
    """The ``new_structures`` array of tscode/torsion_module.py:734-783 for ONE torsion group: every starting point followed by its
    candidates that rotated at least one bond, for the whole angle table.  ``torsions_group``: the group's torsions as ``[T, 4]``
    indices, or objects with ``.torsion`` and ``.n_fold`` like the reference's; the table is ``cartesian_product`` of the n-fold
    angles (``n_folds`` for index input) unless ``angles [A, T]`` is given.  Masks come from the caller (_get_rotation_mask).
    Equals ``csearch_candidates_multi(starting_points, [(torsions, masks, angles)], n_out=None, include_start=True)[0]``."""
    if len(torsions_group) and hasattr(torsions_group[0], "torsion"):
        if n_folds is None:
            n_folds = [t.n_fold for t in torsions_group]
        torsions_group = [t.torsion for t in torsions_group]
    torsions_group = np.asarray(torsions_group, dtype=np.int32).reshape(-1, 4)
    if angles is None:
        if n_folds is None or len(n_folds) != len(torsions_group):
            raise ValueError("either angles or one n_fold per torsion is needed")
        from .utils import cartesian_product
        angles = cartesian_product(*[N_FOLD_ANGLES[int(f)] for f in n_folds])
    return csearch_candidates_multi(starting_points, [(torsions_group, masks, angles)], None, n_out=None, thresh=thresh, include_start=True)[0]


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
