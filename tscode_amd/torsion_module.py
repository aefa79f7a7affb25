"""Drop-in names of the conformational-search rotations and their batched form.

Reference: ``tscode/utils.py:389-414`` (rotate_dihedral), ``tscode/numba_functions.py:26-47`` (torsion_comp_check),
``tscode/torsion_module.py:463-509`` (the loop over angle sets of random_csearch / csearch).  The candidate entry points take
torsions, rotation masks and the shuffled angle table from the caller; everything per candidate runs on the GPU, one wavefront
per candidate.  ``torsion_sets_batch`` makes torsions, folds and masks from coordinates for a whole ensemble (csearch's set-up,
``:559-615``: hydrogen bonds and graph searches on the GPU, the rotatability rules per topology class on the host), and
``csearch_augmentation_batch`` joins the two.  ``group_torsions_batch`` decides per pose which torsions turn together
(``_group_torsions_dbscan``, ``:373-397``, one wavefront per pose), ``clustered_csearch_batch`` drives the pieces round after round
(``clustered_csearch`` mode 1, ``:655-847``) and ``csearch_batch`` is the front door (``csearch``, ``:523-653``).
"""

from __future__ import annotations

import numpy as np

from .algebra import rot_mat_from_pointer
from .engine import get_engine
from .segments import byte_slices, one_or_each, pack

__all__ = ["rotate_dihedral", "rotate_dihedral_batch", "torsion_comp_check", "csearch_rotate", "csearch_candidates",
           "csearch_rotate_multi", "csearch_candidates_multi", "clustered_csearch_step", "most_diverse_conformers", "diverse_select",
           "hydrogen_bonds_batch", "torsion_sets_batch", "csearch_augmentation_batch", "class_graph", "candidate_quadruplets",
           "rotatable_torsions", "class_torsion_set", "group_torsions_batch", "clustered_csearch_batch", "csearch_batch",
           "clustered_csearch", "_group_torsions_dbscan"]


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


# ---- the same for many small ensembles per call ------------------------------------------------------------------------------------------
DIVERSE_BATCH_BYTES = 1 << 30           # device bytes one tsc_diverse_select_batch call may fill with structures (input, aligned, centred)


def _diverse_batch_args(ensembles, k, init_rows, seeds, energies):
    """The checked arguments of diverse_select_batch, per segment: (structures, k, rows or None, uniforms or None, energies or None)."""
    from .hypermolecule_class import _check_structures
    from .kmeans import _check_k, seed_uniforms

    ens = [np.ascontiguousarray(e, dtype=np.float64) for e in ensembles]
    S = len(ens)
    ks = [int(k)] * S if np.ndim(k) == 0 else [int(v) for v in one_or_each(k, S, "cluster counts", None)]
    init_rows, seeds, energies = (one_or_each(v, S, w, None, allow_none=True)
                                  for v, w in ((init_rows, "init_rows entries"), (seeds, "seeds"), (energies, "energies arrays")))
    segs = []
    for s in range(S):
        _check_structures(ens[s])
        N, n = ens[s].shape[:2]
        _check_k(N, 3 * n, ks[s])
        rows = u = e = None
        if init_rows[s] is None:
            u = seed_uniforms(ks[s], seeds[s])
        else:
            rows = np.ascontiguousarray(np.asarray(init_rows[s]).ravel(), dtype=np.int32)
            if len(rows) != ks[s] or rows.min() < 0 or rows.max() >= N:
                raise ValueError(f"ensemble {s}: init_rows: expected {ks[s]} row indices in [0, {N})")
        if energies[s] is not None:
            e = np.ascontiguousarray(energies[s], dtype=np.float64).ravel()
            if len(e) != N:
                raise ValueError(f"ensemble {s}: {len(e)} energies for {N} structures")
            if np.isnan(e).any():
                raise ValueError(f"ensemble {s}: energies contain NaN")
        segs.append((ens[s], ks[s], rows, u, e))
    return segs


def _diverse_select_slice(segs, max_iter, tol):
    """One tsc_diverse_select_batch call."""
    import ctypes as C

    from ._lib import check, ptr
    S = len(segs)
    p = pack([x for x, *_ in segs])
    ks = np.array([k for _, k, *_ in segs], dtype=np.int32)
    row_off, k_off = p.row_off, np.concatenate(([0], np.cumsum(ks.astype(np.int64))))
    rows = np.zeros(int(k_off[-1]), dtype=np.int32)
    u = np.zeros(int(k_off[-1]), dtype=np.float64)
    energies = np.zeros(int(row_off[-1]), dtype=np.float64)
    flags = np.zeros(S, dtype=np.uint8)
    for s, (_, _, r, us, e) in enumerate(segs):
        if r is None:
            u[k_off[s]:k_off[s + 1]] = us
            flags[s] |= 2
        else:
            rows[k_off[s]:k_off[s + 1]] = r
        if e is not None:
            energies[row_off[s]:row_off[s + 1]] = e
            flags[s] |= 1
    aligned = np.empty_like(p.flat)
    labels = np.empty(int(row_off[-1]), dtype=np.int32)
    picked = np.empty(int(k_off[-1]), dtype=np.int32)
    n_iter = np.zeros(S, dtype=np.int32)
    eng = get_engine()
    check(eng.lib.tsc_diverse_select_batch(eng._h, ptr(p.flat), ptr(p.offsets), ptr(p.n_structs), ptr(p.n_atoms), ptr(ks), C.c_int64(S), ptr(rows),
                                           ptr(u) if (flags & 2).any() else None, ptr(energies) if (flags & 1).any() else None, ptr(flags),
                                           C.c_int(int(max_iter)), C.c_double(float(tol)), ptr(aligned), ptr(labels), ptr(picked), ptr(n_iter)))
    return [(a, lab, picked[k_off[s]:k_off[s + 1]], rows[k_off[s]:k_off[s + 1]], int(n_iter[s]))
            for s, (a, lab) in enumerate(zip(p.cut(aligned, doubles=True), p.cut(labels)))]


def diverse_select_batch(ensembles, k, init_rows=None, seeds=None, energies=None, max_iter=300, tol=1e-4):
    """diverse_select for many ensembles per call (tsc_diverse_select_batch): ``[(aligned, labels, picked, init_rows, n_iter)]``, each
    entry what ``diverse_select(ensembles[s], k_s, init_rows[s], seeds[s], energies[s], max_iter, tol)`` returns, bit for bit.

    ``ensembles`` is a list of f64[N_s, n_s, 3]; ``k`` an int or one per ensemble; ``init_rows``, ``seeds`` and ``energies`` are
    lists with None entries allowed (or None for all).  A list whose structures would fill more than ``DIVERSE_BATCH_BYTES`` on the
    device goes in slices of ensembles; a list of one goes to diverse_select."""
    segs = _diverse_batch_args(ensembles, k, init_rows, seeds, energies)
    if len(segs) == 1:
        x, ks, rows, _, e = segs[0]
        sd = None if seeds is None else seeds[0]
        return [diverse_select(x, ks, init_rows=rows, seed=sd, energies=e, max_iter=max_iter, tol=tol)]
    out = []
    for at, end in byte_slices([3 * x.nbytes for x, *_ in segs], DIVERSE_BATCH_BYTES):
        out += _diverse_select_slice(segs[at:end], max_iter, tol) if end - at > 1 else \
            [diverse_select(segs[at][0], segs[at][1], init_rows=segs[at][2], seed=None if seeds is None else seeds[at], energies=segs[at][4],
                            max_iter=max_iter, tol=tol)]
    return out


def most_diverse_conformers_batch(n, ensembles, torsion_arrays, energies=None, *, seeds=None, init_rows=None):
    """most_diverse_conformers for many ensembles per call: ``[array]``, each entry what
    ``most_diverse_conformers(n_s, ensembles[s], torsion_array_s, energies[s], seed=seeds[s], init_rows=init_rows[s])`` returns.

    ``n`` is an int or one per ensemble; ``torsion_arrays`` one i32[T, 4] for all or a list with one per ensemble; ``energies``,
    ``seeds`` and ``init_rows`` are lists with None entries allowed.  Every rule of most_diverse_conformers holds per segment: the
    early returns at ``len <= n`` before and after the TFD prune, ``n > 300`` with that very ``np.random.choice`` call, the
    energies zip quirk, and a seed drawn from ``np.random`` when neither seed nor rows are given.  The ``np.random`` draws are made
    in segment order, so a caller who seeds ``np.random`` gets what the loop over most_diverse_conformers gives.  The TFD prune in
    front is ONE prune_conformers_tfd_batch call over the segments that reach it, the clustering ONE diverse_select_batch call."""
    from . import numba_functions

    S = len(ensembles)
    ns = [int(n)] * S if np.ndim(n) == 0 else [int(v) for v in one_or_each(n, S, "n entries", None)]
    energies, seeds, init_rows = (one_or_each(v, S, w, None, allow_none=True)
                                  for v, w in ((energies, "energies arrays"), (seeds, "seeds"), (init_rows, "init_rows entries")))
    torsion_arrays = one_or_each(torsion_arrays, S, "torsion arrays", 2)
    out = [None] * S
    to_prune = [s for s in range(S) if len(ensembles[s]) > ns[s] and ns[s] <= 300]               # :859, :863
    pruned = dict(zip(to_prune, (p for p, _ in numba_functions.prune_conformers_tfd_batch([ensembles[s] for s in to_prune],
                                                                                          [torsion_arrays[s] for s in to_prune]))))   # :872
    cluster = []
    for s in range(S):                                                                           # (the draws, in segment order)
        structures = ensembles[s]
        if len(structures) <= ns[s]:                                                             # :859
            out[s] = structures
        elif ns[s] > 300:                                                                        # :863-865
            out[s] = structures[np.sort(np.random.choice(len(structures), size=ns[s]))]
        elif len(pruned[s]) <= ns[s]:                                                            # :875
            out[s] = pruned[s]
        else:
            if init_rows[s] is None and seeds[s] is None:
                seeds[s] = int(np.random.randint(0, 2**31 - 1))
            if energies[s] is not None:
                energies[s] = np.asarray(energies[s], dtype=np.float64).ravel()[:len(pruned[s])]   # :896 (zip stops at the shorter)
                if len(energies[s]) < len(pruned[s]):
                    raise ValueError(f"ensemble {s}: {len(energies[s])} energies for {len(pruned[s])} structures")
            cluster.append(s)
    if cluster:
        res = diverse_select_batch([pruned[s] for s in cluster], [ns[s] for s in cluster], init_rows=[init_rows[s] for s in cluster],
                                   seeds=[seeds[s] for s in cluster], energies=[energies[s] for s in cluster])
        for s, (aligned, _, picked, _, _) in zip(cluster, res):
            out[s] = aligned[picked[picked >= 0]]
    return out


# ---- from coordinates to torsion sets (tscode/torsion_module.py:559-615, per TS candidate there; per ensemble here) -------------------
MAX_CONSTRAINT_PAIRS = 64               # TOR_MAX_EXTRA (csrc/torsions.hpp)
HB_MODE_ALL, HB_MODE_LINK = 0, 1        # keep_hb=True / keep_hb=False (include/tscode_hip.h, tsc_hbonds)
AUGMENTATION_TABLE_BYTES = 1 << 30      # angle tables one csearch_candidates_multi call of csearch_augmentation_batch may hold
_CLASS_CACHE, _CLASS_CACHE_MAX = {}, 4096


def _constraint_pairs(constrained_indices, S, n):
    """i32[S, E, 2], -1 for an unused slot, from None, one (E, 2) list shared by all structures, an (S, E, 2) array or a list of S
    lists of pairs of different lengths (Embedder.constrained_indices).  ValueError on anything else."""
    if constrained_indices is None:
        return np.full((S, 0, 2), -1, dtype=np.int32)
    try:
        arr = np.asarray(constrained_indices)
        ragged = arr.dtype == object
    except ValueError:
        ragged = True
    if ragged:
        rows = [np.asarray(c).reshape(-1, 2) for c in constrained_indices]
        if len(rows) != S:
            raise ValueError(f"constraint pairs for {len(rows)} structures, {S} structures")
        arr = np.full((S, max((len(r) for r in rows), default=0), 2), -1, dtype=np.int64)
        for s, r in enumerate(rows):
            if r.size and not np.issubdtype(r.dtype, np.integer):
                raise ValueError("constraint pairs must be integers")
            arr[s, :len(r)] = r
    elif arr.size == 0:
        return np.full((S, 0, 2), -1, dtype=np.int32)
    elif not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("constraint pairs must be integers")
    elif arr.ndim == 2 and arr.shape[1] == 2:
        arr = np.broadcast_to(arr, (S,) + arr.shape)
    elif arr.ndim != 3 or arr.shape[0] != S or arr.shape[2] != 2:
        raise ValueError(f"constraint pairs of shape {arr.shape}: expected (E, 2) or ({S}, E, 2)")
    if arr.shape[1] > MAX_CONSTRAINT_PAIRS:
        raise ValueError(f"{arr.shape[1]} constraint pairs per structure: the engine takes at most {MAX_CONSTRAINT_PAIRS}")
    if arr.size and (arr.min() < -1 or arr.max() >= n):
        raise ValueError(f"constraint atom index outside -1 .. {n - 1}")
    return np.ascontiguousarray(arr, dtype=np.int32)


def _check_search_args(structures, atomnos, constrained_indices, d_min, d_max, max_angle):
    from .graph_manipulations import _atomnos_array, _structures_array
    z = _atomnos_array(atomnos)
    x = _structures_array(structures, len(z))
    extra = _constraint_pairs(constrained_indices, len(x), len(z))
    d_min, d_max, max_angle = float(d_min), float(d_max), float(max_angle)
    if not (np.isfinite(d_min) and np.isfinite(d_max) and np.isfinite(max_angle)):
        raise ValueError("d_min, d_max and max_angle must be finite")
    if not d_min < d_max:
        raise ValueError(f"d_min {d_min} is not below d_max {d_max}")
    return x, z, extra, d_min, d_max, max_angle


def _search_graphs(x, z, extra, keep_hb, d_min, d_max, max_angle, want_double=False, timings=None):
    """Bonds (tsc_bond_delta_dev), hydrogen bonds and the search graph (tsc_hbonds_dev) of every structure, the coordinates and the
    bond bits resident on the device in between.  Returns a namespace: hb (list of i32[K, 2]), segmented bool[S], bonds / graph
    u64[S, n, W] and, with want_double, double u64[S, n, W]."""
    import types

    from .graph_manipulations import bond_tables, double_bond_tables
    S, n = x.shape[:2]
    W = (n + 63) // 64
    out = types.SimpleNamespace(hb=[np.zeros((0, 2), np.int32)] * S, segmented=np.zeros(S, bool), bonds=np.zeros((S, n, W), np.uint64),
                                graph=np.zeros((S, n, W), np.uint64), double=np.zeros((S, n, W), np.uint64) if want_double else None)
    if S == 0:
        return out
    classes, thr = bond_tables(z)
    hetero, hydrogen = ((z == 7) | (z == 8)).astype(np.uint8), (z == 1).astype(np.uint8)
    n_extra = extra.shape[1]
    eng = get_engine()
    held = []

    def room(nbytes):
        held.append(eng.dev_alloc(max(int(nbytes), 1)))
        return held[-1]

    try:
        held.append(eng.dev_upload(x))
        d_x = held[-1]
        d_extra = None
        if n_extra:
            held.append(eng.dev_upload(extra))
            d_extra = held[-1]
        d_mask, d_bonds, d_graph = room(S), room(S * n * W * 8), room(S * n * W * 8)
        d_nhb, d_status = room(S * 4), room(S)
        eng.bond_delta_dev(d_x, S, n, classes, thr, None, None, None, False, 0, d_mask, adj=d_bonds)
        if timings is not None:
            timings["bond_delta_ms"] = eng.topology_kernel_ms()
        n_hb, max_hb = np.zeros(S, np.int32), 8
        while True:                                                          # (again with more slots where a structure overflowed)
            d_hb = room(S * max_hb * 8)
            eng.hbonds_dev(d_x, S, n, hetero, hydrogen, d_bonds, d_extra, n_extra, d_min, d_max, max_angle,
                           HB_MODE_ALL if keep_hb else HB_MODE_LINK, max_hb, d_hb, d_nhb, d_status, None, d_graph)
            if timings is not None:
                timings["hbonds_ms"] = eng.torsions_kernel_ms()[0]
            eng.dev_download(d_nhb, n_hb)
            if n_hb.max() <= max_hb:
                break
            max_hb = int(n_hb.max())
        hb = eng.dev_download(d_hb, np.empty((S, max_hb, 2), np.int32))
        status = eng.dev_download(d_status, np.empty(S, np.uint8))
        eng.dev_download(d_bonds, out.bonds), eng.dev_download(d_graph, out.graph)
        if want_double:
            dcl, dthr, heavy = double_bond_tables(z)
            eng.bond_delta_dev(d_x, S, n, dcl, dthr, heavy.astype(np.uint8), None, None, False, 0, d_mask, adj=d_bonds)
            eng.dev_download(d_bonds, out.double)
        if timings is not None:
            timings["bytes_up"] = x.nbytes + extra.nbytes
            timings["bytes_down"] = n_hb.nbytes + hb.nbytes + status.nbytes + out.bonds.nbytes + out.graph.nbytes + (out.double.nbytes if want_double else 0)
    finally:
        for a in held:
            eng.dev_free(a)
    out.hb = [np.ascontiguousarray(hb[s, :n_hb[s]]) for s in range(S)]
    out.segmented = status != 0
    return out


def hydrogen_bonds_batch(structures, atomnos, constrained_indices=None, keep_hb=True, d_min=2.5, d_max=3.3, max_angle=45):
    """_get_hydrogen_bonds (tscode/torsion_module.py:233-299) as csearch calls it (:559-606), for every structure at once:
    ``(hydrogen_bonds, segmented)`` -- per structure an ``int32[K, 2]`` array of sorted pairs in the reference's list order, and
    ``bool[S]``, True where the reference raises SegmentedGraphError.  ``constrained_indices``: None, one (E, 2) list shared by
    all structures, or one list per structure; the pairs are edges of the graph the neighbour lists are read from.
    ``keep_hb=False`` looks for pairs only where that graph is segmented, and only across its pieces (:593)."""
    x, z, extra, d_min, d_max, max_angle = _check_search_args(structures, atomnos, constrained_indices, d_min, d_max, max_angle)
    r = _search_graphs(x, z, extra, bool(keep_hb), d_min, d_max, max_angle)
    return r.hb, r.segmented


# -- the class graph and its candidate torsions: host code, once per topology class
def _nb(graph, i):
    """neighbors (tscode/graph_manipulations.py:57-62): the adjacency of i in the graph's own order, the self loop left out."""
    return [j for j in graph[i] if j != i]


def class_graph(atomnos, bonds, constraint_pairs=(), hydrogen_bonds=()):
    """The search graph of csearch (:559-569) for one topology class: graphize's graph -- nodes 0 .. n-1, a self loop per atom,
    the bonds by i then j (tscode/graph_manipulations.py:33-55) -- then the constraint pairs, then the hydrogen bonds.  The order
    matters: it is the order of every neighbour list, hence of the candidate quadruplets."""
    import networkx as nx
    graph = nx.Graph()
    graph.add_nodes_from(range(len(atomnos)))
    for i in range(len(atomnos)):
        graph.add_edge(i, i)
    for a, b in sorted((int(min(a, b)), int(max(a, b))) for a, b in bonds):
        graph.add_edge(a, b)
    for a, b in constraint_pairs:
        if a >= 0 and b >= 0:
            graph.add_edge(int(a), int(b))
    for a, b in hydrogen_bonds:
        graph.add_edge(int(a), int(b))
    nx.set_node_attributes(graph, {i: int(z) for i, z in enumerate(atomnos)}, "atomnos")
    return graph


def candidate_quadruplets(graph, double_bonds=()):
    """_get_quadruplets (:327-350) without the central bonds that are double bonds (:362): start atoms ascending, the depth-3
    walk in adjacency order, the first path per unordered central bond.  The walk is findPaths' as written
    (tscode/graph_manipulations.py:212-229): the atoms of the path so far are excluded, and so is every atom a path of this start
    atom has already ENDED on -- the reference adds the last atom of a path to its exclusion set and never takes it out again, so
    later paths from the same start neither pass through nor end on it.  Reproduced as it is."""
    double = {(int(min(a, b)), int(max(a, b))) for a, b in double_bonds}
    adj = {i: list(graph[i]) for i in graph}
    seen, out = set(), []
    for a in graph:
        excluded = {a}
        for b in adj[a]:
            if b in excluded:
                continue
            excluded.add(b)
            for c in adj[b]:
                if c in excluded:
                    continue
                excluded.add(c)
                for d in adj[c]:
                    if d in excluded:
                        continue
                    excluded.add(d)
                    key = (min(b, c), max(b, c))
                    if key not in seen:
                        seen.add(key)
                        if key not in double:
                            out.append((a, b, c, d))
                excluded.remove(c)
            excluded.remove(b)
    return np.array(out, dtype=np.int32).reshape(-1, 4)


def _sp_n(graph, i):
    """get_sp_n (tscode/graph_manipulations.py:73-94).  As in the reference a nitrogen with three neighbours has none."""
    table = {6: {2: 1, 3: 2, 4: 3}, 7: {2: 2, 3: None, 4: 3}, 8: {1: 2, 2: 3, 3: 3, 4: 3}, 15: {2: 2, 3: 3, 4: 3}, 16: {2: 2, 3: 3, 4: 3}}
    z = graph.nodes[i]["atomnos"]
    return table[z].get(len(_nb(graph, i))) if z in table else None


def _amide_n(graph, i, n_hydrogens):
    """is_amide_n (:96-131) with mode 1 (n_hydrogens=1, CONHR) or mode 2 (n_hydrogens=0, CONR2): a nitrogen with that many
    hydrogens next to it and a carbon neighbour that has three neighbours, one of them an oxygen."""
    z = lambda j: graph.nodes[j]["atomnos"]
    if z(i) != 7:
        return False
    nb = _nb(graph, i)
    if sum(z(j) == 1 for j in nb) != n_hydrogens:
        return False
    for c in nb:
        if z(c) == 6:
            around = _nb(graph, c)
            if len(around) == 3 and any(z(j) == 8 for j in around):
                return True
    return False


def _ester_o(graph, i):
    """is_ester_o (:133-150), with its quirk: the test that is meant to rule carboxylic acids out asks whether atom INDEX 1 is a
    neighbour (``1 not in nb``), not whether a hydrogen is.  Reproduced as it is."""
    z = lambda j: graph.nodes[j]["atomnos"]
    if z(i) != 8:
        return False
    nb = _nb(graph, i)
    if 1 in nb:
        return False
    for c in nb:
        if z(c) == 6:
            around = _nb(graph, c)
            if len(around) == 3 and sum(z(j) == 8 for j in around) > 1:
                return True
    return False


def _free(graph, i):
    """_is_free (:134-156): not an sp2 carbon next to an oxygen, not the nitrogen of a secondary amide, not an ester oxygen."""
    z = lambda j: graph.nodes[j]["atomnos"]
    if z(i) == 6 and _sp_n(graph, i) == 2 and any(z(j) == 8 for j in _nb(graph, i)):
        return False
    return not _amide_n(graph, i, 1) and not _ester_o(graph, i)


def _phenyl_ids(graph, i):
    """_get_phenyl_ids (tscode/graph_manipulations.py:197-210): the first simple path of six heavy atoms with three neighbours
    each from i to one of its neighbours."""
    import networkx as nx
    for nbr in _nb(graph, i):
        for path in nx.all_simple_paths(graph, source=i, target=nbr, cutoff=6):
            if len(path) == 6 and all(graph.nodes[j]["atomnos"] != 1 for j in path) and all(len(_nb(graph, j)) == 3 for j in path):
                return path
    return None


def _nondummy(graph, i, root):
    """_is_nondummy (:158-231): turning about root - i changes something, i.e. the substituents of i away from root are not all
    alike (methyl, CF3, tBu, a symmetric phenyl: dummy).  Only carbon and nitrogen are looked at."""
    import copy

    import networkx as nx
    if graph.nodes[i]["atomnos"] not in (6, 7):
        return True
    same = lambda p, q: p["atomnos"] == q["atomnos"]
    g = copy.deepcopy(graph)
    nb = _nb(g, i)
    nb.remove(root)
    if len(nb) == 1 and len(_nb(g, nb[0])) == 2:
        return False
    if len(nb) == 2:
        ring = _phenyl_ids(g, i)
        if ring is not None:
            r1, r2, r3, r4, r5, r6 = ring
            for a, b in ((r3, r4), (r4, r5), (r1, r2), (r1, r6)):
                g.remove_edge(a, b)
            halves = [nx.subgraph(g, c) for c in nx.connected_components(g) if r2 in c or r6 in c]
            if len(halves) == 2:
                return not nx.is_isomorphic(halves[0], halves[1], node_match=same)
            return True
    for j in nb:
        g.remove_edge(i, j)
    parts = [c for c in nx.connected_components(g) if root not in c]
    if len(parts) == 1:
        return True
    subs = [nx.subgraph(g, c) for c in parts]
    return any(not nx.is_isomorphic(subs[0], other, node_match=same) for other in subs[1:])


def _n_fold(graph, i2, i3):
    """Torsion.get_n_fold (:86-110)."""
    nums = (graph.nodes[i2]["atomnos"], graph.nodes[i3]["atomnos"])
    if 1 in nums:
        return 6
    if _amide_n(graph, i2, 0) or _amide_n(graph, i3, 0):
        return 2
    if 6 in nums or 7 in nums or 16 in nums:
        sp = (_sp_n(graph, i2), _sp_n(graph, i3))
        if 3 in sp:
            return 3
        if 2 in sp:
            return 2
    return 4


def rotatable_torsions(graph, candidates, in_cycle, hydrogen_bonds=()):
    """Which candidates _get_torsions keeps (:352-371, keepdummy=False) and their fold: ``(rows, n_folds)``.  ``in_cycle`` bool[T]
    comes from the reachability kernel.  The rules are Torsion.is_rotable's (:63-84): a central bond that is listed as a hydrogen
    bond is never rotatable (the reference's own choice, :68-72); one end must be free and both ends non-dummy.
    Like the reference's in_cycle, every candidate takes its central bond out of the graph and puts it back, which moves the two
    atoms to the end of each other's neighbour list: the lists the later rules read are the reference's."""
    hb = {(int(min(a, b)), int(max(a, b))) for a, b in hydrogen_bonds}
    rows, folds = [], []
    for k, (i1, i2, i3, i4) in enumerate(np.asarray(candidates).reshape(-1, 4).tolist()):
        graph.remove_edge(i2, i3)
        graph.add_edge(i2, i3)
        if in_cycle[k] or (min(i2, i3), max(i2, i3)) in hb:
            continue
        if (_free(graph, i2) or _free(graph, i3)) and _nondummy(graph, i2, i3) and _nondummy(graph, i3, i2):
            rows.append(k)
            folds.append(_n_fold(graph, i2, i3))
    return np.array(rows, dtype=np.int64), np.array(folds, dtype=np.int32)


def _oriented_set(candidates, flags, masks, rows, folds):
    tors = candidates[rows].copy()
    flip = (flags[rows] & 2) != 0
    tors[flip] = tors[flip][:, ::-1]
    return np.ascontiguousarray(tors), np.ascontiguousarray(masks.reshape(len(candidates), -1)[rows]), folds


def class_torsion_set(graph, candidates, flags, masks, hydrogen_bonds=()):
    """One class's ``(torsions i32[T, 4] oriented, masks u8[T, n], n_folds i32[T])`` from its candidates and the answers of
    tsc_torsion_reach: flags bit 0 in_cycle, bit 1 reversed (Torsion.sort_torsion, :120-132), masks as _get_rotation_mask
    (:301-325) of the oriented tuple.  ``graph`` is a fresh class_graph: the rules reorder its neighbour lists as they go."""
    candidates = np.asarray(candidates, dtype=np.int32).reshape(-1, 4)
    flags = np.asarray(flags, dtype=np.uint8)
    rows, folds = rotatable_torsions(graph, candidates, (flags & 1) != 0, hydrogen_bonds)
    return _oriented_set(candidates, flags, np.asarray(masks, dtype=np.uint8), rows, folds)


def torsion_sets_batch(structures, atomnos, constrained_indices=None, keep_hb=True, timings=None):
    """What csearch sets up per TS candidate (tscode/torsion_module.py:559-615) for a whole ensemble: bonds, hydrogen bonds and the
    segmentation verdict per structure on the GPU, then one torsion set per TOPOLOGY CLASS -- the structures that share bond bits,
    double-bond bits, the ordered constraint list and the ordered hydrogen-bond list.  Returns a namespace with

    * ``set_of_structure`` i32[S]: the structure's set, -1 where ``segmented``;
    * ``segmented`` bool[S]; ``hydrogen_bonds``: per structure int32[K, 2];
    * ``sets[k] = (torsions i32[T_k, 4], masks u8[T_k, n], n_folds i32[T_k])``: _get_torsions after sort_torsion, the
      _get_rotation_mask of each, and Torsion.n_fold -- ready for csearch_candidates_multi once an angle table is added.

    No TSCoDe import: the rotatability rules are restated here on the class graph (networkx does the isomorphism tests)."""
    import time
    import types

    from .graph_manipulations import edges_from_bits
    x, z, extra, d_min, d_max, max_angle = _check_search_args(structures, atomnos, constrained_indices, 2.5, 3.3, 45)
    S, n = x.shape[:2]
    r = _search_graphs(x, z, extra, bool(keep_hb), d_min, d_max, max_angle, want_double=True, timings=timings)
    t0 = time.perf_counter()
    set_of = np.full(S, -1, dtype=np.int32)
    keys, members = {}, []
    for s in np.flatnonzero(~r.segmented):
        key = (z.tobytes(), r.bonds[s].tobytes(), r.double[s].tobytes(), extra[s].tobytes(), r.hb[s].tobytes())
        k = keys.setdefault(key, len(members))
        if k == len(members):
            members.append(int(s))
        set_of[s] = k
    t1 = time.perf_counter()
    # per class, cached: the candidates, and the rows and folds the rules gave for these in_cycle answers
    key_list, graphs, cands = list(keys), [], []
    for key, s in zip(key_list, members):
        hit = _CLASS_CACHE.get(key)
        if hit is None:
            graphs.append(class_graph(z, edges_from_bits(r.bonds[s]), extra[s], r.hb[s]))
            cands.append(candidate_quadruplets(graphs[-1], edges_from_bits(r.double[s])))
        else:
            graphs.append(None), cands.append(hit[0])
    t2 = time.perf_counter()
    sets = []
    t2b = t2
    if members:
        set_off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int32)
        flags, masks = get_engine().torsion_reach(r.graph[members], np.concatenate(cands), set_off, extra[members].reshape(len(members), -1))
        if timings is not None:
            timings["reach_ms"] = get_engine().torsions_kernel_ms()[1]
            timings["bytes_up"] += r.graph[members].nbytes + 16 * int(set_off[-1])
            timings["bytes_down"] += flags.nbytes + masks.nbytes
        t2b = time.perf_counter()
        for k, (key, s) in enumerate(zip(key_list, members)):
            f, m = flags[set_off[k]:set_off[k + 1]], masks[set_off[k]:set_off[k + 1]]
            cyc = ((f & 1) != 0).tobytes()
            hit = _CLASS_CACHE.get(key)
            if hit is None or hit[1] != cyc:
                g = graphs[k] if graphs[k] is not None else class_graph(z, edges_from_bits(r.bonds[s]), extra[s], r.hb[s])
                hit = (cands[k], cyc) + rotatable_torsions(g, cands[k], (f & 1) != 0, r.hb[s])
                if len(_CLASS_CACHE) >= _CLASS_CACHE_MAX:
                    _CLASS_CACHE.clear()
                _CLASS_CACHE[key] = hit
            sets.append(_oriented_set(cands[k], f, m, hit[2], hit[3]))
    t3 = time.perf_counter()
    if timings is not None:
        timings.update(n_classes=len(members), grouping_ms=1e3 * (t1 - t0), quadruplets_ms=1e3 * (t2 - t1), chemistry_ms=1e3 * (t3 - t2b))
    return types.SimpleNamespace(set_of_structure=set_of, segmented=r.segmented, hydrogen_bonds=r.hb, sets=sets, constraint_pairs=extra)


def csearch_augmentation_batch(structures, atomnos, constrained_indices, n_out=100, max_tries=10000, keep_hb=True, max_structs=None,
                               timings=None):
    """The loop of Embedder.csearch_augmentation (tscode/embedder.py:1907-1939) without the energy bookkeeping:
    ``(new_structures [K, n, 3], start_index [K])``, structure after structure what ``csearch(structure, atomnos,
    constrained_indices[s], keep_hb=True, mode=2, n_out=n_out)`` returns -- nothing for a segmented structure (:1930), the
    structure itself where no bond is rotatable (tscode/torsion_module.py:619-621), else the candidates of random_csearch.  With
    ``max_structs``, ``n_out`` follows :1904-1905.  The angle table of a structure with torsions is ``cartesian_product`` of its
    n-fold angles shuffled with ``np.random.shuffle`` -- exactly one shuffle per such structure, in order, so a caller who seeds
    ``np.random`` gets the reference's tables.  The rotations are csearch_candidates_multi calls with one set per structure, as
    many structures per call as keep its tables under ``AUGMENTATION_TABLE_BYTES``."""
    import time

    from .utils import cartesian_product
    ts = torsion_sets_batch(structures, atomnos, constrained_indices, keep_hb, timings=timings)
    x = np.ascontiguousarray(structures, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    S, n = x.shape[:2]
    if max_structs is not None:
        n_out = 100 if S * 100 < max_structs else round(max_structs / S)            # embedder.py:1904-1905
        n_out = max((1, n_out))
    t0 = time.perf_counter()
    pieces = [None] * S
    batch, batch_bytes = [], 0

    def flush():
        nonlocal batch, batch_bytes
        if batch:
            rows, start = csearch_candidates_multi(x[[s for s, _ in batch]], [st for _, st in batch], None, n_out=n_out, max_tries=max_tries)
            for local, (s, _) in enumerate(batch):
                pieces[s] = rows[start == local]
        batch, batch_bytes = [], 0

    tables_s = 0.0
    for s in range(S):
        if ts.segmented[s]:
            pieces[s] = np.zeros((0, n, 3))
            continue
        tors, masks, folds = ts.sets[ts.set_of_structure[s]]
        if not len(tors):
            pieces[s] = x[s][None]
            continue
        t1 = time.perf_counter()
        table = cartesian_product(*[N_FOLD_ANGLES[int(f)] for f in folds])            # tscode/torsion_module.py:453
        np.random.shuffle(table)                                                      # :460
        tables_s += time.perf_counter() - t1
        if batch and batch_bytes + table.nbytes > AUGMENTATION_TABLE_BYTES:
            flush()
        batch.append((s, (tors, masks, table)))
        batch_bytes += table.nbytes
    flush()
    if timings is not None:
        timings["tables_ms"] = 1e3 * tables_s
        timings["augmentation_host_ms"] = 1e3 * (time.perf_counter() - t0)
    counts = [len(p) for p in pieces]
    out = np.concatenate(pieces) if pieces else np.zeros((0, n, 3))
    return out, np.repeat(np.arange(S, dtype=np.int32), counts)


# ---- the clustered search (tscode/torsion_module.py:373-397, :655-847, per TS candidate there; per ensemble here) ----------------------
MAX_GROUP_TORSIONS = 512                # GRP_MAX_TORSIONS (csrc/torsions.hpp)
MIN_TORSIONS_TO_GROUP = 9               # :689
_csearch_originals = {}                 # what install(csearch=True) replaced: the drop-ins hand over what they do not cover


def _set_torsions(st):
    """The [T, 4] indices of a torsion set given as ``(torsions, masks, n_folds)`` (torsion_sets_batch) or as the indices alone."""
    t = st[0] if isinstance(st, tuple) else st
    return np.asarray(t, dtype=np.int32).reshape(-1, 4)


def group_torsions_batch(structures, torsion_sets, set_of_structure=None, max_size=5):
    """_group_torsions_dbscan (tscode/torsion_module.py:373-397) with the ``len(torsions) < 9`` branch of clustered_csearch (:689) for
    every structure at once (tsc_torsion_groups): ``(groups, eps_index i32[S], oversize bool[S])``.  ``groups[s]`` is a list of index
    arrays into structure s's torsion set, in the reference's group order (size ascending, ties by first member) and ascending
    inside a group.  ``torsion_sets``: ``(torsions, masks, n_folds)`` tuples as torsion_sets_batch returns them, or ``[T, 4]`` index
    arrays; structure s uses set ``set_of_structure[s]`` (default: the only set, or set s when there are S of them; -1: no
    torsions, no groups).  ``eps_index``: the position of the level kept in 10.0, 9.5, ..., 2.0, -1 where the set was not
    clustered; ``oversize``: no level gave groups of at most ``max_size``, and the groups of the last one stand."""
    x = np.ascontiguousarray(structures, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 3 or not 1 <= x.shape[1] <= 512:
        raise ValueError(f"structures of shape {x.shape}: expected (n_structures, 1 .. 512 atoms, 3)")
    if not np.isfinite(x).all():
        raise ValueError("structures contain NaN or infinity")
    S, n = x.shape[:2]
    if int(max_size) != max_size or max_size < 1:
        raise ValueError("max_size must be a positive integer")
    tors = [_set_torsions(st) for st in torsion_sets]
    if set_of_structure is None:
        if len(tors) == 1:
            set_of_structure = np.zeros(S, dtype=np.int64)
        elif len(tors) == S:
            set_of_structure = np.arange(S)
        else:
            raise ValueError(f"{len(tors)} torsion sets for {S} structures: set_of_structure is needed")
    set_of = np.asarray(set_of_structure, dtype=np.int64).ravel()
    if len(set_of) != S or (S and (set_of.min() < -1 or set_of.max() >= len(tors))):
        raise ValueError(f"set_of_structure: expected {S} set indices in [-1, {len(tors)})")
    for k, t in enumerate(tors):
        if len(t) > MAX_GROUP_TORSIONS:
            raise ValueError(f"torsion set {k}: {len(t)} torsions, the engine groups at most {MAX_GROUP_TORSIONS}")
        if len(t) and (t.min() < 0 or t.max() >= n):
            raise ValueError(f"torsion set {k}: atom index out of range")
    counts = np.array([len(tors[k]) if k >= 0 else 0 for k in set_of], dtype=np.int64)
    if counts.sum() >= 2**31:
        raise ValueError("2^31 torsions or more in one call")
    set_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    eps_index, oversize = np.full(S, -1, dtype=np.int32), np.zeros(S, dtype=bool)
    if counts.sum() == 0:
        return [[] for _ in range(S)], eps_index, oversize
    flat = np.concatenate([tors[k] for k in set_of if k >= 0])
    group_of, n_groups, eps_index, over = get_engine().torsion_groups(x, flat, set_off, int(max_size), MIN_TORSIONS_TO_GROUP)
    groups = []
    for s in range(S):
        g = group_of[set_off[s]:set_off[s + 1]]
        groups.append([np.flatnonzero(g == k) for k in range(n_groups[s])] if counts[s] else [])
    return groups, eps_index, over != 0


# Structures in a slice of a round from which its trims and finals go through the batched calls (close_slice).  Measured (MEASURED.md
# section 20): with one structure the batched calls hand over to the single ones and cost 3 % on top (7.40 against 7.21 ms); from two
# structures on the batch route is ahead by more than the spread of the runs (14.4 against 17.0 ms at 2, 39.7 against 96.3 at 16).
CLUSTERED_BATCH_MIN_POSES = 2


def _trim_seed(seed, coords, call):
    """The k-means seed of most_diverse_conformers call ``call`` of the search that starts from ``coords``: drawn from
    ``np.random.default_rng`` seeded with the caller's seed, the call's number and a checksum of the start structure's own bytes --
    not its position -- so that a structure gets the same rows alone, inside an ensemble, and however the ensemble is sliced."""
    import zlib
    return int(np.random.default_rng([int(seed), zlib.crc32(np.ascontiguousarray(coords).tobytes()), int(call)]).integers(2**31 - 1))


def _clustered_rounds(x, search, n, n_out, seed, init_rows, log=None, timings=None):
    """Rounds :722-840 for the structures ``search = {s: (torsions i32[T, 4], masks u8[T, n_atoms], n_folds i32[T], groups)}`` of
    ``x``.  Returns ({s: output structures}, {s: [(generated, kept) per round]})."""
    import time

    from .numba_functions import prune_conformers_tfd, prune_conformers_tfd_batch
    from .utils import cartesian_product
    init_rows = {} if init_rows is None else init_rows
    n_atoms = x.shape[1]
    starts = {s: x[s][None] for s in search}
    output = {s: [] for s in search}
    calls = {s: 0 for s in search}
    sizes = {s: [] for s in search}
    final = {}
    rot_ms, trim_ms, final_ms = [], [], 0.0

    def next_call(s):
        """(seed, rows) of the next most_diverse_conformers call of structure s."""
        c = calls[s]
        calls[s] += 1
        rows = init_rows.get((s, c))
        return (None if rows is not None or seed is None else _trim_seed(seed, x[s], c)), rows

    def pick(s, k, structures, torsion_array):
        sd, rows = next_call(s)
        return most_diverse_conformers(k, structures, torsion_array, seed=sd, init_rows=rows)

    def pick_batch(members, k, structures, torsion_arrays):
        """pick() for the structures ``members`` in ONE most_diverse_conformers_batch call, each with its own (structure, call) seed or rows."""
        args = [next_call(s) for s in members]
        return most_diverse_conformers_batch(k, structures, torsion_arrays, seeds=[a[0] for a in args], init_rows=[a[1] for a in args])

    def close_round(s, g, new):
        """What follows the candidate loop of group g of structure s (:783-840), as soon as its rows are complete."""
        nonlocal final_ms
        tors, _, _, groups = search[s]
        t0 = time.perf_counter()
        generated = len(new)
        last = g + 1 == len(groups)
        if not last and n is not None and generated > n:                                   # :809-819
            new = pick(s, n, new, tors)
        sizes[s].append((generated, len(new)))
        if log and not last:
            log(s, f"  Group {g + 1}/{len(groups)}: {generated} structures built, kept the most diverse {len(new)} as starting points for the next group")
        if not last:
            new = np.array(new)                                                            # (its own memory: not a window into the call's rows)
            output[s].append(new)                                                           # :823
            starts[s] = new
        t1 = time.perf_counter()
        trim_ms[-1] += 1e3 * (t1 - t0)
        if last:
            out = np.concatenate(output.pop(s) + [new])                                     # :823, :826
            out, _ = prune_conformers_tfd(out, tors)                                        # :827
            if generated > n_out:                                                           # :829: the LAST ROUND's count, not the output's
                out = pick(s, n_out, out, tors)
            final[s] = np.asarray(out)
            del starts[s]
            final_ms += 1e3 * (time.perf_counter() - t1)

    def close_slice(part, g, news):
        """close_round for all structures of a slice at once: the trims in one most_diverse_conformers_batch call, the finals that
        close here in one prune_conformers_tfd_batch plus one most_diverse_conformers_batch call.  Every structure keeps the seeds and
        rows pick() gives it; with neither seed nor rows the np.random draws of a slice's trims come before those of its finals."""
        nonlocal final_ms
        t0 = time.perf_counter()
        generated = [len(new) for new in news]
        lasts = [g + 1 == len(search[s][3]) for s in part]
        trim = [i for i in range(len(part)) if not lasts[i] and n is not None and generated[i] > n]      # :809-819
        if trim:
            for i, new in zip(trim, pick_batch([part[i] for i in trim], n, [news[i] for i in trim], [search[part[i]][0] for i in trim])):
                news[i] = new
        for i, s in enumerate(part):
            sizes[s].append((generated[i], len(news[i])))
            if not lasts[i]:
                if log:
                    n_groups = len(search[s][3])
                    log(s, f"  Group {g + 1}/{n_groups}: {generated[i]} structures built, kept the most diverse {len(news[i])} as starting points for the next group")
                new = np.array(news[i])
                output[s].append(new)                                                           # :823
                starts[s] = new
        t1 = time.perf_counter()
        trim_ms[-1] += 1e3 * (t1 - t0)
        fin = [i for i in range(len(part)) if lasts[i]]
        if fin:
            tors = [search[part[i]][0] for i in fin]
            outs = [np.concatenate(output.pop(part[i]) + [news[i]]) for i in fin]               # :823, :826
            outs = [kept for kept, _ in prune_conformers_tfd_batch(outs, tors)]                 # :827
            again = [j for j, i in enumerate(fin) if generated[i] > n_out]                      # :829: the LAST ROUND's count, not the output's
            if again:
                for j, out in zip(again, pick_batch([part[fin[j]] for j in again], n_out, [outs[j] for j in again], [tors[j] for j in again])):
                    outs[j] = out
            for j, i in enumerate(fin):
                final[part[i]] = np.asarray(outs[j])
                del starts[part[i]]
            final_ms += 1e3 * (time.perf_counter() - t1)

    g = 0
    while starts:
        live = [s for s in search if s in starts]
        rot_ms.append(0.0), trim_ms.append(0.0)
        # a round is ONE candidate call, unless its candidates would exceed a launch slice: then one call per slice of structures
        at = 0
        while at < len(live):
            part, part_bytes = [], 0
            sets, set_index, set_of_start = [], {}, []
            while at < len(live):
                s = live[at]
                tors, masks, folds, groups = search[s]
                idx = groups[g]
                key = (tors[idx].tobytes(), masks[idx].tobytes(), folds[idx].tobytes())
                table_rows = int(np.prod([len(N_FOLD_ANGLES[int(f)]) for f in folds[idx]]))
                need = len(starts[s]) * (table_rows + 1) * n_atoms * 24
                if part and part_bytes + need > MULTI_SCRATCH_BYTES:
                    break
                if key not in set_index:
                    set_index[key] = len(sets)
                    sets.append((tors[idx], masks[idx], cartesian_product(*[N_FOLD_ANGLES[int(f)] for f in folds[idx]])))   # :726
                if log:
                    log(s, f"\n> Group {g + 1}/{len(groups)}: {len(idx)} bonds, n-folds {folds[idx].tolist()}, {len(starts[s])} "
                           f"starting point{'s' if len(starts[s]) > 1 else ''} = {table_rows * len(starts[s])} conformers")
                set_of_start += [set_index[key]] * len(starts[s])
                part.append(s)
                at += 1
                part_bytes += need
            t0 = time.perf_counter()
            rows, start_index = csearch_candidates_multi(np.concatenate([starts[s] for s in part]), sets, set_of_start, n_out=None,
                                                         include_start=True)
            rot_ms[-1] += 1e3 * (time.perf_counter() - t0)
            bounds = np.searchsorted(start_index, np.cumsum([0] + [len(starts[s]) for s in part]))
            if len(part) >= CLUSTERED_BATCH_MIN_POSES:
                close_slice(part, g, [rows[bounds[k]:bounds[k + 1]] for k in range(len(part))])
            else:
                for k, s in enumerate(part):
                    close_round(s, g, rows[bounds[k]:bounds[k + 1]])
            del rows
        g += 1
    if timings is not None:
        timings.update(rotation_ms=rot_ms, trim_ms=trim_ms, final_ms=final_ms)
    return final, sizes


def clustered_csearch_batch(structures, atomnos, constrained_indices=None, keep_hb=False, n=100, n_out=100, max_size=5, seed=None,
                            init_rows=None, info=None, timings=None):
    """clustered_csearch mode 1 (tscode/torsion_module.py:655-847) as csearch reaches it (:523-640), for every structure of an
    ensemble: ``(new_structures [K, n_atoms, 3], start_index [K])``, shaped like csearch_augmentation_batch's.

    * Set-up: torsion_sets_batch.  A segmented structure contributes no rows (``info["segmented"]``), one without rotatable bonds
      contributes itself (:619-621).
    * Groups: group_torsions_batch on each structure's own coordinates -- two poses of one topology class may group differently.
    * Round g: ONE csearch_candidates_multi(..., n_out=None, include_start=True) call with the current starting points of every
      structure that still has a group g, each start carrying its structure's set for that group; the table is cartesian_product
      of the group's n-fold angles, not shuffled (:726).  Where the candidates of a round would take more than MULTI_SCRATCH_BYTES
      the round is split into one call per slice of structures, so the host never holds more than one slice of candidates plus
      the kept rows: a structure's round is closed as soon as its rows are there.
    * Between groups, per structure: ``most_diverse_conformers(n, new_structures, torsion_array)`` iff this is not the last group
      and there are more than ``n`` (:809-819); the next round starts from the ALIGNED coordinates it returns, as in the reference.
      Every round's (trimmed) structures go to the output, the repeated starting points too (:823).
    * After the last group: prune_conformers_tfd on the output, then ``most_diverse_conformers(n_out, ...)`` iff the LAST ROUND
      built more than ``n_out`` structures -- not the output (:829, reproduced as it is).
    * From ``CLUSTERED_BATCH_MIN_POSES`` structures in a slice on, the trims of the slice are ONE most_diverse_conformers_batch call
      and the finals that close in it ONE prune_conformers_tfd_batch plus ONE most_diverse_conformers_batch call, each structure
      with the seed or rows it would get alone: the same structures, bit for bit.  The batched calls copy what they are given
      (concatenated input, pruned and aligned rows), in uploads of at most TFD_BATCH_BYTES / DIVERSE_BATCH_BYTES: on this route
      the host holds one slice of candidates, the kept rows and those copies of the slice's trims.
    * The k-means initialisation, which the reference leaves to chance: ``init_rows`` maps ``(structure, call)`` -- the call's
      number among that structure's most_diverse_conformers calls -- to the rows to start from; otherwise, with ``seed``, each
      such call gets a seed of its own (_trim_seed) that depends on the structure's coordinates and the call, not on its place in
      the ensemble; with neither, most_diverse_conformers draws one from ``np.random``.

    ``info`` (a dict) receives ``segmented``, ``torsions``, ``n_folds``, ``groups``, ``eps_index``, ``oversize`` and ``round_sizes``
    (per structure and round: structures built, structures kept); ``timings`` the stages' milliseconds."""
    import time
    if n is not None and (int(n) != n or n < 1):
        raise ValueError("n must be a positive integer or None")
    if int(n_out) != n_out or n_out < 1:
        raise ValueError("n_out must be a positive integer")
    if int(max_size) != max_size or max_size < 1:
        raise ValueError("max_size must be a positive integer")
    if init_rows is not None and not hasattr(init_rows, "get"):
        raise ValueError("init_rows must map (structure, call) to row indices")
    t0 = time.perf_counter()
    ts = torsion_sets_batch(structures, atomnos, constrained_indices, keep_hb, timings=timings)
    if timings is not None:
        timings["setup_ms"] = 1e3 * (time.perf_counter() - t0)
    x = np.ascontiguousarray(structures, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    S, n_atoms = x.shape[:2]
    t0 = time.perf_counter()
    groups, eps_index, oversize = group_torsions_batch(x, ts.sets, ts.set_of_structure, max_size)
    if timings is not None:
        timings["groups_ms"] = 1e3 * (time.perf_counter() - t0)
        timings["groups_kernel_ms"] = get_engine().torsion_groups_kernel_ms() if any(groups) else -1.0
    search = {}
    for s in range(S):
        if not ts.segmented[s] and groups[s]:
            tors, masks, folds = ts.sets[ts.set_of_structure[s]]
            search[s] = (tors, masks, np.asarray(folds), groups[s])
    final, sizes = _clustered_rounds(x, search, n, int(n_out), seed, init_rows, timings=timings)
    pieces = []
    for s in range(S):
        if ts.segmented[s]:
            pieces.append(np.zeros((0, n_atoms, 3)))
        else:
            pieces.append(final[s] if s in final else x[s][None])                           # :619-621
    if info is not None:
        own = [ts.sets[k] if k >= 0 else None for k in ts.set_of_structure]
        info.update(segmented=ts.segmented, groups=groups, eps_index=eps_index, oversize=oversize,
                    torsions=[None if st is None else st[0] for st in own], n_folds=[None if st is None else st[2] for st in own],
                    round_sizes=[sizes.get(s, []) for s in range(S)])
    out = np.concatenate(pieces) if pieces else np.zeros((0, n_atoms, 3))
    return out, np.repeat(np.arange(S, dtype=np.int32), [len(p) for p in pieces])


def csearch_batch(structures, atomnos, constrained_indices=None, keep_hb=False, mode=1, n=100, n_out=100, **kw):
    """csearch (tscode/torsion_module.py:523-653) for an ensemble: ``(new_structures [K, n_atoms, 3], start_index [K])``.  Mode 1,
    the reference's default: clustered_csearch_batch.  Mode 2: csearch_augmentation_batch with the caller's ``n_out`` (``n`` has no
    part in it).  Mode 0 keeps the structures of lowest energy and needs an external optimiser (ff_opt): ValueError."""
    if mode == 1:
        return clustered_csearch_batch(structures, atomnos, constrained_indices, keep_hb=keep_hb, n=n, n_out=n_out, **kw)
    if mode == 2:
        return csearch_augmentation_batch(structures, atomnos, constrained_indices, n_out=n_out, keep_hb=keep_hb, **kw)
    if mode == 0:
        raise ValueError("mode 0 ranks the conformers by the energies of an external optimiser (ff_opt=True), which this package does not run")
    raise ValueError(f"mode {mode!r}: 1 (clustered, most diverse) or 2 (random rotations)")


# -- drop-ins with the reference's signatures (install(csearch=True))
def _reach_masks(graph, torsions, n_atoms):
    """_get_rotation_mask (:301-325) of every torsion, already oriented, in the caller's graph (tsc_torsion_reach, nothing constrained)."""
    from .graph_manipulations import pack_edges
    bits = pack_edges([(int(a), int(b)) for a, b in graph.edges], n_atoms)[None]
    return get_engine().torsion_reach(bits, torsions, np.array([0, len(torsions)], dtype=np.int32), None)[1]


def _group_torsions_dbscan(coords, torsions, max_size=5):
    """Drop-in for tscode.torsion_module._group_torsions_dbscan (:373-397): the torsion objects in groups, smallest group first.
    Always clusters, like the reference's function (the ``< 9`` branch is its caller's)."""
    torsions = list(torsions)
    quads = np.array([t.torsion for t in torsions], dtype=np.int32).reshape(-1, 4)
    x = np.ascontiguousarray(coords, dtype=np.float64)[None]
    if len(quads) > MAX_GROUP_TORSIONS:
        raise ValueError(f"{len(quads)} torsions, the engine groups at most {MAX_GROUP_TORSIONS}")
    if not len(quads):
        return []
    group_of, n_groups, _, _ = get_engine().torsion_groups(x, quads, np.array([0, len(quads)], dtype=np.int32), int(max_size), 0)
    return [[torsions[t] for t in np.flatnonzero(group_of == k)] for k in range(n_groups[0])]


def clustered_csearch(coords, atomnos, torsions, graph, constrained_indices=None, ff_opt=False, n=100, n_out=100, mode=1, calc=None,
                      method=None, title='test', logfunction=print, interactive_print=True, write_torsions=False, *, seed=None,
                      init_rows=None):
    """Drop-in for tscode.torsion_module.clustered_csearch (:655-847), mode 1: one structure through the rounds of
    clustered_csearch_batch.  ``torsions``: objects with ``.torsion`` (already oriented by sort_torsion) and ``.n_fold``; the
    rotation masks are read off ``graph`` on the GPU.  ``ff_opt``, ``mode == 0`` and ``write_torsions`` go to the function that
    install(csearch=True) replaced; without one that is a RuntimeError.  ``seed`` / ``init_rows`` (keys ``(0, call)``) are this
    package's additions: see clustered_csearch_batch."""
    import time
    if ff_opt or mode == 0 or write_torsions:
        original = _csearch_originals.get("clustered_csearch")
        if original is None:
            raise RuntimeError("clustered_csearch with ff_opt, mode 0 or write_torsions needs the reference's function: "
                               "tscode_amd.install(csearch=True) records it")
        return original(coords, atomnos, torsions, graph, constrained_indices=constrained_indices, ff_opt=ff_opt, n=n, n_out=n_out, mode=mode,
                        calc=calc, method=method, title=title, logfunction=logfunction, interactive_print=interactive_print,
                        write_torsions=write_torsions)
    if mode != 1:
        raise ValueError("The mode keyword can only be 0 or 1")
    t_start = time.perf_counter()
    torsions = list(torsions)
    x = np.ascontiguousarray(coords, dtype=np.float64)[None]
    n_atoms = x.shape[1]
    quads = np.array([t.torsion for t in torsions], dtype=np.int32).reshape(-1, 4)
    folds = np.array([t.n_fold for t in torsions], dtype=np.int32)
    if not len(quads):
        raise ValueError("clustered_csearch needs at least one torsion")
    groups, _, _ = group_torsions_batch(x, [quads], None, max_size=5)
    logfunction('\n> Torsion list: (indices: n-fold)')
    for i, t in enumerate(torsions):
        logfunction(f' {i} - {str(t.torsion):21s} : {t.n_fold}-fold')
    logfunction('\n> Rotable bonds ids: ' + ' '.join(str(i) for i in sorted({int(i) for q in quads for i in q[1:3]})))
    logfunction(f'\n--> Clustered CSearch on {title}\n    mode 1 (diversity) - {len(torsions)} torsions in {len(groups[0])} '
                f'group{"s" if len(groups[0]) != 1 else ""} - {[len(g) for g in groups[0]]}')
    search = {0: (quads, _reach_masks(graph, quads, n_atoms), folds, groups[0])}
    final, _ = _clustered_rounds(x, search, n, n_out, seed, init_rows, log=lambda s, text: logfunction(text))
    out = final[0]
    share = round(100 * len(out) / float(np.prod(folds.astype(np.float64))), 2)
    logfunction(f'  Selected the most diverse {len(out)} conformers, about {share} % of the total conformational space - '
                f'CSearch time {time.perf_counter() - t_start:.1f} s')
    return out
