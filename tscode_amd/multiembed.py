"""A multiembed (tscode/multiembed.py:26-148) as ONE grouped embed: every arrangement of two facing atom pairs between two molecules with
several reactive atoms each, where the reference starts one child Embedder process per arrangement.

All children embed the same two coordinate stacks; only the reactive atoms -- hence pivots, reactive coordinates and facing atoms -- differ.
So the children's group records are concatenated and handed to ``tsc_cyclical_embed_groups`` (one record per (group, molecule), one angle
table for all), and each later stage of a child (``fitness_refining``, ``similarity_refining(rmsd=False)``) is one batched call over all
arrangements.  ``multiembed_batch`` works from plain arrays; ``multiembed_bifunctional`` / ``multiembed_dispatcher`` are the drop-ins that
``tscode_amd.install(multiembed=True)`` puts in place of the reference's.
"""

from __future__ import annotations

from itertools import permutations

import numpy as np

from .embeds import DEFAULT_MAX_POSES_PER_CALL, MAX_GROUP_POSES, _bimolecular_groups, _slabs   # (the pose budget per call: see there)
from .engine import FragmentSet, get_engine
from .reactive_atoms import MAX_ATOMS, check_orbital_args, reactive_molecule
from .utils import cartesian_product

__all__ = ["multiembed_batch", "MultiembedResult", "arrangements", "multiembed_bifunctional", "multiembed_dispatcher", "DEFAULT_MAX_POSES_PER_CALL"]

_ORBITAL_KEYS = ("overrides", "orb_dim", "leaving_group", "sp_seed", "suprafacial", "sigmatropic")
_CHILD_MAX_NORM_DELTA = 5          # a child calls cyclical_embed(embedder): its default reaches the rigid shortcut (tscode/embeds.py:234-241)
_CHILD_ROTATION_RANGE, _CHILD_ROTATION_STEPS = 45, 5     # tscode/embedder_options.py:167, tscode/embedder.py:708


class MultiembedResult:
    """``structures`` f64[K, n1 + n2, 3], ``constrained_indices`` int[K, 2, 2], ``arrangement_of`` int[K] (all in arrangement order),
    ``arrangements`` int[n_arr, 2, 2] = ((ix_1, ix_2), (iy_1, iy_2)) in molecule-local indices, ``counts`` int[n_arr, 6] = candidates, clash_ok,
    kept by the group filter, fit, after TFD, after MOI.  For checking: ``clash_ok`` / ``kept`` bool[candidates], ``candidate_off``
    int[n_arr + 1], and ``masks``: ``fitness`` over the kept poses, ``tfd`` over the fit ones, ``moi`` over those TFD left, each concatenated in
    arrangement order."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def arrangements(reactive1, reactive2):
    """tscode/multiembed.py:36-39: every ordered choice of two facing pairs ``((ix_1, ix_2), (iy_1, iy_2))`` that uses no atom twice, in the
    reference's order (its cartesian_product, then itertools.permutations): R1 R2 (R1 - 1)(R2 - 1) of them, int[n_arr, 2, 2].  Both
    ((a, b), (c, d)) and ((c, d), (a, b)) occur, as in the reference."""
    pairs = cartesian_product(np.asarray(reactive1, dtype=np.int64), np.asarray(reactive2, dtype=np.int64))
    out = [((ix_1, ix_2), (iy_1, iy_2)) for ((ix_1, ix_2), (iy_1, iy_2)) in permutations(pairs.tolist(), 2) if ix_1 != iy_1 and ix_2 != iy_2]
    return np.array(out, dtype=np.int64).reshape(-1, 2, 2)


def child_angles():
    """The angle table of a child: it does not inherit the parent's STEPS / ROTRANGE, only debug, simpleorbitals and shrink
    (tscode/multiembed.py:111-119), so rotation_range 45 and rotation_steps 5 built as tscode/embedder.py:714-715 does.  f64[36, 2]."""
    steps, rr = _CHILD_ROTATION_STEPS, _CHILD_ROTATION_RANGE
    return cartesian_product(np.arange(steps + 1), np.arange(steps + 1)) * 2 * rr / steps - rr


def _reactive_arg(mol, which):
    get = lambda k, d=None: (mol.get(k, d) if isinstance(mol, dict) else getattr(mol, k, d))
    coords, atomnos = check_orbital_args(get("coords"), get("atomnos"))
    n = len(atomnos)
    if not 1 <= n <= MAX_ATOMS:
        raise ValueError(f"molecule {which}: {n} atoms: the engine takes 1 .. {MAX_ATOMS}")
    r = np.asarray(get("reactive_indices"))
    if r.ndim != 1 or r.size and not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"molecule {which}: reactive_indices must be a flat list of atom indices")
    if len(r) < 2:
        raise ValueError(f"molecule {which}: {len(r)} reactive atoms: a multiembed takes at least two on each side")
    if r.min() < 0 or r.max() >= n:
        raise ValueError(f"molecule {which}: reactive index outside 0 .. {n - 1}")
    if len(set(r.tolist())) != len(r):
        raise ValueError(f"molecule {which}: a reactive atom is listed twice")
    return dict(coords=coords, atomnos=atomnos, reactive_indices=r.astype(np.int64), bonds=get("bonds"),
                orbital_args={k: get(k) for k in _ORBITAL_KEYS if get(k) is not None})


def check_args(mol1, mol2, systematic_angles=None):
    """The arguments of ``multiembed_batch`` as it uses them, or ValueError -- host only, before the library is entered: at least two reactive
    atoms on each side, in range, none twice; finite coordinates; atom counts within orbitals_batch's limits; at most MAX_GROUP_POSES angle sets."""
    m1, m2 = _reactive_arg(mol1, 1), _reactive_arg(mol2, 2)
    angles = child_angles() if systematic_angles is None else np.asarray(systematic_angles, dtype=np.float64)
    if angles.ndim != 2 or angles.shape[1] != 2 or len(angles) < 1:
        raise ValueError("systematic_angles must be (A >= 1, 2): one angle per molecule and angle set")
    if len(angles) > MAX_GROUP_POSES:
        raise ValueError(f"{len(angles)} angle sets per group: tsc_cyclical_embed_groups takes groups of up to {MAX_GROUP_POSES} poses")
    if not np.isfinite(angles).all():
        raise ValueError("systematic_angles contain NaN or infinity")
    return m1, m2, np.ascontiguousarray(angles)


def group_records(molecules1, molecules2, arrs, n1, max_norm_delta=_CHILD_MAX_NORM_DELTA):
    """The children's group records, concatenated in arrangement order.  ``molecules*[(ix, iy)]`` is what ``cyclical_embed_batch`` reads from a
    molecule (coords, reactive_indices = (ix, iy), pivots) for that ORDERED reactive pair.  Per arrangement ((ix_1, ix_2), (iy_1, iy_2)) the child's
    input reads ``mol1 ix_1 x iy_1 y`` / ``mol2 ix_2 x iy_2 y`` (tscode/multiembed.py:117-119): the rigid shortcut (tscode/embeds.py:734-860) with
    the two pairings x = [ix_1, ix_2 + n1], y = [iy_1, iy_2 + n1], which leave one of the two polygon orientations (:777).
    Returns (records f64[G, 2, 23], facing atoms int[G, 2, 2], groups per arrangement int[n_arr])."""
    blocks, ids, per = [], [], []
    for (ix_1, ix_2), (iy_1, iy_2) in np.asarray(arrs).tolist():
        a, b = molecules1[(ix_1, iy_1)], molecules2[(ix_2, iy_2)]
        get = lambda m, k: m[k] if isinstance(m, dict) else getattr(m, k)
        coords = [np.asarray(get(m, "coords"), dtype=np.float64) for m in (a, b)]
        reactive = [np.asarray(get(m, "reactive_indices"), dtype=np.int64) for m in (a, b)]
        pairings = [[ix_1, ix_2 + n1], [iy_1, iy_2 + n1]]                                            # embedder.pairings_table.values(), embedder.py:456
        rec, gid, _ = _bimolecular_groups(coords, reactive, [get(a, "pivots"), get(b, "pivots")], True, max_norm_delta, pairings, (), want_meta=False)
        blocks.append(rec), ids.append(gid), per.append(len(rec))
    if not blocks:
        return np.zeros((0, 2, 23)), np.zeros((0, 2, 2), dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(blocks), np.concatenate(ids), np.array(per, dtype=np.int64)


def fitness_targets(arrs, lengths1, lengths2):
    """The target distance of both facing pairs per arrangement, f64[n_arr, 2]: the sum of the two atoms' orbital lengths
    (``get_orbital_length``, tscode/hypermolecule_class.py:366, summed at tscode/embedder.py:951-963).  ``lengths*[(ix, iy)]`` = the lengths of
    ix and iy in the molecule built for that ordered pair.  AS THE REFERENCE: it tests the atom's index for truth (``if r_atom_index :=
    mol_pairing_dict.get(letter)``, :952), so an atom whose index in its molecule is 0 adds nothing to the target."""
    out = np.zeros((len(arrs), 2))
    for k, ((ix_1, ix_2), (iy_1, iy_2)) in enumerate(np.asarray(arrs).tolist()):
        l1, l2 = lengths1[(ix_1, iy_1)], lengths2[(ix_2, iy_2)]
        out[k, 0] = (l1[0] if ix_1 else 0.0) + (l2[0] if ix_2 else 0.0)
        out[k, 1] = (l1[1] if iy_1 else 0.0) + (l2[1] if iy_2 else 0.0)
    return out


def orbital_lengths(lobes, coords0, reactive_pair):
    """``get_orbital_length`` of both atoms of a reactive pair: |first lobe centre - atom| on conformer 0.  ``lobes[j]`` f64[L_j, 3]."""
    return tuple(float(np.linalg.norm(np.asarray(lobes[j], dtype=np.float64)[0] - coords0[int(i)])) for j, i in enumerate(reactive_pair))


def _edge_list(bonds, n):
    """Edges of a molecule's graph in the order networkx lists them for a graph built from an adjacency matrix (ascending pairs)."""
    if hasattr(bonds, "edges") and hasattr(bonds, "nodes"):
        return [(int(a), int(b)) for a, b in bonds.edges]
    from .reactive_atoms import neighbor_lists
    return [(i, j) for i, nb in enumerate(neighbor_lists(bonds, n)) for j in nb if i < j]


def sum_graph(bonds1, bonds2, n1, n2, extra_edges=()):
    """get_sum_graph (tscode/graph_manipulations.py:300-326) for two molecules: the first one's graph, the second one's edges shifted behind it
    (its nodes appear in the order its edges name them, as there), then the extra edges in cumulative numbering."""
    import networkx as nx
    out = nx.Graph()
    out.add_nodes_from(range(n1))
    out.add_edges_from(_edge_list(bonds1, n1))
    for a, b in _edge_list(bonds2, n2):
        out.add_edge(a + n1, b + n1)
    for a, b in extra_edges:
        out.add_edge(int(a), int(b))
    return out


def arrangement_quadruplets(bonds1, bonds2, n1, n2, arrs):
    """Per arrangement the quadruplets of its child's embed_graph: the sum graph plus ``constrained_indices[0]`` (tscode/embedder.py:1165-1169)
    -- the constrained indices of the first STRUCTURE, that is both facing pairs [ix_1, ix_2 + n1], [iy_1, iy_2 + n1] of the arrangement --
    through ``_get_quadruplets`` (= candidate_quadruplets without double bonds).  A list of i32[T, 4]."""
    from .torsion_module import candidate_quadruplets
    out = []
    for (ix_1, ix_2), (iy_1, iy_2) in np.asarray(arrs).tolist():
        out.append(candidate_quadruplets(sum_graph(bonds1, bonds2, n1, n2, [(ix_1, ix_2 + n1), (iy_1, iy_2 + n1)])))
    return out


def multiembed_batch(mol1, mol2, systematic_angles=None, clash_thresh=1.5, max_clashes=0, fitness_threshold=5, max_deviation=1e-2, tfd_thresh=10,
                     max_poses_per_call=DEFAULT_MAX_POSES_PER_CALL, tfd=False):
    """Every child embed of a bifunctional multiembed (tscode/multiembed.py:26-148) in one pass, in run_child_embedder's order.

    mol* = dict (or object) with ``coords`` f64[C, n, 3] (used as given: the reference has subtracted the ensemble's centroid,
    tscode/hypermolecule_class.py:179-184, and a caller who wants that does it), ``atomnos`` int[n], ``reactive_indices`` int[R >= 2],
    ``bonds`` (None: this package's graphize of conformer 0) and optionally the orbital arguments of ``reactive_molecule`` (overrides, orb_dim,
    leaving_group, sp_seed, suprafacial, sigmatropic).

    1. ``arrangements(r1, r2)`` in the reference's order.
    2. ``reactive_molecule`` once per DISTINCT ordered reactive pair (ix, iy) of each molecule -- R (R - 1) calls, not one per arrangement.
    3. ``group_records``: the rigid shortcut's groups per arrangement (max_norm_delta 5, the child's two pairings), concatenated.
    4. ONE ``tsc_cyclical_embed_groups`` call per slab of whole groups holding at most ``max_poses_per_call`` poses (see
       DEFAULT_MAX_POSES_PER_CALL for the arithmetic).  Groups are independent: the result does not depend on the slab size.
       ``systematic_angles=None`` is the child's own table (``child_angles()``).
    5. fitness_refining (tscode/embedder.py:1267-1305): one ``fitness_mask`` call over all kept poses, targets from ``fitness_targets``.
    6. similarity_refining(rmsd=False) (:1307-1354) through ``similarity_refining_batch``, one batched call per stage over all arrangements:
       TFD only with ``tfd=True`` -- the reference enters that stage where ``embed_graph.is_single_molecule``, and get_sum_graph takes that
       flag BEFORE it adds the constrained pair (tscode/graph_manipulations.py:318-322), so a child of two separate molecules never
       does; ``tfd=True`` runs it on ``arrangement_quadruplets`` (skipped where there are none, :1332) -- then MOI where at most 500 are left.
    7. Structures and facing atoms of all arrangements concatenated in ARRANGEMENT order.  The reference concatenates in as_completed order
       (tscode/multiembed.py:65-73), which no run defines; arrangement order is the one order every run of this call gives.  An arrangement
       that ends empty at any stage contributes nothing (the reference's ZeroCandidatesError branch, :139-140); if all do, the arrays are empty.
       The structures are the embed's own coordinates, like ``cyclical_embed_batch``'s: the child's write_structures centres them (the drop-in
       does that).

    Returns a MultiembedResult."""
    from .optimization_methods import fitness_mask, similarity_refining_batch
    m1, m2, angles = check_args(mol1, mol2, systematic_angles)
    if int(max_poses_per_call) < 1:
        raise ValueError("max_poses_per_call must be at least 1")
    n1, n2 = len(m1["atomnos"]), len(m2["atomnos"])
    n, A = n1 + n2, len(angles)
    arrs = arrangements(m1["reactive_indices"], m2["reactive_indices"])
    n_arr = len(arrs)
    for m in (m1, m2):
        if m["bonds"] is None:
            from .graph_manipulations import graphize
            m["bonds"] = graphize(m["coords"][0], m["atomnos"])
    molecules, lengths = [{}, {}], [{}, {}]
    for side, (m, offset) in enumerate(((m1, 0), (m2, n1))):
        for pair in sorted({(int(a[0][side]), int(a[1][side])) for a in arrs.tolist()}):
            rm = reactive_molecule(m["coords"], m["atomnos"], list(pair), m["bonds"], cumnum_offset=offset, **m["orbital_args"])
            molecules[side][pair] = rm
            lengths[side][pair] = orbital_lengths([rm.orbitals["centers"][0, j] for j in range(2)], m["coords"][0], pair)
    blocks, group_ids, groups_per = group_records(molecules[0], molecules[1], arrs, n1)
    targets = fitness_targets(arrs, lengths[0], lengths[1])
    group_off = np.concatenate([[0], np.cumsum(groups_per)]).astype(np.int64)
    G = len(blocks)
    # 4. the embed, slab by slab
    frags = FragmentSet([m1["coords"], m2["coords"]])
    eng = get_engine()
    field = lambda lo, hi, dtype=np.float64: np.ascontiguousarray(blocks[:, :, lo:hi], dtype=dtype)
    fields = [field(lo, lo + 3) for lo in range(0, 21, 3)]
    n_reactive, conf_idx = field(21, 22, np.int32).reshape(G, 2), field(22, 23, np.int32).reshape(G, 2)
    ok_parts, kept_parts, pose_parts = [], [], []
    for at, end in _slabs(G, A, max_poses_per_call):
        ok, kept, poses = eng.cyclical_embed_groups(frags, *[f[at:end] for f in fields], n_reactive[at:end], conf_idx[at:end], angles, clash_thresh, max_clashes)
        ok_parts.append(ok), kept_parts.append(kept), pose_parts.append(poses)
    clash_ok = np.concatenate(ok_parts) if ok_parts else np.zeros(0, bool)
    kept = np.concatenate(kept_parts) if kept_parts else np.zeros(0, bool)
    poses = np.concatenate(pose_parts) if pose_parts else np.zeros((0, n, 3))
    arr_of_group = np.repeat(np.arange(n_arr), groups_per)
    group_of = np.repeat(np.arange(G), A)[kept]
    arr_of = arr_of_group[group_of]
    constrained = group_ids[group_of].reshape(-1, 2, 2)
    counts = np.zeros((n_arr, 6), dtype=np.int64)
    cand_off = group_off * A
    counts[:, 0] = np.diff(cand_off)
    passed = np.concatenate([[0], np.cumsum(clash_ok, dtype=np.int64)])
    counts[:, 1] = passed[cand_off[1:]] - passed[cand_off[:-1]]
    counts[:, 2] = np.bincount(arr_of, minlength=n_arr)
    # 5. fitness
    fit = fitness_mask(poses, constrained, targets[arr_of], fitness_threshold) if len(poses) else np.zeros(0, bool)
    poses_f, constrained_f, arr_f = poses[fit], constrained[fit], arr_of[fit]
    counts[:, 3] = np.bincount(arr_f, minlength=n_arr)
    # 6. similarity: the arrangements that still hold something, each an ensemble of the batched stages
    atomnos = np.concatenate([m1["atomnos"], m2["atomnos"]])
    alive = [a for a in range(n_arr) if counts[a, 3] > 0]
    bounds = np.searchsorted(arr_f, np.arange(n_arr + 1))
    ens = [poses_f[bounds[a]:bounds[a + 1]] for a in alive]
    tfd_mask = np.ones(len(poses_f), dtype=bool)
    if tfd and alive:
        quads = arrangement_quadruplets(m1["bonds"], m2["bonds"], n1, n2, arrs)
        res = similarity_refining_batch(ens, atomnos, quadruplets=[quads[a] for a in alive], tfd=True, moi=False, rmsd=False, tfd_thresh=tfd_thresh)
        for a, (_, mask) in zip(alive, res):
            tfd_mask[bounds[a]:bounds[a + 1]] = mask
        ens = [e for e, _ in res]
    arr_t = arr_f[tfd_mask]
    counts[:, 4] = np.bincount(arr_t, minlength=n_arr)
    moi_mask = np.ones(len(arr_t), dtype=bool)
    if alive:
        bounds_t = np.searchsorted(arr_t, np.arange(n_arr + 1))
        res = similarity_refining_batch(ens, atomnos, tfd=False, moi=True, rmsd=False, max_deviation=max_deviation)
        for a, (_, mask) in zip(alive, res):
            moi_mask[bounds_t[a]:bounds_t[a + 1]] = mask
    final = tfd_mask.copy()
    final[tfd_mask] = moi_mask
    arr_out = arr_f[final]
    counts[:, 5] = np.bincount(arr_out, minlength=n_arr)
    return MultiembedResult(structures=poses_f[final], constrained_indices=constrained_f[final], arrangement_of=arr_out, arrangements=arrs, counts=counts,
                            clash_ok=clash_ok, kept=kept, candidate_off=cand_off, targets=targets,
                            masks={"fitness": fit, "tfd": tfd_mask, "moi": moi_mask})


# ----------------------------------------------------------------------------------------------------------------------
# Drop-ins with the reference's signatures (tscode_amd.install(multiembed=True), _MULTIEMBED_PATCHES)

_originals = {}          # name -> the reference's function, recorded by install()
_WRITE_LIMIT = 10000     # write_structures aligns -- and so centres -- the first 10 000 structures only, unless LET (tscode/embedder.py:1023-1027)


def _theirs(name):
    fn = _originals.get(name)
    if fn is None:
        raise RuntimeError(f"this multiembed needs the reference's own {name} (shrink, simpleorbitals or debug children, or more than two "
                           "molecules): tscode_amd.install(multiembed=True) records it")
    return fn


def multiembed_dispatcher(embedder):
    """Drop-in for tscode/multiembed.py:14-23: two molecules go to ``multiembed_bifunctional`` below, anything else to the reference's own
    dispatcher (which raises InputError)."""
    if len(embedder.objects) == 2:
        return multiembed_bifunctional(embedder)
    return _theirs("multiembed_dispatcher")(embedder)


def multiembed_bifunctional(embedder):
    """Drop-in for tscode/multiembed.py:26-82 ``multiembed_bifunctional(embedder)``: the children's structures and
    ``embedder.constrained_indices`` from ONE ``multiembed_batch`` call instead of one process per arrangement, concatenated in arrangement
    order (the reference: completion order).  Children with ``shrink``, ``simpleorbitals`` or ``debug`` go to the reference's own function.

    What a child hands back has been through its write_structures, whose align_structures centres its input IN PLACE
    (tscode/hypermolecule_class.py:46-55; the first 10 000 structures only when there are more and LET is off, tscode/embedder.py:1023-1027):
    each structure minus the mean of its atoms.  That is applied here, per arrangement."""
    import time
    opts = embedder.options
    if len(embedder.objects) != 2 or getattr(opts, "shrink", False) or getattr(opts, "simpleorbitals", False) or getattr(opts, "debug", False):
        return _theirs("multiembed_bifunctional")(embedder)
    mol1, mol2 = embedder.objects
    packed = [dict(coords=np.asarray(m.atomcoords, dtype=np.float64), atomnos=np.asarray(m.atomnos), reactive_indices=np.asarray(m.reactive_indices),
                   bonds=getattr(m, "graph", None)) for m in (mol1, mol2)]
    embedder.t_start_run = time.perf_counter()
    embedder.log()
    n_arr = len(arrangements(packed[0]["reactive_indices"], packed[1]["reactive_indices"]))
    embedder.log(f"--> Multiembed: running {n_arr} embeds in one grouped call (MI355X engine)")                          # :47
    # (a child is written ``noopt rigid`` and nothing else, :117: its thresholds and angles are the defaults, not the parent's)
    out = multiembed_batch(packed[0], packed[1])
    if not len(out.structures):
        raise ValueError("need at least one array to concatenate")       # what np.concatenate([]) raises at :75 when every child came back empty
    structures = out.structures.copy()
    rank = np.arange(len(structures)) - np.searchsorted(out.arrangement_of, out.arrangement_of)      # row number inside its arrangement
    centred = np.ones(len(structures), dtype=bool) if getattr(opts, "let", False) else rank < _WRITE_LIMIT
    structures[centred] -= structures[centred].mean(axis=1, keepdims=True)
    took = time.perf_counter() - embedder.t_start_run
    embedder.log(f"\n--> Multiembed completed: generated {len(structures)} candidates in {took:.3f} s.")                 # :77
    embedder.constrained_indices = out.constrained_indices                                                              # :80
    return structures
