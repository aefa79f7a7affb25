"""Symmetry-corrected RMSD pruning: tscode/torsion_module.py:953-1161 (prune_conformers_rmsd_rot_corr) on the MI355X engine.

The per-pair torsion search and every pass of the schedule run in one kernel launch per pass (csrc/rot_corr.hpp); the set-up
(the graph work of :1023-1049, once per call) and the graph step that turns each pass's matches into rejects stay on the host.
The pass schedule, the gate ``k == 1 or 5 k < active`` and the graph step are those of prune_conformers_tfd (numba_functions.py:
_pass_schedule / _tfd_reject_matches), which the reference's two functions share line for line.
"""

from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import check, ptr
from .engine import ContextObject, get_engine
from .numba_functions import TFD_KS, _pass_schedule, _tfd_schedule_batch
from .segments import byte_slices, ensemble_list, one_or_each, pack, scalar_or_each

__all__ = ["prune_rmsd_rot_corr_arrays", "prune_conformers_rmsd_rot_corr", "rot_corr_pairs", "last_rot_corr_stats",
           "prune_rmsd_rot_corr_arrays_batch", "last_rot_corr_batch_stats"]

MAX_TORSIONS, MAX_ATOMS, MAX_ANGLES = 16, 512, 6      # csrc/rot_corr.hpp: RC_MAX_TORS, RC_MAX_ATOMS, RC_MAX_ANGLES

ROT_CORR_BATCH_BYTES = 1 << 30          # coordinates plus cache bitmaps (N_s^2 / 8 bytes) one batch upload may hold; a longer list goes in slices

_last_stats = []
_last_batch_stats = []


def last_rot_corr_stats():
    """One dict per schedule slot (k = 5e5 ... 1) of the latest prune_rmsd_rot_corr_arrays call that ran the schedule: the
    active count the gate saw (``n_active``), whether the pass ran and the pairs it evaluated (rotationally_corrected_rmsd calls
    of the reference)."""
    return list(_last_stats)


def _centred(structures):
    structures = np.asarray(structures, dtype=np.float64)
    if len(structures) == 0:
        return structures.reshape(0, *structures.shape[1:]).copy()
    return np.array([s - s.mean(axis=0) for s in structures])          # :1023


class _Setup:
    """The host arrays of the C ABI (include/tscode_hip.h, tsc_rot_corr_begin)."""

    def __init__(self, n_atoms, atomnos, torsions, angles, move_masks, sub_nodes):
        atomnos = np.asarray(atomnos).reshape(-1)
        if len(atomnos) != n_atoms:
            raise ValueError(f"atomnos has {len(atomnos)} entries for structures of {n_atoms} atoms")
        self.heavy = np.ascontiguousarray(np.flatnonzero(atomnos != 1), dtype=np.int32)
        T = len(torsions)
        if T > MAX_TORSIONS or n_atoms > MAX_ATOMS:
            raise ValueError(f"{T} torsions / {n_atoms} atoms: the engine takes at most {MAX_TORSIONS} / {MAX_ATOMS}")
        if len(angles) != T or len(move_masks) != T or len(sub_nodes) != T:
            raise ValueError("torsions, angles, move_masks and sub_nodes must have one entry per torsion")
        self.T = T
        self.tors = np.ascontiguousarray(np.asarray(torsions, dtype=np.int32).reshape(T, 4))
        self.angles = np.zeros((T, MAX_ANGLES), dtype=np.float64)
        self.n_angles = np.zeros(T, dtype=np.int32)
        for t, a in enumerate(angles):
            a = np.asarray(a, dtype=np.float64).reshape(-1)
            if not 1 <= len(a) <= MAX_ANGLES:
                raise ValueError(f"torsion {t}: {len(a)} angles (1 .. {MAX_ANGLES})")
            self.angles[t, :len(a)] = a
            self.n_angles[t] = len(a)
        self.masks = np.ascontiguousarray(np.asarray(move_masks, dtype=bool).reshape(T, n_atoms)).view(np.uint8)
        subs = [np.asarray(s, dtype=np.int32).reshape(-1) for s in sub_nodes]
        self.sub_ptr = np.concatenate(([0], np.cumsum([len(s) for s in subs]))).astype(np.int32)
        self.sub_idx = np.ascontiguousarray(np.concatenate(subs) if subs else np.zeros(0, np.int32), dtype=np.int32)

    def args(self):
        return (ptr(self.heavy), C.c_int(len(self.heavy)), ptr(self.tors), C.c_int(self.T), ptr(self.angles), ptr(self.n_angles),
                ptr(self.masks), ptr(self.sub_ptr), ptr(self.sub_idx))


class _Run(ContextObject):
    """One tsc_rot_corr run: the structures live on the device, turned in place by the passes."""

    def __init__(self, engine, structures, setup):
        self.structures = np.ascontiguousarray(structures, dtype=np.float64)
        self.setup = setup
        h = C.c_void_p()
        check(engine.lib.tsc_rot_corr_begin(engine._h, ptr(self.structures), C.c_int64(len(self.structures)), C.c_int(self.structures.shape[1]),
                                            *setup.args(), C.byref(h)))
        self._own(engine, h, "tsc_rot_corr_destroy")

    def run_pass(self, d, k, num_active, max_rmsd):
        first = np.empty(len(self.structures), dtype=np.int32)
        ev = C.c_int64()
        check(self.e.lib.tsc_rot_corr_pass(self._r, C.c_int64(int(d)), C.c_int64(int(k)), C.c_int64(int(num_active)), C.c_double(float(max_rmsd)),
                                           ptr(first), C.byref(ev)))
        return first, ev.value

    def end(self):
        out = np.empty_like(self.structures)
        check(self.e.lib.tsc_rot_corr_end(self._r, ptr(out)))
        return out


def prune_rmsd_rot_corr_arrays(structures, atomnos, torsions, angles, move_masks, sub_nodes, max_rmsd=0.25, max_structures=750,
                               verbose=False):
    """prune_conformers_rmsd_rot_corr (tscode/torsion_module.py:1013-1161) with its set-up given as arrays:

    torsions    [T, 4] the dummy torsions, oriented as the reference orients them (:1049)
    angles      T sequences of angles in degrees, in the reference's order (``t.get_angles()``, 0 included)
    move_masks  bool [T, n_atoms]: the atoms each torsion turns (``_get_rotation_mask(graph, torsion)``)
    sub_nodes   T index lists: each torsion's local heavy subgraph (:964-977)

    The structures are centred on their all-atom mean (:1023); the function returns ``(centred[mask], mask)`` of the centred
    array AS THE PRUNE LEFT IT (every evaluated pair turns its second structure in place, as the reference does).  With no
    torsion, or more than ``max_structures`` structures (the reference's 750; None lifts the cap), it returns every centred
    structure (:1056)."""
    structures = _centred(structures)
    n = len(structures)
    final_mask = np.ones(n, dtype=bool)
    if len(torsions) == 0 or (max_structures is not None and n > max_structures):
        return structures[final_mask], final_mask
    setup = _Setup(structures.shape[1], atomnos, torsions, angles, move_masks, sub_nodes)
    stats = {int(k): {"k": k, "n_active": None, "ran": False, "pairs_evaluated": 0} for k in TFD_KS}
    run = _Run(get_engine(), structures, setup)
    try:
        def first_similar(d, k, num_active):
            first, ev = run.run_pass(d, k, num_active, max_rmsd)
            stats[k].update(n_active=num_active, ran=True, pairs_evaluated=ev)
            return first

        def gate_seen(k, num_active):
            stats[int(k)]["n_active"] = num_active

        final_mask = _pass_schedule(n, verbose, first_similar, on_slot=gate_seen)
        structures = run.end()
    finally:
        run.close()
    _last_stats[:] = [stats[int(k)] for k in TFD_KS]
    return structures[final_mask], final_mask


# ---- the same for many ensembles per call --------------------------------------------------------------------------------------
def last_rot_corr_batch_stats():
    """Per ensemble of the latest prune_rmsd_rot_corr_arrays_batch call what last_rot_corr_stats() reports after the single call on
    it: one dict per schedule slot.  An ensemble that took no part in the launch (no torsion, more than ``max_structures``
    structures, fewer than two) has an empty list."""
    return [list(s) for s in _last_batch_stats]


class _BatchRun(ContextObject):
    """One tsc_rot_corr_batch run: the structures of every segment live on the device, turned in place by the slots."""

    def __init__(self, engine, ensembles, setups):
        self.packed = pack([np.ascontiguousarray(e, dtype=np.float64) for e in ensembles])
        self.total_rows = int(self.packed.row_off[-1])

        def cat(name, dtype):
            return np.ascontiguousarray(np.concatenate([np.asarray(getattr(st, name)).ravel() for st in setups]), dtype=dtype)
        self.arrays = (cat("heavy", np.int32), np.array([len(st.heavy) for st in setups], dtype=np.int32), cat("tors", np.int32),
                       np.array([st.T for st in setups], dtype=np.int32), cat("angles", np.float64), cat("n_angles", np.int32),
                       cat("masks", np.uint8), cat("sub_ptr", np.int32), cat("sub_idx", np.int32))
        h = C.c_void_p()
        check(engine.lib.tsc_rot_corr_batch_begin(engine._h, *[ptr(a) for a in self.packed[:4]], *[ptr(a) for a in self.arrays],
                                                  C.c_int64(len(ensembles)), C.byref(h)))
        self._own(engine, h, "tsc_rot_corr_batch_destroy")

    def run_slot(self, open_segs, d, k, num_active, max_rmsd):
        """(first i32[total rows]: indices inside each segment, pairs evaluated i64[open segments])"""
        open_segs = np.ascontiguousarray(open_segs, dtype=np.int32)
        d = np.ascontiguousarray(d, dtype=np.int64)
        num_active = np.ascontiguousarray(num_active, dtype=np.int64)
        max_rmsd = np.ascontiguousarray(max_rmsd, dtype=np.float64)
        first = np.empty(self.total_rows, dtype=np.int32)
        ev = np.zeros(len(open_segs), dtype=np.int64)
        check(self.e.lib.tsc_rot_corr_batch_pass(self._r, ptr(open_segs), ptr(d), C.c_int64(int(k)), ptr(num_active), ptr(max_rmsd),
                                                 C.c_int64(len(open_segs)), ptr(first), ptr(ev)))
        return first, ev

    def end(self):
        out = np.empty_like(self.packed.flat)
        check(self.e.lib.tsc_rot_corr_batch_end(self._r, ptr(out)))
        return self.packed.cut(out, doubles=True)


def _batch_setup(s, n_atoms, atomnos, setup):
    """The _Setup of ensemble s, with everything the library would refuse refused here."""
    if not isinstance(setup, dict) or not {"torsions", "angles", "move_masks", "sub_nodes"} <= set(setup):
        raise ValueError(f"ensemble {s}: a set-up is a dict with the keys torsions, angles, move_masks, sub_nodes")
    try:
        st = _Setup(n_atoms, atomnos, setup["torsions"], setup["angles"], setup["move_masks"], setup["sub_nodes"])
    except ValueError as exc:
        raise ValueError(f"ensemble {s}: {exc}") from None
    if st.T == 0:
        return st
    if len(st.heavy) == 0:
        raise ValueError(f"ensemble {s}: no heavy atom")
    if st.tors.min() < 0 or st.tors.max() >= n_atoms:
        raise ValueError(f"ensemble {s}: torsion atom index out of range")
    if (np.diff(st.sub_ptr) <= 0).any() or (np.diff(st.sub_ptr) > n_atoms).any():
        raise ValueError(f"ensemble {s}: a local subgraph is empty or has more than {n_atoms} atoms")
    if st.sub_idx.min() < 0 or st.sub_idx.max() >= n_atoms:
        raise ValueError(f"ensemble {s}: subgraph atom index out of range")
    if not np.isfinite(st.angles).all():
        raise ValueError(f"ensemble {s}: angle not finite")
    return st


def _rot_corr_batch_args(ensembles, atomnos, setups, max_rmsd):
    """The checked arguments of prune_rmsd_rot_corr_arrays_batch: ([f64[N_s, n_s, 3]], [_Setup], f64[S], the atomnos and
    the set-up dict of every ensemble as given); ValueError otherwise."""
    ens = ensemble_list(ensembles, np.float64)
    S = len(ens)
    atomnos = one_or_each(atomnos, S, "atomnos arrays", 1, exact=True)
    setups = one_or_each(setups, S, "set-ups", None)
    th = scalar_or_each(max_rmsd, S, "max_rmsd values")
    if not np.isfinite(th).all():
        raise ValueError("max_rmsd not finite")
    return ens, [_batch_setup(s, e.shape[1], a, st) for s, (e, a, st) in enumerate(zip(ens, atomnos, setups))], th, atomnos, setups


def _rot_corr_batch_upload(ens, setups, th, verbose=False):
    """One upload: the schedule of every segment in lockstep (_tfd_schedule_batch), one launch per slot.  Returns
    ([turned structures], [mask], [stats])."""
    sizes = np.array([len(e) for e in ens], dtype=np.int64)
    stats = [{int(k): {"k": k, "n_active": None, "ran": False, "pairs_evaluated": 0} for k in TFD_KS} for _ in ens]
    run = _BatchRun(get_engine(), ens, setups)
    try:
        def pair_search(open_segs, d, k, num_active):
            first, ev = run.run_slot(open_segs, d, k, num_active, th[open_segs])
            for s, na, e in zip(open_segs.tolist(), num_active.tolist(), ev.tolist()):
                stats[s][k].update(n_active=na, ran=True, pairs_evaluated=e)
            return first

        keep, off = _tfd_schedule_batch(sizes, pair_search, verbose)
        turned = run.end()
    finally:
        run.close()
    for st in stats:                     # the gate's count of a slot that did not run: no pass lies between it and the next one that did
        seen = None
        for k in reversed(TFD_KS):
            if st[int(k)]["ran"]:
                seen = st[int(k)]["n_active"]
            else:
                st[int(k)]["n_active"] = seen
    return turned, [keep[off[s]:off[s + 1]] for s in range(len(ens))], [[st[int(k)] for k in TFD_KS] for st in stats]


def prune_rmsd_rot_corr_arrays_batch(ensembles, atomnos, setups, max_rmsd=0.25, max_structures=750, verbose=False):
    """prune_rmsd_rot_corr_arrays (tscode/torsion_module.py:1013-1161) for many ensembles per call: ``[(centred_s[mask_s], mask_s)]``,
    each entry exactly what ``prune_rmsd_rot_corr_arrays(ensembles[s], atomnos_s, **setups_s, max_rmsd=max_rmsd_s)`` returns.

    ``ensembles`` is a list of f64[N_s, n_s, 3] (every ensemble may be another molecule); ``atomnos`` one array for all or one per
    ensemble; ``setups`` one dict for all or one per ensemble with the keys ``torsions``, ``angles``, ``move_masks``, ``sub_nodes``
    as prune_rmsd_rot_corr_arrays takes them; ``max_rmsd`` a scalar or one value per ensemble.  The schedule's slots are walked in
    lockstep (_tfd_schedule_batch, the schedule :1076-1152 shares with the TFD prune): per slot ONE launch serves every chunk of
    every ensemble whose gate is open in it, one workgroup per chunk -- the same per-chunk device code as the single call's kernel
    (csrc/rot_corr.hpp) -- and one graph step.  An ensemble with no torsion, more than ``max_structures`` structures (:1056) or
    fewer than two takes no part and comes back centred with a full mask.  A list whose coordinates and cache bitmaps exceed
    ``ROT_CORR_BATCH_BYTES`` goes in slices; a list of one goes to prune_rmsd_rot_corr_arrays.  last_rot_corr_batch_stats() has
    the slots of every ensemble."""
    ens, sts, th, raw_atomnos, raw_setups = _rot_corr_batch_args(ensembles, atomnos, setups, max_rmsd)
    S = len(ens)
    if S == 0:
        _last_batch_stats[:] = []
        return []
    takes_part = [st.T > 0 and len(e) >= 2 and (max_structures is None or len(e) <= max_structures) for e, st in zip(ens, sts)]
    if S == 1 and not takes_part[0]:
        _last_batch_stats[:] = [[]]
        return [(_centred(ens[0]), np.ones(len(ens[0]), dtype=bool))]
    if S == 1:
        out = prune_rmsd_rot_corr_arrays(ens[0], raw_atomnos[0], **{key: raw_setups[0][key] for key in ("torsions", "angles", "move_masks", "sub_nodes")},
                                         max_rmsd=float(th[0]), max_structures=max_structures, verbose=verbose)
        _last_batch_stats[:] = [last_rot_corr_stats()]
        return [out]
    centred = [_centred(e) for e in ens]
    masks = [np.ones(len(e), dtype=bool) for e in ens]
    stats = [[] for _ in ens]
    idx = [s for s in range(S) if takes_part[s]]
    for at, end in byte_slices([centred[s].nbytes + (len(centred[s]) ** 2 + 7) // 8 for s in idx], ROT_CORR_BATCH_BYTES):
        part = idx[at:end]
        turned, part_masks, part_stats = _rot_corr_batch_upload([centred[s] for s in part], [sts[s] for s in part], th[part], verbose)
        for s, x, m, st in zip(part, turned, part_masks, part_stats):
            centred[s], masks[s], stats[s] = x, m, st
    _last_batch_stats[:] = stats
    return [(x[m], m) for x, m in zip(centred, masks)]


def rot_corr_pairs(structures, atomnos, torsions, angles, move_masks, sub_nodes, pairs):
    """rotationally_corrected_rmsd(ref=structures[i], coord=structures[j]) (tscode/torsion_module.py:953-1011) for every (i, j)
    of ``pairs`` on private copies (nothing is turned in ``structures``; no centring here).  Returns (rmsd f64[P], best angle
    f64[P, T])."""
    structures = np.ascontiguousarray(structures, dtype=np.float64)
    setup = _Setup(structures.shape[1], atomnos, torsions, angles, move_masks, sub_nodes)
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    rmsd = np.empty(len(pairs), dtype=np.float64)
    best = np.empty((len(pairs), setup.T), dtype=np.float64)
    eng = get_engine()
    check(eng.lib.tsc_rot_corr_pairs(eng._h, ptr(structures), C.c_int64(len(structures)), C.c_int(structures.shape[1]), *setup.args(),
                                     ptr(pairs), C.c_int64(len(pairs)), ptr(rmsd), ptr(best)))
    return rmsd, best


def _local_heavy_subgraph(graph, torsions, torsion, atomnos):
    """:964-977 on a copy of the graph: the heavy nodes of the component holding torsion[1] once every other torsion bond is cut."""
    import networkx as nx
    g = graph.copy()
    for other in torsions:
        if other is not torsion:
            g.remove_edge(other[1], other[2])
    comp = next(s for s in nx.connected_components(g) if torsion[1] in s)
    return sorted(int(i) for i in comp if atomnos[i] != 1)


def prune_conformers_rmsd_rot_corr(structures, atomnos, graph, max_rmsd=0.25, verbose=False, logfunction=None):
    """Drop-in for tscode.torsion_module.prune_conformers_rmsd_rot_corr (same signature, same results).  The set-up of
    :1023-1049 calls the graph helpers of the live ``tscode.torsion_module`` (this package never imports tscode); the prune
    itself is prune_rmsd_rot_corr_arrays.  Returns (structures[mask], mask) of the centred, turned structures."""
    tm = sys.modules.get("tscode.torsion_module")
    if tm is None:
        raise RuntimeError("prune_conformers_rmsd_rot_corr needs a live TSCoDe (tscode.torsion_module imported) for its graph helpers; "
                           "without one, call tscode_amd.prune_rmsd_rot_corr_arrays with the torsions, angles, rotation masks and "
                           "local subgraphs")
    import networkx as nx
    atomnos = np.asarray(atomnos)
    centred = _centred(structures)
    ref = centred[0]
    hydrogen_bonds = tm._get_hydrogen_bonds(ref, atomnos, graph)                          # :1026-1029
    for hb in hydrogen_bonds:
        graph.add_edge(*hb)
    try:
        torsions = tm._get_torsions(graph, hydrogen_bonds=tm._get_hydrogen_bonds(ref, atomnos, graph),
                                    double_bonds=tm.get_double_bonds_indices(ref, atomnos), keepdummy=True)        # :1032-1035
        torsions = [t for t in torsions if not (tm._is_nondummy(t.i2, t.i3, graph) and tm._is_nondummy(t.i3, t.i2, graph))]  # :1038-1040
        torsions = [t for t in torsions if 1 not in [atomnos[i] for i in t.torsion]]                              # :1043
        angles = [t.get_angles() for t in torsions]                                                               # :1046
        torsions = [t.torsion if tm._is_nondummy(t.i2, t.i3, graph) else list(reversed(t.torsion)) for t in torsions]   # :1049
        if len(torsions) == 0 or len(centred) > 750:                                                              # :1056
            return centred, np.ones(len(centred), dtype=bool)
        masks = [np.asarray(tm._get_rotation_mask(graph, t), dtype=bool) for t in torsions]
        subs = [_local_heavy_subgraph(graph, torsions, t, atomnos) for t in torsions]
    finally:
        for hb in hydrogen_bonds:                                                                                  # :1155-1159
            try:
                graph.remove_edge(*hb)
            except nx.NetworkXError:
                pass
    if logfunction is not None:                                                                                    # :1063-1074
        pt = tm.pt
        logfunction('\n >> Dihedrals considered for subsymmetry corrections:')
        for i, (torsion, angle) in enumerate(zip(torsions, angles)):
            logfunction(' {:2s} - {:21s} : {}{}{}{} : {}-fold'.format(str(i), str(torsion), pt[atomnos[torsion[0]]].symbol,
                                                                   pt[atomnos[torsion[1]]].symbol, pt[atomnos[torsion[2]]].symbol,
                                                                   pt[atomnos[torsion[3]]].symbol, len(angle)))
        logfunction("\n")
    return prune_rmsd_rot_corr_arrays(structures, atomnos, torsions, angles, masks, subs, max_rmsd=max_rmsd, max_structures=750,
                                      verbose=verbose)
