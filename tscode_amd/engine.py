"""Engine: one libtscode_hip context (one GPU, one stream) and typed Python entry points.

Host methods take and return NumPy arrays (the drop-in functions are built on them);
``*_dev`` methods take anything with ``data_ptr()`` (torch tensors on the engine's GPU) and
leave results on the device.  Every call goes through the C ABI of include/tscode_hip.h.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import threading
import weakref

import numpy as np

from . import _lib, segments
from ._lib import BatchPassStats, PassStats, TSC_MAX_PASSES, check, ptr

__all__ = ["Engine", "FragmentSet", "get_engine", "device_count"]


def device_count() -> int:
    n = _lib.load().tsc_device_count()
    if n < 0:
        check(n)
    return n


class FragmentSet:
    """Rigid fragments in the layout tsc_transform_batch expects:
    fragment m is a conformer stack f64[n_conf_m, n_m, 3]; all stacks sit back to back in one buffer."""

    def __init__(self, frag_coords):
        stacks = []
        for f in frag_coords:
            f = np.ascontiguousarray(f, dtype=np.float64)
            if f.ndim == 2:
                f = f[None]
            if f.ndim != 3 or f.shape[2] != 3:
                raise ValueError("each fragment must be (n_conf, n_atoms, 3) or (n_atoms, 3)")
            stacks.append(f)
        self.n_mols = len(stacks)
        self.n_atoms = np.array([s.shape[1] for s in stacks], dtype=np.int32)
        self.n_conf = np.array([s.shape[0] for s in stacks], dtype=np.int32)
        sizes = np.array([s.size for s in stacks], dtype=np.int64)
        self.frag_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.flat = np.ascontiguousarray(np.concatenate([s.ravel() for s in stacks]))
        self.n_total = int(self.n_atoms.sum())

    def table_args(self):
        return (self.frag_off.ctypes.data_as(_lib.c_i64p), self.n_atoms.ctypes.data_as(_lib.c_i32p),
                self.n_conf.ctypes.data_as(_lib.c_i32p), C.c_int(self.n_mols))


def _ids_arg(ids):
    if ids is None:
        return None, 0, np.zeros(0, dtype=np.int32)
    a = np.ascontiguousarray(ids, dtype=np.int32).ravel()
    return a.ctypes.data_as(_lib.c_i32p), len(a), a


def _stats_list(stats, n):
    return [stats[i].as_dict() for i in range(n)]


_BATCH_STAT_FIELDS = tuple(f for f, _ in BatchPassStats._fields_)

# Structures per ensemble up to which prune_heavy_batch sends an ensemble longer than "prune_batch_max_n" to tsc_prune_rmsd_team
# instead of a call of its own: the largest size measured at which a call on 16 ensembles was not slower with the team route than
# without (MEASURED.md section 30: 4096 -- level through the host-array call, where gather, packing and upload are nine tenths of the
# time, 2.3 times faster on resident data; at 8192 the route loses on both counts).
PRUNE_TEAM_MAX_N = 4096


def check_team_max_n(team_max_n):
    """The ``team_max_n`` keyword of the batched RMSD prune as a whole number 0 .. TSC_PRUNE_TEAM_MAX_N (None: PRUNE_TEAM_MAX_N).
    No device is touched."""
    if team_max_n is None:
        return PRUNE_TEAM_MAX_N
    if isinstance(team_max_n, (bool, np.bool_)) or not isinstance(team_max_n, (int, np.integer)):
        raise ValueError(f"team_max_n must be a whole number or None, got {team_max_n!r}")
    if not 0 <= team_max_n <= _lib.TSC_PRUNE_TEAM_MAX_N:
        raise ValueError(f"team_max_n = {team_max_n} not in 0 .. {_lib.TSC_PRUNE_TEAM_MAX_N}")
    return int(team_max_n)


def pack_heavy_batch(heavies):
    """The arrays tsc_prune_rmsd_batch takes for a sequence of heavy-atom arrays f64[N_s, h_s, 3]: (flat, offsets, n, h) -- the arrays
    back to back, offsets i64[S + 1] in doubles, n i32[S] structures and h i32[S] heavy atoms per ensemble.  No device is touched."""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in heavies]
    for s, a in enumerate(arrays):
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"ensemble {s}: heavy must be (N, h, 3), got {a.shape}")
    return segments.pack(arrays)[:4]


class PipelineResult:
    """What one tsc_pipeline_dev call returned.  Reads like the dict it used to be (res["n_pass"], res["stats"], ...);
    the per-pass statistics are turned into Python objects only when somebody asks for them -- a dozen structs of a dozen
    fields cost more host time than several of the step's kernels take."""
    __slots__ = ("n_pass", "n_keep", "_stats", "_n_passes", "_tm", "_cache")

    def __init__(self, n_pass, n_keep, stats, n_passes, tm):
        self.n_pass, self.n_keep, self._stats, self._n_passes, self._tm, self._cache = n_pass, n_keep, stats, n_passes, tm, None

    @property
    def stats(self):
        if self._cache is None:
            self._cache = _stats_list(self._stats, self._n_passes)
        return self._cache

    @property
    def ms(self):
        t = self._tm
        return {"embed_clash": t[0], "compact": t[1], "prune": t[2], "total": t[3]}

    def __getitem__(self, key):
        if key in ("n_pass", "n_keep", "stats", "ms"):
            return getattr(self, key)
        raise KeyError(key)

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default

    def keys(self):
        return ("n_pass", "n_keep", "stats", "ms")


class Engine:
    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.tsc_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._runs = weakref.WeakSet()      # the live ContextObjects: they hold blocks, events or mappings of this context

    def close(self):
        if getattr(self, "_h", None):
            # (a run and its engine can become garbage together -- e.g. both held by the traceback of an exception -- and the
            # collector finalises them in no particular order: the runs go first, whichever finaliser is called first.  When they die
            # in ONE collection CPython has cleared the weak references before any finaliser runs and this set is already empty:
            # tsc_ctx_destroy then destroys the runs the context still lists itself, and their close() finds the engine closed)
            for run in list(getattr(self, "_runs", ())):
                run.close()
            self.lib.tsc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stream / timing ------------------------------------------------------------------
    def set_stream(self, hip_stream):
        check(self.lib.tsc_ctx_set_stream(self._h, C.c_void_p(hip_stream) if hip_stream else None))

    def synchronize(self):
        check(self.lib.tsc_ctx_synchronize(self._h))

    def set_option(self, name: str, value: float):
        """tsc_ctx_set_option: set a tunable of the library.  include/tscode_hip.h lists them, with their values, above that function."""
        check(self.lib.tsc_ctx_set_option(self._h, name.encode(), C.c_double(value)))

    def get_option(self, name: str) -> float:
        """tsc_ctx_get_option: the current value of a tunable (every one can be read)."""
        v = C.c_double()
        check(self.lib.tsc_ctx_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def option_defaults(self) -> dict:
        """{name: default} of every tunable, in the library's order (tsc_option_info: the library holds the only list)."""
        out, name, v = {}, C.c_char_p(), C.c_double()
        while self.lib.tsc_option_info(len(out), C.byref(name), C.byref(v)) == 0:
            out[name.value.decode()] = v.value
        return out

    @contextlib.contextmanager
    def options(self, **values):
        """Run a block under other values of some tunables: `with eng.options(cull=2, cull_min_pairs=0): ...` sets them and puts back
        what was there before -- not the defaults -- in reverse order, however the block ends."""
        old = [(name, self.get_option(name)) for name in values]
        try:
            for name, value in values.items():
                self.set_option(name, value)
            yield self
        finally:
            for name, value in reversed(old):
                self.set_option(name, value)

    @property
    def prune_batch_max_n(self) -> int:
        """Structures per ensemble that tsc_prune_rmsd_batch takes (the context's option, read from the library: one copy of the default)."""
        return int(self.get_option("prune_batch_max_n"))

    def timer_begin(self):
        check(self.lib.tsc_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_float()
        check(self.lib.tsc_timer_end(self._h, C.byref(ms)))
        return ms.value

    # ---- K1 ---------------------------------------------------------------------------------
    def transform_batch(self, frags: FragmentSet, conf_idx, rot, pos) -> np.ndarray:
        conf_idx = np.ascontiguousarray(conf_idx, dtype=np.int32).reshape(-1, frags.n_mols)
        rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1, frags.n_mols, 3, 3)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, frags.n_mols, 3)
        n = len(rot)
        if not (len(conf_idx) == n == len(pos)):
            raise ValueError("conf_idx, rot and pos disagree on the number of poses")
        out = np.empty((n, frags.n_total, 3), dtype=np.float64)
        check(self.lib.tsc_transform_batch(self._h, ptr(frags.flat), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos),
                                           C.c_int64(n), ptr(out)))
        return out

    def transform_batch_dev(self, frags: FragmentSet, frags_dev, conf_idx, rot, pos, n_poses, out):
        check(self.lib.tsc_transform_batch_dev(self._h, ptr(frags_dev), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos),
                                               C.c_int64(n_poses), ptr(out)))

    # ---- K2 ---------------------------------------------------------------------------------
    def clash_mask(self, coords, ids=None, thresh=1.5, max_clashes=0, return_counts=False):
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        if coords.ndim != 3 or coords.shape[2] != 3:
            raise ValueError("coords must be (n_poses, n_atoms, 3)")
        n, na = coords.shape[0], coords.shape[1]
        ids_p, n_ids, _keep = _ids_arg(ids)
        mask = np.zeros(n, dtype=np.uint8)
        counts = np.zeros(n, dtype=np.int32) if return_counts else None
        check(self.lib.tsc_clash_mask(self._h, ptr(coords), C.c_int64(n), C.c_int(na), ids_p, C.c_int(n_ids), C.c_double(thresh),
                                      C.c_int64(int(max_clashes)), ptr(mask), ptr(counts)))
        return (mask.astype(bool), counts) if return_counts else mask.astype(bool)

    def clash_mask_dev(self, coords, n_poses, n_atoms, ids, thresh, max_clashes, mask, counts=None):
        ids_p, n_ids, _keep = _ids_arg(ids)
        check(self.lib.tsc_clash_mask_dev(self._h, ptr(coords), C.c_int64(n_poses), C.c_int(n_atoms), ids_p, C.c_int(n_ids),
                                          C.c_double(thresh), C.c_int64(int(max_clashes)), ptr(mask), ptr(counts)))

    def embed_clash_mask_dev(self, frags: FragmentSet, frags_dev, conf_idx, rot, pos, n_poses, thresh, max_clashes, mask, counts=None):
        check(self.lib.tsc_embed_clash_mask_dev(self._h, ptr(frags_dev), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos),
                                                C.c_int64(n_poses), C.c_double(thresh), C.c_int64(int(max_clashes)), ptr(mask),
                                                ptr(counts)))

    def embed_clash_compact_dev(self, frags: FragmentSet, frags_dev, conf_idx, rot, pos, n_poses, heavy_idx, thresh, max_clashes, mask,
                                structures, heavy) -> int:
        """Fused embed + clash verdicts, then the passing poses embedded straight into ``structures`` (may be None) and ``heavy``.
        Returns how many passed."""
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        n_pass = C.c_int64()
        check(self.lib.tsc_embed_clash_compact_dev(self._h, ptr(frags_dev), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos),
                                                   C.c_int64(n_poses), heavy_idx.ctypes.data_as(_lib.c_i32p), C.c_int(len(heavy_idx)),
                                                   C.c_double(thresh), C.c_int64(int(max_clashes)), ptr(mask), ptr(structures), ptr(heavy),
                                                   C.byref(n_pass)))
        return n_pass.value

    def basis_from_poses_dev(self, frags: FragmentSet, frags_dev, conf_idx, rot, pos, n_poses, heavy_idx):
        """Fork the estimate of the prune's descriptor basis from a sample of these poses onto the side stream."""
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        check(self.lib.tsc_basis_from_poses_dev(self._h, ptr(frags_dev), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos), C.c_int64(n_poses),
                                                heavy_idx.ctypes.data_as(_lib.c_i32p), C.c_int(len(heavy_idx))))

    def embed_masked_dev(self, frags: FragmentSet, frags_dev, conf_idx, rot, pos, n_poses, mask, heavy_idx, structures, heavy, want_count=True):
        """The poses selected by a device mask, embedded in order into ``structures`` and / or ``heavy`` (either may be None).
        Returns how many were selected (None with want_count=False: the call then does not synchronise)."""
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        n_sel = C.c_int64()
        check(self.lib.tsc_embed_masked_dev(self._h, ptr(frags_dev), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos), C.c_int64(n_poses),
                                            ptr(mask), heavy_idx.ctypes.data_as(_lib.c_i32p), C.c_int(len(heavy_idx)), ptr(structures), ptr(heavy),
                                            C.byref(n_sel) if want_count else None))
        return n_sel.value if want_count else None

    def all_dists(self, a, b) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != 3 or b.shape[1] != 3:
            raise AssertionError("all_dists needs (n, 3) arrays")          # reference: assert A.shape[1]==B.shape[1]
        out = np.empty((len(a), len(b)), dtype=np.float64)
        check(self.lib.tsc_all_dists(self._h, ptr(a), C.c_int(len(a)), ptr(b), C.c_int(len(b)), ptr(out)))
        return out

    # ---- compaction ---------------------------------------------------------------------------
    def compact_rows_dev(self, src, mask, n_rows, row_bytes, dst) -> int:
        kept = C.c_int64()
        check(self.lib.tsc_compact_rows_dev(self._h, ptr(src), ptr(mask), C.c_int64(n_rows), C.c_int64(row_bytes), ptr(dst),
                                            C.byref(kept)))
        return kept.value

    def gather_heavy_dev(self, coords, mask, n_poses, n_atoms, heavy_idx, heavy_out) -> int:
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        kept = C.c_int64()
        check(self.lib.tsc_gather_heavy_dev(self._h, ptr(coords), ptr(mask), C.c_int64(n_poses), C.c_int(n_atoms),
                                            heavy_idx.ctypes.data_as(_lib.c_i32p), C.c_int(len(heavy_idx)), ptr(heavy_out),
                                            C.byref(kept)))
        return kept.value

    # ---- K3 ---------------------------------------------------------------------------------
    def rmsd_pairs(self, heavy, pairs):
        heavy = np.ascontiguousarray(heavy, dtype=np.float64)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        r = np.empty(len(pairs), dtype=np.float64)
        m = np.empty(len(pairs), dtype=np.float64)
        check(self.lib.tsc_rmsd_pairs(self._h, ptr(heavy), C.c_int64(heavy.shape[0]), C.c_int(heavy.shape[1]), ptr(pairs),
                                      C.c_int64(len(pairs)), ptr(r), ptr(m)))
        return r, m

    # ---- cross-set RMSD (csrc/cross.hpp; argument checks and row blocks: tscode_amd/rmsd_cross.py) ------------------------------
    @staticmethod
    def _cross_args(queries, library, idx):
        """(queries, n_q, library or None, n_l, n_atoms, idx or None, n_idx) as the tsc_rmsd_cross* calls take them; library None: the
        queries against themselves."""
        n_l = queries.shape[0] if library is None else library.shape[0]
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        return (ptr(queries), C.c_int64(queries.shape[0]), ptr(library), C.c_int64(n_l), C.c_int(queries.shape[1]), ptr(idx),
                C.c_int(0 if idx is None else len(idx))), n_l, idx

    def rmsd_cross_rows(self, n_library, max_bytes) -> int:
        """tsc_rmsd_cross_rows: query rows one rmsd_cross call may take so that its two outputs stay within max_bytes (at least 1)."""
        rows = C.c_int64()
        check(self.lib.tsc_rmsd_cross_rows(C.c_int64(n_library), C.c_int64(max_bytes), C.byref(rows)))
        return rows.value

    def rmsd_cross(self, queries, library=None, idx=None, center=False):
        """tsc_rmsd_cross: (rmsd, maxdev) f64[Nq, Nl] of queries f64[Nq, n, 3] against library f64[Nl, n, 3] (None: themselves) on the atoms
        idx (None: all).  Both C-contiguous float64."""
        args, n_l, _keep = self._cross_args(queries, library, idx)
        r = np.empty((queries.shape[0], n_l), dtype=np.float64)
        m = np.empty((queries.shape[0], n_l), dtype=np.float64)
        check(self.lib.tsc_rmsd_cross(self._h, *args, C.c_int(bool(center)), ptr(r), ptr(m), C.c_int64(r.size)))
        return r, m

    def rmsd_cross_first(self, queries, library, idx=None, rmsd_thr=0.5, center=False):
        """tsc_rmsd_cross_first: first i32[Nq], the lowest library index every query is similar to, INT32_MAX where there is none."""
        args, _n_l, _keep = self._cross_args(queries, library, idx)
        first = np.empty(queries.shape[0], dtype=np.int32)
        check(self.lib.tsc_rmsd_cross_first(self._h, *args, C.c_int(bool(center)), C.c_double(rmsd_thr), ptr(first)))
        return first

    def rmsd_cross_nearest(self, queries, library, idx=None, center=False):
        """tsc_rmsd_cross_nearest: (index i32[Nq], rmsd f64[Nq], maxdev f64[Nq]) of the nearest library member of every query."""
        args, _n_l, _keep = self._cross_args(queries, library, idx)
        n = queries.shape[0]
        index, r, m = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        check(self.lib.tsc_rmsd_cross_nearest(self._h, *args, C.c_int(bool(center)), ptr(index), ptr(r), ptr(m)))
        return index, r, m

    def rmsd_cross_dev(self, queries, n_q, library, n_l, n_atoms, idx, n_idx, center, rmsd, maxdev, capacity):
        """tsc_rmsd_cross_dev: every array on the device (torch tensors or raw pointers; library None: the queries themselves, idx None
        with n_idx 0: all atoms); rmsd / maxdev f64 with room for `capacity` values each.  Enqueues and returns; finite input is the
        caller's business."""
        check(self.lib.tsc_rmsd_cross_dev(self._h, ptr(queries), C.c_int64(n_q), ptr(library), C.c_int64(n_l), C.c_int(n_atoms), ptr(idx), C.c_int(n_idx),
                                          C.c_int(bool(center)), ptr(rmsd), ptr(maxdev), C.c_int64(capacity)))

    def rmsd_cross_first_dev(self, queries, n_q, library, n_l, n_atoms, idx, n_idx, center, rmsd_thr, first):
        """tsc_rmsd_cross_first_dev: as rmsd_cross_dev; first i32[n_q] on the device (INT32_MAX: none).  Enqueues and returns."""
        check(self.lib.tsc_rmsd_cross_first_dev(self._h, ptr(queries), C.c_int64(n_q), ptr(library), C.c_int64(n_l), C.c_int(n_atoms), ptr(idx), C.c_int(n_idx),
                                                C.c_int(bool(center)), C.c_double(rmsd_thr), ptr(first)))

    def rmsd_cross_nearest_dev(self, queries, n_q, library, n_l, n_atoms, idx, n_idx, center, index, rmsd, maxdev):
        """tsc_rmsd_cross_nearest_dev: as rmsd_cross_dev; index i32[n_q], rmsd / maxdev f64[n_q] on the device.  Enqueues and returns."""
        check(self.lib.tsc_rmsd_cross_nearest_dev(self._h, ptr(queries), C.c_int64(n_q), ptr(library), C.c_int64(n_l), C.c_int(n_atoms), ptr(idx), C.c_int(n_idx),
                                                  C.c_int(bool(center)), ptr(index), ptr(rmsd), ptr(maxdev)))

    # ---- energy-ordered RMSD prune (csrc/leader.hpp; argument checks: tscode_amd/rmsd_ordered.py) -------------------------------
    def prune_rmsd_ordered(self, structures, library=None, idx=None, order=None, rmsd_thr=0.5, center=False):
        """tsc_prune_rmsd_ordered: (mask u8[N], rep i32[N], lib_rep i32[N], n_kept) of structures f64[N, n, 3] walked in ``order`` (i32[N],
        a permutation; None: as they lie) against library f64[Nl, n, 3] (None: none) on the atoms idx (None: all).  C-contiguous float64."""
        n = structures.shape[0]
        n_l = 0 if library is None else library.shape[0]
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        mask, rep, lib_rep = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        n_kept = C.c_int64()
        check(self.lib.tsc_prune_rmsd_ordered(self._h, ptr(structures), C.c_int64(n), ptr(library) if n_l else None, C.c_int64(n_l), C.c_int(structures.shape[1]),
                                              ptr(idx), C.c_int(0 if idx is None else len(idx)), C.c_int(bool(center)), ptr(order), C.c_double(rmsd_thr),
                                              ptr(mask), ptr(rep), ptr(lib_rep), C.byref(n_kept)))
        return mask, rep, lib_rep, n_kept.value

    def prune_rmsd_ordered_dev(self, structures, n, library, n_l, n_atoms, idx, n_idx, center, order, rmsd_thr, mask, rep, lib_rep) -> int:
        """tsc_prune_rmsd_ordered_dev: every array on the device (torch tensors or raw pointers; library None with n_l 0: none, idx None with
        n_idx 0: all atoms, order None: the rows as they lie); mask u8[n], rep / lib_rep i32[n] on the device.  Returns the kept count; the
        stream is idle and the outputs are complete when it returns.  Finite input and a valid order are the caller's business."""
        n_kept = C.c_int64()
        check(self.lib.tsc_prune_rmsd_ordered_dev(self._h, ptr(structures), C.c_int64(n), ptr(library), C.c_int64(n_l), C.c_int(n_atoms), ptr(idx), C.c_int(n_idx),
                                                  C.c_int(bool(center)), ptr(order), C.c_double(rmsd_thr), ptr(mask), ptr(rep), ptr(lib_rep), C.byref(n_kept)))
        return n_kept.value

    def greedy_group_filter(self, poses, group_off, rmsd_thr=1.0):
        """accepted bool[n_poses]: per group, keep a pose iff it is not similar to a pose kept before it."""
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        group_off = np.ascontiguousarray(group_off, dtype=np.int32)
        if poses.ndim != 3 or poses.shape[2] != 3 or group_off.ndim != 1 or len(group_off) < 1 or group_off[-1] != len(poses):
            raise ValueError("poses must be (n_poses, n_atoms, 3) and group_off[-1] == n_poses")
        acc = np.zeros(len(poses), dtype=np.uint8)
        check(self.lib.tsc_greedy_group_filter(self._h, ptr(poses), ptr(group_off), C.c_int(len(group_off) - 1), C.c_int(poses.shape[1]),
                                               C.c_double(rmsd_thr), ptr(acc)))
        return acc.astype(bool)

    # ---- N2: torsion fingerprints / TFD pair search -----------------------------------------------
    def torsion_fingerprints(self, structures, quadruplets):
        """_get_tf_mat (tscode/numba_functions.py:233-240): f32[N, T] dihedral angles in degrees."""
        structures = np.ascontiguousarray(structures, dtype=np.float64)
        if structures.ndim != 3 or structures.shape[2] != 3:
            raise ValueError("structures must be (N, n_atoms, 3)")
        quads = np.ascontiguousarray(quadruplets, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((len(structures), len(quads)), dtype=np.float32)
        check(self.lib.tsc_torsion_fingerprints(self._h, ptr(structures), C.c_int64(len(structures)), C.c_int(structures.shape[1]), ptr(quads),
                                                C.c_int(len(quads)), ptr(out)))
        return out

    def tfd_first_similar(self, tf_mat, d, k, num_active, thresh=10.0):
        """The pair search of one pass of prune_conformers_tfd (tscode/numba_functions.py:171-199): i32[N], -1 = none."""
        tf = np.ascontiguousarray(tf_mat, dtype=np.float32)
        first = np.full(len(tf), -1, dtype=np.int32)
        check(self.lib.tsc_tfd_first_similar(self._h, ptr(tf), C.c_int64(len(tf)), C.c_int(tf.shape[1]), C.c_int64(int(d)), C.c_int64(int(k)),
                                             C.c_int64(int(num_active)), C.c_double(float(thresh)), ptr(first)))
        return first

    def tfd_batch_fingerprints_dev(self, coords, offsets, n_structs, n_atoms, quads, n_quads):
        """tsc_tfd_batch_fingerprints_dev (include/tscode_hip.h): the fingerprints of every segment, computed once and left on the
        device.  coords f64[sum N n 3] with offsets i64[S + 1], quads i32[sum T, 4]; n_structs, n_atoms, n_quads i32[S].  Returns
        (address, element count); the caller hands the address back with dev_free."""
        count = int(np.dot(n_structs.astype(np.int64), n_quads.astype(np.int64)))
        tf = self.dev_alloc(4 * count)
        try:
            check(self.lib.tsc_tfd_batch_fingerprints_dev(self._h, ptr(coords), ptr(offsets), ptr(n_structs), ptr(n_atoms), ptr(quads), ptr(n_quads),
                                                          C.c_int64(len(n_structs)), C.c_void_p(tf), C.c_int64(count)))
        except BaseException:
            self.dev_free(tf)
            raise
        return tf, count

    def tfd_batch_pass_dev(self, tf, tf_count, elem0, row0, n_structs, n_quads, d, k, num_active, thresh, total_rows):
        """tsc_tfd_batch_pass_dev: one schedule slot of prune_conformers_tfd for every open segment in one launch: i32[total_rows],
        indices inside each segment, -1 = none or a row of no open segment."""
        first = np.full(int(total_rows), -1, dtype=np.int32)
        elem0, row0, d, k, num_active = (np.ascontiguousarray(a, dtype=np.int64) for a in (elem0, row0, d, k, num_active))
        n_structs, n_quads = (np.ascontiguousarray(a, dtype=np.int32) for a in (n_structs, n_quads))
        thresh = np.ascontiguousarray(thresh, dtype=np.float64)
        check(self.lib.tsc_tfd_batch_pass_dev(self._h, C.c_void_p(tf), C.c_int64(int(tf_count)), ptr(elem0), ptr(row0), ptr(n_structs), ptr(n_quads),
                                              ptr(d), ptr(k), ptr(num_active), ptr(thresh), C.c_int64(len(elem0)), C.c_int64(int(total_rows)),
                                              ptr(first)))
        return first

    # ---- N4: moments of inertia, embed scores -------------------------------------------------------
    def inertia_moments(self, structures, masses):
        structures = np.ascontiguousarray(structures, dtype=np.float64)
        masses = np.ascontiguousarray(masses, dtype=np.float64)
        if structures.ndim != 3 or structures.shape[2] != 3 or masses.shape != (structures.shape[1],):
            raise ValueError("structures must be (N, n_atoms, 3) and masses (n_atoms,)")
        out = np.empty((len(structures), 3))
        check(self.lib.tsc_inertia_moments(self._h, ptr(structures), C.c_int64(len(structures)), C.c_int(structures.shape[1]), ptr(masses), ptr(out)))
        return out

    def moi_first_similar(self, moments, max_deviation=1e-2):
        moments = np.ascontiguousarray(moments, dtype=np.float64).reshape(-1, 3)
        first = np.full(len(moments), -1, dtype=np.int32)
        check(self.lib.tsc_moi_first_similar(self._h, ptr(moments), C.c_int64(len(moments)), C.c_double(float(max_deviation)), ptr(first)))
        return first

    def inertia_moments_batch(self, ensembles, masses):
        """inertia_moments of every ensemble ([f64[N_s, n_s, 3]], [f64[n_s]]) in one launch: [f64[N_s, 3]]."""
        ensembles = [np.ascontiguousarray(e, dtype=np.float64) for e in ensembles]
        masses = [np.ascontiguousarray(m, dtype=np.float64) for m in masses]
        if len(masses) != len(ensembles):
            raise ValueError(f"{len(masses)} mass arrays for {len(ensembles)} ensembles")
        for e, m in zip(ensembles, masses):
            if e.ndim != 3 or e.shape[2] != 3 or e.shape[1] < 1 or m.shape != (e.shape[1],):
                raise ValueError("structures must be (N, n_atoms, 3) and masses (n_atoms,)")
        if not ensembles:
            return []
        p = segments.pack(ensembles)
        all_masses = np.concatenate(masses)
        out = np.empty((int(p.row_off[-1]), 3))
        check(self.lib.tsc_inertia_moments_batch(self._h, ptr(p.flat), ptr(p.offsets), ptr(p.n_structs), ptr(p.n_atoms), ptr(all_masses),
                                                 C.c_int64(len(ensembles)), ptr(out)))
        return p.cut(out)

    def moi_first_similar_batch(self, moments, max_deviation):
        """moi_first_similar of every segment ([f64[N_s, 3]], one max_deviation each) in one launch: [i32[N_s]], indices inside the segment."""
        moments = [np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 3) for m in moments]
        dev = np.ascontiguousarray(max_deviation, dtype=np.float64)
        if dev.shape != (len(moments),):
            raise ValueError(f"{dev.size} max_deviation values for {len(moments)} segments")
        if not moments:
            return []
        n_structs = np.array([len(m) for m in moments], dtype=np.int32)      # (rows only: nothing here is (N, n, 3), so no segments.pack)
        rows = np.concatenate(([0], np.cumsum(n_structs.astype(np.int64))))
        all_moments = np.concatenate(moments)
        first = np.full(int(rows[-1]), -1, dtype=np.int32)
        check(self.lib.tsc_moi_first_similar_batch(self._h, ptr(all_moments), ptr(n_structs), ptr(dev), C.c_int64(len(moments)), ptr(first)))
        return [first[rows[s]:rows[s + 1]] for s in range(len(moments))]

    def embed_scores(self, structures, indices, distances):
        structures = np.ascontiguousarray(structures, dtype=np.float64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        distances = np.ascontiguousarray(distances, dtype=np.float64)
        n = len(structures)
        if indices.ndim != 3 or indices.shape[0] != n or indices.shape[2] != 2 or distances.shape != indices.shape[:2]:
            raise ValueError("indices must be (N, n_c, 2) and distances (N, n_c)")
        sc, err = np.zeros(n, dtype=np.float32), np.zeros(n)
        check(self.lib.tsc_embed_scores(self._h, ptr(structures), C.c_int64(n), C.c_int(structures.shape[1]), ptr(indices), ptr(distances),
                                        C.c_int(indices.shape[1]), ptr(sc), ptr(err)))
        return sc, err

    # ---- N1: string-embed pose parameters -------------------------------------------------------
    def string_embed_params(self, p1, p2, ref_vec, mol_vec, conf_pair, angles):
        """tscode/embeds.py:98-116 for every (site, angle): rot f64[S*A, 2, 3, 3], pos f64[S*A, 2, 3], conf_idx i32[S*A, 2]."""
        p1, p2, ref_vec, mol_vec = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (p1, p2, ref_vec, mol_vec))
        conf_pair = np.ascontiguousarray(np.atleast_2d(conf_pair), dtype=np.int32)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        S, A = len(p1), len(angles)
        if not (p1.shape == p2.shape == ref_vec.shape == mol_vec.shape == (S, 3)) or conf_pair.shape != (S, 2):
            raise ValueError("p1, p2, ref_vec, mol_vec must be (n_sites, 3) and conf_pair (n_sites, 2)")
        rot, pos, ci = np.empty((S * A, 2, 3, 3)), np.empty((S * A, 2, 3)), np.empty((S * A, 2), dtype=np.int32)
        check(self.lib.tsc_string_embed_params(self._h, ptr(p1), ptr(p2), ptr(ref_vec), ptr(mol_vec), ptr(conf_pair), C.c_int64(S), ptr(angles),
                                               C.c_int(A), ptr(rot), ptr(pos), ptr(ci)))
        return rot, pos, ci

    def cyclical_embed_params(self, start, end, direction, pivot, meanpoint, r0, r1, n_reactive, angle):
        """tscode/embeds.py:676-713 per (pose, molecule) row: rot f64[n, 3, 3], pos f64[n, 3]."""
        arrs = [np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (start, end, direction, pivot, meanpoint, r0, r1)]
        n_reactive = np.ascontiguousarray(n_reactive, dtype=np.int32)
        angle = np.ascontiguousarray(angle, dtype=np.float64)
        n = len(angle)
        if any(a.shape != (n, 3) for a in arrs) or n_reactive.shape != (n,):
            raise ValueError("all vector inputs must be (n, 3), n_reactive and angle (n,)")
        rot, pos = np.empty((n, 3, 3)), np.empty((n, 3))
        check(self.lib.tsc_cyclical_embed_params(self._h, *[ptr(a) for a in arrs], ptr(n_reactive), ptr(angle), C.c_int64(n), ptr(rot), ptr(pos)))
        return rot, pos

    # ---- N1: the embed loops as one call each ----------------------------------------------------
    def tfd_greedy_filter(self, tf_mat, thresh=10.0):
        """is_new_structure (tscode/embeds.py:47-69) over an ordered list of fingerprints f32[N, T]: bool[N]."""
        tf = np.ascontiguousarray(tf_mat, dtype=np.float32)
        if tf.ndim != 2:
            raise ValueError("tf_mat must be (N, n_quadruplets)")
        acc = np.zeros(len(tf), dtype=np.uint8)
        nk = C.c_int64()
        check(self.lib.tsc_tfd_greedy_filter(self._h, ptr(tf), C.c_int64(len(tf)), C.c_int(tf.shape[1]), C.c_double(float(thresh)), ptr(acc), C.byref(nk)))
        return acc.astype(bool)

    def string_embed(self, frags: FragmentSet, p1, p2, ref_vec, mol_vec, conf_pair, angles, clash_thresh, max_clashes, quadruplets, tfd_thresh=10.0,
                     want_poses=True):
        """tscode/embeds.py:91-120 for every (site, angle) candidate: (clash_ok bool[N], kept bool[N], poses f64[n_kept, n, 3] or None)."""
        if frags.n_mols != 2:
            raise ValueError("the string embed takes two fragments")
        p1, p2, ref_vec, mol_vec = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (p1, p2, ref_vec, mol_vec))
        conf_pair = np.ascontiguousarray(np.atleast_2d(conf_pair), dtype=np.int32)
        angles = np.ascontiguousarray(angles, dtype=np.float64)
        quads = np.ascontiguousarray(quadruplets, dtype=np.int32).reshape(-1, 4)
        S, A = len(p1), len(angles)
        if not (p1.shape == p2.shape == ref_vec.shape == mol_vec.shape == (S, 3)) or conf_pair.shape != (S, 2):
            raise ValueError("p1, p2, ref_vec, mol_vec must be (n_sites, 3) and conf_pair (n_sites, 2)")
        N = S * A
        ok, kept = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
        poses = np.empty((N, frags.n_total, 3)) if want_poses else None        # rows beyond n_kept are never touched
        n_pass, n_kept = C.c_int64(), C.c_int64()
        check(self.lib.tsc_string_embed(self._h, ptr(frags.flat), *frags.table_args()[:3], ptr(p1), ptr(p2), ptr(ref_vec), ptr(mol_vec), ptr(conf_pair),
                                        C.c_int64(S), ptr(angles), C.c_int(A), C.c_double(float(clash_thresh)), C.c_int64(int(max_clashes)),
                                        ptr(quads), C.c_int(len(quads)), C.c_double(float(tfd_thresh)), ptr(ok), ptr(kept), ptr(poses), C.c_int64(N),
                                        C.byref(n_pass), C.byref(n_kept)))
        return ok.astype(bool), kept.astype(bool), (poses[:n_kept.value].copy() if want_poses else None)

    def cyclical_embed(self, frags: FragmentSet, start, end, direction, pivot, meanpoint, r0, r1, n_reactive, angle, conf_idx, group_off, clash_thresh,
                       max_clashes, rmsd_thr=1.0, want_poses=True):
        """tscode/embeds.py:657-717 / :785-847 over rows = pose * n_mols + molecule: (clash_ok bool[N], kept bool[N], poses or None)."""
        arrs = [np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (start, end, direction, pivot, meanpoint, r0, r1)]
        n_reactive = np.ascontiguousarray(n_reactive, dtype=np.int32).ravel()
        angle = np.ascontiguousarray(angle, dtype=np.float64).ravel()
        conf_idx = np.ascontiguousarray(conf_idx, dtype=np.int32).ravel()
        group_off = np.ascontiguousarray(group_off, dtype=np.int32)
        rows = len(angle)
        if rows % frags.n_mols or any(a.shape != (rows, 3) for a in arrs) or n_reactive.shape != (rows,) or conf_idx.shape != (rows,):
            raise ValueError("every per-row input must have n_poses * n_mols rows")
        N = rows // frags.n_mols
        ok, kept = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
        poses = np.empty((N, frags.n_total, 3)) if want_poses else None
        n_pass, n_kept = C.c_int64(), C.c_int64()
        check(self.lib.tsc_cyclical_embed(self._h, ptr(frags.flat), *frags.table_args(), *[ptr(a) for a in arrs], ptr(n_reactive), ptr(angle), ptr(conf_idx),
                                          C.c_int64(N), ptr(group_off), C.c_int(len(group_off) - 1), C.c_double(float(clash_thresh)),
                                          C.c_int64(int(max_clashes)), C.c_double(float(rmsd_thr)), ptr(ok), ptr(kept), ptr(poses), C.c_int64(N),
                                          C.byref(n_pass), C.byref(n_kept)))
        return ok.astype(bool), kept.astype(bool), (poses[:n_kept.value].copy() if want_poses else None)

    def cyclical_embed_groups(self, frags: FragmentSet, start, end, direction, pivot, meanpoint, r0, r1, n_reactive, conf_idx, angles, clash_thresh,
                              max_clashes, rmsd_thr=1.0, want_poses=True):
        """``cyclical_embed`` from one record per (group, molecule), index = group * n_mols + molecule, and ONE angle table f64[A, n_mols] that every
        group walks: pose g * A + a is record g under angle set a.  (clash_ok bool[G * A], kept bool[G * A], poses or None)."""
        arrs = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3) for x in (start, end, direction, pivot, meanpoint, r0, r1)]
        n_reactive = np.ascontiguousarray(n_reactive, dtype=np.int32).ravel()
        conf_idx = np.ascontiguousarray(conf_idx, dtype=np.int32).ravel()
        angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1, frags.n_mols)
        items, A = len(n_reactive), len(angles)
        if items % frags.n_mols or any(a.shape != (items, 3) for a in arrs) or conf_idx.shape != (items,):
            raise ValueError("every per-group input must have n_groups * n_mols rows")
        G = items // frags.n_mols
        N = G * A
        ok, kept = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
        poses = np.empty((N, frags.n_total, 3)) if want_poses else None        # rows beyond n_kept are never touched
        n_pass, n_kept = C.c_int64(), C.c_int64()
        check(self.lib.tsc_cyclical_embed_groups(self._h, ptr(frags.flat), *frags.table_args(), *[ptr(a) for a in arrs], ptr(n_reactive), ptr(conf_idx),
                                                 ptr(angles), C.c_int64(G), C.c_int(A), C.c_double(float(clash_thresh)), C.c_int64(int(max_clashes)),
                                                 C.c_double(float(rmsd_thr)), ptr(ok), ptr(kept), ptr(poses), C.c_int64(N), C.byref(n_pass), C.byref(n_kept)))
        return ok.astype(bool), kept.astype(bool), (poses[:n_kept.value].copy() if want_poses else None)

    def embed_prune_run(self, frags: FragmentSet, heavy_idx):
        """An embed-and-prune run (tsc_embed_prune_*): the fragments go to the device once; ``add_groups`` per slab, ``run``, ``poses``."""
        return EmbedPruneRun(self, frags, heavy_idx)

    def trimolecular_groups(self, frags: FragmentSet, reactive, reactive_cumnums, conf, pivot, meanpoint, cumnums, tri_poly, tri_cost, directions, mask):
        """tsc_trimolecular_groups: the 23-field records of a three-molecule cyclical embed from per-triple arrays (tscode/embeds.py:312-465 inside
        :636-655).  ``reactive[m]`` 1 or 2 atom indices, ``reactive_cumnums[m]`` int[R <= 8, 2] = (atom, cumnum); per pivot triple ``conf`` i32[T, 3],
        ``pivot`` / ``meanpoint`` f64[T, 3, 3], ``cumnums`` i64[T, 3, 2], ``tri_poly`` / ``tri_cost`` f64[T, 3, 3] (the triangle before / after a right
        triangle's nudge), ``directions`` f64[T, 3, 3], ``mask`` u8[T] (bit v: orientation v is embedded).  Returns ``(blocks f64[G, 3, 23], group_ids
        i64[G, 3, 2], best i32[G], base i64[T])``, the groups compacted in (triple, orientation) order, ``base`` the first group of every triple."""
        if frags.n_mols != 3:
            raise ValueError("trimolecular_groups takes three fragments")
        react = np.zeros((3, 2), dtype=np.int32)
        n_react = np.zeros(3, dtype=np.int32)
        for m in range(3):
            r = np.atleast_1d(np.asarray(reactive[m], dtype=np.int64))
            if r.ndim != 1 or len(r) not in (1, 2):
                raise ValueError(f"molecule {m}: 1 or 2 reactive atoms, not {r.shape}")
            react[m, :len(r)], n_react[m] = r, len(r)
        tables = [np.asarray(t, dtype=np.int64).reshape(-1, 2) for t in reactive_cumnums]
        n_rows = np.array([len(t) for t in tables], dtype=np.int32)
        rows = np.ascontiguousarray(np.concatenate(tables)) if n_rows.sum() else np.zeros((1, 2), np.int64)
        conf = np.ascontiguousarray(conf, dtype=np.int32).reshape(-1, 3)
        T = len(conf)
        f9 = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3, 3) for x in (pivot, meanpoint, tri_poly, tri_cost, directions)]
        cumnums = np.ascontiguousarray(cumnums, dtype=np.int64).reshape(-1, 3, 2)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).ravel()
        if any(len(a) != T for a in f9) or len(cumnums) != T or len(mask) != T:
            raise ValueError("every per-triple input must have one row per pivot triple")
        per = np.unpackbits(mask[:, None], axis=1).sum(axis=1, dtype=np.int64)
        base = np.ascontiguousarray(np.concatenate([[0], np.cumsum(per)[:-1]]) if T else np.zeros(0), dtype=np.int64)
        G = int(per.sum())
        blocks, ids, best = np.zeros((G, 3, 23)), np.zeros((G, 3, 2), dtype=np.int64), np.zeros(G, dtype=np.int32)
        check(self.lib.tsc_trimolecular_groups(self._h, ptr(frags.flat), *frags.table_args()[:3], ptr(react), ptr(n_react), ptr(rows), ptr(n_rows), ptr(conf),
                                               ptr(f9[0]), ptr(f9[1]), ptr(cumnums), ptr(f9[2]), ptr(f9[3]), ptr(f9[4]), ptr(mask), ptr(base),
                                               C.c_int64(T), C.c_int64(G), ptr(blocks), ptr(ids), ptr(best)))
        return blocks, ids, best, base

    def trimolecular_groups_kernel_ms(self) -> float:
        """tsc_trimolecular_groups_timings: the kernel time of this thread's latest trimolecular_groups under set_option("pass_timing", 1)."""
        return self._kernel_ms(self.lib.tsc_trimolecular_groups_timings)

    # ---- N3: conformational-search rotations ---------------------------------------------------
    def csearch_rotate(self, coords, torsions, masks, angles, thresh=1.5, max_clashes=0):
        """Every candidate of tscode/torsion_module.py:463-500: (new_coords f64[M, n, 3], rotated_bonds i32[M])."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        torsions = np.ascontiguousarray(torsions, dtype=np.int32).reshape(-1, 4)
        n, nt = len(coords), len(torsions)
        masks = np.ascontiguousarray(masks, dtype=np.uint8).reshape(nt, n)
        angles = np.ascontiguousarray(angles, dtype=np.int32).reshape(-1, nt)
        if coords.ndim != 2 or coords.shape[1] != 3:
            raise ValueError("coords must be (n_atoms, 3)")
        out = np.empty((len(angles), n, 3))
        rb = np.zeros(len(angles), dtype=np.int32)
        check(self.lib.tsc_csearch_rotate(self._h, ptr(coords), C.c_int(n), ptr(torsions), ptr(masks), C.c_int(nt), ptr(angles),
                                          C.c_int64(len(angles)), C.c_double(thresh), C.c_int64(int(max_clashes)), ptr(out), ptr(rb)))
        return out, rb

    def csearch_rotate_dev(self, coords, n_atoms, torsions, masks, n_tors, angles, n_cand, thresh, max_clashes, out, rotated_bonds):
        """The same on device buffers (torch tensors / raw pointers), asynchronous on the engine's stream."""
        check(self.lib.tsc_csearch_rotate_dev(self._h, ptr(coords), C.c_int(n_atoms), ptr(torsions), ptr(masks), C.c_int(n_tors), ptr(angles),
                                              C.c_int64(n_cand), C.c_double(thresh), C.c_int64(int(max_clashes)), ptr(out), ptr(rotated_bonds)))

    def csearch_multi_plan(self, cand_start, start_set, set_off, n_atoms):
        """The work items i32[n_items, 4] of tsc_csearch_rotate_multi_dev for candidates in start order (host arrays, no device work)."""
        n_items = C.c_int64()
        args = (ptr(cand_start), C.c_int64(len(cand_start)), ptr(start_set), C.c_int(len(start_set)), ptr(set_off), C.c_int(len(set_off) - 1),
                C.c_int(n_atoms))
        check(self.lib.tsc_csearch_multi_plan(*args, None, C.c_int64(0), C.byref(n_items)))
        items = np.empty((n_items.value, 4), dtype=np.int32)
        check(self.lib.tsc_csearch_multi_plan(*args, ptr(items), C.c_int64(len(items)), C.byref(n_items)))
        return items

    def csearch_rotate_multi(self, starts, torsions, masks, set_off, start_set, angles, cand_start, cand_row, thresh=1.5, max_clashes=0):
        """tsc_csearch_rotate_multi on host arrays (include/tscode_hip.h): candidate m = start cand_start[m] turned by row cand_row[m]
        of angles i32[R, t_max] with the torsion set start_set[cand_start[m]].  Returns (new_coords f64[K, n, 3], rotated_bonds i32[K])."""
        S, n = starts.shape[:2]
        out = np.empty((len(cand_start), n, 3))
        rb = np.zeros(len(cand_start), dtype=np.int32)
        check(self.lib.tsc_csearch_rotate_multi(self._h, ptr(starts), C.c_int(S), C.c_int(n), ptr(torsions), ptr(masks), ptr(set_off),
                                                C.c_int(len(set_off) - 1), ptr(start_set), ptr(angles), C.c_int64(angles.shape[0]),
                                                C.c_int(angles.shape[1]), ptr(cand_start), ptr(cand_row), C.c_int64(len(cand_start)),
                                                C.c_double(thresh), C.c_int64(int(max_clashes)), ptr(out), ptr(rb)))
        return out, rb

    def csearch_rotate_multi_dev(self, starts, n_atoms, torsions, masks, set_off, angles, t_max, cand_start, cand_row, n_cand, items, n_items,
                                 thresh, max_clashes, out, rotated_bonds):
        """The same on device buffers, asynchronous on the engine's stream; set_off is a host array, items come from csearch_multi_plan."""
        check(self.lib.tsc_csearch_rotate_multi_dev(self._h, ptr(starts), C.c_int(n_atoms), ptr(torsions), ptr(masks), ptr(set_off),
                                                    C.c_int(len(set_off) - 1), ptr(angles), C.c_int(t_max), ptr(cand_start), ptr(cand_row),
                                                    C.c_int64(n_cand), ptr(items), C.c_int64(n_items), C.c_double(thresh),
                                                    C.c_int64(int(max_clashes)), ptr(out), ptr(rotated_bonds)))

    def csearch_select_dev(self, cand, rotated_bonds, n_atoms, seg_off, seg_start, seg_a0, n_seg, n_out, max_tries, kept_count, done,
                           rows_consumed, kept_rows, capacity):
        """tsc_csearch_select_dev: the stop rule of tscode/torsion_module.py:505-511 and the ordered compaction, on device buffers.
        n_out None = keep every rotated row.  Returns the number of rows written to kept_rows."""
        n_kept = C.c_int64()
        check(self.lib.tsc_csearch_select_dev(self._h, ptr(cand), ptr(rotated_bonds), C.c_int(n_atoms), ptr(seg_off), ptr(seg_start), ptr(seg_a0),
                                              C.c_int(n_seg), C.c_int(-1 if n_out is None else int(n_out)), C.c_int64(int(max_tries)),
                                              ptr(kept_count), ptr(done), ptr(rows_consumed), ptr(kept_rows), C.c_int64(capacity),
                                              C.byref(n_kept)))
        return n_kept.value

    # device memory of the context for the callers that keep buffers resident between calls (raw addresses: ptr() takes them)
    def dev_alloc(self, nbytes) -> int:
        p = C.c_void_p()
        check(self.lib.tsc_malloc(self._h, C.c_size_t(int(nbytes)), C.byref(p)))
        return p.value

    def dev_free(self, addr):
        check(self.lib.tsc_free(self._h, C.c_void_p(addr)))

    def dev_upload(self, host: np.ndarray) -> int:
        host = np.ascontiguousarray(host)
        addr = self.dev_alloc(host.nbytes)
        check(self.lib.tsc_memcpy_h2d(self._h, C.c_void_p(addr), ptr(host), C.c_size_t(host.nbytes)))
        return addr

    def dev_download(self, addr, host: np.ndarray):
        check(self.lib.tsc_memcpy_d2h(self._h, ptr(host), C.c_void_p(addr), C.c_size_t(host.nbytes)))
        return host

    def rotate_dihedral_batch(self, coords, torsion, mask, angles):
        """rotate_dihedral (tscode/utils.py:389-414) on structures f64[M, n, 3] sharing torsion and mask: structure s by angles[s]
        degrees (floats).  Returns the rotated copies."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        if coords.ndim != 3 or coords.shape[2] != 3:
            raise ValueError("coords must be (n_structs, n_atoms, 3)")
        torsion = np.ascontiguousarray(torsion, dtype=np.int32).reshape(4)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(coords.shape[1])
        angles = np.ascontiguousarray(np.broadcast_to(np.asarray(angles, dtype=np.float64), (len(coords),)))
        out = np.empty_like(coords)
        check(self.lib.tsc_rotate_dihedral(self._h, ptr(coords), C.c_int64(len(coords)), C.c_int(coords.shape[1]), ptr(torsion), ptr(mask),
                                           ptr(angles), ptr(out)))
        return out

    def torsion_comp_check(self, coords, torsion, mask, thresh=1.5, max_clashes=0):
        """ok i32[M] for structures f64[M, n, 3] sharing one torsion and mask (tscode/numba_functions.py:26-47)."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        if coords.ndim != 3 or coords.shape[2] != 3:
            raise ValueError("coords must be (n_structs, n_atoms, 3)")
        torsion = np.ascontiguousarray(torsion, dtype=np.int32).reshape(4)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(coords.shape[1])
        ok = np.zeros(len(coords), dtype=np.int32)
        check(self.lib.tsc_torsion_comp_check(self._h, ptr(coords), C.c_int64(len(coords)), C.c_int(coords.shape[1]), ptr(torsion), ptr(mask),
                                              C.c_double(thresh), C.c_int64(int(max_clashes)), ptr(ok)))
        return ok

    # ---- topology ---------------------------------------------------------------------------
    def bond_delta(self, coords, classes, thr, active=None, ref_bits=None, excluded=None, max_newbonds=0, want_counts=False, want_adj=False,
                   checked=False):
        """tsc_bond_delta on host arrays (include/tscode_hip.h): the bonds of every structure of coords f64[N, n, 3] from the class
        table thr f64[T, T], compared with the expected bonds ref_bits u64[n, W].  excluded: i32[E] shared or i32[N, E] per structure.
        Returns {"mask": bool[N]} plus "formed" / "broken" i32[N] (want_counts) and "adj" u64[N, n, W] (want_adj)."""
        if not checked:
            from .graph_manipulations import check_bond_delta_args
            coords, classes, thr, active, ref_bits, excluded = check_bond_delta_args(coords, classes, thr, active, ref_bits, excluded)
        n_structs, n = coords.shape[0], coords.shape[1]
        mask = np.zeros(n_structs, dtype=np.uint8)
        formed = np.zeros(n_structs, dtype=np.int32) if want_counts else None
        broken = np.zeros(n_structs, dtype=np.int32) if want_counts else None
        adj = np.zeros((n_structs, n, (n + 63) // 64), dtype=np.uint64) if want_adj else None
        n_excl = 0 if excluded is None else excluded.shape[-1]
        check(self.lib.tsc_bond_delta(self._h, ptr(coords), C.c_int64(n_structs), C.c_int(n), ptr(classes), ptr(thr), C.c_int(len(thr)), ptr(active),
                                      ptr(ref_bits), ptr(excluded), C.c_int(n_excl), C.c_int(int(excluded is not None and excluded.ndim == 2)),
                                      C.c_int64(int(max_newbonds)), ptr(mask), ptr(formed), ptr(broken), ptr(adj)))
        out = {"mask": mask.astype(bool)}
        if want_counts:
            out["formed"], out["broken"] = formed, broken
        if want_adj:
            out["adj"] = adj
        return out

    def bond_delta_dev(self, coords, n_structs, n_atoms, classes, thr, active, ref_bits, excluded, excl_per_struct, max_newbonds, mask,
                       formed=None, broken=None, adj=None):
        """tsc_bond_delta_dev: coords, mask, formed, broken, adj (and excluded i32[N, E] when excl_per_struct) on the device; classes
        u8[n], thr f64[T, T], active u8[n] | None, ref_bits u64[n, W] | None (and excluded i32[E] otherwise) NumPy arrays."""
        classes = np.ascontiguousarray(classes, dtype=np.uint8)
        thr = np.ascontiguousarray(thr, dtype=np.float64)
        active = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        ref_bits = None if ref_bits is None else np.ascontiguousarray(ref_bits, dtype=np.uint64)
        if excluded is None:
            n_excl = 0
        elif excl_per_struct:
            n_excl = int(excluded.shape[-1])
        else:
            excluded = np.ascontiguousarray(excluded, dtype=np.int32).ravel()
            n_excl = len(excluded)
        check(self.lib.tsc_bond_delta_dev(self._h, ptr(coords), C.c_int64(n_structs), C.c_int(n_atoms), ptr(classes), ptr(thr), C.c_int(len(thr)),
                                          ptr(active), ptr(ref_bits), ptr(excluded), C.c_int(n_excl), C.c_int(int(bool(excl_per_struct))),
                                          C.c_int64(int(max_newbonds)), ptr(mask), ptr(formed), ptr(broken), ptr(adj)))

    def _kernel_ms(self, timings) -> float:
        ms = C.c_float()
        check(timings(self._h, C.byref(ms)))
        return ms.value

    def topology_kernel_ms(self) -> float:
        """tsc_topology_timings: the kernel time of this thread's latest bond_delta / bond_delta_dev under set_option("pass_timing", 1)."""
        return self._kernel_ms(self.lib.tsc_topology_timings)

    # ---- hydrogen bonds and torsion reachability ------------------------------------------------
    def hbonds(self, coords, hetero, hydrogen, bonds, extra=None, d_min=2.5, d_max=3.3, max_angle=45.0, mode=0, max_hb=8, want_graph=False):
        """tsc_hbonds on host arrays (include/tscode_hip.h): coords f64[S, n, 3], hetero / hydrogen u8[n], bonds u64[S, n, W], extra
        i32[S, E, 2] | None.  Returns {"hb": i32[S, max_hb, 2] (-1 behind a structure's pairs), "n_hb": i32[S], "status": u8[S],
        "n_components_before": i32[S]} plus "graph" u64[S, n, W] (want_graph)."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        S, n = coords.shape[0], coords.shape[1]
        hetero, hydrogen = np.ascontiguousarray(hetero, dtype=np.uint8), np.ascontiguousarray(hydrogen, dtype=np.uint8)
        bonds = np.ascontiguousarray(bonds, dtype=np.uint64)
        extra = None if extra is None else np.ascontiguousarray(extra, dtype=np.int32)
        n_extra = 0 if extra is None else int(extra.shape[1])
        hb = np.full((S, max(int(max_hb), 0), 2), -1, dtype=np.int32)
        n_hb, status, before = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.uint8), np.zeros(S, dtype=np.int32)
        graph = np.zeros((S, n, (n + 63) // 64), dtype=np.uint64) if want_graph else None
        check(self.lib.tsc_hbonds(self._h, ptr(coords), C.c_int64(S), C.c_int(n), ptr(hetero), ptr(hydrogen), ptr(bonds),
                                  ptr(extra if n_extra else None), C.c_int(n_extra), C.c_double(d_min), C.c_double(d_max), C.c_double(max_angle),
                                  C.c_int(int(mode)), C.c_int(int(max_hb)), ptr(hb if hb.size else None), ptr(n_hb), ptr(status), ptr(before),
                                  ptr(graph)))
        out = {"hb": hb, "n_hb": n_hb, "status": status, "n_components_before": before}
        if want_graph:
            out["graph"] = graph
        return out

    def hbonds_dev(self, coords, n_structs, n_atoms, hetero, hydrogen, bonds, extra, n_extra, d_min, d_max, max_angle, mode, max_hb, hb, n_hb,
                   status, n_components_before=None, graph=None):
        """tsc_hbonds_dev: coords, bonds, extra and the outputs on the device, asynchronous on the engine's stream; hetero and hydrogen
        u8[n] NumPy arrays."""
        hetero, hydrogen = np.ascontiguousarray(hetero, dtype=np.uint8), np.ascontiguousarray(hydrogen, dtype=np.uint8)
        check(self.lib.tsc_hbonds_dev(self._h, ptr(coords), C.c_int64(n_structs), C.c_int(n_atoms), ptr(hetero), ptr(hydrogen), ptr(bonds),
                                      ptr(extra), C.c_int(n_extra), C.c_double(d_min), C.c_double(d_max), C.c_double(max_angle), C.c_int(int(mode)),
                                      C.c_int(int(max_hb)), ptr(hb), ptr(n_hb), ptr(status), ptr(n_components_before), ptr(graph)))

    def torsion_reach(self, graph, torsions, set_off, constrained=None):
        """tsc_torsion_reach on host arrays: graph u64[G, n, W], torsions i32[T, 4], set_off i32[G + 1], constrained i32[G, n_con] | None.
        Returns (flags u8[T]: bit 0 in_cycle, bit 1 reversed; masks u8[T, n])."""
        graph = np.ascontiguousarray(graph, dtype=np.uint64)
        G, n = graph.shape[0], graph.shape[1]
        torsions = np.ascontiguousarray(torsions, dtype=np.int32).reshape(-1, 4)
        set_off = np.ascontiguousarray(set_off, dtype=np.int32)
        constrained = None if constrained is None else np.ascontiguousarray(constrained, dtype=np.int32).reshape(G, -1)
        n_con = 0 if constrained is None else int(constrained.shape[1])
        flags, masks = np.zeros(len(torsions), dtype=np.uint8), np.zeros((len(torsions), n), dtype=np.uint8)
        check(self.lib.tsc_torsion_reach(self._h, ptr(graph), C.c_int(G), C.c_int(n), ptr(torsions), ptr(set_off),
                                         ptr(constrained if n_con else None), C.c_int(n_con), ptr(flags), ptr(masks)))
        return flags, masks

    def torsion_reach_dev(self, graph, n_graphs, n_atoms, torsions, set_off, constrained, n_con, flags, masks):
        """tsc_torsion_reach_dev: graph, torsions, constrained, flags and masks on the device; set_off a NumPy array."""
        set_off = np.ascontiguousarray(set_off, dtype=np.int32)
        check(self.lib.tsc_torsion_reach_dev(self._h, ptr(graph), C.c_int(n_graphs), C.c_int(n_atoms), ptr(torsions), ptr(set_off), ptr(constrained),
                                             C.c_int(n_con), ptr(flags), ptr(masks)))

    def torsions_kernel_ms(self):
        """tsc_torsions_timings: (hydrogen-bond kernel ms, reachability kernel ms) of this thread's latest calls under
        set_option("pass_timing", 1); -1 where none was taken."""
        ms = (C.c_float * 2)()
        check(self.lib.tsc_torsions_timings(self._h, ms))
        return float(ms[0]), float(ms[1])

    def torsion_groups(self, coords, torsions, set_off, max_size=5, min_torsions=9):
        """tsc_torsion_groups on host arrays: coords f64[S, n, 3], torsions i32[T, 4], set_off i32[S + 1].  Returns (group_of i32[T],
        n_groups i32[S], eps_index i32[S], oversize u8[S])."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        S, n = coords.shape[0], coords.shape[1]
        torsions = np.ascontiguousarray(torsions, dtype=np.int32).reshape(-1, 4)
        set_off = np.ascontiguousarray(set_off, dtype=np.int32)
        group_of = np.zeros(len(torsions), dtype=np.int32)
        n_groups, eps_index, oversize = np.zeros(S, dtype=np.int32), np.full(S, -1, dtype=np.int32), np.zeros(S, dtype=np.uint8)
        check(self.lib.tsc_torsion_groups(self._h, ptr(coords), C.c_int(S), C.c_int(n), ptr(torsions), ptr(set_off), C.c_int(int(max_size)),
                                          C.c_int(int(min_torsions)), ptr(group_of), ptr(n_groups), ptr(eps_index), ptr(oversize)))
        return group_of, n_groups, eps_index, oversize

    def torsion_groups_dev(self, coords, n_structs, n_atoms, torsions, set_off, max_size, min_torsions, group_of, n_groups, eps_index, oversize):
        """tsc_torsion_groups_dev: coords, torsions and the four outputs on the device; set_off a NumPy array."""
        set_off = np.ascontiguousarray(set_off, dtype=np.int32)
        check(self.lib.tsc_torsion_groups_dev(self._h, ptr(coords), C.c_int(n_structs), C.c_int(n_atoms), ptr(torsions), ptr(set_off),
                                              C.c_int(int(max_size)), C.c_int(int(min_torsions)), ptr(group_of), ptr(n_groups), ptr(eps_index),
                                              ptr(oversize)))

    def torsion_groups_kernel_ms(self) -> float:
        """tsc_torsion_groups_timings: the kernel time of this thread's latest torsion_groups[_dev] under set_option("pass_timing", 1)."""
        return self._kernel_ms(self.lib.tsc_torsion_groups_timings)

    # ---- non-covalent interactions -----------------------------------------------------------
    def nci(self, coords, classes, thr, atom_mol, n_mols, candidate, ring_thr, ring_ring_thr, constrained=None, owner_rule=0, want=()):
        """tsc_nci on host arrays (include/tscode_hip.h), already checked (tscode_amd.nci.check_nci_args): coords f64[N, n, 3], classes
        u8[n], thr f64[T, T], atom_mol u8[n], candidate u8[n], ring_thr f64[T], constrained i32[E] shared or i32[N, E] per structure.
        Returns {"counts": i32[N, 4], "overflow": bool[N]} plus the arrays named in ``want``."""
        n_structs, n = coords.shape[0], coords.shape[1]
        w = (n + 63) // 64
        shapes = {"pair_bits": ((n_structs, n, w), np.uint64), "ring_atoms": ((n_structs, 64, 6), np.uint16),
                  "ring_owner": ((n_structs, 64), np.uint8), "ring_center": ((n_structs, 64, 3), np.float64),
                  "ring_atom_bits": ((n_structs, 64, w), np.uint64), "ring_ring_bits": ((n_structs, 64), np.uint64)}
        out = {name: (np.zeros(*shapes[name]) if name in want else None) for name in shapes}
        counts = np.zeros((n_structs, 4), dtype=np.int32)
        overflow = np.zeros(n_structs, dtype=np.uint8)
        thr = np.ascontiguousarray(thr, dtype=np.float64)
        ring_thr = np.ascontiguousarray(ring_thr, dtype=np.float64)
        n_con = 0 if constrained is None else constrained.shape[-1]
        check(self.lib.tsc_nci(self._h, ptr(coords), C.c_int64(n_structs), C.c_int(n), ptr(np.ascontiguousarray(classes, dtype=np.uint8)), ptr(thr),
                               C.c_int(len(thr)), ptr(np.ascontiguousarray(atom_mol, dtype=np.uint8)), C.c_int(int(n_mols)),
                               ptr(np.ascontiguousarray(candidate, dtype=np.uint8)), ptr(ring_thr), C.c_double(float(ring_ring_thr)),
                               ptr(constrained), C.c_int(n_con), C.c_int(int(constrained is not None and constrained.ndim == 2)),
                               C.c_int(int(owner_rule)), ptr(counts), ptr(overflow), *[ptr(out[name]) for name in shapes]))
        res = {"counts": counts, "overflow": overflow.astype(bool)}
        res.update({name: arr for name, arr in out.items() if arr is not None})
        return res

    def nci_dev(self, coords, n_structs, n_atoms, classes, thr, atom_mol, n_mols, candidate, ring_thr, ring_ring_thr, constrained, con_per_struct,
                owner_rule, counts, overflow, pair_bits=None, ring_atoms=None, ring_owner=None, ring_center=None, ring_atom_bits=None,
                ring_ring_bits=None):
        """tsc_nci_dev: coords, counts, overflow and the optional outputs (and constrained i32[N, E] when con_per_struct) on the device;
        classes u8[n], thr f64[T, T], atom_mol u8[n], candidate u8[n], ring_thr f64[T] (and constrained i32[E] otherwise) NumPy arrays.
        Enqueued on the context's stream."""
        classes = np.ascontiguousarray(classes, dtype=np.uint8)
        thr = np.ascontiguousarray(thr, dtype=np.float64)
        atom_mol = np.ascontiguousarray(atom_mol, dtype=np.uint8)
        candidate = np.ascontiguousarray(candidate, dtype=np.uint8)
        ring_thr = np.ascontiguousarray(ring_thr, dtype=np.float64)
        if constrained is None:
            n_con = 0
        elif con_per_struct:
            n_con = int(constrained.shape[-1])
        else:
            constrained = np.ascontiguousarray(constrained, dtype=np.int32).ravel()
            n_con = len(constrained)
        check(self.lib.tsc_nci_dev(self._h, ptr(coords), C.c_int64(n_structs), C.c_int(n_atoms), ptr(classes), ptr(thr), C.c_int(len(thr)),
                                   ptr(atom_mol), C.c_int(int(n_mols)), ptr(candidate), ptr(ring_thr), C.c_double(float(ring_ring_thr)),
                                   ptr(constrained), C.c_int(n_con), C.c_int(int(bool(con_per_struct))), C.c_int(int(owner_rule)), ptr(counts),
                                   ptr(overflow), ptr(pair_bits), ptr(ring_atoms), ptr(ring_owner), ptr(ring_center), ptr(ring_atom_bits),
                                   ptr(ring_ring_bits)))

    def nci_kernel_ms(self) -> float:
        """tsc_nci_timings: the kernel time of this thread's latest nci / nci_dev under set_option("pass_timing", 1)."""
        return self._kernel_ms(self.lib.tsc_nci_timings)

    # ---- reactive-atom orbitals and pivots ----------------------------------------------------
    def orbitals(self, coords, recipes, sigmatropic_mode=0, suprafacial=False, want_pivots=True):
        """tsc_orbitals on host arrays (include/tscode_hip.h), already checked (tscode_amd.reactive_atoms): coords f64[C, n, 3], recipes a
        record array of reactive_atoms.RECIPE_DTYPE.  Returns the arrays of the header by name; the four pivot arrays with want_pivots."""
        n_conf, n = coords.shape[0], coords.shape[1]
        recipes = np.ascontiguousarray(recipes)
        r = len(recipes)
        out = {"centers": np.zeros((n_conf, r, 4, 3)), "orb_vecs": np.zeros((n_conf, r, 4, 3)), "n_lobes": np.zeros((n_conf, r), dtype=np.uint8),
               "kind": np.zeros((n_conf, r), dtype=np.uint8), "sigmatropic": np.zeros(n_conf, dtype=np.uint8)}
        piv = {"pivot": np.zeros((n_conf, 16, 3)), "meanpoint": np.zeros((n_conf, 16, 3)), "lobe_index": np.full((n_conf, 16, 2), -1, dtype=np.int8),
               "n_pivots": np.zeros(n_conf, dtype=np.uint8)} if want_pivots else dict.fromkeys(("pivot", "meanpoint", "lobe_index", "n_pivots"))
        check(self.lib.tsc_orbitals(self._h, ptr(coords), C.c_int64(n_conf), C.c_int(n), ptr(recipes), C.c_int(r), C.c_int(int(sigmatropic_mode)),
                                    C.c_int(int(bool(suprafacial))), *[ptr(v) for v in out.values()], *[ptr(v) for v in piv.values()]))
        out["sigmatropic"] = out["sigmatropic"].astype(bool)
        if want_pivots:
            out.update(piv)
        return out

    def orbitals_dev(self, coords, n_conf, n_atoms, recipes, sigmatropic_mode, suprafacial, centers, orb_vecs, n_lobes, kind, sigmatropic,
                     pivot=None, meanpoint=None, lobe_index=None, n_pivots=None):
        """tsc_orbitals_dev: coords and every output on the device, recipes a NumPy record array.  Enqueued on the context's stream."""
        recipes = np.ascontiguousarray(recipes)
        check(self.lib.tsc_orbitals_dev(self._h, ptr(coords), C.c_int64(n_conf), C.c_int(n_atoms), ptr(recipes), C.c_int(len(recipes)),
                                        C.c_int(int(sigmatropic_mode)), C.c_int(int(bool(suprafacial))), ptr(centers), ptr(orb_vecs), ptr(n_lobes),
                                        ptr(kind), ptr(sigmatropic), ptr(pivot), ptr(meanpoint), ptr(lobe_index), ptr(n_pivots)))

    def orbitals_kernel_ms(self) -> float:
        """tsc_orbitals_timings: the kernel time of this thread's latest orbitals / orbitals_dev under set_option("pass_timing", 1)."""
        return self._kernel_ms(self.lib.tsc_orbitals_timings)

    def prune_heavy(self, heavy, rmsd_thr=0.5, mode=0):
        """prune_conformers_rmsd on the heavy-atom array f64[N, h, 3]. Returns (mask bool[N], per-pass stats)."""
        heavy = np.ascontiguousarray(heavy, dtype=np.float64)
        if heavy.ndim != 3 or heavy.shape[2] != 3:
            raise ValueError("heavy must be (N, h, 3)")
        n, h = heavy.shape[0], heavy.shape[1]
        mask = np.zeros(n, dtype=np.uint8)
        stats = (PassStats * TSC_MAX_PASSES)()
        np_ = C.c_int()
        check(self.lib.tsc_prune_rmsd(self._h, ptr(heavy), C.c_int64(n), C.c_int(h), C.c_double(rmsd_thr), C.c_int(mode), ptr(mask),
                                      stats, C.byref(np_)))
        return mask.astype(bool), _stats_list(stats, np_.value)

    def _prune_segments(self, entry, heavies, thr, mode):
        """One call of tsc_prune_rmsd_batch or tsc_prune_rmsd_team (`entry`) on heavy-atom arrays already checked: (masks, stats,
        nonfinite) per ensemble."""
        packed = segments.pack(heavies)
        B = len(heavies)
        mask = np.zeros(int(packed.row_off[-1]), dtype=np.uint8)
        st = (BatchPassStats * (B * TSC_MAX_PASSES))()
        np_ = np.zeros(B, dtype=np.int32)
        nf = np.zeros(B, dtype=np.uint8)
        t = np.ascontiguousarray(thr, dtype=np.float64)
        check(entry(self._h, ptr(packed.flat), packed.offsets.ctypes.data_as(_lib.c_i64p), packed.n_structs.ctypes.data_as(_lib.c_i32p),
                    packed.n_atoms.ctypes.data_as(_lib.c_i32p), t.ctypes.data_as(_lib.c_f64p), C.c_int64(B), C.c_int(int(mode)),
                    ptr(mask), st, np_.ctypes.data_as(_lib.c_i32p), nf.ctypes.data_as(_lib.c_u8p)))
        table = np.frombuffer(st, dtype=np.int64).reshape(B, TSC_MAX_PASSES, len(_BATCH_STAT_FIELDS))
        masks = [m.astype(bool) for m in packed.cut(mask)]
        stats = [[dict(zip(_BATCH_STAT_FIELDS, map(int, row))) for row in table[b, :np_[b]]] for b in range(B)]
        return masks, stats, nf.astype(bool)

    @staticmethod
    def _checked_heavies(heavies, rmsd_thr):
        heavies = [np.ascontiguousarray(a, dtype=np.float64) for a in heavies]
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(rmsd_thr, dtype=np.float64), (len(heavies),)))
        for s, a in enumerate(heavies):
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"ensemble {s}: heavy must be (N, h, 3), got {a.shape}")
            if a.shape[1] < 1:
                raise ValueError(f"ensemble {s}: no heavy atoms")
        return heavies, thr

    def prune_heavy_batch(self, heavies, rmsd_thr=0.5, mode=0, team_max_n=None):
        """prune_conformers_rmsd on many heavy-atom arrays f64[N_s, h_s, 3] (rmsd_thr a scalar or one per ensemble).  Three routes by
        size: ensembles of at most "prune_batch_max_n" structures go through tsc_prune_rmsd_batch in ONE launch, a workgroup each; the
        longer ones of at most ``team_max_n`` (None: PRUNE_TEAM_MAX_N; 0: nobody) through tsc_prune_rmsd_team in ONE call, a team of
        workgroups each; a still longer one takes prune_heavy on its own, which spreads a pass over the device.  Returns (masks, stats,
        nonfinite): per ensemble the mask bool[N_s], the list of its passes (k, n_active_before, n_active_after, pairs_evaluated,
        new_keys) and whether it holds a NaN or infinite coordinate (bool[S])."""
        team_max_n = check_team_max_n(team_max_n)
        heavies, thr = self._checked_heavies(heavies, rmsd_thr)
        S = len(heavies)
        masks, stats, nonfinite = [None] * S, [None] * S, np.zeros(S, dtype=bool)
        max_n = self.prune_batch_max_n
        small = [s for s in range(S) if heavies[s].shape[0] <= max_n]
        mid = [s for s in range(S) if max_n < heavies[s].shape[0] <= team_max_n]
        for entry, which in ((self.lib.tsc_prune_rmsd_batch, small), (self.lib.tsc_prune_rmsd_team, mid)):
            if which:
                m, st, nf = self._prune_segments(entry, [heavies[s] for s in which], thr[which], mode)
                for b, s in enumerate(which):
                    masks[s], stats[s], nonfinite[s] = m[b], st[b], nf[b]
        for s in range(S):
            if masks[s] is None:
                masks[s], full = self.prune_heavy(heavies[s], float(thr[s]), mode)
                stats[s] = [{f: int(p[f]) for f in _BATCH_STAT_FIELDS} for p in full]
                nonfinite[s] = bool(full and full[0].get("nonfinite_input"))
        return masks, stats, nonfinite

    def prune_heavy_team(self, heavies, rmsd_thr=0.5, mode=0):
        """prune_conformers_rmsd on many heavy-atom arrays f64[N_s, h_s, 3] through tsc_prune_rmsd_team alone, whatever their sizes up to
        TSC_PRUNE_TEAM_MAX_N: one call, a team of workgroups per ensemble.  Returns (masks, stats, nonfinite) as prune_heavy_batch."""
        heavies, thr = self._checked_heavies(heavies, rmsd_thr)
        if not heavies:
            return [], [], np.zeros(0, dtype=bool)
        return self._prune_segments(self.lib.tsc_prune_rmsd_team, heavies, thr, mode)

    def _prune_segments_dev(self, entry, heavy, offsets, n, h, rmsd_thr, mode, mask, stats, n_passes, nonfinite):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        h = np.ascontiguousarray(h, dtype=np.int32)
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(rmsd_thr, dtype=np.float64), n.shape))
        st = C.cast(ptr(stats), C.POINTER(BatchPassStats)) if stats is not None else None
        check(entry(self._h, ptr(heavy), offsets.ctypes.data_as(_lib.c_i64p), n.ctypes.data_as(_lib.c_i32p), h.ctypes.data_as(_lib.c_i32p),
                    thr.ctypes.data_as(_lib.c_f64p), C.c_int64(len(n)), C.c_int(int(mode)), ptr(mask), st, ptr(n_passes), ptr(nonfinite)))

    def prune_heavy_batch_dev(self, heavy, offsets, n, h, rmsd_thr, mode, mask, stats=None, n_passes=None, nonfinite=None):
        """tsc_prune_rmsd_batch_dev: heavy f64 and the outputs mask u8[sum n], stats (i64[S, TSC_MAX_PASSES, 5]), n_passes i32[S] and
        nonfinite u8[S] on the device (torch tensors or raw pointers; the last three optional), the tables offsets / n / h / rmsd_thr
        NumPy arrays (pack_heavy_batch).  Every ensemble must have at most "prune_batch_max_n" structures.  Synchronises."""
        self._prune_segments_dev(self.lib.tsc_prune_rmsd_batch_dev, heavy, offsets, n, h, rmsd_thr, mode, mask, stats, n_passes, nonfinite)

    def prune_heavy_team_dev(self, heavy, offsets, n, h, rmsd_thr, mode, mask, stats=None, n_passes=None, nonfinite=None):
        """tsc_prune_rmsd_team_dev: the arguments of prune_heavy_batch_dev; every ensemble must have at most TSC_PRUNE_TEAM_MAX_N
        structures.  Synchronises."""
        self._prune_segments_dev(self.lib.tsc_prune_rmsd_team_dev, heavy, offsets, n, h, rmsd_thr, mode, mask, stats, n_passes, nonfinite)

    def prune_structures(self, structures, heavy_idx, rmsd_thr=0.5, mode=0):
        """The same from all-atom structures f64[N, n_atoms, 3] (C-contiguous) and the indices of the heavy atoms: the gather of
        tscode/rmsd_pruning.py:178-179 runs on the device (on the host it costs ten times the prune at 57k structures)."""
        n, na = structures.shape[0], structures.shape[1]
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        mask = np.zeros(n, dtype=np.uint8)
        stats = (PassStats * TSC_MAX_PASSES)()
        np_ = C.c_int()
        check(self.lib.tsc_prune_structures(self._h, ptr(structures), C.c_int64(n), C.c_int(na), heavy_idx.ctypes.data_as(_lib.c_i32p),
                                            C.c_int(len(heavy_idx)), C.c_double(rmsd_thr), C.c_int(mode), ptr(mask), stats, C.byref(np_)))
        return mask.astype(bool), _stats_list(stats, np_.value)

    def prune_heavy_dev(self, heavy, n, h, rmsd_thr, mode, mask):
        stats = (PassStats * TSC_MAX_PASSES)()
        np_ = C.c_int()
        check(self.lib.tsc_prune_rmsd_dev(self._h, ptr(heavy), C.c_int64(n), C.c_int(h), C.c_double(rmsd_thr), C.c_int(mode),
                                          ptr(mask), stats, C.byref(np_)))
        return _stats_list(stats, np_.value)

    def prune_stepper(self, heavy_dev, n, h, rmsd_thr, mode):
        return PruneStepper(self, heavy_dev, n, h, rmsd_thr, mode)

    # ---- pipeline -----------------------------------------------------------------------------
    def pipeline_dev(self, frags: FragmentSet, frags_dev, conf_idx, rot, pos, n_poses, heavy_idx, clash_thresh, max_clashes,
                     rmsd_thr, mode, clash_mask, structures, keep_mask, keep_mask_host=None):
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        n_pass, n_keep = C.c_int64(), C.c_int64()
        stats = (PassStats * TSC_MAX_PASSES)()
        np_ = C.c_int()
        tm = (C.c_float * 4)()
        check(self.lib.tsc_pipeline_dev(self._h, ptr(frags_dev), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos),
                                        C.c_int64(n_poses), heavy_idx.ctypes.data_as(_lib.c_i32p), C.c_int(len(heavy_idx)),
                                        C.c_double(clash_thresh), C.c_int64(int(max_clashes)), C.c_double(rmsd_thr), C.c_int(mode),
                                        ptr(clash_mask), ptr(structures), ptr(keep_mask), ptr(keep_mask_host), C.byref(n_pass),
                                        C.byref(n_keep), stats,
                                        C.byref(np_), tm))
        return PipelineResult(n_pass.value, n_keep.value, stats, np_.value, tm)

    def pipeline_dev_prepare(self, frags: FragmentSet, frags_dev, conf_idx, rot, pos, n_poses, heavy_idx, clash_thresh, max_clashes,
                             rmsd_thr, mode, clash_mask, structures, keep_mask, keep_mask_host=None):
        """The same call with every argument converted once: returns run() -> PipelineResult for callers that repeat the
        step on resident buffers (the ctypes conversions of 25 arguments are host time in front of the first launch)."""
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        fixed = (self._h, ptr(frags_dev), *frags.table_args(), ptr(conf_idx), ptr(rot), ptr(pos), C.c_int64(n_poses),
                 heavy_idx.ctypes.data_as(_lib.c_i32p), C.c_int(len(heavy_idx)), C.c_double(clash_thresh), C.c_int64(int(max_clashes)),
                 C.c_double(rmsd_thr), C.c_int(mode), ptr(clash_mask), ptr(structures), ptr(keep_mask), ptr(keep_mask_host))
        keep_alive = (frags, frags_dev, conf_idx, rot, pos, heavy_idx, clash_mask, structures, keep_mask, keep_mask_host)
        fn, byref = self.lib.tsc_pipeline_dev, C.byref
        stats_t, tm_t = PassStats * TSC_MAX_PASSES, C.c_float * 4

        def run(_keep=keep_alive):
            n_pass, n_keep, np_ = C.c_int64(), C.c_int64(), C.c_int()
            stats, tm = stats_t(), tm_t()
            check(fn(*fixed, byref(n_pass), byref(n_keep), stats, byref(np_), tm))
            return PipelineResult(n_pass.value, n_keep.value, stats, np_.value, tm)

        return run


class ContextObject:
    """What every object created from an engine's context is (include/tscode_hip.h, "objects created from a context"): the engine, the
    library's handle and the name of the tsc_*_destroy that takes it.  The engine knows its objects and closes them before its context
    goes; ``close()`` may be called any number of times, and after it the handle is ``None``."""

    _handle = None                           # (until _own: a constructor that raised leaves nothing to close)
    _r = _p = _x = property(lambda self: self._handle)     # the names the classes call their handle by

    def _own(self, engine, handle, destroy):
        self.e, self._handle, self._destroy = engine, handle, destroy
        engine._runs.add(self)               # closed with the engine, before its context goes

    def close(self):
        if self._handle:
            # a closed engine has destroyed its objects already: tsc_ctx_destroy destroys what the context still lists, also an
            # object the engine no longer knew (Engine.close), and the handle is not to be used again
            if getattr(self.e, "_h", None):
                getattr(self.e.lib, self._destroy)(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IpcExchange(ContextObject):
    """The exchange inside the library (include/tscode_hip.h, tsc_xchg_*): a receive area of fine-grained device memory per rank, mapped
    into every other rank of the node; an all-reduce is one kernel that writes into all peers and one that waits for their flags and
    folds what they delivered.  ``handle`` (64 bytes) has to reach every other rank -- the caller's business (``connect_over`` does it
    with torch.distributed) -- then ``connect(handles in rank order)``."""

    def __init__(self, engine: Engine, rank, world, slot_bytes):
        self.rank, self.world = int(rank), int(world)
        x = C.c_void_p()
        buf = C.create_string_buffer(_lib.XCHG_HANDLE_BYTES)
        check(engine.lib.tsc_xchg_create(engine._h, C.c_int(rank), C.c_int(world), C.c_int64(int(slot_bytes)), C.byref(x), buf))
        self.handle = bytes(buf.raw)
        self._own(engine, x, "tsc_xchg_destroy")

    @staticmethod
    def slot_bytes(lib, n, mode=0) -> int:
        b = C.c_int64()
        check(lib.tsc_xchg_slot_bytes(C.c_int64(int(n)), C.c_int(mode), C.byref(b)))
        return b.value

    def connect(self, handles):
        handles = [bytes(h) for h in handles]
        if len(handles) != self.world or any(len(h) != _lib.XCHG_HANDLE_BYTES for h in handles):
            raise ValueError("connect() takes the 64-byte handle of every rank, in rank order")
        check(self.e.lib.tsc_xchg_connect(self._x, C.c_char_p(b"".join(handles))))

    def connect_over(self, dist, group=None):
        """All-gather the handles over a torch.distributed process group and map the peers."""
        handles = [None] * self.world
        dist.all_gather_object(handles, self.handle, group=group)
        self.connect(handles)
        dist.barrier(group=group)            # every rank has mapped every area before the first exchange writes into one

    def set_timeout(self, seconds):
        check(self.e.lib.tsc_xchg_set_timeout(self._x, C.c_double(seconds)))

    def allreduce(self, kind, buf_dev, count):
        """In place over the ranks, enqueued on the engine's stream: kind = XCHG_SUM_I64 / XCHG_MIN_I32 (tscode_amd._lib)."""
        check(self.e.lib.tsc_xchg_allreduce(self._x, C.c_int(kind), ptr(buf_dev), C.c_int64(int(count))))

    def status(self):
        """(exchanges made, exchanges that gave up waiting for a peer).  Read it after a synchronisation."""
        n, t = C.c_int64(), C.c_int()
        check(self.e.lib.tsc_xchg_status(self._x, C.byref(n), C.byref(t)))
        return n.value, t.value

    def check_status(self):
        n, t = self.status()
        if t:
            raise _lib.TscodeHipError(-5, f"{t} of {n} in-library exchanges gave up waiting for a peer rank (tsc_xchg_set_timeout): the results of "
                                     "the runs they belonged to are not valid")


class EmbedPruneRun(ContextObject):
    """One embed-and-prune run (include/tscode_hip.h, tsc_embed_prune_*): a cyclical embed whose kept poses stay on the device, are pruned by
    RMSD there, and of which only the poses asked for are embedded again and fetched."""

    def __init__(self, engine: Engine, frags: FragmentSet, heavy_idx):
        self.frags = frags
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32).ravel()
        r = C.c_void_p()
        check(engine.lib.tsc_embed_prune_create(engine._h, ptr(frags.flat), *frags.table_args(), heavy_idx.ctypes.data_as(_lib.c_i32p),
                                                C.c_int(len(heavy_idx)), C.byref(r)))
        self.n_survived = None
        self._own(engine, r, "tsc_embed_prune_destroy")

    def add_groups(self, start, end, direction, pivot, meanpoint, r0, r1, n_reactive, conf_idx, angles, clash_thresh, max_clashes, rmsd_thr=1.0):
        """One slab of groups, arguments as ``Engine.cyclical_embed_groups``: (clash_ok bool[G * A], kept bool[G * A]); the kept poses stay on
        the device, behind those of the slabs before."""
        nm = self.frags.n_mols
        arrs = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3) for x in (start, end, direction, pivot, meanpoint, r0, r1)]
        n_reactive = np.ascontiguousarray(n_reactive, dtype=np.int32).ravel()
        conf_idx = np.ascontiguousarray(conf_idx, dtype=np.int32).ravel()
        angles = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1, nm)
        items, A = len(n_reactive), len(angles)
        if items % nm or any(a.shape != (items, 3) for a in arrs) or conf_idx.shape != (items,):
            raise ValueError("every per-group input must have n_groups * n_mols rows")
        G = items // nm
        ok, kept = np.zeros(G * A, dtype=np.uint8), np.zeros(G * A, dtype=np.uint8)
        n_pass, n_kept = C.c_int64(), C.c_int64()
        check(self.e.lib.tsc_embed_prune_add_groups(self._r, *[ptr(a) for a in arrs], ptr(n_reactive), ptr(conf_idx), ptr(angles), C.c_int64(G), C.c_int(A),
                                                    C.c_double(float(clash_thresh)), C.c_int64(int(max_clashes)), C.c_double(float(rmsd_thr)), ptr(ok),
                                                    ptr(kept), C.byref(n_pass), C.byref(n_kept)))
        return ok.astype(bool), kept.astype(bool)

    def count(self) -> int:
        n = C.c_int64()
        check(self.e.lib.tsc_embed_prune_count(self._r, C.byref(n)))
        return n.value

    def run(self, rmsd_thr=0.5, mode=0):
        """prune_conformers_rmsd over the kept poses: (survived bool[n_kept], per-pass statistics)."""
        survived = np.zeros(max(self.count(), 1), dtype=np.uint8)
        stats = (PassStats * TSC_MAX_PASSES)()
        np_, ns = C.c_int(), C.c_int64()
        check(self.e.lib.tsc_embed_prune_run(self._r, C.c_double(float(rmsd_thr)), C.c_int(int(mode)), ptr(survived), stats, C.byref(np_), C.byref(ns)))
        self.n_survived = ns.value
        return survived[:self.count()].astype(bool), _stats_list(stats, np_.value)

    def poses(self, which=0):
        """which = 0: the poses that survived ``run``; 1: every kept pose.  f64[rows, n_total, 3], embedded from their parameters on the device."""
        rows = self.count() if which else self.n_survived
        if rows is None:
            rows = 0                         # (which = 0 before run(): the library refuses it, with its message)
        out = np.empty((max(rows, 1), self.frags.n_total, 3))
        if rows or not which:
            check(self.e.lib.tsc_embed_prune_poses(self._r, C.c_int(int(which)), ptr(out), C.c_int64(rows)))
        return out[:rows]


class PruneStepper(ContextObject):
    """Stepping form of one prune run (tsc_prune_*), used to shard a pass over ranks."""

    def __init__(self, engine: Engine, heavy_dev, n, h, rmsd_thr, mode):
        self.n = int(n)
        h_ = C.c_void_p()
        check(engine.lib.tsc_prune_create(engine._h, ptr(heavy_dev), C.c_int64(n), C.c_int(h), C.c_double(rmsd_thr), C.c_int(mode),
                                          C.byref(h_)))
        self._keep = heavy_dev
        self._own(engine, h_, "tsc_prune_destroy")

    def next_pass(self) -> int:
        k = C.c_int64()
        check(self.e.lib.tsc_prune_next_pass(self._p, C.byref(k)))
        return k.value

    def pass_estimate(self) -> int:
        n = C.c_int64()
        check(self.e.lib.tsc_prune_pass_estimate(self._p, C.byref(n)))
        return n.value

    def run_replicated(self, world, min_pairs) -> int:
        """Every pass that needs no exchange, in one call; returns the k of the first pass that does (left open) or 0."""
        k = C.c_int64()
        check(self.e.lib.tsc_prune_run_replicated(self._p, C.c_int(world), C.c_int64(int(min_pairs)), C.byref(k)))
        return k.value

    def pass_local(self, rank=0, world=1):
        check(self.e.lib.tsc_prune_pass_local(self._p, C.c_int(rank), C.c_int(world)))

    def pass_rows(self, rank, world):
        """The pair search of another rank's row tiles of the open pass (after pass_local), into the same best[]."""
        check(self.e.lib.tsc_prune_pass_rows(self._p, C.c_int(rank), C.c_int(world)))

    # ---- rank-partitioned passes (include/tscode_hip.h) ----
    @staticmethod
    def exchange_words(lib, n, mode) -> int:
        w = C.c_int64()
        check(lib.tsc_prune_exchange_words(C.c_int64(int(n)), C.c_int(mode), C.byref(w)))
        return w.value

    def set_partition(self, rank, world, min_chunks_per_rank, exch_dev):
        """exch_dev: device tensor of at least exchange_words(n) int64 that the caller can all-reduce."""
        check(self.e.lib.tsc_prune_set_partition(self._p, C.c_int(rank), C.c_int(world), C.c_int(min_chunks_per_rank), ptr(exch_dev),
                                                 C.c_int64(exch_dev.numel())))
        self._keep_exch = exch_dev

    def pass_partitioned(self) -> bool:
        f = C.c_int()
        check(self.e.lib.tsc_prune_pass_partitioned(self._p, C.byref(f)))
        return bool(f.value)

    def pass_range(self):
        check(self.e.lib.tsc_prune_pass_range(self._p))

    def pass_merge(self):
        check(self.e.lib.tsc_prune_pass_merge(self._p))

    def views_range(self):
        """(offset, words) of the block of the exchange buffer that holds the cache views of the passes still to run, to be summed
        over the ranks before the open (not partitioned) pass; words = 0: nothing to exchange."""
        p, off, n = C.c_void_p(), C.c_int64(), C.c_int64()
        check(self.e.lib.tsc_prune_views_ptr(self._p, C.byref(p), C.byref(off), C.byref(n)))
        return off.value, n.value

    def views_merged(self):
        check(self.e.lib.tsc_prune_views_merged(self._p))

    def best_ptr(self):
        p, n = C.c_void_p(), C.c_int64()
        check(self.e.lib.tsc_prune_best_ptr(self._p, C.byref(p), C.byref(n)))
        return p.value, n.value

    def use_best_buffer(self, best_dev):
        check(self.e.lib.tsc_prune_use_best_buffer(self._p, ptr(best_dev)))
        self._keep_best = best_dev

    def pass_finish(self):
        check(self.e.lib.tsc_prune_pass_finish(self._p))

    def run_sharded(self, rank, world, min_chunks_per_rank, min_pairs, exch_dev, exchange):
        """The whole pass loop of a sharded run in ONE library call (tsc_prune_run_sharded): the library walks the schedule and calls
        ``exchange(kind, ptr, count)`` for every collective -- kind XCHG_SUM_I64 / XCHG_MIN_I32 (tscode_amd._lib), ``ptr`` the device
        address of ``count`` elements to reduce over the ranks in place, in stream order with the context's stream.  Returns the list
        of exchanges made as (k, kind, count); k < 0 = the cache views in front of pass -k.  An exception raised by ``exchange``
        aborts the run and is re-raised here."""
        from ._lib import EXCHANGE_FN, ExchangeRecord
        failure = []
        user = None
        if isinstance(exchange, IpcExchange):
            # the library's own exchange (tsc_xchg_allreduce has the signature of tsc_exchange_fn): the pass loop calls it directly,
            # no Python frame per collective
            cb, user = C.cast(self.e.lib.tsc_xchg_allreduce, EXCHANGE_FN), exchange._x
        elif exchange is not None:
            def _cb(_user, kind, buf, count):
                try:
                    exchange(int(kind), int(buf), int(count))
                    return 0
                except BaseException as exc:  # noqa: BLE001  (must not propagate through the C frames)
                    failure.append(exc)
                    return 1
            cb = EXCHANGE_FN(_cb)
        else:
            cb = C.cast(None, EXCHANGE_FN)     # (no callback: a world of one needs none)
        log = (ExchangeRecord * (2 * TSC_MAX_PASSES + 2))()
        n_log = C.c_int()
        rc = self.e.lib.tsc_prune_run_sharded(self._p, C.c_int(rank), C.c_int(world), C.c_int(min_chunks_per_rank), C.c_int64(int(min_pairs)),
                                              ptr(exch_dev), C.c_int64(exch_dev.numel() if exch_dev is not None else 0), cb, user, log,
                                              C.c_int(len(log)), C.byref(n_log))
        if failure:
            raise failure[0]
        check(rc)
        if exch_dev is not None:
            self._keep_exch = exch_dev
        return [(log[i].k, log[i].kind, log[i].count) for i in range(n_log.value)]

    def mask_ptr(self) -> int:
        p = C.c_void_p()
        check(self.e.lib.tsc_prune_mask_dev(self._p, C.byref(p)))
        return p.value

    def copy_mask(self, dst_dev):
        check(self.e.lib.tsc_prune_copy_mask_dev(self._p, ptr(dst_dev)))

    def stats(self):
        stats = (PassStats * TSC_MAX_PASSES)()
        np_ = C.c_int()
        check(self.e.lib.tsc_prune_stats(self._p, stats, C.byref(np_)))
        return _stats_list(stats, np_.value)


_engines = {}
_engines_lock = threading.Lock()


def get_engine(device: int | None = None) -> Engine:
    """Process-wide engine for a device (default: LOCAL_RANK or 0).  multiembed-style use from several
    processes is safe: each process owns its own HIP context (Threading)."""
    import os
    if device is None:
        device = int(os.environ.get("TSCODE_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _engines_lock:
        eng = _engines.get(device)
        if eng is None:
            eng = _engines[device] = Engine(device)
    return eng
