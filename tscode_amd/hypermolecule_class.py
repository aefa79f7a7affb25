"""tscode/hypermolecule_class.py on the MI355X engine: align_structures (:38-72), one wavefront per structure
(csrc/diverse.hpp: dv_align_structures, k_align_structures)."""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, ptr
from .engine import get_engine

__all__ = ["align_structures"]

MAX_ATOMS = 512          # csrc/diverse.hpp: DV_MAX_ATOMS


def _index_array(indices, n_atoms):
    """:48-51: a list / tuple / array of atom indices, ravelled; None or empty = every atom."""
    if indices is None or len(indices) == 0:
        return None
    idx = np.asarray(indices).ravel()
    if idx.dtype == bool or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("align_structures: indices must be integers")
    idx = np.where(idx < 0, idx + n_atoms, idx)
    if idx.min() < 0 or idx.max() >= n_atoms:
        raise ValueError(f"align_structures: index out of range for {n_atoms} atoms")
    return np.ascontiguousarray(idx, dtype=np.int32)


def _check_structures(structures):
    if structures.ndim != 3 or structures.shape[2] != 3 or len(structures) == 0:
        raise ValueError(f"structures of shape {structures.shape}: expected (n_structures >= 1, n_atoms, 3)")
    if not 1 <= structures.shape[1] <= MAX_ATOMS:
        raise ValueError(f"{structures.shape[1]} atoms per structure: the engine takes 1 .. {MAX_ATOMS}")
    if not np.isfinite(structures).all():
        raise ValueError("structures contain NaN or infinity")


def align_structures(structures, indices=None, **kwargs):
    """Drop-in for tscode.hypermolecule_class.align_structures (:38-72): every structure centred on the mean of its indexed atoms,
    structures 1 .. N-1 turned onto structure 0 by the best proper rotation of the indexed atoms (all atoms when ``indices`` is
    None or empty).  Returns a new array.

    Like the reference, it also leaves the CALLER's array centred when that array is a float64 ndarray (``reference -= ...`` and
    ``targets[t] -= ...`` act on views of it, :53-55).  The reference's ``LinAlgError -> identity`` branch has no counterpart:
    the device solver does not fail."""
    src = structures if isinstance(structures, np.ndarray) else np.asarray(structures, dtype=np.float64)
    _check_structures(src)
    idx = _index_array(indices, src.shape[1])
    work = np.ascontiguousarray(src, dtype=np.float64)
    out = np.empty_like(work)
    eng = get_engine()
    check(eng.lib.tsc_align_structures(eng._h, ptr(work), C.c_int64(len(work)), C.c_int(work.shape[1]), ptr(idx),
                                       C.c_int(0 if idx is None else len(idx)), ptr(out)))
    if isinstance(structures, np.ndarray) and structures.dtype == np.float64:
        structures -= (structures if idx is None else structures[:, idx]).mean(axis=1, keepdims=True)       # :53-55, vectorised
    return out
