"""The argument lists of the many-ensembles calls, once: a list of ensembles, "one value for all or one per ensemble", the packed
form the library takes, and the slices of a list that is too long for one upload.  Host code only: nothing here imports the
engine or touches a device, so a front end built on it has checked its arguments before the library is entered."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

__all__ = ["ensemble_list", "one_or_each", "scalar_or_each", "pack", "Packed", "byte_slices"]


def ensemble_list(ensembles, dtype=None):
    """``ensembles`` as a list of (N_s, n_s >= 1, 3) arrays, in the caller's dtype or contiguous in ``dtype``; ValueError otherwise."""
    if isinstance(ensembles, np.ndarray) and ensembles.ndim != 4:
        raise ValueError("ensembles must be a list of (N, n_atoms, 3) arrays")
    ens = [np.asarray(e) if dtype is None else np.ascontiguousarray(e, dtype=dtype) for e in ensembles]
    for s, e in enumerate(ens):
        if e.ndim != 3 or e.shape[2] != 3 or e.shape[1] < 1:
            raise ValueError(f"ensemble {s}: structures must be (N, n_atoms, 3)")
    return ens


def one_or_each(value, S, what, item_ndim, allow_none=False, exact=False, count=True, object_rows=False):
    """``value`` as a list of S entries, where one entry is an array of ``item_ndim`` dimensions.

    A dict stands for all ensembles.  So does a value whose rank is at most ``item_ndim``; the rank is an array's ndim, and for any
    other sequence one more than its first entry's (1 when it is empty).  Anything else must have S entries:
    ValueError ``"{len(value)} {what} for {S} ensembles"``.

    exact        only a rank of exactly ``item_ndim`` stands for all: a flat or an empty list is no (T, 4) array
    item_ndim    None: nothing but a dict stands for all (lists with None entries, such as seeds)
    allow_none   None gives S times None
    object_rows  an array of dtype object never stands for all: it holds one entry per ensemble (arrays of different lengths)
    count        False leaves the count to the caller (similarity_refining_batch names two counts in one message)"""
    if value is None and allow_none:
        return [None] * S
    one = isinstance(value, dict)
    if not one and item_ndim is not None and not (object_rows and isinstance(value, np.ndarray) and value.dtype == object):
        rank = value.ndim if isinstance(value, np.ndarray) else 1 + (np.ndim(value[0]) if len(value) else 0)
        one = rank == item_ndim if exact else rank <= item_ndim
    if one:
        return [value] * S
    if count and len(value) != S:
        raise ValueError(f"{len(value)} {what} for {S} ensembles")
    return list(value)


def scalar_or_each(value, S, what):
    """``value`` as a contiguous f64[S]: a scalar for all ensembles, or one value each."""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(S, float(a))
    if a.shape != (S,):
        raise ValueError(f"{a.size} {what} for {S} ensembles")
    return np.ascontiguousarray(a)


class Packed(NamedTuple):
    """Arrays f64[N_s, n_s, 3] back to back, as the batch entry points of include/tscode_hip.h take them."""
    flat: np.ndarray            # f64[sum N n 3]
    offsets: np.ndarray         # i64[S + 1], in doubles
    n_structs: np.ndarray       # i32[S]
    n_atoms: np.ndarray         # i32[S]
    row_off: np.ndarray         # i64[S + 1], in structures

    def cut(self, result, doubles=False):
        """The per-ensemble views of ``result``: one entry per structure along its first axis, or (``doubles``) one per packed
        double, which come back in the shape (N_s, n_s, 3)."""
        if doubles:
            off = self.offsets.tolist()
            return [result[off[s]:off[s + 1]].reshape(N, n, 3) for s, (N, n) in enumerate(zip(self.n_structs.tolist(), self.n_atoms.tolist()))]
        off = self.row_off.tolist()
        return [result[a:b] for a, b in zip(off, off[1:])]


def pack(arrays):
    """The Packed form of a list of contiguous f64[N_s, n_s, 3] arrays (an empty list: no doubles, offsets [0])."""
    n = np.array([a.shape[0] for a in arrays], dtype=np.int32)
    h = np.array([a.shape[1] for a in arrays], dtype=np.int32)
    offsets, row_off = np.zeros(len(arrays) + 1, dtype=np.int64), np.zeros(len(arrays) + 1, dtype=np.int64)
    np.cumsum(n.astype(np.int64) * h * 3, out=offsets[1:])
    np.cumsum(n, dtype=np.int64, out=row_off[1:])
    flat = np.concatenate([a.ravel() for a in arrays]) if arrays else np.zeros(0)
    return Packed(flat, offsets, n, h, row_off)


def byte_slices(costs, budget):
    """The (at, end) slices of a list whose entries cost ``costs`` bytes, greedily: a slice takes its first entry whatever it costs
    and every further one while the sum stays within ``budget``."""
    out, at = [], 0
    while at < len(costs):
        end, total = at + 1, costs[at]
        while end < len(costs) and total + costs[end] <= budget:
            total += costs[end]
            end += 1
        out.append((at, end))
        at = end
    return out
