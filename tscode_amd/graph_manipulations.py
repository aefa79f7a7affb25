"""tscode/graph_manipulations.py on the MI355X engine: the bond graph from distances (graphize, :33-55; d_min_bond, :28-29) and,
built on it, the batched forms of the topology checks of tscode/utils.py (molecule_check :341-353, scramble_check :355-387,
get_double_bonds_indices :293-314) -- one wavefront per structure (csrc/topology.hpp, k_bond_delta).

The batched forms take a whole ensemble that shares its ``atomnos`` and return one verdict per structure; the drop-ins with the
reference's signatures (graphize here, the other three in tscode_amd.utils) are single-structure calls of them.  Every input is
checked and refused with ValueError BEFORE the library is loaded; nothing handed in is modified.

Bond graphs travel as packed bits: ``uint64[n, W]``, W = ceil(n / 64), bit (j & 63) of word j >> 6 of row i set for a bond i < j
(strict upper triangle; the self loops graphize adds are put on by the drop-in).
"""

from __future__ import annotations

import importlib
import sys

import numpy as np

from .engine import get_engine

__all__ = ["MAX_ATOMS", "MAX_CLASSES", "MAX_EXCLUDED", "covalent_radii", "d_min_bond", "bond_tables", "double_bond_tables", "pack_edges",
           "edges_from_bits", "bond_graph_batch", "scramble_mask", "molecule_check_mask", "double_bonds_batch", "graphize",
           "check_bond_delta_args"]

MAX_ATOMS = 512          # csrc/topology.hpp: TP_MAX_ATOMS
MAX_CLASSES = 16         # TP_MAX_CLASSES
MAX_EXCLUDED = 16        # TP_MAX_EXCL

# Covalent radii / A of the elements the project's fixtures use: the values periodictable ships (Cordero 2008), typed in as in
# tests/golden/_reference.py:ELEMENTS and, like them, not checkable where periodictable is not installed.  The last resort of
# covalent_radii() only: a live tscode.pt or an installed periodictable is asked first.
_BUILTIN_RADII = {1: 0.31, 6: 0.76, 7: 0.71, 8: 0.66, 9: 0.57, 16: 1.05, 17: 1.02}

_DOUBLE_BOND_THRESHOLDS = {(6, 6): 1.4, (6, 7): 1.3}       # tscode/utils.py:288-291 ('CC', 'CN')


# ------------------------------------------------------------------------------------------------------- tables
def _radius_sources(radii):
    """The places a covalent radius is looked up in, in order; each is a function Z -> float or None."""
    def explicit(z):
        v = radii.get(z) if hasattr(radii, "get") else None
        return None if v is None else float(v)

    def live_tscode(z):
        mod = sys.modules.get("tscode.pt")                  # only a tscode that somebody else imported: never imported from here
        try:
            return None if mod is None else float(mod.pt[z].covalent_radius)
        except Exception:  # noqa: BLE001  (an element that table lacks, or a radius of None)
            return None

    state = {}

    def periodictable(z):
        if "mod" not in state:
            try:
                state["mod"] = importlib.import_module("periodictable")
            except ImportError:
                state["mod"] = None
        try:
            return None if state["mod"] is None else float(state["mod"].elements[z].covalent_radius)
        except Exception:  # noqa: BLE001
            return None

    def builtin(z):
        return _BUILTIN_RADII.get(z)

    return ([explicit] if radii is not None else []) + [live_tscode, periodictable, builtin]


def covalent_radii(atomnos, radii=None):
    """Covalent radius / A of every atom, f64[n].  Each element is looked up in: ``radii`` (a mapping Z -> radius) when given, the
    ``pt`` table of a tscode that is ALREADY imported (``tscode.pt`` in sys.modules; tscode is never imported from here),
    ``periodictable`` if it can be imported, the built-in table of seven elements (H C N O F S Cl).  An element none of them knows
    raises ValueError."""
    z_all = _atomnos_array(atomnos)
    sources = _radius_sources(radii)
    known = {}
    for z in sorted(set(z_all.tolist())):
        for src in sources:
            r = src(z)
            if r is not None:
                if not (np.isfinite(r) and r >= 0.0):
                    raise ValueError(f"covalent radius {r} of element {z} is negative or not finite")
                known[z] = r
                break
        else:
            raise ValueError(f"no covalent radius known for element {z}: pass radii={{{z}: ...}}")
    return np.array([known[z] for z in z_all.tolist()], dtype=np.float64)


def d_min_bond(e1, e2, radii=None):
    """tscode/graph_manipulations.py:28-29: the largest distance at which two elements still count as bonded."""
    r = covalent_radii([e1, e2], radii)
    return 1.2 * (float(r[0]) + float(r[1]))


def _atomnos_array(atomnos):
    z = np.asarray(atomnos)
    if z.ndim != 1 or z.dtype == bool or not np.issubdtype(z.dtype, np.integer):
        raise ValueError("atomnos must be a one-dimensional array of integers")
    return z.astype(np.int64)


def bond_tables(atomnos, radii=None):
    """(classes u8[n], thr f64[T, T]): the distinct elements of ``atomnos`` in ascending order are the classes, thr[p, q] is the
    reference's ``1.2 * (r_p + r_q)`` in fp64."""
    z = _atomnos_array(atomnos)
    elements = sorted(set(z.tolist()))
    if len(elements) > MAX_CLASSES:
        raise ValueError(f"{len(elements)} distinct elements: the engine takes at most {MAX_CLASSES}")
    r = [float(v) for v in covalent_radii(elements, radii)] if elements else []
    thr = np.array([[1.2 * (r1 + r2) for r2 in r] for r1 in r], dtype=np.float64).reshape(len(r), len(r))
    index = {e: c for c, e in enumerate(elements)}
    return np.array([index[v] for v in z.tolist()], dtype=np.uint8), thr


def double_bond_tables(atomnos):
    """(classes, thr, active) of get_double_bonds_indices (tscode/utils.py:288-314): heavy atoms only, C-C below 1.4 A, C-N below
    1.3 A, every other pair never (threshold 0)."""
    z = _atomnos_array(atomnos)
    classes = np.where(z == 6, 0, np.where(z == 7, 1, 2)).astype(np.uint8)
    thr = np.zeros((3, 3))
    thr[0, 0] = _DOUBLE_BOND_THRESHOLDS[(6, 6)]
    thr[0, 1] = thr[1, 0] = _DOUBLE_BOND_THRESHOLDS[(6, 7)]
    return classes, thr, (z != 1)


# ------------------------------------------------------------------------------------------------------- packed graphs
def pack_edges(edges, n_atoms):
    """Bonds int[E, 2] (either order; a == b dropped) -> packed u64[n, W]."""
    w = (n_atoms + 63) // 64
    bits = np.zeros((n_atoms, w), dtype=np.uint64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if e.size and (e.min() < 0 or e.max() >= n_atoms):
        raise ValueError(f"bond index out of range for {n_atoms} atoms")
    lo, hi = e.min(axis=1), e.max(axis=1)
    keep = lo != hi
    np.bitwise_or.at(bits, (lo[keep], hi[keep] >> 6), np.uint64(1) << (hi[keep] & 63).astype(np.uint64))
    return bits


def edges_from_bits(row_words):
    """Packed u64[n, W] -> the bonds int32[E, 2], i < j, ordered by i then j."""
    rows = np.ascontiguousarray(row_words, dtype=np.uint64)
    if rows.ndim != 2:
        raise ValueError("edges_from_bits takes one structure's rows, u64[n, W]")
    dense = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little") if sys.byteorder == "little" else None
    if dense is None:   # pragma: no cover  (big-endian hosts)
        dense = ((rows[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(len(rows), -1).astype(np.uint8)
    i, j = np.nonzero(dense)
    return np.stack([i, j], axis=1).astype(np.int32)


def _graph_edges(graphs, n_atoms):
    """scramble_check's bond set (tscode/utils.py:363-369): the molecules' graphs, read by duck type (.nodes, .edges), shifted by
    the atoms in front of them."""
    sizes = [len(g.nodes) for g in graphs]
    if sum(sizes) != n_atoms:
        raise ValueError(f"the graphs hold {sum(sizes)} atoms, the structures {n_atoms}")
    out, pos = [], 0
    for g, size in zip(graphs, sizes):
        out += [(int(a) + pos, int(b) + pos) for a, b in list(g.edges) if a != b]
        pos += size
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def _is_graph_list(obj):
    return isinstance(obj, (list, tuple)) and len(obj) > 0 and all(hasattr(g, "nodes") and hasattr(g, "edges") for g in obj)


# ------------------------------------------------------------------------------------------------------- checks
def _structures_array(structures, n_atoms):
    x = np.ascontiguousarray(structures, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"structures of shape {x.shape}: expected (n_structures, n_atoms, 3)")
    if x.shape[1] != n_atoms:
        raise ValueError(f"{x.shape[1]} atoms per structure, {n_atoms} atomic numbers")
    if not 1 <= n_atoms <= MAX_ATOMS:
        raise ValueError(f"{n_atoms} atoms per structure: the engine takes 1 .. {MAX_ATOMS}")
    if not np.isfinite(x).all():
        raise ValueError("structures contain NaN or infinity")
    return x


def check_bond_delta_args(coords, classes, thr, active=None, ref_bits=None, excluded=None):
    """The arrays of tsc_bond_delta, converted and checked against the limits of include/tscode_hip.h; ValueError on the first
    violation.  Returns (coords f64[N, n, 3], classes u8[n], thr f64[T, T], active u8[n] | None, ref_bits u64[n, W] | None,
    excluded i32[E] | i32[N, E] | None)."""
    classes = np.ascontiguousarray(classes)
    if classes.ndim != 1 or not np.issubdtype(classes.dtype, np.integer):
        raise ValueError("classes must be a one-dimensional array of integers")
    n = len(classes)
    coords = _structures_array(coords, n)
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    if thr.ndim != 2 or thr.shape[0] != thr.shape[1] or not 1 <= thr.shape[0] <= MAX_CLASSES:
        raise ValueError(f"thr of shape {thr.shape}: expected (T, T) with 1 <= T <= {MAX_CLASSES}")
    if not (np.isfinite(thr).all() and (thr >= 0).all()):
        raise ValueError("thr holds a negative or non-finite threshold")
    if classes.min() < 0 or classes.max() >= len(thr):
        raise ValueError(f"class {int(classes.max() if classes.min() >= 0 else classes.min())} with {len(thr)} classes")
    classes = classes.astype(np.uint8)
    w = (n + 63) // 64
    if active is not None:
        active = np.ascontiguousarray(active)
        if active.shape != (n,):
            raise ValueError(f"mask of shape {active.shape} for {n} atoms")
        active = active.astype(bool).astype(np.uint8)
    if ref_bits is not None:
        ref_bits = np.ascontiguousarray(ref_bits, dtype=np.uint64)
        if ref_bits.shape != (n, w):
            raise ValueError(f"ref_bits of shape {ref_bits.shape}: expected ({n}, {w})")
        cols = np.arange(64 * w)
        allowed = pack_dense((cols[None, :] > np.arange(n)[:, None]) & (cols[None, :] < n))
        if (ref_bits & ~allowed).any():
            raise ValueError("ref_bits has bits outside the strict upper triangle")
    if excluded is not None:
        excluded = np.asarray(excluded)
        if excluded.size and not np.issubdtype(excluded.dtype, np.integer):
            raise ValueError("excluded atoms must be integers")
        if excluded.ndim == 2 and excluded.shape[0] != len(coords):
            raise ValueError(f"excluded atoms for {excluded.shape[0]} structures, {len(coords)} structures")
        if excluded.ndim not in (1, 2):
            raise ValueError("excluded atoms: expected shape (E,) or (n_structures, E)")
        if excluded.shape[-1] > MAX_EXCLUDED:
            raise ValueError(f"{excluded.shape[-1]} excluded atoms per structure: the engine takes at most {MAX_EXCLUDED}")
        if excluded.size and (excluded.min() < -1 or excluded.max() >= n):
            raise ValueError(f"excluded atom index outside -1 .. {n - 1}")
        excluded = np.ascontiguousarray(excluded, dtype=np.int32)
        if excluded.shape[-1] == 0:
            excluded = None
    return coords, classes, thr, active, ref_bits, excluded


def pack_dense(dense):
    """bool[n, 64 W] -> u64[n, W]."""
    d = np.ascontiguousarray(dense, dtype=bool)
    words = d.reshape(len(d), -1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(words, axis=2)


def _run(coords, classes, thr, active, ref_bits, excluded, max_newbonds, counts, adj):
    args = check_bond_delta_args(coords, classes, thr, active, ref_bits, excluded)
    max_newbonds = int(max_newbonds)
    return get_engine().bond_delta(*args, max_newbonds=max_newbonds, want_counts=counts, want_adj=adj, checked=True)


# ------------------------------------------------------------------------------------------------------- batched forms
def bond_graph_batch(structures, atomnos, mask=None, radii=None):
    """graphize for a whole ensemble: the bonds of every structure as packed bits u64[N, n, W] (strict upper triangle; ``mask``
    as graphize's: atoms with False take part in no bond)."""
    classes, thr = bond_tables(atomnos, radii)
    return _run(structures, classes, thr, mask, None, None, 0, False, True)["adj"]


def _reference_bits(bonds_or_graphs, n_atoms):
    if _is_graph_list(bonds_or_graphs):
        return pack_edges(_graph_edges(bonds_or_graphs, n_atoms), n_atoms)
    e = np.asarray(bonds_or_graphs)
    if e.size == 0:
        return pack_edges(np.zeros((0, 2), dtype=np.int64), n_atoms)
    if e.ndim != 2 or e.shape[1] != 2 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError("bonds_or_graphs: an (E, 2) array of atom indices or a list of graphs (.nodes, .edges)")
    return pack_edges(e, n_atoms)


def scramble_mask(structures, atomnos, excluded_atoms, bonds_or_graphs, max_newbonds=0, return_counts=False, radii=None):
    """scramble_check (tscode/utils.py:355-387) for a whole ensemble: True where at most ``max_newbonds`` bonds formed or broke
    with respect to the expected bonds, pairs that touch an excluded atom not counted.

    excluded_atoms    int[E] shared by all structures, or int[N, E] per structure (-1 = unused slot), E <= 16
    bonds_or_graphs   the expected bonds as an (E, 2) array in whole-system indices, or the list of per-molecule graphs that
                      scramble_check takes (anything with .nodes and .edges; shifted by the atoms in front of each)
    return_counts     also return (formed i32[N], broken i32[N])"""
    classes, thr = bond_tables(atomnos, radii)
    ref = _reference_bits(bonds_or_graphs, len(classes))
    res = _run(structures, classes, thr, None, ref, excluded_atoms, max_newbonds, return_counts, False)
    return (res["mask"], res["formed"], res["broken"]) if return_counts else res["mask"]


def molecule_check_mask(old_coords, structures, atomnos, max_newbonds=0, return_counts=False, radii=None):
    """molecule_check (tscode/utils.py:341-353) of every structure against ``old_coords``."""
    classes, thr = bond_tables(atomnos, radii)
    old = _structures_array(old_coords, len(classes))
    if len(old) != 1:
        raise ValueError("old_coords is one structure")
    new = _structures_array(structures, len(classes))
    ref = _run(old, classes, thr, None, None, None, 0, False, True)["adj"][0]
    res = _run(new, classes, thr, None, ref, None, max_newbonds, return_counts, False)
    return (res["mask"], res["formed"], res["broken"]) if return_counts else res["mask"]


def double_bonds_batch(structures, atomnos):
    """get_double_bonds_indices (tscode/utils.py:293-314) of every structure: a list of int32[E, 2] arrays, (i, j) in the original
    numbering, ordered by i then j."""
    classes, thr, heavy = double_bond_tables(atomnos)
    adj = _run(structures, classes, thr, heavy, None, None, 0, False, True)["adj"]
    return [edges_from_bits(rows) for rows in adj]


# ------------------------------------------------------------------------------------------------------- drop-in
def graphize(coords, atomnos, mask=None):
    """Drop-in for tscode.graph_manipulations.graphize (:33-55): the connectivity graph on nodes 0 .. n-1, a self loop on every
    active atom (the reference's loop starts at j = i), every edge with weight 1.0 as from_numpy_matrix leaves it, and the
    ``atomnos`` node attribute."""
    import networkx as nx
    atomnos = np.asarray(atomnos)
    n = len(atomnos)
    active = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    bits = bond_graph_batch(np.asarray(coords, dtype=np.float64), atomnos, None if mask is None else active)[0]
    graph = nx.Graph()
    graph.add_nodes_from(range(n))
    graph.add_edges_from([(int(i), int(i)) for i in np.nonzero(active)[0]], weight=1.0)
    graph.add_edges_from([(int(a), int(b)) for a, b in edges_from_bits(bits)], weight=1.0)
    nx.set_node_attributes(graph, dict(enumerate(atomnos)), "atomnos")
    return graph
