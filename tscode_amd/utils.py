"""Mirror of the three helpers of tscode/utils.py the embed loops call.

Host-side NumPy: they run once per (conformer pair, pivot pair), not once per pose.  Pinned by the reference's own
outputs in tests/golden/G10_embed_helpers.npz.

And the drop-ins of its topology checks (molecule_check :341-353, scramble_check :355-387, get_double_bonds_indices :293-314):
single-structure calls of the batched forms of tscode_amd.graph_manipulations, which run on the GPU (csrc/topology.hpp).
"""

from __future__ import annotations

import numpy as np

from .algebra import rotation_matrix_from_vectors  # noqa: F401  (tscode/utils.py:183-208 lives with the 3x3 helpers)

__all__ = ["TriangleError", "cartesian_product", "polygonize", "rotation_matrix_from_vectors", "molecule_check", "scramble_check",
           "get_double_bonds_indices"]


class TriangleError(Exception):
    """tscode/errors.py: raised by polygonize when three lengths do not close a triangle."""


def cartesian_product(*arrays):
    """tscode/utils.py:180-181: all combinations, as rows, in the order NumPy's meshgrid ('xy' indexing) gives them -- NOT
    lexicographic: for two inputs the FIRST index varies fastest ([0 0] [1 0] [0 1] [1 1] ...), for three the third varies
    fastest, then the first, then the second.  The expression is kept as it is because the order of every embed loop
    (conformer pairs, centre pairs, pivots, angle sets) is whatever it produces; pinned by fixture G10."""
    return np.stack(np.meshgrid(*arrays), -1).reshape(-1, len(arrays))


# Which sides of the triangle run backwards (end -> start) in each of the reference's eight orientation patterns, in its order
# (tscode/utils.py:253: the enumeration every trimolecular loop walks; data, pinned by fixture G10)
_TRIANGLE_REVERSED = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 1, 0], [1, 0, 1], [1, 1, 1]], dtype=bool)
_SEGMENT_REVERSED = np.array([[0, 0], [0, 1]], dtype=bool)          # two pivots: the second orientation turns the second segment round


def _oriented(sides, reversed_):
    """sides f64[S, 2, 3] (start, end) under every orientation pattern reversed_[T, S] -> f64[T, S, 2, 3]."""
    return np.where(reversed_[:, :, None, None], sides[None, :, ::-1, :], sides[None])


def polygonize(lengths):
    """tscode/utils.py:210-261: where a cyclical embed puts its pivots -- per orientation pattern, per pivot, a (start, end) pair.

    Two lengths: two segments centred on the origin along x, superposed; the second pattern reverses the second -> f64[2, 2, 2, 3].
    Three lengths: the sides of the triangle (0,0,0) - (L0,0,0) - (x,y,0) walked head to tail, under the reference's eight
    reversal patterns -> f64[8, 3, 2, 3]; TriangleError when the lengths violate the triangle inequality."""
    L = [float(v) for v in lengths]
    if len(L) == 2:
        sides = np.zeros((2, 2, 3))
        sides[:, 0, 0], sides[:, 1, 0] = [-L[0] / 2, -L[1] / 2], [L[0] / 2, L[1] / 2]
        return _oriented(sides, _SEGMENT_REVERSED)
    if len(L) != 3:
        raise AssertionError("polygonize takes two or three lengths")
    if not (L[0] < L[1] + L[2] and L[1] < L[0] + L[2] and L[2] < L[0] + L[1]):
        raise TriangleError(f"Impossible to build a triangle with sides {lengths}")
    # third vertex from the law of cosines, sides 1 and 2 meeting there (the operations and their order are the reference's:
    # the fixture compares the vertices to the last bit)
    a, b, c = np.power(L[0], 2), np.power(L[1], 2), np.power(L[2], 2)
    x = (a - b + c) / (2 * a ** 0.5)
    y = (c - x ** 2) ** 0.5
    corners = np.array([[0.0, 0.0, 0.0], [L[0], 0.0, 0.0], [x, y, 0.0]])
    sides = np.stack([corners, np.roll(corners, -1, axis=0)], axis=1)                        # side s: corner s -> corner s + 1
    return _oriented(sides, _TRIANGLE_REVERSED)


def molecule_check(old_coords, new_coords, atomnos, max_newbonds=0):
    """Drop-in for tscode.utils.molecule_check (:341-353): do two geometries have the same bonds between the same atoms, up to
    ``max_newbonds`` differences?"""
    from .graph_manipulations import molecule_check_mask
    return bool(molecule_check_mask(old_coords, np.asarray(new_coords, dtype=np.float64), np.asarray(atomnos), max_newbonds)[0])


def scramble_check(TS_structure, TS_atomnos, excluded_atoms, mols_graphs, max_newbonds=0, logfunction=None, title=None) -> bool:
    """Drop-in for tscode.utils.scramble_check (:355-387): False when more than ``max_newbonds`` bonds formed or broke with respect
    to the molecules' own graphs, bonds that touch an excluded atom not counted.  The graphs are read by duck type (.nodes, .edges).
    On failure ``logfunction`` receives the reference's line, the changed bonds in ascending order."""
    from . import graph_manipulations as gm
    assert len(TS_structure) == sum([len(graph.nodes) for graph in mols_graphs])
    atomnos = np.asarray(TS_atomnos)
    n = len(atomnos)
    classes, thr = gm.bond_tables(atomnos)
    ref = gm.pack_edges(gm._graph_edges(mols_graphs, n), n)
    # (`a in bond` of :377-379 matches atom indices only: anything else in the list excludes nothing)
    excluded = sorted({int(a) for a in excluded_atoms if 0 <= int(a) < n})
    on_device = len(excluded) <= gm.MAX_EXCLUDED
    res = gm._run(np.asarray(TS_structure, dtype=np.float64), classes, thr, None, ref, excluded if on_device and excluded else None,
                  max_newbonds, False, True)
    ok = bool(res["mask"][0])
    if not on_device or (not ok and logfunction is not None):
        # the changed bonds themselves: from the adjacency the same call returned (and the verdict too where the list of excluded
        # atoms is longer than the kernel's 16 slots)
        delta = {(int(a), int(b)) for a, b in gm.edges_from_bits(res["adj"][0] ^ ref)}
        delta = sorted(bond for bond in delta if bond[0] not in excluded and bond[1] not in excluded)
        ok = len(delta) <= max_newbonds
        if not ok and logfunction is not None:
            logfunction(f"{title}, scramble_check - found {len(delta)} extra bonds: {{{', '.join(str(bond) for bond in delta)}}}")
    return ok


def get_double_bonds_indices(coords, atomnos):
    """Drop-in for tscode.utils.get_double_bonds_indices (:293-314): the (i, j) pairs of heavy atoms closer than the double-bond
    threshold of their elements (C-C 1.4 A, C-N 1.3 A), as a list of 2-tuples of ints."""
    from .graph_manipulations import double_bonds_batch
    return [(int(a), int(b)) for a, b in double_bonds_batch(np.asarray(coords, dtype=np.float64), np.asarray(atomnos))[0]]
