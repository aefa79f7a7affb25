"""tscode/nci.py on the MI355X engine: the non-covalent-interaction finder for a whole ensemble per call -- one wavefront per
structure (csrc/nci.hpp, k_nci) -- and the drop-in with the reference's signature.

get_nci (tscode/nci.py:28-52) reports, for one structure: atomic pairs H-O, H-N, F-F between a molecule and every LATER one, neither
atom constrained (:54-89); the aromatic rings among every 6-combination of a molecule's C / N atoms (:141-181 with is_phenyl,
tscode/graph_manipulations.py:152-174); hydrogens near a ring centre and pairs of ring centres of different molecules (:91-139).
The result equals the reference's, quirks included: in the ring-atom loop the generator expression at :103 shadows ``i``, so the
atom's owner is always 0 and the test is "the ring's molecule is not molecule 0" -- a ring's own hydrogens are reported, rings of
molecule 0 never, constrained atoms are not excluded.  ``owner_rule="intermolecular"`` of nci_batch applies what the comment at
:105-106 intends instead.

Every input is checked and refused with ValueError BEFORE the library is loaded; nothing handed in is modified.
"""

from __future__ import annotations

import sys

import numpy as np

from .engine import get_engine

__all__ = ["NCI_DICT", "MAX_ATOMS", "MAX_MOLECULES", "MAX_CANDIDATES", "MAX_CONSTRAINED", "MAX_RINGS", "WANT_ALL", "nci_tables",
           "check_nci_args", "nci_batch", "get_nci", "differential_nci", "interactions_of"]

MAX_ATOMS = 512          # csrc/nci.hpp: NC_MAX_ATOMS
MAX_MOLECULES = 8        # NC_MAX_MOLS
MAX_CANDIDATES = 64      # NC_MAX_CAND: C / N atoms per molecule
MAX_CONSTRAINED = 16     # NC_MAX_CON
MAX_RINGS = 64           # NC_MAX_RINGS: ring slots per structure

# tscode/parameters.py:56-78 (nci_dict): tag -> (maximum distance / A, the type string); the halogen entries commented out there
# are not carried
NCI_DICT = {
    "HO": (2.2, "O-H hydrogen bond"),                               # :61
    "HN": (2.2, "N-H hydrogen bond"),                               # :62
    "HPh": (2.8, "H-Ar non-conventional hydrogen bond"),            # :65
    "PhPh": (3.8, "pi-stacking interaction"),                       # :66
    "FF": (3.5, "F-F interaction"),                                 # :69
}

_CLASS_OF = {1: 1, 7: 2, 8: 3, 9: 4}                                # H, N, O, F; every other element is class 0
_SYMBOL_OF_CLASS = ("", "H", "N", "O", "F")
_CANDIDATES = (6, 7)                                                # tscode/nci.py:156: s in ('C', 'N')
WANT_ALL = ("pair_bits", "ring_atoms", "ring_owner", "ring_center", "ring_atom_bits", "ring_ring_bits")
_OWNER_RULES = {"reference": 0, "intermolecular": 1}


def nci_tables(atomnos):
    """(classes u8[n], thr f64[5, 5], ring_thr f64[5], candidate u8[n]) of NCI_DICT: class 0 = any other element, 1 H, 2 N, 3 O, 4 F."""
    z = np.asarray(atomnos)
    if z.ndim != 1 or z.dtype == bool or not np.issubdtype(z.dtype, np.integer):
        raise ValueError("atomnos must be a one-dimensional array of integers")
    classes = np.array([_CLASS_OF.get(int(v), 0) for v in z], dtype=np.uint8)
    thr, ring_thr = np.zeros((5, 5)), np.zeros(5)
    for p in range(1, 5):
        for q in range(1, 5):
            tag = "".join(sorted([_SYMBOL_OF_CLASS[p], _SYMBOL_OF_CLASS[q]]))         # nci.py:74
            thr[p, q] = NCI_DICT.get(tag, (0.0, ""))[0]
        ring_thr[p] = NCI_DICT.get("".join(sorted(["Ph", _SYMBOL_OF_CLASS[p]])), (0.0, ""))[0]   # nci.py:108
    return classes, thr, ring_thr, np.isin(z, _CANDIDATES).astype(np.uint8)


def _pair_type(z1, z2):
    tag = "".join(sorted([_SYMBOL_OF_CLASS[_CLASS_OF.get(int(z1), 0)], _SYMBOL_OF_CLASS[_CLASS_OF.get(int(z2), 0)]]))
    return NCI_DICT[tag][1]


def check_nci_args(structures, atomnos, constrained_indices, ids, owner_rule="reference", want=WANT_ALL):
    """The arguments of nci_batch, converted and checked against the limits of include/tscode_hip.h; ValueError on the first
    violation.  Returns (coords f64[N, n, 3], atomnos i64[n], ids i64[m], atom_mol u8[n], constrained i32[E] | i32[N, E] | None,
    owner rule 0 / 1, want tuple)."""
    z = np.asarray(atomnos)
    if z.ndim != 1 or z.dtype == bool or not np.issubdtype(z.dtype, np.integer):
        raise ValueError("atomnos must be a one-dimensional array of integers")
    z = z.astype(np.int64)
    n = len(z)
    x = np.ascontiguousarray(structures, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"structures of shape {x.shape}: expected (n_structures, n_atoms, 3)")
    if x.shape[1] != n:
        raise ValueError(f"{x.shape[1]} atoms per structure, {n} atomic numbers")
    if not 1 <= n <= MAX_ATOMS:
        raise ValueError(f"{n} atoms per structure: the engine takes 1 .. {MAX_ATOMS}")
    if not np.isfinite(x).all():
        raise ValueError("structures contain NaN or infinity")
    m = np.asarray(ids)
    if m.ndim != 1 or m.dtype == bool or not np.issubdtype(m.dtype, np.integer):
        raise ValueError("ids must be a one-dimensional array of integers (atoms per molecule)")
    m = m.astype(np.int64)
    if not 1 <= len(m) <= MAX_MOLECULES:
        raise ValueError(f"{len(m)} molecules: the engine takes 1 .. {MAX_MOLECULES}")
    if (m < 1).any() or int(m.sum()) != n:
        raise ValueError(f"ids {m.tolist()} do not split {n} atoms into non-empty molecules")
    atom_mol = np.repeat(np.arange(len(m)), m).astype(np.uint8)
    cand = np.isin(z, _CANDIDATES)
    per_mol = np.bincount(atom_mol[cand], minlength=len(m))
    if per_mol.max() > MAX_CANDIDATES:
        raise ValueError(f"molecule {int(per_mol.argmax())} has {int(per_mol.max())} C / N atoms: the engine takes at most {MAX_CANDIDATES}")
    con = None
    if constrained_indices is not None:
        con = np.asarray(constrained_indices)
        if con.size and (con.dtype == bool or not np.issubdtype(con.dtype, np.integer)):
            raise ValueError("constrained indices must be integers")
        if con.ndim == 0:
            raise ValueError("constrained indices: expected shape (E,) shared, or (n_structures, ...) per structure")
        if con.ndim >= 2:
            if con.shape[0] != len(x):
                raise ValueError(f"constrained indices for {con.shape[0]} structures, {len(x)} structures")
            con = con.reshape(len(x), -1)
        if con.shape[-1] > MAX_CONSTRAINED:
            raise ValueError(f"{con.shape[-1]} constrained atoms per structure: the engine takes at most {MAX_CONSTRAINED}")
        if con.size and (con.min() < -1 or con.max() >= n):
            raise ValueError(f"constrained atom index outside -1 .. {n - 1}")
        con = None if con.shape[-1] == 0 else np.ascontiguousarray(con, dtype=np.int32)
    if owner_rule not in _OWNER_RULES:
        raise ValueError(f"owner_rule {owner_rule!r}: one of {sorted(_OWNER_RULES)}")
    want = tuple(want)
    if any(w not in WANT_ALL for w in want):
        raise ValueError(f"want {want}: names from {WANT_ALL}")
    return x, z, m, atom_mol, con, _OWNER_RULES[owner_rule], want


def nci_batch(structures, atomnos, constrained_indices, ids, owner_rule="reference", want=WANT_ALL):
    """get_nci for a whole ensemble that shares ``atomnos`` and ``ids``.

    structures            f64[N, n, 3]
    constrained_indices   None, int[E] shared by all structures, or int[N, ...] per structure (flattened per structure; -1 = unused
                          slot); at most 16 per structure
    ids                   atoms per molecule, as the reference's
    owner_rule            "reference": a ring meets every atom unless the ring belongs to molecule 0 (tscode/nci.py:100-105 as
                          written); "intermolecular": a ring meets the atoms of the other molecules (the comment at :105-106)
    want                  which of WANT_ALL to return; () is the counts-only form (16 bytes per structure)

    Returns a dict: "counts" i32[N, 4] (pairs, rings, ring-atom, ring-ring), "overflow" bool[N] (more than 64 rings: the ring
    count is exact, the lists hold the first 64 in order), the wanted arrays as include/tscode_hip.h lays them out, and "atomnos",
    "ids", "owner_rule" for the functions that read the result."""
    x, z, m, atom_mol, con, rule, want = check_nci_args(structures, atomnos, constrained_indices, ids, owner_rule, want)
    classes, thr, ring_thr, cand = nci_tables(z)
    out = get_engine().nci(x, classes, thr, atom_mol, len(m), cand, ring_thr, NCI_DICT["PhPh"][0], con, rule, want)
    out.update(atomnos=z, ids=m, owner_rule=owner_rule)
    return out


def _bits_to_dense(words):
    """u64[..., W] -> bool[..., 64 W]."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    if sys.byteorder == "little":
        return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little").astype(bool)
    return ((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(w.shape[:-1] + (-1,)).astype(bool)   # pragma: no cover


def interactions_of(result, s):
    """The reference's ``nci`` list of structure ``s`` from the bit arrays of an nci_batch result (which must hold pair_bits,
    ring_atom_bits and ring_ring_bits): tuples (type, i1, i2), (type, i, 'ring'), (type, 'ring', 'ring') in the reference's order,
    duplicates kept."""
    z = result["atomnos"]
    out = []
    for i1, i2 in zip(*np.nonzero(_bits_to_dense(result["pair_bits"][s]))):
        out.append((_pair_type(z[i1], z[i2]), int(i1), int(i2)))
    n_rings = min(int(result["counts"][s, 1]), MAX_RINGS)
    for _, i in zip(*np.nonzero(_bits_to_dense(result["ring_atom_bits"][s, :n_rings]))):
        out.append((NCI_DICT["HPh"][1], int(i), "ring"))
    out += [(NCI_DICT["PhPh"][1], "ring", "ring")] * int(_bits_to_dense(result["ring_ring_bits"][s, :n_rings, None]).sum())
    return out


def get_nci(coords, atomnos, constrained_indices, ids):
    """Drop-in for tscode.nci.get_nci (:28-52): (nci, print_list), the reference's tuples and strings.  The distance in each
    string is recomputed on the host for the hits only.  Raises ValueError if the structure has more than 64 rings."""
    coords = np.asarray(coords, dtype=np.float64)
    con = None if constrained_indices is None else np.asarray(constrained_indices).ravel()
    res = nci_batch(coords[None] if coords.ndim == 2 else coords, atomnos, con, ids)
    if res["overflow"][0]:
        raise ValueError(f"{int(res['counts'][0, 1])} aromatic rings in one structure: the engine lists at most {MAX_RINGS}")
    x, z = coords.reshape(-1, 3), res["atomnos"]

    def norm_of(v):                                                 # tscode/algebra.py:90-96
        return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])

    nci, print_list = [], []
    for i1, i2 in zip(*np.nonzero(_bits_to_dense(res["pair_bits"][0]))):
        i1, i2 = int(i1), int(i2)
        kind = _pair_type(z[i1], z[i2])
        print_list.append(kind + f" ({round(norm_of(x[i1] - x[i2]), 2)} A, indices {i1}/{i2})")
        nci.append((kind, i1, i2))
    n_rings = int(res["counts"][0, 1])
    centers = [np.mean(x[res["ring_atoms"][0, r].astype(np.int64)], axis=0) for r in range(n_rings)]        # nci.py:174
    for r, i in zip(*np.nonzero(_bits_to_dense(res["ring_atom_bits"][0, :n_rings]))):
        kind = NCI_DICT["HPh"][1]
        print_list.append(kind + f" ({round(norm_of(centers[r] - x[i]), 2)} A, atom {int(i)}/ring)")
        nci.append((kind, int(i), "ring"))
    for r, s in zip(*np.nonzero(_bits_to_dense(res["ring_ring_bits"][0, :n_rings, None]))):
        kind = NCI_DICT["PhPh"][1]
        print_list.append(kind + f" ({round(norm_of(centers[r] - centers[s]), 2)} A, ring/ring)")
        nci.append((kind, "ring", "ring"))
    return nci, print_list


def differential_nci(result):
    """The second half of print_nci (tscode/embedder.py:2076-2096) on an nci_batch result: the interactions that are not shared
    by all structures, in the order of their first appearance, each with the (0-based) structures that have it --
    [(nci tuple, [structure, ...]), ...].  Interaction identities are the reference's: (type, i1, i2), (type, atom, 'ring'),
    (type, 'ring', 'ring').  Works from the bit arrays on the host."""
    for name in ("pair_bits", "ring_atom_bits", "ring_ring_bits"):
        if name not in result:
            raise ValueError(f"differential_nci needs {name}: ask nci_batch for it (want=...)")
    n = len(result["counts"])
    lists = [interactions_of(result, s) for s in range(n)]
    sets = [set(lst) for lst in lists]
    seen, out = set(), []
    for lst in lists:
        for nci in lst:
            if nci in seen:
                continue
            seen.add(nci)
            shared_by = [j for j, have in enumerate(sets) if nci in have]
            if len(shared_by) != n:
                out.append((nci, shared_by))
    return out
