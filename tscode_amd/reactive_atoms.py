"""tscode/reactive_atoms_classes.py, Hypermolecule.compute_orbitals and Embedder._set_pivots on the MI355X engine: the orbital lobes of
every reactive atom and the pivots of every conformer of a molecule in ONE library call (csrc/orbitals.hpp, k_orbitals: one lane per
conformer) -- what ``string_embed_batch`` and ``cyclical_embed_batch`` take as input, from coordinates.

The reference works one conformer and one reactive atom at a time (tscode/hypermolecule_class.py:212-214, tscode/embedder.py:587-621).
Everything it reads from the bond graph it reads from the graph of conformer 0 (``mol.graph``, hypermolecule_class.py:185), so the work
splits: ``orbital_recipes`` walks that graph once on the host and writes a small recipe per reactive atom (include/tscode_hip.h:
tsc_orbital_recipe); the device evaluates the recipes for every conformer.  The reference's behaviour is kept, quirks included:

* an 'sp' carbon whose two neighbours are carbons is ALWAYS treated as an allene (reactive_atoms_classes.py:458 tests a generator
  expression, which is true);
* an 'sp' atom that is neither allene nor ketene draws ``np.random.rand(3)`` (:495): here that vector is the argument ``sp_seed``;
* ``str()`` of a Ketone is 'Ketone (<subtype>)' and never in is_sigmatropic's ``sp2_types`` (tscode/graph_manipulations.py:246-258): a
  molecule with a reactive Ketone is never sigmatropic and the Ketone 'p' lobes (:350-353) are reached through ``sigmatropic=True`` only;
* Sp3 without sigma-star keeps ``orb_vecs`` unnormalised (:172); Single without a parameter takes the conformer's bond length (:77);
* Metal reads ``neighbors(graph, first_neighbour)[0]`` (:561), which is the metal itself where it has the lowest index there (NaN).

Every argument is checked and refused with ValueError BEFORE the library is loaded; nothing handed in is modified.  (With ``bonds=None``
the bond graph comes from this package's ``graphize``, which runs on the device: after the checks.)
"""

from __future__ import annotations

import numpy as np

from .engine import get_engine

__all__ = ["ORB_DIM_DICT", "RECIPE_DTYPE", "CLASS_IDS", "KIND_NAMES", "MAX_REACTIVE", "MAX_LOBES", "MAX_PIVOTS", "atom_type", "neighbor_lists",
           "is_vicinal", "NeighborLists", "sigmatropic_path", "orbital_recipes", "check_orbital_args", "orbitals_batch", "reactive_molecule", "ReactiveMolecule"]

MAX_REACTIVE = 8         # include/tscode_hip.h: TSC_ORB_MAX_REACTIVE
MAX_LOBES = 4            # TSC_ORB_MAX_LOBES
MAX_PIVOTS = 16          # TSC_ORB_MAX_PIVOTS
MAX_ATOMS = 65536        # TSC_ORB_MAX_ATOMS

# tscode/parameters.py:19-53 (orb_dim_dict): half of the transition-state bonding distance of an atom, by symbol and class name
ORB_DIM_DICT = {
    "H Single Bond": 0.85,      # :20
    "C Single Bond": 1,         # :21
    "O Single Bond": 1,         # :22
    "N Single Bond": 1,         # :23
    "F Single Bond": 1,         # :24
    "Cl Single Bond": 1.5,      # :25
    "Br Single Bond": 1.5,      # :26
    "I Single Bond": 2,         # :27
    "C sp": 1,                  # :29
    "N sp": 1,                  # :30
    "B sp2": 0.8,               # :32
    "C sp2": 1.1,               # :33
    "N sp2": 1,                 # :34
    "B sp3": 1,                 # :36
    "C sp3": 1,                 # :37
    "Br sp3": 1,                # :38
    "O Ether": 1,               # :40
    "S Ether": 1,               # :41
    "O Ketone": 0.85,           # :43
    "S Ketone": 1,              # :44
    "N Imine": 1,               # :46
    "C bent carbene": 1,        # :48
    "Metal": 2.5,               # :50
    "Fallback": 1,              # :52
}

# include/tscode_hip.h: tsc_orbital_recipe (88 bytes, no padding)
RECIPE_DTYPE = np.dtype([("cls", "<i4"), ("flags", "<i4"), ("atom", "<i4"), ("nb", "<i4", (4,)), ("ex", "<i4", (4,)), ("reserved", "<i4"),
                         ("orb_dim", "<f8"), ("orb_dim_bent", "<f8"), ("seed", "<f8", (3,))])
CLASS_IDS = {"Single": 0, "Sp2": 1, "Sp3": 2, "Ether": 3, "Ketone": 4, "Imine": 5, "Sp_or_carbene": 6, "Metal": 7}     # TSC_ORB_*
F_SIGMASTAR, F_BOND_LENGTH, F_ALLENE, F_KETENE, F_KETONE_KETENE, F_KETONE_TWO, F_KETONE_TRILOBE = 1, 2, 4, 8, 16, 32, 48  # TSC_ORB_F_*
# TSC_ORB_KIND_*: what str(r_atom) gives for a conformer
KIND_NAMES = ("Single Bond", "sp2", "sp3", "Ether", "Ketone (p+p)", "Ketone (sp2)", "Ketone (p)", "Ketone (trilobe)", "Imine", "sp",
              "bent carbene", "Metal")
# str() of a class before its orbitals are set (conformer-independent: what is_vicinal and is_sigmatropic compare, and the orb_dim key)
_REPR = {"Single": "Single Bond", "Sp2": "sp2", "Sp3": "sp3", "Ether": "Ether", "Ketone": "Ketone", "Imine": "Imine", "Metal": "Metal"}

_SYMBOLS = {1: "H", 3: "Li", 5: "B", 6: "C", 7: "N", 8: "O", 9: "F", 11: "Na", 12: "Mg", 15: "P", 16: "S", 17: "Cl", 19: "K", 20: "Ca", 22: "Ti",
            30: "Zn", 35: "Br", 37: "Rb", 38: "Sr", 53: "I", 55: "Cs", 56: "Ba"}
_METALS = ("Li", "Na", "Mg", "K", "Ca", "Ti", "Rb", "Sr", "Cs", "Ba", "Zn")                     # reactive_atoms_classes.py:626-638
# reactive_atoms_classes.py:579-624: symbol + number of bonds -> class
_ATOM_TYPE = {"H1": "Single", "B3": "Sp2", "B4": "Sp3", "C1": "Single", "C2": "Sp_or_carbene", "C3": "Sp2", "C4": "Sp3", "N1": "Single",
              "N2": "Imine", "N3": "Sp2", "N4": "Sp3", "O1": "Ketone", "O2": "Ether", "P2": "Imine", "P3": "Sp2", "P4": "Sp3", "S1": "Ketone",
              "S2": "Ether", "S3": "Sp2", "F1": "Single", "Cl1": "Single", "Br1": "Single", "I1": "Single"}
_ATOM_TYPE.update({m + str(b): "Metal" for m in _METALS for b in range(1, 9)})                    # :640-643
_ATOM_TYPE.update({name: name for name in CLASS_IDS})                                             # the name associations, :615-622


def _symbol(z):
    return _SYMBOLS.get(int(z), f"Z{int(z)}")


def _atomnos(atomnos):
    z = np.asarray(atomnos)
    if z.ndim != 1 or z.dtype == bool or not np.issubdtype(z.dtype, np.integer):
        raise ValueError("atomnos must be a one-dimensional array of integers")
    return z.astype(np.int64)


class NeighborLists(list):
    """What ``neighbor_lists`` returns: the marker by which the functions below tell ready-made neighbour lists from an edge list that
    happens to be a list of lists (a molecule with one ring has exactly as many bonds as atoms)."""


def neighbor_lists(bonds, n_atoms):
    """The neighbours of every atom in ascending index without the atom itself -- what ``neighbors()`` returns on a graph built by graphize
    (tscode/graph_manipulations.py:33-62) -- from packed bits u64[n, W] (graph_manipulations.pack_edges), an edge list int[E, 2] (either
    order, self loops and repeats allowed) or a networkx graph on nodes 0 .. n-1 (extra edges allowed, as the reference's constraints add)."""
    if hasattr(bonds, "edges") and hasattr(bonds, "nodes"):
        if len(bonds.nodes) != n_atoms:
            raise ValueError(f"the graph has {len(bonds.nodes)} nodes, the molecule {n_atoms} atoms")
        edges = np.array([(int(a), int(b)) for a, b in bonds.edges], dtype=np.int64).reshape(-1, 2)
    else:
        arr = np.asarray(bonds)
        if arr.dtype == np.uint64:
            from .graph_manipulations import edges_from_bits
            if arr.ndim != 2 or arr.shape != (n_atoms, (n_atoms + 63) // 64):
                raise ValueError(f"packed bonds of shape {arr.shape}: expected ({n_atoms}, {(n_atoms + 63) // 64})")
            edges = edges_from_bits(arr).astype(np.int64)
        else:
            if arr.size and (arr.dtype == bool or not np.issubdtype(arr.dtype, np.integer)):
                raise ValueError("bonds must be integers: an edge list int[E, 2], packed bits u64[n, W] or a graph")
            if arr.size and (arr.ndim != 2 or arr.shape[1] != 2):
                raise ValueError(f"an edge list of shape {arr.shape}: expected (E, 2)")
            edges = arr.astype(np.int64).reshape(-1, 2)
    if edges.size and (edges.min() < 0 or edges.max() >= n_atoms):
        raise ValueError(f"bond index outside 0 .. {n_atoms - 1}")
    sets = [set() for _ in range(n_atoms)]
    for a, b in edges.tolist():
        if a != b:
            sets[a].add(b)
            sets[b].add(a)
    return NeighborLists(sorted(s) for s in sets)


def _neighbors_of(bonds_or_graph, n_atoms):
    if isinstance(bonds_or_graph, NeighborLists):                # (only what neighbor_lists made: a plain list of lists is an edge list)
        if len(bonds_or_graph) != n_atoms:
            raise ValueError(f"neighbour lists of {len(bonds_or_graph)} atoms, the molecule has {n_atoms}")
        return bonds_or_graph
    return neighbor_lists(bonds_or_graph, n_atoms)


def atom_type(bonds_or_graph, atomnos, index, override=None):
    """get_atom_type (tscode/reactive_atoms_classes.py:645-660): the NAME of the class that represents atom ``index`` -- symbol + number
    of neighbours looked up in the reference's table, or the class called ``override``.  ValueError where the reference raises KeyError."""
    if override is not None:
        if override not in _ATOM_TYPE:
            raise ValueError(f"Orbital type {override!r} not known")
        return _ATOM_TYPE[override]
    z = _atomnos(atomnos)
    if not 0 <= int(index) < len(z):
        raise ValueError(f"atom index {index} outside 0 .. {len(z) - 1}")
    nb = _neighbors_of(bonds_or_graph, len(z))[int(index)]
    code = _symbol(z[int(index)]) + str(len(nb))
    if code not in _ATOM_TYPE:
        raise ValueError(f"Orbital type {code} not known (index {index})")
    return _ATOM_TYPE[code]


def is_vicinal(neighbors, reactive_indices, classes):
    """tscode/graph_manipulations.py:275-298: two reactive atoms, both sp3 or Single Bond, bonded."""
    if len(reactive_indices) != 2:
        return False
    i1, i2 = (int(v) for v in reactive_indices)
    return all(c in ("Sp3", "Single") for c in classes) and i1 in neighbors[i2]


def sigmatropic_path(neighbors, reactive_indices, classes):
    """The conformer-independent part of is_sigmatropic (tscode/graph_manipulations.py:231-273): two reactive atoms, every class name in
    ``sp2_types`` (sp2, Imine, sp, bent carbene -- a Ketone's name carries its subtype and never is), and some simple path between the two
    whose inner atoms have at most three neighbours.  The distance test (:256) is the device's, per conformer."""
    if len(reactive_indices) != 2 or not all(c in ("Sp2", "Imine", "Sp_or_carbene") for c in classes):
        return False
    i1, i2 = (int(v) for v in reactive_indices)
    seen, stack = {i1}, [i1]
    while stack:                                                 # (a walk through allowed atoms contains a simple path through them)
        for v in neighbors[stack.pop()]:
            if v == i2:
                return True
            if v not in seen and len(neighbors[v]) <= 3:
                seen.add(v)
                stack.append(v)
    return False


def _per_atom(value, reactive, what, convert):
    """None | one value for all | a mapping atom -> value | one value per reactive atom  ->  a list per reactive atom (None: default)."""
    if value is None:
        return [None] * len(reactive)
    if isinstance(value, dict):
        unknown = [k for k in value if int(k) not in reactive]
        if unknown:
            raise ValueError(f"{what}: atoms {unknown} are not reactive atoms")
        return [convert(value[k]) if k in value else None for k in reactive]
    if isinstance(value, (str, int, float, np.integer, np.floating)):
        return [convert(value)] * len(reactive)
    value = list(value)
    if len(value) != len(reactive):
        raise ValueError(f"{what}: {len(value)} values for {len(reactive)} reactive atoms")
    return [None if v is None else convert(v) for v in value]


def _orb_dim(value):
    v = float(value)
    if not np.isfinite(v):
        raise ValueError(f"orb_dim {value} is not finite")
    return v


def _reactive_list(reactive_indices, n):
    r_arr = np.asarray(reactive_indices)
    if r_arr.ndim != 1 or r_arr.dtype == bool or not np.issubdtype(r_arr.dtype, np.integer):
        raise ValueError("reactive_indices must be a one-dimensional array of integers")
    reactive = [int(v) for v in r_arr]
    if not 1 <= len(reactive) <= MAX_REACTIVE:
        raise ValueError(f"{len(reactive)} reactive atoms: the engine takes 1 .. {MAX_REACTIVE}")
    if min(reactive) < 0 or max(reactive) >= n:
        raise ValueError(f"reactive atom index outside 0 .. {n - 1}")
    if len(set(reactive)) != len(reactive):
        raise ValueError("reactive_indices repeat an atom")
    return reactive


def orbital_recipes(atomnos, reactive_indices, bonds, overrides=None, orb_dim=None, leaving_group=None, sp_seed=None, sigmatropic=None):
    """The host half: everything compute_orbitals reads from the bond graph, once.

    bonds           packed bits, an edge list (an array or a list of pairs), a networkx graph, or the NeighborLists that
                    ``neighbor_lists`` made of one of them: the bonds of conformer 0
    overrides       class names (the reference's ``override``): None, one name for all, a mapping atom -> name, or one per reactive atom
    orb_dim         lobe distance per atom in the same forms: the DIST keyword (tscode/embedder.py:527-535: dist / 2) and what
                    ``_scale_orbs`` amounts to; None = orb_dim_dict by symbol and class name
    leaving_group   Sp3 atoms whose leaving group cannot be inferred (:141-145): the atom, in the same forms
    sp_seed         the vector that stands for np.random.rand(3) of :495; default (1, 0, 0)
    sigmatropic     None: as the reference decides; True / False: for every conformer

    Returns a dict: ``recipes`` (RECIPE_DTYPE[R]), ``classes`` (names), ``neighbors`` (of the reactive atoms), ``sp3_sigmastar``,
    ``sigmatropic_path``, ``sigmatropic_mode`` (0 never, 1 by distance, 2 always)."""
    z = _atomnos(atomnos)
    n = len(z)
    if not 1 <= n <= MAX_ATOMS:
        raise ValueError(f"{n} atoms: the engine takes 1 .. {MAX_ATOMS}")
    reactive = _reactive_list(reactive_indices, n)
    nbs = _neighbors_of(bonds, n)
    names = _per_atom(overrides, reactive, "overrides", str)
    dims = _per_atom(orb_dim, reactive, "orb_dim", _orb_dim)
    leaving = _per_atom(leaving_group, reactive, "leaving_group", int)
    seed = np.array((1.0, 0.0, 0.0) if sp_seed is None else sp_seed, dtype=np.float64)
    if seed.shape != (3,) or not np.isfinite(seed).all():
        raise ValueError("sp_seed must be three finite numbers")
    if sigmatropic not in (None, True, False):
        raise ValueError("sigmatropic must be None, True or False")
    classes = [atom_type(nbs, z, i, names[k]) for k, i in enumerate(reactive)]
    sigmastar = is_vicinal(nbs, reactive, classes)
    path = sigmatropic_path(nbs, reactive, classes)
    sym = lambda i: _symbol(z[i])
    rec = np.zeros(len(reactive), dtype=RECIPE_DTYPE)
    rec["nb"], rec["ex"] = -1, -1
    rec["seed"] = seed
    for k, (i, cls) in enumerate(zip(reactive, classes)):
        nb = nbs[i]
        flags = F_SIGMASTAR if sigmastar else 0
        ex = []
        need = {"Single": 1, "Sp2": 3, "Sp3": 0, "Ether": 2, "Ketone": 1, "Imine": 2, "Sp_or_carbene": 2, "Metal": 1}[cls]
        if len(nb) < need:
            raise ValueError(f"atom {i} has {len(nb)} neighbours: class {cls} reads {need}")
        others = lambda a, without: [v for v in nbs[a] if v != without]
        if cls in ("Single", "Sp3") and sigmastar:
            partner = next(j for j in reactive if j != i and j in nb)                                   # :49-54, :177-182
            second = others(partner, i) if cls == "Single" else others(i, partner)                      # :60-62 / :187-189
            if not second:
                raise ValueError(f"atom {i}: the sigma-star lobes need a third atom on {'its partner' if cls == 'Single' else 'it'}")
            ex = [partner, second[0]]
        elif cls == "Sp3":
            symbols = [sym(v) for v in nb]
            hetero = [s for s in symbols if s in ("O", "N", "Cl", "Br", "I")]
            heavy = [s for s in symbols if s != "H"]
            if len(hetero) == 1:                                                                        # :141-142
                pick = [s for s in symbols if s in ("O", "Cl", "Br", "I")]
                if not pick:
                    raise ValueError(f"atom {i}: its one heteroatom neighbour is a nitrogen, which the reference counts (:141) but cannot pick (:142, "
                                     "an IndexError there)")
                ex = [nb[symbols.index(pick[0])]]
            elif len(heavy) == 1:                                                                       # :144-145
                ex = [nb[symbols.index(heavy[0])]]
            elif leaving[k] is None:
                raise ValueError(f"atom {i}: the leaving group cannot be inferred from its neighbours {symbols} (the reference asks the user): "
                                 "pass leaving_group=")
            elif leaving[k] not in nb:
                raise ValueError(f"atom {leaving[k]} is not bonded to the sp3 centre {i}")
            else:
                ex = [leaving[k]]
        elif cls == "Ketone":
            non = others(nb[0], i)                                                                      # :317-318
            if len(non) == 1:
                sub = others(non[0], nb[0])                                                             # :325-326
                if not sub:
                    raise ValueError(f"atom {i}: the ketene's far carbon {non[0]} has no substituent")
                flags |= F_KETONE_KETENE
                ex = [non[0], sub[0]]
            elif len(non) == 2:
                flags |= F_KETONE_TWO
                ex = non
            elif len(non) == 3:
                flags |= F_KETONE_TRILOBE
                ex = non
            else:
                raise ValueError(f"atom {i}: its neighbour {nb[0]} has {len(non)} other neighbours; the reference sets lobes for 1, 2 or 3")
        elif cls == "Sp_or_carbene":
            symbols = [sym(v) for v in nb[:2]]
            sides = (others(nb[0], i), others(nb[1], i))                                                # :452-456
            if all(s == "C" for s in symbols):
                if not sides[0]:
                    raise ValueError(f"atom {i}: its neighbour {nb[0]} has no other neighbour to orient the allene lobes by")
                flags |= F_ALLENE                                                                       # (:458 is always true)
                ex = [sides[0][0], nb[0]]                                                               # :507-508
            elif sorted(symbols) in (["C", "O"], ["C", "S"]):
                if len(sides[0]) == 2:                                                                  # :471-479
                    flags |= F_KETENE
                    ex = [sides[0][0], nb[0]]
                elif len(sides[1]) == 2:
                    flags |= F_KETENE
                    ex = [sides[1][0], nb[1]]
        elif cls == "Metal":
            ex = [nbs[nb[0]][0]]                                                                        # :561
        if cls == "Sp_or_carbene":
            d_sp = ORB_DIM_DICT.get(sym(i) + " sp", ORB_DIM_DICT["Fallback"])
            d_bent = ORB_DIM_DICT.get(sym(i) + " bent carbene", ORB_DIM_DICT["Fallback"])
        elif cls == "Metal":
            d_sp = d_bent = ORB_DIM_DICT["Metal"]                                                       # :574
        else:
            d_sp = d_bent = ORB_DIM_DICT.get(sym(i) + " " + _REPR[cls])
            if d_sp is None:
                if cls == "Single":
                    flags |= F_BOND_LENGTH                                                              # :77
                    d_sp = d_bent = 0.0
                else:
                    d_sp = d_bent = ORB_DIM_DICT["Fallback"]
        if dims[k] is not None:
            d_sp = d_bent = dims[k]
            flags &= ~F_BOND_LENGTH
        rec[k]["cls"], rec[k]["flags"], rec[k]["atom"] = CLASS_IDS[cls], flags, i
        rec[k]["nb"][:need] = nb[:need]
        rec[k]["ex"][:len(ex)] = ex
        rec[k]["orb_dim"], rec[k]["orb_dim_bent"] = d_sp, d_bent
    mode = (1 if path else 0) if sigmatropic is None else (2 if sigmatropic else 0)
    return {"recipes": rec, "classes": classes, "neighbors": [list(nbs[i]) for i in reactive], "sp3_sigmastar": bool(sigmastar),
            "sigmatropic_path": bool(path), "sigmatropic_mode": mode}


def check_orbital_args(coords, atomnos):
    """coords f64[C, n, 3] (one conformer: [n, 3]), finite, with as many atoms as ``atomnos``; ValueError otherwise."""
    z = _atomnos(atomnos)
    x = np.ascontiguousarray(coords, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"coords of shape {x.shape}: expected (n_conformers, n_atoms, 3)")
    if x.shape[1] != len(z):
        raise ValueError(f"{x.shape[1]} atoms per conformer, {len(z)} atomic numbers")
    if not np.isfinite(x).all():
        raise ValueError("coords contain NaN or infinity")
    return x, z


def orbitals_batch(coords, atomnos, reactive_indices, bonds=None, overrides=None, orb_dim=None, leaving_group=None, sp_seed=None,
                   suprafacial=False, sigmatropic=None):
    """compute_orbitals and _set_pivots of a whole conformer ensemble in one library call.

    coords f64[C, n, 3] are used as given (the reference has subtracted the ensemble's centroid; a caller who wants that does it).
    ``bonds=None`` takes this package's graphize of conformer 0.  The other arguments are those of ``orbital_recipes``.

    Returns a dict: ``centers`` / ``orb_vecs`` f64[C, R, 4, 3] (unused lobes zero), ``n_lobes`` u8[C, R], ``kind`` u8[C, R] with
    ``names`` (per conformer, per atom: KIND_NAMES[kind]), ``sigmatropic`` bool[C], ``sp3_sigmastar``, the recipes (``recipes``,
    ``classes``, ``neighbors``, ``sigmatropic_mode``) and, for one or two reactive atoms, ``pivot`` / ``meanpoint`` f64[C, 16, 3],
    ``lobe_index`` i8[C, 16, 2], ``n_pivots`` u8[C]: the pivots in the reference's order after its two filters."""
    x, z = check_orbital_args(coords, atomnos)
    if not 1 <= len(z) <= MAX_ATOMS:
        raise ValueError(f"{len(z)} atoms: the engine takes 1 .. {MAX_ATOMS}")
    if bonds is None:
        _reactive_list(reactive_indices, len(z))                 # (refused before the device is asked for the graph)
        from .graph_manipulations import graphize
        bonds = graphize(x[0], z)
    host = orbital_recipes(z, reactive_indices, bonds, overrides, orb_dim, leaving_group, sp_seed, sigmatropic)
    out = get_engine().orbitals(x, host["recipes"], host["sigmatropic_mode"], suprafacial, want_pivots=len(host["recipes"]) <= 2)
    out["names"] = [[KIND_NAMES[k] for k in row] for row in out["kind"]]
    out.update(host)
    out["suprafacial"] = bool(suprafacial)
    out["coords"] = x                                            # (the converted array the call ran on)
    return out


class ReactiveMolecule:
    """What ``cyclical_embed_batch`` reads from a molecule (``coords``, ``reactive_indices``, ``pivots``, ``reactive_cumnums``), views
    into the arrays of one orbitals_batch call (``orbitals``), and ``string_inputs()`` for ``string_embed_batch``."""

    def __init__(self, coords, reactive_indices, orbitals, cumnum_offset):
        self.coords = coords
        self.reactive_indices = np.asarray(reactive_indices, dtype=np.int64)
        self.orbitals = orbitals
        cum = self.reactive_indices + int(cumnum_offset)                                                # tscode/embedder.py:363-367
        self.reactive_cumnums = np.stack([self.reactive_indices, cum], axis=1)
        ends = np.array([cum[0], cum[-1]], dtype=np.int64)                                              # (start_atom, end_atom).cumnum
        n_piv = orbitals["n_pivots"]
        self.pivots = [(orbitals["pivot"][c, :p], orbitals["meanpoint"][c, :p], np.broadcast_to(ends, (int(p), 2)))
                       for c, p in enumerate(n_piv.tolist())]

    def __getitem__(self, key):
        return getattr(self, key)

    def string_inputs(self):
        """(centers, orb_vecs) f64[C, L, 3] of the FIRST reactive atom -- ``mol.get_r_atoms(c)[0].center`` / ``.orb_vecs``.  ValueError
        where the lobe count differs between conformers (string_embed counts the centres on conformer 0)."""
        n = self.orbitals["n_lobes"][:, 0]
        if len(n) and (n != n[0]).any():
            raise ValueError(f"the first reactive atom has {sorted(set(n.tolist()))} lobes in different conformers: string_embed_batch takes one count")
        lobes = int(n[0]) if len(n) else 0
        return self.orbitals["centers"][:, 0, :lobes], self.orbitals["orb_vecs"][:, 0, :lobes]


def reactive_molecule(coords, atomnos, reactive_indices, bonds=None, overrides=None, orb_dim=None, leaving_group=None, sp_seed=None,
                      suprafacial=False, sigmatropic=None, cumnum_offset=0):
    """A molecule for the embed drivers from coordinates: orbitals_batch, then a ReactiveMolecule (one or two reactive atoms).
    ``cumnum_offset`` = the number of atoms of the molecules in front of this one in the embedded structure."""
    r = np.asarray(reactive_indices)
    if r.ndim == 1 and len(r) > 2:
        raise ValueError(f"{len(r)} reactive atoms: the embed drivers take molecules with one or two")
    if int(cumnum_offset) != cumnum_offset or cumnum_offset < 0:
        raise ValueError("cumnum_offset must be a non-negative integer")
    out = orbitals_batch(coords, atomnos, reactive_indices, bonds, overrides, orb_dim, leaving_group, sp_seed, suprafacial, sigmatropic)
    return ReactiveMolecule(out["coords"], r, out, cumnum_offset)
