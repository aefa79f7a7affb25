"""Deterministic synthetic conformer ensembles.

Every benchmark and every large parity test draws its input from here, so
that the GPU path, the CPU oracle and the committed golden vectors all see
the same numbers for a given (config, seed).

Layout of one ensemble
----------------------
* ``n_mols`` rigid fragments (2, or 3 for the trimolecular config); atom
  positions are a self-avoiding random walk (1.5 A steps, >= 1.2 A between
  non-bonded atoms), centred at the origin;
* ``atomnos``: 3 heavy atoms (Z=6) then 2 hydrogens, repeating -> 60 % heavy;
* fragment 0 is fixed (R = I, t = 0); the other fragments take ``N / c``
  "parent" transforms (R uniform on SO(3), t in a 4-9 A shell) and ``c``
  slightly perturbed children per parent, shuffled over the whole array.

Nothing in here touches the GPU or the reference.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

__all__ = ["Ensemble", "make_fragment", "make_ensemble", "make_unscreenable", "CONFIGS", "make_config", "quat_to_mat", "make_rot_corr_ensemble",
           "RotorMolecule", "make_rotor_molecule", "make_chain_ensemble",
           "CHAIN_ELEMENTS", "CHAIN_SIGMAS", "aromatic_block", "make_aromatic_ensemble", "AROMATIC_SIGMAS"]


def make_fragment(rng: np.random.Generator, n_atoms: int, step: float = 1.5, min_dist: float = 1.2) -> np.ndarray:
    """Self-avoiding random walk, centred at the origin. Returns f64[n_atoms, 3]."""
    pts = np.zeros((n_atoms, 3))
    i = 1
    tries = 0
    while i < n_atoms:
        v = rng.normal(size=3)
        v *= step / np.sqrt(v @ v)
        # grow from a random earlier atom now and then, so fragments are branched, not chains
        base = i - 1 if rng.random() < 0.7 else int(rng.integers(0, i))
        cand = pts[base] + v
        d = np.sqrt(((pts[:i] - cand) ** 2).sum(axis=1))
        d[base] = np.inf
        tries += 1
        if d.min() >= min_dist:
            pts[i] = cand
            i += 1
        if tries > 100000:
            raise RuntimeError("random walk stuck")
    return pts - pts.mean(axis=0)


def quat_to_mat(q: np.ndarray) -> np.ndarray:
    """Unit quaternions (w, x, y, z) f64[..., 4] -> rotation matrices f64[..., 3, 3]."""
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    m = np.empty(q.shape[:-1] + (3, 3))
    m[..., 0, 0] = 1 - 2 * (y * y + z * z)
    m[..., 0, 1] = 2 * (x * y - w * z)
    m[..., 0, 2] = 2 * (x * z + w * y)
    m[..., 1, 0] = 2 * (x * y + w * z)
    m[..., 1, 1] = 1 - 2 * (x * x + z * z)
    m[..., 1, 2] = 2 * (y * z - w * x)
    m[..., 2, 0] = 2 * (x * z - w * y)
    m[..., 2, 1] = 2 * (y * z + w * x)
    m[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return m


def _axis_angle_to_mat(axis: np.ndarray, angle: np.ndarray) -> np.ndarray:
    axis = axis / np.sqrt((axis * axis).sum(axis=-1, keepdims=True))
    half = 0.5 * angle
    q = np.concatenate([np.cos(half)[..., None], np.sin(half)[..., None] * axis], axis=-1)
    return quat_to_mat(q)


@dataclass
class Ensemble:
    """One synthetic ensemble in the batched form of SURVEY.md section 8 row a16.

    frag_coords[m]: f64[1, n_m, 3] conformer stack of fragment m (one conformer each)
    conf_idx:       i32[N, n_mols]  conformer picked for each pose and fragment (all 0 here)
    rot:            f64[N, n_mols, 3, 3]
    pos:            f64[N, n_mols, 3]
    ids:            i64[n_mols]      atoms per fragment
    atomnos:        i64[n]           atomic numbers of the concatenated pose
    """

    frag_coords: list
    conf_idx: np.ndarray
    rot: np.ndarray
    pos: np.ndarray
    ids: np.ndarray
    atomnos: np.ndarray
    seed: int
    meta: dict = field(default_factory=dict)

    @property
    def n_poses(self) -> int:
        return int(self.rot.shape[0])

    @property
    def n_atoms(self) -> int:
        return int(self.ids.sum())

    @property
    def n_heavy(self) -> int:
        return int((self.atomnos != 1).sum())

    def poses(self, lo: int = 0, hi: int | None = None) -> np.ndarray:
        """NumPy materialisation of poses [lo, hi): the get_embed formula
        ``(R @ X.T).T + t`` per fragment, concatenated (reference embeds.py:961-969)."""
        hi = self.n_poses if hi is None else hi
        parts = []
        for m, frag in enumerate(self.frag_coords):
            x = frag[self.conf_idx[lo:hi, m]]                    # (P, n_m, 3)
            r = self.rot[lo:hi, m]                               # (P, 3, 3)
            parts.append(np.einsum("pij,paj->pai", r, x) + self.pos[lo:hi, m][:, None, :])
        return np.ascontiguousarray(np.concatenate(parts, axis=1))


def make_ensemble(n_poses: int, atoms_per_frag, seed: int, children: int = 10,
                  sigma_rot_deg: float = 1.0, sigma_t: float = 0.03,
                  shell=(4.0, 9.0), local_spread: float | None = None) -> Ensemble:
    """``local_spread`` = None: the children of all parents are shuffled over the whole array (every BASELINE config).
    A number S > 1: a LOCAL shuffle -- every family gets a home position, uniform over the array, and each child lands at
    home +- a log-uniform offset in [1, S]: a few siblings share a chunk of 20, more share a chunk of 200, the rest only meet in
    the coarse passes.  The prune's fine passes (k = 5000 ... 200, rmsd_pruning.py:186-192) then each find duplicates to remove
    while more than 20 k structures stay active, which a global shuffle never gives them (golden fixtures G16 / G17)."""
    rng = np.random.default_rng(seed)
    atoms_per_frag = [int(a) for a in atoms_per_frag]
    n_mols = len(atoms_per_frag)
    frags = [make_fragment(rng, a)[None, :, :] for a in atoms_per_frag]
    atomnos = np.concatenate([np.where(np.arange(a) % 5 < 3, 6, 1) for a in atoms_per_frag]).astype(np.int64)

    n_par = max(1, (n_poses + children - 1) // children)
    rot = np.zeros((n_poses, n_mols, 3, 3))
    pos = np.zeros((n_poses, n_mols, 3))
    rot[:, 0] = np.eye(3)
    parent_of = np.repeat(np.arange(n_par), children)[:n_poses]
    for m in range(1, n_mols):
        pr = quat_to_mat(rng.normal(size=(n_par, 4)))
        direction = rng.normal(size=(n_par, 3))
        direction /= np.sqrt((direction ** 2).sum(axis=1, keepdims=True))
        radius = rng.uniform(shell[0], shell[1], size=(n_par, 1))
        pt = direction * radius
        # children = parent o (small body-frame rotation) + small translation
        d_rot = _axis_angle_to_mat(rng.normal(size=(n_poses, 3)),
                                   np.deg2rad(sigma_rot_deg) * rng.normal(size=n_poses))
        d_t = sigma_t * rng.normal(size=(n_poses, 3))
        rot[:, m] = np.einsum("pij,pjk->pik", pr[parent_of], d_rot)
        pos[:, m] = pt[parent_of] + d_t
    if local_spread is None:
        perm = rng.permutation(n_poses)
    else:
        home = rng.uniform(0.0, n_poses, size=n_par)
        off = np.exp(rng.uniform(0.0, np.log(float(local_spread)), size=n_poses)) * rng.choice([-1.0, 1.0], size=n_poses)
        perm = np.argsort(home[parent_of] + off, kind="stable")
    rot, pos, parent_of = rot[perm], pos[perm], parent_of[perm]
    return Ensemble(
        frag_coords=frags,
        conf_idx=np.zeros((n_poses, n_mols), dtype=np.int32),
        rot=np.ascontiguousarray(rot), pos=np.ascontiguousarray(pos),
        ids=np.asarray(atoms_per_frag, dtype=np.int64), atomnos=atomnos, seed=seed,
        meta={"children": children, "sigma_rot_deg": sigma_rot_deg, "sigma_t": sigma_t,
              "shell": tuple(shell), "parent_of": parent_of, "local_spread": local_spread},
    )


def make_unscreenable(n: int, seed: int = 99, h: int = 30, children: int = 10, jitter: float = 0.004) -> np.ndarray:
    """Heavy-atom array f64[n, h, 3] on which the descriptor sieve of the prune can drop NOTHING: two rigid bodies about the
    origin, the first fixed, the second turned by one of n / children random rotations (+ a tiny jitter) ABOUT THE ORIGIN.  Every
    atom keeps its distance from the origin and every atom pair (a, a + h / 2) lies inside one body and keeps its length, so the
    rotation-invariant descriptors of all n structures coincide, while structures of different parents are far apart in RMSD.
    Every pair a pass looks at therefore reaches H = p^T q (tools/worstcase.py, bench.py's `unscreenable` leg)."""
    rng = np.random.default_rng(seed)
    half = h // 2
    na = half // 2
    ia = list(range(0, na)) + list(range(half, half + na))                   # body A: atoms a and a + h / 2 for a < na
    ib = [a for a in range(h) if a not in set(ia)]                           # body B: the other pairs (and an unpaired last atom)
    A, B = rng.normal(size=(len(ia), 3)) * 3, rng.normal(size=(len(ib), 3)) * 3
    n_par = max(1, n // children)
    rots = quat_to_mat(rng.normal(size=(n_par, 4)))
    which = rng.integers(0, n_par, size=n)
    jit = quat_to_mat(np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 3)) * jitter], axis=1))
    heavy = np.empty((n, h, 3))
    heavy[:, ia] = A
    heavy[:, ib] = np.einsum("nij,njk,ak->nai", rots[which], jit, B)
    return np.ascontiguousarray(heavy)


# BASELINE.json configs -> (N, atoms per fragment, seed); thresholds are fixed for all of them.
CONFIGS = {
    "C2": dict(n_poses=10_000, atoms_per_frag=(15, 15), seed=1002),
    "C3": dict(n_poses=100_000, atoms_per_frag=(25, 25), seed=1003),
    "C4": dict(n_poses=1_000_000, atoms_per_frag=(25, 25), seed=1004),
    # 70-atom fragments are ~6 A in radius: with the 4-9 A shell of the bimolecular configs only 1.5 % of the
    # poses pass the clash check, so the trimolecular config places its fragments in an 8-15 A shell
    "C5": dict(n_poses=500_000, atoms_per_frag=(70, 70, 60), seed=1005, shell=(8.0, 15.0)),
}
RMSD_THR = 0.5
CLASH_THRESH = 1.5
MAX_CLASHES = 0


def make_config(name: str, n_poses: int | None = None, attempt: int = 0) -> Ensemble:
    """Ensemble for a named BASELINE config. ``attempt`` re-draws with seed + 1000*attempt
    (the guard-band rule of SURVEY.md 8d); ``n_poses`` overrides N for bounded CPU samples."""
    cfg = dict(CONFIGS[name])
    if n_poses is not None:
        cfg["n_poses"] = int(n_poses)
    cfg["seed"] = cfg["seed"] + 1000 * attempt
    ens = make_ensemble(**cfg)
    ens.meta["config"] = name
    return ens


def make_rot_corr_ensemble(base, torsions, angles, move_masks, n_clusters, per_cluster, turn=None, seed=0, spread=0.8, noise=0.005):
    """A shuffled ensemble for the symmetry-corrected prune (tscode_amd.rot_corr) whose answer is known.  Cluster c is ``base``
    with every coordinate moved by N(0, spread) -- except the atoms of the turned rotors (move_masks[t] and the bond atoms t1, t2
    of every torsion with turn[t]), which keep their symmetry about their bond -- so clusters lie far apart in RMSD.  Each member
    turns every such rotor by one of its torsion's angles (an exact symmetry turn when the rotor is symmetric in ``base``: the
    atoms are permuted, the all-atom mean the prune centres on stays put, and the torsion search undoes the turn), then takes
    uniform noise of at most ``noise`` per coordinate and a random rigid rotation.
    Returns (structures f64[n_clusters * per_cluster, n, 3], labels int[...])."""
    rng = np.random.default_rng(seed)
    base = np.asarray(base, dtype=np.float64)
    turn = [True] * len(torsions) if turn is None else list(turn)
    keep = np.zeros(len(base), dtype=bool)
    for t, tor in enumerate(torsions):
        if turn[t]:
            keep |= np.asarray(move_masks[t], dtype=bool)
            keep[[int(tor[1]), int(tor[2])]] = True
    out, labels = [], []
    for c in range(n_clusters):
        xc = base + np.where(keep[:, None], 0.0, rng.normal(0.0, spread, size=base.shape))
        for _ in range(per_cluster):
            x = xc.copy()
            for t, (tor, angs, mask) in enumerate(zip(torsions, angles, move_masks)):
                if not turn[t]:
                    continue
                i2, i3 = int(tor[1]), int(tor[2])
                ax = x[i2] - x[i3]
                ax = ax / np.linalg.norm(ax)
                half = np.radians(float(angs[rng.integers(len(angs))])) / 2
                R = quat_to_mat(np.array([[np.cos(half), *(np.sin(half) * ax)]]))[0]
                m = np.asarray(mask, dtype=bool)
                x[m] = (x[m] - x[i3]) @ R.T + x[i3]
            x = x + rng.uniform(-noise, noise, size=x.shape)
            q = rng.normal(size=4)
            out.append(x @ quat_to_mat((q / np.linalg.norm(q))[None])[0].T)
            labels.append(c)
    perm = rng.permutation(len(out))
    return np.array(out)[perm], np.array(labels)[perm]


@dataclass
class RotorMolecule:
    """What make_rotor_molecule returns: the molecule and the set-up arrays of tscode_amd.prune_rmsd_rot_corr_arrays."""

    coords: np.ndarray          # f64[n, 3]
    atomnos: np.ndarray         # int[n]: 6 (tree and hubs), 9 (rotor atoms), 1
    bonds: list                 # [(a, b)], a < b: a tree
    torsions: np.ndarray        # i32[T, 4]: (a neighbour of i2, i2, i3 = the rotor's hub, one of its k atoms)
    angles: list                # T tuples of degrees, 0 first
    folds: list                 # T ints
    move_masks: np.ndarray      # bool[T, n]
    sub_nodes: list             # T sorted index lists

    def setup(self):
        return dict(torsions=self.torsions, angles=self.angles, move_masks=self.move_masks, sub_nodes=self.sub_nodes)


def _unit(v):
    return v / np.sqrt(v @ v)


def _cone(rng, p, back, length, k):
    """k positions bonded to p, 109.47 degrees from the bond p - back, at exact 360 / k steps about it (random phase)."""
    w = _unit(back - p)
    e1 = _unit(np.cross(w, [1.0, 0.0, 0.0] if abs(w[0]) < 0.9 else [0.0, 1.0, 0.0]))
    e2 = np.cross(w, e1)
    th, phi0 = np.radians(109.47), rng.uniform(0.0, 2 * np.pi)
    return [p + length * (np.cos(th) * w + np.sin(th) * (np.cos(phi0 + 2 * np.pi * s / k) * e1 + np.sin(phi0 + 2 * np.pi * s / k) * e2))
            for s in range(k)]


def _component(n, bonds, cut, start):
    """The atoms reachable from ``start`` over ``bonds`` without the bonds of ``cut``."""
    cut = {tuple(sorted(b)) for b in cut}
    nb = [[] for _ in range(n)]
    for a, b in bonds:
        if tuple(sorted((a, b))) not in cut:
            nb[a].append(b)
            nb[b].append(a)
    seen, todo = {start}, [start]
    while todo:
        for b in nb[todo.pop()]:
            if b not in seen:
                seen.add(b)
                todo.append(b)
    return seen


def make_rotor_molecule(n_atoms, groups, seed=0, heavy_share=0.6, order=None, table=None):
    """A tree-shaped molecule with symmetric heavy-atom rotors, and the set-up of the symmetry-corrected prune on it.

    The tree is a branched self-avoiding walk of carbons (1.5 A steps).  Each entry of ``groups`` hangs one rotor group on a tree
    atom and is ``k``, ``(k, kc)`` or either with the string "far" appended:
      k        a hub carbon with k identical atoms (Z = 9) at exact 360 / k steps about the hub's bond: one k-fold torsion;
      (k, kc)  the k atoms are hub carbons themselves, images of one another under the 360 / k turn, each with kc identical atoms
               about its own bond (C(CF3)3 is (3, 3)): one k-fold torsion, then k torsions of fold kc;
      "far"    the group's first torsion turns the OTHER side of its bond (the rest of the molecule), so its moved list is long.
    Hydrogens on tree atoms fill the molecule up to ``n_atoms``; ``heavy_share`` of the atoms outside the groups are tree carbons.

    Per torsion (i1, i2, i3, i4), i3 is the rotor's hub.  ``angles`` are 0, 360 / k, ... (``table`` = {torsion: angles} replaces
    single entries); ``move_masks`` hold one side of the i2 - i3 bond without i2 and i3 (the rotor's side unless "far");
    ``sub_nodes`` are the sorted heavy atoms of the component of i2 once every other torsion's bond is cut.

    ``order``: None leaves heavy atoms first and hydrogens last; "shuffle" draws a permutation from the seed, an array gives one
    (new atom q is old atom order[q]).  Returns a RotorMolecule."""
    rng = np.random.default_rng(seed)
    specs = []
    for g in groups:
        g = (g,) if isinstance(g, int) else tuple(g)
        far = g[-1] == "far"
        g = g[:-1] if far else g
        if len(g) not in (1, 2) or any(k not in (2, 3, 4, 6) for k in g):
            raise ValueError(f"rotor group {g!r}: k or (k, kc) with folds of 2, 3, 4 or 6")
        specs.append((g[0], g[1] if len(g) == 2 else 0, far))
    in_groups = sum(1 + k + k * kc for k, kc, _ in specs)
    n_tree = int(np.ceil((n_atoms - in_groups) * heavy_share))
    n_h = n_atoms - in_groups - n_tree
    if n_tree < 2 or n_h < 0:
        raise ValueError(f"{n_atoms} atoms do not hold these rotor groups and a tree")

    z, x, bonds = [6], [np.zeros(3)], []

    def add(zz, pos, to):
        z.append(zz)
        x.append(np.asarray(pos, dtype=np.float64))
        bonds.append((to, len(z) - 1))
        return len(z) - 1

    tries = 0
    while len(z) < n_tree:                                                          # the tree
        base = len(z) - 1 if rng.random() < 0.7 else int(rng.integers(0, len(z)))
        cand = x[base] + 1.5 * _unit(rng.normal(size=3))
        d = np.sqrt(((np.array(x) - cand) ** 2).sum(axis=1))
        d[base] = np.inf
        tries += 1
        if d.min() >= 1.2:
            add(6, cand, base)
        if tries > 100000:
            raise RuntimeError("random walk stuck")
    tors, folds, far_flags = [], [], []
    anchors = rng.permutation(np.arange(1, n_tree))[:len(specs)] if n_tree > len(specs) else rng.integers(1, n_tree, size=len(specs))
    for (k, kc, far), a in zip(specs, anchors.tolist()):
        back = next(p for p, q in bonds if q == a)                                  # the tree atom that a grew from
        hub = add(6, x[a] + 1.52 * _unit(x[a] - x[back] + 0.5 * rng.normal(size=3)), a)
        first = _cone(rng, x[hub], x[a], 1.54 if kc else 1.35, k)
        ring = [add(6 if kc else 9, p, hub) for p in first]
        tors.append((back, a, hub, ring[0]))
        folds.append(k)
        far_flags.append(far)
        if kc:
            # the first sub-rotor, then its images under the group's 360 / k turn about the hub's bond
            axis = _unit(x[a] - x[hub])                                             # (the sense in which _cone steps)
            leaves = np.array(_cone(rng, x[ring[0]], x[hub], 1.35, kc))
            for s, c in enumerate(ring):
                R = quat_to_mat(np.array([[np.cos(np.pi * s / k), *(np.sin(np.pi * s / k) * axis)]]))[0]
                img = (leaves - x[hub]) @ R.T + x[hub]
                ids = [add(9, p, c) for p in img]
                tors.append((a, hub, c, ids[0]))
                folds.append(kc)
                far_flags.append(False)
    for q in range(n_h):                                                            # hydrogens, round the tree
        a = q % n_tree
        add(1, x[a] + 1.09 * _unit(rng.normal(size=3)), a)
    z, x = np.array(z), np.array(x)
    n = len(z)
    assert n == n_atoms

    masks, subs = np.zeros((len(tors), n), dtype=bool), []
    for t, (i1, i2, i3, i4) in enumerate(tors):
        side = _component(n, bonds, [(i2, i3)], i2 if far_flags[t] else i3)
        masks[t, list(side)] = True
        masks[t, [i2, i3]] = False
        comp = _component(n, bonds, [(o[1], o[2]) for q, o in enumerate(tors) if q != t], i2)
        subs.append(sorted(i for i in comp if z[i] != 1))
    angles = [tuple(360.0 / k * s for s in range(k)) for k in folds]
    for t, a in (table or {}).items():
        angles[t] = tuple(float(v) for v in a)
    if order is None:
        order = np.array(sorted(range(n), key=lambda i: (z[i] == 1, i)))
    elif isinstance(order, str):
        if order != "shuffle":
            raise ValueError(f"order = {order!r}")
        order = rng.permutation(n)
    order = np.asarray(order)
    new = np.empty(n, dtype=np.int64)
    new[order] = np.arange(n)
    return RotorMolecule(coords=np.ascontiguousarray(x[order]), atomnos=z[order],
                         bonds=sorted(tuple(sorted((int(new[a]), int(new[b])))) for a, b in bonds),
                         torsions=new[np.array(tors)].astype(np.int32), angles=angles, folds=list(folds),
                         move_masks=np.ascontiguousarray(masks[:, order]), sub_nodes=[sorted(new[s].tolist()) for s in subs])


# ---- chains for the topology checks (tscode_amd.graph_manipulations; fixtures G21) ---------------------------------------------
CHAIN_ELEMENTS = (6, 6, 8, 7, 6)                 # C, C, O, N, C, repeating
CHAIN_SIGMAS = (0.02, 0.05, 0.08, 0.12)          # A: from "every bond survives" to "hardly any structure keeps its graph"


def make_chain(rng: np.random.Generator, n_atoms: int, step: float = 1.5, min_dist: float = 2.0) -> np.ndarray:
    """A self-avoiding walk: consecutive atoms ``step`` apart (bonded for every pair of CHAIN_ELEMENTS), all others at least
    ``min_dist`` (not bonded).  Returns f64[n_atoms, 3]."""
    pts = np.zeros((n_atoms, 3))
    i, tries = 1, 0
    while i < n_atoms:
        v = rng.normal(size=3)
        cand = pts[i - 1] + v * (step / np.sqrt(v @ v))
        tries += 1
        if i == 1 or np.sqrt(((pts[:i - 1] - cand) ** 2).sum(axis=1)).min() >= min_dist:
            pts[i] = cand
            i += 1
        if tries > 1000000:
            raise RuntimeError("random walk stuck")
    return pts


def make_chain_ensemble(n_structs: int, n_atoms: int, seed: int):
    """(base f64[n, 3], structures f64[N, n, 3], atomnos int[n], sigma f64[N]): the chain plus Gaussian noise whose sigma is drawn
    per structure from CHAIN_SIGMAS."""
    rng = np.random.default_rng(seed)
    base = make_chain(rng, n_atoms)
    atomnos = np.array([CHAIN_ELEMENTS[i % len(CHAIN_ELEMENTS)] for i in range(n_atoms)])
    sigma = np.array(CHAIN_SIGMAS)[rng.integers(0, len(CHAIN_SIGMAS), size=n_structs)]
    structures = base[None] + rng.normal(size=(n_structs, n_atoms, 3)) * sigma[:, None, None]
    return base, np.ascontiguousarray(structures), atomnos, sigma


# ---- aromatic building blocks for the non-covalent-interaction finder (tscode_amd.nci; fixtures G22) ----------------------------
AROMATIC_SIGMAS = (0.0, 0.03, 0.08, 0.15)        # A: from "every ring is flat" to "hardly any ring passes is_phenyl's 10 degrees"


def _hexagon(radius, z_alt=0.0, start=0.0):
    ang = start + np.arange(6) * (np.pi / 3)
    return np.stack([radius * np.cos(ang), radius * np.sin(ang), z_alt * (-1.0) ** np.arange(6)], axis=1)


def aromatic_block(name: str):
    """(atomnos int[k], coords f64[k, 3]) of a building block, its ring(s) in the xy plane about the origin, heavy atoms first:
      benzene      6 C on a hexagon of 1.39 A, 6 H at 2.48 A
      hexagon      the 6 C of benzene alone
      pyridine     N + 5 C on the same hexagon, 5 H
      pyranyl      O + 5 C on the same hexagon, 5 H: exactly 5 ring candidates, never scanned
      naphthalene  10 C (two hexagons sharing an edge), 8 H
      chair        cyclohexane: 6 C on a hexagon of 1.45 A at z = +-0.25 A (all within 3 A of one another, not flat), 12 H
      rod          6 C on the x axis, 0.5 A apart: axis-aligned collinear atoms, the dihedral's atan2(0, 0)
      H O N F C    one atom at the origin (probes)"""
    ring, outer = _hexagon(1.39), _hexagon(2.48)
    if name == "hexagon":
        return np.array([6] * 6), ring
    if name == "benzene":
        return np.array([6] * 6 + [1] * 6), np.concatenate([ring, outer])
    if name in ("pyridine", "pyranyl"):
        return np.array([7 if name == "pyridine" else 8] + [6] * 5 + [1] * 5), np.concatenate([ring, outer[1:]])
    if name == "naphthalene":
        shift = np.array([1.39 * np.sqrt(3.0) / 2, 0.0, 0.0])
        a, b = _hexagon(1.39, start=np.pi / 6) - shift, _hexagon(1.39, start=np.pi / 6) + shift
        carbons = np.concatenate([a, [p for p in b if np.sqrt(((a - p) ** 2).sum(1)).min() > 0.1]])    # (two of b's vertices are the shared edge)
        ha, hb = _hexagon(2.48, start=np.pi / 6) - shift, _hexagon(2.48, start=np.pi / 6) + shift
        hyd = [p for p in np.concatenate([ha, hb]) if np.sqrt(((carbons - p) ** 2).sum(1)).min() > 1.0]
        return np.array([6] * len(carbons) + [1] * len(hyd)), np.concatenate([carbons, hyd])
    if name == "chair":
        c = _hexagon(1.45, z_alt=0.25)
        axial = c + np.array([0.0, 0.0, 1.1]) * np.sign(c[:, 2:3])
        equatorial = c + np.concatenate([c[:, :2] / 1.45 * 1.0, -0.35 * np.sign(c[:, 2:3])], axis=1)
        return np.array([6] * 6 + [1] * 12), np.concatenate([c, axial, equatorial])
    if name == "rod":
        return np.array([6] * 6), np.stack([0.5 * np.arange(6), np.zeros(6), np.zeros(6)], axis=1)
    if name in ("H", "O", "N", "F", "C"):
        return np.array([{"H": 1, "C": 6, "N": 7, "O": 8, "F": 9}[name]]), np.zeros((1, 3))
    raise ValueError(f"no building block {name!r}")


def make_aromatic_ensemble(molecules, n_structs: int, seed: int, sigmas=AROMATIC_SIGMAS, rigid: float = 0.0):
    """An ensemble for the non-covalent-interaction finder.  ``molecules`` is a list of molecules, each a list of placed building
    blocks ``(name, position)`` or ``(name, position, quaternion)`` (aromatic_block; the block is turned by the quaternion, then
    moved to the position).  Every structure is the base with Gaussian noise on every coordinate, sigma drawn per structure from
    ``sigmas``, after each molecule but the first was moved as a whole by N(0, rigid) per axis (so contacts between molecules open
    and close from structure to structure even at sigma = 0, and axis-aligned atoms stay axis-aligned there).
    Returns (base f64[n, 3], structures f64[N, n, 3], atomnos int[n], ids int[n_mols], sigma f64[N])."""
    rng = np.random.default_rng(seed)
    zs, xs, ids = [], [], []
    for mol in molecules:
        count = 0
        for placed in mol:
            z, x = aromatic_block(placed[0])
            if len(placed) > 2 and placed[2] is not None:
                x = x @ quat_to_mat(np.asarray(placed[2], dtype=np.float64)[None])[0].T
            zs.append(z)
            xs.append(x + np.asarray(placed[1], dtype=np.float64))
            count += len(z)
        ids.append(count)
    atomnos, base, ids = np.concatenate(zs), np.concatenate(xs), np.array(ids)
    sigma = np.asarray(sigmas, dtype=np.float64)[rng.integers(0, len(sigmas), size=n_structs)]
    shift = rng.normal(size=(n_structs, len(ids), 3)) * rigid
    shift[:, 0] = 0.0
    structures = base[None] + np.repeat(shift, ids, axis=1) + rng.normal(size=(n_structs, len(base), 3)) * sigma[:, None, None]
    return base, np.ascontiguousarray(structures), atomnos, ids, sigma
