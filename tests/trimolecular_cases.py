"""Inputs and host yardsticks shared by tests/test_trimolecular_prologue.py and tests/test_trimolecular_groups.py: the molecules of fixture
G18, synthetic molecules, and the host loop ``tscode_amd.embeds._trimolecular_groups`` run with a recorder around ``_adjust_directions3`` that
also keeps the 343 costs of every group (for the guard band between the smallest and the second smallest)."""

import numpy as np

from conftest import load_golden

GAP_BAND = 1e-4            # degrees: acos near 0 / 180 degrees carries up to ~1e-6 degrees of rounding per term; three terms on two sides, x20


def g18_case(k):
    g = load_golden("G18_cyclical_embed_trimolecular")
    mols = []
    for m in range(3):
        coords = g[f"coords{m}_{k}"]
        mols.append(dict(coords=coords, reactive_indices=g[f"reactive_indices{m}_{k}"], reactive_cumnums=g[f"reactive_cumnums{m}_{k}"],
                         pivots=[(g[f"pivot_vec{m}_{c}_{k}"], g[f"pivot_mean{m}_{c}_{k}"], g[f"pivot_cumnums{m}_{c}_{k}"]) for c in range(len(coords))]))
    return g, mols


def unpack(mols):
    coords = [np.ascontiguousarray(m["coords"], dtype=np.float64) for m in mols]
    reactive = [np.atleast_1d(np.asarray(m["reactive_indices"], dtype=np.int64)) for m in mols]
    pivots = [m["pivots"] for m in mols]
    cumnums = [np.asarray(m["reactive_cumnums"], dtype=np.int64).reshape(-1, 2) for m in mols]
    return coords, reactive, pivots, cumnums


def synthetic_mols(seed, n_atoms=(5, 33, 70), n_conf=(1, 1, 1), n_pivots=(2, 2, 2), n_reactive=(2, 2, 2), lengths=(2.0, 3.5), extra_rows=()):
    """Three molecules of random coordinates.  Molecule m's atoms carry the cumnums offset[m] + index; a molecule with two reactive atoms has
    pivots between them (either way round), one with a single reactive atom has pivots from that atom to itself (two orbitals of one atom).
    Pivot lengths are drawn from ``lengths`` = (low, high): a wide range leaves triangles that cannot be closed.  ``extra_rows``: (molecule, atom,
    cumnum) rows put IN FRONT of that molecule's reactive_cumnums (a duplicated cumnum: the later row wins)."""
    rng = np.random.default_rng(seed)
    mols, offset = [], 0
    for m in range(3):
        n = n_atoms[m]
        coords = rng.normal(size=(n_conf[m], n, 3)) * 1.5
        reactive = np.sort(rng.choice(n, size=n_reactive[m], replace=False))
        pivots = []
        for c in range(n_conf[m]):
            vec = rng.normal(size=(n_pivots[m], 3))
            vec *= (rng.uniform(lengths[0], lengths[1], size=n_pivots[m]) / np.linalg.norm(vec, axis=1))[:, None]
            mean = coords[c][reactive].mean(axis=0) + rng.normal(size=(n_pivots[m], 3))
            ends = np.array([[reactive[0], reactive[-1]] if q % 2 == 0 else [reactive[-1], reactive[0]] for q in range(n_pivots[m])])
            pivots.append((vec, mean, ends + offset))
        rows = [[int(a), int(cum)] for mm, a, cum in extra_rows if mm == m] + [[int(i), int(i) + offset] for i in reactive]
        mols.append(dict(coords=coords, reactive_indices=reactive, reactive_cumnums=np.array(rows, dtype=np.int64), pivots=pivots))
        offset += n
    return mols


def costs343(E, coords, reactive, cumnums, norms, directions, ids, vecs, pivot, meanpoint, conf_ids):
    """The 343 costs of ``E._adjust_directions3`` for one group, from its own definition (the function returns only what the best one gives);
    ``host_groups`` checks that their argmin reproduces what the function returned."""
    p, p_mean, tri = vecs[:, 1] - vecs[:, 0], vecs.mean(axis=1), E._triangle3(norms)
    rot, pos = [], []
    for i in range(3):
        mol_direction = meanpoint[i] - coords[i][conf_ids[i]][reactive[i]].mean(axis=0)
        if np.all(mol_direction == 0.0):
            mol_direction = meanpoint[i]
        r_i = E.align_vec_pair(np.array([p[i], directions[i]]), np.array([pivot[i], mol_direction]))
        rot.append(r_i), pos.append(p_mean[i] - r_i @ meanpoint[i])
    facing = np.zeros((3, 3), dtype=np.int64)
    for c in ids:
        found = [None, None]
        for m in range(3):
            for index, cum in cumnums[m]:
                if cum == c[0]:
                    found[0] = (m, int(index))
                if cum == c[1]:
                    found[1] = (m, int(index))
        (m0, i0), (m1, i1) = found
        facing[m0, m1], facing[m1, m0] = i0, i1
    steps = np.arange(7) * 10.0 - 30.0
    turn = [np.array([E.rot_mat_from_pointer(p[i], a) for a in steps]) for i in range(3)]
    idx = ((E._ADJUST_ANGLES + 30.0) / 10.0).round().astype(np.int64)
    new = {(m, q): turn[m][idx[:, m]] @ (rot[m] @ coords[m][0][facing[m, q]] + pos[m]) for m, q in ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))}

    def ang(u, w):
        un, wn = u / np.sqrt((u * u).sum(axis=1, keepdims=True)), w / np.sqrt((w * w).sum(axis=1, keepdims=True))
        return np.degrees(np.arccos(np.clip((un * wn).sum(axis=1), -1.0, 1.0)))
    cost = ang(tri[0] - new[0, 2], new[2, 0] - tri[0]) + ang(tri[1] - new[0, 1], new[1, 0] - tri[1]) + ang(tri[2] - new[2, 1], new[1, 2] - tri[2])
    best = int(np.argmin(cost))
    out = np.array([p_mean[0] - (new[0, 1][best] + new[0, 2][best]) / 2, p_mean[1] - (new[1, 0][best] + new[1, 2][best]) / 2,
                    p_mean[2] - (new[2, 0][best] + new[2, 1][best]) / 2])
    return cost, best, out


def host_groups(mols, pairings=None, internal_constraints=()):
    """``_trimolecular_groups`` (the host yardstick) on mols: (blocks, group_ids, meta, best i32[G], gap f64[G], calls) -- best = the argmin of
    every group's 343 costs, gap = second smallest - smallest, calls = the arguments ``_adjust_directions3`` saw, group by group."""
    from tscode_amd import embeds as E
    coords, reactive, pivots, cumnums = unpack(mols)
    seen, original = [], E._adjust_directions3

    def recorder(coords_, reactive_, cumnums_, norms, directions, ids, vecs, pivot, meanpoint, conf_ids):
        args = (coords_, reactive_, cumnums_, norms.copy(), np.array(directions, copy=True), [list(c) for c in ids], np.array(vecs, copy=True),
                [np.array(q) for q in pivot], [np.array(q) for q in meanpoint], np.array(conf_ids))
        out = original(coords_, reactive_, cumnums_, norms, directions, ids, vecs, pivot, meanpoint, conf_ids)
        cost, best, mine = costs343(E, *args)
        assert np.array_equal(mine, out), "the recorder's costs do not reproduce _adjust_directions3"
        two = np.partition(cost, 1)[:2]
        seen.append((best, float(two[1] - two[0]), args))
        return out
    E._adjust_directions3 = recorder
    try:
        blocks, group_ids, meta = E._trimolecular_groups(coords, reactive, pivots, cumnums, pairings, internal_constraints)
    finally:
        E._adjust_directions3 = original
    return (blocks, group_ids, meta, np.array([s[0] for s in seen], dtype=np.int32), np.array([s[1] for s in seen]), [s[2] for s in seen])
