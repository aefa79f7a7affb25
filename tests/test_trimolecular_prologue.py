"""The host part of the three-molecule cyclical embed's groups (tscode_amd.embeds._trimolecular_prologue, trimolecular_groups_batch's argument
checks, the two new C symbols): no GPU.  The prologue works out per pivot triple, for all triples at once, what the host loop
``_trimolecular_groups`` works out with ``_triangle3`` / ``_polygonize3`` / ``_directions3`` one triple at a time; those functions are the
yardstick, and the comparison is bit for bit."""

import os
import re

import numpy as np
import pytest

import trimolecular_cases as tc

NEW_SYMBOLS = ("tsc_trimolecular_groups", "tsc_trimolecular_groups_timings")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pivot_mols(seed, n_random=7):
    """Three one-conformer molecules whose pivots are axis-parallel vectors of lengths 3, 4, 5 and scaled copies (6, 8, 10; 1.5, 2, 2.5: their
    np.linalg.norm is exact), plus random ones: the cartesian product of the pivots holds every 3-4-5 triangle with every side in the
    hypotenuse's place, equilateral (3, 3, 3), obtuse for each vertex ((3, 3, 5), (3, 5, 3), (5, 3, 3)), impossible ((3, 4, 8), (1.5, 2, 10))."""
    rng = np.random.default_rng(seed)
    exact = [3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 1.5, 2.0, 2.5]
    mols, offset = [], 0
    for m in range(3):
        vec = np.zeros((len(exact) + n_random, 3))
        for q, length in enumerate(exact):
            vec[q, (q + m) % 3] = length if q % 2 == 0 else -length
        rnd = rng.normal(size=(n_random, 3))
        vec[len(exact):] = rnd * (rng.uniform(1.0, 7.0, size=n_random) / np.linalg.norm(rnd, axis=1))[:, None]
        P = len(vec)
        coords = rng.normal(size=(1, 6, 3))
        cums = np.array([[offset, offset + 1] if q % 2 == 0 else [offset + 1, offset] for q in range(P)])
        mols.append(dict(coords=coords, reactive_indices=np.array([0, 1]), reactive_cumnums=np.array([[0, offset], [1, offset + 1]]),
                         pivots=[(vec, rng.normal(size=(P, 3)), cums)]))
        offset += 6
    return mols


@pytest.mark.parametrize("seed", [0, 1])
def test_prologue_equals_the_loops_functions_bit_for_bit(seed):
    from tscode_amd import embeds as E
    from tscode_amd.utils import cartesian_product
    mols = _pivot_mols(seed)
    coords, reactive, pivots, cumnums = tc.unpack(mols)
    pro = E._trimolecular_prologue(coords, reactive, pivots, cumnums, None, ())
    vec = [np.asarray(pivots[m][0][0], dtype=np.float64) for m in range(3)]
    n_all = n_pass = n_right = n_equilateral = 0
    flips = np.zeros(3, dtype=int)
    for pi in cartesian_product(*[np.arange(len(v)) for v in vec]):                  # the loop of _trimolecular_groups, its functions
        n_all += 1
        norms = np.array([np.linalg.norm(vec[m][pi[m]]) for m in range(3)])
        if not all(norms[i] < norms[i - 1] + norms[i - 2] for i in (0, 1, 2)):
            continue
        t, n_pass = n_pass, n_pass + 1
        assert np.array_equal(pro.pivot_index[t], pi) and np.array_equal(pro.norms[t], norms)
        before = norms.copy()
        poly = E._polygonize3(norms)
        directions = E._directions3(norms)                                          # (nudges norms in place)
        assert np.array_equal(pro.poly[t], poly), (pi, before)
        assert np.array_equal(pro.tri_poly[t], E._triangle3(before)), (pi, before)
        assert np.array_equal(pro.directions[t], directions), (pi, before, pro.directions[t] - directions)
        assert np.array_equal(pro.norms_cost[t], norms) and np.array_equal(pro.tri_cost[t], E._triangle3(norms)), (pi, before)
        assert np.isfinite(directions).all()
        n_right += int(not np.array_equal(before, norms))
        n_equilateral += int(before[0] == before[1] == before[2])
        v = E._triangle3(before)[:, :2]
        flips += [E._plane_angle(v[1] - v[0], v[2] - v[0]) > 90, E._plane_angle(v[0] - v[1], v[2] - v[1]) > 90, E._plane_angle(v[0] - v[2], v[1] - v[2]) > 90]
    assert n_pass == len(pro.conf) and n_all == 16 ** 3 and n_pass < n_all           # several thousand triangles, some of them impossible
    assert n_pass > 2000 and n_right >= 6 and n_equilateral >= 3 and (flips > 50).all(), (n_pass, n_right, n_equilateral, flips)
    assert (pro.mask == 255).all() and pro.take.all()                               # no pairings: every orientation


def test_exactly_right_triangles_with_every_side_as_the_hypotenuse():
    """3-4-5 and scaled copies, each side in the hypotenuse's place: the circumcentre lies on a side's middle, _directions3 nudges norms[0] by
    1e-5 and recurses.  The arrays must take the same branch and give the same bits, the nudged triangle included."""
    from itertools import permutations
    from tscode_amd import embeds as E
    rows = np.array([np.array(p) * s for s in (1.0, 2.0, 0.5, 3.0) for p in permutations((3.0, 4.0, 5.0))])
    mine = rows.copy()
    directions = E._directions3_all(mine)
    nudged = 0
    for k, norms in enumerate(rows):
        theirs = norms.copy()
        want = E._directions3(theirs)
        assert np.array_equal(directions[k], want) and np.array_equal(mine[k], theirs), (norms, directions[k] - want)
        assert np.array_equal(E._triangle3_all(mine[k:k + 1])[0], E._triangle3(theirs))
        nudged += int(theirs[0] != norms[0])
    assert nudged >= 4                                                               # (which of them come out exactly right is rounding's business)


def test_orientation_mask_follows_the_pairings():
    """Pairings that remove some orientations, one of them matched through internal_constraints: the mask against the groups the host loop keeps
    (G18 case 0, 6 pivot triples)."""
    from tscode_amd import embeds as E
    g, mols = tc.g18_case(0)
    coords, reactive, pivots, cumnums = tc.unpack(mols)
    _, ids_all, meta_all = E._trimolecular_groups(coords, reactive, pivots, cumnums, None, ())
    pair = ids_all[0][0].tolist()
    absent = [int(ids_all.max()) + 5, int(ids_all.max()) + 9]                          # in no group's ids
    for pairings, constraints in (([pair], ()), ([pair, ids_all[0][1].tolist()], ()), ([pair, absent], np.array([[absent[0], 10 ** 6]])),
                                  ([absent], ()), ([pair[::-1]], ())):
        _, ids, meta = E._trimolecular_groups(coords, reactive, pivots, cumnums, pairings, constraints)
        pro = E._trimolecular_prologue(coords, reactive, pivots, cumnums, pairings, constraints)
        t_of, v_of = np.nonzero(pro.take)
        assert [(tuple(pro.conf[t]), tuple(pro.pivot_index[t]), int(v)) for t, v in zip(t_of, v_of)] == [(c, p, v) for c, p, v in meta]
        assert np.array_equal(pro.ids[t_of, v_of].reshape(-1, 3, 2), ids)
        assert np.array_equal(pro.mask, np.packbits(pro.take, axis=1, bitorder="little").ravel())
        assert len(meta) < len(meta_all)
    kept = E._trimolecular_prologue(coords, reactive, pivots, cumnums, [pair], ()).take
    assert 0 < kept.sum() < kept.size and not kept.all(axis=1).any()                  # some orientations of a triple go, others stay


def test_new_symbols_are_declared_and_exported():
    from tscode_amd import _lib
    from tscode_amd.build import build
    build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tscode_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(r"\bint " + s + r"\(tsc_ctx \*ctx", header), s
    assert "embeds.py:312-465" in header and ":636-655" in header
    assert len(_lib._SIGNATURES["tsc_trimolecular_groups"][1]) == header.split("int tsc_trimolecular_groups(")[1].split(");")[0].count(",") + 1


def test_argument_refusals_come_before_the_library(monkeypatch):
    import tscode_amd
    from tscode_amd import embeds as E

    def no_engine():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(E, "get_engine", no_engine)
    fresh = lambda: tc.synthetic_mols(3)

    mols = fresh()
    mols[1]["pivots"][0][2][0, 0] = 9999                                            # a pivot's cumnum that no reactive_cumnums holds
    with pytest.raises(ValueError, match="cumnum 9999"):
        tscode_amd.trimolecular_groups_batch(mols)
    mols = fresh()
    mols[0]["reactive_indices"] = np.array([0, 5])                                  # 5 atoms: index out of range
    with pytest.raises(ValueError, match="reactive"):
        tscode_amd.trimolecular_groups_batch(mols)
    mols = fresh()
    mols[2]["reactive_cumnums"] = np.array([[70, 1], [3, 2]])
    with pytest.raises(ValueError, match="atom"):
        tscode_amd.trimolecular_groups_batch(mols)
    mols = fresh()
    mols[1]["reactive_cumnums"] = np.concatenate([mols[1]["reactive_cumnums"]] * 5)[:9]
    with pytest.raises(ValueError, match="9 rows"):
        tscode_amd.trimolecular_groups_batch(mols)
    with pytest.raises(ValueError):
        tscode_amd.trimolecular_groups_batch(fresh()[:2])
    with pytest.raises(ValueError):
        tscode_amd.cyclical_embed_batch(fresh(), np.zeros((2, 3)), groups_on="nowhere")
    # nothing to do: no pivots, only triangles that cannot be closed, or pairings that leave no orientation -- empty arrays, no library call
    mols = fresh()
    mols[0]["pivots"] = [(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2), dtype=np.int64))]
    cases = [mols, tc.synthetic_mols(3, n_pivots=(1, 1, 1), lengths=(1.0, 1.0)), fresh()]
    cases[1][0]["pivots"][0][0][:] *= 5.0                                           # sides 5, 1, 1
    for k, mols in enumerate(cases):
        out = tscode_amd.trimolecular_groups_batch(mols, pairings=[[10 ** 6, 10 ** 6 + 1]] if k == 2 else None)
        assert out.blocks.shape == (0, 3, 23) and out.group_ids.shape == (0, 3, 2) and out.group_ids.dtype == np.int64
        assert out.conf.shape == (0, 3) and out.pivot_index.shape == (0, 3) and out.orientation.shape == (0,) and out.best.shape == (0,)
        poses, cons = tscode_amd.cyclical_embed_batch(mols, np.zeros((2, 3)), pairings=[[10 ** 6, 10 ** 6 + 1]] if k == 2 else None)
        assert poses.shape == (0, 108, 3) and cons.shape == (0, 3, 2)
