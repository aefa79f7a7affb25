"""The groups of a three-molecule cyclical embed produced on the device (csrc/trimolecular.hpp: k_trimolecular_groups;
tscode_amd.trimolecular_groups_batch; cyclical_embed_batch's three-molecule route) against the host loop ``_trimolecular_groups`` and the
oracle's ``get_directions3`` / ``adjust_directions3`` / ``cyclical_embed3``.  The new code is never its own yardstick.

Every comparison of an argmin first shows a guard band: from the host computation the gap between the smallest and the second smallest of a
group's 343 costs is at least GAP_BAND (tests/trimolecular_cases.py) -- in every group of the fixture cases, and in a sweep all but at most 5 % of
the groups, which are left out together with the later orientations of their triple (the choice is carried over)."""

import numpy as np
import pytest

import trimolecular_cases as tc

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-9             # the project's asserted value-parity tolerance (tests/test_gpu_parity.py)
TSC_ERR_INVALID = -1
TG_WAVES, GRID_CAP = 4, 512           # csrc/trimolecular.hpp, tsc_trimolecular_groups' launch (adjacent.hip)


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def _compare(got, host, max_excluded=0.05):
    """Device groups against the host loop's: ids, conformers, pivots, orientations and best exactly, every float field within VAL_TOL.  Returns
    the fraction of groups left out by the guard band."""
    blocks, group_ids, meta, best, gap, _ = host
    G = len(blocks)
    assert got.blocks.shape == (G, 3, 23) and got.group_ids.shape == (G, 3, 2) and got.best.shape == (G,)
    assert np.array_equal(got.group_ids, group_ids)
    assert [(tuple(c), tuple(p), int(v)) for c, p, v in zip(got.conf.tolist(), got.pivot_index.tolist(), got.orientation)] == [(c, p, v) for c, p, v in meta]
    out = np.zeros(G, dtype=bool)
    for q in range(G):                                                               # a group inside the band, and what its triple carries on from it
        out[q] = gap[q] < tc.GAP_BAND or (q > 0 and out[q - 1] and meta[q][:2] == meta[q - 1][:2])
    assert out.mean() <= max_excluded, (int(out.sum()), G, float(gap.min()))
    keep = ~out
    assert np.array_equal(got.best[keep], best[keep]), np.nonzero(got.best != best)[0]
    assert np.array_equal(got.blocks[:, :, 21:23], blocks[:, :, 21:23])
    err = np.abs(got.blocks[keep] - blocks[keep])
    assert not len(err) or err.max() < VAL_TOL, (float(err.max()), np.unravel_index(err.argmax(), err.shape))
    return float(out.mean())


@pytest.mark.parametrize("k", [0, 1, 2])
def test_g18_groups_against_the_host_loop_and_the_oracle(eng, oracle, k):
    """Fixture G18, case k (case 2 has two conformers on one side: the facing atoms are read from conformer 0, mol_direction from conformer
    conf_ids[m]).  No group may be left out; the directions are also the oracle's own, carried over along each triple."""
    import tscode_amd
    g, mols = tc.g18_case(k)
    host = tc.host_groups(mols)
    blocks, group_ids, meta, best, gap, calls = host
    assert gap.min() >= tc.GAP_BAND and len(blocks) == int(g[f"group_ids_{k}"].shape[0])
    got = tscode_amd.trimolecular_groups_batch(mols)
    assert _compare(got, host, max_excluded=0.0) == 0.0
    assert np.array_equal(got.group_ids, g[f"group_ids_{k}"])
    coords, reactive, pivots, cumnums = tc.unpack(mols)
    directions = None
    for q, (conf_ids, pi, v) in enumerate(meta):
        pvt = [(np.asarray(pivots[m][conf_ids[m]][0][pi[m]], dtype=np.float64), np.asarray(pivots[m][conf_ids[m]][1][pi[m]], dtype=np.float64)) for m in range(3)]
        norms = np.array([float(np.sqrt((pvt[m][0] ** 2).sum())) for m in range(3)])
        if q == 0 or meta[q - 1][:2] != (conf_ids, pi):
            directions = oracle.get_directions3(norms)                               # (nudges norms as the reference does)
        else:
            oracle.get_directions3(norms)
        poly_v = calls[q][6]
        directions = oracle.adjust_directions3(coords, reactive, cumnums, norms, directions, calls[q][5], poly_v, pvt, np.array(conf_ids))
        assert np.abs(got.blocks[q, :, 6:9] - directions).max() < VAL_TOL, (q, meta[q])


SWEEP = {
    # name: (arguments of synthetic_mols, pairings as indices into the molecules' reactive cumnums or None)
    "one_triple": (dict(seed=11, n_pivots=(1, 1, 1)), None),
    "waves_minus_one": (dict(seed=12, n_pivots=(TG_WAVES - 1, 1, 1)), None),
    "waves": (dict(seed=13, n_pivots=(2, TG_WAVES // 2, 1)), None),
    "waves_plus_one": (dict(seed=14, n_pivots=(TG_WAVES + 1, 1, 1)), None),
    "open_and_closed_triangles": (dict(seed=15, n_pivots=(3, 3, 3), lengths=(1.0, 6.0)), None),
    "single_reactive_atom": (dict(seed=16, n_pivots=(2, 2, 2), n_reactive=(2, 1, 2)), None),
    "two_conformers": (dict(seed=17, n_pivots=(2, 1, 2), n_conf=(1, 2, 1)), None),
    "first_orientation_cleared": (dict(seed=18, n_pivots=(2, 2, 1)), "first"),
    "one_orientation": (dict(seed=19, n_pivots=(2, 2, 2)), "one"),
    "duplicated_cumnum": (dict(seed=20, n_pivots=(2, 2, 1), duplicate=True), None),
}


def _sweep_case(name):
    kw, pairing = SWEEP[name]
    kw = dict(kw)
    duplicate = kw.pop("duplicate", False)
    mols = tc.synthetic_mols(**kw)
    if duplicate:                                                                    # the cumnum of molecule 1's first reactive atom, first on another atom
        r = mols[1]["reactive_cumnums"]
        other = next(a for a in range(33) if a not in r[:, 0])
        mols[1]["reactive_cumnums"] = np.concatenate([[[other, r[0, 1]]], r])
    cum = [m["reactive_cumnums"][:, 1] for m in mols]
    pairings = None
    if pairing == "first":      # molecule 0 walked backwards, molecule 1 forwards (for the pivots that run first -> last): orientations 4 and 6
        pairings = [sorted([int(cum[0][0]), int(cum[1][0])])]
    elif pairing == "one":      # ... and molecule 2 forwards too: orientation 4 alone
        pairings = [sorted([int(cum[0][0]), int(cum[1][0])]), sorted([int(cum[1][-1]), int(cum[2][0])])]
    return mols, pairings


@pytest.mark.parametrize("name", list(SWEEP))
def test_sweep_against_the_host_loop(eng, name):
    import tscode_amd
    from tscode_amd import embeds as E
    mols, pairings = _sweep_case(name)
    host = tc.host_groups(mols, pairings)
    got = tscode_amd.trimolecular_groups_batch(mols, pairings)
    _compare(got, host)
    pro = E._trimolecular_prologue(*tc.unpack(mols), pairings, ())
    if name == "open_and_closed_triangles":
        assert 0 < len(pro.conf) < 27                                                # some triangles close and some do not
    if name == "first_orientation_cleared":
        assert any(not (mk & 1) and mk for mk in pro.mask)                           # a triple whose first embedded orientation is a later one
    if name == "one_orientation":
        assert any(bin(mk).count("1") == 1 for mk in pro.mask)
    if name == "single_reactive_atom":
        assert (got.blocks[:, 1, 21] == 1).all() and np.array_equal(got.blocks[:, 1, 15:18], got.blocks[:, 1, 18:21])
    if name == "two_conformers":
        assert set(got.conf[:, 1]) == {0, 1}


def test_triple_without_a_group_between_others(eng):
    """A pairing that only the pivots between molecule 1's first two table atoms can meet: the triples of its other pivot yield no group, in the
    middle of triples that do."""
    import tscode_amd
    from tscode_amd import embeds as E
    mols = tc.synthetic_mols(21, n_pivots=(2, 3, 1))
    r = mols[1]["reactive_cumnums"]
    third = next(a for a in range(33) if a not in r[:, 0])
    mols[1]["reactive_cumnums"] = np.concatenate([r, [[third, 5 + third]]])            # (molecule 1's cumnums start at 5)
    mols[1]["pivots"][0][2][1] = [r[0, 1], 5 + third]                                 # pivot 1 of molecule 1 ends on the third atom
    pairings = [sorted([int(mols[0]["reactive_cumnums"][0, 1]), int(r[1, 1])])]
    pro = E._trimolecular_prologue(*tc.unpack(mols), pairings, ())
    assert (pro.mask == 0).any() and (pro.mask != 0).any() and pro.mask[0] != 0 and pro.mask[-1] != 0 and (pro.mask[1:-1] == 0).any()
    _compare(tscode_amd.trimolecular_groups_batch(mols, pairings), tc.host_groups(mols, pairings))


def test_right_triangle_and_a_meanpoint_on_the_reactive_atoms(eng):
    """Pivots of lengths exactly 3, 4, 5 (the polygon from the triangle as it is, the costs against the nudged one), and a molecule whose meanpoint
    is the mean of its reactive atoms (mol_direction == 0: the meanpoint itself is taken)."""
    import tscode_amd
    from tscode_amd import embeds as E
    mols = tc.synthetic_mols(22, n_pivots=(1, 1, 1))
    for m, (axis, length) in enumerate(((0, 3.0), (1, 4.0), (2, 5.0))):
        mols[m]["pivots"][0][0][0] = 0.0
        mols[m]["pivots"][0][0][0, axis] = length
    c1 = mols[1]["coords"][0][mols[1]["reactive_indices"]]
    mols[1]["pivots"][0][1][0] = c1.mean(axis=0)
    assert np.all(mols[1]["pivots"][0][1][0] - c1.mean(axis=0) == 0.0)
    pro = E._trimolecular_prologue(*tc.unpack(mols), None, ())
    assert len(pro.conf) == 1 and pro.norms_cost[0, 0] != pro.norms[0, 0] and not np.array_equal(pro.tri_cost, pro.tri_poly)
    _compare(tscode_amd.trimolecular_groups_batch(mols), tc.host_groups(mols))


def test_more_triples_than_one_pass_of_the_grid(eng):
    """Identical conformers tiled until the triples pass the grid's cap once (GRID_CAP workgroups of TG_WAVES triples): the first conformer
    triple against the host loop, every copy against the first."""
    import tscode_amd
    one = tc.synthetic_mols(23, n_pivots=(3, 3, 3))
    host = tc.host_groups(one)
    per = len(host[0])                                                               # groups of one conformer triple (27 triples)
    copies = (5, 4, 4)
    mols = [dict(m, coords=np.repeat(m["coords"], copies[i], axis=0), pivots=m["pivots"] * copies[i]) for i, m in enumerate(one)]
    got = tscode_amd.trimolecular_groups_batch(mols)
    n_copies = int(np.prod(copies))
    assert per == 27 * 8 and len(got.blocks) == per * n_copies and 27 * n_copies > GRID_CAP * TG_WAVES
    import types
    first = types.SimpleNamespace(**{key: getattr(got, key)[:per] for key in ("blocks", "group_ids", "conf", "pivot_index", "orientation", "best")})
    _compare(first, host)
    tiled = got.blocks.reshape(n_copies, per, 3, 23)
    assert np.array_equal(tiled[:, :, :, :22], np.broadcast_to(tiled[0, :, :, :22], tiled[:, :, :, :22].shape))
    assert np.array_equal(tiled[:, :, :, 22], np.broadcast_to(got.conf.reshape(n_copies, per, 3)[:, :1], tiled.shape[:3]))
    assert np.array_equal(got.best.reshape(n_copies, per), np.broadcast_to(got.best[:per], (n_copies, per)))
    assert np.array_equal(got.group_ids.reshape(n_copies, per, 3, 2), np.broadcast_to(got.group_ids[:per], (n_copies, per, 3, 2)))


def test_library_refusals_name_the_triple(eng):
    import tscode_amd
    from tscode_amd import embeds as E
    from tscode_amd._lib import TscodeHipError
    mols = tc.synthetic_mols(3)
    coords, reactive, pivots, cumnums = tc.unpack(mols)
    pro = E._trimolecular_prologue(coords, reactive, pivots, cumnums, None, ())
    frags = tscode_amd.FragmentSet(coords)
    args = lambda **kw: {**dict(frags=frags, reactive=reactive, reactive_cumnums=cumnums, conf=pro.conf, pivot=pro.pivot, meanpoint=pro.meanpoint, cumnums=pro.cumnums,
                                tri_poly=pro.tri_poly, tri_cost=pro.tri_cost, directions=pro.directions, mask=pro.mask), **kw}
    bad_cum = pro.cumnums.copy()
    bad_cum[5, 1, 0] = 9999
    bad_conf = pro.conf.copy()
    bad_conf[2, 0] = 1
    for kw, needle in ((dict(cumnums=bad_cum), "triple 5"), (dict(conf=bad_conf), "triple 2"), (dict(reactive=[reactive[0], np.array([0, 33]), reactive[2]]), "atom"),
                       (dict(reactive_cumnums=[cumnums[0], np.concatenate([cumnums[1]] * 5)[:9], cumnums[2]]), "9 reactive_cumnums rows"),
                       (dict(reactive_cumnums=[cumnums[0], np.array([[33, 7]]), cumnums[2]]), "atom 33")):
        with pytest.raises(TscodeHipError) as e:
            eng.trimolecular_groups(**args(**kw))
        assert e.value.code == TSC_ERR_INVALID and needle in str(e.value), str(e.value)
    empty = eng.trimolecular_groups(**args(conf=pro.conf[:0], pivot=pro.pivot[:0], meanpoint=pro.meanpoint[:0], cumnums=pro.cumnums[:0], tri_poly=pro.tri_poly[:0],
                                           tri_cost=pro.tri_cost[:0], directions=pro.directions[:0], mask=pro.mask[:0]))
    assert empty[0].shape == (0, 3, 23) and empty[2].shape == (0,)
    blocks, _, _, base = eng.trimolecular_groups(**args(mask=np.zeros_like(pro.mask)))   # triples, but no orientation of any
    assert blocks.shape == (0, 3, 23) and not base.any()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_whole_embed_on_g18_through_the_device_groups(eng, oracle, k):
    import tscode_amd
    g, mols = tc.g18_case(k)
    thresh = float(g[f"clash_thresh_{k}"])
    assert oracle.clash_margin(g[f"candidates_{k}"], g[f"ids_{k}"], thresh) > 1e-9
    for budget in (1 << 20, 5 * len(g[f"angles_{k}"])):                               # one call, and slabs of five groups
        poses, cons, tr = tscode_amd.cyclical_embed_batch(mols, g[f"angles_{k}"], clash_thresh=thresh, return_trace=True, max_poses_per_call=budget)
        assert np.array_equal(tr.group_of, g[f"group_of_{k}"])
        assert np.array_equal(np.array([grp[3] for grp in tr.groups]), g[f"group_ids_{k}"])
        assert np.array_equal(tr.clash_ok, g[f"clash_ok_{k}"])
        assert np.array_equal(tr.kept, g[f"kept_{k}"]), (k, tr.kept.sum(), g[f"kept_{k}"].sum())
        assert poses.shape == g[f"poses_{k}"].shape and np.abs(poses - g[f"poses_{k}"]).max() < VAL_TOL
        assert np.array_equal(cons, g[f"constrained_indices_{k}"]) and cons.shape[1:] == (3, 2)
    plain = tscode_amd.cyclical_embed_batch(mols, g[f"angles_{k}"], clash_thresh=thresh)
    assert len(plain) == 2 and np.array_equal(plain[0], poses) and np.array_equal(plain[1], cons)
    _, _, tr_host = tscode_amd.cyclical_embed_batch(mols, g[f"angles_{k}"], clash_thresh=thresh, return_trace=True, groups_on="host")
    assert tr_host.groups == tr.groups


WHOLE_SEED, WHOLE_THRESH = 32, 0.5


def test_whole_embed_new_route_against_old_route(eng, oracle):
    """Three 33-atom molecules, 27 angle sets: the device groups + one record per (group, molecule) against the host loop + one row per (pose,
    molecule) -- identical verdicts, poses within VAL_TOL -- with the oracle's candidates at least 1e-9 away from the clash threshold."""
    import tscode_amd
    from tscode_amd.utils import cartesian_product
    mols = tc.synthetic_mols(WHOLE_SEED, n_atoms=(33, 33, 33), n_pivots=(1, 1, 1))
    host = tc.host_groups(mols)
    assert host[4].min() >= tc.GAP_BAND
    steps = np.array([-40.0, 0.0, 40.0])
    angles = cartesian_product(steps, steps, steps)
    assert len(angles) == 27
    coords, reactive, pivots, cumnums = tc.unpack(mols)
    cands, group_of, ok, kept, gids = oracle.cyclical_embed3(coords, reactive, pivots, cumnums, angles, WHOLE_THRESH)
    assert oracle.clash_margin(cands, [33, 33, 33], WHOLE_THRESH) > 1e-9 and 0 < ok.sum() < len(ok)
    new = tscode_amd.cyclical_embed_batch(mols, angles, clash_thresh=WHOLE_THRESH, return_trace=True)
    old = tscode_amd.cyclical_embed_batch(mols, angles, clash_thresh=WHOLE_THRESH, return_trace=True, groups_on="host")
    assert np.array_equal(new[2].clash_ok, old[2].clash_ok) and np.array_equal(new[2].kept, old[2].kept) and np.array_equal(new[2].group_of, old[2].group_of)
    assert new[2].groups == old[2].groups and np.array_equal(new[1], old[1])
    assert new[0].shape == old[0].shape and len(new[0]) and np.abs(new[0] - old[0]).max() < VAL_TOL
    assert np.array_equal(new[2].clash_ok, ok) and np.array_equal(new[2].kept, kept) and np.abs(new[0] - cands[kept]).max() < VAL_TOL


def test_dropin_with_the_trimolecular_switch(eng):
    """tscode_amd.embeds.cyclical_embed(embedder) with TRIMOLECULAR = True on G18 case 0, through the duck-typed embedder of tests/dropin_reads.py:
    the recorded poses and constrained indices."""
    import sys
    from tscode_amd import embeds as E
    import dropin_reads
    from conftest import load_golden
    g18 = load_golden("G18_cyclical_embed_trimolecular")

    class Zero(Exception):
        pass
    logs = []
    saved = sys.modules.get("tscode.embeds")
    sys.modules["tscode.embeds"] = dropin_reads.reference_module_standin(Zero)
    assert E.TRIMOLECULAR is False
    E.TRIMOLECULAR = True
    try:
        emb3 = dropin_reads.duck_cyclical_embedder(g18, 0, logs, n_mols=3)
        calls = []
        original = E.trimolecular_groups_batch
        E.trimolecular_groups_batch = lambda *a, **kw: calls.append(1) or original(*a, **kw)
        try:
            poses3 = E.cyclical_embed(emb3)
        finally:
            E.trimolecular_groups_batch = original
        assert calls == [1]                                                          # the groups came from the device
        assert poses3.shape == g18["poses_0"].shape and np.abs(poses3 - g18["poses_0"]).max() < VAL_TOL
        assert np.array_equal(emb3.constrained_indices, g18["constrained_indices_0"])
    finally:
        E.TRIMOLECULAR = False
        if saved is None:
            sys.modules.pop("tscode.embeds", None)
        else:
            sys.modules["tscode.embeds"] = saved
