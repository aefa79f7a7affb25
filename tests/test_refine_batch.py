"""similarity_refining_batch: the similarity stages of Embedder.similarity_refining (tscode/embedder.py:1310-1388) on a list of ensembles,
one batched call per stage (tscode_amd/optimization_methods.py).  The yardstick is the chain of the single-ensemble calls under the same
gates, never the batch code itself."""

import numpy as np
import pytest

from test_rot_corr import case as g19_case

RMSD_THR = 0.25


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def chain(structures, atomnos, quadruplets, setup, rmsd_thr, masses, tfd=True, moi=True, rmsd=True):
    """tscode/embedder.py:1322-1382 by hand with the single-ensemble calls: (structures, mask over the input rows)."""
    import tscode_amd
    cur, rows = np.asarray(structures), np.arange(len(structures))
    if tfd and quadruplets is not None and len(quadruplets) > 0:                                   # :1332-1333
        cur, mask = tscode_amd.prune_conformers_tfd(cur, quadruplets)
        rows = rows[mask]
    if moi and len(cur) <= 500:                                                                    # :1342
        cur, mask = tscode_amd.prune_by_moment_of_inertia(cur, atomnos, masses=masses)
        rows = rows[mask]
    if rmsd and len(cur) <= 1e5:                                                                   # :1356
        cur, mask = tscode_amd.prune_conformers_rmsd(cur, atomnos, rmsd_thr=rmsd_thr)
        rows = rows[mask]
        if len(cur) <= 500 and setup is not None:                                                  # :1372
            cur, mask = tscode_amd.prune_rmsd_rot_corr_arrays(cur, atomnos, **setup, max_rmsd=rmsd_thr)
            rows = rows[mask]
    full = np.zeros(len(structures), dtype=bool)
    full[rows] = True
    return cur, full


def masses_of(atomnos):
    return np.array([{1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998}[int(z)] for z in atomnos])


_INPUT = {}


def refine_input():
    """G19 n40 with TFD quadruplets (its torsions) and its rot-corr set-up, n150 with a set-up and no quadruplets, the notors molecule
    with neither, and 501 structures (n150's, repeated with noise of 0.5 A per coordinate: every pair lies far above the RMSD threshold,
    so all 501 are left after the RMSD stage) that skip MOI (:1342) and rot-corr (:1372)."""
    if not _INPUT:
        a, b, c = g19_case("n40"), g19_case("n150"), g19_case("notors")
        rng = np.random.default_rng(501)
        many = b.structures[np.arange(501) % len(b.structures)] + rng.normal(scale=0.5, size=(501,) + b.structures.shape[1:])
        _INPUT["v"] = dict(ensembles=[a.structures, b.structures, c.structures, many],
                           atomnos=[a.atomnos, b.atomnos, c.atomnos, b.atomnos],
                           quadruplets=[np.asarray(a.setup["torsions"], dtype=np.int32), None, np.zeros((0, 4), dtype=np.int32), None],
                           rot_corr=[a.setup, b.setup, None, b.setup])
    return _INPUT["v"]


# ------------------------------------------------------------------------------------------------------- CPU
def test_argument_checks_raise_valueerror_before_the_library_is_entered(monkeypatch):
    import tscode_amd
    from tscode_amd import numba_functions, optimization_methods, rmsd_pruning, rot_corr

    def no_device(*a, **k):
        raise AssertionError("the library was entered")
    for module in (numba_functions, optimization_methods, rmsd_pruning, rot_corr):
        monkeypatch.setattr(module, "get_engine", no_device)
    v = refine_input()
    ens, nos, quads, setups = ([x[:5] for x in v["ensembles"][:2]], v["atomnos"][:2], v["quadruplets"][:2], v["rot_corr"][:2])
    refine = tscode_amd.similarity_refining_batch
    n = ens[1].shape[1]
    for bad in (lambda: refine(ens, nos[:1]),
                lambda: refine(ens, nos + nos),
                lambda: refine(ens, nos[0]),                                                       # 23 entries for ensemble 1's 40 atoms
                lambda: refine([ens[0], ens[1][0]], nos),                                          # not (N, n, 3)
                lambda: refine(ens, nos, quadruplets=quads[:1]),
                lambda: refine(ens, nos, quadruplets=[quads[0], np.array([[0, 1, 2, n]])]),        # atom n of n
                lambda: refine(ens, nos, rot_corr=setups + setups),
                lambda: refine(ens, nos, rot_corr=[setups[0], {**setups[1], "sub_nodes": [[n]] * 6}]),
                lambda: refine(ens, nos, rot_corr=[setups[0], {**setups[1], "angles": [np.arange(7.0)] * 6}]),
                lambda: refine(ens, nos, rmsd_thr=[0.25]),
                lambda: refine(ens, nos, masses=[np.ones(23)])):
        with pytest.raises(ValueError):
            bad()
    assert refine([], nos[0]) == []
    # one quadruplet array and one set-up dict stand for all ensembles: ensemble 0's 23 atoms do not hold n150's indices
    same = [ens[1], ens[1][:3]]
    with pytest.raises(ValueError, match="ensemble 0"):
        refine([ens[0], ens[1]], nos, rot_corr=setups[1])
    with pytest.raises(ValueError, match="quadruplet"):
        refine([ens[0], ens[1]], nos, quadruplets=np.array([[0, 1, 2, n - 1]]))
    got = refine(same, nos[1], quadruplets=np.array([[0, 1, 2, n - 1]]), rot_corr=setups[1], tfd=False, moi=False, rmsd=False)
    assert [m.tolist() for _, m in got] == [[True] * 5, [True] * 3]
    # a hydrogen-only ensemble is each stage's own business: with the stages off it passes through
    got = refine([ens[0]], np.ones(ens[0].shape[1], dtype=int), tfd=False, moi=False, rmsd=False)
    assert got[0][1].all()
    # with every stage switched off nothing is computed: every row comes back
    got = refine(ens, nos, quadruplets=quads, rot_corr=setups, tfd=False, moi=False, rmsd=False)
    for e, (kept, mask) in zip(ens, got):
        assert mask.all() and kept.tobytes() == e.tobytes()


# ------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_batch_equals_the_chain_of_single_calls_under_the_same_gates(monkeypatch):
    pytest.importorskip("networkx")
    import tscode_amd
    import tscode_amd.optimization_methods as om
    import tscode_amd.rot_corr as rc
    v = refine_input()
    masses = [masses_of(z) for z in v["atomnos"]]
    seen = {"moi": [], "rot_corr": []}                  # the sizes each gated stage was handed
    real_moi, real_rc = om.prune_by_moment_of_inertia_batch, rc.prune_rmsd_rot_corr_arrays_batch
    monkeypatch.setattr(om, "prune_by_moment_of_inertia_batch", lambda e, *a, **k: (seen["moi"].extend(len(x) for x in e), real_moi(e, *a, **k))[1])
    monkeypatch.setattr(rc, "prune_rmsd_rot_corr_arrays_batch", lambda e, *a, **k: (seen["rot_corr"].extend(len(x) for x in e), real_rc(e, *a, **k))[1])
    got = tscode_amd.similarity_refining_batch(**v, rmsd_thr=RMSD_THR, masses=masses)
    assert len(got) == 4
    for s, (e, z, q, st, m) in enumerate(zip(v["ensembles"], v["atomnos"], v["quadruplets"], v["rot_corr"], masses)):
        kept, mask = chain(e, z, q, st, RMSD_THR, m)
        assert got[s][1].dtype == np.bool_ and got[s][1].shape == (len(e),) and np.array_equal(got[s][1], mask), (s, int(got[s][1].sum()), int(mask.sum()))
        assert got[s][0].shape == kept.shape and np.array_equal(bits(got[s][0]), bits(kept)), s
    # the gates: the 501 structures skip MOI (:1342), all of them are left after RMSD, and so they skip rot-corr too (:1372)
    after_tfd = len(tscode_amd.prune_conformers_tfd(v["ensembles"][0], v["quadruplets"][0])[0])
    assert seen["moi"] == [after_tfd, len(v["ensembles"][1]), len(v["ensembles"][2])], seen
    assert len(seen["rot_corr"]) == 2 and max(seen["rot_corr"]) <= 150, seen            # n40 and n150 alone (the notors molecule has no set-up)
    assert got[3][1].all() and len(got[3][0]) == 501, "the RMSD stage was meant to keep all 501 structures"
    assert got[3][0].tobytes() == np.asarray(v["ensembles"][3]).tobytes(), "501 structures skip rot-corr: they come back as given, not centred"
    assert not np.array_equal(got[0][0], v["ensembles"][0][got[0][1]]), "n40 went through rot-corr: it comes back centred and turned"
    assert np.array_equal(got[2][0], v["ensembles"][2][got[2][1]]), "the notors molecule has no set-up: its rows come back as they were given"
    assert any(0 < int(m.sum()) < len(m) for _, m in got[:2]), "nothing was pruned"


@pytest.mark.gpu
def test_stage_switches():
    pytest.importorskip("networkx")
    import tscode_amd
    v = refine_input()
    three = {k: x[:3] for k, x in v.items()}
    masses = [masses_of(z) for z in three["atomnos"]]
    off = tscode_amd.similarity_refining_batch(**three, rmsd_thr=RMSD_THR, masses=masses, tfd=False, moi=False, rmsd=False)
    for e, (kept, mask) in zip(three["ensembles"], off):
        assert mask.all() and kept.tobytes() == np.asarray(e).tobytes()
    for switches in (dict(tfd=False), dict(moi=False), dict(rmsd=False)):
        got = tscode_amd.similarity_refining_batch(**three, rmsd_thr=RMSD_THR, masses=masses, **switches)
        for s in range(3):
            kept, mask = chain(three["ensembles"][s], three["atomnos"][s], three["quadruplets"][s], three["rot_corr"][s], RMSD_THR, masses[s], **switches)
            assert np.array_equal(got[s][1], mask) and np.array_equal(bits(got[s][0]), bits(kept)), (switches, s)
