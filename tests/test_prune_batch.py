"""prune_conformers_rmsd_batch: many small ensembles pruned in one launch (csrc/prune_batch.hpp, one workgroup per ensemble).

Without a GPU: the argument checks of the Python layer and the packing of a batch.  On the GPU: the reference's own recorded runs
(G3), the CPU oracle on ensembles whose sizes sit on both sides of every gate of the schedule and of the kernel's 64-column step,
the single-ensemble call, and the properties a batch must have (order, independence, routing of long ensembles, non-finite input).

Every oracle comparison first asserts that no pair the reference evaluates lies within 1e-6 of a threshold (oracle.prune_margins):
two correct evaluations of rmsd / maxdev agree to ~1e-13, so beyond that margin they must give the same verdict.  No case is skipped."""

import numpy as np
import pytest

from conftest import load_golden

SIZES = [1, 2, 3, 20, 21, 22, 40, 41, 42, 63, 64, 65, 100, 101, 105, 127, 128, 129, 199, 201, 257, 400, 401, 513, 1003]
HEAVY = [3, 4, 9, 18, 30, 31, 64]
MARGIN = 1e-6
STAT_KEYS = ("k", "n_active_before", "n_active_after", "pairs_evaluated", "new_keys")


def draw_ensemble(rng, n, h):
    """One ensemble of the issue's recipe: noisy copies of a few parents, so that a prune removes something.  Draw order as written."""
    n_par = max(1, n // int(rng.integers(1, 9)))
    spread = float(rng.choice([0.01, 0.05, 0.15, 0.3]))
    parents = rng.normal(size=(n_par, h, 3)) * float(rng.choice([1, 3, 8])) + rng.normal(size=(n_par, 1, 3)) * 2
    structures = parents[rng.integers(0, n_par, n)] + rng.normal(size=(n, h, 3)) * spread
    thr = float(rng.choice([0.25, 0.5, 1.0]))
    return np.ascontiguousarray(structures), thr


_edge, _edge_ref, _many = {}, {}, {}


def edge_batch(seed):
    """50 ensembles: SIZES twice, heavy counts HEAVY[(s * 3 + seed) % 7], all from one default_rng(seed)."""
    if seed not in _edge:
        rng = np.random.default_rng(seed)
        drawn = [draw_ensemble(rng, n, HEAVY[(s * 3 + seed) % 7]) for s, n in enumerate(SIZES + SIZES)]
        _edge[seed] = ([d[0] for d in drawn], [d[1] for d in drawn])
    return _edge[seed]


def edge_reference(oracle, seed, mode):
    """The oracle's run of every ensemble of edge_batch(seed), computed once; the margin condition is asserted here for all of them."""
    if (seed, mode) not in _edge_ref:
        heavies, thrs = edge_batch(seed)
        refs = []
        for s, (hv, thr) in enumerate(zip(heavies, thrs)):
            assert min(oracle.prune_margins(hv, thr, mode)) > MARGIN, (seed, mode, s)
            refs.append(oracle.prune_heavy(hv, thr, mode))
        _edge_ref[(seed, mode)] = refs
    return _edge_ref[(seed, mode)]


MANY_SEED = 2603   # (the first seed tried: no pair of its 3 000 ensembles lies within MARGIN of a threshold)


def many_batch(oracle):
    """3 000 ensembles of 20 .. 60 structures with 9 heavy atoms: the sizes first, then the recipe per ensemble, one default_rng."""
    if not _many:
        rng = np.random.default_rng(MANY_SEED)
        sizes = rng.integers(20, 61, 3000)
        drawn = [draw_ensemble(rng, int(n), 9) for n in sizes]
        heavies, thrs = [d[0] for d in drawn], [d[1] for d in drawn]
        masks = []
        for s, (hv, thr) in enumerate(zip(heavies, thrs)):
            assert min(oracle.prune_margins(hv, thr, 0)) > MARGIN, (MANY_SEED, s)
            masks.append(oracle.prune_heavy(hv, thr, 0)["mask"])
        _many.update(heavies=heavies, thrs=thrs, masks=masks)
    return _many


def carbons(heavies):
    return [np.full(hv.shape[1], 6) for hv in heavies]


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


# ----------------------------------------------------------------------------- without a GPU
def test_batch_arguments_are_refused_before_the_engine_is_touched(monkeypatch):
    import tscode_amd.rmsd_pruning as rp

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(rp, "get_engine", no_engine)
    c3 = np.array([6, 6, 1])
    good = [np.zeros((4, 3, 3)), np.zeros((2, 3, 3))]
    with pytest.raises(ValueError):
        rp.prune_conformers_rmsd_batch([np.zeros((4, 3, 3)), np.zeros((2, 4, 3))], c3)            # atom count against a shared atomnos
    with pytest.raises(ValueError):
        rp.prune_conformers_rmsd_batch([np.zeros((4, 3, 3)), np.zeros((2, 3))], c3)               # not (N, n, 3)
    with pytest.raises(ValueError):
        rp.prune_conformers_rmsd_batch([np.zeros((4, 3, 3)), np.zeros((2, 3, 2))], c3)
    with pytest.raises(ValueError):
        rp.prune_conformers_rmsd_batch(good, [c3, c3, c3])                                        # three atomnos for two ensembles
    with pytest.raises(ValueError):
        rp.prune_conformers_rmsd_batch(good, [c3, np.array([6, 6, 1, 1])])                        # the second does not fit its ensemble
    with pytest.raises(ValueError):
        rp.prune_conformers_rmsd_batch(good, c3, rmsd_thr=[0.5, 0.25, 0.5])                       # three thresholds
    with pytest.raises(ZeroDivisionError):
        rp.prune_conformers_rmsd_batch(good, [c3, np.array([1, 1, 1])])                           # an ensemble without heavy atoms
    with pytest.raises(ZeroDivisionError):
        rp.prune_conformers_rmsd_batch(good, np.array([1, 1, 1]))
    assert rp.prune_conformers_rmsd_batch([], c3) == [] and rp.last_prune_batch_stats() == []     # an empty batch needs no engine either


def test_packing_of_a_three_ensemble_batch():
    from tscode_amd import pack_heavy_batch
    a = np.arange(2 * 3 * 3, dtype=np.float64).reshape(2, 3, 3)
    b = np.zeros((0, 5, 3))
    c = -np.arange(4 * 1 * 3, dtype=np.float32).reshape(4, 1, 3)
    flat, offsets, n, h = pack_heavy_batch([a, b, c[::1]])
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 18, 18, 30]
    assert n.dtype == np.int32 and n.tolist() == [2, 0, 4]
    assert h.dtype == np.int32 and h.tolist() == [3, 5, 1]
    assert flat.dtype == np.float64 and flat.flags.c_contiguous and flat.shape == (30,)
    assert np.array_equal(flat[:18], a.ravel()) and np.array_equal(flat[18:], c.ravel().astype(np.float64))
    assert pack_heavy_batch([])[1].tolist() == [0]
    with pytest.raises(ValueError):
        pack_heavy_batch([a, np.zeros((3, 3))])


# ----------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
def test_reference_runs_in_one_call_under_every_routing(eng):
    """G3: the reference's own six runs (N = 40 .. 2500, a remainder chunk at 1003) as one batch; with the option at its default the
    2500-structure case is routed to the single-ensemble path, at 4096 the kernel takes all six, at 64 only the first."""
    import tscode_amd
    g = load_golden("G3_prune")
    cases = range(int(g["n_cases"]))
    structures, atomnos = [g[f"structures{c}"] for c in cases], [g[f"atomnos{c}"] for c in cases]
    thrs = [float(g[f"thr{c}"]) for c in cases]
    assert sorted(len(s) for s in structures) == [40, 600, 600, 720, 1003, 2500]
    default = eng.prune_batch_max_n
    results = []
    for max_n in (default, 4096, 64):
        with eng.options(prune_batch_max_n=max_n):
            out = tscode_amd.prune_conformers_rmsd_batch(structures, atomnos, thrs)
            stats = tscode_amd.last_prune_batch_stats()
            for c in cases:
                assert np.array_equal(out[c][1], g[f"mask{c}"]), (max_n, c)
                assert np.array_equal(out[c][0], structures[c][g[f"mask{c}"]])
                assert [p["k"] for p in stats[c]] == g[f"ks{c}"].tolist(), (max_n, c)
                assert [p["n_active_after"] for p in stats[c]] == g[f"pass_masks{c}"].sum(axis=1).tolist(), (max_n, c)
                assert np.cumsum([p["new_keys"] for p in stats[c]]).tolist() == g[f"pass_nkeys{c}"].tolist(), (max_n, c)
            results.append(([m for _, m in out], stats))
    for masks, stats in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(masks, results[0][0]))
        assert stats == results[0][1]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", [2601, 2602])
def test_edge_sizes_against_the_oracle(eng, oracle, seed, mode):
    heavies, thrs = edge_batch(seed)
    refs = edge_reference(oracle, seed, mode)
    if seed == 2601:
        # precondition on the generator: both modes are really exercised -- the reference's cache changes the outcome of 33 of these 50 ensembles
        other = edge_reference(oracle, seed, 1 - mode)
        assert sum(1 for x, y in zip(refs, other) if not np.array_equal(x["mask"], y["mask"])) == 33
    masks, stats, nonfinite = eng.prune_heavy_batch(heavies, thrs, mode)
    assert not nonfinite.any()
    for s, ref in enumerate(refs):
        assert np.array_equal(masks[s], ref["mask"]), (s, len(heavies[s]))
        for key in STAT_KEYS:
            assert [p[key] for p in stats[s]] == [p[key] for p in ref["stats"]], (s, len(heavies[s]), key)
    assert {p["k"] for st in stats for p in st} == {1, 2, 5, 10, 20, 50}
    assert sum(1 for m in masks if not m.all()) > 25      # (the recipe makes near-duplicates: most ensembles lose something)


@pytest.mark.gpu
def test_same_as_the_single_call(eng):
    import tscode_amd
    heavies, thrs = edge_batch(2601)
    out = tscode_amd.prune_conformers_rmsd_batch(heavies, carbons(heavies), thrs)
    for s, (hv, thr) in enumerate(zip(heavies, thrs)):
        _, single = tscode_amd.prune_conformers_rmsd(hv, np.full(hv.shape[1], 6), thr)
        assert np.array_equal(out[s][1], single), (s, len(hv))


@pytest.mark.gpu
def test_ensembles_of_a_batch_are_independent(eng, oracle):
    heavies, thrs = edge_batch(2601)
    refs = edge_reference(oracle, 2601, 0)
    masks, stats, _ = eng.prune_heavy_batch(heavies, thrs, 0)
    r_masks, r_stats, _ = eng.prune_heavy_batch(heavies[::-1], thrs[::-1], 0)
    assert all(np.array_equal(a, b) for a, b in zip(r_masks[::-1], masks)) and r_stats[::-1] == stats
    for s in (0, 13, 24, 49):
        m1, s1, _ = eng.prune_heavy_batch([heavies[s]], [thrs[s]], 0)
        assert np.array_equal(m1[0], masks[s]) and s1[0] == stats[s]
    # an empty ensemble and a single structure among others
    mixed = [np.zeros((0, 7, 3)), heavies[20], np.ones((1, 2, 3)), np.zeros((0, 1, 3))]
    m, st, nf = eng.prune_heavy_batch(mixed, [0.5, thrs[20], 0.5, 0.25], 0)
    assert m[0].shape == (0,) and m[0].dtype == bool and st[0] == [] and m[3].shape == (0,) and st[3] == []
    assert np.array_equal(m[1], refs[20]["mask"])
    assert m[2].tolist() == [True] and [p["k"] for p in st[2]] == [1] and st[2][0]["pairs_evaluated"] == 0 and not nf.any()


@pytest.mark.gpu
def test_all_atom_interface(eng, oracle):
    """Ensembles with hydrogens and different atom counts, one atomnos per ensemble, one threshold per ensemble."""
    import tscode_amd
    rng = np.random.default_rng(2604)
    ensembles, atomnos, thrs = [], [], []
    for n, n_atoms, thr in ((60, 12, 0.5), (0, 5, 0.5), (150, 31, 0.25), (45, 7, 1.0)):
        z = rng.choice([1, 6, 7, 8], n_atoms)
        z[0] = 6
        parents = rng.normal(size=(5, n_atoms, 3)) * 3
        ensembles.append(parents[rng.integers(0, 5, n)] + rng.normal(size=(n, n_atoms, 3)) * 0.05)
        atomnos.append(z)
        thrs.append(thr)
    out = tscode_amd.prune_conformers_rmsd_batch(ensembles, atomnos, thrs)
    assert len(out) == 4 and len(tscode_amd.last_prune_batch_stats()) == 4
    for e, z, thr, (pruned, mask) in zip(ensembles, atomnos, thrs, out):
        assert mask.dtype == bool and mask.shape == (len(e),)
        assert np.array_equal(pruned, e[mask])
        if len(e):
            heavy = np.ascontiguousarray(e[:, z != 1])
            assert min(oracle.prune_margins(heavy, thr, 0)) > MARGIN
            assert np.array_equal(mask, oracle.prune_heavy(heavy, thr, 0)["mask"])
            assert 0 < mask.sum() < len(e)
    # one atomnos shared by all
    shared = tscode_amd.prune_conformers_rmsd_batch([ensembles[0], ensembles[0][:20]], atomnos[0], 0.5)
    assert np.array_equal(shared[0][1], out[0][1]) and len(shared[1][1]) == 20


@pytest.mark.gpu
def test_more_ensembles_than_resident_workgroups(eng, oracle):
    ref = many_batch(oracle)
    masks, _, nonfinite = eng.prune_heavy_batch(ref["heavies"], ref["thrs"], 0)
    assert len(masks) == 3000 and not nonfinite.any()
    wrong = [s for s in range(3000) if not np.array_equal(masks[s], ref["masks"][s])]
    assert not wrong, wrong[:10]
    assert sum(1 for m in masks if not m.all()) > 1500


@pytest.mark.gpu
def test_nonfinite_input_is_flagged_on_its_ensemble_only(eng, oracle):
    import tscode_amd
    heavies, thrs = edge_batch(2601)
    refs = edge_reference(oracle, 2601, 0)
    picks = [12, 15, 20]                                   # 100, 127 and 257 structures
    batch = [heavies[s].copy() for s in picks]
    batch[1][50, 2, 1] = np.nan
    t = [thrs[s] for s in picks]
    masks, _, nonfinite = eng.prune_heavy_batch(batch, t, 0)
    assert nonfinite.tolist() == [False, True, False]
    assert np.array_equal(masks[0], refs[12]["mask"]) and np.array_equal(masks[2], refs[20]["mask"])
    assert masks[1][50]                                    # similar to nothing: kept
    with pytest.raises(np.linalg.LinAlgError, match="ensemble 1"):
        tscode_amd.prune_conformers_rmsd_batch(batch, carbons(batch), t)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_device_array_form_equals_the_host_form(eng, mode):
    """tsc_prune_rmsd_batch_dev on torch tensors: heavy atoms and every output on the device, the tables on the host."""
    import torch
    from tscode_amd import pack_heavy_batch
    from tscode_amd._lib import TSC_MAX_PASSES
    heavies, thrs = edge_batch(2602)
    heavies, thrs = heavies[:25][::-1] + [np.zeros((0, 4, 3))], thrs[:25][::-1] + [0.5]      # (1003 structures first, an empty one last)
    masks, stats, _ = eng.prune_heavy_batch(heavies, thrs, mode)
    flat, offsets, n, h = pack_heavy_batch(heavies)
    S = len(heavies)
    dev = torch.device("cuda", eng.device)
    d_heavy = torch.from_numpy(flat).to(dev)
    d_mask = torch.full((int(n.sum()),), 7, dtype=torch.uint8, device=dev)
    d_stats = torch.full((S, TSC_MAX_PASSES, 5), -1, dtype=torch.int64, device=dev)
    d_np = torch.full((S,), -1, dtype=torch.int32, device=dev)
    d_nf = torch.full((S,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    eng.prune_heavy_batch_dev(d_heavy, offsets, n, h, thrs, mode, d_mask, d_stats, d_np, d_nf)
    assert np.array_equal(d_mask.cpu().numpy().astype(bool), np.concatenate(masks))
    assert d_np.cpu().tolist() == [len(st) for st in stats] and not d_nf.cpu().any()
    table = d_stats.cpu().numpy()
    for s, st in enumerate(stats):
        assert table[s, :len(st)].tolist() == [[p[key] for key in STAT_KEYS] for p in st], s
        assert not table[s, len(st):].any()
    # the optional outputs left out
    d_mask.fill_(7)
    eng.prune_heavy_batch_dev(d_heavy, offsets, n, h, thrs, mode, d_mask)
    assert np.array_equal(d_mask.cpu().numpy().astype(bool), np.concatenate(masks))
    # a segment beyond the option is refused, with nothing written
    from tscode_amd._lib import TscodeHipError
    default = eng.prune_batch_max_n
    with eng.options(prune_batch_max_n=512):
        with pytest.raises(TscodeHipError, match="prune_batch_max_n"):
            eng.prune_heavy_batch_dev(d_heavy, offsets, n, h, thrs, mode, d_mask)
    assert eng.prune_batch_max_n == default
