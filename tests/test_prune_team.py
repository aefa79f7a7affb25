"""The team route of prune_conformers_rmsd_batch: mid-size ensembles pruned in one call, a team of workgroups each (csrc/prune_team.hpp).

Without a GPU: the exports, the argument checks of the Python layer and the routing of a mixed batch by size.  On the GPU: the CPU
oracle on ensembles whose sizes sit on both sides of the 64-column step, of the 64-row work item and of the schedule's gates, ensembles
whose gates close by count where their size alone would open them, the reference's own recorded runs (G3, G16a), and the properties a
batch must have (order, independence, tiny segments, non-finite input, the device form, the size cap, the three routes together).

Every oracle comparison first asserts that no pair the reference evaluates lies within 1e-6 of a threshold (oracle.prune_margins), as
tests/test_prune_batch.py does.  No case is skipped."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, load_large_prune
from test_prune_batch import HEAVY, MARGIN, draw_ensemble

STAT_KEYS = ("k", "n_active_before", "n_active_after", "pairs_evaluated", "new_keys")
ROWS = 16                  # PT_ROWS of csrc/prune_batch_plan.hpp: the rows of one work item, four items to a word of the masks
LISTED = [65, 127, 128, 129, 191, 193, 255, 257, 401, 419, 1003, 2049, 2500, 4099]
SIZES = LISTED + [4 * ROWS - 1, 4 * ROWS, 32 * ROWS - 1, 32 * ROWS, 32 * ROWS + 1, ROWS - 1, ROWS, ROWS + 1]       # (4 * ROWS + 1 = 65 is listed)
GATES = ((2711, 2100, 9, 5), (2712, 4100, 4, 7), (2713, 1100, 18, 3))         # (seed, n, h, parents)
GATE_SLOTS = {2711: ([100, 20, 10, 5, 2, 1], [100, 20, 2, 1]), 2712: ([200, 50, 20, 10, 5, 2, 1], [200, 50, 10, 2, 1]), 2713: ([50, 5, 2, 1], [50, 5, 1])}
GATE_KEPT = {2711: (369, 5), 2712: (168, 7), 2713: (65, 3)}

_edge, _edge_ref, _gate, _gate_ref = {}, {}, {}, {}


def edge_batch(seed):
    """SIZES in order, heavy counts HEAVY[(s * 3 + seed) % 7], all from one default_rng(seed)."""
    if seed not in _edge:
        rng = np.random.default_rng(seed)
        drawn = [draw_ensemble(rng, n, HEAVY[(s * 3 + seed) % 7]) for s, n in enumerate(SIZES)]
        _edge[seed] = ([d[0] for d in drawn], [d[1] for d in drawn])
    return _edge[seed]


def reference(oracle, cache, key, heavies, thrs, mode):
    """The oracle's run of every ensemble, computed once per key; the margin condition is asserted here for all of them."""
    if key not in cache:
        refs = []
        for s, (hv, thr) in enumerate(zip(heavies, thrs)):
            assert min(oracle.prune_margins(hv, thr, mode)) > MARGIN, (key, s)
            refs.append(oracle.prune_heavy(hv, thr, mode))
        cache[key] = refs
    return cache[key]


def edge_reference(oracle, seed, mode):
    return reference(oracle, _edge_ref, (seed, mode), *edge_batch(seed), mode)


def gate_batch():
    """Few parents, tight copies, thr 0.5: the count of the survivors falls below 20 k for slots that N alone would open."""
    if not _gate:
        heavies = []
        for seed, n, h, n_par in GATES:
            rng = np.random.default_rng(seed)
            parents = 3 * rng.normal(size=(n_par, h, 3))
            heavies.append(np.ascontiguousarray(parents[rng.integers(0, n_par, n)] + 0.01 * rng.normal(size=(n, h, 3))))
        _gate.update(heavies=heavies, thrs=[0.5] * len(GATES))
    return _gate["heavies"], _gate["thrs"]


def gate_reference(oracle, mode):
    return reference(oracle, _gate_ref, mode, *gate_batch(), mode)


def same_as(oracle_run, mask, stats, where):
    assert np.array_equal(mask, oracle_run["mask"]), where
    for key in STAT_KEYS:
        assert [p[key] for p in stats] == [p[key] for p in oracle_run["stats"]], (where, key)


def carbons(heavies):
    return [np.full(hv.shape[1], 6) for hv in heavies]


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


@pytest.fixture(scope="module")
def cap():
    from tscode_amd._lib import TSC_PRUNE_TEAM_MAX_N
    return TSC_PRUNE_TEAM_MAX_N


# ----------------------------------------------------------------------------- without a GPU
def test_header_and_library_export_the_team_entry_points():
    from tscode_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "tscode_hip.h")).read()
    cap = int(re.search(r"#define TSC_PRUNE_TEAM_MAX_N (\d+)", header).group(1))
    assert 65536 <= cap <= 200000 and cap == _lib.TSC_PRUNE_TEAM_MAX_N
    assert "prune_batch.hip" in build.SOURCES and "prune_team.hpp" in build.HEADERS and "prune_batch_plan.hpp" in build.HEADERS
    kernels = open(os.path.join(build.CSRC, "prune_batch_plan.hpp")).read()     # (the item table is made there)
    assert int(re.search(r"constexpr int PT_ROWS = (\d+);", kernels).group(1)) == ROWS, "the edge sizes of this file follow the work item's rows"
    build.build()
    lib = _lib.load()
    for name in ("tsc_prune_rmsd_team", "tsc_prune_rmsd_team_dev"):
        assert re.search(r"\bint " + name + r"\(", header) and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == len(_lib._SIGNATURES[name.replace("team", "batch")][1]) == 12


def test_team_max_n_is_refused_before_the_engine_is_asked_for(monkeypatch, cap):
    import tscode_amd.engine as engine
    import tscode_amd.rmsd_pruning as rp

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(rp, "get_engine", no_engine)
    c3 = np.array([6, 6, 1])
    good = [np.zeros((4, 3, 3)), np.zeros((2, 3, 3))]
    for bad in (-1, cap + 1, 2.5, "64", True):
        with pytest.raises(ValueError, match="team_max_n"):
            rp.prune_conformers_rmsd_batch(good, c3, team_max_n=bad)
    with pytest.raises(ValueError):
        rp.prune_conformers_rmsd_batch([np.zeros((4, 3, 3)), np.zeros((2, 4, 3))], c3, team_max_n=100)     # the checks of the batch call stay
    with pytest.raises(AssertionError, match="asked for"):
        rp.prune_conformers_rmsd_batch(good, c3, team_max_n=np.int64(cap))                                  # a legal value gets that far
    assert rp.prune_conformers_rmsd_batch([], c3, team_max_n=0) == []
    assert 0 <= engine.PRUNE_TEAM_MAX_N <= cap and engine.check_team_max_n(None) == engine.PRUNE_TEAM_MAX_N


class StubLib:
    """What Engine.prune_heavy_batch asks of the library, recorded: the sizes each entry point was handed."""

    def __init__(self, batch_max_n):
        self.batch_max_n, self.calls = batch_max_n, []

    def tsc_ctx_get_option(self, handle, name, value):
        assert name == b"prune_batch_max_n"
        value._obj.value = self.batch_max_n
        return 0

    def _entry(self, route, handle, heavy, offsets, n, h, thr, n_segments, mode, *outputs):
        self.calls.append((route, np.ctypeslib.as_array(n, (n_segments.value,)).tolist()))
        return 0

    def tsc_prune_rmsd_batch(self, *a):
        return self._entry("batch", *a)

    def tsc_prune_rmsd_team(self, *a):
        return self._entry("team", *a)


@pytest.mark.parametrize("team_max_n,expected", [(None, [("batch", [5, 10]), ("team", [30, 50]), ("single", [70]), ("single", [200])]),
                                                 (0, [("batch", [5, 10]), ("single", [30]), ("single", [70]), ("single", [50]), ("single", [200])]),
                                                 (100, [("batch", [5, 10]), ("team", [30, 70, 50]), ("single", [200])])])
def test_a_mixed_batch_is_routed_by_size(monkeypatch, team_max_n, expected):
    """Sizes 5, 30, 70, 10, 50, 200 under "prune_batch_max_n" = 10 and a module default of 50: at most one call of each batched entry,
    with the ensembles in the caller's order, and a call of its own for every longer ensemble."""
    import tscode_amd.engine as engine
    monkeypatch.setattr(engine, "PRUNE_TEAM_MAX_N", 50)
    eng = engine.Engine.__new__(engine.Engine)
    eng.lib, eng._h = StubLib(10), None

    def single(heavy, thr, mode):
        eng.lib.calls.append(("single", [len(heavy)]))
        return np.ones(len(heavy), dtype=bool), []
    eng.prune_heavy = single
    sizes = [5, 30, 70, 10, 50, 200]
    masks, stats, nonfinite = eng.prune_heavy_batch([np.zeros((n, 2, 3)) for n in sizes], 0.5, 0, team_max_n=team_max_n)
    assert eng.lib.calls == expected
    assert [len(m) for m in masks] == sizes and len(stats) == len(sizes) and nonfinite.shape == (len(sizes),)
    eng._h = None        # (nothing to destroy)


# ----------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", [2701, 2702])
def test_edge_sizes_against_the_oracle(eng, oracle, seed, mode):
    heavies, thrs = edge_batch(seed)
    refs = edge_reference(oracle, seed, mode)
    # precondition on the generator: both modes are really exercised -- the reference's cache changes the outcome of these ensembles
    other = edge_reference(oracle, seed, 1 - mode)
    changed = [not np.array_equal(x["mask"], y["mask"]) for x, y in zip(refs, other)]
    assert sum(changed[:len(LISTED)]) == {2701: 12, 2702: 14}[seed]
    masks, stats, nonfinite = eng.prune_heavy_team(heavies, thrs, mode)
    assert not nonfinite.any()
    for s, ref in enumerate(refs):
        same_as(ref, masks[s], stats[s], (s, len(heavies[s])))
    assert {p["k"] for st in stats for p in st} == {200, 100, 50, 20, 10, 5, 2, 1}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_gates_that_close_on_the_device(eng, oracle, mode):
    heavies, thrs = gate_batch()
    refs = gate_reference(oracle, mode)
    for (seed, n, _, _), ref in zip(GATES, refs):
        ks = [p["k"] for p in ref["stats"]]
        assert ks == GATE_SLOTS[seed][mode] and int(ref["mask"].sum()) == GATE_KEPT[seed][mode]
        assert [k for k in (200, 100, 50, 20, 10, 5, 2, 1) if 20 * k < n and k not in ks], "no slot that N alone would open is skipped by count"
    e_heavies, e_thrs = edge_batch(2701)
    e_refs = edge_reference(oracle, 2701, mode)
    picks = [9, 12]                                        # 419 and 2500 structures
    batch = [heavies[0], e_heavies[picks[0]], heavies[1], heavies[2], e_heavies[picks[1]]]
    t = [thrs[0], e_thrs[picks[0]], thrs[1], thrs[2], e_thrs[picks[1]]]
    want = [refs[0], e_refs[picks[0]], refs[1], refs[2], e_refs[picks[1]]]
    masks, stats, nonfinite = eng.prune_heavy_team(batch, t, mode)
    assert not nonfinite.any()
    for s, ref in enumerate(want):
        same_as(ref, masks[s], stats[s], (s, len(batch[s])))


@pytest.mark.gpu
def test_reference_runs_of_g3_through_the_team_route(eng, cap):
    """G3: the reference's own six runs (N = 40 .. 2500, a remainder chunk at 1003).  Under "prune_batch_max_n" = 64 the five longer ones
    take the team route, under 1 all six."""
    import tscode_amd
    g = load_golden("G3_prune")
    cases = range(int(g["n_cases"]))
    structures, atomnos = [g[f"structures{c}"] for c in cases], [g[f"atomnos{c}"] for c in cases]
    thrs = [float(g[f"thr{c}"]) for c in cases]
    assert sorted(len(s) for s in structures) == [40, 600, 600, 720, 1003, 2500]
    results = []
    for max_n in (64, 1):
        with eng.options(prune_batch_max_n=max_n):
            out = tscode_amd.prune_conformers_rmsd_batch(structures, atomnos, thrs, team_max_n=cap)
            stats = tscode_amd.last_prune_batch_stats()
            for c in cases:
                assert np.array_equal(out[c][1], g[f"mask{c}"]), (max_n, c)
                assert np.array_equal(out[c][0], structures[c][g[f"mask{c}"]])
                assert [p["k"] for p in stats[c]] == g[f"ks{c}"].tolist(), (max_n, c)
                assert [p["n_active_after"] for p in stats[c]] == g[f"pass_masks{c}"].sum(axis=1).tolist(), (max_n, c)
                assert np.cumsum([p["new_keys"] for p in stats[c]]).tolist() == g[f"pass_nkeys{c}"].tolist(), (max_n, c)
            results.append(([m for _, m in out], stats))
    with eng.options(prune_batch_max_n=64):
        out = tscode_amd.prune_conformers_rmsd_batch(structures, atomnos, thrs, team_max_n=0)       # the batch kernel and the single calls
        results.append(([m for _, m in out], tscode_amd.last_prune_batch_stats()))
    for masks, stats in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(masks, results[0][0]))
        assert stats == results[0][1]                                                               # (pairs_evaluated among them)


@pytest.mark.gpu
def test_reference_run_of_g16a_through_the_team_route(eng):
    """G16a: the reference's own run on 40 023 structures (passes k = 2000 .. 1 and their cache-key collisions), one segment of 626 items."""
    fx = load_large_prune("G16a")
    g = fx.g
    assert fx.n == 40023
    (mask,), (stats,), nonfinite = eng.prune_heavy_team([fx.heavy], fx.thr, 0)
    assert not nonfinite.any()
    assert np.array_equal(np.packbits(mask), g["mask_bits"]), (int(mask.sum()), int(np.unpackbits(g["mask_bits"])[:fx.n].sum()))
    assert [s["k"] for s in stats] == g["ks"].tolist()
    assert [s["n_active_after"] for s in stats] == [int(np.unpackbits(b)[:fx.n].sum()) for b in g["pass_mask_bits"]]
    assert np.cumsum([s["new_keys"] for s in stats]).tolist() == g["pass_nkeys"].tolist()


@pytest.mark.gpu
def test_ensembles_of_a_batch_are_independent(eng, oracle):
    heavies, thrs = edge_batch(2701)
    refs = edge_reference(oracle, 2701, 0)
    masks, stats, _ = eng.prune_heavy_team(heavies, thrs, 0)
    r_masks, r_stats, _ = eng.prune_heavy_team(heavies[::-1], thrs[::-1], 0)
    assert all(np.array_equal(a, b) for a, b in zip(r_masks[::-1], masks)) and r_stats[::-1] == stats
    for s in (0, 8, 11, 13, 14):
        m1, s1, _ = eng.prune_heavy_team([heavies[s]], [thrs[s]], 0)
        assert np.array_equal(m1[0], masks[s]) and s1[0] == stats[s]
    # an empty ensemble, a single structure and a pair among others
    two = np.stack([heavies[3][0], heavies[3][0] + 1e-3])
    mixed = [np.zeros((0, 7, 3)), heavies[8], np.ones((1, 2, 3)), two, np.zeros((0, 1, 3)), two[:, :, ::-1] * np.array([1.0, 50.0])[:, None, None]]
    m, st, nf = eng.prune_heavy_team(mixed, [0.5, thrs[8], 0.5, 0.5, 0.25, 0.5], 0)
    assert m[0].shape == (0,) and m[0].dtype == bool and st[0] == [] and m[4].shape == (0,) and st[4] == []
    same_as(refs[8], m[1], st[1], "among tiny ones")
    assert m[2].tolist() == [True] and [p["k"] for p in st[2]] == [1] and st[2][0]["pairs_evaluated"] == 0
    assert m[3].tolist() == [False, True] and st[3] == [dict(k=1, n_active_before=2, n_active_after=1, pairs_evaluated=1, new_keys=1)]
    assert m[5].tolist() == [True, True] and st[5] == [dict(k=1, n_active_before=2, n_active_after=2, pairs_evaluated=1, new_keys=0)]
    for s in (3, 5):
        assert min(oracle.prune_margins(mixed[s], 0.5, 0)) > MARGIN
        same_as(oracle.prune_heavy(mixed[s], 0.5, 0), m[s], st[s], s)
    assert not nf.any()
    assert eng.prune_heavy_team([], 0.5, 0)[0] == []


@pytest.mark.gpu
def test_nonfinite_input_is_flagged_on_its_ensemble_only(eng, oracle, cap):
    import tscode_amd
    heavies, thrs = edge_batch(2701)
    refs = edge_reference(oracle, 2701, 0)
    picks = [4, 7, 9]                                      # 191, 257 and 419 structures
    batch = [heavies[s].copy() for s in picks]
    batch[1][150, 2, 1] = np.nan
    t = [thrs[s] for s in picks]
    masks, _, nonfinite = eng.prune_heavy_team(batch, t, 0)
    assert nonfinite.tolist() == [False, True, False]
    assert np.array_equal(masks[0], refs[4]["mask"]) and np.array_equal(masks[2], refs[9]["mask"])
    assert masks[1][150]                                   # similar to nothing: kept
    with eng.options(prune_batch_max_n=100):
        with pytest.raises(np.linalg.LinAlgError, match="ensemble 1"):
            tscode_amd.prune_conformers_rmsd_batch(batch, carbons(batch), t, team_max_n=cap)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_device_array_form_equals_the_host_form(eng, mode, cap):
    """tsc_prune_rmsd_team_dev on torch tensors: heavy atoms and every output on the device, the tables on the host."""
    import torch
    from tscode_amd import pack_heavy_batch
    from tscode_amd._lib import TSC_MAX_PASSES, TscodeHipError
    heavies, thrs = edge_batch(2702)
    heavies, thrs = heavies[:12][::-1] + [np.zeros((0, 4, 3))], thrs[:12][::-1] + [0.5]      # (2049 structures first, an empty one last)
    masks, stats, _ = eng.prune_heavy_team(heavies, thrs, mode)
    flat, offsets, n, h = pack_heavy_batch(heavies)
    S = len(heavies)
    dev = torch.device("cuda", eng.device)
    d_heavy = torch.from_numpy(flat).to(dev)
    d_mask = torch.full((int(n.sum()),), 7, dtype=torch.uint8, device=dev)
    d_stats = torch.full((S, TSC_MAX_PASSES, 5), -1, dtype=torch.int64, device=dev)
    d_np = torch.full((S,), -1, dtype=torch.int32, device=dev)
    d_nf = torch.full((S,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    eng.prune_heavy_team_dev(d_heavy, offsets, n, h, thrs, mode, d_mask, d_stats, d_np, d_nf)
    assert np.array_equal(d_mask.cpu().numpy().astype(bool), np.concatenate(masks))
    assert d_np.cpu().tolist() == [len(st) for st in stats] and not d_nf.cpu().any()
    table = d_stats.cpu().numpy()
    for s, st in enumerate(stats):
        assert table[s, :len(st)].tolist() == [[p[key] for key in STAT_KEYS] for p in st], s
        assert not table[s, len(st):].any()
    # the optional outputs left out
    d_mask.fill_(7)
    eng.prune_heavy_team_dev(d_heavy, offsets, n, h, thrs, mode, d_mask)
    assert np.array_equal(d_mask.cpu().numpy().astype(bool), np.concatenate(masks))
    # what is refused is refused with the segment named and nothing written: a segment above the cap (only the tables say so), no heavy
    # atoms, an offset table that does not fit, a threshold that is not finite; and a bad mode
    d_mask.fill_(7)
    n2, h2 = np.array([3, cap + 1, 2], dtype=np.int32), np.array([1, 1, 1], dtype=np.int32)
    off2 = np.concatenate([[0], np.cumsum(n2.astype(np.int64) * h2 * 3)])
    with pytest.raises(TscodeHipError, match=f"segment 1 has {cap + 1} structures"):
        eng.prune_heavy_team_dev(d_heavy, off2, n2, h2, 0.5, mode, d_mask)
    with pytest.raises(TscodeHipError, match="segment 2 has 0 heavy atoms"):
        eng.prune_heavy_team_dev(d_heavy, offsets, n, np.where(np.arange(S) == 2, 0, h), thrs, mode, d_mask)
    with pytest.raises(TscodeHipError, match=r"offsets\[3\]"):
        eng.prune_heavy_team_dev(d_heavy, np.where(np.arange(S + 1) == 4, offsets + 3, offsets), n, h, thrs, mode, d_mask)
    with pytest.raises(TscodeHipError, match=r"thr\[5\]"):
        eng.prune_heavy_team_dev(d_heavy, offsets, n, h, np.where(np.arange(S) == 5, np.inf, thrs), mode, d_mask)
    with pytest.raises(TscodeHipError, match="mode 2"):
        eng.prune_heavy_team_dev(d_heavy, offsets, n, h, thrs, 2, d_mask)
    assert (d_mask.cpu().numpy() == 7).all()
    with pytest.raises(TscodeHipError, match=f"segment 0 has {cap + 1} structures"):
        eng.prune_heavy_team([np.zeros((cap + 1, 1, 3))], 0.5, mode)


@pytest.mark.gpu
def test_three_routes_in_one_call_give_what_the_single_calls_give(eng, oracle):
    """65 / 257 / 1003 / 129 / 401 structures under "prune_batch_max_n" = 128: the default routing, no team route, and a team route up
    to 512 structures (the batch kernel, the team route and a call of its own for the 1003), beside prune_conformers_rmsd on each."""
    import tscode_amd
    heavies, thrs = edge_batch(2702)
    picks = [0, 7, 10, 3, 8]
    batch, t = [heavies[s] for s in picks], [thrs[s] for s in picks]
    refs = edge_reference(oracle, 2702, 0)
    results = []
    with eng.options(prune_batch_max_n=128):
        for team_max_n in (None, 0, 512):
            out = tscode_amd.prune_conformers_rmsd_batch(batch, carbons(batch), t, team_max_n=team_max_n)
            results.append(([m for _, m in out], tscode_amd.last_prune_batch_stats()))
    for masks, stats in results:
        for b, s in enumerate(picks):
            same_as(refs[s], masks[b], stats[b], (b, s))
    for b, (hv, thr) in enumerate(zip(batch, t)):
        _, single = tscode_amd.prune_conformers_rmsd(hv, np.full(hv.shape[1], 6), thr)
        assert np.array_equal(results[0][0][b], single), b
