"""A cyclical embed whose kept poses are pruned by RMSD without leaving the device (include/tscode_hip.h: tsc_embed_prune_*;
tscode_amd.cyclical_embed_prune_batch) against the two calls it stands for -- ``cyclical_embed_batch`` then ``prune_conformers_rmsd`` -- and
against the oracle's loops.  The new call is never its own yardstick: flags, verdicts and statistics must be equal, poses equal to the last bit.

The synthetic molecules (``noisy_mols``) have conformers that are copies with 0.01 A of noise and share their pivots, so the poses of different
conformer groups come out as near duplicates: the embed's per-group filter keeps them, the prune must remove them.  Every comparison with the
oracle first shows its guard bands: no candidate within 1e-9 of the clash threshold, no pair within 1e-6 of either prune threshold."""

import ctypes as C

import numpy as np
import pytest

import trimolecular_cases as tc
from conftest import load_golden

gpu = pytest.mark.gpu

TSC_ERR_INVALID, TSC_ERR_STATE = -1, -5
THRESH, RMSD_THR = 0.5, 0.5
STEPS = np.array([-40.0, 0.0, 40.0])


def noisy_mols(seed, n_atoms, n_conf, n_pivots, lengths, sigma=0.01):
    rng = np.random.default_rng(seed); mols, off = [], 0
    for m, n in enumerate(n_atoms):
        base = rng.normal(size=(n, 3)) * 2.0
        coords = np.stack([base + (0 if c == 0 else rng.normal(size=(n, 3)) * sigma) for c in range(n_conf[m])])
        reactive = np.sort(rng.choice(n, size=2, replace=False))
        vec = rng.normal(size=(n_pivots[m], 3)); vec *= (rng.uniform(*lengths, size=n_pivots[m]) / np.linalg.norm(vec, axis=1))[:, None]
        mean = base[reactive].mean(axis=0) + rng.normal(size=(n_pivots[m], 3))
        ends = np.array([[reactive[0], reactive[1]] if q % 2 == 0 else [reactive[1], reactive[0]] for q in range(n_pivots[m])])
        mols.append(dict(coords=coords, reactive_indices=reactive, pivots=[(vec.copy(), mean.copy(), ends + off)] * n_conf[m],
                         reactive_cumnums=np.array([[i, i + off] for i in reactive], dtype=np.int64))); off += n
    return mols


def atomnos_for(n_total):
    return np.where(np.arange(n_total) % 5 < 3, 6, 1)


def angle_sets(n_mols):
    from tscode_amd.utils import cartesian_product
    return np.ascontiguousarray(cartesian_product(*[STEPS] * n_mols), dtype=np.float64)


CASES = {
    "two": dict(mols=lambda: noisy_mols(1, (20, 24), (3, 2), (2, 2), (2.0, 3.5))),
    "three": dict(mols=lambda: noisy_mols(12, (12, 14, 16), (2, 2, 1), (1, 1, 1), (2.0, 3.0))),
}


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


_yard = {}


def yardstick(name, oracle):
    """Per case, computed once and left unchanged: the molecules, the oracle's loop (candidates, flags, the prune's mask per mode, its guard
    bands) and the two-call route on the GPU (trace, poses, and per mode the prune's mask, poses and statistics)."""
    if name in _yard:
        return _yard[name]
    import types

    import tscode_amd
    mols = CASES[name]["mols"]()
    n_mols = len(mols)
    angles = angle_sets(n_mols)
    sizes = [m["coords"].shape[1] for m in mols]
    atomnos = atomnos_for(sum(sizes))
    coords, reactive, pivots, cumnums = tc.unpack(mols)
    if n_mols == 3:
        cands, group_of, ok, kept, _ = oracle.cyclical_embed3(coords, reactive, pivots, cumnums, angles, THRESH)
    else:
        cands, group_of, ok, kept, _ = oracle.cyclical_embed(coords, reactive, pivots, angles, THRESH)
    ok, kept = np.asarray(ok, dtype=bool), np.asarray(kept, dtype=bool)
    y = types.SimpleNamespace(mols=mols, angles=angles, atomnos=atomnos, n_total=sum(sizes), orc_ok=ok, orc_kept=kept, orc_mask={}, margins={}, gpu={},
                              clash_margin=oracle.clash_margin(cands, sizes, THRESH))
    heavy = np.ascontiguousarray(cands[kept][:, atomnos != 1])
    for mode in (0, 1):
        y.orc_mask[mode] = np.asarray(oracle.prune_conformers_rmsd(cands[kept], atomnos, RMSD_THR, mode)[1], dtype=bool)
        y.margins[mode] = oracle.prune_margins(heavy, RMSD_THR, mode)
    y.poses, y.cons, y.trace = tscode_amd.cyclical_embed_batch(mols, angles, clash_thresh=THRESH, return_trace=True)
    for mode in (0, 1):
        out, mask = tscode_amd.prune_conformers_rmsd(y.poses, atomnos, RMSD_THR, mode)
        y.gpu[mode] = (out, mask, tscode_amd.last_prune_stats())
    _yard[name] = y
    return y


def same_passes(got, want):
    """Pass by pass: the k, the active counts and the reference's pair evaluations."""
    pick = lambda stats: [(s["k"], s["n_active_before"], s["n_active_after"], s["pairs_evaluated"]) for s in stats]
    return pick(got) == pick(want)


@gpu
@pytest.mark.parametrize("name", ["two", "three"])
def test_counts_and_guard_bands_against_the_oracle(eng, oracle, name):
    """Candidates, candidates that pass the clash check, poses kept and poses that survive the prune: the new call against the oracle's loops,
    with the oracle's own margins in front (the verdicts compared lie clear of every threshold)."""
    import tscode_amd
    y = yardstick(name, oracle)
    if name == "three":
        assert tc.host_groups(y.mols)[4].min() >= tc.GAP_BAND
    assert y.clash_margin > 1e-9
    assert min(y.margins[0]) > 1e-6 and min(y.margins[1]) > 1e-6
    poses, cons, tr = tscode_amd.cyclical_embed_prune_batch(y.mols, y.angles, y.atomnos, RMSD_THR, clash_thresh=THRESH, return_trace=True)
    got = (len(tr.clash_ok), int(tr.clash_ok.sum()), int(tr.kept.sum()), int(tr.survived.sum()))
    want = (len(y.orc_ok), int(y.orc_ok.sum()), int(y.orc_kept.sum()), int(y.orc_mask[0].sum()))
    print(f"{name}: candidates / pass / kept / survive: GPU {got}, oracle {want}; prune margins {y.margins[0]}, clash margin {y.clash_margin:.3g}")
    assert got == want
    assert 0 < got[3] < got[2] < got[0]
    assert np.array_equal(tr.clash_ok, y.orc_ok) and np.array_equal(tr.kept, y.orc_kept) and len(poses) == got[3]


@gpu
@pytest.mark.parametrize("slab", ["whole", "slabs"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["two", "three"])
def test_equals_the_two_calls(eng, oracle, name, mode, slab):
    import tscode_amd
    y = yardstick(name, oracle)
    max_poses = 1 << 20 if slab == "whole" else 5 * len(y.angles)
    poses, cons, tr = tscode_amd.cyclical_embed_prune_batch(y.mols, y.angles, y.atomnos, RMSD_THR, mode, clash_thresh=THRESH, return_trace=True,
                                                            max_poses_per_call=max_poses)
    out, mask, stats = y.gpu[mode]
    assert np.array_equal(tr.survived, y.orc_mask[mode]) and np.array_equal(tr.survived, mask)
    assert np.array_equal(tr.clash_ok, y.trace.clash_ok) and np.array_equal(tr.kept, y.trace.kept) and np.array_equal(tr.group_of, y.trace.group_of)
    assert tr.groups == y.trace.groups
    assert np.array_equal(cons, y.cons[mask]) and cons.shape[1:] == (len(y.mols), 2)
    assert poses.shape == out.shape and poses.dtype == out.dtype and poses.tobytes() == out.tobytes()
    assert same_passes(tr.prune_stats, stats) and len(stats) >= 1
    # every kept pose, embedded again from its parameters: what cyclical_embed_batch returned, to the last bit
    run, _, kept = run_object(eng, y.mols, y.angles, y.atomnos, max_poses)
    try:
        assert np.array_equal(kept, y.trace.kept) and run.count() == len(y.poses)
        assert run.poses(1).tobytes() == y.poses.tobytes()
    finally:
        run.close()


def group_records(mols, pairings=None):
    """(coords, blocks, group_ids) as the drivers build them."""
    from tscode_amd import embeds as E
    coords = [np.ascontiguousarray(m["coords"], dtype=np.float64) for m in mols]
    if len(mols) == 3:
        g = E.trimolecular_groups_batch(mols, pairings, ())
        return coords, g.blocks, g.group_ids
    reactive = [np.atleast_1d(np.asarray(m["reactive_indices"], dtype=np.int64)) for m in mols]
    blocks, group_ids, _ = E._bimolecular_groups(coords, reactive, [m["pivots"] for m in mols], True, 5, pairings, (), False)
    return coords, blocks, group_ids


def slab_args(blocks, lo, hi, angles):
    b = blocks[lo:hi]
    return [np.ascontiguousarray(b[:, :, f:f + 3]) for f in range(0, 21, 3)] + [b[:, :, 21].astype(np.int32), b[:, :, 22].astype(np.int32), angles]


def run_object(eng, mols, angles, atomnos, max_poses, thresh=THRESH):
    """An EmbedPruneRun fed slab by slab, not yet pruned: (run, clash_ok, kept)."""
    from tscode_amd import embeds as E
    from tscode_amd.engine import FragmentSet
    coords, blocks, _ = group_records(mols)
    run = eng.embed_prune_run(FragmentSet(coords), np.flatnonzero(atomnos != 1))
    oks, kepts = [], []
    for lo, hi in E._slabs(len(blocks), len(angles), max_poses):
        ok, kept = run.add_groups(*slab_args(blocks, lo, hi, angles), thresh, 0, 1.0)
        oks.append(ok), kepts.append(kept)
    return run, np.concatenate(oks), np.concatenate(kepts)


def golden_cases():
    g12, g18 = load_golden("G12_cyclical_embed"), load_golden("G18_cyclical_embed_trimolecular")
    for k in range(int(g12["n_cases"])):
        coords = [g12[f"coords{m}_{k}"] for m in range(2)]
        mols = [dict(coords=coords[m], reactive_indices=g12[f"reactive_indices{m}_{k}"],
                     pivots=[(g12[f"pivot_vec{m}_{c}_{k}"], g12[f"pivot_mean{m}_{c}_{k}"], g12[f"pivot_cumnums{m}_{c}_{k}"]) for c in range(len(coords[m]))])
                for m in range(2)]
        yield f"G12[{k}]", mols, g12[f"angles_{k}"], dict(clash_thresh=float(g12[f"clash_thresh_{k}"]), rigid_shortcut=bool(g12[f"rigid_{k}"]))
    for k in range(int(g18["n_cases"])):
        yield f"G18[{k}]", tc.g18_case(k)[1], g18[f"angles_{k}"], dict(clash_thresh=float(g18[f"clash_thresh_{k}"]))


@gpu
def test_recorded_embeds_agree_with_the_two_calls(eng):
    """Fixtures G12 (every case) and G18 (all three): however few poses they keep, the new route and the old agree on the project's recorded embeds."""
    import tscode_amd
    seen = []
    for label, mols, angles, kw in golden_cases():
        atomnos = atomnos_for(sum(np.asarray(m["coords"]).shape[1] for m in mols))
        p, c, tr0 = tscode_amd.cyclical_embed_batch(mols, angles, return_trace=True, **kw)
        for mode in (0, 1):
            out, mask = tscode_amd.prune_conformers_rmsd(p, atomnos, RMSD_THR, mode)
            stats = tscode_amd.last_prune_stats() if len(p) else []
            poses, cons, tr = tscode_amd.cyclical_embed_prune_batch(mols, angles, atomnos, RMSD_THR, mode, return_trace=True, **kw)
            assert np.array_equal(tr.clash_ok, tr0.clash_ok) and np.array_equal(tr.kept, tr0.kept) and np.array_equal(tr.group_of, tr0.group_of), label
            assert np.array_equal(tr.survived, mask) and np.array_equal(cons, c[mask]), label
            assert poses.shape == out.shape and poses.tobytes() == np.ascontiguousarray(out).tobytes(), label
            assert same_passes(tr.prune_stats, stats), label
        seen.append((label, len(p), int(mask.sum())))
    print("kept / survived per recorded case:", seen)
    assert len(seen) >= 4 and sum(label.startswith("G18") for label, _, _ in seen) == 3


@gpu
def test_nothing_passes_the_clash_check(eng, oracle):
    import tscode_amd
    y = yardstick("two", oracle)
    poses, cons, tr = tscode_amd.cyclical_embed_prune_batch(y.mols, y.angles, y.atomnos, RMSD_THR, clash_thresh=50, return_trace=True)
    assert poses.shape == (0, y.n_total, 3) and cons.shape == (0, 2, 2) and tr.survived.shape == (0,) and tr.prune_stats == []
    assert len(tr.clash_ok) == len(y.orc_ok) and not tr.clash_ok.any() and not tr.kept.any()
    run, ok, kept = run_object(eng, y.mols, y.angles, y.atomnos, 1 << 20, thresh=50)
    try:
        assert run.count() == 0 and run.poses(1).shape == (0, y.n_total, 3)
        survived, stats = run.run(RMSD_THR, 0)                                       # (launches nothing: no pass is reported)
        assert survived.shape == (0,) and stats == [] and run.n_survived == 0 and run.poses(0).shape == (0, y.n_total, 3)
    finally:
        run.close()


@gpu
@pytest.mark.parametrize("name", ["two", "three"])
def test_one_group_that_keeps_one_pose(eng, oracle, name):
    """A single group under a single angle set, nothing clashing (a threshold of 0 is never undercut): one candidate, one kept pose, which
    survives a prune that has nothing to compare it with."""
    from tscode_amd.engine import FragmentSet
    y = yardstick(name, oracle)
    coords, blocks, _ = group_records(y.mols)
    args = slab_args(blocks, 0, 1, y.angles[1:2])
    ok0, kept0, pose0 = eng.cyclical_embed_groups(FragmentSet(coords), *args, 0.0, 0, 1.0)
    assert ok0.tolist() == [True] and kept0.tolist() == [True] and pose0.shape == (1, y.n_total, 3)
    run = eng.embed_prune_run(FragmentSet(coords), np.flatnonzero(y.atomnos != 1))
    try:
        ok, kept = run.add_groups(*args, 0.0, 0, 1.0)
        assert ok.tolist() == [True] and kept.tolist() == [True] and run.count() == 1
        survived, stats = run.run(RMSD_THR, 0)
        assert survived.tolist() == [True] and run.n_survived == 1
        assert run.poses(0).tobytes() == pose0.tobytes() and run.poses(1).tobytes() == pose0.tobytes()
    finally:
        run.close()


@gpu
@pytest.mark.parametrize("name", ["two", "three"])
def test_a_slab_that_keeps_nothing_between_two_that_do(eng, oracle, name):
    import tscode_amd
    from tscode_amd.engine import FragmentSet
    y = yardstick(name, oracle)
    coords, blocks, _ = group_records(y.mols)
    G = len(blocks)
    cuts = [(0, G // 3, THRESH), (G // 3, 2 * G // 3, 50.0), (2 * G // 3, G, THRESH)]
    frags = FragmentSet(coords)
    want = [eng.cyclical_embed_groups(frags, *slab_args(blocks, lo, hi, y.angles), thr, 0, 1.0) for lo, hi, thr in cuts]
    assert want[0][1].any() and not want[1][1].any() and want[2][1].any()
    all_poses = np.concatenate([w[2] for w in want])
    run = eng.embed_prune_run(frags, np.flatnonzero(y.atomnos != 1))
    try:
        for (lo, hi, thr), w in zip(cuts, want):
            ok, kept = run.add_groups(*slab_args(blocks, lo, hi, y.angles), thr, 0, 1.0)
            assert np.array_equal(ok, w[0]) and np.array_equal(kept, w[1])
        assert run.count() == len(all_poses) and run.poses(1).tobytes() == all_poses.tobytes()
        out, mask = tscode_amd.prune_conformers_rmsd(all_poses, y.atomnos, RMSD_THR, 0)
        stats = tscode_amd.last_prune_stats()
        survived, got_stats = run.run(RMSD_THR, 0)
        assert np.array_equal(survived, mask) and 0 < mask.sum() < len(mask) and same_passes(got_stats, stats)
        assert run.poses(0).tobytes() == np.ascontiguousarray(out).tobytes()
    finally:
        run.close()


@gpu
def test_the_buffers_grow_over_many_slabs(eng, oracle):
    """More kept poses than the run's first allocation holds (1024 rows), a few groups at a time: the buffers double under the rows already
    there.  Against one tsc_cyclical_embed_groups call over all groups."""
    from tscode_amd.engine import FragmentSet
    mols = noisy_mols(3, (9, 8), (6, 5), (2, 2), (2.0, 3.5))
    angles = angle_sets(2)
    coords, blocks, _ = group_records(mols)
    frags, atomnos = FragmentSet(coords), atomnos_for(17)
    ok0, kept0, poses0 = eng.cyclical_embed_groups(frags, *slab_args(blocks, 0, len(blocks), angles), 0.0, 0, 1e-3)
    assert len(poses0) > 1024 and len(poses0) == kept0.sum()                          # (0.001 A: the filter keeps every pose of a group)
    run = eng.embed_prune_run(frags, np.flatnonzero(atomnos != 1))
    try:
        per = 7
        kept = np.concatenate([run.add_groups(*slab_args(blocks, lo, min(lo + per, len(blocks)), angles), 0.0, 0, 1e-3)[1]
                               for lo in range(0, len(blocks), per)])
        assert np.array_equal(kept, kept0) and run.count() == len(poses0)
        assert run.poses(1).tobytes() == poses0.tobytes()
    finally:
        run.close()


@gpu
def test_python_argument_checks():
    import tscode_amd
    mols = CASES["two"]["mols"]()
    angles = angle_sets(2)
    with pytest.raises(ValueError, match="one entry per atom"):
        tscode_amd.cyclical_embed_prune_batch(mols, angles, np.full(43, 6))
    with pytest.raises(ValueError, match="not hydrogen"):
        tscode_amd.cyclical_embed_prune_batch(mols, angles, np.ones(44, dtype=int))
    with pytest.raises(ValueError, match="two or three"):
        tscode_amd.cyclical_embed_prune_batch(mols[:1], angles, np.full(20, 6))
    with pytest.raises(ValueError, match="max_poses_per_call"):
        tscode_amd.cyclical_embed_prune_batch(mols, angles, atomnos_for(44), max_poses_per_call=0)


# ---- the C ABI's refusals and lifetimes, through ctypes


def _abi(eng, oracle):
    """(lib, last_error, create(heavy_idx, n_heavy=None, frags=...), add(run, thresh=...), a good call) on the two-molecule case."""
    from tscode_amd.engine import FragmentSet
    y = yardstick("two", oracle)
    coords, blocks, _ = group_records(y.mols)
    frags = FragmentSet(coords)
    lib = eng.lib
    err = lambda: lib.tsc_last_error().decode()
    args = slab_args(blocks, 0, 2, y.angles)
    arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in args[:7]]
    n_reactive, conf_idx = np.ascontiguousarray(args[7]).ravel(), np.ascontiguousarray(args[8]).ravel()
    A, N = len(y.angles), 2 * len(y.angles)
    p = lambda a: C.c_void_p(a.ctypes.data)
    i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    want = eng.cyclical_embed_groups(frags, *args, THRESH, 0, 1.0)

    def create(ctx, heavy_idx, n_heavy=None, null_frags=False):
        heavy_idx = np.ascontiguousarray(heavy_idx, dtype=np.int32)
        run = C.c_void_p()
        rc = lib.tsc_embed_prune_create(ctx, None if null_frags else p(frags.flat), *frags.table_args(), i32p(heavy_idx),
                                        C.c_int(len(heavy_idx) if n_heavy is None else n_heavy), C.byref(run))
        return rc, run

    def add(run, null=None):
        ok, kept = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        n_pass, n_kept = C.c_int64(-1), C.c_int64(-1)
        ptrs = [p(a) for a in arrs] + [p(n_reactive), p(conf_idx), p(y.angles)]
        if null is not None:
            ptrs[null] = None
        rc = lib.tsc_embed_prune_add_groups(run, *ptrs, C.c_int64(2), C.c_int(A), C.c_double(THRESH), C.c_int64(0), C.c_double(1.0), p(ok), p(kept),
                                            C.byref(n_pass), C.byref(n_kept))
        return rc, ok.astype(bool), kept.astype(bool), n_pass.value, n_kept.value

    def good(ctx):
        """One whole good sequence on a fresh run: the context still serves."""
        rc, run = create(ctx, np.flatnonzero(y.atomnos != 1))
        assert rc == 0, err()
        rc, ok, kept, n_pass, n_kept = add(run)
        assert rc == 0 and np.array_equal(ok, want[0]) and np.array_equal(kept, want[1]) and (n_pass, n_kept) == (want[0].sum(), want[1].sum()), err()
        out = np.empty((n_kept, y.n_total, 3))
        assert lib.tsc_embed_prune_poses(run, 1, p(out), C.c_int64(n_kept)) == 0 and out.tobytes() == want[2].tobytes()
        assert lib.tsc_embed_prune_destroy(run) == 0
    return y, lib, err, create, add, good, want


@gpu
def test_refusals(eng, oracle):
    """Every state rule of include/tscode_hip.h: the status, the message, and a good call after each."""
    y, lib, err, create, add, good, want = _abi(eng, oracle)
    ctx = eng._h
    heavy = np.flatnonzero(y.atomnos != 1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    n_kept = int(want[1].sum())
    assert n_kept >= 2
    # create: n_heavy < 1, an index out of range, indices that do not increase, a null pointer
    for kw, text in ((dict(heavy_idx=heavy, n_heavy=0), "0 heavy atoms"), (dict(heavy_idx=[0, 3, y.n_total]), f"heavy_idx[2] = {y.n_total} is not an atom"),
                     (dict(heavy_idx=[-1, 3]), "heavy_idx[0] = -1 is not an atom"), (dict(heavy_idx=[0, 5, 5, 7]), "heavy_idx[2] = 5 does not increase"),
                     (dict(heavy_idx=[4, 2]), "heavy_idx[1] = 2 does not increase"), (dict(heavy_idx=heavy, null_frags=True), "tsc_embed_prune_create: null argument")):
        rc, run = create(ctx, **kw)
        assert rc == TSC_ERR_INVALID and text in err() and not run.value, (kw, rc, err())
        good(ctx)
    assert lib.tsc_embed_prune_create(ctx, p(np.zeros(3)), None, None, None, 2, None, 1, None) == TSC_ERR_INVALID and "null argument" in err()
    good(ctx)
    rc, run = create(ctx, heavy)
    assert rc == 0
    try:
        # add_groups: a null pointer; the checks and messages of tsc_cyclical_embed_groups
        rc = add(run, null=3)[0]
        assert rc == TSC_ERR_INVALID and "tsc_embed_prune_add_groups: null argument" in err()
        good(ctx)
        assert lib.tsc_embed_prune_add_groups(None, *[None] * 10, 2, 9, 0.5, 0, 1.0, None, None, None, None) == TSC_ERR_INVALID and "null argument" in err()
        good(ctx)
        # poses: the survivors before the prune has run; a null pointer; a capacity below the row count
        out = np.empty((n_kept, y.n_total, 3))
        assert lib.tsc_embed_prune_poses(run, 0, p(out), C.c_int64(n_kept)) == TSC_ERR_STATE and "once tsc_embed_prune_run has run" in err()
        good(ctx)
        assert add(run)[0] == 0 and lib.tsc_embed_prune_poses(run, 1, None, C.c_int64(n_kept)) == TSC_ERR_INVALID and "null argument" in err()
        good(ctx)
        assert lib.tsc_embed_prune_poses(run, 1, p(out), C.c_int64(n_kept - 1)) == TSC_ERR_INVALID
        assert f"poses holds {n_kept - 1} rows, {n_kept} are asked for" in err()
        good(ctx)
        assert lib.tsc_embed_prune_poses(run, 2, p(out), C.c_int64(n_kept)) == TSC_ERR_INVALID and "which = 2" in err()
        # run: null pointers, a mode that does not exist
        survived = np.zeros(n_kept, np.uint8)
        ns = C.c_int64()
        assert lib.tsc_embed_prune_run(run, 0.5, 0, p(survived), None, None, None) == TSC_ERR_INVALID and "tsc_embed_prune_run: null argument" in err()
        good(ctx)
        assert lib.tsc_embed_prune_run(run, 0.5, 0, None, None, None, C.byref(ns)) == TSC_ERR_INVALID and "null argument" in err()
        good(ctx)
        assert lib.tsc_embed_prune_run(run, 0.5, 2, p(survived), None, None, C.byref(ns)) == TSC_ERR_INVALID and "mode 2" in err()
        good(ctx)
        # none of the refusals above closed the run or touched its rows
        assert lib.tsc_embed_prune_poses(run, 1, p(out), C.c_int64(n_kept)) == 0 and out.tobytes() == want[2].tobytes()
        assert lib.tsc_embed_prune_run(run, 0.5, 0, p(survived), None, None, C.byref(ns)) == 0 and ns.value == survived.sum() > 0
        # add_groups after the prune
        rc = add(run)[0]
        assert rc == TSC_ERR_STATE and "the run has been pruned" in err()
        good(ctx)
        n = C.c_int64()
        assert lib.tsc_embed_prune_count(run, C.byref(n)) == 0 and n.value == n_kept
        assert lib.tsc_embed_prune_count(run, None) == TSC_ERR_INVALID and lib.tsc_embed_prune_count(None, C.byref(n)) == TSC_ERR_INVALID
        assert lib.tsc_embed_prune_poses(run, 0, p(out), C.c_int64(ns.value - 1)) == TSC_ERR_INVALID and f"{ns.value} are asked for" in err()
        good(ctx)
    finally:
        assert lib.tsc_embed_prune_destroy(run) == 0
    assert lib.tsc_embed_prune_destroy(None) == 0


@gpu
def test_a_slab_is_checked_as_tsc_cyclical_embed_groups_checks_it(eng, oracle):
    """The same checks with the same messages, before anything is launched: a bad slab leaves the run's rows as they were."""
    from tscode_amd._lib import TscodeHipError
    from tscode_amd.engine import FragmentSet
    y = yardstick("two", oracle)
    coords, blocks, _ = group_records(y.mols)
    frags = FragmentSet(coords)
    good = slab_args(blocks, 0, 2, y.angles)
    run = eng.embed_prune_run(frags, np.flatnonzero(y.atomnos != 1))
    try:
        assert run.add_groups(*good, THRESH, 0, 1.0)[1].any()
        before, rows = run.count(), run.poses(1).tobytes()

        def both(args, rmsd_thr=1.0):
            texts = []
            for call in (lambda: eng.cyclical_embed_groups(frags, *args, THRESH, 0, rmsd_thr), lambda: run.add_groups(*args, THRESH, 0, rmsd_thr)):
                with pytest.raises(TscodeHipError) as info:
                    call()
                assert info.value.code == TSC_ERR_INVALID
                texts.append(str(info.value))
            assert texts[0] == texts[1], texts
            assert run.count() == before and run.poses(1).tobytes() == rows
            return texts[0]
        bad = [a.copy() for a in good]
        bad[7][1, 0] = 3
        assert "group 1, molecule 0: n_reactive must be 1 or 2" in both(bad)
        bad = [a.copy() for a in good]
        bad[8][0, 1] = coords[1].shape[0]
        assert "group 0, molecule 1: conformer index out of range" in both(bad)
        assert "bad sizes" in both(good, rmsd_thr=0.0)
        wide = good[:9] + [np.zeros((8193, 2))]
        assert "8193 angle sets per group: must be in [1, 8192]" in both(wide)
        assert run.add_groups(*good, THRESH, 0, 1.0)[1].any() and run.count() == 2 * before
    finally:
        run.close()


@gpu
def test_a_context_frees_its_live_runs(eng, oracle):
    """tsc_ctx_destroy with a run alive (rows in its buffers, pruned or not) frees it with the context; and fifty runs created, asked for their
    count and destroyed leave the context's bookkeeping where it was."""
    y, lib, err, create, add, good, want = _abi(eng, oracle)
    heavy = np.flatnonzero(y.atomnos != 1)
    ctx = C.c_void_p()
    assert lib.tsc_ctx_create(eng.device, C.byref(ctx)) == 0, err()
    n = C.c_int64(-1)
    for i in range(50):
        rc, run = create(ctx, heavy)
        assert rc == 0 and lib.tsc_embed_prune_count(run, C.byref(n)) == 0 and n.value == 0, err()
        if i % 10 == 0:
            assert add(run)[0] == 0 and lib.tsc_embed_prune_count(run, C.byref(n)) == 0 and n.value == want[1].sum()
        assert lib.tsc_embed_prune_destroy(run) == 0
    good(ctx)
    live = [create(ctx, heavy)[1] for _ in range(3)]
    assert add(live[0])[0] == 0 and add(live[1])[0] == 0
    survived, ns = np.zeros(int(want[1].sum()), np.uint8), C.c_int64()
    assert lib.tsc_embed_prune_run(live[1], 0.5, 0, C.c_void_p(survived.ctypes.data), None, None, C.byref(ns)) == 0
    assert lib.tsc_embed_prune_destroy(live[2]) == 0                                  # (one of them goes first, by hand)
    assert lib.tsc_ctx_destroy(ctx) == 0
    good(eng._h)                                                                      # the process's other context is untouched


@gpu
def test_an_engine_closes_its_runs(oracle):
    """The Python side of the same: closing an engine closes the runs it handed out, and their own close() afterwards is a no-op."""
    import tscode_amd
    from tscode_amd.engine import FragmentSet
    y = yardstick("two", oracle)
    coords, blocks, _ = group_records(y.mols)
    e2 = tscode_amd.Engine(0)
    run = e2.embed_prune_run(FragmentSet(coords), np.flatnonzero(y.atomnos != 1))
    assert run.add_groups(*slab_args(blocks, 0, 2, y.angles), THRESH, 0, 1.0)[1].any() and run.count() > 0
    e2.close()
    assert run._r is None
    run.close()
