"""The energy-ordered RMSD prune (csrc/leader.hpp, tscode_amd/rmsd_ordered.py): keep a row iff no row KEPT before it in the order is similar.

Yardstick: the project's C restatement of the greedy filter (oracle.greedy_group_filter) on the compared atoms in walking order for the mask,
and for ``rep`` the lowest kept row in front that oracle.rmsd_pairs calls similar.  Every input is first held against the condition that makes
an exact comparison of verdicts meaningful: under the oracle every pair i > j lies at least 1e-6 from both thresholds (asserted, over all
pairs, never skipped).  Masks, representatives and populations are then asserted exactly.  The host tests at the end need no GPU."""

import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT

THR = 0.5
MARGIN = 1e-6
gpu = pytest.mark.gpu


# ----------------------------------------------------------------------------- yardstick
def yardstick(oracle, xc, thr=THR, n_lib=0):
    """xc f64[n, h, 3]: the compared atoms in walking order, the library's rows (n_lib of them) in front.  mask bool[n] and rep i64[n]
    (positions in xc; a kept row itself) of the sequential rule, and sim[i, j] (i > j) of the oracle.  Asserts the margin condition."""
    xc = np.ascontiguousarray(xc, dtype=np.float64)
    n = len(xc)
    i, j = np.tril_indices(n, -1)                                            # every pair i > j: row i turned onto row j
    r, m = oracle.rmsd_pairs(xc, np.stack([i, j], axis=1)) if n > 1 else (np.zeros(0), np.zeros(0))
    margin = min(np.abs(r - thr).min(), np.abs(m - 2 * thr).min()) if len(r) else np.inf
    print(f"n={n} h={xc.shape[1]}: {len(r)} pairs, margin to the thresholds {margin:.3g}")
    assert margin >= MARGIN, f"the input does not separate the verdicts: margin {margin:.3g}"
    sim = np.zeros((n, n), dtype=bool)
    sim[i, j] = (r < thr) & (m < 2 * thr)
    mask = oracle.greedy_group_filter(xc, thr)
    assert mask[:n_lib].all(), "two library rows are similar: the concatenation is no yardstick for a library that is never removed"
    rep = np.arange(n)
    for s in np.flatnonzero(~mask):
        rep[s] = np.flatnonzero(sim[s, :s] & mask[:s])[0]                    # kept rows are met in the order they were kept
    return SimpleNamespace(mask=mask, rep=rep, sim=sim, margin=margin)


def compared(x, atomnos=None, center=False):
    x = x if atomnos is None else x[:, np.asarray(atomnos) != 1]
    return x - x.mean(axis=1, keepdims=True) if center else x


def assert_result(res, y, order=None, n_lib=0):
    """res of leader_clusters on the batch against the yardstick y on concat(library, batch[order])"""
    n = len(res.mask)
    order = np.arange(n) if order is None else order
    ym, yr = y.mask[n_lib:], y.rep[n_lib:]
    assert res.mask.dtype == bool and res.rep.dtype == np.int32 and res.library_rep.dtype == np.int32 and res.population.dtype == np.int64
    assert np.array_equal(res.mask[order], ym), (int(res.mask.sum()), int(ym.sum()))
    by_lib = yr < n_lib
    want_rep = np.where(by_lib, -1, order[np.maximum(yr - n_lib, 0)])
    want_lib = np.where(by_lib, yr, -1)
    assert np.array_equal(res.rep[order], want_rep)
    assert np.array_equal(res.library_rep[order], want_lib)
    assert np.array_equal(res.population, np.bincount(want_rep[~by_lib], minlength=n))
    assert np.array_equal(res.library_population, np.bincount(want_lib[by_lib], minlength=n_lib))
    assert res.population.sum() + res.library_population.sum() == n and (res.population[~res.mask] == 0).all()


# ----------------------------------------------------------------------------- inputs
def chain(n, step):
    """the 12-atom fragment, centred, shifted along x by i * step: neighbours are similar at THR, second neighbours are not"""
    from tscode_amd.synthetic import make_fragment
    frag = make_fragment(np.random.default_rng(5), 12)
    x = np.repeat(frag[None], n, axis=0)
    x[:, :, 0] += (np.arange(n) * step)[:, None]
    return x


_ensembles = {}


def ensemble(n, children):
    """(structures f64[n, 50, 3], atomnos) of make_ensemble(n, (25, 25), seed=77): 30 heavy atoms, the children shuffled over the array"""
    if (n, children) not in _ensembles:
        from tscode_amd.synthetic import make_ensemble
        ens = make_ensemble(n, (25, 25), seed=77, children=children)
        _ensembles[n, children] = (ens.poses(), ens.atomnos)
    return _ensembles[n, children]


_yards = {}


def ensemble_yard(oracle, n, children):
    if (n, children) not in _yards:
        x, atomnos = ensemble(n, children)
        _yards[n, children] = yardstick(oracle, compared(x, atomnos))
    return _yards[n, children]


def families(rng, n, h, n_par, noise=0.03, scale=3.0):
    """n structures of h atoms: n_par parents several A apart, every row a parent with N(0, noise^2) on each coordinate, rows shuffled"""
    parents = rng.normal(scale=scale, size=(n_par, h, 3))
    return parents[rng.integers(0, n_par, size=n)] + rng.normal(scale=noise, size=(n, h, 3))


# ----------------------------------------------------------------------------- 1. the chain
@gpu
def test_the_chain_a_removed_row_covers_nothing(oracle):
    import tscode_amd
    x = chain(41, 0.4)
    y = yardstick(oracle, x)
    assert np.array_equal(y.mask, np.arange(41) % 2 == 0)
    # the input proves something only if a removed row j and a later KEPT row s with similar(s -> j) exist
    witness = y.sim & ~y.mask[None, :] & y.mask[:, None]
    assert witness.any()
    res = tscode_amd.leader_clusters(x, None, THR)
    assert_result(res, y)
    assert res.mask.sum() == 21 and np.array_equal(res.rep[1::2], np.arange(0, 40, 2))
    kept, mask = tscode_amd.prune_conformers_rmsd_ordered(x, None, THR)
    assert np.array_equal(mask, res.mask) and np.array_equal(kept, x[mask])
    # the reference-exact prune is another rule and gives another set
    _, other = tscode_amd.prune_conformers_rmsd(x, np.full(12, 6), THR)
    assert np.array_equal(other, oracle.prune_conformers_rmsd(x, np.full(12, 6), THR)[1]) and not np.array_equal(other, res.mask)


# ----------------------------------------------------------------------------- 2. block edges
def _block():
    from tscode_amd import rmsd_ordered
    return rmsd_ordered.LEADER_BLOCK


@gpu
@pytest.mark.parametrize("which", ("1", "2", "B-1", "B", "B+1", "2B+1"))
def test_chains_across_the_block_edges(oracle, which):
    import tscode_amd
    B = _block()
    n = {"1": 1, "2": 2, "B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[which]
    step = {"1": 0.3, "2": 0.3, "B-1": 0.35, "B": 0.4, "B+1": 0.3, "2B+1": 0.35}[which]
    x = chain(n, step)
    y = yardstick(oracle, x)
    assert np.array_equal(y.mask, np.arange(n) % 2 == 0)                     # the alternation runs through every boundary
    res = tscode_amd.leader_clusters(x, None, THR, library=np.zeros((0, 12, 3)))   # the first block meets an empty library
    assert_result(res, y)


@gpu
def test_a_block_the_library_covers_whole(oracle):
    """library: the even rows of a chain; batch: its odd rows, B + 1 of them -- the library decides every row of both blocks, the in-block
    work has no open row and the second block's library walk sees a pack that did not grow"""
    import tscode_amd
    B = _block()
    x = chain(2 * B + 3, 0.4)
    lib, batch = x[0::2], x[1::2]
    assert len(batch) == B + 1 and len(lib) == B + 2
    y = yardstick(oracle, np.concatenate([lib, batch]), n_lib=len(lib))
    assert not y.mask[len(lib):].any()
    res = tscode_amd.leader_clusters(batch, None, THR, library=lib)
    assert_result(res, y, n_lib=len(lib))
    assert np.array_equal(res.library_rep, np.arange(B + 1)) and (res.rep == -1).all()     # rows 2k and 2k + 2 both cover 2k + 1: the lower


# ----------------------------------------------------------------------------- 3. clustered parity
@gpu
@pytest.mark.parametrize("n, children, n_kept", ((1500, 10, 150), (2100, 6, 350)))
def test_clustered_ensembles_collapse_to_their_parents(oracle, n, children, n_kept):
    import tscode_amd
    x, atomnos = ensemble(n, children)
    y = ensemble_yard(oracle, n, children)
    assert y.mask.sum() == n_kept
    res = tscode_amd.leader_clusters(x, atomnos, THR)
    assert_result(res, y)
    assert res.population.sum() == n and res.mask.sum() == n_kept


# ----------------------------------------------------------------------------- 4. order
@gpu
def test_energies_with_ties_give_the_stable_order(oracle):
    import tscode_amd
    x, atomnos = ensemble(1500, 10)
    x = x[:1300]                                                            # two blocks
    e = np.random.default_rng(3).integers(0, 60, size=len(x)) * 0.25        # many ties
    order = np.argsort(e, kind="stable")
    y = yardstick(oracle, compared(x[order], atomnos))
    res = tscode_amd.leader_clusters(x, atomnos, THR, energies=e)
    assert_result(res, y, order=order)
    pre = tscode_amd.leader_clusters(x[order], atomnos, THR)
    assert np.array_equal(pre.mask, res.mask[order]) and np.array_equal(order[pre.rep], res.rep[order])
    plain = tscode_amd.leader_clusters(x, atomnos, THR)
    assert not np.array_equal(plain.mask, res.mask)                         # (the order matters on this input)
    kept, mask = tscode_amd.prune_conformers_rmsd_ordered(x, atomnos, THR, energies=e)
    assert np.array_equal(mask, res.mask) and np.array_equal(kept, x[mask])


# ----------------------------------------------------------------------------- 5. library
@gpu
def test_a_second_batch_against_the_kept_set_of_the_first(oracle):
    import tscode_amd
    x, atomnos = ensemble(2100, 6)
    a, b = x[:900], x[900:]                                                 # the batch spans two blocks
    first = tscode_amd.leader_clusters(a, atomnos, THR)
    lib = a[first.mask]
    lib_before = lib.copy()
    y = yardstick(oracle, compared(np.concatenate([lib, b]), atomnos), n_lib=len(lib))
    res = tscode_amd.leader_clusters(b, atomnos, THR, library=lib)
    assert_result(res, y, n_lib=len(lib))
    assert (res.library_rep >= 0).any() and res.mask.any() and (res.rep[~res.mask] >= 0).any()     # all three fates occur
    assert np.array_equal(lib, lib_before)
    # both calls together keep what one call on the whole array keeps
    whole = ensemble_yard(oracle, 2100, 6)
    assert np.array_equal(np.concatenate([first.mask, res.mask]), whole.mask)


# ----------------------------------------------------------------------------- 6. same rule, other route
@gpu
def test_all_atoms_equal_the_group_filter_on_one_group(oracle):
    import tscode_amd
    x, _ = ensemble(1500, 10)
    x = x[:700]
    y = yardstick(oracle, x)
    res = tscode_amd.leader_clusters(x, None, THR)
    assert_result(res, y)
    assert np.array_equal(res.mask, tscode_amd.filter_angular_groups(x, [len(x)], THR))


# ----------------------------------------------------------------------------- 7. compared-atom counts
@gpu
@pytest.mark.parametrize("h", (3, 4, 18, 32, 33, 60))
def test_compared_atom_counts(oracle, h):
    """the register path's padding steps (3 -> 4, 4, 18 -> 20), its last size (32) and the general path (33, 60); hydrogens interleaved, so
    the compared atoms are no prefix; more than one block, so that both the library walk and the in-block bits decide rows"""
    import tscode_amd
    atomnos = np.array([1 if k % 3 == 0 else 6 for k in range(3 * h)])[: h + (h + 1) // 2]
    while (atomnos != 1).sum() < h:
        atomnos = np.append(atomnos, 6)
    assert (atomnos != 1).sum() == h
    x = families(np.random.default_rng(200 + h), _block() + 100, len(atomnos), 90, scale=3.0 if h > 4 else 6.0)
    y = yardstick(oracle, compared(x, atomnos))
    assert 1 < y.mask.sum() < len(x)
    res = tscode_amd.leader_clusters(x, atomnos, THR)
    assert_result(res, y)


# ----------------------------------------------------------------------------- 8. centring
@gpu
def test_center_equals_the_yardstick_on_centred_copies(oracle):
    import tscode_amd
    rng = np.random.default_rng(8)
    atomnos = np.array([6, 1, 6] * 9)                                       # 18 compared atoms
    x = families(rng, 300, len(atomnos), 25) + rng.normal(scale=5.0, size=(300, 1, 3))      # every structure in a frame of its own
    lib = families(np.random.default_rng(8), 300, len(atomnos), 25)[:0]     # (an empty library is centred too: nothing happens)
    y = yardstick(oracle, compared(x, atomnos, center=True))
    assert 1 < y.mask.sum() <= 25
    before = x.copy()
    res = tscode_amd.leader_clusters(x, atomnos, THR, center=True, library=lib)
    assert_result(res, y)
    assert np.array_equal(x, before)
    plain = yardstick(oracle, compared(x, atomnos))                         # uncentred, translation counts as deviation: another result
    assert not np.array_equal(plain.mask, y.mask)
    assert_result(tscode_amd.leader_clusters(x, atomnos, THR), plain)


# ----------------------------------------------------------------------------- 9. determinism
@gpu
def test_two_calls_return_identical_results():
    import tscode_amd
    x, atomnos = ensemble(2100, 6)
    a, b = tscode_amd.leader_clusters(x, atomnos, THR), tscode_amd.leader_clusters(x, atomnos, THR)
    assert a.mask.tobytes() == b.mask.tobytes() and a.rep.tobytes() == b.rep.tobytes() and a.library_rep.tobytes() == b.library_rep.tobytes()


# ----------------------------------------------------------------------------- 10. degenerate inputs
@gpu
def test_identical_structures_keep_one_row_and_tiny_inputs(oracle):
    import tscode_amd
    B = _block()
    x = np.repeat(chain(1, 0.3), B + 5, axis=0)
    y = yardstick(oracle, x)
    assert y.mask.sum() == 1
    res = tscode_amd.leader_clusters(x, None, THR)
    assert_result(res, y)
    assert res.mask[0] and (res.rep == 0).all() and res.population[0] == B + 5
    one = tscode_amd.leader_clusters(x[:1], np.full(12, 6), THR)
    assert one.mask.tolist() == [True] and one.rep.tolist() == [0] and one.library_rep.tolist() == [-1] and one.population.tolist() == [1]
    none = tscode_amd.leader_clusters(x[:0], None, THR, library=x[:1])
    assert none.mask.shape == none.rep.shape == none.library_rep.shape == none.population.shape == (0,) and none.library_population.tolist() == [0]
    kept, mask = tscode_amd.prune_conformers_rmsd_ordered(x[:0], None)
    assert kept.shape == (0, 12, 3) and mask.shape == (0,) and mask.dtype == bool


# ----------------------------------------------------------------------------- host tests (no GPU)
@pytest.fixture
def no_engine(monkeypatch):
    """every way from rmsd_ordered.py to the device fails the test: the errors below are raised before an engine is asked for"""
    from tscode_amd import rmsd_ordered

    def refuse(*_a, **_k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(rmsd_ordered, "get_engine", refuse)


def test_argument_errors_come_without_an_engine(no_engine):
    import tscode_amd

    def calls(x, atomnos, **kw):
        return (lambda: tscode_amd.leader_clusters(x, atomnos, **kw), lambda: tscode_amd.prune_conformers_rmsd_ordered(x, atomnos, **kw))
    x, lib = np.zeros((4, 5, 3)), np.ones((6, 5, 3))
    for bad in (np.zeros((5, 3)), np.zeros((4, 5, 2)), np.zeros((4, 5, 3, 1))):            # wrong rank or last extent
        for call in calls(bad, None) + calls(x, None, library=bad):
            with pytest.raises(ValueError, match=r"must be \(N, n_atoms, 3\)"):
                call()
    for call in calls(x, None, library=np.ones((6, 4, 3))):                               # unequal atom counts
        with pytest.raises(ValueError, match="5 atoms, library has 4"):
            call()
    for atomnos in (np.full(4, 6), np.full((5, 1), 6)):                                   # atomnos of the wrong length
        for call in calls(x, atomnos):
            with pytest.raises(ValueError, match="atomnos must be"):
                call()
    for call in calls(x, np.ones(5, dtype=int)):                                          # no compared atom
        with pytest.raises(ZeroDivisionError):
            call()
    for energies in (np.zeros(3), np.zeros((4, 1)), np.zeros(5)):                          # energies of the wrong length
        for call in calls(x, None, energies=energies):
            with pytest.raises(ValueError, match="energies must be"):
                call()
    for call in calls(x, None, energies=np.array([0.0, np.nan, 1.0, 2.0])):
        with pytest.raises(ValueError, match="NaN"):
            call()
    for value in (np.nan, np.inf):
        q, bad_lib = x.copy(), lib.copy()
        q[2, 3, 1] = value
        bad_lib[5, 0, 2] = value
        for call in calls(q, None) + calls(x, None, library=bad_lib):                     # a coordinate that is not finite
            with pytest.raises(ValueError, match="not finite"):
                call()
    for call in calls(x, None, rmsd_thr=np.nan):
        with pytest.raises(ValueError, match="rmsd_thr"):
            call()


def test_empty_input_needs_no_engine(no_engine):
    import tscode_amd
    res = tscode_amd.leader_clusters(np.zeros((0, 5, 3)), np.full(5, 6), library=np.ones((6, 5, 3)), energies=np.zeros(0))
    assert res.mask.shape == (0,) and res.mask.dtype == bool and res.rep.dtype == res.library_rep.dtype == np.int32
    assert res.population.shape == (0,) and res.library_population.tolist() == [0] * 6 and res.library_population.dtype == np.int64


def test_exports_and_the_block_constant():
    import tscode_amd
    from tscode_amd import _lib, rmsd_ordered
    from tscode_amd.build import SOURCES, build
    for name in ("prune_conformers_rmsd_ordered", "leader_clusters"):
        assert getattr(tscode_amd, name) is getattr(rmsd_ordered, name) and name in rmsd_ordered.__all__
    assert rmsd_ordered.LEADER_BLOCK % 64 == 0 and rmsd_ordered.LEADER_BLOCK >= 64
    assert "leader.hip" in SOURCES
    for s in ("tsc_prune_rmsd_ordered", "tsc_prune_rmsd_ordered_dev", "tsc_leader_block"):
        assert s in _lib.EXPORTED_SYMBOLS
    build()
    assert _lib.load().tsc_leader_block() == rmsd_ordered.LEADER_BLOCK        # what the library walks is what the tests read
    plan = open(os.path.join(ROOT, "tscode_amd", "csrc", "leader_plan.hpp")).read()
    assert re.search(r"constexpr int LEADER_BLOCK = %d;" % rmsd_ordered.LEADER_BLOCK, plan)
    assert "assign_to_kept" in rmsd_ordered.leader_clusters.__doc__               # rep is the leader, not the nearest: the docstring says where the nearest is


def test_plan_at_hand_worked_sizes(tmp_path):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "leader_plan_check.py"), "--keep", str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"leader_plan_check: \d+ checks passed", run.stdout), run.stdout + run.stderr
    assert "clean under ASan and UBSan" in run.stdout


def test_the_plan_probe_includes_no_header_that_defines_a_kernel():
    from tscode_amd.build import CFLAGS, _hipcc
    out = subprocess.run([_hipcc()] + CFLAGS + ["--cuda-host-only", "-MM", os.path.join("tools", "probe", "leader_plan_check.cpp")], check=True, cwd=ROOT,
                         capture_output=True, text=True).stdout
    deps = [os.path.normpath(w) for w in out.replace("\\\n", " ").split()[1:] if not os.path.isabs(w)]
    assert os.path.join("tscode_amd", "csrc", "leader_plan.hpp") in deps and os.path.join("tscode_amd", "csrc", "cross_plan.hpp") in deps
    assert not [d for d in deps if "__global__" in open(os.path.join(ROOT, d)).read()]
