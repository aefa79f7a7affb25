"""Cross-set RMSD on the MI355X (csrc/cross.hpp, tscode_amd/rmsd_cross.py) against the project's CPU restatement of rmsd_and_max_numba
(oracle.rmsd_pairs): the matrix of values at the edges of every tiling, the first similar library member on inputs built far from the
thresholds, the nearest member with its tie rule and its determinism, centring, the two composites and the forms on device pointers.
Values are asserted at VAL_TOL (tests/test_gpu_parity.py: asserted 1e-9, stated bar 1e-5), verdicts and indices exactly."""

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-9
THR = 0.5
SHAPES = ((1, 1), (1, 65), (16, 63), (17, 64), (33, 130), (5, 700))
ATOM_COUNTS = (3, 4, 5, 29, 32, 33, 200)       # register path exact and padded (<= 32), general path beyond


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def interleaved_atomnos(h):
    """atomnos with h non-hydrogen atoms and a hydrogen at every third position from 0 on: the gather is not a prefix"""
    a = []
    while sum(1 for z in a if z != 1) < h:
        a.append(1 if len(a) % 3 == 0 else 6)
    return np.array(a)


def compared(x, atomnos, center):
    """what the oracle is given: the compared atoms, host-centred on their mean where the call centres"""
    x = x if atomnos is None else x[:, atomnos != 1]
    return x - x.mean(axis=1, keepdims=True) if center else x


def oracle_matrix(oracle, q, l):
    """oracle (rmsd, maxdev) f64[Nq, Nl] of queries q against library l, both (N, h, 3)"""
    nq, nl = len(q), len(l)
    pairs = np.stack([np.repeat(np.arange(nq), nl), nq + np.tile(np.arange(nl), nq)], axis=1)
    r, m = oracle.rmsd_pairs(np.concatenate([q, l]), pairs)
    return r.reshape(nq, nl), m.reshape(nq, nl)


def random_sets(rng, nq, nl, n_atoms):
    library = rng.normal(scale=2.0, size=(nl, n_atoms, 3))
    queries = rng.normal(scale=2.0, size=(nq, n_atoms, 3))
    queries[0] = library[-1] + rng.normal(scale=0.01, size=(n_atoms, 3))      # one near pair, at the last column
    return queries, library


# ----------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("h", ATOM_COUNTS)
def test_values_at_the_edges_of_every_tiling(oracle, h):
    import tscode_amd
    rng = np.random.default_rng(100 + h)
    for nq, nl in SHAPES:
        for atomnos in (None, interleaved_atomnos(h)):
            queries, library = random_sets(rng, nq, nl, h if atomnos is None else len(atomnos))
            for center in (False, True):
                r, m = tscode_amd.rmsd_matrix(queries, library, atomnos, center=center)
                ro, mo = oracle_matrix(oracle, compared(queries, atomnos, center), compared(library, atomnos, center))
                assert r.shape == m.shape == (nq, nl) and r.dtype == m.dtype == np.float64
                dr, dm = np.abs(r - ro).max(), np.abs(m - mo).max()
                print(f"h={h} {nq}x{nl} atomnos={'given' if atomnos is not None else None} center={center}: |d rmsd| {dr:.2e} |d maxdev| {dm:.2e}")
                assert dr < VAL_TOL and dm < VAL_TOL, (h, nq, nl, atomnos is not None, center, dr, dm)


@pytest.mark.parametrize("h", (5, 32, 33))
def test_values_of_a_set_against_itself(oracle, h):
    import tscode_amd
    x = np.random.default_rng(7 + h).normal(scale=2.0, size=(33, h, 3))
    r, m = tscode_amd.rmsd_matrix(x)
    ro, mo = oracle_matrix(oracle, x, x)
    assert r.shape == (33, 33) and np.abs(r - ro).max() < VAL_TOL and np.abs(m - mo).max() < VAL_TOL
    assert np.abs(np.diag(r)).max() < VAL_TOL and np.abs(np.diag(m)).max() < VAL_TOL
    r2, m2 = tscode_amd.rmsd_matrix(x, x)
    assert r2.tobytes() == r.tobytes() and m2.tobytes() == m.tobytes()


@pytest.mark.parametrize("h", (29, 33))
def test_values_do_not_depend_on_the_row_blocks(monkeypatch, h):
    import tscode_amd
    from tscode_amd import rmsd_cross
    queries, library = random_sets(np.random.default_rng(11), 33, 130, h)
    whole = tscode_amd.rmsd_matrix(queries, library)
    square = tscode_amd.rmsd_matrix(queries)
    assert rmsd_cross.CROSS_MATRIX_BYTES == 1 << 30
    # 130 columns are 2080 bytes a row: 12 rows a block, three blocks of 12, 12 and 9; the square has 33 columns, 528 bytes a row: 47 rows
    # under 25 000 bytes, so it gets 6000 bytes: 11 rows, three blocks
    monkeypatch.setattr(rmsd_cross, "CROSS_MATRIX_BYTES", 25000)
    assert tscode_amd.get_engine().rmsd_cross_rows(130, 25000) == 12
    blocks = tscode_amd.rmsd_matrix(queries, library)
    assert blocks[0].tobytes() == whole[0].tobytes() and blocks[1].tobytes() == whole[1].tobytes()
    monkeypatch.setattr(rmsd_cross, "CROSS_MATRIX_BYTES", 6000)
    assert tscode_amd.get_engine().rmsd_cross_rows(33, 6000) == 11
    sq = tscode_amd.rmsd_matrix(queries)
    assert sq[0].tobytes() == square[0].tobytes() and sq[1].tobytes() == square[1].tobytes()


# ----------------------------------------------------------------------------- 2. first match
FIRST_CASES = ((30, 65, 1), (30, 130, 2), (40, 65, 3), (40, 130, 4))     # (compared atoms, library size, seed)
_first_cache = {}


def first_case(h, nl, seed):
    """(queries, library, expected kinds).  The library: distinct parents of N(0, 3^2) coordinates, several A apart, but for two triples of
    rows that are copies of one parent each with N(0, 0.03^2) noise -- what "similar to three library rows" needs.  The queries, every
    kind twice:  parent + noise; an exact copy of a row; similar to the three rows of a triple; similar to the last row only
    (nl % 64 != 0); similar to none; a row with one atom moved by 1.5 A (passes on rmsd, fails on maxdev)."""
    if (h, nl, seed) not in _first_cache:
        assert nl % 64 != 0
        rng = np.random.default_rng(seed)
        library = rng.normal(scale=3.0, size=(nl, h, 3))
        triples = ((7, 40, nl - 2), (3, 21, 62))        # (neither holds the last row; with 130 rows the first spans three 64-column tiles)
        for tr in triples:
            for i in tr[1:]:
                library[i] = library[tr[0]] + rng.normal(scale=0.03, size=(h, 3))
        free = [i for i in range(nl - 1) if all(i not in tr for tr in triples)]
        noise = lambda: rng.normal(scale=0.03, size=(h, 3))     # noqa: E731
        moved = []
        for i in (free[5], free[-1]):
            x = library[i].copy()
            x[h // 2] += 1.5 * np.array([0.6, 0.0, 0.8])
            moved.append(x)
        queries = [library[free[0]] + noise(), library[free[20]] + noise(),            # parent + noise
                   library[free[1]].copy(), library[nl - 1].copy(),                   # exact copies
                   library[7] + noise(), library[3] + noise(),                        # similar to three rows
                   library[nl - 1] + noise(), library[nl - 1] + noise(),              # similar to the last row only
                   rng.normal(scale=3.0, size=(h, 3)), rng.normal(scale=3.0, size=(h, 3)),   # similar to none
                   moved[0], moved[1]]                                                # rmsd passes, maxdev fails
        want = [free[0], free[20], free[1], nl - 1, 7, 3, nl - 1, nl - 1, -1, -1, -1, -1]
        _first_cache[(h, nl, seed)] = (np.array(queries), library, np.array(want, dtype=np.int32))
    return _first_cache[(h, nl, seed)]


def far_from_thresholds(ro, mo):
    """the precondition of the first-match tests, from the oracle's values alone: no pair within 1e-3 of either threshold"""
    return np.abs(ro - THR).min() > 1e-3 and np.abs(mo - 2 * THR).min() > 1e-3


@pytest.mark.parametrize("h,nl,seed", FIRST_CASES)
def test_first_match(oracle, h, nl, seed):
    import tscode_amd
    queries, library, want = first_case(h, nl, seed)
    ro, mo = oracle_matrix(oracle, queries, library)
    assert far_from_thresholds(ro, mo), (np.abs(ro - THR).min(), np.abs(mo - 2 * THR).min())
    sim_o = (ro < THR) & (mo < 2 * THR)
    first_o = np.where(sim_o.any(axis=1), sim_o.argmax(axis=1), -1).astype(np.int32)
    # the construction itself: every kind is what it was built to be
    assert np.array_equal(first_o, want), (first_o, want)
    assert sim_o[4].sum() == 3 and sim_o[5].sum() == 3 and (ro[10:] < THR).any(axis=1).all() and not sim_o[10:].any()
    similar, first = tscode_amd.rmsd_similarity_mask(queries, library, None, THR)
    assert similar.dtype == bool and first.dtype == np.int32
    assert np.array_equal(similar, sim_o.any(axis=1)) and np.array_equal(first, first_o)
    loop = np.array([tscode_amd._rmsd_similarity(q, library, THR) for q in queries])
    assert np.array_equal(similar, loop)


# ----------------------------------------------------------------------------- 3. nearest
def check_nearest(oracle, queries, library, got, atomnos=None, center=False):
    index, r, m = got
    ro, mo = oracle_matrix(oracle, compared(queries, atomnos, center), compared(library, atomnos, center))
    rows = np.arange(len(queries))
    assert index.dtype == np.int32 and index.shape == (len(queries),) and (index >= 0).all() and (index < len(library)).all()
    assert np.abs(ro[rows, index] - ro.min(axis=1)).max() < VAL_TOL
    assert np.abs(r - ro[rows, index]).max() < VAL_TOL and np.abs(m - mo[rows, index]).max() < VAL_TOL


@pytest.mark.parametrize("nq,nl", ((1, 700), (40, 3)))
@pytest.mark.parametrize("h", (30, 40))
def test_nearest(oracle, nq, nl, h):
    import tscode_amd
    queries, library = random_sets(np.random.default_rng(nq + h), nq, nl, h)
    got = tscode_amd.nearest_structures(queries, library)
    check_nearest(oracle, queries, library, got)
    assert got[0][0] == nl - 1                       # (random_sets: query 0 lies beside the last library row)
    again = tscode_amd.nearest_structures(queries, library)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    atomnos = interleaved_atomnos(h)
    q2, l2 = random_sets(np.random.default_rng(nq), nq, nl, len(atomnos))
    check_nearest(oracle, q2, l2, tscode_amd.nearest_structures(q2, l2, atomnos, center=True), atomnos, True)


@pytest.mark.parametrize("h", (30, 40))
def test_nearest_of_two_identical_rows_is_the_lower(h):
    import tscode_amd
    rng = np.random.default_rng(5)
    library = rng.normal(scale=2.0, size=(700, h, 3))
    target = rng.normal(scale=2.0, size=(h, 3))
    for lo, hi in ((10, 11), (63, 64), (100, 699)):          # one tile, two tiles of one segment, two segments
        lib = library.copy()
        lib[lo] = lib[hi] = target
        queries = np.stack([target + rng.normal(scale=0.01, size=(h, 3)), target])
        index, r, _m = tscode_amd.nearest_structures(queries, lib)
        assert index.tolist() == [lo, lo] and r[0] < 0.05 and r[1] < VAL_TOL


# ----------------------------------------------------------------------------- 4. translation
@pytest.mark.parametrize("h", (30, 40))
def test_centring_removes_a_translation_of_the_queries(h):
    import tscode_amd
    queries, library = random_sets(np.random.default_rng(3), 17, 64, h)
    shifted = queries + np.array([100.0, -50.0, 25.0])
    r0, m0 = tscode_amd.rmsd_matrix(queries, library, center=True)
    r1, m1 = tscode_amd.rmsd_matrix(shifted, library, center=True)
    assert np.abs(r1 - r0).max() < VAL_TOL and np.abs(m1 - m0).max() < VAL_TOL
    r2, _ = tscode_amd.rmsd_matrix(queries, library)
    r3, _ = tscode_amd.rmsd_matrix(shifted, library)
    assert np.abs(r3 - r2).max() > 1.0
    assert shifted[0, 0, 0] == queries[0, 0, 0] + 100.0      # (the caller's arrays are not modified)


# ----------------------------------------------------------------------------- 5. composites
@pytest.mark.parametrize("h,nl,seed", FIRST_CASES)
def test_prune_against_a_library(h, nl, seed):
    import tscode_amd
    queries, library, want = first_case(h, nl, seed)
    atomnos = np.full(h, 6)
    novel, mask = tscode_amd.prune_conformers_rmsd_against(queries, library, atomnos, THR)
    similar, _ = tscode_amd.rmsd_similarity_mask(queries, library, None, THR)
    assert mask.dtype == bool and np.array_equal(mask, ~similar) and np.array_equal(mask, want < 0)
    assert np.array_equal(novel, queries[mask])


def test_assign_to_kept_after_a_prune(oracle):
    import tscode_amd
    g = load_golden("G3_prune")
    removed_any = False
    for c in range(int(g["n_cases"])):
        structures, atomnos, thr = g[f"structures{c}"], g[f"atomnos{c}"], float(g[f"thr{c}"])
        _, mask = tscode_amd.prune_conformers_rmsd(structures, atomnos, thr)
        rep, population = tscode_amd.assign_to_kept(structures, mask, atomnos)
        n = len(structures)
        kept, removed = np.flatnonzero(mask), np.flatnonzero(~mask)
        assert rep.dtype == np.int32 and population.dtype == np.int64 and rep.shape == population.shape == (n,)
        assert mask[rep].all() and np.array_equal(rep[kept], kept)
        assert population.sum() == n and (population[removed] == 0).all() and (population[kept] >= 1).all()
        assert np.array_equal(population, np.bincount(rep, minlength=n))
        if len(removed):
            removed_any = True
            heavy = structures[:, atomnos != 1]
            ro, _ = oracle_matrix(oracle, heavy[removed], heavy[kept])
            at = np.searchsorted(kept, rep[removed])
            assert np.abs(ro[np.arange(len(removed)), at] - ro.min(axis=1)).max() < VAL_TOL
    assert removed_any


# ----------------------------------------------------------------------------- 6. device pointers
def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    return t


def _room(shape, dtype):
    import torch
    t = torch.zeros(shape, dtype=dtype, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("h", (29, 33))
def test_device_pointer_forms_equal_the_host_array_forms(eng, h):
    import torch
    atomnos = interleaved_atomnos(h)
    idx = np.flatnonzero(atomnos != 1).astype(np.int32)
    n = len(atomnos)
    queries, library = random_sets(np.random.default_rng(h), 33, 130, n)
    library[70] = queries[5] + 0.01
    d_q, d_l, d_idx = _dev(queries), _dev(library), _dev(idx)
    for center in (False, True):
        d_r, d_m = _room((33, 130), torch.float64), _room((33, 130), torch.float64)
        eng.rmsd_cross_dev(d_q, 33, d_l, 130, n, d_idx, len(idx), center, d_r, d_m, 33 * 130)
        eng.synchronize()
        r, m = eng.rmsd_cross(queries, library, idx, center)
        assert d_r.cpu().numpy().tobytes() == r.tobytes() and d_m.cpu().numpy().tobytes() == m.tobytes()
        d_first = _room((33,), torch.int32)
        eng.rmsd_cross_first_dev(d_q, 33, d_l, 130, n, d_idx, len(idx), center, THR, d_first)
        eng.synchronize()
        first = eng.rmsd_cross_first(queries, library, idx, THR, center)
        assert np.array_equal(d_first.cpu().numpy(), first) and first[0] == 129 and first[5] == 70 and (first == np.iinfo(np.int32).max).sum() == 31
        d_i, d_nr, d_nm = _room((33,), torch.int32), _room((33,), torch.float64), _room((33,), torch.float64)
        eng.rmsd_cross_nearest_dev(d_q, 33, d_l, 130, n, d_idx, len(idx), center, d_i, d_nr, d_nm)
        eng.synchronize()
        index, nr, nm = eng.rmsd_cross_nearest(queries, library, idx, center)
        assert np.array_equal(d_i.cpu().numpy(), index) and d_nr.cpu().numpy().tobytes() == nr.tobytes() and d_nm.cpu().numpy().tobytes() == nm.tobytes()
    # all atoms, the set against itself: no library, no index list
    d_r, d_m = _room((33, 33), torch.float64), _room((33, 33), torch.float64)
    eng.rmsd_cross_dev(d_q, 33, None, 33, n, None, 0, False, d_r, d_m, 33 * 33)
    eng.synchronize()
    r, m = eng.rmsd_cross(queries)
    assert d_r.cpu().numpy().tobytes() == r.tobytes() and d_m.cpu().numpy().tobytes() == m.tobytes()
    # a request beyond the room the caller has is refused
    from tscode_amd._lib import TscodeHipError
    with pytest.raises(TscodeHipError, match="room for"):
        eng.rmsd_cross_dev(d_q, 33, d_l, 130, n, None, 0, False, d_r, d_m, 33 * 33)
