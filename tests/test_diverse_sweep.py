"""Shape sweep of alignment, k-means, seeding and the pick (tscode_amd/csrc/diverse.hpp, diverse.hip) at the shapes the G20 fixtures, the
scale case and the batch test do not compare with anything but the library itself.  The yardsticks are the NumPy restatements of
tests/test_diverse.py (lloyd_restated, seed_restated, pick_restated, kabsch_align_numpy -- the first pinned to scikit-learn by G20 and,
for several clusters empty at once, by G20e) and, where the optimal rotation is not unique, properties that hold for every optimum.
Every input is built here from a committed seed; the unmarked twin of each GPU test (test_*_inputs_meet_the_conditions_...) builds the
same inputs and checks, with the yardstick alone, the conditions the comparison leans on.  The GPU tests assert equality with no case
left out.

Which path of diverse.hpp each shape is there for:

1. tsc_kmeans_lloyd, k / D / N edges (dv_kmeans_assign<NT>, dv_kmeans_update, dv_col_partial, dv_label_bucket)
   k = 49, 64        template width 4 (its first and its full tile count), one centre block
   k = 129, 130      width 5, two centre blocks of 80: bd[] / bc[] carried across the c0 loop, 49 and 50 centres live in the second
                     (c >= k masked to infinity, one and two of them in its fourth tile)
   k = 192           width 6, two full blocks
   k = 256, 257      width 8 in two blocks; width 6 in three (the third trip of the c0 loop)
   k = 300           width 7, three blocks, 76 of 112 centres in the last
   tie115, tie129    init centre 115 / 128 a copy of centre 3: an exact tie ACROSS centre blocks, cluster 115 / 128 empty in iteration 1.
                     Centre 115 = 80 + 2 * 16 + 3 sits in centre 3's own lane, where only the strict < of the c0 loop keeps centre 3;
                     centre 128 sits in lane 0, where the reduction over the 16 lanes of a row decides.  Both are also run with
                     max_iter = 1: the centres right after the relocation, before later iterations can mend them
   D = 1, 3, 31, 32, 33, 63, 64, 65, 1536 (k = 17), 33 and 65 (k = 129)
                     the 32-column slices of the assignment with their zero-filled tail, the 64-column slices of the update and of the
                     column statistics, the limit 3 * DV_MAX_ATOMS
   N = 17, 18, 63, 64, 65, 255, 256, 257, 512, 16387 (k = 17, D = 9)
                     N == k, the 64-row tile of the assignment, the 256-row sweep of the bucket kernel, 1 / 2 / 64 chunks of the column
                     statistics (16387 = 64 * 256 + 3: the cap, chunks of 257 rows with a last one of 196)
2. several clusters empty at once (dv_kmeans_relocate beyond j = 0, the replay of the whole table in dv_kmeans_update): G20e, recorded
   from scikit-learn -- exact copies of an init centre (ties), centres far outside the data (no tie), two relocations out of one donor
   cluster, two farthest rows that are copies of one another.  k = 12 and k = 140 (copies and far centres on both sides of centre 128).
   Each case also with max_iter = 1 against the restatement: a converged run forgives a wrong centre of iteration 1, this one does not.
3. tsc_kmeans_seed (dv_kmeans_seed_pick, dv_kmeans_seed_update): N < 1024 (pieces of one row, empty pieces behind them), 1024, 1025 (two rows
   per piece, 512 empty pieces), 2047, 2049 (three rows), 5000; D = 1, 33, 65 (the lane-strided distance); k = 2, 40.  Exact cases (every
   sum is a sum of zeros or of small integers, exact in any order): a target of 0 with five leading copies of the seed, every row a copy
   (the total == 0 exit), and u = nextafter(1, 0) over a total of 64 (the target is the double below 64).
4. tsc_diverse_pick (dv_diverse_pick): member positions p >= k (no centre left out), n = 1 / 63 / 64 / 65 / 200 atoms (the lane-strided
   k * n loop), clusters of 257 and 600 members on the energies path (a second and third trip of the 256 stride, the four-wavefront
   reduction), an empty cluster, and exact ties: copies of a row (cumdist), equal energies at positions 3 / 300 (one wavefront, two
   trips) and 70 / 130 (two wavefronts).
5. align_structures (dv_align_structures, dv_centroid, exact_quaternion of pair_math.hpp): 1, 2, 3, 4, 63, 64, 65, 512 atoms (lane-strided
   loops, DV_MAX_ATOMS); 1, 2, 4, 5, 9 structures (four per workgroup); index sets sorted, unsorted, with a repeat, of one atom; noisy
   copies, unrelated structures, mirror images (det S < 0), planar molecules, structures 1000 A out.  Where Horn's top eigenvalue is
   separated by HORN_BAND relative: coordinates against numpy's SVD route.  Where it is not (1 or 2 atoms, collinear sets, and two
   one-parameter families that walk the gap from 1e-2 to 0 through the hand-over of rotation_quaternion_fast to the Jacobi solver at
   best <= 1e-4 scale^3): the output is finite, a proper rotation of the centred input, and optimal -- its residual over the indexed atoms
   equals Gp + Gq - 2 lambda_max (eigvalsh) within OPTIMUM_TOL * (Gp + Gq).
   OPTIMUM_TOL: measured on the CPU over these same inputs, numpy's SVD route lies within SVD_FROM_OPTIMUM = 2e-15 (relative to Gp + Gq;
   the largest measured figure is 6.9e-16, the twin re-measures it and holds it under SVD_FROM_OPTIMUM) of that optimum.  Ten times that
   is 2e-14, under the floor of 1e-12 for the rounding of the sums themselves: OPTIMUM_TOL = 1e-12.
6. diverse_select beyond k = 128 end to end (600 x 11 atoms, k = 129, the batch test's shape), each stage against its restatement, and the
   same bits as the middle segment of a diverse_select_batch call.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from test_diverse import (COORD_TOL, EMPTY_CASES, HORN_BAND, MARGIN_BAND, PICK_BAND, RELOC_BAND, g20, kabsch_align_numpy, lloyd_restated, moved,
                          pick_restated, relocation_gap, seed_restated)

SEED_CLEAR = 1e-9                                       # test_kmeans_plusplus_rows_follows_the_stated_rule's guard
ENERGY_BAND = 1e-9
SVD_FROM_OPTIMUM = 2e-15                                # module docstring, section 5
OPTIMUM_TOL = max(10 * SVD_FROM_OPTIMUM, 1e-12)


# ===================================================================================================== 1. assignment and update
# name: (k, N, D, seed).  N = 4 k where k is the subject (a few members per cluster: k + 40 rows converge in 2 or 3 iterations)
LLOYD_CASES = {
    "k49": (49, 196, 9, 0), "k64": (64, 256, 9, 0), "k129": (129, 516, 9, 0), "k130": (130, 520, 9, 0), "k192": (192, 768, 9, 0),
    "k256": (256, 1024, 9, 0), "k257": (257, 1028, 9, 0), "k300": (300, 1200, 9, 0), "tie115": (129, 516, 9, 0), "tie129": (129, 516, 9, 0),
    "D1": (17, 68, 1, 0), "D3": (17, 68, 3, 0), "D31": (17, 68, 31, 0), "D32": (17, 68, 32, 0), "D33": (17, 68, 33, 0), "D63": (17, 68, 63, 0),
    "D64": (17, 68, 64, 0), "D65": (17, 68, 65, 0), "D1536": (17, 68, 1536, 0), "k129-D33": (129, 516, 33, 0), "k129-D65": (129, 516, 65, 0),
    "N17": (17, 17, 9, 0), "N18": (17, 18, 9, 0), "N63": (17, 63, 9, 0), "N64": (17, 64, 9, 0), "N65": (17, 65, 9, 0), "N255": (17, 255, 9, 0),
    "N256": (17, 256, 9, 0), "N257": (17, 257, 9, 0), "N512": (17, 512, 9, 0), "N16387": (17, 16387, 9, 0),
}
TIES = {"tie115": 115, "tie129": 128}                   # the init centre that is a copy of centre 3
LONG_RUN = "k300"                                       # a case beyond k = 128 that takes 5 or more iterations


def lloyd_input(name, seed=None):
    """As _width_case of tests/test_diverse.py: normal rows, init centres taken from rows."""
    k, N, D, s = LLOYD_CASES[name]
    rng = np.random.default_rng(4000 + (s if seed is None else seed))
    X = rng.normal(size=(N, D))
    init = X[rng.choice(N, k, replace=False)].copy()
    if name in TIES:
        init[TIES[name]] = init[3]
    return X, init


@functools.lru_cache(maxsize=None)
def lloyd_expected(name):
    X, init = lloyd_input(name)
    rel = []
    return lloyd_restated(X, init, ignore_copies=name in TIES, relocations=rel) + (rel,)


def first_iteration(X, init):
    """The run cut off after one iteration -- the centres right after the relocation, and the labels they give -- as compare_lloyd takes
    it, with its own margin (centres that are copies left out)."""
    labels, centres, inertia, n_iter, margin, max_empty = lloyd_restated(X, init, max_iter=1, ignore_copies=True)
    return (labels, centres, inertia, n_iter, max_empty), margin


def lloyd_guard(name, X, init, expected):
    """The conditions of the comparison, on the yardstick alone; the reason a case fails them, or None."""
    labels, centres, inertia, n_iter, margin, max_empty, rel = expected
    k = len(init)
    if margin < MARGIN_BAND:
        return f"margin {margin:.2e}"
    if name in TIES:
        nearest = np.stack([((X - c) ** 2).sum(1) for c in init], axis=1).argmin(1)
        if not (max_empty == 1 and len(rel) == 1 and rel[0][0] == 0 and rel[0][1].tolist() == [TIES[name]] and (nearest == 3).sum() >= 2 and n_iter >= 2):
            return f"the tie: {max_empty} empty, {[(r[0], r[1].tolist()) for r in rel]}, {(nearest == 3).sum()} rows tied"
        if relocation_gap(X, rel) < RELOC_BAND:
            return f"relocation gap {relocation_gap(X, rel):.2e}"
        if first_iteration(X, init)[1] < MARGIN_BAND:
            return f"margin after one iteration {first_iteration(X, init)[1]:.2e}"
        return None
    if max_empty != 0:
        return f"{max_empty} empty"
    if len(X) == k:
        return None if n_iter == 1 else f"n_iter {n_iter}"          # every row its own centre: nothing moves, the shift of iteration 1 is 0
    if n_iter < 2:
        return f"n_iter {n_iter}"
    if name == LONG_RUN and n_iter < 5:
        return f"n_iter {n_iter} < 5"
    return None


@pytest.mark.parametrize("name", list(LLOYD_CASES))
def test_lloyd_sweep_inputs_meet_the_conditions_the_gpu_tests_lean_on(name):
    X, init = lloyd_input(name)
    k, N, D, _ = LLOYD_CASES[name]
    assert X.shape == (N, D) and init.shape == (k, D) and len(np.unique(init, axis=0)) == (k - 1 if name in TIES else k)
    assert lloyd_guard(name, X, init, lloyd_expected(name)) is None
    tiles = -(-k // 16)
    blocks = -(-tiles // 8)
    width = -(-tiles // blocks)
    want = {"k49": (4, 1), "k64": (4, 1), "k129": (5, 2), "k130": (5, 2), "k192": (6, 2), "k256": (8, 2), "k257": (6, 3), "k300": (7, 3), "tie115": (5, 2), "tie129": (5, 2)}
    assert (width, blocks) == want.get(name, (5, 2) if k == 129 else (2, 1)), "the case no longer reaches the template width it is there for"
    if name == "N16387":                                 # col_stats: min(64, N / 256) chunks of ceil(N / 64) rows, a ragged last one
        assert N // 256 == 64 and -(-N // 64) == 257 and N - 63 * 257 == 196


def abi_lloyd(X, init, max_iter=300, tol=1e-4):
    from tscode_amd import _lib
    from tscode_amd.engine import get_engine
    eng = get_engine()
    X, init = np.ascontiguousarray(X), np.ascontiguousarray(init)
    (N, D), k = X.shape, len(init)
    labels, centres = np.empty(N, np.int32), np.empty((k, D))
    inertia, n_iter, max_empty = C.c_double(), C.c_int(), C.c_int()
    _lib.check(eng.lib.tsc_kmeans_lloyd(eng._h, _lib.ptr(X), C.c_int64(N), C.c_int64(D), _lib.ptr(init), C.c_int(k), C.c_int(max_iter), C.c_double(tol),
                                        _lib.ptr(labels), _lib.ptr(centres), C.byref(inertia), C.byref(n_iter), C.byref(max_empty)))
    return labels, centres, inertia.value, n_iter.value, max_empty.value


def compare_lloyd(what, got, want):
    labels, centres, inertia, n_iter, max_empty = got
    w_labels, w_centres, w_inertia, w_iter, w_empty = want
    print(f"{what}: n_iter {n_iter} (want {w_iter}), labels differing {int((labels != w_labels).sum())}, max_empty {max_empty} (want {w_empty}), "
          f"|centres - want| = {np.abs(centres - w_centres).max():.3e}, inertia rel. {abs(inertia - w_inertia) / (w_inertia or 1.0):.3e}")
    assert np.array_equal(labels, w_labels) and n_iter == w_iter and max_empty == w_empty
    assert np.abs(centres - w_centres).max() <= COORD_TOL
    assert abs(inertia - w_inertia) <= 1e-9 * w_inertia


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LLOYD_CASES))
def test_kmeans_lloyd_against_the_restatement_at_the_k_D_and_N_edges(name):
    X, init = lloyd_input(name)
    want = lloyd_expected(name)
    assert lloyd_guard(name, X, init, want) is None
    compare_lloyd(name, abi_lloyd(X, init), want[:4] + (want[5],))
    if name in TIES:
        compare_lloyd(name + ", max_iter = 1", abi_lloyd(X, init, max_iter=1), first_iteration(X, init)[0])


# ===================================================================================================== 2. several empty clusters
def empty_case_guard(name):
    c = g20(name)
    copies = not name.startswith("far")
    rel = []
    labels, centres, inertia, n_iter, margin, max_empty = lloyd_restated(c.X, c.init, ignore_copies=copies, relocations=rel)
    return c, rel, margin, max_empty


@pytest.mark.parametrize("name", EMPTY_CASES)
def test_empty_cluster_inputs_meet_the_conditions_the_gpu_tests_lean_on(name):
    """(That the restatement reproduces the recorded scikit-learn run is test_restatement_reproduces_scikit_learn_on_g20.)"""
    c, rel, margin, max_empty = empty_case_guard(name)
    m = int(c.m)
    it, empty, far, donors, own = rel[0]
    assert max_empty == int(c.max_empty) >= 2 and it == 0 and len(empty) == max_empty, "the clusters are empty together, in iteration 1"
    assert margin >= MARGIN_BAND                         # (copies of a centre left out: there the tie is the case)
    assert relocation_gap(c.X, rel) >= RELOC_BAND and float(c.reloc_gap) >= RELOC_BAND
    k = len(c.init)
    assert k == 12 or (empty.min() < 128 <= empty.max()), "empty clusters on both sides of the second centre block"
    one, margin_one = first_iteration(c.X, c.init)
    assert margin_one >= MARGIN_BAND and one[3] == 1 and one[4] == max_empty
    if name.startswith("copies"):
        assert len(empty) == m - 1 and all(np.array_equal(c.init[e], c.init[empty[0]]) for e in empty)
        assert np.flatnonzero((c.init == c.init[empty[0]]).all(1)).min() < empty.min(), "the copy that keeps the rows is the lowest"
    else:
        assert len(empty) == m and donors[0] == donors[1], "two relocations draw from one donor"
        twins = np.array_equal(c.X[far[0]], c.X[far[1]])
        assert twins == (name == "twins_k12") and (not twins or far[0] < far[1]), "the lower of two copies goes to the lower empty cluster"
        assert m == 2 or len(set(donors.tolist())) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", EMPTY_CASES)
def test_kmeans_lloyd_with_several_clusters_empty_at_once_matches_scikit_learn(name):
    c = g20(name)
    compare_lloyd(name, abi_lloyd(c.X, c.init), (c.labels, c.centers, float(c.inertia), int(c.n_iter), int(c.max_empty)))
    one, margin = first_iteration(c.X, c.init)
    assert margin >= MARGIN_BAND
    compare_lloyd(name + ", max_iter = 1", abi_lloyd(c.X, c.init, max_iter=1), one)


# ===================================================================================================== 3. seeding
SEED_N = ("k", 700, 1023, 1024, 1025, 2047, 2049, 5000)
SEED_DK = [(D, k) for D in (1, 33, 65) for k in (2, 40)]


def seed_input(D, k, N):
    N = k if N == "k" else N
    rng = np.random.default_rng([6000, D, k, N])
    return rng.normal(size=(N, D)), np.ascontiguousarray(rng.random(k))


def seed_exact_cases():
    """name -> (X, u, the rows in closed form).  Every running sum is a sum of zeros or of small integers: exact in any order, so the
    guard on the distance to a running-sum boundary is not needed (and, the target of 0 lying ON one, could not hold)."""
    out = {}
    for N in (700, 2049):
        rng = np.random.default_rng([6100, N])
        X = rng.integers(-4, 5, size=(N, 3)).astype(np.float64)
        X[5] = X[0] + 1.0
        X[:5] = X[0]
        out[f"target0-N{N}"] = (X, np.array([0.0, 0.0]), [0, 5])               # rows 0 .. 4 are the seed: the first running sum above 0 is row 5's
        Y = np.tile(rng.normal(size=(1, 33)), (N, 1))
        out[f"copies-N{N}"] = (Y, np.array([0.3, 0.5, 0.0]), [int(0.3 * N), N - 1, N - 1])
        Z = np.zeros((N, 1))
        ones = np.sort(rng.choice(np.arange(1, N - 40), 64, replace=False))     # 64 rows at distance 1 of the seed (row 0), 40 or more zeros behind the last
        Z[ones, 0] = rng.choice([-1.0, 1.0], 64)
        out[f"below1-N{N}"] = (Z, np.array([0.0, np.nextafter(1.0, 0.0)]), [0, int(ones[-1])])
    return out


@pytest.mark.parametrize("D,k", SEED_DK)
def test_seed_sweep_inputs_meet_the_conditions_the_gpu_tests_lean_on(D, k):
    for N in SEED_N:
        X, u = seed_input(D, k, N)
        rows, clear = seed_restated(X, u)
        assert clear >= SEED_CLEAR, (N, clear)
        assert len(set(rows.tolist())) == k


def test_seed_exact_cases_are_what_their_names_say():
    for name, (X, u, want) in seed_exact_cases().items():
        rows, _ = seed_restated(X, u)
        assert rows.tolist() == want, name
        assert np.array_equal(X, np.round(X)) or name.startswith("copies")
        if name.startswith("below1"):
            total = float(((X - X[0]) ** 2).sum())
            assert total == 64.0 and u[1] * total == np.nextafter(64.0, 0.0) and want[1] < len(X) - 40       # not the N - 1 of the exits


def abi_seed(X, u):
    from tscode_amd import _lib
    from tscode_amd.engine import get_engine
    eng = get_engine()
    X, u = np.ascontiguousarray(X), np.ascontiguousarray(u)
    rows = np.empty(len(u), np.int32)
    _lib.check(eng.lib.tsc_kmeans_seed(eng._h, _lib.ptr(X), C.c_int64(len(X)), C.c_int64(X.shape[1]), C.c_int(len(u)), _lib.ptr(u), _lib.ptr(rows)))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", SEED_DK)
def test_kmeans_seed_against_the_restatement(D, k):
    for N in SEED_N:
        X, u = seed_input(D, k, N)
        want, clear = seed_restated(X, u)
        assert clear >= SEED_CLEAR
        rows = abi_seed(X, u)
        print(f"D {D}, k {k}, N {len(X)}: rows differing {int((rows != want).sum())}, clear {clear:.1e}")
        assert np.array_equal(rows, want), (D, k, N)


@pytest.mark.gpu
def test_kmeans_seed_exact_cases():
    for name, (X, u, want) in seed_exact_cases().items():
        rows = abi_seed(X, u)
        print(f"{name}: rows {rows.tolist()}, want {want}")
        assert rows.tolist() == want, name


# ===================================================================================================== 4. the pick
PICK_CASES = ("k2-3+40", "k300-n1", "k5-n63", "k5-n64", "k5-n65", "k5-n200", "big", "empty", "tie-copies", "tie-e-3-300", "tie-e-70-130")


@functools.lru_cache(maxsize=None)
def pick_input(name):
    """(aligned f64[N, n, 3], labels i32[N], centres f64[k, n, 3], energies f64[N], the tie: (cluster, winning position, other position,
    with energies?) or None).  Labels and centres are made up: the pick takes them as they come."""
    rng = np.random.default_rng([7000, PICK_CASES.index(name)])
    tie = None
    if name == "k2-3+40":
        n, counts = 7, [3, 40]
    elif name == "k300-n1":
        n, counts = 1, [3] * 300
    elif name.startswith("k5-n"):
        n, counts = int(name[4:]), [12] * 5
    elif name == "empty":
        n, counts = 5, [20, 13, 0, 17]
    elif name == "tie-copies":
        n, counts = 6, [10, 20]
    else:
        n, counts = 4, [257, 600, 20]
    k, N = len(counts), sum(counts)
    labels = rng.permutation(np.repeat(np.arange(k), counts)).astype(np.int32)
    aligned = rng.normal(size=(N, n, 3))
    centres = rng.normal(size=(k, n, 3))
    energies = rng.normal(size=N)
    if name == "k2-3+40":                                # the winner of cluster 1 at position 17 >= k: no centre is left out of its sum
        aligned[np.flatnonzero(labels == 1)[17]] *= 3.0
    if name == "big":                                    # the lowest energy of cluster 1 at position 400: the second trip of the 256 stride
        energies[np.flatnonzero(labels == 1)[400]] = -10.0
    if name == "tie-copies":                             # positions 6 (wavefront 2) and 9 (wavefront 1) of cluster 1, both >= k, both the farthest out
        tie = (1, 6, 9, False)
        members = np.flatnonzero(labels == 1)
        aligned[members[6]] *= 10.0
        aligned[members[9]] = aligned[members[6]]
    elif name.startswith("tie-e"):
        cl, a, b = (1, 3, 300) if name == "tie-e-3-300" else (0, 70, 130)
        tie = (cl, a, b, True)
        members = np.flatnonzero(labels == cl)
        energies[members[a]] = energies[members[b]] = -50.0
    return aligned, labels, centres, energies, tie


@pytest.mark.parametrize("name", PICK_CASES)
def test_pick_sweep_inputs_meet_the_conditions_the_gpu_tests_lean_on(name):
    aligned, labels, centres, energies, tie = pick_input(name)
    k = len(centres)
    counts = np.bincount(labels, minlength=k)
    picked_d, gap_d = pick_restated(aligned, labels, centres)
    picked_e, _ = pick_restated(aligned, labels, centres, energies)
    assert gap_d >= PICK_BAND, gap_d
    for cl in range(k):                                  # energies inside a cluster: distinct by the band, or equal to the bit (the tie cases)
        d = np.diff(np.sort(energies[labels == cl]))
        assert ((d >= ENERGY_BAND) | (d == 0.0)).all() and (d == 0.0).sum() == (1 if tie and tie[3] and tie[0] == cl else 0)
    assert ((picked_d >= 0) == (counts > 0)).all() and ((picked_e >= 0) == (counts > 0)).all()
    if name == "k2-3+40":
        assert counts.tolist() == [3, 40] and np.flatnonzero(labels == 1).tolist().index(picked_d[1]) == 17, "the winner's position leaves no centre out"
    if name == "big":
        assert counts.tolist() == [257, 600, 20]
        assert np.flatnonzero(labels == 1).tolist().index(picked_e[1]) == 400, "the lowest energy is found on a later trip of the stride"
    if name == "empty":
        assert picked_d[2] == picked_e[2] == -1
    if tie:
        cl, a, b, with_energies = tie
        members = np.flatnonzero(labels == cl)
        assert (picked_e if with_energies else picked_d)[cl] == members[a] and a < b
        if with_energies:
            assert energies[members[a]] == energies[members[b]] == energies[members].min()
        else:
            assert np.array_equal(aligned[members[a]], aligned[members[b]]) and min(a, b) >= k and a % 4 > b % 4      # the later wavefront wins


def abi_pick(aligned, labels, centres, energies):
    from tscode_amd import _lib
    from tscode_amd.engine import get_engine
    eng = get_engine()
    aligned, labels, centres = np.ascontiguousarray(aligned), np.ascontiguousarray(labels, dtype=np.int32), np.ascontiguousarray(centres)
    picked = np.empty(len(centres), np.int32)
    _lib.check(eng.lib.tsc_diverse_pick(eng._h, _lib.ptr(aligned), C.c_int64(len(aligned)), C.c_int(aligned.shape[1]), _lib.ptr(labels), _lib.ptr(centres),
                                        C.c_int(len(centres)), _lib.ptr(None if energies is None else np.ascontiguousarray(energies)), _lib.ptr(picked)))
    return picked


@pytest.mark.gpu
@pytest.mark.parametrize("name", PICK_CASES)
def test_tsc_diverse_pick_against_the_restatement(name):
    aligned, labels, centres, energies, tie = pick_input(name)
    for e in (None, energies):
        want, gap = pick_restated(aligned, labels, centres, e)
        assert e is not None or gap >= PICK_BAND
        picked = abi_pick(aligned, labels, centres, e)
        print(f"{name} ({'energies' if e is not None else 'cumdist'}): picks differing {int((picked != want).sum())} of {len(want)}, gap {gap:.1e}")
        assert np.array_equal(picked, want)


# ===================================================================================================== 5. alignment
FAMILY_GAPS = (3e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 3e-6, 3e-8, 3e-10, 0.0)      # (about three times the relative Horn gap they give)
# name: (atoms, structures, family, index set).  "coords": every target's Horn gap is inside the band; "props": none is asked to be
ALIGN_COORDS = {
    "a3-noisy": (3, 4, "noisy", None), "a4-noisy-N1": (4, 1, "noisy", None), "a4-noisy-N2": (4, 2, "noisy", None), "a63-unrelated": (63, 4, "unrelated", None),
    "a64-mirror": (64, 5, "mirror", None), "a64-planar": (64, 9, "planar", None), "a65-far": (65, 9, "far", None), "a512-unrelated": (512, 5, "unrelated", None),
    "a512-mirror": (512, 2, "mirror", None), "a65-idx3": (65, 4, "noisy", "sorted3"), "a512-idx64": (512, 5, "noisy", "sorted64"),
    "a512-idx65": (512, 4, "unrelated", "sorted65"), "a65-unsorted": (65, 5, "mirror", "unsorted20"), "a20-repeat": (20, 9, "noisy", "repeat"),
}
ALIGN_PROPS = {
    "a1": (1, 4, "unrelated", None), "a2": (2, 5, "unrelated", None), "a9-one-atom": (9, 4, "unrelated", "single"), "a9-line-idx": (9, 5, "line3", "first3"),
    "a64-line": (64, 5, "line", None), "mirror-family": (16, 1 + len(FAMILY_GAPS), "mirror-family", None),
    "squeeze-family": (8, 1 + len(FAMILY_GAPS), "squeeze-family", None),
}
ALIGN_CASES = {**ALIGN_COORDS, **ALIGN_PROPS}


@functools.lru_cache(maxsize=None)
def align_input(name):
    n, N, family, index = ALIGN_CASES[name]
    rng = np.random.default_rng([8000, list(ALIGN_CASES).index(name)])
    ref = 2.0 * rng.normal(size=(n, 3))
    if family == "noisy":
        s = ref + 0.1 * rng.normal(size=(N, n, 3))
    elif family == "unrelated":
        s = 2.0 * rng.normal(size=(N, n, 3))
    elif family == "mirror":                             # the reference seen in a mirror, plus noise: det S < 0
        s = ref * np.array([1.0, 1.0, -1.0]) + 0.1 * rng.normal(size=(N, n, 3))
        s[0] = ref
    elif family == "planar":
        ref[:, 2] = 0.0
        s = ref + 0.1 * rng.normal(size=(N, n, 3)) * np.array([1.0, 1.0, 0.0])
    elif family == "far":
        s = ref + 0.1 * rng.normal(size=(N, n, 3)) + 1000.0 * rng.normal(size=(N, 1, 3))
    elif family == "line":                               # every atom on one line
        s = rng.normal(size=(N, n, 1)) * np.array([1.0, 0.0, 0.0])
    elif family == "line3":                              # the three indexed atoms on a line, the rest anywhere
        s = 2.0 * rng.normal(size=(N, n, 3))
        s[:, :3] = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.5, 0, 0]]) + rng.normal(size=(N, 1, 3))
    elif family == "mirror-family":                      # the box (+-2, +-b, +-1) and its half, against the box with b = 1 seen in the mirror z -> -z:
        # S = 10 diag(4, b, -1), det S < 0, and the gap of Horn's top eigenvalues is 2 (sigma_2 - sigma_3) = 20 (b - 1)
        signs = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
        box = lambda b: np.concatenate([signs * np.array([2.0, b, 1.0]), 0.5 * signs * np.array([2.0, b, 1.0])])     # noqa: E731
        s = np.stack([box(1.0)] + [box(1.0 + g) * np.array([1.0, 1.0, -1.0]) for g in FAMILY_GAPS])
    else:                                                # a rectangle (+-2, +-y) squeezed onto a line: planar, the gap 2 sigma_2 ~ y
        assert family == "squeeze-family"
        signs = np.array([[x, y, 0] for x in (-1, 1) for y in (-1, 1)], dtype=np.float64)
        box = lambda y: np.concatenate([signs * np.array([2.0, y, 0.0]), 0.5 * signs * np.array([2.0, y, 0.0])])     # noqa: E731
        s = np.stack([box(1.0)] + [box(g) for g in FAMILY_GAPS])
    s = moved(np.ascontiguousarray(s), 8000 + len(name))
    if index is None:
        return s, None
    if index.startswith("sorted"):
        idx = np.sort(rng.choice(n, int(index[6:]), replace=False))
    else:
        idx = {"unsorted20": rng.permutation(n)[:20], "single": np.array([4]), "first3": np.arange(3), "repeat": np.array([7, 2, 11, 2, 15, 0, 7, 19])}[index]
    return s, idx.astype(np.int32)


def horn(s, idx):
    """Per target t >= 1, over the indexed atoms of the centred structures: (relative gap of the two largest eigenvalues of Horn's matrix
    over (Gp + Gq) / 2, Gp + Gq, the largest eigenvalue, the ratio the device's fast path tests against 1e-4)."""
    sel = np.arange(s.shape[1]) if idx is None else idx
    c = s - s[:, sel].mean(axis=1, keepdims=True)
    q = c[0][sel]
    out = []
    for t in range(1, len(s)):
        p = c[t][sel]
        S = p.T @ q
        M = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                      [0, S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                      [0, 0, -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                      [0, 0, 0, -S[0, 0] - S[1, 1] + S[2, 2]]])
        M = M + np.triu(M, 1).T
        ev = np.linalg.eigvalsh(M)
        G = float((p * p).sum() + (q * q).sum())
        # what rotation_quaternion_fast (pair_math.hpp) tests before it trusts the adjugate of A = M - lambda_max I: best / scale^3 > 1e-4
        A = M - ev[-1] * np.eye(4)
        best = max(abs(np.linalg.det(np.delete(np.delete(A, i, 0), i, 1))) for i in range(4))
        ratio = best / np.abs(A).max() ** 3 if np.abs(A).max() > 0.0 else 0.0
        out.append((float(ev[-1] - ev[-2]) / (0.5 * G) if G > 0.0 else 0.0, G, float(ev[-1]), ratio))
    return out


def from_optimum(out, s, idx):
    """Per target: |residual over the indexed atoms - (Gp + Gq - 2 lambda_max)| / (Gp + Gq); 0 where Gp + Gq == 0 == residual."""
    sel = np.arange(s.shape[1]) if idx is None else idx
    ref = (s[0] - s[0][sel].mean(axis=0))[sel]
    worst = []
    for t, (gap, G, lam, _) in enumerate(horn(s, idx), start=1):
        resid = float(((out[t][sel] - ref) ** 2).sum())
        worst.append(abs(resid - (G - 2.0 * lam)) / G if G > 0.0 else (0.0 if resid == 0.0 else np.inf))
    return worst


def assert_proper_rotation(out, s, idx, what):
    """out[t] is the centred s[t] turned by a proper rotation: for a structure that spans space, the map between them is orthogonal to 1e-9
    with a positive determinant (as test_align_structures_on_a_collinear_index_set_is_finite_and_proper has it); a flat or thinner
    structure has no handedness, and every distance is kept."""
    sel = np.arange(s.shape[1]) if idx is None else idx
    cen = s - s[:, sel].mean(axis=1, keepdims=True)
    for t in range(1, len(s)):
        sv = np.linalg.svd(cen[t], compute_uv=False)
        if len(sv) == 3 and sv[2] > 1e-6 * sv[0]:
            R, *_ = np.linalg.lstsq(cen[t], out[t], rcond=None)
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0.0, (what, t)
        else:
            assert np.abs(out[t] @ out[t].T - cen[t] @ cen[t].T).max() <= 1e-9 * max(1.0, float((cen[t] ** 2).sum(1).max())), (what, t)


@pytest.mark.parametrize("name", list(ALIGN_CASES))
def test_align_sweep_inputs_meet_the_conditions_the_gpu_tests_lean_on(name):
    s, idx = align_input(name)
    n, N, family, index = ALIGN_CASES[name]
    assert s.shape == (N, n, 3) and (idx is None) == (index is None)
    gaps = [g for g, *_ in horn(s, idx)]
    want = kabsch_align_numpy(s, idx)
    if name in ALIGN_COORDS:
        assert N == 1 or min(gaps) >= HORN_BAND, min(gaps)
        if family == "mirror":                           # the best orthogonal map is a reflection: the sign fix is what makes the answer proper
            sel = np.arange(n) if idx is None else idx
            c = s - s[:, sel].mean(axis=1, keepdims=True)
            assert all(np.linalg.det(c[t][sel].T @ c[0][sel]) < 0.0 for t in range(1, N))
        if index == "repeat":
            assert len(set(idx.tolist())) < len(idx)
        if index and index.startswith("unsorted"):
            assert (np.diff(idx) < 0).any()
    else:
        if name.endswith("family"):                      # the gap walks down through the hand-over to the Jacobi solver, to 0
            assert len(gaps) == len(FAMILY_GAPS) and (np.diff(gaps) < 0).all() and gaps[-1] < 1e-13
            assert all(0.1 * g <= got <= 10 * g for g, got in zip(FAMILY_GAPS[:-1], gaps[:-1])), gaps
            ratios = [r for *_, r in horn(s, idx)]           # members on either side of the hand-over at 1e-4, by a factor of two and more
            assert sum(r > 2e-4 for r in ratios) >= 2 and sum(r < 5e-5 for r in ratios) >= 2 and sum(0.0 < r < 5e-5 for r in ratios) >= 1, ratios
        else:
            assert max(gaps) < HORN_BAND, max(gaps)
        assert_proper_rotation(want, s, idx, name)       # the check itself, on an answer known to be a proper rotation
    measured = max(from_optimum(want, s, idx), default=0.0)
    assert measured <= SVD_FROM_OPTIMUM, f"numpy's SVD route lies {measured:.2e} (Gp + Gq) from the optimum: the module docstring's figure is too small"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ALIGN_CASES))
def test_align_structures_against_numpy_or_the_optimum(name):
    import tscode_amd
    s, idx = align_input(name)
    work = s.copy()
    out = tscode_amd.align_structures(work, None if idx is None else idx.tolist())
    sel = np.arange(s.shape[1]) if idx is None else idx
    centred = s - s[:, sel].mean(axis=1, keepdims=True)
    gaps = [g for g, *_ in horn(s, idx)]
    off = max(from_optimum(out, s, idx), default=0.0)
    assert out.shape == s.shape and np.isfinite(out).all()
    assert np.abs(out[0] - centred[0]).max() <= COORD_TOL
    assert np.abs(work - centred).max() <= COORD_TOL, "the caller's array is left centred by the reference (:53-55)"
    if name in ALIGN_COORDS:
        assert len(s) == 1 or min(gaps) >= HORN_BAND
        want = kabsch_align_numpy(s, idx)
        print(f"{name}: |out - numpy Kabsch| = {np.abs(out - want).max():.3e}, from the optimum {off:.2e} (Gp + Gq), smallest gap {min(gaps, default=np.inf):.1e}")
        assert np.abs(out - want).max() <= COORD_TOL
    else:
        print(f"{name}: from the optimum {off:.2e} (Gp + Gq) per target {['%.1e' % v for v in from_optimum(out, s, idx)]}, gaps {['%.1e' % g for g in gaps]}")
        assert_proper_rotation(out, s, idx, name)
    assert off <= OPTIMUM_TOL


# ===================================================================================================== 6. end to end beyond k = 128
SELECT_SEED = 9005


@functools.lru_cache(maxsize=None)
def select_input(seed=SELECT_SEED):
    from tscode_amd.synthetic import make_ensemble
    s = moved(make_ensemble(600, (5, 6), seed=seed, children=7).poses(), seed)
    rows = np.random.default_rng(seed).choice(600, 129, replace=False).astype(np.int32)
    return np.ascontiguousarray(s), rows


@functools.lru_cache(maxsize=None)
def select_expected(seed=SELECT_SEED):
    s, rows = select_input(seed)
    aligned = kabsch_align_numpy(s)
    X = aligned.reshape(len(s), -1)
    labels, centres, inertia, n_iter, margin, max_empty = lloyd_restated(X, X[rows])
    picked, gap = pick_restated(aligned, labels, centres)
    return aligned, labels, n_iter, picked, margin, max_empty, gap


def test_select_input_meets_the_conditions_the_gpu_test_leans_on():
    s, rows = select_input()
    aligned, labels, n_iter, picked, margin, max_empty, gap = select_expected()
    assert s.shape == (600, 11, 3) and len(set(rows.tolist())) == 129
    assert min(g for g, *_ in horn(s, None)) >= HORN_BAND
    assert margin >= MARGIN_BAND and gap >= PICK_BAND and max_empty == 0 and n_iter >= 2
    assert (picked >= 0).all() and np.array_equal(labels[picked], np.arange(129))
    assert np.bincount(labels, minlength=129).min() >= 1 and np.bincount(labels).max() >= 2


@pytest.mark.gpu
def test_diverse_select_k129_against_the_three_restatements_and_inside_a_batch():
    import tscode_amd
    s, rows = select_input()
    w_aligned, w_labels, w_iter, w_picked, margin, _, gap = select_expected()
    assert margin >= MARGIN_BAND and gap >= PICK_BAND
    aligned, labels, picked, got_rows, n_iter = tscode_amd.diverse_select(s, 129, init_rows=rows)
    print(f"k = 129: |aligned - numpy Kabsch| = {np.abs(aligned - w_aligned).max():.3e}, n_iter {n_iter} (want {w_iter}), "
          f"labels differing {int((labels != w_labels).sum())}, picks differing {int((picked != w_picked).sum())}")
    assert np.abs(aligned - w_aligned).max() <= COORD_TOL
    assert np.array_equal(labels, w_labels) and n_iter == w_iter and np.array_equal(got_rows, rows)
    assert np.array_equal(picked, w_picked)
    rng = np.random.default_rng(9002)
    before, after = rng.normal(size=(20, 10, 3)), rng.normal(size=(30, 4, 3))
    batch = tscode_amd.diverse_select_batch([before, s, after], [3, 129, 2], init_rows=[np.array([0, 7, 19], np.int32), rows, np.array([4, 5], np.int32)])
    for name, a, b in zip(("aligned", "labels", "picked", "init_rows"), batch[1][:4], (aligned, labels, picked, got_rows)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"the middle segment's {name} differ from the single call's bits"
    assert batch[1][4] == n_iter
