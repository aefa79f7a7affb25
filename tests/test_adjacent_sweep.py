"""Shape sweeps of the "adjacent row" kernels (tscode_amd/csrc/tfd_kernels.hpp, moi_kernels.hpp, launched from adjacent.hip) at the sizes and edges the
fixture tests do not reach: grid-stride loops past one pass of the grid, clamped chunk geometries, first hits many 64-column steps
away, degenerate inertia tensors, signed and non-finite denominators.

Two references: the C oracle (oracle/) and plain numpy restatements written here, in np.longdouble where values are compared.
Every input comes from np.random.default_rng(seed); the unmarked guard test at the end regenerates all of them and checks, with the
oracle alone, the conditions the GPU tests lean on (margins, far-hit counts, excluded shares, the expected vectors of the edge
cases), so that a seed that drifts shows up without a GPU.
"""

import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

VAL_TOL = 1e-9          # the tolerance of test_gpu_parity.py for rotated coordinates
EPS = 2.0 ** -52
GRID_ROWS = 4096 * 4    # k_tfd_first_similar / k_moi_first_similar: 4096 workgroups of 4 wavefronts, one row per wavefront and pass
GRID_ELEMS = 2048 * 256 # the one-thread-per-element kernels: 2048 workgroups of 256 threads per pass


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def _rotations(rng, n):
    """n proper rotation matrices (QR of a normal matrix, signs fixed)."""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return q


# ===================================================================================================== 1. tfd_first_similar
def clustered_fingerprints(rng, n, T, n_par, noise):
    """As test_tfd_greedy_filter_vs_oracle builds them: parents uniform in +-180, children = parent + N(0, noise), wrapped, float32."""
    parents = rng.uniform(-180, 180, size=(n_par, T))
    tf = (parents[rng.integers(0, n_par, size=n)] + rng.normal(size=(n, T)) * noise).astype(np.float32)
    return ((tf + 180) % 360 - 180).astype(np.float32)


def tfd_similar_restated(a, b, thresh):
    """tfd_similarity: float32 difference, float64 after the wrap; the sum in long double (exact for these lengths)."""
    d32 = np.abs(a - b)
    assert d32.dtype == np.float32
    dd = np.abs(d32.astype(np.float64) - (d32 > np.float32(180.0)) * 360.0)
    total = np.longdouble(0)
    for x in dd:
        total += np.longdouble(x)
    return bool(total < np.longdouble(thresh))


def tfd_first_restated(tf, d, k, num_active, thresh):
    """The literal triple loop: chunk s is [d s, d s + d), the last chunk ends at num_active, rows outside every chunk give -1."""
    first = np.full(len(tf), -1, dtype=np.int32)
    for s in range(k):
        lo = d * s
        hi = num_active if s == k - 1 else lo + d
        for i in range(lo, hi):
            for j in range(i + 1, hi):
                if tfd_similar_restated(tf[i], tf[j], thresh):
                    first[i] = j
                    break
    return first


TFD_GEOMETRIES = [(10, 5, 50), (10, 5, 47), (10, 4, 50), (10, 5, 35), (10, 5, 40), (7, 7, 49), (1, 50, 50), (50, 1, 0)]


def tfd_small_input():
    return clustered_fingerprints(np.random.default_rng(101), 50, 3, 6, 0.8)


TFD_T_SWEEP = [0, 1, 2, 8, 9, 40]


def tfd_t_input(T):
    """n = 700 in three chunks, the last one cut short; the noise shrinks with T so that siblings stay near the threshold of 10."""
    n = 700
    tf = clustered_fingerprints(np.random.default_rng(200 + T), n, T, 90, min(0.8, 8.0 / max(T, 1)))
    return tf, (n // 3, 3, n - 5)


def tfd_stride_input():
    n = 20_000
    tf = clustered_fingerprints(np.random.default_rng(0), n, 6, 3000, 0.8)
    return tf, [(n, 1, n), (n // 7, 7, n - 5), (n // 3, 3, n // 2)]


TFD_EDGE = np.array([[0, 0], [180, 0], [180.00002, 0], [-179.99998, 0.5], [np.nan, 0], [0, 0]], dtype=np.float32)
TFD_EDGE_EXPECTED = {1.0: [5, 2, 3, -1, -1, -1], 10.0: [5, 2, 3, -1, -1, -1], 180.00001: [1, 2, 3, -1, -1, -1], 181.0: [1, 2, 3, 5, -1, -1]}


def far_hits(first, columns=64):
    """Hits more than `columns` columns away: the ballot loop of their row took more than one step."""
    return int(((first >= 0) & (first - np.arange(len(first)) > columns)).sum())


@pytest.mark.gpu
def test_tfd_first_similar_chunk_geometries(eng, oracle):
    """d k < n, num_active < d (k - 1) (the negative length clamped to 0), num_active == n, one-row chunks, an empty pass."""
    tf = tfd_small_input()
    for d, k, na in TFD_GEOMETRIES:
        want = tfd_first_restated(tf, d, k, na, 10.0)
        ref, margin = oracle.tfd_first_similar(tf, d, k, na, 10.0, return_margin=True)
        assert margin > 1e-6
        got = eng.tfd_first_similar(tf, d, k, na, 10.0)
        assert np.array_equal(ref, want) and np.array_equal(got, want), (d, k, na, got.tolist(), want.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("T", TFD_T_SWEEP)
def test_tfd_first_similar_fingerprint_lengths(eng, oracle, T):
    tf, (d, k, na) = tfd_t_input(T)
    ref, margin = oracle.tfd_first_similar(tf, d, k, na, 10.0, return_margin=True)
    assert margin > 1e-6
    got = eng.tfd_first_similar(tf, d, k, na, 10.0)
    assert np.array_equal(got, ref), (T, int((got != ref).sum()))
    if T == 0:                                              # an empty sum is 0 < thresh: every row matches the next one of its chunk
        want = np.arange(1, len(tf) + 1, dtype=np.int32)
        want[[d - 1, 2 * d - 1]] = -1
        want[na - 1:] = -1
        assert np.array_equal(got, want)


@pytest.mark.gpu
def test_tfd_first_similar_far_columns_and_grid_stride(eng, oracle):
    """20 000 rows: rows >= 16 384 are the second pass of the grid-stride loop; thousands of first hits lie several 64-column steps away."""
    tf, passes = tfd_stride_input()
    assert len(tf) > GRID_ROWS
    for d, k, na in passes:
        ref, margin = oracle.tfd_first_similar(tf, d, k, na, 10.0, return_margin=True)
        assert margin > 1e-6 and far_hits(ref) > 1000, (d, k, na, margin, far_hits(ref))
        got = eng.tfd_first_similar(tf, d, k, na, 10.0)
        assert np.array_equal(got[GRID_ROWS:], ref[GRID_ROWS:]), (d, k, na, "second pass of the grid")
        assert np.array_equal(got, ref), (d, k, na)


@pytest.mark.gpu
def test_tfd_first_similar_wrap_boundary_and_nan(eng, oracle):
    """|difference| of exactly 180, one float32 above it, and a NaN row (it neither finds a match nor is found)."""
    for thresh, want in TFD_EDGE_EXPECTED.items():
        assert eng.tfd_first_similar(TFD_EDGE, 6, 1, 6, thresh).tolist() == want, thresh
        assert oracle.tfd_first_similar(TFD_EDGE, 6, 1, 6, thresh).tolist() == want
        assert tfd_first_restated(TFD_EDGE, 6, 1, 6, thresh).tolist() == want


# ===================================================================================================== 2. torsion_fingerprints
TIE_BAND = 1e-9     # degrees.  Device and host do the same operations with contraction off and differ only in atan2 and sqrt: a few fp64
                    # ulps at 180 degrees, about 1e-13 degrees; a cancellation error (coordinates far from the origin) is common to both.
TORSION_CASES = [(30_011, 24, 20, 2.0, 0.0), (9_001, 60, 64, 3.0, 500.0)]       # N, atoms, T, scale, offset: N T > 524 288 in both


def torsion_input(case):
    N, atoms, T, scale, offset = TORSION_CASES[case]
    rng = np.random.default_rng(300 + case)
    quads = np.array([rng.permutation(atoms)[:4] for _ in range(T)], dtype=np.int32)
    return rng.normal(size=(N, atoms, 3)) * scale + offset, quads


def torsion_angles_f64(oracle, structures, quads):
    s = np.ascontiguousarray(structures, dtype=np.float64)
    q = np.ascontiguousarray(quads, dtype=np.int32).reshape(-1, 4)
    out = np.empty((len(s), len(q)))
    fn = oracle.lib().orc_torsion_angles_f64
    fn.restype = None
    fn(s.ctypes.data_as(C.c_void_p), C.c_int64(len(s)), C.c_int(s.shape[1]), q.ctypes.data_as(C.c_void_p), C.c_int(len(q)), out.ctypes.data_as(C.c_void_p))
    return out


def tie_distance(angles):
    """Per element: the distance (degrees) of the fp64 angle from the nearest float32 rounding tie (oracle.torsion_rounding_margin, not reduced)."""
    f = angles.astype(np.float32)
    f64 = f.astype(np.float64)
    lo = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    hi = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    return np.minimum(np.abs((lo + f64) / 2 - angles), np.abs((hi + f64) / 2 - angles))


def assert_float32_of_the_same_angle(got, ref, angles, what):
    """Bit-equal where the fp64 angle is TIE_BAND or more from a rounding tie, at most one float32 ulp apart elsewhere."""
    decidable = tie_distance(angles) >= TIE_BAND
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    assert same[decidable].all(), (what, int((~same & decidable).sum()), "elements differ outside the tie band")
    one_ulp = (got == np.nextafter(ref, np.float32(np.inf))) | (got == np.nextafter(ref, np.float32(-np.inf)))
    assert (same | one_ulp).all(), (what, "an element inside the tie band is more than one ulp off")
    return 1.0 - decidable.mean()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(TORSION_CASES)))
def test_torsion_fingerprints_bit_equal_outside_the_tie_band(eng, oracle, case):
    structures, quads = torsion_input(case)
    assert structures.shape[0] * len(quads) > GRID_ELEMS
    ref = oracle.torsion_fingerprints(structures, quads)
    got = eng.torsion_fingerprints(structures, quads)
    assert got.dtype == np.float32 and got.shape == ref.shape
    left_out = assert_float32_of_the_same_angle(got, ref, torsion_angles_f64(oracle, structures, quads), TORSION_CASES[case])
    assert left_out < 0.01, left_out


def torsion_degenerate_input():
    """Rows: collinear, p1 == p2, planar cis, planar trans.  The last quadruplet repeats an atom."""
    s = np.zeros((4, 6, 3))
    s[0, :, 0] = [0, 1, 2, 3, 4.5, 6]                                               # all on the x axis
    s[1] = [[0, 1, 0], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [1, 1, 0.4], [-1, 0.5, 2], [2, -1, 0.7]]       # atoms 1 and 2 coincide
    s[2] = [[0, 1, 0], [0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 2, 0], [3, 1, 0]]         # 0-1-2-3 cis
    s[3] = [[0, 1, 0], [0, 0, 0], [1, 0, 0], [1, -1, 0], [2, 2, 0], [3, 1, 0]]        # 0-1-2-3 trans
    quads = np.array([[0, 1, 2, 3], [4, 1, 2, 5], [0, 1, 3, 4], [0, 1, 2, 0]], dtype=np.int32)
    return s, quads


def check_torsion_degenerate_values(fp):
    assert np.array_equal(fp[0], np.zeros(4, np.float32))                            # collinear: atan2(0, 0)
    assert np.isnan(fp[1, [0, 1, 3]]).all() and np.isfinite(fp[1, 2])                 # every quadruplet over the zero-length bond, and only those
    assert fp[2, 0] == 0 and fp[3, 0] == 180
    assert fp[2, 3] == 0 and fp[3, 3] == 0                                            # a repeated atom: the first and the last arm coincide, cis


@pytest.mark.gpu
def test_torsion_fingerprints_degenerate_rows(eng, oracle):
    s, quads = torsion_degenerate_input()
    ref = oracle.torsion_fingerprints(s, quads)
    got = eng.torsion_fingerprints(s, quads)
    assert np.array_equal(got, ref, equal_nan=True), (got.tolist(), ref.tolist())
    check_torsion_degenerate_values(got)


# ===================================================================================================== 3. inertia_moments
def moments_longdouble(structures, masses):
    """Centre of mass and tensor in long double, np.linalg.eigvalsh on its float64, ordered by |value|."""
    s = np.asarray(structures, dtype=np.longdouble)
    m = np.asarray(masses, dtype=np.longdouble)
    x = s - ((s * m[None, :, None]).sum(axis=1) / m.sum())[:, None, :]
    r2 = (x * x).sum(axis=2)
    I = np.empty((len(s), 3, 3), dtype=np.longdouble)
    for i in range(3):
        for j in range(3):
            I[:, i, j] = (m[None] * ((r2 if i == j else 0) - x[:, :, i] * x[:, :, j])).sum(axis=1)
    ev = np.linalg.eigvalsh(I.astype(np.float64))
    return np.take_along_axis(ev, np.argsort(np.abs(ev), axis=1, kind="stable"), axis=1)


def moment_scale(structures, masses, ref):
    """What an error is measured against: the structure's largest |moment| -- and, for a structure whose moments all vanish (one atom),
    one ulp of its moment about the origin, below which the input coordinates themselves do not resolve a moment."""
    about_origin = (np.asarray(masses)[None, :] * (np.asarray(structures) ** 2).sum(axis=2)).sum(axis=1)
    return np.maximum(np.abs(ref).max(axis=1), EPS * about_origin)


MOI_CASES = ["random-50", "random-200", "random-1000", "shifted-1000A", "linear", "planar", "spherical-top", "symmetric-top", "one-atom", "two-atoms",
             "stride"]


def moi_input(name):
    rng = np.random.default_rng(400 + MOI_CASES.index(name))
    if name.startswith("random-"):
        N, n = {"random-50": (2000, 50), "random-200": (500, 200), "random-1000": (200, 1000)}[name]
        return rng.normal(size=(N, n, 3)) * 3, rng.uniform(1, 127, size=n)
    if name == "shifted-1000A":
        return rng.normal(size=(2000, 30, 3)) * 3 + 1000.0, rng.uniform(1, 127, size=30)
    if name == "linear":                                     # random step lengths along one random direction per structure
        direction = rng.normal(size=(100, 3))
        direction /= np.linalg.norm(direction, axis=1)[:, None]
        along = np.cumsum(rng.uniform(0.9, 1.6, size=(100, 6)), axis=1)
        return along[:, :, None] * direction[:, None, :] + rng.normal(size=(100, 1, 3)), rng.uniform(1, 127, size=6)
    if name == "planar":
        flat = rng.normal(size=(500, 12, 3)) * 2
        flat[:, :, 2] = 0
        return np.einsum("nij,naj->nai", _rotations(rng, 500), flat), rng.uniform(1, 127, size=12)
    if name == "spherical-top":                              # tetrahedral AB4
        base = np.array([[0, 0, 0], [1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) * (1.09 / np.sqrt(3))
        return np.einsum("nij,aj->nai", _rotations(rng, 200), base), np.array([12.0, 1, 1, 1, 1])
    if name == "symmetric-top":                              # AB3 with a C3 axis
        phi = np.radians([0, 120, 240])
        base = np.concatenate([[[0, 0, 0.38]], np.stack([0.94 * np.cos(phi), 0.94 * np.sin(phi), np.zeros(3)], axis=1)])
        return np.einsum("nij,aj->nai", _rotations(rng, 200), base), np.array([14.0, 1, 1, 1])
    if name == "one-atom":
        return np.array([[[1.3, -2.7, 0.4]]]), np.array([12.011])
    if name == "two-atoms":
        return rng.normal(size=(50, 2, 3)) * 2, np.array([1.008, 126.9])
    assert name == "stride"
    return rng.normal(size=(600_001, 3, 3)) * 1.5, np.array([1.0, 12.0, 16.0])


def moi_bound(oracle, structures, masses):
    """(reference, scale, the oracle's own deviation, the bound): 16 x the oracle's deviation from the long-double reference on this case --
    two backward-stable eigensolvers, two summation orders -- never below 64 ulps, never above the 1e-12 of test_moi_and_scores_golden."""
    ref = moments_longdouble(structures, masses)
    scale = moment_scale(structures, masses, ref)
    dev = float((np.abs(oracle.inertia_moments(structures, masses) - ref).max(axis=1) / scale).max())
    return ref, scale, dev, min(max(16 * dev, 64 * EPS), 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MOI_CASES)
def test_inertia_moments_against_long_double(eng, oracle, name):
    structures, masses = moi_input(name)
    ref, scale, dev, bound = moi_bound(oracle, structures, masses)
    got = eng.inertia_moments(structures, masses)
    err = np.abs(got - ref).max(axis=1) / scale
    print(f"\ninertia_moments {name}: oracle vs long double {dev:.3e}, GPU vs long double {err.max():.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all() and err.max() <= bound, (name, float(err.max()), bound, int(err.argmax()))
    assert (np.abs(got[:, 0]) <= np.abs(got[:, 1])).all() and (np.abs(got[:, 1]) <= np.abs(got[:, 2])).all()
    if name == "stride":
        assert len(structures) > GRID_ELEMS and err[GRID_ELEMS:].max() <= bound
    if name == "planar":                                     # the perpendicular-axis theorem
        assert (np.abs(got[:, 2] - got[:, 0] - got[:, 1]) / scale).max() <= bound
    if name in ("linear", "two-atoms"):                      # the moment about the axis vanishes; its sign is Jacobi's business
        assert (np.abs(got[:, 0]) / scale).max() < bound


# ===================================================================================================== 4. moi_first_similar
MOI_EDGE = np.array([[0, 5, 5], [0, 5, 5], [-1e-16, 5, 5], [1e-16, 5, 5], [-1e-16, 5.01, 5.01], [3, 4, 5], [np.inf, 4, 5], [3, 4, 5.0001],
                     [np.nan, 4, 5], [3, 4, 5]])
MOI_EDGE_EXPECTED = [-1, -1, 3, -1, -1, 7, -1, 9, -1, -1]      # the negative denominator makes row 2 match row 3, as in the reference


def moi_first_restated(mo, dev):
    first = np.full(len(mo), -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i in range(len(mo)):
            for j in range(i + 1, len(mo)):
                if np.all(np.abs(mo[i] - mo[j]) / mo[i] < dev):
                    first[i] = j
                    break
    return first


def moi_stride_input():
    rng = np.random.default_rng(1)
    n = 20_000
    parents = np.sort(np.abs(rng.normal(200, 50, size=(400, 3))), axis=1)
    return parents[rng.integers(0, 400, size=n)] * (1 + rng.normal(size=(n, 3)) * 4e-3)


@pytest.mark.gpu
def test_moi_first_similar_signed_and_non_finite_denominators(eng, oracle):
    assert eng.moi_first_similar(MOI_EDGE, 1e-2).tolist() == MOI_EDGE_EXPECTED
    assert oracle.moi_first_similar(MOI_EDGE, 1e-2).tolist() == MOI_EDGE_EXPECTED
    assert moi_first_restated(MOI_EDGE, 1e-2).tolist() == MOI_EDGE_EXPECTED


@pytest.mark.gpu
def test_moi_first_similar_far_columns_and_grid_stride(eng, oracle):
    mo = moi_stride_input()
    ref, margin = oracle.moi_first_similar(mo, 1e-2, return_margin=True)
    assert margin > 1e-9 and far_hits(ref) > 1000 and len(mo) > GRID_ROWS
    got = eng.moi_first_similar(mo, 1e-2)
    assert np.array_equal(got[GRID_ROWS:], ref[GRID_ROWS:]), "second pass of the grid"
    assert np.array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["linear", "planar"])
def test_moi_first_similar_follows_the_signs_jacobi_produced(eng, oracle, name):
    """End to end: the GPU's own moments (a linear molecule's smallest one is +-1e-16 of the largest) into both searches."""
    structures, masses = moi_input(name)
    mo = eng.inertia_moments(structures, masses)
    assert np.array_equal(eng.moi_first_similar(mo, 1e-2), oracle.moi_first_similar(mo, 1e-2))
    assert np.array_equal(eng.moi_first_similar(mo[:40], 1e-2), moi_first_restated(mo[:40], 1e-2))


# ===================================================================================================== 5. embed_scores
EMBED_CASES = [(1000, 12, 0), (1000, 12, 1), (1000, 12, 8), (600_001, 4, 2)]      # N, atoms, n_c


def embed_input(case):
    N, n, n_c = EMBED_CASES[case]
    rng = np.random.default_rng(500 + case)
    structures = rng.normal(size=(N, n, 3)) * 1.5
    indices = rng.integers(0, n, size=(N, n_c, 2)).astype(np.int32)              # a == b included
    targets = rng.uniform(1, 3, size=(N, n_c))
    targets[rng.random((N, n_c)) < 0.3] = np.nan
    if n_c:                                                                      # whatever the draw: an all-NaN row, a first and a last NaN
        targets[0], targets[1, 0], targets[2, -1] = np.nan, np.nan, np.nan
    return structures, indices, targets


def embed_scores_restated(structures, indices, targets):
    """(sum |dist - target|, sum (dist - target)) over the constraints with a target, in long double."""
    s = np.asarray(structures, dtype=np.longdouble)
    rows = np.arange(len(s))[:, None]
    delta = s[rows, indices[:, :, 0]] - s[rows, indices[:, :, 1]]
    diff = np.where(np.isnan(targets), np.longdouble(0), np.sqrt((delta * delta).sum(axis=2)) - np.nan_to_num(targets).astype(np.longdouble))
    return np.abs(diff).sum(axis=1), diff.sum(axis=1)


def fitness_threshold(err):
    """A threshold at the median |err|, and the rows that sit on it."""
    thr = float(np.median(np.abs(err.astype(np.float64))))
    return thr, np.abs(np.abs(err.astype(np.float64)) - thr) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(EMBED_CASES)))
def test_embed_scores_constraint_counts_and_nan_targets(eng, oracle, case):
    import tscode_amd
    structures, indices, targets = embed_input(case)
    N, n, n_c = EMBED_CASES[case]
    sc, err = eng.embed_scores(structures, indices, targets)
    so, eo = oracle.embed_scores(structures, indices, targets)
    assert sc.dtype == np.float32 and np.array_equal(sc, so) and np.abs(err - eo).max(initial=0) < 1e-12
    sr, er = embed_scores_restated(structures, indices, targets)
    # one float32 rounding of the running sum per term
    assert (np.abs(sc.astype(np.longdouble) - sr) <= n_c * 2.0 ** -24 * sr + 1e-12).all()
    assert np.abs(err - er.astype(np.float64)).max(initial=0) < 1e-12
    if n_c == 0:
        assert not sc.any() and not err.any()
        assert tscode_amd.fitness_mask(structures, indices, targets, 0.5).all() and not tscode_amd.fitness_mask(structures, indices, targets, 0.0).any()
        return
    if N > GRID_ELEMS:
        assert np.array_equal(sc[GRID_ELEMS:], so[GRID_ELEMS:])
        return
    all_nan = np.isnan(targets).all(axis=1)
    assert all_nan.any() and not sc[all_nan].any() and not err[all_nan].any()
    # fitness_check compares the SIGNED sum with the threshold (tscode/optimization_methods.py:544-557): rows with |err| < thr pass, and so
    # do rows with err <= -thr
    thr, on_it = fitness_threshold(er)
    assert on_it.mean() < 0.01
    mask = tscode_amd.fitness_mask(structures, indices, targets, thr)
    assert mask[(np.abs(er) < thr) & ~on_it].all()
    assert np.array_equal(mask[~on_it], (er < thr)[~on_it])


# ===================================================================================================== 6. the other grid-stride seams
def string_params_input():
    rng = np.random.default_rng(600)
    S = 15_001
    p1, p2, rv, mv = rng.normal(size=(4, S, 3)) * 2
    return p1, p2, rv, mv, rng.integers(0, 5, size=(S, 2)).astype(np.int32), np.arange(0, 360, 10).astype(np.float64)


@pytest.mark.gpu
def test_string_embed_params_grid_stride(eng, oracle):
    p1, p2, rv, mv, cp, angles = string_params_input()
    A = len(angles)
    assert len(p1) * A > GRID_ELEMS
    rot, pos, ci = eng.string_embed_params(p1, p2, rv, mv, cp, angles)
    ro, po, co = oracle.string_embed_params(p1, p2, rv, mv, cp, angles)
    assert np.array_equal(ci, co) and np.abs(rot - ro).max() < 1e-12 and np.abs(pos - po).max() < 1e-11
    site = np.arange(GRID_ELEMS, len(rot)) // A                                   # rows of the second pass: the reactive centres coincide
    assert np.abs(np.einsum("nij,nj->ni", rot[GRID_ELEMS:, 1], p2[site]) + pos[GRID_ELEMS:, 1] - p1[site]).max() < 1e-11


def cyclical_params_input():
    rng = np.random.default_rng(601)
    n = 600_001
    vecs = rng.normal(size=(7, n, 3)) * 2
    return (*vecs, rng.integers(1, 3, size=n).astype(np.int32), rng.choice(np.arange(0, 360, 10), size=n).astype(np.float64))


@pytest.mark.gpu
def test_cyclical_embed_params_grid_stride(eng, oracle):
    args = cyclical_params_input()
    assert len(args[-1]) > GRID_ELEMS
    rot, pos = eng.cyclical_embed_params(*args)
    ro, po = oracle.cyclical_embed_params(*args)
    assert np.abs(rot - ro).max() < 1e-9 and np.abs(pos - po).max() < 1e-8
    assert np.abs(rot[GRID_ELEMS:] - ro[GRID_ELEMS:]).max() < 1e-9
    assert np.abs(np.einsum("nij,nkj->nik", rot, rot) - np.eye(3)).max() < 1e-12


ROTATE_SHAPE = (30_011, 37)
ROTATE_GRID = 4096 * 256      # k_rotate_dihedral: one thread per (structure, atom), 4096 workgroups per pass


def rotate_input():
    rng = np.random.default_rng(602)
    M, n = ROTATE_SHAPE
    seam = ROTATE_GRID // n                                                       # the structure that element 1 048 576 belongs to
    rows = np.unique(np.concatenate([np.arange(21), np.arange(seam - 20, seam + 20), np.arange(M - 20, M), rng.integers(0, M, size=200)]))
    return rng.normal(size=(M, n, 3)) * 4, rng.random(n) < 0.4, rng.uniform(-360, 360, size=M), rows


@pytest.mark.gpu
def test_rotate_dihedral_batch_grid_stride(eng, oracle):
    big, m, ang, rows = rotate_input()
    assert big.shape[0] * big.shape[1] > ROTATE_GRID and ROTATE_GRID // 37 == 28_339
    got = eng.rotate_dihedral_batch(big, [4, 9, 20, 30], m, ang)
    for s in rows:
        assert np.abs(got[s] - oracle.rotate_dihedral(big[s], [4, 9, 20, 30], float(ang[s]), m.astype(np.uint8))).max() < VAL_TOL, s
    assert np.array_equal(got[:, ~m], big[:, ~m])                                 # unmoved atoms are copied, bit for bit, on all rows
    assert not np.array_equal(got[rows][:, m], big[rows][:, m])


def comp_check_waves_per_pass():
    """Workgroups per pass x wavefronts per workgroup of the k_torsion_comp_check launch, read from adjacent.hip."""
    src = open(os.path.join(ROOT, "tscode_amd", "csrc", "adjacent.hip")).read()
    launch = re.search(r"k_torsion_comp_check, dim3\(grid_for\(n_structs, waves, (\d+) \* (\d+)\)\)", src)
    waves = re.search(r"static int csearch_waves\(.*?int w = (\d+);", src, re.S)
    assert launch and waves
    return int(launch.group(1)) * int(launch.group(2)) * int(waves.group(1))


COMP_M = 20_011
# (torsion of G7 case 0, threshold, max_clashes): 1.4 with 0 and 2 clashes allowed -- this chain never comes that close to itself, every
# structure passes; 2.8 about torsion 2 with 2 clashes allowed and 2.6 about torsion 0 with none -- both verdicts occur, on the fp64 count path
# and on the fp32-screened one
COMP_CASES = [(2, 1.4, 0), (2, 1.4, 2), (2, 2.8, 2), (0, 2.6, 0)]


def comp_check_input(oracle, t, thresh):
    """csearch_rotate outputs of the 14-atom chain of G7 case 0 under random angle sets, every rotation kept as it falls (no walk-back);
    checked about torsion t.  Returns structures, torsion, mask, and per structure the smallest |distance - threshold| over the
    moved-fixed pairs."""
    g = load_golden("G7_csearch")
    coords, torsions, masks = g["coords0"], g["torsions0"], g["masks0"].astype(np.uint8)
    angles = np.random.default_rng(603).integers(-179, 181, size=(COMP_M, len(torsions))).astype(np.int32)
    out, _ = oracle.csearch_rotate(coords, torsions, masks, angles, 1.4, 10 ** 6)
    tor, mask = torsions[t], masks[t]
    fixed = mask == 0
    fixed[[tor[1], tor[2]]] = False
    d = np.sqrt(((out[:, fixed][:, :, None] - out[:, mask == 1][:, None]) ** 2).sum(axis=-1))
    return out, tor, mask, np.abs(d - thresh).reshape(len(out), -1).min(axis=1)


def comp_check_reference(oracle, out, tor, mask, thresh, max_clashes):
    return np.array([oracle.torsion_comp_check(o, tor, mask, thresh, max_clashes) for o in out], dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("t,thresh,max_clashes", COMP_CASES)
def test_torsion_comp_check_grid_stride(eng, oracle, t, thresh, max_clashes):
    out, tor, mask, margin = comp_check_input(oracle, t, thresh)
    per_pass = comp_check_waves_per_pass()
    assert len(out) > per_pass
    near = margin < 1e-9
    assert near.mean() < 0.01
    want = comp_check_reference(oracle, out, tor, mask, thresh, max_clashes)
    got = eng.torsion_comp_check(out, tor, mask, thresh, max_clashes)
    assert np.array_equal(got[per_pass:][~near[per_pass:]], want[per_pass:][~near[per_pass:]]), "later passes of the grid"
    assert np.array_equal(got[~near], want[~near]), int((got != want)[~near].sum())


# ===================================================================================================== 7. input guards, no GPU
GUARDS = ["tfd-geometries", "tfd-lengths", "tfd-stride", "tfd-edge", "torsion-0", "torsion-1", "torsion-degenerate", "moi-bounds", "moi-edge",
          "moi-stride", "embed-scores", "comp-check", "grid-seams"]


@pytest.mark.parametrize("what", GUARDS)
def test_sweep_inputs_meet_the_conditions_the_gpu_tests_lean_on(oracle, what):
    if what == "tfd-geometries":
        tf = tfd_small_input()
        for d, k, na in TFD_GEOMETRIES:
            ref, margin = oracle.tfd_first_similar(tf, d, k, na, 10.0, return_margin=True)
            assert margin > 1e-6 and np.array_equal(ref, tfd_first_restated(tf, d, k, na, 10.0)), (d, k, na)
        assert (oracle.tfd_first_similar(tf, 10, 5, 50, 10.0) >= 0).sum() > 5
    elif what == "tfd-lengths":
        for T in TFD_T_SWEEP:
            tf, (d, k, na) = tfd_t_input(T)
            ref, margin = oracle.tfd_first_similar(tf, d, k, na, 10.0, return_margin=True)
            print(f"\ntfd T = {T}: margin {margin:.2e}, {(ref >= 0).sum()} hits of {len(tf)}")
            assert margin > 1e-6 and 50 < (ref >= 0).sum() < (len(tf) if T else len(tf) - 7), T
    elif what == "tfd-stride":
        tf, passes = tfd_stride_input()
        for d, k, na in passes:
            ref, margin = oracle.tfd_first_similar(tf, d, k, na, 10.0, return_margin=True)
            print(f"\ntfd pass {(d, k, na)}: margin {margin:.2e}, {far_hits(ref)} hits beyond 64 columns, {(ref[GRID_ROWS:] >= 0).sum()} hits in the second pass")
            assert margin > 1e-6 and far_hits(ref) > 1000
        assert (oracle.tfd_first_similar(tf, *passes[0], 10.0)[GRID_ROWS:] >= 0).sum() > 100
    elif what == "tfd-edge":
        for thresh, want in TFD_EDGE_EXPECTED.items():
            assert oracle.tfd_first_similar(TFD_EDGE, 6, 1, 6, thresh).tolist() == want == tfd_first_restated(TFD_EDGE, 6, 1, 6, thresh).tolist()
    elif what in ("torsion-0", "torsion-1"):
        structures, quads = torsion_input(int(what[-1]))
        assert (np.sort(quads, axis=1)[:, 1:] != np.sort(quads, axis=1)[:, :-1]).all()
        angles = torsion_angles_f64(oracle, structures, quads)
        left_out = assert_float32_of_the_same_angle(angles.astype(np.float32), oracle.torsion_fingerprints(structures, quads), angles, what)
        print(f"\n{what}: {left_out:.4%} of the elements lie within {TIE_BAND} degrees of a float32 rounding tie")
        assert left_out < 0.01
    elif what == "torsion-degenerate":
        check_torsion_degenerate_values(oracle.torsion_fingerprints(*torsion_degenerate_input()))
    elif what == "moi-bounds":
        for name in MOI_CASES:
            structures, masses = moi_input(name)
            ref, scale, dev, bound = moi_bound(oracle, structures, masses)
            print(f"\ninertia_moments {name}: oracle vs long double {dev:.3e}, bound {bound:.3e}")
            assert dev < 64 * EPS, name                      # the reference and the oracle agree far inside the floor of the bound
            if name in ("linear", "two-atoms"):
                assert (np.abs(ref[:, 0]) / scale).max() < bound
    elif what == "moi-edge":
        assert oracle.moi_first_similar(MOI_EDGE, 1e-2).tolist() == MOI_EDGE_EXPECTED == moi_first_restated(MOI_EDGE, 1e-2).tolist()
    elif what == "moi-stride":
        ref, margin = oracle.moi_first_similar(moi_stride_input(), 1e-2, return_margin=True)
        print(f"\nmoi stride: margin {margin:.2e}, {far_hits(ref)} hits beyond 64 columns, {(ref[GRID_ROWS:] >= 0).sum()} hits in the second pass")
        assert margin > 1e-9 and far_hits(ref) > 1000 and (ref[GRID_ROWS:] >= 0).sum() > 100
    elif what == "embed-scores":
        for case, (N, n, n_c) in enumerate(EMBED_CASES):
            structures, indices, targets = embed_input(case)
            so, eo = oracle.embed_scores(structures, indices, targets)
            sr, er = embed_scores_restated(structures, indices, targets)
            assert (np.abs(so.astype(np.longdouble) - sr) <= n_c * 2.0 ** -24 * sr + 1e-12).all() and np.abs(eo - er.astype(np.float64)).max(initial=0) < 1e-12
            if 0 < n_c and N <= GRID_ELEMS:
                nan = np.isnan(targets)
                assert nan.all(axis=1).any() and nan[:, 0].any() and nan[:, -1].any() and (indices[:, :, 0] == indices[:, :, 1]).any()
                thr, on_it = fitness_threshold(er)
                assert on_it.mean() < 0.01 and 0.2 < (er < thr).mean() < 0.9 and (er <= -thr).any()
    elif what == "comp-check":
        for t, thresh, max_clashes in COMP_CASES:
            out, tor, mask, margin = comp_check_input(oracle, t, thresh)
            assert len(out) > comp_check_waves_per_pass() and (margin < 1e-9).mean() < 0.01
            want = comp_check_reference(oracle, out, tor, mask, thresh, max_clashes)
            print(f"\ntorsion_comp_check {(t, thresh, max_clashes)}: {want.sum()} of {len(want)} pass, {(margin < 1e-9).sum()} within 1e-9 of the threshold")
            assert want.all() if thresh == 1.4 else 0.02 * len(want) < want.sum() < 0.98 * len(want)
    else:
        assert what == "grid-seams"
        # the caps the sizes above were chosen against, as the launches in adjacent.hip state them
        src = open(os.path.join(ROOT, "tscode_amd", "csrc", "adjacent.hip")).read()
        for kernel, per_block, cap in (("k_tfd_first_similar", "4", "256 * 16"), ("k_moi_first_similar", "4", "256 * 16"),
                                       ("k_torsion_fingerprints", "256", "256 * 8"), ("k_inertia_moments", "256", "256 * 8"),
                                       ("k_embed_scores", "256", "256 * 8"), ("k_string_embed_params", "256", "256 * 8"),
                                       ("k_cyclical_embed_params", "256", "256 * 8")):
            assert re.search(re.escape(kernel) + r", dim3\(grid_for\([^;]*?, " + per_block + ", " + re.escape(cap) + r"\)\)", src), kernel
        assert re.search(r"k_rotate_dihedral, dim3\(grid_for\(n_structs \* n_atoms, 256\)\)", src)      # the default cap: 256 * 16 workgroups
        assert comp_check_waves_per_pass() == 2048 * 4
