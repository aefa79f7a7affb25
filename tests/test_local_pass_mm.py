"""The chunk-local pass kernel with its descriptor screen on the matrix cores (csrc/local_pass.hpp, k_pass_chunks<true>; option
"sieve_mm16" = 1, which the walked passes' 16-row kernel follows as well) against the packed-fp32 form of the same kernel (sieve_mm16 = 0) and against oracle.prune_heavy.

Every case runs the WHOLE prune through the stepping API, in both modes and under sieve_mm16 = 0 and 1, so that later passes see removed
rows and ranks differ from structure indices.  Compared with the oracle, exactly (no tolerance is involved): the mask after EVERY pass,
the final mask and per pass (k, n_active_before, n_active_after, pairs_evaluated).  The passes a case is there for must have taken the
chunk-local kernel (PassStats.algo 3): a case cannot pass by running the walked kernel.  pairs_computed, pairs_screened and the
candidate counts may differ between the two forms (float16 rounding, another queue order) and are not compared.

Shapes: a pass of k chunks exists only while 20 k < n (rmsd_pruning.py:192), so a regular chunk has at least 20 structures; chunks of 1,
15, 16 and 17 are the single chunk of the k = 1 pass of ensembles that small."""
import ctypes as C

import numpy as np
import pytest

from test_pass_close import copies_at_distances, per_pass, triplets

THR = 0.5
LOCAL = 3      # PassStats.algo of a pass that ran in k_pass_chunks (include/tscode_hip.h)
KS = (500000, 200000, 100000, 50000, 20000, 10000, 5000, 2000, 1000, 500, 200, 100, 50, 20, 10, 5, 2, 1)   # rmsd_pruning.py:186-188


def families(n, h, seed, per_family=3, noise=0.01):
    """n structures drawn from n / per_family bases (+ noise far below the threshold), every row's base picked at random: near-copies at
    every distance, so that every pass of the schedule finds rows to remove and the later ones see what the earlier ones left."""
    rng = np.random.default_rng(seed)
    bases = rng.normal(size=(max(1, n // per_family), h, 3)) * 2
    heavy = bases[rng.integers(0, len(bases), size=n)] + rng.normal(size=(n, h, 3)) * noise
    return np.ascontiguousarray(heavy)


def cached_keys(n=2000, seed=41):
    """make_ensemble with a local shuffle: siblings meet in the fine passes, so mode 0 leaves cache keys and the stop columns they set
    fall inside a 16-column block and in the middle of a 64-column step of the coarser passes."""
    from tscode_amd.synthetic import make_ensemble
    ens = make_ensemble(n, (15, 15), seed=seed, children=10, local_spread=200.0)
    return np.ascontiguousarray(ens.poses()[:, ens.atomnos != 1])


def rigid_motions(x):
    """Orthonormal basis (columns) of the translations and infinitesimal rotations of the structure x[h, 3], as vectors of 3 h numbers."""
    h = len(x)
    xc = x - x.mean(axis=0)
    rigid = [np.tile(e, (h, 1)) for e in np.eye(3)] + [np.cross(e, xc) for e in np.eye(3)]
    q, _ = np.linalg.qr(np.stack([r.ravel() for r in rigid], axis=1))
    return q


def near_threshold_h30(n=64, h=30, seed=7):
    """Copies of one base (the construction of tests/test_local_pass_stages.py's exact-queue case) whose displacements are orthonormal
    patterns with the rigid motions projected out: structure i = base + c_i U_i, so the pair (i, j) has RMSD sqrt((c_i^2 + c_j^2) / h)
    to first order, whatever the alignment.  Every atom moves by the same length in a pattern (a direction of its own), which keeps the
    largest deviation of a pair well below twice the threshold.  The c_i are drawn so that the pair RMSDs lie between 0.90 and 0.999 of
    the threshold."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(h, 3)) * 2
    q = rigid_motions(base)
    d = rng.normal(size=(n, h, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    pat = d.reshape(n, 3 * h).T
    pat -= q @ (q.T @ pat)
    u, _ = np.linalg.qr(pat)                                                                      # orthonormal, orthogonal to the rigid motions
    # c_i^2 + c_j^2 = h (f thr)^2 with f in [0.93, 0.98] for every pair
    c = np.sqrt(rng.uniform(0.93 ** 2, 0.98 ** 2, size=n) * h * THR * THR / 2)
    heavy = base[None] + (u * c[None, :]).T.reshape(n, h, 3)
    return np.ascontiguousarray(heavy)


def near_threshold_h3(n=41, seed=9):
    """h = 3: the fewest heavy atoms for which the reference's alignment is defined (its rotation of two collinear point sets is not an
    optimum, and one atom always coincides with itself; the sieve itself takes any h > 0).  A chain: row i + 1 is row i moved along one
    of its three internal coordinates -- a displacement orthogonal to its rigid motions -- by f thr sqrt(h), f in [0.93, 0.97], then
    turned as a whole about its centroid: RMSD(i, i + 1) = f thr to first order."""
    rng = np.random.default_rng(seed)
    h = 3
    x = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [1.0, 2.5, 0.0]])
    x -= x.mean(axis=0)          # (the centroid stays at the origin: the steps are orthogonal to the translations, the turns are about it)
    out = []
    for i in range(n):
        rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        rot *= np.sign(np.linalg.det(rot))
        out.append(x @ rot.T)
        q = rigid_motions(x)
        step = rng.normal(size=3 * h)
        step -= q @ (q.T @ step)
        step *= rng.uniform(0.93, 0.97) * THR * np.sqrt(h) / np.linalg.norm(step)
        x = x + step.reshape(h, 3)
    return np.ascontiguousarray(np.stack(out))


def one_far(n=300, h=10, seed=13):
    """One structure ten thousand times farther from the origin than the rest (every coordinate times 10^4): the largest descriptor
    component of the run is its, and the scale that takes it into [32, 64) pushes everybody else's towards the float16 flush limit."""
    heavy = families(n, h, seed)
    heavy[n // 2] *= 1.0e4
    return heavy


def identical(n=100, h=10, seed=15):
    return np.ascontiguousarray(np.repeat(np.random.default_rng(seed).normal(size=(1, h, 3)) * 2, n, axis=0))


# name: (builder, "local_max_chunk" of the run, the k whose pass must be chunk-local -- None: every pass that runs)
CASES = {
    # MFMA block and step edges: the chunk of the k = 1 pass is n itself; (n, k) with shorter chunks come along
    "chunk1": (lambda: families(1, 10, 101), 384, None),
    "chunk15": (lambda: families(15, 10, 115), 384, None),
    "chunk16": (lambda: families(16, 10, 116), 384, None),
    "chunk17": (lambda: families(17, 10, 117), 384, None),          # a second row tile of ONE row
    "chunk63": (lambda: families(63, 10, 163), 384, None),
    "chunk64": (lambda: families(64, 10, 164), 384, None),
    "chunk65": (lambda: families(65, 10, 165), 384, None),          # a second column step of ONE column
    "chunk127": (lambda: families(127, 10, 1127), 384, None),
    "chunk128": (lambda: families(128, 10, 1128), 384, None),
    "chunk129": (lambda: families(129, 10, 1129), 384, None),
    "chunk384": (lambda: families(384, 10, 1384), 384, None),        # the longest chunk the default limit lets through, 24 row tiles
    # the last chunk takes the remainder: 1 219 = 49 x 24 + 43 (k = 50), 19 x 60 + 79 (k = 20), 9 x 121 + 130, 4 x 243 + 247; k = 2 and 1 are walked
    "last_longer": (lambda: copies_at_distances(1219, 10, 31, distances=(1, 20, 50, 120), per_distance=100), 384, (50, 20, 10, 5)),
    "stop_columns": (cached_keys, 2048, None),
    "near_thr_h30": (near_threshold_h30, 384, None),
    "near_thr_h3": (near_threshold_h3, 384, None),
    "one_far": (one_far, 384, None),
    "identical": (identical, 384, None),
    # 450 structures: k = 20 is the first pass of the run (chunk-local: the records are read by the first kernel behind the one that wrote
    # them), k = 10 is in the schedule and gated off (tests/test_pass_close.py, GATE_CASES), k = 5 runs again; the one chunk of k = 1 is walked
    "gated_slot": (lambda: triplets(150, 10, 1, 0), 384, (20, 5, 2)),
}

_heavy, _refs = {}, {}


def heavy_of(name):
    if name not in _heavy:
        _heavy[name] = CASES[name][0]()
    return _heavy[name]


def reference(oracle, name, mode):
    """The oracle's run of a case with the mask after every pass, computed once and shared."""
    if (name, mode) not in _refs:
        _refs[name, mode] = oracle.prune_heavy(heavy_of(name), THR, mode=mode, row_parallel=True, trace=True)
    return _refs[name, mode]


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def stepped_run(eng, heavy, mode):
    """The run pass by pass (as tests/test_gpu_parity.py::test_prune_large_golden_every_pass_mask): {k: mask after the pass}, the statistics."""
    from tscode_amd import _lib
    lib, n = eng.lib, len(heavy)
    d_heavy = C.c_void_p()
    _lib.check(lib.tsc_malloc(eng._h, heavy.nbytes, C.byref(d_heavy)))
    _lib.check(lib.tsc_memcpy_h2d(eng._h, d_heavy, _lib.ptr(heavy), heavy.nbytes))
    st = eng.prune_stepper(d_heavy.value, n, heavy.shape[1], THR, mode)
    after = {}
    try:
        while True:
            k = st.next_pass()
            if k == 0:
                break
            st.pass_local(0, 1)
            st.pass_finish()
            m = np.empty(n, dtype=np.uint8)
            _lib.check(lib.tsc_memcpy_d2h(eng._h, _lib.ptr(m), C.c_void_p(st.mask_ptr()), m.nbytes))
            after[int(k)] = m.astype(bool)
        stats = st.stats()
    finally:
        st.close()
        _lib.check(lib.tsc_free(eng._h, d_heavy))
    return after, stats


@pytest.mark.gpu
@pytest.mark.parametrize("screen_mm", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_every_pass_mask_and_evaluated_pairs_equal_the_oracle(eng, oracle, name, mode, screen_mm):
    _, max_chunk, local_ks = CASES[name]
    heavy = heavy_of(name)
    ref = reference(oracle, name, mode)
    with eng.options(sieve_mm16=screen_mm, local_max_chunk=max_chunk):
        after, stats = stepped_run(eng, heavy, mode)
    assert per_pass(stats) == per_pass(ref["stats"]), (name, mode, screen_mm)
    for s, ref_mask in zip(stats, ref["pass_masks"]):
        k = int(s["k"])
        assert np.array_equal(after[k], ref_mask), f"{name}, mode {mode}, screen_mm {screen_mm}: the mask after the k = {k} pass differs from the oracle's"
    assert np.array_equal(after[1], ref["mask"]), (name, mode, screen_mm, int(after[1].sum()), int(ref["mask"].sum()))
    algos = {int(s["k"]): int(s["algo"]) for s in stats}
    meant = list(algos) if local_ks is None else list(local_ks)
    assert meant and all(algos.get(k) == LOCAL for k in meant), (name, algos, "these passes were meant to take the chunk-local kernel")
    if name == "last_longer":
        assert algos[2] != LOCAL and algos[1] != LOCAL, (algos, "both pass shapes were meant to run")


@pytest.mark.gpu
@pytest.mark.parametrize("screen_mm", [0, 1])
def test_pipeline_records_written_with_the_initial_state(oracle, screen_mm):
    """The fused pipeline hands the prune descriptors that are final before the run is created: its records by structure are written by the
    kernel that sets up the run's initial state (a run that builds its own descriptors, as every case above, gets them from a launch
    behind the descriptor build).  2 000 poses: every pass of the prune is chunk-local."""
    from tscode_amd.pipeline import DevicePipeline
    from tscode_amd.synthetic import make_config
    ens = make_config("C2", 2000)
    poses = oracle.transform_batch(ens.frag_coords, ens.conf_idx, ens.rot, ens.pos)
    cm = oracle.compenetration_mask(poses, ens.ids, 1.5, 0)
    _, mask_ref = oracle.prune_conformers_rmsd(poses[cm], ens.atomnos, THR)
    pipe = DevicePipeline(ens, device_index=0, mode=0)
    pipe.set_option("sieve_mm16", screen_mm)
    res = pipe.step()
    assert res["n_pass"] == int(cm.sum()) and res["n_keep"] == int(mask_ref.sum())
    assert np.array_equal(pipe.h_keep[:res["n_pass"]].numpy().astype(bool), mask_ref)


# ---- without a GPU: the inputs are what the cases say they are ----

def test_case_shapes_land_on_the_lengths_named():
    def chunks(n, k):
        return n // k, n - (k - 1) * (n // k)
    for n in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 384):
        assert len(heavy_of(f"chunk{n}")) == n and chunks(n, 1) == (n, n)
    assert [k for k in KS if k == 1 or 20 * k < 17] == [1] and [k for k in KS if k == 1 or 20 * k < 65] == [2, 1]
    assert chunks(65, 2) == (32, 33) and chunks(129, 5) == (25, 29) and chunks(384, 10) == (38, 42)
    n = len(heavy_of("last_longer"))
    assert [chunks(n, k) for k in (50, 20, 10, 5, 2)] == [(24, 43), (60, 79), (121, 130), (243, 247), (609, 610)]
    assert all(max(chunks(n, k)) <= 384 for k in (50, 20, 10, 5)) and min(chunks(n, 2)) > 384
    n = len(heavy_of("stop_columns"))
    assert max(chunks(n, 1)) <= 2048
    n = len(heavy_of("gated_slot"))
    assert [k for k in KS if k == 1 or 20 * k < n][:3] == [20, 10, 5]


@pytest.mark.parametrize("name", ["near_thr_h30", "near_thr_h3"])
def test_near_threshold_pairs_are_similar_for_the_oracle(oracle, name):
    """The pairs the two near-threshold cases are built around lie between 0.90 and 0.999 of the threshold, and the oracle calls at least
    95 % of them similar (rmsd_pruning.py:75: RMSD below the threshold and largest deviation below twice the threshold)."""
    heavy = heavy_of(name)
    n = len(heavy)
    pairs = [(i, i + 1) for i in range(n - 1)] if name == "near_thr_h3" else [(i, j) for i in range(n) for j in range(i + 1, n)]
    rm = np.empty(len(pairs))
    md = np.empty(len(pairs))
    for x, (i, j) in enumerate(pairs):
        rm[x], md[x] = oracle.rmsd_and_max_numba(heavy[i], heavy[j])
    in_band = (rm >= 0.90 * THR) & (rm <= 0.999 * THR)
    similar = (rm < THR) & (md < 2 * THR)
    assert in_band.mean() >= 0.95, (name, float(rm.min()), float(rm.max()))
    assert (similar & in_band).sum() >= 0.95 * len(pairs), (name, int(similar.sum()), len(pairs))


def test_stop_column_case_leaves_cache_keys(oracle):
    ref = reference(oracle, "stop_columns", 0)
    removing = [int(s["k"]) for s in ref["stats"] if s["n_active_after"] < s["n_active_before"]]
    assert len(ref["keys"]) > 100 and len(removing) >= 3, (len(ref["keys"]), removing)
    # (the cache changes what later passes evaluate: mode 1 on the same ensemble evaluates more pairs)
    ev0 = sum(int(s["pairs_evaluated"]) for s in ref["stats"])
    ev1 = sum(int(s["pairs_evaluated"]) for s in reference(oracle, "stop_columns", 1)["stats"])
    assert ev0 < ev1, (ev0, ev1)
