"""The known prefix of a row (csrc/rmsd.hpp: known[], cbeg[]; csrc/mm.hpp: k_rmsd_sieve_mm16 starts a row at cbeg): a row that survives a
pass had every active column before its stop position found dissimilar, so later passes leave those columns out.  The skip is a hint: with
it on and off, in both modes, a run must give the oracle's final mask, the oracle's mask after EVERY pass (the stepping API), and per pass
its n_active, pairs_evaluated and new_keys.  (The key SET is not readable through the API; in mode 0 every key decides where rows of the
later passes stop, i.e. their pairs_evaluated and masks, which are compared.)  tsc_pass_stats.pairs_known must be what the CPU model of
tools/known_prefix_model.py counts from the oracle's trace with the skip on, and 0 with it off.

"local_max_chunk" = 16 makes every pass of these small runs a walked one (k_open_rows + the 16-row matrix-core kernel; algo 2 is asserted),
so a few hundred to 3 415 structures have five to seven walked passes.  The shapes:
  * what the pair kernel branches on is in RANK space -- a tile's smallest first column against the 128-column tiles and the 256- or
    512-column segments counted from the tile's first segment -- and the opener's second ranking in POSITION space (the scan block of
    known[i]).  boundary_hits() counts, from the model's rows, the rows and tiles whose first column lies one before, on and one behind a
    multiple of 16, a 128-column tile boundary, a 256- and a 512-column segment boundary, and the rows whose known[] is 2 047, 2 048 and
    2 049; the CPU test asserts at least three of every kind over the cases.  The cases get there by `front` copies at the head of the
    array, which shift every rank behind them (the settings were found with the model); 2 560 = 20 x 128 has chunk ends on 2 048,
    2 311 = 23 x 100 + 11 one on 2 047 = 89 x 23, 3 415 = 5 x 683 one on 2 049, and in 2 049 the last chunk's end is n itself;
  * 2 540 = 20 x 127 and 2 580 = 20 x 129: chunk ends just before and just after multiples of 128 in position space;
  * 2 000: divisible by every k that runs (50 ... 1), every chunk a union of the chunks before it; 2 311: prime, divisible by none, a last
    partial tile (as 2 540 and 2 580 have); 50: fewer than 64 structures, two passes;
  * copies at distances 1 ... 1 100, which first share a chunk in different passes -- removed columns inside later prefixes --, and copies whose
    original sits just in front of a chunk end of an earlier pass with the copy exactly ON it: the first similar column is at known[i];
  * 2 000 and 2 560 nest their chunks: the rows in the later part of a merged chunk know all of it already, their tiles are dead only
    because of cbeg and still owe pairs_evaluated (asserted from the model's rows, then by the pairs_evaluated comparison)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

THR = 0.5
H = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("known_prefix_model", os.path.join(ROOT, "tools", "known_prefix_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def ensemble(n, seed, distances, per_distance, on_ends=(), front=0):
    """Unrelated structures (pairwise RMSD far above the threshold); some have a near-copy d rows further on (noise far below it), and for
    every (chunk length c, d) of on_ends some originals sit d in front of a multiple of c with their copy exactly on it.  front: that many
    originals at positions 0, 3, 6 ... with their copy right behind them -- removed by the first pass (by the second where a chunk end parts
    them), they move the RANK of everything behind them: what the cases are tuned with so that first columns land on the kernels' boundaries."""
    rng = np.random.default_rng(seed)
    heavy = rng.normal(size=(n, H, 3)) * 2
    used = np.zeros(n, dtype=bool)
    pairs = []

    def plant(i, j):
        if j < n and not used[i] and not used[j]:
            heavy[j] = heavy[i] + rng.normal(size=(H, 3)) * 0.01
            used[i] = used[j] = True
            pairs.append((i, j))
            return True
        return False

    for m in range(front):
        plant(3 * m, 3 * m + 1)
    for c, d in on_ends:
        for end in range(c, n, 3 * c):
            plant(end - d, end)
    for d in distances:
        placed = 0
        for i in rng.permutation(max(n - d, 0)):
            if placed == per_distance:
                break
            placed += plant(int(i), int(i) + d)
    return np.ascontiguousarray(heavy), pairs


CASES = {
    "2560-ends-on-boundaries": dict(n=2560, seed=1, distances=(1, 30, 130, 260, 520, 1100), per_distance=12, on_ends=((128, 5), (256, 40)), front=34),
    "2540-ends-just-before": dict(n=2540, seed=2, distances=(1, 30, 130, 260, 520, 1100), per_distance=12, on_ends=((127, 5), (254, 40))),
    "2580-ends-just-after": dict(n=2580, seed=3, distances=(1, 30, 130, 260, 520, 1100), per_distance=12, on_ends=((129, 5), (258, 40))),
    "2000-divisible-by-every-k": dict(n=2000, seed=4, distances=(1, 45, 110, 450, 900), per_distance=10, on_ends=((200, 3), (400, 2))),
    "2311-divisible-by-none": dict(n=2311, seed=5, distances=(1, 25, 120, 240, 470, 1200), per_distance=10, on_ends=((115, 7),)),
    "50-below-one-wavefront": dict(n=50, seed=6, distances=(1, 30), per_distance=2, on_ends=((25, 3),)),
    # 3 415 = 5 x 683: 3 x 683 = 2 049, one position behind a scan block; the three settings of `front` put the tiles' smallest first columns
    # before, on and behind the boundaries of 128-column tiles and of 256- and 512-column segments (BOUNDARIES below counts them)
    "3415-ranks-a": dict(n=3415, seed=9, distances=(1, 30, 130, 700, 1400), per_distance=10, front=20),
    "3415-ranks-b": dict(n=3415, seed=9, distances=(1, 30, 130, 700, 1400), per_distance=10, front=21),
    "3415-ranks-c": dict(n=3415, seed=9, distances=(1, 30, 130, 700, 1400), per_distance=10, front=22),
    # the last chunk's end, n itself, one position behind a scan block: its rank comes from the block that holds one structure
    "2049-one-past-a-scan-block": dict(n=2049, seed=7, distances=(1, 30, 130, 260, 520, 1100), per_distance=10, front=20),
}
_heavy, _pairs, _refs = {}, {}, {}


def reference(oracle, name, mode):
    """The ensemble of a case, the oracle's traced run of it and the model's rows: computed once, shared by the four runs of the case."""
    if name not in _heavy:
        _heavy[name], _pairs[name] = ensemble(**CASES[name])
    if (name, mode) not in _refs:
        km = _model()
        heavy = _heavy[name]
        ref = oracle.prune_heavy(heavy, THR, mode=mode, row_parallel=True, trace=True)
        rows = km.model(len(heavy), mode, km.passes_of_trace(ref), ref["keys"], rows=True)
        _refs[name, mode] = (ref, rows)
    return (_heavy[name],) + _refs[name, mode]


def seg_cols_of(n, k):
    """Columns per work item of the 16-row matrix-core kernel in a run of n <= 100 000 structures (csrc/pass_plan.hpp, mm16_item_shape with a
    range below 8 192): 512, halved to 256 while the longest chunk of the pass is shorter than four segments."""
    longest, seg = n - (k - 1) * (n // k), 512
    while seg > 256 and longest < 4 * seg:
        seg //= 2
    return seg


def boundary_hits(n, rows):
    """Where the first columns of a run land against what the kernels branch on, counted from the model's rows of the passes behind the first:
      t16-1 / t16+0 / t16+1     rows with columns left whose cbeg is one before, on, one behind a multiple of 16 (a row tile of the columns);
      c128.. / s256.. / s512..  row tiles whose smallest such cbeg (tile_cmax[2 t + 1]) lies one before, on, one behind a boundary of a 128-column
                                tile / of a segment of the pass's length, counted from the tile's first segment ((16 t + 1) & ~63) as
                                k_rmsd_sieve_mm16 counts, the boundary at least one tile or segment in: where an item leaves, where the
                                column loop starts, how many items a tile's arrival count expects;
      pos2047 / 2048 / 2049     rows whose known[] entry is that position: the last of a scan block, the first of the next, one behind it."""
    import collections
    c = collections.Counter()
    for r in rows[1:]:
        seg, cbeg, cend = seg_cols_of(n, r["k"]), r["cbeg"], r["cend"]
        for pos in (2047, 2048, 2049):
            c[f"pos{pos}"] += int((r["known_pos"] == pos).sum())
        for t0 in range(0, len(cbeg), 16):
            b, e = cbeg[t0:t0 + 16], cend[t0:t0 + 16]
            live = b < e
            if not live.any():
                continue
            for off in (-1, 0, 1):
                c[f"t16{off:+d}"] += int(((b[live] - off) % 16 == 0).sum())
            x = int(b[live].min()) - ((t0 + 1) & ~63)
            for m, name in ((128, "c128"), (seg, f"s{seg}")):
                for off in (-1, 0, 1):
                    if x - off >= m and (x - off) % m == 0:
                        c[f"{name}{off:+d}"] += 1
    return c


BOUNDARIES = [f"{name}{off:+d}" for name in ("t16", "c128", "s256", "s512") for off in (-1, 0, 1)] + ["pos2047", "pos2048", "pos2049"]


def stepped_run(eng, heavy, mode, skip):
    """One run through the stepping API under local_max_chunk = 16: the mask after every pass, and the statistics."""
    from tscode_amd import _lib
    lib, n = eng.lib, len(heavy)
    with eng.options(local_max_chunk=16, skip_known=skip):
        d_heavy = C.c_void_p()
        _lib.check(lib.tsc_malloc(eng._h, heavy.nbytes, C.byref(d_heavy)))
        _lib.check(lib.tsc_memcpy_h2d(eng._h, d_heavy, _lib.ptr(heavy), heavy.nbytes))
        st = eng.prune_stepper(d_heavy.value, n, heavy.shape[1], THR, mode)
        after = []
        try:
            while st.next_pass() != 0:
                st.pass_local(0, 1)
                st.pass_finish()
                m = np.empty(n, dtype=np.uint8)
                _lib.check(lib.tsc_memcpy_d2h(eng._h, _lib.ptr(m), C.c_void_p(st.mask_ptr()), m.nbytes))
                after.append(m.astype(bool))
            stats = st.stats()
        finally:
            st.close()
            _lib.check(lib.tsc_free(eng._h, d_heavy))
    return after, stats


def test_the_cases_hold_the_shapes_they_are_there_for(oracle):
    """From the oracle and the model alone, so that a changed generator cannot make the GPU cases vacuous."""
    for name, c in CASES.items():
        n = c["n"]
        for mode in (0, 1):
            heavy, ref, rows = reference(oracle, name, mode)
            ks = [r["k"] for r in rows]
            assert len(ks) >= (2 if n < 64 else 5) and all(n - (k - 1) * (n // k) > 16 for k in ks), (name, ks, "every pass must be a walked one")
            assert sum(1 for r in rows if r["known"] > 0) >= (1 if n < 64 else 3), (name, mode, [r["known"] for r in rows])
            removing = [s["k"] for s in ref["stats"] if s["n_active_after"] < s["n_active_before"]]
            assert len(removing) >= (1 if n < 64 else 3), (name, mode, removing, "copies must first meet their originals in several passes")
        ran = [r["k"] for r in reference(oracle, name, 0)[2]]
        if name.startswith("2000"):
            assert all(n % k == 0 for k in ran)
        if name.startswith("2311"):
            assert all(n % k for k in ran if k > 1) and n % 16
    # first columns one before, on and one behind every boundary the kernels branch on, and known[] on both sides of a scan block's end
    import collections
    total = collections.Counter()
    for name, c in CASES.items():
        for mode in (0, 1):
            total += boundary_hits(c["n"], reference(oracle, name, mode)[2])
    print("boundary hits:", {b: total[b] for b in BOUNDARIES})
    assert all(total[b] >= 3 for b in BOUNDARIES), {b: total[b] for b in BOUNDARIES}
    # a tile that is dead only because of cbeg and owes pairs_evaluated: 16 consecutive rows, all with cbeg >= cend, some with cend > r + 1
    for name in ("2000-divisible-by-every-k", "2560-ends-on-boundaries"):
        for mode in (0, 1):
            owing = 0
            for r in reference(oracle, name, mode)[2][1:]:
                cbeg, cend = r["cbeg"], r["cend"]
                rr = np.arange(len(cend))
                for t in range(0, len(cend) - 15, 16):
                    s = slice(t, t + 16)
                    owing += bool((cbeg[s] >= cend[s]).all() and (cend[s] > rr[s] + 1).any())
            assert owing >= 10, (name, mode, owing)
    # a row whose first similar column is exactly at known[i]: a planted pair (i, j), both active when a pass begins, i removed by it, and
    # known[i] == j as that pass finds it (the copy sits ON the end of the chunk that held i in the pass before)
    for mode in (0, 1):
        hits = []
        for name in CASES:
            heavy, ref, rows = reference(oracle, name, mode)
            for p in range(1, len(rows)):
                before, after = ref["pass_masks"][p - 1], ref["pass_masks"][p]
                known_at = dict(zip(rows[p]["pos"].tolist(), rows[p]["known_pos"].tolist()))
                hits += [(name, rows[p]["k"], i, j) for i, j in _pairs[name] if before[i] and before[j] and not after[i] and known_at[i] == j]
        assert len(hits) >= 2, (mode, hits)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [1, 0], ids=["skip-on", "skip-off"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_run_with_and_without_the_skip_against_the_oracle(eng, oracle, name, mode, skip):
    heavy, ref, rows = reference(oracle, name, mode)
    after, stats = stepped_run(eng, heavy, mode, skip)
    assert [int(s["k"]) for s in stats] == [int(s["k"]) for s in ref["stats"]]
    assert all(int(s["algo"]) == 2 for s in stats), ([s["algo"] for s in stats], "every pass was meant to be walked")
    for p, (s, r) in enumerate(zip(stats, ref["stats"])):
        k = int(s["k"])
        assert np.array_equal(after[p], ref["pass_masks"][p]), f"{name} mode {mode} skip {skip}: the mask after the k = {k} pass differs"
        for f in ("n_active_before", "n_active_after", "pairs_evaluated", "new_keys"):
            assert int(s[f]) == int(r[f]), (name, mode, skip, k, f, int(s[f]), int(r[f]))
    assert np.array_equal(after[-1], ref["mask"])
    known = [int(s["pairs_known"]) for s in stats]
    print(f"{name} mode {mode} skip {skip}: pairs_known {known}, model {[r['known'] for r in rows]}, inside the ranges {[r['today'] for r in rows]}")
    if skip:
        assert known == [r["known"] for r in rows]
        assert known[0] == 0 and sum(1 for v in known[1:] if v > 0) >= (1 if len(heavy) < 64 else 3)
        # what the screen multiplied + the known prefix = the pairs inside the rows' ranges, for the rows that looked to their range's end
        for s, r in zip(stats, rows):
            assert int(s["pairs_screened"]) <= r["today"] and int(s["pairs_screened"]) >= int(s["pairs_known"])
    else:
        assert known == [0] * len(stats)
