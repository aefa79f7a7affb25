"""The conformational-search candidates of MANY start structures and torsion sets in one launch (tsc_csearch_rotate_multi,
tsc_csearch_select_dev; tscode_amd.csearch_rotate_multi / csearch_candidates_multi / clustered_csearch_step).

Yardsticks: fixture G24 (tests/golden/gen_csearch_multi.py: the reference's own clustered_csearch and random_csearch; its pick of
starting points between groups, an unseeded k-means, is replaced there by ``structures[:n]``, so what G24 pins is the candidate
loop of every group for the starting points it was given), the CPU oracle per start (oracle.csearch_rotate, itself pinned by G7;
used only where its margin to the clash threshold exceeds 1e-9), the shipped single-start path, and a literal transcription of
tscode/torsion_module.py:505-511 for the stop rule.  Coordinates are compared at VAL_TOL = 1e-9 A; rotated_bonds, kept rows, their
order and every counter exactly."""

import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

VAL_TOL = 1e-9
SYMBOLS = ("tsc_csearch_multi_plan", "tsc_csearch_rotate_multi", "tsc_csearch_rotate_multi_dev", "tsc_csearch_select_dev")
THRESH = 1.4        # the synthetic molecules are walks of exactly 1.5 A steps: 1.5 would sit on the bonded distances
ANGLES = np.array([0, 0, 60, 120, 180, -60, 25])


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


# ----------------------------------------------------------------------------- helpers
def literal_loop(rotated, n_out, max_tries):
    """tscode/torsion_module.py:465-511 with the rotations taken out: the rows appended, and how many the loop walked."""
    new_structures, walked = [], len(rotated)
    for a, rotated_bonds in enumerate(rotated):
        if rotated_bonds != 0:
            new_structures.append(a)
            if len(new_structures) == n_out or a == max_tries:
                walked = a + 1
                break
    return new_structures, walked


def make_set(rng, n, n_tors, n_rows, turn_i2=None, big=None):
    """n_tors torsions along consecutive atoms; torsion t turns the atoms behind its bond.  turn_i2: that torsion's mask also turns
    its axis atom i2; big: that torsion is (0, 1, 2, 3) and turns every atom from 2 on, more than 64 of them (needs n > 66)."""
    centres = rng.choice(np.arange(1, n - 3), size=n_tors, replace=False)
    torsions = np.array([(c - 1, c, c + 1, c + 2) for c in centres], dtype=np.int32)
    masks = np.zeros((n_tors, n), dtype=np.uint8)
    for t, c in enumerate(centres):
        masks[t, c + 1:min(n, c + 1 + int(rng.integers(2, max(3, n // 2))))] = 1
    if turn_i2 is not None:
        masks[turn_i2, centres[turn_i2]] = 1
    if big is not None:
        torsions[big] = (0, 1, 2, 3)
        masks[big] = 0
        masks[big, 2:] = 1
        assert int(masks[big].sum()) > 64
    angles = rng.choice(ANGLES, size=(n_rows, n_tors)).astype(np.int32)
    return torsions, masks, angles


def rigid_copies(rng, base, count):
    """`base` and count - 1 rotated and shifted copies of it: a candidate built from the wrong start is off by angstroms."""
    from tscode_amd.synthetic import quat_to_mat
    out = [base]
    for _ in range(count - 1):
        out.append(base @ quat_to_mat(rng.normal(size=4)).T + rng.normal(size=3) * 4.0)
    return np.array(out)


def oracle_per_start(oracle, starts, sets, set_of_start, rows, thresh=THRESH, max_clashes=0):
    """The yardstick: one oracle.csearch_rotate per start, each required to sit more than 1e-9 A from the clash threshold."""
    outs, rbs = [], []
    for s, x in enumerate(starts):
        torsions, masks, angles = sets[set_of_start[s]]
        r = np.arange(len(angles)) if rows is None else np.asarray(rows[s], dtype=int)
        if not len(r):
            continue
        out, rb, margin = oracle.csearch_rotate(x, torsions, masks, angles[r], thresh, max_clashes, return_margin=True)
        assert margin > 1e-9, f"start {s}: a clash decision within {margin:.1e} A of the threshold"
        outs.append(out), rbs.append(rb)
    return np.concatenate(outs), np.concatenate(rbs)


def check_multi(oracle, starts, sets, set_of_start, rows, max_clashes=0):
    import tscode_amd
    out, rb, si, ri = tscode_amd.csearch_rotate_multi(starts, sets, set_of_start, rows, THRESH, max_clashes)
    ref_out, ref_rb = oracle_per_start(oracle, starts, sets, set_of_start, rows, THRESH, max_clashes)
    want_rows = [np.arange(len(sets[set_of_start[s]][2])) if rows is None else np.asarray(rows[s], dtype=int) for s in range(len(starts))]
    assert np.array_equal(si, np.repeat(np.arange(len(starts)), [len(r) for r in want_rows]))
    assert np.array_equal(ri, np.concatenate(want_rows))
    assert np.array_equal(rb, ref_rb)
    assert out.shape == ref_out.shape and np.abs(out - ref_out).max() < VAL_TOL
    return rb


_g24 = {}


def g24():
    if "g" not in _g24:
        _g24["g"] = load_golden("G24_csearch_multi")
    return _g24["g"]


def g24_b_sets(g):
    return [(g[f"b_torsions{s}"], g[f"b_masks{s}"], g[f"b_angles{s}"]) for s in range(int(g["b_n_starts"]))]


# ----------------------------------------------------------------------------- host (no GPU)
def test_header_prototypes_and_library_declare_the_entry_points():
    import tscode_amd
    from tscode_amd import _lib
    from tscode_amd.build import build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tscode_hip.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", build()], check=True, capture_output=True, text=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"{s} not declared in include/tscode_hip.h"
        assert s in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bT %s$" % s, exported, flags=re.M), f"{s} not exported by the library"
    for name in ("csearch_rotate_multi", "csearch_candidates_multi", "clustered_csearch_step"):
        assert callable(getattr(tscode_amd, name))


def test_kept_rows_is_the_reference_loop():
    from tscode_amd.torsion_module import _kept_rows
    rng = np.random.default_rng(2401)
    cases = [np.zeros(0, int), np.zeros(9, int), np.ones(9, int), np.array([0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1]), np.array([3, 0, 2, 0, 0, 1])]
    cases += [(rng.random(int(rng.integers(1, 300))) < p).astype(int) for p in (0.05, 0.3, 0.5, 0.9) for _ in range(12)]
    for rotated in cases:
        kept_at = np.flatnonzero(rotated)
        dropped_at = np.flatnonzero(rotated == 0)
        tries = [10000, len(rotated), len(rotated) + 5, 0]
        tries += [int(kept_at[len(kept_at) // 2])] if len(kept_at) else []           # row max_tries is a kept row
        tries += [int(dropped_at[len(dropped_at) // 2])] if len(dropped_at) else []   # ... a dropped row: the walk does not stop there
        for n_out in (1, 7, len(kept_at), len(kept_at) + 3, 0, None):
            for max_tries in tries:
                rows, walked = _kept_rows(rotated, n_out, max_tries)
                want_rows, want_walked = literal_loop(rotated.tolist(), n_out, max_tries)
                assert rows.tolist() == want_rows and walked == want_walked, (rotated.tolist(), n_out, max_tries)
    # a dropped row max_tries does not stop the walk; a kept one does, after being appended
    assert _kept_rows([1, 0, 1, 1], None, 1)[0].tolist() == [0, 2, 3]
    assert _kept_rows([1, 0, 1, 1], None, 2)[0].tolist() == [0, 2]


def test_refusals_raise_value_error_before_the_library_is_loaded(monkeypatch):
    import tscode_amd as ta
    from tscode_amd import torsion_module as tm

    def no_library(*a, **k):
        raise AssertionError("the library was asked for before the arguments were refused")
    monkeypatch.setattr(tm, "get_engine", no_library)
    x = np.zeros((2, 6, 3))
    tors, mask = [(0, 1, 2, 3)], np.zeros((1, 6), np.uint8)
    one = (tors, mask, np.zeros((4, 1), np.int32))
    refusals = [
        lambda f: f([np.zeros((6, 3)), np.zeros((5, 3))], [one]),                              # unequal atom counts among the starts
        lambda f: f(x, [(tors, np.zeros((1, 5), np.uint8), np.zeros((4, 1), np.int32))]),      # ... between a set and the starts
        lambda f: f(x, [one, one], [0, 2]),                                                    # set_of_start out of range
        lambda f: f(x, [one, one], [0, -1]),
        lambda f: f(np.zeros((3, 6, 3)), [one, one]),                                          # 2 sets for 3 starts and no set_of_start
        lambda f: f(x, [(tors, mask, np.zeros((4, 2), np.int32))]),                            # a table wider than its set
        lambda f: f(x, [([(0, 1, 2, 6)], mask, np.zeros((4, 1), np.int32))]),                  # atom index out of range
        lambda f: f(np.zeros((1, 3000, 3)), [([(0, 1, 2, 3)] * 20, np.zeros((20, 3000), np.uint8), np.zeros((2, 20), np.int32))]),   # LDS overflow
    ]
    for fn in (ta.csearch_rotate_multi, ta.csearch_candidates_multi):
        for refusal in refusals:
            with pytest.raises(ValueError):
                refusal(fn)
    with pytest.raises(ValueError, match="torsion set 1: 3000 atoms x 20 torsions exceed the LDS staging"):
        ta.csearch_rotate_multi(np.zeros((1, 3000, 3)), [([(0, 1, 2, 3)], np.zeros((1, 3000), np.uint8), np.zeros((2, 1), np.int32)),
                                                        ([(0, 1, 2, 3)] * 20, np.zeros((20, 3000), np.uint8), np.zeros((2, 20), np.int32))], [0])
    with pytest.raises(ValueError):
        ta.csearch_rotate_multi(x, [one], rows=[[0], [4]])                                     # a row past the table
    with pytest.raises(ValueError):
        ta.clustered_csearch_step(x, tors, mask)                                               # neither angles nor n-folds


# ----------------------------------------------------------------------------- G24 (GPU)
@pytest.mark.gpu
def test_g24_part_a_clustered_csearch_groups():
    """Every torsion group of the reference's clustered_csearch: starting points -> its ``new_structures`` array (:734-783)."""
    import tscode_amd
    g = g24()
    assert int(g["a_n_groups"]) >= 2
    differing = False
    for k in range(int(g["a_n_groups"])):
        starts, tors, masks, want = g[f"a_starts{k}"], g[f"a_torsions{k}"], g[f"a_masks{k}"], g[f"a_out{k}"]
        got = tscode_amd.clustered_csearch_step(starts, tors, masks, n_folds=g[f"a_nfolds{k}"])
        assert got.shape == want.shape and np.abs(got - want).max() < VAL_TOL
        got = tscode_amd.clustered_csearch_step(starts, tors, masks, angles=g[f"a_angles{k}"])
        assert got.shape == want.shape and np.abs(got - want).max() < VAL_TOL
        same, index = tscode_amd.csearch_candidates_multi(starts, [(tors, masks, g[f"a_angles{k}"])], n_out=None, include_start=True)
        assert np.array_equal(same, got)
        assert np.array_equal(np.bincount(index, minlength=len(starts)), g[f"a_kept_per_start{k}"] + 1)
        differing |= len(set(g[f"a_kept_per_start{k}"].tolist())) > 1
    assert differing            # starts of one group that keep different numbers of candidates


@pytest.mark.gpu
@pytest.mark.parametrize("block", [None, 64, 128, 1000])
def test_g24_part_b_random_csearch_per_start(block):
    """The reference's random_csearch once per start (own torsions, own shuffled table): stop on n_out (run 0), and a max_tries
    that is a kept row of start 1's table and a dropped row of start 2's (run 1).  The same result for every block size."""
    import tscode_amd
    g = g24()
    sets = g24_b_sets(g)
    assert block is None or block != 1000 or all(block > len(s[2]) for s in sets)
    for run in (0, 1):
        got, index = tscode_amd.csearch_candidates_multi(g["b_starts"], sets, n_out=int(g[f"b_n_out{run}"]), max_tries=int(g[f"b_max_tries{run}"]),
                                                         block=block)
        assert np.array_equal(np.bincount(index, minlength=len(sets)), g[f"b_counts{run}"])
        assert got.shape == g[f"b_out{run}"].shape and np.abs(got - g[f"b_out{run}"]).max() < VAL_TOL
    assert g["b_counts1"][1] < g["b_full_count1"] and g["b_counts1"][2] == g["b_full_count2"]


# ----------------------------------------------------------------------------- the oracle per start (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("n", [12, 38, 70, 200])
def test_multi_equals_the_oracle_per_start(oracle, n):
    """3 sets of 1, 5 and 8 torsions (zero-padded columns), 7 starts that are rigid copies of one another with a set order that is
    not monotone, one start without rows, one mask that turns i2, and (n > 68) one torsion that turns more than 64 atoms."""
    from tscode_amd.synthetic import make_fragment
    rng = np.random.default_rng(2400 + n)
    base = make_fragment(rng, n)
    sets = [make_set(rng, n, 1, 23), make_set(rng, n, 5, 41, turn_i2=2), make_set(rng, n, 8, 33, turn_i2=6, big=3 if n > 68 else None)]
    assert int(sets[1][1][2, sets[1][0][2, 1]]) == 1
    starts = rigid_copies(rng, base, 7)
    set_of_start = [2, 0, 1, 0, 2, 1, 0]
    rows = [None, np.arange(23), np.arange(5, 41), [], np.arange(0, 33, 2), [40, 3, 3, 17], np.arange(22, -1, -1)]
    rows[0] = np.arange(33)
    rb = check_multi(oracle, starts, sets, set_of_start, rows)
    assert (rb == 0).any() and (rb > 1).any()
    rb_all = check_multi(oracle, starts, sets, set_of_start, None)            # rows=None: every start walks its whole table
    assert len(rb_all) == 3 * 23 + 2 * 41 + 2 * 33


@pytest.mark.gpu
def test_set_boundaries_inside_a_workgroups_batch(oracle):
    """Consecutive starts of different sets with 1, 5 and 67 candidates, enough of them (2400 work items of at most 4 candidates,
    2048 workgroups) that every workgroup walks items of several sets: one that kept the previous set's torsion lists fails."""
    from tscode_amd.synthetic import make_fragment
    rng = np.random.default_rng(2405)
    n = 20
    base = make_fragment(rng, n)
    sets = [make_set(rng, n, 1, 1), make_set(rng, n, 5, 5), make_set(rng, n, 8, 67)]
    starts = rigid_copies(rng, base, 9)[np.arange(360) % 9]
    set_of_start = np.arange(360) % 3
    check_multi(oracle, starts, sets, set_of_start, None)


@pytest.mark.gpu
def test_grid_stride_over_20000_candidates(oracle):
    """40 starts x 500 rows of a 12-atom, 2-torsion molecule: more work than the grid cap of 2048 workgroups covers at once."""
    from tscode_amd.synthetic import make_fragment
    rng = np.random.default_rng(2406)
    base = make_fragment(rng, 12)
    sets = [make_set(rng, 12, 2, 500)]
    rb = check_multi(oracle, rigid_copies(rng, base, 40), sets, np.zeros(40, int), None)
    assert len(rb) == 20000


@pytest.mark.gpu
def test_one_clash_allowed_takes_the_fp64_count(oracle):
    from tscode_amd.synthetic import make_fragment
    rng = np.random.default_rng(2407)
    base = make_fragment(rng, 38)
    sets = [make_set(rng, 38, 5, 60), make_set(rng, 38, 8, 60)]
    starts = rigid_copies(rng, base, 4)
    rb1 = check_multi(oracle, starts, sets, [1, 0, 0, 1], None, max_clashes=1)
    rb0 = check_multi(oracle, starts, sets, [1, 0, 0, 1], None, max_clashes=0)
    assert not np.array_equal(rb0, rb1)


# ----------------------------------------------------------------------------- selection (GPU)
def select_rounds(eng, flags, n_out, max_tries, block):
    """tsc_csearch_select_dev driven in rounds on made-up rotated_bonds: per start the rows taken (their coordinates carry the row's
    identity), kept_count, done and the rows walked; and the number of rounds each start took part in."""
    S, n = len(flags), 5
    state = [np.zeros(S, np.int32) for _ in range(3)]
    d_state = [eng.dev_upload(a) for a in state]
    next_row, rounds, walked = np.zeros(S, int), np.zeros(S, int), np.zeros(S, int)
    taken = [[] for _ in range(S)]
    try:
        while True:
            live = [s for s in range(S) if not state[1][s] and next_row[s] < len(flags[s])]
            if not live:
                break
            seg_len = [min(block, len(flags[s]) - next_row[s]) for s in live]
            rb = np.concatenate([flags[s][next_row[s]:next_row[s] + k] for s, k in zip(live, seg_len)]).astype(np.int32)
            ident = np.concatenate([1000.0 * s + np.arange(next_row[s], next_row[s] + k) for s, k in zip(live, seg_len)])
            cand = np.ascontiguousarray(ident[:, None, None] + np.arange(n * 3).reshape(n, 3) / 64.0)
            seg_off = np.concatenate([[0], np.cumsum(seg_len)]).astype(np.int32)
            bufs = [eng.dev_upload(a) for a in (cand, rb, seg_off, np.array(live, np.int32), next_row[live].astype(np.int32))]
            d_kept = eng.dev_alloc(cand.nbytes)
            before = state[0].copy()
            try:
                k = eng.csearch_select_dev(bufs[0], bufs[1], n, bufs[2], bufs[3], bufs[4], len(live), n_out, max_tries, *d_state, d_kept, len(cand))
                for a, d in zip(state, d_state):
                    eng.dev_download(d, a)
                rows = eng.dev_download(d_kept, np.empty((k, n, 3)))
            finally:
                for b in bufs + [d_kept]:
                    eng.dev_free(b)
            assert np.array_equal(rows - rows[:, :1, :1], np.broadcast_to(np.arange(n * 3).reshape(n, 3) / 64.0, rows.shape))   # whole rows
            at = 0
            for s, kk in zip(live, seg_len):
                got = state[0][s] - before[s]
                ids = rows[at:at + got, 0, 0]
                assert np.all(ids // 1000 == s)
                taken[s] += (ids - 1000.0 * s).astype(int).tolist()
                at += got
                walked[s] += state[2][s]
                rounds[s] += 1
                next_row[s] += kk
            assert at == k
    finally:
        for d in d_state:
            eng.dev_free(d)
    return taken, state[0].copy(), state[1].copy(), walked, rounds


@pytest.mark.gpu
@pytest.mark.parametrize("n_out", [1, 7, 500, None])
def test_device_selection_equals_the_host_rule(eng, n_out):
    """n_out below, at and above the rows available; max_tries on a kept row, on a dropped row and beyond the table; a start that
    finishes in round 1 beside one that needs 3 rounds, one whose table ends inside a wavefront's chunk, one with nothing kept."""
    from tscode_amd.torsion_module import _kept_rows
    rng = np.random.default_rng(2408)
    dense = np.ones(150, int)
    sparse = np.zeros(190, int)
    sparse[np.arange(19, 190, 20)] = 1                               # 1 row in 20: the 7th kept row is row 139, in round 3 of 64
    flags = [dense, sparse, (rng.random(131) < 0.5).astype(int), np.zeros(70, int), (rng.random(64) < 0.3).astype(int), np.ones(1, int)]
    flags[2][77], flags[2][78] = 1, 0
    for max_tries in (77, 78, 10000):                                # rows 77 / 78 of start 2: kept / dropped
        taken, kept_count, done, walked, rounds = select_rounds(eng, flags, n_out, max_tries, 64)
        for s, f in enumerate(flags):
            rows, consumed = _kept_rows(f, n_out, max_tries)
            assert taken[s] == rows.tolist() and kept_count[s] == len(rows), (s, n_out, max_tries)
            assert done[s] == int(consumed < len(f) or (len(rows) and (len(rows) == n_out or rows[-1] == max_tries)))
            assert walked[s] == consumed
            assert rounds[s] == -(-consumed // 64)
        if n_out == 7 and max_tries == 10000:
            assert rounds[0] == 1 and rounds[1] == 3
        one_block = select_rounds(eng, flags, n_out, max_tries, 1000)
        assert one_block[0] == taken and np.array_equal(one_block[1], kept_count) and np.array_equal(one_block[3], walked)


@pytest.mark.gpu
def test_candidates_multi_equals_the_single_start_path_and_orders_the_starts(oracle):
    """Per start the rows csearch_candidates returns; include_start puts each start in front of its own candidates; one start
    finishes in the first round while another walks three."""
    import tscode_amd
    from tscode_amd.synthetic import make_fragment
    rng = np.random.default_rng(2409)
    n = 38
    base = make_fragment(rng, n)
    sets = [make_set(rng, n, 5, 300), make_set(rng, n, 8, 170), make_set(rng, n, 1, 90)]
    sets[1][2][rng.random(170) < 0.9] = 0                            # a table that mostly rotates nothing: 10 kept rows need many rows
    starts = rigid_copies(rng, base, 5)
    set_of_start = [1, 0, 2, 1, 0]
    for n_out, max_tries in ((10, 10000), (25, 40), (None, 10000)):
        singles = [tscode_amd.csearch_candidates(starts[s], *sets[k], n_out=10**9 if n_out is None else n_out,
                                                 max_tries=-1 if n_out is None else max_tries, thresh=THRESH) for s, k in enumerate(set_of_start)]
        for block in (None, 64):
            got, index = tscode_amd.csearch_candidates_multi(starts, sets, set_of_start, n_out=n_out, max_tries=max_tries, thresh=THRESH, block=block)
            assert np.array_equal(np.bincount(index, minlength=5), [len(x) for x in singles])
            assert np.abs(got - np.concatenate(singles)).max() < VAL_TOL
        with_start, index2 = tscode_amd.csearch_candidates_multi(starts, sets, set_of_start, n_out=n_out, max_tries=max_tries, thresh=THRESH,
                                                                 include_start=True)
        want = np.concatenate([np.concatenate([starts[s][None], singles[s]]) for s in range(5)])
        assert np.array_equal(np.bincount(index2, minlength=5), [len(x) + 1 for x in singles])
        assert np.array_equal(with_start[np.flatnonzero(np.diff(index2, prepend=-1))], starts)
        assert np.abs(with_start - want).max() < VAL_TOL
    # the single-start yardstick itself against the oracle, once
    ref_out, ref_rb = oracle_per_start(oracle, starts[:1], sets, set_of_start[:1], None)
    assert np.abs(tscode_amd.csearch_candidates(starts[0], *sets[1], n_out=10**9, max_tries=-1, thresh=THRESH) - ref_out[ref_rb != 0]).max() < VAL_TOL
