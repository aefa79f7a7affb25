"""The work items of the 16-row matrix-core pair kernel (csrc/mm.hpp: k_rmsd_sieve_mm16, sieve_item_mm16) at the shapes where an item's
shape can go wrong: the segment ends, the alignment of the segment base, the last partial row and column tile, both sides of every threshold
of the rule that picks segment length and items per workgroup (csrc/pass_plan.hpp: mm16_item_shape), items that leave in their prologue, and
queues that drain between column tiles.

Every case runs the whole prune with "local_pass" = 0 -- every pass walks -- and "sieve_mm16" = 1, in both modes, and is compared with
oracle.prune_heavy exactly (no tolerance is involved): the mask, and per pass n_active_after and pairs_evaluated.

A pass of k chunks exists only while 20 k < n (rmsd_pruning.py:192).  The k = 1 pass has max_range = n, so its last segment ends
n + 64 - n_seg x seg_cols columns into (or short of) a segment: the "end_*" cases put n + 64 one below, at and one above a whole number of
segments of every length (forced through "seg_cols").  A forced length is halved like the rule's own while a row's range is shorter than four
segments (pass_plan.hpp: plan_walked), so "one segment" and "two segments" exist at 256 columns only; at 512 and 1 024 the cases stand at
five and at six segments (n >= 4 x the length: END_SEGS), at 2 048 at five (10 176 structures; six would be 12 224 and seconds of oracle
time).  The length named is the length of the k = 1 pass only: the shorter ranges of the other passes halve it.  tools/probe/pass_plan_check.cpp
asserts, without a GPU, that plan_walked gives every case's k = 1 pass the length and the segment count the case is named for.
All of those n are 64 m - 1, 64 m and 64 m + 1, the three alignments of the segment base ((r0 + 1) & ~63) against the last row tile.

Items per workgroup (pass_plan.hpp: mm16_items_per_workgroup; tools/probe/pass_plan_check.cpp works these shapes out by hand, without a GPU).
The sweep that led to the rule found one item per workgroup no better than two in any pass, so that instantiation was not added: there are two.
  * 2: every pass of every case but one -- a row's range of at most 64 segments (of 512 columns, or of the shorter ones "seg_cols" sets);
  * 4: the k = 1 pass of "seg256_16321" ("seg_cols" = 256 on 16 321 structures: 16 385 columns > 64 x 256, 65 segments); its other passes take 2.
    Four items on segments of 1 024 columns -- the flagship's last pass -- need a row's range beyond 32 704 columns, i.e. 32 705 structures and
    more, whose reference takes the oracle tens of seconds: no case here; the bench's parity check (57 046 structures) is what covers it."""
import numpy as np
import pytest

from test_pass_close import per_pass

THR = 0.5


def families(n, h, seed, per_family=3, noise=0.01):
    """n structures drawn from n / per_family bases (+ noise), every row's base picked at random: near-copies at every distance, so that
    every pass of the schedule finds rows to remove and the later ones see what the earlier ones left."""
    rng = np.random.default_rng(seed)
    bases = rng.normal(size=(max(1, n // per_family), h, 3)) * 2
    return np.ascontiguousarray(bases[rng.integers(0, len(bases), size=n)] + rng.normal(size=(n, h, 3)) * noise)


def adjacent_copies(bases, copies, h, seed):
    rng = np.random.default_rng(seed)
    heavy = np.repeat(rng.normal(size=(bases, h, 3)) * 2, copies, axis=0)
    return np.ascontiguousarray(heavy + rng.normal(size=heavy.shape) * 0.01)


def local_children(n, seed, children=10, spread=200.0):
    """tscode_amd.synthetic.make_ensemble with a local shuffle (the parity tests' generator): siblings meet in the fine passes, so that
    every pass finds duplicates and mode 0 leaves cache keys that stop rows early."""
    from tscode_amd.synthetic import make_ensemble
    ens = make_ensemble(n, (15, 15), seed=seed, children=children, local_spread=spread)
    return np.ascontiguousarray(ens.poses()[:, ens.atomnos != 1])


# segment length: the whole numbers of segments n + 64 is put around (the fewest that leave the forced length unhalved, and one more)
END_SEGS = {256: (1, 2), 512: (5, 6), 1024: (5, 6), 2048: (5,)}
# name: (builder, "seg_cols" -- 0: the rule's own choice)
CASES = {}
for seg, counts in END_SEGS.items():
    for n_seg in counts:
        for d in (-1, 0, 1):
            n = n_seg * seg - 64 + d        # max_range + 64 of the k = 1 pass = n + 64 = n_seg x seg + d
            CASES[f"end_{seg}_{n_seg}seg{d:+d}"] = (lambda n=n: families(n, 10, 7000 + n), seg)
# the last partial row tile and the last partial column tile: 1 000 = 62 x 16 + 8 = 7 x 128 + 104 on 256 columns; 4 200 = 262 x 16 + 8 = 32 x 128 + 104
# on 1 024 (4 200 >= 4 x 1 024)
CASES["partial_tiles_256"] = (lambda: families(1000, 10, 11), 256)
CASES["partial_tiles_1024"] = (lambda: families(4200, 10, 13), 1024)
# the rule's own choice on either side of its thresholds, in the k = 1 pass (max_range = n): 2 047 columns a row take segments of 256 and
# 2 048 of 512; 8 191 take 512 and 8 192 take 1 024.  9 000 (chunks of 4 500 in its k = 2 pass: 512; 1 024 in its k = 1 pass) with a local shuffle
CASES["rule_1000"] = (lambda: families(1000, 10, 11), 0)
CASES["rule_2111"] = (lambda: local_children(2111, 23), 0)
CASES["rule_2047"] = (lambda: families(2047, 10, 2047), 0)
CASES["rule_2048"] = (lambda: families(2048, 10, 2048), 0)
CASES["rule_8191"] = (lambda: families(8191, 10, 8191), 0)
CASES["rule_8192"] = (lambda: families(8192, 10, 8192), 0)
CASES["rule_9000"] = (lambda: local_children(9000, 29, children=6), 0)
CASES["seg256_16321"] = (lambda: families(16321, 10, 16321), 256)
# items that leave in their prologue: six ADJACENT copies of every base (found in the first pass, whose chunks of 30 hold five bases whole)
# leave the later passes a sixth of the rows the grid was sized for (tiles with
# r0 >= A); cached keys (mode 0) stop every row of some tiles before the segment (alive == 0 behind the loads).  Both under the rule's own lengths
CASES["dead_tiles"] = (lambda: adjacent_copies(500, 6, 10, 31), 0)
CASES["cached_keys"] = (lambda: local_children(3000, 41), 0)
# dense candidates: families of 50 at about the threshold from one another (noise 0.2: RMSD 0.4 - 0.6) -- most pairs of a family pass the
# screen, some are similar: the queue drains between tiles, the exact queue fills past 64, rows find their column mid-segment.  On the longest
# segments of this file: 2 048 columns in the k = 1 pass (8 256 structures >= 4 x 2 048), 1 024 in the k = 2 pass
CASES["dense"] = (lambda: families(8256, 10, 51, per_family=50, noise=0.2), 2048)

# the same ensemble under several segment lengths is built once and has one reference
SAME_AS = {"rule_1000": "partial_tiles_256"}

_heavy, _refs = {}, {}


def heavy_of(name):
    name = SAME_AS.get(name, name)
    if name not in _heavy:
        _heavy[name] = CASES[name][0]()
    return _heavy[name]


def reference(oracle, name, mode):
    name = SAME_AS.get(name, name)
    if (name, mode) not in _refs:
        _refs[name, mode] = oracle.prune_heavy(heavy_of(name), THR, mode=mode, row_parallel=True)
    return _refs[name, mode]


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_mask_and_every_pass_equal_the_oracle(eng, oracle, name, mode):
    heavy = heavy_of(name)
    ref = reference(oracle, name, mode)
    with eng.options(local_pass=0, sieve_mm16=1, seg_cols=CASES[name][1]):
        mask, stats = eng.prune_heavy(heavy, THR, mode)
    assert np.array_equal(mask, ref["mask"]), (name, mode, int(mask.sum()), int(ref["mask"].sum()))
    assert [(k, a) for k, _, a, _ in per_pass(stats)] == [(k, a) for k, _, a, _ in per_pass(ref["stats"])], (name, mode, "n_active_after")
    assert [(k, e) for k, _, _, e in per_pass(stats)] == [(k, e) for k, _, _, e in per_pass(ref["stats"])], (name, mode, "pairs_evaluated")
    assert all(int(s["algo"]) != 3 for s in stats), (name, "every pass was meant to walk")
    removing = [int(s["k"]) for s in ref["stats"] if s["n_active_after"] < s["n_active_before"]]
    if name in ("rule_2111", "rule_9000", "cached_keys"):
        assert len(removing) >= 3, (name, removing, "the local shuffle was meant to give several passes duplicates")
    if name == "dead_tiles":
        assert ref["stats"][-1]["n_active_before"] * 4 < len(heavy), "the last passes were meant to have far fewer rows than the grid"
    if name == "dense":
        # (8 evaluated pairs a row are 128 a row tile, two full batches of 64: no item of such a tile gets by with the one drain at its end)
        assert sum(int(s["pairs_evaluated"]) for s in ref["stats"]) > 8 * len(heavy), "the items were meant to evaluate many pairs"


# ---- without a GPU: the cases are what they say ----

def test_case_shapes():
    for seg, counts in END_SEGS.items():
        sizes = [len(heavy_of(f"end_{seg}_{n_seg}seg{d:+d}")) + 64 for n_seg in counts for d in (-1, 0, 1)]
        assert sizes == [m * seg + d for m in counts for d in (-1, 0, 1)]
        assert [-(-x // seg) for x in sizes] == [m + e for m in counts for e in (0, 0, 1)]
        assert sorted({(x - 64) % 64 for x in sizes}) == [0, 1, 63]
        # (plan_walked halves a length while max_range < 4 x the length, down to 256: the k = 1 pass of every case keeps the length it names)
        assert seg == 256 or min(sizes) - 64 >= 4 * seg
    n = len(heavy_of("partial_tiles_256"))
    assert n % 16 != 0 and n % 128 != 0
    n = len(heavy_of("partial_tiles_1024"))
    assert n % 16 != 0 and n % 128 != 0 and n >= 4 * 1024
    assert len(heavy_of("dense")) >= 4 * 2048
    assert [len(heavy_of(f"rule_{n}")) for n in (2047, 2048, 8191, 8192)] == [2047, 2048, 8191, 8192]    # 4 x 512, and MM16_WIDE_RANGE
    n = len(heavy_of("rule_9000"))
    assert [k for k in (500, 200, 100, 50, 20, 10, 5, 2, 1) if k == 1 or 20 * k < n] == [200, 100, 50, 20, 10, 5, 2, 1]
    assert n - (n // 2) < 8192 <= n
    n = len(heavy_of("seg256_16321"))
    assert -(-(n + 64) // 256) == 65 and n + 64 > 64 * 256      # four items per workgroup in the k = 1 pass
