"""The chunk-local pass kernel (csrc/local_pass.hpp, k_pass_chunks) evaluates its queues in ONE drain loop behind the column step: the exact
stage while 64 candidates have gathered, the sign stage while 64 pairs are queued, and behind the last column step the two remainders.
Every case goes through eng.prune_heavy in both modes and is compared with oracle.prune_heavy exactly as tests/test_pass_close.py does
(the final mask; per pass k, n_active_before, n_active_after, pairs_evaluated), and asserts from the run's statistics that the passes meant
took the chunk-local route (algo 3) and reached the path the case is there for.  Shapes: the smallest at which that path is taken."""
import numpy as np
import pytest

from test_pass_close import check, copies_at_distances, triplets

pytestmark = pytest.mark.gpu

LOCAL = 3      # PassStats.algo of a pass that ran in k_pass_chunks (include/tscode_hip.h)
TILE = 16      # rows of a work item (LP_TI)
WAVES = 4      # row tiles a workgroup is sized for (LP_TILES_PER_BLOCK)


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def by_k(stats):
    return {int(s["k"]): s for s in stats}


def blocks_of_chunk(rows):
    """Workgroups that share a chunk of `rows` structures (csrc/pass_plan.hpp, plan_local)."""
    return max(1, -(-(-(-rows // TILE)) // WAVES))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [600, 130])
def test_sign_queue_flushed_inside_the_column_loop(eng, oracle, n, mode):
    """Coinciding descriptors and (a rotation of its own per structure) next to nothing similar: the screen drops nothing and hardly a row
    leaves, so a 16-row tile queues up to 1 024 pairs per column step and the sign stage runs between the steps, batch after batch of
    64, then once more on the remainder.  n = 600: the k = 2 pass has chunks of 300 (19 row tiles, five column steps); n = 130: chunks of
    65, the second column tile holds ONE column.  The count is asserted on the run's first pass (chunks of 30 and 26 rows: one column step,
    drained where the steps of a longer chunk are) and, in mode 1, on the k = 2 pass: in mode 0 the cache's stop columns leave the later
    passes too few pairs for a statement from the pass's totals."""
    from tscode_amd.synthetic import make_unscreenable
    heavy = make_unscreenable(n, children=1)
    _, stats, _ = check(eng, oracle, f"unscreenable{n}", heavy, mode)
    assert int(by_k(stats)[2]["algo"]) == LOCAL, stats
    for k in [int(stats[0]["k"])] + ([2] if mode == 1 else []):
        s = by_k(stats)[k]
        assert int(s["algo"]) == LOCAL, s
        chunk = n // k + n % k                                   # the longest chunk of the pass
        steps = k * (-(-chunk // TILE)) * (-(-chunk // 64))      # (row tile, column step) combinations of the pass, at most
        # more pairs formed than 64 per combination: at least one step left 64 or more in the queue (in fact nearly all do)
        assert int(s["pairs_computed"]) > 64 * steps, (k, int(s["pairs_computed"]), steps)


@pytest.mark.parametrize("mode", [0, 1])
def test_exact_queue_flushed_at_64(eng, oracle, mode):
    """100 noisy copies of one base, 0.3 A apart: below the threshold, beyond what the near-duplicate test takes (2 thr / sqrt(h) = 0.18 A),
    so the sign stage can decide none of them and every pair it forms goes on to the exact stage: a sign batch of 64 fills the exact
    queue to 64 and the exact stage runs between two sign batches.  (Pairs ABOVE the threshold never get there: the sign test rejects
    them unless the margin is a rounding error.)  The k = 2 pass has two chunks of 50, four row tiles each."""
    rng = np.random.default_rng(17)
    n, h = 100, 30
    base = rng.normal(size=(h, 3)) * 2
    heavy = np.ascontiguousarray(base[None] + rng.normal(size=(n, h, 3)) * 0.12)
    _, stats, _ = check(eng, oracle, "copies100", heavy, mode)
    s = by_k(stats)[2]
    assert int(s["algo"]) == LOCAL, s
    tiles = 2 * (-(-50 // TILE))
    # more candidates than 64 per row tile: one tile at least sent more than 64 pairs to the exact stage
    assert int(s["candidates"]) > 64 * tiles, (int(s["candidates"]), tiles)


@pytest.mark.parametrize("mode", [0, 1])
def test_rows_stop_early_while_others_go_on(eng, oracle, mode):
    """Triplets of near-copies in chunks of 44, 88 and 176 rows (k = 20, 10, 5 of 880 structures; 44 is no multiple of 3, so triplets
    straddle chunk boundaries and meet in later passes): the last row tile of a chunk is partial, the active rows of a chunk are no
    multiple of 16, rows leave the screen as they find their copy, and in mode 0 the cache's stop columns cut rows short from the
    second pass on."""
    heavy = triplets(200, 10, 23, 280)
    assert len(heavy) == 880
    _, stats, ref = check(eng, oracle, "triplets880", heavy, mode)
    s = by_k(stats)
    assert all(k in s and int(s[k]["algo"]) == LOCAL for k in (20, 10, 5)), {k: int(v["algo"]) for k, v in s.items()}
    removing = [k for k in (20, 10, 5) if s[k]["n_active_after"] < s[k]["n_active_before"]]
    assert len(removing) >= 2, (removing, "the triplets were meant to meet in more than one pass")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,k", [(3299, 100), (1219, 20)])
def test_last_chunk_shared_by_several_workgroups(eng, oracle, n, k, mode):
    """The last chunk of a pass takes the remainder: 3 299 structures at k = 100 are chunks of 32 (one workgroup each) and a last chunk of
    131 (three workgroups deal its row tiles); 1 219 at k = 20 chunks of 60 and a last one of 79 (two).  Copies 1 to 120 rows apart, so
    rows of every workgroup of the last chunk find theirs."""
    last = n - (k - 1) * (n // k)
    assert blocks_of_chunk(n // k) == 1 and blocks_of_chunk(last) > 1, (n // k, last)
    heavy = copies_at_distances(n, 10, 31, distances=(1, 20, 50, 120), per_distance=min(150, n // 12))
    _, stats, _ = check(eng, oracle, f"copies{n}", heavy, mode)
    s = by_k(stats)
    assert int(s[k]["algo"]) == LOCAL, s[k]
    assert s[k]["n_active_after"] < s[k]["n_active_before"]
