"""A prune pass is closed by the first kernel of the NEXT pass (csrc/pass_state.hpp, pass_derive), not by the last wavefront of its own: the
count of active structures, the bit copy of the mask in use and the gate of rmsd_pruning.py:192 are worked out from the state block and
the counters the pass left behind.  Checked here against oracle.prune_heavy, in both modes, through the one-call entry point: the final
mask and, per pass, (k, n_active_before, n_active_after, pairs_evaluated).

The fused device pipeline (tsc_pipeline_dev) embeds fragment ensembles itself and cannot be handed a heavy-atom array, so the first case is
not repeated through it; tests/test_gpu_parity.py::test_pipeline_c2_vs_oracle runs that entry point against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (500000, 200000, 100000, 50000, 20000, 10000, 5000, 2000, 1000, 500, 200, 100, 50, 20, 10, 5, 2, 1)   # rmsd_pruning.py:186-188
THR = 0.5


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def triplets(B, h, seed, tail):
    """Every base structure three times in adjacent rows, with noise far below the threshold; `tail` unrelated structures behind them."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(B, h, 3)) * 2
    heavy = np.repeat(base, 3, axis=0)
    heavy = heavy + rng.normal(size=heavy.shape) * 0.01
    if tail:
        heavy = np.concatenate([heavy, rng.normal(size=(tail, h, 3)) * 2])
    return np.ascontiguousarray(heavy)


def copies_at_distances(n, h, seed, distances=(1, 40, 400, 4000), per_distance=150):
    """Unrelated structures, some of which have a near-copy d rows further on: a pair meets in the first pass whose chunk holds both."""
    rng = np.random.default_rng(seed)
    heavy = rng.normal(size=(n, h, 3)) * 2
    used = np.zeros(n, dtype=bool)
    for d in distances:
        placed = 0
        for i in rng.permutation(n - d):
            if placed == per_distance:
                break
            if used[i] or used[i + d]:
                continue
            heavy[i + d] = heavy[i] + rng.normal(size=(h, 3)) * 0.01
            used[i] = used[i + d] = True
            placed += 1
        assert placed == per_distance
    return np.ascontiguousarray(heavy)


_refs = {}


def reference(oracle, key, heavy, mode):
    """The oracle's run of a case, computed once and shared (the rows of a pass side by side: the same masks and counts, sooner)."""
    if (key, mode) not in _refs:
        _refs[key, mode] = oracle.prune_heavy(heavy, THR, mode=mode, row_parallel=True)
    return _refs[key, mode]


def per_pass(stats):
    return [(int(s["k"]), int(s["n_active_before"]), int(s["n_active_after"]), int(s["pairs_evaluated"])) for s in stats]


def check(eng, oracle, key, heavy, mode):
    ref = reference(oracle, key, heavy, mode)
    mask, stats = eng.prune_heavy(heavy, THR, mode)
    assert np.array_equal(mask, ref["mask"]), (key, mode, int(mask.sum()), int(ref["mask"].sum()))
    assert per_pass(stats) == per_pass(ref["stats"]), (key, mode)
    return mask, stats, ref


GATE_CASES = {"450": (150, 10, 1, 0, 20, 10, 5, (151, 150)), "2111": (700, 10, 3, 11, 100, 50, 20, (711, 711))}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(GATE_CASES))
def test_gate_closes_between_two_passes_that_run(eng, oracle, name, mode):
    """A pass that is gated off between two that run: the derive carries the count and the bit copy through it unchanged."""
    B, h, seed, tail, k_before, k_off, k_after, survivors = GATE_CASES[name]
    heavy = triplets(B, h, seed, tail)
    n = len(heavy)
    ref = reference(oracle, name, heavy, mode)
    ran = [int(s["k"]) for s in ref["stats"]]
    # (from the oracle's own statistics, so that a changed generator cannot make the test vacuous)
    assert 20 * k_off < n, "the pass is in the schedule of this ensemble"
    assert k_before in ran and k_after in ran and k_off not in ran, (ran, "no pass gated off between two passes that ran")
    assert int(ref["mask"].sum()) == survivors[mode]
    check(eng, oracle, name, heavy, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_removals_in_consecutive_passes_of_both_shapes(eng, oracle, mode):
    """9 013 structures, divisible by no k: k = 200 has chunks of 45 (one launch per pass), k = 20 chunks of 450 and a longer last one
    (rows opened, then walked); the copies first meet their originals in different passes."""
    n = 9013
    assert all(n % k for k in KS if 1 < k and 20 * k < n)
    heavy = copies_at_distances(n, 10, 5)
    ref = reference(oracle, "9013", heavy, mode)
    removing = [int(s["k"]) for s in ref["stats"] if s["n_active_after"] < s["n_active_before"]]
    assert len(removing) >= 3, (removing, "fewer than three passes remove anything: move the copies")
    _, stats, _ = check(eng, oracle, "9013", heavy, mode)
    algos = {int(s["k"]): int(s["algo"]) for s in stats}
    assert algos[200] == 3 and algos[20] != 3, (algos, "both pass shapes were meant to run")


def test_three_runs_on_one_context(eng, oracle):
    """The state blocks and counters of every slot start afresh with each run: nothing of a longer schedule is left for a shorter one."""
    small, large = triplets(150, 10, 1, 0), triplets(700, 10, 3, 11)
    first = check(eng, oracle, "450", small, 0)
    check(eng, oracle, "2111", large, 0)
    third = check(eng, oracle, "450", small, 0)
    assert np.array_equal(first[0], third[0])
    assert per_pass(first[1]) == per_pass(third[1])


@pytest.mark.parametrize("mode", [0, 1])
def test_single_pass_run(eng, oracle, mode):
    """n = 37: 20 * 2 is not below 37, only k = 1 runs -- a pass that nothing precedes, closed where the run is exported."""
    rng = np.random.default_rng(9)
    base = rng.normal(size=(30, 6, 3)) * 2
    heavy = np.ascontiguousarray(np.concatenate([base, base[:7] + rng.normal(size=(7, 6, 3)) * 0.01]))
    assert len(heavy) == 37
    ref = reference(oracle, "37", heavy, mode)
    assert [int(s["k"]) for s in ref["stats"]] == [1]
    assert int(ref["mask"].sum()) == 30
    check(eng, oracle, "37", heavy, mode)
