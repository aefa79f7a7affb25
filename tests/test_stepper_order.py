"""The call order of the stepping API (tsc_prune_next_pass, _pass_local, _pass_rows, _pass_finish, ... -- include/tscode_hip.h): a call made
where the run's cursor (csrc/pass_cursor.hpp) does not allow it is refused by a host check with TSC_ERR_STATE before anything is enqueued, and
leaves the run as it was.  The triplet ensemble of tests/test_pass_close.py (450 structures of 10 heavy atoms: k = 20, 10, 5, 2, 1) is stepped
with every such call made at every point of the run that a single rank can reach without an exchange buffer; the run is then finished and
must still give oracle.prune_heavy's mask and per-pass counts, in both modes.  Three ways through the run, one per kind of launched pass:
chunk-local passes (the default at this size), walked passes that apply their own rows (local_max_chunk = 16), and passes whose row tiles
are dealt to two ranks -- pass_local(0, 2), pass_rows(1, 2) -- and applied behind the pair kernels."""
import ctypes as C

import numpy as np
import pytest

from test_pass_close import THR, per_pass, reference, triplets

pytestmark = pytest.mark.gpu

TSC_ERR_STATE = -5


@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def refused(call, text):
    from tscode_amd._lib import TscodeHipError
    with pytest.raises(TscodeHipError) as err:
        call()
    assert err.value.code == TSC_ERR_STATE and text in str(err.value), str(err.value)


def idle_calls(st):
    """what needs an open pass, made while none is"""
    return [(lambda: st.pass_local(0, 1), "tsc_prune_pass_local: no pass open (call tsc_prune_next_pass)"),
            (st.pass_range, "tsc_prune_pass_range: no pass open (call tsc_prune_next_pass)"),
            (st.pass_merge, "tsc_prune_pass_merge: tsc_prune_pass_range has not run"),
            (lambda: st.pass_rows(0, 2), "tsc_prune_pass_rows: needs an open pass whose tsc_prune_pass_local ran with world_size > 1"),
            (st.pass_finish, "tsc_prune_pass_finish: tsc_prune_pass_local has not run"),
            (st.pass_estimate, "tsc_prune_pass_estimate: no pass open"),
            (st.pass_partitioned, "tsc_prune_pass_partitioned: no pass open"),
            (st.views_range, "tsc_prune_views_ptr: no pass open"),
            (st.views_merged, "tsc_prune_views_merged: no pass open"),
            (st.best_ptr, "tsc_prune_best_ptr: no pass open")]


def open_calls(st, some_dev):
    """a pass is open and nothing of it has been launched"""
    return [(st.next_pass, "tsc_prune_next_pass: previous pass not finished"),
            (st.pass_range, "is not rank-partitioned"),
            (st.pass_merge, "tsc_prune_pass_merge: tsc_prune_pass_range has not run"),
            (lambda: st.pass_rows(0, 2), "tsc_prune_pass_rows: needs an open pass"),
            (st.pass_finish, "tsc_prune_pass_finish: tsc_prune_pass_local has not run"),
            (st.stats, "tsc_prune_stats: a pass is still open"),
            (lambda: st.use_best_buffer(some_dev), "tsc_prune_use_best_buffer: call it right after tsc_prune_create")]


def launched_calls(st, some_dev, dealt):
    """the pass's kernels are enqueued; pass_rows is legal only where the pass is applied behind them"""
    calls = [(st.next_pass, "tsc_prune_next_pass: previous pass not finished"),
             (lambda: st.pass_local(0, 1), "tsc_prune_pass_local: no pass open (call tsc_prune_next_pass)"),
             (st.pass_range, "tsc_prune_pass_range: no pass open (call tsc_prune_next_pass)"),
             (st.pass_merge, "tsc_prune_pass_merge: tsc_prune_pass_range has not run"),
             (st.stats, "tsc_prune_stats: a pass is still open"),
             (lambda: st.use_best_buffer(some_dev), "tsc_prune_use_best_buffer: call it right after tsc_prune_create")]
    if not dealt:
        calls.append((lambda: st.pass_rows(0, 2), "tsc_prune_pass_rows: needs an open pass"))
    return calls


WAYS = {"chunk-local": {}, "walked": {"local_max_chunk": 16}, "dealt": {}}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("way", list(WAYS))
def test_illegal_calls_are_refused_and_leave_the_run_as_it_was(eng, oracle, way, mode):
    from tscode_amd import _lib
    heavy = triplets(150, 10, 1, 0)
    n, lib = len(heavy), eng.lib
    ref = reference(oracle, "450", heavy, mode)
    dealt = way == "dealt"
    with eng.options(**WAYS[way]):
        d_heavy = C.c_void_p()
        _lib.check(lib.tsc_malloc(eng._h, heavy.nbytes, C.byref(d_heavy)))
        _lib.check(lib.tsc_memcpy_h2d(eng._h, d_heavy, _lib.ptr(heavy), heavy.nbytes))
        st = eng.prune_stepper(d_heavy.value, n, heavy.shape[1], THR, mode)
        ks = []
        try:
            for call, text in idle_calls(st):
                refused(call, text)
            while True:
                k = st.next_pass()
                if k == 0:
                    break
                ks.append(k)
                for call, text in open_calls(st, d_heavy.value):
                    refused(call, text)
                assert st.pass_estimate() == n * (n // k) // 2 and not st.pass_partitioned()
                st.pass_local(0, 2 if dealt else 1)
                for call, text in launched_calls(st, d_heavy.value, dealt):
                    refused(call, text)
                if dealt:
                    st.pass_rows(1, 2)
                    for call, text in launched_calls(st, d_heavy.value, dealt):
                        refused(call, text)
                st.pass_finish()
                for call, text in idle_calls(st) + [(lambda: st.use_best_buffer(d_heavy.value), "tsc_prune_use_best_buffer: call it right after")]:
                    refused(call, text)
            stats = st.stats()
            mask = np.empty(n, dtype=np.uint8)
            _lib.check(lib.tsc_memcpy_d2h(eng._h, _lib.ptr(mask), C.c_void_p(st.mask_ptr()), mask.nbytes))
        finally:
            st.close()
            _lib.check(lib.tsc_free(eng._h, d_heavy))
    assert ks == [20, 10, 5, 2, 1]
    assert np.array_equal(mask.astype(bool), ref["mask"]), (way, mode, int(mask.sum()), int(ref["mask"].sum()))
    assert per_pass(stats) == per_pass(ref["stats"]), (way, mode)
    algos = {int(s["algo"]) for s in stats}
    assert (3 in algos) == (way == "chunk-local"), (way, algos, "3: a pass of the chunk-local kernel")
