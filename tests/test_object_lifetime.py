"""The one ownership rule of the objects created from a context (include/tscode_hip.h, "objects created from a context"; csrc/owned.hpp;
tscode_amd.engine.ContextObject), for all five kinds at their smallest shapes: tsc_prune, tsc_rot_corr, tsc_rot_corr_batch, tsc_embed_prune
and tsc_xchg.  Per kind: the object is destroyed, then its context; the context is destroyed with the object alive, listed by nothing but
the context; the engine is closed before the object's own close().  After every teardown a fresh context on the same device prunes 64
structures and must give the oracle's verdicts -- the yardstick is never the library.  No test destroys an object twice or uses one
after its context has gone: those remain the caller's error.  The list itself is checked on the CPU, under sanitizers (test_owned.py)."""

import ctypes as C

import numpy as np
import pytest

from test_embed_prune import CASES, THRESH, angle_sets, atomnos_for, group_records, slab_args
from test_rot_corr import centred
from test_rot_corr_batch import EDGE_SIZES, edge_ensembles
from test_rot_corr_sweep import THR

gpu = pytest.mark.gpu

KINDS = ["prune", "rot_corr", "rot_corr_batch", "embed_prune", "xchg"]
DESTROY = {"prune": "tsc_prune_destroy", "rot_corr": "tsc_rot_corr_destroy", "rot_corr_batch": "tsc_rot_corr_batch_destroy",
           "embed_prune": "tsc_embed_prune_destroy", "xchg": "tsc_xchg_destroy"}
HANDLE = {"prune": "_p", "rot_corr": "_r", "rot_corr_batch": "_r", "embed_prune": "_r", "xchg": "_x"}      # the name each class reads its handle by
RMSD_THR = 0.5


def small_heavy():
    """64 structures of 4 heavy atoms: 16 shapes, four copies of each with 0.01 A of noise, shuffled."""
    rng = np.random.default_rng(3600)
    shapes = rng.normal(size=(16, 4, 3)) * 2.0
    heavy = np.repeat(shapes, 4, axis=0) + rng.normal(size=(64, 4, 3)) * 0.01
    return np.ascontiguousarray(heavy[rng.permutation(64)])


_want = {}


def oracle_mask(oracle):
    """The oracle's verdicts on small_heavy(), computed once and left unchanged, with its guard band shown first."""
    if not _want:
        heavy = small_heavy()
        margins = oracle.prune_margins(heavy, RMSD_THR, 0)
        assert min(margins) > 1e-6, margins
        mask = np.asarray(oracle.prune_conformers_rmsd(heavy, np.full(4, 6), RMSD_THR, 0)[1], dtype=bool)
        assert 0 < mask.sum() < 64                         # (something is pruned, something survives)
        _want["mask"] = mask
    return _want["mask"]


def a_fresh_context_works(oracle):
    from tscode_amd.engine import Engine
    fresh = Engine(0)
    try:
        mask, stats = fresh.prune_heavy(small_heavy(), RMSD_THR, 0)
        assert np.array_equal(mask, oracle_mask(oracle)) and len(stats) >= 1
    finally:
        fresh.close()


def make(kind, e, oracle):
    """Objects of one kind on engine e, each having done some work: (objects, what to free on e before its context goes)."""
    from tscode_amd import _lib
    from tscode_amd.engine import FragmentSet, IpcExchange
    import tscode_amd.rot_corr as rc
    if kind == "prune":
        heavy = small_heavy()
        d_heavy = C.c_void_p()
        _lib.check(e.lib.tsc_malloc(e._h, heavy.nbytes, C.byref(d_heavy)))
        _lib.check(e.lib.tsc_memcpy_h2d(e._h, d_heavy, _lib.ptr(heavy), heavy.nbytes))
        st = e.prune_stepper(d_heavy.value, 64, 4, RMSD_THR, 0)
        passes = 0
        while st.next_pass() != 0:
            st.pass_local(0, 1)
            st.pass_finish()
            passes += 1
        mask = np.empty(64, dtype=np.uint8)
        _lib.check(e.lib.tsc_memcpy_d2h(e._h, _lib.ptr(mask), C.c_void_p(st.mask_ptr()), mask.nbytes))
        assert passes >= 1 and np.array_equal(mask.astype(bool), oracle_mask(oracle))
        return [st], lambda: _lib.check(e.lib.tsc_free(e._h, d_heavy))
    if kind in ("rot_corr", "rot_corr_batch"):
        mol, ens = edge_ensembles()
        two = [centred(ens[EDGE_SIZES.index(N)]) for N in (9, 17)]
        setup = rc._Setup(mol.coords.shape[0], mol.atomnos, **mol.setup())
        if kind == "rot_corr":
            runs = [rc._Run(e, s, setup) for s in two]
            for run, N in zip(runs, (9, 17)):
                first, ev = run.run_pass(N, 1, N, THR)
                assert first.shape == (N,) and ev > 0
            return runs, None
        run = rc._BatchRun(e, two, [setup] * 2)
        first, ev = run.run_slot(np.array([0, 1]), np.array([9, 17]), 1, np.array([9, 17]), np.array([THR, THR]))
        assert first.shape == (26,) and ev.shape == (2,) and ev.min() > 0
        return [run], None
    if kind == "embed_prune":
        mols = CASES["two"]["mols"]()
        coords, blocks, _ = group_records(mols)
        run = e.embed_prune_run(FragmentSet(coords), np.flatnonzero(atomnos_for(sum(c.shape[1] for c in coords)) != 1))
        assert run.add_groups(*slab_args(blocks, 0, 2, angle_sets(2)), THRESH, 0, 1.0)[1].any() and run.count() > 0
        return [run], None
    x = IpcExchange(e, 0, 1, IpcExchange.slot_bytes(e.lib, 64, 0))      # (a world of one: no peer is mapped, no kernel is launched)
    assert len(x.handle) == _lib.XCHG_HANDLE_BYTES and x.status() == (0, 0)
    return [x], None


def forget(objs):
    """The handles are gone with their context: nothing is to be called on them again, not even by a finaliser."""
    for o in objs:
        o._handle = None


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_object_goes_first_then_its_context(kind, oracle):
    from tscode_amd.engine import Engine
    e = Engine(0)
    lib = e.lib
    destroy = getattr(lib, DESTROY[kind])
    assert destroy(None) == 0                              # (null is success)
    objs, release = make(kind, e, oracle)
    e._runs.clear()
    for o in objs:                                         # (oldest first: the order is the caller's)
        assert destroy(o._handle) == 0, lib.tsc_last_error().decode()
    forget(objs)
    if release:
        release()
    assert lib.tsc_ctx_destroy(e._h) == 0
    e._h = None
    a_fresh_context_works(oracle)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_context_goes_with_the_object_alive(kind, oracle):
    from tscode_amd.engine import Engine
    e = Engine(0)
    objs, release = make(kind, e, oracle)
    e._runs.clear()                                        # nobody but the context lists them
    if release:
        release()
    assert e.lib.tsc_ctx_destroy(e._h) == 0
    e._h = None
    forget(objs)
    a_fresh_context_works(oracle)


class Spy:
    """The library, with the names of the entry points called through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


@gpu
@pytest.mark.parametrize("known", [True, False], ids=["known", "discarded"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_closed_engine_has_closed_its_objects(kind, known, oracle):
    """engine.close(), then the object's close() is a no-op and its handle is None: with the object known to engine._runs (the engine closes
    it, once) and after discard (tsc_ctx_destroy frees it; no destroy call is made on its handle, then or later)."""
    from tscode_amd.engine import Engine
    e = Engine(0)
    objs, release = make(kind, e, oracle)
    if release:
        release()
    if not known:
        for o in objs:
            e._runs.discard(o)
    e.lib = spy = Spy(e.lib)
    e.close()
    assert e._h is None
    assert sorted(spy.calls) == sorted([DESTROY[kind]] * (len(objs) if known else 0) + ["tsc_ctx_destroy"]), spy.calls
    if known:
        assert all(o._handle is None for o in objs)
    for o in objs:
        o.close()
        assert o._handle is None and getattr(o, HANDLE[kind]) is None
        o.close()
    assert spy.calls.count("tsc_ctx_destroy") == 1 and len(spy.calls) == (len(objs) if known else 0) + 1, spy.calls
    del objs
    a_fresh_context_works(oracle)
