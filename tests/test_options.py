"""The library's tunables through the Python layer (tsc_ctx_set_option / tsc_ctx_get_option / tsc_option_info, csrc/options.hpp): a
context is enough, no workload runs.  Every test takes an engine of its own, not the process's shared one."""

import pytest

pytestmark = pytest.mark.gpu

# name: (a legal value that is not the default, a value the option refuses or None where it takes anything)
VALUES = {
    "prune_algo": (2, 3), "seg_cols": (512, 300), "drain_min": (16, 65), "sieve_trim": (0, 2), "sieve_mm": (2, 3), "mm_min_n": (5000, -1),
    "sieve_mm16": (0, 2), "mm_seg_cols": (128, 100), "sieve_cpl": (4, 3), "pca_min_n": (0, 2e9), "fuse_descriptors": (0, -1),
    "early_basis": (0, 0.5), "clash_first": (1, 2), "cull_tile_block": (16, 0), "stage1_f32": (2, None), "local_max_chunk": (128, 2049),
    "local_pass": (0, 2), "fused_apply": (0, 2), "open_lds_blocks": (128, -1), "clash_fp32": (0, 2), "clash_lanes": (0, 2),
    "deterministic_basis": (1, None), "cull": (2, 3), "cull_min_pairs": (5e6, -1), "cull_grid": (100, 0), "cull_xcd": (0, None),
    "prune_batch_max_n": (4096, 8193), "pass_timing": (2, 3),
}


@pytest.fixture
def eng():
    from tscode_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_a_fresh_context_holds_the_listed_defaults(eng):
    defaults = eng.option_defaults()
    assert len(defaults) >= 28
    for name, value in defaults.items():
        assert eng.get_option(name) == value, name
    assert eng.prune_batch_max_n == defaults["prune_batch_max_n"]


def test_every_option_takes_a_legal_value_and_refuses_an_illegal_one(eng):
    from tscode_amd._lib import TscodeHipError
    defaults = eng.option_defaults()
    listed = {name: v for name, v in VALUES.items() if name in defaults}
    assert set(defaults) - set(listed) <= {"dbg_stamp_k"} and len(listed) == len(VALUES)     # (dbg_stamp_k: measurement builds only)
    for name, (legal, illegal) in listed.items():
        assert legal != defaults[name], name
        eng.set_option(name, legal)
        assert eng.get_option(name) == legal, name
        if illegal is not None:
            with pytest.raises(TscodeHipError, match=name):
                eng.set_option(name, illegal)
            assert eng.get_option(name) == legal, name
    for name in ("no_such_option", ""):
        with pytest.raises(TscodeHipError, match="unknown option"):
            eng.set_option(name, 1)
        with pytest.raises(TscodeHipError, match="unknown option"):
            eng.get_option(name)
    eng.set_option("deterministic_basis", 5)        # non-zero means 1: what is stored is what is read
    assert eng.get_option("deterministic_basis") == 1


@pytest.mark.parametrize("before", [{}, {"cull": 0, "cull_min_pairs": 7e6, "sieve_mm": 2}], ids=["from-defaults", "from-other-values"])
def test_options_block_puts_back_what_was_there_when_it_raises(eng, before):
    for name, value in before.items():
        eng.set_option(name, value)
    was = {name: eng.get_option(name) for name in ("cull", "cull_min_pairs", "sieve_mm")}
    assert all(was[name] == value for name, value in before.items())
    with pytest.raises(ZeroDivisionError):
        with eng.options(cull=2, cull_min_pairs=0, sieve_mm=0):
            assert [eng.get_option(name) for name in ("cull", "cull_min_pairs", "sieve_mm")] == [2, 0, 0]
            raise ZeroDivisionError
    assert {name: eng.get_option(name) for name in was} == was
    # a refused value inside the block's own settings: the ones already set come back too
    from tscode_amd._lib import TscodeHipError
    with pytest.raises(TscodeHipError, match="sieve_mm"):
        with eng.options(cull=2, sieve_mm=7):
            pass
    assert {name: eng.get_option(name) for name in was} == was
