"""clustered_csearch_batch with the trims and finals of a slice going through the batched calls (most_diverse_conformers_batch,
prune_conformers_tfd_batch) and with every structure closed on its own: identical arrays.  The per-structure route is the yardstick."""

import numpy as np
import pytest

from test_clustered_csearch import g26, part_b_inputs


def run(monkeypatch, min_poses, poses, atomnos, **kw):
    import tscode_amd
    from tscode_amd import torsion_module as tm
    monkeypatch.setattr(tm, "CLUSTERED_BATCH_MIN_POSES", min_poses)
    info, timings = {}, {}
    out, start = tscode_amd.clustered_csearch_batch(poses, atomnos, info=info, timings=timings, **kw)
    return out, start, info, timings


@pytest.mark.gpu
def test_batch_route_and_per_structure_route_return_identical_arrays(monkeypatch):
    from tscode_amd import torsion_module as tm
    _, meta = g26()
    poses, atomnos, init_rows = part_b_inputs()
    # the three poses, and five with the first two again at the end: slices in which some structures close while others go on
    more = np.concatenate([poses, poses[:2]])
    rows5 = dict(init_rows)
    rows5.update({(3 + k, c): v for (k, c), v in init_rows.items() if k < 2})
    calls = {"batch": 0}
    real = tm.most_diverse_conformers_batch
    monkeypatch.setattr(tm, "most_diverse_conformers_batch", lambda *a, **k: (calls.__setitem__("batch", calls["batch"] + 1), real(*a, **k))[1])
    for x, kw in ((poses, dict(init_rows=init_rows)), (poses, dict(seed=77)), (more, dict(init_rows=rows5)), (more, dict(seed=5, n=30, n_out=40))):
        kw = dict(dict(n=meta["n"], n_out=meta["n_out"]), **kw)
        calls["batch"] = 0
        off = run(monkeypatch, 10**9, x, atomnos, **kw)
        assert calls["batch"] == 0, "the per-structure route went through the batched call"
        on = run(monkeypatch, 1, x, atomnos, **kw)
        assert calls["batch"] > 0, "the forced batch route never reached the batched call"
        assert on[0].shape == off[0].shape and np.array_equal(on[0].view(np.uint64), off[0].view(np.uint64)), "the structures differ in their bits"
        assert np.array_equal(on[1], off[1]) and on[2]["round_sizes"] == off[2]["round_sizes"]
        assert set(on[3]) == set(off[3]) and len(on[3]["trim_ms"]) == len(off[3]["trim_ms"]) == len(on[3]["rotation_ms"])
        assert len(on[0]) > len(x)


def test_the_route_constant_is_a_module_constant():
    from tscode_amd import torsion_module as tm
    assert isinstance(tm.CLUSTERED_BATCH_MIN_POSES, int) and tm.CLUSTERED_BATCH_MIN_POSES >= 1
