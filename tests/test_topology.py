"""Batched bond graphs and scramble checks (tscode_amd.graph_manipulations, csrc/topology.hpp) against G21
(tests/golden/gen_topology.py): the reference's own graphize, molecule_check, scramble_check and get_double_bonds_indices.
The yardstick of the shapes G21 does not hold is the NumPy restatement below, itself pinned to G21 on the CPU."""

import importlib
import json
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

GUARD = 1e-10                     # the generator's guard: no pair within this distance of its threshold
MAX_NEWBONDS = (0, 1, 3)
SYMBOLS = ("tsc_bond_delta", "tsc_bond_delta_dev", "tsc_topology_timings")
CHAIN_CASES = ("chain50", "chain200")
_G21 = {}


def g21(case):
    if not _G21:
        _G21["meta"] = json.load(open(os.path.join(GOLDEN, "G21_topology.json")))
        _G21["files"] = {}
    meta = _G21["meta"]["cases"][case]
    fn = meta["file"]
    if fn not in _G21["files"]:
        _G21["files"][fn] = np.load(os.path.join(GOLDEN, fn), allow_pickle=False)
    z = _G21["files"][fn]
    d = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}
    return types.SimpleNamespace(meta=meta, **d)


def split_edges(flat, off):
    return [flat[off[s]:off[s + 1]].astype(np.int64) for s in range(len(off) - 1)]


# ------------------------------------------------------------------------------------------------------- the restatement
def restate(coords, classes, thr, active=None, ref_edges=None, excluded=None, max_newbonds=0):
    """Section "Semantics" of include/tscode_hip.h in NumPy: atoms i < j are bonded iff both are active and
    sqrt(dx dx + dy dy + dz dz) < thr[class_i][class_j] (a threshold of 0: never); care = neither atom excluded;
    formed = #{care & bonded & ~ref}, broken = #{care & ~bonded & ref}; mask = formed + broken <= max_newbonds.
    Returns (dense bool[N, n, n] upper triangle, formed, broken, mask, the smallest |distance - threshold|)."""
    coords = np.asarray(coords, dtype=np.float64)
    N, n = coords.shape[:2]
    iu = np.triu_indices(n, 1)
    t = np.asarray(thr, dtype=np.float64)[classes[iu[0]], classes[iu[1]]]
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    live = act[iu[0]] & act[iu[1]] & (t > 0)
    ref = np.zeros(len(t), bool)
    if ref_edges is not None and len(ref_edges):
        dense = np.zeros((n, n), bool)
        e = np.asarray(ref_edges).reshape(-1, 2)
        dense[e.min(1), e.max(1)] = True
        ref = dense[iu]
    exc = np.zeros((N, n), bool)
    if excluded is not None:
        ex = np.broadcast_to(np.asarray(excluded).reshape(-1, np.asarray(excluded).shape[-1]), (N, np.asarray(excluded).shape[-1]))
        for s in range(N):
            exc[s, ex[s][ex[s] >= 0]] = True
    adj = np.zeros((N, n, n), bool)
    formed, broken, margin = np.zeros(N, np.int32), np.zeros(N, np.int32), np.inf
    for lo in range(0, N, 256):
        x = coords[lo:lo + 256]
        d = x[:, iu[0]] - x[:, iu[1]]
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        if (t > 0).any():
            margin = min(margin, float(np.abs(dist - t)[:, t > 0].min()))
        bonded = live & (dist < t)
        care = ~(exc[lo:lo + 256][:, iu[0]] | exc[lo:lo + 256][:, iu[1]])
        formed[lo:lo + 256] = (care & bonded & ~ref).sum(1)
        broken[lo:lo + 256] = (care & ~bonded & ref).sum(1)
        adj[lo:lo + 256, iu[0], iu[1]] = bonded
    return adj, formed, broken, (formed.astype(np.int64) + broken) <= max_newbonds, margin


def packed(dense):
    """bool[N, n, n] -> u64[N, n, W] in the layout of tsc_bond_delta: bit (j & 63) of word j >> 6 of row i.  Plain NumPy, nothing
    from the module under test."""
    N, n = dense.shape[:2]
    w = (n + 63) // 64
    out = np.zeros((N, n, w), dtype=np.uint64)
    for j in range(n):
        out[:, :, j >> 6] |= dense[:, :, j].astype(np.uint64) * np.uint64(1 << (j & 63))
    return out


def unpacked_edges(rows):
    """u64[n, W] -> the bonds int64[E, 2] ordered by i then j, decoded here bit by bit."""
    rows = np.asarray(rows, dtype=np.uint64)
    return np.array([(i, 64 * w + b) for i in range(rows.shape[0]) for w in range(rows.shape[1]) for b in range(64)
                     if (int(rows[i, w]) >> b) & 1], dtype=np.int64).reshape(-1, 2)


def dense_edges(dense_one):
    i, j = np.nonzero(dense_one)
    return np.stack([i, j], 1)


def tables(g):
    from tscode_amd.graph_manipulations import bond_tables
    radii = {int(z): float(r) for z, r in zip(g.elements, g.radii)}
    return bond_tables(g.atomnos, radii)


# ------------------------------------------------------------------------------------------------------- CPU: the fixtures
def verdict_arrays(case):
    g = g21(case)
    if case == "masked50":
        return [("shared", g.shared_verdicts, g.shared_formed, g.shared_broken), ("per", g.per_verdicts, g.per_formed, g.per_broken)]
    return [("scramble", g.scramble_verdicts, g.formed, g.broken)]


@pytest.mark.parametrize("case", ["chain50", "chain200", "masked50", "bimol"])
def test_fixture_conditions(case):
    """What the generator asserts, asserted again on the files: both verdicts in every array (20 % each at least), formed and
    broken bonds in every family."""
    for name, verdicts, formed, broken in verdict_arrays(case):
        assert verdicts.shape[0] == len(MAX_NEWBONDS)
        for m, v in zip(MAX_NEWBONDS, verdicts):
            assert 0.2 <= v.mean() <= 0.8, (case, name, m, float(v.mean()))
        assert (formed > 0).any() and (broken > 0).any(), (case, name)


@pytest.mark.parametrize("case", ["chain50", "chain200", "bimol"])
def test_restatement_reproduces_the_reference(case):
    g = g21(case)
    classes, thr = tables(g)
    assert thr.tobytes() == g.thr.tobytes(), "bond_tables differs from the reference's 1.2 * (r1 + r2) in some bit"
    excluded = g.excluded if case == "bimol" else None
    ref_edges = split_edges(g.edges, g.edge_off)
    for m, mnb in enumerate(MAX_NEWBONDS):
        adj, formed, broken, mask, margin = restate(g.structures, classes, thr, None, g.expected_edges, excluded, mnb)
        assert margin > GUARD
        assert (mask == g.scramble_verdicts[m]).all()
        if case != "bimol":
            assert (mask == g.molecule_verdicts[m]).all()
    assert (formed == g.formed).all() and (broken == g.broken).all()
    for s in range(len(adj)):
        assert np.array_equal(dense_edges(adj[s]), ref_edges[s]), s
    if case != "bimol":   # the expected graph is the reference's graphize of the base
        base_adj = restate(g.base[None], classes, thr)[0][0]
        assert np.array_equal(dense_edges(base_adj), g.expected_edges.astype(np.int64))


def test_restatement_reproduces_the_masked_case():
    g, m50 = g21("chain50"), g21("masked50")
    classes, thr = tables(g)
    adj = restate(g.structures, classes, thr, m50.mask)[0]
    for s, e in enumerate(split_edges(m50.mask_edges, m50.mask_edge_off)):
        assert np.array_equal(dense_edges(adj[s]), e), s
    assert (m50.excluded_per == -1).all(axis=1).any(), "no row of all -1 in the per-structure list"
    for excluded, verdicts, f, b in ((m50.excluded_shared, m50.shared_verdicts, m50.shared_formed, m50.shared_broken),
                                     (m50.excluded_per, m50.per_verdicts, m50.per_formed, m50.per_broken)):
        for m, mnb in enumerate(MAX_NEWBONDS):
            _, formed, broken, mask, _ = restate(g.structures, classes, thr, None, g.expected_edges, excluded, mnb)
            assert (mask == verdicts[m]).all() and (formed == f).all() and (broken == b).all()


def test_restatement_reproduces_the_double_bonds():
    from tscode_amd.graph_manipulations import double_bond_tables
    g = g21("double")
    classes, thr, heavy = double_bond_tables(g.atomnos)
    adj, _, _, _, margin = restate(g.structures, classes, thr, heavy)
    assert margin > GUARD
    want = split_edges(g.edges, g.edge_off)
    assert len({e.tobytes() for e in want}) >= 10
    for s in range(len(adj)):
        assert np.array_equal(dense_edges(adj[s]), want[s]), s


def test_packing_round_trip():
    from tscode_amd.graph_manipulations import edges_from_bits, pack_edges
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 130, 512):
        dense = np.triu(rng.random((n, n)) < 0.1, 1)
        e = dense_edges(dense)
        bits = pack_edges(e[:, ::-1], n)                    # (either order of a bond)
        assert bits.shape == (n, (n + 63) // 64) and np.array_equal(bits, packed(dense[None])[0])
        assert np.array_equal(edges_from_bits(bits), e.astype(np.int32)) and np.array_equal(unpacked_edges(bits), e)


# ------------------------------------------------------------------------------------------------------- CPU: ABI, install, refusals
def test_header_and_prototype_table_declare_the_entry_points():
    from tscode_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tscode_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"{s} not declared in include/tscode_hip.h"
        assert s in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["tsc_bond_delta"] == _lib._SIGNATURES["tsc_bond_delta_dev"]
    assert "topology.hip" in build.SOURCES and "topology.hpp" in build.HEADERS


def test_topology_patch_table_equals_the_recorded_sites():
    inst = importlib.import_module("tscode_amd.install")
    g = json.load(open(os.path.join(GOLDEN, "G21_topology_sites.json")))
    assert not g["modules_not_importable_here"] and len(g["modules_imported"]) >= 25
    assert {k: sorted(v[1]) for k, v in inst._TOPOLOGY_PATCHES.items()} == {k: v["bound_in"] for k, v in g["sites"].items()}
    assert all(v["defined_in"] in v["bound_in"] for v in g["sites"].values())
    assert not set(inst._TOPOLOGY_PATCHES) & (set(inst._PATCHES) | set(inst._ROT_CORR_PATCHES) | set(inst._DIVERSE_PATCHES))


def test_install_topology_is_opt_in_and_uninstall_restores():
    import tscode_amd
    inst = importlib.import_module("tscode_amd.install")
    sites = sorted({name for _, names in inst._TOPOLOGY_PATCHES.values() for name in names})
    fake, originals = {}, {}
    for name in sites:
        mod = types.ModuleType(name)
        for attr, (_, names) in inst._TOPOLOGY_PATCHES.items():
            if name in names:
                originals[(name, attr)] = (lambda *a, _k=(name, attr), **kw: _k)
                setattr(mod, attr, originals[(name, attr)])
        fake[name] = mod
    try:
        done = tscode_amd.install(modules=fake, per_item=True, rot_corr=True, diverse=True)
        assert not [d for d in done if d[1] in inst._TOPOLOGY_PATCHES], "install() without topology=True must not patch the topology checks"
        assert all(getattr(fake[n], a) is fn for (n, a), fn in originals.items())
        done = tscode_amd.install(modules=fake, topology=True)
        assert sorted(d for d in done if d[1] in inst._TOPOLOGY_PATCHES) == sorted(originals)
        for (name, attr) in originals:
            assert getattr(fake[name], attr) is inst._TOPOLOGY_PATCHES[attr][0]
    finally:
        tscode_amd.uninstall(modules=fake)
    assert all(getattr(fake[n], a) is fn for (n, a), fn in originals.items())


def test_refusals_raise_value_error_before_the_library_is_loaded():
    import tscode_amd as ta
    from tscode_amd.graph_manipulations import check_bond_delta_args as chk
    z = np.array([6, 6, 8, 1])
    x = np.zeros((2, 4, 3)) + np.arange(4)[None, :, None]
    thr = np.full((2, 2), 1.5)
    cls = np.array([0, 0, 1, 1])
    chk(x, cls, thr, np.ones(4, bool), np.zeros((4, 1), np.uint64), np.array([[0, -1], [-1, -1]]))          # (a valid call)
    bad = x.copy()
    bad[1, 2, 0] = np.nan
    refusals = [
        lambda: ta.bond_graph_batch(bad, z),                                             # non-finite coordinates
        lambda: ta.bond_graph_batch(x[:, :3], z),                                        # shape mismatch
        lambda: ta.bond_graph_batch(np.zeros((2, 4, 2)), z),
        lambda: ta.bond_graph_batch(np.zeros((1, 513, 3)), np.full(513, 6)),             # n_atoms > 512
        lambda: ta.bond_graph_batch(np.zeros((1, 0, 3)), np.zeros(0, int)),              # n_atoms < 1
        lambda: ta.bond_graph_batch(x, z, mask=np.ones(3, bool)),
        lambda: ta.bond_tables(np.arange(1, 18), {k: 1.0 for k in range(1, 18)}),        # 17 classes
        lambda: ta.bond_graph_batch(x, np.array([6, 6, 8, 92])),                         # an element nobody knows
        lambda: chk(x, cls, np.full((17, 17), 1.0)),                                     # n_classes > 16
        lambda: chk(x, cls, np.zeros((0, 0))),                                           # n_classes < 1
        lambda: chk(x, np.array([0, 0, 1, 2]), thr),                                     # class >= n_classes
        lambda: chk(x, cls, np.array([[1.0, -1.0], [-1.0, 1.0]])),                       # negative threshold
        lambda: chk(x, cls, np.array([[1.0, np.inf], [np.inf, 1.0]])),                   # non-finite threshold
        lambda: chk(x, cls, thr, excluded=np.array([4])),                                # excluded index >= n_atoms
        lambda: chk(x, cls, thr, excluded=np.array([-2])),                               # excluded index < -1
        lambda: chk(x, cls, thr, excluded=np.zeros(17, int)),                            # n_excl > 16
        lambda: chk(x, cls, thr, excluded=np.zeros((3, 2), int)),                        # rows != structures
        lambda: chk(x, cls, thr, ref_bits=np.zeros((4, 2), np.uint64)),                  # ref_bits shape
        lambda: chk(x, cls, thr, ref_bits=np.full((4, 1), 1, np.uint64)),                # a bit on / below the diagonal
        lambda: ta.scramble_mask(x, z, [], np.array([[0, 7]])),                          # a bond index out of range
        lambda: ta.scramble_mask(x, z, [], [types.SimpleNamespace(nodes=range(3), edges=[])]),   # graphs of another size
        lambda: ta.molecule_check_mask(x, x, z),                                         # old_coords is one structure
    ]
    for k, call in enumerate(refusals):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} did not raise")


def test_covalent_radii_resolution_order():
    from tscode_amd.graph_manipulations import _BUILTIN_RADII, covalent_radii, d_min_bond
    assert "tscode" not in sys.modules and "tscode.pt" not in sys.modules
    z = np.array([1, 6, 7, 8, 9, 16, 17])
    assert sorted(_BUILTIN_RADII) == z.tolist()
    builtin = covalent_radii(z)
    assert builtin.tolist() == [0.31, 0.76, 0.71, 0.66, 0.57, 1.05, 1.02]
    assert d_min_bond(6, 8) == 1.2 * (0.76 + 0.66)
    assert covalent_radii(z, {6: 0.5})[1] == 0.5 and covalent_radii(z, {6: 0.5})[0] == 0.31        # the explicit mapping first
    with pytest.raises(ValueError, match="35"):
        covalent_radii([6, 35])
    live = types.ModuleType("tscode.pt")
    live.pt = {k: types.SimpleNamespace(covalent_radius=v + 0.01) for k, v in _BUILTIN_RADII.items() if k != 9}
    sys.modules["tscode.pt"] = live
    try:
        got = covalent_radii(z)
        assert got[1] == 0.76 + 0.01 and got[4] == 0.57, "a live tscode.pt comes before the built-in table, element by element"
        assert covalent_radii(z, {6: 0.5})[1] == 0.5
    finally:
        del sys.modules["tscode.pt"]
    assert "tscode" not in sys.modules, "covalent_radii imported tscode"
    assert covalent_radii(z).tolist() == builtin.tolist()


# ------------------------------------------------------------------------------------------------------- GPU
def engine():
    import tscode_amd
    return tscode_amd.get_engine()


def run_dev(eng, coords, classes, thr, active, ref_bits, excluded, mnb, outputs):
    """tsc_bond_delta_dev on torch buffers; returns the same dict Engine.bond_delta does."""
    import torch
    N, n = coords.shape[:2]
    w = (n + 63) // 64
    dev = torch.device("cuda", eng.device)
    d_coords = torch.from_numpy(np.ascontiguousarray(coords)).to(dev)
    mask = torch.full((N,), 7, dtype=torch.uint8, device=dev)
    formed = torch.full((N,), -7, dtype=torch.int32, device=dev) if outputs else None
    broken = torch.full((N,), -7, dtype=torch.int32, device=dev) if outputs else None
    adj = torch.full((N, n, w), -1, dtype=torch.int64, device=dev) if outputs else None
    per = excluded is not None and np.asarray(excluded).ndim == 2
    d_excl = torch.from_numpy(np.ascontiguousarray(excluded, dtype=np.int32)).to(dev) if per else excluded
    torch.cuda.synchronize()
    eng.bond_delta_dev(d_coords, N, n, classes, thr, active, ref_bits, d_excl, per, mnb, mask, formed, broken, adj)
    eng.synchronize()
    out = {"mask": mask.cpu().numpy().astype(bool)}
    if outputs:
        out.update(formed=formed.cpu().numpy(), broken=broken.cpu().numpy(), adj=adj.cpu().numpy().view(np.uint64))
    return out


def assert_equal_to_restatement(got, want, outputs, what):
    adj, formed, broken, mask, _ = want
    assert np.array_equal(got["mask"], mask), what
    if outputs:
        assert np.array_equal(got["formed"], formed) and np.array_equal(got["broken"], broken), what
        assert np.array_equal(got["adj"], packed(adj)), what


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("case", ["chain50", "chain200", "masked50", "bimol", "double"])
def test_g21_parity(case, path):
    """adj, formed, broken and mask equal what the reference recorded, through tsc_bond_delta and tsc_bond_delta_dev."""
    from tscode_amd.graph_manipulations import double_bond_tables, pack_edges
    eng = engine()

    def call(coords, classes, thr, active, ref, excluded, mnb):
        if path == "host":
            return eng.bond_delta(coords, classes, thr, active, ref, excluded, mnb, want_counts=True, want_adj=True)
        return run_dev(eng, coords, classes, thr, None if active is None else np.asarray(active, np.uint8), ref, excluded, mnb, True)

    def edges_of(got):
        return [unpacked_edges(rows) for rows in got["adj"]]

    if case == "double":
        g = g21(case)
        classes, thr, heavy = double_bond_tables(g.atomnos)
        got = call(g.structures, classes, thr, heavy, None, None, 0)
        for s, (a, b) in enumerate(zip(edges_of(got), split_edges(g.edges, g.edge_off))):
            assert np.array_equal(a, b), s
        return
    g = g21("chain50" if case == "masked50" else case)
    classes, thr = tables(g)
    n = len(classes)
    ref = pack_edges(g.expected_edges, n)
    if case == "masked50":
        m50 = g21("masked50")
        got = call(g.structures, classes, thr, m50.mask, None, None, 0)
        for s, (a, b) in enumerate(zip(edges_of(got), split_edges(m50.mask_edges, m50.mask_edge_off))):
            assert np.array_equal(a, b), s
        runs = [(m50.excluded_shared, m50.shared_verdicts, m50.shared_formed, m50.shared_broken),
                (m50.excluded_per, m50.per_verdicts, m50.per_formed, m50.per_broken)]
    else:
        runs = [(g.excluded if case == "bimol" else None, g.scramble_verdicts, g.formed, g.broken)]
    want_edges = split_edges(g.edges, g.edge_off)
    for excluded, verdicts, formed, broken in runs:
        for m, mnb in enumerate(MAX_NEWBONDS):
            got = call(g.structures, classes, thr, None, ref, excluded, mnb)
            assert np.array_equal(got["mask"], verdicts[m]), (case, mnb)
            assert np.array_equal(got["formed"], formed) and np.array_equal(got["broken"], broken), (case, mnb)
        for s, (a, b) in enumerate(zip(edges_of(got), want_edges)):
            assert np.array_equal(a, b), s


SWEEP = [(n, N) for n in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 512) for N in (2, 65)] + \
        [(50, N) for N in (1, 2, 63, 64, 65, 1000)]


def sweep_inputs(k, n, N):
    """Inputs drawn as the fixtures' chains are; the options walk through their combinations with the case number."""
    from tscode_amd.graph_manipulations import bond_tables
    from tscode_amd.synthetic import make_chain_ensemble
    _, structures, atomnos, _ = make_chain_ensemble(N, n, 7000 + k)
    classes, thr = bond_tables(atomnos)
    rng = np.random.default_rng(9000 + k)
    active = (rng.random(n) < 0.85) if k % 4 else None
    mode = k % 3
    excluded = None
    if mode == 1:
        excluded = rng.integers(0, n, size=min(3, n)).astype(np.int32)
    elif mode == 2:
        excluded = rng.integers(-1, n, size=(N, 4)).astype(np.int32)
        excluded[0] = -1
    expected = np.array([(i, i + 1) for i in range(n - 1)], dtype=np.int64).reshape(-1, 2) if (k // 2) % 2 else None
    return structures, classes, thr, active, expected, excluded, MAX_NEWBONDS[(k // 3) % 3], bool((k // 4) % 2)


def test_sweep_seeds_pass_the_guard_on_their_first_draw():
    for k, (n, N) in enumerate(SWEEP):
        structures, classes, thr, active, expected, excluded, mnb, outputs = sweep_inputs(k, n, N)
        assert n == 1 or restate(structures, classes, thr, active, expected, excluded, mnb)[4] > GUARD, (k, n, N)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SWEEP)))
def test_shape_sweep_equals_the_restatement(k):
    from tscode_amd.graph_manipulations import pack_edges
    n, N = SWEEP[k]
    structures, classes, thr, active, expected, excluded, mnb, outputs = sweep_inputs(k, n, N)
    want = restate(structures, classes, thr, active, expected, excluded, mnb)
    assert n == 1 or want[4] > GUARD
    ref = None if expected is None else pack_edges(expected, n)
    eng = engine()
    got = eng.bond_delta(structures, classes, thr, active, ref, excluded, mnb, want_counts=outputs, want_adj=outputs)
    assert_equal_to_restatement(got, want, outputs, ("host", k, n, N))
    got = run_dev(eng, structures, classes, thr, None if active is None else active.astype(np.uint8), ref, excluded, mnb, outputs)
    assert_equal_to_restatement(got, want, outputs, ("dev", k, n, N))


@pytest.mark.gpu
@pytest.mark.parametrize("N,n", [(20011, 50), (3001, 200)])
def test_large_grids_equal_the_restatement(N, n):
    """More structures than the grid has wavefronts in flight; the last workgroup and its last wavefront are partial."""
    from tscode_amd.graph_manipulations import bond_tables, pack_edges
    from tscode_amd.synthetic import make_chain_ensemble
    _, structures, atomnos, _ = make_chain_ensemble(N, n, 7700 + n)
    classes, thr = bond_tables(atomnos)
    expected = np.array([(i, i + 1) for i in range(n - 1)])
    excluded = np.array([3, n - 2], dtype=np.int32)
    want = restate(structures, classes, thr, None, expected, excluded, 1)
    assert want[4] > GUARD
    assert 0 < want[3].sum() < N
    got = engine().bond_delta(structures, classes, thr, None, pack_edges(expected, n), excluded, 1, want_counts=True, want_adj=True)
    assert_equal_to_restatement(got, want, True, (N, n))


@pytest.mark.gpu
def test_zero_structures_succeed_and_write_nothing():
    import torch
    eng = engine()
    dev = torch.device("cuda", eng.device)
    mask = torch.full((4,), 7, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -7, dtype=torch.int32, device=dev)
    adj = torch.full((4, 3, 1), -1, dtype=torch.int64, device=dev)
    coords = torch.zeros((4, 3, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.bond_delta_dev(coords, 0, 3, np.zeros(3, np.uint8), np.ones((1, 1)), None, None, None, False, 0, mask, counts, counts, adj)
    eng.synchronize()
    assert (mask.cpu() == 7).all() and (counts.cpu() == -7).all() and (adj.cpu() == -1).all()
    out = eng.bond_delta(np.zeros((0, 3, 3)), np.zeros(3, np.uint8), np.ones((1, 1)), want_counts=True, want_adj=True)
    assert out["mask"].shape == (0,) and out["adj"].shape == (0, 3, 1)


@pytest.mark.gpu
def test_drop_ins_against_the_reference():
    import tscode_amd as ta
    g = g21("chain50")
    for s in range(12):
        for m, mnb in enumerate(MAX_NEWBONDS):
            assert ta.molecule_check(g.base, g.structures[s], g.atomnos, max_newbonds=mnb) == bool(g.molecule_verdicts[m][s])
    b = g21("bimol")
    n1, n2 = (int(v) for v in b.mol_sizes)
    graphs = [types.SimpleNamespace(nodes=range(n1), edges=[tuple(e) for e in b.mol1_edges.tolist()] + [(0, 0)]),
              types.SimpleNamespace(nodes=range(n2), edges=[tuple(e) for e in b.mol2_edges.tolist()])]
    failures = 0
    for s in range(40):
        for m, mnb in enumerate(MAX_NEWBONDS):
            log = []
            ok = ta.scramble_check(b.structures[s], b.atomnos, list(b.excluded), graphs, max_newbonds=mnb, logfunction=log.append, title="pose")
            assert ok == bool(b.scramble_verdicts[m][s])
            assert len(log) == (0 if ok else 1)
            if not ok:
                failures += 1
                found = re.fullmatch(r"pose, scramble_check - found (\d+) extra bonds: \{(.*)\}", log[0])
                assert found and int(found.group(1)) == int(b.formed[s]) + int(b.broken[s])
                assert len(re.findall(r"\(\d+, \d+\)", found.group(2))) == int(found.group(1))
    assert failures > 0
    with pytest.raises(AssertionError):
        ta.scramble_check(b.structures[0][:-1], b.atomnos[:-1], [], graphs)
    d = g21("double")
    for s, want in enumerate(split_edges(d.edges, d.edge_off)[:10]):
        got = ta.get_double_bonds_indices(d.structures[s], d.atomnos)
        assert got == [tuple(e) for e in want.tolist()] and all(type(v) is int for e in got for v in e)


@pytest.mark.gpu
def test_graphize_drop_in():
    pytest.importorskip("networkx")
    import tscode_amd as ta
    g, m50 = g21("chain50"), g21("masked50")
    for s, want in enumerate(split_edges(m50.mask_edges, m50.mask_edge_off)[:3]):
        graph = ta.graphize(g.structures[s], g.atomnos, m50.mask)
        assert sorted(graph.nodes) == list(range(50))
        loops = sorted(a for a, b in graph.edges if a == b)
        assert loops == np.nonzero(m50.mask)[0].tolist()
        assert sorted(tuple(sorted(e)) for e in graph.edges if e[0] != e[1]) == [tuple(e) for e in want.tolist()]
        assert [graph.nodes[i]["atomnos"] for i in range(50)] == g.atomnos.tolist()
    full = ta.graphize(g.base, g.atomnos)
    assert sorted(a for a, b in full.edges if a == b) == list(range(50))


def read_from_a_fresh_thread(read):
    import threading
    got = []
    t = threading.Thread(target=lambda: got.append(read()))
    t.start()
    t.join()
    return got[0]


@pytest.mark.gpu
def test_kernel_time_is_taken_only_under_pass_timing_and_per_thread():
    """tsc_topology_timings on 3 structures of 5 atoms: -1 without the option, a positive time with it through both entries, -1
    after zero structures, -1 again once the option is off, -1 in a thread that never called."""
    import math
    from tscode_amd.graph_manipulations import bond_tables
    from tscode_amd.synthetic import make_chain_ensemble
    _, structures, atomnos, _ = make_chain_ensemble(3, 5, 7100)
    classes, thr = bond_tables(atomnos)
    eng = engine()
    with eng.options(pass_timing=0):
        eng.bond_delta(structures, classes, thr)
        assert eng.topology_kernel_ms() == -1.0
        run_dev(eng, structures, classes, thr, None, None, None, 0, False)
        assert eng.topology_kernel_ms() == -1.0
        with eng.options(pass_timing=1):
            eng.bond_delta(structures, classes, thr)
            host_ms = eng.topology_kernel_ms()
            assert math.isfinite(host_ms) and host_ms > 0.0
            assert read_from_a_fresh_thread(eng.topology_kernel_ms) == -1.0
            run_dev(eng, structures, classes, thr, None, None, None, 0, False)
            dev_ms = eng.topology_kernel_ms()
            assert math.isfinite(dev_ms) and dev_ms > 0.0
            eng.bond_delta(structures[:0], classes, thr)
            assert eng.topology_kernel_ms() == -1.0
            eng.bond_delta(structures, classes, thr)
            assert eng.topology_kernel_ms() > 0.0
        eng.bond_delta(structures, classes, thr)
        assert eng.topology_kernel_ms() == -1.0
