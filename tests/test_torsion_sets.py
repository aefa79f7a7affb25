"""Hydrogen bonds, the search graph and the torsion sets of a conformational search (csrc/torsions.hpp, tscode_amd.torsion_module):
fixture G25 (tests/golden/gen_torsion_sets.py: the reference's csearch set-up and its csearch_augmentation loop) and sweeps of the
two kernels against yardsticks written here from the definitions at tsc_hbonds / tsc_torsion_reach in include/tscode_hip.h."""

import json
from collections import deque

import numpy as np
import pytest

from conftest import load_golden

VAL_TOL = 1e-9                 # Angstrom (test_csearch_multi.py)
D_MIN, D_MAX, MAX_ANGLE = 2.5, 3.3, 45.0
DIST_BAND, ANGLE_BAND = 1e-9, 1e-6
N_LIST = (1, 2, 3, 63, 64, 65, 129, 512)
TSC_ERR_INVALID = -1


# ------------------------------------------------------------------------------------------------------- fixture
_g25 = {}


def g25():
    if not _g25:
        g = load_golden("G25_torsion_sets")
        _g25["g"] = g
        _g25["meta"] = json.loads(g["meta_json"].tobytes().decode())
    return _g25["g"], _g25["meta"]


def g25_structures():
    g, meta = g25()
    out = []
    for rec in meta["structures"]:
        k = rec["index"]
        out.append((rec, g[f"s{k}_atomnos"].astype(np.int64), g[f"s{k}_coords"], g[f"s{k}_masks"]))
    return out


# ------------------------------------------------------------------------------------------------------- yardsticks
def neighbour_lists(n, bonds, extra=(), more=()):
    """Neighbour lists of the search graph: bonded atoms ascending, then the partners from `extra` and `more` in their order; an
    edge that already exists keeps its first position."""
    nb = [[] for _ in range(n)]
    for a, b in sorted((min(a, b), max(a, b)) for a, b in bonds):
        nb[a].append(b), nb[b].append(a)
    nb = [sorted(x) for x in nb]
    for a, b in list(extra) + list(more):
        a, b = int(a), int(b)
        if a < 0 or b < 0 or a == b:
            continue
        if b not in nb[a]:
            nb[a].append(b), nb[b].append(a)
    return nb


def reachable(nb, src, cut=None):
    """bool[n]: the atoms reachable from src, the edge `cut` taken out (the closure of one atom under the neighbour relation)."""
    seen = np.zeros(len(nb), dtype=bool)
    seen[src] = True
    todo = deque([src])
    while todo:
        a = todo.popleft()
        for b in nb[a]:
            if cut is not None and ((a, b) == cut or (b, a) == cut):
                continue
            if not seen[b]:
                seen[b] = True
                todo.append(b)
    return seen


def n_components(nb):
    seen = np.zeros(len(nb), dtype=bool)
    label = np.zeros(len(nb), dtype=np.int64)
    count = 0
    for a in range(len(nb)):
        if not seen[a]:
            r = reachable(nb, a)
            label[r] = count
            seen |= r
            count += 1
    return count, label


def yard_reach(n, nb, torsions, constrained):
    """flags u8[T], masks u8[T, n] from the definitions of tsc_torsion_reach."""
    flags, masks = np.zeros(len(torsions), np.uint8), np.zeros((len(torsions), n), np.uint8)
    for t, (i1, i2, i3, i4) in enumerate(np.asarray(torsions).reshape(-1, 4).tolist()):
        cut = (i2, i3)
        in_cycle = bool(reachable(nb, i1, cut)[i4])
        from_i2 = reachable(nb, i2, cut)
        n_reached = sum(1 for d in constrained if d >= 0 and from_i2[d])
        rev = n_reached % 2 == 1
        a, b = (i4, i3) if rev else (i1, i2)
        m = reachable(nb, a, cut)
        if np.count_nonzero(m) > n // 2:
            m = ~m
        m[b] = False
        flags[t] = (1 if in_cycle else 0) | (2 if rev else 0)
        if not in_cycle:
            masks[t] = m
    return flags, masks


def _norm_of(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def yard_hbonds(x, z_het, z_hyd, bonds, extra, mode, d_min=D_MIN, d_max=D_MAX, max_angle=MAX_ANGLE):
    """(pairs, status, n_components_before, graph edges, guarded) from the definitions of tsc_hbonds; `guarded`: a tested quantity
    lies inside the guard band, so the structure decides nothing."""
    n = len(x)
    nb = neighbour_lists(n, bonds, extra)
    n0, label = n_components(nb)
    het = [i for i in range(n) if z_het[i]]
    pairs, guarded = [], False
    search = mode == 0 or n0 > 1
    with np.errstate(all="ignore"):
        for k, i1 in enumerate(het):
            rest = np.array(het[k + 1:], dtype=np.int64)
            if not len(rest):
                continue
            diff = x[i1] - x[rest]
            dist = np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
            if (np.minimum(np.abs(dist - d_min), np.abs(dist - d_max)) < DIST_BAND).any():
                guarded = True
            if not search:
                continue
            for i2 in rest[(dist > d_min) & (dist < d_max)].tolist():
                if mode == 1 and label[i1] == label[i2]:
                    continue
                u = (x[i2] - x[i1]) / _norm_of(x[i2] - x[i1])
                for h in [j for j in nb[i1] + nb[i2] if z_hyd[j]]:
                    v1, v2 = x[h] - x[i1], x[h] - x[i2]
                    d1, d2 = _norm_of(v1), _norm_of(v2)
                    l1, l2 = v1 @ u, v2 @ -u
                    va, vb = (v1, u) if l1 < l2 else (v2, -u)
                    alfa = np.degrees(np.arccos(np.clip((va / _norm_of(va)) @ (vb / _norm_of(vb)), -1.0, 1.0)))
                    if abs(l1 - l2) < DIST_BAND or abs(d1 - d2) < DIST_BAND or abs(alfa - max_angle) < ANGLE_BAND:
                        guarded = True
                    if alfa < max_angle:
                        pairs.append(sorted((h, i2)) if d1 < d2 else sorted((h, i1)))
                        break
    after = neighbour_lists(n, bonds, extra, pairs)
    n1 = n_components(after)[0] if pairs else n0
    edges = sorted({(min(a, b), max(a, b)) for a in range(n) for b in after[a]})
    return pairs, int(n1 > 1), n0, edges, guarded


# ------------------------------------------------------------------------------------------------------- CPU: host restatement
def test_host_restatement_against_g25():
    """Class graph, hydrogen bonds and double bonds from the fixture; in_cycle, orientation and masks from the numpy yardstick; the
    rotatability rules and folds from tscode_amd.torsion_module: torsions, folds and masks equal the reference's exactly."""
    from tscode_amd import torsion_module as tm
    checked = 0
    for rec, z, x, ref_masks in g25_structures():
        if rec["segmented"]:
            continue
        n = len(z)
        graph = tm.class_graph(z, rec["bonds"], rec["pairs"], rec["hydrogen_bonds"])
        cands = tm.candidate_quadruplets(graph, rec["double_bonds"])
        nb = neighbour_lists(n, rec["bonds"], rec["pairs"], rec["hydrogen_bonds"])
        flags, masks = yard_reach(n, nb, cands, [i for p in rec["pairs"] for i in p])
        tors, m, folds = tm.class_torsion_set(graph, cands, flags, masks, rec["hydrogen_bonds"])
        assert tors.tolist() == rec["torsions"], rec["name"]
        assert folds.tolist() == rec["n_folds"], rec["name"]
        assert np.array_equal(m.astype(bool), ref_masks), rec["name"]
        checked += len(tors)
    assert checked >= 60


def test_argument_checks_raise_before_the_library_is_loaded(monkeypatch):
    from tscode_amd import torsion_module as tm

    def no_engine():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(tm, "get_engine", no_engine)
    z = np.array([8, 1, 1, 6])
    x = np.zeros((2, 4, 3))
    for fn in (tm.hydrogen_bonds_batch, tm.torsion_sets_batch):
        with pytest.raises(ValueError):
            fn(np.zeros((2, 5, 3)), z)                                    # atoms differ
        with pytest.raises(ValueError):
            fn(x, z, constrained_indices=[(0, 4)])                       # index out of range
        with pytest.raises(ValueError):
            fn(x, z, constrained_indices=[(0, -2)])
        with pytest.raises(ValueError):
            fn(x, z, constrained_indices=[[(0, 1)]])                     # one list for two structures
        with pytest.raises(ValueError):
            fn(x, z, constrained_indices=np.array([[0.5, 1.0]]))
        with pytest.raises(ValueError):
            fn(x, z, constrained_indices=[(0, 1)] * 65)
        with pytest.raises(ValueError):
            fn(x, z.astype(float))
        with pytest.raises(ValueError):
            fn(np.full((2, 4, 3), np.nan), z)
    with pytest.raises(ValueError):
        tm.hydrogen_bonds_batch(x, z, d_min=3.3, d_max=3.3)
    with pytest.raises(ValueError):
        tm.hydrogen_bonds_batch(x, z, max_angle=np.inf)
    with pytest.raises(ValueError):
        tm.csearch_augmentation_batch(np.zeros((2, 5, 3)), z, None)


# ------------------------------------------------------------------------------------------------------- GPU: G25
def _batches():
    """The fixture's structures grouped into calls: same atoms and the same mode."""
    groups = {}
    for item in g25_structures():
        rec, z = item[0], item[1]
        groups.setdefault((z.tobytes(), rec["keep_hb"]), []).append(item)
    return list(groups.values())


@pytest.mark.gpu
def test_g25_through_the_public_functions():
    import tscode_amd
    for batch in _batches():
        z, keep_hb = batch[0][1], batch[0][0]["keep_hb"]
        x = np.array([b[2] for b in batch])
        pairs = [b[0]["pairs"] for b in batch]
        hb, seg = tscode_amd.hydrogen_bonds_batch(x, z, pairs, keep_hb=keep_hb)
        ts = tscode_amd.torsion_sets_batch(x, z, pairs, keep_hb=keep_hb)
        by_class = {}
        for s, (rec, _, _, ref_masks) in enumerate(batch):
            name = rec["name"]
            assert bool(seg[s]) == rec["segmented"] == bool(ts.segmented[s]), name
            if rec["segmented"]:
                assert ts.set_of_structure[s] == -1
                if keep_hb:
                    assert hb[s].tolist() == rec["hydrogen_bonds"], name
                continue
            assert hb[s].tolist() == rec["hydrogen_bonds"] == ts.hydrogen_bonds[s].tolist(), name
            tors, masks, folds = ts.sets[ts.set_of_structure[s]]
            assert tors.tolist() == rec["torsions"], name
            assert folds.tolist() == rec["n_folds"], name
            assert np.array_equal(masks.astype(bool), ref_masks), name
            key = json.dumps([rec["bonds"], rec["double_bonds"], rec["pairs"], rec["hydrogen_bonds"]])
            by_class.setdefault(key, set()).add(int(ts.set_of_structure[s]))
        assert all(len(v) == 1 for v in by_class.values())                 # structures of one recorded class share a set
        assert len({min(v) for v in by_class.values()}) == len(by_class)


@pytest.mark.gpu
def test_g25_augmentation_loop():
    import tscode_amd
    g, meta = g25()
    recs = {r["index"]: r for r in meta["structures"]}
    for case in meta["part_c"]:
        members = case["members"]
        outs = [g[f"{case['name']}_out{j}"] for j in range(len(members))]
        np.random.seed(case["seed"])
        if case["same_atoms"]:
            x = np.array([g[f"s{k}_coords"] for k in members])
            new, start = tscode_amd.csearch_augmentation_batch(x, g[f"s{members[0]}_atomnos"], [recs[k]["pairs"] for k in members], n_out=case["n_out"])
            got = [new[start == j] for j in range(len(members))]
        else:                                                               # (structures of different molecules: one call each, in order)
            got = [tscode_amd.csearch_augmentation_batch(g[f"s{k}_coords"][None], g[f"s{k}_atomnos"], [recs[k]["pairs"]], n_out=case["n_out"])[0]
                   for k in members]
        assert [len(o) for o in got] == case["counts"], case["name"]
        for o, ref in zip(got, outs):
            if len(ref):
                assert np.abs(o - ref).max() <= VAL_TOL, case["name"]


# ------------------------------------------------------------------------------------------------------- GPU: tsc_hbonds sweep
def soup(seed, S, n, n_extra):
    """Random N / O / H / C soups with bonds and constraint pairs handed in: (x f64[S, n, 3], het u8[n], hyd u8[n], bond lists,
    extra i32[S, n_extra, 2]).  The box holds a few hetero pairs between 2.5 and 3.3 A; a hydrogen sits 1 A from its parent; half
    the structures have their heavy atoms bonded into one tree (connected: no search in the linking mode)."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, size=n, p=[0.3, 0.35, 0.15, 0.2])                 # 0 N/O, 1 H, 2 C, 3 N/O
    het, hyd = ((kind == 0) | (kind == 3)).astype(np.uint8), (kind == 1).astype(np.uint8)
    n_het = max(int(het.sum()), 1)
    side = max(3.0, (n_het * n_het * 85.0 / 40.0) ** (1.0 / 3.0))
    xs, bonds, extras = [], [], []
    heavy = np.flatnonzero(hyd == 0)
    for s in range(S):
        x = rng.uniform(0.0, side, size=(n, 3))
        b = set()
        for h in np.flatnonzero(hyd):
            if n > 1:
                p = int(rng.choice(heavy)) if len(heavy) and rng.random() < 0.9 else int((h + 1 + rng.integers(n - 1)) % n)
                d = rng.normal(size=3)
                x[h] = x[p] + d / np.linalg.norm(d)
                b.add((min(h, p), max(h, p)))
        if s % 2 == 0 and len(heavy) > 1:
            order = rng.permutation(heavy)
            for k in range(1, len(order)):
                p = int(order[rng.integers(k)])
                b.add((min(p, int(order[k])), max(p, int(order[k]))))
        else:
            for _ in range(n // 8):
                p, q = (int(v) for v in rng.integers(n, size=2))
                if p != q:
                    b.add((min(p, q), max(p, q)))
        ex = np.full((n_extra, 2), -1, dtype=np.int32)
        for q in range(n_extra):
            roll = rng.random()
            if roll < 0.2 or n < 2:
                continue                                                    # an unused slot
            if roll < 0.4 and b:
                ex[q] = sorted(b)[rng.integers(len(b))][::-1]               # an edge that exists already
            elif roll < 0.8 and hyd.any() and het.any():
                ex[q] = (rng.choice(np.flatnonzero(het)), rng.choice(np.flatnonzero(hyd)))   # a hydrogen through a constraint pair only
            else:
                ex[q] = rng.integers(n, size=2)                             # (may be twice the same atom: an unused slot)
        xs.append(x), bonds.append(sorted(b)), extras.append(ex)
    return np.array(xs).reshape(S, n, 3), het, hyd, bonds, np.array(extras, dtype=np.int32).reshape(S, n_extra, 2)


def bond_bits(bonds, n):
    from tscode_amd.graph_manipulations import pack_edges
    return np.array([pack_edges(np.array(b, dtype=np.int64).reshape(-1, 2), n) for b in bonds], dtype=np.uint64).reshape(len(bonds), n, (n + 63) // 64)


def hbonds_plan():
    """(n, S, n_extra, mode) of the sweep: every n with S = 5 in both modes and with both n_extra, S = 0 and 1 once per n, S = 257
    where a grid wraps (small structures) and at the largest structure."""
    plan = []
    for n in N_LIST:
        plan += [(n, 5, 0, 0), (n, 5, 3, 0), (n, 5, 0, 1), (n, 5, 3, 1), (n, 0, 3, 0), (n, 1, 3, 1)]
    plan += [(3, 257, 3, 0), (64, 257, 3, 1), (65, 257, 0, 0), (512, 257, 3, 0)]
    return plan


def check_hbonds_case(eng, n, S, n_extra, mode, stats):
    x, het, hyd, bonds, extra = soup(1000 * n + 10 * S + n_extra, S, n, n_extra)
    bits = bond_bits(bonds, n)
    yard = [yard_hbonds(x[s], het, hyd, bonds[s], extra[s], mode) for s in range(S)]
    max_hb = max([len(y[0]) for y in yard] + [1])
    out = eng.hbonds(x, het, hyd, bits, extra if n_extra else None, D_MIN, D_MAX, MAX_ANGLE, mode, max_hb, want_graph=True)
    for s, (pairs, status, n0, edges, guarded) in enumerate(yard):
        stats[0] += 1
        if guarded:
            stats[1] += 1
            continue
        tag = (n, S, n_extra, mode, s)
        assert out["n_hb"][s] == len(pairs), tag
        assert out["hb"][s, :len(pairs)].tolist() == pairs, tag
        assert (out["hb"][s, len(pairs):] == -1).all(), tag
        assert out["status"][s] == status and out["n_components_before"][s] == n0, tag
        assert np.array_equal(out["graph"][s], bond_bits([edges], n)[0]), tag
        stats[2] += len(pairs)
    return x, het, hyd, bits, extra, out, max_hb


@pytest.mark.gpu
def test_hbonds_sweep():
    from tscode_amd.engine import get_engine
    eng = get_engine()
    stats = [0, 0, 0]                                                       # structures, left out, pairs found
    for n, S, n_extra, mode in hbonds_plan():
        check_hbonds_case(eng, n, S, n_extra, mode, stats)
    print(f"hbonds sweep: {stats[0]} structures, {stats[1]} inside the guard band, {stats[2]} pairs")
    assert stats[1] <= 0.05 * stats[0]
    assert stats[2] >= 100                                                  # the soups do hold hydrogen bonds


@pytest.mark.gpu
@pytest.mark.parametrize("n,S,n_extra,mode", [(65, 5, 3, 0), (512, 5, 3, 1), (3, 257, 3, 0)])
def test_hbonds_dev_equals_host_and_respects_the_slots(n, S, n_extra, mode):
    from tscode_amd.engine import get_engine
    eng = get_engine()
    x, het, hyd, bits, extra, host, max_hb = check_hbonds_case(eng, n, S, n_extra, mode, [0, 0, 0])
    W = (n + 63) // 64
    held = [eng.dev_upload(a) for a in (x, bits, extra)]
    try:
        for slots in (max_hb, 1, 0):
            guard = 64                                                      # sentinel words behind the last slot
            hb = np.full(S * slots * 2 + guard, -7, dtype=np.int32)
            d_hb, d_n, d_st, d_b, d_g = eng.dev_upload(hb), eng.dev_alloc(S * 4), eng.dev_alloc(S), eng.dev_alloc(S * 4), eng.dev_alloc(S * n * W * 8)
            held += [d_hb, d_n, d_st, d_b, d_g]
            eng.hbonds_dev(held[0], S, n, het, hyd, held[1], held[2], n_extra, D_MIN, D_MAX, MAX_ANGLE, mode, slots, d_hb, d_n, d_st, d_b, d_g)
            eng.dev_download(d_hb, hb)
            n_hb = eng.dev_download(d_n, np.empty(S, np.int32))
            assert np.array_equal(n_hb, host["n_hb"])                       # the true count, whatever the slots
            assert np.array_equal(eng.dev_download(d_st, np.empty(S, np.uint8)), host["status"])
            assert np.array_equal(eng.dev_download(d_b, np.empty(S, np.int32)), host["n_components_before"])
            assert np.array_equal(eng.dev_download(d_g, np.empty((S, n, W), np.uint64)), host["graph"])
            assert (hb[S * slots * 2:] == -7).all()                         # nothing behind the slots
            got = hb[:S * slots * 2].reshape(S, slots, 2)
            for s in range(S):
                k = min(int(n_hb[s]), slots)
                assert np.array_equal(got[s, :k], host["hb"][s, :k]) and (got[s, k:] == -7).all()
        if max_hb > 1:
            small = eng.hbonds(x, het, hyd, bits, extra, D_MIN, D_MAX, MAX_ANGLE, mode, 1)
            assert np.array_equal(small["n_hb"], host["n_hb"]) and small["n_hb"].max() > 1
    finally:
        for a in held:
            eng.dev_free(a)


# ------------------------------------------------------------------------------------------------------- GPU: tsc_torsion_reach sweep
def random_graph(rng, n, n_closing):
    """A random tree on n atoms plus a few cycle-closing edges."""
    edges = set()
    order = rng.permutation(n)
    for k in range(1, n):
        p = int(order[rng.integers(k)])
        edges.add((min(p, int(order[k])), max(p, int(order[k]))))
    for _ in range(n_closing):
        if n > 2:
            p, q = (int(v) for v in rng.choice(n, size=2, replace=False))
            edges.add((min(p, q), max(p, q)))
    return sorted(edges)


def random_candidates(rng, n, nb, count):
    """Half along the graph (i1 - i2 - i3 - i4 a walk), half any indices with i2 != i3."""
    out = []
    edges = [(a, b) for a in range(n) for b in nb[a]]
    while len(out) < count and n >= 2:
        if edges and rng.random() < 0.5:
            i2, i3 = edges[rng.integers(len(edges))]
            out.append((int(rng.choice(nb[i2])), i2, i3, int(rng.choice(nb[i3]))))
        else:
            t = [int(v) for v in rng.integers(n, size=4)]
            if t[1] != t[2]:
                out.append(tuple(t))
    return out


def reach_case(n, n_con, seed):
    rng = np.random.default_rng(seed)
    graphs, tors, cons = [], [], []
    for count in (0, 1, 7, 70):
        edges = random_graph(rng, n, int(rng.integers(0, 4)))
        nb = neighbour_lists(n, edges)
        graphs.append((edges, nb))
        tors.append(random_candidates(rng, n, nb, count))
        con = rng.integers(-1, n, size=n_con)
        if n_con >= 2 and rng.random() < 0.7:
            con[1] = con[0]                                                 # a duplicate: two flips
        cons.append(con.astype(np.int32))
    return graphs, tors, np.array(cons, dtype=np.int32).reshape(4, n_con)


def run_reach(eng, n, graphs, tors, cons):
    set_off = np.concatenate([[0], np.cumsum([len(t) for t in tors])]).astype(np.int32)
    flat = np.array([q for t in tors for q in t], dtype=np.int32).reshape(-1, 4)
    bits = bond_bits([g[0] for g in graphs], n)
    flags, masks = eng.torsion_reach(bits, flat, set_off, cons if cons.shape[1] else None)
    want = [yard_reach(n, g[1], t, c.tolist()) for g, t, c in zip(graphs, tors, cons)]
    wf = np.concatenate([w[0] for w in want]) if len(flat) else np.zeros(0, np.uint8)
    wm = np.concatenate([w[1] for w in want]) if len(flat) else np.zeros((0, n), np.uint8)
    assert np.array_equal(flags, wf), (n, np.flatnonzero(flags != wf)[:5])
    assert np.array_equal(masks, wm), n
    return bits, flat, set_off, flags, masks


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_LIST)
def test_torsion_reach_sweep(n):
    from tscode_amd.engine import get_engine
    eng = get_engine()
    seen_flags = set()
    for n_con in (0, 1, 2, 3):
        graphs, tors, cons = reach_case(n, n_con, 77 * n + n_con)
        bits, flat, set_off, flags, masks = run_reach(eng, n, graphs, tors, cons)
        seen_flags |= set(flags.tolist())
        if n_con == 3 and len(flat):                                        # the _dev form on the same arrays
            held = [eng.dev_upload(a) for a in (bits, flat, cons)] + [eng.dev_alloc(len(flat)), eng.dev_alloc(len(flat) * n)]
            try:
                eng.torsion_reach_dev(held[0], len(graphs), n, held[1], set_off, held[2], 3, held[3], held[4])
                assert np.array_equal(eng.dev_download(held[3], np.empty(len(flat), np.uint8)), flags)
                assert np.array_equal(eng.dev_download(held[4], np.empty((len(flat), n), np.uint8)), masks)
            finally:
                for a in held:
                    eng.dev_free(a)
    if n >= 63:
        assert seen_flags == {0, 1, 2, 3}                                   # cyclic and not, reversed and not


@pytest.mark.gpu
@pytest.mark.parametrize("n", (64, 65, 512))
def test_torsion_reach_inversion_boundary(n):
    """A path graph cut so that exactly n // 2 and n // 2 + 1 atoms are reachable from i1 (kept as it is; inverted), from both
    ends and through a reversal; at n = 512 also a cut whose moved side holds 200 atoms."""
    from tscode_amd.engine import get_engine
    edges = [(k, k + 1) for k in range(n - 1)]
    nb = neighbour_lists(n, edges)
    tors, want_count = [], []
    for reach_n in (n // 2, n // 2 + 1) + ((200,) if n == 512 else ()):
        k = reach_n - 1                                                    # atoms 0 .. k on i1's side
        tors.append((k - 1, k, k + 1, k + 2))
        want_count.append(reach_n - 1 if reach_n <= n // 2 else n - reach_n)
        tors.append((k + 2, k + 1, k, k - 1))                              # from the other end: n - reach_n atoms reachable
        want_count.append(n - reach_n - 1 if n - reach_n <= n // 2 else reach_n)
    for cons in (np.zeros((1, 0), np.int32), np.array([[0]], np.int32)):    # atom 0 constrained: the tuples that start there turn round
        bits, flat, set_off, flags, masks = run_reach(get_engine(), n, [(edges, nb)], [tors], cons)
        if cons.shape[1] == 0:
            assert masks.sum(axis=1).tolist() == want_count
            assert max(want_count) > 64 or n < 512
        else:
            assert ((flags & 2) != 0).tolist() == [True, False] * (len(tors) // 2)


# ------------------------------------------------------------------------------------------------------- GPU: refusals
@pytest.mark.gpu
def test_refusals():
    import ctypes as C

    from tscode_amd._lib import TscodeHipError, ptr
    from tscode_amd.engine import get_engine
    eng = get_engine()
    lib, h = eng.lib, eng._h
    n, S = 4, 2
    x = np.zeros((S, n, 3))
    het, hyd = np.array([1, 0, 0, 1], np.uint8), np.array([0, 1, 1, 0], np.uint8)
    bits = np.zeros((S, n, 1), np.uint64)
    extra = np.full((S, 1, 2), -1, np.int32)
    outs = dict(hb=np.full((S, 2, 2), -7, np.int32), n_hb=np.full(S, -7, np.int32), status=np.full(S, 7, np.uint8))

    def hbonds(fn=lib.tsc_hbonds, **kw):
        a = dict(coords=x, n_structs=S, n_atoms=n, hetero=het, hydrogen=hyd, bonds=bits, extra=extra, n_extra=1, d_min=D_MIN, d_max=D_MAX,
                 max_angle=MAX_ANGLE, mode=0, max_hb=2, **outs)
        a.update(kw)
        return fn(h, ptr(a["coords"]), C.c_int64(a["n_structs"]), C.c_int(a["n_atoms"]), ptr(a["hetero"]), ptr(a["hydrogen"]), ptr(a["bonds"]),
                  ptr(a["extra"]), C.c_int(a["n_extra"]), C.c_double(a["d_min"]), C.c_double(a["d_max"]), C.c_double(a["max_angle"]),
                  C.c_int(a["mode"]), C.c_int(a["max_hb"]), ptr(a["hb"]), ptr(a["n_hb"]), ptr(a["status"]), None, None)

    bad_extra = extra.copy()
    bad_extra[1, 0] = (0, n)
    low_extra = extra.copy()
    low_extra[0, 0] = (-2, 1)
    refused = [dict(coords=None), dict(hetero=None), dict(hydrogen=None), dict(bonds=None), dict(n_hb=None), dict(status=None), dict(hb=None),
               dict(extra=None), dict(n_atoms=0), dict(n_atoms=513), dict(max_hb=-1), dict(extra=bad_extra), dict(extra=low_extra),
               dict(d_min=np.nan), dict(d_max=np.inf), dict(max_angle=np.nan), dict(d_min=3.3), dict(d_min=3.4), dict(mode=2), dict(n_extra=65),
               dict(n_structs=-1), dict(hydrogen=np.array([1, 1, 1, 0], np.uint8))]
    for kw in refused:
        assert hbonds(**kw) == TSC_ERR_INVALID, kw
    for kw in refused:                                                      # (the _dev form checks what lies on the host the same way)
        if "extra" in kw and kw["extra"] is not None:
            continue
        assert hbonds(fn=lib.tsc_hbonds_dev, **kw) == TSC_ERR_INVALID, kw
    assert all((v == (7 if k == "status" else -7)).all() for k, v in outs.items())   # nothing was launched: nothing was written
    assert hbonds(n_structs=0) == 0
    assert all((v == (7 if k == "status" else -7)).all() for k, v in outs.items())

    tors = np.array([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32)
    set_off = np.array([0, 2], np.int32)
    con = np.array([[0, -1]], np.int32)
    flags, masks = np.full(2, 7, np.uint8), np.full((2, n), 7, np.uint8)

    def reach(fn=lib.tsc_torsion_reach, **kw):
        a = dict(graph=bits[:1], n_graphs=1, n_atoms=n, torsions=tors, set_off=set_off, constrained=con, n_con=2, flags=flags, masks=masks)
        a.update(kw)
        return fn(h, ptr(a["graph"]), C.c_int(a["n_graphs"]), C.c_int(a["n_atoms"]), ptr(a["torsions"]), ptr(a["set_off"]), ptr(a["constrained"]),
                  C.c_int(a["n_con"]), ptr(a["flags"]), ptr(a["masks"]))

    def t(row, k, v):
        out = tors.copy()
        out[row, k] = v
        return out
    refused = [dict(graph=None), dict(torsions=None), dict(set_off=None), dict(constrained=None), dict(flags=None), dict(masks=None),
               dict(n_atoms=0), dict(n_atoms=513), dict(n_graphs=-1), dict(n_con=-1), dict(set_off=np.array([1, 2], np.int32)),
               dict(set_off=np.array([0, -1], np.int32)), dict(torsions=t(0, 0, -1)), dict(torsions=t(1, 3, n)), dict(torsions=t(0, 1, 2)),
               dict(constrained=np.array([[0, n]], np.int32)), dict(constrained=np.array([[-2, 0]], np.int32))]
    for kw in refused:
        assert reach(**kw) == TSC_ERR_INVALID, kw
    for kw in refused[:12]:
        assert reach(fn=lib.tsc_torsion_reach_dev, **kw) == TSC_ERR_INVALID, kw
    assert (flags == 7).all() and (masks == 7).all()
    assert reach(n_graphs=0) == 0 and reach(set_off=np.array([0, 0], np.int32)) == 0
    assert reach(fn=lib.tsc_torsion_reach_dev, n_graphs=0) == 0
    assert (flags == 7).all() and (masks == 7).all()
    with pytest.raises(TscodeHipError) as err:
        eng.torsion_reach(bits[:1], t(0, 1, 2), set_off, None)
    assert err.value.code == TSC_ERR_INVALID
