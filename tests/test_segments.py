"""tscode_amd.segments: the argument lists of the many-ensembles calls.

The corpus below is a table of calls of the six batch front ends.  tests/golden/segments_corpus.json states for each of them what
the commit BEFORE the front ends moved onto tscode_amd.segments did with it, recorded by running that commit's package on this very
table (``PYTHONPATH=<a checkout of that commit> python tests/test_segments.py --record <file>``): the exception type and full
message of a refusal, the module whose get_engine() was asked for an input that reaches the library, or the number of results of a
call that returns without it.  The test asserts the same outcomes of the package as it is now."""

import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = os.path.join(ROOT, "tests", "golden", "segments_corpus.json")

_rng = np.random.default_rng(20)
A, B, Cc = _rng.normal(size=(6, 5, 3)), _rng.normal(size=(4, 7, 3)), _rng.normal(size=(2, 3, 3))
ENS = [A, B, Cc]                                        # differing atom counts, a two-structure segment
SAME = [A, A[:4] + 0.1, A[:2] - 0.1]                     # one molecule: what "one array for all" is for
ZA, ZB, ZC = np.array([6, 1, 8, 6, 1]), np.array([6, 6, 1, 7, 8, 1, 1]), np.array([8, 1, 1])
Z = [ZA, ZB, ZC]
MA, MB, MC = np.arange(1.0, 6.0), np.arange(1.0, 8.0), np.arange(1.0, 4.0)
Q = np.array([[0, 1, 2, 1]], dtype=np.int32)            # in range for every ensemble
Q5 = np.array([[0, 1, 2, 3], [1, 2, 3, 4]])             # in range for five atoms and more
NAN, INF = float("nan"), float("inf")


def objarr(entries):
    """The 1-D array of dtype object that holds ``entries`` (what np.array gives for arrays of different lengths, where it gives one)."""
    a = np.empty(len(entries), dtype=object)
    for i, e in enumerate(entries):
        a[i] = e
    return a


def setup(n, torsions=((0, 1, 2, 1),), **changed):
    """A rot-corr set-up for n atoms whose every atom is in every local subgraph (only its shape is looked at before the library)."""
    T = len(torsions)
    out = dict(torsions=np.array(torsions, dtype=np.int32).reshape(T, 4), angles=[[0.0, 120.0, 240.0]] * T,
               move_masks=np.tile(np.arange(n) >= n - 1, (T, 1)), sub_nodes=[[0]] * T)
    out.update(changed)
    return out


SA, SB, SC, S0 = setup(5), setup(7), setup(3), setup(5, torsions=())
SETUPS = [SA, SB, SC]


def corpus():
    """[(id, front end, args, kwargs)]"""
    c = []

    def add(name, fn, *args, **kwargs):
        c.append((f"{fn}:{name}", fn, args, kwargs))

    # ---- what every front end takes as its list of ensembles
    lists = {"rmsd": ("prune_conformers_rmsd_batch", lambda e, z: ((e, z), {})),
             "tfd": ("prune_conformers_tfd_batch", lambda e, z: ((e, Q), {})),
             "moi": ("prune_by_moment_of_inertia_batch", lambda e, z: ((e, z), {"masses": None if z is None else [np.ones(len(a)) for a in z]})),
             "rot_corr": ("prune_rmsd_rot_corr_arrays_batch", lambda e, z: ((e, z, None if z is None else [setup(len(a)) for a in z]), {})),
             "refine": ("similarity_refining_batch", lambda e, z: ((e, z), {})),
             "diverse": ("diverse_select_batch", lambda e, z: ((e, 2), {"seeds": None if z is None else list(range(len(z)))}))}
    for key, (fn, build) in lists.items():
        for name, e, z in (("mixed", ENS, Z), ("same", SAME, [ZA] * 3), ("empty_list", [], []), ("list_of_one", [A], [ZA]),
                           ("tuple", tuple(ENS), Z), ("stacked_4d", np.stack([A, A, A]), [ZA] * 3), ("no_structures_in_one", [A, B[:0], Cc], Z),
                           ("array_3d_as_list", A, [ZA] * 6), ("entry_2d", [A, B[0], Cc], Z), ("entry_xy_only", [A, B[:, :, :2], Cc], Z),
                           ("entry_4d", [A, B[None], Cc], Z), ("no_atoms_in_one", [A, B[:, :0], Cc], [ZA, ZB[:0], ZC]),
                           ("float32", [x.astype(np.float32) for x in ENS], Z), ("nested_lists", [x.tolist() for x in ENS], Z)):
            args, kwargs = build(e, z)
            add(name, fn, *args, **kwargs)

    # ---- atomnos (and masses): one array for all, or one per ensemble
    for key in ("rmsd", "moi", "rot_corr", "refine"):
        fn = lists[key][0]
        tail = {"rot_corr": lambda e: (SA if e is SAME else SETUPS,)}.get(key, lambda e: ())
        for name, e, z in (("atomnos_one_array", SAME, ZA), ("atomnos_flat_list", SAME, ZA.tolist()), ("atomnos_flat_tuple", SAME, tuple(ZA.tolist())),
                           ("atomnos_stacked", SAME, np.stack([ZA] * 3)), ("atomnos_list_of_lists", SAME, [ZA.tolist()] * 3),
                           ("atomnos_one_array_mixed", ENS, ZA), ("atomnos_two_for_three", ENS, Z[:2]), ("atomnos_four_for_three", ENS, Z + [ZC]),
                           ("atomnos_one_in_a_list", ENS, [ZA]), ("atomnos_empty_list", ENS, []), ("atomnos_an_atom_short", ENS, [ZA, ZB[:-1], ZC]),
                           ("atomnos_object_array", ENS, objarr(Z)), ("atomnos_object_array_of_lists", ENS, objarr([z.tolist() for z in Z])),
                           ("atomnos_object_array_same", SAME, objarr([ZA] * 3)), ("atomnos_object_array_two_for_three", ENS, objarr(Z[:2])),
                           ("atomnos_object_array_of_numbers", SAME, objarr(ZA.tolist())),
                           ("atomnos_2d_entry", ENS, [ZA, ZB[None], ZC]), ("atomnos_stacked_two", SAME, np.stack([ZA] * 2)),
                           ("hydrogens_only_in_one", ENS, [ZA, np.ones(7, dtype=int), ZC]),
                           ("hydrogens_only_first_and_short_second", ENS, [np.ones(5, dtype=int), ZB[:-1], ZC])):
            add(name, fn, e, z, *tail(e))
    for key in ("moi", "refine"):
        fn = lists[key][0]
        for name, e, z, m in (("masses_one_array", SAME, ZA, MA), ("masses_flat_list", SAME, ZA, MA.tolist()), ("masses_stacked", SAME, ZA, np.stack([MA] * 3)),
                              ("masses_each", ENS, Z, [MA, MB, MC]), ("masses_one_array_mixed", ENS, Z, MA), ("masses_two_for_three", ENS, Z, [MA, MB]),
                              ("masses_one_short", ENS, Z, [MA, MB[:-1], MC]), ("masses_none_entry", ENS, Z, [MA, None, MC]),
                              ("masses_object_array", ENS, Z, objarr([MA, MB, MC])), ("masses_object_array_same", SAME, ZA, objarr([MA] * 3)),
                              ("masses_empty_list", ENS, Z, []), ("no_builtin_mass", ENS, [ZA, np.array([6, 6, 1, 7, 8, 1, 92]), ZC], None)):
            add(name, fn, e, z, masses=m)

    # ---- scalar or one per ensemble
    for key, kw, tail in (("rmsd", "rmsd_thr", ()), ("tfd", "thresh", ()), ("moi", "max_deviation", ()), ("rot_corr", "max_rmsd", (SETUPS,)),
                          ("refine", "rmsd_thr", ())):
        fn = lists[key][0]
        second = Q if key == "tfd" else Z
        for name, v in (("python_float", 0.3), ("array_0d", np.array(0.3)), ("each_list", [0.3, 0.2, 0.1]), ("each_array", np.array([0.3, 0.2, 0.1])),
                        ("each_int", [1, 2, 3]), ("one_in_a_list", [0.3]), ("four_for_three", [0.3] * 4), ("two_d", [[0.3, 0.2, 0.1]]),
                        ("empty", []), ("nan", NAN), ("inf_in_one", [0.3, INF, 0.1]), ("nan_in_one", [0.3, NAN, 0.1]), ("negative", -1.0)):
            add(f"{kw}_{name}", fn, ENS, second, *tail, **{kw: v})

    # ---- quadruplets: one (T, 4) array for all, or one per ensemble
    q_each = [Q5, np.zeros((0, 4), dtype=np.int32), Q]
    for fn, call in (("prune_conformers_tfd_batch", lambda q: ((ENS, q), {})),
                     ("similarity_refining_batch", lambda q: ((ENS, Z), {"quadruplets": q})),
                     ("most_diverse_conformers_batch", lambda q: ((2, ENS, q), {"seeds": [1, 2, 3]}))):
        for name, q in (("one_array", Q), ("list_of_4_tuples", [(0, 1, 2, 1)]), ("three_4_tuples", [(0, 1, 2, 1), (1, 2, 0, 1), (2, 1, 0, 1)]),
                        ("one_flat_quadruplet", [0, 1, 2, 1]), ("one_flat_array", np.array([0, 1, 2, 1])), ("stacked", np.stack([Q] * 3)),
                        ("each", q_each), ("each_as_lists", [q.tolist() for q in q_each]), ("empty_list", []), ("empty_array", np.zeros((0, 4), dtype=np.int32)),
                        ("two_for_three", q_each[:2]), ("four_for_three", q_each + [Q]), ("one_in_a_list", [Q]), ("stacked_two", np.stack([Q] * 2)),
                        ("object_array", objarr(q_each)), ("object_array_same", objarr([Q, Q, Q])), ("object_array_of_lists", objarr([q.tolist() for q in q_each])),
                        ("object_array_two_for_three", objarr(q_each[:2])), ("object_array_none_entries", objarr([Q5, None, None])),
                        ("none_entries", [Q5, None, None]), ("none_first", [None, Q5, Q]), ("none", None),
                        ("index_out_of_range_for_one", np.array([[0, 1, 2, 3]])), ("negative_index", [Q5, np.array([[0, -1, 2, 3]]), Q]),
                        ("index_n_of_n", [Q5, np.array([[0, 1, 2, 7]]), Q]), ("five_columns", np.array([[0, 1, 2, 1, 0]]))):
            args, kwargs = call(q)
            add(f"quadruplets_{name}", fn, *args, **kwargs)

    # ---- rot-corr set-ups: one dict for all, or one per ensemble
    n = 5
    for fn, call in (("prune_rmsd_rot_corr_arrays_batch", lambda e, z, st, **kw: ((e, z, st), kw)),
                     ("similarity_refining_batch", lambda e, z, st, **kw: ((e, z), dict(rot_corr=st, **kw)))):
        for name, e, z, st in (("one_dict", SAME, ZA, SA), ("one_dict_mixed", ENS, Z, SA), ("each", ENS, Z, SETUPS), ("each_tuple", ENS, Z, tuple(SETUPS)),
                               ("object_array", ENS, Z, objarr(SETUPS)), ("object_array_two_for_three", ENS, Z, objarr(SETUPS[:2])),
                               ("two_for_three", ENS, Z, SETUPS[:2]), ("four_for_three", ENS, Z, SETUPS + [SC]), ("one_in_a_list", ENS, Z, [SA]),
                               ("empty_list", ENS, Z, []), ("none", ENS, Z, None), ("none_entry", ENS, Z, [SA, None, SC]),
                               ("none_then_bad", ENS, Z, [None, setup(7, torsions=((0, 1, 2, 7),)), SC]),
                               ("not_a_dict", ENS, Z, [SA, "torsions", SC]), ("key_missing", ENS, Z, [SA, {k: v for k, v in SB.items() if k != "angles"}, SC]),
                               ("no_torsion_anywhere", SAME, ZA, S0), ("no_torsion_in_one", SAME, ZA, [SA, S0, SA]),
                               ("torsion_index_n_of_n", SAME, ZA, [SA, setup(n, torsions=((0, 1, 2, n),)), SA]),
                               ("torsion_index_negative", SAME, ZA, [SA, SA, setup(n, torsions=((0, -1, 2, 3),))]),
                               ("subgraph_index_out_of_range", SAME, ZA, [setup(n, sub_nodes=[[0, n]]), SA, SA]),
                               ("subgraph_empty", SAME, ZA, [SA, setup(n, sub_nodes=[[]]), SA]),
                               ("seventeen_torsions", SAME, ZA, [SA, setup(n, torsions=((0, 1, 2, 1),) * 17), SA]),
                               ("seven_angles", SAME, ZA, [SA, setup(n, angles=[np.arange(7.0)]), SA]),
                               ("angle_not_finite", SAME, ZA, [SA, setup(n, angles=[[0.0, NAN]]), SA]),
                               ("masks_of_another_molecule", SAME, ZA, [SA, SB, SA]),
                               ("hydrogens_only_with_torsions", SAME, [ZA, np.ones(5, dtype=int), ZA], SA),
                               ("hydrogens_only_without_torsions", SAME, [ZA, np.ones(5, dtype=int), ZA], [SA, S0, SA])):
            args, kwargs = call(e, z, st)
            add(f"setups_{name}", fn, *args, **kwargs)
    for name, kw in (("max_structures_lets_one_in", dict(max_structures=3)), ("max_structures_lets_none_in", dict(max_structures=1)),
                     ("max_structures_none", dict(max_structures=None))):
        add(name, "prune_rmsd_rot_corr_arrays_batch", ENS, Z, SETUPS, **kw)
    add("list_of_one_without_torsions", "prune_rmsd_rot_corr_arrays_batch", [A], ZA, S0)
    add("list_of_one_of_one_structure", "prune_rmsd_rot_corr_arrays_batch", [A[:1]], [ZA], [SA])
    for name, kw in (("all_stages_off", dict(tfd=False, moi=False, rmsd=False)), ("only_rmsd", dict(tfd=False, moi=False)), ("only_moi", dict(tfd=False, rmsd=False)),
                     ("only_tfd", dict(moi=False, rmsd=False))):
        add(name, "similarity_refining_batch", ENS, Z, quadruplets=[Q5, None, Q], rot_corr=[SA, None, SC], masses=[MA, MB, MC], **kw)
        add(name + "_nothing_given", "similarity_refining_batch", ENS, Z, **kw)
    add("hydrogens_only_all_stages_off", "similarity_refining_batch", [A], np.ones(5, dtype=int), tfd=False, moi=False, rmsd=False)

    # ---- diverse selection: k, init_rows, seeds, energies as lists with None entries
    en = [np.arange(6.0), np.arange(4.0), np.arange(2.0)]
    for name, k, kw in (("k_int", 2, {}), ("k_each", [3, 2, 1], {}), ("k_each_array", np.array([3, 2, 1]), {}), ("k_two_for_three", [3, 2], {}),
                        ("k_too_large_for_one", 3, {}), ("k_zero", 0, {}), ("k_array_0d", np.array(2), {}),
                        ("seeds_each", 2, dict(seeds=[1, 2, 3])), ("seeds_none_entry", 2, dict(seeds=[1, None, 3])), ("seeds_two_for_three", 2, dict(seeds=[1, 2])),
                        ("seeds_empty_list", 2, dict(seeds=[])), ("seeds_one_int", 2, dict(seeds=7)), ("seeds_array", 2, dict(seeds=np.array([1, 2, 3]))),
                        ("init_rows_each", 2, dict(init_rows=[[0, 1], [1, 3], [0, 1]])), ("init_rows_none_entry", 2, dict(init_rows=[[0, 1], None, [1, 0]])),
                        ("init_rows_stacked", 2, dict(init_rows=np.array([[0, 1], [1, 3], [0, 1]]))), ("init_rows_one_for_all", 2, dict(init_rows=[0, 1])),
                        ("init_rows_two_for_three", 2, dict(init_rows=[[0, 1], [1, 3]])), ("init_rows_out_of_range", 2, dict(init_rows=[[0, 1], [1, 4], [0, 1]])),
                        ("init_rows_wrong_count_in_one", 2, dict(init_rows=[[0, 1], [1, 2, 3], [0, 1]])),
                        ("energies_object_array", 2, dict(energies=objarr(en))), ("init_rows_object_array", 2, dict(init_rows=objarr([[0, 1], None, [1, 0]]))),
                        ("seeds_object_array", 2, dict(seeds=objarr([1, None, 3]))), ("k_object_array", objarr([3, 2, 1]), {}),
                        ("energies_each", 2, dict(energies=en)), ("energies_none_entry", 2, dict(energies=[en[0], None, en[2]])),
                        ("energies_two_for_three", 2, dict(energies=en[:2])), ("energies_one_for_all", 2, dict(energies=en[0])),
                        ("energies_short_in_one", 2, dict(energies=[en[0], en[1][:-1], en[2]])), ("energies_nan", 2, dict(energies=[en[0], en[1], [0.0, NAN]])),
                        ("structures_not_finite", 2, dict(ensembles=[A, np.where(np.arange(7)[:, None] == 3, NAN, B), Cc]))):
        kw = dict(kw)
        add(name, "diverse_select_batch", kw.pop("ensembles", ENS), k, **kw)
    for name, nn, kw in (("n_int", 2, {}), ("n_each", [3, 2, 1], {}), ("n_two_for_three", [3, 2], {}), ("n_covers_all", 6, {}), ("n_above_300", [301, 2, 1], {}),
                         ("energies_each", 2, dict(energies=en)), ("energies_two_for_three", 2, dict(energies=en[:2])), ("seeds_two_for_three", 2, dict(seeds=[1, 2])),
                         ("init_rows_four_for_three", 2, dict(init_rows=[None] * 4)), ("empty_list", 2, dict(ensembles=[])),
                         ("list_of_one", 2, dict(ensembles=[A])), ("stacked_4d", 2, dict(ensembles=np.stack([A, A, A])))):
        kw = dict(kw)
        add(name, "most_diverse_conformers_batch", nn, kw.pop("ensembles", ENS), Q, **kw)
    assert len({name for name, *_ in c}) == len(c), "two corpus entries of one name"
    return c


class Reached(Exception):
    """get_engine() was called: the arguments passed every check made before the library is entered."""


def outcomes(patch):
    """{id: outcome} of the corpus on the tscode_amd that is importable; ``patch(module, name, value)`` replaces an attribute."""
    import importlib
    import warnings

    import tscode_amd
    for name in sorted(f[:-3] for f in os.listdir(tscode_amd.__path__[0]) if f.endswith(".py") and f not in ("__init__.py", "engine.py")):
        module = importlib.import_module("tscode_amd." + name)
        if hasattr(module, "get_engine"):
            def reached(*a, _name=name, **k):
                raise Reached(_name)
            patch(module, "get_engine", reached)
    out = {}
    for name, fn, args, kwargs in corpus():
        np.random.seed(5)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = getattr(tscode_amd, fn)(*args, **kwargs)
            out[name] = ["returns", len(got)]
        except Reached as r:
            out[name] = ["library", str(r)]
        except Exception as exc:              # noqa: BLE001  (the type and the message are the outcome)
            out[name] = ["raises", type(exc).__name__, str(exc)]
    return out


def test_the_front_ends_do_with_the_corpus_what_they_did_before_they_shared_their_argument_handling(monkeypatch):
    pytest.importorskip("networkx")
    recorded = json.load(open(RECORDED))
    got = outcomes(monkeypatch.setattr)
    assert sorted(got) == sorted(recorded), "the corpus and its recording list different calls"
    differ = {name: (got[name], recorded[name]) for name in got if got[name] != recorded[name]}
    assert not differ, "\n".join(f"{name}: now {g}, recorded {r}" for name, (g, r) in differ.items())
    kinds = {o[0] for o in recorded.values()}
    assert kinds == {"returns", "library", "raises"}


def test_every_front_end_is_in_the_corpus_with_every_kind_of_outcome():
    recorded = json.load(open(RECORDED))
    for fn in ("prune_conformers_rmsd_batch", "prune_conformers_tfd_batch", "diverse_select_batch", "most_diverse_conformers_batch",
               "prune_by_moment_of_inertia_batch", "prune_rmsd_rot_corr_arrays_batch", "similarity_refining_batch"):
        kinds = {o[0] for name, o in recorded.items() if name.startswith(fn + ":")}
        assert kinds == {"returns", "library", "raises"}, (fn, kinds)


# ---- the helpers ------------------------------------------------------------------------------------------------------------------
def slices_as_the_front_ends_wrote_them(costs, budget):
    out, at = [], 0
    while at < len(costs):
        end, nbytes = at, 0
        while end < len(costs) and (end == at or nbytes + costs[end] <= budget):
            nbytes += costs[end]
            end += 1
        out.append((at, end))
        at = end
    return out


def test_byte_slices_are_those_of_the_loop_the_front_ends_wrote_out():
    from tscode_amd.segments import byte_slices
    rng = np.random.default_rng(7)
    assert byte_slices([], 10) == []
    assert byte_slices([5, 5, 5], 0) == [(0, 1), (1, 2), (2, 3)]                  # every slice takes its first entry whatever it costs
    assert byte_slices([3, 20, 3, 3], 10) == [(0, 1), (1, 2), (2, 4)]             # a cost above the budget goes alone
    assert byte_slices([4, 6, 1], 10) == [(0, 2), (2, 3)]                         # a sum that meets the budget still fits
    for _ in range(400):
        costs = rng.integers(0, 50, size=rng.integers(0, 12)).tolist()
        budget = int(rng.choice([0, 1, 10, 49, 60, 200, 10**6]))
        got = byte_slices(costs, budget)
        assert got == slices_as_the_front_ends_wrote_them(costs, budget), (costs, budget)
        assert [i for at, end in got for i in range(at, end)] == list(range(len(costs)))


def pack_heavy_batch_as_it_was(heavies):
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in heavies]
    n = np.array([a.shape[0] for a in arrays], dtype=np.int32)
    h = np.array([a.shape[1] for a in arrays], dtype=np.int32)
    offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
    np.cumsum(n.astype(np.int64) * h * 3, out=offsets[1:])
    flat = np.concatenate([a.ravel() for a in arrays]) if arrays else np.zeros(0)
    return flat, offsets, n, h


@pytest.mark.parametrize("shapes", [[], [(6, 5)], [(6, 5), (4, 7), (2, 3)], [(3, 2), (0, 4), (5, 1)], [(0, 3)], [(1, 1), (0, 9), (0, 2), (7, 3)]])
def test_pack_gives_the_arrays_pack_heavy_batch_gave_and_cuts_results_back(shapes):
    from tscode_amd import pack_heavy_batch
    from tscode_amd.segments import pack
    rng = np.random.default_rng(len(shapes))
    arrays = [rng.normal(size=(N, n, 3)) for N, n in shapes]
    p = pack(arrays)
    for got, wrapped, was in zip(p[:4], pack_heavy_batch(arrays), pack_heavy_batch_as_it_was(arrays)):
        assert got.dtype == wrapped.dtype == was.dtype and got.shape == wrapped.shape == was.shape
        assert got.tobytes() == wrapped.tobytes() == was.tobytes()
        assert got.flags.c_contiguous
    assert p.row_off.dtype == np.int64 and p.row_off.tolist() == np.concatenate(([0], np.cumsum([N for N, _ in shapes]))).tolist()
    assert p.flat.shape == (p.offsets[-1],) and p.offsets[0] == 0
    # the cutter: what was packed comes back ensemble by ensemble, as views of the result array
    back = p.cut(p.flat, doubles=True)
    assert len(back) == len(arrays) and all(b.shape == a.shape and b.tobytes() == a.tobytes() for a, b in zip(arrays, back))
    assert all(b.base is not None and np.shares_memory(b, p.flat) for b in back if b.size)
    rows = np.arange(int(p.row_off[-1]))
    per_row = p.cut(rows)
    assert [r.tolist() for r in per_row] == [list(range(int(p.row_off[s]), int(p.row_off[s + 1]))) for s in range(len(shapes))]
    wide = p.cut(np.stack([rows, -rows], axis=1))                                 # any trailing axes ride along
    assert [w.shape for w in wide] == [(N, 2) for N, _ in shapes] and all(np.array_equal(w[:, 0], r) for w, r in zip(wide, per_row))


def test_pack_heavy_batch_keeps_its_own_refusal():
    from tscode_amd import pack_heavy_batch
    with pytest.raises(ValueError, match=r"ensemble 1: heavy must be \(N, h, 3\), got \(3, 3\)"):
        pack_heavy_batch([np.zeros((2, 4, 3)), np.zeros((3, 3))])


def test_ensemble_list_one_or_each_and_scalar_or_each():
    from tscode_amd.segments import ensemble_list, one_or_each, scalar_or_each
    assert ensemble_list([]) == [] and ensemble_list([A.astype(np.float32)])[0].dtype == np.float32
    sliced = ensemble_list([A[::2], B.tolist()], np.float64)
    assert all(e.flags.c_contiguous and e.dtype == np.float64 for e in sliced) and np.array_equal(sliced[0], A[::2])
    with pytest.raises(ValueError, match="^ensembles must be a list of \\(N, n_atoms, 3\\) arrays$"):
        ensemble_list(A)
    for bad in (B[0], B[:, :, :2], B[:, :0]):
        with pytest.raises(ValueError, match="^ensemble 1: structures must be \\(N, n_atoms, 3\\)$"):
            ensemble_list([A, bad])
    # a (T, 4) array: loosely, whatever has at most its rank stands for all; exactly, only what has its rank
    q = [[0, 1, 2, 3]]
    for value, loose, exact in ((np.array(q), True, True), (q, True, True), ([0, 1, 2, 3], True, False), (np.array(q[0]), True, False), ([], True, False),
                                ([np.array(q)] * 3, False, False), (np.array([q] * 3), False, False), ([None, q, q], True, False)):
        for is_exact, one in ((False, loose), (True, exact)):
            if one or len(value) == 3:
                got = one_or_each(value, 3, "quadruplet arrays", 2, exact=is_exact)
                assert len(got) == 3 and all(g is value for g in got) == one, (value, is_exact)
            else:
                with pytest.raises(ValueError, match=f"^{len(value)} quadruplet arrays for 3 ensembles$"):
                    one_or_each(value, 3, "quadruplet arrays", 2, exact=is_exact)
    assert [len(one_or_each([], 3, "atomnos arrays", 1, exact=e)) for e in (False, True)] == [3, 3]    # an empty list has rank 1
    o = objarr([ZA, ZB])                                                          # an object array: its rank decides, unless the caller says otherwise
    assert all(g is o for g in one_or_each(o, 2, "atomnos arrays", 1, exact=True))
    assert [g is z for g, z in zip(one_or_each(o, 2, "atomnos arrays", 1, exact=True, object_rows=True), (ZA, ZB))] == [True, True]
    with pytest.raises(ValueError, match="^2 atomnos arrays for 3 ensembles$"):
        one_or_each(o, 3, "atomnos arrays", 1, exact=True, object_rows=True)
    d = {"torsions": []}
    assert one_or_each(d, 2, "set-ups", None) == [d, d] and one_or_each(None, 2, "seeds", None, allow_none=True) == [None, None]
    assert one_or_each([1, None], 2, "seeds", None) == [1, None]                  # item_ndim None: nothing but a dict stands for all
    with pytest.raises(ValueError, match="^3 seeds for 2 ensembles$"):
        one_or_each([1, 2, 3], 2, "seeds", None)
    with pytest.raises(ValueError, match="^0 seeds for 2 ensembles$"):
        one_or_each([], 2, "seeds", None)
    assert one_or_each([1, 2, 3], 2, "seeds", None, count=False) == [1, 2, 3]
    with pytest.raises(TypeError):
        one_or_each(None, 2, "set-ups", None)
    t = scalar_or_each(0.5, 3, "thresholds")
    assert t.dtype == np.float64 and t.tolist() == [0.5] * 3 and scalar_or_each(np.arange(6.0)[::2], 3, "thresholds").flags.c_contiguous
    assert scalar_or_each([], 0, "thresholds").shape == (0,) and scalar_or_each(1, 0, "thresholds").shape == (0,)
    for bad, size in (([0.5], 1), ([[0.5, 0.5, 0.5]], 3), ([], 0)):
        with pytest.raises(ValueError, match=f"^{size} thresholds for 3 ensembles$"):
            scalar_or_each(bad, 3, "thresholds")


def test_segments_imports_nothing_of_the_engine():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "tscode_amd", "segments.py")).read())
    imported = {a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names} | \
               {node.module for node in ast.walk(tree) if isinstance(node, ast.ImportFrom)}
    assert imported <= {"__future__", "typing", "numpy"}, imported


if __name__ == "__main__":
    # record what the importable tscode_amd does with the corpus (see the module's docstring)
    assert sys.argv[1] == "--record"
    with open(sys.argv[2], "w") as f:
        json.dump(outcomes(setattr), f, indent=1, sort_keys=True)
        f.write("\n")
