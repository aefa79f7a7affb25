"""The front half of the pipeline kernel by kernel -- fused embed + clash verdicts, ordered compaction, masked embed, the embed that writes
the prune's descriptors -- at the sizes where each mechanism begins or ends.  References: the oracle (transform_batch, compenetration_mask,
clash_margin, prune_heavy) and NumPy in float64.

A.  k_clash_lanes_multi (csrc/embed_clash_kernels.hpp) through embed_clash_mask_dev, threshold 1.5, no clash allowed, against the oracle's embed +
    compenetration_mask, and the same call under clash_lanes = 0 (k_clash) and clash_fp32 = 0 (the float64 count).  Every mask starts as
    0xAA bytes and must come back as zeros and ones.
  random    fragments are Gaussian blobs (sigma 1.6 A), several conformers each, the conformer of a pose drawn at random, random rotations,
            fragment 0 at the origin (+ the case's offset), the others at Gaussian distances whose scale is chosen so that, by the oracle,
            20 - 80 % of the poses clash.  The shapes hit every register tile (the launcher's cost rule, restated: tile_cost / chosen_tile),
            an "A" fragment of 2 NA2 - 1, 2 NA2 and 2 NA2 + 1 atoms for every tile (one padded lane, none, a second tile of one atom), a
            one-atom fragment in each position, and offsets 1e5 (a wide band: many float64 recounts) and 1e16 (no usable band: all recounted);
  counts    the first 63 ... 3011 poses of one ensemble of three fragments and of one of two (CLM_POSES = 512: the workgroup's block; 64: the
            wavefront), and a single pose of either verdict;
  pairs     three compact fragments whose centres coincide for the pairs meant to clash and lie 40 A apart otherwise: a fifth of the poses
            clash in (m2, m1) only, in (m3, m2) only, in (m1, m3) only, in none, in all three, shuffled -- except the second block of 512,
            where every pose clashes in the first pair and nothing is left to pack; one ensemble where all clash in the first pair, one
            where none clashes;
  band      fragments are one exposed atom and a tight clump 9 A from it; the exposed atoms of one fragment pair sit 1.5 + eps apart, eps
            from 0 to +-1e-3, the rest is far away -- for each of the three pairs; then the first pair inside the band while (m1, m3) clashes
            clearly, and the reverse.  Compared from |eps| >= 1e-9 on (below that the last bits of the embedding decide);
  non-finite a NaN translation, an all-infinite pose, one infinite coordinate of a conformer: count(D < thresh) <= 0 decides.
B.  compact_rows_dev / gather_heavy_dev (csrc/scan_kernels.hpp, gather_rows.hpp) bit for bit against NumPy's src[mask != 0] at the row counts around the scan's 8-byte
    load, its 2048-byte tile, more than 256 scan blocks and more output words than the gather's grid holds threads; embed_clash_compact_dev
    and embed_masked_dev (k_transform with an index list and a slot table) at selected counts around TR_POSES = 32, with heavy-atom patterns
    of every kind, against the oracle within 4 * 2^-53 (|R| |x| + |t|) per component (three products, three sums, fused or not), the
    outputs of one kernel bit-identical whatever the entry point; the tables the context caches between calls (heavy_slot_table,
    basis_sample_table in csrc/pipeline.hip) against fresh contexts.
C.  k_transform_describe (csrc/describe.hpp): the structure-level cases of tests/test_screen_limit.py -- pairs PLACED at the descriptor
    screens' limit -- as pose lists that embed exactly (every structure is conformer s of two fragments, identity rotations, zero
    translations), through tsc_pipeline_dev and through the multi-rank front's sequence basis_from_poses_dev -> embed_masked_dev ->
    tsc_prune_create, also with a basis forked from a foreign ensemble; random ensembles on both sides of the kernel's LDS gate.

Left out: the grid-stride second rounds of k_clash_lanes_multi (more than 8192 x 512 poses), of k_clash (more than 8192 x 4 wavefronts of
poses) and of k_transform / k_transform_describe (more than 16384 x 32 selected poses) need millions of poses: not a seconds-sized test.
"""
import zlib

import numpy as np
import pytest

from test_screen_limit import CACHE_SKIPS, MM16, MM64_CULLED, STRUCT_CASES, THR, per_pass, struct_case, struct_reference

THRESH = 1.5
BAND_EPS = (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)
BAND_REPS = 6
BAND_SKIP = 3 * BAND_REPS                      # eps = 0, +-1e-12: decided by the last bits of the embedding
CLM_POSES, TR_POSES, SCAN_TILE = 512, 32, 2048
U53 = 2.0 ** -53


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rotations(rng, shape):
    from tscode_amd.synthetic import quat_to_mat
    return quat_to_mat(rng.normal(size=tuple(shape) + (4,)))


# ------------------------------------------------------------------------------------------------------------------ A: the tile rule
def tile_cost(sizes, na2):
    """csrc/embed.hip, the `cost` lambda of launch_clash: padded distances over the fragment pairs (A, B) = (m2, m1), (m3, m2), (m1, m3)
    (two fragments: (m2, m1)), the B atoms embedded once per tile counted in."""
    pairs = [(1, 0)] if len(sizes) == 2 else [(1, 0), (2, 1), (0, 2)]
    return sum(-(-sizes[a] // (2 * na2)) * sizes[b] * (2 * na2 + 4) for a, b in pairs)


def chosen_tile(sizes):
    best = 12
    for na2 in (16, 18):
        if tile_cost(sizes, na2) < tile_cost(sizes, best):
            best = na2
    return best


def takes_multi(sizes):
    """Two fragments reach k_clash_lanes_multi only when the smaller one has more than 32 atoms (k_clash_lanes takes the others)."""
    return len(sizes) == 3 or min(sizes) > 32


# name: (atoms per fragment, conformers per fragment, poses, scale of the placement, offset, half-tile the rule must choose)
RANDOM_CASES = {
    "two-33-37": ((33, 37), (2, 3), 700, 4.5, 0.0, 12),
    "two-35-49": ((35, 49), (3, 1), 700, 5.0, 0.0, 16),
    "two-33-33": ((33, 33), (1, 2), 700, 4.5, 0.0, 18),
    "three-24-24-24": ((24, 24, 24), (2, 1, 3), 700, 6.0, 0.0, 12),
    "three-25-24-23": ((25, 24, 23), (3, 1, 4), 700, 6.0, 0.0, 16),
    "three-36-36-36": ((36, 36, 36), (1, 2, 2), 700, 6.4, 0.0, 18),
    "three-1-1-1": ((1, 1, 1), (4, 2, 3), 700, 1.2, 0.0, 12),
    "three-70-70-60": ((70, 70, 60), (2, 2, 1), 700, 7.5, 0.0, 18),
    # an "A" fragment (m2, m3 and m1 all are one, in turn) of 2 NA2 - 1 / 2 NA2 / 2 NA2 + 1 atoms under every tile size
    "tile12-edges": ((24, 23, 24), (2, 2, 2), 600, 6.0, 0.0, 12),
    "tile12-over": ((12, 25, 12), (1, 3, 2), 600, 5.0, 0.0, 12),
    "tile16-edges": ((32, 31, 32), (2, 1, 2), 600, 6.4, 0.0, 16),
    "tile16-over": ((7, 33, 30), (2, 2, 1), 600, 5.5, 0.0, 16),
    "tile18-edges": ((36, 35, 36), (1, 2, 2), 600, 6.4, 0.0, 18),
    "tile18-over": ((29, 37, 35), (2, 1, 3), 600, 6.4, 0.0, 18),
    "one-atom-first": ((1, 30, 40), (3, 2, 2), 600, 4.5, 0.0, None),
    "one-atom-middle": ((30, 1, 40), (2, 3, 2), 600, 4.9, 0.0, None),
    "one-atom-last": ((30, 40, 1), (2, 2, 3), 600, 4.9, 0.0, None),
    "offset-1e5": ((25, 24, 23), (2, 2, 2), 1500, 6.0, 1.0e5, 16),
    "offset-1e16": ((25, 24, 23), (2, 2, 2), 600, 5.5, 1.0e16, 16),
    # the ensembles whose leading poses make the pose counts around the workgroup's block and the wavefront
    "counts-three": ((25, 24, 23), (3, 1, 4), 3011, 6.0, 0.0, 16),
    "counts-two": ((33, 37), (2, 5), 3011, 4.5, 0.0, 12),
}
POSE_COUNTS = (63, 64, 65, 511, 512, 513, 1025, 3011)
TILE_EDGES = {"tile12-edges": (23, 24), "tile12-over": (25,), "tile16-edges": (31, 32), "tile16-over": (33,), "tile18-edges": (35, 36),
              "tile18-over": (37,)}
_cases, _refs = {}, {}


def random_case(name):
    """(fragments, conf_idx i32[n, m], rot f64[n, m, 3, 3], pos f64[n, m, 3], ids) of a random ensemble, built once."""
    if name not in _cases:
        sizes, n_conf, n, scale, offset, _ = RANDOM_CASES[name]
        rng = _rng(name)
        frags = [rng.normal(size=(c, a, 3)) * (1.6 if a > 1 else 0.4) for a, c in zip(sizes, n_conf)]
        ci = np.stack([rng.integers(0, c, size=n) for c in n_conf], axis=1).astype(np.int32)
        rot = _rotations(rng, (n, len(sizes)))
        pos = rng.normal(size=(n, len(sizes), 3)) * scale
        pos[:, 0] = 0.0
        _cases[name] = (frags, ci, np.ascontiguousarray(rot), np.ascontiguousarray(pos + offset), np.array(sizes, dtype=np.int32))
    return _cases[name]


def clash_reference(oracle, key, case):
    """(the oracle's verdicts bool[n], its embedded poses) of a case, computed once and left unchanged."""
    if key not in _refs:
        frags, ci, rot, pos, ids = case
        poses = oracle.transform_batch(frags, ci, rot, pos)
        mask = oracle.compenetration_mask(poses, ids, THRESH, 0).astype(bool)
        mask.setflags(write=False)
        poses.setflags(write=False)
        _refs[key] = (mask, poses)
    return _refs[key]


# ------------------------------------------------------------------------------------------------------- A: which pair clashes
PAIR_SIZES, PAIR_CONF = (14, 11, 17), (2, 3, 2)
PAIRS = ((1, 0), (2, 1), (0, 2))               # numba_functions.py:87-105: (m2, m1), (m3, m2), (m1, m3)
ONLY_0, ONLY_1, ONLY_2, NONE, ALL = range(5)
PAIR_CASES = ("mixed", "all-in-first-pair", "none-anywhere")


def pair_case(name):
    """Three compact fragments; cls[s] says which fragment pairs of pose s clash: the centres of the fragments of such a pair coincide (to
    0.3 A), all others lie 40 A apart.  Returns (case, cls)."""
    key = "pairs-" + name
    if key not in _cases:
        rng = _rng(key)
        if name == "mixed":
            n = 3 * CLM_POSES + 217
            cls = rng.permutation(n) % 5
            cls[CLM_POSES:2 * CLM_POSES] = rng.choice([ONLY_0, ALL], size=CLM_POSES)      # nothing of this block survives the first pair
        elif name == "all-in-first-pair":
            n = CLM_POSES + 301
            cls = rng.choice([ONLY_0, ALL], size=n)
        else:
            n = CLM_POSES + 301
            cls = np.full(n, NONE)
        frags = [rng.normal(size=(c, a, 3)) * 1.2 for a, c in zip(PAIR_SIZES, PAIR_CONF)]
        ci = np.stack([rng.integers(0, c, size=n) for c in PAIR_CONF], axis=1).astype(np.int32)
        rot = _rotations(rng, (n, 3))
        home = np.array([[0.0, 0.0, 0.0], [40.0, 0.0, 0.0], [0.0, 40.0, 0.0]])
        pos = home[None] + rng.normal(size=(n, 3, 3))
        jitter = rng.normal(size=(n, 3, 3)) * 0.3
        for c, (a, b) in enumerate(PAIRS):
            sel = cls == c
            pos[sel, a] = pos[sel, b] + jitter[sel, a]
        sel = cls == ALL
        pos[sel, 1] = pos[sel, 0] + jitter[sel, 1]
        pos[sel, 2] = pos[sel, 0] + jitter[sel, 2]
        pos = pos + rng.normal(size=(n, 1, 3)) * 5.0                    # (no fragment always near the origin)
        _cases[key] = ((frags, ci, np.ascontiguousarray(rot), np.ascontiguousarray(pos), np.array(PAIR_SIZES, dtype=np.int32)), cls)
    return _cases[key]


def pair_table(oracle, poses):
    """clash[s, p]: does fragment pair p of pose s hold a distance below the threshold (the oracle on the two fragments alone)."""
    off = np.concatenate([[0], np.cumsum(PAIR_SIZES)])
    out = np.empty((len(poses), 3), dtype=bool)
    for p, (a, b) in enumerate(PAIRS):
        two = np.ascontiguousarray(np.concatenate([poses[:, off[a]:off[a + 1]], poses[:, off[b]:off[b + 1]]], axis=1))
        out[:, p] = ~oracle.compenetration_mask(two, [PAIR_SIZES[a], PAIR_SIZES[b]], THRESH, 0).astype(bool)
    return out


# ------------------------------------------------------------------------------------------------------------------- A: the band
BAND_SIZES = (25, 20, 30)
# name: (the two fragments whose exposed atoms sit 1.5 + eps apart, the third fragment, the fragment the third one runs into or None)
BAND_CASES = {
    "band-in-m2-m1": ((0, 1), 2, None),
    "band-in-m3-m2": ((1, 2), 0, None),
    "band-in-m1-m3": ((2, 0), 1, None),
    "band-in-m2-m1-clash-in-m1-m3": ((0, 1), 2, 0),        # the carried minimum ends below the band: a clash, whatever eps
    "clash-in-m2-m1-band-in-m1-m3": ((0, 2), 1, 0),        # leaves after the first pair
}


def band_case(name):
    """Fragments: atom 0 at the origin, the others a clump (sigma 0.4) 9 A along +x.  Fragment A stands upright at a random place; B is
    turned so that its clump points along d, away from A's (d_x <= 0), its atom 0 at A's atom 0 + d (1.5 + eps).  The third fragment: 40 A
    off, or with its atom 0 in the middle of the clump of the fragment it runs into, its own clump a further 9 A out."""
    key = "band-" + name
    if key not in _cases:
        from tscode_amd.algebra import rotation_matrix_from_vectors
        (fa, fb), fc, into = BAND_CASES[name]
        rng = _rng(key)
        frags = []
        for a in BAND_SIZES:
            f = rng.normal(size=(1, a, 3)) * 0.4 + np.array([9.0, 0.0, 0.0])
            f[0, 0] = 0.0
            frags.append(f)
        ex = np.array([1.0, 0.0, 0.0])
        rot_l, pos_l = [], []
        for eps in BAND_EPS:
            for _ in range(BAND_REPS):
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                d[0] = -abs(d[0])
                shift = rng.normal(size=3) * 15.0                      # (large coordinates widen the band)
                R, t = np.empty((3, 3, 3)), np.empty((3, 3))
                R[fa], t[fa] = np.eye(3), shift
                R[fb], t[fb] = rotation_matrix_from_vectors(ex, d), shift + d * (1.5 + eps)
                if into is None:
                    R[fc], t[fc] = np.eye(3), shift + np.array([0.0, 0.0, 40.0])
                else:
                    assert into == fa
                    R[fc], t[fc] = np.eye(3), shift + 9.0 * ex
                rot_l.append(R), pos_l.append(t)
        n = len(rot_l)
        _cases[key] = (frags, np.zeros((n, 3), dtype=np.int32), np.array(rot_l), np.array(pos_l), np.array(BAND_SIZES, dtype=np.int32))
    return _cases[key]


# --------------------------------------------------------------------------------------------------------------- A: non-finite
def nonfinite_case():
    key = "non-finite"
    if key not in _cases:
        frags, ci, rot, pos, ids = random_case("three-25-24-23")
        frags = [f.copy() for f in frags]
        ci, pos = ci.copy(), pos.copy()
        pos[5, 1, 2] = np.nan                                          # a NaN translation
        pos[77] = np.inf                                               # an all-infinite pose
        pos[78, 2] = -np.inf
        extra = frags[2][:1].copy()                                    # one infinite coordinate: a conformer of its own, used by two poses
        extra[0, 7, 1] = np.inf
        frags[2] = np.concatenate([frags[2], extra])
        ci[300, 2] = ci[601, 2] = len(frags[2]) - 1
        pos[650, 0, 0] = np.nan
        _cases[key] = (frags, ci, rot, pos, ids)
    return _cases[key]


# --------------------------------------------------------------------------------------------------------- A: without a GPU
def test_cost_rule_sends_the_shapes_to_every_tile_size():
    assert {chosen_tile(c[0]) for c in RANDOM_CASES.values() if len(c[0]) == 2} == {12, 16, 18}
    assert {chosen_tile(c[0]) for c in RANDOM_CASES.values() if len(c[0]) == 3} == {12, 16, 18}
    for name, (sizes, n_conf, n, _, _, tile) in RANDOM_CASES.items():
        assert takes_multi(sizes), name
        assert tile is None or chosen_tile(sizes) == tile, (name, chosen_tile(sizes))
        assert len(n_conf) == len(sizes) and n % 64 != 0 and n > CLM_POSES
    # what the issue's table says of the rule as it stands
    for sizes, tile in (((33, 37), 12), ((35, 49), 16), ((33, 33), 18), ((24, 24, 24), 12), ((25, 24, 23), 16), ((36, 36, 36), 18),
                        ((1, 1, 1), 12), ((70, 70, 60), 18)):
        assert chosen_tile(sizes) == tile, sizes
    for name, a_sizes in TILE_EDGES.items():
        sizes, tile = RANDOM_CASES[name][0], RANDOM_CASES[name][5]
        for a in a_sizes:
            assert a in sizes and a in (2 * tile - 1, 2 * tile, 2 * tile + 1), (name, a)
    assert {a - 2 * RANDOM_CASES[k][5] for k, v in TILE_EDGES.items() for a in v} == {-1, 0, 1}
    assert [RANDOM_CASES[k][0].index(1) for k in ("one-atom-first", "one-atom-middle", "one-atom-last")] == [0, 1, 2]
    assert any(len(set(c[1])) > 1 for c in RANDOM_CASES.values())
    assert {63, 64, 65, CLM_POSES - 1, CLM_POSES, CLM_POSES + 1, 2 * CLM_POSES + 1} <= set(POSE_COUNTS) and max(POSE_COUNTS) >= 3000


@pytest.mark.parametrize("name", list(RANDOM_CASES))
def test_random_ensembles_clash_in_a_fair_share_and_keep_their_distance_from_the_threshold(oracle, name):
    case = random_case(name)
    mask, poses = clash_reference(oracle, name, case)
    share = 1.0 - mask.mean()
    assert 0.2 <= share <= 0.8, (name, share)
    assert oracle.clash_margin(poses, case[4], THRESH) > 1e-9
    if name.startswith("counts-"):
        for n in POSE_COUNTS:
            assert 0 < mask[:n].sum() < n, (name, n)


@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_ensembles_clash_in_the_pairs_they_were_built_for(oracle, name):
    case, cls = pair_case(name)
    mask, poses = clash_reference(oracle, "pairs-" + name, case)
    table = pair_table(oracle, poses)
    want = np.zeros((len(cls), 3), dtype=bool)
    for c in range(3):
        want[cls == c, c] = True
    want[cls == ALL] = True
    assert np.array_equal(table, want)
    assert np.array_equal(mask, cls == NONE)
    assert oracle.clash_margin(poses, case[4], THRESH) > 1e-9
    if name == "mixed":
        assert len(cls) > 3 * CLM_POSES
        assert all((cls == c).mean() >= 0.1 for c in range(5)), np.bincount(cls) / len(cls)
        goes_on = ~table[:, 0]                                        # what the first pair leaves of every block of the workgroups
        left = [int(goes_on[b:b + CLM_POSES].sum()) for b in range(0, len(cls), CLM_POSES)]
        assert 0 in left and any(x % 64 for x in left) and max(left) > 64, left
    elif name == "all-in-first-pair":
        assert table[:, 0].all()
    else:
        assert not table.any()


@pytest.mark.parametrize("name", list(BAND_CASES))
def test_band_poses_sit_on_the_threshold(oracle, name):
    case = band_case(name)
    (fa, fb), fc, into = BAND_CASES[name]
    mask, poses = clash_reference(oracle, "band-" + name, case)
    assert oracle.clash_margin(poses, case[4], THRESH) < 1e-9           # (this set is MEANT to sit on the threshold)
    off = np.concatenate([[0], np.cumsum(BAND_SIZES)])
    d = np.linalg.norm(poses[:, off[fa]] - poses[:, off[fb]], axis=1)
    eps = np.repeat(BAND_EPS, BAND_REPS)
    assert np.abs(d - (1.5 + eps)).max() < 5e-13
    # every other distance of the pair, and of the pairs meant to be far: more than 5 A
    for a, b in ((fa, fb), (fa, fc), (fb, fc)):
        D = np.linalg.norm(poses[:, off[a]:off[a + 1], None] - poses[:, None, off[b]:off[b + 1]], axis=3)
        if (a, b) == (fa, fb):
            D[:, 0, 0] = np.inf
        if into is not None and (a, b) == (fa, fc):
            assert (D.min(axis=(1, 2)) < 1.2).all()                    # a clear clash
        else:
            assert D.min() > 5.0, (name, a, b, float(D.min()))
    tail = mask[BAND_SKIP:]
    if into is None:
        assert np.array_equal(tail, eps[BAND_SKIP:] > 0) and 0 < tail.sum() < len(tail)
    else:
        assert not mask.any()


def test_non_finite_poses_have_verdicts_of_both_kinds(oracle):
    case = nonfinite_case()
    mask, poses = clash_reference(oracle, "non-finite", case)
    assert np.isnan(poses[5]).any() and np.isinf(poses[77]).all() and not np.isfinite(poses[300]).all() and np.isnan(poses[650]).any()
    assert mask[77]                                                    # inf - inf: no distance is below anything
    assert 0 < mask.sum() < len(mask)


# ------------------------------------------------------------------------------------------------------------- A: on the GPU
@pytest.fixture(scope="module")
def eng():
    import tscode_amd
    return tscode_amd.get_engine(0)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    return t


def _filled(shape, value, dtype):
    """A device tensor of one value, complete before the engine's own stream can touch it."""
    import torch
    t = torch.full(shape, value, dtype=dtype, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    return t


CLASH_OPTIONS = ({}, {"clash_lanes": 0}, {"clash_fp32": 0})            # k_clash_lanes_multi; k_clash, packed float32; k_clash, float64


def clash_masks(eng, case, lo=0, hi=None):
    """The verdict bytes of poses [lo, hi) under each of CLASH_OPTIONS, every byte asserted to have been written."""
    import torch

    from tscode_amd.engine import FragmentSet
    frags, ci, rot, pos, _ = case
    hi = len(ci) if hi is None else hi
    fs = FragmentSet(frags)
    d_frags, d_ci, d_rot, d_pos = _dev(fs.flat), _dev(ci[lo:hi]), _dev(rot[lo:hi]), _dev(pos[lo:hi])
    out = []
    for opts in CLASH_OPTIONS:
        d_mask = _filled((hi - lo + 64,), 0xAA, torch.uint8)
        with eng.options(**opts):
            eng.embed_clash_mask_dev(fs, d_frags, d_ci, d_rot, d_pos, hi - lo, THRESH, 0, d_mask)
            eng.synchronize()
        got = d_mask.cpu().numpy()
        assert (got[hi - lo:] == 0xAA).all(), (opts, "bytes behind the last pose were written")
        assert set(np.unique(got[:hi - lo])) <= {0, 1}, (opts, np.unique(got[:hi - lo]))
        out.append(got[:hi - lo].astype(bool))
    return out


def assert_masks(got_all, ref, what, lo=0):
    for opts, got in zip(CLASH_OPTIONS, got_all):
        wrong = np.flatnonzero(got != ref)
        assert len(wrong) == 0, f"{what}, options {opts}: {len(wrong)} verdicts differ from the oracle's, first at pose {lo + int(wrong[0])}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in RANDOM_CASES if not k.startswith("counts-")])
def test_fused_clash_any_fragments_random(eng, oracle, name):
    case = random_case(name)
    ref, _ = clash_reference(oracle, name, case)
    assert_masks(clash_masks(eng, case), ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1,) + POSE_COUNTS)
@pytest.mark.parametrize("name", ["counts-three", "counts-two"])
def test_fused_clash_pose_counts_around_the_block_and_the_wavefront(eng, oracle, name, n):
    case = random_case(name)
    ref, _ = clash_reference(oracle, name, case)
    if n == 1:                                                          # a single pose of either verdict
        for s in (int(np.flatnonzero(ref)[0]), int(np.flatnonzero(~ref)[0])):
            assert_masks(clash_masks(eng, case, s, s + 1), ref[s:s + 1], f"{name}, pose {s} alone", s)
    else:
        assert_masks(clash_masks(eng, case, 0, n), ref[:n], f"{name}, {n} poses")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIR_CASES)
def test_fused_clash_finds_the_clash_in_whichever_pair_it_is(eng, oracle, name):
    case, cls = pair_case(name)
    ref, _ = clash_reference(oracle, "pairs-" + name, case)
    got_all = clash_masks(eng, case)
    for opts, got in zip(CLASH_OPTIONS, got_all):
        for c, label in enumerate(("only (m2, m1)", "only (m3, m2)", "only (m1, m3)", "none", "all three")):
            sel = cls == c
            assert np.array_equal(got[sel], ref[sel]), (name, opts, label, int((got[sel] != ref[sel]).sum()), int(sel.sum()))
    assert_masks(got_all, ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BAND_CASES))
def test_fused_clash_inside_the_band_of_any_pair(eng, oracle, name):
    case = band_case(name)
    ref, _ = clash_reference(oracle, "band-" + name, case)
    got_all = clash_masks(eng, case)
    assert_masks([g[BAND_SKIP:] for g in got_all], ref[BAND_SKIP:], name, BAND_SKIP)


@pytest.mark.gpu
def test_fused_clash_non_finite_inputs(eng, oracle):
    case = nonfinite_case()
    ref, _ = clash_reference(oracle, "non-finite", case)
    assert_masks(clash_masks(eng, case), ref, "non-finite")


# --------------------------------------------------------------------------------------------- B1: ordered compaction and gathers
GATHER_CAP_WORDS = 1 << 20                       # launch_gather_rows: at most 4096 workgroups of 256 threads, one output word each per trip
MANY_BLOCKS = SCAN_TILE * 257 + 5                # more than 256 scan blocks: the block-offset loop of scan_write_block takes a second trip
ROW_COUNTS = (1, 7, 8, 9, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, MANY_BLOCKS)
MASK_KINDS = ("zero", "one", "first", "last", "1%", "50%", "99%")
SENTINEL = 0xA5


def row_mask(kind, n, rng):
    """u8[n]: which rows are kept, the kept ones marked with 1, 2, 128 and 255 in turn."""
    if kind == "zero":
        on = np.zeros(n, dtype=bool)
    elif kind == "one":
        on = np.ones(n, dtype=bool)
    elif kind in ("first", "last"):
        on = np.zeros(n, dtype=bool)
        on[0 if kind == "first" else n - 1] = True
    else:
        on = rng.random(n) < float(kind[:-1]) / 100.0
    values = np.array([1, 2, 128, 255], dtype=np.uint8)[np.arange(n) % 4]
    return np.where(on, values, 0).astype(np.uint8)


def compact_and_check(eng, src, mask, row_bytes, what):
    import torch
    n = len(mask)
    want = src[mask != 0]
    d_dst = _filled((n + 1, row_bytes), SENTINEL, torch.uint8)
    kept = eng.compact_rows_dev(_dev(src), _dev(mask), n, row_bytes, d_dst)
    eng.synchronize()
    got = d_dst.cpu().numpy()
    assert kept == len(want), (what, kept, len(want))
    assert np.array_equal(got[:kept], want), what
    assert (got[kept:] == SENTINEL).all(), (what, "rows behind the kept ones were written")


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_compact_rows_is_numpy_boolean_indexing(eng, n):
    rng = _rng(f"compact-{n}")
    for row_bytes in (8,) if n == MANY_BLOCKS else (8, 24, 1200):
        src = rng.integers(0, 256, size=(n, row_bytes), dtype=np.uint8)          # (any bit pattern, NaNs among them: the copy is by words)
        for kind in MASK_KINDS:
            compact_and_check(eng, src, row_mask(kind, n, rng), row_bytes, (n, row_bytes, kind))


@pytest.mark.gpu
def test_compact_rows_with_more_words_than_the_gather_grid_has_threads(eng):
    rng = _rng("compact-cap")
    for n, row_bytes, kind in ((9001, 1200, "99%"), (MANY_BLOCKS, 24, "one")):
        mask = row_mask(kind, n, rng)
        assert int((mask != 0).sum()) * (row_bytes // 8) > GATHER_CAP_WORDS
        compact_and_check(eng, rng.integers(0, 256, size=(n, row_bytes), dtype=np.uint8), mask, row_bytes, (n, row_bytes, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_gather_heavy_is_numpy_fancy_indexing(eng, n):
    import torch
    rng = _rng(f"gather-{n}")
    big = n == MANY_BLOCKS                                             # (two atoms and two masks there: the scan is what that size is for)
    n_atoms = 2 if big else 11
    coords = rng.normal(size=(n, n_atoms, 3))
    d_coords = _dev(coords)
    for heavy_idx in ([1], [0, 1]) if big else ([4], list(range(n_atoms)), [0, 3, 4, 9, 10], [10, 2, 7]):
        for kind in (None, "50%") if big else (None,) + MASK_KINDS:
            mask = None if kind is None else row_mask(kind, n, rng)
            want = (coords if mask is None else coords[mask != 0])[:, heavy_idx]
            d_out = _filled((n + 1, len(heavy_idx), 3), -777.25, torch.float64)
            kept = eng.gather_heavy_dev(d_coords, None if mask is None else _dev(mask), n, n_atoms, heavy_idx, d_out)
            eng.synchronize()
            got = d_out.cpu().numpy()
            assert kept == len(want), (n, heavy_idx, kind)
            assert np.array_equal(got[:kept].view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (n, heavy_idx, kind)
            assert (got[kept:] == -777.25).all(), (n, heavy_idx, kind)


@pytest.mark.gpu
def test_compaction_refuses_what_it_cannot_take_and_writes_nothing(eng):
    import torch

    from tscode_amd._lib import TscodeHipError
    n, n_atoms = 100, 6
    rng = _rng("refusals")
    d_src = _dev(rng.normal(size=(n, n_atoms, 3)))
    d_mask = _dev(np.ones(n, dtype=np.uint8))
    d_dst = _filled((n, n_atoms, 3), -777.25, torch.float64)
    for row_bytes in (12, 7, 0, -8):
        with pytest.raises((TscodeHipError, ValueError)):
            eng.compact_rows_dev(d_src, d_mask, n, row_bytes, d_dst)
    for heavy_idx in ([0, 6], [-1], [0, 1, 2, 3, 4, 5, 5], []):
        with pytest.raises((TscodeHipError, ValueError)):
            eng.gather_heavy_dev(d_src, d_mask, n, n_atoms, heavy_idx, d_dst)
    eng.synchronize()
    assert bool((d_dst == -777.25).all())
    # ... and the context goes on working
    kept = eng.compact_rows_dev(d_src, d_mask, n, n_atoms * 24, d_dst)
    eng.synchronize()
    assert kept == n and torch.equal(d_dst, d_src)


# ------------------------------------------------------------------------------------------ B2: the embed of the selected poses
EMBED_SHAPES = {2: ((9, 14), (3, 2)), 3: ((7, 5, 9), (2, 3, 2))}     # fragments: (atoms, conformers)
EMBED_POSES = 1100
SELECTED = (0, 1, TR_POSES - 1, TR_POSES, TR_POSES + 1, 1003)
FILL = -777.25


def heavy_patterns(sizes):
    """Strictly increasing atom lists: all atoms, one atom, the atoms of fragment 1 only, an irregular subset that spans the fragments."""
    n, off = sum(sizes), np.concatenate([[0], np.cumsum(sizes)])
    return {"all": list(range(n)), "one": [n // 2], "one-fragment": list(range(off[1], off[2])),
            "irregular": [a for a in range(n) if (a * 7 + a // 4) % 5 in (0, 2, 3)]}


def embed_case(nm, k, offset=0.0):
    """EMBED_POSES poses of nm compact fragments of which exactly k, drawn at random, pass the clash check: their fragments lie 40 A
    apart, fragment 1 of every other pose sits on its fragment 0.  The same fragments, conformer picks and rotations for every k."""
    key = f"embed-{nm}-{k}-{offset}"
    if key not in _cases:
        sizes, n_conf = EMBED_SHAPES[nm]
        rng, n = _rng(f"embed-{nm}"), EMBED_POSES
        frags = [rng.normal(size=(c, a, 3)) * 0.7 for a, c in zip(sizes, n_conf)]
        ci = np.stack([rng.integers(0, c, size=n) for c in n_conf], axis=1).astype(np.int32)
        rot = _rotations(rng, (n, nm))
        pos = 40.0 * np.eye(3)[None, :nm] + rng.normal(size=(n, nm, 3))
        near = pos[:, 0] + rng.normal(size=(n, 3)) * 0.3
        passing = np.zeros(n, dtype=bool)
        passing[_rng(key).choice(n, size=k, replace=False)] = True
        pos[~passing, 1] = near[~passing]
        _cases[key] = ((frags, ci, np.ascontiguousarray(rot), np.ascontiguousarray(pos + offset), np.array(sizes, dtype=np.int32)), passing)
    return _cases[key]


def embed_bound(case):
    """What a correctly rounded evaluation of R x + t in any order, fused or not, may differ by from another, per component: three
    products and three sums, 4 * 2^-53 (|R| |x| + |t|).  f64[n, atoms, 3]."""
    frags, ci, rot, pos, _ = case
    parts = []
    for m, f in enumerate(frags):
        x = np.abs(f[ci[:, m]])
        parts.append(np.einsum("pij,paj->pai", np.abs(rot[:, m]), x) + np.abs(pos[:, m])[:, None, :])
    return 4.0 * U53 * np.concatenate(parts, axis=1)


@pytest.mark.parametrize("nm,k,offset", [(nm, k, 0.0) for nm in (2, 3) for k in SELECTED] + [(3, TR_POSES + 1, 1.0e5)])
def test_embed_ensembles_pass_the_clash_check_where_they_were_built_to(oracle, nm, k, offset):
    case, passing = embed_case(nm, k, offset)
    mask, poses = clash_reference(oracle, f"embed-{nm}-{k}-{offset}", case)
    assert np.array_equal(mask, passing) and int(mask.sum()) == k
    assert oracle.clash_margin(poses, case[4], THRESH) > 1e-9
    bound = embed_bound(case)
    assert bound.shape == poses.shape and (bound.max() < 1e-12 if offset == 0.0 else 4e-11 < bound.max() < 1e-10)
    for name, idx in heavy_patterns(EMBED_SHAPES[nm][0]).items():
        assert all(b > a for a, b in zip(idx, idx[1:])) and 0 <= idx[0] and idx[-1] < sum(EMBED_SHAPES[nm][0]), name
    irregular = np.array(heavy_patterns(EMBED_SHAPES[nm][0])["irregular"])
    assert len(set(np.searchsorted(np.cumsum(EMBED_SHAPES[nm][0]), irregular, side="right"))) == nm and (np.diff(irregular) > 1).any()


class EmbedRun:
    """The device copies of a case and one call of either entry point, outputs pre-filled with FILL."""

    def __init__(self, eng, case):
        from tscode_amd.engine import FragmentSet
        frags, ci, rot, pos, _ = case
        self.eng, self.fs, self.n, self.n_atoms = eng, FragmentSet(frags), len(ci), sum(f.shape[1] for f in frags)
        self.dev = (_dev(self.fs.flat), _dev(ci), _dev(rot), _dev(pos))

    def _out(self, heavy_idx, structures, heavy):
        import torch
        return (_filled((self.n + 1, self.n_atoms, 3), FILL, torch.float64) if structures else None,
                _filled((self.n + 1, len(heavy_idx), 3), FILL, torch.float64) if heavy else None)

    @staticmethod
    def _host(t):
        return None if t is None else t.cpu().numpy()

    def clash_compact(self, heavy_idx, structures=True):
        import torch
        d_s, d_h = self._out(heavy_idx, structures, True)
        d_mask = _filled((self.n,), 0xAA, torch.uint8)
        count = self.eng.embed_clash_compact_dev(self.fs, *self.dev, self.n, heavy_idx, THRESH, 0, d_mask, d_s, d_h)
        self.eng.synchronize()
        return count, d_mask.cpu().numpy(), self._host(d_s), self._host(d_h)

    def fork(self, heavy_idx):
        self.eng.basis_from_poses_dev(self.fs, *self.dev, self.n, heavy_idx)

    def masked(self, mask, heavy_idx, structures=True, heavy=True):
        d_s, d_h = self._out(heavy_idx, structures, heavy)
        count = self.eng.embed_masked_dev(self.fs, *self.dev, self.n, _dev(mask), heavy_idx, d_s, d_h)
        self.eng.synchronize()
        return count, self._host(d_s), self._host(d_h)


def check_embedded(what, count, structures, heavy, heavy_idx, ref_rows, bound_rows):
    """structures / heavy (host copies, either may be None) of one call against the oracle's rows: within the bound, heavy bit-identical to
    the heavy atoms of structures, nothing written from row `count` on."""
    assert count == len(ref_rows), (what, count, len(ref_rows))
    if structures is not None:
        assert (np.abs(structures[:count] - ref_rows) <= bound_rows).all(), (what, float(np.abs(structures[:count] - ref_rows).max()))
        assert (structures[count:] == FILL).all(), (what, "structures written behind the selected rows")
    if heavy is not None:
        assert (np.abs(heavy[:count] - ref_rows[:, heavy_idx]) <= bound_rows[:, heavy_idx]).all(), what
        assert (heavy[count:] == FILL).all(), (what, "heavy atoms written behind the selected rows")
    if structures is not None and heavy is not None:
        assert np.array_equal(heavy[:count].view(np.uint64), np.ascontiguousarray(structures[:count][:, heavy_idx]).view(np.uint64)), what


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("nm,k,offset", [(nm, k, 0.0) for nm in (2, 3) for k in SELECTED] + [(3, TR_POSES + 1, 1.0e5)])
def test_clash_compact_and_masked_embed_write_the_passing_poses_in_order(eng, oracle, nm, k, offset):
    """embed_clash_compact_dev (k_transform), then embed_masked_dev with the mask it wrote (its non-zero bytes re-marked 1, 2, 128, 255):
      heavy atoms only     the basis the first call forked is pending: k_transform_describe;
      both, structures     that basis is used up: k_transform;
      both                 behind a new fork: k_transform_describe;
      both                 behind a new fork, fuse_descriptors = 0: k_transform.
    Every output lies within the bound of the oracle's; the outputs of ONE kernel, whatever the entry point, are bit-identical.  (Not so
    between the two kernels: both inline embed_atom_staged, but the compiler contracts R x + t into a product and two fused steps in
    a different order of the three terms in k_transform_describe's first component -- last-bit differences, inside the bound.)"""
    case, passing = embed_case(nm, k, offset)
    ref_mask, poses = clash_reference(oracle, f"embed-{nm}-{k}-{offset}", case)
    assert np.array_equal(ref_mask, passing)
    rows, bound = poses[ref_mask], embed_bound(case)[ref_mask]
    run = EmbedRun(eng, case)
    for name, heavy_idx in heavy_patterns(EMBED_SHAPES[nm][0]).items():
        what = (nm, k, offset, name)
        count, mask, s0, h0 = run.clash_compact(heavy_idx)
        assert set(np.unique(mask)) <= {0, 1} and np.array_equal(mask.astype(bool), ref_mask), what
        assert count == int(ref_mask.sum()) == k
        check_embedded(what + ("clash_compact",), count, s0, h0, heavy_idx, rows, bound)
        marked = np.where(mask != 0, np.array([1, 2, 128, 255], dtype=np.uint8)[np.arange(len(mask)) % 4], 0).astype(np.uint8)
        c1, _, h1 = run.masked(marked, heavy_idx, structures=False)
        c2, s2, h2 = run.masked(marked, heavy_idx)
        c3, s3, _ = run.masked(marked, heavy_idx, heavy=False)
        run.fork(heavy_idx)
        c4, s4, h4 = run.masked(marked, heavy_idx)
        with eng.options(fuse_descriptors=0):
            run.fork(heavy_idx)
            c5, s5, h5 = run.masked(marked, heavy_idx)
        check_embedded(what + ("masked, heavy only, fused",), c1, None, h1, heavy_idx, rows, bound)
        check_embedded(what + ("masked, both",), c2, s2, h2, heavy_idx, rows, bound)
        check_embedded(what + ("masked, structures only",), c3, s3, None, heavy_idx, rows, bound)
        check_embedded(what + ("masked, both, fused",), c4, s4, h4, heavy_idx, rows, bound)
        check_embedded(what + ("masked, both, not fused",), c5, s5, h5, heavy_idx, rows, bound)
        for label, got, want in (("both: heavy", h2, h0), ("both: structures", s2, s0), ("structures only", s3, s0), ("not fused: heavy", h5, h0),
                                 ("not fused: structures", s5, s0), ("fused, heavy only against both", h1, h4)):
            assert same_bits(got, want), what + (label,)


@pytest.mark.gpu
@pytest.mark.parametrize("nm", [2, 3])
def test_masked_embed_takes_any_mask(eng, oracle, nm):
    """Masks that are no clash verdicts: the selected counts around TR_POSES anywhere in the list, the first and the last pose, all, none."""
    case, _ = embed_case(nm, SELECTED[-1])
    _, poses = clash_reference(oracle, f"embed-{nm}-{SELECTED[-1]}-0.0", case)
    bound = embed_bound(case)
    run, rng = EmbedRun(eng, case), _rng(f"any-mask-{nm}")
    heavy_idx = heavy_patterns(EMBED_SHAPES[nm][0])["irregular"]
    masks = {f"{k} anywhere": np.isin(np.arange(EMBED_POSES), rng.choice(EMBED_POSES, size=k, replace=False)) for k in SELECTED + (EMBED_POSES,)}
    masks["first"], masks["last"] = np.arange(EMBED_POSES) == 0, np.arange(EMBED_POSES) == EMBED_POSES - 1
    for name, on in masks.items():
        marked = np.where(on, np.array([255, 1, 128, 2], dtype=np.uint8)[np.arange(len(on)) % 4], 0).astype(np.uint8)
        count, s, h = run.masked(marked, heavy_idx)
        check_embedded((nm, name), count, s, h, heavy_idx, poses[on], bound[on])


# ------------------------------------------------------------------------------------------------ B3: the context's caches
CACHE_PATTERNS = {"P1": [0, 2, 4, 6, 8, 10], "P2": [1, 2, 5, 6, 9, 11]}          # two heavy-atom patterns of one length
# (fragments: the two-fragment set has 23 atoms, the three-fragment set 21; poses; pattern; entry point).  Consecutive calls change the
# pattern at equal length, the fragment set under one pattern, and the pose count -- 3000: every pose is a sample of the basis; 4096: the
# last count with stride 1; 5000, 8192, 12289: strides 1, 2, 3 of 4096 samples
CACHE_CALLS = ((3, 3000, "P1", "compact"), (3, 3000, "P2", "compact"), (2, 3000, "P2", "masked"), (3, 4096, "P2", "pipeline"),
               (3, 5000, "P1", "pipeline"), (2, 8192, "P1", "compact"), (3, 12289, "P1", "pipeline"), (3, 3000, "P1", "pipeline"),
               (2, 12289, "P2", "masked"), (2, 5000, "P2", "pipeline"), (3, 8192, "P1", "masked"))


def cache_case(nm, n):
    """n poses of the fragments of embed_case(nm): two in three have their fragments apart, and every pose has four near copies."""
    key = f"cache-{nm}-{n}"
    if key not in _cases:
        frags = embed_case(nm, 0)[0][0]
        rng = _rng(key)
        parents = -(-n // 5)
        ci = np.stack([rng.integers(0, f.shape[0], size=parents) for f in frags], axis=1).astype(np.int32)
        q = rng.normal(size=(parents, nm, 4))
        pos = 6.0 * np.eye(3)[None, :nm] + rng.normal(size=(parents, nm, 3))
        clash = rng.random(parents) < 1.0 / 3.0
        pos[clash, 1] = pos[clash, 0]
        who = rng.permutation(np.repeat(np.arange(parents), 5)[:n])
        from tscode_amd.synthetic import quat_to_mat
        rot = quat_to_mat(q[who] + rng.normal(size=(n, nm, 4)) * 0.01)
        _cases[key] = (frags, np.ascontiguousarray(ci[who]), np.ascontiguousarray(rot), np.ascontiguousarray(pos[who] + rng.normal(size=(n, nm, 3)) * 0.02),
                       np.array([f.shape[1] for f in frags], dtype=np.int32))
    return _cases[key]


def cache_call(e, nm, n, pattern, entry):
    """One call of CACHE_CALLS on the engine e: everything it returned, as host arrays."""
    import torch
    case, heavy_idx = cache_case(nm, n), CACHE_PATTERNS[pattern]
    run = EmbedRun(e, case)
    if entry == "compact":
        count, mask, s, h = run.clash_compact(heavy_idx)
        return [np.array([count]), mask, s[:count], h[:count]]
    if entry == "masked":
        mask = (np.arange(n) % 3 != 1).astype(np.uint8)
        run.fork(heavy_idx)
        count, s, h = run.masked(mask, heavy_idx)
        return [np.array([count]), s[:count], h[:count]]
    d_clash, d_keep = _filled((n,), 0xAA, torch.uint8), _filled((n,), 0xAA, torch.uint8)
    d_s = _filled((n, run.n_atoms, 3), FILL, torch.float64)
    res = e.pipeline_dev(run.fs, *run.dev, n, heavy_idx, THRESH, 0, THR, 0, d_clash, d_s, d_keep)
    e.synchronize()
    return [np.array([res["n_pass"], res["n_keep"]]), d_clash.cpu().numpy(), d_s.cpu().numpy()[:res["n_pass"]], d_keep.cpu().numpy()[:res["n_pass"]],
            np.array(per_pass(res["stats"]))]


@pytest.mark.gpu
def test_tables_cached_on_the_context_follow_their_inputs(oracle):
    """heavy_slot_table and basis_sample_table (csrc/pipeline.hip) keep their last upload: every call of a sequence on ONE context returns
    what the same call returns on a context that has seen nothing.  (A stale slot table puts heavy atoms in the wrong place or leaves
    them out; a stale sample table reads poses that are not there -- or a basis that differs, which the verdicts must not notice.)"""
    from tscode_amd.engine import Engine
    shared = Engine(0)
    try:
        for i, call in enumerate(CACHE_CALLS):
            got = cache_call(shared, *call)
            fresh = Engine(0)
            try:
                want = cache_call(fresh, *call)
            finally:
                fresh.close()
            assert len(got) == len(want)
            for j, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and np.array_equal(a, b), (i, call, j)
            if call[3] == "pipeline":                                   # ... and what both return is right
                nm, n, pattern, _ = call
                case = cache_case(nm, n)
                ref_mask, poses = clash_reference(oracle, f"cache-{nm}-{n}", case)
                assert np.array_equal(got[1].astype(bool), ref_mask) and got[0][0] == ref_mask.sum() and 0 < ref_mask.sum() < n
                ref = oracle.prune_heavy(np.ascontiguousarray(poses[ref_mask][:, CACHE_PATTERNS[pattern]]), THR, mode=0, row_parallel=True)
                assert np.array_equal(got[3].astype(bool), ref["mask"]) and 0 < ref["mask"].sum() < 0.95 * ref_mask.sum(), (i, call)
                assert [tuple(r) for r in got[4]] == per_pass(ref["stats"])
    finally:
        shared.close()


# ------------------------------------------------------------------------------- C: the fused descriptor route at the screens' limit
FUSED_CLASH_THRESH = 0.05                          # no two atoms of a breathing structure come that close: every pose passes


def fused_case(name):
    """A structure-level case of test_screen_limit as a pose list that embeds EXACTLY: structure s is conformer s of two fragments (the first
    ceil(h / 2) atoms and the rest), rotations the identity, translations zero -- 1 x + 0 y + 0 z + 0 in any order, fused or not."""
    key = "fused-" + name
    if key not in _cases:
        heavy = struct_case(name)[0]
        n, h = heavy.shape[:2]
        cut = (h + 1) // 2
        frags = [np.ascontiguousarray(heavy[:, :cut]), np.ascontiguousarray(heavy[:, cut:])]
        ci = np.ascontiguousarray(np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32))
        rot = np.ascontiguousarray(np.broadcast_to(np.eye(3), (n, 2, 3, 3)))
        _cases[key] = (frags, ci, rot, np.zeros((n, 2, 3)), np.array([cut, h - cut], dtype=np.int32))
    return _cases[key]


@pytest.mark.parametrize("name", [c for c in STRUCT_CASES if "-pca" not in c])
def test_breathing_structures_embed_exactly_and_never_clash(oracle, name):
    heavy = struct_case(name)[0]
    case = fused_case(name)
    poses = oracle.transform_batch(*case[:4])
    assert poses.shape == heavy.shape and np.array_equal(poses.view(np.uint64), heavy.view(np.uint64))
    assert oracle.compenetration_mask(poses, case[4], FUSED_CLASH_THRESH, 0).all()
    assert oracle.clash_margin(poses, case[4], FUSED_CLASH_THRESH) > 1e-3


# name: options of the run beside the case's own
PIPELINE_OPTIONS = {
    "default": {},
    "descriptors-by-k_descriptors": dict(fuse_descriptors=0),
    "basis-from-the-survivors": dict(early_basis=0),
    "principal-axes": dict(pca_min_n=0),
    "mm16": dict(MM16, prune_algo=2),
    "mm64-culled": dict(MM64_CULLED, prune_algo=2),
    "mm16-f32-stage1": dict(MM16, prune_algo=2, stage1_f32=2),              # the pair kernels read the float32 copy the fused kernel wrote
    "mm64-culled-f32-stage1": dict(MM64_CULLED, prune_algo=2, stage1_f32=2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(STRUCT_CASES))
def test_pipeline_keeps_every_pair_placed_at_the_limit(eng, oracle, name, mode):
    import torch

    from tscode_amd.engine import FragmentSet
    heavy, _, inside = struct_case(name)
    frags, ci, rot, pos, _ = fused_case(name)
    ref = struct_reference(oracle, name, mode)
    n, h = heavy.shape[:2]
    fs = FragmentSet(frags)
    dev = (_dev(fs.flat), _dev(ci), _dev(rot), _dev(pos))
    for label, opts in PIPELINE_OPTIONS.items():
        d_clash, d_keep = _filled((n,), 0xAA, torch.uint8), _filled((n,), 0xAA, torch.uint8)
        d_s = _filled((n, h, 3), FILL, torch.float64)
        with eng.options(**dict(opts, **STRUCT_CASES[name][4])):
            res = eng.pipeline_dev(fs, *dev, n, np.arange(h), FUSED_CLASH_THRESH, 0, THR, mode, d_clash, d_s, d_keep)
            eng.synchronize()
        what = f"{name}, mode {mode}, {label}"
        assert res["n_pass"] == n and bool((d_clash == 1).all()), what
        assert np.array_equal(d_s.cpu().numpy().view(np.uint64), heavy.view(np.uint64)), what
        keep = d_keep.cpu().numpy()
        assert set(np.unique(keep)) <= {0, 1}, what
        keep = keep.astype(bool)
        extra, missing = int((keep & ~ref["mask"]).sum()), int((~keep & ref["mask"]).sum())
        assert np.array_equal(keep, ref["mask"]), f"{what}: {extra} survivors the oracle removes, {missing} removed that it keeps"
        assert res["n_keep"] == int(ref["mask"].sum()), what
        assert per_pass(res["stats"]) == per_pass(ref["stats"]), what
        if mode == 1 or name not in CACHE_SKIPS:
            assert res["n_keep"] == n - int(inside.sum()), what


def foreign_case(h, n=700):
    """An unrelated random ensemble of two one-conformer fragments with the atom counts fused_case gives h heavy atoms."""
    key = f"foreign-{h}"
    if key not in _cases:
        rng = _rng(key)
        cut = (h + 1) // 2
        frags = [rng.normal(size=(1, a, 3)) * 2.0 for a in (cut, h - cut)]
        _cases[key] = (frags, np.zeros((n, 2), dtype=np.int32), np.ascontiguousarray(_rotations(rng, (n, 2))), rng.normal(size=(n, 2, 3)) * 4.0,
                       np.array([cut, h - cut], dtype=np.int32))
    return _cases[key]


def run_stepper(st, n):
    import torch
    while st.next_pass():
        st.pass_local(0, 1)
        st.pass_finish()
    d_mask = _filled((n,), 0xAA, torch.uint8)
    st.copy_mask(d_mask)
    st.e.synchronize()
    stats = st.stats()
    st.close()
    return d_mask.cpu().numpy(), stats


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(STRUCT_CASES))
def test_multi_rank_front_sequence_keeps_every_pair_placed_at_the_limit(oracle, name, mode):
    """basis_from_poses_dev -> embed_masked_dev(all poses, heavy) -> tsc_prune_create over that heavy array (prune_stepper, as
    DevicePipeline's multi-rank backend does): the run takes the descriptors k_transform_describe wrote -- shown by the context refusing
    to regrow their buffers while the run lives --, once with the basis of the ensemble itself, once with a foreign one."""
    import torch

    from tscode_amd._lib import TscodeHipError
    from tscode_amd.engine import Engine, FragmentSet
    heavy, _, inside = struct_case(name)
    frags, ci, rot, pos, _ = fused_case(name)
    ref = struct_reference(oracle, name, mode)
    n, h = heavy.shape[:2]
    heavy_idx = np.arange(h)
    more = n + 500                                                      # the same fragments, more poses: the descriptor buffers would have to grow
    ci_more = np.ascontiguousarray(ci[np.arange(more) % n])
    rot_more, pos_more = np.ascontiguousarray(np.broadcast_to(np.eye(3), (more, 2, 3, 3))), np.zeros((more, 2, 3))
    f_frags, f_ci, f_rot, f_pos, _ = foreign_case(h)
    e = Engine(0)                                                        # (a context of its own: nothing has sized its buffers yet)
    try:
        fs, f_fs = FragmentSet(frags), FragmentSet(f_frags)
        d_frags, d_ci, d_rot, d_pos = _dev(fs.flat), _dev(ci), _dev(rot), _dev(pos)
        d_more = (_dev(ci_more), _dev(rot_more), _dev(pos_more))
        f_dev = (_dev(f_fs.flat), _dev(f_ci), _dev(f_rot), _dev(f_pos))
        d_ones, d_ones_more = _filled((n,), 1, torch.uint8), _filled((more,), 1, torch.uint8)
        d_heavy_more = _filled((more, h, 3), FILL, torch.float64)
        with e.options(**STRUCT_CASES[name][4]):
            for basis in ("own", "foreign"):
                what = f"{name}, mode {mode}, {basis} basis"
                d_heavy = _filled((n, h, 3), FILL, torch.float64)
                if basis == "own":
                    e.basis_from_poses_dev(fs, d_frags, d_ci, d_rot, d_pos, n, heavy_idx)
                else:
                    e.basis_from_poses_dev(f_fs, *f_dev, len(f_ci), heavy_idx)
                assert e.embed_masked_dev(fs, d_frags, d_ci, d_rot, d_pos, n, d_ones, heavy_idx, None, d_heavy) == n
                e.synchronize()
                assert np.array_equal(d_heavy.cpu().numpy().view(np.uint64), heavy.view(np.uint64)), what
                st = e.prune_stepper(d_heavy, n, h, THR, mode)
                if basis == "own":
                    e.basis_from_poses_dev(fs, d_frags, *d_more, more, heavy_idx)
                    with pytest.raises(TscodeHipError) as err:
                        e.embed_masked_dev(fs, d_frags, *d_more, more, d_ones_more, heavy_idx, None, d_heavy_more)
                    assert "still read" in str(err.value), what
                keep, stats = run_stepper(st, n)
                assert set(np.unique(keep)) <= {0, 1}, what
                keep = keep.astype(bool)
                extra, missing = int((keep & ~ref["mask"]).sum()), int((~keep & ref["mask"]).sum())
                assert np.array_equal(keep, ref["mask"]), f"{what}: {extra} survivors the oracle removes, {missing} removed that it keeps"
                assert per_pass(stats) == per_pass(ref["stats"]), what
                if mode == 1 or name not in CACHE_SKIPS:
                    assert int(keep.sum()) == n - int(inside.sum()), what
                if basis == "own":                                      # the run is gone: now the buffers may grow
                    e.basis_from_poses_dev(fs, d_frags, *d_more, more, heavy_idx)
                    assert e.embed_masked_dev(fs, d_frags, *d_more, more, d_ones_more, heavy_idx, None, d_heavy_more) == more
                    e.synchronize()
                    assert np.array_equal(d_heavy_more.cpu().numpy()[n:], heavy[:more - n])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------ C3: the LDS gate
def transform_describe_lds_bytes(n_mols, h):
    """csrc/describe.hpp, restated: the staged pose parameters of k_transform (TR_POSES x n_mols x (12 doubles + an int) + TR_POSES indices), rounded
    up to 16 bytes, the basis ([8][features of both families]) and TR_POSES rows of (3 h | 1) doubles."""
    transform = TR_POSES * n_mols * (12 * 8 + 4) + TR_POSES * 8
    features = min(h, 256) + min(h // 2, 256)
    return (transform + 15) // 16 * 16 + (8 * features + TR_POSES * ((3 * h) | 1)) * 8


def last_fitting(n_mols):
    return max(h for h in range(1, 200) if transform_describe_lds_bytes(n_mols, h) <= 64 * 1024)


GATE_FRAGMENTS = {2: (45, 45), 3: (30, 30, 30)}
GATE_CASES = [(2, 0), (2, 1), (3, 0), (3, 1), (2, -1), (2, -2), (2, -3)]       # (fragments, heavy atoms beyond the last fitting count; -k: k atoms)


def gate_case(n_mols, delta):
    """(ensemble, heavy_idx): 600 poses in families of 8 whose members lie around the prune's threshold from each other, shuffled locally."""
    from tscode_amd.synthetic import make_ensemble
    key = f"gate-{n_mols}"
    if key not in _cases:
        _cases[key] = make_ensemble(600, GATE_FRAGMENTS[n_mols], seed=zlib.crc32(key.encode()), children=8, sigma_rot_deg=4.0, sigma_t=0.2,
                                    shell=(9.0, 16.0), local_spread=40.0)
    ens = _cases[key]
    h = last_fitting(n_mols) + delta if delta >= 0 else -delta
    heavy_idx = np.sort(_rng(f"gate-{n_mols}-{h}").choice(ens.n_atoms, size=h, replace=False)).astype(np.int32)
    return ens, heavy_idx


def gate_reference(oracle, n_mols, delta, mode):
    key = ("gate", n_mols, delta, mode)
    if key not in _refs:
        ens, heavy_idx = gate_case(n_mols, delta)
        cm, poses = clash_reference(oracle, f"gate-{n_mols}", (ens.frag_coords, ens.conf_idx, ens.rot, ens.pos, ens.ids))
        _refs[key] = oracle.prune_heavy(np.ascontiguousarray(poses[cm][:, heavy_idx]), THR, mode=mode, row_parallel=True)
    return _refs[key]


def test_the_lds_gate_is_where_the_formula_puts_it():
    assert (last_fitting(2), last_fitting(3)) == (67, 64)
    for n_mols in (2, 3):
        h = last_fitting(n_mols)
        assert transform_describe_lds_bytes(n_mols, h) <= 65536 < transform_describe_lds_bytes(n_mols, h + 1)
        assert h + 1 <= sum(GATE_FRAGMENTS[n_mols])


@pytest.mark.parametrize("n_mols,delta", GATE_CASES)
def test_gate_ensembles_give_the_prune_something_to_decide(oracle, n_mols, delta):
    ens, heavy_idx = gate_case(n_mols, delta)
    cm, _ = clash_reference(oracle, f"gate-{n_mols}", (ens.frag_coords, ens.conf_idx, ens.rot, ens.pos, ens.ids))
    assert 200 <= cm.sum() < ens.n_poses
    if delta >= 0:
        assert len(set(np.searchsorted(np.cumsum(ens.ids), heavy_idx, side="right"))) == n_mols
        for mode in (0, 1):
            kept = int(gate_reference(oracle, n_mols, delta, mode)["mask"].sum())
            assert cm.sum() / 8 < kept < 0.9 * cm.sum(), (n_mols, delta, mode, kept, int(cm.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_mols,delta", GATE_CASES)
def test_pipeline_on_both_sides_of_the_lds_gate(eng, oracle, n_mols, delta, mode):
    import torch

    from tscode_amd.engine import FragmentSet
    ens, heavy_idx = gate_case(n_mols, delta)
    case = (ens.frag_coords, ens.conf_idx, ens.rot, ens.pos, ens.ids)
    cm, poses = clash_reference(oracle, f"gate-{n_mols}", case)
    ref = gate_reference(oracle, n_mols, delta, mode)
    n, n_pass = ens.n_poses, int(cm.sum())
    fs = FragmentSet(ens.frag_coords)
    dev = (_dev(fs.flat), _dev(ens.conf_idx), _dev(ens.rot), _dev(ens.pos))
    bound = embed_bound(case)[cm]
    for opts in ({}, dict(pca_min_n=0), dict(prune_algo=2, stage1_f32=2)):
        d_clash, d_keep = _filled((n,), 0xAA, torch.uint8), _filled((n,), 0xAA, torch.uint8)
        d_s = _filled((n, ens.n_atoms, 3), FILL, torch.float64)
        with eng.options(**opts):
            res = eng.pipeline_dev(fs, *dev, n, heavy_idx, THRESH, 0, THR, mode, d_clash, d_s, d_keep)
            eng.synchronize()
        what = (n_mols, len(heavy_idx), mode, opts)
        assert np.array_equal(d_clash.cpu().numpy(), cm.astype(np.uint8)) and res["n_pass"] == n_pass, what
        got = d_s.cpu().numpy()
        assert (np.abs(got[:n_pass] - poses[cm]) <= bound).all() and (got[n_pass:] == FILL).all(), what
        keep = d_keep.cpu().numpy()[:n_pass]
        assert set(np.unique(keep)) <= {0, 1} and np.array_equal(keep.astype(bool), ref["mask"]), what
        assert res["n_keep"] == int(ref["mask"].sum()) and per_pass(res["stats"]) == per_pass(ref["stats"]), what
