"""Golden vectors G27: a multiembed's children (tscode/multiembed.py:26-148), THE REFERENCE'S FUNCTIONS DRIVEN IN run_child_embedder'S ORDER.

BUILD CONTAINER ONLY: it imports the reference's own modules, which exist where fixtures are recorded and nowhere else.  The real run_child_embedder does not run under the stand-ins of tests/golden/_reference.py:
it parses an input file through the whole Embedder constructor (calculator settings, cclib, a log file per child).  So, per arrangement, this
generator does what the child does, step by step, with the reference's own code:

  Hypermolecule + compute_orbitals for ``{mol1} {ix_1}x {iy_1}y`` / ``{mol2} {ix_2}x {iy_2}y``   (multiembed.py:117-119; gen_golden_embeds._molecule)
  _set_reactive_atoms_cumnums, _set_pivots, the default angle table (rotation_range 45, rotation_steps 5: embedder.py:708-715; a child
      inherits debug / simpleorbitals / shrink only, multiembed.py:111-119)
  the pairings of the two letters: pairings_table = {x: [ix_1, ix_2 + n1], y: [iy_1, iy_2 + n1]} (embedder.py:456), pairings_dict (:376-426)
  cyclical_embed(embedder)             -> the rigid shortcut with max_norm_delta = 5 (embeds.py:234-241)     [generate_candidates, :1154]
  atomnos, embed_graph = get_sum_graph(graphs, constrained_indices[0]), write_structures('embedded')        [:1157-1174]
  compenetration_refining              -> energies / exit_status only for a cyclical embed (:1236, :1265-1266)
  fitness_refining()                   (threshold 5; :1267-1305)
  similarity_refining(rmsd=False)      (:1307-1354)
  write_structures('unoptimized')      -> align_structures centres self.structures IN PLACE (hypermolecule_class.py:46-55)

WHAT THE REFERENCE DOES AT THE TFD STAGE.  similarity_refining enters it only where ``embed_graph.is_single_molecule`` (:1326), and
get_sum_graph evaluates that flag BEFORE it adds the extra edges (graph_manipulations.py:318-322): for two separate molecules it is
False, so a child never takes the TFD stage.  The fixture records that (``tfd_entered`` False, the stage's mask all True: chain "ref").
It ALSO records, as chain "tfd", the same state run once more with the flag set -- the reference's own prune_conformers_tfd on the
quadruplets of that embed_graph, then its MOI stage -- which is what ``multiembed_batch(tfd=True)`` is checked against.

Cases (tscode/tests/*.xyz, the child's default orbitals and thresholds):
  a  C2H4 [0, 3] x HCOOH [1, 3]                      4 arrangements
  b  C2H4 [0, 3] x HCOOH [0, 1, 3]                   12 arrangements: the order of itertools.permutations
  c  conformer stacks of both (G12's _conformers)    4 arrangements
  d  case a once more with a lowered fitness threshold, only if no case above loses a structure to fitness_refining(threshold=5)

Coverage: across the fixture the clash mask, the group filter, MOI (chain "ref"), TFD (chain "tfd") and fitness each remove a
structure somewhere, and two arrangements of a case differ in their counts; the generator prints the counts and fails otherwise.
Margins: a case is refused when a clash distance lies within 1e-9 of the threshold, a group-filter RMSD / deviation within 1e-9 of its
bound, a fitness error within 1e-9 of the threshold, a relative MOI difference within 1e-9 of max_deviation, or a TFD sum within 1e-3
degrees of its threshold (float32 fingerprints).

Usage:  python -B tests/golden/gen_multiembed.py
"""

from __future__ import annotations

import copy
import json
import os
import re
import sys
import types
from itertools import permutations

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_embeds as G     # noqa: E402  (installs the stand-ins, imports the reference's modules)

R = G.R
ref_embedder, ref_embeds, ref_utils, ref_alg = G.ref_embedder, G.ref_embeds, G.ref_utils, G.ref_alg
import tscode.graph_manipulations as ref_graph     # noqa: E402
import tscode.multiembed as ref_multi              # noqa: E402
import tscode.rmsd_pruning as ref_rmsd             # noqa: E402
from tscode.errors import ZeroCandidatesError      # noqa: E402

sys.path.insert(0, R.REPO)
import oracle                                      # noqa: E402

# align_structures turns every structure onto the first with the `rmsd` package's kabsch (a name-only stand-in here) for the FILE it writes;
# what it leaves in self.structures is the in-place centring in front of that (hypermolecule_class.py:46-55), which is all the child returns
G.ref_hc.kabsch = lambda p, q: np.eye(3)

NAME = "G27_multiembed"
SCRATCH = "/tmp/tscode_amd_golden"
GUARD = 1e-9
TFD_GUARD = 1e-3


def arrangements_of(r1, r2):
    """multiembed.py:36-39, the reference's lines on the reference's cartesian_product."""
    pairs = ref_utils.cartesian_product(np.asarray(r1), np.asarray(r2))
    return [((ix_1, ix_2), (iy_1, iy_2)) for ((ix_1, ix_2), (iy_1, iy_2)) in permutations(pairs, 2) if ix_1 != iy_1 and ix_2 != iy_2]


def _bind(e, *names):
    for name in names:
        setattr(e, name, types.MethodType(getattr(ref_embedder.RunEmbedding, name), e))


def _child(files, arrangement):
    """The child's Embedder state up to generate_candidates, on the stand-in namespace of gen_golden_embeds._embedder."""
    (ix_1, ix_2), (iy_1, iy_2) = (tuple(int(v) for v in p) for p in arrangement)
    mols = [G._molecule(files[0], [ix_1, iy_1]), G._molecule(files[1], [ix_2, iy_2])]
    e = G._embedder(mols, "cyclical")
    for m in mols:
        ref_embedder.Embedder._set_pivots(e, m)
    rr, steps = 45, 5
    e.systematic_angles = ref_utils.cartesian_product(*[range(steps + 1) for _ in mols]) * 2 * rr / steps - rr
    n1 = len(mols[0].atomnos)
    e.pairings_table = {"x": sorted([ix_1, ix_2 + n1]), "y": sorted([iy_1, iy_2 + n1])}
    e.pairings_dict = {0: {"x": ix_1, "y": iy_1}, 1: {"x": ix_2, "y": iy_2}}
    e.graphs = [m.graph for m in mols]
    e.options.shrink, e.options.let, e.options.ff_level = False, False, ""
    e.stamp = "golden"
    e.log_warnings = lambda: None
    _bind(e, "apply_mask", "zero_candidates_check", "get_pairing_dist_from_letter", "get_pairing_dists_from_constrained_indices", "write_structures",
          "compenetration_refining", "fitness_refining", "similarity_refining")
    return e, mols


def _embed(e):
    """cyclical_embed with G12's tracing wrappers, plus the smallest distance of a group-filter comparison from its two bounds."""
    margin = [np.inf]
    real = ref_rmsd.rmsd_and_max_numba

    def noted(p, q):
        r, m = real(p, q)
        margin[0] = min(margin[0], abs(r - 1.0), abs(m - 2.0))
        return r, m
    ref_rmsd.rmsd_and_max_numba = noted
    try:
        tr = G._trace_cyclical_embed(e)
    finally:
        ref_rmsd.rmsd_and_max_numba = real
    tr["filter_margin"] = margin[0]
    return tr


def _refine(e, fitness_threshold, force_tfd):
    """fitness_refining, similarity_refining(rmsd=False), write_structures on a copy of the child's state after generate_candidates.  Returns the
    stage masks (each over the rows the stage saw), whether the TFD stage was entered, and what the child would hand back."""
    e = copy.copy(e)
    e.structures, e.constrained_indices = e.structures.copy(), e.constrained_indices.copy()
    e.embed_graph = copy.deepcopy(e.embed_graph)
    _bind(e, "apply_mask", "zero_candidates_check", "get_pairing_dist_from_letter", "get_pairing_dists_from_constrained_indices", "write_structures",
          "compenetration_refining", "fitness_refining", "similarity_refining")
    if force_tfd:
        e.embed_graph.is_single_molecule = True
    n0 = len(e.structures)
    out = {"fitness": np.ones(n0, bool), "tfd": None, "moi": None, "tfd_entered": False, "moi_entered": False, "tfd_margin": np.inf, "moi_margin": np.inf}
    real_tfd, real_moi, real_fit = ref_embedder.prune_conformers_tfd, ref_embedder.prune_by_moment_of_inertia, ref_embedder.fitness_check
    errors = []

    def fit(structure, constraints, targets, threshold):
        errors.append(sum(np.linalg.norm(structure[a] - structure[b]) - t for (a, b), t in zip(constraints, targets) if t is not None))
        return real_fit(structure, constraints, targets, threshold=threshold)

    def tfd(structures, quadruplets, **kw):
        kept, mask = real_tfd(structures, quadruplets, **kw)
        out["tfd"], out["tfd_entered"] = np.asarray(mask, bool), True
        fp = np.array([ref_embeds.get_torsion_fingerprint(s, quadruplets) for s in structures], dtype=np.float32)
        d = np.abs(fp[:, None] - fp[None])
        d = np.abs(d - (d > 180) * 360).sum(axis=2)
        out["tfd_margin"] = float(np.abs(d[np.triu_indices(len(fp), 1)] - 10).min()) if len(fp) > 1 else np.inf
        return kept, mask

    def moi(structures, atomnos, **kw):
        kept, mask = real_moi(structures, atomnos, **kw)
        out["moi"], out["moi_entered"] = np.asarray(mask, bool), True
        heavy = atomnos != 1
        masses = np.array([R.ELEMENTS[int(a)][2] for a in atomnos[heavy]])
        im = np.array([ref_alg.get_inertia_moments(s[heavy], masses) for s in structures])
        rel = np.abs(im[:, None] - im[None]) / im[:, None]
        iu = np.triu_indices(len(im), 1)
        out["moi_margin"] = float(np.abs(rel[iu] - 1e-2).min()) if len(im) > 1 else np.inf
        return kept, mask

    ref_embedder.prune_conformers_tfd, ref_embedder.prune_by_moment_of_inertia, ref_embedder.fitness_check = tfd, moi, fit
    cwd = os.getcwd()
    os.chdir(SCRATCH)
    try:
        try:
            e.compenetration_refining()
            real_apply = e.apply_mask

            def apply_fitness(attr, mask):
                out["fitness"] = np.asarray(mask, bool).copy()
                real_apply(attr, mask)
            e.apply_mask = apply_fitness
            try:
                e.fitness_refining(threshold=fitness_threshold)
            finally:
                e.apply_mask = real_apply
            e.similarity_refining(rmsd=False, verbose=True)
            e.write_structures("unoptimized", energies=False)
        except ZeroCandidatesError:
            e.structures = np.zeros((0, e.structures.shape[1], 3))
            e.constrained_indices = np.zeros((0, 2, 2), dtype=np.int64)
    finally:
        os.chdir(cwd)
        ref_embedder.prune_conformers_tfd, ref_embedder.prune_by_moment_of_inertia, ref_embedder.fitness_check = real_tfd, real_moi, real_fit
    n_fit = int(out["fitness"].sum())
    if out["tfd"] is None:
        out["tfd"] = np.ones(n_fit, bool)
    if out["moi"] is None:
        out["moi"] = np.ones(int(out["tfd"].sum()), bool)
    out["errors"] = np.array(errors, dtype=np.float64)
    out["fitness_margin"] = float(np.abs(out["errors"] - fitness_threshold).min()) if len(errors) else np.inf
    out["final"] = np.asarray(e.structures, dtype=np.float64).reshape(-1, e.ids.sum(), 3)
    out["final_constrained"] = np.asarray(e.constrained_indices).reshape(-1, 2, 2)
    return out


def record_case(flat, key, files, reactive, fitness_threshold=5):
    arrs = arrangements_of(*reactive)
    flat[f"arrangements_{key}"] = np.array(arrs, dtype=np.int64).reshape(-1, 2, 2)
    flat[f"reactive0_{key}"], flat[f"reactive1_{key}"] = np.asarray(reactive[0]), np.asarray(reactive[1])
    flat[f"fitness_threshold_{key}"] = float(fitness_threshold)
    counts, margins = [], dict(clash=np.inf, filter=np.inf, fitness=np.inf, moi=np.inf, tfd=np.inf)
    removed = dict(clash=0, filter=0, fitness=0, moi_ref=0, tfd_forced=0)
    for a, arr in enumerate(arrs):
        e, mols = _child(files, arr)
        k = f"{key}_{a}"
        if a == 0:
            for m, mol in enumerate(mols):
                flat[f"coords{m}_{key}"], flat[f"atomnos{m}_{key}"] = np.asarray(mol.atomcoords), np.asarray(mol.atomnos)
                flat[f"edges{m}_{key}"] = np.array(sorted(tuple(sorted(ed)) for ed in mol.graph.edges() if ed[0] != ed[1]), dtype=np.int64).reshape(-1, 2)
            flat[f"angles_{key}"] = np.asarray(e.systematic_angles, dtype=np.float64)
            flat[f"ids_{key}"] = np.asarray(e.ids)
        inp = G._cyclical_inputs(e)
        for name, v in inp.items():
            if name.startswith(("reactive_indices", "pivot_")):
                flat[f"{name}_{k}"] = v
        for m, mol in enumerate(mols):       # the lobes of conformer 0: what get_orbital_length reads (hypermolecule_class.py:366)
            for j, idx in enumerate(mol.reactive_indices):
                r_atom = mol.reactive_atoms_classes_dict[0][int(idx)]
                flat[f"lobes{m}_{j}_{k}"] = np.asarray(r_atom.center, dtype=np.float64).reshape(-1, 3)
        try:
            tr = _embed(e)
        except ZeroCandidatesError:
            raise SystemExit(f"case {key}, arrangement {a}: the embed itself found nothing; choose another case")
        margins["clash"] = min(margins["clash"], oracle.clash_margin(tr["candidates"], e.ids, 1.5))
        margins["filter"] = min(margins["filter"], tr["filter_margin"])
        n_groups = len(tr["group_ids"])
        for name in ("group_of", "group_ids", "clash_ok", "kept", "poses", "constrained_indices"):
            flat[f"{name}_{k}"] = tr[name]
        # generate_candidates, :1154-1174
        e.structures = np.asarray(tr["poses"]).copy()
        e.atomnos = np.concatenate([m.atomnos for m in mols])
        e.embed_graph = ref_graph.get_sum_graph(e.graphs, e.constrained_indices[0])
        flat[f"is_single_molecule_{k}"] = bool(e.embed_graph.is_single_molecule)
        quads = np.asarray(ref_embedder._get_quadruplets(e.embed_graph), dtype=np.int64).reshape(-1, 4)
        flat[f"quadruplets_{k}"] = quads
        flat[f"targets_{k}"] = np.array([e.get_pairing_dists_from_constrained_indices(c) for c in e.constrained_indices[0]], dtype=np.float64)
        cwd = os.getcwd()
        os.chdir(SCRATCH)
        try:
            e.write_structures("embedded", energies=False)
        finally:
            os.chdir(cwd)
        row = None
        for chain, force in (("ref", False), ("tfd", True)):
            out = _refine(e, fitness_threshold, force)
            for name in ("fitness", "tfd", "moi"):
                flat[f"{chain}_{name}_mask_{k}"] = out[name]
            flat[f"{chain}_tfd_entered_{k}"], flat[f"{chain}_moi_entered_{k}"] = out["tfd_entered"], out["moi_entered"]
            flat[f"{chain}_final_{k}"], flat[f"{chain}_final_constrained_{k}"] = out["final"], out["final_constrained"]
            c6 = [len(tr["clash_ok"]), int(tr["clash_ok"].sum()), int(tr["kept"].sum()), int(out["fitness"].sum()), int(out["tfd"].sum()),
                  int(out["moi"].sum())]
            assert c6[5] == len(out["final"]), (c6, len(out["final"]))
            flat[f"{chain}_counts_{k}"] = np.array(c6, dtype=np.int64)
            margins["fitness"] = min(margins["fitness"], out["fitness_margin"])
            margins["moi"] = min(margins["moi"], out["moi_margin"])
            margins["tfd"] = min(margins["tfd"], out["tfd_margin"])
            if chain == "ref":
                assert not out["tfd_entered"], "the reference entered the TFD stage of a two-molecule child: read the module docstring again"
                flat[f"fitness_errors_{k}"] = out["errors"]
                row = c6
                removed["moi_ref"] += c6[4] - c6[5]
                removed["fitness"] += c6[2] - c6[3]
            else:
                removed["tfd_forced"] += c6[3] - c6[4]
                print(f"    case {key} arrangement {a:2d} {arr}: {n_groups} groups, counts {row}; with the TFD stage forced {c6}")
        removed["clash"] += row[0] - row[1]
        removed["filter"] += row[1] - row[2]
        counts.append(tuple(row))
    flat[f"n_arrangements_{key}"] = len(arrs)
    print(f"  case {key}: margins " + ", ".join(f"{n} {v:.3e}" for n, v in margins.items()) + f"; removed {removed}")
    for name, v in margins.items():
        if not v > (TFD_GUARD if name == "tfd" else GUARD):
            raise SystemExit(f"case {key}: a {name} verdict sits on a knife edge ({v:.3e})")
    return counts, removed


def import_sites():
    """Where the reference binds multiembed_dispatcher / multiembed_bifunctional: the defining module, and every module whose import lines name them."""
    sites = {"multiembed_dispatcher": ["tscode.multiembed"], "multiembed_bifunctional": ["tscode.multiembed"]}
    root = os.path.join(R.REFERENCE, "tscode")
    for dirpath, _, files in os.walk(root):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            mod = "tscode." + os.path.relpath(path, root)[:-3].replace(os.sep, ".")
            if mod == "tscode.multiembed":
                continue
            text = open(path).read()
            for block in re.findall(r"from\s+tscode\.multiembed\s+import\s+(\([^)]*\)|[^\n]*)", text):
                for name in re.findall(r"[A-Za-z_][A-Za-z_0-9]*", block):
                    if name in sites and mod not in sites[name]:
                        sites[name].append(mod)
    return {k: sorted(v) for k, v in sites.items()}


def main():
    print("G27 multiembed children (the reference's functions driven in run_child_embedder's order)")
    os.makedirs(SCRATCH, exist_ok=True)
    flat = {"seed": 9127, "label": "the reference's functions driven in run_child_embedder's order"}
    C2H4, HCOOH = (os.path.join(G.TESTS, f) for f in ("C2H4.xyz", "HCOOH.xyz"))
    rng = np.random.default_rng(9127)
    pc, ph = os.path.join(SCRATCH, "C2H4_confs_m.xyz"), os.path.join(SCRATCH, "HCOOH_confs_m.xyz")
    zc, cc_ = R.read_xyz_data(C2H4)
    zh, ch_ = R.read_xyz_data(HCOOH)
    G._write_xyz(pc, zc, G._conformers(zc, cc_[0], rng, 2, (0, 3), [1, 2], jitter=0.03, jitter_first=True))
    G._write_xyz(ph, zh, G._conformers(zh, ch_[0], rng, 3, (0, 3), [4]))
    cases = [("a", (C2H4, HCOOH), ([0, 3], [1, 3])), ("b", (C2H4, HCOOH), ([0, 3], [0, 1, 3])), ("c", (pc, ph), ([0, 3], [1, 3]))]
    total = dict(clash=0, filter=0, fitness=0, moi_ref=0, tfd_forced=0)
    differ = False
    keys = []
    for key, files, reactive in cases:
        counts, removed = record_case(flat, key, files, reactive)
        keys.append(key)
        differ = differ or len(set(counts)) > 1
        for name, v in removed.items():
            total[name] += v
    if total["fitness"] == 0:
        # no real case trips the fitness stage at threshold 5: case a once more, the threshold lowered into the widest gap of its errors
        errs = np.sort(np.concatenate([flat[f"fitness_errors_a_{a}"] for a in range(int(flat["n_arrangements_a"]))]))
        gaps = np.diff(errs)
        at = int(np.argmax(gaps))
        thr = float((errs[at] + errs[at + 1]) / 2)
        print(f"  no case loses a structure at fitness threshold 5 (errors {errs.min():.3f} .. {errs.max():.3f}): case d = case a at threshold {thr:.6f}")
        counts, removed = record_case(flat, "d", cases[0][1], cases[0][2], fitness_threshold=thr)
        keys.append("d")
        for name, v in removed.items():
            total[name] += v
    flat["cases"] = np.array(keys)
    print(f"  removed across the fixture: {total}; counts differ between arrangements: {differ}")
    if not (differ and all(v > 0 for v in total.values())):
        raise SystemExit("coverage condition not met: every stage must remove a structure somewhere and two arrangements must differ")
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **flat)
    print(f"  wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")
    sites = import_sites()
    with open(os.path.join(HERE, NAME + ".json"), "w") as f:
        json.dump({"label": "import sites of the multiembed functions in the reference (module names)", "sites": sites}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"  sites: {sites}")
    assert hasattr(ref_multi, "multiembed_bifunctional")


if __name__ == "__main__":
    main()
