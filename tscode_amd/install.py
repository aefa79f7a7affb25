"""Patch a live TSCoDe so that its hot path runs on the MI355X engine.

TSCoDe binds the hot-path functions by name at import time (``from tscode.rmsd_pruning import
prune_conformers_rmsd`` in embedder.py:56, operators.py:39, optimization_methods.py:32,
atropisomer_module.py:33; ``compenetration_check`` in embedder.py:48, embeds.py:28; ...), so the
replacement has to be set on every importing module, not only on the defining one.
This module never imports tscode itself: it only touches modules already in sys.modules.
"""

from __future__ import annotations

import sys

from . import algebra, embeds, graph_manipulations, hypermolecule_class, nci, numba_functions, optimization_methods, rmsd_pruning, rot_corr, torsion_module
from . import multiembed as _multiembed      # (install() has a switch of the module's name)
from . import utils

# attribute -> (replacement, modules that bind it)
_PATCHES = {
    "prune_conformers_rmsd": (rmsd_pruning.prune_conformers_rmsd,
                              ("tscode.rmsd_pruning", "tscode.embedder", "tscode.operators", "tscode.optimization_methods",
                               "tscode.atropisomer_module")),
    "rmsd_and_max_numba": (rmsd_pruning.rmsd_and_max_numba, ("tscode.rmsd_pruning", "tscode.automep")),
    "_rmsd_similarity": (rmsd_pruning._rmsd_similarity, ("tscode.rmsd_pruning", "tscode.embeds")),
    "compenetration_check": (numba_functions.compenetration_check, ("tscode.numba_functions", "tscode.embedder", "tscode.embeds")),
    "count_clashes": (numba_functions.count_clashes, ("tscode.numba_functions", "tscode.embedder")),
    "get_embed": (embeds.get_embed, ("tscode.embeds",)),
    "all_dists": (algebra.all_dists, ("tscode.algebra", "tscode.numba_functions", "tscode.graph_manipulations")),
    "transform_coords": (algebra.transform_coords, ("tscode.algebra",)),
    # (any real angle: tscode/torsion_module.py:984-1005 calls it with fractional corrections; the candidate loops of the
    # conformational search belong on tscode_amd.csearch_rotate, which takes their integer tables whole)
    "rotate_dihedral": (torsion_module.rotate_dihedral, ("tscode.utils", "tscode.torsion_module")),
    "torsion_comp_check": (torsion_module.torsion_comp_check, ("tscode.numba_functions", "tscode.torsion_module")),
    "get_moi_similarity_matches": (optimization_methods.get_moi_similarity_matches, ("tscode.algebra", "tscode.optimization_methods")),
    "_score_embed_poses": (optimization_methods._score_embed_poses, ("tscode.numba_functions",)),
    "fitness_check": (optimization_methods.fitness_check, ("tscode.optimization_methods", "tscode.embedder")),
    "prune_conformers_tfd": (numba_functions.prune_conformers_tfd,
                             ("tscode.numba_functions", "tscode.embedder", "tscode.operators", "tscode.torsion_module")),
    # the embed loops themselves (tscode/embedder.py:39-40 binds both names; generate_candidates looks them up at call time, :1141-1154)
    "string_embed": (embeds.string_embed, ("tscode.embeds", "tscode.embedder")),
    "cyclical_embed": (embeds.cyclical_embed, ("tscode.embeds", "tscode.embedder")),
}

# Functions that take a whole ensemble per call: what install() replaces by default.  The others are called by TSCoDe once per
# pose / pair from Python loops; a GPU call (upload, launch, download, synchronise) takes 35-185 us against the few microseconds of
# the reference's jitted function (tools/dropin_latency.py), so replacing them would SLOW those loops down -- they are drop-in
# equivalents for checking and for callers that move to the batched forms, patched only on request.
_WHOLE_ENSEMBLE = ("prune_conformers_rmsd", "prune_conformers_tfd", "get_moi_similarity_matches", "_score_embed_poses", "string_embed",
                   "cyclical_embed")

# Opt-in (install(rot_corr=True)): the symmetry-corrected prune of the refinement stage (tscode/embedder.py:1372-1382,
# tscode/operators.py:571), bound by name in these three modules.  Off by default until it has a number from hardware.
_ROT_CORR_PATCHES = {
    "prune_conformers_rmsd_rot_corr": (rot_corr.prune_conformers_rmsd_rot_corr,
                                       ("tscode.torsion_module", "tscode.embedder", "tscode.operators")),
}

# Opt-in (install(diverse=True)): the end of a conformational search (tscode/torsion_module.py:817, :837) and the alignment that
# embedder.py runs on the whole ensemble at every checkpoint (:1195, 1405, 1515, 1581, 1749, 1818, 2045).  align_structures is bound
# by name in eight modules, most_diverse_conformers only where it is defined.
_DIVERSE_PATCHES = {
    "align_structures": (hypermolecule_class.align_structures,
                         ("tscode.hypermolecule_class", "tscode.embedder", "tscode.operators", "tscode.torsion_module",
                          "tscode.ase_manipulations", "tscode.mep_relaxer", "tscode.atropisomer_module", "tscode.automep")),
    "most_diverse_conformers": (torsion_module.most_diverse_conformers, ("tscode.torsion_module",)),
}

# Opt-in (install(topology=True)): the topology checks the reference applies to every structure that survives the embed and prune steps
# (tscode/embedder.py:1489, 1725, tscode/optimization_methods.py:115-117, tscode/ase_manipulations.py:286, 342-344, 830, ...).  The sites
# are the ones tests/golden/gen_topology.py records from the reference's import lines (G21_topology_sites.json).  Off by default until
# the per-call latency has a number from hardware (tools/dropin_latency.py).
_TOPOLOGY_PATCHES = {
    "graphize": (graph_manipulations.graphize,
                 ("tscode.ase_manipulations", "tscode.atropisomer_module", "tscode.embedder", "tscode.graph_manipulations",
                  "tscode.hypermolecule_class", "tscode.operators", "tscode.pka", "tscode.torsion_module", "tscode.utils")),
    "molecule_check": (utils.molecule_check,
                       ("tscode.ase_manipulations", "tscode.atropisomer_module", "tscode.operators", "tscode.optimization_methods",
                        "tscode.utils")),
    "scramble_check": (utils.scramble_check,
                       ("tscode.ase_manipulations", "tscode.calculators._openbabel", "tscode.embedder", "tscode.optimization_methods",
                        "tscode.utils")),
    "get_double_bonds_indices": (utils.get_double_bonds_indices, ("tscode.ase_manipulations", "tscode.torsion_module", "tscode.utils")),
}

# Opt-in (install(nci=True)): the non-covalent-interaction finder that print_nci calls once per structure (tscode/embedder.py:2063; bound
# by name at :47).  The sites are the ones tests/golden/gen_nci.py records from the reference's import lines (G22_nci_sites.json).  Off by
# default like the other per-structure drop-ins; a caller with an ensemble wants tscode_amd.nci_batch and differential_nci.
_NCI_PATCHES = {
    "get_nci": (nci.get_nci, ("tscode.embedder", "tscode.nci")),
}

# Opt-in (install(csearch=True)): the clustered conformational search, which csearch reaches with its default mode
# (tscode/torsion_module.py:623-640), and the grouping it starts with (:693).  Both names are bound only where they are defined; the
# sites are the ones tests/golden/gen_clustered_csearch.py records from the reference's import lines (G26_clustered_csearch_sites.json).
# The drop-in hands ff_opt, mode 0 and write_torsions to the function it replaced (torsion_module._csearch_originals).
_CSEARCH_PATCHES = {
    "clustered_csearch": (torsion_module.clustered_csearch, ("tscode.torsion_module",)),
    "_group_torsions_dbscan": (torsion_module._group_torsions_dbscan, ("tscode.torsion_module",)),
}

# Opt-in (install(multiembed=True)): the multiembed, the one embed of generate_candidates' table (tscode/embedder.py:1141-1147) that fans out
# to child processes (tscode/multiembed.py:49-73).  The sites are the ones tests/golden/gen_multiembed.py records from the reference's
# import lines (G27_multiembed.json): the dispatcher is bound by name in tscode.embedder, the bifunctional driver only where it is
# defined (the reference's dispatcher looks it up there at call time).  The drop-ins hand shrink / simpleorbitals / debug children and
# runs of more than two molecules to the functions they replaced (multiembed._originals).
_MULTIEMBED_PATCHES = {
    "multiembed_dispatcher": (_multiembed.multiembed_dispatcher, ("tscode.embedder", "tscode.multiembed")),
    "multiembed_bifunctional": (_multiembed.multiembed_bifunctional, ("tscode.multiembed",)),
}

_OPT_IN = (_ROT_CORR_PATCHES, _DIVERSE_PATCHES, _TOPOLOGY_PATCHES, _NCI_PATCHES, _CSEARCH_PATCHES, _MULTIEMBED_PATCHES)

_saved = {}


def install(modules=None, per_item=False, rot_corr=False, diverse=False, topology=False, nci=False, csearch=False, multiembed=False):
    """Replace the hot-path functions in every already-imported tscode module: by default those that work on a whole ensemble
    per call (prune_conformers_rmsd, prune_conformers_tfd, get_moi_similarity_matches, _score_embed_poses) and the two embed
    loops (string_embed, cyclical_embed: one GPU call each instead of one Python iteration per pose); with
    ``per_item=True`` also the per-pose / per-pair ones (compenetration_check, get_embed, rmsd_and_max_numba, ...), which are
    equivalent but slower than the reference's jitted code when called one item at a time; with ``rot_corr=True`` also
    prune_conformers_rmsd_rot_corr (_ROT_CORR_PATCHES); with ``diverse=True`` also align_structures and most_diverse_conformers
    (_DIVERSE_PATCHES); with ``topology=True`` also graphize, molecule_check, scramble_check and get_double_bonds_indices
    (_TOPOLOGY_PATCHES); with ``nci=True`` also get_nci (_NCI_PATCHES); with ``csearch=True`` also clustered_csearch and
    _group_torsions_dbscan (_CSEARCH_PATCHES); with ``multiembed=True`` also multiembed_dispatcher and multiembed_bifunctional
    (_MULTIEMBED_PATCHES).
    Returns the list of (module, attribute) pairs that were patched."""
    mods = sys.modules if modules is None else modules
    done = []
    table = (list(_PATCHES.items()) + (list(_ROT_CORR_PATCHES.items()) if rot_corr else []) +
             (list(_DIVERSE_PATCHES.items()) if diverse else []) + (list(_TOPOLOGY_PATCHES.items()) if topology else []) +
             (list(_NCI_PATCHES.items()) if nci else []) + (list(_CSEARCH_PATCHES.items()) if csearch else []) +
             (list(_MULTIEMBED_PATCHES.items()) if multiembed else []))
    for attr, (fn, names) in table:
        if not per_item and attr not in _WHOLE_ENSEMBLE and not any(attr in t for t in _OPT_IN):
            continue
        for name in names:
            mod = mods.get(name)
            if mod is not None and hasattr(mod, attr):
                _saved.setdefault((name, attr), getattr(mod, attr))
                if attr in ("string_embed", "cyclical_embed") and name == "tscode.embeds":
                    embeds._originals[attr] = _saved[(name, attr)]      # what the drop-in hands the cases it does not cover to
                if attr in _CSEARCH_PATCHES and name == "tscode.torsion_module":
                    torsion_module._csearch_originals[attr] = _saved[(name, attr)]
                if attr in _MULTIEMBED_PATCHES and name == "tscode.multiembed":
                    _multiembed._originals[attr] = _saved[(name, attr)]
                setattr(mod, attr, fn)
                done.append((name, attr))
    return done


def uninstall(modules=None):
    mods = sys.modules if modules is None else modules
    for (name, attr), fn in list(_saved.items()):
        mod = mods.get(name)
        if mod is not None:
            setattr(mod, attr, fn)
        del _saved[(name, attr)]
    embeds._originals.clear()
    torsion_module._csearch_originals.clear()
    _multiembed._originals.clear()
