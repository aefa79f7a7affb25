"""tscode_amd -- MI355X (gfx950) engine for TSCoDe's geometry hot path.

Drop-in mirrors of the reference's functions (same names and signatures):

    from tscode_amd import prune_conformers_rmsd, compenetration_check, get_embed
    import tscode_amd; tscode_amd.install()      # patch an already imported tscode

Everything numeric runs in libtscode_hip.so (hand-written HIP kernels behind the C ABI of
include/tscode_hip.h).  There is no CPU fallback; importing this package does not touch the GPU.
"""

from .algebra import (align_vec_pair, all_dists, norm, norm_of, quaternion_to_rotation_matrix,  # noqa: F401
                      rot_mat_from_pointer, rotation_matrix_from_vectors, transform_coords, vec_angle)
from .embeds import (EmbedTrace, cyclical_embed_batch, cyclical_embed_params, cyclical_embed_prune_batch, embed_batch, filter_angular_groups, get_embed,  # noqa: F401
                     string_embed_batch, string_embed_params, string_embed_poses, trimolecular_groups_batch)
from .utils import (TriangleError, cartesian_product, get_double_bonds_indices, molecule_check, polygonize,  # noqa: F401
                    scramble_check)
from .graph_manipulations import (bond_graph_batch, bond_tables, covalent_radii, d_min_bond, double_bonds_batch,  # noqa: F401
                                  edges_from_bits, graphize, molecule_check_mask, pack_edges, scramble_mask)
from .nci import NCI_DICT, differential_nci, get_nci, interactions_of, nci_batch, nci_tables  # noqa: F401
from .reactive_atoms import (ORB_DIM_DICT, ReactiveMolecule, atom_type, orbital_recipes, orbitals_batch,  # noqa: F401
                             reactive_molecule)
from .multiembed import MultiembedResult, multiembed_batch  # noqa: F401
from .engine import Engine, FragmentSet, device_count, get_engine  # noqa: F401
from .install import install, uninstall  # noqa: F401
from .numba_functions import (_get_tf_mat, compenetration_check, compenetration_mask, count_clashes, get_torsion_fingerprint,  # noqa: F401
                              prune_conformers_tfd, prune_conformers_tfd_batch, tfd_similarity)
from .optimization_methods import (_score_embed_poses, fitness_check, fitness_mask, get_inertia_moments,  # noqa: F401
                                   get_moi_similarity_matches, prune_by_moment_of_inertia, prune_by_moment_of_inertia_batch,
                                   similarity_refining_batch)
from .torsion_module import (clustered_csearch_batch, clustered_csearch_step, csearch_augmentation_batch, csearch_batch, csearch_candidates, csearch_candidates_multi,  # noqa: F401
                             csearch_rotate, csearch_rotate_multi, diverse_select, diverse_select_batch, group_torsions_batch, hydrogen_bonds_batch, torsion_sets_batch, most_diverse_conformers, most_diverse_conformers_batch, rotate_dihedral, rotate_dihedral_batch,
                             torsion_comp_check)
from .hypermolecule_class import align_structures  # noqa: F401
from .kmeans import kmeans_lloyd, kmeans_plusplus_rows  # noqa: F401
from .rot_corr import (last_rot_corr_batch_stats, last_rot_corr_stats, prune_conformers_rmsd_rot_corr,  # noqa: F401
                       prune_rmsd_rot_corr_arrays, prune_rmsd_rot_corr_arrays_batch, rot_corr_pairs)
from .rmsd_pruning import (_rmsd_similarity, last_prune_batch_stats, last_prune_stats, pack_heavy_batch, prune_conformers_rmsd,  # noqa: F401
                           prune_conformers_rmsd_batch, rmsd_and_max_numba)
from .rmsd_cross import assign_to_kept, nearest_structures, prune_conformers_rmsd_against, rmsd_matrix, rmsd_similarity_mask  # noqa: F401
from .rmsd_ordered import leader_clusters, prune_conformers_rmsd_ordered  # noqa: F401

__version__ = "0.1.0"
