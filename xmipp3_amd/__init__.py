"""xmipp3_amd -- MI355X-native projection matching + Fourier gridding (Xmipp hot path).

The product is libxmipp_hip.so (hand-written HIP for gfx950 behind the C ABI of
include/xmipp_hip.h).  This package is the thin Python host side used by the tests and
bench.py: torch supplies device memory, streams and torch.distributed; every numerical step
runs in the HIP library.  There is no CPU fallback: importing works anywhere, but creating
a Context without the built library or without a gfx950 device raises.
"""
from ._lib import XhError, lib, lib_path  # noqa: F401
from .api import (AlignSignificant, AngularSphAlignment, asa_stage_active, ForwardArtZernike3D, faz_sort_orthogonal, faz_save_schedule, ContinuousAssign2, Context, CtfOps, FindSymmetry, fsym_axis_matrices, fsym_grid, fsym_helical_depth, fsym_helical_gate, FSO, fso_cone, fso_decide, fso_directions, fso_incomplete_gamma, fso_resolution_distribution, fso_unit_vectors, HalvesRestoration, halves_binary_mask, halves_circular_mask, halves_cylinder_mask, halves_tube_mask, LocalDeblur, ldb_bands, MonoRes, mono_cliff_radius, mono_icdf_gauss, mono_num_shells, mono_resolution_sweep, powell_minimize, powell_minimize_batch, ShiftCorrEstimator, SubtractProjection, Symmetrize, sym_helical_depth, sub_choose, sub_fit, sub_freq_map, VolumeAlign, valign_trials, VolumeDeformSph, VolumeSubtraction, vsub_radial_bins, vds_normalize_robust, vds_num_terms, vds_terms, vds_zsh, apply_geometry2d, correlation_merit, extrema_find, iterative_alignment, rotation_estimate, CtfParams, Fft2D, FlexAlign, FourierProjector, ProjectionMatcher, RealSpaceProjector, RecFourier, RecFourier2, ReconstructSignificant, ReconstructWbp, PsdEstimator, psd_patches, psd_pieces, psd_strip, wbp_even_distribution, wbp_image_matrices, wbp_nearest_direction, wbp_tile, search5d_offsets, shard_range,  # noqa: F401
                  allreduce_reconstruction, debug_fft_lines, fa_correlate, frc_dpr, movie_bin_frame, movie_binned_size, movie_dose_filter, movie_frames_to_float, reduce_reconstructions)
