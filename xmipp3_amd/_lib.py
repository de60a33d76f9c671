"""ctypes loader for libxmipp_hip.so (C ABI: include/xmipp_hip.h). Fails loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class XhError(RuntimeError):
    pass


def lib_path():
    # XMIPP_HIP_LIB: another build of the same library (A/B measurements of kernel variants on one box)
    return os.environ.get("XMIPP_HIP_LIB") or os.path.join(_HERE, "libxmipp_hip.so")


class RfParams(C.Structure):
    _fields_ = [("imgSize", C.c_int32), ("padding_proj", C.c_double), ("padding_vol", C.c_double),
                ("max_resolution", C.c_double), ("blob_radius", C.c_double),
                ("blob_order", C.c_int32), ("blob_alpha", C.c_double), ("use_fast", C.c_int32),
                ("phase_flipped", C.c_int32), ("min_ctf", C.c_double), ("sampling", C.c_double)]


class CtfParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "Tm", "kV", "DeltafU", "DeltafV", "azimuthal_angle", "Cs", "Ca", "espr", "ispr", "alpha",
        "DeltaF", "DeltaR", "Q0", "K", "envR0", "envR1", "envR2", "phase_shift", "VPP_radius")]


class MonoParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("sampling", "minRes", "maxRes", "freq_step", "significance")] + [("gaussian", C.c_int32),
                                                                                                           ("noise_only_in_halves", C.c_int32)]


class MonoStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("NS", "NN", "sumS", "sumS2", "sumN", "sumN2", "meanS", "sdS2", "meanN", "sdN2", "thr95")]


class MonoStep(C.Structure):
    _fields_ = [("stats", MonoStats)] + [(n, C.c_double) for n in ("resolution", "freq", "freqH", "freqL", "threshold", "z", "max_meanS")] + [
        ("assigned", C.c_int32), ("pad_", C.c_int32)]


class LdbIter(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("norm", "porc", "subst", "lambda_")] + [("stop", C.c_int32), ("pad_", C.c_int32)]


class VsubEnergy(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("amplitude", "minmax", "mask", "phase", "nonneg", "scale", "filter")]


class Ca2Params(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "max_shift", "max_scale", "max_angular_change", "max_defocus_change", "max_resolution", "max_gray_scale", "max_gray_shift",
        "sampling", "Rmax", "padding")] + [(n, C.c_int32) for n in (
            "optimize_gray", "optimize_shift", "optimize_scale", "optimize_angles", "optimize_defocus", "phase_flipped", "same_defocus")]


class Ca2Row(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("rot", "tilt", "psi", "shift_x", "shift_y", "scale_x", "scale_y", "scale_angle", "gray_a",
                                          "gray_b")] + [("flip", C.c_int32), ("has_ctf", C.c_int32), ("ctf", CtfParams)]


class AsaParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("max_shift", "max_angular_change", "max_resolution", "sampling", "Rmax", "RDef", "lambda_")] + [
        (n, C.c_int32) for n in ("l1", "l2", "optimize_alignment", "optimize_deformation", "optimize_defocus", "phase_flipped")]


class AsaRow(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("rot", "tilt", "psi", "shift_x", "shift_y")] + [("flip", C.c_int32), ("has_ctf", C.c_int32),
                                                                                          ("ctf", CtfParams)]


class FazParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("RDef", "sampling", "lambda_", "ltv", "ltk", "ll1", "lst")] + [
        (n, C.c_int32) for n in ("l1", "l2", "step", "use_zernike", "use_ctf", "phase_flipped")]


class FazRow(C.Structure):
    _fields_ = AsaRow._fields_


class SubParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("sampling", "max_resolution", "padding", "cirmaskrad")] + [
        (n, C.c_int32) for n in ("subtract", "real_space", "ignore_ctf", "boost", "non_negative", "pad_")]


class SubRow(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("rot", "tilt", "psi", "shift_x", "shift_y")] + [("has_ctf", C.c_int32), ("pad_", C.c_int32),
                                                                                          ("ctf", CtfParams)]


class SubResult(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("R2adj", "beta0", "beta1", "b", "beta00", "R20adj")] + [
        (n, C.c_int32) for n in ("model", "disable", "enabled", "pad_")]


# every symbol include/xmipp_hip.h declares: name -> (restype, argtypes)
vp, i32, i64, d, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_size_t
pvp = C.POINTER(C.c_void_p)
# xh_cost_fn: double (*)(double *x, void *user), x read 1-based
COST_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_void_p)
# xh_batch_cost_fn: int32 (*)(int32 m, const int32 *problem, const double *x, double *cost, void *user)
BATCH_COST_FN = C.CFUNCTYPE(C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
SIGNATURES = {
    "xh_last_error": (C.c_char_p, []),
    "xh_version": (C.c_char_p, []),
    "xh_ctx_create": (C.c_int, [C.c_int, vp, pvp]),
    "xh_ctx_create_private": (C.c_int, [C.c_int, pvp]),
    "xh_ctx_destroy": (C.c_int, [vp]),
    "xh_ctx_sync": (C.c_int, [vp]),
    "xh_ctx_stream": (vp, [vp]),
    "xh_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "xh_device_numa_node": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "xh_malloc": (C.c_int, [vp, sz, pvp]),
    "xh_free": (C.c_int, [vp, vp]),
    "xh_memset": (C.c_int, [vp, vp, C.c_int, sz]),
    "xh_memcpy_h2d": (C.c_int, [vp, vp, vp, sz]),
    "xh_memcpy_d2h": (C.c_int, [vp, vp, vp, sz]),
    "xh_device_bytes_held": (C.c_int, [C.POINTER(C.c_int64)]),
    "xh_host_alloc": (C.c_int, [vp, sz, pvp]),
    "xh_host_free": (C.c_int, [vp, vp]),
    "xh_memcpy_h2d_async": (C.c_int, [vp, vp, vp, sz]),
    "xh_memcpy_d2h_async": (C.c_int, [vp, vp, vp, sz]),
    "xh_ctx_wait_for": (C.c_int, [vp, vp]),
    "xh_timer_create": (C.c_int, [vp, pvp]),
    "xh_timer_start": (C.c_int, [vp, vp]),
    "xh_timer_stop": (C.c_int, [vp, vp]),
    "xh_timer_elapsed_ms": (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
    "xh_timer_destroy": (C.c_int, [vp, vp]),
    "xh_ctf_defaults": (None, [C.POINTER(CtfParams)]),
    "xh_rf_create": (C.c_int, [vp, C.POINTER(RfParams), pvp]),
    "xh_rf_destroy": (C.c_int, [vp]),
    "xh_rf_set_option": (C.c_int, [vp, C.c_char_p, d]),
    "xh_rf_sizes": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "xh_rf_tables": (C.c_int, [vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "xh_rf_temp_floats": (sz, [vp]),
    "xh_rf_attach_temp": (C.c_int, [vp, vp]),
    "xh_rf_temp_ptr": (C.c_int, [vp, pvp]),
    "xh_rf_reset": (C.c_int, [vp]),
    "xh_rf_shift_images": (C.c_int, [vp, vp, vp, vp, i32, vp]),
    "xh_rf_shift_images_coefs": (C.c_int, [vp, vp, vp, vp, vp, i32, vp]),
    "xh_rf_prepare_images": (C.c_int, [vp, vp, i32, vp]),
    "xh_rf_ctf_arrays": (C.c_int, [vp, C.POINTER(CtfParams), i32, vp, vp]),
    "xh_rf_insert": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, vp, i32]),
    "xh_rf_insert_images": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, i32]),
    "xh_rf_insert_images_dev": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, i32]),
    "xh_rf_shift_images_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, vp]),
    "xh_rf_insert_matrices": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, vp, i32]),
    "xh_rf_mirror_and_crop": (C.c_int, [vp]),
    "xh_rf_cropped_floats": (sz, [vp]),
    "xh_rf_cropped_export": (C.c_int, [vp, vp]),
    "xh_rf_cropped_import": (C.c_int, [vp, vp, i32]),
    "xh_rf_reduce": (C.c_int, [pvp, i32]),
    "xh_rf_finish": (C.c_int, [vp, vp]),
    "xh_rf2_create": (C.c_int, [vp, C.POINTER(RfParams), i32, pvp]),
    "xh_rf2_destroy": (C.c_int, [vp]),
    "xh_rf2_reset": (C.c_int, [vp]),
    "xh_rf2_insert": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, i32, i32]),
    "xh_rf2_weights_step": (C.c_int, [vp, i32]),
    "xh_rf2_state_doubles": (sz, [vp]),
    "xh_rf2_state_export": (C.c_int, [vp, vp]),
    "xh_rf2_state_import": (C.c_int, [vp, vp, i32]),
    "xh_rf2_finish": (C.c_int, [vp, vp]),
    "xh_fa_create": (C.c_int, [vp, i32, i32, C.c_float, C.c_float, pvp]),
    "xh_fa_destroy": (C.c_int, [vp]),
    "xh_fa_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(d)]),
    "xh_fa_set_option": (C.c_int, [vp, C.c_char_p, d]),
    "xh_fa_last_full_pairs": (C.c_int, [vp]),
    "xh_fa_global_alignment": (C.c_int, [vp, vp, i32, vp, vp, C.c_float, vp, vp, vp, vp, C.POINTER(i32)]),
    "xh_fa_local_alignment": (C.c_int, [vp, vp, i32, vp, vp, vp, vp, i32, C.c_float, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "xh_extrema_find": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, C.c_float, vp, vp]),
    "xh_shiftcorr_create": (C.c_int, [vp, i32, i32, i32, pvp]),
    "xh_shiftcorr_destroy": (C.c_int, [vp]),
    "xh_shiftcorr_load_reference": (C.c_int, [vp, vp]),
    "xh_shiftcorr_correlate": (C.c_int, [vp, vp, vp, i32, i32, i32, i32]),
    "xh_shiftcorr_compute_shifts": (C.c_int, [vp, vp, i32, vp]),
    "xh_apply_geometry2d": (C.c_int, [vp, vp, i32, i32, i32, vp, vp]),
    "xh_correlation_merit": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "xh_iterative_alignment": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "xh_align_sig_create": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, i32, pvp]),
    "xh_align_sig_destroy": (C.c_int, [vp]),
    "xh_align_sig_load_references": (C.c_int, [vp, vp, i32]),
    "xh_align_sig_align": (C.c_int, [vp, vp, i32, vp, vp]),
    "xh_align_sig_weights": (C.c_int, [vp, vp, vp, d, vp, i32, i32, vp]),
    "xh_align_sig_update_refs": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "xh_rsig_create": (C.c_int, [vp, i32, i32, i32, pvp]),
    "xh_rsig_destroy": (C.c_int, [vp]),
    "xh_rsig_load_gallery": (C.c_int, [vp, vp, i32]),
    "xh_rsig_align": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "xh_rsig_weights": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp, vp, d, d, i32, i32, i32, d, vp]),
    "xh_rsig_stats": (C.c_int, [vp, vp]),
    "xh_rsig_set_timing": (C.c_int, [vp, i32]),
    "xh_halves_create": (C.c_int, [vp, i32, i32, i32, pvp]),
    "xh_halves_destroy": (C.c_int, [vp]),
    "xh_halves_load": (C.c_int, [vp, vp, vp]),
    "xh_halves_denoise": (C.c_int, [vp, i32, vp]),
    "xh_halves_deconvolve": (C.c_int, [vp, i32, d, d, vp]),
    "xh_halves_filter_bank": (C.c_int, [vp, d, d, i32, d]),
    "xh_halves_difference": (C.c_int, [vp, i32, d, vp]),
    "xh_halves_output": (C.c_int, [vp, i32, vp, C.POINTER(C.c_int32)]),
    "xh_halves_deconv_spectra": (C.c_int, [vp]),
    "xh_halves_sigma_cost": (C.c_int, [vp, d, d, C.POINTER(C.c_double)]),
    "xh_halves_fft_r2c": (C.c_int, [vp, vp, vp]),
    "xh_halves_fft_c2r": (C.c_int, [vp, vp, vp, d]),
    "xh_halves_cdf": (C.c_int, [vp, vp, vp, vp, d, vp]),
    "xh_halves_set_timing": (C.c_int, [vp, i32]),
    "xh_halves_band_timing": (C.c_int, [vp, C.POINTER(C.c_int32), vp]),
    "xh_halves_circular_mask": (C.c_int, [i32, i32, i32, d, d, d, d, vp]),
    "xh_halves_binary_mask": (C.c_int, [vp, sz, vp]),
    "xh_mono_defaults": (None, [vp]),
    "xh_mono_icdf_gauss": (C.c_int, [d, C.POINTER(C.c_double)]),
    "xh_mono_resolution2eval": (C.c_int, [C.POINTER(i32), d, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(i32), i32, C.POINTER(i32), C.POINTER(i32), d, d]),
    "xh_mono_cliff_radius": (C.c_int, [vp, vp, vp, i32, i32, i32, C.POINTER(i32)]),
    "xh_mono_num_shells": (C.c_int, [i32, i32, i32, C.POINTER(i32)]),
    "xh_mono_create": (C.c_int, [vp, i32, i32, i32, pvp]),
    "xh_mono_destroy": (C.c_int, [vp]),
    "xh_mono_run": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32), vp, vp, vp, vp]),
    "xh_mono_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32)]),
    "xh_mono_amplitude": (C.c_int, [vp, vp, d, d, d, i32, vp]),
    "xh_mono_gaussian": (C.c_int, [vp, vp, d]),
    "xh_mono_statistics": (C.c_int, [vp, vp, vp, vp, d, vp]),
    "xh_mono_select": (C.c_int, [vp, vp, vp, sz, sz, C.POINTER(C.c_double)]),
    "xh_mono_assign": (C.c_int, [vp, vp, vp, vp, sz, d, d, d, i32]),
    "xh_mono_shell_sums": (C.c_int, [vp, vp, vp, vp, vp]),
    "xh_mono_set_timing": (C.c_int, [vp, i32]),
    "xh_mono_stage_ms": (C.c_int, [vp, vp]),
    "xh_ldb_bands": (C.c_int, [i32, d, d, vp, i32, C.POINTER(i32)]),
    "xh_ldb_create": (C.c_int, [vp, i32, i32, i32, i32, pvp]),
    "xh_ldb_destroy": (C.c_int, [vp]),
    "xh_ldb_load": (C.c_int, [vp, vp, vp, d, d]),
    "xh_ldb_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i32), vp, i32]),
    "xh_ldb_resmap": (C.c_int, [vp, vp]),
    "xh_ldb_localfilter": (C.c_int, [vp, vp, vp]),
    "xh_ldb_run": (C.c_int, [vp, d, i32, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double), vp]),
    "xh_ldb_set_timing": (C.c_int, [vp, i32]),
    "xh_ldb_stage_ms": (C.c_int, [vp, vp]),
    "xh_fso_directions": (C.c_int, [i32, vp, i32, C.POINTER(i32)]),
    "xh_fso_unit_vectors": (C.c_int, [vp, i32, vp]),
    "xh_fso_incomplete_gamma": (C.c_double, [d]),
    "xh_fso_cone": (C.c_int, [d, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "xh_fso_decide": (C.c_int, [vp, vp, i32, i32, i32, d, d, vp, vp, vp, vp]),
    "xh_fso_resolution_distribution": (C.c_int, [vp, i32, vp, d, vp]),
    "xh_fso_create": (C.c_int, [vp, i32, i32, i32, i32, pvp]),
    "xh_fso_destroy": (C.c_int, [vp]),
    "xh_fso_load": (C.c_int, [vp, vp, vp, vp, vp, vp, C.POINTER(i64)]),
    "xh_fso_info": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "xh_fso_layout": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "xh_fso_directional": (C.c_int, [vp, vp, i32, C.c_float, C.c_float, vp, vp]),
    "xh_fso_threedfsc": (C.c_int, [vp, vp, i32, C.c_float, C.c_float, vp, vp, vp]),
    "xh_fso_set_timing": (C.c_int, [vp, i32]),
    "xh_fso_stage_ms": (C.c_int, [vp, vp]),
    "xh_vsub_radial_bins": (C.c_int, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "xh_vsub_create": (C.c_int, [vp, i32, i32, i32, pvp]),
    "xh_vsub_destroy": (C.c_int, [vp]),
    "xh_vsub_set_reference": (C.c_int, [vp, vp, vp, i32]),
    "xh_vsub_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)]),
    "xh_vsub_reference_magnitude": (C.c_int, [vp, vp]),
    "xh_vsub_radial_mean": (C.c_int, [vp, vp, vp]),
    "xh_vsub_quotient": (C.c_int, [vp, vp, vp]),
    "xh_vsub_iteration": (C.c_int, [vp, vp, vp, d, i32, d, vp]),
    "xh_vsub_adjust": (C.c_int, [vp, vp, i32, d, i32, d, vp, vp]),
    "xh_vsub_lowpass": (C.c_int, [vp, vp, d, vp]),
    "xh_vsub_smooth_mask": (C.c_int, [vp, vp, d, vp]),
    "xh_vsub_subtract": (C.c_int, [vp, vp, vp, vp, d, vp, vp]),
    "xh_vsub_set_timing": (C.c_int, [vp, i32]),
    "xh_vsub_stage_ms": (C.c_int, [vp, vp]),
    "xh_sym_create": (C.c_int, [vp, i32, i32, i32, pvp]),
    "xh_sym_destroy": (C.c_int, [vp]),
    "xh_sym_set_matrices": (C.c_int, [vp, vp, i32]),
    "xh_sym_symmetrize": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "xh_sym_symmetrize_images": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "xh_sym_helical": (C.c_int, [vp, vp, d, d, d, i32, i32, d, i32, vp]),
    "xh_sym_helical_depth": (C.c_int, [i32, d, d, i32, C.POINTER(i32)]),
    "xh_sym_apply_geometry3d": (C.c_int, [vp, vp, vp, i32, i32, d, vp]),
    "xh_sym_coefficients": (C.c_int, [vp, vp, vp]),
    "xh_sym_outside_mean": (C.c_int, [vp, vp, C.POINTER(C.c_double)]),
    "xh_sym_set_timing": (C.c_int, [vp, i32]),
    "xh_sym_stage_ms": (C.c_int, [vp, vp]),
    "xh_valign_create": (C.c_int, [vp, i32, i32, i32, i32, pvp]),
    "xh_valign_destroy": (C.c_int, [vp]),
    "xh_valign_set_volumes": (C.c_int, [vp, vp, vp, vp]),
    "xh_valign_stats": (C.c_int, [vp, vp]),
    "xh_valign_matrix": (C.c_int, [vp, vp, vp, C.POINTER(i32)]),
    "xh_valign_trials": (C.c_int, [vp, i32, i64, vp, C.POINTER(i64), C.POINTER(i64)]),
    "xh_valign_fit": (C.c_int, [vp, vp, i64, i32, i32, vp]),
    "xh_valign_search": (C.c_int, [vp, vp, i64, i32, i32, C.POINTER(i64), C.POINTER(C.c_double), vp]),
    "xh_valign_apply": (C.c_int, [vp, vp, i32, vp]),
    "xh_valign_set_timing": (C.c_int, [vp, i32]),
    "xh_valign_stage_ms": (C.c_int, [vp, vp]),
    "xh_fsym_create": (C.c_int, [vp, i32, i32, i32, i32, pvp]),
    "xh_fsym_destroy": (C.c_int, [vp]),
    "xh_fsym_set_volume": (C.c_int, [vp, vp, vp, i32]),
    "xh_fsym_stats": (C.c_int, [vp, i32, vp]),
    "xh_fsym_axis_matrices": (C.c_int, [d, d, i32, vp, vp]),
    "xh_fsym_grid": (C.c_int, [d, d, d, d, d, d, i64, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
    "xh_fsym_helical_gate": (C.c_int, [i32, d, d, d, d, d, d, C.POINTER(i32)]),
    "xh_fsym_helical_depth": (C.c_int, [i32, d, d, i32, C.POINTER(i32)]),
    "xh_fsym_axis_fit": (C.c_int, [vp, vp, i64, i32, vp]),
    "xh_fsym_axis_search": (C.c_int, [vp, vp, i64, i32, C.POINTER(i64), C.POINTER(C.c_double), vp]),
    "xh_fsym_helical_fit": (C.c_int, [vp, vp, i64, vp, i32, d, i32, vp]),
    "xh_fsym_helical_search": (C.c_int, [vp, vp, i64, vp, i32, d, i32, C.POINTER(i64), C.POINTER(C.c_double), vp]),
    "xh_fsym_axis_volume": (C.c_int, [vp, d, d, i32, vp]),
    "xh_fsym_helical_volume": (C.c_int, [vp, d, d, i32, d, i32, vp]),
    "xh_fsym_set_timing": (C.c_int, [vp, i32]),
    "xh_fsym_stage_ms": (C.c_int, [vp, vp]),
    "xh_wbp_create": (C.c_int, [vp, i32, i32, pvp]),
    "xh_wbp_destroy": (C.c_int, [vp]),
    "xh_wbp_reset": (C.c_int, [vp]),
    "xh_wbp_set_directions": (C.c_int, [vp, vp, i32, d, i32]),
    "xh_wbp_add": (C.c_int, [vp, vp, vp, i32, vp]),
    "xh_wbp_finish": (C.c_int, [vp, vp, i32]),
    "xh_wbp_volume": (C.c_int, [vp, vp]),
    "xh_wbp_count_thr": (C.c_int, [vp, C.POINTER(i64)]),
    "xh_wbp_weights": (C.c_int, [vp, vp, vp]),
    "xh_wbp_table": (C.c_int, [vp, vp, C.POINTER(i64)]),
    "xh_wbp_tile": (C.c_int, []),
    "xh_wbp_image_matrices": (C.c_int, [d, d, d, vp, vp, vp]),
    "xh_wbp_even_distribution": (C.c_int, [d, vp, vp, i32, C.POINTER(i32)]),
    "xh_wbp_nearest_direction": (C.c_int, [d, d, vp, vp, i32, C.POINTER(i32)]),
    "xh_wbp_set_timing": (C.c_int, [vp, i32]),
    "xh_wbp_stage_ms": (C.c_int, [vp, vp]),
    "xh_psd_create": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, pvp]),
    "xh_psd_destroy": (C.c_int, [vp]),
    "xh_psd_load": (C.c_int, [vp, vp]),
    "xh_psd_add": (C.c_int, [vp, vp, i32, i32, vp]),
    "xh_psd_result": (C.c_int, [vp, vp, vp, C.POINTER(i64)]),
    "xh_psd_reset": (C.c_int, [vp]),
    "xh_psd_smoother": (C.c_int, [vp, vp]),
    "xh_psd_piece": (C.c_int, [vp, vp, i32, i32, vp]),
    "xh_psd_strip": (C.c_int, []),
    "xh_psd_set_timing": (C.c_int, [vp, i32]),
    "xh_psd_stage_ms": (C.c_int, [vp, vp]),
    "xh_psd_pieces": (C.c_int, [i32, i32, i32, d, i32, i32, vp, i32, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]),
    "xh_psd_patches": (C.c_int, [i32, i32, i32, i32, i32, i32, C.c_float, vp, i32, C.POINTER(i32)]),
    "xh_halves_cylinder_mask": (C.c_int, [i32, i32, i32, d, d, d, d, d, vp]),
    "xh_halves_tube_mask": (C.c_int, [i32, i32, i32, d, d, d, d, d, d, vp]),
    "xh_powell_minimize": (C.c_int, [i32, vp, vp, d, COST_FN, vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "xh_powell_minimize_batch": (C.c_int, [i32, vp, i32, vp, vp, d, i32, BATCH_COST_FN, vp, vp, vp, vp]),
    "xh_ca2_defaults": (None, [C.POINTER(Ca2Params)]),
    "xh_ca2_create": (C.c_int, [vp, vp, i32, C.POINTER(Ca2Params), i32, pvp]),
    "xh_ca2_destroy": (C.c_int, [vp]),
    "xh_ca2_load": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "xh_ca2_cost": (C.c_int, [vp, i32, vp, vp, vp]),
    "xh_ca2_last_images": (C.c_int, [vp, i32, vp, vp, vp]),
    "xh_ca2_measures": (C.c_int, [vp, i32, vp]),
    "xh_ca2_apply": (C.c_int, [vp, vp, vp, vp]),
    "xh_ca2_filtered": (C.c_int, [vp, i32, vp, C.POINTER(C.c_double)]),
    "xh_ca2_refine": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "xh_ca2_stats": (C.c_int, [vp, vp]),
    "xh_vds_num_terms": (C.c_int, [i32, i32, C.POINTER(i32)]),
    "xh_vds_terms": (C.c_int, [i32, i32, vp]),
    "xh_vds_zsh": (C.c_int, [i32, i32, i32, i32, d, d, d, d, C.POINTER(C.c_double)]),
    "xh_vds_normalize_robust": (C.c_int, [vp, sz, d]),
    "xh_vds_create": (C.c_int, [vp, i32, i32, i32, i32, i32, d, d, pvp]),
    "xh_vds_destroy": (C.c_int, [vp]),
    "xh_vds_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(C.c_double)]),
    "xh_vds_gauss": (C.c_int, [vp, d, vp, vp]),
    "xh_vds_set_pairs": (C.c_int, [vp, i32, vp, vp]),
    "xh_vds_cost": (C.c_int, [vp, vp, vp]),
    "xh_vds_refine_stage": (C.c_int, [vp, i32, vp, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i64)]),
    "xh_vds_apply": (C.c_int, [vp, vp, vp, vp, vp]),
    "xh_vds_strain": (C.c_int, [vp, vp, vp, vp]),
    "xh_asa_defaults": (None, [C.POINTER(AsaParams)]),
    "xh_asa_stage_active": (C.c_int, [i32, i32, i32, i32, vp, C.POINTER(i32)]),
    "xh_asa_create": (C.c_int, [vp, vp, i32, vp, C.POINTER(AsaParams), i32, pvp]),
    "xh_asa_destroy": (C.c_int, [vp]),
    "xh_asa_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double)]),
    "xh_asa_load": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "xh_asa_cost": (C.c_int, [vp, i32, vp, vp, vp]),
    "xh_asa_last": (C.c_int, [vp, i32, vp, vp, vp, vp]),
    "xh_asa_refine": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
    "xh_asa_stats": (C.c_int, [vp, vp]),
    "xh_faz_defaults": (None, [C.POINTER(FazParams)]),
    "xh_faz_sort_orthogonal": (C.c_int, [i32, vp, vp, i32, vp]),
    "xh_faz_save_schedule": (C.c_int, [i32, i32, vp]),
    "xh_faz_check": (C.c_int, [i32, i32, i32]),
    "xh_faz_create": (C.c_int, [vp, i32, vp, vp, vp, vp, i32, vp, i32, C.POINTER(FazParams), pvp]),
    "xh_faz_destroy": (C.c_int, [vp]),
    "xh_faz_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "xh_faz_load": (C.c_int, [vp, vp, i32, i32, i32, vp, vp]),
    "xh_faz_sweep": (C.c_int, [vp, i32, i32, vp]),
    "xh_faz_forward": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]),
    "xh_faz_get_volume": (C.c_int, [vp, vp]),
    "xh_faz_set_volume": (C.c_int, [vp, vp]),
    "xh_faz_set_timing": (C.c_int, [vp, i32]),
    "xh_faz_stage_ms": (C.c_int, [vp, vp]),
    "xh_rsp_create": (C.c_int, [vp, vp, i32, i32, pvp]),
    "xh_rsp_destroy": (C.c_int, [vp]),
    "xh_rsp_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "xh_rsp_project": (C.c_int, [vp, vp, vp, i32, vp]),
    "xh_rsp_steps": (C.c_int, [vp, vp, vp, i32, vp]),
    "xh_sub_defaults": (None, [C.POINTER(SubParams)]),
    "xh_sub_freq_map": (C.c_int, [i32, d, d, vp, C.POINTER(i32)]),
    "xh_sub_fit": (C.c_int, [vp, i32, d, vp]),
    "xh_sub_choose": (C.c_int, [d, d, d, d, d, vp]),
    "xh_sub_create": (C.c_int, [vp, vp, i32, vp, vp, C.POINTER(SubParams), i32, pvp]),
    "xh_sub_destroy": (C.c_int, [vp]),
    "xh_sub_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double)]),
    "xh_sub_load": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "xh_sub_run": (C.c_int, [vp, vp, vp]),
    "xh_sub_last": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "xh_sub_set_timing": (C.c_int, [vp, i32]),
    "xh_sub_stage_ms": (C.c_int, [vp, vp]),
    "xh_rotation_estimate": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "xh_movie_dose_filter": (C.c_int, [vp, vp, vp, i32, i32, d, d, d, d]),
    "xh_movie_bin_frame": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, vp, i32, i32]),
    "xh_movie_crop_frames": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "xh_movie_frame_to_float": (C.c_int, [vp, vp, i32, C.c_int64, vp]),
    "xh_fa_correlate": (C.c_int, [vp, vp, i32, i32, i32, C.c_float, vp]),
    "xh_fa_local_from_global": (C.c_int, [vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "xh_fa_apply_bspline": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "xh_fa_apply_bspline_frames": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "xh_ctfop_create": (C.c_int, [vp, i32, i32, d, pvp]),
    "xh_ctfop_destroy": (C.c_int, [vp]),
    "xh_ctfop_phase_flip": (C.c_int, [vp, vp, C.POINTER(CtfParams), d]),
    "xh_ctfop_wiener2d": (C.c_int, [vp, vp, i32, vp, d, i32, i32, d, i32]),
    "xh_pm_create": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, i32, pvp]),
    "xh_pm_destroy": (C.c_int, [vp]),
    "xh_pm_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "xh_pm_match": (C.c_int, [vp, vp, i32, vp, vp, i32, vp, vp, vp]),
    "xh_frc_dpr": (C.c_int, [vp, vp, vp, i32, i32, i32, d, i32, i32, d, d, vp, vp, vp, vp, vp, vp]),
    "xh_rf_kernel_ms": (C.c_int, [vp, vp, vp, i32]),
    "xh_fft2d_create": (C.c_int, [vp, i32, i32, pvp]),
    "xh_fft2d_destroy": (C.c_int, [vp]),
    "xh_fft2d_factors": (C.c_int, [vp, vp]),
    "xh_fft2d_exec": (C.c_int, [vp, vp, i32]),
    "xh_fft2d_exec_axis": (C.c_int, [vp, vp, i32, i32]),
    "xh_debug_fft_lines": (C.c_int, [vp, i32, i32, vp, sz, sz, sz, sz, sz, i32, i32]),
    "xh_fft2d_debug_real_rows": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "xh_fp_create": (C.c_int, [vp, vp, i32, C.c_double, C.c_double, i32, pvp]),
    "xh_fp_destroy": (C.c_int, [vp]),
    "xh_fp_info": (C.c_int, [vp, vp, vp, vp]),
    "xh_fp_coefs": (C.c_int, [vp, vp, vp]),
    "xh_fp_project": (C.c_int, [vp, vp, i32, vp, vp]),
    "xh_pm_match_ex": (C.c_int, [vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "xh_pm_translate": (C.c_int, [vp, vp, i32, vp, vp, vp, d, vp, vp, vp]),
    "xh_pm_last_stats": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
    "xh_pm_translate_stats": (C.c_int, [vp, C.POINTER(i64)]),
    "xh_pm_last_coefficients": (C.c_int, [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]),
    "xh_pm_stage_ms": (C.c_int, [vp, vp, i32]),
    "xh_pm_rows_pruned": (C.c_int, [vp, vp]),
    "xh_pm_two_level_cut": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32)]),
    "xh_pm_set_option": (C.c_int, [vp, C.c_char_p, d]),
    "xh_pm_debug_prepare": (C.c_int, [vp, vp, i32, i32, vp, vp]),
    "xh_pm_debug_ref": (C.c_int, [vp, i32, vp, vp]),
    "xh_pm_debug_corr_rows": (C.c_int, [vp, vp, i32, i32, vp]),
    "xh_pm_debug_s6_maps": (C.c_int, [vp, i32, vp]),
    "xh_pm_get_option": (C.c_int, [vp, C.c_char_p, C.POINTER(d)]),
}


def lib():
    """Load the HIP library; raise XhError if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch bundles its own HIP runtime; load it first so that this process ends up with ONE
    # libamdhip64 (ours would otherwise pull /opt/rocm's next to torch's and lose the device)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path()
    if not os.path.exists(path):
        raise XhError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(xmipp3_amd/csrc/build.sh). There is no CPU fallback.")
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise XhError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            f = getattr(L, name)
        except AttributeError as e:
            raise XhError(f"{path} does not export {name}") from e
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def check(rc):
    if rc != 0:
        raise XhError(f"xmipp_hip error {rc}: {lib().xh_last_error().decode()}")
