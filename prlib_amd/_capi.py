"""ctypes binding of libprlib_hip.so — the C ABI declared in include/prl_hip.h.

This module only marshals pointers, sizes and strides.  It never computes: if the shared library
is missing it raises, and if no gfx950 device is usable the library itself returns
PRL_ERR_NO_DEVICE.  There is no CPU fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libprlib_hip.so")
# the same library built with -DPRL_TEST_HOOKS (`make -C prlib_amd/csrc hooks`): reads the PRL_HIP_* tuning knobs; loaded only
# by tests / tools that call use_library(HOOKS_LIB_PATH) before their first call
HOOKS_LIB_PATH = os.path.join(_HERE, "libprlib_hip_testhooks.so")


def use_library(path: str) -> None:
    """Load another build of the library (tests: the hooks build; tools: A/B of kernel experiments).  Before the first call."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("the library is already loaded")
    LIB_PATH = os.path.abspath(path)

PRL_OK = 0
PRL_ERR_EMPTY = 1
PRL_ERR_BAD_WINDOW = 2
PRL_ERR_BAD_CHANNELS = 3
PRL_ERR_EMPTY_RECT = 4
PRL_ERR_BAD_ARG = 5
PRL_ERR_NO_DEVICE = 6
PRL_ERR_HIP = 7
PRL_ERR_NOMEM = 8
PRL_ERR_LITERAL_BUDGET = 9
PRL_ERR_UNSUPPORTED = 10

SAUVOLA, NIBLACK, WOLFJOLION, NICK, FENG = range(5)
MODE_AUTO, MODE_LITERAL = 0, 1

# every symbol include/prl_hip.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = [
    "prl_hip_abi_version", "prl_hip_strerror", "prl_hip_last_error_detail", "prl_hip_device_count",
    "prl_hip_set_device", "prl_hip_set_exec_mode", "prl_hip_get_exec_mode", "prl_hip_last_stats",
    "prl_hip_release_workspace", "prl_hip_set_profiling", "prl_hip_last_kernel_ms", "prl_hip_last_call_ms", "prl_hip_set_deferred_completion", "prl_hip_finish", "prl_hip_default_params", "prl_hip_binarize_geometry",
    "prl_hip_binarize_batch_device", "prl_hip_binarize_pages_device", "prl_hip_binarize_host",
    "prl_hip_morph_batch_device", "prl_hip_nlm_planes_device", "prl_hip_denoise_batch_device",
    "prl_hip_denoise_host", "prl_hip_thin_batch_device", "prl_hip_thin_host",
    "prl_hip_bgr2gray_batch_device", "prl_hip_gray2bgr_batch_device", "prl_hip_invert_batch_device",
    "prl_hip_default_chain_params", "prl_hip_chain_batch_device",
    "prl_hip_bgnorm_out_channels", "prl_hip_bgnorm_batch_device", "prl_hip_bgnorm_host",
    "prl_hip_rotate_out_size", "prl_hip_rotate_batch_device", "prl_hip_houghp_device", "prl_hip_deskew_batch_device",
    "prl_hip_rotate_host", "prl_hip_deskew_host", "prl_hip_find_angle_batch_device", "prl_hip_find_angle_host", "prl_hip_last_deskew_stats", "prl_hip_reset_deskew_stats", "prl_hip_set_literal_page_budget", "prl_hip_get_literal_page_budget", "prl_hip_chain_max_out_size", "prl_hip_chain_pages_device",
    "prl_hip_binarize_batch_host", "prl_hip_page_range", "prl_hip_binarize_lv_batch_device", "prl_hip_binarize_lv_host",
    "prl_hip_chain_batch_host", "prl_hip_alloc_host", "prl_hip_free_host", "prl_hip_host_register", "prl_hip_host_unregister",
    "prl_hip_median_batch_device", "prl_hip_median_host",
    "prl_hip_adaptive_threshold_batch_device", "prl_hip_adaptive_threshold_host", "prl_hip_default_adaptive_params",
    "prl_hip_binarize_adaptive_batch_device", "prl_hip_binarize_adaptive_host",
    "prl_hip_morphology_batch_device", "prl_hip_morphology_host", "prl_hip_morphology_ex_batch_device", "prl_hip_morphology_ex_host",
    "prl_hip_correct_nuil_batch_device", "prl_hip_correct_nuil_host",
    "prl_hip_remove_lines_batch_device", "prl_hip_remove_lines_host",
    "prl_hip_histogram_batch_device", "prl_hip_lut_batch_device",
    "prl_hip_gamma_correction_batch_device", "prl_hip_gamma_correction_host",
    "prl_hip_simple_white_balance_batch_device", "prl_hip_simple_white_balance_host",
    "prl_hip_gray_world_batch_device", "prl_hip_gray_world_host",
    "prl_hip_clean_background_batch_device", "prl_hip_clean_background_host",
    "prl_hip_gamma_lut", "prl_hip_clean_background_lut", "prl_hip_simple_white_balance_luts", "prl_hip_gray_world_luts",
    "prl_hip_binarize_mokji_batch_device", "prl_hip_binarize_mokji_host", "prl_hip_mokji_thresholds_batch_device",
    "prl_hip_cooccurrence_batch_device", "prl_hip_mokji_threshold",
    "prl_hip_warp_crop_size", "prl_hip_perspective_transform", "prl_hip_warp_perspective_batch_device",
    "prl_hip_warp_crop_batch_device", "prl_hip_warp_crop_host",
    "prl_hip_pyr_down_size", "prl_hip_pyr_down_batch_device", "prl_hip_pyr_down_host",
    "prl_hip_canny_classes_batch_device", "prl_hip_edge_link_batch_device", "prl_hip_canny_batch_device", "prl_hip_canny_host",
    "prl_hip_document_edges_geometry", "prl_hip_document_edges_batch_device", "prl_hip_document_edges_host",
    "prl_hip_resize_pyramid_levels", "prl_hip_resize_replicate_batch_device", "prl_hip_resize_replicate_host",
    "prl_hip_find_contours", "prl_hip_approx_poly_closed", "prl_hip_document_quad", "prl_hip_document_quad_finish",
    "prl_hip_document_contour_batch_device", "prl_hip_document_contour_host",
    "prl_hip_hough_lines_geometry", "prl_hip_hough_accumulator_batch_device", "prl_hip_hough_lines_batch_device", "prl_hip_hough_lines_host",
    "prl_hip_hough_edges_batch_device", "prl_hip_hough_edges_host", "prl_hip_hough_line_quad",
    "prl_hip_hough_line_contour_batch_device", "prl_hip_hough_line_contour_host",
    "prl_hip_focus_sums_batch_device", "prl_hip_focus_measures_host", "prl_hip_focus_from_sums",
    "prl_hip_basic_deblur_batch_device", "prl_hip_basic_deblur_host", "prl_hip_gaussian_blur_f32_batch_device",
    "prl_hip_gaussian_blur_f32_host", "prl_hip_gaussian_blur_size", "prl_hip_gaussian_kernel_f32",
    "prl_hip_clahe_geometry", "prl_hip_clahe_tile_lut", "prl_hip_equalize_hist_lut", "prl_hip_clahe_luts_batch_device",
    "prl_hip_clahe_batch_device", "prl_hip_clahe_host", "prl_hip_equalize_hist_batch_device", "prl_hip_equalize_hist_host",
    "prl_hip_enhance_local_contrast_batch_device", "prl_hip_enhance_local_contrast_host",
    "prl_hip_gaussian_kernel_u8", "prl_hip_sep_filter_u8_batch_device", "prl_hip_gaussian_blur_u8_batch_device",
    "prl_hip_gaussian_blur_u8_host", "prl_hip_canny_edge_detection_batch_device", "prl_hip_canny_edge_detection_host",
    "prl_hip_external_rects", "prl_hip_rect_otsu_batch_device", "prl_hip_binarize_local_otsu_batch_device",
    "prl_hip_binarize_local_otsu_host", "prl_hip_connected_components_batch_device", "prl_hip_external_rects_batch_device",
    "prl_hip_bilateral_tables", "prl_hip_bilateral_filter_batch_device", "prl_hip_bilateral_filter_host",
    "prl_hip_variance_mask_batch_device", "prl_hip_find_contours_tree", "prl_hip_remove_children_contours", "prl_hip_fbcitb_contours",
    "prl_hip_rect_paint_batch_device", "prl_hip_default_fbcitb_params", "prl_hip_binarize_fbcitb_batch_device",
    "prl_hip_binarize_fbcitb_host",
]


class BinarizeParams(C.Structure):
    """struct prl_binarize_params."""

    _fields_ = [
        ("method", C.c_int32),
        ("window_size", C.c_int32),
        ("k", C.c_double),
        ("morph_iterations", C.c_int32),
        ("reserved0", C.c_int32),
        ("feng_alpha1", C.c_double),
        ("feng_k1", C.c_double),
        ("feng_k2", C.c_double),
        ("feng_gamma", C.c_double),
    ]


class ChainParams(C.Structure):
    """struct prl_chain_params."""

    _fields_ = [("denoise", C.c_int32), ("denoise_strength", C.c_float), ("binarize", BinarizeParams), ("thin", C.c_int32),
                ("deskew", C.c_int32), ("background_normalization", C.c_int32)]


class AdaptiveParams(C.Structure):
    """struct prl_adaptive_params."""

    _fields_ = [("median_ksize", C.c_int32), ("median_on_color", C.c_int32), ("method", C.c_int32), ("type", C.c_int32),
                ("max_value", C.c_double), ("block_size", C.c_int32), ("auto_invert", C.c_int32), ("delta", C.c_double)]


class FbcitbParams(C.Structure):
    """struct prl_fbcitb_params."""

    _fields_ = [(n, C.c_int32) for n in ("use_canny", "use_variances_map", "use_clahe", "use_bilateral", "use_other_colorspace",
                                          "use_morphology", "use_canny_on_variances", "bilateral_kernel_size")] + \
               [(n, C.c_double) for n in ("variance_map_threshold", "clahe_clip_limit", "gaussian_blur_kernel_size",
                                          "canny_upper_threshold_coeff", "canny_lower_threshold_coeff", "bounding_rectangle_max_area",
                                          "bilateral_kernel_intensity_sigma", "bilateral_kernel_spatial_sigma",
                                          "bounding_rect_max_area_coeff")]


class BinarizeGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("w", "half", "padded_w", "padded_h", "out_w", "out_h")]


class BinarizeStats(C.Structure):
    _fields_ = [
        ("pixels", C.c_uint64),
        ("refined_pixels", C.c_uint64),
        ("exact_pixels", C.c_uint64),
        ("literal_pages", C.c_uint64),
        ("wolf_candidates", C.c_uint64),
        ("exact_sweep_pages", C.c_uint64),
        ("reserved", C.c_uint64 * 2),
    ]


class PrlError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). prlib_amd has no CPU fallback.")
        # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7.  When torch is going to be used (it owns
        # the device tensors of the Python layer), it must be loaded FIRST so that this library binds to the same
        # runtime; loaded the other way round, two runtimes open the device and the second finds none.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        P = C.POINTER
        L.prl_hip_strerror.restype = C.c_char_p
        L.prl_hip_strerror.argtypes = [i]
        L.prl_hip_last_error_detail.restype = C.c_char_p
        L.prl_hip_device_count.argtypes = [P(C.c_int)]
        L.prl_hip_set_device.argtypes = [i]
        L.prl_hip_set_exec_mode.argtypes = [i]
        L.prl_hip_last_stats.argtypes = [P(BinarizeStats)]
        L.prl_hip_set_profiling.argtypes = [i]
        L.prl_hip_last_kernel_ms.argtypes = [P(C.c_float)]
        L.prl_hip_last_call_ms.argtypes = [P(C.c_float)]
        L.prl_hip_set_deferred_completion.argtypes = [i]
        L.prl_hip_alloc_host.argtypes = [sz, P(vp)]
        L.prl_hip_free_host.argtypes = [vp]
        L.prl_hip_host_register.argtypes = [vp, sz]
        L.prl_hip_host_unregister.argtypes = [vp]
        L.prl_hip_finish.argtypes = [vp]
        L.prl_hip_default_params.argtypes = [i, P(BinarizeParams)]
        L.prl_hip_binarize_geometry.argtypes = [P(BinarizeParams), i, i, P(BinarizeGeometry)]
        L.prl_hip_binarize_batch_device.argtypes = [P(BinarizeParams), i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_binarize_pages_device.argtypes = [P(BinarizeParams), i, P(vp), sz, i, i, P(vp), sz, vp]
        L.prl_hip_binarize_host.argtypes = [P(BinarizeParams), vp, sz, i, i, vp, sz, vp, sz]
        L.prl_hip_morph_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_nlm_planes_device.argtypes = [i, i, C.c_float, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_denoise_batch_device.argtypes = [i, i, C.c_float, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_denoise_host.argtypes = [i, C.c_float, vp, sz, i, i, vp, sz]
        L.prl_hip_thin_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_thin_host.argtypes = [i, vp, sz, i, i, vp, sz]
        L.prl_hip_bgr2gray_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_gray2bgr_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_invert_batch_device.argtypes = [i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_default_chain_params.argtypes = [P(ChainParams)]
        L.prl_hip_default_chain_params.restype = None
        L.prl_hip_chain_batch_device.argtypes = [P(ChainParams), i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_bgnorm_out_channels.argtypes = [i]
        L.prl_hip_bgnorm_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_bgnorm_host.argtypes = [i, vp, sz, i, i, vp, sz]
        L.prl_hip_rotate_out_size.argtypes = [i, i, C.c_double, P(C.c_int), P(C.c_int)]
        L.prl_hip_rotate_batch_device.argtypes = [i, i, vp, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_houghp_device.argtypes = [vp, sz, i, i, i, i, i, vp, i, P(C.c_int), vp]
        L.prl_hip_deskew_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp, vp, vp]
        L.prl_hip_rotate_host.argtypes = [i, C.c_double, vp, sz, i, i, vp, sz]
        L.prl_hip_deskew_host.argtypes = [i, vp, sz, i, i, vp, sz, P(C.c_int), P(C.c_int), P(C.c_double)]
        L.prl_hip_find_angle_batch_device.argtypes = [i, vp, sz, sz, i, i, vp, vp, vp]
        L.prl_hip_find_angle_host.argtypes = [vp, sz, i, i, P(C.c_double), P(C.c_int32)]
        L.prl_hip_chain_max_out_size.argtypes = [P(ChainParams), i, i, P(C.c_int), P(C.c_int)]
        L.prl_hip_chain_pages_device.argtypes = [P(ChainParams), i, i, vp, sz, sz, i, i, vp, sz, sz, vp, vp, vp]
        L.prl_hip_binarize_batch_host.argtypes = [P(BinarizeParams), i, P(vp), sz, i, i, P(vp), sz, i]
        L.prl_hip_chain_batch_host.argtypes = [P(ChainParams), i, i, P(vp), sz, i, i, P(vp), sz, vp, vp, i]
        L.prl_hip_page_range.argtypes = [i, i, i, P(C.c_int), P(C.c_int)]
        L.prl_hip_binarize_lv_batch_device.argtypes = [i, i, C.c_double, i, C.c_double, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_binarize_lv_host.argtypes = [i, C.c_double, i, C.c_double, vp, sz, i, i, vp, sz]
        L.prl_hip_median_batch_device.argtypes = [i, i, i, sz, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_median_host.argtypes = [i, i, sz, vp, sz, i, i, vp, sz]
        d = C.c_double
        L.prl_hip_adaptive_threshold_batch_device.argtypes = [i, i, i, d, i, d, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_adaptive_threshold_host.argtypes = [i, i, d, i, d, i, vp, sz, i, i, vp, sz]
        L.prl_hip_default_adaptive_params.argtypes = [P(AdaptiveParams)]
        L.prl_hip_default_adaptive_params.restype = None
        L.prl_hip_binarize_adaptive_batch_device.argtypes = [P(AdaptiveParams), i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_binarize_adaptive_host.argtypes = [P(AdaptiveParams), i, vp, sz, i, i, vp, sz]
        L.prl_hip_morphology_batch_device.argtypes = [i, i, i, i, i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_morphology_host.argtypes = [i, i, i, i, i, vp, sz, i, i, vp, sz]
        L.prl_hip_morphology_ex_batch_device.argtypes = [i, i, i, i, i, i, i, i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_morphology_ex_host.argtypes = [i, i, i, i, i, i, i, i, vp, sz, i, i, vp, sz]
        L.prl_hip_correct_nuil_batch_device.argtypes = [i, i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_correct_nuil_host.argtypes = [i, i, vp, sz, i, i, vp, sz]
        L.prl_hip_remove_lines_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_remove_lines_host.argtypes = [i, vp, sz, i, i, vp, sz]
        L.prl_hip_histogram_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, vp]
        L.prl_hip_lut_batch_device.argtypes = [i, i, vp, sz, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_gamma_correction_batch_device.argtypes = [i, i, d, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_gamma_correction_host.argtypes = [i, d, d, vp, sz, i, i, vp, sz]
        L.prl_hip_simple_white_balance_batch_device.argtypes = [i, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_simple_white_balance_host.argtypes = [d, vp, sz, i, i, vp, sz]
        L.prl_hip_gray_world_batch_device.argtypes = [i, d, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_gray_world_host.argtypes = [d, i, vp, sz, i, i, vp, sz]
        L.prl_hip_clean_background_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_clean_background_host.argtypes = [i, vp, sz, i, i, vp, sz]
        L.prl_hip_gamma_lut.argtypes = [d, d, vp]
        L.prl_hip_clean_background_lut.argtypes = [vp]
        L.prl_hip_simple_white_balance_luts.argtypes = [d, vp, vp]
        L.prl_hip_gray_world_luts.argtypes = [d, i, vp, vp]
        L.prl_hip_binarize_mokji_batch_device.argtypes = [i, i, i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_binarize_mokji_host.argtypes = [i, i, i, vp, sz, i, i, vp, sz]
        L.prl_hip_mokji_thresholds_batch_device.argtypes = [i, i, i, i, vp, sz, sz, i, i, vp, vp]
        L.prl_hip_cooccurrence_batch_device.argtypes = [i, i, i, vp, sz, sz, vp, sz, sz, i, i, vp, vp]
        L.prl_hip_mokji_threshold.argtypes = [vp, i, P(C.c_int)]
        L.prl_hip_warp_crop_size.argtypes = [vp, d, P(C.c_int), P(C.c_int)]
        L.prl_hip_perspective_transform.argtypes = [vp, vp, vp]
        L.prl_hip_warp_perspective_batch_device.argtypes = [i, i, vp, i, vp, sz, sz, i, i, vp, sz, sz, vp, i, vp, vp]
        L.prl_hip_warp_crop_batch_device.argtypes = [i, i, vp, d, vp, sz, sz, i, i, vp, sz, sz, vp, i, vp, vp]
        L.prl_hip_warp_crop_host.argtypes = [i, vp, d, vp, sz, i, i, vp, sz, i, vp]
        L.prl_hip_pyr_down_size.argtypes = [i, i, i, P(C.c_int), P(C.c_int)]
        L.prl_hip_pyr_down_batch_device.argtypes = [i, i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_pyr_down_host.argtypes = [i, i, vp, sz, i, i, vp, sz]
        L.prl_hip_canny_classes_batch_device.argtypes = [i, i, d, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_edge_link_batch_device.argtypes = [i, vp, sz, sz, i, i, vp, sz, sz, vp, vp]
        L.prl_hip_canny_batch_device.argtypes = [i, i, d, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_canny_host.argtypes = [i, d, d, vp, sz, i, i, vp, sz]
        L.prl_hip_document_edges_geometry.argtypes = [i, i, P(C.c_int), P(C.c_int), P(C.c_int)]
        L.prl_hip_document_edges_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp, vp]
        L.prl_hip_document_edges_host.argtypes = [i, vp, sz, i, i, vp, sz, vp]
        L.prl_hip_resize_pyramid_levels.argtypes = [i, i, i, P(C.c_int), P(C.c_int), P(C.c_int)]
        L.prl_hip_resize_replicate_batch_device.argtypes = [i, i, i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_resize_replicate_host.argtypes = [i, i, i, vp, sz, i, i, vp, sz]
        L.prl_hip_find_contours.argtypes = [vp, sz, i, i, vp, i, vp, i, P(C.c_int), P(C.c_int)]
        L.prl_hip_approx_poly_closed.argtypes = [vp, i, d, vp, P(C.c_int)]
        L.prl_hip_document_quad.argtypes = [vp, sz, i, i, vp, P(C.c_int)]
        L.prl_hip_document_quad_finish.argtypes = [vp, i, i, i, i, vp]
        L.prl_hip_document_contour_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, vp, vp, vp]
        L.prl_hip_document_contour_host.argtypes = [i, vp, sz, i, i, vp, vp, vp]
        L.prl_hip_hough_lines_geometry.argtypes = [i, i, P(C.c_int), P(C.c_int)]
        L.prl_hip_hough_accumulator_batch_device.argtypes = [i, vp, sz, sz, i, i, vp, sz, vp]
        L.prl_hip_hough_lines_batch_device.argtypes = [i, vp, sz, sz, i, i, i, vp, i, vp, vp]
        L.prl_hip_hough_lines_host.argtypes = [vp, sz, i, i, i, vp, i, vp]
        L.prl_hip_hough_edges_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_hough_edges_host.argtypes = [i, vp, sz, i, i, vp, sz]
        L.prl_hip_hough_line_quad.argtypes = [vp, i, i, i, vp, P(C.c_int)]
        L.prl_hip_hough_line_contour_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, vp, vp, vp]
        L.prl_hip_hough_line_contour_host.argtypes = [i, vp, sz, i, i, vp, vp, vp]
        L.prl_hip_focus_sums_batch_device.argtypes = [i, i, i, vp, sz, sz, i, i, vp, vp]
        L.prl_hip_focus_measures_host.argtypes = [i, i, vp, sz, i, i, vp, vp]
        L.prl_hip_focus_from_sums.argtypes = [vp, i, i, vp]
        ll = C.c_longlong
        L.prl_hip_basic_deblur_batch_device.argtypes = [i, i, ll, d, d, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_basic_deblur_host.argtypes = [i, ll, d, d, d, vp, sz, i, i, vp, sz]
        L.prl_hip_gaussian_blur_f32_batch_device.argtypes = [i, i, ll, ll, d, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_gaussian_blur_f32_host.argtypes = [i, ll, ll, d, d, vp, sz, i, i, vp, sz]
        L.prl_hip_gaussian_blur_size.argtypes = [ll, ll, d, d, P(C.c_int), P(C.c_int)]
        L.prl_hip_gaussian_kernel_f32.argtypes = [i, d, vp]
        L.prl_hip_clahe_geometry.argtypes = [i, i, i, i, d] + [P(C.c_int)] * 5
        L.prl_hip_clahe_tile_lut.argtypes = [vp, i, i, vp]
        L.prl_hip_equalize_hist_lut.argtypes = [vp, vp]
        L.prl_hip_clahe_luts_batch_device.argtypes = [i, i, d, i, i, vp, sz, sz, i, i, vp, vp]
        L.prl_hip_clahe_batch_device.argtypes = [i, i, d, i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_clahe_host.argtypes = [i, d, i, i, vp, sz, i, i, vp, sz]
        L.prl_hip_equalize_hist_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_equalize_hist_host.argtypes = [i, vp, sz, i, i, vp, sz]
        L.prl_hip_enhance_local_contrast_batch_device.argtypes = [i, i, d, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_enhance_local_contrast_host.argtypes = [i, d, i, vp, sz, i, i, vp, sz]
        L.prl_hip_gaussian_kernel_u8.argtypes = [i, d, vp]
        L.prl_hip_sep_filter_u8_batch_device.argtypes = [i, i, vp, i, vp, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_gaussian_blur_u8_batch_device.argtypes = [i, i, i, i, d, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_gaussian_blur_u8_host.argtypes = [i, i, i, d, d, vp, sz, i, i, vp, sz]
        L.prl_hip_canny_edge_detection_batch_device.argtypes = [i, i, i, d, d, i, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_canny_edge_detection_host.argtypes = [i, i, d, d, i, vp, sz, i, i, vp, sz]
        L.prl_hip_external_rects.argtypes = [vp, sz, i, i, vp, i, P(C.c_int), P(C.c_int)]
        L.prl_hip_rect_otsu_batch_device.argtypes = [i, vp, vp, d, vp, sz, sz, i, i, vp, sz, sz, vp, vp]
        L.prl_hip_binarize_local_otsu_batch_device.argtypes = [i, i, d, d, i, d, d, i, vp, sz, sz, i, i, vp, sz, sz, vp, vp, vp]
        L.prl_hip_binarize_local_otsu_host.argtypes = [i, d, d, i, d, d, i, vp, sz, i, i, vp, sz, vp, vp]
        L.prl_hip_connected_components_batch_device.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp, vp, i, vp]
        L.prl_hip_external_rects_batch_device.argtypes = [i, vp, sz, sz, i, i, vp, i, vp, vp, vp, vp]
        L.prl_hip_bilateral_tables.argtypes = [i, d, d, P(C.c_int), P(C.c_int), vp, vp, vp, vp]
        L.prl_hip_bilateral_filter_batch_device.argtypes = [i, i, i, d, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_bilateral_filter_host.argtypes = [i, i, d, d, vp, sz, i, i, vp, sz]
        L.prl_hip_variance_mask_batch_device.argtypes = [i, i, d, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_find_contours_tree.argtypes = [vp, sz, i, i, vp, i, vp, i, P(C.c_int), P(C.c_int)]
        L.prl_hip_remove_children_contours.argtypes = [vp, i, vp]
        L.prl_hip_fbcitb_contours.argtypes = [vp, sz, vp, sz, i, i, d, vp, i, vp]
        L.prl_hip_rect_paint_batch_device.argtypes = [i, vp, vp, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_default_fbcitb_params.argtypes = [P(FbcitbParams)]
        L.prl_hip_default_fbcitb_params.restype = None
        L.prl_hip_binarize_fbcitb_batch_device.argtypes = [P(FbcitbParams), i, i, vp, sz, sz, i, i, vp, sz, sz, vp, vp]
        L.prl_hip_binarize_fbcitb_host.argtypes = [P(FbcitbParams), i, vp, sz, i, i, vp, sz, vp]
        _lib = L
    return _lib


def stream_on(where) -> int:
    """Makes the device of a tensor (or a torch.device) the library's current one and returns the handle of torch's current
    stream on it: what every *_device entry is given."""
    import torch

    device = where.device if isinstance(where, torch.Tensor) else where
    check(lib().prl_hip_set_device(device.index or 0))
    return torch.cuda.current_stream(device).cuda_stream


def check(status: int) -> None:
    if status != PRL_OK:
        L = lib()
        msg = L.prl_hip_strerror(status).decode()
        detail = L.prl_hip_last_error_detail().decode()
        raise PrlError(status, f"{msg}" + (f" [{detail}]" if detail and status in (PRL_ERR_HIP, PRL_ERR_NO_DEVICE, PRL_ERR_NOMEM, PRL_ERR_BAD_ARG, PRL_ERR_LITERAL_BUDGET) else ""))
