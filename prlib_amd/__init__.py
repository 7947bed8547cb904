"""prlib_amd — MI355X (gfx950) implementation of PRLib's local-adaptive binarization hot path.

The product is libprlib_hip.so (hand-written HIP kernels behind the C ABI of include/prl_hip.h).
This package is the thin Python host layer used by the tests and the benchmark; the C++ host layer
with the reference's prl::binarize*(cv::Mat&, cv::Mat&, ...) signatures lives in csrc/prl/.
"""
from . import _capi, binarizations  # noqa: F401
from .denoise import denoise, denoiseSaltPepper, nlm_planes  # noqa: F401
from .adaptive import adaptiveThreshold, binarizeAGT, binarizeAT, binarizeNativeAdaptive, binarizePureAdaptiveGaussian  # noqa: F401
from .morphology import correctNUIL, morphologyEx, morphology_ex  # noqa: F401
from .lines import removeLines  # noqa: F401
from .tone import cleanBackgroundToWhite, gammaCorrection, grayWorldWhiteBalance, histogram, lut, simpleWhiteBalance  # noqa: F401
from .mokji import binarizeMokji, cooccurrence, mokjiThreshold, mokjiThresholds  # noqa: F401
from .detectors import focusFromSums, focusMeasures, focusSums  # noqa: F401
from .deblur import basicDeblur, gaussianBlurF32, gaussianBlurSize, gaussianKernelF32  # noqa: F401
from .contrast import clahe, claheGeometry, claheLuts, claheTileLut, enhanceLocalContrast, equalizeHist, equalizeHistLut  # noqa: F401
from .components import connectedComponents  # noqa: F401
from .fbcitb import (bilateralFilter, bilateralTables, binarizeFBCITB, fbcitbContours, findContoursTree, rectPaint,  # noqa: F401
                     removeChildrenContours, varianceMask)
from .localotsu import (binarizeLocalOtsu, cannyEdgeDetection, externalRects, gaussianBlurU8, gaussianKernelU8, rectOtsu,  # noqa: F401
                        sepFilterU8)
from .thinning import thinGuoHall, thinZhangSuen  # noqa: F401
from .background import backgroundNormalization  # noqa: F401
from .deskew import deskew, deskew_stats, find_angle as findAngle, find_orientation as findOrientation, houghp, rotate  # noqa: F401
from .warp import perspective_transform, warp_crop, warp_crop_host, warp_crop_size, warp_perspective  # noqa: F401
from .edges import (canny, canny_classes, document_edges, document_edges_geometry, edge_link, pyr_down, pyr_down_size, resize,  # noqa: F401
                    resize_pyramid_levels, approx_poly_closed, auto_crop, document_contour, document_quad, document_quad_finish,
                    find_contours)
from .houghline import hough_accumulator, hough_edges, hough_line_contour, hough_line_quad, hough_lines, hough_lines_geometry  # noqa: F401
from .chain import bitwise_not, cvtColorBGR2GRAY, cvtColorGRAY2BGR, process_pages, process_pages_host  # noqa: F401
from .binarizations import (  # noqa: F401
    FENG, NICK, NIBLACK, SAUVOLA, WOLFJOLION, binarize, binarizeFeng, binarizeNICK, binarizeNiblack,
    binarizeSauvola, binarizeWolfJolion, default_params, geometry, last_stats, make_params, morph,
    set_exec_mode, set_literal_page_budget, set_deferred_completion, finish, binarize_pages_host, PinnedPages, binarizeByLocalVariances, binarizeByLocalVariancesWithoutFilters,
)

__all__ = [
    "binarize", "binarizeSauvola", "binarizeNiblack", "binarizeWolfJolion", "binarizeNICK", "binarizeFeng", "binarizeByLocalVariances", "binarizeByLocalVariancesWithoutFilters",
    "adaptiveThreshold", "binarizeNativeAdaptive", "binarizeAT", "binarizeAGT", "binarizePureAdaptiveGaussian",
    "denoise", "denoiseSaltPepper", "nlm_planes", "correctNUIL", "morphologyEx", "morphology_ex", "removeLines", "gammaCorrection", "simpleWhiteBalance", "grayWorldWhiteBalance", "cleanBackgroundToWhite", "histogram", "lut", "binarizeMokji", "mokjiThresholds", "mokjiThreshold", "cooccurrence", "focusSums", "focusMeasures", "focusFromSums", "basicDeblur", "gaussianBlurF32", "gaussianKernelF32", "gaussianBlurSize", "clahe", "claheLuts", "equalizeHist", "enhanceLocalContrast", "claheGeometry", "claheTileLut", "equalizeHistLut", "connectedComponents", "binarizeLocalOtsu", "cannyEdgeDetection", "externalRects", "gaussianBlurU8", "gaussianKernelU8", "rectOtsu", "sepFilterU8", "backgroundNormalization", "deskew", "rotate", "houghp", "findAngle", "findOrientation", "deskew_stats", "warp_crop_size", "perspective_transform", "warp_perspective", "warp_crop", "warp_crop_host", "pyr_down", "pyr_down_size", "canny", "canny_classes", "edge_link", "document_edges", "document_edges_geometry", "resize", "resize_pyramid_levels", "find_contours", "approx_poly_closed", "document_quad", "document_quad_finish", "document_contour", "auto_crop", "hough_lines_geometry", "hough_accumulator", "hough_lines", "hough_edges", "hough_line_quad", "hough_line_contour", "thinZhangSuen", "thinGuoHall", "cvtColorBGR2GRAY", "cvtColorGRAY2BGR", "bitwise_not", "process_pages", "process_pages_host", "make_params", "default_params", "geometry", "last_stats", "morph", "set_exec_mode", "set_literal_page_budget", "set_deferred_completion", "finish", "binarize_pages_host", "PinnedPages",
    "SAUVOLA", "NIBLACK", "WOLFJOLION", "NICK", "FENG",
]
