// prl.h — C++ host layer with the reference's signatures for the hot path, over the C ABI of
// include/prl_hip.h.  A caller of PRLib switches by including this header instead of the six reference
// headers and linking libprlib_hip.so + prl_host.cpp:
//
//   reference header (PRLib tree)                          function
//   src/binarizations/binarizeSauvola.h:43-47              prl::binarizeSauvola
//   src/binarizations/binarizeNiblack.h:43-47              prl::binarizeNiblack
//   src/binarizations/binarizeWolfJolion.h:43-47           prl::binarizeWolfJolion
//   src/binarizations/binarizeNICK.h:43-47                 prl::binarizeNICK
//   src/binarizations/binarizeFeng.h:46-53                 prl::binarizeFeng
//   src/denoise/denoiseNLM.h:32                            prl::denoise
//   src/denoise/denoiseSaltPepper.h:40                     prl::denoiseSaltPepper
//   src/binarizations/binarizeNativeAdaptive.h:62-74       prl::binarizeNativeAdaptive
//   src/binarizations/binarizeAT.h:33, binarizeAGT.h:32    prl::binarizeAT, prl::binarizeAGT
//   src/binarizations/binarizePureAdaptiveGaussian.h:33    prl::binarizePureAdaptiveGaussian
//   src/correctNUIL.h:32                                   prl::correctNUIL
//   src/removeLines.h:38                                   prl::removeLines
//   src/balance/gammaCorrection.h:33                       prl::gammaCorrection
//   src/balance/balanceSimpleWhite.h:33                    prl::simpleWhiteBalance
//   src/balance/balanceGrayWorldWhite.h:33                 prl::grayWorldWhiteBalance
//   src/cleanBackgroundToWhite.h:40                        prl::cleanBackgroundToWhite
//   src/binarizations/binarizeMokji.h:46                   prl::binarizeMokji
//   src/detectors/blurDetection.h:35                       prl::isBlurred (+ prl::focusMeasures)
//   src/deblur/basicDeblur.h:32-34                         prl::basicDeblur
//   src/binarizations/binarizeLocalOtsu.h                  prl::binarizeLocalOtsu
//   src/binarizations/binarizeFBCITB.h                     prl::binarizeFBCITB
//   src/warp.h:49-73                                       prl::warpCrop
//   src/border_detection/autoCrop.h:42-53                  prl::documentContour, prl::autoCrop
//   src/border_detection/houghLine.h                       prl::findHoughLineContour
//   src/resize.h:32                                        prl::resize
//
// Same names, argument order, defaults, exceptions (std::invalid_argument for an empty image or a bad
// window, binarizeSauvola.cpp:38-47) and side effects: the caller's input Mat is converted to gray
// (:51) and replaced by the replicate-padded page (:65); the output Mat is (re)allocated (:122).
// Define PRL_KEEP_INPUT before including to opt out of the input mutation.
// include/prl/ holds one forwarding header per reference header (binarizeSauvola.h, ..., denoiseNLM.h), so a caller keeps
// its #include lines and only changes the include path.
#pragma once

#include <vector>

#if defined(__has_include)
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#define PRL_HAVE_OPENCV 1
#endif
#endif
#if defined(PRL_REQUIRE_OPENCV) && !defined(PRL_HAVE_OPENCV)
#error "PRL_REQUIRE_OPENCV: <opencv2/core/core.hpp> was not found on the include path"
#endif
#ifndef PRL_HAVE_OPENCV
#include "cvmat_shim.h"
#endif
#ifndef CV_EXPORTS   // (OpenCV defines it; the shim build exports the same way)
#define CV_EXPORTS __attribute__((visibility("default")))
#endif

namespace prl {

CV_EXPORTS void binarizeSauvola(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize = 101,
                     double thresholdCoefficient = 0.01, int morphIterationCount = 2);

CV_EXPORTS void binarizeNiblack(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize = 101,
                     double thresholdCoefficient = 0.01, int morphIterationCount = 2);

CV_EXPORTS void binarizeWolfJolion(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize = 101,
                        double thresholdCoefficient = 0.01, int morphIterationCount = 2);

CV_EXPORTS void binarizeNICK(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize = 21,
                  double thresholdCoefficient = -0.01, int morphIterationCount = 0);

CV_EXPORTS void binarizeFeng(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize = 21,
                  double thresholdCoefficient_alpha1 = 0.75, double thresholdCoefficient_k1 = 0.2,
                  double thresholdCoefficient_k2 = 0.03, double thresholdCoefficient_gamma = 2.0,
                  int morphIterationCount = 2);

CV_EXPORTS void denoise(const cv::Mat& inputImage, cv::Mat& outputImage, double strength = 5.5);

// src/denoise/denoiseSaltPepper.h:40 - out = in.clone(), then `times` passes of cv::medianBlur(out, out, kernelSize) (.cpp:29-36):
// the exact median of every kernelSize x kernelSize window, BORDER_REPLICATE, channels independent.  times == 0: a clone of any
// Mat.  Otherwise cv::Exception: StsAssert for an empty input or an even / non-positive kernelSize, and for 2 channels with
// kernelSize >= 7 ([upstream] medianBlur's k > 5 path); StsUnsupportedFormat for a depth other than CV_8U or more than 4
// channels (OpenCV also takes 16U / 16S / 32F at k <= 5: not here).  The output is a new continuous Mat; the input's pixels
// are never written (out may be in, or a view of it).
CV_EXPORTS void denoiseSaltPepper(const cv::Mat& in, cv::Mat& out, int kernelSize, size_t times);

// src/binarizations/binarizeNativeAdaptive.h:62-74 - [BGR -> gray], cv::medianBlur, cv::adaptiveThreshold(THRESH_BINARY_INV),
// 255 - mask where the mask's mean is below 128 (.cpp:34-135), in the reference's statement order: std::invalid_argument for an
// empty input, then for a max value outside [0; 255] (NaN included); a colour input becomes gray in the caller's Mat (:60; not
// with PRL_KEEP_INPUT); cv::Exception(StsAssert) for medianBlurKernelSize < 3 or even; adaptiveThresholdingBlockSize < 3 means
// (int)(sqrt(rows^2 + cols^2) / 333 + 7), and an even block size is cv::adaptiveThreshold's StsAssert (a 4096 x 4096 page gives
// 24).  Not provided, cv::Exception(StsNotImplemented) after the reference's own checks: isGaussianBlurReqiured (OpenCV's 8-bit
// fixed-point GaussianBlur), bilateralFilterBlockSize >= 3 (outputImage then already holds the mask), block sizes above 255.
// Where the block size is rejected outputImage stays untouched (the reference leaves the median-filtered page there).
CV_EXPORTS void binarizeNativeAdaptive(cv::Mat& inputImage, cv::Mat& outputImage, bool isGaussianBlurReqiured = 0,
                            int medianBlurKernelSize = 5, int GaussianBlurKernelSize = 7, double GaussianBlurSigma = 150.0,
                            bool isAdaptiveThresholdCalculatedByGaussian = true, double adaptiveThresholdingMaxValue = 255.0,
                            int adaptiveThresholdingBlockSize = 19, double adaptiveThresholdingShift = 9,
                            int bilateralFilterBlockSize = 0, double bilateralFilterColorSigma = 150.0,
                            double bilateralFilterSpaceSigma = 150.0);

// src/binarizations/binarizeAT.h:33, binarizeAGT.h:32, binarizePureAdaptiveGaussian.h:33 - cv::medianBlur on the COLOUR page
// (AT, AGT), BGR -> gray, cv::adaptiveThreshold(MEAN_C for AT / GAUSSIAN_C for the others, THRESH_BINARY).  std::invalid_argument
// for an empty input; cv::medianBlur's checks (odd kernel; 1 = no filter); a 1-channel input is cv::Exception(StsAssert) with
// outputImage untouched: the reference hands cv::adaptiveThreshold an empty Mat there (binarizeAT.cpp:56-65); an even or
// < 3 block size is StsAssert.  The input is never written.
CV_EXPORTS void binarizeAT(const cv::Mat& inputImage, cv::Mat& outputImage, const int medianKernelSize, const double maxValue,
                const int blockSize, const int shift);
CV_EXPORTS void binarizeAGT(const cv::Mat& inputImage, cv::Mat& outputImage, const int medianKernelSize, const double maxValue,
                 const int blockSize, const int shift);
CV_EXPORTS void binarizePureAdaptiveGaussian(const cv::Mat& inputImage, cv::Mat& outputImage, const double maxValue,
                                  const int blockSize, const int shift);

// src/correctNUIL.h:32 - removes non-uniform illumination (correctNUIL.cpp:33-90): per channel, x ^ 255 where cv::mean over the
// page is below 128, then 255 - cv::morphologyEx(channel, MORPH_BLACKHAT, getStructuringElement(MORPH_ELLIPSE, Size(size, size))).
// std::invalid_argument("Input image for filtration is empty"); cv::Exception: StsAssert for more than 4 channels (cv::mean) and
// for structuringElementSize < 1 (getStructuringElement), StsUnsupportedFormat for a depth other than CV_8U, StsBadArg for a
// size above 255 (OpenCV has no upper limit: not here).  The output is a new continuous Mat of the input's size and type; the
// input's pixels are never written (out may be in, or a view of it).
CV_EXPORTS void correctNUIL(const cv::Mat& inputImage, cv::Mat& outputImage, int structuringElementSize = 31);

// src/removeLines.h:38 - strips ruled lines, table grids and form boxes (removeLines.cpp:30-76): [BGR -> gray],
// bw = cv::threshold(~gray, THRESH_BINARY | THRESH_OTSU), horizontal / vertical = cv::erode then cv::dilate of bw with
// getStructuringElement(MORPH_RECT, Size(cols / 50, 1)) / Size(1, rows / 50), out = ~((bw - horizontal) - vertical): 8UC1 at the
// input's size.  cv::Exception: StsAssert for an empty input and for cols < 50 or rows < 50 (getStructuringElement's size 0);
// StsUnsupportedFormat for channel counts other than 1 and 3 (cv::threshold's Otsu takes 8UC1 only) and for a depth other than
// CV_8U.  On every error outputImage stays untouched.  The output is a new continuous Mat; the input's pixels are never
// written (out may be in, or a view of it).
CV_EXPORTS void removeLines(const cv::Mat& inputImage, cv::Mat& outputImage);

// src/balance/gammaCorrection.h:33, balanceSimpleWhite.h:33, balanceGrayWorldWhite.h:33, src/cleanBackgroundToWhite.h:40 - point
// operations whose table depends on page statistics (tone.hip; the arithmetic is stated in prl_hip.h).  No default arguments,
// as in the reference.  std::invalid_argument with the reference's messages for an empty input and, for the two white
// balances, for a channel count other than 3; cv::Exception StsUnsupportedFormat for a depth other than CV_8U and for channel
// counts the conversion rejects (gammaCorrection: above 4; cleanBackgroundToWhite: other than 1, 3, 4: "Cannot convert RAW image
// to Pix", formatConvert.cpp:103-104).  gammaCorrection of a 4-channel Mat returns 3 channels with only the k step applied
// (gammaCorrection.cpp:74-97: BGRA -> BGR, and the switch has no case for 4); cleanBackgroundToWhite returns 3 channels for 3 and 4.
// On every error outputImage stays untouched.  The output is a new continuous Mat; the input's pixels are never written.
CV_EXPORTS void gammaCorrection(const cv::Mat& inputImage, cv::Mat& outputImage, const double k, const double gamma);
CV_EXPORTS void simpleWhiteBalance(const cv::Mat& inputImage, cv::Mat& outputImage, const double k);
CV_EXPORTS void grayWorldWhiteBalance(const cv::Mat& inputImage, cv::Mat& outputImage, const double pNorm, const bool withMax);
CV_EXPORTS void cleanBackgroundToWhite(const cv::Mat& inputImage, cv::Mat& outputImage);

// src/binarizations/binarizeMokji.h:46 - one global threshold from the co-occurrence matrix of the page and its dilation
// (binarizeMokji.cpp:35-94, mokji.hip; the arithmetic is stated in prl_hip.h): out = gray > t ? 255 : 0, 8UC1 at the input's size.
// std::invalid_argument("mokjiThreshold: invalid maxEdgeWidth") for maxEdgeWidth < 1, then ("mokjiThreshold: invalid
// minEdgeMagnitude") for minEdgeMagnitude < 1, both before the image is looked at.  cv::cvtColor(BGR2GRAY) runs unconditionally in
// the reference: an empty or 1-channel Mat (and any count other than 3 and 4) is cv::Exception StsUnsupportedFormat, as is a depth
// other than CV_8U.  Where the reference is undefined (no interior: cols <= 2 maxEdgeWidth or rows <= 2 maxEdgeWidth; no pair with
// an edge of minEdgeMagnitude; minEdgeMagnitude >= 256) the page comes out all 255, which is what x86 gives.  Limit: maxEdgeWidth
// above 127 on a page with an interior is StsBadArg.  On every error outputImage stays untouched.  The output is a new continuous
// Mat; the input's pixels are never written (out may be in, or a view of it).
CV_EXPORTS void binarizeMokji(const cv::Mat& inputImage, cv::Mat& outputImage, size_t maxEdgeWidth = 3, size_t minEdgeMagnitude = 20);

// src/detectors/blurDetection.h:35 - returns false without looking at the image, as blurDetection.cpp:85-89 does: the reference
// has no threshold for its four focus measures (LAPM_Algo, LAPV_Algo, TENG_Algo, GLVN_Algo, :32-83) and calls none of them.
CV_EXPORTS bool isBlurred(const cv::Mat& inputImage);

// An extension, not in the reference's header: those four measures of CHANNEL 0 of an 8-bit image of 1, 3 or 4 channels, as
// cv::mean(FM).val[0] and mu.val[0] give them there (focus.hip; the arithmetic is stated in prl_hip.h, "focus measures").
// tengKernelSize is cv::Sobel's ksize, 3 or 1.  std::invalid_argument for an empty image; cv::Exception StsUnsupportedFormat for a
// depth other than CV_8U or channels other than 1, 3, 4; StsBadArg for another tengKernelSize or a side above 32768.  An
// all-zero image has glvn NaN.  The input's pixels are never written.
struct FocusMeasures {
    double lapm, lapv, teng, glvn;
};
CV_EXPORTS FocusMeasures focusMeasures(const cv::Mat& inputImage, int tengKernelSize = 3);

// src/deblur/basicDeblur.h:32-34 - the unsharp mask of basicDeblur.cpp:33-70 on every channel of an 8-bit image of 1 to 4 channels:
// out = saturate_u8(cvRound(x * (float)(2 w) + GaussianBlur_f32(x) * (float)(2 w - 2))) (deblur.hip; the rules are stated in
// prl_hip.h, "basicDeblur").  std::invalid_argument("Input image for deblurring is empty") for an empty image; cv::Exception
// StsAssert where cv::GaussianBlur's CV_Assert on the kernel size fails (an even size, or size 0 without a positive sigma);
// StsNotImplemented for a depth other than CV_8U; StsUnsupportedFormat for more than 4 channels; StsBadArg for a kernel side above
// 255, a size beyond int, a NaN or infinite sigma or weight, an image side above 32768 (documented deviations).  outputImage may be
// inputImage: the result is a new Mat, and the input's pixels are never written.
CV_EXPORTS void basicDeblur(const cv::Mat& inputImage, cv::Mat& outputImage, const size_t gaussianKernelSize = 0, const double sigmaX = 9.0,
                            const double sigmaY = 0.0, const double imageWeight = 0.75);

// src/binarizations/binarizeLocalOtsu.h - binarizeLocalOtsu.cpp:37-163 on an 8-bit image of 1, 3 or 4 channels: gray (a colour image
// through cv::COLOR_RGB2GRAY, as the reference converts it), EnhanceLocalContrastByCLAHE(CLAHEClipLimit, true) when the limit is
// positive, CannyEdgeDetection, three 3 x 3 dilations, the bounding rectangles of the external contours, and Otsu's threshold of
// every rectangle painted into a white mask (localotsu.hip; the rules are stated in prl_hip.h, "binarizeLocalOtsu").
// std::invalid_argument with the reference's messages: an empty image, maxValue outside [0, 255], CannyEdgeDetection's checks
// (GaussianBlurKernelSize < 3, a coefficient outside [0, 1], lower > upper), and "Contours array is empty" when the edge map has no
// contour (outputImage then stays as it was).  cv::Exception StsAssert for an even GaussianBlurKernelSize (cv::GaussianBlur's
// assertion); StsUnsupportedFormat for a depth other than CV_8U or 2 channels; StsBadArg for a kernel size above 255, a NaN clip limit
// or a side above 32768 (documented deviations).  outputImage may be inputImage: the result is a new CV_8UC1 Mat, and the input's
// pixels are never written.
CV_EXPORTS void binarizeLocalOtsu(cv::Mat& inputImage, cv::Mat& outputImage, double maxValue = 255.0, double CLAHEClipLimit = 0.0,
                                  int GaussianBlurKernelSize = 19, double CannyUpperThresholdCoeff = 0.15,
                                  double CannyLowerThresholdCoeff = 0.01, int CannyMorphIters = 1);

// src/binarizations/binarizeFBCITB.h - binarizeFBCITB.cpp:73-404, "font and background color independent text binarization", on an
// 8UC3 (BGR) or one-channel 8-bit image (fbcitb.hip, bilateral.hip; the rules are stated in prl_hip.h, "binarizeFBCITB").  As in the
// reference a one-channel inputImage is REPLACED by its cv::COLOR_GRAY2BGR conversion (the caller's Mat becomes 8UC3); a colour
// image's pixels are never written.  useOtherColorspace and boundingRectMaxAreaCoeff are unused, as there.  An image whose contour
// map has no contour gives an all-white mask.  std::invalid_argument with the reference's messages for an empty image and for any
// other type ("Invalid type of image for binarization (required 24 bits per pixel)"), and CannyEdgeDetection's when that stage
// runs; cv::Exception StsAssert for an even blur size, StsBadArg for a parameter that is not finite, a blur size above 255, a
// bilateral side above 31 or an image side above 32768 (documented deviations).  outputImage is a new CV_8UC1 Mat.
CV_EXPORTS void binarizeFBCITB(cv::Mat& inputImage, cv::Mat& outputImage, bool useCanny = true, bool useVariancesMap = true,
                               bool useCLAHE = true, bool useBilateral = true, bool useOtherColorspace = false, bool useMorphology = true,
                               bool useCannyOnVariances = true, double varianceMapThreshold = 200.0, double CLAHEClipLimit = 2.0,
                               double gaussianBlurKernelSize = 9.0, double cannyUpperThresholdCoeff = 0.6,
                               double cannyLowerThresholdCoeff = 0.4, double boundingRectangleMaxArea = 0.3, int bilateralKernelSize = 5,
                               double bilateralKernelIntensitySigma = 150.0, double bilateralKernelSpatialSigma = 150.0,
                               double boundingRectMaxAreaCoeff = 0.3);

// SURVEY.md §8f rank 1 — src/thinning/thinZhangSuen.h, src/thinning/thinGuoHall.h.  8UC1 or 8UC3 (BGR is
// converted to gray first, thinZhangSuen.cpp:78-81); foreground = pixels with bit 0 set; output 0/255.
// std::invalid_argument for an empty image or another type (:59-68).
CV_EXPORTS void thinZhangSuen(cv::Mat& inputImage, cv::Mat& outputImage);
CV_EXPORTS void thinGuoHall(cv::Mat& inputImage, cv::Mat& outputImage);

// SURVEY.md §8f rank 4b — src/binarizations/binarizeByLocalVariances.h:8-12.  8UC3 input (the reference reads three
// variance planes); std::invalid_argument for an empty image (binarizeByLocalVariances.cpp:16-19, :151-154).
CV_EXPORTS void binarizeByLocalVariances(cv::Mat& inputImage, cv::Mat& outputImage, double varianceThresholdCoeff = 0.125,
                              int minResultVariance = 25, double gamma = 2.0);
CV_EXPORTS void binarizeByLocalVariancesWithoutFilters(cv::Mat& inputImage, cv::Mat& outputImage, double varianceThresholdCoeff = 0.125,
                                            int minResultVariance = 10);

// SURVEY.md §8f rank 3 — src/backgroundNormalization.h:40.  8UC1 -> 8UC1; 8UC3 / 8UC4 -> 8UC3 (the reference's
// Leptonica round trip drops a fourth channel, src/formatConvert.cpp:193-206).  std::invalid_argument for an empty image
// (src/backgroundNormalization.cpp:40-43).
CV_EXPORTS void backgroundNormalization(const cv::Mat& inputImage, cv::Mat& outputImage);

// SURVEY.md §8f rank 4a — src/deskew/deskew.h:42, src/rotate.h:39.  deskew: gray -> Otsu -> HoughLinesP angle vote ->
// rotate; the result is max(cols, rows) square when an angle was found (src/rotate.cpp:64-68), a clone otherwise.
// The orientation step (src/deskew/deskew.cpp:238) is a no-op for the page the reference hands it.
CV_EXPORTS bool deskew(const cv::Mat& inputImage, cv::Mat& outputImage);
// src/deskew/deskew.h:62 - the angle prl::deskew rotates by: HoughLinesP on the complement of a 1-channel (thresholded)
// page, first-fit vote over the segments' atan2, in degrees; 0.0 when no segment is found (deskew.cpp:139-205).
CV_EXPORTS double findAngle(const cv::Mat& inputImage);
// src/deskew/deskew.h:52 - 0.0 (see prl_host.cpp: a no-op for the page prl::deskew hands it, deskew.cpp:70-84, :238).
CV_EXPORTS double findOrientation(const cv::Mat& inputImage);
CV_EXPORTS void rotate(const cv::Mat& inputImage, cv::Mat& outputImage, double angle);

// src/warp.h:49-73 - the quadrilateral (x0, y0) top left, (x1, y1) top right, (x2, y2) bottom right, (x3, y3) bottom left as a
// rectangle (warp.cpp:32-102, warp.hip; the arithmetic is stated in prl_hip.h): W = cvRound(max of the top and bottom sides),
// H = cvRound(max of the left and right sides), W = cvRound(H / ratio) for ratio > 0, cv::getPerspectiveTransform,
// cv::warpPerspective(INTER_LINEAR, borderMode, borderValue).  The defaults are the reference's: -1.0, cv::BORDER_CONSTANT
// (written 0 here) and cv::Scalar().  The vector overload throws std::invalid_argument("Image for warping is empty") and
// ("Size of array of base points for warping isn't equal 4") as warp.cpp:82-90 does; the coordinate overload has no check of its
// own, so an empty input is cv::warpPerspective's cv::Exception StsAssert [upstream].  cv::Exception StsUnsupportedFormat for a
// depth other than CV_8U or more than 4 channels; StsNotImplemented for a border mode other than cv::BORDER_CONSTANT and
// cv::BORDER_REPLICATE; StsBadArg for the limits (sides above 32767, a result side <= 0, corners that give a singular system).
// On every error outputImage stays untouched.  The output is a new continuous Mat; the input's pixels are never written.
CV_EXPORTS void warpCrop(const cv::Mat& inputImage, cv::Mat& outputImage, const int x0, const int y0, const int x1, const int y1,
              const int x2, const int y2, const int x3, const int y3, double ratio = -1.0, const int borderMode = 0,
              const cv::Scalar& borderValue = cv::Scalar());
CV_EXPORTS void warpCrop(cv::Mat& inputImage, cv::Mat& outputImage, const std::vector<cv::Point>& points, double ratio = -1.0,
              int borderMode = 0, const cv::Scalar& borderValue = cv::Scalar());

// src/border_detection/autoCrop.h:42-53 - the page in a photograph as four corners, and the page itself (autoCrop.cpp:43-175; the
// arithmetic is stated in prl_hip.h, "document contour").  documentContour: the edge map on the device (pyramid, most informative
// channel, cv::Canny(25, 50)), the quad search on the host, one retry after a closing; true and the corners top left, top right,
// bottom right, bottom left in source coordinates, or false and an empty vector.  cv::Point_<float> is cv::Point2f.  Positive
// scaleX and scaleY (cv::resize, INTER_AREA) are cv::Exception StsNotImplemented; std::invalid_argument for an empty image;
// StsUnsupportedFormat for a depth other than CV_8U or channels other than 1, 3, 4.  autoCrop: as the reference, a CV_8UC1 input
// becomes BGR in the caller's Mat; the corners are truncated to int and handed to prl::warpCrop(in, out, points); false, and
// outputImage untouched, when no quad is found; std::invalid_argument("autoCrop: Image for cropping is empty").
CV_EXPORTS bool documentContour(cv::Mat& inputImage, const double scaleX, const double scaleY,
                                std::vector<cv::Point_<float> >& resultContour);
CV_EXPORTS bool autoCrop(cv::Mat& inputImage, cv::Mat& outputImage);

// src/border_detection/houghLine.h - the reference's second border detector (houghLine.cpp:177-256; the arithmetic is stated in
// prl_hip.h, "Hough lines"): medianBlur(3) x 3, medianBlur(5) x 3, cv::Canny(25, 50) on the image's own 1, 3 or 4 channels and
// cv::HoughLines(1, CV_PI / 180, 50) on the device, the line filter and the search for the largest valid quadrilateral on the host.
// true and the four corners, truncated to int, APPENDED to resultContour as the reference does; false and resultContour untouched.
// std::invalid_argument("Input image is empty"); cv::Exception StsUnsupportedFormat for a depth other than CV_8U or channels other
// than 1, 3, 4.  The input's pixels are never written, and no file is (the reference's cv::imwrite calls are debugging leftovers).
CV_EXPORTS bool findHoughLineContour(cv::Mat& inputImage, std::vector<cv::Point>& resultContour);

// src/resize.h:32 (no defaults, as there) - resize.cpp:29-62 (pyr.hip; the arithmetic is stated in prl_hip.h).  scaleX > 0 and
// scaleY > 0: cv::resize(INTER_AREA) to cols * scaleX x rows * scaleY, an exact replication through OpenCV's float64 index tables.
// Otherwise dst = src.clone(), then cv::pyrDown while the long side exceeds maxSize.  cv::Exception StsBadArg for maxSize < 1 on
// that path (the reference loops for ever) and for a result side above 32768; StsAssert for an empty source on the scale path
// [upstream]; StsUnsupportedFormat for a depth other than CV_8U or more than 4 channels.  On every error dst stays untouched.
// The output is a new continuous Mat; the input's pixels are never written.
CV_EXPORTS void resize(const cv::Mat& src, cv::Mat& dst, int scaleX, int scaleY, int maxSize);

// BASELINE config 1 (plumbing, host only): global Otsu, the one global threshold the reference uses
// (cv::threshold(..., THRESH_BINARY | THRESH_OTSU), src/deskew/deskew.cpp:224).  Not a GPU path.
CV_EXPORTS void binarize(cv::Mat& inputImage, cv::Mat& outputImage);

}  // namespace prl
