// imageLibCommon.h - the part of PRLib's src/imageLibCommon.h that exists here: EnhanceLocalContrastByCLAHE (:151,
// imageLibCommon.cpp:327-395) and CannyEdgeDetection (imageLibCommon.cpp:244-324), declared in the global namespace with the reference's signature, and the two OpenCV functions it is
// made of as extensions in namespace prl.  Implemented in prl_host.cpp over the C ABI (clahe.hip; the arithmetic is stated in
// prl_hip.h, "contrast").  The header's other helpers are not provided.
#pragma once

#include "prl.h"

// cv::createCLAHE() with setClipLimit(CLAHEClipLimit) - the default 8 x 8 grid - applied to every channel of an 8-bit image of 1 to
// 4 channels, then, with equalizeHistFlag, cv::equalizeHist of that channel's result.  A limit <= 0 means no clipping, as in
// cv::CLAHE (the reference's callers guard it themselves).  std::invalid_argument("Image for histograms enhancing is empty") for an
// empty image; cv::Exception StsUnsupportedFormat for a depth other than CV_8U or more than 4 channels, StsBadArg for a NaN limit or a
// side above 32768 (documented deviations: cv::CLAHE also takes 16-bit images).  outputImage may be inputImage: the result is a new
// continuous Mat of the input's type, and the input's pixels are never written.
CV_EXPORTS void EnhanceLocalContrastByCLAHE(cv::Mat& inputImage, cv::Mat& outputImage, double CLAHEClipLimit, bool equalizeHistFlag);

// imageLibCommon.cpp:244-324 on an 8-bit image of 1 to 4 channels: per channel the 8-bit cv::GaussianBlur(size x size, sigma 0), the
// Otsu value t, cv::Canny(lower * upper * t, upper * t), the 3 x 3 closing (CannyMorphIters > 0) or opening (< 0); the channels
// OR-ed into resultCanny, a new CV_8UC1 Mat (edgedet.hip; prl_hip.h, "CannyEdgeDetection").  std::invalid_argument with the
// reference's messages, in its order: an empty image, GaussianBlurKernelSize < 3, a coefficient outside [0, 1], lower > upper;
// cv::Exception StsAssert for an even size (cv::GaussianBlur's assertion), StsUnsupportedFormat for a depth other than CV_8U or more
// than 4 channels, StsBadArg for a size above 255, |CannyMorphIters| above 255 or a side above 32768 (documented deviations).
CV_EXPORTS void CannyEdgeDetection(cv::Mat& imageToProc, cv::Mat& resultCanny, int GaussianBlurKernelSize, double CannyUpperThresholdCoeff,
                                   double CannyLowerThresholdCoeff, int CannyMorphIters);

namespace prl {

// Extensions, not in the reference's header: cv::createCLAHE(clipLimit, cv::Size(tilesX, tilesY))->apply and cv::equalizeHist on
// every channel of an 8-bit image of 1 to 4 channels.  Exceptions as above; StsBadArg also for a grid side outside 1..64.
CV_EXPORTS void clahe(const cv::Mat& inputImage, cv::Mat& outputImage, double clipLimit = 40.0, int tilesX = 8, int tilesY = 8);
CV_EXPORTS void equalizeHist(const cv::Mat& inputImage, cv::Mat& outputImage);
// cv::bilateralFilter(inputImage, outputImage, d, sigmaColor, sigmaSpace) with BORDER_REFLECT_101 on an 8-bit image of 1 to 4
// channels, EVERY CHANNEL FILTERED AS A PLANE OF ITS OWN - cv::bilateralFilter's result for one channel, and what the reference
// computes for more by splitting them; not OpenCV's joint colour distance for 3 channels (bilateral.hip; prl_hip.h,
// "cv::bilateralFilter").  std::invalid_argument for an empty image; cv::Exception StsUnsupportedFormat for another depth or more
// than 4 channels, StsBadArg for a side 2 * radius + 1 above 31 or a sigma that is not finite, StsAssert when outputImage shares
// inputImage's pixels (cv::bilateralFilter does not work in place either).
CV_EXPORTS void bilateralFilter(const cv::Mat& inputImage, cv::Mat& outputImage, int d, double sigmaColor, double sigmaSpace);

}  // namespace prl
