// prl_host.cpp — thin C++ shims: validate like the reference, hand (data, step, rows, cols) to the C ABI.
//
// Builds against real OpenCV (PRL_HAVE_OPENCV, set by prl.h when <opencv2/core/core.hpp> exists) and against cvmat_shim.h.
// Only names both have are used; tests/test_cpp_host.py compiles this file against OpenCV's declared signatures
// (tests/cpp/opencv_api/).  With OpenCV present the colour conversion is OpenCV's own cv::cvtColor, as in the reference.
#include "prl.h"
#include "imageLibCommon.h"

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef PRL_HAVE_OPENCV
#include <opencv2/imgproc/imgproc.hpp>   // cv::cvtColor — the header the reference includes (binarizeSauvola.cpp:29)
#endif

#include "../../../include/prl_hip.h"

namespace {

// Every cv::Exception of this layer is thrown here, through the constructor OpenCV has:
// Exception(int code, const String& err, const String& func, const String& file, int line).
[[noreturn]] void fail_cv(int code, const std::string& err, const char* func, int line)
{
    throw cv::Exception(code, err, func, __FILE__, line);
}
#define PRL_FAIL_CV(code, err) fail_cv((code), (err), __func__, __LINE__)

// A C-ABI status as the exception the reference would raise at that point.
[[noreturn]] void raise_at(int status, const char* func, int line)
{
    const std::string msg = prl_hip_strerror(status);
    if (status == PRL_ERR_EMPTY || status == PRL_ERR_BAD_WINDOW)
        throw std::invalid_argument(msg);  // binarizeSauvola.cpp:38-47
    const std::string detail = prl_hip_last_error_detail();
    int code = cv::Error::StsError;
    switch (status) {
    case PRL_ERR_BAD_CHANNELS: code = cv::Error::StsUnsupportedFormat; break;   // cvtColor / NLM reject the type
    case PRL_ERR_EMPTY_RECT: code = cv::Error::StsAssert; break;                // the ROI assertion of cv::Mat::operator()
    case PRL_ERR_BAD_ARG: code = cv::Error::StsBadArg; break;
    case PRL_ERR_NO_DEVICE:
    case PRL_ERR_HIP: code = cv::Error::GpuApiCallError; break;
    case PRL_ERR_NOMEM: code = cv::Error::StsNoMem; break;
    case PRL_ERR_UNSUPPORTED: code = cv::Error::StsNotImplemented; break;
    default: break;
    }
    fail_cv(code, detail.empty() ? msg : msg + " [" + detail + "]", func, line);
}
#define raise(status) raise_at((status), __func__, __LINE__)

// cv::cvtColor(in, in, cv::COLOR_BGR2GRAY) on 8-bit BGR/BGRA — binarizeSauvola.cpp:51.
// With OpenCV: the installed cv::cvtColor itself (its luma coefficients differ between versions, SURVEY.md Appendix B, and
// the reference gets whatever the machine has).  Without: the 14-bit fixed-point luma, a per-pixel conversion on the host.
void bgr2gray_inplace(cv::Mat& m)
{
#ifdef PRL_HAVE_OPENCV
    cv::cvtColor(m, m, cv::COLOR_BGR2GRAY);
#else
    const int cn = m.channels();
    cv::Mat g(m.rows, m.cols, CV_8UC1);
    for (int y = 0; y < m.rows; ++y) {
        const unsigned char* s = m.ptr(y);
        unsigned char* d = g.ptr(y);
        for (int x = 0; x < m.cols; ++x, s += cn)
            d[x] = (unsigned char)((s[0] * 1868 + s[1] * 9617 + s[2] * 4899 + (1 << 13)) >> 14);
    }
    m = g;
#endif
}

void run(int method, cv::Mat& in, cv::Mat& out, int windowSize, double k, int morph, double a1 = 0.75,
         double k1 = 0.2, double k2 = 0.03, double gamma = 2.0)
{
    if (in.empty()) throw std::invalid_argument("Input image for binarization is empty");
    if (!((windowSize > 1) && ((windowSize % 2) == 1)))
        throw std::invalid_argument(prl_hip_strerror(PRL_ERR_BAD_WINDOW));
    if (in.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl: 8-bit images only");
    if (in.channels() != 1) {
        if (in.channels() != 3 && in.channels() != 4) raise(PRL_ERR_BAD_CHANNELS);
        bgr2gray_inplace(in);
    }
    prl_binarize_params p{};
    p.method = method;
    p.window_size = windowSize;
    p.k = k;
    p.morph_iterations = morph;
    p.feng_alpha1 = a1;
    p.feng_k1 = k1;
    p.feng_k2 = k2;
    p.feng_gamma = gamma;
    prl_binarize_geometry g{};
    int st = prl_hip_binarize_geometry(&p, in.cols, in.rows, &g);
    if (st != PRL_OK) raise(st);
    cv::Mat result(g.out_h, g.out_w, CV_8UC1);
#ifndef PRL_KEEP_INPUT
    cv::Mat padded(g.padded_h, g.padded_w, CV_8UC1);
    st = prl_hip_binarize_host(&p, in.data, in.step, in.cols, in.rows, result.data, result.step, padded.data,
                               padded.step);
#else
    st = prl_hip_binarize_host(&p, in.data, in.step, in.cols, in.rows, result.data, result.step, nullptr, 0);
#endif
    if (st != PRL_OK) raise(st);
#ifndef PRL_KEEP_INPUT
    in = padded;  // cv::copyMakeBorder(in, in, ...) — binarizeSauvola.cpp:65
#endif
    out = result;  // outputImage = in(rect) > T — :122
}

}  // namespace

void prl::binarizeSauvola(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize,
                          double thresholdCoefficient, int morphIterationCount)
{
    run(PRL_SAUVOLA, inputImage, outputImage, windowSize, thresholdCoefficient, morphIterationCount);
}

void prl::binarizeNiblack(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize,
                          double thresholdCoefficient, int morphIterationCount)
{
    run(PRL_NIBLACK, inputImage, outputImage, windowSize, thresholdCoefficient, morphIterationCount);
}

void prl::binarizeWolfJolion(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize,
                             double thresholdCoefficient, int morphIterationCount)
{
    run(PRL_WOLFJOLION, inputImage, outputImage, windowSize, thresholdCoefficient, morphIterationCount);
}

void prl::binarizeNICK(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize, double thresholdCoefficient,
                       int morphIterationCount)
{
    run(PRL_NICK, inputImage, outputImage, windowSize, thresholdCoefficient, morphIterationCount);
}

void prl::binarizeFeng(cv::Mat& inputImage, cv::Mat& outputImage, int windowSize,
                       double thresholdCoefficient_alpha1, double thresholdCoefficient_k1,
                       double thresholdCoefficient_k2, double thresholdCoefficient_gamma, int morphIterationCount)
{
    run(PRL_FENG, inputImage, outputImage, windowSize, 0.0, morphIterationCount, thresholdCoefficient_alpha1,
        thresholdCoefficient_k1, thresholdCoefficient_k2, thresholdCoefficient_gamma);
}

void prl::denoise(const cv::Mat& inputImage, cv::Mat& outputImage, double strength)
{
    // [upstream] an empty Mat has type CV_8UC1: "Type of input image should be CV_8UC3 or CV_8UC4!"
    if (inputImage.empty()) raise(PRL_ERR_BAD_CHANNELS);
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::denoise: 8-bit images only");
    cv::Mat result(inputImage.rows, inputImage.cols, inputImage.type());
    const int st = prl_hip_denoise_host(inputImage.channels(), (float)strength, inputImage.data, inputImage.step,
                                        inputImage.cols, inputImage.rows, result.data, result.step);
    if (st != PRL_OK) raise(st);  // 1/2-channel input: "Type of input image should be CV_8UC3 or CV_8UC4!" upstream
    outputImage = result;
}

// denoiseSaltPepper.cpp:29-36: out = in.clone(); for (times) cv::medianBlur(out, out, kernelSize).  The checks below are
// cv::medianBlur's; `out` holds the clone before any of them throws, as in the reference.
void prl::denoiseSaltPepper(const cv::Mat& in, cv::Mat& out, int kernelSize, size_t times)
{
    if (times == 0) {
        out = in.clone();
        return;
    }
    const char* fail = nullptr;
    int code = cv::Error::StsAssert;
    if (in.empty()) fail = "!_src0.empty()";                        // [upstream] OpenCV >= 4
    else if (kernelSize % 2 != 1) fail = "(ksize % 2 == 1) && (_src0.dims() <= 2 )";
    else if (in.depth() != CV_8U || in.channels() > 4) {
        code = cv::Error::StsUnsupportedFormat;                       // documented deviation: 8-bit only
        fail = "prl::denoiseSaltPepper: 8-bit images of 1..4 channels only";
    } else if (in.channels() == 2 && kernelSize >= 7) {
        fail = "cn == 1 || cn == 3 || cn == 4";                       // [upstream] medianBlur's k > 5 path
    }
    if (fail) {
        out = in.clone();
        PRL_FAIL_CV(code, fail);
    }
    cv::Mat result(in.rows, in.cols, in.type());
    const int st = prl_hip_median_host(in.channels(), kernelSize, times, in.data, in.step, in.cols, in.rows, result.data,
                                       result.step);
    if (st != PRL_OK) {
        out = in.clone();
        raise(st);
    }
    out = result;
}

// correctNUIL.cpp:55-90.  The reference's order: the empty check, cv::mean (at most 4 channels), then per channel
// getStructuringElement's assertion on the size before cv::morphologyEx runs.
void prl::correctNUIL(const cv::Mat& inputImage, cv::Mat& outputImage, int structuringElementSize)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for filtration is empty");
    if (inputImage.channels() > 4) PRL_FAIL_CV(cv::Error::StsAssert, "cn <= 4");                       // [upstream] cv::mean
    if (inputImage.depth() != CV_8U)
        PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::correctNUIL: 8-bit images only");          // documented deviation
    if (structuringElementSize < 1) PRL_FAIL_CV(cv::Error::StsAssert, "ksize.width > 0 && ksize.height > 0");
    cv::Mat result(inputImage.rows, inputImage.cols, inputImage.type());
    const int st = prl_hip_correct_nuil_host(inputImage.channels(), structuringElementSize, inputImage.data, inputImage.step,
                                             inputImage.cols, inputImage.rows, result.data, result.step);
    if (st != PRL_OK) raise(st);   // a size above 255: StsBadArg
    outputImage = result;
}

// removeLines.cpp:30-76.  The reference's order: cvtColor for 3 channels, cv::threshold (8UC1 only: its assertions cover the
// empty Mat, the other channel counts and depths), then getStructuringElement's assertion on a size of 0.
void prl::removeLines(const cv::Mat& inputImage, cv::Mat& outputImage)
{
    if (inputImage.empty()) PRL_FAIL_CV(cv::Error::StsAssert, "!_src.empty()");                      // [upstream] cv::threshold
    if (inputImage.depth() != CV_8U || (inputImage.channels() != 1 && inputImage.channels() != 3))
        PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::removeLines: 8-bit images of 1 or 3 channels only");
    if (inputImage.cols < 50 || inputImage.rows < 50)
        PRL_FAIL_CV(cv::Error::StsAssert, "ksize.width > 0 && ksize.height > 0");                   // [upstream] normalizeAnchor
    cv::Mat result(inputImage.rows, inputImage.cols, CV_8UC1);
    const int st = prl_hip_remove_lines_host(inputImage.channels(), inputImage.data, inputImage.step, inputImage.cols,
                                             inputImage.rows, result.data, result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

// gammaCorrection.cpp:52-106.  4 channels: cvtColor(BGRA2BGR), then the switch has no case for 4 - three channels come back
// with only the k step applied (prl_hip_gamma_correction_host reproduces it).
void prl::gammaCorrection(const cv::Mat& inputImage, cv::Mat& outputImage, const double k, const double gamma)
{
    if (inputImage.empty()) throw std::invalid_argument("Invalid parameter for GammaCorrectionFilter_OpenCV");
    if (inputImage.depth() != CV_8U)
        PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::gammaCorrection: 8-bit images only");        // documented deviation
    const int cn = inputImage.channels();
    if (cn > 4) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::gammaCorrection: 8-bit images of 1..4 channels only");
    cv::Mat result(inputImage.rows, inputImage.cols, CV_MAKETYPE(CV_8U, cn == 4 ? 3 : cn));
    const int st = prl_hip_gamma_correction_host(cn, k, gamma, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                                                 result.data, result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

// balanceSimpleWhite.cpp:33-142
void prl::simpleWhiteBalance(const cv::Mat& inputImage, cv::Mat& outputImage, const double k)
{
    if (inputImage.empty()) throw std::invalid_argument("SimpleWhiteBalance: input image is empty.");
    if (inputImage.channels() != 3) throw std::invalid_argument("SimpleWhiteBalance: input image hasn't 3 channels.");
    if (inputImage.depth() != CV_8U)
        PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::simpleWhiteBalance: 8-bit images only");     // documented deviation
    cv::Mat result(inputImage.rows, inputImage.cols, CV_8UC3);
    const int st = prl_hip_simple_white_balance_host(k, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows, result.data,
                                                     result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

// balanceGrayWorldWhite.cpp:58-115
void prl::grayWorldWhiteBalance(const cv::Mat& inputImage, cv::Mat& outputImage, const double pNorm, const bool withMax)
{
    if (inputImage.empty()) throw std::invalid_argument("GrayWorldWhiteBalance: input image is empty");
    if (inputImage.channels() != 3) throw std::invalid_argument("GrayWorldWhiteBalance: input image hasn't 3 channels");
    if (inputImage.depth() != CV_8U)
        PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::grayWorldWhiteBalance: 8-bit images only");  // documented deviation
    cv::Mat result(inputImage.rows, inputImage.cols, CV_8UC3);
    const int st = prl_hip_gray_world_host(pNorm, withMax ? 1 : 0, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                                           result.data, result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

// cleanBackgroundToWhite.cpp:39-64: the converters and channel rules of prl::backgroundNormalization
void prl::cleanBackgroundToWhite(const cv::Mat& inputImage, cv::Mat& outputImage)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for flipping is empty");   // cleanBackgroundToWhite.cpp:43-46
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "Cannot convert RAW image to Pix\n");   // formatConvert.cpp:103-104
    const int cn = inputImage.channels();
    if (cn != 1 && cn != 3 && cn != 4) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "Cannot convert RAW image to Pix\n");
    cv::Mat result(inputImage.rows, inputImage.cols, cn == 1 ? CV_8UC1 : CV_8UC3);
    const int st = prl_hip_clean_background_host(cn, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows, result.data,
                                                 result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

// binarizeMokji.cpp:35-94.  The reference's order: the two argument checks, then cv::cvtColor(BGR2GRAY) whatever the input is.
// The C layer takes the gray page: with OpenCV present the conversion is the installed cv::cvtColor, as everywhere in this file.
void prl::binarizeMokji(const cv::Mat& inputImage, cv::Mat& outputImage, size_t maxEdgeWidth, size_t minEdgeMagnitude)
{
    if (maxEdgeWidth < 1) throw std::invalid_argument("mokjiThreshold: invalid maxEdgeWidth");
    if (minEdgeMagnitude < 1) throw std::invalid_argument("mokjiThreshold: invalid minEdgeMagnitude");
    if (inputImage.empty() || (inputImage.channels() != 3 && inputImage.channels() != 4)) raise(PRL_ERR_BAD_CHANNELS);
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::binarizeMokji: 8-bit images only");
    // into int without changing the result: 256 and above is "no pair"; 2^30 and above leaves no interior on any Mat
    const int M = (int)(minEdgeMagnitude < 256 ? minEdgeMagnitude : 256);
    const int E = (int)(maxEdgeWidth < ((size_t)1 << 30) ? maxEdgeWidth : ((size_t)1 << 30));
    cv::Mat gray = inputImage;      // a header: the conversion gives it a buffer of its own, the input's pixels are only read
    bgr2gray_inplace(gray);
    cv::Mat result(gray.rows, gray.cols, CV_8UC1);
    const int st = prl_hip_binarize_mokji_host(1, E, M, gray.data, gray.step, gray.cols, gray.rows, result.data, result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

// blurDetection.cpp:85-89: "TODO: find constants for blurring check for every algorithm", return false
bool prl::isBlurred(const cv::Mat&)
{
    return false;
}

// blurDetection.cpp:32-83, channel 0 (cv::mean(FM).val[0], sigma.val[0], mu.val[0])
prl::FocusMeasures prl::focusMeasures(const cv::Mat& inputImage, int tengKernelSize)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for focus measures is empty");
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::focusMeasures: 8-bit images only");
    const int cn = inputImage.channels();
    if (cn != 1 && cn != 3 && cn != 4) raise(PRL_ERR_BAD_CHANNELS);
    double m[4 * 4];
    const int st = prl_hip_focus_measures_host(cn, tengKernelSize, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows, m,
                                               nullptr);
    if (st != PRL_OK) raise(st);
    return prl::FocusMeasures{m[PRL_FOCUS_LAPM], m[PRL_FOCUS_LAPV], m[PRL_FOCUS_TENG], m[PRL_FOCUS_GLVN]};
}

// basicDeblur.cpp:33-70.  The reference's order: the empty check, cv::split and convertTo (any depth, any channel count), then
// cv::GaussianBlur's assertion on the kernel size.
void prl::basicDeblur(const cv::Mat& inputImage, cv::Mat& outputImage, const size_t gaussianKernelSize, const double sigmaX,
                      const double sigmaY, const double imageWeight)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for deblurring is empty");
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsNotImplemented, "prl::basicDeblur: 8-bit images only");   // documented deviation
    const int cn = inputImage.channels();
    if (cn > 4) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::basicDeblur: 8-bit images of 1..4 channels only");
    if (gaussianKernelSize > (size_t)2147483647) PRL_FAIL_CV(cv::Error::StsBadArg, "prl::basicDeblur: the kernel size does not fit an int");
    const long long k = (long long)gaussianKernelSize;
    const double sy = sigmaY <= 0 ? sigmaX : sigmaY;
    if (k > 0 ? k % 2 != 1 : !(sigmaX > 0 && sy > 0))   // [upstream] createGaussianKernels
        PRL_FAIL_CV(cv::Error::StsAssert, "ksize.width > 0 && ksize.width % 2 == 1 && ksize.height > 0 && ksize.height % 2 == 1");
    int kw = 0, kh = 0;
    int st = prl_hip_gaussian_blur_size(k, k, sigmaX, sigmaY, &kw, &kh);
    if (st == PRL_ERR_BAD_WINDOW) PRL_FAIL_CV(cv::Error::StsBadArg, "prl::basicDeblur: kernel sides up to 255 only");   // documented deviation
    if (st != PRL_OK) raise(st);
    cv::Mat result(inputImage.rows, inputImage.cols, inputImage.type());
    st = prl_hip_basic_deblur_host(cn, k, sigmaX, sigmaY, imageWeight, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                                   result.data, result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

namespace {

// what the three contrast functions share: the reference's empty check, the depth and channel limits, a new Mat for the result
template <typename Call>
void contrast_call(const cv::Mat& in, cv::Mat& out, const char* what, Call&& call)
{
    if (in.empty()) throw std::invalid_argument("Image for histograms enhancing is empty");
    if (in.depth() != CV_8U || in.channels() > 4)
        fail_cv(cv::Error::StsUnsupportedFormat, std::string(what) + ": 8-bit images of 1..4 channels only", what, __LINE__);   // documented deviation
    cv::Mat result(in.rows, in.cols, in.type());
    const int st = call(in.channels(), in.data, in.step, in.cols, in.rows, result.data, result.step);
    if (st != PRL_OK) raise_at(st, what, __LINE__);   // (the exception names the public function, not this helper)
    out = result;
}

}  // namespace

// imageLibCommon.cpp:327-395: _1 for one channel, _MCh (split, per channel, merge) for more - the same thing per channel
void EnhanceLocalContrastByCLAHE(cv::Mat& inputImage, cv::Mat& outputImage, double CLAHEClipLimit, bool equalizeHistFlag)
{
    contrast_call(inputImage, outputImage, "EnhanceLocalContrastByCLAHE",
                  [&](int cn, const unsigned char* s, size_t ss, int w, int h, unsigned char* d, size_t ds) {
                      return prl_hip_enhance_local_contrast_host(cn, CLAHEClipLimit, equalizeHistFlag ? 1 : 0, s, ss, w, h, d, ds);
                  });
}

void prl::clahe(const cv::Mat& inputImage, cv::Mat& outputImage, double clipLimit, int tilesX, int tilesY)
{
    contrast_call(inputImage, outputImage, "prl::clahe", [&](int cn, const unsigned char* s, size_t ss, int w, int h, unsigned char* d, size_t ds) {
        return prl_hip_clahe_host(cn, clipLimit, tilesX, tilesY, s, ss, w, h, d, ds);
    });
}

void prl::equalizeHist(const cv::Mat& inputImage, cv::Mat& outputImage)
{
    contrast_call(inputImage, outputImage, "prl::equalizeHist", [&](int cn, const unsigned char* s, size_t ss, int w, int h, unsigned char* d, size_t ds) {
        return prl_hip_equalize_hist_host(cn, s, ss, w, h, d, ds);
    });
}

void prl::bilateralFilter(const cv::Mat& inputImage, cv::Mat& outputImage, int d, double sigmaColor, double sigmaSpace)
{
    if (inputImage.empty()) throw std::invalid_argument("Image for bilateral filtration is empty");
    if (inputImage.data == outputImage.data) PRL_FAIL_CV(cv::Error::StsAssert, "src.data != dst.data");
    contrast_call(inputImage, outputImage, "prl::bilateralFilter", [&](int cn, const unsigned char* s, size_t ss, int w, int h, unsigned char* dd, size_t ds) {
        return prl_hip_bilateral_filter_host(cn, d, sigmaColor, sigmaSpace, s, ss, w, h, dd, ds);
    });
}

namespace {

// CannyEdgeDetection's own checks in the reference's order (imageLibCommon.cpp:253-272), then cv::GaussianBlur's assertion
void canny_edge_checks(int size, double upper, double lower, const char* func, int line)
{
    if (size < 3) throw std::invalid_argument("Gaussian blur kernel size is lesser than 3");
    if (upper < 0 || upper > 1 || upper != upper) throw std::invalid_argument("Canny upper threshold coefficient isn't in range [0;1]");
    if (lower < 0 || lower > 1 || lower != lower) throw std::invalid_argument("Canny lower threshold coefficient isn't in range [0;1]");
    if (lower > upper)
        throw std::invalid_argument("Canny lower threshold coefficient is greater than Canny upper threshold coefficient");
    if (size % 2 != 1)
        fail_cv(cv::Error::StsAssert, "ksize.width > 0 && ksize.width % 2 == 1 && ksize.height > 0 && ksize.height % 2 == 1", func, line);
}

}  // namespace

void CannyEdgeDetection(cv::Mat& imageToProc, cv::Mat& resultCanny, int GaussianBlurKernelSize, double CannyUpperThresholdCoeff,
                        double CannyLowerThresholdCoeff, int CannyMorphIters)
{
    if (imageToProc.empty()) throw std::invalid_argument("Image for histograms extraction is empty");
    canny_edge_checks(GaussianBlurKernelSize, CannyUpperThresholdCoeff, CannyLowerThresholdCoeff, __func__, __LINE__);
    if (imageToProc.depth() != CV_8U || imageToProc.channels() > 4)
        PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "CannyEdgeDetection: 8-bit images of 1..4 channels only");   // documented deviation
    if (GaussianBlurKernelSize > PRL_GAUSS_MAX_SIDE) PRL_FAIL_CV(cv::Error::StsBadArg, "CannyEdgeDetection: kernel sizes up to 255 only");
    cv::Mat result(imageToProc.rows, imageToProc.cols, CV_8UC1);
    const int st = prl_hip_canny_edge_detection_host(imageToProc.channels(), GaussianBlurKernelSize, CannyUpperThresholdCoeff,
                                                     CannyLowerThresholdCoeff, CannyMorphIters, imageToProc.data, imageToProc.step,
                                                     imageToProc.cols, imageToProc.rows, result.data, result.step);
    if (st != PRL_OK) raise(st);
    resultCanny = result;
}

// binarizeLocalOtsu.cpp:37-163 in the reference's statement order: its two checks, the gray conversion (cv::cvtColor rejects two
// channels), CannyEdgeDetection's checks, and RemoveChildrenContours' exception for an edge map without contours.
void prl::binarizeLocalOtsu(cv::Mat& inputImage, cv::Mat& outputImage, double maxValue, double CLAHEClipLimit, int GaussianBlurKernelSize,
                            double CannyUpperThresholdCoeff, double CannyLowerThresholdCoeff, int CannyMorphIters)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for binarization is empty");
    if (!(maxValue >= 0 && maxValue <= 255)) throw std::invalid_argument("Max value must be in range [0; 255]");
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl: 8-bit images only");
    const int cn = inputImage.channels();
    if (cn != 1 && cn != 3 && cn != 4) raise(PRL_ERR_BAD_CHANNELS);
    canny_edge_checks(GaussianBlurKernelSize, CannyUpperThresholdCoeff, CannyLowerThresholdCoeff, __func__, __LINE__);
    if (GaussianBlurKernelSize > PRL_GAUSS_MAX_SIDE) PRL_FAIL_CV(cv::Error::StsBadArg, "prl::binarizeLocalOtsu: kernel sizes up to 255 only");
    cv::Mat result(inputImage.rows, inputImage.cols, CV_8UC1);
    int32_t found = 0, kept = 0;
    const int st = prl_hip_binarize_local_otsu_host(cn, maxValue, CLAHEClipLimit, GaussianBlurKernelSize, CannyUpperThresholdCoeff,
                                                    CannyLowerThresholdCoeff, CannyMorphIters, inputImage.data, inputImage.step,
                                                    inputImage.cols, inputImage.rows, result.data, result.step, &found, &kept);
    if (st != PRL_OK) raise(st);
    if (found == 0) throw std::invalid_argument("Contours array is empty");   // RemoveChildrenContours, imageLibCommon.cpp:643-646
    outputImage = result;
}

// binarizeFBCITB.cpp:73-404 in the reference's statement order: the empty check, the type check with its side effect on a
// one-channel image (cv::cvtColor(inputImage, inputImage, COLOR_GRAY2BGR)), then - where the Canny stage runs - CannyEdgeDetection's
// checks.  The C layer takes the BGR page; a page without contours is all 255, as the reference's early return makes it.
void prl::binarizeFBCITB(cv::Mat& inputImage, cv::Mat& outputImage, bool useCanny, bool useVariancesMap, bool useCLAHE, bool useBilateral,
                         bool useOtherColorspace, bool useMorphology, bool useCannyOnVariances, double varianceMapThreshold,
                         double CLAHEClipLimit, double gaussianBlurKernelSize, double cannyUpperThresholdCoeff,
                         double cannyLowerThresholdCoeff, double boundingRectangleMaxArea, int bilateralKernelSize,
                         double bilateralKernelIntensitySigma, double bilateralKernelSpatialSigma, double boundingRectMaxAreaCoeff)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for binarization is empty");
    if (inputImage.type() != CV_8UC3) {
        if (inputImage.channels() != 1 || inputImage.depth() != CV_8U)
            throw std::invalid_argument("Invalid type of image for binarization (required 24 bits per pixel)");
#ifdef PRL_HAVE_OPENCV
        cv::cvtColor(inputImage, inputImage, cv::COLOR_GRAY2BGR);
#else
        cv::Mat bgr(inputImage.rows, inputImage.cols, CV_8UC3);
        for (int y = 0; y < inputImage.rows; ++y) {
            const unsigned char* s = inputImage.ptr(y);
            unsigned char* d = bgr.ptr(y);
            for (int x = 0; x < inputImage.cols; ++x) d[3 * x] = d[3 * x + 1] = d[3 * x + 2] = s[x];
        }
        inputImage = bgr;
#endif
    }
    prl_fbcitb_params p;
    prl_hip_default_fbcitb_params(&p);
    p.use_canny = useCanny; p.use_variances_map = useVariancesMap; p.use_clahe = useCLAHE; p.use_bilateral = useBilateral;
    p.use_other_colorspace = useOtherColorspace; p.use_morphology = useMorphology; p.use_canny_on_variances = useCannyOnVariances;
    p.variance_map_threshold = varianceMapThreshold; p.clahe_clip_limit = CLAHEClipLimit;
    p.gaussian_blur_kernel_size = gaussianBlurKernelSize;
    p.canny_upper_threshold_coeff = cannyUpperThresholdCoeff; p.canny_lower_threshold_coeff = cannyLowerThresholdCoeff;
    p.bounding_rectangle_max_area = boundingRectangleMaxArea; p.bilateral_kernel_size = bilateralKernelSize;
    p.bilateral_kernel_intensity_sigma = bilateralKernelIntensitySigma; p.bilateral_kernel_spatial_sigma = bilateralKernelSpatialSigma;
    p.bounding_rect_max_area_coeff = boundingRectMaxAreaCoeff;
    if ((useCanny || !useVariancesMap) && gaussianBlurKernelSize == gaussianBlurKernelSize && gaussianBlurKernelSize < 2147483647.0 &&
        gaussianBlurKernelSize > -2147483647.0) {
        const int size = static_cast<int>(gaussianBlurKernelSize);
        canny_edge_checks(size, cannyUpperThresholdCoeff, cannyLowerThresholdCoeff, __func__, __LINE__);
        if (size > PRL_GAUSS_MAX_SIDE) PRL_FAIL_CV(cv::Error::StsBadArg, "prl::binarizeFBCITB: kernel sizes up to 255 only");
    }
    cv::Mat result(inputImage.rows, inputImage.cols, CV_8UC1);
    const int st = prl_hip_binarize_fbcitb_host(&p, 3, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows, result.data,
                                                result.step, nullptr);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

namespace {

constexpr int kAdaptiveMaxBlock = 255;   // prl_hip.h: block_size 3 .. 255

// cv::medianBlur's own checks ([upstream] OpenCV >= 4), as prl::denoiseSaltPepper states them
void median_checks(const cv::Mat& in, int ksize, const char* func, int line)
{
    if (ksize % 2 != 1) fail_cv(cv::Error::StsAssert, "(ksize % 2 == 1) && (_src0.dims() <= 2 )", func, line);
    if (in.depth() != CV_8U || in.channels() > 4)
        fail_cv(cv::Error::StsUnsupportedFormat, "prl: cv::medianBlur on 8-bit images of 1..4 channels only", func, line);
    if (in.channels() == 2 && ksize >= 7) fail_cv(cv::Error::StsAssert, "cn == 1 || cn == 3 || cn == 4", func, line);
}

// cv::adaptiveThreshold's CV_Assert( blockSize % 2 == 1 && blockSize > 1 ), then this library's own limit
void block_checks(int blockSize, const char* func, int line)
{
    if (!(blockSize % 2 == 1 && blockSize > 1)) fail_cv(cv::Error::StsAssert, "blockSize % 2 == 1 && blockSize > 1", func, line);
    if (blockSize > kAdaptiveMaxBlock)
        fail_cv(cv::Error::StsNotImplemented, "prl: cv::adaptiveThreshold with a block size above 255 is not provided", func, line);
}

void adaptive_call(const prl_adaptive_params& p, const cv::Mat& in, cv::Mat& out, const char* func, int line)
{
    cv::Mat result(in.rows, in.cols, CV_8UC1);
    const int st = prl_hip_binarize_adaptive_host(&p, in.channels(), in.data, in.step, in.cols, in.rows, result.data, result.step);
    if (st != PRL_OK) raise_at(st, func, line);
    out = result;
}

// binarizeAT.cpp:33-68, binarizeAGT.cpp:33-60 (median != 0), binarizePureAdaptiveGaussian.cpp:32-75 (median == 0)
void at_impl(const cv::Mat& in, cv::Mat& out, bool with_median, int medianKernelSize, int method, double maxValue, int blockSize,
             int shift, const char* func)
{
    if (in.empty()) throw std::invalid_argument("Input image for binarization is empty");
    if (with_median) median_checks(in, medianKernelSize, func, __LINE__);
    else if (in.depth() != CV_8U) fail_cv(cv::Error::StsUnsupportedFormat, "prl: 8-bit images only", func, __LINE__);
    // 1 channel: the reference hands an EMPTY Mat to cv::adaptiveThreshold (binarizeAT.cpp:56-65); [upstream] OpenCV >= 4
    // asserts on it.  outputImage stays as it was.
    if (in.channels() == 1) fail_cv(cv::Error::StsAssert, "!_src.empty()", func, __LINE__);
    if (in.channels() != 3 && in.channels() != 4) raise_at(PRL_ERR_BAD_CHANNELS, func, __LINE__);   // cv::cvtColor(BGR2GRAY)
    block_checks(blockSize, func, __LINE__);
    prl_adaptive_params p{};
    p.median_ksize = with_median ? medianKernelSize : 0;
    p.median_on_color = 1;
    p.method = method;
    p.type = PRL_THRESH_BINARY;
    p.max_value = maxValue;
    p.block_size = blockSize;
    p.delta = (double)shift;
    p.auto_invert = 0;
    adaptive_call(p, in, out, func, __LINE__);
}

}  // namespace

// binarizeNativeAdaptive.cpp:34-135 in the reference's statement order.
void prl::binarizeNativeAdaptive(cv::Mat& inputImage, cv::Mat& outputImage, bool isGaussianBlurReqiured, int medianBlurKernelSize,
                                 int GaussianBlurKernelSize, double GaussianBlurSigma, bool isAdaptiveThresholdCalculatedByGaussian,
                                 double adaptiveThresholdingMaxValue, int adaptiveThresholdingBlockSize,
                                 double adaptiveThresholdingShift, int bilateralFilterBlockSize, double bilateralFilterColorSigma,
                                 double bilateralFilterSpaceSigma)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for binarization is empty");
    if (!(adaptiveThresholdingMaxValue >= 0 && adaptiveThresholdingMaxValue <= 255))
        throw std::invalid_argument("Max value must be in range [0; 255]");
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl: 8-bit images only");
    if (inputImage.channels() > 1) {
        if (inputImage.channels() != 3 && inputImage.channels() != 4) raise(PRL_ERR_BAD_CHANNELS);
#ifndef PRL_KEEP_INPUT
        bgr2gray_inplace(inputImage);   // cv::cvtColor(inputImage, inputImage, cv::COLOR_BGR2GRAY) - :60
#endif
    }
    if (!isGaussianBlurReqiured) {
        if (!(medianBlurKernelSize >= 3)) PRL_FAIL_CV(cv::Error::StsAssert, "medianBlurKernelSize >= 3");
        median_checks(inputImage, medianBlurKernelSize, __func__, __LINE__);
    } else {
        if (!(GaussianBlurKernelSize >= 3)) PRL_FAIL_CV(cv::Error::StsAssert, "GaussianBlurKernelSize >= 3");
        if (!(GaussianBlurSigma > 0)) PRL_FAIL_CV(cv::Error::StsAssert, "GaussianBlurSigma > 0");
        PRL_FAIL_CV(cv::Error::StsNotImplemented,
                    "prl::binarizeNativeAdaptive with isGaussianBlurReqiured needs OpenCV's 8-bit fixed-point cv::GaussianBlur, which this library does not provide");
    }
    if (adaptiveThresholdingBlockSize < 3) {
        const double diagonal = std::sqrt((double)(inputImage.rows * inputImage.rows + inputImage.cols * inputImage.cols));
        adaptiveThresholdingBlockSize = static_cast<int>(diagonal / 333 + 7);   // may be even: cv::adaptiveThreshold then throws
    }
    block_checks(adaptiveThresholdingBlockSize, __func__, __LINE__);
    prl_adaptive_params p{};
    p.median_ksize = medianBlurKernelSize;
    p.median_on_color = 0;
    p.method = isAdaptiveThresholdCalculatedByGaussian ? PRL_ADAPTIVE_GAUSSIAN_C : PRL_ADAPTIVE_MEAN_C;
    p.type = PRL_THRESH_BINARY_INV;
    p.max_value = adaptiveThresholdingMaxValue;
    p.block_size = adaptiveThresholdingBlockSize;
    p.delta = adaptiveThresholdingShift;
    p.auto_invert = 1;
    adaptive_call(p, inputImage, outputImage, __func__, __LINE__);
    if (bilateralFilterBlockSize >= 3) {   // outputImage holds the mask, as in the reference (:113-133)
        if (bilateralFilterColorSigma <= 0) throw std::invalid_argument("Color sigma for bilateral filtration must be greater than 0");
        if (bilateralFilterSpaceSigma <= 0) throw std::invalid_argument("Space sigma for bilateral filtration must be greater than 0");
        PRL_FAIL_CV(cv::Error::StsNotImplemented,
                    "prl::binarizeNativeAdaptive with bilateralFilterBlockSize >= 3 needs cv::bilateralFilter, which this library does not provide");
    }
}

void prl::binarizeAT(const cv::Mat& inputImage, cv::Mat& outputImage, const int medianKernelSize, const double maxValue,
                     const int blockSize, const int shift)
{
    at_impl(inputImage, outputImage, true, medianKernelSize, PRL_ADAPTIVE_MEAN_C, maxValue, blockSize, shift, __func__);
}

void prl::binarizeAGT(const cv::Mat& inputImage, cv::Mat& outputImage, const int medianKernelSize, const double maxValue,
                      const int blockSize, const int shift)
{
    at_impl(inputImage, outputImage, true, medianKernelSize, PRL_ADAPTIVE_GAUSSIAN_C, maxValue, blockSize, shift, __func__);
}

void prl::binarizePureAdaptiveGaussian(const cv::Mat& inputImage, cv::Mat& outputImage, const double maxValue, const int blockSize,
                                       const int shift)
{
    at_impl(inputImage, outputImage, false, 0, PRL_ADAPTIVE_GAUSSIAN_C, maxValue, blockSize, shift, __func__);
}

namespace {
void lv_impl(int with_filters, cv::Mat& in, cv::Mat& out, double coeff, int minVar, double gamma, const char* empty_msg)
{
    if (in.empty()) throw std::invalid_argument(empty_msg);
    // [upstream] MatToLocalVarianceMap accepts 8UC1 / 8UC3 (imageLibCommon.cpp:404-408), but the callers index three planes
    if (in.type() != CV_8UC3)
        throw std::invalid_argument("Image for local variance map extraction has unsupported type (3 channels, 8 bits required here)");
    cv::Mat result(in.rows, in.cols, CV_8UC1);
    const int st = prl_hip_binarize_lv_host(with_filters, coeff, minVar, gamma, in.data, in.step, in.cols, in.rows, result.data, result.step);
    if (st != PRL_OK) raise(st);
    out = result;
}
}  // namespace

void prl::binarizeByLocalVariances(cv::Mat& inputImage, cv::Mat& outputImage, double varianceThresholdCoeff, int minResultVariance,
                                   double gamma)
{
    lv_impl(1, inputImage, outputImage, varianceThresholdCoeff, minResultVariance, gamma,
            "binarizeByLocalVariances: Input inputImage for binarization is empty");
}

void prl::binarizeByLocalVariancesWithoutFilters(cv::Mat& inputImage, cv::Mat& outputImage, double varianceThresholdCoeff,
                                                 int minResultVariance)
{
    lv_impl(0, inputImage, outputImage, varianceThresholdCoeff, minResultVariance, 2.0,
            "binarizeByLocalVariancesWithoutFilters: Input inputImage for binarization is empty");
}

void prl::backgroundNormalization(const cv::Mat& inputImage, cv::Mat& outputImage)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for flipping is empty");  // backgroundNormalization.cpp:40-43
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "Cannot convert RAW image to Pix\n");   // formatConvert.cpp:103-104
    const int cn = inputImage.channels();
    if (cn != 1 && cn != 3 && cn != 4) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "Cannot convert RAW image to Pix\n");
    cv::Mat result(inputImage.rows, inputImage.cols, cn == 1 ? CV_8UC1 : CV_8UC3);
    const int st = prl_hip_bgnorm_host(cn, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows, result.data,
                                       result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

void prl::rotate(const cv::Mat& inputImage, cv::Mat& outputImage, double angle)
{
    if (inputImage.empty()) raise(PRL_ERR_EMPTY);  // [upstream] cv::transpose / cv::warpAffine assert on an empty source
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::rotate: 8-bit images only");
    int ow = 0, oh = 0;
    int st = prl_hip_rotate_out_size(inputImage.cols, inputImage.rows, angle, &ow, &oh);
    if (st != PRL_OK) raise(st);
    cv::Mat result(oh, ow, inputImage.type());
    st = prl_hip_rotate_host(inputImage.channels(), angle, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                             result.data, result.step);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

void prl::warpCrop(const cv::Mat& inputImage, cv::Mat& outputImage, const int x0, const int y0, const int x1, const int y1, const int x2,
                   const int y2, const int x3, const int y3, double ratio, const int borderMode, const cv::Scalar& borderValue)
{
    if (inputImage.empty()) PRL_FAIL_CV(cv::Error::StsAssert, "!_src.empty()");  // [upstream] cv::warpPerspective's own check
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::warpCrop: 8-bit images only");
    if (inputImage.channels() > 4) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::warpCrop: at most 4 channels");
    if (borderMode != PRL_BORDER_CONSTANT && borderMode != PRL_BORDER_REPLICATE)
        PRL_FAIL_CV(cv::Error::StsNotImplemented, "prl::warpCrop: border modes other than BORDER_CONSTANT and BORDER_REPLICATE are not provided");
    const int32_t quad[8] = {x0, y0, x1, y1, x2, y2, x3, y3};
    int ow = 0, oh = 0;
    int st = prl_hip_warp_crop_size(quad, ratio, &ow, &oh);
    if (st != PRL_OK) raise(st);
    cv::Mat result(oh, ow, inputImage.type());
    const double value[4] = {borderValue.val[0], borderValue.val[1], borderValue.val[2], borderValue.val[3]};
    st = prl_hip_warp_crop_host(inputImage.channels(), quad, ratio, inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                                result.data, result.step, borderMode, value);
    if (st != PRL_OK) raise(st);
    outputImage = result;
}

void prl::warpCrop(cv::Mat& inputImage, cv::Mat& outputImage, const std::vector<cv::Point>& points, double ratio, int borderMode,
                   const cv::Scalar& borderValue)
{
    if (inputImage.empty()) throw std::invalid_argument("Image for warping is empty");   // warp.cpp:82-85
    if (points.size() != 4) throw std::invalid_argument("Size of array of base points for warping isn't equal 4");   // :87-90
    // (cvRound of an int coordinate is the coordinate, :92-99)
    warpCrop(inputImage, outputImage, points[0].x, points[0].y, points[1].x, points[1].y, points[2].x, points[2].y, points[3].x,
             points[3].y, ratio, borderMode, borderValue);
}

// autoCrop.cpp:43-131.  The reference reads the image without a check of its own: an empty one fails in cv::meanStdDev / cv::split
// [upstream]; here it is the C layer's PRL_ERR_EMPTY, std::invalid_argument.
bool prl::documentContour(cv::Mat& inputImage, const double scaleX, const double scaleY, std::vector<cv::Point_<float> >& resultContour)
{
    if (scaleX > 0 && scaleY > 0)
        PRL_FAIL_CV(cv::Error::StsNotImplemented, "prl::documentContour: positive scaleX / scaleY (cv::resize, INTER_AREA) are not provided");
    if (inputImage.empty()) raise(PRL_ERR_EMPTY);
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::documentContour: 8-bit images only");
    float quad[8];
    int32_t found = 0;
    const int st = prl_hip_document_contour_host(inputImage.channels(), inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                                                 quad, &found, nullptr);
    if (st != PRL_OK) raise(st);
    if (!found) {
        resultContour.clear();   // :116
        return false;
    }
    // findDocumentContour appends its four corners to what the caller's vector holds (autoCropUtils.cpp:248-256); scaleContour
    // and cropVerticesOrdering then want exactly four, so anything but an empty vector throws there (:278-281)
    if (!resultContour.empty()) throw std::invalid_argument("Points number in input contour isn't equal 4");
    for (int i = 0; i < 4; ++i) resultContour.push_back(cv::Point_<float>(quad[2 * i], quad[2 * i + 1]));
    return true;
}

// autoCrop.cpp:133-175
bool prl::autoCrop(cv::Mat& inputImage, cv::Mat& outputImage)
{
    if (inputImage.empty()) throw std::invalid_argument("autoCrop: Image for cropping is empty");
    if (inputImage.type() == CV_8UC1) {   // cv::cvtColor(inputImage, inputImage, cv::COLOR_GRAY2BGR): the caller's Mat becomes BGR
#ifdef PRL_HAVE_OPENCV
        cv::cvtColor(inputImage, inputImage, cv::COLOR_GRAY2BGR);
#else
        cv::Mat bgr(inputImage.rows, inputImage.cols, CV_8UC3);
        for (int y = 0; y < inputImage.rows; ++y) {
            const unsigned char* s = inputImage.ptr(y);
            unsigned char* d = bgr.ptr(y);
            for (int x = 0; x < inputImage.cols; ++x) d[3 * x] = d[3 * x + 1] = d[3 * x + 2] = s[x];
        }
        inputImage = bgr;
#endif
    }
    std::vector<cv::Point_<float> > resultContour;
    if (!documentContour(inputImage, -1, -1, resultContour)) return false;
    std::vector<cv::Point> temp;
    temp.reserve(resultContour.size());
    for (const auto& point : resultContour) temp.push_back(cv::Point((int)point.x, (int)point.y));   // :164-169: truncated
    warpCrop(inputImage, outputImage, temp);
    return true;
}

// houghLine.cpp:177-256
bool prl::findHoughLineContour(cv::Mat& inputImage, std::vector<cv::Point>& resultContour)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image is empty");
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::findHoughLineContour: 8-bit images only");
    int32_t quad[8], found = 0;
    const int st = prl_hip_hough_line_contour_host(inputImage.channels(), inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                                                   quad, &found, nullptr);
    if (st != PRL_OK) raise(st);
    if (!found) return false;
    for (int i = 0; i < 4; ++i) resultContour.push_back(cv::Point(quad[2 * i], quad[2 * i + 1]));   // :248-251: appended
    return true;
}

void prl::resize(const cv::Mat& src, cv::Mat& dst, int scaleX, int scaleY, int maxSize)
{
    const bool by_scale = scaleX > 0 && scaleY > 0;
    if (!by_scale && maxSize < 1) PRL_FAIL_CV(cv::Error::StsBadArg, "prl::resize: maxSize < 1 (the reference never returns)");
    if (src.empty()) {
        if (by_scale) PRL_FAIL_CV(cv::Error::StsAssert, "!ssize.empty()");   // [upstream] cv::resize's own check
        dst = cv::Mat();                                                     // src.clone(), and no level to take (resize.cpp:49-51)
        return;
    }
    if (src.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::resize: 8-bit images only");
    if (src.channels() > 4) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::resize: at most 4 channels");
    int st, levels = 0, ow = src.cols, oh = src.rows;
    if (by_scale) {
        if ((long long)src.cols * scaleX > 32768 || (long long)src.rows * scaleY > 32768) raise(PRL_ERR_BAD_ARG);
        ow = src.cols * scaleX;
        oh = src.rows * scaleY;
    } else if ((st = prl_hip_resize_pyramid_levels(src.cols, src.rows, maxSize, &levels, &ow, &oh)) != PRL_OK) {
        raise(st);
    }
    cv::Mat result(oh, ow, src.type());
    if (by_scale) {
        st = prl_hip_resize_replicate_host(src.channels(), scaleX, scaleY, src.data, src.step, src.cols, src.rows, result.data, result.step);
    } else if (levels == 0) {   // dst = src.clone()
        for (int y = 0; y < src.rows; ++y) std::memcpy(result.ptr(y), src.ptr(y), (size_t)src.cols * src.channels());
        st = PRL_OK;
    } else {
        st = prl_hip_pyr_down_host(src.channels(), levels, src.data, src.step, src.cols, src.rows, result.data, result.step);
    }
    if (st != PRL_OK) raise(st);
    dst = result;
}

bool prl::deskew(const cv::Mat& inputImage, cv::Mat& outputImage)
{
    if (inputImage.empty()) PRL_FAIL_CV(cv::Error::StsAssert, "!inputImage.empty()");  // CV_Assert, deskew.cpp:210
    if (inputImage.depth() != CV_8U) PRL_FAIL_CV(cv::Error::StsUnsupportedFormat, "prl::deskew: 8-bit images only");
    const int len = inputImage.cols > inputImage.rows ? inputImage.cols : inputImage.rows;
    cv::Mat big(len, len, inputImage.type());
    int ow = 0, oh = 0;
    const int st = prl_hip_deskew_host(inputImage.channels(), inputImage.data, inputImage.step, inputImage.cols, inputImage.rows,
                                       big.data, big.step, &ow, &oh, nullptr);
    if (st != PRL_OK) raise(st);
    outputImage = (ow == len && oh == len) ? big : big(cv::Rect(0, 0, ow, oh)).clone();
    return !outputImage.empty();  // deskew.cpp:245-250
}

// deskew.h:62, deskew.cpp:139-205.  The reference hands cv::HoughLinesP the complement of the page; HoughLinesP takes
// CV_8UC1 only ([upstream] CV_Assert(image.type() == CV_8UC1)) and finds no line on an empty image, so 0.0 (:154-157).
double prl::findAngle(const cv::Mat& inputImage)
{
    if (inputImage.empty()) return 0.0;
    if (inputImage.type() != CV_8UC1) PRL_FAIL_CV(cv::Error::StsAssert, "image.type() == CV_8UC1");
    double angle = 0.0;
    const int st = prl_hip_find_angle_host(inputImage.data, inputImage.step, inputImage.cols, inputImage.rows, &angle, nullptr);
    if (st != PRL_OK) raise(st);
    return angle;
}

// deskew.h:52, deskew.cpp:70-136.  The reference fills its gray page only for 3-channel input (:73-76), thresholds it
// (cv::adaptiveThreshold, :78) and asks Leptonica's pixOrientDetectDwa / makeOrientDecision for one of four orientations
// (:91, :101).  prl::deskew - its only caller (:238) - always hands it the 1-channel thresholded page, for which the gray page
// is EMPTY: the function leaves through its NULL-pix exit with 0 (:80-84) or throws inside adaptiveThreshold, depending on the
// OpenCV version.  This layer answers that 0.0 for every input that is not 3-channel: the orientation step of the hot path is a
// no-op.  For a 3-CHANNEL caller the reference really looks (and can answer 90 / 180 / 270): Leptonica's
// DWA text-orientation detector is outside this library's scope and its source is not available to restate - such
// a call fails loudly instead of answering "up" without having looked.
double prl::findOrientation(const cv::Mat& inputImage)
{
    if (!inputImage.empty() && inputImage.channels() == 3)
        PRL_FAIL_CV(cv::Error::StsNotImplemented,
                    "prl::findOrientation on a 3-channel image needs Leptonica's pixOrientDetectDwa (deskew.cpp:91), which this library does not provide");
    return 0.0;
}

namespace {
void thin_impl(int method, cv::Mat& inputImage, cv::Mat& outputImage)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for thinning is empty");
    if (inputImage.type() != CV_8UC3 && inputImage.type() != CV_8UC1)
        throw std::invalid_argument("Invalid type of image for thinning (required 8 or 24 bits per pixel)");
    // The reference works on the caller's buffer when input and output share data, else on a clone (thinZhangSuen.cpp:71-80).
    // In place, 1 channel: every step (&= 1, the iterations, *= 255 at :100-103) writes through the shared buffer; the two headers
    // stay as they are.  In place, 3 channels: cvtColor (:84) gives the working Mat a new 1-channel buffer, the skeleton is
    // computed there and dropped - neither of the caller's Mats changes (reproduced: nothing to compute).
    const bool in_place = inputImage.data == outputImage.data;
    if (in_place && inputImage.channels() == 3) return;
    cv::Mat work = in_place ? inputImage : inputImage.clone();
    if (work.channels() == 3) bgr2gray_inplace(work);
    cv::Mat result(work.rows, work.cols, CV_8UC1);
    const int st = prl_hip_thin_host(method, work.data, work.step, work.cols, work.rows, result.data, result.step);
    if (st != PRL_OK) raise(st);
    if (in_place) {
        for (int y = 0; y < result.rows; ++y) std::memcpy(inputImage.ptr(y), result.ptr(y), (size_t)result.cols);
        return;
    }
    outputImage = result;
}
}  // namespace

void prl::thinZhangSuen(cv::Mat& inputImage, cv::Mat& outputImage) { thin_impl(PRL_THIN_ZHANGSUEN, inputImage, outputImage); }
void prl::thinGuoHall(cv::Mat& inputImage, cv::Mat& outputImage) { thin_impl(PRL_THIN_GUOHALL, inputImage, outputImage); }

// Global Otsu on the host (BASELINE config 1: plumbing, no GPU).  [upstream getThreshVal_Otsu_8u]
void prl::binarize(cv::Mat& inputImage, cv::Mat& outputImage)
{
    if (inputImage.empty()) throw std::invalid_argument("Input image for binarization is empty");
    if (inputImage.channels() != 1) bgr2gray_inplace(inputImage);
    const cv::Mat& in = inputImage;
    long hist[256] = {0};
    for (int y = 0; y < in.rows; ++y) {
        const unsigned char* s = in.ptr(y);
        for (int x = 0; x < in.cols; ++x) hist[s[x]]++;
    }
    const double scale = 1.0 / ((double)in.rows * in.cols);
    double mu = 0;
    for (int i = 0; i < 256; ++i) mu += i * (double)hist[i];
    mu *= scale;
    double mu1 = 0, q1 = 0, best_sigma = 0;
    int best = 0;
    for (int i = 0; i < 256; ++i) {
        const double p_i = hist[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        const double lo = q1 < q2 ? q1 : q2, hi = q1 < q2 ? q2 : q1;
        if (lo < 1.1920928955078125e-07 || hi > 1.0 - 1.1920928955078125e-07) continue;
        mu1 = (mu1 + i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > best_sigma) {
            best_sigma = sigma;
            best = i;
        }
    }
    cv::Mat result(in.rows, in.cols, CV_8UC1);
    for (int y = 0; y < in.rows; ++y) {
        const unsigned char* s = in.ptr(y);
        unsigned char* d = result.ptr(y);
        for (int x = 0; x < in.cols; ++x) d[x] = s[x] > best ? 255 : 0;
    }
    outputImage = result;
}
