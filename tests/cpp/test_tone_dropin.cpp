// test_tone_dropin.cpp — a caller of prl::gammaCorrection, prl::simpleWhiteBalance, prl::grayWorldWhiteBalance and
// prl::cleanBackgroundToWhite that keeps the reference's #include lines and finds them through `-I include/prl` alone; built
// with g++ by tests/test_tone_cpu.py.
//   test_tone_dropin cpu
//       the exceptions of the contract (empty input, channel counts, depth) with the reference's messages and the output
//       untouched; a 4-channel page passes gammaCorrection's checks; without a device, a loud GpuApiCallError for a valid call
//   test_tone_dropin run <gamma|swb|gw|clean> <a> <b> <rows> <cols> <cn> <in.raw> <out.raw> [roi]
//       reads rows x cols x cn bytes, runs the function (gamma: k = a, gamma = b; swb: k = a; gw: pNorm = a, withMax = b != 0) on
//       the Mat (or, with `roi`, on the view Rect(3, 2, cols - 7, rows - 5) of it), checks that the input's bytes are unchanged and
//       that the result is a new continuous 8-bit Mat of the input's size with the channel count of the contract (4 -> 3 for
//       gamma and clean), and writes the result's bytes
#include "gammaCorrection.h"
#include "balanceSimpleWhite.h"
#include "balanceGrayWorldWhite.h"
#include "cleanBackgroundToWhite.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond, what)                                                  \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL: %s (line %d)\n", what, __LINE__);           \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// 0: no exception; a cv::Exception's code; 1: std::invalid_argument; 2: anything else
template <typename F> static int code_of(F f, std::string* msg = nullptr)
{
    try {
        f();
    } catch (const cv::Exception& e) {
        if (msg) *msg = e.what();
        return e.code;
    } catch (const std::invalid_argument& e) {
        if (msg) *msg = e.what();
        return 1;
    } catch (...) {
        return 2;
    }
    return 0;
}

static cv::Mat page(int rows, int cols, int type)
{
    cv::Mat m(rows, cols, type);
    unsigned s = 2463534242u;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols * m.channels(); ++x) {
            s = s * 1664525u + 1013904223u;
            m.ptr(y)[x] = (unsigned char)(s >> 24);
        }
    return m;
}

static bool untouched(const cv::Mat& m, const cv::Mat& marker)
{
    return m.data == marker.data && m.rows == marker.rows && m.cols == marker.cols;
}

static int cpu_mode()
{
    cv::Mat marker = page(2, 2, CV_8UC1);
    std::string msg;
    {
        cv::Mat empty, out = marker;
        CHECK(code_of([&] { prl::gammaCorrection(empty, out, 1.0, 2.2); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "Invalid parameter for GammaCorrectionFilter_OpenCV", "gamma: empty input");
        CHECK(code_of([&] { prl::simpleWhiteBalance(empty, out, 0.01); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "SimpleWhiteBalance: input image is empty.", "simple white balance: empty input");
        CHECK(code_of([&] { prl::grayWorldWhiteBalance(empty, out, 1.0, false); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "GrayWorldWhiteBalance: input image is empty", "gray world: empty input");
        CHECK(code_of([&] { prl::cleanBackgroundToWhite(empty, out); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "Input image for flipping is empty", "clean background: empty input");
    }
    for (int cn : {1, 2, 4}) {
        cv::Mat out = marker;
        const cv::Mat m = page(20, 24, CV_MAKETYPE(CV_8U, cn));
        CHECK(code_of([&] { prl::simpleWhiteBalance(m, out, 0.01); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "SimpleWhiteBalance: input image hasn't 3 channels.", "simple white balance: 3 channels only");
        CHECK(code_of([&] { prl::grayWorldWhiteBalance(m, out, 2.0, true); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "GrayWorldWhiteBalance: input image hasn't 3 channels", "gray world: 3 channels only");
    }
    {
        cv::Mat out = marker;
        const cv::Mat two = page(20, 24, CV_8UC2);
        CHECK(code_of([&] { prl::cleanBackgroundToWhite(two, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker),
              "clean background: 2 channels cannot become a Pix");
        const cv::Mat deep1(20, 24, CV_MAKETYPE(2, 1)), deep3(20, 24, CV_MAKETYPE(2, 3));   // CV_16U
        CHECK(code_of([&] { prl::gammaCorrection(deep1, out, 1.0, 2.2); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker),
              "gamma: depth");
        CHECK(code_of([&] { prl::simpleWhiteBalance(deep3, out, 0.01); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker),
              "simple white balance: depth");
        CHECK(code_of([&] { prl::grayWorldWhiteBalance(deep3, out, 1.0, false); }) == cv::Error::StsUnsupportedFormat &&
                  untouched(out, marker), "gray world: depth");
        CHECK(code_of([&] { prl::cleanBackgroundToWhite(deep1, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker),
              "clean background: depth");
    }
    // valid calls without a device fail loudly; 1 .. 4 channels all pass gammaCorrection's own checks
    for (int cn : {1, 2, 3, 4}) {
        cv::Mat out = marker;
        const cv::Mat m = page(20, 24, CV_MAKETYPE(CV_8U, cn));
        const int code = code_of([&] { prl::gammaCorrection(m, out, 0.5, 2.2); }, &msg);
        CHECK(code == cv::Error::GpuApiCallError && untouched(out, marker), "gamma without a device: GpuApiCallError");
        CHECK(msg.find("gammaCorrection") != std::string::npos, "the message names the function");
    }
    {
        cv::Mat out = marker;
        const cv::Mat m = page(20, 24, CV_8UC3);
        CHECK(code_of([&] { prl::simpleWhiteBalance(m, out, 0.01); }) == cv::Error::GpuApiCallError && untouched(out, marker),
              "simple white balance without a device");
        CHECK(code_of([&] { prl::grayWorldWhiteBalance(m, out, 1.0, false); }) == cv::Error::GpuApiCallError && untouched(out, marker),
              "gray world without a device");
        for (int cn : {1, 3, 4}) {
            const cv::Mat c = page(20, 24, CV_MAKETYPE(CV_8U, cn));
            CHECK(code_of([&] { prl::cleanBackgroundToWhite(c, out); }) == cv::Error::GpuApiCallError && untouched(out, marker),
                  "clean background without a device");
        }
    }
    if (failures == 0) std::printf("tone dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 10) return 2;
    const std::string fn = argv[2];
    const double a = std::atof(argv[3]), b = std::atof(argv[4]);
    const int rows = std::atoi(argv[5]), cols = std::atoi(argv[6]), cn = std::atoi(argv[7]);
    const bool roi = argc > 10 && std::string(argv[10]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[8], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    const cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    cv::Mat out = in;   // the output Mat starts as the input's header: its pixels must still not be written
    int want_cn = cn;
    if (fn == "gamma") {
        prl::gammaCorrection(in, out, a, b);
        want_cn = cn == 4 ? 3 : cn;   // BGRA -> BGR, and no gamma (the reference's switch has no case for 4)
    } else if (fn == "swb") {
        prl::simpleWhiteBalance(in, out, a);
    } else if (fn == "gw") {
        prl::grayWorldWhiteBalance(in, out, a, b != 0.0);
    } else if (fn == "clean") {
        prl::cleanBackgroundToWhite(in, out);
        want_cn = cn == 1 ? 1 : 3;
    } else {
        return 2;
    }
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.rows == in.rows && out.cols == in.cols && out.depth() == CV_8U && out.channels() == want_cn && out.isContinuous(),
          "new continuous 8-bit Mat with the contract's channel count");
    CHECK(out.data != in.data, "a new buffer");
    FILE* g = std::fopen(argv[9], "wb");
    if (!g) return 4;
    std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols * out.channels(), g);
    std::fclose(g);
    if (failures == 0) std::printf("tone dropin run: OK channels=%d\n", out.channels());
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
