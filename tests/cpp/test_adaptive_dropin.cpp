// test_adaptive_dropin.cpp — a caller of prl::binarizeNativeAdaptive, prl::binarizeAT, prl::binarizeAGT and
// prl::binarizePureAdaptiveGaussian that keeps the reference's #include lines and finds them through `-I include/prl` alone;
// built with g++ by tests/test_adaptive_cpu.py.
//   test_adaptive_dropin cpu
//       every exception of the contract, its type, the order of the checks and the state of the input / output Mats
//       afterwards; without a device a valid call ends in a loud GpuApiCallError
//   test_adaptive_dropin run <native|at|agt|pag> <rows> <cols> <cn> <in.raw> <want.raw> <median> <maxValue> <block> <shift> <gaussian>
//       reads rows x cols x cn bytes, runs the function, compares the mask with want.raw (rows x cols bytes) byte by byte and
//       checks the side effects on the input (native: a colour input becomes gray; the others never write it)
#include "binarizeAGT.h"
#include "binarizeAT.h"
#include "binarizeNativeAdaptive.h"
#include "binarizePureAdaptiveGaussian.h"

#include <cmath>
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

enum { kNone = 0, kInvalidArgument = 1, kOther = 2 };   // cv::Exception codes are negative

template <typename F> static int code_of(F f)
{
    try {
        f();
    } catch (const cv::Exception& e) {
        return e.code;
    } catch (const std::invalid_argument&) {
        return kInvalidArgument;
    } catch (...) {
        return kOther;
    }
    return kNone;
}

static cv::Mat page(int rows, int cols, int type)
{
    cv::Mat m(rows, cols, type);
    unsigned s = 12345u;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols * m.channels(); ++x) {
            s = s * 1664525u + 1013904223u;
            m.ptr(y)[x] = (unsigned char)(s >> 24);
        }
    return m;
}

static bool same_bytes(const cv::Mat& a, const cv::Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols || a.type() != b.type()) return false;
    for (int y = 0; y < a.rows; ++y)
        if (std::memcmp(a.ptr(y), b.ptr(y), (size_t)a.cols * a.channels()) != 0) return false;
    return true;
}

// `out` keeps the 2 x 2 marker page it held before the call
static bool untouched(const cv::Mat& out, const cv::Mat& marker) { return out.data == marker.data && out.rows == 2 && out.cols == 2; }

static int cpu_mode()
{
    const cv::Mat marker = page(2, 2, CV_8UC1);
    const double nan = std::nan("");

    // ---- prl::binarizeNativeAdaptive, in the reference's statement order ----
    {
        cv::Mat empty, out = marker;
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(empty, out); }) == kInvalidArgument && untouched(out, marker), "native: empty input");
        // the empty check comes before the max-value check
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(empty, out, false, 5, 7, 150.0, true, 300.0); }) == kInvalidArgument, "native: empty first");
    }
    for (double mv : {-0.5, 255.5, 1e9, nan}) {
        cv::Mat in = page(9, 11, CV_8UC3), keep = in, out = marker;
        // a bad max value throws BEFORE the input becomes gray and before the median's checks (kernel 4 would throw StsAssert)
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, false, 4, 7, 150.0, true, mv); }) == kInvalidArgument, "native: max value outside [0; 255]");
        CHECK(in.channels() == 3 && in.data == keep.data && untouched(out, marker), "native: nothing touched by the max-value throw");
    }
    {   // 2 channels: cv::cvtColor(BGR2GRAY) rejects the type
        cv::Mat in = page(9, 11, CV_MAKETYPE(CV_8U, 2)), out = marker;
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out); }) == cv::Error::StsUnsupportedFormat && in.channels() == 2 && untouched(out, marker),
              "native: 2 channels");
    }
    for (int k : {2, 1, 0, -3}) {   // CV_Assert(medianBlurKernelSize >= 3), AFTER the input became gray
        cv::Mat in = page(9, 11, CV_8UC3), out = marker;
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, false, k); }) == cv::Error::StsAssert, "native: median kernel < 3");
        CHECK(in.channels() == 1 && in.rows == 9 && in.cols == 11 && untouched(out, marker), "native: the input is gray when the median's assert throws");
    }
    {   // cv::medianBlur's own check
        cv::Mat in = page(9, 11, CV_8UC1), out = marker;
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, false, 4); }) == cv::Error::StsAssert && untouched(out, marker), "native: even median kernel");
    }
    {   // the Gaussian-blur variant: the reference's two asserts, then StsNotImplemented
        cv::Mat in = page(9, 11, CV_8UC1), out = marker;
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, true, 5, 2); }) == cv::Error::StsAssert, "native: GaussianBlurKernelSize < 3");
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, true, 5, 7, 0.0); }) == cv::Error::StsAssert, "native: GaussianBlurSigma <= 0");
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, true, 5, 7, nan); }) == cv::Error::StsAssert, "native: GaussianBlurSigma NaN");
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, true, 0); }) == cv::Error::StsNotImplemented && untouched(out, marker),
              "native: Gaussian blur is not provided (the median kernel is not looked at)");
    }
    {   // block sizes: even -> cv::adaptiveThreshold's assert; the automatic size of a 4096 x 4096 page is 24
        cv::Mat in = page(9, 11, CV_8UC1), out = marker;
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, false, 5, 7, 150.0, true, 255.0, 20); }) == cv::Error::StsAssert && untouched(out, marker),
              "native: even block size");
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, false, 5, 7, 150.0, true, 255.0, 257); }) == cv::Error::StsNotImplemented,
              "native: block size above 255");
        cv::Mat big(4096, 4096, CV_8UC1);
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(big, out, false, 5, 7, 150.0, true, 255.0, 0); }) == cv::Error::StsAssert && untouched(out, marker),
              "native: the automatic block size of 4096 x 4096 is 24");
    }
    {   // valid calls reach the device: loud failure without one; a 9 x 11 page's automatic block size is 7 (odd)
        cv::Mat in = page(9, 11, CV_8UC3), out = marker;
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out); }) == cv::Error::GpuApiCallError && in.channels() == 1 && untouched(out, marker),
              "native: no device");
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, false, 5, 7, 150.0, false, 0.0, 0, -3.5); }) == cv::Error::GpuApiCallError, "native: no device (auto block)");
        // the bilateral filter's checks come after the mask: the device failure is first
        CHECK(code_of([&] { prl::binarizeNativeAdaptive(in, out, false, 5, 7, 150.0, true, 255.0, 19, 9.0, 3, -1.0); }) == cv::Error::GpuApiCallError,
              "native: the mask is computed before the bilateral filter's checks");
    }

    // ---- prl::binarizeAT / binarizeAGT / binarizePureAdaptiveGaussian ----
    typedef void (*Fn)(const cv::Mat&, cv::Mat&, int, double, int, int);
    const Fn at = [](const cv::Mat& i, cv::Mat& o, int k, double mv, int bs, int sh) { prl::binarizeAT(i, o, k, mv, bs, sh); };
    const Fn agt = [](const cv::Mat& i, cv::Mat& o, int k, double mv, int bs, int sh) { prl::binarizeAGT(i, o, k, mv, bs, sh); };
    const Fn pag = [](const cv::Mat& i, cv::Mat& o, int, double mv, int bs, int sh) { prl::binarizePureAdaptiveGaussian(i, o, mv, bs, sh); };
    const Fn fns[3] = {at, agt, pag};
    for (int f = 0; f < 3; ++f) {
        const bool med = f < 2;
        cv::Mat empty, out = marker;
        CHECK(code_of([&] { fns[f](empty, out, 4, 255.0, 4, 1); }) == kInvalidArgument && untouched(out, marker), "AT family: empty input first");
        const cv::Mat bgr = page(9, 11, CV_8UC3), gray = page(9, 11, CV_8UC1), two = page(9, 11, CV_MAKETYPE(CV_8U, 2));
        if (med) {
            for (int k : {4, 0, -1, 2})   // the median's check comes before the 1-channel assert and the block size
                CHECK(code_of([&] { fns[f](gray, out, k, 255.0, 4, 1); }) == cv::Error::StsAssert && untouched(out, marker), "AT family: even / non-positive median kernel");
            CHECK(code_of([&] { fns[f](two, out, 7, 255.0, 19, 1); }) == cv::Error::StsAssert, "AT family: 2 channels at k >= 7 (cv::medianBlur)");
        }
        // 1 channel: the reference hands cv::adaptiveThreshold an empty Mat
        CHECK(code_of([&] { fns[f](gray, out, 3, 255.0, 19, 1); }) == cv::Error::StsAssert && untouched(out, marker), "AT family: 1-channel input");
        CHECK(code_of([&] { fns[f](two, out, 3, 255.0, 19, 1); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker), "AT family: 2 channels (cv::cvtColor)");
        for (int bs : {4, 1, 0, -3, 20})
            CHECK(code_of([&] { fns[f](bgr, out, 3, 255.0, bs, 1); }) == cv::Error::StsAssert && untouched(out, marker), "AT family: even or < 3 block size");
        CHECK(code_of([&] { fns[f](bgr, out, 3, 255.0, 257, 1); }) == cv::Error::StsNotImplemented, "AT family: block size above 255");
        const cv::Mat keep = bgr.clone();
        CHECK(code_of([&] { fns[f](bgr, out, 1, -1.0, 19, -2); }) == cv::Error::GpuApiCallError && untouched(out, marker), "AT family: no device");
        CHECK(same_bytes(bgr, keep), "AT family: the input is never written");
    }
    std::printf(failures ? "adaptive dropin cpu: %d FAILED\n" : "adaptive dropin cpu: OK\n", failures);
    return failures ? 1 : 0;
}

static std::vector<unsigned char> read_file(const char* path, size_t n)
{
    std::vector<unsigned char> v(n);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), 1, n, f) != n) {
        std::printf("cannot read %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static int run_mode(char** a)
{
    const std::string fn = a[0];
    const int rows = std::atoi(a[1]), cols = std::atoi(a[2]), cn = std::atoi(a[3]);
    const std::vector<unsigned char> src = read_file(a[4], (size_t)rows * cols * cn), want = read_file(a[5], (size_t)rows * cols);
    const int median = std::atoi(a[6]);
    const double max_value = std::atof(a[7]);
    const int block = std::atoi(a[8]);
    const double shift = std::atof(a[9]);
    const bool gaussian = std::atoi(a[10]) != 0;
    cv::Mat in(rows, cols, CV_MAKETYPE(CV_8U, cn));
    for (int y = 0; y < rows; ++y) std::memcpy(in.ptr(y), src.data() + (size_t)y * cols * cn, (size_t)cols * cn);
    const cv::Mat keep = in.clone();
    cv::Mat out;
    if (fn == "native") {
        prl::binarizeNativeAdaptive(in, out, false, median, 7, 150.0, gaussian, max_value, block, shift);
        CHECK(in.channels() == 1 && in.rows == rows && in.cols == cols, "native: the caller's input is gray afterwards");
    } else {
        if (fn == "at") prl::binarizeAT(in, out, median, max_value, block, (int)shift);
        else if (fn == "agt") prl::binarizeAGT(in, out, median, max_value, block, (int)shift);
        else prl::binarizePureAdaptiveGaussian(in, out, max_value, block, (int)shift);
        CHECK(same_bytes(in, keep), "the input is never written");
    }
    CHECK(out.rows == rows && out.cols == cols && out.type() == CV_8UC1, "the result is a rows x cols 8UC1 Mat");
    size_t bad = 0;
    if (!failures)
        for (int y = 0; y < rows; ++y) bad += std::memcmp(out.ptr(y), want.data() + (size_t)y * cols, (size_t)cols) != 0;
    CHECK(bad == 0, "every byte equals the restatement's");
    if (fn == "native" && !failures) {
        // the bilateral filter (not provided): the reference's two sigma checks, then StsNotImplemented, each with the mask
        // already in outputImage (binarizeNativeAdaptive.cpp:113-133)
        const cv::Mat mask = out.clone();
        const double sig[3][2] = {{0.0, 150.0}, {150.0, -1.0}, {150.0, 150.0}};
        const int expect[3] = {kInvalidArgument, kInvalidArgument, cv::Error::StsNotImplemented};
        for (int i = 0; i < 3; ++i) {
            cv::Mat in2 = keep.clone(), out2;
            const int code = code_of([&] { prl::binarizeNativeAdaptive(in2, out2, false, median, 7, 150.0, gaussian, max_value, block, shift, 3, sig[i][0], sig[i][1]); });
            CHECK(code == expect[i], "native: bilateral filter checks");
            CHECK(same_bytes(out2, mask), "native: outputImage holds the mask when the bilateral step throws");
        }
    }
    std::printf(failures ? "adaptive dropin run: %d FAILED\n" : "adaptive dropin run: OK\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "cpu") return cpu_mode();
    if (argc == 13 && std::string(argv[1]) == "run") return run_mode(argv + 2);
    std::printf("usage: test_adaptive_dropin cpu | run <native|at|agt|pag> <rows> <cols> <cn> <in.raw> <want.raw> <median> <maxValue> <block> <shift> <gaussian>\n");
    return 2;
}
