// test_focus_dropin.cpp — a caller of prl::isBlurred that keeps the reference's #include line and finds it through
// `-I include/prl` alone, and of the extension prl::focusMeasures; built with g++ by tests/test_focus_cpu.py.
//   test_focus_dropin cpu
//       the contract without a device: prl::isBlurred is false for any Mat, an empty one included, and touches no device;
//       prl::focusMeasures throws std::invalid_argument for an empty image, StsUnsupportedFormat for a depth or a channel count it
//       does not take, StsBadArg for a Sobel size other than 1 and 3; a valid call fails loudly with GpuApiCallError
//   test_focus_dropin run <ksize> <rows> <cols> <cn> <in.raw> [roi]
//       reads rows x cols x cn bytes, runs prl::focusMeasures on the Mat (or, with `roi`, on the view Rect(3, 2, cols - 7, rows - 5)
//       of it; ksize 0: the header's default), checks that the input's bytes are unchanged and prints "lapm lapv teng glvn" as the
//       16 hex digits of their float64 bits
#include "blurDetection.h"

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

static int cpu_mode()
{
    const cv::Mat empty, gray = page(20, 24, CV_8UC1), bgr = page(20, 24, CV_8UC3), bgra = page(20, 24, CV_8UC4);
    bool (*fn)(const cv::Mat&) = &prl::isBlurred;   // the reference's signature
    CHECK(!fn(empty) && !fn(gray) && !fn(bgr) && !fn(bgra), "isBlurred returns false, as the reference does");
    std::string msg;
    CHECK(code_of([&] { prl::focusMeasures(empty); }) == 1, "empty input: std::invalid_argument");
    CHECK(code_of([&] { prl::focusMeasures(empty, 5); }) == 1, "empty before the Sobel size");
    const cv::Mat two = page(20, 24, CV_8UC2), deep(20, 24, CV_MAKETYPE(2, 1));   // CV_16U
    CHECK(code_of([&] { prl::focusMeasures(two); }) == cv::Error::StsUnsupportedFormat, "2 channels");
    CHECK(code_of([&] { prl::focusMeasures(deep); }) == cv::Error::StsUnsupportedFormat, "depth");
    for (int ks : {0, 2, 5, 7, -1})
        CHECK(code_of([&] { prl::focusMeasures(gray, ks); }) == cv::Error::StsBadArg, "a Sobel size other than 1 and 3: StsBadArg");
    for (const cv::Mat* m : {&gray, &bgr, &bgra}) {
        const std::vector<unsigned char> keep(m->ptr(0), m->ptr(0) + (size_t)20 * 24 * m->channels());
        CHECK(code_of([&] { prl::focusMeasures(*m); }, &msg) == cv::Error::GpuApiCallError, "without a device: GpuApiCallError");
        CHECK(msg.find("focusMeasures") != std::string::npos, "the message names the function");
        CHECK(code_of([&] { prl::focusMeasures(*m, 1); }) == cv::Error::GpuApiCallError, "ksize 1 is a valid call");
        CHECK(std::memcmp(m->ptr(0), keep.data(), keep.size()) == 0, "the input is unmodified");
    }
    const prl::FocusMeasures z{1.0, 2.0, 3.0, 4.0};
    CHECK(z.lapm == 1.0 && z.lapv == 2.0 && z.teng == 3.0 && z.glvn == 4.0, "the members in their order");
    if (failures == 0) std::printf("focus dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int ks = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), cn = std::atoi(argv[5]);
    const bool roi = argc > 7 && std::string(argv[7]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[6], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    const cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    const prl::FocusMeasures m = ks == 0 ? prl::focusMeasures(in) : prl::focusMeasures(in, ks);
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(!prl::isBlurred(in), "isBlurred");
    for (double v : {m.lapm, m.lapv, m.teng, m.glvn}) {
        unsigned long long bits;
        std::memcpy(&bits, &v, 8);
        std::printf("%016llx ", bits);
    }
    std::printf("\n");
    if (failures == 0) std::printf("focus dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
