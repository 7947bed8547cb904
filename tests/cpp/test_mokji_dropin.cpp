// test_mokji_dropin.cpp — a caller of prl::binarizeMokji that keeps the reference's #include line and finds it through
// `-I include/prl` alone; built with g++ by tests/test_mokji_cpu.py.
//   test_mokji_dropin cpu
//       the contract without a device: the two std::invalid_argument messages in the reference's order, both before the image is
//       looked at; an empty and a 1-channel input throw as cv::cvtColor(BGR2GRAY) would; the output stays untouched on every
//       error; a valid call fails loudly with GpuApiCallError
//   test_mokji_dropin run <E> <M> <rows> <cols> <cn> <in.raw> <out.raw> [roi]
//       reads rows x cols x cn bytes, runs prl::binarizeMokji(in, out, E, M) on the Mat (or, with `roi`, on the view
//       Rect(3, 2, cols - 7, rows - 5) of it), checks that the input's bytes are unchanged and that the result is a new continuous
//       8UC1 Mat of the input's size, and writes the result's bytes.  E = M = 0 on the command line: the header's defaults.
#include "binarizeMokji.h"

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
    const cv::Mat bgr = page(20, 24, CV_8UC3);
    {
        cv::Mat out = marker;
        CHECK(code_of([&] { prl::binarizeMokji(bgr, out, 0, 20); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "mokjiThreshold: invalid maxEdgeWidth", "maxEdgeWidth < 1");
        CHECK(code_of([&] { prl::binarizeMokji(bgr, out, 3, 0); }, &msg) == 1 && untouched(out, marker) &&
                  msg == "mokjiThreshold: invalid minEdgeMagnitude", "minEdgeMagnitude < 1");
        CHECK(code_of([&] { prl::binarizeMokji(bgr, out, 0, 0); }, &msg) == 1 && msg == "mokjiThreshold: invalid maxEdgeWidth",
              "both invalid: maxEdgeWidth is reported");
        // the arguments are checked before the image is looked at
        const cv::Mat empty, one = page(20, 24, CV_8UC1);
        CHECK(code_of([&] { prl::binarizeMokji(empty, out, 0, 20); }, &msg) == 1 && msg == "mokjiThreshold: invalid maxEdgeWidth",
              "arguments before an empty image");
        CHECK(code_of([&] { prl::binarizeMokji(one, out, 3, 0); }, &msg) == 1 && msg == "mokjiThreshold: invalid minEdgeMagnitude",
              "arguments before a 1-channel image");
        CHECK(code_of([&] { prl::binarizeMokji(empty, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker),
              "empty input: cv::cvtColor throws");
        CHECK(code_of([&] { prl::binarizeMokji(one, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker),
              "1-channel input: cv::cvtColor(BGR2GRAY) throws");
        const cv::Mat two = page(20, 24, CV_8UC2), deep(20, 24, CV_MAKETYPE(2, 3));   // CV_16U
        CHECK(code_of([&] { prl::binarizeMokji(two, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker), "2 channels");
        CHECK(code_of([&] { prl::binarizeMokji(deep, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker), "depth");
    }
    // valid calls without a device fail loudly, the defaults and the extremes of size_t included; the input is not modified
    for (int cn : {3, 4}) {
        cv::Mat out = marker;
        const cv::Mat m = page(20, 24, CV_MAKETYPE(CV_8U, cn));
        const std::vector<unsigned char> keep(m.ptr(0), m.ptr(0) + (size_t)20 * 24 * cn);
        CHECK(code_of([&] { prl::binarizeMokji(m, out); }, &msg) == cv::Error::GpuApiCallError && untouched(out, marker),
              "without a device: GpuApiCallError");
        CHECK(msg.find("binarizeMokji") != std::string::npos, "the message names the function");
        CHECK(code_of([&] { prl::binarizeMokji(m, out, (size_t)-1, (size_t)-1); }) == cv::Error::GpuApiCallError && untouched(out, marker),
              "the largest size_t arguments: no interior, no pair - a valid call");
        CHECK(std::memcmp(m.ptr(0), keep.data(), keep.size()) == 0 && m.channels() == cn, "the input is unmodified");
    }
    {
        cv::Mat out = marker;
        const cv::Mat big = page(300, 300, CV_8UC3);
        CHECK(code_of([&] { prl::binarizeMokji(big, out, 128, 20); }) == cv::Error::StsBadArg && untouched(out, marker),
              "maxEdgeWidth 128 on a page with an interior: StsBadArg");
    }
    if (failures == 0) std::printf("mokji dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 9) return 2;
    const size_t E = (size_t)std::atol(argv[2]), M = (size_t)std::atol(argv[3]);
    const int rows = std::atoi(argv[4]), cols = std::atoi(argv[5]), cn = std::atoi(argv[6]);
    const bool roi = argc > 9 && std::string(argv[9]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[7], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    const cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    cv::Mat out = in;   // the output Mat starts as the input's header: its pixels must still not be written
    if (E == 0 && M == 0) prl::binarizeMokji(in, out);
    else prl::binarizeMokji(in, out, E, M);
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(in.channels() == cn && in.data == (roi ? full.ptr(2) + 3 * cn : full.ptr(0)), "the input's header is unchanged");
    CHECK(out.rows == in.rows && out.cols == in.cols && out.type() == CV_8UC1 && out.isContinuous(), "new continuous 8UC1 Mat of the input's size");
    CHECK(out.data != in.data, "a new buffer");
    FILE* g = std::fopen(argv[8], "wb");
    if (!g) return 4;
    std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols, g);
    std::fclose(g);
    if (failures == 0) std::printf("mokji dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
