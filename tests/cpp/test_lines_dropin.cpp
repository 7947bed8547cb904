// test_lines_dropin.cpp — a caller of prl::removeLines that keeps the reference's #include line ("removeLines.h") and finds it
// through `-I include/prl` alone; built with g++ by tests/test_lines_cpu.py.
//   test_lines_dropin cpu
//       the exceptions of the contract (empty input, pages below 50 pixels, depth, channels) with the output untouched and,
//       without a device, a loud GpuApiCallError for a valid call
//   test_lines_dropin run <rows> <cols> <cn> <in.raw> <out.raw> [roi]
//       reads rows x cols x cn bytes, runs prl::removeLines on the Mat (or, with `roi`, on the view Rect(3, 2, cols - 7, rows - 5)
//       of it), checks that the input's bytes are unchanged and that the result is a new continuous 8UC1 Mat of the input's
//       size, and writes the result's bytes
#include "removeLines.h"

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
    {
        cv::Mat empty, out = marker;
        CHECK(code_of([&] { prl::removeLines(empty, out); }) == cv::Error::StsAssert && untouched(out, marker), "empty input");
    }
    for (int cn : {1, 3}) {
        cv::Mat out = marker;
        const cv::Mat narrow = page(60, 49, CV_MAKETYPE(CV_8U, cn)), low = page(49, 60, CV_MAKETYPE(CV_8U, cn));
        CHECK(code_of([&] { prl::removeLines(narrow, out); }) == cv::Error::StsAssert && untouched(out, marker), "cols < 50");
        CHECK(code_of([&] { prl::removeLines(low, out); }) == cv::Error::StsAssert && untouched(out, marker), "rows < 50");
    }
    {
        cv::Mat out = marker;
        cv::Mat deep(60, 60, CV_MAKETYPE(2, 1));   // CV_16U
        CHECK(code_of([&] { prl::removeLines(deep, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker), "depth");
        for (int cn : {2, 4}) {
            const cv::Mat m = page(60, 60, CV_MAKETYPE(CV_8U, cn));
            CHECK(code_of([&] { prl::removeLines(m, out); }) == cv::Error::StsUnsupportedFormat && untouched(out, marker),
                  "2 and 4 channels: cv::threshold's Otsu takes 8UC1 only");
        }
    }
    for (int cn : {1, 3}) {   // a valid call without a device fails loudly
        cv::Mat out = marker;
        std::string msg;
        const cv::Mat m = page(50, 64, CV_MAKETYPE(CV_8U, cn));
        const int code = code_of([&] { prl::removeLines(m, out); }, &msg);
        CHECK(code == cv::Error::GpuApiCallError && untouched(out, marker), "valid call without a device: GpuApiCallError");
        CHECK(msg.find("removeLines") != std::string::npos, "the message names the function");
    }
    if (failures == 0) std::printf("lines dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    const bool roi = argc > 7 && std::string(argv[7]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    const cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    cv::Mat out = in;   // the output Mat starts as the input's header: its pixels must still not be written
    prl::removeLines(in, out);
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.rows == in.rows && out.cols == in.cols && out.type() == CV_8UC1 && out.isContinuous(), "new continuous 8UC1 Mat");
    CHECK(out.data != in.data, "a new buffer");
    FILE* g = std::fopen(argv[6], "wb");
    if (!g) return 4;
    std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols, g);
    std::fclose(g);
    if (failures == 0) std::printf("lines dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
