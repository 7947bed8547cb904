// test_resize_dropin.cpp — a caller of prl::resize that keeps the reference's #include line ("resize.h", src/resize.h) and finds
// it through `-I include/prl` alone; built with g++ by tests/test_edges_cpu.py.
//   test_resize_dropin cpu
//       the contract without a device: the exceptions, the limits, the copy that needs no device, and a loud GpuApiCallError for a
//       valid call where no device exists
//   test_resize_dropin run <rows> <cols> <cn> <in.raw> <out.raw> <scaleX> <scaleY> <maxSize> [roi]
//       reads rows x cols x cn bytes, runs prl::resize on the Mat (or, with `roi`, on the view Rect(3, 2, cols - 7, rows - 5) of
//       it), checks that the input's bytes are unchanged and that the result is a new continuous Mat of the input's type, prints
//       "size W H" and writes the result's bytes
#include "resize.h"

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

// 0: no exception; -1: std::invalid_argument; else cv::Exception's code
template <typename F> static int code_of(F f, std::string* msg = nullptr)
{
    try {
        f();
    } catch (const cv::Exception& e) {
        if (msg) *msg = e.what();
        return e.code;
    } catch (const std::invalid_argument& e) {
        if (msg) *msg = e.what();
        return -1;
    } catch (...) {
        return 1;
    }
    return 0;
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

static int cpu_mode()
{
    cv::Mat in = page(40, 60, CV_8UC3);
    const cv::Mat& cin = in;   // the source is const
    std::string msg;
    {
        cv::Mat out = page(2, 2, CV_8UC1);
        for (int ms : {0, -1, -1000})
            CHECK(code_of([&] { prl::resize(cin, out, 0, 0, ms); }) == cv::Error::StsBadArg, "maxSize < 1 on the pyramid path: StsBadArg");
        CHECK(code_of([&] { prl::resize(cin, out, 3, -1, 0); }) == cv::Error::StsBadArg, "one factor not positive is the pyramid path");
        CHECK(code_of([&] { prl::resize(cin, out, 547, 1, 0); }) == cv::Error::StsBadArg, "60 * 547 > 32768");
        CHECK(code_of([&] { prl::resize(cin, out, 1, 820, 0); }) == cv::Error::StsBadArg, "40 * 820 > 32768");
        cv::Mat empty;
        CHECK(code_of([&] { prl::resize(empty, out, 2, 2, 100); }) == cv::Error::StsAssert, "empty source on the scale path: StsAssert");
        cv::Mat deep(8, 8, CV_MAKETYPE(2, 1));   // CV_16U
        CHECK(code_of([&] { prl::resize(deep, out, 2, 2, 0); }) == cv::Error::StsUnsupportedFormat, "depth != CV_8U");
        cv::Mat five(8, 8, CV_MAKETYPE(CV_8U, 5));
        CHECK(code_of([&] { prl::resize(five, out, 0, 0, 4); }) == cv::Error::StsUnsupportedFormat, "5 channels");
        CHECK(out.rows == 2 && out.cols == 2, "the output stays untouched on an error");
        CHECK(code_of([&] { prl::resize(empty, out, 0, 0, 100); }) == 0 && out.empty(), "the clone of an empty source is empty");
    }
    {   // the long side does not exceed maxSize: dst = src.clone(), no device needed
        cv::Mat out;
        CHECK(code_of([&] { prl::resize(cin, out, 0, 0, 60); }) == 0, "a copy");
        CHECK(out.rows == 40 && out.cols == 60 && out.type() == in.type() && out.data != in.data && out.isContinuous(), "a new Mat of the same size");
        bool same = !out.empty();
        for (int y = 0; same && y < 40; ++y) same = std::memcmp(out.ptr(y), in.ptr(y), 180) == 0;
        CHECK(same, "with the same bytes");
    }
    {   // valid calls without a device fail loudly
        cv::Mat out;
        CHECK(code_of([&] { prl::resize(cin, out, 0, 0, 59); }, &msg) == cv::Error::GpuApiCallError, "pyramid path without a device: GpuApiCallError");
        CHECK(msg.find("resize") != std::string::npos, "the message names the function");
        CHECK(code_of([&] { prl::resize(cin, out, 2, 3, 0); }) == cv::Error::GpuApiCallError, "scale path without a device");
        CHECK(code_of([&] { prl::resize(cin, out, 1, 1, 0); }) == cv::Error::GpuApiCallError, "factors (1, 1) are the scale path too");
        CHECK(out.empty(), "the output stays untouched");
    }
    if (failures == 0) std::printf("resize dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 10) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    const int scaleX = std::atoi(argv[7]), scaleY = std::atoi(argv[8]), maxSize = std::atoi(argv[9]);
    const bool roi = argc > 10 && std::string(argv[10]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    cv::Mat out = in;   // the output Mat starts as the input's header: its pixels must still not be written
    prl::resize(in, out, scaleX, scaleY, maxSize);
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.type() == in.type() && out.isContinuous(), "new continuous Mat of the input's type");
    CHECK(out.data != in.data, "a new buffer");
    std::printf("size %d %d\n", out.cols, out.rows);
    FILE* g = std::fopen(argv[6], "wb");
    if (!g) return 4;
    std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols * out.channels(), g);
    std::fclose(g);
    if (failures == 0) std::printf("resize dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
