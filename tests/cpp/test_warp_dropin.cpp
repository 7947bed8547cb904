// test_warp_dropin.cpp — a caller of prl::warpCrop that keeps the reference's #include line ("warp.h", src/warp.h) and finds it
// through `-I include/prl` alone; built with g++ by tests/test_warp_cpu.py.
//   test_warp_dropin cpu
//       the contract without a device: the exceptions of both overloads in the reference's order and with its messages
//       (warp.cpp:82-90), the defaults (ratio -1.0, BORDER_CONSTANT, Scalar()), the limits, and a loud GpuApiCallError for a
//       valid call where no device exists
//   test_warp_dropin run <rows> <cols> <cn> <in.raw> <out.raw> <points|coords> <ratio> <border> <v0> <v1> <v2> <v3> <x0> <y0> ... <x3> <y3> [roi]
//       reads rows x cols x cn bytes, runs prl::warpCrop on the Mat (or, with `roi`, on the view Rect(3, 2, cols - 7, rows - 5)
//       of it) through the vector or the coordinate overload, checks that the input's bytes are unchanged and that the result is
//       a new continuous Mat of the input's type, prints "size W H" and writes the result's bytes
#include "warp.h"

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

// 0: no exception; -1: std::invalid_argument (message in *msg); else cv::Exception's code
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
    const std::vector<cv::Point> quad = {cv::Point(5, 4), cv::Point(50, 6), cv::Point(52, 35), cv::Point(3, 33)};
    std::string msg;
    {   // the vector overload: the reference's two checks, in its order, with its messages
        cv::Mat empty, out = page(2, 2, CV_8UC1);
        const std::vector<cv::Point> three(quad.begin(), quad.begin() + 3);
        CHECK(code_of([&] { prl::warpCrop(empty, out, three); }, &msg) == -1 && msg == "Image for warping is empty",
              "empty input comes first: std::invalid_argument");
        CHECK(code_of([&] { prl::warpCrop(in, out, three); }, &msg) == -1 && msg == "Size of array of base points for warping isn't equal 4",
              "three points: std::invalid_argument");
        const std::vector<cv::Point> five(5, cv::Point(1, 1));
        CHECK(code_of([&] { prl::warpCrop(in, out, five); }) == -1, "five points: std::invalid_argument");
        CHECK(out.rows == 2 && out.cols == 2, "the output stays untouched on an error");
    }
    {   // the coordinate overload has no check of its own: cv::warpPerspective asserts
        cv::Mat empty, out;
        CHECK(code_of([&] { prl::warpCrop(empty, out, 0, 0, 9, 0, 9, 9, 0, 9); }) == cv::Error::StsAssert, "empty input: StsAssert");
    }
    {
        cv::Mat out = page(2, 2, CV_8UC1);
        cv::Mat deep(8, 8, CV_MAKETYPE(2, 1));   // CV_16U
        CHECK(code_of([&] { prl::warpCrop(deep, out, quad); }) == cv::Error::StsUnsupportedFormat, "depth != CV_8U");
        cv::Mat five(8, 8, CV_MAKETYPE(CV_8U, 5));
        CHECK(code_of([&] { prl::warpCrop(five, out, quad); }) == cv::Error::StsUnsupportedFormat, "5 channels");
        for (int mode : {2, 3, 4, 5, -1, 16})
            CHECK(code_of([&] { prl::warpCrop(in, out, quad, -1.0, mode); }) == cv::Error::StsNotImplemented, "other border modes: StsNotImplemented");
        CHECK(cv::BORDER_CONSTANT == 0 && cv::BORDER_REPLICATE == 1, "the border modes' values");
        // the limits: a repeated corner and three collinear corners (singular), a degenerate quad (W = 0), a result above 32767
        CHECK(code_of([&] { prl::warpCrop(in, out, 5, 4, 5, 4, 52, 35, 3, 33); }) == cv::Error::StsBadArg, "a repeated corner");
        CHECK(code_of([&] { prl::warpCrop(in, out, 0, 0, 10, 10, 20, 20, 0, 30); }) == cv::Error::StsBadArg, "three collinear corners");
        CHECK(code_of([&] { prl::warpCrop(in, out, 7, 7, 7, 7, 7, 7, 7, 7); }) == cv::Error::StsBadArg, "all corners equal: W = H = 0");
        CHECK(code_of([&] { prl::warpCrop(in, out, 0, 0, 40000, 0, 40000, 10, 0, 10); }) == cv::Error::StsBadArg, "a result side above 32767");
        CHECK(code_of([&] { prl::warpCrop(in, out, 0, 0, 10, 0, 10, 10, 0, 10, 1e-9); }) == cv::Error::StsBadArg, "a ratio that makes W leave the int range");
        CHECK(out.rows == 2 && out.cols == 2, "the output stays untouched on an error");
    }
    {   // valid calls without a device fail loudly; the defaults compile as in the reference (ratio, borderMode, borderValue)
        cv::Mat out;
        const int c1 = code_of([&] { prl::warpCrop(in, out, quad); }, &msg);
        CHECK(c1 == cv::Error::GpuApiCallError, "valid call (vector, defaults) without a device: GpuApiCallError");
        CHECK(msg.find("warpCrop") != std::string::npos, "the message names the function");
        const int c2 = code_of([&] { prl::warpCrop(in, out, 5, 4, 50, 6, 52, 35, 3, 33); });
        CHECK(c2 == cv::Error::GpuApiCallError, "valid call (coordinates, defaults) without a device");
        const int c3 = code_of([&] { prl::warpCrop(in, out, quad, 1.4142, cv::BORDER_REPLICATE, cv::Scalar(1, 2, 3)); });
        CHECK(c3 == cv::Error::GpuApiCallError, "valid call with every argument given");
        const cv::Mat& cin = in;   // the coordinate overload takes a const Mat
        const int c4 = code_of([&] { prl::warpCrop(cin, out, 5, 4, 50, 6, 52, 35, 3, 33, -1.0, cv::BORDER_CONSTANT, cv::Scalar(255)); });
        CHECK(c4 == cv::Error::GpuApiCallError, "const input");
        CHECK(out.empty(), "the output stays untouched");
    }
    if (failures == 0) std::printf("warp dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 22) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    const bool by_points = std::string(argv[7]) == "points";
    const double ratio = std::atof(argv[8]);
    const int border = std::atoi(argv[9]);
    const cv::Scalar value(std::atof(argv[10]), std::atof(argv[11]), std::atof(argv[12]), std::atof(argv[13]));
    int q[8];
    for (int i = 0; i < 8; ++i) q[i] = std::atoi(argv[14 + i]);
    const bool roi = argc > 22 && std::string(argv[22]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    cv::Mat out = in;   // the output Mat starts as the input's header: its pixels must still not be written
    if (by_points) {
        const std::vector<cv::Point> pts = {cv::Point(q[0], q[1]), cv::Point(q[2], q[3]), cv::Point(q[4], q[5]), cv::Point(q[6], q[7])};
        prl::warpCrop(in, out, pts, ratio, border, value);
    } else {
        prl::warpCrop(in, out, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], ratio, border, value);
    }
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.type() == in.type() && out.isContinuous(), "new continuous Mat of the input's type");
    CHECK(out.data != in.data, "a new buffer");
    std::printf("size %d %d\n", out.cols, out.rows);
    FILE* g = std::fopen(argv[6], "wb");
    if (!g) return 4;
    std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols * out.channels(), g);
    std::fclose(g);
    if (failures == 0) std::printf("warp dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
