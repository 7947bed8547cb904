// test_autocrop_dropin.cpp — a caller of prl::autoCrop / prl::documentContour that keeps the reference's #include line
// ("autoCrop.h", src/border_detection/autoCrop.h) and finds it through `-I include/prl` alone; built with g++ by
// tests/test_autocrop_cpu.py.
//   test_autocrop_dropin cpu
//       the contract without a device: the exceptions in the reference's order and with its messages, the scale path, the gray
//       input that becomes BGR in the caller's Mat, and a loud GpuApiCallError for a valid call where no device exists
//   test_autocrop_dropin run <rows> <cols> <cn> <in.raw> <out.raw>
//       reads rows x cols x cn bytes, runs prl::documentContour and prl::autoCrop, prints "found 0|1", "quad x0 y0 ... x3 y3" (the
//       float corners, %.9g) and "size W H", and writes the crop's bytes
#include "autoCrop.h"

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

static int cpu_mode()
{
    std::string msg;
    std::vector<cv::Point2f> contour;
    {
        cv::Mat empty, out(2, 2, CV_8UC1);
        CHECK(code_of([&] { prl::autoCrop(empty, out); }, &msg) == -1 && msg == "autoCrop: Image for cropping is empty", "empty input");
        CHECK(code_of([&] { prl::documentContour(empty, -1, -1, contour); }) == -1, "documentContour: empty input");
        CHECK(out.rows == 2 && out.cols == 2, "the output stays untouched on an error");
    }
    {
        cv::Mat in(40, 60, CV_8UC3), out;
        std::memset(in.ptr(0), 90, (size_t)40 * 60 * 3);
        CHECK(code_of([&] { prl::documentContour(in, 0.5, 0.5, contour); }) == cv::Error::StsNotImplemented, "positive scales: StsNotImplemented");
        cv::Mat deep(8, 8, CV_MAKETYPE(2, 3));   // CV_16U
        CHECK(code_of([&] { prl::documentContour(deep, -1, -1, contour); }) == cv::Error::StsUnsupportedFormat, "depth != CV_8U");
        cv::Mat two(8, 8, CV_MAKETYPE(CV_8U, 2));
        CHECK(code_of([&] { prl::documentContour(two, -1, -1, contour); }) == cv::Error::StsUnsupportedFormat, "2 channels");
        CHECK(code_of([&] { prl::documentContour(in, -1, -1, contour); }) == cv::Error::GpuApiCallError, "valid call without a device");
        CHECK(code_of([&] { prl::autoCrop(in, out); }) == cv::Error::GpuApiCallError && out.empty(), "autoCrop without a device");
    }
    {   // the reference's side effect comes before the search: a gray input is BGR afterwards
        cv::Mat gray(6, 5, CV_8UC1), out;
        for (int i = 0; i < 30; ++i) gray.ptr(0)[i] = (unsigned char)(7 * i);
        (void)code_of([&] { prl::autoCrop(gray, out); });
        CHECK(gray.type() == CV_8UC3 && gray.rows == 6 && gray.cols == 5, "gray input became BGR");
        bool same = gray.type() == CV_8UC3;
        for (int i = 0; same && i < 30; ++i)
            same = gray.ptr(i / 5)[3 * (i % 5)] == 7 * i && gray.ptr(i / 5)[3 * (i % 5) + 1] == 7 * i && gray.ptr(i / 5)[3 * (i % 5) + 2] == 7 * i;
        CHECK(same, "every channel holds the gray value");
    }
    if (failures == 0) std::printf("autocrop dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    cv::Mat in(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(in.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    std::vector<cv::Point2f> contour;
    const bool found = prl::documentContour(in, -1, -1, contour);
    CHECK(contour.size() == (found ? 4u : 0u), "four corners or none");
    std::printf("found %d\n", found ? 1 : 0);
    if (found) {
        std::printf("quad");
        for (const cv::Point2f& p : contour) std::printf(" %.9g %.9g", (double)p.x, (double)p.y);
        std::printf("\n");
    }
    cv::Mat out;
    const bool cropped = prl::autoCrop(in, out);
    CHECK(cropped == found, "autoCrop finds what documentContour finds");
    CHECK(in.channels() == (cn == 1 ? 3 : cn), "a gray input is BGR afterwards");
    if (cropped) {
        CHECK(out.type() == in.type() && out.isContinuous() && out.data != in.data, "a new continuous Mat of the input's type");
        std::printf("size %d %d\n", out.cols, out.rows);
        FILE* g = std::fopen(argv[6], "wb");
        if (!g) return 4;
        std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols * out.channels(), g);
        std::fclose(g);
    } else {
        CHECK(out.empty(), "no quad: the output stays untouched");
    }
    if (failures == 0) std::printf("autocrop dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
