// test_houghline_dropin.cpp — a caller of prl::findHoughLineContour that keeps the reference's #include line ("houghLine.h",
// src/border_detection/houghLine.h) and finds it through `-I include/prl` alone; built with g++ by tests/test_houghline_cpu.py.
//   test_houghline_dropin cpu
//       the contract without a device: the reference's exception for an empty image, the format checks, the caller's vector and
//       pixels untouched, and a loud GpuApiCallError for a valid call where no device exists
//   test_houghline_dropin run <rows> <cols> <cn> <in.raw>
//       reads rows x cols x cn bytes, runs prl::findHoughLineContour on a vector that already holds one point, prints "found 0|1"
//       and "quad x0 y0 ... x3 y3"
#include "houghLine.h"

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

// the reference's signature, letter for letter
static bool (*const find_contour)(cv::Mat& inputImage, std::vector<cv::Point>& resultContour) = &prl::findHoughLineContour;

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
    std::vector<cv::Point> contour(1, cv::Point(7, 9));
    {
        cv::Mat empty;
        CHECK(code_of([&] { find_contour(empty, contour); }, &msg) == -1 && msg == "Input image is empty", "empty input");
    }
    {
        cv::Mat deep(8, 8, CV_MAKETYPE(2, 3));   // CV_16U
        CHECK(code_of([&] { find_contour(deep, contour); }) == cv::Error::StsUnsupportedFormat, "depth != CV_8U");
        cv::Mat two(8, 8, CV_MAKETYPE(CV_8U, 2));
        CHECK(code_of([&] { find_contour(two, contour); }) == cv::Error::StsUnsupportedFormat, "2 channels");
        cv::Mat in(40, 60, CV_8UC3);
        std::memset(in.ptr(0), 90, (size_t)40 * 60 * 3);
        CHECK(code_of([&] { find_contour(in, contour); }) == cv::Error::GpuApiCallError, "valid call without a device");
        bool same = true;
        for (size_t i = 0; same && i < (size_t)40 * 60 * 3; ++i) same = in.ptr(0)[i] == 90;
        CHECK(same && in.type() == CV_8UC3, "the input is never written");
    }
    CHECK(contour.size() == 1 && contour[0].x == 7 && contour[0].y == 9, "the caller's vector stays as it was on every error");
    if (failures == 0) std::printf("houghline dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    cv::Mat in(rows, cols, CV_MAKETYPE(CV_8U, cn));
    const size_t bytes = (size_t)rows * cols * cn;
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(in.ptr(0), 1, bytes, f) != bytes) return 3;
    std::fclose(f);
    std::vector<unsigned char> before(in.ptr(0), in.ptr(0) + bytes);
    std::vector<cv::Point> contour(1, cv::Point(7, 9));
    const bool found = prl::findHoughLineContour(in, contour);
    CHECK(contour.size() == (found ? 5u : 1u) && contour[0].x == 7 && contour[0].y == 9, "four corners appended, or none");
    CHECK(in.type() == CV_MAKETYPE(CV_8U, cn) && std::memcmp(before.data(), in.ptr(0), bytes) == 0, "the input is never written");
    std::printf("found %d\n", found ? 1 : 0);
    if (found) {
        std::printf("quad");
        for (size_t i = 1; i < contour.size(); ++i) std::printf(" %d %d", contour[i].x, contour[i].y);
        std::printf("\n");
    }
    if (failures == 0) std::printf("houghline dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
