// test_fbcitb_dropin.cpp — a caller of prl::binarizeFBCITB and prl::bilateralFilter that keeps the reference's #include line and finds
// it through `-I include/prl` alone; built with g++ by tests/test_fbcitb_cpu.py and tests/test_fbcitb_gpu.py.
//   test_fbcitb_dropin cpu
//       the contract without a device: std::invalid_argument with the reference's messages for an empty image and for a type that
//       is neither 8UC3 nor one 8-bit channel; a gray image becomes 8UC3 BEFORE anything else can fail (the reference's side
//       effect), then CannyEdgeDetection's checks where that stage runs
//   test_fbcitb_dropin run <rows> <cols> <cn> <in.raw> <out.raw> <useCanny> <useVariancesMap>
//       reads rows x cols x cn bytes, calls prl::binarizeFBCITB(in, out, useCanny, useVariancesMap), writes the mask's bytes and
//       checks what became of the caller's Mat: a gray one is now its GRAY2BGR conversion, a colour one is untouched
//   test_fbcitb_dropin filter <rows> <cols> <cn> <in.raw> <out.raw> <d> <sigmaColor> <sigmaSpace>
#include "binarizeFBCITB.h"
#include "imageLibCommon.h"

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

static bool read_mat(const char* path, cv::Mat& m)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    bool ok = true;
    for (int y = 0; y < m.rows && ok; ++y) ok = std::fread(m.ptr(y), 1, (size_t)m.cols * m.channels(), f) == (size_t)m.cols * m.channels();
    std::fclose(f);
    return ok;
}

static bool write_mat(const char* path, const cv::Mat& m)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    bool ok = true;
    for (int y = 0; y < m.rows && ok; ++y) ok = std::fwrite(m.ptr(y), 1, (size_t)m.cols * m.channels(), f) == (size_t)m.cols * m.channels();
    std::fclose(f);
    return ok;
}

static int cpu_mode()
{
    std::string msg;
    cv::Mat empty, out;
    CHECK(code_of([&] { prl::binarizeFBCITB(empty, out); }, &msg) == 1 && msg == "Input image for binarization is empty", "empty image");
    cv::Mat two(8, 8, CV_8UC2), four(8, 8, CV_8UC4);
    CHECK(code_of([&] { prl::binarizeFBCITB(two, out); }, &msg) == 1 && msg.find("required 24 bits per pixel") != std::string::npos, "two channels");
    CHECK(code_of([&] { prl::binarizeFBCITB(four, out); }, &msg) == 1 && msg.find("required 24 bits per pixel") != std::string::npos, "four channels");
    cv::Mat gray(8, 9, CV_8UC1);
    for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 9; ++x) gray.ptr(y)[x] = (unsigned char)(y * 9 + x);
    // the blur size 2 fails CannyEdgeDetection's first check - after the gray image was converted
    CHECK(code_of([&] { prl::binarizeFBCITB(gray, out, true, true, true, true, false, true, true, 200.0, 2.0, 2.0); }, &msg) == 1 &&
              msg == "Gaussian blur kernel size is lesser than 3", "blur size 2");
    CHECK(gray.type() == CV_8UC3 && gray.rows == 8 && gray.cols == 9, "the gray image became 8UC3");
    bool same = gray.type() == CV_8UC3;
    for (int y = 0; same && y < 8; ++y)
        for (int x = 0; x < 9; ++x) same = same && gray.ptr(y)[3 * x] == y * 9 + x && gray.ptr(y)[3 * x + 1] == y * 9 + x && gray.ptr(y)[3 * x + 2] == y * 9 + x;
    CHECK(same, "its channels are the gray bytes");
    cv::Mat bgr(8, 8, CV_8UC3);
    CHECK(code_of([&] { prl::binarizeFBCITB(bgr, out, true, false, true, true, false, true, true, 200.0, 2.0, 9.0, 0.4, 0.6); }, &msg) == 1 &&
              msg.find("lower threshold coefficient is greater") != std::string::npos, "lower above upper");
    CHECK(code_of([&] { prl::binarizeFBCITB(bgr, out, true, true, true, true, false, true, true, 200.0, 2.0, 8.0); }) == cv::Error::StsAssert, "an even blur size");
    CHECK(code_of([&] { prl::bilateralFilter(empty, out, 5, 1.0, 1.0); }) == 1, "bilateral: empty image");
    CHECK(code_of([&] { prl::bilateralFilter(bgr, bgr, 5, 1.0, 1.0); }) == cv::Error::StsAssert, "bilateral: in place");
    if (failures) return 1;
    std::printf("fbcitb dropin cpu: OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "cpu") == 0) return cpu_mode();
    if (argc < 7) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    cv::Mat in(rows, cols, CV_MAKETYPE(CV_8U, cn)), out;
    if (!read_mat(argv[5], in)) return 2;
    const cv::Mat before = in.clone();
    if (std::strcmp(argv[1], "filter") == 0 && argc == 10) {
        prl::bilateralFilter(in, out, std::atoi(argv[7]), std::atof(argv[8]), std::atof(argv[9]));
        CHECK(out.type() == in.type() && out.rows == rows && out.cols == cols, "the result has the input's type");
    } else if (std::strcmp(argv[1], "run") == 0 && argc == 9) {
        prl::binarizeFBCITB(in, out, std::atoi(argv[7]) != 0, std::atoi(argv[8]) != 0);
        CHECK(out.type() == CV_8UC1 && out.rows == rows && out.cols == cols, "the mask is 8UC1");
        CHECK(in.type() == CV_8UC3 && in.rows == rows && in.cols == cols, "the caller's image is 8UC3 after the call");
        bool same = in.type() == CV_8UC3;
        for (int y = 0; same && y < rows; ++y)
            for (int x = 0; x < cols; ++x)
                for (int c = 0; c < 3; ++c) same = same && in.ptr(y)[3 * x + c] == (cn == 1 ? before.ptr(y)[x] : before.ptr(y)[3 * x + c]);
        CHECK(same, cn == 1 ? "a gray input became its GRAY2BGR conversion" : "a colour input is untouched");
    } else {
        return 2;
    }
    if (!write_mat(argv[6], out)) return 2;
    if (failures) return 1;
    std::printf("fbcitb dropin run: OK\n");
    return 0;
}
