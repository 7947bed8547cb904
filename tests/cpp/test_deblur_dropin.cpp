// test_deblur_dropin.cpp — a caller of prl::basicDeblur that keeps the reference's #include line and finds it through
// `-I include/prl` alone; built with g++ by tests/test_deblur_cpu.py and tests/test_deblur_gpu.py.
//   test_deblur_dropin cpu
//       the contract without a device: the reference's signature and defaults; std::invalid_argument with the reference's message
//       for an empty image, before anything else; StsAssert where cv::GaussianBlur's CV_Assert fails; StsNotImplemented for a
//       depth other than 8-bit; StsBadArg for a side above 255; a valid call fails loudly with GpuApiCallError
//   test_deblur_dropin run <rows> <cols> <cn> <in.raw> <out.raw> [defaults | inplace | view | k sigma_x sigma_y weight]
//       reads rows x cols x cn bytes and writes the result's bytes: `defaults` calls prl::basicDeblur(in, out); `inplace` passes the
//       same Mat as input and output; `view` runs on Rect(3, 2, cols - 7, rows - 5) of the Mat (the result is that size) and
//       checks that the Mat's bytes are unchanged
#include "basicDeblur.h"

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
        for (int x = 0; x < cols * (int)m.elemSize(); ++x) {
            s = s * 1664525u + 1013904223u;
            m.ptr(y)[x] = (unsigned char)(s >> 24);
        }
    return m;
}

static int cpu_mode()
{
    void (*fn)(const cv::Mat&, cv::Mat&, const size_t, const double, const double, const double) = &prl::basicDeblur;   // the reference's signature
    (void)fn;
    const cv::Mat empty, gray = page(20, 24, CV_8UC1), bgr = page(20, 24, CV_8UC3), bgra = page(20, 24, CV_8UC4);
    cv::Mat out;
    std::string msg;
    CHECK(code_of([&] { prl::basicDeblur(empty, out); }, &msg) == 1 && msg == "Input image for deblurring is empty",
          "empty input: the reference's std::invalid_argument");
    CHECK(code_of([&] { prl::basicDeblur(empty, out, 4, -1.0); }) == 1, "empty before the kernel size");
    for (size_t k : {(size_t)2, (size_t)4, (size_t)74})
        CHECK(code_of([&] { prl::basicDeblur(gray, out, k); }) == cv::Error::StsAssert, "an even size: GaussianBlur's assertion");
    CHECK(code_of([&] { prl::basicDeblur(gray, out, 0, 0.0); }) == cv::Error::StsAssert, "no size and no sigma: the assertion");
    CHECK(code_of([&] { prl::basicDeblur(gray, out, 0, -2.0, 3.0); }) == cv::Error::StsAssert, "no size and a negative sigmaX");
    CHECK(code_of([&] { prl::basicDeblur(gray, out, 257); }) == cv::Error::StsBadArg, "a side above 255");
    CHECK(code_of([&] { prl::basicDeblur(gray, out, 0, 40.0); }) == cv::Error::StsBadArg, "a derived side above 255");
    CHECK(code_of([&] { prl::basicDeblur(gray, out, (size_t)1 << 32 | 3); }) == cv::Error::StsBadArg, "a size beyond int");
    const cv::Mat deep = page(20, 24, CV_MAKETYPE(2, 1)), fl = page(20, 24, CV_MAKETYPE(5, 3));   // CV_16U, CV_32FC3
    CHECK(code_of([&] { prl::basicDeblur(deep, out); }) == cv::Error::StsNotImplemented, "16-bit");
    CHECK(code_of([&] { prl::basicDeblur(fl, out); }) == cv::Error::StsNotImplemented, "float");
    CHECK(out.empty(), "a refused call leaves the output alone");
    for (const cv::Mat* m : {&gray, &bgr, &bgra}) {
        const std::vector<unsigned char> keep(m->ptr(0), m->ptr(0) + (size_t)20 * 24 * m->channels());
        CHECK(code_of([&] { prl::basicDeblur(*m, out); }, &msg) == cv::Error::GpuApiCallError, "without a device: GpuApiCallError");
        CHECK(msg.find("basicDeblur") != std::string::npos, "the message names the function");
        CHECK(code_of([&] { prl::basicDeblur(*m, out, 5, 0.0, 0.0, 1.0); }) == cv::Error::GpuApiCallError, "5 x 5 from the table is a valid call");
        CHECK(std::memcmp(m->ptr(0), keep.data(), keep.size()) == 0, "the input is unmodified");
    }
    if (failures == 0) std::printf("deblur dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 8) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    const std::string how = argv[7];
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    const size_t bytes = (size_t)rows * cols * cn;
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(full.ptr(0), 1, bytes, f) != bytes) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + bytes);
    cv::Mat out;
    if (how == "defaults") {
        prl::basicDeblur(full, out);
    } else if (how == "inplace") {
        prl::basicDeblur(full, full);
        out = full;
    } else if (how == "view") {
        const cv::Mat in = full(cv::Rect(3, 2, cols - 7, rows - 5));
        prl::basicDeblur(in, out);
        CHECK(out.rows == rows - 5 && out.cols == cols - 7, "the result has the view's size");
    } else {
        if (argc < 11) return 2;
        prl::basicDeblur(full, out, (size_t)std::atol(argv[7]), std::atof(argv[8]), std::atof(argv[9]), std::atof(argv[10]));
    }
    if (how != "inplace") CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.type() == full.type(), "the result has the input's type");
    f = std::fopen(argv[6], "wb");
    if (!f) return 4;
    for (int y = 0; y < out.rows; ++y) std::fwrite(out.ptr(y), 1, (size_t)out.cols * cn, f);
    std::fclose(f);
    if (failures == 0) std::printf("deblur dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
