// test_clahe_dropin.cpp — a caller of EnhanceLocalContrastByCLAHE that keeps the reference's #include line and finds it through
// `-I include/prl` alone; built with g++ by tests/test_clahe_cpu.py and tests/test_clahe_gpu.py.
//   test_clahe_dropin cpu
//       the contract without a device: the reference's signature in the global namespace; std::invalid_argument with the reference's
//       message for an empty image, before anything else; StsUnsupportedFormat for a depth other than 8-bit; StsBadArg for a NaN limit
//       or a grid side outside 1..64; a valid call fails loudly with GpuApiCallError and leaves input and output alone
//   test_clahe_dropin run <rows> <cols> <cn> <in.raw> <out.raw> <how> [clip_limit equalize | clip_limit tiles_x tiles_y]
//       reads rows x cols x cn bytes and writes the result's bytes.  how = enhance: EnhanceLocalContrastByCLAHE(in, out, clip_limit,
//       equalize); inplace: the same with one Mat as input and output, as the reference's callers do; view: on Rect(3, 2, cols - 7,
//       rows - 5) of the Mat (the result is that size; the Mat's bytes stay); clahe: prl::clahe(in, out, clip_limit, tiles_x,
//       tiles_y); equalize: prl::equalizeHist(in, out)
#include "imageLibCommon.h"

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
    void (*fn)(cv::Mat&, cv::Mat&, double, bool) = &EnhanceLocalContrastByCLAHE;   // the reference's signature, global namespace
    (void)fn;
    cv::Mat empty, gray = page(20, 24, CV_8UC1), bgr = page(20, 24, CV_8UC3), bgra = page(20, 24, CV_8UC4);
    cv::Mat out;
    std::string msg;
    CHECK(code_of([&] { EnhanceLocalContrastByCLAHE(empty, out, 2.0, true); }, &msg) == 1 && msg == "Image for histograms enhancing is empty",
          "empty input: the reference's std::invalid_argument");
    CHECK(code_of([&] { EnhanceLocalContrastByCLAHE(empty, out, std::nan(""), false); }) == 1, "empty before the limit");
    CHECK(code_of([&] { prl::clahe(empty, out, 2.0, 0, 99); }) == 1 && code_of([&] { prl::equalizeHist(empty, out); }) == 1, "the extensions too");
    cv::Mat deep = page(20, 24, CV_MAKETYPE(2, 1)), fl = page(20, 24, CV_MAKETYPE(5, 3));   // CV_16U, CV_32FC3
    CHECK(code_of([&] { EnhanceLocalContrastByCLAHE(deep, out, 2.0, false); }) == cv::Error::StsUnsupportedFormat, "16-bit");
    CHECK(code_of([&] { EnhanceLocalContrastByCLAHE(fl, out, 2.0, true); }) == cv::Error::StsUnsupportedFormat, "float");
    CHECK(code_of([&] { prl::equalizeHist(deep, out); }) == cv::Error::StsUnsupportedFormat, "equalizeHist, 16-bit");
    CHECK(code_of([&] { EnhanceLocalContrastByCLAHE(gray, out, std::nan(""), false); }) == cv::Error::StsBadArg, "a NaN limit");
    for (int t : {0, -1, 65})
        CHECK(code_of([&] { prl::clahe(gray, out, 2.0, t, 8); }) == cv::Error::StsBadArg && code_of([&] { prl::clahe(gray, out, 2.0, 8, t); }) == cv::Error::StsBadArg,
              "a grid side outside 1..64");
    CHECK(out.empty(), "a refused call leaves the output alone");
    for (cv::Mat* m : {&gray, &bgr, &bgra}) {
        const std::vector<unsigned char> keep(m->ptr(0), m->ptr(0) + (size_t)20 * 24 * m->channels());
        CHECK(code_of([&] { EnhanceLocalContrastByCLAHE(*m, out, 2.0, true); }, &msg) == cv::Error::GpuApiCallError, "without a device: GpuApiCallError");
        CHECK(msg.find("EnhanceLocalContrastByCLAHE") != std::string::npos, "the message names the function");
        CHECK(code_of([&] { EnhanceLocalContrastByCLAHE(*m, *m, -1.0, false); }) == cv::Error::GpuApiCallError, "in place with a limit below 0 is a valid call");
        CHECK(code_of([&] { prl::clahe(*m, out, 40.0, 64, 1); }) == cv::Error::GpuApiCallError, "a 64 x 1 grid is a valid call");
        CHECK(code_of([&] { prl::equalizeHist(*m, out); }) == cv::Error::GpuApiCallError, "equalizeHist is a valid call");
        CHECK(std::memcmp(m->ptr(0), keep.data(), keep.size()) == 0, "the input is unmodified");
    }
    CHECK(out.empty(), "a failed call leaves the output alone");
    if (failures == 0) std::printf("clahe dropin cpu: OK\n");
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
    const double clip = argc > 8 ? std::atof(argv[8]) : 40.0;
    cv::Mat out;
    if (how == "enhance" && argc == 10) {
        EnhanceLocalContrastByCLAHE(full, out, clip, std::atoi(argv[9]) != 0);
    } else if (how == "inplace" && argc == 10) {
        EnhanceLocalContrastByCLAHE(full, full, clip, std::atoi(argv[9]) != 0);
        out = full;
    } else if (how == "view" && argc == 10) {
        cv::Mat in = full(cv::Rect(3, 2, cols - 7, rows - 5));
        EnhanceLocalContrastByCLAHE(in, out, clip, std::atoi(argv[9]) != 0);
        CHECK(out.rows == rows - 5 && out.cols == cols - 7, "the result has the view's size");
    } else if (how == "clahe" && argc == 11) {
        prl::clahe(full, out, clip, std::atoi(argv[9]), std::atoi(argv[10]));
    } else if (how == "equalize") {
        prl::equalizeHist(full, out);
    } else {
        return 2;
    }
    if (how != "inplace") CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.type() == full.type(), "the result has the input's type");
    f = std::fopen(argv[6], "wb");
    if (!f) return 4;
    for (int y = 0; y < out.rows; ++y) std::fwrite(out.ptr(y), 1, (size_t)out.cols * cn, f);
    std::fclose(f);
    if (failures == 0) std::printf("clahe dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
