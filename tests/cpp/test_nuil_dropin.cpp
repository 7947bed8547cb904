// test_nuil_dropin.cpp — a caller of prl::correctNUIL that keeps the reference's #include line ("correctNUIL.h") and finds it
// through `-I include/prl` alone; built with g++ by tests/test_nuil_cpu.py.
//   test_nuil_dropin cpu
//       the exceptions of the contract (empty input, size < 1, size > 255, depth, channels), the header default and, without a
//       device, a loud GpuApiCallError for a valid call
//   test_nuil_dropin run <size> <rows> <cols> <cn> <in.raw> <out.raw> [roi]
//       reads rows x cols x cn bytes, runs prl::correctNUIL on the Mat (or, with `roi`, on the view Rect(3, 2, cols - 7, rows - 5)
//       of it; size 0 = the header default), checks that the input's bytes are unchanged and that the result is a new
//       continuous Mat of the input's size and type, and writes the result's bytes
#include "correctNUIL.h"

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

// 0: no exception; a cv::Exception's code; 1: std::invalid_argument (its text in *msg); 2: anything else
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
    const cv::Mat in = page(9, 11, CV_8UC3);
    cv::Mat marker = page(2, 2, CV_8UC1);
    {
        cv::Mat empty, out = marker;
        std::string msg;
        CHECK(code_of([&] { prl::correctNUIL(empty, out, 31); }, &msg) == 1 && msg == "Input image for filtration is empty",
              "empty input: std::invalid_argument with the reference's text");
        CHECK(untouched(out, marker), "the output is untouched when the input is empty");
        CHECK(code_of([&] { prl::correctNUIL(empty, out, 0); }) == 1, "the empty check comes before the size");
    }
    for (int size : {0, -1, -31}) {
        cv::Mat out = marker;
        CHECK(code_of([&] { prl::correctNUIL(in, out, size); }) == cv::Error::StsAssert && untouched(out, marker),
              "size < 1: getStructuringElement's assertion");
    }
    {
        cv::Mat out = marker;
        CHECK(code_of([&] { prl::correctNUIL(in, out, 256); }) == cv::Error::StsBadArg && untouched(out, marker), "size above 255");
        cv::Mat deep(4, 4, CV_MAKETYPE(2, 1));   // CV_16U
        CHECK(code_of([&] { prl::correctNUIL(deep, out, 3); }) == cv::Error::StsUnsupportedFormat, "depth != CV_8U");
        cv::Mat five(4, 4, CV_MAKETYPE(CV_8U, 5));
        CHECK(code_of([&] { prl::correctNUIL(five, out, 3); }) == cv::Error::StsAssert, "5 channels (cv::mean)");
        CHECK(code_of([&] { prl::correctNUIL(five, out, 0); }) == cv::Error::StsAssert, "5 channels before the size");
    }
    {   // a valid call without a device fails loudly; the header default needs no third argument
        cv::Mat out = marker;
        std::string msg;
        const int code = code_of([&] { prl::correctNUIL(in, out); }, &msg);
        CHECK(code == cv::Error::GpuApiCallError && untouched(out, marker), "valid call without a device: GpuApiCallError");
        CHECK(msg.find("correctNUIL") != std::string::npos, "the message names the function");
        for (int cn = 1; cn <= 4; ++cn) {
            const cv::Mat m = page(5, 6, CV_MAKETYPE(CV_8U, cn));
            CHECK(code_of([&] { prl::correctNUIL(m, out, 1); }) == cv::Error::GpuApiCallError, "1..4 channels pass the checks");
        }
    }
    if (failures == 0) std::printf("nuil dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 8) return 2;
    const int size = std::atoi(argv[2]);
    const int rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), cn = std::atoi(argv[5]);
    const bool roi = argc > 8 && std::string(argv[8]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[6], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    const cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    cv::Mat out = in;   // the output Mat starts as the input's header: its pixels must still not be written
    if (size == 0) prl::correctNUIL(in, out);
    else prl::correctNUIL(in, out, size);
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.rows == in.rows && out.cols == in.cols && out.type() == in.type() && out.isContinuous(), "new continuous Mat");
    CHECK(out.data != in.data, "a new buffer");
    FILE* g = std::fopen(argv[7], "wb");
    if (!g) return 4;
    std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols * out.channels(), g);
    std::fclose(g);
    if (failures == 0) std::printf("nuil dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
