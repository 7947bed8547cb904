// test_localotsu_dropin.cpp — a caller of prl::binarizeLocalOtsu that keeps the reference's #include line and finds it through
// `-I include/prl` alone; built with g++ by tests/test_localotsu_cpu.py and tests/test_localotsu_gpu.py.
//   test_localotsu_dropin cpu
//       the contract without a device: the reference's signature and defaults; std::invalid_argument with the reference's messages
//       for an empty image, a max value outside [0, 255] and CannyEdgeDetection's argument checks, in the reference's order;
//       StsAssert for an even kernel size; StsUnsupportedFormat for another depth or two channels; a valid call fails loudly with
//       GpuApiCallError and leaves input and output alone
//   test_localotsu_dropin run <rows> <cols> <cn> <in.raw> <out.raw> <how> [maxValue clip size upper lower iters]
//       reads rows x cols x cn bytes and writes the mask's bytes.  how = defaults: prl::binarizeLocalOtsu(in, out); inplace: the same
//       with one Mat as input and output; args: the six arguments that follow; empty: expects the reference's "Contours array is
//       empty" (a page whose edge map has no contour) and writes nothing; edges: CannyEdgeDetection(in, out, size, upper, lower, iters)
//       (imageLibCommon.h, global namespace) with the four arguments that follow, the map's bytes written
#include "binarizeLocalOtsu.h"
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
    void (*fn)(cv::Mat&, cv::Mat&, double, double, int, double, double, int) = &prl::binarizeLocalOtsu;   // the reference's signature
    (void)fn;
    cv::Mat empty, gray = page(40, 48, CV_8UC1), bgr = page(40, 48, CV_8UC3), bgra = page(40, 48, CV_8UC4), out;
    std::string msg;
    CHECK(code_of([&] { prl::binarizeLocalOtsu(empty, out); }, &msg) == 1 && msg == "Input image for binarization is empty", "empty input");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(empty, out, 300.0, 0.0, 2); }, &msg) == 1 && msg == "Input image for binarization is empty",
          "empty comes first");
    for (double mv : {-0.5, 255.5, (double)NAN})
        CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, mv); }, &msg) == 1 && msg == "Max value must be in range [0; 255]", "max value");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 300.0, 0.0, 2); }, &msg) == 1 && msg == "Max value must be in range [0; 255]",
          "the max value before the kernel size");
    cv::Mat two = page(40, 48, CV_8UC2), deep = page(40, 48, CV_MAKETYPE(2, 1));
    CHECK(code_of([&] { prl::binarizeLocalOtsu(two, out, 255.0, 0.0, 2); }) == cv::Error::StsUnsupportedFormat, "two channels: cv::cvtColor, before the kernel size");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(deep, out); }) == cv::Error::StsUnsupportedFormat, "16-bit");
    // CannyEdgeDetection's checks, in its order
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 2, 2.0, 3.0); }, &msg) == 1 && msg == "Gaussian blur kernel size is lesser than 3", "size < 3 first");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 1); }) == 1, "size 1 is below 3, odd or not");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 4, 1.5, 3.0); }, &msg) == 1 && msg == "Canny upper threshold coefficient isn't in range [0;1]",
          "the upper coefficient before the lower one and before the even size");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 4, -0.1, 0.5); }) == 1, "a negative upper coefficient");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 4, 0.5, 1.5); }, &msg) == 1 && msg == "Canny lower threshold coefficient isn't in range [0;1]",
          "the lower coefficient");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 4, 0.2, 0.5); }, &msg) == 1 &&
              msg == "Canny lower threshold coefficient is greater than Canny upper threshold coefficient",
          "lower > upper before the even size");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 4); }) == cv::Error::StsAssert, "an even size: cv::GaussianBlur's assertion");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 18, 0.15, 0.01, 1); }) == cv::Error::StsAssert, "18 too");
    CHECK(code_of([&] { prl::binarizeLocalOtsu(gray, out, 255.0, 0.0, 257); }) == cv::Error::StsBadArg, "a size above 255 (documented deviation)");
    CHECK(out.empty(), "a refused call leaves the output alone");
    for (cv::Mat* m : {&gray, &bgr, &bgra}) {
        const std::vector<unsigned char> keep(m->ptr(0), m->ptr(0) + (size_t)40 * 48 * m->channels());
        CHECK(code_of([&] { prl::binarizeLocalOtsu(*m, out); }, &msg) == cv::Error::GpuApiCallError, "without a device: GpuApiCallError");
        CHECK(code_of([&] { prl::binarizeLocalOtsu(*m, *m, 0.0, 2.0, 3, 1.0, 1.0, -2); }) == cv::Error::GpuApiCallError, "the ends of every range are valid");
        CHECK(std::memcmp(m->ptr(0), keep.data(), keep.size()) == 0, "the input is unmodified");
    }
    CHECK(out.empty(), "a failed call leaves the output alone");
    // CannyEdgeDetection itself: the reference's signature in the global namespace, its own messages in its order
    void (*ced)(cv::Mat&, cv::Mat&, int, double, double, int) = &CannyEdgeDetection;
    (void)ced;
    CHECK(code_of([&] { CannyEdgeDetection(empty, out, 2, 2.0, 3.0, 0); }, &msg) == 1 && msg == "Image for histograms extraction is empty", "CannyEdgeDetection: empty first");
    CHECK(code_of([&] { CannyEdgeDetection(gray, out, 2, 2.0, 3.0, 0); }, &msg) == 1 && msg == "Gaussian blur kernel size is lesser than 3", "CannyEdgeDetection: size < 3");
    CHECK(code_of([&] { CannyEdgeDetection(gray, out, 4, 1.5, 3.0, 0); }, &msg) == 1 && msg == "Canny upper threshold coefficient isn't in range [0;1]", "CannyEdgeDetection: upper");
    CHECK(code_of([&] { CannyEdgeDetection(gray, out, 4, 0.5, -1.0, 0); }, &msg) == 1 && msg == "Canny lower threshold coefficient isn't in range [0;1]", "CannyEdgeDetection: lower");
    CHECK(code_of([&] { CannyEdgeDetection(gray, out, 4, 0.2, 0.5, 0); }) == 1, "CannyEdgeDetection: lower > upper");
    CHECK(code_of([&] { CannyEdgeDetection(gray, out, 4, 0.5, 0.2, 0); }) == cv::Error::StsAssert, "CannyEdgeDetection: an even size");
    CHECK(code_of([&] { CannyEdgeDetection(deep, out, 5, 0.5, 0.2, 0); }) == cv::Error::StsUnsupportedFormat, "CannyEdgeDetection: 16-bit");
    CHECK(code_of([&] { CannyEdgeDetection(gray, out, 257, 0.5, 0.2, 0); }) == cv::Error::StsBadArg, "CannyEdgeDetection: a size above 255");
    CHECK(code_of([&] { CannyEdgeDetection(gray, out, 5, 0.5, 0.2, 256); }) == cv::Error::StsBadArg, "CannyEdgeDetection: more than 255 iterations");
    for (cv::Mat* m : {&gray, &two, &bgr, &bgra})
        CHECK(code_of([&] { CannyEdgeDetection(*m, out, 19, 0.15, 0.01, 1); }) == cv::Error::GpuApiCallError, "CannyEdgeDetection: 1 to 4 channels are valid calls");
    CHECK(out.empty(), "CannyEdgeDetection: a failed call leaves the output alone");
    if (failures == 0) std::printf("localotsu dropin cpu: OK\n");
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
        prl::binarizeLocalOtsu(full, out);
    } else if (how == "inplace") {
        prl::binarizeLocalOtsu(full, full);
        out = full;
    } else if (how == "args" && argc == 14) {
        prl::binarizeLocalOtsu(full, out, std::atof(argv[8]), std::atof(argv[9]), std::atoi(argv[10]), std::atof(argv[11]), std::atof(argv[12]),
                               std::atoi(argv[13]));
    } else if (how == "edges" && argc == 12) {
        CannyEdgeDetection(full, out, std::atoi(argv[8]), std::atof(argv[9]), std::atof(argv[10]), std::atoi(argv[11]));
    } else if (how == "empty") {
        std::string msg;
        CHECK(code_of([&] { prl::binarizeLocalOtsu(full, out); }, &msg) == 1 && msg == "Contours array is empty", "no contour: the reference's exception");
        CHECK(out.empty(), "and the output stays as it was");
        if (failures == 0) std::printf("localotsu dropin run: OK\n");
        return failures ? 1 : 0;
    } else {
        return 2;
    }
    if (how != "inplace") CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.type() == CV_8UC1 && out.rows == rows && out.cols == cols, "the result is a CV_8UC1 mask of the input's size");
    f = std::fopen(argv[6], "wb");
    if (!f) return 4;
    for (int y = 0; y < out.rows; ++y) std::fwrite(out.ptr(y), 1, (size_t)out.cols, f);
    std::fclose(f);
    if (failures == 0) std::printf("localotsu dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
