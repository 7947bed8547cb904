// test_median_dropin.cpp — a caller of prl::denoiseSaltPepper that keeps the reference sample's #include line
// (samples/denoise/denoiseSaltPepper_sample.cpp) and finds it through `-I include/prl` alone; built with g++ by
// tests/test_median_cpu.py.
//   test_median_dropin cpu
//       the exceptions of the contract (empty input, even / non-positive kernel, depth, channels, 2 channels at k >= 7), the
//       clone for times == 0 and, without a device, a loud GpuApiCallError for a valid call
//   test_median_dropin run <k> <times> <rows> <cols> <cn> <in.raw> <out.raw> [roi]
//       reads rows x cols x cn bytes, runs prl::denoiseSaltPepper on the Mat (or, with `roi`, on the view
//       Rect(3, 2, cols - 7, rows - 5) of it), checks that the input's bytes are unchanged and that the result is a new
//       continuous Mat of the input's size and type, and writes the result's bytes
#include "denoiseSaltPepper.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <typename F> static int code_of(F f, std::string* msg = nullptr)
{
    try {
        f();
    } catch (const cv::Exception& e) {
        if (msg) *msg = e.what();
        return e.code;
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
    // times == 0: out = in.clone() for any Mat, the empty one included (denoiseSaltPepper.cpp:31)
    {
        cv::Mat empty, out = page(2, 2, CV_8UC1);
        CHECK(code_of([&] { prl::denoiseSaltPepper(empty, out, 3, 0); }) == 0 && out.empty(), "times 0 on an empty Mat");
        cv::Mat in = page(5, 7, CV_8UC3), o;
        CHECK(code_of([&] { prl::denoiseSaltPepper(in, o, 4, 0); }) == 0, "times 0 ignores the kernel size");
        CHECK(o.rows == 5 && o.cols == 7 && o.type() == CV_8UC3 && o.data != in.data &&
                  std::memcmp(o.ptr(0), in.ptr(0), (size_t)5 * 7 * 3) == 0,
              "times 0 clones");
    }
    cv::Mat in = page(9, 11, CV_8UC1);
    // [upstream] OpenCV >= 4 asserts !src.empty()
    {
        cv::Mat empty, out = page(2, 2, CV_8UC1);
        CHECK(code_of([&] { prl::denoiseSaltPepper(empty, out, 3, 1); }) == cv::Error::StsAssert && out.empty(),
              "empty input: StsAssert after out = in.clone()");
    }
    for (int k : {4, 0, -1, -3, 2}) {
        cv::Mat out;
        CHECK(code_of([&] { prl::denoiseSaltPepper(in, out, k, 1); }) == cv::Error::StsAssert, "even / non-positive kernel");
        CHECK(out.rows == 9 && out.cols == 11 && out.data != in.data && std::memcmp(out.ptr(0), in.ptr(0), 11) == 0,
              "the clone is assigned before the throw");
    }
    {
        cv::Mat deep(4, 4, CV_MAKETYPE(2, 1)), out;   // CV_16U
        CHECK(code_of([&] { prl::denoiseSaltPepper(deep, out, 3, 1); }) == cv::Error::StsUnsupportedFormat, "depth != CV_8U");
        cv::Mat five(4, 4, CV_MAKETYPE(CV_8U, 5));
        CHECK(code_of([&] { prl::denoiseSaltPepper(five, out, 3, 1); }) == cv::Error::StsUnsupportedFormat, "5 channels");
        cv::Mat two = page(6, 6, CV_8UC2);
        CHECK(code_of([&] { prl::denoiseSaltPepper(two, out, 7, 1); }) == cv::Error::StsAssert, "2 channels at k = 7");
    }
    {   // a valid call without a device fails loudly
        cv::Mat out;
        std::string msg;
        const int code = code_of([&] { prl::denoiseSaltPepper(in, out, 3, 1); }, &msg);
        CHECK(code == cv::Error::GpuApiCallError, "valid call without a device: GpuApiCallError");
        CHECK(msg.find("denoiseSaltPepper") != std::string::npos, "the message names the function");
        const int code1 = code_of([&] { prl::denoiseSaltPepper(in, out, 1, 1); });
        CHECK(code1 == cv::Error::GpuApiCallError, "k = 1 also goes through the device");
    }
    if (failures == 0) std::printf("median dropin cpu: OK\n");
    return failures ? 1 : 0;
}

static int run_mode(int argc, char** argv)
{
    if (argc < 9) return 2;
    const int k = std::atoi(argv[2]);
    const size_t times = (size_t)std::atoll(argv[3]);
    const int rows = std::atoi(argv[4]), cols = std::atoi(argv[5]), cn = std::atoi(argv[6]);
    const bool roi = argc > 9 && std::string(argv[9]) == "roi";
    cv::Mat full(rows, cols, CV_MAKETYPE(CV_8U, cn));
    FILE* f = std::fopen(argv[7], "rb");
    if (!f || std::fread(full.ptr(0), 1, (size_t)rows * cols * cn, f) != (size_t)rows * cols * cn) return 3;
    std::fclose(f);
    const std::vector<unsigned char> keep(full.ptr(0), full.ptr(0) + (size_t)rows * cols * cn);
    cv::Mat in = roi ? full(cv::Rect(3, 2, cols - 7, rows - 5)) : full;
    cv::Mat out = in;   // the output Mat starts as the input's header: its pixels must still not be written
    prl::denoiseSaltPepper(in, out, k, times);
    CHECK(std::memcmp(full.ptr(0), keep.data(), keep.size()) == 0, "the input's bytes are unchanged");
    CHECK(out.rows == in.rows && out.cols == in.cols && out.type() == in.type() && out.isContinuous(), "new continuous Mat");
    CHECK(out.data != full.ptr(0) || out.rows == 0, "a new buffer");
    FILE* g = std::fopen(argv[8], "wb");
    if (!g) return 4;
    std::fwrite(out.ptr(0), 1, (size_t)out.rows * out.cols * out.channels(), g);
    std::fclose(g);
    if (failures == 0) std::printf("median dropin run: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "run") return run_mode(argc, argv);
    return cpu_mode();
}
