// focus.h — the arithmetic of the focus measures LAPM, LAPV, TENG, GLVN (src/detectors/blurDetection.cpp:32-83): the indices of
// the six per-channel sums and of the four measures, the terms one pixel adds to the sums from its 3 x 3 neighbourhood (the code
// k_focus runs on the pixels at a page's left and right edges), the sums of a page as a plain loop - the yardstick of tests/cpp/test_focus.cpp,
// never the product path - and the measures from the sums (prl_hip_focus_from_sums).  The arithmetic is stated in
// include/prl_hip.h ("focus measures") and restated in tests/focus_ref.py.  Plain C++17: no HIP header, no environment, no I/O.
// Build with -ffp-contract=off: the float64 expressions of focus_from_sums keep one rounding per operation.
//
// Bounds on an 8-bit page: |L| <= 1020, |X|, |Y| <= 2040, |Gx|, |Gy| <= 1020, Gx^2 + Gy^2 <= 2 * 1020^2 = 2 080 800.  On a
// 32768 x 32768 page the largest sum is 2^30 * 2 080 800 = 2.3e15 < 2^53: every sum converts to float64 exactly, so the order in
// which OpenCV adds its doubles cannot show.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PRL_FOCUS_FN __host__ __device__ inline
#else
#define PRL_FOCUS_FN inline
#endif

namespace prl_hip {

enum { kFocusSumP = 0, kFocusSumP2 = 1, kFocusSumLap = 2, kFocusSumLap2 = 3, kFocusSumLapm4 = 4, kFocusSumTeng = 5, kFocusSums = 6 };
enum { kFocusLapm = 0, kFocusLapv = 1, kFocusTeng = 2, kFocusGlvn = 3, kFocusMeasures = 4 };

// cv::borderInterpolate(i, n, BORDER_REFLECT_101) for i in [-1, n]: -1 -> 1, n -> n - 2; a side of 1 maps everything to 0
PRL_FOCUS_FN int focus_reflect101(int i, int n)
{
    if (n == 1) return 0;
    return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

PRL_FOCUS_FN bool focus_ksize_ok(int teng_ksize) { return teng_ksize == 1 || teng_ksize == 3; }

// What the pixel at the centre of t[row][column] (one channel, neighbours already reflected) adds to the six sums.
//   L  = cv::Laplacian(CV_64F), ksize 1: 0 1 0 / 1 -4 1 / 0 1 0
//   X  = (-1, 2, -1) along x of the three rows weighted (1, 2, 1); Y the same with the axes exchanged: 4 Lx, 4 Ly of LAPM
//   Gx = cv::Sobel(1, 0, ksize): (-1, 0, 1) along x, (1, 2, 1) across it for ksize 3, alone for ksize 1; Gy with the axes exchanged
PRL_FOCUS_FN void focus_terms(const int t[3][3], int teng_ksize, int out[kFocusSums])
{
    const int p = t[1][1];
    const int L = t[0][1] + t[2][1] + t[1][0] + t[1][2] - 4 * p;
    int X = 0, Y = 0, gx3 = 0, gy3 = 0;
    for (int i = 0; i < 3; ++i) {
        const int w = i == 1 ? 2 : 1;
        X += w * (2 * t[i][1] - t[i][0] - t[i][2]);
        Y += w * (2 * t[1][i] - t[0][i] - t[2][i]);
        gx3 += w * (t[i][2] - t[i][0]);
        gy3 += w * (t[2][i] - t[0][i]);
    }
    const int gx = teng_ksize == 3 ? gx3 : t[1][2] - t[1][0], gy = teng_ksize == 3 ? gy3 : t[2][1] - t[0][1];
    out[kFocusSumP] = p;
    out[kFocusSumP2] = p * p;
    out[kFocusSumLap] = L;
    out[kFocusSumLap2] = L * L;
    out[kFocusSumLapm4] = (X < 0 ? -X : X) + (Y < 0 ? -Y : Y);
    out[kFocusSumTeng] = gx * gx + gy * gy;
}

// the terms of pixel (x, y), channel c, of a page of `channels` interleaved bytes per pixel
PRL_FOCUS_FN void focus_terms_at(const uint8_t* page, size_t step, int width, int height, int channels, int x, int y, int c,
                                 int teng_ksize, int out[kFocusSums])
{
    int t[3][3];
    for (int dy = -1; dy <= 1; ++dy) {
        const uint8_t* row = page + (size_t)focus_reflect101(y + dy, height) * step;
        for (int dx = -1; dx <= 1; ++dx) t[dy + 1][dx + 1] = row[(size_t)focus_reflect101(x + dx, width) * channels + c];
    }
    focus_terms(t, teng_ksize, out);
}

// the six sums of every channel of one page, sums[channel][6]: the definition, pixel by pixel
inline void focus_sums_page(const uint8_t* page, size_t step, int width, int height, int channels, int teng_ksize, int64_t* sums)
{
    for (int i = 0; i < channels * kFocusSums; ++i) sums[i] = 0;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x)
            for (int c = 0; c < channels; ++c) {
                int term[kFocusSums];
                focus_terms_at(page, step, width, height, channels, x, y, c, teng_ksize, term);
                for (int k = 0; k < kFocusSums; ++k) sums[c * kFocusSums + k] += term[k];
            }
}

// The measures of one channel from its sums, in float64 with one rounding per written operation; cv::mean and cv::meanStdDev
// are taken as sum * (1.0 / N) [upstream, generic path].  An all-zero page gives NaN for GLVN (0 / 0), as in the reference.
inline void focus_from_sums(const int64_t sums[kFocusSums], int width, int height, double measures[kFocusMeasures])
{
    const double scale = 1.0 / ((double)width * (double)height);
    measures[kFocusLapm] = ((double)sums[kFocusSumLapm4] / 4.0) * scale;
    const double m = (double)sums[kFocusSumLap] * scale;
    const double var_l = (double)sums[kFocusSumLap2] * scale - m * m;
    const double sd = std::sqrt(var_l > 0.0 ? var_l : 0.0);
    measures[kFocusLapv] = sd * sd;
    measures[kFocusTeng] = (double)sums[kFocusSumTeng] * scale;
    const double mu = (double)sums[kFocusSumP] * scale;
    const double var_p = (double)sums[kFocusSumP2] * scale - mu * mu;
    const double sg = std::sqrt(var_p > 0.0 ? var_p : 0.0);
    measures[kFocusGlvn] = (sg * sg) / mu;
}

}  // namespace prl_hip
