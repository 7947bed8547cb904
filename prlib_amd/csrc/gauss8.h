// gauss8.h — the 8-bit cv::GaussianBlur as the host states it: the 8.8 fixed-point weights of a side (float64 Gaussian, error
// diffusion, the centre taking the rest of 256) and the separable integer filter as plain loops - the yardstick of
// tests/cpp/test_localotsu.cpp, never the product path (blur8.hip runs the same sums).  The rules are stated in include/prl_hip.h
// ("the 8-bit cv::GaussianBlur") and restated in tests/localotsu_ref.py.  Plain C++17: no HIP header, no environment, no I/O.
// Build with -ffp-contract=off: adj = k * 256 + err is a product and a sum, one float64 rounding each.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "gauss.h"

namespace prl_hip {

// The float64 weights of a side of n (odd, positive): the tables for n = 1, 3, 5, 7 when sigma <= 0; else
// s = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8, k_i = exp(-0.5 / s^2 * (i - (n - 1) / 2)^2) / sum (the sum in index order)
inline void gauss8_kernel_f64(int n, double sigma, double* k)
{
    static const double tab1[] = {1.}, tab3[] = {0.25, 0.5, 0.25}, tab5[] = {0.0625, 0.25, 0.375, 0.25, 0.0625},
                        tab7[] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
    if (n <= 7 && !(sigma > 0)) {
        const double* t = n == 1 ? tab1 : n == 3 ? tab3 : n == 5 ? tab5 : tab7;
        for (int i = 0; i < n; ++i) k[i] = t[i];
        return;
    }
    const double s = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2x = -0.5 / (s * s);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) * 0.5;
        k[i] = std::exp(scale2x * x * x);
        sum += k[i];
    }
    for (int i = 0; i < n; ++i) k[i] /= sum;
}

// The n 8.8 weights: the error of each rounding is carried into the next weight, the two halves mirror, the centre is what is
// left of 256.  margin (optional): the smallest distance of an adj from a rounding tie.
inline void gauss8_kernel(int n, double sigma, uint16_t* w, double* margin = nullptr)
{
    std::vector<double> k((size_t)n);
    gauss8_kernel_f64(n, sigma, k.data());
    double err = 0, m = 0.5;
    int others = 0;
    for (int i = 0; i < n / 2; ++i) {
        const double adj = k[(size_t)i] * 256 + err;
        const double v = std::nearbyint(adj);   // cvRound: ties to even
        err = adj - v;
        const double tie = std::fabs(std::fabs(adj - std::floor(adj)) - 0.5);
        if (tie < m) m = tie;
        w[i] = w[n - 1 - i] = (uint16_t)(int)v;
        others += 2 * (int)v;
    }
    w[n / 2] = (uint16_t)(256 - others);
    if (margin) *margin = m;
}

// dst = the separable 8.8 filter of an 8-bit page of C interleaved channels; wx, wy: nx and ny weights in tap order, each side
// summing to at most 256.  dst must not overlap src.
inline void sep_filter_u8_page(const uint8_t* src, size_t step, int W, int H, int C, const uint16_t* wx, int nx, const uint16_t* wy, int ny,
                               uint8_t* dst, size_t dst_step)
{
    const int rx = nx / 2, ry = ny / 2;
    const size_t row = (size_t)W * C;
    std::vector<uint16_t> rows(row * (size_t)H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < C; ++c) {
                uint32_t a = 0;
                for (int i = 0; i < nx; ++i) a += (uint32_t)wx[i] * src[(size_t)y * step + (size_t)gauss_reflect101(x + i - rx, W) * C + c];
                rows[(size_t)y * row + (size_t)x * C + c] = (uint16_t)a;
            }
    for (int y = 0; y < H; ++y)
        for (size_t s = 0; s < row; ++s) {
            uint32_t a = 32768;
            for (int j = 0; j < ny; ++j) a += (uint32_t)wy[j] * rows[(size_t)gauss_reflect101(y + j - ry, H) * row + s];
            dst[(size_t)y * dst_step + s] = (uint8_t)(a >> 16);
        }
}

}  // namespace prl_hip
