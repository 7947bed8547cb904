// bilateral.h — cv::bilateralFilter on 8-bit planes as the host states it: the radius, the taps in their order, the two weight tables
// and the filter as a plain loop (the rules: include/prl_hip.h, "cv::bilateralFilter").  Plain C++17: no HIP header, no
// environment, no I/O - tests/cpp/test_fbcitb.cpp drives it on the CPU under the sanitizers; bilateral.hip takes its tables from
// here and runs the same float32 sequence per pixel.  The loop below is for tests, never the product path.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/prl_hip.h"

namespace prl_hip {

constexpr int kBilMaxSide = PRL_BILATERAL_MAX_SIDE;
constexpr int kBilMaxRadius = kBilMaxSide / 2;
constexpr int kBilMaxTaps = PRL_BILATERAL_MAX_TAPS;   // the lattice points of a disc of radius 15, without its centre

struct BilTables {
    int radius, n_taps;
    int8_t dy[kBilMaxTaps], dx[kBilMaxTaps];   // tap order: rows outer, columns inner
    float space[kBilMaxTaps];
    float color[256];
};

// d <= 0: cvRound(sigma_space * 1.5) (ties to even), else d / 2; at least 1.  A radius beyond the int range comes back as INT32_MAX.
inline int bil_radius(int d, double sigma_space)
{
    if (sigma_space <= 0) sigma_space = 1;
    if (d > 0) return d / 2 > 1 ? d / 2 : 1;
    const double r = std::nearbyint(sigma_space * 1.5);
    if (!(r < 2147483647.0)) return 2147483647;
    return r > 1 ? (int)r : 1;
}

// false: the side 2 radius + 1 is above kBilMaxSide (nothing is written but t->radius)
inline bool bil_tables(int d, double sigma_color, double sigma_space, BilTables* t)
{
    if (sigma_color <= 0) sigma_color = 1;
    if (sigma_space <= 0) sigma_space = 1;
    const double gc = -0.5 / (sigma_color * sigma_color), gs = -0.5 / (sigma_space * sigma_space);
    const int radius = t->radius = bil_radius(d, sigma_space);
    if (radius > kBilMaxRadius) return false;
    for (int i = 0; i < 256; ++i) t->color[i] = (float)std::exp(i * i * gc);
    int n = 0;
    for (int i = -radius; i <= radius; ++i)
        for (int j = -radius; j <= radius; ++j) {
            const double r = std::sqrt((double)i * i + (double)j * j);
            if (r > radius || (i == 0 && j == 0)) continue;
            t->space[n] = (float)std::exp(r * r * gs);
            t->dy[n] = (int8_t)i;
            t->dx[n++] = (int8_t)j;
        }
    t->n_taps = n;
    return true;
}

// cv::borderInterpolate(p, len, BORDER_REFLECT_101) in closed form
inline int bil_reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int period = 2 * len - 2;
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}

// One plane: pixel (x, y) at src[y * src_step + x * src_pix].  Per pixel in float32, every operation rounded on its own, taps in
// table order; then (uchar)cvRound((sum + c) / (wsum + 1)).
inline void bil_filter_plane(const uint8_t* src, size_t src_step, size_t src_pix, int W, int H, const BilTables& t, uint8_t* dst,
                             size_t dst_step, size_t dst_pix)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int c = src[(size_t)y * src_step + (size_t)x * src_pix];
            volatile float sum = 0.f, wsum = 0.f;   // (volatile: no fused multiply-add whatever the flags)
            for (int k = 0; k < t.n_taps; ++k) {
                const int v = src[(size_t)bil_reflect101(y + t.dy[k], H) * src_step + (size_t)bil_reflect101(x + t.dx[k], W) * src_pix];
                const volatile float w = t.space[k] * t.color[v > c ? v - c : c - v];
                const volatile float vw = (float)v * w;
                sum = sum + vw;
                wsum = wsum + w;
            }
            const float q = (sum + (float)c) / (wsum + 1.f);
            const float r = std::nearbyint(q);
            dst[(size_t)y * dst_step + (size_t)x * dst_pix] = (uint8_t)(r < 0.f ? 0 : r > 255.f ? 255 : (int)r);
        }
}

}  // namespace prl_hip
