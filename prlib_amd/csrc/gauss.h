// gauss.h — the float32 cv::GaussianBlur of 8-bit pages and prl::basicDeblur on it (src/deblur/basicDeblur.cpp:33-70), as the
// host states them: the kernel-size and sigma rules of cv::GaussianBlur, the weights of cv::getGaussianKernel for a given sigma,
// cv::borderInterpolate(BORDER_REFLECT_101) with its loop, the rounding to a byte, and both functions as plain loops - the
// yardstick of tests/cpp/test_deblur.cpp, never the product path (deblur.hip runs the same order of operations).  The rules are
// stated in include/prl_hip.h ("basicDeblur") and restated in tests/deblur_ref.py.  Plain C++17: no HIP header, no environment,
// no I/O.  Build with -ffp-contract=off: every product and every sum is one float32 rounding.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PRL_GAUSS_FN __host__ __device__ inline
#else
#define PRL_GAUSS_FN inline
#endif

namespace prl_hip {

constexpr int kGaussMaxSide = 255;   // the largest kernel side deblur.hip takes: its half weights travel as kernel arguments

// cv::borderInterpolate(p, len, BORDER_REFLECT_101): ... 2 1 | 0 1 2 ... len-1 | len-2 ...; a page narrower than the radius
// reflects more than once, and len == 1 gives 0
PRL_GAUSS_FN int gauss_reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        p = p < 0 ? -p : 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

// saturate_cast<uchar>(cvRound(t)) of a float: half to even; NaN, +-inf and what lies outside int32 give 0 (tone.hip: sat_u8_host)
PRL_GAUSS_FN uint8_t gauss_sat_u8(float t)
{
    if (!(t >= -2147483648.0f && t < 2147483648.0f)) return 0;
    const float r = rintf(t);
    return r < 0.0f ? (uint8_t)0 : (r > 255.0f ? (uint8_t)255 : (uint8_t)r);
}

// One side of cv::GaussianBlur's kernel (createGaussianKernels, a depth that is not 8-bit): k <= 0 with sigma > 0 gives
// cvRound(sigma * 4 * 2 + 1) | 1; the side must then be positive and odd.  0: no valid side (k <= 0 without a positive sigma -
// a NaN is none -, an even k, a k or a derived side beyond int).
inline int gauss_side(long long k, double sigma)
{
    if (k > 2147483647LL || k < -2147483648LL) return 0;
    if (k <= 0) {
        if (!(sigma > 0)) return 0;
        const double v = sigma * 4 * 2 + 1;
        if (!(v < 2147483647.0)) return 0;
        k = (long long)std::nearbyint(v) | 1;
    }
    return (k & 1) ? (int)k : 0;
}

// What cv::GaussianBlur(Size(kw, kh), sigma_x, sigma_y) filters with: sigma_y <= 0 means sigma_x; the sides by gauss_side; the
// sigmas the weights are made from (negative ones count as 0: the tables, or the sigma derived from the side).
struct GaussPlan {
    int nx, ny;          // 0: no valid side
    double sx, sy;
    bool shared;         // ky is kx: equal sides and |sx - sy| < DBL_EPSILON
};
inline GaussPlan gauss_plan(long long kw, long long kh, double sigma_x, double sigma_y)
{
    GaussPlan p{};
    if (sigma_y <= 0) sigma_y = sigma_x;
    p.nx = gauss_side(kw, sigma_x);
    p.ny = gauss_side(kh, sigma_y);
    p.sx = sigma_x > 0 ? sigma_x : 0.0;   // std::max(sigma, 0.)
    p.sy = sigma_y > 0 ? sigma_y : 0.0;
    p.shared = p.nx == p.ny && std::fabs(p.sx - p.sy) < DBL_EPSILON;
    return p;
}

// cv::getGaussianKernel(n, sigma, CV_32F), n odd and positive: the fixed tables for n = 1, 3, 5, 7 only when sigma <= 0; else
// sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8, float64 terms, the sum in index order, w_i = (float)(t_i * (1 / sum)).
// Symmetric bit for bit (x_i = -x_(n-1-i) exactly).
inline void gauss_kernel(int n, double sigma, float* w)
{
    static const float tab1[] = {1.f}, tab3[] = {0.25f, 0.5f, 0.25f}, tab5[] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                       tab7[] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    if (n <= 7 && !(sigma > 0)) {
        const float* t = n == 1 ? tab1 : n == 3 ? tab3 : n == 5 ? tab5 : tab7;
        for (int i = 0; i < n; ++i) w[i] = t[i];
        return;
    }
    const double s = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2x = -0.5 / (s * s);
    std::vector<double> t((size_t)n);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) * 0.5;
        t[(size_t)i] = std::exp(scale2x * x * x);
        sum += t[(size_t)i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < n; ++i) w[i] = (float)(t[(size_t)i] * sum);
}

// The float32 weights of addWeighted in basicDeblur.cpp:57-61: alpha = 2 w, beta = 2 w - 2, each computed in float64 and rounded once
inline void deblur_weights(double image_weight, float* alpha, float* beta)
{
    *alpha = (float)(2.0 * image_weight);
    *beta = (float)(2.0 * image_weight - 2.0);
}

// ---- the functions as plain loops ---------------------------------------------------------------------------------------------

// g[y][s] (dense, W * C floats a row) = cv::GaussianBlur of every channel of an 8-bit page of C interleaved channels, in float32.
// wx, wy: the nx and ny weights.  Row pass: nx 3 or 5 centre, then pairs; else the taps in ascending order.  Column pass: centre,
// then pairs outward.  A 1 x 1 kernel leaves g = x (the weight is 1.0f: the product is exact).
inline void gauss_blur_page(const uint8_t* src, size_t step, int W, int H, int C, int nx, int ny, const float* wx, const float* wy,
                            float* g)
{
    const int rx = nx / 2, ry = ny / 2;
    const size_t row = (size_t)W * C;
    std::vector<float> rows(row * (size_t)H);
    std::vector<int> xi((size_t)W * nx);   // the reflected pixel of tap k at pixel x
    for (int x = 0; x < W; ++x)
        for (int k = 0; k < nx; ++k) xi[(size_t)x * nx + k] = gauss_reflect101(x - rx + k, W);
    for (int y = 0; y < H; ++y) {
        const uint8_t* p = src + (size_t)y * step;
        for (int x = 0; x < W; ++x) {
            const int* t = &xi[(size_t)x * nx];
            for (int c = 0; c < C; ++c) {
                float a;
                if (nx == 3 || nx == 5) {
                    a = (float)p[(size_t)t[rx] * C + c] * wx[rx];
                    for (int k = 1; k <= rx; ++k) {
                        const float pair = (float)p[(size_t)t[rx + k] * C + c] + (float)p[(size_t)t[rx - k] * C + c];
                        a = a + pair * wx[rx + k];
                    }
                } else {
                    a = wx[0] * (float)p[(size_t)t[0] * C + c];
                    for (int k = 1; k < nx; ++k) {
                        const float prod = wx[k] * (float)p[(size_t)t[k] * C + c];
                        a = a + prod;
                    }
                }
                rows[(size_t)y * row + (size_t)x * C + c] = a;
            }
        }
    }
    for (int y = 0; y < H; ++y)
        for (size_t s = 0; s < row; ++s) {
            float m = wy[ry] * rows[(size_t)y * row + s];
            for (int k = 1; k <= ry; ++k) {
                const float pair = rows[(size_t)gauss_reflect101(y + k, H) * row + s] + rows[(size_t)gauss_reflect101(y - k, H) * row + s];
                const float prod = wy[ry + k] * pair;
                m = m + prod;
            }
            g[(size_t)y * row + s] = m;
        }
}

// out = saturate_u8(cvRound((x * alpha + g * beta) + 0)) per sample: cv::addWeighted on CV_32F, then convertTo(CV_8U)
PRL_GAUSS_FN uint8_t deblur_sample(uint8_t x, float g, float alpha, float beta)
{
    const float xa = (float)x * alpha;
    const float gb = g * beta;
    const float t = xa + gb;
    return gauss_sat_u8(t + 0.0f);
}

// prl::basicDeblur on one page; nx, ny, wx, wy as gauss_plan / gauss_kernel give them.  dst must not overlap src.
inline void deblur_page(const uint8_t* src, size_t step, int W, int H, int C, int nx, int ny, const float* wx, const float* wy,
                        double image_weight, uint8_t* dst, size_t dst_step)
{
    const size_t row = (size_t)W * C;
    std::vector<float> g(row * (size_t)H);
    gauss_blur_page(src, step, W, H, C, nx, ny, wx, wy, g.data());
    float alpha, beta;
    deblur_weights(image_weight, &alpha, &beta);
    for (int y = 0; y < H; ++y)
        for (size_t s = 0; s < row; ++s) dst[(size_t)y * dst_step + s] = deblur_sample(src[(size_t)y * step + s], g[(size_t)y * row + s], alpha, beta);
}

}  // namespace prl_hip
