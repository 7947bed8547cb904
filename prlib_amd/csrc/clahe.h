// clahe.h — the arithmetic of cv::CLAHE::apply on 8-bit pages, of cv::equalizeHist and of EnhanceLocalContrastByCLAHE
// (src/imageLibCommon.cpp:327-395): the tile geometry with OpenCV's extension quirk, the reflected source index, one tile's table
// from its histogram (clip, redistribution with the stepped residual in closed form, running sum), the per-axis weights and the
// bilinear blend of four tables, the equalization table, and all of them over a page as plain loops - the yardstick of
// tests/cpp/test_clahe.cpp, never the product path.  The kernels of clahe.hip and the host builders (prl_hip_clahe_geometry,
// prl_hip_clahe_tile_lut, prl_hip_equalize_hist_lut) run these functions.  The arithmetic is stated in include/prl_hip.h
// ("contrast") and restated in tests/clahe_ref.py.  Plain C++17: no HIP header, no environment, no I/O.
// Build with -ffp-contract=off: every float32 expression keeps one rounding per written operation.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PRL_CLAHE_FN __host__ __device__ inline
#else
#define PRL_CLAHE_FN inline
#endif

namespace prl_hip {

constexpr int kClaheMaxTiles = 64;       // tiles a side at most (PRL_CLAHE_MAX_TILES)
// the geometry of clahe.hip's kernels (tests/clahe_ref.py names its sizes from the same numbers)
constexpr int kClaheHistBandRows = 64;   // k_clahe_hist: a tile taller than this is split into bands of so many rows, a workgroup each
constexpr int kClaheHistUnitPx = 4096;   // k_clahe_hist: a workgroup takes several tiles (bands) until it has about this many pixels
constexpr int kClaheBlockW = 128;        // k_clahe_interp: pixels of a workgroup's block, across ...
constexpr int kClaheBlockH = 64;         // ... and down
constexpr int kClaheStageTables = 16;    // k_clahe_interp: tile tables per channel a block stages in LDS at most; more: global memory

// cv::borderInterpolate(i, n, BORDER_REFLECT_101) for any i: a side of 1 maps everything to 0, else the index reflects until it
// lies inside (the pad of a CLAHE page can exceed the side)
PRL_CLAHE_FN int clahe_reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

struct ClaheGeom {
    int tiles_x, tiles_y;
    int tile_w, tile_h;   // of the extended page
    int ext_w, ext_h;     // the page the tiles are cut from: the page itself, or grown on the right and at the bottom
    int clip;             // 0: no clipping
    float lut_scale;      // (float)255 / (tile_w * tile_h)
    float inv_tw, inv_th; // 1.0f / tile_w, 1.0f / tile_h
};

// (int)t as x86's cvttsd2si converts: NaN and what lies outside int32 give INT_MIN
PRL_CLAHE_FN int clahe_trunc_x86(double t)
{
    return t >= -2147483648.0 && t < 2147483648.0 ? (int)t : (int)0x80000000;
}

// [upstream] CLAHE_Impl::apply: either both sides divide, or BOTH grow - a side that divides grows by a whole `tiles`
PRL_CLAHE_FN ClaheGeom clahe_geometry(int width, int height, int tiles_x, int tiles_y, double clip_limit)
{
    ClaheGeom g;
    g.tiles_x = tiles_x;
    g.tiles_y = tiles_y;
    if (width % tiles_x == 0 && height % tiles_y == 0) {
        g.ext_w = width;
        g.ext_h = height;
    } else {
        g.ext_w = width + (tiles_x - width % tiles_x);
        g.ext_h = height + (tiles_y - height % tiles_y);
    }
    g.tile_w = g.ext_w / tiles_x;
    g.tile_h = g.ext_h / tiles_y;
    const int area = g.tile_w * g.tile_h;
    g.lut_scale = (float)255 / (float)area;
    g.clip = 0;
    if (clip_limit > 0.0) {
        const int c = clahe_trunc_x86(clip_limit * area / 256);
        g.clip = c > 1 ? c : 1;
    }
    g.inv_tw = 1.0f / (float)g.tile_w;
    g.inv_th = 1.0f / (float)g.tile_h;
    return g;
}

// saturate_cast<uchar>(float): round half to even, then clamp; the values here are finite and far inside int32
PRL_CLAHE_FN uint8_t clahe_sat_u8(float t)
{
    const float r = rintf(t);
    return r < 0.0f ? 0 : (r > 255.0f ? 255 : (uint8_t)r);
}

// ---- one tile's table ----------------------------------------------------------------------------------------------------------

// what the redistribution adds to bin i: clipped / 256 to every bin, and one more where the stepped loop
//     for (i = 0; i < 256 && residual > 0; i += step, --residual) ++h[i]        step = max(256 / residual, 1)
// lands: its k-th trip is at i = k * step, and residual * step <= 256, so all `residual` trips are made
PRL_CLAHE_FN int clahe_redistributed(int i, int clipped)
{
    const int batch = clipped / 256, residual = clipped - 256 * batch;
    if (residual == 0) return batch;
    const int step = 256 / residual > 1 ? 256 / residual : 1;
    return batch + (i % step == 0 && i / step < residual ? 1 : 0);
}

PRL_CLAHE_FN int clahe_excess(int h, int clip) { return h > clip ? h - clip : 0; }

PRL_CLAHE_FN uint8_t clahe_lut_entry(int sum, float lut_scale) { return clahe_sat_u8((float)sum * lut_scale); }

// hist -> lut with the per-bin functions above (what a wavefront of k_clahe_luts does four bins a lane)
inline void clahe_tile_lut(const uint32_t hist[256], int clip, float lut_scale, uint8_t lut[256])
{
    int clipped = 0;
    if (clip > 0)
        for (int i = 0; i < 256; ++i) clipped += clahe_excess((int)hist[i], clip);
    int sum = 0;
    for (int i = 0; i < 256; ++i) {
        int h = (int)hist[i];
        if (clip > 0) h = (h < clip ? h : clip) + clahe_redistributed(i, clipped);
        sum += h;
        lut[i] = clahe_lut_entry(sum, lut_scale);
    }
}

// the same as [upstream] clahe.cpp writes it, loop for loop: the yardstick of the closed form (tests only)
inline void clahe_tile_lut_literal(const uint32_t hist[256], int clip, float lut_scale, uint8_t lut[256])
{
    int h[256];
    for (int i = 0; i < 256; ++i) h[i] = (int)hist[i];
    if (clip > 0) {
        int clipped = 0;
        for (int i = 0; i < 256; ++i)
            if (h[i] > clip) {
                clipped += h[i] - clip;
                h[i] = clip;
            }
        const int batch = clipped / 256;
        int residual = clipped - batch * 256;
        for (int i = 0; i < 256; ++i) h[i] += batch;
        if (residual != 0) {
            const int step = 256 / residual > 1 ? 256 / residual : 1;
            for (int i = 0; i < 256 && residual > 0; i += step, --residual) ++h[i];
        }
    }
    int sum = 0;
    for (int i = 0; i < 256; ++i) {
        sum += h[i];
        lut[i] = clahe_sat_u8((float)sum * lut_scale);
    }
}

// ---- the blend -----------------------------------------------------------------------------------------------------------------

// One axis of [upstream] CLAHE_Interpolation_Body: the two tile indices of coordinate x and their weights
PRL_CLAHE_FN void clahe_axis(int x, float inv_tile, int tiles, int* t1, int* t2, float* a, float* a1)
{
    const float txf = (float)x * inv_tile - 0.5f;
    const int f = (int)floorf(txf);
    *a = txf - (float)f;
    *a1 = 1.0f - *a;
    *t1 = f > 0 ? f : 0;
    *t2 = f + 1 < tiles - 1 ? f + 1 : tiles - 1;
}

// res = (L11 xa1 + L12 xa) ya1 + (L21 xa1 + L22 xa) ya, left to right: seven float32 operations
PRL_CLAHE_FN uint8_t clahe_blend(uint8_t l11, uint8_t l12, uint8_t l21, uint8_t l22, float xa, float xa1, float ya, float ya1)
{
    const float top = (float)l11 * xa1 + (float)l12 * xa;
    const float bottom = (float)l21 * xa1 + (float)l22 * xa;
    return clahe_sat_u8(top * ya1 + bottom * ya);
}

// ---- cv::equalizeHist ------------------------------------------------------------------------------------------------------------

// hist -> lut.  One value on the whole page: the reference fills the page with it, which is the identity table here.
PRL_CLAHE_FN void equalize_lut(const uint32_t* hist, uint8_t* lut)
{
    unsigned total = 0;
    for (int v = 0; v < 256; ++v) total += hist[v];
    int i = 0;
    while (i < 255 && !hist[i]) ++i;
    if (hist[i] == total) {
        for (int v = 0; v < 256; ++v) lut[v] = (uint8_t)v;
        return;
    }
    const float scale = 255.0f / (float)(total - hist[i]);
    int sum = 0;
    for (int v = 0; v < 256; ++v) {
        if (v <= i) {
            lut[v] = 0;
            continue;
        }
        sum += (int)hist[v];
        lut[v] = clahe_sat_u8((float)sum * scale);
    }
}

// ---- a page as plain loops (tests only) --------------------------------------------------------------------------------------------

// the tables of every tile of one channel: luts[tile_y][tile_x][256]
inline void clahe_page_luts(const uint8_t* page, size_t step, int width, int height, int channels, int c, const ClaheGeom& g,
                            uint8_t* luts)
{
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            uint32_t hist[256] = {0};
            for (int y = ty * g.tile_h; y < (ty + 1) * g.tile_h; ++y) {
                const uint8_t* row = page + (size_t)clahe_reflect101(y, height) * step;
                for (int x = tx * g.tile_w; x < (tx + 1) * g.tile_w; ++x) ++hist[row[(size_t)clahe_reflect101(x, width) * channels + c]];
            }
            clahe_tile_lut(hist, g.clip, g.lut_scale, luts + ((size_t)ty * g.tiles_x + tx) * 256);
        }
}

// cv::CLAHE::apply on every channel of one page; dst may be page
inline void clahe_page(const uint8_t* page, size_t step, int width, int height, int channels, int tiles_x, int tiles_y,
                       double clip_limit, uint8_t* dst, size_t dst_step)
{
    const ClaheGeom g = clahe_geometry(width, height, tiles_x, tiles_y, clip_limit);
    std::vector<uint8_t> luts((size_t)channels * tiles_x * tiles_y * 256);
    for (int c = 0; c < channels; ++c) clahe_page_luts(page, step, width, height, channels, c, g, luts.data() + (size_t)c * tiles_x * tiles_y * 256);
    for (int y = 0; y < height; ++y) {
        int ty1, ty2;
        float ya, ya1;
        clahe_axis(y, g.inv_th, tiles_y, &ty1, &ty2, &ya, &ya1);
        for (int x = 0; x < width; ++x) {
            int tx1, tx2;
            float xa, xa1;
            clahe_axis(x, g.inv_tw, tiles_x, &tx1, &tx2, &xa, &xa1);
            for (int c = 0; c < channels; ++c) {
                const uint8_t* L = luts.data() + (size_t)c * tiles_x * tiles_y * 256;
                const int v = page[(size_t)y * step + (size_t)x * channels + c];
                dst[(size_t)y * dst_step + (size_t)x * channels + c] =
                    clahe_blend(L[((size_t)ty1 * tiles_x + tx1) * 256 + v], L[((size_t)ty1 * tiles_x + tx2) * 256 + v],
                                L[((size_t)ty2 * tiles_x + tx1) * 256 + v], L[((size_t)ty2 * tiles_x + tx2) * 256 + v], xa, xa1, ya, ya1);
            }
        }
    }
}

// cv::equalizeHist on every channel of one page; dst may be page
inline void equalize_page(const uint8_t* page, size_t step, int width, int height, int channels, uint8_t* dst, size_t dst_step)
{
    for (int c = 0; c < channels; ++c) {
        uint32_t hist[256] = {0};
        uint8_t lut[256];
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) ++hist[page[(size_t)y * step + (size_t)x * channels + c]];
        equalize_lut(hist, lut);
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) dst[(size_t)y * dst_step + (size_t)x * channels + c] = lut[page[(size_t)y * step + (size_t)x * channels + c]];
    }
}

}  // namespace prl_hip
