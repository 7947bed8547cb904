// bilateral.hip — cv::bilateralFilter on batched 8-bit pages of 1 to 4 interleaved channels, every channel a plane of its own (the
// rules: include/prl_hip.h, "cv::bilateralFilter"; in C++: bilateral.h).
//
//   per pixel, float32, taps (i, j) in row-major order inside the disc, the centre left out:
//       w = space[i, j] * color[|v - c|];  sum += v * w;  wsum += w;        dst = cvRound((sum + c) / (wsum + 1))
//
// One kernel, k_bilateral.  A workgroup of 256 lanes owns a tile of 64 x 16 pixels of one plane: it stages the tile and its halo as
// bytes in LDS (rows kBilLdsStep bytes apart: 48 words, so the two rows a 32-lane half reads lie 16 banks apart) and the 256 colour
// weights beside them, one copy.  A lane owns four adjacent pixels: it reads a tap row's bytes a word at a time and uses each byte
// for up to four pixels, every pixel still meeting its taps in increasing j.  The space weight depends on i * i + j * j alone, so it
// travels as a table over that sum inside the kernel's arguments and is read by uniform index (scalar loads); which taps a row has
// (|j| <= ext[i]) travels the same way.  The result hangs on the order of the taps, on the separate roundings of v * w and of the
// two sums (-ffp-contract=off, and the pragma below), on float32 denormals being kept (the compiler's default for gfx950) and on
// the IEEE division (v_div_scale / v_div_fmas / v_div_fixup in the built object, no reciprocal multiply): DESIGN.md §4.4q.
#include <algorithm>
#include <cmath>

#include "bilateral.h"
#include "prl_internal.h"

namespace prl_hip {

namespace {

constexpr int kBilTileW = 64, kBilTileH = 16;
constexpr int kBilLdsStep = 192;                                   // >= 64 + 2 * 16, and 64 mod 128
constexpr int kBilLdsRows = kBilTileH + 2 * kBilMaxRadius;
constexpr int kBilR2 = kBilMaxRadius * kBilMaxRadius + 1;

struct BilCfg {
    int W, H, C, radius;
    int ext[2 * kBilMaxRadius + 1];   // row i of the disc has the taps |j| <= ext[i + radius]
    float space_r2[kBilR2];           // the space weight of a tap with i * i + j * j = index
    float color[256];
};

__device__ __forceinline__ int bil_dev_reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int period = 2 * len - 2;
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}

// grid = (ceil(W / 64), ceil(H / 16), pages * C)
__global__ __launch_bounds__(256) void k_bilateral(BilCfg c, PageSet src, PageSetOut dst)
{
#pragma clang fp contract(off)
    __shared__ float ct[256];
    __shared__ __attribute__((aligned(16))) uint8_t tile[kBilLdsRows * kBilLdsStep];
    const int t = threadIdx.x;
    const int r = c.radius, r4 = (r + 3) & ~3;   // the halo to the left and right, whole words
    const int plane = blockIdx.z, page = plane / c.C, ch = plane - page * c.C;
    const int x0 = blockIdx.x * kBilTileW, y0 = blockIdx.y * kBilTileH;
    ct[t] = c.color[t];
    {   // the tile with its halo: two rows a pass, a lane per column
        const int sw = kBilTileW + 2 * r4, sh = kBilTileH + 2 * r;
        const int xx = t & 127;
        if (xx < sw) {
            const uint8_t* sp = src.page(page) + (size_t)bil_dev_reflect101(x0 - r4 + xx, c.W) * c.C + ch;
            for (int yy = t >> 7; yy < sh; yy += 2) tile[yy * kBilLdsStep + xx] = sp[(size_t)bil_dev_reflect101(y0 - r + yy, c.H) * src.step];
        }
    }
    __syncthreads();
    const int lx = t & 15, ly = t >> 4;
    const int px = x0 + 4 * lx, py = y0 + ly;
    if (px >= c.W || py >= c.H) return;
    const uint8_t* cp = tile + (ly + r) * kBilLdsStep + r4 + 4 * lx;   // this lane's four pixels: a word
    const unsigned cw = *reinterpret_cast<const unsigned*>(cp);
    int cen[4];
    float sum[4], wsum[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        cen[p] = (int)((cw >> (8 * p)) & 255u);
        sum[p] = 0.f;
        wsum[p] = 0.f;
    }
    for (int i = -r; i <= r; ++i) {
        const int jm = c.ext[i + r], wq1 = (jm + 3) >> 2, ii = i * i;
        const uint8_t* rp = cp + i * kBilLdsStep;
        for (int wq = -wq1; wq <= wq1; ++wq) {
            const unsigned word = *reinterpret_cast<const unsigned*>(rp + 4 * wq);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int v = (int)((word >> (8 * b)) & 255u);
                const float fv = (float)v;
                const int col = 4 * wq + b;   // the byte's column, counted from the lane's first pixel
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int j = col - p;    // uniform: which tap of pixel p this byte is
                    if (j < -jm || j > jm || (ii | j) == 0) continue;
                    const float w = c.space_r2[ii + j * j] * ct[abs(v - cen[p])];
                    const float vw = fv * w;
                    sum[p] = sum[p] + vw;
                    wsum[p] = wsum[p] + w;
                }
            }
        }
    }
    uint8_t* dp = dst.page(page) + (size_t)py * dst.step + (size_t)px * c.C + ch;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (px + p >= c.W) break;
        const float q = (sum[p] + (float)cen[p]) / (wsum[p] + 1.f);
        dp[(size_t)p * c.C] = (uint8_t)min(max((int)rintf(q), 0), 255);
    }
}

int bil_bad_arg(const char* why)
{
    set_error_detail(why);
    return PRL_ERR_BAD_ARG;
}

// The checks of the entries in the documented order (no device is touched); fills the tables.
int bil_checks(const PageArgs& a, int channels, int d, double sigma_color, double sigma_space, bool batch, BilTables* t)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_ARG;
    if (!std::isfinite(sigma_color) || !std::isfinite(sigma_space)) return PRL_ERR_BAD_ARG;
    if (!bil_tables(d, sigma_color, sigma_space, t)) return bil_bad_arg("bilateralFilter: the side 2 * radius + 1 is above 31");
    if ((st = pages_rows_ok(a, channels, channels, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    return pages_overlap_ok(a, channels, channels, false);
}

}  // namespace

// after the checks; n_pages >= 1.  No workspace and no lock: the destination is the only memory written.  Enqueues only.
int bilateral_planes_run(const BilTables& t, const PageArgs& a, int channels, hipStream_t stream)
{
    BilCfg c{};
    c.W = a.width; c.H = a.height; c.C = channels; c.radius = t.radius;
    for (int k = 0; k < t.n_taps; ++k) {
        const int i = t.dy[k], j = t.dx[k];
        c.space_r2[i * i + j * j] = t.space[k];   // (a function of i * i + j * j alone: bilateral.h)
        c.ext[i + t.radius] = std::max(c.ext[i + t.radius], std::abs(j));
    }
    std::copy(t.color, t.color + 256, c.color);
    const int chunk = stage_chunk(a.n_pages, 0, 0, 65535 / channels);
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int cnt = std::min(chunk, a.n_pages - first);
        const dim3 grid((unsigned)((a.width + kBilTileW - 1) / kBilTileW), (unsigned)((a.height + kBilTileH - 1) / kBilTileH),
                        (unsigned)(cnt * channels));
        hipLaunchKernelGGL(k_bilateral, grid, dim3(256), 0, stream, c, src_pages(a, first), dst_pages(a, first));
        PRL_HIP_CHECK(hipGetLastError());
    }
    return PRL_OK;
}

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_bilateral_tables(int d, double sigma_color, double sigma_space, int* radius, int* n_taps, int8_t* dy, int8_t* dx,
                             float* space_weight, float* color_weight)
{
    if (!radius || !n_taps || !std::isfinite(sigma_color) || !std::isfinite(sigma_space)) return PRL_ERR_BAD_ARG;
    BilTables t;
    const bool ok = bil_tables(d, sigma_color, sigma_space, &t);
    *radius = t.radius;
    *n_taps = 0;
    if (!ok) return bil_bad_arg("bilateralFilter: the side 2 * radius + 1 is above 31");
    *n_taps = t.n_taps;
    if (dy) std::copy(t.dy, t.dy + t.n_taps, dy);
    if (dx) std::copy(t.dx, t.dx + t.n_taps, dx);
    if (space_weight) std::copy(t.space, t.space + t.n_taps, space_weight);
    if (color_weight) std::copy(t.color, t.color + 256, color_weight);
    return PRL_OK;
}

int prl_hip_bilateral_filter_batch_device(int n_pages, int channels, int d, double sigma_color, double sigma_space, const uint8_t* d_src,
                                          size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                          size_t dst_page_stride, size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    BilTables t;
    int st = bil_checks(a, channels, d, sigma_color, sigma_space, true, &t);
    if (st != PRL_OK || n_pages == 0) return st;
    int dev;   // the device check alone
    if ((st = current_device(&dev)) != PRL_OK) return st;
    return bilateral_planes_run(t, a, channels, static_cast<hipStream_t>(stream));
}

int prl_hip_bilateral_filter_host(int channels, int d, double sigma_color, double sigma_space, const uint8_t* src, size_t src_step,
                                  int width, int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs h{1, src, 0, src_step, width, height, dst, 0, dst_step};
    BilTables t;
    const int st = bil_checks(h, channels, d, sigma_color, sigma_space, false, &t);
    if (st != PRL_OK) return st;
    return stage_host_pages(h, channels, channels, width, height,
                            [&](const PageArgs& page, hipStream_t s) { return bilateral_planes_run(t, page, channels, s); });
}

}  // extern "C"
