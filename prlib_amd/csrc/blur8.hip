// blur8.hip — the 8-bit cv::GaussianBlur on batched pages of 1 to 4 interleaved channels: a separable filter with 8.8 fixed-point
// weights, all integer (the rules: include/prl_hip.h, "the 8-bit cv::GaussianBlur"; in C++: gauss8.h).
//
//   h(x, y) = sum_i wx[i] p(R(x + i - rx, W), y);  dst(x, y) = (sum_j wy[j] h(x, R(y + j - ry, H)) + 32768) >> 16
//
// One kernel, k_blur8<TW>, in the manner of k_deblur (deblur.hip): a row of an interleaved page is a row of W * C samples, the row
// pass a 1-D filter over samples with tap stride C, reflected on the PIXEL index.  A workgroup owns TW samples of a run of rows and
// walks down the page.  Per source row (a reflected row index above and below the page) it stages TW + 2 rx C samples in LDS (two
// buffers: one barrier per row; the bytes of the next row are fetched into registers before the barrier), every lane forms the row
// sum of its sample - at most 255 * 256, 16 bits - and keeps it in its own column of an LDS ring of ny rows (no lane reads another
// lane's ring entries: no second barrier), reads its ny ring entries for the column sum of the row ry rows up, and writes that
// row's byte: the only global write.  The weights travel as kernel arguments in tap order (they need not be symmetric: the
// explicit-weight entry is the kernel's test seam) and are read by uniform index: scalar loads.  The ring (ny x TW halfwords) and
// the row buffers must fit 64 KiB, so TW follows the sides (blur8_tile_width): 256, 128 or 64 samples; 19 x 19 runs at 256.
#include "prl_internal.h"

#include "gauss8.h"

#include <algorithm>
#include <cmath>

namespace prl_hip {

namespace {

constexpr int kB8Chunk = 65535;            // pages per launch (grid.z)
constexpr size_t kB8LdsBytes = 64 << 10;   // dynamic LDS of a workgroup at most

struct B8Cfg {
    int W, H, C;
    int row;           // W * C: samples in a row
    int nx, ny;
    int rows;          // output rows per workgroup
    unsigned wx[kGaussMaxSide];   // tap order; a word each: a scalar load gives the multiplier as it is
    unsigned wy[kGaussMaxSide];
};

// cv::borderInterpolate(p, len, BORDER_REFLECT_101) in closed form (deblur.hip: db_reflect101)
__device__ __forceinline__ int b8_reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int period = 2 * len - 2;
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}

__device__ __forceinline__ int b8_div(int q, int C) { return C == 1 ? q : C == 2 ? q >> 1 : C == 4 ? q >> 2 : q / 3; }

// grid = (ceil(W C / TW), ceil(H / rows), pages); dynamic LDS: (ny * TW + 2 * (TW + 2 rx C)) halfwords
template <int TW>
__global__ __launch_bounds__(TW) void k_blur8(B8Cfg c, PageSet src, PageSetOut dst)
{
    extern __shared__ uint16_t b8_lds[];
    const int C = c.C, nx = c.nx, ny = c.ny, rx = nx >> 1, ry = ny >> 1, SW = TW + 2 * rx * C;
    uint16_t* ring = b8_lds;              // [ny][TW]: source row y0 - ry + i lives in slot i % ny
    uint16_t* srow = b8_lds + ny * TW;    // [2][SW]: sample s0 - rx C + i of the source row
    const int t = threadIdx.x, s0 = blockIdx.x * TW, s = s0 + t;
    const bool active = s < c.row;
    const int page = blockIdx.z;
    const uint8_t* sp = src.page(page);
    uint8_t* dp = dst.page(page);
    const int y0 = blockIdx.y * c.rows, y1 = min(y0 + c.rows, c.H);
    // what this lane stages of every source row: samples i = t + j TW of the row buffer, from the same bytes of each row
    constexpr int NJ = (TW + 2 * (kGaussMaxSide / 2) * 4 + TW - 1) / TW;
    int col[NJ];
    unsigned pre[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = s0 + t + j * TW, px = b8_div(q, C), ch = q - px * C;   // sample q - rx C: pixel px - rx, channel ch
        col[j] = b8_reflect101(px - rx, c.W) * C + ch;
        pre[j] = 0;
    }
    const auto fetch = [&](int yy) {   // the bytes of source row yy into registers: in flight while the row before is filtered
        const uint8_t* prow = sp + (size_t)b8_reflect101(yy, c.H) * src.step;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (t + j * TW < SW) pre[j] = prow[col[j]];
    };
    fetch(y0 - ry);
    int slot = 0;
    for (int it = 0, yy = y0 - ry; yy < y1 + ry; ++yy, ++it) {
        uint16_t* sb = srow + (it & 1) * SW;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (t + j * TW < SW) sb[t + j * TW] = (uint16_t)pre[j];
        if (yy + 1 < y1 + ry) fetch(yy + 1);
        __syncthreads();
        if (active) {
            const uint16_t* sf = sb + t;   // tap k of this lane's sample: sf[k C]
            uint16_t* rf = ring + t;
            unsigned a = 0;
#pragma unroll 8
            for (int k = 0; k < nx; ++k) a += c.wx[k] * sf[k * C];
            rf[slot * TW] = (uint16_t)a;
            if (it >= 2 * ry) {
                // tap 0 is the oldest row of the ring, slot + 1: the slots up to the ring's end, then those from its start
                const int n1 = ny - 1 - slot;
                const uint16_t* r1 = rf + (slot + 1) * TW;
                const unsigned* w2 = c.wy + n1;
                unsigned m = 32768u;
#pragma unroll 8
                for (int k = 0; k < n1; ++k) m += c.wy[k] * r1[k * TW];
#pragma unroll 8
                for (int k = 0; k <= slot; ++k) m += w2[k] * rf[k * TW];
                dp[(size_t)(yy - ry) * dst.step + s] = (uint8_t)(m >> 16);
            }
        }
        slot = slot + 1 == ny ? 0 : slot + 1;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

size_t b8_lds_bytes(int tw, int nx, int ny, int C) { return ((size_t)ny * tw + 2 * ((size_t)tw + 2 * (size_t)(nx / 2) * C)) * 2; }

// the widest tile whose ring and row buffers fit the workgroup's LDS (255 x 255 on four channels fits at 64)
int blur8_tile_width(int nx, int ny, int C)
{
    for (int tw : {256, 128}) if (b8_lds_bytes(tw, nx, ny, C) <= kB8LdsBytes) return tw;
    return 64;
}

struct B8Spec {
    int nx, ny;
    uint16_t wx[kGaussMaxSide], wy[kGaussMaxSide];
};

bool side_ok(int n) { return n > 0 && (n & 1) && n <= kGaussMaxSide; }

// The checks of the entries, in the documented order (no device is touched).  wx / wy: the explicit weights, or null for the
// Gaussian ones of the sigmas.
int blur8_checks(const PageArgs& a, int channels, int nx, int ny, double sigma_x, double sigma_y, const uint16_t* wx, const uint16_t* wy,
                 bool explicit_weights, bool batch, B8Spec* spec)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (!side_ok(nx) || !side_ok(ny)) return PRL_ERR_BAD_WINDOW;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_ARG;
    if (!std::isfinite(sigma_x) || !std::isfinite(sigma_y)) return PRL_ERR_BAD_ARG;
    spec->nx = nx;
    spec->ny = ny;
    if (explicit_weights) {
        if (!wx || !wy) return PRL_ERR_BAD_ARG;
        unsigned sx = 0, sy = 0;
        for (int i = 0; i < nx; ++i) sx += spec->wx[i] = wx[i];
        for (int i = 0; i < ny; ++i) sy += spec->wy[i] = wy[i];
        if (sx > 256 || sy > 256) return PRL_ERR_BAD_ARG;
    } else {
        if (sigma_y <= 0) sigma_y = sigma_x;
        gauss8_kernel(nx, sigma_x, spec->wx);
        gauss8_kernel(ny, sigma_y, spec->wy);
    }
    if ((st = pages_rows_ok(a, channels, channels, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    return pages_overlap_ok(a, channels, channels, false);
}

template <int TW>
void launch_tw(const B8Cfg& c, const PageSet& s, const PageSetOut& d, int n, hipStream_t stream)
{
    const dim3 grid((unsigned)((c.row + TW - 1) / TW), (unsigned)((c.H + c.rows - 1) / c.rows), (unsigned)n);
    hipLaunchKernelGGL((k_blur8<TW>), grid, dim3(TW), b8_lds_bytes(TW, c.nx, c.ny, c.C), stream, c, s, d);
}

}  // namespace

// after the checks; n_pages >= 1.  No workspace and no lock: the destination is the only memory written.
int sep_filter_u8_batch(const uint16_t* wx, int nx, const uint16_t* wy, int ny, const PageArgs& a, int channels, hipStream_t stream)
{
    B8Cfg c{};
    c.W = a.width; c.H = a.height; c.C = channels; c.row = a.width * channels;
    c.nx = nx; c.ny = ny;
    c.rows = std::min(a.height, std::max(96, 6 * ny));
    std::copy(wx, wx + nx, c.wx);
    std::copy(wy, wy + ny, c.wy);
    const int tw = blur8_tile_width(nx, ny, channels);
    const int chunk = stage_chunk(a.n_pages, 0, 0, kB8Chunk);
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int cnt = std::min(chunk, a.n_pages - first);
        const PageSet s = src_pages(a, first);
        const PageSetOut d = dst_pages(a, first);
        switch (tw) {
        case 256: launch_tw<256>(c, s, d, cnt, stream); break;
        case 128: launch_tw<128>(c, s, d, cnt, stream); break;
        default: launch_tw<64>(c, s, d, cnt, stream); break;
        }
        PRL_HIP_CHECK(hipGetLastError());
    }
    return PRL_OK;
}

namespace {

int blur8_device_entry(const PageArgs& a, int channels, int nx, int ny, double sigma_x, double sigma_y, const uint16_t* wx,
                       const uint16_t* wy, bool explicit_weights, void* stream)
{
    B8Spec sp;
    int st = blur8_checks(a, channels, nx, ny, sigma_x, sigma_y, wx, wy, explicit_weights, true, &sp);
    if (st != PRL_OK) return st;
    if (a.n_pages == 0) return PRL_OK;
    int dev;   // the device check alone
    st = current_device(&dev);
    if (st != PRL_OK) return st;
    return sep_filter_u8_batch(sp.wx, sp.nx, sp.wy, sp.ny, a, channels, static_cast<hipStream_t>(stream));
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_gaussian_kernel_u8(int n, double sigma, uint16_t* w)
{
    if (!side_ok(n)) return PRL_ERR_BAD_WINDOW;
    if (!w || !std::isfinite(sigma)) return PRL_ERR_BAD_ARG;
    gauss8_kernel(n, sigma, w);
    return PRL_OK;
}

int prl_hip_sep_filter_u8_batch_device(int n_pages, int channels, const uint16_t* wx, int nx, const uint16_t* wy, int ny,
                                       const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width, int height,
                                       uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return blur8_device_entry(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step},
                              channels, nx, ny, 0.0, 0.0, wx, wy, true, stream);
}

int prl_hip_gaussian_blur_u8_batch_device(int n_pages, int channels, int kernel_w, int kernel_h, double sigma_x, double sigma_y,
                                          const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width, int height,
                                          uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return blur8_device_entry(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step},
                              channels, kernel_w, kernel_h, sigma_x, sigma_y, nullptr, nullptr, false, stream);
}

int prl_hip_gaussian_blur_u8_host(int channels, int kernel_w, int kernel_h, double sigma_x, double sigma_y, const uint8_t* src,
                                  size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs h{1, src, 0, src_step, width, height, dst, 0, dst_step};
    B8Spec sp;
    const int st = blur8_checks(h, channels, kernel_w, kernel_h, sigma_x, sigma_y, nullptr, nullptr, false, false, &sp);
    if (st != PRL_OK) return st;
    return stage_host_pages(h, channels, channels, h.width, h.height, [&](const PageArgs& page, hipStream_t s) {
        return sep_filter_u8_batch(sp.wx, sp.nx, sp.wy, sp.ny, page, channels, s);
    });
}

}  // extern "C"
