// deblur.hip — prl::basicDeblur (src/deblur/basicDeblur.cpp:33-70) on batched 8-bit pages of 1 to 4 interleaved channels, and the
// float32 cv::GaussianBlur of such pages it is built on (the rules: include/prl_hip.h, "basicDeblur"; in C++: gauss.h).
//
//   x = (float)p;  g = GaussianBlur(x), float32, BORDER_REFLECT_101;  t = (x * alpha + g * beta) + 0;  out = saturate_u8(cvRound(t))
//
// One kernel, k_deblur<TW, F32>, for every channel count and every pair of kernel sides.  A row of an interleaved page is a row of
// W * C samples; the row pass is a 1-D filter over samples with tap stride C, reflected on the PIXEL index, and the column pass
// does not see channels.  A workgroup owns TW samples of a run of rows and walks down the page.  Per source row (a reflected row
// index above and below the page) it stages TW + 2 rx C samples as floats in LDS (two buffers: one barrier per row; the bytes of
// the next row are fetched into registers before the barrier and are in flight while this row is filtered), every lane
// computes the row pass of its sample and keeps it in its own column of an LDS ring of ny rows (no lane reads another lane's
// ring entries: no second barrier), reads its ny ring entries for the column pass of the row ry rows up, and writes that row's
// byte (F32: g itself, the second entry).  The centre sample of step 3 is read again from the page (a byte the workgroup staged
// ry rows earlier): the destination byte is the only global write, and no float plane goes to memory.  The weights travel as
// kernel arguments (kx whole, in tap order; ky by halves: it is symmetric bit for bit) and are read by uniform index: scalar loads.
// The ring (ny x TW words) and the row buffers must fit 64 KiB, so TW follows the sides (deblur_tile_width): 256, 128, 64 or 32
// samples (at 32 half a wavefront idles); 73 x 73, the header default, runs at 128.  Operation order: §4.4c's, __fmul_rn /
// __fadd_rn, never contracted.  Sides up to kGaussMaxSide = 255.
#include "prl_internal.h"

#include "gauss.h"

#include <algorithm>
#include <cmath>

namespace prl_hip {

namespace {

constexpr int kDbHalf = (kGaussMaxSide + 1) / 2;
constexpr int kDbChunk = 65535;            // pages per launch (grid.z)
constexpr size_t kDbLdsBytes = 64 << 10;   // dynamic LDS of a workgroup at most

struct DbCfg {
    int W, H, C;
    int row;           // W * C: samples in a row
    int nx, ny;
    int rows;          // output rows per workgroup
    float alpha, beta;
    float wx[kGaussMaxSide];   // kx in tap order: the row pass walks it upwards, eight scalars a load
    float wy[kDbHalf];         // wy[j] = ky[ry + j] = ky[ry - j]
};

// cv::borderInterpolate(p, len, BORDER_REFLECT_101) in closed form: the loop's reflections about 0 and len - 1 keep p's class
// under p -> -p, p -> p + 2 (len - 1), and [0, len) holds one member of each class
__device__ __forceinline__ int db_reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int period = 2 * len - 2;
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}

__device__ __forceinline__ int db_div(int q, int C) { return C == 1 ? q : C == 2 ? q >> 1 : C == 4 ? q >> 2 : q / 3; }

// grid = (ceil(W C / TW), ceil(H / rows), pages); dynamic LDS: (ny * TW + 2 * (TW + 2 rx C)) words
template <int TW, bool F32>
__global__ __launch_bounds__(TW < 64 ? 64 : TW) void k_deblur(DbCfg c, PageSet src, PageSetOut dst)
{
    constexpr int NT = TW < 64 ? 64 : TW;
    extern __shared__ float db_lds[];
    const int C = c.C, nx = c.nx, ny = c.ny, rx = nx >> 1, ry = ny >> 1, SW = TW + 2 * rx * C;
    float* ring = db_lds;              // [ny][TW]: source row y0 - ry + i lives in slot i % ny
    float* srow = db_lds + ny * TW;    // [2][SW]: sample s0 - rx C + i of the source row
    const int t = threadIdx.x, s0 = blockIdx.x * TW, s = s0 + t;
    const bool active = t < TW && s < c.row;
    const int page = blockIdx.z;
    const uint8_t* sp = src.page(page);
    const int y0 = blockIdx.y * c.rows, y1 = min(y0 + c.rows, c.H);
    const bool pairs = nx == 3 || nx == 5;
    // what this lane stages of every source row: samples i = t + j NT of the row buffer, from the same bytes of each row
    constexpr int NJ = (TW + 2 * (kGaussMaxSide / 2) * 4 + NT - 1) / NT;
    int col[NJ];
    unsigned pre[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = s0 + t + j * NT, px = db_div(q, C), ch = q - px * C;   // sample q - rx C: pixel px - rx, channel ch
        col[j] = db_reflect101(px - rx, c.W) * C + ch;
        pre[j] = 0;
    }
    const auto fetch = [&](int yy) {   // the bytes of source row yy into registers: in flight while the row before is filtered
        const uint8_t* prow = sp + (size_t)db_reflect101(yy, c.H) * src.step;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (t + j * NT < SW) pre[j] = prow[col[j]];
    };
    fetch(y0 - ry);
    int slot = 0;
    for (int it = 0, yy = y0 - ry; yy < y1 + ry; ++yy, ++it) {
        float* sb = srow + (it & 1) * SW;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (t + j * NT < SW) sb[t + j * NT] = (float)pre[j];
        unsigned xb = 0;   // the centre sample of the row this iteration finishes
        if (!F32 && active && it >= 2 * ry) xb = sp[(size_t)(yy - ry) * src.step + s];
        if (yy + 1 < y1 + ry) fetch(yy + 1);
        __syncthreads();
        if (active) {
            const float* sf = sb + t;   // tap k of this lane's sample: sf[k C]
            float* rf = ring + t;
            float a;
            if (pairs) {
                a = __fmul_rn(sf[rx * C], c.wx[rx]);
                for (int k = 1; k <= rx; ++k) a = __fadd_rn(a, __fmul_rn(__fadd_rn(sf[(rx + k) * C], sf[(rx - k) * C]), c.wx[rx + k]));
            } else {
                a = __fmul_rn(c.wx[0], sf[0]);
#pragma unroll 16
                for (int k = 1; k < nx; ++k) a = __fadd_rn(a, __fmul_rn(c.wx[k], sf[k * C]));
            }
            rf[slot * TW] = a;
            if (it >= 2 * ry) {
                int sc = slot - ry;   // the centre row's slot
                if (sc < 0) sc += ny;
                float m = __fmul_rn(c.wy[0], rf[sc * TW]);
                int su = sc, sd = sc;
                for (int k = 1; k <= ry; ++k) {
                    su = su + 1 == ny ? 0 : su + 1;
                    sd = sd == 0 ? ny - 1 : sd - 1;
                    m = __fadd_rn(m, __fmul_rn(c.wy[k], __fadd_rn(rf[su * TW], rf[sd * TW])));
                }
                const int y = yy - ry;
                if (F32) {
                    *reinterpret_cast<float*>(dst.page(page) + (size_t)y * dst.step + (size_t)s * 4) = m;
                } else {
                    const float x = (float)xb;
                    const float tt = __fadd_rn(__fadd_rn(__fmul_rn(x, c.alpha), __fmul_rn(m, c.beta)), 0.0f);
                    dst.page(page)[(size_t)y * dst.step + s] = gauss_sat_u8(tt);
                }
            }
        }
        slot = slot + 1 == ny ? 0 : slot + 1;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

size_t db_lds_bytes(int tw, int nx, int ny, int C) { return ((size_t)ny * tw + 2 * ((size_t)tw + 2 * (size_t)(nx / 2) * C)) * 4; }

// the widest tile whose ring and row buffers fit the workgroup's LDS
int deblur_tile_width(int nx, int ny, int C)
{
    for (int tw : {256, 128, 64}) if (db_lds_bytes(tw, nx, ny, C) <= kDbLdsBytes) return tw;
    return 32;
}

struct DbSpec {
    GaussPlan plan;
    double weight;   // basicDeblur's imageWeight (unused by the blur alone)
};

// The checks of the four entries, in the documented order (no device is touched).  out_bytes: bytes per destination sample.
int deblur_checks(const PageArgs& a, int channels, int out_bytes, long long kw, long long kh, double sigma_x, double sigma_y,
                  double weight, bool batch, DbSpec* spec)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    const GaussPlan p = gauss_plan(kw, kh, sigma_x, sigma_y);
    if (p.nx == 0 || p.ny == 0 || p.nx > kGaussMaxSide || p.ny > kGaussMaxSide) return PRL_ERR_BAD_WINDOW;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_ARG;
    if (!std::isfinite(sigma_x) || !std::isfinite(sigma_y) || !std::isfinite(weight)) return PRL_ERR_BAD_ARG;
    if ((st = pages_rows_ok(a, channels, channels * out_bytes, batch)) != PRL_OK) return st;
    if (out_bytes == 4 && (((size_t)a.dst | a.dst_step | a.dst_page_stride) & 3)) return PRL_ERR_BAD_ARG;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    if ((st = pages_overlap_ok(a, channels, channels * out_bytes, false)) != PRL_OK) return st;
    spec->plan = p;
    spec->weight = weight;
    return PRL_OK;
}

DbCfg make_cfg(const DbSpec& sp, int W, int H, int C)
{
    DbCfg c{};
    c.W = W; c.H = H; c.C = C; c.row = W * C;
    c.nx = sp.plan.nx; c.ny = sp.plan.ny;
    c.rows = std::min(H, std::max(96, 6 * c.ny));
    deblur_weights(sp.weight, &c.alpha, &c.beta);
    float w[kGaussMaxSide];
    gauss_kernel(c.nx, sp.plan.sx, w);
    std::copy(w, w + c.nx, c.wx);
    if (!sp.plan.shared) gauss_kernel(c.ny, sp.plan.sy, w);
    for (int j = 0; j <= c.ny / 2; ++j) c.wy[j] = w[c.ny / 2 + j];
    return c;
}

template <int TW>
void launch_tw(const DbCfg& c, bool f32, const PageSet& s, const PageSetOut& d, int n, hipStream_t stream)
{
    constexpr int NT = TW < 64 ? 64 : TW;
    const dim3 grid((unsigned)((c.row + TW - 1) / TW), (unsigned)((c.H + c.rows - 1) / c.rows), (unsigned)n);
    const size_t lds = db_lds_bytes(TW, c.nx, c.ny, c.C);
    if (f32) hipLaunchKernelGGL((k_deblur<TW, true>), grid, dim3(NT), lds, stream, c, s, d);
    else hipLaunchKernelGGL((k_deblur<TW, false>), grid, dim3(NT), lds, stream, c, s, d);
}

// after the checks; n_pages >= 1.  No workspace and no lock: the destination is the only memory written.
int deblur_batch(const DbSpec& sp, const PageArgs& a, int channels, bool f32, hipStream_t stream)
{
    const DbCfg c = make_cfg(sp, a.width, a.height, channels);
    const int tw = deblur_tile_width(c.nx, c.ny, channels);
    const int chunk = stage_chunk(a.n_pages, 0, 0, kDbChunk);
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int cnt = std::min(chunk, a.n_pages - first);
        const PageSet s = src_pages(a, first);
        const PageSetOut d = dst_pages(a, first);
        switch (tw) {
        case 256: launch_tw<256>(c, f32, s, d, cnt, stream); break;
        case 128: launch_tw<128>(c, f32, s, d, cnt, stream); break;
        case 64: launch_tw<64>(c, f32, s, d, cnt, stream); break;
        default: launch_tw<32>(c, f32, s, d, cnt, stream); break;
        }
        PRL_HIP_CHECK(hipGetLastError());
    }
    return PRL_OK;
}

int deblur_device_entry(const PageArgs& a, int channels, bool f32, long long kw, long long kh, double sigma_x, double sigma_y,
                        double weight, void* stream)
{
    DbSpec sp;
    int st = deblur_checks(a, channels, f32 ? 4 : 1, kw, kh, sigma_x, sigma_y, weight, true, &sp);
    if (st != PRL_OK) return st;
    if (a.n_pages == 0) return PRL_OK;
    int dev;   // the device check alone
    st = current_device(&dev);
    if (st != PRL_OK) return st;
    return deblur_batch(sp, a, channels, f32, static_cast<hipStream_t>(stream));
}

int deblur_host_entry(const PageArgs& h, int channels, bool f32, long long kw, long long kh, double sigma_x, double sigma_y,
                      double weight)
{
    DbSpec sp;
    const int st = deblur_checks(h, channels, f32 ? 4 : 1, kw, kh, sigma_x, sigma_y, weight, false, &sp);
    if (st != PRL_OK) return st;
    return stage_host_pages(h, channels, channels * (f32 ? 4 : 1), h.width, h.height,
                            [&](const PageArgs& page, hipStream_t s) { return deblur_batch(sp, page, channels, f32, s); });
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_basic_deblur_batch_device(int n_pages, int channels, long long kernel_size, double sigma_x, double sigma_y,
                                      double image_weight, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                      int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return deblur_device_entry(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step},
                               channels, false, kernel_size, kernel_size, sigma_x, sigma_y, image_weight, stream);
}

int prl_hip_basic_deblur_host(int channels, long long kernel_size, double sigma_x, double sigma_y, double image_weight,
                              const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    return deblur_host_entry(PageArgs{1, src, 0, src_step, width, height, dst, 0, dst_step}, channels, false, kernel_size, kernel_size,
                             sigma_x, sigma_y, image_weight);
}

int prl_hip_gaussian_blur_f32_batch_device(int n_pages, int channels, long long kernel_w, long long kernel_h, double sigma_x,
                                           double sigma_y, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                           int height, float* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return deblur_device_entry(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, reinterpret_cast<uint8_t*>(d_dst),
                                        dst_page_stride, dst_step},
                               channels, true, kernel_w, kernel_h, sigma_x, sigma_y, 1.0, stream);
}

int prl_hip_gaussian_blur_f32_host(int channels, long long kernel_w, long long kernel_h, double sigma_x, double sigma_y,
                                   const uint8_t* src, size_t src_step, int width, int height, float* dst, size_t dst_step)
{
    return deblur_host_entry(PageArgs{1, src, 0, src_step, width, height, reinterpret_cast<uint8_t*>(dst), 0, dst_step}, channels, true,
                             kernel_w, kernel_h, sigma_x, sigma_y, 1.0);
}

int prl_hip_gaussian_blur_size(long long kernel_w, long long kernel_h, double sigma_x, double sigma_y, int* out_w, int* out_h)
{
    const GaussPlan p = gauss_plan(kernel_w, kernel_h, sigma_x, sigma_y);
    if (p.nx == 0 || p.ny == 0 || p.nx > kGaussMaxSide || p.ny > kGaussMaxSide) return PRL_ERR_BAD_WINDOW;
    if (!out_w || !out_h || !std::isfinite(sigma_x) || !std::isfinite(sigma_y)) return PRL_ERR_BAD_ARG;
    *out_w = p.nx;
    *out_h = p.ny;
    return PRL_OK;
}

int prl_hip_gaussian_kernel_f32(int n, double sigma, float* w)
{
    if (n <= 0 || (n & 1) == 0 || n > kGaussMaxSide) return PRL_ERR_BAD_WINDOW;
    if (!w || !std::isfinite(sigma)) return PRL_ERR_BAD_ARG;
    gauss_kernel(n, sigma, w);
    return PRL_OK;
}

}  // extern "C"
