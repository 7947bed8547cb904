// adaptive.hip — cv::adaptiveThreshold on batched 8-bit gray pages, and the reference's binarizers built on it:
// prl::binarizeNativeAdaptive, prl::binarizeAT, prl::binarizeAGT, prl::binarizePureAdaptiveGaussian (src/binarizations/).
//
//   M(y, x)  = local mean of the bs x bs block around (y, x), BORDER_REPLICATE by clamped addresses
//     MEAN_C      S = integer sum of the block, M = saturate_u8(cvRound(S * (1.0 / (bs*bs)))), product in float64
//     GAUSSIAN_C  float32 page -> separable float32 Gaussian -> saturate_u8(cvRound(.)); weights from the host (gauss_weights);
//                 row pass bs >= 7: taps in ascending order, bs 3 / 5: centre, then pairs; column pass: centre, then pairs
//                 outward; every product and every sum rounded to float32 (__fmul_rn / __fadd_rn: never contracted)
//   on       = p - M > -idelta        idelta = ceil(delta) (BINARY) / floor(delta) (BINARY_INV)
//   out      = BINARY: on ? imax : 0, BINARY_INV: on ? 0 : imax      imax = saturate_u8(cvRound(maxValue)); maxValue < 0: 0
//   auto-invert (binarizeNativeAdaptive.cpp:108-111): mean(out) < 128, i.e. imax * #{out == imax} < 128 W H  ->  255 - out
//
// One kernel, k_adaptive<TW, GAUSS, BITS>.  A workgroup owns TW output columns of a run of rows and walks down the page.  Per
// source row it stages TW + bs - 1 clamped pixels in LDS (two buffers: one barrier per row), every lane computes the row
// pass of its column and keeps it in its own column of an LDS ring of bs rows (no lane reads another lane's ring entries).
// MEAN_C slides the column sum (add the entering row sum, subtract the one the ring slot held); GAUSSIAN_C reads its bs ring
// entries per output row.  The ring (bs x TW words) and the row buffers must fit 64 KiB, so TW follows bs:
//     bs <= 61: TW 256     bs <= 123: TW 128     bs <= 245: TW 64     bs <= 255: TW 32 (half a wavefront idles)
// Without auto-invert the kernel writes the byte mask.  With it (on documents the flip is the common outcome) the kernel
// writes one BIT per pixel (a wavefront's ballot, 8 bytes per 64 pixels) into the device scratch and counts the set bits per
// page; k_adaptive_expand then writes the byte mask once with the flip applied: 2.25 bytes of traffic per pixel instead of
// the 4 a read-modify-write pass over the byte mask would need.
//
// The composed entry runs BGR -> gray (glue.hip) and the median (median.hip) in the order the reference's function has, with
// the intermediates in the device scratch and nothing but stream order between the stages.
#include "prl_internal.h"

#include <algorithm>
#include <cmath>

namespace prl_hip {

namespace {

constexpr int kAdMaxBlock = 255;   // the weights travel as kernel arguments: (bs + 1) / 2 floats
constexpr size_t kAdChunkBytes = (size_t)4 << 30;   // scratch per group of launches at most (one page at least)

struct AdCfg {
    int W, H, bs;
    int inv;        // THRESH_BINARY_INV
    int idelta;     // clamped to [-256, 256]: p - M lies in [-255, 255]
    int imax;
    int rows;       // output rows per workgroup
    double f;       // 1.0 / (bs * bs)
    float wh[(kAdMaxBlock + 1) / 2];   // wh[j] = w[bs / 2 + j] = w[bs / 2 - j]
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid = (ceil(W / TW), ceil(H / rows), pages); dynamic LDS: (bs * TW + 2 * (TW + bs - 1)) words
template <int TW, bool GAUSS, bool BITS>
__global__ __launch_bounds__(TW < 64 ? 64 : TW) void k_adaptive(AdCfg c, PageSet src, PageSetOut dst, uint8_t* bits, size_t bits_page,
                                                                size_t bits_step, unsigned* count)
{
    constexpr int NT = TW < 64 ? 64 : TW;
    extern __shared__ uint32_t lds[];
    const int bs = c.bs, r = bs >> 1, SW = TW + 2 * r;
    uint32_t* ring = lds;              // [bs][TW]: source row y0 - r + i lives in slot i % bs
    uint32_t* srow = lds + bs * TW;    // [2][SW]
    const int t = threadIdx.x, x0 = blockIdx.x * TW, x = x0 + t;
    const bool active = t < TW && x < c.W;
    const int page = blockIdx.z;
    const uint8_t* sp = src.page(page);
    const int y0 = blockIdx.y * c.rows, y1 = min(y0 + c.rows, c.H);
    unsigned V = 0, n_set = 0;
    int slot = 0;
    for (int it = 0, yy = y0 - r; yy < y1 + r; ++yy, ++it) {
        const uint8_t* prow = sp + (size_t)clampi(yy, 0, c.H - 1) * src.step;
        uint32_t* sb = srow + (it & 1) * SW;
        for (int i = t; i < SW; i += NT) {
            const uint32_t v = prow[clampi(x0 - r + i, 0, c.W - 1)];
            sb[i] = GAUSS ? __float_as_uint((float)v) : v;
        }
        __syncthreads();
        bool set = false;
        if (active) {
            int M = 0;
            if (GAUSS) {
                const float* sf = reinterpret_cast<const float*>(sb) + t;
                float* rf = reinterpret_cast<float*>(ring) + t;
                float a;
                if (bs >= 7) {
                    a = __fmul_rn(c.wh[r], sf[0]);
                    for (int k = 1; k < bs; ++k) a = __fadd_rn(a, __fmul_rn(c.wh[k < r ? r - k : k - r], sf[k]));
                } else {
                    a = __fmul_rn(sf[r], c.wh[0]);
                    for (int k = 1; k <= r; ++k) a = __fadd_rn(a, __fmul_rn(__fadd_rn(sf[r + k], sf[r - k]), c.wh[k]));
                }
                rf[slot * TW] = a;
                if (it >= 2 * r) {
                    int sc = slot - r;   // the centre row's slot
                    if (sc < 0) sc += bs;
                    float m = __fmul_rn(c.wh[0], rf[sc * TW]);
                    int su = sc, sd = sc;
                    for (int k = 1; k <= r; ++k) {
                        su = su + 1 == bs ? 0 : su + 1;
                        sd = sd == 0 ? bs - 1 : sd - 1;
                        m = __fadd_rn(m, __fmul_rn(c.wh[k], __fadd_rn(rf[su * TW], rf[sd * TW])));
                    }
                    M = (int)fminf(fmaxf(rintf(m), 0.f), 255.f);
                }
            } else {
                const uint32_t* su = sb + t;
                unsigned hs = 0;
                for (int k = 0; k < bs; ++k) hs += su[k];
                if (it >= bs) V -= ring[slot * TW + t];
                V += hs;
                ring[slot * TW + t] = hs;
                if (it >= 2 * r) M = clampi(__double2int_rn((double)V * c.f), 0, 255);
            }
            if (it >= 2 * r) {
                const int y = yy - r;
                const int p = sp[(size_t)y * src.step + x];
                set = (p - M > -c.idelta) != (c.inv != 0);
                if (!BITS) dst.page(page)[(size_t)y * dst.step + x] = set ? (uint8_t)c.imax : (uint8_t)0;
            }
        }
        if (BITS && it >= 2 * r) {
            const unsigned long long mask = __ballot(set);
            n_set += (unsigned)__popcll(mask);
            if ((t & 63) == 0) {
                uint8_t* brow = bits + (size_t)page * bits_page + (size_t)(yy - r) * bits_step;
                if (TW >= 64) {
                    if (x < c.W) *reinterpret_cast<unsigned long long*>(brow + (size_t)(x >> 6) * 8) = mask;
                } else {
                    *reinterpret_cast<uint32_t*>(brow + (size_t)(x0 >> 5) * 4) = (uint32_t)mask;
                }
            }
        }
        slot = slot + 1 == bs ? 0 : slot + 1;
    }
    if (BITS && (t & 63) == 0 && n_set) atomicAdd(count + page, n_set);
}

// a lane expands one byte of the bit plane: 8 pixels
__global__ __launch_bounds__(256) void k_adaptive_expand(const uint8_t* bits, size_t bits_page, size_t bits_step, const unsigned* count,
                                                         PageSetOut dst, int W, int H, int imax)
{
    const int page = blockIdx.z, y = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x, x = b * 8;
    if (x >= W) return;
    const bool flip = (unsigned long long)imax * count[page] < 128ull * (unsigned long long)W * (unsigned long long)H;
    const uint32_t von = flip ? 255u - (uint32_t)imax : (uint32_t)imax, voff = flip ? 255u : 0u;
    const uint32_t m = bits[(size_t)page * bits_page + (size_t)y * bits_step + b];
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + x;
    const int n = min(8, W - x);
    if (n == 8 && ((size_t)d & 7) == 0) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (((m >> i) & 1u) ? von : voff) << (8 * i);
            hi |= (((m >> (4 + i)) & 1u) ? von : voff) << (8 * i);
        }
        *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
    } else {
        for (int i = 0; i < n; ++i) d[i] = (uint8_t)(((m >> i) & 1u) ? von : voff);
    }
}

__global__ __launch_bounds__(256) void k_adaptive_zero(unsigned* count, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) count[i] = 0;
}

// cv::getGaussianKernel(bs, -1, CV_32F) as cv::GaussianBlur asks for it: fixed tables up to 7, else float64 terms, the sum
// in index order, one float32 rounding of t_i * (1 / sum).  Symmetric bit for bit (x_i = -x_(bs-1-i) exactly).
void gauss_weights(int bs, float* wh)
{
    const int r = bs / 2;
    if (bs == 3) { wh[0] = 0.5f; wh[1] = 0.25f; return; }
    if (bs == 5) { wh[0] = 0.375f; wh[1] = 0.25f; wh[2] = 0.0625f; return; }
    if (bs == 7) { wh[0] = 0.28125f; wh[1] = 0.21875f; wh[2] = 0.109375f; wh[3] = 0.03125f; return; }
    const double sigma = ((bs - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2x = -0.5 / (sigma * sigma);
    double t[kAdMaxBlock];
    double sum = 0;
    for (int i = 0; i < bs; ++i) {
        const double x = i - (bs - 1) * 0.5;
        t[i] = std::exp(scale2x * x * x);
        sum += t[i];
    }
    sum = 1.0 / sum;
    for (int j = 0; j <= r; ++j) wh[j] = (float)(t[r + j] * sum);
}

struct AdSpec {
    int method, type, block, auto_invert;
    double max_value, delta;
};

// EMPTY is the caller's; BAD_WINDOW here, BAD_ARG for the values after the caller's channel check (spec_args)
int spec_window(const AdSpec& s)
{
    return (s.block < 3 || (s.block & 1) == 0 || s.block > kAdMaxBlock) ? PRL_ERR_BAD_WINDOW : PRL_OK;
}
int spec_args(const AdSpec& s)
{
    if (s.method != PRL_ADAPTIVE_MEAN_C && s.method != PRL_ADAPTIVE_GAUSSIAN_C) return PRL_ERR_BAD_ARG;
    if (s.type != PRL_THRESH_BINARY && s.type != PRL_THRESH_BINARY_INV) return PRL_ERR_BAD_ARG;
    if (std::isnan(s.max_value) || std::isnan(s.delta)) return PRL_ERR_BAD_ARG;
    return PRL_OK;
}

AdCfg make_cfg(const AdSpec& s, int W, int H)
{
    AdCfg c{};
    c.W = W; c.H = H; c.bs = s.block;
    c.inv = s.type == PRL_THRESH_BINARY_INV;
    const double d = c.inv ? std::floor(s.delta) : std::ceil(s.delta);
    c.idelta = (int)std::min(256.0, std::max(-256.0, d));
    c.imax = s.max_value < 0 ? 0 : (int)std::min(255.0, std::max(0.0, std::nearbyint(s.max_value)));   // half to even
    c.rows = std::min(H, std::max(96, 6 * s.block));
    c.f = 1.0 / ((double)s.block * s.block);
    if (s.method == PRL_ADAPTIVE_GAUSSIAN_C) gauss_weights(s.block, c.wh);
    return c;
}

size_t bits_step_of(int W) { return (size_t)((W + 63) / 64) * 8; }

template <int TW>
void launch_tw(const AdCfg& c, bool gauss, bool bits, const PageSet& s, const PageSetOut& d, int n, uint8_t* bp, size_t bits_page,
               unsigned* count, hipStream_t stream)
{
    constexpr int NT = TW < 64 ? 64 : TW;
    const dim3 grid((unsigned)((c.W + TW - 1) / TW), (unsigned)((c.H + c.rows - 1) / c.rows), (unsigned)n);
    const size_t lds = ((size_t)c.bs * TW + 2 * (size_t)(TW + c.bs - 1)) * 4;
    const size_t bstep = bits_step_of(c.W);
    if (gauss) {
        if (bits) hipLaunchKernelGGL((k_adaptive<TW, true, true>), grid, dim3(NT), lds, stream, c, s, d, bp, bits_page, bstep, count);
        else hipLaunchKernelGGL((k_adaptive<TW, true, false>), grid, dim3(NT), lds, stream, c, s, d, bp, bits_page, bstep, count);
    } else {
        if (bits) hipLaunchKernelGGL((k_adaptive<TW, false, true>), grid, dim3(NT), lds, stream, c, s, d, bp, bits_page, bstep, count);
        else hipLaunchKernelGGL((k_adaptive<TW, false, false>), grid, dim3(NT), lds, stream, c, s, d, bp, bits_page, bstep, count);
    }
}

size_t bits_bytes_per_page(int W, int H) { return r256(bits_step_of(W) * (size_t)H); }

// n <= 65535 gray pages; with auto-invert `work` holds [n counters | n bit planes] (ad_work_bytes)
size_t ad_work_bytes(const AdSpec& s, int W, int H, int n)
{
    return s.auto_invert ? r256((size_t)n * 4) + bits_bytes_per_page(W, H) * (size_t)n : 0;
}

int adaptive_run(const AdSpec& sp, int W, int H, const PageSet& s, const PageSetOut& d, int n, uint8_t* work, hipStream_t stream)
{
    const AdCfg c = make_cfg(sp, W, H);
    const bool gauss = sp.method == PRL_ADAPTIVE_GAUSSIAN_C, bits = sp.auto_invert != 0;
    unsigned* count = reinterpret_cast<unsigned*>(work);
    uint8_t* bp = bits ? work + r256((size_t)n * 4) : nullptr;
    const size_t bits_page = bits_bytes_per_page(W, H);
    if (bits) hipLaunchKernelGGL(k_adaptive_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, count, n);
    if (c.bs <= 61) launch_tw<256>(c, gauss, bits, s, d, n, bp, bits_page, count, stream);
    else if (c.bs <= 123) launch_tw<128>(c, gauss, bits, s, d, n, bp, bits_page, count, stream);
    else if (c.bs <= 245) launch_tw<64>(c, gauss, bits, s, d, n, bp, bits_page, count, stream);
    else launch_tw<32>(c, gauss, bits, s, d, n, bp, bits_page, count, stream);
    if (bits) {
        const dim3 grid((unsigned)(((W + 7) / 8 + 255) / 256), (unsigned)H, (unsigned)n);
        hipLaunchKernelGGL(k_adaptive_expand, grid, dim3(256), 0, stream, bp, bits_page, bits_step_of(W), count, d, W, H, c.imax);
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

AdSpec spec_of(const prl_adaptive_params* p)
{
    return AdSpec{p->method, p->type, p->block_size, p->auto_invert, p->max_value, p->delta};
}

// statuses of the composed entry, before any device is touched; batch: the *_batch_device entry
int binarize_check(const prl_adaptive_params* p, const PageArgs& a, int channels, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (!p) return PRL_ERR_BAD_ARG;
    st = spec_window(spec_of(p));
    if (st != PRL_OK) return st;
    if (p->median_ksize < 0 || (p->median_ksize != 0 && (p->median_ksize & 1) == 0)) return PRL_ERR_BAD_WINDOW;
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, 1, batch)) != PRL_OK) return st;
    if (pages_sides_ok(a) != PRL_OK || p->median_ksize > 65535) return PRL_ERR_BAD_ARG;
    // never in place: every output reads its neighbours' inputs
    if (batch && (st = pages_overlap_ok(a, channels, 1, false)) != PRL_OK) return st;
    return spec_args(spec_of(p));
}

int binarize_batch_device(const prl_adaptive_params* p, int channels, const PageArgs& a, void* stream)
{
    int st = binarize_check(p, a, channels, true);
    if (st != PRL_OK) return st;
    if (a.n_pages == 0) return PRL_OK;
    const int width = a.width, height = a.height;
    const size_t R = (size_t)width * channels;
    const AdSpec sp = spec_of(p);
    const bool med = p->median_ksize >= 3, color = channels > 1;
    const bool med_color = med && color && p->median_on_color;
    // planes per page in the scratch: A = the first stage's result when two stages precede the threshold, G = the gray page
    // the threshold reads when any does
    const size_t gray = r256((size_t)width * height);
    const size_t a_bytes = (med && color) ? (med_color ? r256(R * (size_t)height) : gray) : 0;
    const size_t g_bytes = (med || color) ? gray : 0;
    const size_t per_page = a_bytes + g_bytes + ad_work_bytes(sp, width, height, 1) + 4;
    const int chunk = stage_chunk(a.n_pages, per_page, kAdChunkBytes);
    const size_t work_bytes = ad_work_bytes(sp, width, height, chunk);
    WorkScope w;
    st = w.open(stream, work_bytes + (a_bytes + g_bytes) * (size_t)chunk, 0, 0);
    if (st != PRL_OK) return st;
    const hipStream_t hs = w.stream;
    uint8_t* work = w.scratch();
    uint8_t* A = work + work_bytes;
    uint8_t* G = A + a_bytes * (size_t)chunk;
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int cnt = std::min(chunk, a.n_pages - first);
        PageSet cur = src_pages(a, first);
        const PageSetOut ga = page_set_out(G, gray, (size_t)width);
        if (med_color) {   // binarizeAT.cpp / binarizeAGT.cpp: medianBlur on the colour page, then cvtColor
            const PageSetOut pa = page_set_out(A, a_bytes, R);
            st = median_pass_pages(width, height, channels, p->median_ksize, cur, pa, cnt, hs);
            if (st != PRL_OK) return st;
            st = prl_hip_bgr2gray_batch_device(cnt, channels, A, a_bytes, R, width, height, G, gray, (size_t)width, stream);
            if (st != PRL_OK) return st;
        } else if (color) {   // binarizeNativeAdaptive.cpp: cvtColor, then medianBlur
            uint8_t* g1 = med ? A : G;
            st = prl_hip_bgr2gray_batch_device(cnt, channels, cur.base, a.src_page_stride, a.src_step, width, height, g1, gray,
                                               (size_t)width, stream);
            if (st != PRL_OK) return st;
            if (med) {
                const PageSet pa = page_set(A, gray, (size_t)width);
                st = median_pass_pages(width, height, 1, p->median_ksize, pa, ga, cnt, hs);
                if (st != PRL_OK) return st;
            }
        } else if (med) {
            st = median_pass_pages(width, height, 1, p->median_ksize, cur, ga, cnt, hs);
            if (st != PRL_OK) return st;
        }
        if (med || color) cur = as_source(ga);
        st = adaptive_run(sp, width, height, cur, dst_pages(a, first), cnt, work, hs);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_adaptive_threshold_batch_device(int n_pages, int method, int type, double max_value, int block_size, double delta,
                                            int auto_invert, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                            int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    prl_adaptive_params p{};
    p.method = method; p.type = type; p.max_value = max_value; p.block_size = block_size; p.delta = delta;
    p.auto_invert = auto_invert;
    return prl_hip_binarize_adaptive_batch_device(&p, n_pages, 1, d_src, src_page_stride, src_step, width, height, d_dst,
                                                  dst_page_stride, dst_step, stream);
}

int prl_hip_adaptive_threshold_host(int method, int type, double max_value, int block_size, double delta, int auto_invert,
                                    const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    prl_adaptive_params p{};
    p.method = method; p.type = type; p.max_value = max_value; p.block_size = block_size; p.delta = delta;
    p.auto_invert = auto_invert;
    return prl_hip_binarize_adaptive_host(&p, 1, src, src_step, width, height, dst, dst_step);
}

void prl_hip_default_adaptive_params(prl_adaptive_params* out)
{
    if (!out) return;
    *out = prl_adaptive_params{};
    out->median_ksize = 5;                       // binarizeNativeAdaptive.h:62-74
    out->median_on_color = 0;
    out->method = PRL_ADAPTIVE_GAUSSIAN_C;
    out->type = PRL_THRESH_BINARY_INV;
    out->max_value = 255.0;
    out->block_size = 19;
    out->delta = 9.0;
    out->auto_invert = 1;
}

int prl_hip_binarize_adaptive_batch_device(const prl_adaptive_params* p, int n_pages, int channels, const uint8_t* d_src,
                                           size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                           size_t dst_page_stride, size_t dst_step, void* stream)
{
    return binarize_batch_device(p, channels, PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step},
                                 stream);
}

int prl_hip_binarize_adaptive_host(const prl_adaptive_params* p, int channels, const uint8_t* src, size_t src_step, int width,
                                   int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = binarize_check(p, a, channels, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, 1, width, height,
                            [&](const PageArgs& page, hipStream_t s) { return binarize_batch_device(p, channels, page, s); });
}

}  // extern "C"
