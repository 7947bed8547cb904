// tone.hip — point operations whose table depends on page statistics: prl::gammaCorrection (src/balance/gammaCorrection.cpp:52-106),
// prl::simpleWhiteBalance (balanceSimpleWhite.cpp:33-142), prl::grayWorldWhiteBalance (balanceGrayWorldWhite.cpp:37-115) and
// prl::cleanBackgroundToWhite (src/cleanBackgroundToWhite.cpp:39-64), plus the two primitives they are made of.
//
// Every output byte of the four is a function of the input byte and of the page's per-channel histograms only, so each runs as
//   histogram[page][channel][256]  ->  table[page][channel][256]  ->  dst = table[src]
// and is exact by construction, also where the reference computes in float or double per pixel.
//   k_tone_hist<C>     C = 1..4 interleaved channels.  A lane takes 4 pixels (C dwords, bytes unpacked at compile-time positions);
//                      bins in LDS, one global atomic per non-empty bin and workgroup.  A wavefront whose 256 pixels agree in a
//                      channel adds once for that channel (the test is per channel: paper is flat in each, not across them).
//   k_tone_derive      one workgroup per page: the tables of simpleWhiteBalance and of grayWorld with pNorm == 1 from the
//                      histograms, with the same inline functions the host builders (prl_hip_*_luts) run.
//   k_tone_put         a 256-byte table passed by value into device memory (gamma, the clean-background curve: no copy from
//                      host memory, nothing to keep alive).
//   k_tone_lut<C, OC>  dst(y, x, c) = table[page][c][src(y, x, c)], c < OC (OC == C, or 4 -> 3: the alpha byte is dropped).
//                      Tables in LDS, 8 pixels per thread, dword loads and stores, a scalar tail per row.
// cleanBackgroundToWhite = bgnorm.hip's pixBackgroundNormSimple into the destination, then k_tone_lut in place with the fixed
// pixGammaTRC(1.0, 70, 170) table: a second pass over the result instead of a second instantiation of k_bg_apply, whose code
// and arguments stay what they are.
#include "prl_internal.h"

#include <algorithm>
#include <cmath>

namespace prl_hip {

// bgnorm.hip
int bgnorm_run(int n_pages, int channels, const PageSet& src, int width, int height, const PageSetOut& dst, void* work,
               hipStream_t stream, uint8_t* out_raw, unsigned short* out_inv, int* out_fail);
size_t bgnorm_work_bytes(int n_pages, int channels, int width, int height);

namespace {

constexpr int kToneThreads = 256;
constexpr int kTonePx = 8;            // pixels per thread of k_tone_lut
constexpr int kToneChunk = 16384;     // pages per launch (grid.y / grid.z; 3840 bytes of tables and bins per page)

// ---- the arithmetic, shared by the host builders and k_tone_derive ---------------------------------------------------------

// balanceSimpleWhite.cpp:66-88 for one channel: the cumulative histogram as int, both scans stopped at the array's ends
// (the reference reads outside it for an all-zero channel and for k > 1), the +1 below 254.
__host__ __device__ inline void swb_range(double k, const unsigned* hist, int pixels, int* vmin_out, int* vmax_out)
{
    const size_t total = (size_t)pixels;   // cols * rows
    int all = 0;
    for (int v = 0; v < 256; ++v) all += (int)hist[v];
    int vmin = 0, vmax = 255;
    int cum = (int)hist[0];   // hists[i][vmin] after the running sum
    while (vmin < 255 && cum < k * total) {
        vmin += 1;
        cum += (int)hist[vmin];
    }
    cum = all;                // hists[i][vmax]
    while (vmax > 0 && cum > (1 - k) * total) {
        cum -= (int)hist[vmax];
        vmax -= 1;
    }
    if (vmax < 255 - 1) vmax += 1;
    *vmin_out = vmin;
    *vmax_out = vmax;
}

// :90-137: clamp to vmin, then to vmax, int times float, truncation.  0 * inf (vmax == vmin) is NaN and converts to 0, as
// cvttss2si's 0x80000000 does; every other product lies in [0, 256).
__host__ __device__ inline uint8_t swb_entry(int v, int vmin, int vmax)
{
    const float scale = 255.0f / (vmax - vmin);
    int val = v;
    if (val < vmin) val = vmin;
    if (val > vmax) val = vmax;
    const float f = (val - vmin) * scale;
    if (f != f) return 0;
    return (uint8_t)(int)f;
}

// balanceGrayWorldWhite.cpp:37-56 with pNorm == 1 for one channel: every term and partial sum is an exact integer, so the sum
// over the bins equals the reference's raster-order sum bit for bit; pow(x, 1) is skipped.
__host__ __device__ inline double gw_mean_p1(const unsigned* hist, int pixels)
{
    double s = 0.0;
    for (int v = 0; v < 256; ++v)
        if (hist[v]) s += (double)hist[v] * (double)v;
    return s / pixels;
}

// :77-87 from the three means (ml, ma, mb = channels 0, 1, 2)
__host__ __device__ inline void gw_ratios(const double m[3], int with_max, double ratio[3])
{
    const double ml = m[0], ma = m[1], mb = m[2];
    double r = (ma + mb + ml) / 3.0;
    if (with_max) {
        const double inner = mb < ml ? ml : mb;   // std::max(mb, ml)
        r = ma < inner ? inner : ma;              // std::max(ma, ...)
    }
    for (int c = 0; c < 3; ++c) ratio[c] = r / m[c];
}

// :97-108: std::min(255.0, l) hands a NaN through as 255 (an all-zero channel comes out all 255)
__host__ __device__ inline uint8_t gw_entry(int v, double ratio)
{
    const double l = v * ratio;
    return (uint8_t)(l < 255.0 ? l : 255.0);
}

// saturate_cast<uchar> of a double / of a float (sat_u8_literal): round half to even; NaN, +-inf and what lies
// outside int32 give 0
inline uint8_t sat_u8_host(double t)
{
    if (t != t) return 0;
    const double r = std::nearbyint(t);
    if (!(r >= -2147483648.0 && r <= 2147483647.0)) return 0;
    return r < 0.0 ? 0 : (r > 255.0 ? 255 : (uint8_t)r);
}

struct ToneTab { uint8_t v[256]; };

// the k step of gammaCorrection.cpp:99-102: Mat *= k on 8U is convertTo(8U, k), float32 [upstream]
void gamma_k_step(double k, ToneTab* t)
{
    if (std::abs(k - 1.0) <= 1e-7) return;   // eq_d
    for (int v = 0; v < 256; ++v) t->v[v] = sat_u8_host((double)((float)t->v[v] * (float)k));
}

void gamma_table(double k, double gamma, bool with_gamma, ToneTab* t)
{
    for (int v = 0; v < 256; ++v)
        t->v[v] = with_gamma ? sat_u8_host(std::pow((double)(v / 255.0), gamma) * 255.0) : (uint8_t)v;
    gamma_k_step(k, t);
}

// numaGammaTRC(1.0, 70, 170) [upstream]
void clean_table(ToneTab* t)
{
    const int minval = 70, maxval = 170;
    for (int i = 0; i < 256; ++i) {
        if (i < minval) t->v[i] = 0;
        else if (i > maxval) t->v[i] = 255;
        else {
            const float x = (float)(i - minval) / (float)(maxval - minval);
            int val = (int)(255. * x + 0.5);   // powf(x, 1.f) is x
            val = std::max(val, 0);
            val = std::min(val, 255);
            t->v[i] = (uint8_t)val;
        }
    }
}

void swb_tables(double k, const unsigned* hist, int pixels, uint8_t* luts)
{
    for (int c = 0; c < 3; ++c) {
        int vmin, vmax;
        swb_range(k, hist + c * 256, pixels, &vmin, &vmax);
        for (int v = 0; v < 256; ++v) luts[c * 256 + v] = swb_entry(v, vmin, vmax);
    }
}

// the canonical sum of the header: ascending bins, (double)hist[v] * pow(v, p); empty bins add nothing
void gw_tables(double p, int with_max, const unsigned* hist, int pixels, uint8_t* luts)
{
    double m[3], ratio[3];
    for (int c = 0; c < 3; ++c) {
        const unsigned* h = hist + c * 256;
        if (p == 1.0) {
            m[c] = gw_mean_p1(h, pixels);
            continue;
        }
        double s = 0.0;
        for (int v = 0; v < 256; ++v)
            if (h[v]) s += (double)h[v] * std::pow((double)v, p);
        m[c] = std::pow(s / pixels, 1.0 / p);
    }
    gw_ratios(m, with_max, ratio);
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) luts[c * 256 + v] = gw_entry(v, ratio[c]);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

// grid = (column groups, row groups, pages).  hist: [page][C][256], zeroed before the launch.
template <int C>
__global__ __launch_bounds__(kToneThreads) void k_tone_hist(PageSet src, int W, int H, unsigned* __restrict__ hist)
{
    __shared__ unsigned h[C * 256];
    const int page = blockIdx.z, t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < C; ++c) h[c * 256 + t] = 0;
    __syncthreads();
    const uint8_t* base = src.page(page);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint8_t* row = base + (size_t)y * src.step;
        // every lane of a wavefront makes the same number of trips (the ballot below needs them all)
        for (int xb = blockIdx.x * kToneThreads * 4; xb < W; xb += gridDim.x * kToneThreads * 4) {
            const int x = xb + t * 4;
            const int n = min(4, W - x);   // <= 0: no pixel
            unsigned v[4][C];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) v[i][c] = 0;
            if (n == 4) {
                const uint8_t* s = row + (size_t)x * C;
                unsigned w[C];   // C == 3: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
#pragma unroll
                for (int i = 0; i < C; ++i) __builtin_memcpy(&w[i], s + 4 * i, 4);   // (any alignment)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int b = i * C + c;
                        v[i][c] = (w[b / 4] >> (8 * (b % 4))) & 0xffu;
                    }
            } else if (n > 0) {
                const uint8_t* s = row + (size_t)x * C;
                for (int i = 0; i < n; ++i)
#pragma unroll
                    for (int c = 0; c < C; ++c) v[i][c] = s[i * C + c];
            }
            // a page is mostly paper: a wavefront that sees one value in a channel adds once instead of 64 times to one LDS word
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool flat = n == 4 && v[1][c] == v[0][c] && v[2][c] == v[0][c] && v[3][c] == v[0][c];
                const unsigned v0 = (unsigned)__shfl((int)v[0][c], 0);
                if (__all(flat && v[0][c] == v0)) {
                    if ((t & 63) == 0) atomicAdd(&h[c * 256 + v0], 256u);
                } else if (flat) {
                    atomicAdd(&h[c * 256 + v[0][c]], 4u);
                } else {
                    for (int i = 0; i < n; ++i) atomicAdd(&h[c * 256 + v[i][c]], 1u);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (h[c * 256 + t]) atomicAdd(&hist[((size_t)page * C + c) * 256 + t], h[c * 256 + t]);
}

// grid = (ceil(groups * H / 256), pages), groups of 8 pixels numbered row after row.  lut: [page][OC][256] bytes, a page
// lut_page_stride bytes after the previous one (0: one set for all pages).
template <int C, int OC>
__global__ __launch_bounds__(kToneThreads) void k_tone_lut(PageSet src, PageSetOut dst, int W, int H, const uint8_t* __restrict__ lut,
                                                           size_t lut_page_stride)
{
    __shared__ unsigned tabw[OC * 64];
    uint8_t* tab = reinterpret_cast<uint8_t*>(tabw);
    const int page = blockIdx.y, t = threadIdx.x;
    const uint8_t* lp = lut + (size_t)page * lut_page_stride;
#pragma unroll
    for (int c = 0; c < OC; ++c) tab[c * 256 + t] = lp[c * 256 + t];
    __syncthreads();
    const unsigned groups = (unsigned)(W + kTonePx - 1) / (unsigned)kTonePx;
    const unsigned gi = blockIdx.x * (unsigned)kToneThreads + t;
    const int y = (int)(gi / groups);
    if (y >= H) return;
    const int x0 = (int)(gi - (unsigned)y * groups) * kTonePx;
    const int n = min(kTonePx, W - x0);
    const uint8_t* s = src.page(page) + (size_t)y * src.step + (size_t)x0 * C;
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + (size_t)x0 * OC;
    if (n == kTonePx) {
        unsigned in[kTonePx * C / 4], out[kTonePx * OC / 4];
#pragma unroll
        for (int i = 0; i < kTonePx * C / 4; ++i) __builtin_memcpy(&in[i], s + 4 * i, 4);   // (any alignment)
#pragma unroll
        for (int i = 0; i < kTonePx * OC / 4; ++i) out[i] = 0;
#pragma unroll
        for (int px = 0; px < kTonePx; ++px)
#pragma unroll
            for (int c = 0; c < OC; ++c) {
                const int bi = px * C + c, bo = px * OC + c;
                const unsigned p = (in[bi / 4] >> (8 * (bi % 4))) & 0xffu;
                out[bo / 4] |= (unsigned)tab[c * 256 + p] << (8 * (bo % 4));
            }
#pragma unroll
        for (int i = 0; i < kTonePx * OC / 4; ++i) __builtin_memcpy(d + 4 * i, &out[i], 4);
    } else {
        for (int px = 0; px < n; ++px)
#pragma unroll
            for (int c = 0; c < OC; ++c) d[px * OC + c] = tab[c * 256 + s[px * C + c]];
    }
}

enum { kDeriveSimpleWhite = 0, kDeriveGrayWorld1 = 1 };

// grid = pages, 256 threads.  hist: [page][3][256]; lut: [page][3][256] bytes.
__global__ __launch_bounds__(kToneThreads) void k_tone_derive(int mode, double k, int with_max, int W, int H,
                                                              const unsigned* __restrict__ hist, uint8_t* __restrict__ lut)
{
    __shared__ int s_vmin[3], s_vmax[3];
    __shared__ double s_mean[3], s_ratio[3];
    const int page = blockIdx.x, t = threadIdx.x;
    const unsigned* h = hist + (size_t)page * 3 * 256;
    uint8_t* out = lut + (size_t)page * 3 * 256;
    if (t < 3) {   // the scans are chains of 256 dependent steps: one lane per channel
        if (mode == kDeriveSimpleWhite) swb_range(k, h + t * 256, W * H, &s_vmin[t], &s_vmax[t]);
        else s_mean[t] = gw_mean_p1(h + t * 256, W * H);
    }
    __syncthreads();
    if (mode == kDeriveGrayWorld1) {
        if (t == 0) gw_ratios(s_mean, with_max, s_ratio);
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * 256 + t] = mode == kDeriveSimpleWhite ? swb_entry(t, s_vmin[c], s_vmax[c]) : gw_entry(t, s_ratio[c]);
}

// grid = copies, 256 threads
__global__ __launch_bounds__(kToneThreads) void k_tone_put(ToneTab tab, uint8_t* __restrict__ out)
{
    out[blockIdx.x * 256 + threadIdx.x] = tab.v[threadIdx.x];
}

// ---- host ------------------------------------------------------------------------------------------------------------------

// the checks every entry makes, in the documented order (no device is touched).  channels_ok: the entry's own rule; oc: channels
// of the result (0: the entry has no destination); batch: a *_batch_device entry (a page count, and source and destination may
// meet)
int tone_checks(const PageArgs& a, bool channels_ok, int channels, int oc, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (!channels_ok) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, oc, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    // in place: as many channels out as in, at the same strides (a thread reads its pixels before it writes them)
    return batch ? pages_overlap_ok(a, channels, oc, true) : PRL_OK;
}

}  // namespace

// the histogram pass and the table pass, also for clahe.hip (cv::equalizeHist); they enqueue only
int hist_launch(int channels, const PageSet& src, int n, int W, int H, unsigned* hist, hipStream_t stream)
{
    PRL_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n * channels * 256 * sizeof(unsigned), stream));
    const dim3 grid((unsigned)std::min(8, (W + kToneThreads * 4 - 1) / (kToneThreads * 4)), (unsigned)std::min(H, 64), (unsigned)n);
    switch (channels) {
    case 1: hipLaunchKernelGGL(k_tone_hist<1>, grid, dim3(kToneThreads), 0, stream, src, W, H, hist); break;
    case 2: hipLaunchKernelGGL(k_tone_hist<2>, grid, dim3(kToneThreads), 0, stream, src, W, H, hist); break;
    case 3: hipLaunchKernelGGL(k_tone_hist<3>, grid, dim3(kToneThreads), 0, stream, src, W, H, hist); break;
    default: hipLaunchKernelGGL(k_tone_hist<4>, grid, dim3(kToneThreads), 0, stream, src, W, H, hist); break;
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// oc == channels, or channels == 4 and oc == 3
int lut_launch(int channels, int oc, const PageSet& src, const PageSetOut& dst, int n, int W, int H, const uint8_t* lut,
               size_t lut_page_stride, hipStream_t stream)
{
    const size_t groups = (size_t)((W + kTonePx - 1) / kTonePx) * H;
    const dim3 grid((unsigned)((groups + kToneThreads - 1) / kToneThreads), (unsigned)n), block(kToneThreads);
    if (channels == 4 && oc == 3) hipLaunchKernelGGL((k_tone_lut<4, 3>), grid, block, 0, stream, src, dst, W, H, lut, lut_page_stride);
    else if (channels == 1) hipLaunchKernelGGL((k_tone_lut<1, 1>), grid, block, 0, stream, src, dst, W, H, lut, lut_page_stride);
    else if (channels == 2) hipLaunchKernelGGL((k_tone_lut<2, 2>), grid, block, 0, stream, src, dst, W, H, lut, lut_page_stride);
    else if (channels == 3) hipLaunchKernelGGL((k_tone_lut<3, 3>), grid, block, 0, stream, src, dst, W, H, lut, lut_page_stride);
    else hipLaunchKernelGGL((k_tone_lut<4, 4>), grid, block, 0, stream, src, dst, W, H, lut, lut_page_stride);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

namespace {

// one table for every page and channel: gamma, the clean-background curve
int shared_table_run(const PageArgs& a, int channels, int oc, const ToneTab& tab, bool bgnorm_first, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const int chunk = stage_chunk(a.n_pages, 0, 0, kToneChunk);
    WorkScope w;   // `small`: the table; `scratch`: what bgnorm asks for
    int st = w.open(stream, bgnorm_first ? bgnorm_work_bytes(chunk, channels, a.width, a.height) : 0, 4 * 256, 0);
    if (st != PRL_OK) return st;
    const hipStream_t hs = w.stream;
    uint8_t* lut = w.small();
    hipLaunchKernelGGL(k_tone_put, dim3((unsigned)oc), dim3(kToneThreads), 0, hs, tab, lut);
    PRL_HIP_CHECK(hipGetLastError());
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int n = std::min(chunk, a.n_pages - first);
        const PageSetOut d = dst_pages(a, first);
        if (bgnorm_first) {
            st = bgnorm_run(n, channels, src_pages(a, first), a.width, a.height, d, w.scratch(), hs, nullptr, nullptr, nullptr);
            if (st != PRL_OK) return st;
            st = lut_launch(oc, oc, as_source(d), d, n, a.width, a.height, lut, 0, hs);
        } else {
            st = lut_launch(channels, oc, src_pages(a, first), d, n, a.width, a.height, lut, 0, hs);
        }
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

// simpleWhiteBalance (mode 0) and grayWorld (mode 1): 3 channels, a table set per page from the page's histograms
int derived_table_run(const PageArgs& a, int mode, double param, int with_max, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const bool on_host = mode == kDeriveGrayWorld1 && !(param == 1.0);
    const int chunk = stage_chunk(a.n_pages, 0, 0, kToneChunk);
    const size_t hist_bytes = (size_t)chunk * 3 * 256 * sizeof(unsigned), lut_bytes = (size_t)chunk * 3 * 256;
    WorkScope w;   // `small` (and `pinned` for tables built on the host): [bins of a chunk | tables of a chunk]
    int st = w.open(stream, 0, hist_bytes + lut_bytes, on_host ? hist_bytes + lut_bytes : 0);
    if (st != PRL_OK) return st;
    const hipStream_t hs = w.stream;
    unsigned* hist = w.small<unsigned>();
    uint8_t* lut = w.small() + hist_bytes;
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int n = std::min(chunk, a.n_pages - first);
        const PageSet s = src_pages(a, first);
        st = hist_launch(3, s, n, a.width, a.height, hist, hs);
        if (st != PRL_OK) return st;
        if (!on_host) {
            hipLaunchKernelGGL(k_tone_derive, dim3((unsigned)n), dim3(kToneThreads), 0, hs, mode, param, with_max, a.width, a.height, hist,
                               lut);
            PRL_HIP_CHECK(hipGetLastError());
        } else {
            // pow with a general exponent is the host libm's: the bins come down, the tables go up, the stream is drained twice
            unsigned* h_hist = w.pinned<unsigned>();
            uint8_t* h_lut = w.pinned() + hist_bytes;
            PRL_HIP_CHECK(hipMemcpyAsync(h_hist, hist, (size_t)n * 3 * 256 * sizeof(unsigned), hipMemcpyDeviceToHost, hs));
            PRL_HIP_CHECK(hipStreamSynchronize(hs));
            for (int i = 0; i < n; ++i)
                gw_tables(param, with_max, h_hist + (size_t)i * 3 * 256, a.width * a.height, h_lut + (size_t)i * 3 * 256);
            PRL_HIP_CHECK(hipMemcpyAsync(lut, h_lut, (size_t)n * 3 * 256, hipMemcpyHostToDevice, hs));
            PRL_HIP_CHECK(hipStreamSynchronize(hs));   // the pinned block is the next call's too
        }
        st = lut_launch(3, 3, s, dst_pages(a, first), n, a.width, a.height, lut, (size_t)3 * 256, hs);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int gamma_oc(int channels) { return channels == 4 ? 3 : channels; }
int clean_oc(int channels) { return channels == 1 ? 1 : 3; }

int gamma_device(int channels, double k, double gamma, const PageArgs& a, void* stream)
{
    const bool ok = channels >= 1 && channels <= 4;
    const int st = tone_checks(a, ok, channels, ok ? gamma_oc(channels) : 0, true);
    if (st != PRL_OK) return st;
    ToneTab tab;
    gamma_table(k, gamma, channels != 4, &tab);   // 4 channels: BGRA -> BGR, and the reference's switch has no case for them
    return shared_table_run(a, channels, gamma_oc(channels), tab, false, stream);
}

int clean_device(int channels, const PageArgs& a, void* stream)
{
    const bool ok = channels == 1 || channels == 3 || channels == 4;
    const int st = tone_checks(a, ok, channels, ok ? clean_oc(channels) : 0, true);
    if (st != PRL_OK) return st;
    ToneTab tab;
    clean_table(&tab);
    return shared_table_run(a, channels, clean_oc(channels), tab, true, stream);
}

int balance_device(int mode, double param, int with_max, const PageArgs& a, void* stream)
{
    const int st = tone_checks(a, true, 3, 3, true);
    if (st != PRL_OK) return st;
    return derived_table_run(a, mode, param, with_max, stream);
}

// a *_host entry: the checks without a device, then one page through the staging area
template <typename Run>
int tone_host(int channels, bool channels_ok, int oc, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
              size_t dst_step, Run&& run)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = tone_checks(a, channels_ok, channels, channels_ok ? oc : 0, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, oc, width, height, run);
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_histogram_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                   int height, uint32_t* d_hist, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, nullptr, 0, 0};
    int st = tone_checks(a, channels >= 1 && channels <= 4, channels, 0, true);
    if (st != PRL_OK) return st;
    if (!d_hist) return PRL_ERR_BAD_ARG;
    if (n_pages == 0) return PRL_OK;
    int dev;   // no workspace and no lock: the device check alone
    st = current_device(&dev);
    if (st != PRL_OK) return st;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const int chunk = stage_chunk(n_pages, 0, 0, kToneChunk);
    for (int first = 0; first < n_pages; first += chunk) {
        st = hist_launch(channels, src_pages(a, first), std::min(chunk, n_pages - first), width, height,
                         d_hist + (size_t)first * channels * 256, hs);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int prl_hip_lut_batch_device(int n_pages, int channels, const uint8_t* d_lut, size_t lut_page_stride, const uint8_t* d_src,
                             size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                             size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const bool ok = channels >= 1 && channels <= 4;
    int st = tone_checks(a, ok, channels, ok ? channels : 0, true);
    if (st != PRL_OK) return st;
    if (!d_lut) return PRL_ERR_BAD_ARG;
    if (n_pages == 0) return PRL_OK;
    int dev;   // no workspace and no lock: the device check alone
    st = current_device(&dev);
    if (st != PRL_OK) return st;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const int chunk = stage_chunk(n_pages, 0, 0, kToneChunk);
    for (int first = 0; first < n_pages; first += chunk) {
        st = lut_launch(channels, channels, src_pages(a, first), dst_pages(a, first), std::min(chunk, n_pages - first), width, height,
                        d_lut + (size_t)first * lut_page_stride, lut_page_stride, hs);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int prl_hip_gamma_correction_batch_device(int n_pages, int channels, double k, double gamma, const uint8_t* d_src, size_t src_page_stride,
                                          size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                          size_t dst_step, void* stream)
{
    return gamma_device(channels, k, gamma, PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step},
                        stream);
}

int prl_hip_gamma_correction_host(int channels, double k, double gamma, const uint8_t* src, size_t src_step, int width, int height,
                                  uint8_t* dst, size_t dst_step)
{
    return tone_host(channels, channels >= 1 && channels <= 4, gamma_oc(channels), src, src_step, width, height, dst, dst_step,
                     [&](const PageArgs& a, hipStream_t s) { return gamma_device(channels, k, gamma, a, s); });
}

int prl_hip_simple_white_balance_batch_device(int n_pages, double k, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                              int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                              void* stream)
{
    return balance_device(kDeriveSimpleWhite, k, 0,
                          PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, stream);
}

int prl_hip_simple_white_balance_host(double k, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                                      size_t dst_step)
{
    return tone_host(3, true, 3, src, src_step, width, height, dst, dst_step,
                     [&](const PageArgs& a, hipStream_t s) { return balance_device(kDeriveSimpleWhite, k, 0, a, s); });
}

int prl_hip_gray_world_batch_device(int n_pages, double p_norm, int with_max, const uint8_t* d_src, size_t src_page_stride,
                                    size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                    void* stream)
{
    return balance_device(kDeriveGrayWorld1, p_norm, with_max != 0,
                          PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, stream);
}

int prl_hip_gray_world_host(double p_norm, int with_max, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                            size_t dst_step)
{
    return tone_host(3, true, 3, src, src_step, width, height, dst, dst_step,
                     [&](const PageArgs& a, hipStream_t s) { return balance_device(kDeriveGrayWorld1, p_norm, with_max != 0, a, s); });
}

int prl_hip_clean_background_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                          int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return clean_device(channels, PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step},
                        stream);
}

int prl_hip_clean_background_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                                  size_t dst_step)
{
    return tone_host(channels, channels == 1 || channels == 3 || channels == 4, clean_oc(channels), src, src_step, width, height, dst,
                     dst_step, [&](const PageArgs& a, hipStream_t s) { return clean_device(channels, a, s); });
}

int prl_hip_gamma_lut(double k, double gamma, uint8_t lut[256])
{
    if (!lut) return PRL_ERR_BAD_ARG;
    ToneTab t;
    gamma_table(k, gamma, true, &t);
    std::copy(t.v, t.v + 256, lut);
    return PRL_OK;
}

int prl_hip_clean_background_lut(uint8_t lut[256])
{
    if (!lut) return PRL_ERR_BAD_ARG;
    ToneTab t;
    clean_table(&t);
    std::copy(t.v, t.v + 256, lut);
    return PRL_OK;
}

// cols * rows of the page the three histograms were taken from: every channel's bins sum to it
static int luts_pixels(const uint32_t* hist, int* pixels)
{
    unsigned long long total[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) total[c] += hist[c * 256 + v];
    if (total[0] == 0) return PRL_ERR_EMPTY;
    if (total[1] != total[0] || total[2] != total[0] || total[0] > (unsigned long long)kStageMaxSide * kStageMaxSide) return PRL_ERR_BAD_ARG;
    *pixels = (int)total[0];
    return PRL_OK;
}

int prl_hip_simple_white_balance_luts(double k, const uint32_t hist[3 * 256], uint8_t luts[3 * 256])
{
    if (!hist || !luts) return PRL_ERR_BAD_ARG;
    int pixels;
    const int st = luts_pixels(hist, &pixels);
    if (st != PRL_OK) return st;
    swb_tables(k, hist, pixels, luts);
    return PRL_OK;
}

int prl_hip_gray_world_luts(double p_norm, int with_max, const uint32_t hist[3 * 256], uint8_t luts[3 * 256])
{
    if (!hist || !luts) return PRL_ERR_BAD_ARG;
    int pixels;
    const int st = luts_pixels(hist, &pixels);
    if (st != PRL_OK) return st;
    gw_tables(p_norm, with_max != 0, hist, pixels, luts);
    return PRL_OK;
}

}  // extern "C"
