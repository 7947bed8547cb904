// lines.hip — prl::removeLines (src/removeLines.cpp:30-76): strips ruled lines, table grids and form boxes from a page.
//
//   gray = channels == 3 ? the 14-bit BGR luma : the page;  inv = 255 - gray;  t = getThreshVal_Otsu_8u(inv);
//   bw = inv > t;  horizontal = dilate(erode(bw, RECT L x 1), RECT L x 1), L = width / 50;  vertical the same with
//   RECT 1 x Lv, Lv = height / 50;  out = bw && !horizontal && !vertical ? 0 : 255.
//   Both operators take the offsets -k/2 .. k-1-k/2 (the element is not reflected), taps outside the page are ignored.
//
// The mask holds one bit of information per pixel, so everything between the threshold and the output runs on bit planes:
// rows of 64-bit words, bit b of word k = pixel 64 k + b, rows padded to whole words (the pad bits are 0 in memory).
//   k_ln_hist<C>  256-bin histogram of gray per page (LDS-privatised; a wavefront whose pixels are all equal adds once).
//                 For 3 channels the luma is computed here and the gray page is written to scratch for the mask pass.
//   k_ln_otsu     getThreshVal_Otsu_8u's float64 scan (k_otsu of ppht.hip) over the REVERSED bins = the histogram of inv;
//                 leaves g = 255 - t per page on the device, so that bw = gray < g.
//   k_ln_mask     a wavefront ballot per 64 pixels -> one word of the bw plane.
//   k_ln_hopen    horizontal opening.  A workgroup keeps whole rows in LDS, loaded shifted by 2 (L/2) bits so that no step
//                 looks left.  A_s(p) = AND of the s bits from p is built by doubling (A_2s(p) = A_s(p) & A_s(p + s), a funnel
//                 shift across two words), then A_L = A_p & A_p(. + L - p) with p the largest power of two <= L: floor(log2 L)
//                 + 1 word operations per word.  Outside the page the erosion reads ones; its result is cleared outside the
//                 page (the dilation ignores those taps) and the same steps run again with OR.
//   k_ln_vopen    vertical opening: the same doubling over rows.  A workgroup holds a band of rows plus 2 (Lv - 1) halo rows of
//                 CW word columns in LDS, a lane per word; it reads the horizontal plane and writes bw & ~h & ~v.
//   k_ln_expand   a lane per 8 pixels: 0 where the bit is set, else 255.
// The hooks build routes the two openings through k_gm_span's byte path (gmorph.hip) with PRL_HIP_LINES_BYTES=1 where both
// elements are at most 255 long: the on-device executable specification.
#include "prl_internal.h"

#include <algorithm>
#include <cfloat>

namespace prl_hip {

namespace {

typedef unsigned long long u64;

constexpr int kLnMinSide = 50;        // below it width / 50 == 0: cv::getStructuringElement asserts
constexpr int kLnThreads = 256;
constexpr int kLnLdsWords = 3840;     // words per level buffer; two buffers = 60 KiB: two workgroups per CU
constexpr int kLnHWords = 2048;       // k_ln_hopen: words per level buffer aimed at (whole rows)
constexpr int kLnBytesMaxK = 255;     // the byte path's element limit (gmorph.hip)

__device__ __forceinline__ unsigned ln_gray14(unsigned b, unsigned g, unsigned r)
{
    return (b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14;
}

__device__ __forceinline__ u64 ln_ones_below(int n) { return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// bits sh .. sh + 63 of {hi : lo}
__device__ __forceinline__ u64 ln_funnel(u64 lo, u64 hi, int sh) { return sh ? (lo >> sh) | (hi << (64 - sh)) : lo; }

// ---- histogram and threshold ---------------------------------------------------------------------------------------------

// grid = (column groups, row groups, pages); a lane takes 4 pixels at a time.  C == 3: also writes the gray page.
template <int C>
__global__ __launch_bounds__(kLnThreads) void k_ln_hist(PageSet src, PageSetOut gray, int W, int H, unsigned* __restrict__ hist)
{
    __shared__ unsigned h[256];
    const int page = blockIdx.z, t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const uint8_t* base = src.page(page);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint8_t* row = base + (size_t)y * src.step;
        uint8_t* grow = C == 3 ? gray.page(page) + (size_t)y * gray.step : nullptr;
        // every lane of a wavefront makes the same number of trips (the ballot below needs them all)
        for (int xb = blockIdx.x * kLnThreads * 4; xb < W; xb += gridDim.x * kLnThreads * 4) {
            const int x = xb + t * 4;
            const int n = min(4, W - x);   // <= 0: no pixel
            unsigned g[4] = {0, 0, 0, 0};
            if (n > 0) {
                const uint8_t* s = row + (size_t)x * C;
                if (n == 4 && (((size_t)s) & 3) == 0) {
                    const unsigned* q = reinterpret_cast<const unsigned*>(s);
                    if (C == 3) {
                        const unsigned w0 = q[0], w1 = q[1], w2 = q[2];   // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
                        g[0] = ln_gray14(w0 & 0xff, (w0 >> 8) & 0xff, (w0 >> 16) & 0xff);
                        g[1] = ln_gray14(w0 >> 24, w1 & 0xff, (w1 >> 8) & 0xff);
                        g[2] = ln_gray14((w1 >> 16) & 0xff, w1 >> 24, w2 & 0xff);
                        g[3] = ln_gray14((w2 >> 8) & 0xff, (w2 >> 16) & 0xff, w2 >> 24);
                    } else {
                        const unsigned w0 = q[0];
                        g[0] = w0 & 0xff; g[1] = (w0 >> 8) & 0xff; g[2] = (w0 >> 16) & 0xff; g[3] = w0 >> 24;
                    }
                } else {
                    for (int i = 0; i < n; ++i) g[i] = C == 3 ? ln_gray14(s[i * 3], s[i * 3 + 1], s[i * 3 + 2]) : s[i];
                }
                if (C == 3) {
                    uint8_t* d = grow + x;
                    if (n == 4 && (((size_t)d) & 3) == 0) *reinterpret_cast<unsigned*>(d) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
                    else for (int i = 0; i < n; ++i) d[i] = (uint8_t)g[i];
                }
            }
            // a page is mostly paper: a wavefront that sees one value adds once instead of 64 times to one LDS word
            const bool flat = n == 4 && g[1] == g[0] && g[2] == g[0] && g[3] == g[0];
            const unsigned g0 = (unsigned)__shfl((int)g[0], 0);
            if (__all(flat && g[0] == g0)) {
                if ((t & 63) == 0) atomicAdd(&h[g0], 256u);
            } else if (flat) {
                atomicAdd(&h[g[0]], 4u);
            } else {
                for (int i = 0; i < n; ++i) atomicAdd(&h[g[i]], 1u);
            }
        }
    }
    __syncthreads();
    if (h[t]) atomicAdd(&hist[(size_t)page * 256 + t], h[t]);
}

// getThreshVal_Otsu_8u [upstream] on inv = 255 - gray: bin i of inv is bin 255 - i of gray.  One thread per page.
// gthr[page] = 255 - t: bw = inv > t = gray < gthr.
__global__ void k_ln_otsu(const unsigned* __restrict__ hist, int width, int height, int n_pages, int* __restrict__ gthr)
{
    const int page = blockIdx.x * blockDim.x + threadIdx.x;
    if (page >= n_pages) return;
    const unsigned* h = hist + (size_t)page * 256;
    double mu = 0;
    const double scale = 1. / ((double)width * height);
    for (int i = 0; i < 256; ++i) mu += i * (double)h[255 - i];
    mu *= scale;
    double mu1 = 0, q1 = 0, max_sigma = 0, max_val = 0;
    for (int i = 0; i < 256; ++i) {
        const double p_i = h[255 - i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1. - q1;
        if (fmin(q1, q2) < (double)FLT_EPSILON || fmax(q1, q2) > 1. - (double)FLT_EPSILON) continue;
        mu1 = (mu1 + i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) {
            max_sigma = sigma;
            max_val = i;
        }
    }
    gthr[page] = 255 - (int)max_val;
}

// ---- mask ----------------------------------------------------------------------------------------------------------------

// grid = (ceil(wp / 16), H, pages): a wavefront writes 4 words of a row.  Plane layout: word (page * H + y) * wp + k.
__global__ __launch_bounds__(kLnThreads) void k_ln_mask(PageSet gray, int W, int H, int wp, const int* __restrict__ gthr,
                                                        u64* __restrict__ bw)
{
    const int page = blockIdx.z, y = blockIdx.y, lane = threadIdx.x & 63;
    const int w0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    const int t = gthr[page];
    const uint8_t* row = gray.page(page) + (size_t)y * gray.step;
    u64* out = bw + ((size_t)page * H + y) * wp;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = (w0 + k) * 64 + lane;
        v[k] = x < W ? (int)row[x] : 255;   // 255 < t never holds (t <= 255): pad bits are 0
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u64 m = __ballot(v[k] < t);
        if (lane == 0 && w0 + k < wp) out[w0 + k] = m;
    }
}

// ---- horizontal opening ----------------------------------------------------------------------------------------------------

// grid = (ceil(H / nr), pages); dynamic LDS = 2 * nr * P words.  P = ceil((W + 2 (L - 1)) / 64) words per LDS row: LDS bit p of
// a row is pixel p - 2 (L / 2).
__global__ __launch_bounds__(kLnThreads) void k_ln_hopen(const u64* __restrict__ bw, u64* __restrict__ hout, int W, int H, int wp,
                                                         int L, int P, int nr)
{
    extern __shared__ u64 ln_lds[];
    u64* cur = ln_lds;
    u64* oth = ln_lds + nr * P;
    const int tid = threadIdx.x, page = blockIdx.y;
    const int y0 = blockIdx.x * nr;
    const int n = min(nr, H - y0) * P;
    const int a = L / 2;
    const u64 tail = ln_ones_below(W - 64 * (wp - 1));   // the page's bits of a row's last word
    const u64* src = bw + ((size_t)page * H + y0) * wp;

    for (int d = tid; d < n; d += kLnThreads) {
        const int r = d / P, c = d - r * P;
        const int s = 64 * c - 2 * a;
        const int q = s >> 6, sh = s & 63;   // floor and remainder, s may be negative
        const u64* row = src + (size_t)r * wp;
        u64 lo = ~0ull, hi = ~0ull;          // outside the page the erosion reads ones
        if (q >= 0 && q < wp) lo = q == wp - 1 ? row[q] | ~tail : row[q];
        if (sh && q + 1 >= 0 && q + 1 < wp) hi = q + 1 == wp - 1 ? row[q + 1] | ~tail : row[q + 1];
        cur[d] = ln_funnel(lo, hi, sh);
    }
    __syncthreads();

    for (int phase = 0; phase < 2; ++phase) {   // 0: erode (AND, ones outside), 1: dilate (OR, zeros outside)
        const u64 pad = phase ? 0ull : ~0ull;
        int s = 1;
        while (true) {
            int sft;
            if (2 * s <= L) sft = s;            // span s -> 2 s
            else if (L > s) sft = L - s;        // the overlapping last step: span s -> L
            else break;
            const int q = sft >> 6, sh = sft & 63;
            for (int d = tid; d < n; d += kLnThreads) {
                const int r = d / P, c = d - r * P;
                const int i = c + q;
                const u64 lo = i < P ? cur[d + q] : pad;
                const u64 hi = (sh && i + 1 < P) ? cur[d + q + 1] : pad;
                const u64 v = ln_funnel(lo, hi, sh);
                oth[d] = phase ? (cur[d] | v) : (cur[d] & v);
            }
            __syncthreads();
            u64* x = cur;
            cur = oth;
            oth = x;
            if (sft != s) break;
            s *= 2;
        }
        if (phase == 0) {   // LDS bit p now holds erode at pixel p - a: the dilation ignores what lies outside the page
            for (int d = tid; d < n; d += kLnThreads) {
                const int c = d % P;
                cur[d] &= ln_ones_below(a + W - 64 * c) & ~ln_ones_below(a - 64 * c);
            }
            __syncthreads();
        }
    }

    // LDS bit p holds the opening at pixel p
    u64* dst = hout + ((size_t)page * H + y0) * wp;
    for (int d = tid; d < n; d += kLnThreads) {
        const int r = d / P, c = d - r * P;
        if (c < wp) dst[(size_t)r * wp + c] = c == wp - 1 ? cur[d] & tail : cur[d];
    }
}

// ---- vertical opening and composition ------------------------------------------------------------------------------------

// grid = (ceil(wp / CW), ceil(H / TH), pages); dynamic LDS = 2 * (TH + 2 (Lv - 1)) * CW words.  LDS row r is page row
// y0 - 2 (Lv / 2) + r.  out = bw & ~h & ~open_v(bw).
__global__ __launch_bounds__(kLnThreads) void k_ln_vopen(const u64* __restrict__ bw, const u64* __restrict__ hpl, u64* __restrict__ out,
                                                         int H, int wp, int Lv, int CW, int TH)
{
    extern __shared__ u64 ln_lds[];
    const int tid = threadIdx.x, page = blockIdx.z;
    const int x0 = blockIdx.x * CW, y0 = blockIdx.y * TH;
    const int a = Lv / 2;
    const int n = (TH + 2 * (Lv - 1)) * CW;
    u64* cur = ln_lds;
    u64* oth = ln_lds + n;
    const size_t pbase = (size_t)page * H * wp;

    for (int d = tid; d < n; d += kLnThreads) {
        const int r = d / CW, col = x0 + d - r * CW;
        const int yy = y0 - 2 * a + r;
        cur[d] = (yy >= 0 && yy < H && col < wp) ? bw[pbase + (size_t)yy * wp + col] : ~0ull;
    }
    __syncthreads();

    for (int phase = 0; phase < 2; ++phase) {
        const u64 pad = phase ? 0ull : ~0ull;
        int s = 1;
        while (true) {
            int sft;
            if (2 * s <= Lv) sft = s;
            else if (Lv > s) sft = Lv - s;
            else break;
            const int off = sft * CW;
            for (int d = tid; d < n; d += kLnThreads) {
                const u64 v = d + off < n ? cur[d + off] : pad;
                oth[d] = phase ? (cur[d] | v) : (cur[d] & v);
            }
            __syncthreads();
            u64* x = cur;
            cur = oth;
            oth = x;
            if (sft != s) break;
            s *= 2;
        }
        if (phase == 0) {   // LDS row r now holds erode at page row y0 - a + r
            for (int d = tid; d < n; d += kLnThreads) {
                const int yy = y0 - a + d / CW;
                if (yy < 0 || yy >= H) cur[d] = 0ull;
            }
            __syncthreads();
        }
    }

    // LDS row r holds the opening at page row y0 + r
    for (int d = tid; d < TH * CW; d += kLnThreads) {
        const int r = d / CW, col = x0 + d - r * CW;
        const int y = y0 + r;
        if (y < H && col < wp) {
            const size_t idx = pbase + (size_t)y * wp + col;
            out[idx] = bw[idx] & ~hpl[idx] & ~cur[d];
        }
    }
}

// a lane expands one byte of the result plane: 8 pixels, 0 where the bit is set (ink that is no line), else 255
__global__ __launch_bounds__(kLnThreads) void k_ln_expand(const uint8_t* __restrict__ bits, size_t bits_step, PageSetOut dst, int W,
                                                          int H)
{
    const int page = blockIdx.z, y = blockIdx.y;
    const int b = blockIdx.x * kLnThreads + threadIdx.x, x = b * 8;
    if (x >= W) return;
    const uint32_t m = bits[((size_t)page * H + y) * bits_step + b];
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + x;
    const int n = min(8, W - x);
    if (n == 8 && ((size_t)d & 7) == 0) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (((m >> i) & 1u) ? 0u : 255u) << (8 * i);
            hi |= (((m >> (4 + i)) & 1u) ? 0u : 255u) << (8 * i);
        }
        *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
    } else {
        for (int i = 0; i < n; ++i) d[i] = (uint8_t)(((m >> i) & 1u) ? 0u : 255u);
    }
}

// ---- the byte path of the hooks build --------------------------------------------------------------------------------------

__global__ __launch_bounds__(kLnThreads) void k_ln_mask_bytes(PageSet gray, int W, const int* __restrict__ gthr, PageSetOut bw)
{
    const int page = blockIdx.z, y = blockIdx.y, x = blockIdx.x * kLnThreads + threadIdx.x;
    if (x >= W) return;
    bw.page(page)[(size_t)y * bw.step + x] = gray.page(page)[(size_t)y * gray.step + x] < gthr[page] ? 255 : 0;
}

__global__ __launch_bounds__(kLnThreads) void k_ln_compose_bytes(PageSet bw, PageSet h, PageSet v, int W, PageSetOut dst)
{
    const int page = blockIdx.z, y = blockIdx.y, x = blockIdx.x * kLnThreads + threadIdx.x;
    if (x >= W) return;
    const size_t o = (size_t)y * bw.step + x;
    const bool keep = bw.page(page)[o] && !h.page(page)[o] && !v.page(page)[o];
    dst.page(page)[(size_t)y * dst.step + x] = keep ? 0 : 255;
}

// ---- host ----------------------------------------------------------------------------------------------------------------

struct LnGeom {
    int W, H, C;
    int wp;            // words per bit row
    int L, Lv;
    int P, nr;         // k_ln_hopen: LDS words per row, rows per workgroup
    int CW, TH;        // k_ln_vopen: word columns and output rows per workgroup
};

LnGeom ln_geom(int W, int H, int C)
{
    LnGeom g{};
    g.W = W;
    g.H = H;
    g.C = C;
    g.wp = (W + 63) / 64;
    g.L = W / 50;
    g.Lv = H / 50;
    g.P = (W + 2 * (g.L - 1) + 63) / 64;
    g.nr = std::max(1, std::min(kLnHWords / g.P, H));
    // the widest tile whose halo (2 (Lv - 1) rows) is at most a third of its rows; one column where none is
    const int halo = 2 * (g.Lv - 1);
    for (g.CW = 32;; g.CW /= 2) {
        g.TH = kLnLdsWords / g.CW - halo;
        if (g.TH >= 2 * halo || g.CW == 1) break;
    }
    g.TH = std::min(g.TH, H);
    return g;
}

// the checks every entry makes, in the documented order (no device is touched); batch: the *_batch_device entry
int ln_checks(const PageArgs& a, int channels, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels != 1 && channels != 3) return PRL_ERR_BAD_CHANNELS;
    if (a.width < kLnMinSide || a.height < kLnMinSide) {
        set_error_detail("removeLines: width / 50 or height / 50 is 0 (ksize.width > 0 && ksize.height > 0)");
        return PRL_ERR_BAD_ARG;
    }
    if ((st = pages_rows_ok(a, channels, 1, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    // in place: 1-channel pages at the same strides (every source pixel is read before the first one is written)
    return batch ? pages_overlap_ok(a, channels, 1, true) : PRL_OK;
}

size_t ln_scratch_per_page(const LnGeom& g, bool bytes)
{
    const size_t gray = g.C == 3 ? r256((size_t)g.W * g.H) : 0;
    if (bytes) return gray + 4 * r256((size_t)g.W * g.H);
    return gray + 3 * r256((size_t)g.wp * 8 * g.H);
}

// one chunk of pages
int ln_run(const LnGeom& g, bool bytes, const PageSet& src, const PageSetOut& dst, int n, uint8_t* scratch, unsigned* hist, int* gthr,
           hipStream_t stream)
{
    const int W = g.W, H = g.H;
    const size_t gray_page = r256((size_t)W * H);
    PageSet gray = src;
    uint8_t* p = scratch;
    PageSetOut gout{};
    if (g.C == 3) {
        gout = page_set_out(p, gray_page, (size_t)W);
        gray = as_source(gout);
        p += gray_page * (size_t)n;
    }
    PRL_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(unsigned), stream));
    {
        const dim3 grid((unsigned)std::min(8, (W + kLnThreads * 4 - 1) / (kLnThreads * 4)), (unsigned)std::min(H, 64), (unsigned)n);
        if (g.C == 3) hipLaunchKernelGGL(k_ln_hist<3>, grid, dim3(kLnThreads), 0, stream, src, gout, W, H, hist);
        else hipLaunchKernelGGL(k_ln_hist<1>, grid, dim3(kLnThreads), 0, stream, src, gout, W, H, hist);
        hipLaunchKernelGGL(k_ln_otsu, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, hist, W, H, n, gthr);
        PRL_HIP_CHECK(hipGetLastError());
    }
    if (bytes) {
        const size_t plane = gray_page * (size_t)n;
        const PageSetOut bw = page_set_out(p, gray_page, (size_t)W), hb = page_set_out(p + plane, gray_page, (size_t)W),
                         vb = page_set_out(p + 2 * plane, gray_page, (size_t)W);
        uint8_t* tmp = p + 3 * plane;
        const dim3 grid((unsigned)((W + kLnThreads - 1) / kLnThreads), (unsigned)H, (unsigned)n);
        hipLaunchKernelGGL(k_ln_mask_bytes, grid, dim3(kLnThreads), 0, stream, gray, W, gthr, bw);
        PRL_HIP_CHECK(hipGetLastError());
        int st = gmorph_open_rect_run(g.L, 1, W, H, as_source(bw), hb, n, tmp, stream);
        if (st != PRL_OK) return st;
        st = gmorph_open_rect_run(1, g.Lv, W, H, as_source(bw), vb, n, tmp, stream);
        if (st != PRL_OK) return st;
        hipLaunchKernelGGL(k_ln_compose_bytes, grid, dim3(kLnThreads), 0, stream, as_source(bw), as_source(hb), as_source(vb), W, dst);
        PRL_HIP_CHECK(hipGetLastError());
        return PRL_OK;
    }
    const size_t plane = r256((size_t)g.wp * 8 * H) * (size_t)n;   // (pages are packed: only the chunk's end is rounded)
    u64* bw = reinterpret_cast<u64*>(p);
    u64* hp = reinterpret_cast<u64*>(p + plane);
    u64* rp = reinterpret_cast<u64*>(p + 2 * plane);
    hipLaunchKernelGGL(k_ln_mask, dim3((unsigned)((g.wp + 15) / 16), (unsigned)H, (unsigned)n), dim3(kLnThreads), 0, stream, gray, W, H,
                       g.wp, gthr, bw);
    hipLaunchKernelGGL(k_ln_hopen, dim3((unsigned)((H + g.nr - 1) / g.nr), (unsigned)n), dim3(kLnThreads),
                       (size_t)2 * g.nr * g.P * sizeof(u64), stream, bw, hp, W, H, g.wp, g.L, g.P, g.nr);
    hipLaunchKernelGGL(k_ln_vopen, dim3((unsigned)((g.wp + g.CW - 1) / g.CW), (unsigned)((H + g.TH - 1) / g.TH), (unsigned)n),
                       dim3(kLnThreads), (size_t)2 * (g.TH + 2 * (g.Lv - 1)) * g.CW * sizeof(u64), stream, bw, hp, rp, H, g.wp, g.Lv,
                       g.CW, g.TH);
    hipLaunchKernelGGL(k_ln_expand, dim3((unsigned)((g.wp * 8 + kLnThreads - 1) / kLnThreads), (unsigned)H, (unsigned)n),
                       dim3(kLnThreads), 0, stream, reinterpret_cast<const uint8_t*>(rp), (size_t)g.wp * 8, dst, W, H);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

int ln_batch_device(const PageArgs& a, int channels, void* stream)
{
    int st = ln_checks(a, channels, true);
    if (st != PRL_OK) return st;
    if (a.n_pages == 0) return PRL_OK;
    const LnGeom g = ln_geom(a.width, a.height, channels);
    const bool bytes = env_knobs().lines_bytes && g.L <= kLnBytesMaxK && g.Lv <= kLnBytesMaxK;
    const size_t per_page = ln_scratch_per_page(g, bytes);
    // pages per launch: grid.z, and at most 4 GiB of scratch (one page at least)
    const int chunk = stage_chunk(a.n_pages, per_page);
    WorkScope w;   // `small`: [bins of a chunk | Otsu thresholds of a chunk]
    st = w.open(stream, per_page * (size_t)chunk, (size_t)chunk * (256 * sizeof(unsigned) + sizeof(int)), 0);
    if (st != PRL_OK) return st;
    unsigned* hist = w.small<unsigned>();
    int* gthr = reinterpret_cast<int*>(hist + (size_t)chunk * 256);
    for (int first = 0; first < a.n_pages; first += chunk) {
        st = ln_run(g, bytes, src_pages(a, first), dst_pages(a, first), std::min(chunk, a.n_pages - first), w.scratch(), hist, gthr,
                    w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_remove_lines_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                      int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return ln_batch_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           stream);
}

int prl_hip_remove_lines_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = ln_checks(a, channels, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, 1, width, height,
                            [&](const PageArgs& page, hipStream_t s) { return ln_batch_device(page, channels, s); });
}

}  // extern "C"
