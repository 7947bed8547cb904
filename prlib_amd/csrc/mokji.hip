// mokji.hip — prl::binarizeMokji (src/binarizations/binarizeMokji.cpp:35-94; Mokji & Abu-Bakar 2007): one threshold per page from
// the co-occurrence matrix of the page and its square dilation.  Write E for maxEdgeWidth and M for minEdgeMagnitude.
//
//   gray = channels == 1 ? the page : the 14-bit BGR luma;  dil = dilate(gray, RECT (2E + 1)^2) (gmorph.hip, taps outside the page
//   ignored);  matrix[dil][gray] += 1 over the interior [E, rows - E) x [E, cols - E), from zeros;  nom = sum (m + n) matrix[n][m],
//   den = sum matrix[n][m] over n - m >= M;  t = (int)(0.5 * nom / den + 0.5) = (nom + den) / (2 den);  out = gray > t ? 255 : 0.
//   den == 0 (empty interior, no pair, M >= 256): the reference converts a NaN to int and thresholds at INT_MIN on x86 - the page
//   comes out all 255; t is reported as -1.
//
//   k_mokji_gray<C>    3 / 4 channels -> the gray plane in scratch, a lane per 4 pixels (rows padded to whole dwords).
//   k_mokji_cooc       the 2-D histogram.  A workgroup of 1024 lanes keeps the triangle b >= a of the matrix - 32 896 uint32 bins,
//                      131 584 bytes - in LDS (dynamic, one workgroup per CU), walks its share of the interior's rows a lane per 4
//                      pixels, and adds its non-zero bins to the page's matrix with global atomics at the end.  A pair with
//                      b - a < min_diff drops out before any atomic; a wavefront whose 256 pairs are one pair adds once.  Pairs with
//                      b < a (counted only for min_diff == 0, never by the binarizer, where b = dil >= gray = a) go straight to the
//                      global matrix.  Integer sums: the result does not depend on the order.
//   k_mokji_threshold  a workgroup per page: nom and den as 64-bit integers, lane m down column m (coalesced rows), then
//                      mokji_threshold_of - the function prl_hip_mokji_threshold runs on the host.  t stays on the device.
//   k_mokji_apply      dst = gray > t[page] ? 255 : 0, 8 pixels per lane; t = -1 gives all 255.
#include "prl_internal.h"

#include <algorithm>

namespace prl_hip {

namespace {

constexpr int kMkMaxE = 127;                        // the dilation's element is 2E + 1 <= 255 wide (gmorph.hip)
constexpr int kMkThreads = 256;
constexpr int kMkCoocThreads = 1024;
constexpr int kMkTriBins = 256 * 257 / 2;           // bins (b, a) with b >= a; bin b (b + 1) / 2 + a
constexpr size_t kMkTriBytes = (size_t)kMkTriBins * sizeof(unsigned);
constexpr size_t kMkCoocBytes = (size_t)256 * 256 * sizeof(unsigned);
constexpr int kMkPx = 8;                            // pixels per lane of k_mokji_apply

// ---- the arithmetic, shared by prl_hip_mokji_threshold and k_mokji_threshold ------------------------------------------------

// binarizeMokji.cpp:92.  nom <= 510 * 2^30 < 2^53, so 0.5 * nom is exact and the double quotient lies at least 1 / (2 den) >= 2^-31
// from any k - 0.5 it does not equal, with an ulp of at most 2^-45: the truncation equals the integer quotient below
// (tests/test_mokji_cpu.py holds the two equal).  den == 0: -1, the page comes out all 255.
__host__ __device__ inline int mokji_threshold_of(unsigned long long nom, unsigned long long den)
{
    if (den == 0) return -1;
    return (int)((nom + den) / (2 * den));
}

__device__ __forceinline__ unsigned mk_gray14(unsigned b, unsigned g, unsigned r)
{
    return (b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

// one pair (a, b) seen `weight` times: the triangle in LDS for b >= a, the page's matrix itself below the diagonal (min_diff == 0 only)
__device__ __forceinline__ void mk_count(unsigned* tri, unsigned* out, int pa, int pb, int min_diff, unsigned weight)
{
    if (min_diff > 0 && pb - pa < min_diff) return;   // 0: every pair, those below the diagonal included
    if (pb >= pa) atomicAdd(&tri[pb * (pb + 1) / 2 + pa], weight);
    else atomicAdd(&out[pb * 256 + pa], weight);
}

// grid = (ceil(quads * H / 256), pages), quads = ceil(W / 4) numbered row after row.  gray rows are whole dwords (gray.step % 4 == 0,
// 256-byte aligned pages): the bytes past W in a row's last dword are written as 0 and never read.
template <int C>
__global__ __launch_bounds__(kMkThreads) void k_mokji_gray(PageSet src, PageSetOut gray, int W, int H)
{
    const int page = blockIdx.y;
    const unsigned quads = (unsigned)(W + 3) / 4u;
    const unsigned qi = blockIdx.x * (unsigned)kMkThreads + threadIdx.x;
    const int y = (int)(qi / quads);
    if (y >= H) return;
    const int x = (int)(qi - (unsigned)y * quads) * 4;
    const int n = min(4, W - x);
    const uint8_t* s = src.page(page) + (size_t)y * src.step + (size_t)x * C;
    unsigned g[4] = {0, 0, 0, 0};
    if (n == 4) {
        unsigned w[C];   // C == 3: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3;  C == 4: a pixel per dword
#pragma unroll
        for (int i = 0; i < C; ++i) __builtin_memcpy(&w[i], s + 4 * i, 4);   // (any alignment)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned ch[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = i * C + c;
                ch[c] = (w[b / 4] >> (8 * (b % 4))) & 0xffu;
            }
            g[i] = mk_gray14(ch[0], ch[1], ch[2]);
        }
    } else {
        for (int i = 0; i < n; ++i) g[i] = mk_gray14(s[i * C], s[i * C + 1], s[i * C + 2]);
    }
    *reinterpret_cast<unsigned*>(gray.page(page) + (size_t)y * gray.step + x) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
}

// grid = (workgroups per page, pages), 1024 lanes, dynamic LDS = kMkTriBytes.  The interior is [bo, H - bo) x [bo, W - bo), not
// empty; workgroup g takes its rows g, g + gridDim.x, ... .  cooc: [page][256][256], zeroed before the launch.
__global__ __launch_bounds__(kMkCoocThreads) void k_mokji_cooc(PageSet a, PageSet b, int W, int H, int bo, int min_diff,
                                                               unsigned* __restrict__ cooc)
{
    extern __shared__ unsigned mk_tri[];
    const int page = blockIdx.y, t = threadIdx.x;
    for (int i = t; i < kMkTriBins; i += kMkCoocThreads) mk_tri[i] = 0;
    __syncthreads();
    const int iw = W - 2 * bo, ih = H - 2 * bo;
    const int quads = (iw + 3) / 4;
    unsigned* out = cooc + (size_t)page * 256 * 256;
    const uint8_t* ap = a.page(page);
    const uint8_t* bp = b.page(page);
    for (int r = blockIdx.x; r < ih; r += gridDim.x) {
        const uint8_t* arow = ap + (size_t)(bo + r) * a.step + bo;
        const uint8_t* brow = bp + (size_t)(bo + r) * b.step + bo;
        // every lane of a wavefront makes the same number of trips (the vote below needs them all)
        for (int q0 = 0; q0 < quads; q0 += kMkCoocThreads) {
            const int x = (q0 + t) * 4;
            const int n = min(4, iw - x);   // <= 0: no pixel
            unsigned va[4] = {0, 0, 0, 0}, vb[4] = {0, 0, 0, 0};
            if (n == 4) {
                unsigned wa, wb;
                __builtin_memcpy(&wa, arow + x, 4);   // (any alignment)
                __builtin_memcpy(&wb, brow + x, 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    va[i] = (wa >> (8 * i)) & 0xffu;
                    vb[i] = (wb >> (8 * i)) & 0xffu;
                }
            } else {
                for (int i = 0; i < n; ++i) {
                    va[i] = arow[x + i];
                    vb[i] = brow[x + i];
                }
            }
            unsigned key[4];   // b * 256 + a
#pragma unroll
            for (int i = 0; i < 4; ++i) key[i] = vb[i] * 256u + va[i];
            // a page is mostly flat paper: a wavefront that sees one pair adds once instead of 64 times to one LDS word
            const bool flat = n == 4 && key[1] == key[0] && key[2] == key[0] && key[3] == key[0];
            const unsigned k0 = (unsigned)__shfl((int)key[0], 0);
            if (__all(flat && key[0] == k0)) {
                if ((t & 63) == 0) mk_count(mk_tri, out, (int)va[0], (int)vb[0], min_diff, 256u);
            } else if (flat) {
                mk_count(mk_tri, out, (int)va[0], (int)vb[0], min_diff, 4u);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) mk_count(mk_tri, out, (int)va[i], (int)vb[i], min_diff, 1u);
            }
        }
    }
    __syncthreads();
    // row pb of the triangle to the wavefront pb % 16, a lane per column
    const int wave = t >> 6, lane = t & 63;
    for (int pb = wave; pb < 256; pb += kMkCoocThreads / 64)
        for (int pa = lane; pa <= pb; pa += 64) {
            const unsigned v = mk_tri[pb * (pb + 1) / 2 + pa];
            if (v) atomicAdd(&out[pb * 256 + pa], v);
        }
}

// grid = pages, 256 lanes.  valid == 0 (an empty interior: no matrix was made): -1.
__global__ __launch_bounds__(kMkThreads) void k_mokji_threshold(const unsigned* __restrict__ cooc, int M, int valid, int* __restrict__ thr)
{
    __shared__ unsigned long long s_nom[kMkThreads], s_den[kMkThreads];
    const int page = blockIdx.x, m = threadIdx.x;
    unsigned long long nom = 0, den = 0;
    if (valid) {
        const unsigned* c = cooc + (size_t)page * 256 * 256;
        for (int n = m + M; n < 256; ++n) {   // M >= 1; M >= 256: no pair
            const unsigned long long v = c[n * 256 + m];
            nom += (unsigned long long)(m + n) * v;
            den += v;
        }
    }
    s_nom[m] = nom;
    s_den[m] = den;
    __syncthreads();
    for (int s = kMkThreads / 2; s > 0; s >>= 1) {
        if (m < s) {
            s_nom[m] += s_nom[m + s];
            s_den[m] += s_den[m + s];
        }
        __syncthreads();
    }
    if (m == 0) thr[page] = mokji_threshold_of(s_nom[0], s_den[0]);
}

// grid = (ceil(groups * H / 256), pages), groups of 8 pixels numbered row after row.  In place (gray == dst): a lane reads its
// pixels before it writes them.
__global__ __launch_bounds__(kMkThreads) void k_mokji_apply(PageSet gray, PageSetOut dst, int W, int H, const int* __restrict__ thr)
{
    const int page = blockIdx.y;
    const int t = thr[page];
    const unsigned groups = (unsigned)(W + kMkPx - 1) / (unsigned)kMkPx;
    const unsigned gi = blockIdx.x * (unsigned)kMkThreads + threadIdx.x;
    const int y = (int)(gi / groups);
    if (y >= H) return;
    const int x0 = (int)(gi - (unsigned)y * groups) * kMkPx;
    const int n = min(kMkPx, W - x0);
    const uint8_t* s = gray.page(page) + (size_t)y * gray.step + x0;
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + x0;
    if (n == kMkPx) {
        unsigned in[2], out[2] = {0, 0};
        __builtin_memcpy(&in[0], s, 4);   // (any alignment)
        __builtin_memcpy(&in[1], s + 4, 4);
#pragma unroll
        for (int i = 0; i < kMkPx; ++i) {
            const int v = (int)((in[i / 4] >> (8 * (i % 4))) & 0xffu);
            out[i / 4] |= (v > t ? 255u : 0u) << (8 * (i % 4));
        }
        __builtin_memcpy(d, &out[0], 4);
        __builtin_memcpy(d + 4, &out[1], 4);
    } else {
        for (int i = 0; i < n; ++i) d[i] = (int)s[i] > t ? 255 : 0;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

bool mk_interior_empty(int width, int height, long long border) { return width <= 2 * border || height <= 2 * border; }

// the checks of the binarizer and of the thresholds entry (which has no destination: with_mask == false), in the documented order
// (no device is touched); batch: a *_batch_device entry
int mk_checks(const PageArgs& a, int channels, int E, int M, bool with_mask, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (E < 1 || M < 1) return PRL_ERR_BAD_ARG;
    if (E > kMkMaxE && !mk_interior_empty(a.width, a.height, E)) {
        set_error_detail("binarizeMokji: maxEdgeWidth above 127 (a dilation element above 255) on a page with an interior");
        return PRL_ERR_BAD_ARG;
    }
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, with_mask ? 1 : 0, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    // in place: 1-channel pages at the same strides (every statistic is taken before the first pixel is written)
    return batch ? pages_overlap_ok(a, channels, with_mask ? 1 : 0, true) : PRL_OK;
}

// workgroups per page of k_mokji_cooc: about two per CU over the call, at least 8 interior rows each, at most 64
int mk_cooc_blocks(int n_pages, int interior_rows, int cu_count)
{
    const int want = (2 * std::max(cu_count, 1) + n_pages - 1) / n_pages;
    return std::max(1, std::min(std::min(want, 64), (interior_rows + 7) / 8));
}

// a, b: 1-channel planes; cooc is overwritten
int mk_cooc_launch(const PageSet& a, const PageSet& b, int n, int W, int H, int border, int min_diff, unsigned* cooc, int cu_count,
                   hipStream_t stream)
{
    PRL_HIP_CHECK(hipMemsetAsync(cooc, 0, (size_t)n * kMkCoocBytes, stream));
    if (mk_interior_empty(W, H, border) || min_diff > 255) return PRL_OK;
    PRL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_mokji_cooc), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kMkTriBytes));
    const dim3 grid((unsigned)mk_cooc_blocks(n, H - 2 * border, cu_count), (unsigned)n);
    hipLaunchKernelGGL(k_mokji_cooc, grid, dim3(kMkCoocThreads), kMkTriBytes, stream, a, b, W, H, border, min_diff, cooc);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

struct MkGeom {
    int W, H, C, E, M;
    bool empty;          // no interior: no dilation, no matrix, t = -1
    size_t gstep;        // row bytes of the gray and dilated planes (whole dwords)
    size_t plane;        // bytes of such a plane per page
};

MkGeom mk_geom(int W, int H, int C, int E, int M)
{
    MkGeom g{};
    g.W = W;
    g.H = H;
    g.C = C;
    g.E = E;
    g.M = std::min(M, 256);
    g.empty = mk_interior_empty(W, H, E);
    g.gstep = ((size_t)W + 3) / 4 * 4;
    g.plane = r256(g.gstep * (size_t)H);
    return g;
}

// per page: [gray (3 / 4 channels)] [dil] [the dilation's intermediate plane] [matrix]; masks alone need the gray plane even
// where the interior is empty
size_t mk_scratch_per_page(const MkGeom& g, bool with_mask)
{
    size_t bytes = 0;
    if (g.C != 1 && (with_mask || !g.empty)) bytes += g.plane;
    if (!g.empty) bytes += g.plane + r256((size_t)g.W * g.H) + kMkCoocBytes;
    return bytes;
}

// one chunk of pages: thresholds into thr; the mask into dst where dst != nullptr
int mk_run(const MkGeom& g, const PageSet& src, const PageSetOut* dst, int n, uint8_t* scratch, int* thr, int cu_count, hipStream_t stream)
{
    const int W = g.W, H = g.H;
    PageSet gray = src;
    uint8_t* p = scratch;
    if (g.C != 1 && (dst || !g.empty)) {
        const PageSetOut gout = page_set_out(p, g.plane, g.gstep);
        p += g.plane * (size_t)n;
        const size_t quads = (size_t)((W + 3) / 4) * H;
        const dim3 grid((unsigned)((quads + kMkThreads - 1) / kMkThreads), (unsigned)n);
        if (g.C == 3) hipLaunchKernelGGL(k_mokji_gray<3>, grid, dim3(kMkThreads), 0, stream, src, gout, W, H);
        else hipLaunchKernelGGL(k_mokji_gray<4>, grid, dim3(kMkThreads), 0, stream, src, gout, W, H);
        PRL_HIP_CHECK(hipGetLastError());
        gray = as_source(gout);
    }
    unsigned* cooc = nullptr;
    if (!g.empty) {
        const PageSetOut dil = page_set_out(p, g.plane, g.gstep);
        p += g.plane * (size_t)n;
        uint8_t* tmp = p;
        p += r256((size_t)W * H) * (size_t)n;
        cooc = reinterpret_cast<unsigned*>(p);
        int st = gmorph_dilate_rect_run(2 * g.E + 1, W, H, gray, dil, n, tmp, stream);
        if (st != PRL_OK) return st;
        st = mk_cooc_launch(gray, as_source(dil), n, W, H, g.E, g.M, cooc, cu_count, stream);
        if (st != PRL_OK) return st;
    }
    hipLaunchKernelGGL(k_mokji_threshold, dim3((unsigned)n), dim3(kMkThreads), 0, stream, cooc, g.M, g.empty ? 0 : 1, thr);
    PRL_HIP_CHECK(hipGetLastError());
    if (dst) {
        const size_t groups = (size_t)((W + kMkPx - 1) / kMkPx) * H;
        const dim3 grid((unsigned)((groups + kMkThreads - 1) / kMkThreads), (unsigned)n);
        hipLaunchKernelGGL(k_mokji_apply, grid, dim3(kMkThreads), 0, stream, gray, *dst, W, H, thr);
        PRL_HIP_CHECK(hipGetLastError());
    }
    return PRL_OK;
}

// with_mask: the binarizer (thresholds in the device's small block); else d_thr receives the thresholds
int mk_batch_device(const PageArgs& a, int channels, int E, int M, bool with_mask, int32_t* d_thr, void* stream)
{
    int st = mk_checks(a, channels, E, M, with_mask, true);
    if (st != PRL_OK) return st;
    if (!with_mask && !d_thr) return PRL_ERR_BAD_ARG;
    if (a.n_pages == 0) return PRL_OK;
    const MkGeom g = mk_geom(a.width, a.height, channels, E, M);
    const size_t per_page = mk_scratch_per_page(g, with_mask);
    // pages per launch: grid.y, and at most 4 GiB of scratch (one page at least)
    const int chunk = stage_chunk(a.n_pages, per_page);
    WorkScope w;
    st = w.open(stream, per_page * (size_t)chunk, with_mask ? (size_t)chunk * sizeof(int) : 0, 0);
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        const PageSetOut d = dst_pages(a, first);
        st = mk_run(g, src_pages(a, first), with_mask ? &d : nullptr, std::min(chunk, a.n_pages - first), w.scratch(),
                    with_mask ? w.small<int>() : d_thr + first, w.ctx->cu_count, w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_binarize_mokji_batch_device(int n_pages, int channels, int max_edge_width, int min_edge_magnitude, const uint8_t* d_src,
                                        size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                        size_t dst_page_stride, size_t dst_step, void* stream)
{
    return mk_batch_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           max_edge_width, min_edge_magnitude, true, nullptr, stream);
}

int prl_hip_binarize_mokji_host(int channels, int max_edge_width, int min_edge_magnitude, const uint8_t* src, size_t src_step, int width,
                                int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = mk_checks(a, channels, max_edge_width, min_edge_magnitude, true, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, 1, width, height, [&](const PageArgs& page, hipStream_t s) {
        return mk_batch_device(page, channels, max_edge_width, min_edge_magnitude, true, nullptr, s);
    });
}

int prl_hip_mokji_thresholds_batch_device(int n_pages, int channels, int max_edge_width, int min_edge_magnitude, const uint8_t* d_src,
                                          size_t src_page_stride, size_t src_step, int width, int height, int32_t* d_thresholds,
                                          void* stream)
{
    return mk_batch_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, nullptr, 0, 0}, channels, max_edge_width,
                           min_edge_magnitude, false, d_thresholds, stream);
}

int prl_hip_cooccurrence_batch_device(int n_pages, int border, int min_diff, const uint8_t* d_a, size_t a_page_stride, size_t a_step,
                                      const uint8_t* d_b, size_t b_page_stride, size_t b_step, int width, int height, uint32_t* d_cooc,
                                      void* stream)
{
    const PageArgs a{n_pages, d_a, a_page_stride, a_step, width, height, nullptr, 0, 0};
    const PageArgs b{n_pages, d_b, b_page_stride, b_step, width, height, nullptr, 0, 0};
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (border < 0 || min_diff < 0 || min_diff > 256) return PRL_ERR_BAD_ARG;
    if (pages_rows_ok(a, 1, 0, true) != PRL_OK || pages_rows_ok(b, 1, 0, true) != PRL_OK || !d_cooc) return PRL_ERR_BAD_ARG;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    if (n_pages == 0) return PRL_OK;
    int dev;   // no workspace and no lock: the device check alone
    st = current_device(&dev);
    if (st != PRL_OK) return st;
    const int cu_count = device_ctx(dev)->cu_count;
    const int chunk = stage_chunk(n_pages, 0);
    for (int first = 0; first < n_pages; first += chunk) {
        st = mk_cooc_launch(src_pages(a, first), src_pages(b, first), std::min(chunk, n_pages - first), width, height, border, min_diff,
                            d_cooc + (size_t)first * 256 * 256, cu_count, static_cast<hipStream_t>(stream));
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int prl_hip_mokji_threshold(const uint32_t cooc[256 * 256], int min_edge_magnitude, int* threshold)
{
    if (!cooc || !threshold || min_edge_magnitude < 1) return PRL_ERR_BAD_ARG;
    const int M = std::min(min_edge_magnitude, 256);   // 256 and above: no pair
    unsigned long long nom = 0, den = 0;
    for (int m = 0; m + M < 256; ++m)
        for (int n = m + M; n < 256; ++n) {
            const unsigned long long v = cooc[n * 256 + m];
            nom += (unsigned long long)(m + n) * v;
            den += v;
        }
    *threshold = mokji_threshold_of(nom, den);
    return PRL_OK;
}

}  // extern "C"
