// edgedet.hip — CannyEdgeDetection (src/imageLibCommon.cpp:244-324), the edge stage of prl::binarizeLocalOtsu, binarizeCOCOCLUST
// and binarizeFBCITB, on batched pages of 1 to 4 interleaved channels (the rules: include/prl_hip.h, "CannyEdgeDetection").  Per
// channel: the 8-bit cv::GaussianBlur (blur8.hip), the Otsu value t of the blurred plane (ppht.hip), cv::Canny(lower, upper) with
// upper = upperCoeff * t and lower = lowerCoeff * upper (canny.hip), the 3 x 3 closing or opening (morph.hip); the channels' maps
// are OR-ed.  The channels of a chunk become n * C gray planes, so every stage runs once per chunk.  t never leaves the device:
// the host uploads the 256 (low, high) pairs of every possible t and the classes kernel looks its page's pair up.
#include <algorithm>
#include <cmath>

#include "gauss8.h"
#include "prl_internal.h"

namespace prl_hip {

namespace {

struct LutArg {
    int v[512];
};

__global__ __launch_bounds__(256) void k_store_lut(LutArg lut, int* __restrict__ d_lut)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 512) d_lut[i] = lut.v[i];
}

// plane page * C + ch = channel ch of page `page`; grid = (ceil(W / 256), H, pages)
template <int C>
__global__ __launch_bounds__(256) void k_split(PageSet src, int W, uint8_t* __restrict__ planes, size_t plane_bytes)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, page = blockIdx.z;
    if (x >= W) return;
    const uint8_t* s = src.page(page) + (size_t)y * src.step + (size_t)x * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) planes[((size_t)page * C + ch) * plane_bytes + (size_t)y * W + x] = s[ch];
}

// dst = plane 0 | ... | plane C - 1 of every page
__global__ __launch_bounds__(256) void k_or_planes(const uint8_t* __restrict__ planes, size_t plane_bytes, int C, int W, PageSetOut dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, page = blockIdx.z;
    if (x >= W) return;
    unsigned v = 0;
    for (int ch = 0; ch < C; ++ch) v |= planes[((size_t)page * C + ch) * plane_bytes + (size_t)y * W + x];
    dst.page(page)[(size_t)y * dst.step + x] = (uint8_t)v;
}

size_t tmp_step(int W) { return ((size_t)W + 63) / 64 * 64; }

// scratch of one page beside cv::Canny's own: [blurred planes | edge maps | the blurred interleaved page | the morphology's plane]
size_t per_page_bytes(const CedSpec& sp, int W, int H, int C)
{
    const size_t plane = r256((size_t)W * H);
    return 2 * C * plane + (C > 1 ? r256((size_t)W * C * H) : 0) + (std::abs(sp.iterations) > kMorphMaxFusedRadius ? C * r256(tmp_step(W) * H) : 0);
}

}  // namespace

// The reference's checks in its order (imageLibCommon.cpp:253-272), then cv::GaussianBlur's own on the size: 0, or which one failed
int ced_spec_check(const CedSpec& sp)
{
    if (sp.size < 3) return 1;
    if (!(sp.upper_coeff >= 0 && sp.upper_coeff <= 1)) return 2;
    if (!(sp.lower_coeff >= 0 && sp.lower_coeff <= 1)) return 3;
    if (sp.lower_coeff > sp.upper_coeff) return 4;
    if ((sp.size & 1) == 0) return 5;
    return 0;
}

int ced_pages_per_chunk(const CedSpec& sp, int n_pages, int W, int H, int C, size_t extra_per_page)
{
    const size_t per_plane = (per_page_bytes(sp, W, H, C) + extra_per_page + C - 1) / C;
    long long planes = (long long)n_pages * C;
    const int chunk_planes = canny_pages_per_chunk((int)std::min<long long>(planes, 0x7fffffff), W, H, per_plane);
    return std::max(1, std::min(n_pages, chunk_planes / C));
}

size_t ced_work_bytes(const CedSpec& sp, int n, int W, int H, int C) { return per_page_bytes(sp, W, H, C) * (size_t)n + r256(canny_work_bytes(n * C, W, H)); }
size_t ced_small_bytes(int n, int C) { return r256((size_t)n * C * 256 * sizeof(unsigned)) + r256((size_t)n * C * sizeof(int)) + 2048; }
size_t ced_pinned_bytes(int n, int C) { return canny_pinned_bytes(n * C); }

// n pages (a chunk) into 0 / 255 maps; synchronises the stream (cv::Canny's hysteresis does); caller holds ctx->mu
int ced_run(const CedSpec& sp, const PageSet& src, const PageSetOut& dst, int n, int W, int H, int C, uint8_t* work, uint8_t* small,
            unsigned* h_flags, hipStream_t hs)
{
    const size_t plane = r256((size_t)W * H), planes_n = (size_t)n * C;
    uint8_t* P = work;                        // blurred planes; later the morphology's result
    uint8_t* M = P + planes_n * plane;        // edge maps
    uint8_t* A = M + planes_n * plane;        // the blurred interleaved pages (C > 1)
    const size_t a_bytes = C > 1 ? r256((size_t)W * C * H) : 0;
    uint8_t* T = A + a_bytes * (size_t)n;     // the morphology's second plane (iterations above the fused kernels')
    const bool large = std::abs(sp.iterations) > kMorphMaxFusedRadius;
    uint8_t* canny_work = T + (large ? planes_n * r256(tmp_step(W) * H) : 0);
    unsigned* d_hist = reinterpret_cast<unsigned*>(small);
    int* d_thr = reinterpret_cast<int*>(small + r256(planes_n * 256 * sizeof(unsigned)));
    int* d_lut = reinterpret_cast<int*>(reinterpret_cast<uint8_t*>(d_thr) + r256(planes_n * sizeof(int)));

    // 1. blur with (size, size) and sigma 0
    uint16_t wk[kGaussMaxSide];
    gauss8_kernel(sp.size, 0.0, wk);
    PageArgs ba{n, src.base, src.page_stride, src.step, W, H, C > 1 ? A : P, C > 1 ? a_bytes : plane, (size_t)W * C};
    int st = sep_filter_u8_batch(wk, sp.size, wk, sp.size, ba, C, hs);
    if (st != PRL_OK) return st;
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)n);
    if (C > 1) {
        const PageSet as = page_set(A, a_bytes, (size_t)W * C);
        if (C == 2) hipLaunchKernelGGL(k_split<2>, grid, dim3(256), 0, hs, as, W, P, plane);
        else if (C == 3) hipLaunchKernelGGL(k_split<3>, grid, dim3(256), 0, hs, as, W, P, plane);
        else hipLaunchKernelGGL(k_split<4>, grid, dim3(256), 0, hs, as, W, P, plane);
        PRL_HIP_CHECK(hipGetLastError());
    }
    // 2. the Otsu value of every blurred plane; 3. its thresholds: the table of all 256
    const PageSet pp = page_set(P, plane, (size_t)W);
    const PageSetOut mp = page_set_out(M, plane, (size_t)W);
    if ((st = otsu_thresholds(pp, W, H, (int)planes_n, d_hist, d_thr, hs)) != PRL_OK) return st;
    LutArg lut;
    canny_threshold_table(sp.upper_coeff, sp.lower_coeff, lut.v);
    hipLaunchKernelGGL(k_store_lut, dim3(2), dim3(256), 0, hs, lut, d_lut);
    PRL_HIP_CHECK(hipGetLastError());
    // 4. cv::Canny
    if ((st = canny_run(W, H, 0, 0, pp, mp, (int)planes_n, canny_work, h_flags, hs, 1, d_lut, d_thr)) != PRL_OK) return st;
    // 5. the closing (iterations > 0) or opening (< 0) of every map
    const uint8_t* result = M;
    if (sp.iterations != 0) {
        const PageSetOut po = page_set_out(P, plane, (size_t)W);
        st = large ? morph_large_run(sp.iterations, as_source(mp), (int)planes_n, W, H, po, T, tmp_step(W), hs)
                   : morph_run(sp.iterations, as_source(mp), (int)planes_n, W, H, po, hs);
        if (st != PRL_OK) return st;
        result = P;
    }
    hipLaunchKernelGGL(k_or_planes, grid, dim3(256), 0, hs, result, plane, C, W, dst);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

namespace {

constexpr int kCedMaxIterations = 255;

int ced_checks(const PageArgs& a, int channels, const CedSpec& sp, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (ced_spec_check(sp)) return PRL_ERR_BAD_ARG;
    if (sp.size > kGaussMaxSide) return PRL_ERR_BAD_WINDOW;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    if (sp.iterations < -kCedMaxIterations || sp.iterations > kCedMaxIterations) return PRL_ERR_BAD_ARG;
    if ((st = pages_rows_ok(a, channels, 1, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    return pages_overlap_ok(a, channels, 1, false);
}

int ced_batch(const PageArgs& a, int C, const CedSpec& sp, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const int chunk = ced_pages_per_chunk(sp, a.n_pages, a.width, a.height, C, 0);
    WorkScope w;
    int st = w.open(stream, ced_work_bytes(sp, chunk, a.width, a.height, C), ced_small_bytes(chunk, C), ced_pinned_bytes(chunk, C));
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        st = ced_run(sp, src_pages(a, first), dst_pages(a, first), std::min(chunk, a.n_pages - first), a.width, a.height, C, w.scratch(),
                     w.small(), w.pinned<unsigned>(), w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_canny_edge_detection_batch_device(int n_pages, int channels, int blur_size, double upper_coeff, double lower_coeff,
                                              int morph_iterations, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                              int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const CedSpec sp{blur_size, upper_coeff, lower_coeff, morph_iterations};
    const int st = ced_checks(a, channels, sp, true);
    return st != PRL_OK ? st : ced_batch(a, channels, sp, stream);
}

int prl_hip_canny_edge_detection_host(int channels, int blur_size, double upper_coeff, double lower_coeff, int morph_iterations,
                                      const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs h{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const CedSpec sp{blur_size, upper_coeff, lower_coeff, morph_iterations};
    const int st = ced_checks(h, channels, sp, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(h, channels, 1, width, height, [&](const PageArgs& page, hipStream_t s) { return ced_batch(page, channels, sp, s); });
}

}  // extern "C"
