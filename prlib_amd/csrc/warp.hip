// warp.hip — prl::warpCrop (src/warp.cpp:32-102, src/warp.h:49-73) and its building block cv::warpPerspective(INTER_LINEAR) for
// 8-bit pages resident in device memory.  The arithmetic is stated in full in include/prl_hip.h ("perspective crop"); OpenCV's
// part of it [upstream] is restated in tests/warp_ref.py.
//
//   host             the size rule (warp.cpp:42-53), cv::getPerspectiveTransform's 8 x 8 system solved by LU with partial pivoting
//                    and cv::invert's closed form for 3 x 3, all in float64 with one rounding per written operation
//   k_warp_persp     warpPerspectiveInvoker + remapBilinear: per pixel (X0 + M[0] x1) * (32 / (W0 + M[6] x1)) in float64, rounded
//                    half to even to 5-bit fixed point, four taps weighted 32 (32 - fx)(32 - fy) ..., (sum + 2^14) >> 15.  The
//                    shape is k_warp's (rotate.hip): a workgroup makes 256 consecutive pixels of kPerspRows output rows, the bytes
//                    leave through LDS as aligned dwords, and both taps of a source row come with one 8-byte load where all four
//                    taps are inside the page.  OpenCV walks the output in blocks of bw columns and forms X0 / Y0 / W0 at the
//                    block's first column: the block width is part of the arithmetic (M[0] x is not M[0] xb + M[0] x1 in floating
//                    point), so the kernel forms the row terms once per (row, block) - one lane each - and every pixel adds its
//                    own M[0] x1.  The division is the IEEE one; nothing is reassociated or fused (-ffp-contract=off).
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "prl_internal.h"

namespace prl_hip {
namespace {

struct PerspPage {
    double M[9];   // result -> source, what cv::warpPerspective works with after its inversion
    int ow, oh;
    int bw;        // OpenCV's block width for this result size
    int reserved;
};
struct BorderBytes { int v[4]; };

constexpr int kPerspRows = 4;
// blocks a 256-pixel segment can touch: a row with more than one block has bw >= 64 (bw = min(1024 / min(16, oh), ow)), so the
// segment's last pixel lies at most ceil(255 / 64) = 4 blocks behind its first
constexpr int kPerspBlocks = 5;
constexpr int kMaxSide = 32767;

// 8 bytes at any alignment (global memory takes unaligned dword accesses on gfx9+); as in rotate.hip
__device__ __forceinline__ uint2 load8u(const uint8_t* p)
{
    uint2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ unsigned byte_at(uint2 v, int i) { return ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 0xffu; }

// saturate_cast<int>(max(INT_MIN, min(INT_MAX, f))) with std::min / std::max's comparisons: a NaN ends as INT_MAX
__device__ __forceinline__ int fixed_coord(double f)
{
    f = f < 2147483647.0 ? f : 2147483647.0;
    f = -2147483648.0 < f ? f : -2147483648.0;
    return __double2int_rn(f);
}

template <int CH, int BORDER>
__global__ void __launch_bounds__(256) k_warp_persp(PageSet src, PageSetOut dst, int width, int height, const PerspPage* __restrict__ pp,
                                                    BorderBytes cval)
{
    __shared__ __attribute__((aligned(16))) uint8_t seg[256 * CH + 16];
    __shared__ double rowT[kPerspRows][kPerspBlocks][3];
    const int page = blockIdx.z, y0 = blockIdx.y * kPerspRows, x0 = blockIdx.x * 256, x = x0 + (int)threadIdx.x;
    const PerspPage& p = pp[page];
    if (x0 >= p.ow || y0 >= p.oh) return;
    const uint8_t* s = src.page(page);
    const int bw = p.bw, b0 = x0 / bw;
    if (threadIdx.x < kPerspRows * kPerspBlocks) {
        const int ry = (int)threadIdx.x / kPerspBlocks, b = (int)threadIdx.x % kPerspBlocks;
        const double xb = (double)((b0 + b) * bw), y = (double)(y0 + ry);
        rowT[ry][b][0] = p.M[0] * xb + p.M[1] * y + p.M[2];
        rowT[ry][b][1] = p.M[3] * xb + p.M[4] * y + p.M[5];
        rowT[ry][b][2] = p.M[6] * xb + p.M[7] * y + p.M[8];
    }
    const int blk = x / bw, bl = min(blk - b0, kPerspBlocks - 1);
    const double x1 = (double)(x - blk * bw);
    const double ax = p.M[0] * x1, ay = p.M[3] * x1, aw = p.M[6] * x1;   // the same products in every row of the block
    __syncthreads();
    const int nrows = min(kPerspRows, p.oh - y0);
    for (int ry = 0; ry < nrows; ++ry) {
        const int y = y0 + ry;
        unsigned res[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) res[c] = 0;
        if (x < p.ow) {
            double W = rowT[ry][bl][2] + aw;
            W = W != 0 ? 32.0 / W : 0;
            const int X = fixed_coord((rowT[ry][bl][0] + ax) * W), Y = fixed_coord((rowT[ry][bl][1] + ay) * W);
            const int sx = max(-32768, min(32767, X >> 5)), sy = max(-32768, min(32767, Y >> 5));
            const int fx = X & 31, fy = Y & 31;
            const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
            const bool x0in = sx >= 0 && sx < width, x1in = sx + 1 >= 0 && sx + 1 < width;
            const bool y0in = sy >= 0 && sy < height, y1in = sy + 1 >= 0 && sy + 1 < height;
            // both taps of a row are 2 * CH <= 8 consecutive bytes: one 8-byte fetch per row when all four taps are inside and
            // the fetch stays inside the page (its last row may be the end of the allocation)
            const bool wide = x0in && x1in && y0in && y1in && (sy + 2 < height || sx * CH + 8 <= width * CH);
            if (wide) {
                const uint8_t* r0 = s + (size_t)sy * src.step + (size_t)sx * CH;
                const uint2 a = load8u(r0), b = load8u(r0 + src.step);
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int sum = (int)byte_at(a, c) * w00 + (int)byte_at(a, CH + c) * w01 + (int)byte_at(b, c) * w10 +
                                    (int)byte_at(b, CH + c) * w11;
                    res[c] = (unsigned)((sum + (1 << 14)) >> 15);
                }
            } else if (BORDER == PRL_BORDER_REPLICATE) {
                const int cx0 = max(0, min(width - 1, sx)), cx1 = max(0, min(width - 1, sx + 1));
                const uint8_t* r0 = s + (size_t)max(0, min(height - 1, sy)) * src.step;
                const uint8_t* r1 = s + (size_t)max(0, min(height - 1, sy + 1)) * src.step;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int sum = (int)r0[cx0 * CH + c] * w00 + (int)r0[cx1 * CH + c] * w01 + (int)r1[cx0 * CH + c] * w10 +
                                    (int)r1[cx1 * CH + c] * w11;
                    res[c] = (unsigned)((sum + (1 << 14)) >> 15);
                }
            } else {
                // rows and columns are only formed where the flags allow
                const uint8_t* r0 = s + (size_t)(y0in ? sy : 0) * src.step;
                const uint8_t* r1 = s + (size_t)(y1in ? sy + 1 : 0) * src.step;
                const int c0 = (x0in ? sx : 0) * CH, c1 = (x1in ? sx + 1 : 0) * CH;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int v00 = (x0in && y0in) ? r0[c0 + c] : cval.v[c], v01 = (x1in && y0in) ? r0[c1 + c] : cval.v[c];
                    const int v10 = (x0in && y1in) ? r1[c0 + c] : cval.v[c], v11 = (x1in && y1in) ? r1[c1 + c] : cval.v[c];
                    res[c] = (unsigned)((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15);
                }
            }
        }
        // the segment's bytes: [head up to the first 4-byte boundary of the destination][dwords][tail]
        uint8_t* d0 = dst.page(page) + (size_t)y * dst.step + (size_t)x0 * CH;
        const int nbytes = min(256, p.ow - x0) * CH;
        const int head = min(nbytes, (int)((4 - ((size_t)d0 & 3)) & 3));
        // the LDS image is shifted so that destination-aligned dwords are LDS-aligned dwords
        const int shift = (4 - head) & 3;
        if (ry) __syncthreads();  // the previous row's segment has been stored
#pragma unroll
        for (int c = 0; c < CH; ++c) seg[shift + (int)threadIdx.x * CH + c] = (uint8_t)res[c];
        __syncthreads();
        if ((int)threadIdx.x < head) d0[threadIdx.x] = seg[shift + threadIdx.x];
        const int ndw = (nbytes - head) / 4;
        const unsigned* sw = reinterpret_cast<const unsigned*>(seg + shift + head);
        unsigned* dw = reinterpret_cast<unsigned*>(d0 + head);
        for (int i = threadIdx.x; i < ndw; i += 256) dw[i] = sw[i];
        const int tail0 = head + ndw * 4;
        if ((int)threadIdx.x < nbytes - tail0) d0[tail0 + threadIdx.x] = seg[shift + tail0 + threadIdx.x];
    }
}

template <int BORDER>
int launch_persp(int channels, const PageSet& s, const PageSetOut& d, int width, int height, int n_pages, int max_ow, int max_oh,
                 const PerspPage* d_pp, const BorderBytes& cv, hipStream_t stream)
{
    const dim3 grid((unsigned)((max_ow + 255) / 256), (unsigned)((max_oh + kPerspRows - 1) / kPerspRows), (unsigned)n_pages);
    switch (channels) {
    case 1: hipLaunchKernelGGL((k_warp_persp<1, BORDER>), grid, dim3(256), 0, stream, s, d, width, height, d_pp, cv); break;
    case 2: hipLaunchKernelGGL((k_warp_persp<2, BORDER>), grid, dim3(256), 0, stream, s, d, width, height, d_pp, cv); break;
    case 3: hipLaunchKernelGGL((k_warp_persp<3, BORDER>), grid, dim3(256), 0, stream, s, d, width, height, d_pp, cv); break;
    default: hipLaunchKernelGGL((k_warp_persp<4, BORDER>), grid, dim3(256), 0, stream, s, d, width, height, d_pp, cv); break;
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// ---- host arithmetic -------------------------------------------------------------------------------------------------------------

// cvRound: half to even (the default rounding mode); a NaN and a value that does not fit an int give INT_MIN, which is what the
// x86 conversion answers [upstream]
int cv_round(double v)
{
    if (!(v >= -2147483648.5 && v <= 2147483647.5)) return INT_MIN;
    const double r = std::nearbyint(v);
    if (r >= 2147483648.0 || r < -2147483648.0) return INT_MIN;
    return (int)r;
}

// std::sqrt((bx - ax) * (bx - ax) + (by - ay) * (by - ay)): the reference's expression is an int one (warp.cpp:42-45); it wraps
// like 32-bit two's complement here, and a negative result makes the side a NaN
double side_length(int32_t ax, int32_t ay, int32_t bx, int32_t by)
{
    const uint32_t dx = (uint32_t)bx - (uint32_t)ax, dy = (uint32_t)by - (uint32_t)ay;
    const int32_t e = (int32_t)(dx * dx + dy * dy);
    return std::sqrt((double)e);
}

// warp.cpp:42-53 without the limits
void crop_size(const int32_t q[8], double ratio, int* w, int* h)
{
    const double side1 = side_length(q[0], q[1], q[2], q[3]), side2 = side_length(q[4], q[5], q[6], q[7]);
    const double side3 = side_length(q[0], q[1], q[6], q[7]), side4 = side_length(q[2], q[3], q[4], q[5]);
    long bitmapWidth = cv_round(side1 < side2 ? side2 : side1);    // std::max(a, b) = a < b ? b : a
    const long bitmapHeight = cv_round(side3 < side4 ? side4 : side3);
    if (ratio > 0.0) bitmapWidth = cv_round(bitmapHeight / ratio);
    *w = (int)bitmapWidth;
    *h = (int)bitmapHeight;
}
bool size_ok(int w, int h) { return w > 0 && h > 0 && w <= kMaxSide && h <= kMaxSide; }

// OpenCV's LU with partial pivoting (hal::LU64f) on the 8 x 8 system; false: singular
bool lu_solve8(double a[8][8], double b[8])
{
    const int n = 8;
    const double eps = DBL_EPSILON * 100;
    for (int i = 0; i < n; ++i) {
        int k = i;
        for (int j = i + 1; j < n; ++j)
            if (std::fabs(a[j][i]) > std::fabs(a[k][i])) k = j;
        if (std::fabs(a[k][i]) < eps) return false;
        if (k != i) {
            for (int j = 0; j < n; ++j) std::swap(a[i][j], a[k][j]);
            std::swap(b[i], b[k]);
        }
        const double d = -1 / a[i][i];
        for (int j = i + 1; j < n; ++j) {
            const double alpha = a[j][i] * d;
            for (int c = i + 1; c < n; ++c) a[j][c] += alpha * a[i][c];
            b[j] += alpha * b[i];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
        for (int k = i + 1; k < n; ++k) s -= a[i][k] * b[k];
        b[i] = s / a[i][i];
    }
    return true;
}

// cv::getPerspectiveTransform(src, dst) on CV_32FC2 corners
bool perspective_matrix(const double src_xy[8], const double dst_xy[8], double M[9])
{
    double a[8][8], b[8];
    for (int i = 0; i < 4; ++i) {
        const double sx = (double)(float)src_xy[2 * i], sy = (double)(float)src_xy[2 * i + 1];
        const double dx = (double)(float)dst_xy[2 * i], dy = (double)(float)dst_xy[2 * i + 1];
        const double r0[8] = {sx, sy, 1, 0, 0, 0, -sx * dx, -sy * dx}, r1[8] = {0, 0, 0, sx, sy, 1, -sx * dy, -sy * dy};
        std::memcpy(a[i], r0, sizeof(r0));
        std::memcpy(a[i + 4], r1, sizeof(r1));
        b[i] = dx;
        b[i + 4] = dy;
    }
    if (!lu_solve8(a, b)) return false;
    std::memcpy(M, b, sizeof(b));
    M[8] = 1;
    return true;
}

// cv::invert of a 3 x 3 float64 matrix (the closed form); false: det == 0 (or a NaN)
bool invert3(const double m[9], double t[9])
{
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (det == 0 || det != det) return false;
    const double d = 1 / det;
    t[0] = (m[4] * m[8] - m[5] * m[7]) * d;
    t[1] = (m[2] * m[7] - m[1] * m[8]) * d;
    t[2] = (m[1] * m[5] - m[2] * m[4]) * d;
    t[3] = (m[5] * m[6] - m[3] * m[8]) * d;
    t[4] = (m[0] * m[8] - m[2] * m[6]) * d;
    t[5] = (m[2] * m[3] - m[0] * m[5]) * d;
    t[6] = (m[3] * m[7] - m[4] * m[6]) * d;
    t[7] = (m[1] * m[6] - m[0] * m[7]) * d;
    t[8] = (m[0] * m[4] - m[1] * m[3]) * d;
    return true;
}

// every entry finite and at most 2^500 in magnitude: no intermediate of the per-pixel sequence can then overflow to infinity
// before the division, and none can become a NaN
bool matrix_ok(const double m[9])
{
    const double limit = std::ldexp(1.0, 500);
    for (int i = 0; i < 9; ++i)
        if (!(std::fabs(m[i]) <= limit)) return false;
    return true;
}

int bad_arg(const char* why)
{
    set_error_detail(why);
    return PRL_ERR_BAD_ARG;
}

// The checks every entry shares, before any device is touched.  tables: the per-page arguments are all there; batch: a
// *_batch_device entry, which never works in place.  The destination's rows are checked page by page against each result's own
// size (fill_page), and there is no span check: the results' sizes differ.
int persp_checks(const PageArgs& a, int channels, bool tables, int border_mode, bool batch)
{
    const int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    if (border_mode != PRL_BORDER_CONSTANT && border_mode != PRL_BORDER_REPLICATE) return PRL_ERR_UNSUPPORTED;
    if (pages_rows_ok(a, channels, 0, batch) != PRL_OK || !tables || !a.dst || (batch && a.src == a.dst)) return PRL_ERR_BAD_ARG;
    if (pages_sides_ok(a, kMaxSide) != PRL_OK) return bad_arg("warp: page sides above 32767");
    return PRL_OK;
}

// Fills the record of one page from the matrix warpPerspective is handed (`inverse_map`: it already maps result -> source).
int fill_page(const double M[9], int inverse_map, int ow, int oh, int channels, size_t dst_step, PerspPage* pg)
{
    if (!size_ok(ow, oh)) return bad_arg("warp: a result side is <= 0 or above 32767");
    if (dst_step < (size_t)ow * channels) return bad_arg("warp: dst_step below a result's row bytes");
    if (!matrix_ok(M)) return bad_arg("warp: a matrix entry is not finite or exceeds 2^500");
    if (inverse_map) std::memcpy(pg->M, M, sizeof(pg->M));
    else if (!invert3(M, pg->M)) return bad_arg("warp: the matrix is singular (det == 0)");
    if (!matrix_ok(pg->M)) return bad_arg("warp: an entry of the inverted matrix is not finite or exceeds 2^500");
    pg->ow = ow;
    pg->oh = oh;
    pg->bw = std::min(1024 / std::min(16, oh), ow);
    pg->reserved = 0;
    return PRL_OK;
}

BorderBytes border_bytes(const double* value)
{
    BorderBytes b;
    for (int c = 0; c < 4; ++c) b.v[c] = value ? std::max(0, std::min(255, cv_round(value[c]))) : 0;   // saturate_cast<uchar>(double)
    return b;
}

// The records go up through the device's shared workspace (pinned bounce block -> `small`) and the launches follow on the
// caller's stream: nothing here waits for the device's work.  The host only waits until the previous call's copy has left
// the bounce block before it overwrites it.
int persp_run(int channels, const std::vector<PerspPage>& pages, const PageArgs& a, int border_mode, const BorderBytes& cv, void* stream)
{
    const int n_pages = (int)pages.size();
    if (n_pages == 0) return PRL_OK;
    const size_t bytes = sizeof(PerspPage) * (size_t)n_pages;
    WorkScope w;
    int st = w.open(stream, 0, bytes, bytes);
    if (st != PRL_OK) return st;
    DeviceCtx* ctx = w.ctx;
    const hipStream_t hs = w.stream;
    if (ctx->pinned_use) PRL_HIP_CHECK(hipEventSynchronize(ctx->pinned_use));
    else PRL_HIP_CHECK(hipEventCreateWithFlags(&ctx->pinned_use, hipEventDisableTiming));
    std::memcpy(ctx->pinned, pages.data(), bytes);
    PRL_HIP_CHECK(hipMemcpyAsync(ctx->small, ctx->pinned, bytes, hipMemcpyHostToDevice, hs));
    PRL_HIP_CHECK(hipEventRecord(ctx->pinned_use, hs));
    const PerspPage* d_pp = w.small<const PerspPage>();
    const int chunk = stage_chunk(n_pages, 0);   // grid.z
    for (int first = 0; first < n_pages; first += chunk) {
        const int cnt = std::min(chunk, n_pages - first);
        int max_ow = 0, max_oh = 0;
        for (int i = 0; i < cnt; ++i) {
            max_ow = std::max(max_ow, pages[(size_t)(first + i)].ow);
            max_oh = std::max(max_oh, pages[(size_t)(first + i)].oh);
        }
        const PageSet s = src_pages(a, first);
        const PageSetOut d = dst_pages(a, first);
        st = border_mode == PRL_BORDER_REPLICATE
                 ? launch_persp<PRL_BORDER_REPLICATE>(channels, s, d, a.width, a.height, cnt, max_ow, max_oh, d_pp + first, cv, hs)
                 : launch_persp<PRL_BORDER_CONSTANT>(channels, s, d, a.width, a.height, cnt, max_ow, max_oh, d_pp + first, cv, hs);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

// cv::warpPerspective of every page with its own matrix and result size (the checks have passed)
int persp_pages(const PageArgs& a, int channels, const double* matrices, int inverse_map, const int32_t* out_wh, int border_mode,
                const double* border_value, void* stream)
{
    std::vector<PerspPage> pages((size_t)a.n_pages);
    for (int i = 0; i < a.n_pages; ++i) {
        const int st = fill_page(matrices + 9 * (size_t)i, inverse_map, out_wh[2 * i], out_wh[2 * i + 1], channels, a.dst_step, &pages[(size_t)i]);
        if (st != PRL_OK) return st;
    }
    return persp_run(channels, pages, a, border_mode, border_bytes(border_value), stream);
}

// size and matrix of one prl::warpCrop call (warp.cpp:42-68)
int crop_plan(const int32_t q[8], double ratio, int* ow, int* oh, double M[9])
{
    crop_size(q, ratio, ow, oh);
    if (!size_ok(*ow, *oh)) return bad_arg("warpCrop: the result's size is <= 0 or above 32767");
    double s[8], d[8] = {0, 0, (double)*ow, 0, (double)*ow, (double)*oh, 0, (double)*oh};
    for (int i = 0; i < 8; ++i) s[i] = (double)q[i];
    if (!perspective_matrix(s, d, M)) return bad_arg("warpCrop: the corners give a singular system");
    return PRL_OK;
}

}  // namespace
}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_warp_crop_size(const int32_t quad[8], double ratio, int* out_w, int* out_h)
{
    if (!quad || !out_w || !out_h) return PRL_ERR_BAD_ARG;
    int w, h;
    crop_size(quad, ratio, &w, &h);
    if (!size_ok(w, h)) return bad_arg("warpCrop: the result's size is <= 0 or above 32767");
    *out_w = w;
    *out_h = h;
    return PRL_OK;
}

int prl_hip_perspective_transform(const double src_xy[8], const double dst_xy[8], double M[9])
{
    if (!src_xy || !dst_xy || !M) return PRL_ERR_BAD_ARG;
    double m[9];
    if (!perspective_matrix(src_xy, dst_xy, m)) return bad_arg("getPerspectiveTransform: singular system");
    std::memcpy(M, m, sizeof(m));
    return PRL_OK;
}

int prl_hip_warp_perspective_batch_device(int n_pages, int channels, const double* matrices, int inverse_map, const uint8_t* d_src,
                                          size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                          size_t dst_page_stride, size_t dst_step, const int32_t* out_wh, int border_mode,
                                          const double* border_value, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const int st = persp_checks(a, channels, matrices && out_wh, border_mode, true);
    if (st != PRL_OK) return st;
    return persp_pages(a, channels, matrices, inverse_map, out_wh, border_mode, border_value, stream);
}

int prl_hip_warp_crop_batch_device(int n_pages, int channels, const int32_t* quads, double ratio, const uint8_t* d_src,
                                   size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                   size_t dst_page_stride, size_t dst_step, int32_t* out_wh, int border_mode,
                                   const double* border_value, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = persp_checks(a, channels, quads && out_wh, border_mode, true);
    if (st != PRL_OK) return st;
    std::vector<PerspPage> pages((size_t)n_pages);
    std::vector<int32_t> wh(2 * (size_t)n_pages);
    for (int i = 0; i < n_pages; ++i) {
        int ow, oh;
        double M[9];
        st = crop_plan(quads + 8 * (size_t)i, ratio, &ow, &oh, M);
        if (st == PRL_OK) st = fill_page(M, 0, ow, oh, channels, dst_step, &pages[(size_t)i]);
        if (st != PRL_OK) return st;
        wh[2 * (size_t)i] = ow;
        wh[2 * (size_t)i + 1] = oh;
    }
    st = persp_run(channels, pages, a, border_mode, border_bytes(border_value), stream);
    if (st == PRL_OK) std::copy(wh.begin(), wh.end(), out_wh);
    return st;
}

int prl_hip_warp_crop_host(int channels, const int32_t quad[8], double ratio, const uint8_t* src, size_t src_step, int width, int height,
                           uint8_t* dst, size_t dst_step, int border_mode, const double* border_value)
{
    if (!src) return PRL_ERR_EMPTY;   // a null image is an empty cv::Mat
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    int st = persp_checks(a, channels, quad != nullptr, border_mode, false);
    if (st != PRL_OK) return st;
    int ow, oh;
    double M[9];
    st = crop_plan(quad, ratio, &ow, &oh, M);
    if (st != PRL_OK) return st;
    PerspPage probe;
    st = fill_page(M, 0, ow, oh, channels, dst_step, &probe);   // the matrix checks, before anything is copied
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, channels, ow, oh, [&](const PageArgs& page, hipStream_t s) {
        const int32_t wh[2] = {ow, oh};
        return persp_pages(page, channels, M, 0, wh, border_mode, border_value, s);
    });
}

}  // extern "C"
