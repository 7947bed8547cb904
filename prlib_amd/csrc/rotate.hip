// rotate.hip — prl::rotate for pages resident in device memory; prl::deskew's second half.
//
// Reference: src/rotate.cpp:35-72.  OpenCV's arithmetic [upstream] is restated with citations in the test oracle (oracle/,
// deskew file); the kernels below reproduce it bit for bit:
//
//   host                 matrices of getRotationMatrix2D / warpAffine's inversion, one WarpPage record per page
//   k_warp<CH>           warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) between the two bitwise_not of rotate.cpp:61-70: 10-bit
//                        fixed-point coordinates from float64 (one rounding per operation), 5-bit bilinear weights,
//                        (sum + 2^14) >> 15.  k_rot90<CH>: the transpose/flip branches (:38-58).
#include <algorithm>
#include <cmath>
#include <vector>

#include "prl_internal.h"

namespace prl_hip {
namespace {

// 8 bytes at any alignment (global memory takes unaligned dword accesses on gfx9+)
__device__ __forceinline__ uint2 load8u(const uint8_t* p)
{
    uint2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ unsigned byte_at(uint2 v, int i) { return ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 0xffu; }

// A workgroup produces 256 consecutive pixels of kWarpRows output rows; the result bytes go through LDS so that a row segment is
// stored as dwords (byte stores of CH-byte pixels cost three to four instructions per pixel).  The column terms of the source
// coordinates (warpAffine's adelta / bdelta tables, float64) are formed once per thread and reused for its rows, the row terms
// once per row by one lane.  Pages of kind 1 / 3 (quarter turns) are left to k_rot90.
constexpr int kWarpRows = 4;
template <int CH>
__global__ void __launch_bounds__(256) k_warp(PageSet src, PageSetOut dst, int width, int height, const WarpPage* __restrict__ wp)
{
    __shared__ __attribute__((aligned(16))) uint8_t seg[256 * CH + 16];
    __shared__ int rowXY[kWarpRows][2];
    const int page = blockIdx.z, y0 = blockIdx.y * kWarpRows, x0 = blockIdx.x * 256, x = x0 + (int)threadIdx.x;
    const WarpPage& p = wp[page];
    if (p.kind == 1 || p.kind == 3 || x0 >= p.ow || y0 >= p.oh) return;
    const uint8_t* s = src.page(page);
    int adelta = 0, bdelta = 0;
    if (p.kind == 0) {
        if (threadIdx.x < kWarpRows) {
            const int y = y0 + (int)threadIdx.x;
            rowXY[threadIdx.x][0] = __double2int_rn((p.M[1] * y + p.M[2]) * 1024) + 16;
            rowXY[threadIdx.x][1] = __double2int_rn((p.M[4] * y + p.M[5]) * 1024) + 16;
        }
        adelta = __double2int_rn(p.M[0] * x * 1024);
        bdelta = __double2int_rn(p.M[3] * x * 1024);
        __syncthreads();
    }
    const int nrows = min(kWarpRows, p.oh - y0);
    for (int ry = 0; ry < nrows; ++ry) {
        const int y = y0 + ry;
        unsigned res[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) res[c] = 0;
        if (x < p.ow) {
            if (p.kind != 0) {  // 2: half turn; 4: copy
                const int sx = p.kind == 2 ? width - 1 - x : x, sy = p.kind == 2 ? height - 1 - y : y;
                const uint8_t* q = s + (size_t)sy * src.step + (size_t)sx * CH;
#pragma unroll
                for (int c = 0; c < CH; ++c) res[c] = q[c];
            } else {
                const int X = (rowXY[ry][0] + adelta) >> 5, Y = (rowXY[ry][1] + bdelta) >> 5;
                const int sx = max(-32768, min(32767, X >> 5)), sy = max(-32768, min(32767, Y >> 5));
                const int fx = X & 31, fy = Y & 31;
                const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
                const bool x0in = sx >= 0 && sx < width, x1in = sx + 1 >= 0 && sx + 1 < width;
                const bool y0in = sy >= 0 && sy < height, y1in = sy + 1 >= 0 && sy + 1 < height;
                const uint8_t* r0 = s + (size_t)sy * src.step + (size_t)sx * CH;  // only dereferenced where the flags allow
                const uint8_t* r1 = r0 + src.step;
                // both taps of a row are 2 * CH <= 8 consecutive bytes: one 8-byte fetch per row when all four taps are inside
                // and the fetch cannot run past the page's last row
                const bool wide = x0in && x1in && y0in && y1in && (sy + 2 < height || sx * CH + 8 <= (int)src.step);
                if (wide) {
                    const uint2 a = load8u(r0), b = load8u(r1);
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        // the source is cv::bitwise_not(input) and the weights add up to 2^15:
                        // sum w (255 - v) = 255 * 2^15 - sum w v
                        const int wv = (int)byte_at(a, c) * w00 + (int)byte_at(a, CH + c) * w01 + (int)byte_at(b, c) * w10 +
                                       (int)byte_at(b, CH + c) * w11;
                        res[c] = (unsigned)(255 - ((255 * 32768 - wv + (1 << 14)) >> 15));
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        // outside the (inverted) source the border value 0
                        const int v00 = (x0in && y0in) ? 255 - r0[c] : 0, v01 = (x1in && y0in) ? 255 - r0[CH + c] : 0;
                        const int v10 = (x0in && y1in) ? 255 - r1[c] : 0, v11 = (x1in && y1in) ? 255 - r1[CH + c] : 0;
                        res[c] = (unsigned)(255 - ((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15));
                    }
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

// Quarter turns (rotate.cpp:38-58): out(y, x) = in(height - 1 - x, y) for 90, in(x, width - 1 - y) for 270.  A 32 x 32 tile
// is read along source rows, turned in LDS and written along destination rows (the straightforward one-thread-per-pixel
// form reads a different source row in every lane: 7.0 ms for 64 A4 colour pages, 6 % of the roofline).
template <int CH>
__global__ void __launch_bounds__(256) k_rot90(PageSet src, PageSetOut dst, int width, int height, const WarpPage* __restrict__ wp)
{
    __shared__ uint8_t tile[32][32 * CH + 4];
    const int page = blockIdx.z;
    const WarpPage& p = wp[page];
    if (p.kind != 1 && p.kind != 3) return;
    const int ox0 = blockIdx.x * 32, oy0 = blockIdx.y * 32;  // output tile; output is height (cols) x width (rows)
    if (ox0 >= p.ow || oy0 >= p.oh) return;
    const uint8_t* s = src.page(page);
    // source tile: rows sy0 .. sy0+31, cols sx0 .. sx0+31 (clipped)
    const int sx0 = p.kind == 1 ? oy0 : width - 32 - oy0, sy0 = p.kind == 1 ? height - 32 - ox0 : ox0;
    for (int i = threadIdx.x; i < 32 * 32; i += 256) {
        const int r = i >> 5, c = i & 31;
        const int sy = sy0 + r, sx = sx0 + c;
        if (sy >= 0 && sy < height && sx >= 0 && sx < width) {
            const uint8_t* q = s + (size_t)sy * src.step + (size_t)sx * CH;
#pragma unroll
            for (int k = 0; k < CH; ++k) tile[r][c * CH + k] = q[k];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * 32; i += 256) {
        const int oy = i >> 5, ox = i & 31;
        const int y = oy0 + oy, x = ox0 + ox;
        if (y >= p.oh || x >= p.ow) continue;
        // kind 1: in(height-1-x, y): row index height-1-x - sy0 = 31 - ox, col y - sx0 = oy
        // kind 3: in(x, width-1-y): row x - sy0 = ox, col width-1-y - sx0 = 31 - oy
        const int r = p.kind == 1 ? 31 - ox : ox, c = p.kind == 1 ? oy : 31 - oy;
        uint8_t* d = dst.page(page) + (size_t)y * dst.step + (size_t)x * CH;
#pragma unroll
        for (int k = 0; k < CH; ++k) d[k] = tile[r][c * CH + k];
    }
}

bool eq_d(double a, double b, double delta) { return std::fabs(a - b) <= delta; }

// rotate.cpp:37-58
int rotate_kind(double angle)
{
    angle = std::fmod(angle, 360.0);
    if (eq_d(angle, 90.0, 1e-7)) return 1;
    if (eq_d(angle, 180.0, 1e-7)) return 2;
    if (eq_d(angle, 270.0, 1e-7)) return 3;
    return 0;
}

// getRotationMatrix2D((len/2, len/2), angle, 1.0) then warpAffine's inversion [upstream, see the oracle]
void rotate_matrix(int width, int height, double angle, double M[6])
{
    const int len = std::max(width, height);
    const float cx = static_cast<float>(len / 2.0), cy = static_cast<float>(len / 2.0);
    angle = std::fmod(angle, 360.0);
    angle *= 3.1415926535897932384626433832795 / 180;
    const double alpha = std::cos(angle) * 1.0, beta = std::sin(angle) * 1.0;
    M[0] = alpha; M[1] = beta; M[2] = (1 - alpha) * cx - beta * cy;
    M[3] = -beta; M[4] = alpha; M[5] = beta * cx + (1 - alpha) * cy;
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
}

}  // namespace

void fill_warp_page(int width, int height, double angle, bool copy, WarpPage* wp)
{
    wp->kind = copy ? 4 : rotate_kind(angle);
    if (wp->kind == 1 || wp->kind == 3) { wp->ow = height; wp->oh = width; }
    else if (wp->kind == 2 || wp->kind == 4) { wp->ow = width; wp->oh = height; }
    else { wp->ow = wp->oh = std::max(width, height); rotate_matrix(width, height, angle, wp->M); }
}

int launch_warp(int channels, const PageSet& s, const PageSetOut& d, int width, int height, int n_pages, int max_ow, int max_oh,
                const WarpPage* d_wp, hipStream_t stream, bool any_quarter)
{
    const dim3 grid((unsigned)((max_ow + 255) / 256), (unsigned)((max_oh + kWarpRows - 1) / kWarpRows), (unsigned)n_pages);
    switch (channels) {
    case 1: hipLaunchKernelGGL(k_warp<1>, grid, dim3(256), 0, stream, s, d, width, height, d_wp); break;
    case 2: hipLaunchKernelGGL(k_warp<2>, grid, dim3(256), 0, stream, s, d, width, height, d_wp); break;
    case 3: hipLaunchKernelGGL(k_warp<3>, grid, dim3(256), 0, stream, s, d, width, height, d_wp); break;
    default: hipLaunchKernelGGL(k_warp<4>, grid, dim3(256), 0, stream, s, d, width, height, d_wp); break;
    }
    PRL_HIP_CHECK(hipGetLastError());
    if (any_quarter) {
        const dim3 g2((unsigned)((max_ow + 31) / 32), (unsigned)((max_oh + 31) / 32), (unsigned)n_pages);
        switch (channels) {
        case 1: hipLaunchKernelGGL(k_rot90<1>, g2, dim3(256), 0, stream, s, d, width, height, d_wp); break;
        case 2: hipLaunchKernelGGL(k_rot90<2>, g2, dim3(256), 0, stream, s, d, width, height, d_wp); break;
        case 3: hipLaunchKernelGGL(k_rot90<3>, g2, dim3(256), 0, stream, s, d, width, height, d_wp); break;
        default: hipLaunchKernelGGL(k_rot90<4>, g2, dim3(256), 0, stream, s, d, width, height, d_wp); break;
        }
        PRL_HIP_CHECK(hipGetLastError());
    }
    return PRL_OK;
}

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_rotate_out_size(int width, int height, double angle, int* out_w, int* out_h)
{
    if (!out_w || !out_h) return PRL_ERR_BAD_ARG;
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    WarpPage wp{};
    fill_warp_page(width, height, angle, false, &wp);
    *out_w = wp.ow;
    *out_h = wp.oh;
    return PRL_OK;
}

// prl::rotate on device pages, one angle per page (angles == NULL: not allowed).
int prl_hip_rotate_batch_device(int n_pages, int channels, const double* angles, const uint8_t* d_src, size_t src_page_stride,
                                size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    // (the destination's rows are checked per page below, against the page's own result width)
    if ((st = pages_rows_ok(a, channels, 0, true)) != PRL_OK || !angles || !d_dst || d_src == d_dst) return PRL_ERR_BAD_ARG;
    if ((st = pages_sides_ok(a, 32767)) != PRL_OK) return st;
    if (n_pages == 0) return PRL_OK;
    const int chunk = stage_chunk(n_pages, 0, 0, 32768);
    WorkScope w;
    st = w.open(stream, 0, sizeof(WarpPage) * (size_t)chunk, 0);
    if (st != PRL_OK) return st;
    const hipStream_t hs = w.stream;
    std::vector<WarpPage> wp((size_t)chunk);
    for (int first = 0; first < n_pages; first += chunk) {
        const int cnt = std::min(chunk, n_pages - first);
        int max_ow = 0, max_oh = 0;
        for (int i = 0; i < cnt; ++i) {
            fill_warp_page(width, height, angles[first + i], false, &wp[(size_t)i]);
            max_ow = std::max(max_ow, wp[(size_t)i].ow);
            max_oh = std::max(max_oh, wp[(size_t)i].oh);
            if (dst_step < (size_t)wp[(size_t)i].ow * channels) return PRL_ERR_BAD_ARG;
        }
        PRL_HIP_CHECK(hipMemcpyAsync(w.small(), wp.data(), sizeof(WarpPage) * (size_t)cnt, hipMemcpyHostToDevice, hs));
        PRL_HIP_CHECK(hipStreamSynchronize(hs));  // `wp` is pageable host memory reused by the next chunk
        st = launch_warp(channels, src_pages(a, first), dst_pages(a, first), width, height, cnt, max_ow, max_oh, w.small<const WarpPage>(), hs);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

/* prl::rotate on one host image; dst must hold the size prl_hip_rotate_out_size reports (dst_step is compared with it after the
 * device stage).  The batch entry refuses what is left: sides above 32767. */
int prl_hip_rotate_host(int channels, double angle, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                        size_t dst_step)
{
    const PageArgs h{1, src, 0, src_step, width, height, dst, 0, dst_step};
    if (pages_nonempty(h) != PRL_OK || !src) return PRL_ERR_EMPTY;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    if (!dst || pages_rows_ok(h, channels, 0, false) != PRL_OK) return PRL_ERR_BAD_ARG;
    int ow = 0, oh = 0;
    const int st = prl_hip_rotate_out_size(width, height, angle, &ow, &oh);
    if (st != PRL_OK) return st;
    return host_roundtrip(h, channels, ow, oh, &ow, &oh, [&](const PageArgs& p, hipStream_t s) {
        return prl_hip_rotate_batch_device(1, channels, &angle, p.src, p.src_page_stride, p.src_step, width, height, p.dst,
                                           p.dst_page_stride, p.dst_step, s);
    });
}

}  // extern "C"
