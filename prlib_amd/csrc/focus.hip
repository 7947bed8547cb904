// focus.hip — the focus measures of blur detection, LAPM, LAPV, TENG and GLVN (src/detectors/blurDetection.cpp:32-83), as one
// read-only pass over a batch of 8-bit pages of 1, 3 or 4 interleaved channels that leaves six integer sums per page and channel
// (focus.h: the indices, the terms of a pixel, the measures from the sums; the arithmetic is stated in include/prl_hip.h).
//
//   k_focus<C, KS>  A wavefront takes a tile: a strip of kFocusStripPx columns, 4 pixels a lane, and kFocusRows rows, which it
//                   walks down.  A row of a lane is C + 2 dwords - its 4 pixels and the 4 bytes on either side, which hold the
//                   pixel to the left and to the right (the x-neighbour of an interleaved pixel is C bytes away) - at any
//                   alignment; every byte sits at a compile-time position.  Each row is read and unpacked once per tile; what
//                   the window of three rows a, b, c needs of the older two is carried in registers:
//                       per byte column  b and a + b, which with the new row give V1 = a + 2b + c
//                       per pixel        the (1, 2, 1) sums along x of the rows a and b: Ah, Bh; the new row gives Ch
//                   and the terms are  L = V1(m) + Bh - 8 p,  X = 2 V1(m) - (V1(l) + V1(r)),  Y = 2 Bh - (Ah + Ch),
//                   Gx = V1(r) - V1(l), Gy = Ch - Ah for KS == 3 (the byte differences themselves for KS == 1): |X| and |Y| are
//                   absolute differences of two non-negative sums below 2^16, one v_sad_u16 each with the accumulation; the
//                   squares are 24-bit multiplies.  Rows above and below the page are BORDER_REFLECT_101 rows: a row index, the
//                   same for the wavefront.  The groups of 4 whose dwords would leave the row - the first of a row, the last
//                   one to three, a row shorter than 8 pixels - are left out there and belong to an edge tile, one per
//                   kFocusRows rows: a lane per row, the pixels one by one through focus_terms, the function of the CPU
//                   yardstick, the 3 x 3 window sliding along x.  (As lanes of the strips' own wavefronts they made those run
//                   both paths one after the other: 2.94 ms instead of 1.54 on 256 A4 gray pages.)
//                   A lane adds at most 4 * kFocusRows = 256 pixels, 5.3e8 at most, in 32 bits; everything wider is 64-bit: the
//                   64 lanes by shuffles, the kFocusWaves wavefronts of a workgroup through LDS, the workgroups by one 64-bit
//                   integer atomic per sum and channel into the result, zeroed before the launch.  Integer sums: exact in any
//                   order.  (A slab of per-workgroup partial sums and a finishing kernel instead of the atomics measured the
//                   same, 3.490 against 3.493 ms on 256 A4 gray pages with the kernel of that day - profiles/r20/INDEX.md - and
//                   needs a workspace and its lock: not kept.)
#include "prl_internal.h"

#include "focus.h"

#include <algorithm>

namespace prl_hip {

namespace {

constexpr int kFocusLanePx = 4;                       // pixels per lane and row
constexpr int kFocusStripPx = 64 * kFocusLanePx;      // columns of a tile
constexpr int kFocusRows = 64;                        // rows of a tile
constexpr int kFocusWaves = 4;                        // tiles per workgroup
constexpr int kFocusThreads = 64 * kFocusWaves;
constexpr int kFocusChunk = 65535;                    // pages per launch (grid.y)

// ---- kernel ----------------------------------------------------------------------------------------------------------------

// One row of a lane: C + 2 dwords at s (the byte 4 before the lane's first pixel); out[j], j = 0 .. 6 C - 1: the bytes of the
// pixels x0 - 1 .. x0 + 4 (byte 4 - C + j of the dwords)
template <int C>
__device__ __forceinline__ void fc_row(const uint8_t* s, int (&out)[6 * C])
{
    unsigned w[C + 2];
#pragma unroll
    for (int i = 0; i < C + 2; ++i) __builtin_memcpy(&w[i], s + 4 * i, 4);   // (any alignment)
#pragma unroll
    for (int j = 0; j < 6 * C; ++j) {
        const int pos = 4 - C + j;
        out[j] = (int)((w[pos / 4] >> (8 * (pos % 4))) & 0xffu);
    }
}

// a group of 4 pixels at x0 (a multiple of 4) is on the dword path when its window's bytes [x0 C - 4, (x0 + 4) C + 4) lie inside
// the row; the groups that are not are the first and those from focus_edge_start on
__host__ __device__ inline bool fc_on_dword_path(int x0, int W, int C)
{
    return x0 >= kFocusLanePx && (size_t)(x0 + kFocusLanePx) * C + 4 <= (size_t)W * C;
}
__host__ __device__ inline int fc_edge_start(int W, int C)
{
    const int last = W - kFocusLanePx - (4 + C - 1) / C;   // the largest x0 that passes
    return last < kFocusLanePx ? kFocusLanePx : (last / kFocusLanePx + 1) * kFocusLanePx;
}

// the pixels [xa, xb) of row y one by one, the 3 x 3 window sliding along x: three byte loads per pixel and channel
template <int C, int KS>
__device__ __forceinline__ void fc_edge_run(const uint8_t* base, size_t step, int W, int H, int y, int xa, int xb,
                                            unsigned (&acc)[C][kFocusSums])
{
    if (xa >= xb) return;
    const uint8_t* row[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) row[k] = base + (size_t)focus_reflect101(y - 1 + k, H) * step;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int t[3][3];
        const size_t xl = (size_t)focus_reflect101(xa - 1, W) * C + c, xm = (size_t)xa * C + c;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t[k][1] = row[k][xl];
            t[k][2] = row[k][xm];
        }
        for (int x = xa; x < xb; ++x) {
            const size_t xr = (size_t)focus_reflect101(x + 1, W) * C + c;
            int term[kFocusSums];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t[k][0] = t[k][1];
                t[k][1] = t[k][2];
                t[k][2] = row[k][xr];
            }
            focus_terms(t, KS, term);
#pragma unroll
            for (int k = 0; k < kFocusSums; ++k) acc[c][k] += (unsigned)term[k];
        }
    }
}

// grid = (ceil(tiles / kFocusWaves), pages); chunks = ceil(H / kFocusRows), tiles = (strips + 1) * chunks: tile = chunk * strips +
// strip below strips * chunks, then one edge tile per chunk - a lane per row, the pixels off the dword path.
// sums: [page][C][6] 64-bit words, zeroed before the launch.
template <int C, int KS>
__global__ __launch_bounds__(kFocusThreads) void k_focus(PageSet src, int W, int H, int strips, int chunks,
                                                         unsigned long long* __restrict__ sums)
{
    __shared__ long long s_part[kFocusWaves][C * kFocusSums];
    const int page = blockIdx.y, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int tile = blockIdx.x * kFocusWaves + wave;
    unsigned acc[C][kFocusSums];   // (S_LAP in two's complement)
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < kFocusSums; ++k) acc[c][k] = 0;
    const uint8_t* base = src.page(page);
    if (tile < strips * chunks) {
        const int strip = tile % strips, chunk = tile / strips;
        const int x0 = strip * kFocusStripPx + lane * kFocusLanePx;
        const int y0 = chunk * kFocusRows, y1 = min(H, y0 + kFocusRows);
        if (fc_on_dword_path(x0, W, C)) {
            const uint8_t* col = base + (size_t)x0 * C - 4;
            // pixel-channel q = i C + c of the lane has its byte columns at l = q, m = q + C, r = q + 2 C
            int pb[6 * C], sab[6 * C], ah[4 * C], bh[4 * C];
            fc_row<C>(col + (size_t)focus_reflect101(y0 - 1, H) * src.step, sab);
            fc_row<C>(col + (size_t)y0 * src.step, pb);
#pragma unroll
            for (int q = 0; q < 4 * C; ++q) {
                ah[q] = sab[q] + 2 * sab[q + C] + sab[q + 2 * C];
                bh[q] = pb[q] + 2 * pb[q + C] + pb[q + 2 * C];
            }
#pragma unroll
            for (int j = 0; j < 6 * C; ++j) sab[j] += pb[j];
            const uint8_t* next = col + (size_t)focus_reflect101(y0 + 1, H) * src.step;   // row y + 1
#pragma unroll 2
            for (int y = y0; y < y1; ++y) {
                int pc[6 * C], sbc[6 * C], v1[6 * C];
                fc_row<C>(next, pc);
                // row y + 2, or its reflection H - 2 (read at y = H - 1 only): one row on, or one row back
                next = y + 2 < H ? next + src.step : next - src.step;
#pragma unroll
                for (int j = 0; j < 6 * C; ++j) {
                    sbc[j] = pb[j] + pc[j];
                    v1[j] = sab[j] + sbc[j];
                }
#pragma unroll
                for (int q = 0; q < 4 * C; ++q) {
                    const int c = q % C, l = q, m = q + C, r = q + 2 * C;
                    const int p = pb[m];
                    const int ch = pc[l] + 2 * pc[m] + pc[r];
                    const int L = v1[m] + bh[q] - 8 * p;
                    const int gx = KS == 3 ? v1[r] - v1[l] : pb[r] - pb[l];
                    const int gy = KS == 3 ? ch - ah[q] : sbc[m] - sab[m];   // (b + c) - (a + b)
                    acc[c][kFocusSumP] += (unsigned)p;
                    acc[c][kFocusSumP2] += (unsigned)__mul24(p, p);
                    acc[c][kFocusSumLap] += (unsigned)L;
                    acc[c][kFocusSumLap2] += (unsigned)__mul24(L, L);
                    acc[c][kFocusSumLapm4] = __builtin_amdgcn_sad_u16((unsigned)(2 * v1[m]), (unsigned)(v1[l] + v1[r]), acc[c][kFocusSumLapm4]);
                    acc[c][kFocusSumLapm4] = __builtin_amdgcn_sad_u16((unsigned)(2 * bh[q]), (unsigned)(ah[q] + ch), acc[c][kFocusSumLapm4]);
                    acc[c][kFocusSumTeng] += (unsigned)(__mul24(gx, gx) + __mul24(gy, gy));
                    ah[q] = bh[q];
                    bh[q] = ch;
                }
#pragma unroll
                for (int j = 0; j < 6 * C; ++j) {
                    sab[j] = sbc[j];
                    pb[j] = pc[j];
                }
            }
        }
    } else if (tile < (strips + 1) * chunks) {
        const int y = (tile - strips * chunks) * kFocusRows + lane;
        if (y < H) {
            fc_edge_run<C, KS>(base, src.step, W, H, y, 0, min(kFocusLanePx, W), acc);
            fc_edge_run<C, KS>(base, src.step, W, H, y, fc_edge_start(W, C), W, acc);
        }
    }
    // every lane of the workgroup is here: 64 lanes -> lane 0, in 64 bits
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < kFocusSums; ++k) {
            long long v = (int)acc[c][k];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
            if (lane == 0) s_part[wave][c * kFocusSums + k] = v;
        }
    __syncthreads();
    if (t < C * kFocusSums) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kFocusWaves; ++w) v += s_part[w][t];
        if (v != 0) atomicAdd(&sums[(size_t)page * C * kFocusSums + t], (unsigned long long)v);   // (two's complement: S_LAP may be negative)
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

bool focus_channels_ok(int channels) { return channels == 1 || channels == 3 || channels == 4; }

// the checks of both entries, in the documented order (no device is touched); `result`: the entry's own output pointer
int focus_checks(const PageArgs& a, int channels, int teng_ksize, const void* result, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (!focus_ksize_ok(teng_ksize)) return PRL_ERR_BAD_ARG;
    if (!focus_channels_ok(channels)) return PRL_ERR_BAD_CHANNELS;
    if (!result) return PRL_ERR_BAD_ARG;
    if ((st = pages_rows_ok(a, channels, 0, batch)) != PRL_OK) return st;
    return pages_sides_ok(a);
}

template <int C>
void focus_launch_c(int ks, const dim3& grid, hipStream_t stream, const PageSet& src, int W, int H, int strips, int chunks,
                    unsigned long long* out)
{
    if (ks == 3) hipLaunchKernelGGL((k_focus<C, 3>), grid, dim3(kFocusThreads), 0, stream, src, W, H, strips, chunks, out);
    else hipLaunchKernelGGL((k_focus<C, 1>), grid, dim3(kFocusThreads), 0, stream, src, W, H, strips, chunks, out);
}

// n pages (a chunk); sums is overwritten
int focus_launch(int channels, int ks, const PageSet& src, int n, int W, int H, int64_t* sums, hipStream_t stream)
{
    PRL_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)n * channels * kFocusSums * sizeof(int64_t), stream));
    const int strips = (W + kFocusStripPx - 1) / kFocusStripPx, chunks = (H + kFocusRows - 1) / kFocusRows;
    const int tiles = (strips + 1) * chunks;   // and an edge tile per chunk
    const dim3 grid((unsigned)((tiles + kFocusWaves - 1) / kFocusWaves), (unsigned)n);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
    switch (channels) {
    case 1: focus_launch_c<1>(ks, grid, stream, src, W, H, strips, chunks, out); break;
    case 3: focus_launch_c<3>(ks, grid, stream, src, W, H, strips, chunks, out); break;
    default: focus_launch_c<4>(ks, grid, stream, src, W, H, strips, chunks, out); break;
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// after the checks; n_pages >= 1.  No workspace and no lock: the result is the only memory written.
int focus_batch(const PageArgs& a, int channels, int ks, int64_t* d_sums, hipStream_t stream)
{
    const int chunk = stage_chunk(a.n_pages, 0, 0, kFocusChunk);
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int st = focus_launch(channels, ks, src_pages(a, first), std::min(chunk, a.n_pages - first), a.width, a.height,
                                    d_sums + (size_t)first * channels * kFocusSums, stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_focus_sums_batch_device(int n_pages, int channels, int teng_ksize, const uint8_t* d_src, size_t src_page_stride,
                                    size_t src_step, int width, int height, int64_t* d_sums, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, nullptr, 0, 0};
    int st = focus_checks(a, channels, teng_ksize, d_sums, true);
    if (st != PRL_OK) return st;
    if (n_pages == 0) return PRL_OK;
    int dev;   // the device check alone
    st = current_device(&dev);
    if (st != PRL_OK) return st;
    return focus_batch(a, channels, teng_ksize, d_sums, static_cast<hipStream_t>(stream));
}

int prl_hip_focus_measures_host(int channels, int teng_ksize, const uint8_t* src, size_t src_step, int width, int height,
                                double* measures, int64_t* sums)
{
    const PageArgs h{1, src, 0, src_step, width, height, nullptr, 0, 0};
    int st = focus_checks(h, channels, teng_ksize, measures, false);
    if (st != PRL_OK) return st;
    int64_t got[4 * kFocusSums];
    // the page goes up through the staging area; the sums come down through the device's small and pinned blocks
    st = stage_host_pages(h, channels, 0, 0, 0, [&](const PageArgs& page, hipStream_t s) -> int {
        const size_t bytes = (size_t)channels * kFocusSums * sizeof(int64_t);
        WorkScope w;
        int r = w.open(s, 0, bytes, bytes);
        if (r != PRL_OK) return r;
        if ((r = focus_batch(page, channels, teng_ksize, w.small<int64_t>(), w.stream)) != PRL_OK) return r;
        PRL_HIP_CHECK(hipMemcpyAsync(w.pinned(), w.small(), bytes, hipMemcpyDeviceToHost, w.stream));
        PRL_HIP_CHECK(hipStreamSynchronize(w.stream));
        std::copy(w.pinned<int64_t>(), w.pinned<int64_t>() + channels * kFocusSums, got);
        return PRL_OK;
    });
    if (st != PRL_OK) return st;
    for (int c = 0; c < channels; ++c) {
        focus_from_sums(got + c * kFocusSums, width, height, measures + c * kFocusMeasures);
        if (sums) std::copy(got + c * kFocusSums, got + (c + 1) * kFocusSums, sums + c * kFocusSums);
    }
    return PRL_OK;
}

int prl_hip_focus_from_sums(const int64_t sums[6], int width, int height, double measures[4])
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!sums || !measures || width > kStageMaxSide || height > kStageMaxSide) return PRL_ERR_BAD_ARG;
    focus_from_sums(sums, width, height, measures);
    return PRL_OK;
}

}  // extern "C"
