// clahe.hip — cv::CLAHE::apply on 8-bit pages, cv::equalizeHist, and the reference's EnhanceLocalContrastByCLAHE
// (src/imageLibCommon.cpp:327-395), which is the first followed by the second on every channel.  The arithmetic is in clahe.h.
//   k_clahe_hist<C>    hist[page][channel][tileY][tileX][256] over the EXTENDED page, the pad read through reflected source
//                      coordinates.  A work unit is a tile, or a band of kClaheHistBandRows rows of a tall one; a workgroup takes
//                      units until it has about kClaheHistUnitPx pixels (one band of an A4 page's tile, hundreds of tiny tiles).
//                      A lane takes 4 pixels; bins in LDS, one global atomic per non-empty bin and unit; a wavefront whose 256
//                      pixels agree in a channel adds once (k_tone_hist's test: same-address LDS atomics serialise).
//   k_clahe_luts       a wavefront per tile, four bins a lane: the clipped excess by a butterfly, the redistribution bin by bin
//                      (clahe_redistributed: the stepped residual in closed form), the running sum by a scan, 256 bytes out.
//   k_clahe_interp<C>  the only pass that writes pixels; 1..4 interleaved channels, source and destination may be the same.  A
//                      workgroup takes a block of kClaheBlockW x kClaheBlockH pixels, 8 rows a trip, 4 pixels a lane, and stages
//                      the tile tables its block touches in LDS (up to kClaheStageTables per channel); a block over tinier tiles
//                      reads them from global memory.  With out_hist it also counts the bytes it writes, per page and channel,
//                      for the equalization that follows: three passes over the pixels instead of four.
//   k_equalize_derive  hist[page][channel][256] -> table, a lane per (page, channel), by equalize_lut.
// The equalization's histogram (alone) and its table pass are tone.hip's k_tone_hist and k_tone_lut.
#include "prl_internal.h"

#include "clahe.h"

#include <algorithm>
#include <cmath>

namespace prl_hip {

// tone.hip
int hist_launch(int channels, const PageSet& src, int n, int W, int H, unsigned* hist, hipStream_t stream);
int lut_launch(int channels, int oc, const PageSet& src, const PageSetOut& dst, int n, int W, int H, const uint8_t* lut,
               size_t lut_page_stride, hipStream_t stream);

namespace {

constexpr int kClaheThreads = 256;
constexpr int kClaheRowsPerTrip = kClaheThreads * 4 / kClaheBlockW;   // 8
static_assert(kClaheBlockW % 4 == 0 && kClaheThreads * 4 % kClaheBlockW == 0 && kClaheBlockH % kClaheRowsPerTrip == 0, "block shape");

// 4 pixels of C interleaved bytes at s (any alignment) into v[pixel][channel]
template <int C>
__device__ inline void load4(const uint8_t* s, unsigned v[4][C])
{
    unsigned w[C];   // C == 3: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
#pragma unroll
    for (int i = 0; i < C; ++i) __builtin_memcpy(&w[i], s + 4 * i, 4);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int b = i * C + c;
            v[i][c] = (w[b / 4] >> (8 * (b % 4))) & 0xffu;
        }
}

// n (0..4) values of a lane into the 256 bins of one channel.  Every lane of the wavefront calls it (the vote needs them all).
// A page is mostly paper: a wavefront that sees one value adds once instead of 64 times to one LDS word.
__device__ inline void add4(unsigned* bins, const unsigned v0, const unsigned v1, const unsigned v2, const unsigned v3, int n)
{
    const bool flat = n == 4 && v1 == v0 && v2 == v0 && v3 == v0;
    const unsigned first = (unsigned)__shfl((int)v0, 0);
    if (__all(flat && v0 == first)) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&bins[first], 256u);
    } else if (flat) {
        atomicAdd(&bins[v0], 4u);
    } else {
        if (n > 0) atomicAdd(&bins[v0], 1u);
        if (n > 1) atomicAdd(&bins[v1], 1u);
        if (n > 2) atomicAdd(&bins[v2], 1u);
        if (n > 3) atomicAdd(&bins[v3], 1u);
    }
}

// grid = (ceil(units / units_per_group), pages); units = tiles * bands.  hist: [page][C][tile][256], zeroed before the launch.
template <int C>
__global__ __launch_bounds__(kClaheThreads) void k_clahe_hist(PageSet src, int W, int H, ClaheGeom g, int bands, int units_per_group,
                                                              unsigned* __restrict__ hist)
{
    __shared__ unsigned h[C * 256];
    const int page = blockIdx.y, t = threadIdx.x;
    const int tiles = g.tiles_x * g.tiles_y, units = tiles * bands;
    const int gpr = (g.tile_w + 3) / 4;   // groups of 4 pixels per tile row
    const uint8_t* base = src.page(page);
#pragma unroll
    for (int c = 0; c < C; ++c) h[c * 256 + t] = 0;
    __syncthreads();
    const int u_end = min(units, ((int)blockIdx.x + 1) * units_per_group);
    for (int u = blockIdx.x * units_per_group; u < u_end; ++u) {
        const int tile = u / bands, band = u - tile * bands;
        const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        const int y0 = ty * g.tile_h + band * kClaheHistBandRows, rows = min(kClaheHistBandRows, g.tile_h - band * kClaheHistBandRows);
        const int x0 = tx * g.tile_w;
        const int groups = rows * gpr;
        for (int gb = 0; gb < groups; gb += kClaheThreads) {   // every lane makes the same trips
            const int gi = gb + t;
            int n = 0;
            unsigned v[4][C];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) v[i][c] = 0;
            if (gi < groups) {
                const int r = gi / gpr, q = gi - r * gpr;
                const int xe = x0 + q * 4;   // a coordinate of the extended page
                n = min(4, g.tile_w - q * 4);
                const uint8_t* row = base + (size_t)clahe_reflect101(y0 + r, H) * src.step;
                if (n == 4 && xe + 4 <= W) {
                    load4<C>(row + (size_t)xe * C, v);
                } else {
                    for (int i = 0; i < n; ++i) {
                        const uint8_t* s = row + (size_t)clahe_reflect101(xe + i, W) * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) v[i][c] = s[c];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) add4(h + c * 256, v[0][c], v[1][c], v[2][c], v[3][c], n);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const unsigned cnt = h[c * 256 + t];
            if (cnt) {
                atomicAdd(&hist[(((size_t)page * C + c) * tiles + tile) * 256 + t], cnt);
                h[c * 256 + t] = 0;
            }
        }
        __syncthreads();
    }
}

// grid = ceil(n_tiles / 4): a wavefront per tile of hist[n_tiles][256] (tiles of every page and channel, one after the other)
__global__ __launch_bounds__(kClaheThreads) void k_clahe_luts(int n_tiles, int clip, float lut_scale, const unsigned* __restrict__ hist,
                                                              uint8_t* __restrict__ luts)
{
    const int tile = blockIdx.x * (kClaheThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= n_tiles) return;   // (a whole wavefront)
    const unsigned* hp = hist + (size_t)tile * 256 + lane * 4;
    int h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = (int)hp[i];
    if (clip > 0) {
        int clipped = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) clipped += clahe_excess(h[i], clip);
        for (int o = 32; o > 0; o >>= 1) clipped += __shfl_xor(clipped, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = min(h[i], clip) + clahe_redistributed(lane * 4 + i, clipped);
    }
    const int own = h[0] + h[1] + h[2] + h[3];
    int upto = own;   // inclusive scan over the lanes
    for (int o = 1; o < 64; o <<= 1) {
        const int below = __shfl_up(upto, o);
        if (lane >= o) upto += below;
    }
    int sum = upto - own;
    unsigned packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sum += h[i];
        packed |= (unsigned)clahe_lut_entry(sum, lut_scale) << (8 * i);
    }
    __builtin_memcpy(luts + (size_t)tile * 256 + lane * 4, &packed, 4);   // (the caller's memory: any alignment)
}

// grid = (ceil(W / kClaheBlockW), ceil(H / kClaheBlockH), pages).  luts: [page][C][tileY][tileX][256]; out_hist: null, or
// [page][C][256] zeroed before the launch.
template <int C>
__global__ __launch_bounds__(kClaheThreads) void k_clahe_interp(PageSet src, PageSetOut dst, int W, int H, ClaheGeom g,
                                                                const uint8_t* __restrict__ luts, unsigned* __restrict__ out_hist)
{
    __shared__ unsigned tabw[kClaheStageTables * C * 64];
    __shared__ unsigned bins[C * 256];
    const int page = blockIdx.z, t = threadIdx.x;
    const int bx0 = blockIdx.x * kClaheBlockW, by0 = blockIdx.y * kClaheBlockH;
    const int tiles = g.tiles_x * g.tiles_y;
    const uint8_t* lp = luts + (size_t)page * C * tiles * 256;
    // the tables of the block: the first pixel's lower index to the last pixel's upper one, each way (the indices rise with x)
    int tx_lo, tx_hi, ty_lo, ty_hi, unused;
    float fa, fb;
    clahe_axis(bx0, g.inv_tw, g.tiles_x, &tx_lo, &unused, &fa, &fb);
    clahe_axis(min(bx0 + kClaheBlockW, W) - 1, g.inv_tw, g.tiles_x, &unused, &tx_hi, &fa, &fb);
    clahe_axis(by0, g.inv_th, g.tiles_y, &ty_lo, &unused, &fa, &fb);
    clahe_axis(min(by0 + kClaheBlockH, H) - 1, g.inv_th, g.tiles_y, &unused, &ty_hi, &fa, &fb);
    const int ntx = tx_hi - tx_lo + 1, nty = ty_hi - ty_lo + 1;
    const bool staged = ntx * nty <= kClaheStageTables;
    if (staged) {
        const int words = ntx * nty * C * 64;   // slot (jy * ntx + jx) * C + c
        for (int i = t; i < words; i += kClaheThreads) {
            const int slot = i >> 6, w = i & 63;
            const int c = slot % C, j = slot / C;
            const int jy = j / ntx, jx = j - jy * ntx;
            unsigned word;
            __builtin_memcpy(&word, lp + ((size_t)(c * g.tiles_y + ty_lo + jy) * g.tiles_x + tx_lo + jx) * 256 + w * 4, 4);
            tabw[i] = word;
        }
    }
    if (out_hist) {
#pragma unroll
        for (int c = 0; c < C; ++c) bins[c * 256 + t] = 0;
    }
    __syncthreads();
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
    // entry p of the table of tile (ty, tx), channel c: from the stage, or from global memory (each load in its own address space)
    auto entry = [&](int ty, int tx, int c, unsigned p) -> uint8_t {
        return staged ? tab[(((ty - ty_lo) * ntx + (tx - tx_lo)) * C + c) * 256 + p]
                      : lp[((size_t)(c * g.tiles_y + ty) * g.tiles_x + tx) * 256 + p];
    };
    const int x = bx0 + (t % (kClaheBlockW / 4)) * 4, ly = t / (kClaheBlockW / 4);
    const int n = min(4, W - x);   // <= 0: no pixel
    int tx1[4], tx2[4];
    float xa[4], xa1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) clahe_axis(min(x + i, W - 1), g.inv_tw, g.tiles_x, &tx1[i], &tx2[i], &xa[i], &xa1[i]);
    for (int trip = 0; trip < kClaheBlockH / kClaheRowsPerTrip; ++trip) {   // every lane makes the same trips
        const int y = by0 + trip * kClaheRowsPerTrip + ly;
        const int live = y < H && n > 0 ? n : 0;
        unsigned o[4][C];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) o[i][c] = 0;
        if (live) {
            int ty1, ty2;
            float ya, ya1;
            clahe_axis(y, g.inv_th, g.tiles_y, &ty1, &ty2, &ya, &ya1);
            const uint8_t* s = src.page(page) + (size_t)y * src.step + (size_t)x * C;
            uint8_t* d = dst.page(page) + (size_t)y * dst.step + (size_t)x * C;
            unsigned v[4][C];
            if (live == 4) {
                load4<C>(s, v);
            } else {
                for (int i = 0; i < live; ++i)
#pragma unroll
                    for (int c = 0; c < C; ++c) v[i][c] = s[i * C + c];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < live) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const unsigned p = v[i][c];
                        o[i][c] = clahe_blend(entry(ty1, tx1[i], c, p), entry(ty1, tx2[i], c, p), entry(ty2, tx1[i], c, p),
                                              entry(ty2, tx2[i], c, p), xa[i], xa1[i], ya, ya1);
                    }
                }
            }
            if (live == 4) {
                unsigned out[C];
#pragma unroll
                for (int i = 0; i < C; ++i) out[i] = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int b = i * C + c;
                        out[b / 4] |= o[i][c] << (8 * (b % 4));
                    }
#pragma unroll
                for (int i = 0; i < C; ++i) __builtin_memcpy(d + 4 * i, &out[i], 4);
            } else {
                for (int i = 0; i < live; ++i)
#pragma unroll
                    for (int c = 0; c < C; ++c) d[i * C + c] = (uint8_t)o[i][c];
            }
        }
        if (out_hist) {
#pragma unroll
            for (int c = 0; c < C; ++c) add4(bins + c * 256, o[0][c], o[1][c], o[2][c], o[3][c], live);
        }
    }
    if (out_hist) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (bins[c * 256 + t]) atomicAdd(&out_hist[((size_t)page * C + c) * 256 + t], bins[c * 256 + t]);
    }
}

// grid = ceil(count / 64), 64 threads: the chain of 256 dependent steps, a lane per (page, channel)
__global__ __launch_bounds__(64) void k_equalize_derive(int count, const unsigned* __restrict__ hist, uint8_t* __restrict__ lut)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < count) equalize_lut(hist + (size_t)i * 256, lut + (size_t)i * 256);
}

// ---- host ------------------------------------------------------------------------------------------------------------------

struct ContrastSpec {
    bool clahe = false, equalize = false;
    int tiles_x = 8, tiles_y = 8;
    double clip_limit = 40.0;
};

// The checks of every entry, in the documented order (no device is touched).  oc: 0 for the entry without a destination.
int contrast_checks(const PageArgs& a, int channels, int oc, const ContrastSpec& sp, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, oc, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    if (sp.clahe && (sp.tiles_x < 1 || sp.tiles_x > kClaheMaxTiles || sp.tiles_y < 1 || sp.tiles_y > kClaheMaxTiles ||
                     sp.clip_limit != sp.clip_limit))
        return PRL_ERR_BAD_ARG;
    // in place: the same pointer at the same strides (a thread reads its pixels before it writes them)
    return batch ? pages_overlap_ok(a, channels, oc, true) : PRL_OK;
}

int clahe_hist_launch(int C, const PageSet& s, int n, int W, int H, const ClaheGeom& g, unsigned* hist, hipStream_t hs)
{
    const int tiles = g.tiles_x * g.tiles_y;
    PRL_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n * C * tiles * 256 * sizeof(unsigned), hs));
    const int bands = (g.tile_h + kClaheHistBandRows - 1) / kClaheHistBandRows;
    const int unit_px = g.tile_w * std::min(g.tile_h, kClaheHistBandRows);
    const int per_group = std::max(1, kClaheHistUnitPx / unit_px), units = tiles * bands;
    const dim3 grid((unsigned)((units + per_group - 1) / per_group), (unsigned)n), block(kClaheThreads);
    switch (C) {
    case 1: hipLaunchKernelGGL(k_clahe_hist<1>, grid, block, 0, hs, s, W, H, g, bands, per_group, hist); break;
    case 2: hipLaunchKernelGGL(k_clahe_hist<2>, grid, block, 0, hs, s, W, H, g, bands, per_group, hist); break;
    case 3: hipLaunchKernelGGL(k_clahe_hist<3>, grid, block, 0, hs, s, W, H, g, bands, per_group, hist); break;
    default: hipLaunchKernelGGL(k_clahe_hist<4>, grid, block, 0, hs, s, W, H, g, bands, per_group, hist); break;
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

int clahe_interp_launch(int C, const PageSet& s, const PageSetOut& d, int n, int W, int H, const ClaheGeom& g, const uint8_t* luts,
                        unsigned* out_hist, hipStream_t hs)
{
    if (out_hist) PRL_HIP_CHECK(hipMemsetAsync(out_hist, 0, (size_t)n * C * 256 * sizeof(unsigned), hs));
    const dim3 grid((unsigned)((W + kClaheBlockW - 1) / kClaheBlockW), (unsigned)((H + kClaheBlockH - 1) / kClaheBlockH), (unsigned)n);
    const dim3 block(kClaheThreads);
    switch (C) {
    case 1: hipLaunchKernelGGL(k_clahe_interp<1>, grid, block, 0, hs, s, d, W, H, g, luts, out_hist); break;
    case 2: hipLaunchKernelGGL(k_clahe_interp<2>, grid, block, 0, hs, s, d, W, H, g, luts, out_hist); break;
    case 3: hipLaunchKernelGGL(k_clahe_interp<3>, grid, block, 0, hs, s, d, W, H, g, luts, out_hist); break;
    default: hipLaunchKernelGGL(k_clahe_interp<4>, grid, block, 0, hs, s, d, W, H, g, luts, out_hist); break;
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// The workspace of a chunk of pages: [tile bins | tile tables | the pages' bins | the pages' tables], each block 256-byte aligned
struct ContrastWork {
    size_t p_thist, p_tlut, p_hist, p_lut;   // bytes per page
    size_t per_page() const { return p_thist + p_tlut + p_hist + p_lut + 4 * 256; }
    size_t bytes(int chunk) const { return r256(chunk * p_thist) + r256(chunk * p_tlut) + r256(chunk * p_hist) + r256(chunk * p_lut); }
};

ContrastWork contrast_work(int C, const ContrastSpec& sp, bool luts_out)
{
    const size_t tiles = sp.clahe ? (size_t)sp.tiles_x * sp.tiles_y : 0;
    ContrastWork cw;
    cw.p_thist = (size_t)C * tiles * 256 * sizeof(unsigned);
    cw.p_tlut = luts_out ? 0 : (size_t)C * tiles * 256;
    cw.p_hist = sp.equalize ? (size_t)C * 256 * sizeof(unsigned) : 0;
    cw.p_lut = sp.equalize ? (size_t)C * 256 : 0;
    return cw;
}

// n pages (at most the `chunk` the workspace `work` was sized for) from s into d; luts_out: the tile tables of these pages go
// there and no pixel is written.  Enqueues only.
int contrast_chunk(int C, const ContrastSpec& sp, const PageSet& s, const PageSetOut& d, int n, int W, int H, const ContrastWork& cw,
                   int chunk, uint8_t* work, uint8_t* luts_out, hipStream_t hs)
{
    const ClaheGeom g = clahe_geometry(W, H, sp.tiles_x, sp.tiles_y, sp.clip_limit);
    const size_t tiles = sp.clahe ? (size_t)sp.tiles_x * sp.tiles_y : 0;
    unsigned* d_thist = reinterpret_cast<unsigned*>(work);
    uint8_t* d_tlut = work + r256(chunk * cw.p_thist);
    unsigned* d_hist = reinterpret_cast<unsigned*>(d_tlut + r256(chunk * cw.p_tlut));
    uint8_t* d_lut = reinterpret_cast<uint8_t*>(d_hist) + r256(chunk * cw.p_hist);
    int st;
    if (sp.clahe) {
        st = clahe_hist_launch(C, s, n, W, H, g, d_thist, hs);
        if (st != PRL_OK) return st;
        uint8_t* tl = luts_out ? luts_out : d_tlut;
        const int n_tiles = (int)((size_t)n * C * tiles);
        hipLaunchKernelGGL(k_clahe_luts, dim3((unsigned)((n_tiles + 3) / 4)), dim3(kClaheThreads), 0, hs, n_tiles, g.clip, g.lut_scale,
                           d_thist, tl);
        PRL_HIP_CHECK(hipGetLastError());
        if (luts_out) return PRL_OK;
        st = clahe_interp_launch(C, s, d, n, W, H, g, tl, sp.equalize ? d_hist : nullptr, hs);
        if (st != PRL_OK) return st;
    } else {
        st = hist_launch(C, s, n, W, H, d_hist, hs);
        if (st != PRL_OK) return st;
    }
    if (!sp.equalize) return PRL_OK;
    hipLaunchKernelGGL(k_equalize_derive, dim3((unsigned)((n * C + 63) / 64)), dim3(64), 0, hs, n * C, d_hist, d_lut);
    PRL_HIP_CHECK(hipGetLastError());
    return lut_launch(C, C, sp.clahe ? as_source(d) : s, d, n, W, H, d_lut, (size_t)C * 256, hs);   // (in place after CLAHE)
}

// After the checks: CLAHE, equalization, or one after the other, on every channel of every page.  luts_out (the entry without a
// destination): the tile tables go to the caller's memory and no pixel is written.
int contrast_run(const PageArgs& a, int C, const ContrastSpec& sp, uint8_t* luts_out, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const size_t tiles = sp.clahe ? (size_t)sp.tiles_x * sp.tiles_y : 0;
    const ContrastWork cw = contrast_work(C, sp, luts_out != nullptr);
    const int chunk = stage_chunk(a.n_pages, cw.per_page());
    WorkScope w;
    int st = w.open(stream, cw.bytes(chunk), 0, 0);
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int n = std::min(chunk, a.n_pages - first);
        st = contrast_chunk(C, sp, src_pages(a, first), dst_pages(a, first), n, a.width, a.height, cw, chunk, w.scratch(),
                            luts_out ? luts_out + (size_t)first * C * tiles * 256 : nullptr, w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int contrast_device(const PageArgs& a, int channels, const ContrastSpec& sp, void* stream)
{
    const int st = contrast_checks(a, channels, channels, sp, true);
    return st != PRL_OK ? st : contrast_run(a, channels, sp, nullptr, stream);
}

int contrast_host(const PageArgs& h, int channels, const ContrastSpec& sp)
{
    const int st = contrast_checks(h, channels, channels, sp, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(h, channels, channels, h.width, h.height,
                            [&](const PageArgs& page, hipStream_t s) { return contrast_run(page, channels, sp, nullptr, s); });
}

ContrastSpec clahe_spec(double clip_limit, int tiles_x, int tiles_y, bool equalize)
{
    ContrastSpec sp;
    sp.clahe = true;
    sp.equalize = equalize;
    sp.tiles_x = tiles_x;
    sp.tiles_y = tiles_y;
    sp.clip_limit = clip_limit;
    return sp;
}

ContrastSpec equalize_spec()
{
    ContrastSpec sp;
    sp.equalize = true;
    return sp;
}

}  // namespace

// ---- what prl_internal.h declares of this file: EnhanceLocalContrastByCLAHE(clip_limit, equalize = true) on gray pages inside a
// caller's workspace (prl::binarizeLocalOtsu, localotsu.hip) ------
size_t enhance_contrast_work_bytes(int chunk) { return contrast_work(1, clahe_spec(40.0, 8, 8, true), false).bytes(chunk); }
size_t enhance_contrast_work_per_page() { return contrast_work(1, clahe_spec(40.0, 8, 8, true), false).per_page(); }
int enhance_contrast_gray_run(double clip_limit, const PageSet& s, const PageSetOut& d, int n, int W, int H, int chunk, uint8_t* work,
                              hipStream_t hs)
{
    const ContrastSpec sp = clahe_spec(clip_limit, 8, 8, true);
    return contrast_chunk(1, sp, s, d, n, W, H, contrast_work(1, sp, false), chunk, work, nullptr, hs);
}

// the same with C interleaved channels and either flag (prl::binarizeFBCITB, fbcitb.hip: three channels, no equalization), in place or not
size_t enhance_contrast_channels_work_bytes(int C, bool equalize, int chunk) { return contrast_work(C, clahe_spec(40.0, 8, 8, equalize), false).bytes(chunk); }
size_t enhance_contrast_channels_work_per_page(int C, bool equalize) { return contrast_work(C, clahe_spec(40.0, 8, 8, equalize), false).per_page(); }
int enhance_contrast_channels_run(int C, bool equalize, double clip_limit, const PageSet& s, const PageSetOut& d, int n, int W, int H, int chunk,
                                  uint8_t* work, hipStream_t hs)
{
    const ContrastSpec sp = clahe_spec(clip_limit, 8, 8, equalize);
    return contrast_chunk(C, sp, s, d, n, W, H, contrast_work(C, sp, false), chunk, work, nullptr, hs);
}

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_clahe_geometry(int width, int height, int tiles_x, int tiles_y, double clip_limit, int* tile_w, int* tile_h, int* ext_w,
                           int* ext_h, int* clip)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!tile_w || !tile_h || !ext_w || !ext_h || !clip || width > kStageMaxSide || height > kStageMaxSide || tiles_x < 1 ||
        tiles_x > kClaheMaxTiles || tiles_y < 1 || tiles_y > kClaheMaxTiles || clip_limit != clip_limit)
        return PRL_ERR_BAD_ARG;
    const ClaheGeom g = clahe_geometry(width, height, tiles_x, tiles_y, clip_limit);
    *tile_w = g.tile_w;
    *tile_h = g.tile_h;
    *ext_w = g.ext_w;
    *ext_h = g.ext_h;
    *clip = g.clip;
    return PRL_OK;
}

int prl_hip_clahe_tile_lut(const uint32_t hist[256], int clip, int tile_area, uint8_t lut[256])
{
    if (tile_area <= 0) return PRL_ERR_EMPTY;
    if (!hist || !lut || clip < 0) return PRL_ERR_BAD_ARG;
    unsigned long long total = 0;
    for (int v = 0; v < 256; ++v) total += hist[v];
    if (total != (unsigned long long)tile_area) return PRL_ERR_BAD_ARG;
    clahe_tile_lut(hist, clip, (float)255 / (float)tile_area, lut);
    return PRL_OK;
}

int prl_hip_equalize_hist_lut(const uint32_t hist[256], uint8_t lut[256])
{
    if (!hist || !lut) return PRL_ERR_BAD_ARG;
    unsigned long long total = 0;
    for (int v = 0; v < 256; ++v) total += hist[v];
    if (total == 0) return PRL_ERR_EMPTY;
    if (total > (unsigned long long)kStageMaxSide * kStageMaxSide) return PRL_ERR_BAD_ARG;
    equalize_lut(hist, lut);
    return PRL_OK;
}

int prl_hip_clahe_luts_batch_device(int n_pages, int channels, double clip_limit, int tiles_x, int tiles_y, const uint8_t* d_src,
                                    size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_luts, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, nullptr, 0, 0};
    const ContrastSpec sp = clahe_spec(clip_limit, tiles_x, tiles_y, false);
    const int st = contrast_checks(a, channels, 0, sp, true);
    if (st != PRL_OK) return st;
    if (!d_luts) return PRL_ERR_BAD_ARG;
    return contrast_run(a, channels, sp, d_luts, stream);
}

int prl_hip_clahe_batch_device(int n_pages, int channels, double clip_limit, int tiles_x, int tiles_y, const uint8_t* d_src,
                               size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                               size_t dst_step, void* stream)
{
    return contrast_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           clahe_spec(clip_limit, tiles_x, tiles_y, false), stream);
}

int prl_hip_clahe_host(int channels, double clip_limit, int tiles_x, int tiles_y, const uint8_t* src, size_t src_step, int width,
                       int height, uint8_t* dst, size_t dst_step)
{
    return contrast_host(PageArgs{1, src, 0, src_step, width, height, dst, 0, dst_step}, channels,
                         clahe_spec(clip_limit, tiles_x, tiles_y, false));
}

int prl_hip_equalize_hist_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                       int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return contrast_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           equalize_spec(), stream);
}

int prl_hip_equalize_hist_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    return contrast_host(PageArgs{1, src, 0, src_step, width, height, dst, 0, dst_step}, channels, equalize_spec());
}

int prl_hip_enhance_local_contrast_batch_device(int n_pages, int channels, double clip_limit, int equalize, const uint8_t* d_src,
                                                size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                                size_t dst_page_stride, size_t dst_step, void* stream)
{
    return contrast_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           clahe_spec(clip_limit, 8, 8, equalize != 0), stream);
}

int prl_hip_enhance_local_contrast_host(int channels, double clip_limit, int equalize, const uint8_t* src, size_t src_step, int width,
                                        int height, uint8_t* dst, size_t dst_step)
{
    return contrast_host(PageArgs{1, src, 0, src_step, width, height, dst, 0, dst_step}, channels,
                         clahe_spec(clip_limit, 8, 8, equalize != 0));
}

}  // extern "C"
