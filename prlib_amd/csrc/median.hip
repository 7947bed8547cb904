// median.hip — prl::denoiseSaltPepper (src/denoise/denoiseSaltPepper.cpp:29-36): `times` passes of cv::medianBlur(out, out, k).
//
// out(y, x, c) = the value at rank (k*k - 1) / 2 of in(clamp(y + i, 0, H-1), clamp(x + j, 0, W-1), c), |i|, |j| <= k/2
// (BORDER_REPLICATE, channels independent).  The result is an order statistic of bytes: every path below is exact.
//
// Two kernels, chosen by k (no user option; the hooks build forces the generic one with PRL_HIP_MEDIAN_GENERIC=1):
//   k_median_small<K, C, AL>  k = 3 and 5.  A lane owns 4 adjacent bytes of the interleaved row (a channel's horizontal
//                             neighbours are C bytes apart) and walks down kMedRows output rows.  It keeps the K source rows of
//                             its window as raw dwords in a ring, sorts each of the 4 + 2 (K/2) C columns once per output row
//                             (shared by the 4 outputs) and combines K sorted columns per output: k = 3 med3(max3 of the lows,
//                             med3 of the middles, min3 of the highs); k = 5 the 13 candidates that survive a row sort of the
//                             column-sorted 5 x 5 and a 39-comparator median-of-13 network.  Bytes become f32 (v_cvt_f32_ubyteN),
//                             compare in v_min3/v_med3/v_max3_f32 and go back with v_cvt_pk_u8_f32: all exact on 0..255.
//                             Lanes whose window crosses the row's ends are not launched as interior lanes: the last workgroup
//                             column of the grid computes those few bytes per row from clamped byte loads (same network).
//   k_median_hist<CT>         any odd k (k >= 7 by default).  A lane owns one byte column of a run of rows and keeps a 256-bin
//                             histogram of its window in LDS (Huang's sliding window: per output row one source row leaves and
//                             one enters; the median bin moves from the previous one).  Rows and columns outside the page add to
//                             the edge pixel's bin with their multiplicity, so a window larger than the page costs what the page
//                             costs.  Counters are 16-bit up to k = 255 (k^2 <= 65025) and 32-bit above: exact for every odd
//                             k up to kMedMaxK.
// One launch per pass for all pages of the call; passes alternate between d_dst and the device context's scratch so that the
// last one lands in d_dst.
#include "prl_internal.h"

#include <algorithm>

namespace prl_hip {

namespace {

constexpr int kMedWave = 64;
constexpr int kMedRows = 30;    // output rows per lane of k_median_small (a multiple of 3 and 5: the ring's slots stay static)
constexpr int kMedMaxK = 65535; // k^2 < 2^32

__device__ __forceinline__ void ce(float& a, float& b)
{
    const float lo = fminf(a, b);
    b = fmaxf(a, b);
    a = lo;
}

// sort K values ascending in place
template <int K> __device__ __forceinline__ void sort_k(float* v);
template <> __device__ __forceinline__ void sort_k<3>(float* v)
{
    const float lo = fminf(fminf(v[0], v[1]), v[2]), hi = fmaxf(fmaxf(v[0], v[1]), v[2]);
    v[1] = __builtin_amdgcn_fmed3f(v[0], v[1], v[2]);
    v[0] = lo;
    v[2] = hi;
}
template <> __device__ __forceinline__ void sort_k<5>(float* v)
{
    ce(v[0], v[1]); ce(v[3], v[4]); ce(v[2], v[4]); ce(v[2], v[3]); ce(v[1], v[4]);
    ce(v[0], v[3]); ce(v[0], v[2]); ce(v[1], v[3]); ce(v[1], v[2]);
}

// median of the K x K window given its K columns, each sorted ascending: col(j)[r]
template <int K> struct Combine;
template <> struct Combine<3> {
    template <typename F> __device__ __forceinline__ static float run(F col)
    {
        const float* a = col(0);
        const float* b = col(1);
        const float* c = col(2);
        const float lo = fmaxf(fmaxf(a[0], b[0]), c[0]);
        const float mi = __builtin_amdgcn_fmed3f(a[1], b[1], c[1]);
        const float hi = fminf(fminf(a[2], b[2]), c[2]);
        return __builtin_amdgcn_fmed3f(lo, mi, hi);
    }
};
template <> struct Combine<5> {
    // Sorting the rows of a column-sorted matrix keeps its columns sorted; then 6 entries are known to lie below rank 12 and 6
    // above, and the median is the median of the other 13 (row r keeps sorted positions 3-4, 2-4, 1-3, 0-2, 0-1).
    template <typename F> __device__ __forceinline__ static float run(F col)
    {
        float r[5][5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
#pragma unroll
            for (int j = 0; j < 5; ++j) r[i][j] = col(j)[i];
            sort_k<5>(r[i]);
        }
        float m[13] = {r[0][3], r[0][4], r[1][2], r[1][3], r[1][4], r[2][1], r[2][2], r[2][3],
                       r[3][0], r[3][1], r[3][2], r[4][0], r[4][1]};
        // Batcher's odd-even merge sort of 16 with the three +inf pads dropped, pruned to output 6 (checked on all 2^13 0/1 inputs)
        ce(m[0], m[1]); ce(m[2], m[3]); ce(m[4], m[5]); ce(m[6], m[7]); ce(m[8], m[9]); ce(m[10], m[11]);
        ce(m[0], m[2]); ce(m[1], m[3]); ce(m[4], m[6]); ce(m[5], m[7]); ce(m[8], m[10]); ce(m[9], m[11]);
        ce(m[1], m[2]); ce(m[5], m[6]); ce(m[9], m[10]);
        ce(m[0], m[4]); ce(m[1], m[5]); ce(m[2], m[6]); ce(m[3], m[7]); ce(m[8], m[12]);
        ce(m[2], m[4]); ce(m[3], m[5]); ce(m[10], m[12]);
        ce(m[1], m[2]); ce(m[3], m[4]); ce(m[5], m[6]); ce(m[9], m[10]); ce(m[11], m[12]);
        ce(m[0], m[8]); ce(m[1], m[9]); ce(m[2], m[10]); ce(m[3], m[11]); ce(m[4], m[12]);
        ce(m[4], m[8]); ce(m[5], m[9]); ce(m[6], m[10]);
        ce(m[3], m[5]); ce(m[6], m[8]);
        ce(m[5], m[6]);
        return m[6];
    }
};

__device__ __forceinline__ float ubyte(uint32_t w, int i)   // i is a constant after unrolling: one v_cvt_f32_ubyteN
{
    return (float)((w >> (8 * i)) & 255u);
}

// Bytes [4q, 4q + 4) of a row; the caller keeps q inside the row.  AL: row pointers are 4-byte aligned.
template <bool AL> __device__ __forceinline__ uint32_t load_dw(const uint8_t* row, int q)
{
    if (AL) return reinterpret_cast<const uint32_t*>(row)[q];
    const uint8_t* p = row + 4 * q;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Interior lanes: byte columns [4 qa, 4 qe), each lane 4 of them; the last workgroup column: the bytes [0, ia) and [ib, R)
// whose windows cross the row's ends.  grid = (interior workgroups + 1, ceil(H / kMedRows), pages).
template <int K, int C, bool AL>
__global__ __launch_bounds__(kMedWave) void k_median_small(PageSet src, PageSetOut dst, int W, int H, int qa, int qe, int ia,
                                                           int ib)
{
    constexpr int h = K / 2;
    constexpr int HALO = h;                 // dwords on each side: h * C <= 4 h bytes
    constexpr int ND = 2 * HALO + 1;
    constexpr int NCOL = 4 + 2 * h * C;     // byte columns the 4 outputs read
    constexpr int COL0 = 4 * HALO - h * C;  // window byte of column 0
    const int R = W * C;
    const int page = blockIdx.z;
    const uint8_t* sp = src.page(page);
    uint8_t* dp = dst.page(page);
    const int y0 = blockIdx.y * kMedRows;
    const int y1 = min(y0 + kMedRows, H);

    if (blockIdx.x == gridDim.x - 1) {
        // edge bytes: item = (row, byte) over the run's rows; clamped byte loads, the same column sort and combine
        const int ne = ia + (R - ib);
        const int items = ne * (y1 - y0);
        for (int it = threadIdx.x; it < items; it += kMedWave) {
            const int y = y0 + it / ne;
            int e = it - (it / ne) * ne;
            const int b = e < ia ? e : ib + (e - ia);
            const int x = b / C, c = b - (b / C) * C;
            float v[K][K];   // v[column][row]
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const uint8_t* row = sp + (size_t)min(max(y + i - h, 0), H - 1) * src.step;
#pragma unroll
                for (int j = 0; j < K; ++j) v[j][i] = (float)row[min(max(x + j - h, 0), W - 1) * C + c];
            }
#pragma unroll
            for (int j = 0; j < K; ++j) sort_k<K>(v[j]);
            const float m = Combine<K>::run([&](int j) { return v[j]; });
            dp[(size_t)y * dst.step + b] = (uint8_t)m;
        }
        return;
    }

    const int q = qa + blockIdx.x * kMedWave + threadIdx.x;
    if (q >= qe) return;
    uint32_t ring[K][ND];   // source row y0 - h + i lives in slot i % K
#pragma unroll
    for (int i = 0; i < K - 1; ++i) {
        const uint8_t* row = sp + (size_t)min(max(y0 - h + i, 0), H - 1) * src.step;
#pragma unroll
        for (int d = 0; d < ND; ++d) ring[i][d] = load_dw<AL>(row, q - HALO + d);
    }
    for (int yb = y0; yb < y1; yb += K) {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const int y = yb + s;
            if (y >= y1) break;
            {   // the window's new bottom row (source row y + h) goes to slot (s + K - 1) % K
                const uint8_t* row = sp + (size_t)min(y + h, H - 1) * src.step;
#pragma unroll
                for (int d = 0; d < ND; ++d) ring[(s + K - 1) % K][d] = load_dw<AL>(row, q - HALO + d);
            }
            float col[NCOL][K];
#pragma unroll
            for (int m = 0; m < NCOL; ++m) {
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const int wb = COL0 + m;   // window byte
                    col[m][i] = ubyte(ring[(s + i) % K][wb >> 2], wb & 3);
                }
                sort_k<K>(col[m]);
            }
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float m = Combine<K>::run([&](int jj) { return col[j + jj * C]; });
                out = __builtin_amdgcn_cvt_pk_u8_f32(m, j, out);
            }
            uint8_t* orow = dp + (size_t)y * dst.step;
            if (AL) {
                reinterpret_cast<uint32_t*>(orow)[q] = out;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) orow[4 * q + j] = (uint8_t)(out >> (8 * j));
            }
        }
    }
}

// Histogram path.  CT: counter type (uint16_t while k^2 < 2^16).  A lane owns byte column b = blockIdx.x * 64 + lane of rows
// [blockIdx.y * run, +run); hist[bin * 64 + lane] (lane-minor: a lane always hits bank lane % 32).
template <typename CT>
__global__ __launch_bounds__(kMedWave) void k_median_hist(PageSet src, PageSetOut dst, int W, int H, int C, int k, int run)
{
    __shared__ CT hist[256 * kMedWave];
    const int lane = threadIdx.x;
    const int R = W * C;
    const int b = blockIdx.x * kMedWave + lane;
    if (b >= R) return;   // (no barrier below: every lane owns its own bins)
    const uint8_t* sp = src.page(blockIdx.z);
    uint8_t* dp = dst.page(blockIdx.z);
    const int h = k / 2;
    const int x = b / C, c = b - (b / C) * C;
    const int y0 = blockIdx.y * run;
    const int y1 = min(y0 + run, H);
    CT* hl = hist + lane;
    for (int i = 0; i < 256; ++i) hl[i * kMedWave] = 0;

    // columns of the window: [xa, xb] inside the page, plus nl / nr positions clamped onto the first / last pixel
    const int xa = max(x - h, 0), xb = min(x + h, W - 1);
    const uint32_t nl = (uint32_t)max(h - x, 0), nr = (uint32_t)max(x + h - (W - 1), 0);
    uint32_t med = 0, lt = 0;   // current median bin, count of window values below it
    // adds (sign = +1) or removes (sign = -1, unsigned wrap) `weight` copies of source row yy's window columns
    auto row_update = [&](int yy, uint32_t weight, uint32_t sign) {
        const uint8_t* row = sp + (size_t)yy * src.step + c;
        for (int xx = xa; xx <= xb; ++xx) {
            uint32_t w = weight;
            if (xx == 0) w += weight * nl;
            if (xx == W - 1) w += weight * nr;
            const uint32_t v = row[xx * C];
            w *= sign;
            hl[v * kMedWave] = (CT)(hl[v * kMedWave] + (CT)w);
            if (v < med) lt += w;
        }
    };
    const uint32_t t = ((uint32_t)k * (uint32_t)k - 1u) / 2u;
    auto settle = [&]() {
        for (;;) {
            if (lt > t) {
                --med;
                lt -= (uint32_t)hl[med * kMedWave];
            } else {
                const uint32_t here = (uint32_t)hl[med * kMedWave];
                if (lt + here <= t) {
                    lt += here;
                    ++med;
                } else {
                    break;
                }
            }
        }
    };
    {   // the window of row y0: rows [ya, yb] inside the page, plus the rows clamped onto the first / last one
        const int ya = max(y0 - h, 0), yb = min(y0 + h, H - 1);
        const uint32_t nt = (uint32_t)max(h - y0, 0), nb = (uint32_t)max(y0 + h - (H - 1), 0);
        for (int yy = ya; yy <= yb; ++yy) {
            uint32_t w = 1;
            if (yy == 0) w += nt;
            if (yy == H - 1) w += nb;
            row_update(yy, w, 1u);
        }
    }
    settle();
    dp[(size_t)y0 * dst.step + b] = (uint8_t)med;
    for (int y = y0 + 1; y < y1; ++y) {
        row_update(max(y - 1 - h, 0), 1u, 0xffffffffu);
        row_update(min(y + h, H - 1), 1u, 1u);
        settle();
        dp[(size_t)y * dst.step + b] = (uint8_t)med;
    }
}

// ksize == 1, times == 0 and the first copy of an in-place call with an odd number of passes: 4 bytes per lane, byte access
// (strides and pointers of any alignment)
__global__ __launch_bounds__(256) void k_median_copy(PageSet src, PageSetOut dst, int R)
{
    const int b = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (b >= R) return;
    const uint8_t* s = src.page(blockIdx.z) + (size_t)blockIdx.y * src.step + b;
    uint8_t* d = dst.page(blockIdx.z) + (size_t)blockIdx.y * dst.step + b;
    const int n = min(4, R - b);
    for (int i = 0; i < n; ++i) d[i] = s[i];
}

struct MedGeom {
    int W, H, C, k;
    int qa, qe, ia, ib;   // k_median_small's interior dwords [qa, qe) and edge bytes [0, ia), [ib, R)
};

MedGeom med_geom(int W, int H, int C, int k)
{
    MedGeom g{W, H, C, k, 0, 0, 0, 0};
    const int R = W * C, halo = k / 2;
    g.qa = halo;
    g.qe = std::max(g.qa, R / 4 - halo);
    g.ia = std::min(4 * g.qa, R);
    g.ib = std::min(4 * g.qe, R);
    return g;
}

bool aligned4(const void* p, size_t a, size_t b) { return ((reinterpret_cast<uintptr_t>(p) | a | b) & 3u) == 0; }

template <int K, int C>
void launch_small(const MedGeom& g, const PageSet& s, const PageSetOut& d, int n, hipStream_t stream)
{
    const int nb_in = (g.qe - g.qa + kMedWave - 1) / kMedWave;
    const dim3 grid((unsigned)(nb_in + 1), (unsigned)((g.H + kMedRows - 1) / kMedRows), (unsigned)n);
    if (aligned4(s.base, s.step, s.page_stride) && aligned4(d.base, d.step, d.page_stride))
        hipLaunchKernelGGL((k_median_small<K, C, true>), grid, dim3(kMedWave), 0, stream, s, d, g.W, g.H, g.qa, g.qe, g.ia, g.ib);
    else
        hipLaunchKernelGGL((k_median_small<K, C, false>), grid, dim3(kMedWave), 0, stream, s, d, g.W, g.H, g.qa, g.qe, g.ia, g.ib);
}

template <int K>
void launch_small_c(const MedGeom& g, const PageSet& s, const PageSetOut& d, int n, hipStream_t stream)
{
    switch (g.C) {
    case 1: launch_small<K, 1>(g, s, d, n, stream); break;
    case 2: launch_small<K, 2>(g, s, d, n, stream); break;
    case 3: launch_small<K, 3>(g, s, d, n, stream); break;
    default: launch_small<K, 4>(g, s, d, n, stream); break;
    }
}

int median_pass(const MedGeom& g, bool generic, const PageSet& s, const PageSetOut& d, int n, hipStream_t stream)
{
    if (!generic && g.k == 3) {
        launch_small_c<3>(g, s, d, n, stream);
    } else if (!generic && g.k == 5) {
        launch_small_c<5>(g, s, d, n, stream);
    } else {
        const int run = std::min(g.H, std::max(32, 2 * g.k));
        const dim3 grid((unsigned)((g.W * g.C + kMedWave - 1) / kMedWave), (unsigned)((g.H + run - 1) / run), (unsigned)n);
        if (g.k <= 255)
            hipLaunchKernelGGL(k_median_hist<uint16_t>, grid, dim3(kMedWave), 0, stream, s, d, g.W, g.H, g.C, g.k, run);
        else
            hipLaunchKernelGGL(k_median_hist<uint32_t>, grid, dim3(kMedWave), 0, stream, s, d, g.W, g.H, g.C, g.k, run);
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

int median_copy(const PageSet& s, const PageSetOut& d, int R, int H, int n, hipStream_t stream)
{
    const dim3 grid((unsigned)((R + 1023) / 1024), (unsigned)H, (unsigned)n);
    hipLaunchKernelGGL(k_median_copy, grid, dim3(256), 0, stream, s, d, R);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// one chunk of pages; `tmp`: R * H bytes per page (tight rows), needed when times >= 2 or the call is in place
int median_run(const MedGeom& g, size_t times, const PageSet& src, const PageSetOut& dst, int n, bool in_place, uint8_t* tmp,
               hipStream_t stream)
{
    const int R = g.W * g.C;
    if (g.k == 1 || times == 0) return in_place ? PRL_OK : median_copy(src, dst, R, g.H, n, stream);
    const PageSetOut t = page_set_out(tmp, (size_t)R * g.H, (size_t)R);
    const PageSet ts = as_source(t), ds = as_source(dst);
    const bool generic = env_knobs().median_generic;
    PageSet cur = src;
    int st = PRL_OK;
    if (in_place && (times & 1)) {   // pass 1 must not write the pages it reads: start from a copy
        st = median_copy(src, t, R, g.H, n, stream);
        if (st != PRL_OK) return st;
        cur = ts;
    }
    for (size_t i = 1; i <= times; ++i) {
        const bool to_dst = ((times - i) & 1) == 0;   // the last pass lands in d_dst
        st = median_pass(g, generic, cur, to_dst ? dst : t, n, stream);
        if (st != PRL_OK) return st;
        cur = to_dst ? ds : ts;
    }
    return PRL_OK;
}

// the checks of both entries, in the documented order (no device is touched); batch: the *_batch_device entry
int median_checks(const PageArgs& a, int channels, int ksize, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (ksize < 1 || (ksize & 1) == 0) return PRL_ERR_BAD_WINDOW;             // cv::medianBlur: ksize % 2 == 1
    if (channels < 1 || channels > 4 || (channels == 2 && ksize >= 7)) return PRL_ERR_BAD_CHANNELS;   // k > 5: cn 1, 3, 4
    if ((st = pages_rows_ok(a, channels, channels, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK || ksize > kMedMaxK) return PRL_ERR_BAD_ARG;
    // in place: the same pages at the same strides; any other overlap of source and destination is refused
    return batch ? pages_overlap_ok(a, channels, channels, true) : PRL_OK;
}

int median_batch_device(int channels, int ksize, size_t times, const PageArgs& a, void* stream)
{
    int st = median_checks(a, channels, ksize, true);
    if (st != PRL_OK) return st;
    if (a.n_pages == 0) return PRL_OK;
    const bool work = ksize > 1 && times > 0;
    const bool in_place = pages_in_place(a, channels, channels);
    const bool need_tmp = work && (times >= 2 || in_place);
    const MedGeom g = med_geom(a.width, a.height, channels, ksize);
    const size_t page_bytes = (size_t)a.width * channels * (size_t)a.height;
    // pages per launch: grid.z, and at most 4 GiB of scratch (one page at least)
    const int chunk = stage_chunk(a.n_pages, need_tmp ? page_bytes : 0);
    WorkScope w;
    st = w.open(stream, need_tmp ? page_bytes * (size_t)chunk : 0, 0, 0);
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        st = median_run(g, work ? times : 0, src_pages(a, first), dst_pages(a, first), std::min(chunk, a.n_pages - first), in_place,
                        need_tmp ? w.scratch() : nullptr, w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

// one pass over pages that the caller owns (adaptive.hip; the source is not the destination, the caller holds the device)
int median_pass_pages(int width, int height, int channels, int ksize, const PageSet& src, const PageSetOut& dst, int n_pages,
                      hipStream_t stream)
{
    return median_pass(med_geom(width, height, channels, ksize), env_knobs().median_generic, src, dst, n_pages, stream);
}

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_median_batch_device(int n_pages, int channels, int ksize, size_t times, const uint8_t* d_src, size_t src_page_stride,
                                size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                void* stream)
{
    return median_batch_device(channels, ksize, times,
                               PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, stream);
}

int prl_hip_median_host(int channels, int ksize, size_t times, const uint8_t* src, size_t src_step, int width, int height,
                        uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = median_checks(a, channels, ksize, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, channels, width, height,
                            [&](const PageArgs& page, hipStream_t s) { return median_batch_device(channels, ksize, times, page, s); });
}

}  // extern "C"
