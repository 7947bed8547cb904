// page_args.h — the page arguments every stage entry shares (median, adaptive, gmorph, lines, tone, mokji, warp, bgnorm, pyr,
// canny, thinning, the local-variance binarizers, NL-means and denoise, the mask morphology, rotate, and the single-page *_host
// entries of all of them and of the binarizers), the checks made on them and the rule that cuts a batch into chunks of pages.
// Plain C++17: no HIP header, no environment, no I/O - tests/cpp/test_page_args.cpp drives it on the CPU.  An entry lists the
// check pieces in its own documented order, with its stage-specific checks in between (the older entries refuse source ==
// destination by pointer, or not at all, where the newer ones use pages_overlap_ok); every piece returns a PRL_* status and
// touches no device.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/prl_hip.h"

namespace prl_hip {

// n_pages pages of width x height pixels: page i of the source at src + i * src_page_stride, its rows src_step bytes apart;
// the same for the destination.  Not a kernel argument (those are PageSet / PageSetOut, prl_internal.h).
struct PageArgs {
    int n_pages;
    const uint8_t* src; size_t src_page_stride, src_step;
    int width, height;
    uint8_t* dst; size_t dst_page_stride, dst_step;
};

constexpr int kStageMaxSide = 32768;

inline size_t r256(size_t v) { return (v + 255) / 256 * 256; }   // sizes and offsets of 256-byte aligned blocks

inline int pages_nonempty(const PageArgs& a) { return a.width <= 0 || a.height <= 0 ? PRL_ERR_EMPTY : PRL_OK; }

// null pointers and steps below the row bytes; a negative page count where the entry takes one (`batch`).  out_channels == 0:
// the entry has no destination.
inline int pages_rows_ok(const PageArgs& a, int in_channels, int out_channels, bool batch)
{
    if (!a.src || (out_channels && !a.dst) || (batch && a.n_pages < 0)) return PRL_ERR_BAD_ARG;
    if (a.src_step < (size_t)a.width * in_channels || (out_channels && a.dst_step < (size_t)a.width * out_channels)) return PRL_ERR_BAD_ARG;
    return PRL_OK;
}

inline int pages_sides_ok(const PageArgs& a, int max_side = kStageMaxSide)
{
    return a.width > max_side || a.height > max_side ? PRL_ERR_BAD_ARG : PRL_OK;
}

// bytes from the first byte of page 0 to the last byte of the last page's last row (n_pages, height >= 1)
inline size_t pages_span(int n_pages, size_t page_stride, int height, size_t step, size_t row_bytes)
{
    return (size_t)(n_pages - 1) * page_stride + (size_t)(height - 1) * step + row_bytes;
}

inline bool ranges_overlap(const uint8_t* a, size_t a_bytes, const uint8_t* b, size_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

// In place: the same pointer at the same strides with as many channels out as in.
inline bool pages_in_place(const PageArgs& a, int in_channels, int out_channels)
{
    return out_channels == in_channels && a.src == a.dst && a.src_page_stride == a.dst_page_stride && a.src_step == a.dst_step;
}

// Source and destination of a batch must not share a byte, except in place where the entry allows it (its kernels then read
// a pixel before they write it).  Nothing to check without a destination or without pages.
inline int pages_overlap_ok(const PageArgs& a, int in_channels, int out_channels, bool allow_in_place)
{
    if (!out_channels || a.n_pages <= 0) return PRL_OK;
    if (allow_in_place && pages_in_place(a, in_channels, out_channels)) return PRL_OK;
    const size_t src_span = pages_span(a.n_pages, a.src_page_stride, a.height, a.src_step, (size_t)a.width * in_channels);
    const size_t dst_span = pages_span(a.n_pages, a.dst_page_stride, a.height, a.dst_step, (size_t)a.width * out_channels);
    return ranges_overlap(a.src, src_span, a.dst, dst_span) ? PRL_ERR_BAD_ARG : PRL_OK;
}

// Pages per launch: at most grid_limit (the grid dimension that counts pages) and at most budget_bytes of workspace at
// per_page_bytes a page, one page at least.  per_page_bytes == 0: the stage needs no workspace.
inline int pages_per_chunk(int n_pages, size_t per_page_bytes, size_t budget_bytes = (size_t)4 << 30, int grid_limit = 65535)
{
    const size_t chunk = (size_t)std::min(n_pages, grid_limit);
    if (!per_page_bytes) return (int)chunk;
    return (int)std::max<size_t>(1, std::min(chunk, budget_bytes / per_page_bytes));
}

}  // namespace prl_hip
