// CPU test of prlib_amd/csrc/page_args.h (the page arguments, check pieces and chunk rule the stage entries share): every
// expected status and count is worked out by hand from the rules - two byte ranges overlap iff they share a byte; the span of
// a batch ends with the last row of its last page; in place means the same pointer, strides and channel count - not taken
// from the code under test.  No pointer is dereferenced.  Built by tests/cpp/Makefile (g++).
#include <cstdio>

#include "../../prlib_amd/csrc/page_args.h"

using namespace prl_hip;

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++bad; } } while (0)

static uint8_t arena[1 << 16];   // addresses only

// 3 pages of 10 x 4 gray pixels, rows 16 bytes apart, pages 100 bytes apart: the source ends 2 * 100 + 3 * 16 + 10 = 258 bytes in
static PageArgs base()
{
    return PageArgs{3, arena, 100, 16, 10, 4, arena + 258, 100, 16};
}

int main()
{
    {   // the span of a batch, of one page, of one row
        CHECK(pages_span(3, 100, 4, 16, 10) == 258);
        CHECK(pages_span(1, 100, 4, 16, 10) == 58);     // the page stride of a single page does not count
        CHECK(pages_span(1, 1 << 20, 4, 16, 10) == 58);
        CHECK(pages_span(3, 100, 1, 16, 10) == 210);    // nor the step of a single row
        CHECK(pages_span(1, 100, 1, 1 << 20, 10) == 10);
    }
    {   // the predicate: adjacent ranges do not overlap, one shared byte does (either way round)
        CHECK(!ranges_overlap(arena, 258, arena + 258, 258));
        CHECK(!ranges_overlap(arena + 258, 258, arena, 258));
        CHECK(ranges_overlap(arena, 259, arena + 258, 258));
        CHECK(ranges_overlap(arena + 258, 258, arena, 259));
        CHECK(ranges_overlap(arena, 258, arena + 100, 1));   // one inside the other
    }
    {   // source and destination of a batch
        PageArgs a = base();
        CHECK(pages_overlap_ok(a, 1, 1, true) == PRL_OK);          // the destination starts right behind the source
        a.dst = arena + 257;
        CHECK(pages_overlap_ok(a, 1, 1, true) == PRL_ERR_BAD_ARG); // one byte shared
        a.dst = arena + 258;
        a.src = arena + 1;
        CHECK(pages_overlap_ok(a, 1, 1, false) == PRL_ERR_BAD_ARG);
        a = base();
        a.src = arena + 258 + 258;                                  // the source right behind the destination
        CHECK(pages_overlap_ok(a, 1, 1, false) == PRL_OK);
        a.src = arena + 258 + 257;
        CHECK(pages_overlap_ok(a, 1, 1, false) == PRL_ERR_BAD_ARG);
        // three channels in, one out, source rows 32 bytes apart: the source ends 2 * 100 + 3 * 32 + 30 = 326 bytes in
        a = PageArgs{3, arena, 100, 32, 10, 4, arena + 326, 100, 16};
        CHECK(pages_overlap_ok(a, 3, 1, true) == PRL_OK);
        a.dst = arena + 325;
        CHECK(pages_overlap_ok(a, 3, 1, true) == PRL_ERR_BAD_ARG);
        // n_pages == 1 and height == 1: 10 bytes each, whatever the strides
        a = PageArgs{1, arena, 1 << 20, 1 << 20, 10, 1, arena + 10, 1 << 20, 1 << 20};
        CHECK(pages_overlap_ok(a, 1, 1, false) == PRL_OK);
        a.dst = arena + 9;
        CHECK(pages_overlap_ok(a, 1, 1, false) == PRL_ERR_BAD_ARG);
        // no pages: nothing is read or written
        a.n_pages = 0;
        CHECK(pages_overlap_ok(a, 1, 1, false) == PRL_OK);
    }
    {   // in place: equal pointer, page stride, step and channel count, and only where the entry allows it
        PageArgs a = base();
        a.dst = arena;
        CHECK(pages_overlap_ok(a, 1, 1, true) == PRL_OK);
        CHECK(pages_overlap_ok(a, 3, 3, true) == PRL_OK);
        CHECK(pages_overlap_ok(a, 1, 1, false) == PRL_ERR_BAD_ARG);
        CHECK(pages_overlap_ok(a, 3, 1, true) == PRL_ERR_BAD_ARG);   // fewer channels out than in
        CHECK(pages_overlap_ok(a, 4, 3, true) == PRL_ERR_BAD_ARG);
        a.dst_page_stride = 101;
        CHECK(pages_overlap_ok(a, 1, 1, true) == PRL_ERR_BAD_ARG);
        a = base();
        a.dst = arena;
        a.dst_step = 17;
        CHECK(pages_overlap_ok(a, 1, 1, true) == PRL_ERR_BAD_ARG);
        a = base();
        a.dst = arena + 1;
        CHECK(pages_overlap_ok(a, 1, 1, true) == PRL_ERR_BAD_ARG);
    }
    {   // out_channels == 0: no destination, and none of its checks
        PageArgs a = base();
        a.dst = nullptr;
        a.dst_page_stride = a.dst_step = 0;
        CHECK(pages_rows_ok(a, 1, 0, true) == PRL_OK);
        CHECK(pages_overlap_ok(a, 1, 0, true) == PRL_OK);
        CHECK(pages_overlap_ok(a, 1, 0, false) == PRL_OK);
        CHECK(pages_rows_ok(a, 1, 1, true) == PRL_ERR_BAD_ARG);      // with a destination the null pointer counts
        a.dst = arena;                                               // ... and on top of the source it is still no destination
        CHECK(pages_overlap_ok(a, 1, 0, false) == PRL_OK);
    }
    {   // pointers, the page count, steps at and one below the row bytes
        PageArgs a = base();
        CHECK(pages_rows_ok(a, 1, 1, true) == PRL_OK);
        a.src = nullptr;
        CHECK(pages_rows_ok(a, 1, 1, true) == PRL_ERR_BAD_ARG);
        a = base();
        a.n_pages = -1;
        CHECK(pages_rows_ok(a, 1, 1, true) == PRL_ERR_BAD_ARG);
        CHECK(pages_rows_ok(a, 1, 1, false) == PRL_OK);              // a *_host entry has no page count
        a.n_pages = 0;
        CHECK(pages_rows_ok(a, 1, 1, true) == PRL_OK);
        a = base();
        a.src_step = 30;                                             // 10 pixels of 3 channels
        a.dst_step = 10;
        CHECK(pages_rows_ok(a, 3, 1, true) == PRL_OK);
        a.src_step = 29;
        CHECK(pages_rows_ok(a, 3, 1, true) == PRL_ERR_BAD_ARG);
        a.src_step = 30;
        a.dst_step = 9;
        CHECK(pages_rows_ok(a, 3, 1, true) == PRL_ERR_BAD_ARG);
        CHECK(pages_rows_ok(a, 3, 0, true) == PRL_OK);               // no destination: its step does not count
        a.dst_step = 29;
        CHECK(pages_rows_ok(a, 3, 3, true) == PRL_ERR_BAD_ARG);
        a.dst_step = 30;
        CHECK(pages_rows_ok(a, 3, 3, true) == PRL_OK);
    }
    {   // empty pages and the side limit
        PageArgs a = base();
        CHECK(pages_nonempty(a) == PRL_OK);
        a.width = 0;
        CHECK(pages_nonempty(a) == PRL_ERR_EMPTY);
        a = base();
        a.height = -1;
        CHECK(pages_nonempty(a) == PRL_ERR_EMPTY);
        a = base();
        a.width = 32768;
        a.height = 32768;
        CHECK(kStageMaxSide == 32768);
        CHECK(pages_sides_ok(a) == PRL_OK);
        a.width = 32769;
        CHECK(pages_sides_ok(a) == PRL_ERR_BAD_ARG);
        a.width = 1;
        a.height = 32769;
        CHECK(pages_sides_ok(a) == PRL_ERR_BAD_ARG);
        a.height = 32768;
        CHECK(pages_sides_ok(a, 32767) == PRL_ERR_BAD_ARG);          // an entry's own limit
        a.height = 32767;
        CHECK(pages_sides_ok(a, 32767) == PRL_OK);
    }
    {   // pages per chunk
        const size_t G4 = (size_t)4 << 30;
        CHECK(pages_per_chunk(5, 0) == 5);                           // no workspace: the grid limit alone
        CHECK(pages_per_chunk(65535, 0) == 65535);
        CHECK(pages_per_chunk(65536, 0) == 65535);
        CHECK(pages_per_chunk(100000, 0, 0, 16384) == 16384);
        CHECK(pages_per_chunk(100, 0, 0, 16384) == 100);
        CHECK(pages_per_chunk(7, G4 + 1) == 1);                      // a page above the budget: one page at least
        CHECK(pages_per_chunk(1, G4 + 1) == 1);
        CHECK(pages_per_chunk(100, (size_t)1 << 30) == 4);           // exact division: 4 GiB / 1 GiB
        CHECK(pages_per_chunk(100, ((size_t)1 << 30) + 1) == 3);
        CHECK(pages_per_chunk(3, (size_t)1 << 30) == 3);             // fewer pages than the budget holds
        CHECK(pages_per_chunk(100000, 1) == 65535);                  // the budget holds more than the grid takes
        CHECK(pages_per_chunk(100, 1000, 3000, 65535) == 3);         // another budget
        CHECK(pages_per_chunk(100, 1000, 2999, 65535) == 2);
        CHECK(pages_per_chunk(2, 1000, 3000, 65535) == 2);
    }
    if (bad) {
        std::printf("page_args: %d check(s) failed\n", bad);
        return 1;
    }
    std::printf("page_args: OK\n");
    return 0;
}
