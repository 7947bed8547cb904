// prl_internal.h — shared host-side declarations of libprlib_hip.so (not part of the public ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <vector>
#include <string>

#include "../../include/prl_hip.h"
#include "page_args.h"

namespace prl_hip {

// ---- error plumbing -----------------------------------------------------------------------
void set_error_detail(const std::string& s);

#define PRL_HIP_CHECK(expr)                                                                       \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            ::prl_hip::set_error_detail(std::string(#expr) + ": " + hipGetErrorString(_e));       \
            return (_e == hipErrorOutOfMemory) ? PRL_ERR_NOMEM : PRL_ERR_HIP;                     \
        }                                                                                         \
    } while (0)

struct StreamWs;  // per-(device, stream) workspace of the binarizers (prl_capi.hip)

// ---- per-device context: cached scratch memory ------------------------------------------------
struct DeviceCtx {
    std::mutex streams_mu;  // guards `streams` only (never held across device work: deskew holds `mu` for seconds)
    std::map<hipStream_t, std::unique_ptr<StreamWs>> streams;  // the entries have their own locks
    ~DeviceCtx();
    std::mutex mu;          // one call at a time per device on the shared workspace (scratch, small, pinned)
    int device = -1;
    void* scratch = nullptr;   // page-sized work planes of the batch entries (bgnorm, LV, thinning, NL-means, median, morph, gmorph)
    size_t scratch_bytes = 0;
    void* small = nullptr;  // counters / work lists / per-page globals
    size_t small_bytes = 0;
    std::mutex stage_mu;    // one *_host call at a time per device (taken before `mu`)
    void* stage = nullptr;  // device staging of the *_host entry points (page in + page out)
    size_t stage_bytes = 0;
    void* stage_pinned = nullptr;  // pinned host bounce buffer of the *_host entry points (same lock)
    size_t stage_pinned_bytes = 0;
    std::vector<hipEvent_t> stage_events;  // one per download band (same lock)
    // NL-means weight tables already resident in `small` (slot 0 / 1): rebuilt only when (channels, h) or `small` change
    int lut_channels[2] = {0, 0};
    float lut_h[2] = {0.f, 0.f};
    int lut_n[2] = {0, 0};
    const void* lut_small[2] = {nullptr, nullptr};
    void* pinned = nullptr; // pinned host staging for tiny transfers
    size_t pinned_bytes = 0;
    int cu_count = 0;
    hipEvent_t prof_start = nullptr, prof_stop = nullptr;  // prl_hip_set_profiling
    bool prof_valid = false;
    hipEvent_t last_use = nullptr;  // last use of scratch / small / pinned: a WorkScope waits on it when it opens and records it when it ends
    hipEvent_t stage_use = nullptr; // same for the staging area (`stage`): recorded by its last user (guarded by stage_mu)
    hipEvent_t pinned_use = nullptr; // the last asynchronous copy OUT of `pinned` (warp.hip's page records): the host waits for it before it overwrites the block (guarded by mu)
    // The angle search of prl::deskew has its own workspace, lock and stream: in the chain it runs for the next pass
    // while the other stages of the current one use `scratch` / `small` (glue.hip).
    std::mutex ppht_mu;
    // fixed part (masks, lists' layout ...), point / segment lists, gray pages, the group kernel's workspace (ppht_group.hip),
    // accumulators in device memory (k_ppht_mw, for the pages the group kernel did not take), cv::RNG's output
    static constexpr int kPphtBufs = 6;
    void* ppht_buf[kPphtBufs] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t ppht_bytes[kPphtBufs] = {0, 0, 0, 0, 0, 0};
    size_t ppht_rnd_n = 0;          // numbers of cv::RNG(-1)'s sequence resident in ppht_buf[5]
    hipStream_t host_run = nullptr; // stream of prl_hip_chain_batch_host's device work (kept: its per-stream workspaces persist)
    // page buffers and pinned bounce slots of prl_hip_chain_batch_host, kept between calls (allocating and freeing tens of
    // gigabytes per call cost two seconds); one such call at a time per device
    std::mutex host_mu;
    void* host_buf[4] = {nullptr, nullptr, nullptr, nullptr};  // in 0 / 1, out 0 / 1
    size_t host_buf_bytes[4] = {0, 0, 0, 0};
    void* host_slots[2] = {nullptr, nullptr};   // PinSlots of host_batch.hip (replaced when they grow, never freed at exit)
    void* host_bin = nullptr;                   // HostBin of host_batch.hip: streams and chunk slots of prl_hip_binarize_batch_host (same lock)
    void* chain_planes = nullptr;   // Lab planes of a whole chain pass (split mode of glue.hip; guarded by stage_mu)
    size_t chain_planes_bytes = 0;
    hipStream_t side = nullptr;     // created on first use (non-blocking)
    hipEvent_t side_ev = nullptr;
};

// Knobs of the PRL_* environment variables, read ONCE (first use) instead of on every call.  The product library reads the
// user-facing ones (PRL_HIP_DEBUG, PRL_HIP_MODE, the memory budgets *_MB, the copy-thread counts); the kernel-selection and
// schedule knobs below keep their defaults unless the library is built with -DPRL_TEST_HOOKS (libprlib_hip_testhooks.so,
// `make hooks`: what tests/ and tools/ load for A/B runs and for forcing rarely taken paths).
struct EnvKnobs {
    int fused_wpb = 1;            // PRL_HIP_WPB          wavefronts per workgroup of k_fused (1..4)
    bool flt = true;              // PRL_HIP_FLT=0        forces the integer sum pipeline everywhere
    bool nt_store = true;         // PRL_HIP_NT=0         plain instead of non-temporal mask stores
    int rows_per_seg = 0;         // PRL_HIP_ROWS_PER_SEG (0 = chosen from the batch size)
    bool tiers = true;            // PRL_HIP_TIERS=0      one segment length for the whole call (A/B of the tiered schedule)
    bool ext_strip = true;        // PRL_HIP_EXT_STRIP=0  no extended last strip (binarize_fused.hip strip_layout)
    int fused_qint = 2;           // PRL_HIP_FUSED_QINT=0 windows of 33..129 columns stay on k_fused's integer loop (1: k_fused_q for interior strips only, 2: border strips too)
    bool ragged_uo = true;        // PRL_HIP_RAGGED_UO=0  outputs per strip always a multiple of 8
    bool wolf_side = true;        // PRL_HIP_WOLF_SIDE=0  Wolf-Jolion on one stream, the threshold sweep after the literal devianceMax (round-3 schedule)
    int wolf_tier_max = 128;      // PRL_HIP_WOLF_TIER_MAX longest row segment of a tiered Wolf-Jolion call (profiles/r03/wolf_tier_max.txt)
    bool debug = false;           // PRL_HIP_DEBUG
    bool byte_mask = false;       // PRL_HIP_BYTE_MASK    byte instead of bit-plane hand-off to the morphology pass
    int morph_rps = 0, morph_wpb = 1;   // PRL_MORPH_RPS, PRL_MORPH_WPB
    int thin_rps = 0, thin_wpb = 4;     // PRL_THIN_RPS, PRL_THIN_WPB
    int nlm_xl = 3;               // PRL_NLM_XL
    int nlm_glut = 0;             // PRL_NLM_GLUT   bit 0 / 1: L / ab plane read the weight table from memory instead of LDS
    size_t literal_scratch_mb = 8192;   // PRL_HIP_LITERAL_SCRATCH_MB
    size_t deskew_work_mb = 24576;      // PRL_HIP_DESKEW_WORK_MB
    int ppht_mw = -1;                   // PRL_HIP_PPHT_MW   1 / 0: always / never three wavefronts per page (default: by batch size)
    int ppht_prio = 3;                  // PRL_HIP_PPHT_PRIO=0   k_ppht does not raise its wavefront priority
    int ppht_group = -1;                // PRL_HIP_PPHT_GROUP    1 / 0: always (where a page qualifies) / never the on-chip group kernel (ppht_group.hip)
    int ppht_group_g = 1;               // PRL_HIP_PPHT_GROUP_G  at least this many workgroups per page
    int ppht_group_xcd = 0;             // PRL_HIP_PPHT_GROUP_XCD=1   a group's members on one XCD (workgroups b, b + 8, ...) instead of consecutive ids: 24 instead of 28 groups of 9, no faster exchange
    int ppht_group_spin_ms = 10000;     // PRL_HIP_PPHT_GROUP_SPIN_MS how long a member waits for its group before the group gives up
    int ppht_group_kill = -1;           // PRL_HIP_PPHT_GROUP_KILL=n  (tests) member 1 of group 0 falls silent after n exchanges
    int ppht_group_cus = 0;             // PRL_HIP_PPHT_GROUP_CUS     workgroups of the group kernel at most (0: one per CU)
    int chain_pass = 0, chain_first_pass = 0;   // PRL_HIP_CHAIN_PASS / PRL_HIP_CHAIN_FIRST_PASS   pages per pass of the chain with deskew (0: start at 192 with denoise, then follow the measured search / NL-means times; else 256)
    int chain_overlap = 2;              // PRL_HIP_CHAIN_OVERLAP   0: passes one after the other; 1: the search of the next pass beside all stages
                                        //                         of this one; 2: beside its NL-means kernels only (head / body / tail, glue.hip)
    size_t chain_work_mb = 49152;       // PRL_HIP_CHAIN_WORK_MB
    size_t host_chunk_mb = 128;         // PRL_HIP_HOST_CHUNK_MB   pages staged per buffer of prl_hip_binarize_batch_host
    int chain_host_pages = 0;           // PRL_HIP_CHAIN_HOST_PAGES   pages per device chunk of prl_hip_chain_batch_host (0: from the budget)
    size_t chain_host_mb = 65536;       // PRL_HIP_CHAIN_HOST_MB      device memory for the page buffers of prl_hip_chain_batch_host
    int fake_devices = 0;               // PRL_HIP_FAKE_DEVICES   (tests) logical devices of the *_batch_host entries, mapped onto the real ones
    int host_copy_threads = 0;          // PRL_HIP_HOST_COPY_THREADS  threads of the pool that copies pageable pages in / out of pinned memory (0: half of the cores, at most 32)
    unsigned segmax_cap = 1u << 20;     // PRL_HIP_SEGMAX_CAP   wavefronts per Wolf-Jolion call (tests shrink it)
    bool force_exact = false;           // PRL_HIP_FORCE_EXACT=1  (tests) every page whose fix-up list did not overflow is redone by the exact sweep (resolve_front)
    int literal_mode = 0;         // PRL_HIP_MODE=literal
    bool median_generic = false;  // PRL_HIP_MEDIAN_GENERIC=1  the histogram kernel for every window (median.hip), k = 3 and 5 included
    bool gmorph_literal = false;  // PRL_HIP_GMORPH_LITERAL=1  the by-the-definition kernel for every element (gmorph.hip)
    bool lines_bytes = false;     // PRL_HIP_LINES_BYTES=1     removeLines' openings on byte masks through k_gm_span (lines.hip)
    int stage_chunk_pages = 0;    // PRL_HIP_STAGE_CHUNK=n     (tests) the stage entries take at most n pages per chunk (stage_chunk below; 0: off)
    int bgnorm_lds_map = 60000;   // PRL_HIP_BGNORM_LDS_MAP=n  (tests) the largest map in bytes k_bg_maps copies into LDS (bgnorm.hip; 0: every map stays in global memory)
    bool lo_host_rects = true;    // PRL_HIP_LO_HOST_RECTS=0   binarizeLocalOtsu takes its rectangles from components.hip instead of reading its edge maps back for the host scan (contour.h): the A/B of the two paths (the device path measured no faster: profiles/r24/INDEX.md)
    int cc_pass = 1 << 20;        // PRL_HIP_CC_PASS=n         (tests) components per statistics pass of components.hip
};
const EnvKnobs& env_knobs();

// While alive, binarize calls of this thread only enqueue (as with prl_hip_set_deferred_completion(1)); the owner calls
// prl_hip_finish(stream) itself.
class DeferredScope {
public:
    DeferredScope();
    ~DeferredScope();
private:
    bool prev_;
};

int current_device(int* dev);             // validates that a gfx950 device is usable
DeviceCtx* device_ctx(int dev);
inline int current_ctx(DeviceCtx** ctx)   // the two in sequence: the current device's context
{
    int dev;
    const int st = current_device(&dev);
    if (st == PRL_OK) *ctx = device_ctx(dev);
    return st;
}
// Grow-only cached buffers, one pair per memory kind: device (hipMalloc) and pinned host (hipHostMalloc).  A buffer that has to
// grow is freed once the whole device has drained, then allocated anew; free_* leave {nullptr, 0} behind.
int ensure_buffer(void** buf, size_t* have, size_t bytes);
int ensure_host_buffer(void** buf, size_t* have, size_t bytes);
hipError_t free_buffer(void** buf, size_t* have);
hipError_t free_host_buffer(void** buf, size_t* have);
int ensure_scratch(DeviceCtx* ctx, size_t bytes);
int ensure_small(DeviceCtx* ctx, size_t bytes);   // at least 1 MiB
int ensure_pinned(DeviceCtx* ctx, size_t bytes);  // at least 64 KiB
// The shared device workspace (scratch, small, pinned) serves every stream of the device, one call at a time: a WorkScope,
// which alone takes `mu`, makes its stream wait for the previous user's work (device_acquire) before the first write and records
// its own work as the new last use when it ends.
int device_acquire(DeviceCtx* ctx, hipStream_t stream);
// One call on the shared workspace, from the checks' end to the return, in two steps.  lock() takes the current device (lock_on():
// the context its caller already holds) and `mu`; grow() sizes the blocks the call asks for (0 bytes: not needed), drops NL-means'
// cached tables whenever `small` is asked for (its head is about to be overwritten; NL-means itself passes kKeepNlmTables) and
// makes the stream wait for the previous user.  open() / open_on() are the two in sequence; an entry that may still refuse its arguments
// after the device check, before anything is allocated, calls them apart (thin.hip).  On every exit after a successful grow(),
// error exits included, the call's work is recorded as the new last use before `mu` is released.
// Not on it, each with a workspace and lock of its own: deskew.hip's host_roundtrip (its own buffers, a result size per page),
// and the angle search under `ppht_mu` (ppht.hip; deskew_find and deskew_ink_census of deskew.hip), which the chain runs beside
// the stages that are on it.  The deskew, find_angle and houghp entries do share the check pieces of page_args.h.
enum class NlmTables { kDrop, kKeep };   // (a type of its own: no size can be passed in its place)
constexpr NlmTables kKeepNlmTables = NlmTables::kKeep;
class WorkScope {
public:
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    void lock_on(DeviceCtx* c, hipStream_t s)
    {
        ctx = c;
        stream = s;
        lk_ = std::unique_lock<std::mutex>(ctx->mu);
    }
    int lock(void* stream_arg)
    {
        int dev;
        const int st = current_device(&dev);
        if (st == PRL_OK) lock_on(device_ctx(dev), static_cast<hipStream_t>(stream_arg));
        return st;
    }
    int grow(size_t scratch_bytes, size_t small_bytes, size_t pinned_bytes, NlmTables tables = NlmTables::kDrop)
    {
        int st;
        if (scratch_bytes && (st = ensure_scratch(ctx, scratch_bytes)) != PRL_OK) return st;
        if (small_bytes && (st = ensure_small(ctx, small_bytes)) != PRL_OK) return st;
        if (pinned_bytes && (st = ensure_pinned(ctx, pinned_bytes)) != PRL_OK) return st;
        if (small_bytes && tables == NlmTables::kDrop) ctx->lut_small[0] = ctx->lut_small[1] = nullptr;
        st = device_acquire(ctx, stream);
        acquired_ = st == PRL_OK;
        return st;
    }
    int open(void* stream_arg, size_t scratch_bytes, size_t small_bytes, size_t pinned_bytes, NlmTables tables = NlmTables::kDrop)
    {
        const int st = lock(stream_arg);
        return st != PRL_OK ? st : grow(scratch_bytes, small_bytes, pinned_bytes, tables);
    }
    int open_on(DeviceCtx* c, hipStream_t s, size_t scratch_bytes, size_t small_bytes, size_t pinned_bytes, NlmTables tables = NlmTables::kDrop)
    {
        lock_on(c, s);
        return grow(scratch_bytes, small_bytes, pinned_bytes, tables);
    }
    ~WorkScope() { if (acquired_) (void)hipEventRecord(ctx->last_use, stream); }   // (lk_ is released after this body)
    template <typename T = uint8_t> T* scratch() const { return static_cast<T*>(ctx->scratch); }
    template <typename T = uint8_t> T* small() const { return static_cast<T*>(ctx->small); }
    template <typename T = uint8_t> T* pinned() const { return static_cast<T*>(ctx->pinned); }
private:
    std::unique_lock<std::mutex> lk_;
    bool acquired_ = false;
};
// Pages per chunk of a stage entry: pages_per_chunk (page_args.h), capped by the test hook PRL_HIP_STAGE_CHUNK - the one place
// that reads it - so that a handful of small pages runs the second chunk's offsets of every entry.
inline int stage_chunk(int n_pages, size_t per_page_bytes, size_t budget_bytes = (size_t)4 << 30, int grid_limit = 65535)
{
    const int chunk = pages_per_chunk(n_pages, per_page_bytes, budget_bytes, grid_limit), cap = env_knobs().stage_chunk_pages;
    return cap > 0 ? std::min(chunk, cap) : chunk;
}
int ensure_stage(DeviceCtx* ctx, size_t bytes);  // caller holds stage_mu
// The staging area is shared by every stream of the device: a user makes its stream wait for the previous user's work
// (stage_acquire) before the first write and records its own work at the end (stage_release).  Caller holds stage_mu.
int stage_acquire(DeviceCtx* ctx, hipStream_t stream);
int stage_release(DeviceCtx* ctx, hipStream_t stream);
struct StageRelease {   // records the area's new last use on every exit of the scope, error exits included
    DeviceCtx* c; hipStream_t s;
    ~StageRelease() { (void)stage_release(c, s); }
};
// Host image <-> device staging through the cached pinned bounce buffer (caller holds stage_mu).  hipMemcpy2D from
// pageable memory runs at ~1 GB/s on this stack; row memcpy into pinned memory + one DMA is an order faster.
// `pin_off`: byte offset inside the bounce buffer (so an upload and a download can share it).
int stage_upload(DeviceCtx* ctx, size_t pin_off, const uint8_t* src, size_t src_step, size_t row_bytes, int rows,
                 uint8_t* d_dst, hipStream_t stream);                      // rows packed tightly on the device
int stage_download(DeviceCtx* ctx, size_t pin_off, const uint8_t* d_src, size_t row_bytes, int rows, uint8_t* dst,
                   size_t dst_step, hipStream_t stream);                  // synchronises `stream`
int ensure_stage_pinned(DeviceCtx* ctx, size_t bytes);
bool host_range_pinned(const void* p, size_t bytes);   // pinned host memory: the DMA engines may use it directly

// The *_host entries may start a DMA straight from / into the CALLER's pinned pixels (stage_upload / stage_download).  Whatever
// way such an entry returns - also early, on an error of a later step - nothing may still be reading or writing that memory:
// the stream is drained at scope exit (a no-op after the success path's own wait).
struct DrainOnExit {
    hipStream_t s;
    ~DrainOnExit() { (void)hipStreamSynchronize(s); }
};

// ---- page addressing: contiguous batch or table of page pointers ---------------------------------
struct PageSet {
    const uint8_t* base = nullptr;   // page i at base + i*page_stride ...
    size_t page_stride = 0;
    const uint8_t* const* table = nullptr;  // ... unless a DEVICE array of page pointers is given
    size_t step = 0;
    __host__ __device__ const uint8_t* page(int i) const {
        return table ? table[i] : base + (size_t)i * page_stride;
    }
};
struct PageSetOut {
    uint8_t* base = nullptr;
    size_t page_stride = 0;
    uint8_t* const* table = nullptr;
    size_t step = 0;
    __host__ __device__ uint8_t* page(int i) const {
        return table ? table[i] : base + (size_t)i * page_stride;
    }
};
// Host helpers (free functions: both sets are kernel arguments and stay plain aggregates).  page_table*: `table` is a DEVICE array.
inline PageSet page_set(const uint8_t* base, size_t page_stride, size_t step) { return PageSet{base, page_stride, nullptr, step}; }
inline PageSetOut page_set_out(uint8_t* base, size_t page_stride, size_t step) { return PageSetOut{base, page_stride, nullptr, step}; }
inline PageSet page_table(const uint8_t* const* table, size_t step) { return PageSet{nullptr, 0, table, step}; }
inline PageSetOut page_table_out(uint8_t* const* table, size_t step) { return PageSetOut{nullptr, 0, table, step}; }
inline PageSet as_source(const PageSetOut& d) { return PageSet{d.base, d.page_stride, d.table, d.step}; }   // an output set re-read
// the same set starting `first` pages later (a null base stays null: the entry checks answer for it)
template <typename Set>
inline Set pages_from(Set s, int first)
{
    if (s.table) s.table += first;
    else if (s.base) s.base += (size_t)first * s.page_stride;
    return s;
}
// the pages of a stage entry's arguments from page `first` on
inline PageSet src_pages(const PageArgs& a, int first) { return pages_from(page_set(a.src, a.src_page_stride, a.src_step), first); }
inline PageSetOut dst_pages(const PageArgs& a, int first) { return pages_from(page_set_out(a.dst, a.dst_page_stride, a.dst_step), first); }

// A single-page *_host stage entry after its checks: the page `h` describes (host pointers; in_channels / out_channels bytes per
// pixel, the result out_width x out_height) goes through the device.  Under stage_mu the cached staging area holds [in | out] at
// 256-byte offsets, rows packed tightly; the source goes up, then
//     int run(const PageArgs& page, hipStream_t stream)
// gets the staging area as a one-page batch of the same width and height on the null stream, and the result comes down into h.dst.
// An entry whose result is not a page leaves h.dst null (and the three out_* zero): no [out], a null destination, no download.
template <typename Run>
int stage_host_pages(const PageArgs& h, int in_channels, int out_channels, int out_width, int out_height, Run&& run)
{
    int dev;
    int st = current_device(&dev);
    if (st != PRL_OK) return st;
    DeviceCtx* ctx = device_ctx(dev);
    const size_t in_row = (size_t)h.width * in_channels, out_row = (size_t)out_width * out_channels;
    const size_t in_bytes = r256(in_row * (size_t)h.height), out_bytes = h.dst ? r256(out_row * (size_t)out_height) : 0;
    std::lock_guard<std::mutex> slk(ctx->stage_mu);  // cached device + pinned staging: no allocation per page (lock order: stage_mu, then mu)
    st = ensure_stage(ctx, in_bytes + out_bytes);
    if (st != PRL_OK) return st;
    st = ensure_stage_pinned(ctx, in_bytes + out_bytes);
    if (st != PRL_OK) return st;
    uint8_t* d_in = static_cast<uint8_t*>(ctx->stage);
    uint8_t* d_out = h.dst ? d_in + in_bytes : nullptr;
    const hipStream_t stream = nullptr;
    DrainOnExit drain_guard{stream};
    st = stage_upload(ctx, 0, h.src, h.src_step, in_row, h.height, d_in, stream);
    if (st != PRL_OK) return st;
    st = run(PageArgs{1, d_in, in_bytes, in_row, h.width, h.height, d_out, out_bytes, out_row}, stream);
    if (st != PRL_OK || !h.dst) return st;
    return stage_download(ctx, in_bytes, d_out, out_row, out_height, h.dst, h.dst_step, stream);
}

// Threshold constants shared by the literal and fused kernels (host-prepared, passed by value).
struct ThrParams {
    int method;
    int w;         // effective window
    int half;
    int width, height;      // unpadded page
    int pw, ph;             // padded page
    int ow, oh;             // output
    double f;      // 1.0 / (double)(w*w)                  binarizeSauvola.cpp:58-59
    double k;
    double a, b;   // Sauvola: k*(1/128), 1-k             binarizeSauvola.cpp:117
    double c1;     // Feng: 1 - alpha1                    binarizeFeng.cpp:133
    double k2;     // Feng
    double gamma;  // Feng
};
ThrParams make_thr_params(const prl_binarize_params* p, const prl_binarize_geometry& g, int width, int height);   // prl_capi.hip

// Per-page globals living in device memory (Wolf-Jolion / Feng reductions, fix-up bookkeeping).
struct PageGlobals {
    int imin;                       // min over the page (cv::minMaxLoc(imageInput), binarizeWolfJolion.cpp:116)
    int smax_found;                 // any non-NaN deviation seen
    unsigned long long smax_bits;   // bit pattern of max deviation (>= +0, so integer order == value order)
    double coeff;                   // k / devianceMax             binarizeWolfJolion.cpp:121
    unsigned int n_refined;         // pixels decided by the float64 interval test
    unsigned int n_exact;           // pixels sent to the absolute-integral fix-up
    unsigned int worklist_overflow; // bit 0: the refine queue overflowed (too many pixels inside the float32 band: the exact sweep redoes the page); bit 1: the fix-up list or Wolf-Jolion's candidate list overflowed (the literal pipeline redoes it)
    unsigned int v32max_bits;       // Wolf fused sweep A: float32 bits of the page's largest variance estimate
    unsigned int n_cand;            // Wolf: candidate pixels for the literal devianceMax (sweep B; statistics)
    unsigned int need_literal;      // Wolf: a pixel of this page reached the literal fix-up -> the literal devianceMax is computed (lazily)
    unsigned long long kmax_bits;   // Wolf: exact integer maximum of K = w^2 Q - S^2 over the output region (sweep B)
    double coeff_rel;               // Wolf: |k / devianceMax_literal - coeff| <= coeff_rel |coeff| (coeff = k / (f sqrt(Kmax)) until need_literal)
    unsigned int cand_overflow;     // Wolf: the candidate list overflowed: the literal devianceMax is not available for this page
    unsigned int reserved0;
};

// ---- literal pipeline (binarize_literal.hip) ---------------------------------------------------
size_t literal_scratch_per_page(const ThrParams& tp);
int literal_run(const ThrParams& tp, const PageSet& src, int first_page, int n_pages,
                const PageSetOut& dst, void* scratch, PageGlobals* d_globals, hipStream_t stream);

// ---- fused pipeline (binarize_fused.hip) -------------------------------------------------------
// Counter block at the start of the fused work area: words 0..63 = list lengths and the epilogue's arrival counter, then
// one counter per refine-queue bucket on its own 128-byte line (kRefBuckets of them): every queued pixel costs a device-scope
// atomic, and 4 * 10^5 of them on ONE address serialised (2.8 ns each: the threshold sweep of 256 real 4K scans took 4.27 ms
// instead of 3.18) - a wavefront adds to the bucket its id selects.
constexpr int kRefBuckets = 256;
constexpr int kRefCounterStride = 32;                                             // words
constexpr int kFusedCounterWords = 64 + kRefBuckets * kRefCounterStride;
constexpr size_t kFusedCounterBytes = ((size_t)kFusedCounterWords * 4 + 255) / 256 * 256;
// Wolf-Jolion's side stream (per workspace): the literal devianceMax - candidate sweep, absolute corner sums of the
// candidates, k / devianceMax - and the page minimum of the border bands run here, beside the two big sweeps on the caller's
// stream (see fused_run).
struct WolfSide {
    hipStream_t stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_min = nullptr, ev_a = nullptr, ev_coeff = nullptr;
};
size_t fused_small_bytes(int n_pages);
struct FusedCall {   // the arguments of fused_run, filled by field name
    ThrParams tp{};
    PageSet src{};
    PageSetOut dst{};
    int n_pages = 0;
    void* small = nullptr;               // the fused work area, fused_small_bytes(n_pages) bytes
    PageGlobals* d_globals = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // optional: recorded around the threshold sweep
    bool bit_out = false;                // dst is a bit plane (rows of dst.step bytes, 1 bit per output pixel) instead of a 0/255 byte mask
    bool counters_zeroed = false;        // the counter block at the start of `small` is already zero
    PageGlobals* host_globals = nullptr; // (pinned, n_pages entries): see FusedParams::ep_host
    const WolfSide* wolf_side = nullptr;
    bool exact = false;                  // the second chance of flagged pages (k_fused_exact: the float64 interval test inline, no queue)
};
int fused_run(const FusedCall& c);
bool fused_supports(const ThrParams& tp);
int fused_max_pages(const ThrParams& tp);  // pages one fused_run call can take (Wolf-Jolion: per-wavefront maxima storage)

// ---- thinning (thin.hip): the C entry plus the option to thin cv::bitwise_not of the source (chain glue) ------
// (arguments as checked by prl_hip_thin_batch_device; n_pages >= 1)
int thin_batch_device(int method, int n_pages, const PageSet& src, int width, int height, const PageSetOut& dst, void* stream,
                      bool invert_input);

// ---- prl::denoise in three parts (nlm.hip; the chain separates its streaming parts from its compute part), each one
// WorkScope on ctx ----------------
size_t denoise_plane_bytes(int width, int height);   // per page: L, ab, L', ab'
int denoise_convert_in(DeviceCtx* ctx, int cnt, int channels, const PageSet& src, int width, int height, uint8_t* planes, hipStream_t s);
int denoise_nlm(DeviceCtx* ctx, int cnt, float strength, uint8_t* planes, int width, int height, hipStream_t s);
int denoise_convert_out(DeviceCtx* ctx, int cnt, int channels, const uint8_t* planes, int width, int height, const PageSetOut& dst,
                        hipStream_t s);

// ---- prl::rotate (rotate.hip): one record per page, as the host fills it and k_warp / k_rot90 read it ------
struct WarpPage {
    double M[6];   // the inverted matrix warpAffine works with
    int kind;      // 0 warp, 1/2/3 = 90/180/270, 4 = copy (deskew without an angle)
    int ow, oh;
};
// the record of a width x height page turned by `angle` degrees (copy: left as it is), its result size included
void fill_warp_page(int width, int height, double angle, bool copy, WarpPage* wp);
// every page by its record (d_wp: device); max_ow x max_oh: the largest result.  any_quarter = false: no page is of kind 1 / 3.
// Enqueues only.
int launch_warp(int channels, const PageSet& s, const PageSetOut& d, int width, int height, int n_pages, int max_ow, int max_oh,
                const WarpPage* d_wp, hipStream_t stream, bool any_quarter = true);

// ---- HoughLinesP and findAngle (ppht.hip) ------
// Otsu's threshold of n_pages 1-channel pages into d_thr, by way of their histograms (d_hist: 256 words per page); enqueues only
int otsu_thresholds(const PageSet& gray, int width, int height, int n_pages, unsigned* d_hist, int* d_thr, hipStream_t stream);
struct SearchStart;
// The segments findAngle's cv::HoughLinesP(1, CV_PI/180, 100, width/8.f, 20) finds on `cnt` 1-channel pages (a contiguous batch),
// per page in `lines` (host, 4 ints each).  Points are the pixels at or below the page's Otsu threshold (prl::deskew's gray page)
// or, otsu = false, below 255 (findAngle's binarized page).  Synchronises `hs`; the caller holds ctx->ppht_mu.
int find_angle_segments(DeviceCtx* ctx, int cnt, const PageSet& gray, int width, int height, bool otsu,
                        std::vector<std::vector<int>>* lines, hipStream_t hs, SearchStart* start);
double vote_angle(const int* segments, int n_segments);   // findAngle's vote over one page's segments, in degrees

// ---- deskew (deskew.hip): one pass over `cnt` pages, as its two halves (the chain overlaps them) or in one go ------
int deskew_pages_per_pass(int n_pages, int width, int height);
struct DeskewPlan {                   // what the angle search of a pass hands to its rotation
    std::vector<WarpPage> warp;       // one record per page
    std::vector<int32_t> wh;          // result size per page
    std::vector<double> angles;       // findAngle's degrees per page
    int max_ow = 0, max_oh = 0;
};
// gray -> Otsu -> HoughLinesP -> vote on `hs` (synchronises it); own workspace, takes ctx->ppht_mu only
// Lets a caller order its own work behind the START of the search's long kernel (the Hough transform): deskew_find records
// `ev` on the search's stream right before it launches that kernel - the event completes when the streaming prelude (gray, Otsu,
// point lists) is through - and then calls launched().  wait() returns true once that has happened, false when the search
// ended without getting there (finish() is called by whoever ran deskew_find).
struct SearchStart {
    hipEvent_t ev = nullptr;
    bool prefer_mw = false;   // this search runs beside compute-bound work that needs the CUs (the chain's NL-means) and would hide behind it: take k_ppht_mw (accumulators in device memory, no LDS) instead of the group kernel
    std::mutex mu;
    std::condition_variable cv;
    bool recorded = false, done = false;
    void reset() { std::lock_guard<std::mutex> lk(mu); recorded = done = false; }
    void launched() { { std::lock_guard<std::mutex> lk(mu); recorded = true; } cv.notify_all(); }
    void finish() { { std::lock_guard<std::mutex> lk(mu); done = true; } cv.notify_all(); }
    bool wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return recorded || done; }); return recorded; }
};
// (the page sets of the deskew functions are contiguous batches: base + page_stride, no pointer table)
int deskew_find(DeviceCtx* ctx, int cnt, int channels, const PageSet& src, int width, int height, DeskewPlan* plan, hipStream_t hs,
                SearchStart* start = nullptr);
// dark pixels (<= the page's Otsu threshold) per page = the points HoughLinesP will visit; takes ctx->ppht_mu, synchronises hs
int deskew_ink_census(DeviceCtx* ctx, int n_pages, int channels, const PageSet& src, int width, int height,
                      std::vector<unsigned>* points, hipStream_t hs);
// prl::rotate of every page by its angle (copy where none was found); one WorkScope on ctx
int deskew_apply(DeviceCtx* ctx, const DeskewPlan& plan, int cnt, int channels, const PageSet& src, int width, int height,
                 const PageSetOut& dst, hipStream_t hs);
int deskew_pages(DeviceCtx* ctx, int cnt, int channels, const PageSet& src, int width, int height, const PageSetOut& dst,
                 int32_t* out_wh, double* angles, hipStream_t hs);
// One page at a time host -> device -> host around a device-side stage whose result has a size of its own (the *_host entries of
// deskew, rotate and find_angle): h describes the host page; `stage` gets it as a one-page batch in buffers of this call's own,
// the destination max_w x max_h, and leaves the result's size in *out_w / *out_h, against which h.dst_step is then checked.
// h.dst null: nothing comes down (no destination for the stage, out_w / out_h unused).  Takes stage_mu around the two copies.
int host_roundtrip(const PageArgs& h, int channels, int max_w, int max_h, const int* out_w, const int* out_h,
                   const std::function<int(const PageArgs&, hipStream_t)>& stage);
// The lists of one pass of the search (ppht.hip), device pointers into its workspace and the host arrays that travel with them
// (alive until the stream has been synchronised): what the point stage leaves to HoughLinesP's second stage, whichever kernel runs it.
struct PphtPass {
    uint8_t* d_mask = nullptr; size_t mask_page = 0;                // byte masks (k_dark_mask)
    unsigned* d_nz = nullptr; unsigned long long* d_nzoff = nullptr; unsigned* d_count = nullptr;   // point list, a page's start, its points
    const unsigned long long* h_nzoff = nullptr; const unsigned* h_count = nullptr;
    float* d_ttab = nullptr; const float* h_ttab = nullptr;         // kNumAngle x {cos, sin}
    int* d_lines = nullptr; unsigned long long* d_lnoff = nullptr; unsigned* d_cap = nullptr; unsigned* d_nlines = nullptr;   // segment list, a page's start, its room, segments found
    const unsigned long long* h_lnoff = nullptr; const unsigned* h_cap = nullptr;
};
// ppht_group.hip: HoughLinesP's second stage with the accumulator in LDS, a group of workgroups per page.
struct PphtGroupIn {
    int n_pages = 0, width = 0, height = 0, threshold = 0, line_length = 0, line_gap = 0;
    PphtPass pass;
    std::vector<int> page_list;          // pages to process, heaviest first
    int cu_limit = 0;                    // workgroups at most (0: one per CU)
    hipEvent_t ev[2] = {nullptr, nullptr};   // optional: recorded before / after the group kernel (diagnostics)
    unsigned* status_out = nullptr;      // host, n_pages: 1 = finished by the group kernel (valid after the stream sync)
    unsigned long long* prof_out = nullptr;   // host, 16 per page (optional)
    int geometry_out[4] = {0, 0, 0, 0};  // members per group, groups, workgroups, LDS bytes
    std::vector<unsigned char> keep;     // host tables the asynchronous copies read
};
bool ppht_group_eligible(int width, int height, int threshold);
int ppht_group_run(DeviceCtx* ctx, PphtGroupIn& in, hipStream_t stream);
// glue.hip: pages per pass of the chain and its workspace bytes per page (host_batch.hip sizes device chunks in whole passes)
int chain_pass_layout(const prl_chain_params* cp, int n_pages, int channels, int width, int height, int* pass_pages,
                      size_t* per_page_out, size_t* desk_page_out);
void host_slots_free(DeviceCtx* ctx);  // host_batch.hip: the pinned bounce slots of prl_hip_chain_batch_host (caller holds host_mu)

// ---- median (median.hip): one cv::medianBlur pass, odd ksize >= 3, source and destination distinct; enqueues only ----------
int median_pass_pages(int width, int height, int channels, int ksize, const PageSet& src, const PageSetOut& dst, int n_pages,
                      hipStream_t stream);

// ---- flat-element morphology (gmorph.hip): OPEN with a kw x kh rectangle (1..255 each way) on 1-channel pages of a contiguous
// batch, source and destination distinct; `tmp`: n_pages * width * height bytes; enqueues only (caller holds ctx->mu) ----------
int gmorph_open_rect_run(int kw, int kh, int width, int height, const PageSet& src, const PageSetOut& dst, int n_pages, uint8_t* tmp,
                         hipStream_t stream);
// DILATE with a k x k rectangle (k odd, 3..255), anchor at the centre: the same conditions and `tmp` (binarizeMokji, mokji.hip)
int gmorph_dilate_rect_run(int k, int width, int height, const PageSet& src, const PageSetOut& dst, int n_pages, uint8_t* tmp,
                           hipStream_t stream);
// CLOSE with a k x k rectangle, default anchor, `iterations` times, IN PLACE on the 1-channel pages a DEVICE table of page
// pointers names (rows `step` bytes apart): the border detector's retry on the pages without a quad (border.hip).  `tmp`:
// 2 * n_pages * width * height bytes; enqueues only (caller holds ctx->mu)
int gmorph_close_rect_table_run(int k, int iterations, int width, int height, uint8_t* const* d_table, size_t step, int n_pages,
                                uint8_t* tmp, hipStream_t stream);

// ---- the host thread pool (host_batch.hip): the page copies of the host-list entries and the per-page host work of the stage
// entries (the quad search of prl::documentContour) share it; parallel_for(n, f) as prl/work_pool.h states ----------
void host_pool_for(int n, const std::function<void(int)>& f);
int host_pool_threads();

// ---- cv::pyrDown (pyr.hip): `levels` >= 1 pyramid levels of n pages of 1..4 channels into `dst` (pages of the last level's size);
// `work`: n * pyr_work_per_page bytes for the levels between; enqueues only (caller holds ctx->mu) ----------
size_t pyr_work_per_page(int width, int height, int channels, int levels);
int pyr_run(int channels, const PageSet& src, int width, int height, int levels, const PageSetOut& dst, int n_pages, uint8_t* work,
            hipStream_t stream);
// the destination of an entry whose result is out_width x out_height: its rows, and no byte shared with the source
int resized_dst_ok(const PageArgs& a, int channels, int out_width, int out_height, bool batch);

// ---- cv::Canny (canny.hip) of n pages (a chunk) of W x H: 1 channel, or 3 / 4 with the colour rule of prl::findHoughLineContour,
// into 0 / 255 maps.  work: canny_work_bytes(n, W, H); h_flags: pinned, canny_pinned_bytes(n).  Synchronises the stream (caller
// holds ctx->mu).  canny_pages_per_chunk: the pages a chunk takes when a page costs extra_per_page bytes beside Canny's own ------
size_t canny_work_bytes(int n, int W, int H);
size_t canny_pinned_bytes(int n);
int canny_pages_per_chunk(int n_pages, int W, int H, size_t extra_per_page);
// d_page_t (device, n ints in 0 .. 255) with d_lut (device, 256 pairs): page i takes the thresholds d_lut[2 t], d_lut[2 t + 1] of its
// t = d_page_t[i] instead of low / high (CannyEdgeDetection: the pair follows the page's Otsu value, which never leaves the device)
int canny_run(int W, int H, int low, int high, const PageSet& src, const PageSetOut& dst, int n, uint8_t* work, unsigned* h_flags,
              hipStream_t stream, int channels = 1, const int* d_lut = nullptr, const int* d_page_t = nullptr);
// lut[2 t], lut[2 t + 1] = cv::Canny's integer pair for threshold2 = upper_coeff * t, threshold1 = lower_coeff * threshold2, t = 0 .. 255
void canny_threshold_table(double upper_coeff, double lower_coeff, int* lut);

// ---- the 8-bit separable filter (blur8.hip): wx / wy are nx / ny 8.8 weights in tap order, each side summing to at most 256; n
// pages of 1..4 channels, source and destination distinct; needs no workspace; enqueues only ----------
int sep_filter_u8_batch(const uint16_t* wx, int nx, const uint16_t* wy, int ny, const PageArgs& a, int channels, hipStream_t stream);

// ---- cv::bilateralFilter (bilateral.hip): every channel of n pages of 1..4 channels as a plane of its own, with the tables of
// bilateral.h; source and destination distinct; needs no workspace; enqueues only ----------
struct BilTables;
int bilateral_planes_run(const BilTables& t, const PageArgs& a, int channels, hipStream_t stream);

// ---- CannyEdgeDetection (edgedet.hip; imageLibCommon.cpp:244-324) of n pages (a chunk) of C channels into 0 / 255 maps.  work:
// ced_work_bytes; small: ced_small_bytes; h_flags: pinned, ced_pinned_bytes.  Synchronises the stream (caller holds ctx->mu).
// ced_pages_per_chunk: the pages a chunk takes when a page costs extra_per_page bytes beside the stage's own ------
struct CedSpec {
    int size;                          // GaussianBlurKernelSize
    double upper_coeff, lower_coeff;   // CannyUpperThresholdCoeff, CannyLowerThresholdCoeff
    int iterations;                    // CannyMorphIters
};
int ced_spec_check(const CedSpec& sp);   // 0, or the number of the reference's check that fails (5: an even size)
int ced_pages_per_chunk(const CedSpec& sp, int n_pages, int W, int H, int C, size_t extra_per_page);
size_t ced_work_bytes(const CedSpec& sp, int n, int W, int H, int C);
size_t ced_small_bytes(int n, int C);
size_t ced_pinned_bytes(int n, int C);
int ced_run(const CedSpec& sp, const PageSet& src, const PageSetOut& dst, int n, int W, int H, int C, uint8_t* work, uint8_t* small,
            unsigned* h_flags, hipStream_t stream);

// ---- EnhanceLocalContrastByCLAHE(clip_limit, equalize = true) on n gray pages inside a caller's workspace (clahe.hip), in place
// or not; work: enhance_contrast_work_bytes(chunk) for the chunk the n pages are part of; enqueues only ----------
size_t enhance_contrast_work_bytes(int chunk);
size_t enhance_contrast_work_per_page();
int enhance_contrast_gray_run(double clip_limit, const PageSet& src, const PageSetOut& dst, int n, int W, int H, int chunk, uint8_t* work,
                              hipStream_t stream);

// the same on pages of C interleaved channels, with or without the equalization (prl::binarizeFBCITB)
size_t enhance_contrast_channels_work_bytes(int C, bool equalize, int chunk);
size_t enhance_contrast_channels_work_per_page(int C, bool equalize);
int enhance_contrast_channels_run(int C, bool equalize, double clip_limit, const PageSet& src, const PageSetOut& dst, int n, int W, int H,
                                  int chunk, uint8_t* work, hipStream_t stream);

// ---- connected components and rule R's rectangles (components.hip; the rules: include/prl_hip.h) of n maps (a chunk) of W x H on a
// caller's workspace.  work: cc_work_bytes(n, W, H), 256-byte aligned - the label planes, the scan's block counts, one pass of
// statistics and rectangles; small: cc_small_bytes(n); pinned: cc_pinned_bytes(n).  The caller holds ctx->mu. ----------
struct CcRun {
    PageSet maps;
    int n = 0, W = 0, H = 0;
    int connectivity = 8;     // the foreground's: 8 or 4 (the background is always 4-connected)
    bool external = true;     // number rule R's external components only, not every foreground component
    uint8_t* work = nullptr;
    uint8_t* small = nullptr;
    int32_t* pinned = nullptr;
    hipStream_t stream = nullptr;
};
size_t cc_work_per_page(int W, int H);   // the part of the workspace that grows with the pages
size_t cc_work_bytes(int n, int W, int H);
size_t cc_small_bytes(int n);
size_t cc_pinned_bytes(int n);
int cc_pass_components();                // components a statistics pass takes at most
// Labels, outer flags and the numbering.  Waits for the stream; then r.pinned[i] = the components numbered on page i (n_found), and
// the device holds their prefix sums: component k of page i is number r.pinned[0] + .. + r.pinned[i - 1] + k of the chunk.
int cc_label(const CcRun& r);
// The statistics of components [c0, c0 + m) of the chunk, m <= cc_pass_components(); then either their five numbers to
// d_stats[5 (c - c0)] (device), or the kept filter and the ordered compaction: the pass's kept rectangles to cc_pass_rects(r), x, y,
// w, h each.  Enqueues only.  cc_read_kept waits for the stream; then r.pinned[n + i] = the rectangles page i has kept in the
// passes since cc_label (they lie page after page in a pass: a pass's per-page share is the difference to the previous read).
int cc_stats_pass(const CcRun& r, int c0, int m, int32_t* d_stats);
int32_t* cc_pass_rects(const CcRun& r);
int cc_read_kept(const CcRun& r);
// 0 / 1 .. K into a caller's label planes (rows step bytes apart); enqueues only
int cc_write_labels(const CcRun& r, int32_t* d_labels, size_t page_stride, size_t step);

// ---- cv::HoughLines(rho 1, theta pi / 180) (hough.hip): the sizes of a W x H map's transform, per page and rounded to 256 bytes ----
struct HoughPlan {
    int W, H, numrho;
    int cells, ranges;          // rho cells a workgroup of k_hough_vote keeps in LDS, and how many such ranges a row takes
    size_t point_cap, points_bytes, accum_cells, accum_bytes, peak_cap, peaks_bytes;
};
struct HlPeak;   // houghline.h
HoughPlan hough_plan(int width, int height);
size_t hough_work_per_page(const HoughPlan& p);
// The sorted peaks of n maps (a chunk), page by page through `sink` on the calling thread; work: n * hough_work_per_page bytes,
// w's `small`: 2 * n words, its pinned block: n words at least (it grows to the lists).  Waits for the stream.
int hough_lines_run(const HoughPlan& p, const PageSet& maps, int n, int threshold, uint8_t* work, const WorkScope& w,
                    const std::function<void(int, const HlPeak*, size_t)>& sink);

// ---- morphology (morph.hip) ------------------------------------------------------------------
int morph_run(int iterations, const PageSet& src, int n_pages, int width, int height,
              const PageSetOut& dst, hipStream_t stream);
// kernel_run (optional) receives which kernel was launched; rows_per_seg > 0 replaces the segment height of the two streaming
// kernels (both for the prl_hip_internal_mask_morph entry of the test-hooks build: product calls leave them out)
enum { kMorphRanBitsFromBytes = 1, kMorphRanBitsFromBits = 2, kMorphRanStream = 3, kMorphRanBinary = 4 };
int morph_binary_run(int iterations, const PageSet& src, int n_pages, int width, int height,
                     const PageSetOut& dst, hipStream_t stream, int* kernel_run = nullptr, int rows_per_seg = 0);
int morph_large_run(int iterations, const PageSet& src, int n_pages, int width, int height, const PageSetOut& dst,
                    uint8_t* tmp, size_t tmp_step, hipStream_t stream);
int morph_bits_max_radius();
// source = bit plane (rows of bits.step bytes, 1 bit per pixel, bit j of byte i = pixel 8 i + j)
int morph_bitplane_run(int iterations, const PageSet& bits, int n_pages, int width, int height, const PageSetOut& dst,
                       hipStream_t stream, int* kernel_run = nullptr, int rows_per_seg = 0);
int pack_mask_run(const uint8_t* src, size_t src_step, int width, int height, uint8_t* bits, size_t bit_step,
                  hipStream_t stream);
constexpr int kMorphMaxFusedRadius = 8;  // morph_run / morph_binary_run handle |iterations| up to this

// ---- page reductions (binarize_literal.hip) ---------------------------------------------------
int page_min_run(const ThrParams& tp, const PageSet& src, int n_pages, PageGlobals* d_globals,
                 hipStream_t stream);
int wolf_coeff_run(const ThrParams& tp, PageGlobals* d_globals, int first_page, int n_pages, hipStream_t stream);

}  // namespace prl_hip
