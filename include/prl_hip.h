/*
 * prl_hip.h — C ABI of the MI355X (gfx950) implementation of PRLib's local-adaptive
 * binarization hot path and its NL-means pre-stage.
 *
 * This is the drop-in boundary: everything above it (the prl::binarize*(cv::Mat&, cv::Mat&, ...)
 * wrappers in prlib_amd/csrc/prl/, the ctypes binding in prlib_amd/_capi.py) only marshals
 * pointers, sizes and strides.  No C++ or torch types appear in any signature.
 *
 * Reference interfaces replaced (paths relative to the PRLib tree):
 *   prl::binarizeSauvola     src/binarizations/binarizeSauvola.h:43-47     .cpp:32-134
 *   prl::binarizeNiblack     src/binarizations/binarizeNiblack.h:43-47     .cpp:32-127
 *   prl::binarizeWolfJolion  src/binarizations/binarizeWolfJolion.h:43-47  .cpp:33-148
 *   prl::binarizeNICK        src/binarizations/binarizeNICK.h:43-47        .cpp:33-144
 *   prl::binarizeFeng        src/binarizations/binarizeFeng.h:46-53        .cpp:31-164
 *   prl::denoise             src/denoise/denoiseNLM.h:32                   .cpp:29-32
 *
 * Conventions
 *   - Images are 8-bit, row-major, `step` bytes between row starts (step >= width*channels),
 *     exactly cv::Mat's (data, step, rows, cols) view.
 *   - `*_device` entry points take DEVICE pointers and a hipStream_t (passed as void*; NULL = the
 *     null stream); they enqueue work and return without synchronising unless stated.
 *   - `*_host` entry points take HOST pointers, stage through the device and return when the
 *     result is in the caller's buffer.
 *   - All functions return PRL_OK (0) or a prl_status error; prl_hip_strerror() explains it and
 *     prl_hip_last_error_detail() carries the HIP runtime message for PRL_ERR_HIP.
 *   - Threading: every entry point may be called from any thread.  Calls that name different (device, stream) pairs share
 *     no workspace and overlap; calls on one stream - from one thread or several - are serialised by that stream's
 *     workspace lock and ordered by the stream.  The *_host entries and the stages that use the per-device staging area
 *     (denoise, deskew, backgroundNormalization, the chain) take a per-device lock for their duration.  Process-wide
 *     switches (exec mode, deferred completion, profiling, literal-page budget) are atomics; prl_hip_set_device, the error
 *     detail and prl_hip_last_stats are per thread.  Held by tests/test_concurrency_gpu.py (four threads on their own
 *     streams, two threads on one, 2 000 mixed calls with the device's free memory back at its baseline after
 *     prl_hip_release_workspace).
 *   - The library never falls back to a CPU implementation.  Without a usable gfx950 device every
 *     compute entry point fails with PRL_ERR_NO_DEVICE.
 */
#ifndef PRL_HIP_H_
#define PRL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRL_HIP_ABI_VERSION 4   /* 2: prl_chain_params grew deskew / background_normalization; 3: prl_hip_last_call_ms, prl_binarize_stats.wolf_candidates; 4: prl_hip_find_angle_*, prl_deskew_stats */

typedef enum prl_status {
    PRL_OK = 0,
    PRL_ERR_EMPTY = 1,       /* empty input image: reference throws std::invalid_argument (binarizeSauvola.cpp:38-41) */
    PRL_ERR_BAD_WINDOW = 2,  /* !(windowSize > 1 && windowSize odd): std::invalid_argument (binarizeSauvola.cpp:43-47) */
    PRL_ERR_BAD_CHANNELS = 3,/* channel count the reference's cvtColor / NLM would reject */
    PRL_ERR_EMPTY_RECT = 4,  /* processing rectangle has no pixels (reference: cv::Exception from the ROI/filter2D) */
    PRL_ERR_BAD_ARG = 5,     /* null pointer, step < row bytes, negative count, unknown method ... */
    PRL_ERR_NO_DEVICE = 6,   /* no gfx950 device / HIP runtime unusable */
    PRL_ERR_HIP = 7,         /* a HIP call failed; see prl_hip_last_error_detail() */
    PRL_ERR_NOMEM = 8,       /* device or host allocation failed */
    PRL_ERR_UNSUPPORTED = 10,/* a value the reference's interface accepts and this library does not provide (a border mode of
                              * prl::warpCrop other than CONSTANT / REPLICATE) */
    PRL_ERR_LITERAL_BUDGET = 9 /* more pages of the call need the literal redo than prl_hip_set_literal_page_budget() allows:
                                  the masks of those pages are UNFINISHED (every other page is complete); see INTEGRATION.md §3 */
} prl_status;

/* The five local-adaptive binarizers of src/binarizations named by the north star. */
typedef enum prl_method {
    PRL_SAUVOLA = 0,     /* T = m * (1 + k*(s/128 - 1))            binarizeSauvola.cpp:115-118   */
    PRL_NIBLACK = 1,     /* T = m + k*s                             binarizeNiblack.cpp:108       */
    PRL_WOLFJOLION = 2,  /* T = m + (k*s/max(s) - k)*(m - min(I))   binarizeWolfJolion.cpp:115-130 */
    PRL_NICK = 3,        /* T = m + k*sqrt(m*m + s*s)               binarizeNICK.cpp:121-126      */
    PRL_FENG = 4         /* as written in binarizeFeng.cpp:111-142 (Rs aliases s)                */
} prl_method;

/*
 * Parameters of one binarization call; field meaning = the reference's default arguments.
 *   Sauvola / Niblack / WolfJolion: window_size=101, k=0.01, morph_iterations=2
 *   NICK:                            window_size=21,  k=-0.01, morph_iterations=0
 *   Feng: window_size=21, feng_alpha1=0.75, feng_k1=0.2, feng_k2=0.03, feng_gamma=2.0, morph=2
 * prl_hip_default_params() fills these.
 */
typedef struct prl_binarize_params {
    int32_t method;            /* prl_method */
    int32_t window_size;       /* windowSize: must be > 1 and odd (checked before clamping to min(W,H)) */
    double  k;                 /* thresholdCoefficient (unused by Feng) */
    int32_t morph_iterations;  /* >0: dilate^n then erode^n; <0: erode^n then dilate^n; 0: none */
    int32_t reserved0;
    double  feng_alpha1;
    double  feng_k1;           /* dead in the reference (binarizeFeng.cpp:128); carried for signature parity */
    double  feng_k2;
    double  feng_gamma;
} prl_binarize_params;

/* Geometry derived from (params, W, H) exactly as the reference derives it. */
typedef struct prl_binarize_geometry {
    int32_t w;        /* effective window = min(windowSize, min(W,H))      binarizeSauvola.cpp:57 */
    int32_t half;     /* w/2 = replicate padding on each side              binarizeSauvola.cpp:65 */
    int32_t padded_w; /* W + 2*half : size the caller's input Mat ends up with */
    int32_t padded_h; /* H + 2*half */
    int32_t out_w;    /* Sauvola/Niblack: W+2*half-w ; Wolf/NICK/Feng: W-w  (binarizeSauvola.cpp:66 vs binarizeWolfJolion.cpp:69) */
    int32_t out_h;
} prl_binarize_geometry;

/* Execution mode of the binarizers (process-wide; default PRL_MODE_AUTO). */
typedef enum prl_exec_mode {
    PRL_MODE_AUTO = 0,     /* fused sliding-window kernel + exact fix-up of the few undecided pixels */
    PRL_MODE_LITERAL = 1   /* materialised float64 integral images, one literal evaluation per pixel */
} prl_exec_mode;

/* Counters of the last binarize call on the calling thread (for tests and the bench report).  Every page counts once, in
 * the pass that wrote its final bytes; a call that was split into page chunks reports the sum of its chunks. */
typedef struct prl_binarize_stats {
    uint64_t pixels;            /* output pixels produced */
    uint64_t refined_pixels;    /* decided by the in-kernel float64 interval test instead of the float32 one */
    uint64_t exact_pixels;      /* decided by the absolute-integral literal evaluation (fix-up kernel) */
    uint64_t literal_pages;     /* pages that ran the full literal pipeline */
    uint64_t wolf_candidates;   /* Wolf-Jolion: pixels whose deviation was evaluated literally to find devianceMax (a lower bound: a wavefront stops counting once its page's list is full) */
    uint64_t exact_sweep_pages; /* pages whose refine queue overflowed and which the exact sweep redid (the float64 interval test inline; was reserved[0]) */
    uint64_t reserved[2];
} prl_binarize_stats;

/* ---- library / device ------------------------------------------------------------------- */

int         prl_hip_abi_version(void);
const char* prl_hip_strerror(int status);
const char* prl_hip_last_error_detail(void);           /* thread-local, never NULL */
int         prl_hip_device_count(int* count);          /* number of visible HIP devices */
/* Device used by subsequent calls of this thread (thread-local, sticky).  Each call then makes it the thread's current HIP
 * device, exactly as hipSetDevice(device) would, and leaves it so: a caller that juggles several devices on one thread sets
 * its own device again afterwards.  Without this call the library follows hipGetDevice(). */
int         prl_hip_set_device(int device);
int         prl_hip_set_exec_mode(int mode);           /* prl_exec_mode */
int         prl_hip_get_exec_mode(void);
int         prl_hip_last_stats(prl_binarize_stats* out);
/* Cost bound for hostile input (process-wide; INTEGRATION.md §3 "What a hostile input costs").  A page whose queues of
 * undecided pixels overflow is redone by the literal pipeline (~50 x the fast path's time per pixel); an exact two-level
 * periodic pattern makes every page of a call do that.  With a budget >= 0 a call that would redo more than `max_pages`
 * pages does not: it returns PRL_ERR_LITERAL_BUDGET (prl_hip_last_stats().literal_pages says how many needed it) and the
 * caller decides where that request runs.  -1 (default; env PRL_HIP_LITERAL_PAGE_BUDGET): no limit.  Results are never
 * approximated: a page is either bit-exact or reported unfinished. */
int         prl_hip_set_literal_page_budget(int max_pages);
int         prl_hip_get_literal_page_budget(void);
int         prl_hip_release_workspace(void);           /* free cached device scratch of the current device */
/* Measurement aid: when enabled, HIP events bracket the dominant kernel of each binarize call
 * (k_fused in PRL_MODE_AUTO, the whole integral+threshold chain in PRL_MODE_LITERAL) on the stream it
 * is launched on; prl_hip_last_kernel_ms() waits for them and returns the elapsed milliseconds. */
int         prl_hip_set_profiling(int enabled);
int         prl_hip_last_kernel_ms(float* ms);
/* Same switch, the WHOLE call: events around everything the last binarize call of this thread enqueued on its stream (every
 * sweep of Wolf-Jolion, interval refinement, literal fix-up, morphology pass, flag copy) - what one prl::binarize*() costs
 * on the device.  Calls that were split into page chunks report their last chunk. */
int         prl_hip_last_call_ms(float* ms);
/* Deferred completion of prl_hip_binarize_*_device (process-wide switch, default off): see the comment there. */
int         prl_hip_set_deferred_completion(int enabled);
/* Completes every binarize call enqueued on `stream` of the current device (flag check, literal redo of overflowing
 * pages) and waits for the stream.  Cheap when nothing is pending. */
int         prl_hip_finish(void* stream);

/* ---- binarizers -------------------------------------------------------------------------- */

int prl_hip_default_params(int method, prl_binarize_params* out);

/* Validation + geometry; returns the status the reference's argument checks imply. */
int prl_hip_binarize_geometry(const prl_binarize_params* p, int width, int height,
                              prl_binarize_geometry* out);

/*
 * Binarize n_pages single-channel pages of equal size that already live in device memory.
 *   d_src        first page; page i starts at d_src + i*src_page_stride
 *   d_dst        first output page (out_w x out_h, see prl_hip_binarize_geometry); values {0,255}
 *   stream       hipStream_t or NULL
 * Everything is enqueued on `stream` (threshold sweep, interval refinement, literal fix-up - the last two find their
 * work lists on the device and do nothing when they are empty - and the morphology pass).  One thing needs the host:
 * a page with more than 2^17 pixels within ~1e-6 of their threshold (pathological input) is flagged and redone by the
 * literal pipeline.  Default: the call waits for its own work once, looks at the flags and returns with the result
 * complete.  With prl_hip_set_deferred_completion(1) it returns right after enqueuing; the flags are looked at later
 * (a later call that needs the slot, prl_hip_last_stats, prl_hip_finish), so the caller must call
 * prl_hip_finish(stream) before consuming the masks.  Calls on different streams of a device use separate
 * workspaces and overlap.
 * Replaces the body of prl::binarize{Sauvola,Niblack,WolfJolion,NICK,Feng} after cvtColor.
 */
int prl_hip_binarize_batch_device(const prl_binarize_params* p, int n_pages,
                                  const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                  int width, int height,
                                  uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                  void* stream);

/* Same, pages addressed through host arrays of device pointers (pages need not be contiguous). */
int prl_hip_binarize_pages_device(const prl_binarize_params* p, int n_pages,
                                  const uint8_t* const* d_src_pages, size_t src_step,
                                  int width, int height,
                                  uint8_t* const* d_dst_pages, size_t dst_step,
                                  void* stream);

/*
 * One page from/to host memory (what the cv::Mat wrapper calls).  `src` is 1-channel.
 * If padded_out != NULL it receives the replicate-padded gray image (padded_w x padded_h) the
 * reference leaves in the caller's input Mat (binarizeSauvola.cpp:65).
 */
int prl_hip_binarize_host(const prl_binarize_params* p,
                          const uint8_t* src, size_t src_step, int width, int height,
                          uint8_t* dst, size_t dst_step,
                          uint8_t* padded_out, size_t padded_step);

/*
 * A list of n_pages equal-size 1-channel pages in HOST memory (what a caller holding n cv::Mat has,
 * samples/binarizations/binarizeSauvola_sample.cpp:48-53), sharded over the devices of the node: contiguous blocks
 * (prl_hip_page_range); per device a three-stage pipeline (upload / kernels / download of neighbouring chunks of pages on
 * three streams, chunk slots kept between calls), results in the caller's buffers in the caller's order.
 * n_devices: 0 = every visible device.  No collective; returns when all pages are done.
 */
int prl_hip_binarize_batch_host(const prl_binarize_params* p, int n_pages, const uint8_t* const* src, size_t src_step,
                                int width, int height, uint8_t* const* dst, size_t dst_step, int n_devices);

/*
 * Pinned host memory for a caller's pages.  The reference's callers hold pages as cv::Mat (pageable memory,
 * samples/binarizations/binarizeSauvola_sample.cpp:48); a Mat header over memory from prl_hip_alloc_host -
 * cv::Mat(rows, cols, CV_8UC1, ptr, step) - or over memory pinned in place with prl_hip_host_register is moved by the
 * DMA engines directly: prl_hip_binarize_batch_host detects such pages (hipPointerGetAttributes) and skips its bounce
 * buffers and the two CPU copies per page.  Pageable pages keep working (bounce path).
 * prl_hip_host_register page-locks `bytes` at `p` (costs about one copy of them; pays from the second call on).
 */
int prl_hip_alloc_host(size_t bytes, void** out);
int prl_hip_free_host(void* p);
int prl_hip_host_register(void* p, size_t bytes);
int prl_hip_host_unregister(void* p);

/* The block of a list of n_items that part `part` of `n_parts` owns (sizes differ by at most one): the split used by
 * prl_hip_binarize_batch_host over devices and by one-process-per-GPU launchers over ranks. */
int prl_hip_page_range(int n_items, int n_parts, int part, int* first, int* count);

/* (2n+1)x(2n+1) rectangular closing (n>0) / opening (n<0) with out-of-image pixels ignored:
 * the cv::dilate/cv::erode pair at binarizeSauvola.cpp:125-134.  In place is NOT allowed. */
int prl_hip_morph_batch_device(int morph_iterations, int n_pages,
                               const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                               int width, int height,
                               uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                               void* stream);

/* ---- NL-means denoise (prl::denoise -> cv::fastNlMeansDenoisingColored) -------------------- */

/*
 * Non-local means on interleaved 8-bit planes, template 7x7, search 21x21, integer SSD and
 * fixed-point weights as in OpenCV's FastNlMeansDenoisingInvoker.
 *   channels 1: the L plane (h = strength); channels 2: the ab planes (h = 3);
 *   channels 3: treated as three jointly weighted planes (cv::fastNlMeansDenoising on 8UC3).
 */
int prl_hip_nlm_planes_device(int n_pages, int channels, float h,
                              const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                              int width, int height,
                              uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                              void* stream);

/*
 * prl::denoise on BGR (channels=3) or BGRA (channels=4) device pages:
 * LBGR->Lab, NLM(L, strength), NLM(ab, 3), Lab->LBGR  (denoiseNLM.cpp:31).
 */
int prl_hip_denoise_batch_device(int n_pages, int channels, float strength,
                                 const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                 int width, int height,
                                 uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                 void* stream);

int prl_hip_denoise_host(int channels, float strength,
                         const uint8_t* src, size_t src_step, int width, int height,
                         uint8_t* dst, size_t dst_step);

/* ---- thinning (prl::thinZhangSuen / prl::thinGuoHall) --------------------------- */

typedef enum prl_thin_method {
    PRL_THIN_ZHANGSUEN = 0,  /* src/thinning/thinZhangSuen.cpp:15-108 */
    PRL_THIN_GUOHALL = 1     /* src/thinning/thinGuoHall.cpp:15-107   */
} prl_thin_method;

/*
 * Iterative thinning of 1-channel 8-bit pages: foreground = pixels with bit 0 set (the reference's `&= 1`),
 * output 0 / 255.  Replaces the body of prl::thinZhangSuen / prl::thinGuoHall after cvtColor.  d_src == d_dst is
 * allowed.  Synchronises the stream every few passes to read the convergence flags.
 */
int prl_hip_thin_batch_device(int method, int n_pages, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                              int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                              void* stream);

int prl_hip_thin_host(int method, const uint8_t* src, size_t src_step, int width, int height,
                      uint8_t* dst, size_t dst_step);

/* ---- channel adapters and the device-resident chain ---------------------- */

/*
 * cv::cvtColor(src, dst, cv::COLOR_BGR2GRAY) on 8-bit BGR (channels = 3) / BGRA (4) pages already in device
 * memory: the first call of every binarizer for a colour input (src/binarizations/binarizeSauvola.cpp:51, same
 * line in the other four; src/thinning/thinZhangSuen.cpp:78).  14-bit fixed point, bit-exact.
 */
int prl_hip_bgr2gray_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride,
                                  size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                  size_t dst_step, void* stream);

/* cv::cvtColor(COLOR_GRAY2BGR / GRAY2BGRA): what a caller needs in front of prl::denoise, which only accepts
 * 3/4-channel input (src/denoise/denoiseNLM.cpp:31 -> fastNlMeansDenoisingColored). */
int prl_hip_gray2bgr_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride,
                                  size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                  size_t dst_step, void* stream);

/* cv::bitwise_not on 1-channel pages (d_src == d_dst allowed): the binarizers emit white = background while
 * prl::thinZhangSuen thins white (src/thinning/thinZhangSuen.cpp:85). */
int prl_hip_invert_batch_device(int n_pages, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                void* stream);

#define PRL_CHAIN_NO_THINNING (-1)

/* One page through prl::deskew -> prl::denoise -> prl::backgroundNormalization -> cvtColor -> prl::binarize* ->
 * bitwise_not -> prl::thin* (BASELINE config 5; every stage but the binarizer optional).  Not a function of the
 * reference: a caller writes these calls one after the other; here the intermediates stay in device memory. */
typedef struct prl_chain_params {
    int denoise;                   /* != 0: prl::denoise(denoise_strength); needs a 3/4-channel input */
    float denoise_strength;        /* src/denoise/denoiseNLM.h:32 default 5.5 */
    prl_binarize_params binarize;  /* which binarizer and its arguments */
    int thin;                      /* PRL_CHAIN_NO_THINNING, PRL_THIN_ZHANGSUEN or PRL_THIN_GUOHALL */
    int deskew;                    /* != 0: prl::deskew first (per-page result sizes: prl_hip_chain_pages_device) */
    int background_normalization;  /* != 0: prl::backgroundNormalization after the denoise stage (4 channels become 3) */
} prl_chain_params;

void prl_hip_default_chain_params(prl_chain_params* out);

/* d_dst: out_w x out_h bytes per page (prl_hip_binarize_geometry): the binarizer's mask, or, with thinning, the
 * skeleton of the dark strokes (white on black).  Synchronises `stream` where the stages do.  params->deskew must be 0
 * here (a deskewed page has its own size). */
int prl_hip_chain_batch_device(const prl_chain_params* params, int n_pages, int channels, const uint8_t* d_src,
                               size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                               size_t dst_page_stride, size_t dst_step, void* stream);

/* Largest result a page of width x height can have through the chain (with deskew: a max(width,height) square in, so
 * the binarizer's geometry of that). */
int prl_hip_chain_max_out_size(const prl_chain_params* params, int width, int height, int* out_w, int* out_h);

/* The chain with per-page result sizes (needed as soon as params->deskew is set): page i's result is
 * out_wh[2i] x out_wh[2i+1] bytes (host array), written at dst_step bytes per row into a d_dst page with room for
 * prl_hip_chain_max_out_size; angles (host, optional) receives findAngle's degrees per page.  Synchronises. */
int prl_hip_chain_pages_device(const prl_chain_params* params, int n_pages, int channels, const uint8_t* d_src,
                               size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                               size_t dst_page_stride, size_t dst_step, int32_t* out_wh, double* angles, void* stream);

/* The same chain on a list of HOST pages of one size (the cv::Mats of a caller that loops over prl::deskew, prl::denoise,
 * prl::backgroundNormalization, prl::binarizeSauvola, prl::thinZhangSuen page by page, BASELINE config 5), sharded over the
 * first n_devices GPUs (0 = all visible) in contiguous blocks (prl_hip_page_range), no collective.  Per device: a worker
 * thread, chunks of PRL_HIP_CHAIN_HOST_PAGES pages, the upload of chunk k+1 and the download of chunk k-1 overlapped with the
 * chain on chunk k.  dst[i]: room for prl_hip_chain_max_out_size at dst_step >= that width; out_wh[2i], out_wh[2i+1]: the
 * size of page i's result; angles: optional.  Returns when every page is in the caller's memory. */
int prl_hip_chain_batch_host(const prl_chain_params* params, int n_pages, int channels, const uint8_t* const* src,
                             size_t src_step, int width, int height, uint8_t* const* dst, size_t dst_step, int32_t* out_wh,
                             double* angles, int n_devices);

/* ---- background normalisation (prl::backgroundNormalization) ------------------------------ */

/*
 * prl::backgroundNormalization(const cv::Mat&, cv::Mat&) (src/backgroundNormalization.cpp:36-61) =
 * Leptonica's pixBackgroundNormSimple(pixs, NULL, NULL) between prl::opencvToLeptonica / prl::leptonicaToOpenCV
 * (src/formatConvert.cpp:38-218): channels 1 -> 1-channel result, 3 or 4 -> 3-channel result (the fourth byte is
 * dropped by the reference's converter).  d_dst rows hold width * prl_hip_bgnorm_out_channels(channels) bytes.
 * Enqueues on `stream`, no synchronisation.
 */
int prl_hip_bgnorm_out_channels(int channels);
int prl_hip_bgnorm_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_bgnorm_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                        size_t dst_step);

/* ---- salt-and-pepper denoising (prl::denoiseSaltPepper) ----------------------------------------------------------- */

/*
 * prl::denoiseSaltPepper(in, out, kernelSize, times) (src/denoise/denoiseSaltPepper.h:40, .cpp:29-36) = `times` passes of
 * cv::medianBlur(out, out, kernelSize) over a copy of the input: out(y, x, c) is the value at rank (k*k - 1) / 2 of the
 * k x k window around (y, x) in channel c, BORDER_REPLICATE, each pass reading the previous pass's result.  Exact for every
 * odd ksize up to 65535 (a window larger than the page included).  8-bit pages of 1..4 interleaved channels; 2 channels only
 * with ksize <= 5 (cv::medianBlur's k > 5 path takes 1, 3, 4).  ksize == 1 or times == 0 copies.  Sizes: width, height
 * <= 32768.  d_src == d_dst with the same strides (in place) is allowed; any other overlap returns PRL_ERR_BAD_ARG, and d_src
 * is otherwise never written.  Passes alternate between d_dst and the device's cached scratch (R x H bytes per page,
 * R = width * channels, when times >= 2 or in place).  Enqueues on `stream`, no synchronisation.
 * PRL_ERR_EMPTY: width or height <= 0; PRL_ERR_BAD_WINDOW: ksize < 1 or even; PRL_ERR_BAD_CHANNELS: channels outside 1..4, or
 * 2 with ksize >= 7; PRL_ERR_BAD_ARG: null pointer, negative n_pages, step < row bytes, size above the limits.
 */
int prl_hip_median_batch_device(int n_pages, int channels, int ksize, size_t times, const uint8_t* d_src, size_t src_page_stride,
                                size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                void* stream);
int prl_hip_median_host(int channels, int ksize, size_t times, const uint8_t* src, size_t src_step, int width, int height,
                        uint8_t* dst, size_t dst_step);

/* ---- grayscale morphology with a flat element, prl::correctNUIL ----------------------------------------------------- */

#define PRL_MORPH_ERODE 0     /* cv::MORPH_ERODE */
#define PRL_MORPH_DILATE 1    /* cv::MORPH_DILATE */
#define PRL_MORPH_OPEN 2      /* cv::MORPH_OPEN: erode, then dilate */
#define PRL_MORPH_CLOSE 3     /* cv::MORPH_CLOSE: dilate, then erode */
#define PRL_MORPH_TOPHAT 5    /* cv::MORPH_TOPHAT: src - open, saturating */
#define PRL_MORPH_BLACKHAT 6  /* cv::MORPH_BLACKHAT: close - src, saturating */
#define PRL_SHAPE_RECT 0      /* cv::MORPH_RECT */
#define PRL_SHAPE_CROSS 1     /* cv::MORPH_CROSS */
#define PRL_SHAPE_ELLIPSE 2   /* cv::MORPH_ELLIPSE */

/*
 * cv::morphologyEx(src, dst, op, cv::getStructuringElement(shape, Size(ksize_w, ksize_h))), one iteration, on 8-bit pages of
 * 1..4 interleaved channels in device memory: dst(y, x, c) = min (erode) / max (dilate) over the element's set pixels (i, j)
 * of src(y + i - ksize_h/2, x + j - ksize_w/2, c); taps outside the page are ignored (morphologyDefaultBorderValue) and the
 * element is not reflected between the two operators.  Exact.  Element sizes 1..255 each way (OpenCV has no upper limit);
 * width, height <= 32768.  d_src == d_dst with the same strides (in place) is allowed; any other overlap returns
 * PRL_ERR_BAD_ARG, and d_src is otherwise never written.  Intermediate planes (at most two of width * channels * height bytes
 * per page) live in the device's cached scratch.  Enqueues on `stream`, no synchronisation.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_ARG (unknown op or
 * shape, a size < 1 or > 255); PRL_ERR_BAD_CHANNELS (channels outside 1..4); PRL_ERR_BAD_ARG (null pointer, negative n_pages,
 * step < row bytes, width or height above the limit, overlapping source and destination).
 */
int prl_hip_morphology_batch_device(int n_pages, int channels, int op, int shape, int ksize_w, int ksize_h, const uint8_t* d_src,
                                    size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                    size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_morphology_host(int channels, int op, int shape, int ksize_w, int ksize_h, const uint8_t* src, size_t src_step, int width,
                            int height, uint8_t* dst, size_t dst_step);

/*
 * cv::morphologyEx(src, dst, op, element, Point(anchor_x, anchor_y), iterations): the entries above with the two arguments they
 * fix; (-1, -1, 1) is exactly them.  An anchor of -1 is the centre ksize / 2, taken per coordinate; otherwise it lies in
 * 0 .. ksize - 1 and dst(y, x, c) = min / max of src(y + i - anchor_y, x + j - anchor_x, c).  iterations = n in 1..16
 * [upstream, morph.cpp]: an element whose every pixel is set (a rectangle, whatever `shape` says) runs ONCE as the rectangle of
 * 1 + n (ksize_w - 1) x 1 + n (ksize_h - 1) with the anchor (n anchor_x, n anchor_y), which equals n passes because taps outside
 * the page are ignored and the anchor lies inside the element; a grown side above 255 is PRL_ERR_BAD_ARG.  Cross and ellipse run n
 * real passes.  The composite operators apply n to each half: CLOSE is n dilations, then n erosions; TOPHAT and BLACKHAT subtract
 * once, at the end.  Everything else - layouts, in place, limits, stream semantics - as above; the anchor and iterations are
 * checked with the element (PRL_ERR_BAD_ARG, second in the order).
 */
int prl_hip_morphology_ex_batch_device(int n_pages, int channels, int op, int shape, int ksize_w, int ksize_h, int anchor_x, int anchor_y,
                                       int iterations, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width, int height,
                                       uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_morphology_ex_host(int channels, int op, int shape, int ksize_w, int ksize_h, int anchor_x, int anchor_y, int iterations,
                               const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/*
 * prl::correctNUIL(in, out, structuringElementSize = 31) (src/correctNUIL.cpp:33-90): per page and channel, the channel is
 * inverted (x ^ 255) where its mean over the page is below 128 (decided on the device as sum < 128 * width * height), then
 * dst = 255 - blackhat(channel, ellipse(size, size)).  Same layouts, aliasing rule, limits, stream semantics and order of the
 * checks as prl_hip_morphology_batch_device (size < 1 or > 255: PRL_ERR_BAD_ARG).
 */
int prl_hip_correct_nuil_batch_device(int n_pages, int channels, int size, const uint8_t* d_src, size_t src_page_stride,
                                      size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                      void* stream);
int prl_hip_correct_nuil_host(int channels, int size, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                              size_t dst_step);

/* ---- prl::removeLines --------------------------------------------------------------------------------------------------- */

/*
 * prl::removeLines(in, out) (src/removeLines.cpp:30-76) on 8-bit pages of 1 or 3 (BGR) channels in device memory; the result
 * is one channel at the input's size.  gray = the 14-bit luma for 3 channels, else the page; t = getThreshVal_Otsu_8u(255 -
 * gray) (the float64 scan, per page, on the device); bw = 255 - gray > t; horizontal = dilate(erode(bw)) with a
 * (width / 50) x 1 rectangle, vertical the same with 1 x (height / 50), both with the offsets -k/2 .. k-1-k/2 and taps outside
 * the page ignored; dst = 0 where bw is set and neither opening is, else 255.  Exact.  The mask and the openings run on bit
 * planes in the device's cached scratch (3/8 byte per pixel and page, plus one gray byte for 3 channels); element lengths are
 * not limited (width, height <= 32768 gives at most 655).  d_src == d_dst with the same strides (in place) is allowed for
 * 1-channel pages; any other overlap returns PRL_ERR_BAD_ARG, and d_src is otherwise never written.  Enqueues on `stream`, no
 * synchronisation.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_CHANNELS (channels
 * other than 1 and 3: cv::threshold's Otsu takes 8UC1 only); PRL_ERR_BAD_ARG (width or height below 50: an element of size 0,
 * cv::getStructuringElement's assertion; null pointer, negative n_pages, step < row bytes, width or height above the limit,
 * overlapping source and destination).
 */
int prl_hip_remove_lines_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                      int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_remove_lines_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/* ---- tone: histogram, table look-up, prl::gammaCorrection, the white balances, prl::cleanBackgroundToWhite -------------- */

/*
 * Point operations on 8-bit pages in device memory whose table depends on page statistics (tone.hip).  Every output byte of
 * the four reference functions below is a function of the input byte and of the page's per-channel histograms only, so each
 * runs as histogram -> 256-entry table per (page, channel) -> dst = table[src], and is exact also where the reference computes
 * in float or double per pixel.  Pages hold `channels` interleaved bytes per pixel; pages and rows may be strided.
 *
 * Every entry checks in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_CHANNELS
 * (channels outside 1..4 for the two primitives and for gamma, other than 1, 3, 4 for clean-background; the white balances take
 * 3-channel pages and have no channel argument); PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row bytes, width or
 * height above 32768, overlapping source and destination).  d_src == d_dst with the same strides (in place) is allowed where the
 * result has as many channels as the source; any other overlap is PRL_ERR_BAD_ARG.  The *_batch_device entries enqueue on
 * `stream` and do not synchronise, except where stated; the *_host entries take one page in host memory.
 */

/* d_hist[page][channel][256] = the number of pixels of the page with that value in that channel; the call overwrites it. */
int prl_hip_histogram_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                   int height, uint32_t* d_hist, void* stream);

/*
 * cv::LUT: dst(y, x, c) = d_lut[c * 256 + src(y, x, c)].  d_lut holds [channel][256] bytes in device memory; page i reads its
 * tables lut_page_stride bytes after page i - 1's, and a lut_page_stride of 0 gives every page the same set.
 */
int prl_hip_lut_batch_device(int n_pages, int channels, const uint8_t* d_lut, size_t lut_page_stride, const uint8_t* d_src,
                             size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                             size_t dst_step, void* stream);

/*
 * prl::gammaCorrection(in, out, k, gamma) (src/balance/gammaCorrection.cpp:52-106).  g[v] = sat_u8(pow(v / 255.0, gamma) * 255.0)
 * in double with the host's pow, then, unless |k - 1| <= 1e-7, t[v] = sat_u8((float)g[v] * (float)k) (Mat *= k on 8U is
 * convertTo(8U, k), float32 [upstream]); sat_u8 rounds half to even and clamps, and NaN, +-inf and what lies outside int32 give 0
 * (SURVEY.md A.6).  1, 2 or 3 channels come back with as many.  4 channels: the reference converts BGRA to BGR and its switch has
 * no case for 4, so the result has 3 channels, the alpha byte dropped and only the k step applied; reproduced.  The table is built
 * on the host and handed to the kernel by value.
 */
int prl_hip_gamma_correction_batch_device(int n_pages, int channels, double k, double gamma, const uint8_t* d_src, size_t src_page_stride,
                                          size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                          size_t dst_step, void* stream);
int prl_hip_gamma_correction_host(int channels, double k, double gamma, const uint8_t* src, size_t src_step, int width, int height,
                                  uint8_t* dst, size_t dst_step);

/*
 * prl::simpleWhiteBalance(in, out, k) (src/balance/balanceSimpleWhite.cpp:33-142) on 3-channel pages.  Per channel: the cumulative
 * histogram as int; vmin = the first v with cum[v] >= k * total (a double product); vmax scans down from 255 while cum[vmax] >
 * (1 - k) * total, then + 1 if below 254; scale = 255.0f / (vmax - vmin); out = (uchar)((clamp(v, vmin, vmax) - vmin) * scale),
 * int times float, truncated.  Where the reference's behaviour is undefined: both scans stop at the array's ends (the reference
 * reads outside its histogram for an all-zero channel and for k > 1), and a channel with vmax == vmin (0 * inf) comes out 0, which
 * is what the x86 conversion gives.  A NaN or negative k gives the identity, by the literal comparisons.  Histograms and tables
 * stay on the device.
 */
int prl_hip_simple_white_balance_batch_device(int n_pages, double k, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                              int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                              void* stream);
int prl_hip_simple_white_balance_host(double k, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                                      size_t dst_step);

/*
 * prl::grayWorldWhiteBalance(in, out, pNorm, withMax) (src/balance/balanceGrayWorldWhite.cpp:37-115) on 3-channel pages.
 * S_c = sum over v = 0..255, ascending, of (double)hist[v] * pow((double)v, p) (empty bins add nothing); m_c = pow(S_c / (cols *
 * rows), 1 / p); r = (m1 + m2 + m0) / 3.0, or std::max(m1, std::max(m2, m0)) with with_max; out = (uchar)std::min(255.0, v * (r /
 * m_c)), so an all-zero channel (a NaN) comes out all 255.  The reference sums pow(v, p) in raster order: for p = 1, 2, 3 every
 * term and partial sum is an exact integer and the sum over the bins equals it bit for bit; for other p the means can differ in
 * their last bits, and an output byte only where v * ratio lies that close to an integer.  p_norm == 1.0 runs on the device without
 * synchronising (pow(x, 1) is skipped).  Any other p_norm needs the host's pow: the histograms are copied to the host, the tables
 * built there (prl_hip_gray_world_luts) and copied back - that path SYNCHRONISES `stream`.
 */
int prl_hip_gray_world_batch_device(int n_pages, double p_norm, int with_max, const uint8_t* d_src, size_t src_page_stride,
                                    size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                    void* stream);
int prl_hip_gray_world_host(double p_norm, int with_max, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                            size_t dst_step);

/*
 * prl::cleanBackgroundToWhite(in, out) (src/cleanBackgroundToWhite.cpp:39-64) = pixCleanBackgroundToWhite(pixs, NULL, NULL, 1.0, 70,
 * 170) [upstream]: pixBackgroundNormSimple (exactly prl_hip_bgnorm_*: 1 channel -> 1, 3 or 4 -> 3) followed by pixGammaTRC(1.0, 70,
 * 170) in place, the table of prl_hip_clean_background_lut.  A page that the normalisation copies gets the table applied to the
 * copy.  Uses the device's cached scratch like prl_hip_bgnorm_batch_device.
 */
int prl_hip_clean_background_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                          int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_clean_background_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                                  size_t dst_step);

/*
 * The tables themselves, built on the host: no device is needed.  The kernel that derives the white-balance tables on the device
 * runs the same code.  prl_hip_clean_background_lut: numaGammaTRC(1.0, 70, 170) [upstream]: 0 below 70, 255 above 170, else
 * (int)(255. * x + 0.5) with x = (float)(i - 70) / (float)100.  The two *_luts take hist[channel][256] of one 3-channel page (the
 * layout of prl_hip_histogram_batch_device) and write luts[channel][256]; cols * rows is the sum of a channel's bins:
 * PRL_ERR_EMPTY where it is 0, PRL_ERR_BAD_ARG where the three channels' sums differ or exceed 32768 * 32768, and for a null pointer.
 */
int prl_hip_gamma_lut(double k, double gamma, uint8_t lut[256]);
int prl_hip_clean_background_lut(uint8_t lut[256]);
int prl_hip_simple_white_balance_luts(double k, const uint32_t hist[3 * 256], uint8_t luts[3 * 256]);
int prl_hip_gray_world_luts(double p_norm, int with_max, const uint32_t hist[3 * 256], uint8_t luts[3 * 256]);

/* ---- contrast: cv::CLAHE, cv::equalizeHist, EnhanceLocalContrastByCLAHE (src/imageLibCommon.cpp:327-395) ------------------------ */

#define PRL_CLAHE_MAX_TILES 64   /* tiles a side at most */

/*
 * cv::CLAHE::apply and cv::equalizeHist on 8-bit pages in device memory, every channel on its own (clahe.hip; the arithmetic as
 * plain code: prlib_amd/csrc/clahe.h).  Both are [upstream] OpenCV 3.4 / 4.x (clahe.cpp, histogram.cpp), stated from memory.
 * Every float operation is float32 with one rounding, evaluated left to right as written, never fused; sat_u8 rounds half to even
 * and clamps.
 *
 * CLAHE of one W x H channel, grid tiles_x x tiles_y (cv::createCLAHE's default is 8 x 8), clip_limit a double:
 *   1. W % tiles_x == 0 and H % tiles_y == 0: the tiles are cut from the page.  Otherwise from copyMakeBorder(src, 0, tiles_y -
 *      H % tiles_y, 0, tiles_x - W % tiles_x, BORDER_REFLECT_101): BOTH sides grow, a side that divides by a whole `tiles` (16 x
 *      13 on 8 x 8 becomes 24 x 16).  The border index is borderInterpolate's: a side of 1 gives 0, else the index reflects until
 *      it lies inside (the pad can exceed the side).  tile_w = ext_w / tiles_x, tile_h = ext_h / tiles_y, area = tile_w * tile_h.
 *   2. lut_scale = (float)255 / (float)area.  clip = 0 for clip_limit <= 0, else max((int)(clip_limit * area / 256), 1) with the
 *      product and the quotient in double; a value outside int converts as x86 does, to INT_MIN, hence clip = 1.
 *   3. Per tile the 256 int bins of the extended page's tile; with clip > 0: clipped = sum of max(h[i] - clip, 0), h[i] = min(h[i],
 *      clip), every bin += clipped / 256, and with residual = clipped % 256 != 0 and step = max(256 / residual, 1) the loop
 *      for (i = 0; i < 256 && residual > 0; i += step, --residual) ++h[i] (bin i gets one more where i % step == 0 and i / step <
 *      residual).  Then sum += h[i], lut[i] = sat_u8((float)sum * lut_scale).
 *   4. Over the W x H pixels of the page itself: txf = (float)x * (1.0f / tile_w) - 0.5f, tx1 = floor(txf), xa = txf - (float)tx1,
 *      xa1 = 1.0f - xa, then tx2 = min(tx1 + 1, tiles_x - 1) and tx1 = max(tx1, 0); the same per row with 1.0f / tile_h; with v =
 *      src(y, x): dst = sat_u8((L(ty1,tx1)[v] * xa1 + L(ty1,tx2)[v] * xa) * ya1 + (L(ty2,tx1)[v] * xa1 + L(ty2,tx2)[v] * xa) * ya).
 *
 * equalizeHist of one channel: i = the first non-empty bin, total = W * H.  hist[i] == total: the page comes back as it is (the
 * reference fills it with i; the table of prl_hip_equalize_hist_lut is then the identity).  Else scale = 255.0f / (float)(total -
 * hist[i]), lut[v] = 0 for v <= i and, with sum += hist[v] from v = i + 1 on, lut[v] = sat_u8((float)sum * scale); dst = lut[src].
 *
 * EnhanceLocalContrastByCLAHE(in, out, clipLimit, equalizeHistFlag): CLAHE on the 8 x 8 grid with clipLimit on every channel,
 * then, with the flag, equalizeHist of that channel's result.
 *
 * Every entry with pages checks in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0);
 * PRL_ERR_BAD_CHANNELS (channels outside 1..4); PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row bytes, width or height
 * above 32768, tiles_x or tiles_y outside 1..PRL_CLAHE_MAX_TILES, a NaN clip_limit, overlapping source and destination).  d_src ==
 * d_dst with the same strides (in place) is allowed; any other overlap is PRL_ERR_BAD_ARG.  The *_batch_device entries enqueue on
 * `stream` and do not synchronise; they use the device's cached scratch (per page and channel 1280 bytes per tile, and 1280 for
 * the equalization).  The *_host entries take one page in host memory.  16-bit pages and larger grids are not provided.
 */

/* Step 1 and 2 for one page size, on the host: no device is needed.  PRL_ERR_EMPTY, then PRL_ERR_BAD_ARG as above. */
int prl_hip_clahe_geometry(int width, int height, int tiles_x, int tiles_y, double clip_limit, int* tile_w, int* tile_h, int* ext_w,
                           int* ext_h, int* clip);
/* Step 3 for one tile, on the host, by the code the kernel runs.  PRL_ERR_EMPTY for tile_area <= 0; PRL_ERR_BAD_ARG for a null
 * pointer, clip < 0, or bins that do not sum to tile_area. */
int prl_hip_clahe_tile_lut(const uint32_t hist[256], int clip, int tile_area, uint8_t lut[256]);
/* equalizeHist's table from one channel's histogram, on the host, by the code the kernel runs.  PRL_ERR_BAD_ARG for a null
 * pointer or a sum above 32768 * 32768; PRL_ERR_EMPTY for a sum of 0. */
int prl_hip_equalize_hist_lut(const uint32_t hist[256], uint8_t lut[256]);

/* Steps 1 to 3: d_luts[page][channel][tile_y][tile_x][256] bytes, the tables step 4 blends (any alignment). */
int prl_hip_clahe_luts_batch_device(int n_pages, int channels, double clip_limit, int tiles_x, int tiles_y, const uint8_t* d_src,
                                    size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_luts, void* stream);

int prl_hip_clahe_batch_device(int n_pages, int channels, double clip_limit, int tiles_x, int tiles_y, const uint8_t* d_src,
                               size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                               size_t dst_step, void* stream);
int prl_hip_clahe_host(int channels, double clip_limit, int tiles_x, int tiles_y, const uint8_t* src, size_t src_step, int width,
                       int height, uint8_t* dst, size_t dst_step);

int prl_hip_equalize_hist_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                       int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_equalize_hist_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/* The reference's helper: the 8 x 8 grid; `equalize` != 0: equalizeHist after CLAHE (the interpolation pass counts its own output,
 * so the pair costs three passes over the pixels). */
int prl_hip_enhance_local_contrast_batch_device(int n_pages, int channels, double clip_limit, int equalize, const uint8_t* d_src,
                                                size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                                size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_enhance_local_contrast_host(int channels, double clip_limit, int equalize, const uint8_t* src, size_t src_step, int width,
                                        int height, uint8_t* dst, size_t dst_step);

/* ---- prl::binarizeMokji and the grey-level co-occurrence matrix ------------------------------------------------------------ */

/*
 * prl::binarizeMokji(in, out, maxEdgeWidth = 3, minEdgeMagnitude = 20) (src/binarizations/binarizeMokji.cpp:35-94; Mokji & Abu-Bakar
 * 2007) on 8-bit pages of 1, 3 (BGR) or 4 (BGRA) channels in device memory; the result is one channel at the input's size.  Write E
 * for max_edge_width and M for min_edge_magnitude.
 *   gray = the 14-bit luma for 3 / 4 channels, else the page;  dil = cv::dilate(gray, RECT (2E + 1) x (2E + 1)), anchor at the
 *   centre, taps outside the page ignored;  matrix[dil(y, x)][gray(y, x)] += 1 over y in [E, height - E), x in [E, width - E), from
 *   zeros (the reference never initialises its matrix: zeros are the only defined reading);  nom = sum of (m + n) matrix[n][m] and
 *   den = sum of matrix[n][m] over the pairs with n - m >= M;  t = (int)(0.5 * nom / den + 0.5) in double, which equals
 *   (nom + den) / (2 den) in integers for every matrix a page can give (nom < 2^53);  dst = gray > t ? 255 : 0.
 * Exact.  Where the reference is undefined: den == 0 (an empty interior: width <= 2E or height <= 2E; no pair with n - m >= M)
 * makes it convert a NaN to int, which on x86 is INT_MIN, and cv::threshold with a negative threshold sets every pixel: the page
 * comes out all 255 and the threshold is reported as -1.  M >= 256 (the reference wraps 256 - M and reads outside its matrix) is
 * "no pair", the same.  Limit: the dilation's element is at most 255 wide, so E <= 127 unless the interior is empty.
 * The gray and dilated planes, the dilation's intermediate plane and one 256 x 256 uint32 matrix per page live in the device's
 * cached scratch; the threshold stays on the device.  d_src == d_dst with the same strides (in place) is allowed for 1-channel
 * pages; any other overlap returns PRL_ERR_BAD_ARG, and d_src is otherwise never written.  width, height <= 32768.  Enqueues on
 * `stream`, no synchronisation.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_ARG (max_edge_width < 1,
 * min_edge_magnitude < 1, max_edge_width > 127 with a non-empty interior); PRL_ERR_BAD_CHANNELS (channels other than 1, 3, 4);
 * PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row bytes, width or height above the limit, overlapping source and
 * destination).
 */
int prl_hip_binarize_mokji_batch_device(int n_pages, int channels, int max_edge_width, int min_edge_magnitude, const uint8_t* d_src,
                                        size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                        size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_binarize_mokji_host(int channels, int max_edge_width, int min_edge_magnitude, const uint8_t* src, size_t src_step, int width,
                                int height, uint8_t* dst, size_t dst_step);

/* The threshold alone: d_thresholds[page] = t as above, -1 where den == 0.  Same source arguments, checks and workspace. */
int prl_hip_mokji_thresholds_batch_device(int n_pages, int channels, int max_edge_width, int min_edge_magnitude, const uint8_t* d_src,
                                          size_t src_page_stride, size_t src_step, int width, int height, int32_t* d_thresholds,
                                          void* stream);

/*
 * The co-occurrence matrix of two 1-channel planes a and b of the same size: d_cooc[page][b(y, x)][a(y, x)] = the number of pixels
 * of the interior y in [border, height - border), x in [border, width - border) with that pair of values, for the pairs with
 * b - a >= min_diff; every other bin is 0.  min_diff == 0 counts every pair, those with b < a included (the square matrix is the
 * contract); min_diff == 256 counts none.  d_cooc holds 256 * 256 uint32 per page; the call overwrites it.  An empty interior gives
 * zeros.  Checked in this order: PRL_ERR_EMPTY; PRL_ERR_BAD_ARG (border < 0, min_diff outside 0..256); PRL_ERR_BAD_ARG (null
 * pointer, negative n_pages, step < width, width or height above 32768).  Enqueues on `stream`, no synchronisation, no workspace.
 */
int prl_hip_cooccurrence_batch_device(int n_pages, int border, int min_diff, const uint8_t* d_a, size_t a_page_stride, size_t a_step,
                                      const uint8_t* d_b, size_t b_page_stride, size_t b_step, int width, int height, uint32_t* d_cooc,
                                      void* stream);

/*
 * Step 6 on the host, no device needed: *threshold = (nom + den) / (2 den) over the pairs n - m >= min_edge_magnitude of
 * cooc[n * 256 + m], or -1 where den == 0 (min_edge_magnitude >= 256 included); the kernel runs the same inline code.
 * PRL_ERR_BAD_ARG for a null pointer or min_edge_magnitude < 1.
 */
int prl_hip_mokji_threshold(const uint32_t cooc[256 * 256], int min_edge_magnitude, int* threshold);

/* ---- focus measures: the blur detection of src/detectors/blurDetection.cpp (LAPM, LAPV, TENG, GLVN) ------------------------- */

#define PRL_FOCUS_SUM_P 0       /* sum of p */
#define PRL_FOCUS_SUM_P2 1      /* sum of p^2 */
#define PRL_FOCUS_SUM_LAP 2     /* sum of L */
#define PRL_FOCUS_SUM_LAP2 3    /* sum of L^2 */
#define PRL_FOCUS_SUM_LAPM4 4   /* sum of |X| + |Y| */
#define PRL_FOCUS_SUM_TENG 5    /* sum of Gx^2 + Gy^2 */
#define PRL_FOCUS_LAPM 0
#define PRL_FOCUS_LAPV 1
#define PRL_FOCUS_TENG 2
#define PRL_FOCUS_GLVN 3

/*
 * The four focus measures of the reference (blurDetection.cpp:32-83; its prl::isBlurred returns false and calls none of them) on
 * 8-bit pages of 1, 3 or 4 interleaved channels: one read-only pass (focus.hip) leaves six integer sums per page AND channel, and
 * the measures follow from the sums on the host in float64.  Write p(y, x) for one channel of one page and N = width * height.
 * Neighbours outside the page are BORDER_REFLECT_101 (cv::borderInterpolate: index -1 -> 1, n -> n - 2, a side of length 1 maps
 * everything to 0).  Every sum runs over all N pixels, in int64:
 *   [0] S_P = sum p;  [1] S_P2 = sum p^2;
 *   [2] S_LAP = sum L, L = p(y-1, x) + p(y+1, x) + p(y, x-1) + p(y, x+1) - 4 p(y, x): cv::Laplacian(src, CV_64F), ksize 1 (:53);
 *   [3] S_LAP2 = sum L^2;
 *   [4] S_LAPM4 = sum (|X| + |Y|), X = the (-1, 2, -1) filter along x of the rows y-1, y, y+1 weighted (1, 2, 1), Y the same with
 *       the axes exchanged: four times Lx, Ly of :34-41 (cv::getGaussianKernel(3, -1) is exactly (1/4, 1/2, 1/4));
 *   [5] S_TENG = sum (Gx^2 + Gy^2), Gx, Gy = cv::Sobel(..., teng_ksize), unnormalised: (-1, 0, 1) along the axis and, for
 *       teng_ksize == 3, (1, 2, 1) across it; teng_ksize == 1: (-1, 0, 1) alone.  Other sizes and the Scharr kernel are
 *       PRL_ERR_BAD_ARG (from 5 on a sum can pass 2^53 on a large page, where the order of OpenCV's double sum would show).
 * Bounds: |L| <= 1020, |X|, |Y| <= 2040, Gx^2 + Gy^2 <= 2 * 1020^2; on a 32768 x 32768 page the largest sum is 2.3e15 < 2^53, so
 * every intermediate of the reference (an integer or a multiple of 1/4) and every sum is exact in float64 in any order.
 * The measures of a channel from its sums, float64, one rounding per written operation, scale = 1.0 / N (cv::mean and
 * cv::meanStdDev as sum * scale [upstream, generic path]: the canonical choice, parity unpinned as in DESIGN.md §2):
 *   [0] LAPM = (S_LAPM4 / 4.0) * scale
 *   [1] LAPV: m = S_LAP * scale; sd = sqrt(max(S_LAP2 * scale - m * m, 0.0)); sd * sd
 *   [2] TENG = S_TENG * scale
 *   [3] GLVN: mu = S_P * scale; sg = sqrt(max(S_P2 * scale - mu * mu, 0.0)); (sg * sg) / mu  (an all-zero page: NaN, as 0 / 0 is
 *       in the reference)
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_ARG (teng_ksize other
 * than 1 and 3); PRL_ERR_BAD_CHANNELS (channels other than 1, 3, 4); PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row
 * bytes, width or height above 32768).  n_pages == 0 is PRL_OK.
 */

/*
 * d_sums[page][channel][6] (device memory, int64) = the six sums; the call overwrites it.  Pages and rows may be strided.  Enqueues
 * on `stream` and does not synchronise; d_src is never written; no workspace.  The workgroups' partial sums meet in d_sums by
 * 64-bit integer atomics: the result does not depend on their order.
 */
int prl_hip_focus_sums_batch_device(int n_pages, int channels, int teng_ksize, const uint8_t* d_src, size_t src_page_stride,
                                    size_t src_step, int width, int height, int64_t* d_sums, void* stream);

/*
 * One page in host memory: measures[channel][4]; sums (optional, may be null) receives [channel][6].  Same checks (no page count).
 */
int prl_hip_focus_measures_host(int channels, int teng_ksize, const uint8_t* src, size_t src_step, int width, int height,
                                double* measures, int64_t* sums);

/*
 * The four measures of one channel from its six sums, no device needed.  PRL_ERR_EMPTY for width or height <= 0; PRL_ERR_BAD_ARG
 * for a null pointer or a side above 32768.
 */
int prl_hip_focus_from_sums(const int64_t sums[6], int width, int height, double measures[4]);

/* ---- basicDeblur: the float32 cv::GaussianBlur of 8-bit pages and the unsharp mask of src/deblur/basicDeblur.cpp:33-70 ------- */

#define PRL_GAUSS_MAX_SIDE 255   /* the largest kernel side; above it PRL_ERR_BAD_WINDOW */

/*
 * prl::basicDeblur(in, out, gaussianKernelSize = 0, sigmaX = 9.0, sigmaY = 0.0, imageWeight = 0.75) on 8-bit pages of 1 to 4
 * interleaved channels.  For every channel, with p the byte of a sample:
 *   1. x = (float)p
 *   2. g = cv::GaussianBlur(x, Size(k, k), sigmaX, sigmaY) in float32, BORDER_REFLECT_101
 *   3. t = (x * alpha + g * beta) + 0.0f, alpha = (float)(2 * imageWeight), beta = (float)(2 * imageWeight - 2) (each computed in
 *      float64 and rounded once): cv::addWeighted on CV_32F
 *   4. out = saturate_u8(cvRound(t)): half to even; NaN, +-inf and what lies outside int32 give 0
 * One fused kernel (deblur.hip) does the four steps; its only global write is the destination byte.  The rules of step 2, as
 * cv::GaussianBlur has them for a depth that is not 8-bit (gauss.h states them in C++, tests/deblur_ref.py in numpy):
 *   sigmaY            sigmaY <= 0 -> sigmaY = sigmaX.
 *   derived side      a side k <= 0 with its sigma > 0 is cvRound(sigma * 4 * 2 + 1) | 1, per axis (the factor is 4, not 3: the depth
 *                     is not 8-bit): k = 0, sigmaX = 9 gives 73 x 73; k = 0, sigmaX = 1, sigmaY = 3 gives 9 x 25.
 *   valid side        after that step a side must be positive and odd, and here at most PRL_GAUSS_MAX_SIDE.
 *   weights           cv::getGaussianKernel(n, max(sigma, 0), CV_32F): the fixed tables for n = 1, 3, 5, 7 ({1}, {1/4, 1/2, 1/4},
 *                     {1/16, 1/4, 3/8, 1/4, 1/16}, {1/32, 7/64, 7/32, 9/32, ...}) apply only when sigma <= 0; otherwise
 *                     s = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8, t_i = exp(-0.5 / (s * s) * x_i * x_i) with
 *                     x_i = i - (n - 1) * 0.5 in float64, the sum in index order, w_i = (float)(t_i * (1 / sum)).
 *   shared weights    ky is kx when the sides are equal and |sigmaX - sigmaY| < DBL_EPSILON; else ky is made from its own side and sigma.
 *   1 x 1             a copy: g = x (the only weight is 1.0f).
 *   thin pages        a page of one row or one column gets no special case (the default border type carries no BORDER_ISOLATED):
 *                     it is filtered through its reflections.
 *   border            cv::borderInterpolate(i, len, BORDER_REFLECT_101) with its loop: -1 -> 1, len -> len - 2; a page narrower
 *                     than the radius reflects more than once; len == 1 gives index 0.
 *   operation order   row pass with n >= 7 (and n == 1): w_0 x_0, then + w_k x_k for k ascending; row pass with n = 3 or 5: the centre
 *                     x_r w_r, then + (x_(r+k) + x_(r-k)) w_(r+k) for k = 1 .. r; column pass: the centre w_r v_r, then
 *                     + w_(r+k) (v_(r+k) + v_(r-k)) outward.  Every product and every sum is one float32 rounding, never contracted:
 *                     the order DESIGN.md §4.4c pins for ADAPTIVE_THRESH_GAUSSIAN_C.  Parity with an OpenCV build is unpinned (§2).
 * On interleaved pages the row pass is a 1-D filter over samples with tap stride `channels`, reflected on the pixel index.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_WINDOW (a kernel size
 * that does not fit an int; a side <= 0 whose sigma is not > 0, a NaN included; an even side; a side, given or derived, above
 * PRL_GAUSS_MAX_SIDE); PRL_ERR_BAD_ARG (channels outside 1..4; a NaN or infinite sigma or weight; a null pointer; negative n_pages;
 * a step below the row bytes; a float destination or a step of it that is no multiple of 4; width or height above 32768; source
 * and destination sharing a byte: in place is not allowed, every output reads its neighbours' inputs).  n_pages == 0 is PRL_OK.
 * Not built: sides above PRL_GAUSS_MAX_SIDE, depths other than 8-bit, and the reference's wienerFilter (a DFT).
 */

/*
 * n pages per call; pages and rows may be strided.  Enqueues on `stream` and does not synchronise; needs no workspace; d_src is
 * never written.  kernel_size is the reference's size_t (both sides); a value <= 0 derives the sides from the sigmas.
 */
int prl_hip_basic_deblur_batch_device(int n_pages, int channels, long long kernel_size, double sigma_x, double sigma_y,
                                      double image_weight, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                      int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
/* One page in host memory, through the staging area.  Same checks (no page count; the two may not overlap either). */
int prl_hip_basic_deblur_host(int channels, long long kernel_size, double sigma_x, double sigma_y, double image_weight,
                              const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/*
 * Step 2 alone, the float32 cv::GaussianBlur(Size(kernel_w, kernel_h), sigma_x, sigma_y) of 8-bit pages: the same kernel writing g
 * instead of the byte.  d_dst holds float32 samples, width * channels a row; dst_page_stride and dst_step are in BYTES and, like
 * d_dst, multiples of 4.  The same checks in the same order.
 */
int prl_hip_gaussian_blur_f32_batch_device(int n_pages, int channels, long long kernel_w, long long kernel_h, double sigma_x,
                                           double sigma_y, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                           int height, float* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_gaussian_blur_f32_host(int channels, long long kernel_w, long long kernel_h, double sigma_x, double sigma_y,
                                   const uint8_t* src, size_t src_step, int width, int height, float* dst, size_t dst_step);

/*
 * The rules on the host, no device needed.  prl_hip_gaussian_blur_size: the sides cv::GaussianBlur(Size(kernel_w, kernel_h),
 * sigma_x, sigma_y) filters with (sigma_y <= 0 -> sigma_x, the derived side); PRL_ERR_BAD_WINDOW as above, PRL_ERR_BAD_ARG for a
 * null pointer or a NaN or infinite sigma.  prl_hip_gaussian_kernel_f32: the n weights of cv::getGaussianKernel(n, sigma, CV_32F)
 * (sigma <= 0: the tables up to 7, else the sigma derived from n); PRL_ERR_BAD_WINDOW for n <= 0, even or above PRL_GAUSS_MAX_SIDE,
 * PRL_ERR_BAD_ARG for a null pointer or a NaN or infinite sigma.
 */
int prl_hip_gaussian_blur_size(long long kernel_w, long long kernel_h, double sigma_x, double sigma_y, int* out_w, int* out_h);
int prl_hip_gaussian_kernel_f32(int n, double sigma, float* w);

/* ---- the 8-bit cv::GaussianBlur: 8.8 fixed-point weights, integer arithmetic (blur8.hip, gauss8.h) ------------ */

/*
 * cv::GaussianBlur(src, dst, Size(kernel_w, kernel_h), sigma_x, sigma_y) on 8-bit pages of 1 to 4 interleaved channels, as the
 * OpenCV line 4.1.1 and later filters a CV_8U image without an accelerator [upstream: smooth.dispatch.cpp / fixedpoint.inl.hpp,
 * stated from memory; parity unpinned, DESIGN.md §2].  All of it is integer: exact and independent of the order of summation.
 *   sides             each odd and in 1 .. PRL_GAUSS_MAX_SIDE (a side <= 0, which OpenCV derives from sigma, is not taken).
 *   sigmas            sigma_y <= 0 -> sigma_y = sigma_x; a sigma <= 0 for a side of n is ((n - 1) * 0.5 - 1) * 0.3 + 0.8.
 *   float64 weights   sigma <= 0 and n in {1, 3, 5, 7}: the tables {1}, {.25, .5, .25}, {.0625, .25, .375, .25, .0625},
 *                     {.03125, .109375, .21875, .28125, .21875, .109375, .03125}; otherwise k_i = exp(-0.5 / sigma^2 * (i - (n - 1) / 2)^2)
 *                     divided by the sum of all k (index order).
 *   8.8 weights       by error diffusion: err = 0; for i = 0 .. n / 2 - 1: adj = k_i * 256 + err, v = cvRound(adj) (ties to even),
 *                     err = adj - v, w_i = w_(n-1-i) = v; the centre w_(n/2) = 256 - the sum of the others.  A side sums to 256.
 *                     Side 3 at sigma 0: 64 128 64; 5: 16 64 96 64 16; 9: 4 13 30 51 60 51 30 13 4.  The centre need not be the
 *                     largest weight (25 at sigma 0: 24 between two 25s).  OpenCV evaluates exp in soft-float, this library with
 *                     std::exp: no adj of any odd n <= 255 (sigma 0, or sigma 0.1, 0.2 .. 100) lies within 1e-8 of a rounding tie,
 *                     far above the error of either (tests/test_localotsu_cpu.py re-derives the margin).
 *   the filter        per channel, with R(p, len) = cv::borderInterpolate(p, len, BORDER_REFLECT_101) (as for pyrDown above), rx = nx / 2,
 *                     ry = ny / 2:  h(x, y) = sum_i wx_i * p(R(x + i - rx, W), y)  (at most 255 * 256: 16 bits),
 *                     dst(x, y) = (sum_j wy_j * h(x, R(y + j - ry, H)) + 32768) >> 16  (32 bits).  Nothing saturates, since a side
 *                     sums to 256; a 1 x 1 kernel copies; thin pages are filtered through their reflections.
 * NOT restated: the rule of OpenCV 3.4.x - 4.1.0 (every weight rounded on its own) and accelerator builds (IPP, OpenVX).  Another
 * weight rule is a change of the host table alone: the kernel takes the weights as they come (prl_hip_sep_filter_u8_batch_device).
 * One fused kernel (blur8.hip): row pass into an LDS ring of 16-bit row results, column pass, the rounded byte; its only global
 * write is the destination.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_WINDOW (a side <= 0, even
 * or above PRL_GAUSS_MAX_SIDE); PRL_ERR_BAD_ARG (channels outside 1..4; a NaN or infinite sigma; the explicit-weight entry: a null
 * weight pointer or a side whose weights sum to more than 256; a null page pointer; negative n_pages; a step below the row bytes;
 * width or height above 32768; source and destination sharing a byte).  n_pages == 0 is PRL_OK.
 */

/* The n 8.8 weights of a side, on the host, no device needed.  PRL_ERR_BAD_WINDOW for n <= 0, even or above PRL_GAUSS_MAX_SIDE;
 * PRL_ERR_BAD_ARG for a null pointer or a NaN or infinite sigma. */
int prl_hip_gaussian_kernel_u8(int n, double sigma, uint16_t* w);

/*
 * The filter alone with explicit 8.8 weights in host memory (wx: nx weights in tap order, wy: ny; they need not be symmetric): the
 * seam the kernel is tested at.  n pages per call; pages and rows may be strided.  Enqueues on `stream` and does not synchronise;
 * needs no workspace; d_src is never written.
 */
int prl_hip_sep_filter_u8_batch_device(int n_pages, int channels, const uint16_t* wx, int nx, const uint16_t* wy, int ny,
                                       const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width, int height,
                                       uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_gaussian_blur_u8_batch_device(int n_pages, int channels, int kernel_w, int kernel_h, double sigma_x, double sigma_y,
                                          const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width, int height,
                                          uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
/* One page in host memory, through the staging area.  Same checks (no page count; the two may not overlap either). */
int prl_hip_gaussian_blur_u8_host(int channels, int kernel_w, int kernel_h, double sigma_x, double sigma_y, const uint8_t* src,
                                  size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/* ---- CannyEdgeDetection (src/imageLibCommon.cpp:244-324): the edge stage of binarizeLocalOtsu, COCOCLUST and FBCITB (edgedet.hip) --- */

/*
 * CannyEdgeDetection(image, result, GaussianBlurKernelSize, CannyUpperThresholdCoeff, CannyLowerThresholdCoeff, CannyMorphIters)
 * on 8-bit pages of 1 to 4 interleaved channels -> width x height maps of 0 / 255.  Per channel:
 *   1. the 8-bit cv::GaussianBlur above with Size(blur_size, blur_size) and sigma 0
 *   2. t = the Otsu value of the blurred plane (getThreshVal_Otsu_8u: float64 scan, scale 1 / (width * height)), an integer in 0 .. 255
 *   3. upper = upper_coeff * t, lower = lower_coeff * upper, in float64
 *   4. cv::Canny(lower, upper) as stated under "pyramid, edge map, resize" (aperture 3, L1 magnitude)
 *   5. morph_iterations > 0: cv::dilate 3 x 3 that many times, then cv::erode as many; < 0: erode, then dilate
 * and the channels' maps are OR-ed.  The thresholds differ per page and per channel; t stays on the device: the host uploads the
 * (low, high) pair of each of the 256 values t can take, and the kernel of step 4 looks its page's pair up.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY; PRL_ERR_BAD_ARG in the reference's order (blur_size < 3; a
 * coefficient outside [0, 1], a NaN included; lower_coeff > upper_coeff; an even blur_size - cv::GaussianBlur's assertion);
 * PRL_ERR_BAD_WINDOW (blur_size above PRL_GAUSS_MAX_SIDE); PRL_ERR_BAD_CHANNELS (not 1 .. 4); PRL_ERR_BAD_ARG (|morph_iterations| above
 * 255; a null pointer; negative n_pages; a step below the row bytes; width or height above 32768; source and destination sharing
 * a byte).  n_pages == 0 is PRL_OK.  Waits for the stream (cv::Canny's hysteresis does).
 */
int prl_hip_canny_edge_detection_batch_device(int n_pages, int channels, int blur_size, double upper_coeff, double lower_coeff,
                                              int morph_iterations, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                              int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_canny_edge_detection_host(int channels, int blur_size, double upper_coeff, double lower_coeff, int morph_iterations,
                                      const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/* ---- binarizeLocalOtsu (src/binarizations/binarizeLocalOtsu.cpp:37-163): localotsu.hip, contour.h ------------------------------- */

/*
 * The cv::boundingRect (x, y, width, height) of every contour of at least 3 points that
 * cv::findContours(map, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) finds on an 8UC1 map in host memory (non-zero = foreground), in
 * discovery order: what binarizeLocalOtsu keeps of its contours (RemoveChildrenContours on a flat hierarchy drops the contours of
 * fewer than 3 points).  The scan is OpenCV's retrieval mode 0, literally [upstream, from memory; parity unpinned]: per row, lnbd
 * starts at the frame column; at a change prev -> p that is not 0 -> 1: nothing if p != 0 or prev < 1, else a hole start, which
 * moves lnbd to x - 1 when prev is a traced pixel (prev & -2) and is never traced; an outer start (0 -> 1) is skipped when the pixel
 * at lnbd is positive; after either, prev = p (read again after a trace) and lnbd = x when prev & -2.  Borders are followed and
 * marked as cv::findContours does (see "document contour").  The scan is restated as written, not replaced by the topological
 * rule "the outermost component".  *n_found: all contours; *n_kept: those of at least 3 points.  With n_kept > max_rects only the counts are
 * written (call again with room).  Host code, no device: plain C++ on the calling thread.
 * PRL_ERR_EMPTY for width or height <= 0; PRL_ERR_BAD_ARG for a null pointer, a step below the width, a negative max_rects or a
 * side above 32768.
 */
int prl_hip_external_rects(const uint8_t* map, size_t step, int width, int height, int32_t* rects, int max_rects, int* n_found,
                           int* n_kept);

/*
 * Rule R: what the scan above gives, said without a scan (components.h, components.hip; the evidence: DESIGN.md §4.4p).
 * Foreground is every non-zero byte.  Foreground components are 8-connected, background components 4-connected.  A background
 * component is OUTER if it holds a pixel of the page's border (the page is thought of as surrounded by background).  A
 * foreground component's FIRST PIXEL is its smallest y * width + x.  A foreground component is EXTERNAL if its first pixel has
 * x == 0 or if the pixel to the left of it belongs to an outer background component.  n_found is the number of external
 * components.  An external component is KEPT unless it is a straight one-pixel line: area == max(bw, bh) and (min(bw, bh) == 1
 * or bw == bh), a single pixel included (the contours of fewer than 3 points).  The result is the bounding rectangles
 * (x, y, bw, bh) of the kept components in increasing order of first pixel.  Everything is integer: the device entries below
 * and prl_hip_external_rects agree byte for byte (tests/test_components_cpu.py pins the equivalence on the host).
 *
 * prl_hip_connected_components_batch_device: the foreground components of n_pages maps in device memory, `connectivity` 8 or 4.
 * d_labels (device, int32, rows labels_step BYTES apart, pages labels_page_stride bytes; NULL: not wanted): 0 for background,
 * 1 .. K for the page's components in increasing order of first pixel.  n_components (HOST, n_pages values): K of every page.
 * d_stats (device, NULL: not wanted): five int32 per component - left, top, width, height, area - page after page in label
 * order, written only if the components of all pages together are at most max_components (else the labels and the counts alone:
 * call again with room).  Inside, ONE int32 plane per page holds, for every pixel, the smallest linear index of its own-class
 * component (foreground at `connectivity`, background 4-connected, labelled in the same passes): a union-find per 32 x 32 tile in
 * LDS, unions across the tile seams by atomic minimum, a flatten pass; a component's number is an ordered prefix count of the
 * roots.  Every kernel finishes for any input: labels only decrease, and no workgroup waits for another.
 *
 * prl_hip_external_rects_batch_device: rule R on n_pages maps in device memory.  n_found, n_kept (HOST, n_pages values each)
 * and rect_offsets (HOST, n_pages + 1 values: the kept rectangles of page i are [rect_offsets[i], rect_offsets[i + 1])) are
 * always written; d_rects (device, x, y, width, height each, page after page) only if rect_offsets[n_pages] <= max_rects (the
 * capacity rule of prl_hip_external_rects: else the counts alone, d_rects untouched).  The total is known only after the last
 * page: a batch that needs more than one chunk of pages (4 B of labels a pixel against the workspace budget) or more than one
 * statistics pass (2^20 components) is therefore labelled twice, once for the counts and once to write.
 *
 * Both wait for the stream (the counts are host values).  Checked in this order, before any device is touched: PRL_ERR_EMPTY;
 * PRL_ERR_BAD_ARG (a connectivity other than 4 and 8; a null map or count pointer; negative n_pages; a step below the row bytes;
 * a side above 32768; a negative capacity, or a positive one with a null array; labels not aligned to 4 bytes).  n_pages == 0
 * is PRL_OK.
 */
int prl_hip_connected_components_batch_device(int n_pages, int connectivity, const uint8_t* d_map, size_t map_page_stride, size_t map_step,
                                              int width, int height, int32_t* d_labels, size_t labels_page_stride, size_t labels_step,
                                              int32_t* n_components, int32_t* d_stats, int max_components, void* stream);
int prl_hip_external_rects_batch_device(int n_pages, const uint8_t* d_map, size_t map_page_stride, size_t map_step, int width, int height,
                                        int32_t* d_rects, int max_rects, int32_t* rect_offsets, int32_t* n_found, int32_t* n_kept,
                                        void* stream);

#define PRL_RECT_OTSU_SMALL_AREA 4096   /* a rectangle of at most this many pixels is one wavefront's; a larger one is split */

/*
 * The per-rectangle Otsu and the paint: d_dst = 255 everywhere except, for every rectangle, 0 where (v ^ 255) != 0 with
 * v = p > thr ? imax : 0, p the byte of the gray page, imax = saturate_u8(cvRound(max_value)) and thr = getThreshVal_Otsu_8u of the
 * rectangle's own histogram with scale = 1 / (w * h), in float64 (cv::threshold(THRESH_OTSU) on a copy of the rectangle, then
 * setTo(0, v ^ 255): binarizeLocalOtsu.cpp:145-160).  So with imax == 255 a pixel of a rectangle is black iff p <= thr, and with
 * any other imax the whole rectangle is black.  Rectangles may overlap: only 0 is ever stored, the result does not depend on
 * their order.  rect_offsets (HOST memory, n_pages + 1 values, the first 0, not decreasing; copied before the call returns): the rectangles of page i are
 * d_rects[4 * rect_offsets[i]] .. d_rects[4 * rect_offsets[i + 1]] (DEVICE memory: x, y, width, height each); a rectangle that does
 * not lie on the page is ignored.  d_thresholds (device, one int32 per rectangle) receives every thr; NULL: not wanted.
 * A rectangle of at most PRL_RECT_OTSU_SMALL_AREA pixels is one wavefront's work (bins in LDS, scan, store); a larger one is split
 * across workgroups (bins by atomics into a slab of the workspace, a threshold launch, a paint launch).  Enqueues on `stream`.
 * Checked in this order: PRL_ERR_EMPTY; PRL_ERR_BAD_ARG (max_value outside [0, 255] or a NaN; a null page pointer; negative n_pages;
 * a step below the width; a side above 32768; gray and destination sharing a byte; null or malformed rect_offsets; d_rects null
 * with rectangles to read).
 */
int prl_hip_rect_otsu_batch_device(int n_pages, const int32_t* rect_offsets, const int32_t* d_rects, double max_value, const uint8_t* d_gray,
                                   size_t gray_page_stride, size_t gray_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                   size_t dst_step, int32_t* d_thresholds, void* stream);

/*
 * prl::binarizeLocalOtsu(in, out, maxValue = 255, CLAHEClipLimit = 0, GaussianBlurKernelSize = 19, CannyUpperThresholdCoeff = 0.15,
 * CannyLowerThresholdCoeff = 0.01, CannyMorphIters = 1) on pages of 1, 3 or 4 interleaved channels -> width x height masks:
 *   1. gray: a colour page through cv::COLOR_RGB2GRAY, (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14 (the reference converts its BGR
 *      pages as RGB: the weights of prl_hip_bgr2gray_batch_device, swapped); of four channels the fourth is ignored
 *   2. clahe_clip_limit > 0: EnhanceLocalContrastByCLAHE(clip, equalize = true) on the gray page
 *   3. CannyEdgeDetection above; 4. cv::dilate 3 x 3, three iterations
 *   5. one read-back of the edge maps; 6. prl_hip_external_rects of each on the host thread pool
 *   7. the rectangles go up; prl_hip_rect_otsu_batch_device's kernels on the gray page of step 2 (not the blurred one)
 * (steps 5 and 6 on the device - the labels of the maps, rule R's rectangles written where step 7 reads them, only the per-page
 * counts crossing to the host - are built and give the same bytes, but measured no faster: the test-hooks build selects them with
 * PRL_HIP_LO_HOST_RECTS=0)
 * n_found / n_kept (host memory, n_pages values each, or NULL): the contours and the rectangles of every page.  A page without
 * contours (n_found == 0) is all 255; the C++ function throws the reference's std::invalid_argument for it.
 * Checked in this order: PRL_ERR_EMPTY; PRL_ERR_BAD_ARG (max_value outside [0, 255]; CannyEdgeDetection's argument checks in its
 * order); PRL_ERR_BAD_WINDOW (blur_size above PRL_GAUSS_MAX_SIDE); PRL_ERR_BAD_CHANNELS (not 1, 3 or 4); PRL_ERR_BAD_ARG (a NaN clip
 * limit, |morph_iterations| above 255, then the pages as above).  Waits for the stream.
 */
int prl_hip_binarize_local_otsu_batch_device(int n_pages, int channels, double max_value, double clahe_clip_limit, int blur_size,
                                             double upper_coeff, double lower_coeff, int morph_iterations, const uint8_t* d_src,
                                             size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                             size_t dst_page_stride, size_t dst_step, int32_t* n_found, int32_t* n_kept, void* stream);
int prl_hip_binarize_local_otsu_host(int channels, double max_value, double clahe_clip_limit, int blur_size, double upper_coeff,
                                     double lower_coeff, int morph_iterations, const uint8_t* src, size_t src_step, int width, int height,
                                     uint8_t* dst, size_t dst_step, int32_t* n_found, int32_t* n_kept);

/* ---- cv::bilateralFilter on 8-bit planes (bilateral.hip, bilateral.h) ----------------------------------------- */

#define PRL_BILATERAL_MAX_SIDE 31    /* the largest side 2 * radius + 1; above it PRL_ERR_BAD_ARG with a detail string */
#define PRL_BILATERAL_MAX_TAPS 708   /* the taps of that side: the lattice points of a disc of radius 15, without its centre */

/*
 * cv::bilateralFilter(src, dst, d, sigmaColor, sigmaSpace) on 8-bit pages of 1 to 4 interleaved channels, EVERY CHANNEL FILTERED AS A
 * PLANE OF ITS OWN (the one-channel path of bilateralFilter_8u; the only form the reference calls: binarizeFBCITB splits its
 * channels, binarizeNativeAdaptive filters a mask), BORDER_REFLECT_101.  The rule is ONE form, that of the OpenCV 4.x scalar /
 * baseline path whose tap list leaves the centre pixel out [upstream: bilateral_filter.dispatch.cpp / .simd.hpp, stated from memory,
 * the release that introduced it not pinned; parity unpinned, DESIGN.md §2]:
 *   sigmas     a sigma <= 0 becomes 1.
 *   radius     d <= 0: cvRound(sigmaSpace * 1.5) (ties to even), else d / 2; then max(radius, 1).  The side is 2 * radius + 1, here
 *              at most PRL_BILATERAL_MAX_SIDE.
 *   tables     float64 gc = -0.5 / sigmaColor^2, gs = -0.5 / sigmaSpace^2; color[i] = (float)std::exp(i * i * gc), i = 0 .. 255;
 *              taps (i, j) in row-major order, i (rows) outer, both from -radius to radius: r = std::sqrt((double)i * i + (double)j * j);
 *              a tap with r > radius is skipped, and so is the centre; space[k] = (float)std::exp(r * r * gs).  12 taps at d = 5.
 *   per pixel  c its byte, v a tap's byte; all in float32, every operation rounded on its own (no fused multiply-add), denormal
 *              weights kept (color[14] at sigmaColor 1 is one): sum = wsum = 0; for every tap in order w = space[k] * color[|v - c|],
 *              sum += v * w, wsum += w; dst = (uchar)cvRound((sum + c) / (wsum + 1.f)), an IEEE division, ties to even.
 * NOT restated: the centre-first form of older lines (the centre a tap of its own, sum / wsum), which gives other bytes; the
 * joint colour distance of 3-channel images; float32 input; other borders; accelerator builds (IPP).
 * Pages smaller than the radius are filtered through their reflections.  One kernel; needs no workspace; its only global write
 * is the destination.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_ARG (channels outside 1..4; a
 * NaN or infinite sigma; a side above PRL_BILATERAL_MAX_SIDE, with a detail string; a null page pointer; negative n_pages; a step
 * below the row bytes; width or height above 32768; source and destination sharing a byte: src == dst is refused).  n_pages == 0 is
 * PRL_OK.
 */

/* The rules on the host, no device needed: *radius, *n_taps, and where the pointer is not NULL the taps' offsets dy / dx and
 * space weights in tap order (room for PRL_BILATERAL_MAX_TAPS each) and the 256 colour weights.  PRL_ERR_BAD_ARG for a null radius
 * or n_taps, a NaN or infinite sigma, or a side above the limit (*radius is still written, *n_taps = 0). */
int prl_hip_bilateral_tables(int d, double sigma_color, double sigma_space, int* radius, int* n_taps, int8_t* dy, int8_t* dx,
                             float* space_weight, float* color_weight);
/* n pages per call; pages and rows may be strided.  Enqueues on `stream` and does not synchronise; d_src is never written. */
int prl_hip_bilateral_filter_batch_device(int n_pages, int channels, int d, double sigma_color, double sigma_space, const uint8_t* d_src,
                                          size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                          size_t dst_page_stride, size_t dst_step, void* stream);
/* One page in host memory, through the staging area.  Same checks (no page count; the two may not overlap either). */
int prl_hip_bilateral_filter_host(int channels, int d, double sigma_color, double sigma_space, const uint8_t* src, size_t src_step,
                                  int width, int height, uint8_t* dst, size_t dst_step);

/* ---- binarizeFBCITB (src/binarizations/binarizeFBCITB.cpp:73-404): fbcitb.hip, fbcitb.h, contour.h; DESIGN.md §4.4q ------------- */

/*
 * The variance mask (binarizeFBCITB.cpp:172-183): MatToLocalVarianceMap(page, map, 3) > threshold on every channel, the channels
 * AND-ed to a 0 / 255 byte plane (convertScaleAbs(., 255, 0) changes nothing on it).  Pages of 1 or 3 channels; a gray page stands
 * for three equal channels.  The map is max((float)D * (1.f / (9.f * 9.f)), 0.01f) with D = 9 * sum(p^2) - sum(p)^2 over the 3 x 3
 * window of the edge-replicated page, an integer below 2^24 (binarizeByLocalVariances above).  The comparison is made in float32
 * against (float)threshold [upstream: cv::compare converts the scalar to the array's depth; parity unpinned].  The map is monotone
 * in D, so the host finds once per call the smallest D that passes and the kernel compares integers: a threshold below the 0.01
 * floor passes every pixel, a NaN or one above the largest map value none.
 * PRL_ERR_EMPTY; PRL_ERR_BAD_CHANNELS (not 1 or 3); PRL_ERR_BAD_ARG (the pages, as for the filters above).  Enqueues on `stream`.
 */
int prl_hip_variance_mask_batch_device(int n_pages, int channels, double threshold, const uint8_t* d_src, size_t src_page_stride,
                                       size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                       void* stream);

/*
 * cv::findContours(map, RETR_TREE, CHAIN_APPROX_SIMPLE) on an 8UC1 map in host memory, in OpenCV's output order [upstream, from
 * memory; parity unpinned].  points: x, y per point, the borders one after the other (followed as "document contour" states);
 * contours: six int32 per border - its number of points, 1 for a hole border, and the hierarchy's next, previous, first child and
 * parent (-1: none).  Parents are the topological ones: an outer border's parent is the hole border of the background region
 * (4-connected) round its component (8-connected), none in the outer background; a hole border's parent is its component's outer
 * border.  A new border enters at the HEAD of its parent's child list and the output is the pre-order walk, so siblings come last
 * discovered first (the RETR_CCOMP order of prl_hip_find_contours, nested).  n_points / n_contours always receive the totals; the
 * arrays are written only if both have room.  Host code, no device.  PRL_ERR_EMPTY, then PRL_ERR_BAD_ARG (null, step < width, a
 * side above 32768).
 */
int prl_hip_find_contours_tree(const uint8_t* map, size_t step, int width, int height, int32_t* points, int max_points, int32_t* contours,
                               int max_contours, int* n_points, int* n_contours);
/*
 * RemoveChildrenContours (imageLibCommon.cpp:483-523, 641-780) on a hierarchy in the layout above, in pre-order: approved[i] = 1 for
 * the contours it keeps.  Literally: the walk starts at contour 0 and follows `next`; a contour of fewer than 3 points is ignored;
 * one with fewer than 6 descendants is approved and its direct children are ignored (deeper ones are never visited, hence not
 * kept); otherwise it is ignored and the walk descends into its children.  Host code.  PRL_ERR_BAD_ARG for a null pointer, a link
 * outside the list or a list that is not in pre-order.
 */
int prl_hip_remove_children_contours(const int32_t* contours, int n_contours, uint8_t* approved);
/*
 * binarizeFBCITB.cpp:196-357 on one page in host memory: `map` the contour map, `gray` the processed page after COLOR_BGR2GRAY
 * (after GRAY2BGR its three channels are equal, so the AND of the reference's three channel masks is the gray decision).
 *   contours   prl_hip_find_contours_tree, then prl_hip_remove_children_contours
 *   filters    on cv::boundingRect: area > 10, area < int(max_area * width * height), rect width < int(0.8 * width), rect height <
 *              int(0.8 * height)
 *   F          the float32 sum of the gray bytes at the contour's points in point order, then (float)((double)F * (1. / N))
 *   B          element size / 2 of the sorted gray bytes at those of the twelve corner neighbours (:284-331) that lie on the page;
 *              never empty for a kept contour (the width filter leaves two columns outside the rectangle: fbcitb.h)
 *   decision   F < B: a pixel p becomes 255 iff p >= F, else iff p < F.  cv::compare of bytes with a scalar is the exact real
 *              comparison [upstream], so with cut = ceil(F) these are p >= cut and p < cut.
 * rects: six int32 per kept contour in index order - x, y, width, height, cut, below (1: white iff p < cut) - written only if
 * max_rects has room; counts: contours found, approved by RemoveChildrenContours, kept by the filters.  Host code.
 */
int prl_hip_fbcitb_contours(const uint8_t* map, size_t map_step, const uint8_t* gray, size_t gray_step, int width, int height,
                            double max_area, int32_t* rects, int max_rects, int32_t counts[3]);
/*
 * The ordered paint (:359-390): d_dst = 255, then for every rectangle IN INDEX ORDER its pixels become 255 or 0 by its decision on
 * the gray page; where rectangles overlap the one with the larger index wins.  rect_offsets (HOST, n_pages + 1 values, the first 0,
 * not decreasing); d_rects (DEVICE, six int32 each as above); a rectangle that does not lie on the page is ignored.  Not
 * serialised: an int32 owner plane per page, atomicMax of index + 1 over every rectangle (a wavefront per rectangle of at most
 * 4096 pixels, larger ones sliced over 32 workgroups), and a resolve pass.  Enqueues on `stream`.
 * PRL_ERR_EMPTY; PRL_ERR_BAD_ARG (the pages; gray and destination sharing a byte; null or malformed offsets; d_rects null with
 * rectangles to read).
 */
int prl_hip_rect_paint_batch_device(int n_pages, const int32_t* rect_offsets, const int32_t* d_rects, const uint8_t* d_gray,
                                    size_t gray_page_stride, size_t gray_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                    size_t dst_step, void* stream);

/* prl::binarizeFBCITB's arguments behind the two images, with the reference's defaults (binarizeFBCITB.h:87-103) */
typedef struct prl_fbcitb_params {
    int32_t use_canny, use_variances_map, use_clahe, use_bilateral;
    int32_t use_other_colorspace;          /* unused, as in the reference */
    int32_t use_morphology, use_canny_on_variances;
    int32_t bilateral_kernel_size;
    double variance_map_threshold, clahe_clip_limit, gaussian_blur_kernel_size;
    double canny_upper_threshold_coeff, canny_lower_threshold_coeff;
    double bounding_rectangle_max_area;
    double bilateral_kernel_intensity_sigma, bilateral_kernel_spatial_sigma;
    double bounding_rect_max_area_coeff;   /* unused, as in the reference */
} prl_fbcitb_params;
void prl_hip_default_fbcitb_params(prl_fbcitb_params* p);

/*
 * prl::binarizeFBCITB on pages of 1 or 3 channels (BGR) -> width x height masks.  A gray page stands for the three equal channels
 * the reference makes of it (every stage works per channel, and COLOR_BGR2GRAY of equal channels is the channel).
 *   flags      use_canny and use_variances_map both 0 switches both stages on while the flags "required" stay 0: the contours then
 *              come from the variance mask alone, without the AND (and CannyEdgeDetection's map, which the reference computes and
 *              drops, is not computed; its argument checks still hold).
 *   1. use_clahe: EnhanceLocalContrastByCLAHE(clip, equalize = false) per channel; use_bilateral: the bilateral filter above per
 *      channel (bilateral_kernel_size, intensity sigma, spatial sigma)
 *   2. use_canny: CannyEdgeDetection(processed page, int(gaussian_blur_kernel_size), upper, lower, 1)
 *   3. use_variances_map: the variance mask of the ORIGINAL page; use_canny_on_variances: cv::Canny(64, 128) on it; both flags
 *      required: mask &= Canny's map.  The contour map is the mask, or Canny's map when only use_canny is set.
 *   4. the gray plane of the processed page (COLOR_BGR2GRAY); ONE read-back of map and gray plane per chunk of pages
 *   5. prl_hip_fbcitb_contours per page on the host thread pool; the rectangles go up; prl_hip_rect_paint_batch_device's kernels
 *   6. use_morphology: cv::dilate 3 x 3 twice, then cv::erode twice
 * A page without contours is all 255.  counts (HOST, three int32 per page, or NULL): contours found / approved / kept.
 * Checked in this order: PRL_ERR_EMPTY; PRL_ERR_BAD_CHANNELS (not 1 or 3); PRL_ERR_BAD_ARG (null params; a parameter that is not
 * finite; a bilateral side above PRL_BILATERAL_MAX_SIDE; with the Canny stage on, CannyEdgeDetection's argument checks);
 * PRL_ERR_BAD_WINDOW (a blur side above PRL_GAUSS_MAX_SIDE); PRL_ERR_BAD_ARG (the pages).  Waits for the stream.
 */
int prl_hip_binarize_fbcitb_batch_device(const prl_fbcitb_params* params, int n_pages, int channels, const uint8_t* d_src,
                                         size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                         size_t dst_page_stride, size_t dst_step, int32_t* counts, void* stream);
int prl_hip_binarize_fbcitb_host(const prl_fbcitb_params* params, int channels, const uint8_t* src, size_t src_step, int width, int height,
                                 uint8_t* dst, size_t dst_step, int32_t* counts);

/* ---- adaptive-threshold binarizers (prl::binarizeNativeAdaptive, binarizeAT, binarizeAGT, binarizePureAdaptiveGaussian) ---- */

#define PRL_ADAPTIVE_MEAN_C 0      /* cv::ADAPTIVE_THRESH_MEAN_C */
#define PRL_ADAPTIVE_GAUSSIAN_C 1  /* cv::ADAPTIVE_THRESH_GAUSSIAN_C */
#define PRL_THRESH_BINARY 0        /* cv::THRESH_BINARY */
#define PRL_THRESH_BINARY_INV 1    /* cv::THRESH_BINARY_INV */

/*
 * cv::adaptiveThreshold(src, dst, max_value, method, type, block_size, delta) on 8-bit gray pages in device memory.
 * M = the block_size x block_size local mean around a pixel (BORDER_REPLICATE): MEAN_C the integer block sum times
 * 1.0 / block_size^2 in float64, rounded half to even; GAUSSIAN_C a separable float32 Gaussian of the float32 page in
 * OpenCV's tap order, rounded half to even.  on = p - M > -idelta with idelta = ceil(delta) for BINARY and
 * floor(delta) for BINARY_INV; BINARY writes on ? imax : 0, BINARY_INV on ? 0 : imax, imax = saturate_u8(cvRound(max_value));
 * max_value < 0 gives 0 everywhere.  auto_invert != 0 adds the last step of prl::binarizeNativeAdaptive
 * (binarizeNativeAdaptive.cpp:108-111): a page whose mask has a mean below 128 becomes 255 - mask (decided per page, applied
 * while the mask is written).  block_size: odd, 3 .. 255.  Sizes: width, height <= 32768.  Source and destination must not
 * overlap.  Enqueues on `stream`, no synchronisation.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_WINDOW (block_size
 * < 3, even or > 255); PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row bytes, size above the limit, unknown method
 * or type, NaN max_value or delta, overlapping source and destination).
 */
int prl_hip_adaptive_threshold_batch_device(int n_pages, int method, int type, double max_value, int block_size, double delta,
                                            int auto_invert, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                            int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                            void* stream);
int prl_hip_adaptive_threshold_host(int method, int type, double max_value, int block_size, double delta, int auto_invert,
                                    const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/* The reference's functions on top of it, device resident: [BGR -> gray], [cv::medianBlur], cv::adaptiveThreshold, [flip]. */
typedef struct prl_adaptive_params {
    int median_ksize;     /* cv::medianBlur's window, odd >= 3; 0 or 1: no median (binarizePureAdaptiveGaussian) */
    int median_on_color;  /* 0: gray first, then the median (binarizeNativeAdaptive.cpp:60-73); != 0: the median on the colour
                             page, then gray (binarizeAT.cpp:45-54, binarizeAGT.cpp:45-52) */
    int method;           /* PRL_ADAPTIVE_MEAN_C / PRL_ADAPTIVE_GAUSSIAN_C */
    int type;             /* PRL_THRESH_BINARY / PRL_THRESH_BINARY_INV */
    double max_value;
    int block_size;       /* odd, 3 .. 255 (the reference's "automatic" size is the caller's: (int)(sqrt(rows^2 + cols^2) / 333 + 7)) */
    int auto_invert;      /* != 0: 255 - mask where the mask's mean is below 128 */
    double delta;
} prl_adaptive_params;

/* prl::binarizeNativeAdaptive's header defaults (binarizeNativeAdaptive.h:62-74): median 5, gray first, GAUSSIAN_C,
 * BINARY_INV, 255, block 19, shift 9, auto-invert. */
void prl_hip_default_adaptive_params(prl_adaptive_params* out);

/*
 * Pages of 1, 3 or 4 interleaved channels -> width x height byte masks.  The intermediates (gray page, median result, bit
 * plane of the undecided mask) live in the device's cached scratch; the stages are ordered by `stream` alone.
 * Order of the checks: PRL_ERR_EMPTY; PRL_ERR_BAD_ARG for params == NULL; PRL_ERR_BAD_WINDOW (block_size, then median_ksize
 * negative or even); PRL_ERR_BAD_CHANNELS (not 1, 3 or 4); PRL_ERR_BAD_ARG as above (median_ksize > 65535 included).
 */
int prl_hip_binarize_adaptive_batch_device(const prl_adaptive_params* params, int n_pages, int channels, const uint8_t* d_src,
                                           size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                           size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_binarize_adaptive_host(const prl_adaptive_params* params, int channels, const uint8_t* src, size_t src_step, int width,
                                   int height, uint8_t* dst, size_t dst_step);

/* ---- local-variance binarizers ------------------------------------------------------------- */

/*
 * prl::binarizeByLocalVariances(in, out, varianceThresholdCoeff = 0.125, minResultVariance = 25, gamma = 2.0)
 * (with_filters != 0; src/binarizations/binarizeByLocalVariances.cpp:13-145) and
 * prl::binarizeByLocalVariancesWithoutFilters(in, out, varianceThresholdCoeff = 0.125, minResultVariance = 10)
 * (with_filters == 0; :148-292, gamma ignored) on 8-bit 3-CHANNEL pages (the reference reads three variance planes);
 * d_dst: width x height bytes, 0 / 255.  Enqueues on `stream`.  The filtered variant evaluates float32 log / exp / pow
 * (cv::log, cv::exp in the reference): identical results across libraries are not defined, see DESIGN.md.
 */
int prl_hip_binarize_lv_batch_device(int n_pages, int with_filters, double coeff, int min_result_variance, double gamma,
                                     const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width, int height,
                                     uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_binarize_lv_host(int with_filters, double coeff, int min_result_variance, double gamma, const uint8_t* src,
                             size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);

/* ---- deskew / rotate (prl::deskew, prl::rotate) ----------------------------------------------- */

/* Size of prl::rotate's result (src/rotate.cpp:35-72): transposed for 90 / 270 degrees, unchanged for 180, else a square
 * of side max(width, height). */
int prl_hip_rotate_out_size(int width, int height, double angle, int* out_w, int* out_h);

/* prl::rotate(input, output, angles[i]) per page; d_dst pages need room for the largest result, rows of dst_step bytes.
 * 1..4 channels.  In place is not allowed. */
int prl_hip_rotate_batch_device(int n_pages, int channels, const double* angles, const uint8_t* d_src, size_t src_page_stride,
                                size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                void* stream);

/* cv::HoughLinesP(image, lines, 1, CV_PI/180, threshold, line_length, line_gap) on one 1-channel device page, the call
 * of prl::findAngle (src/deskew/deskew.cpp:148); segments as (x0, y0, x1, y1) into the host array `lines` (4*cap ints),
 * *n_lines = number found (may exceed cap).  Synchronises. */
int prl_hip_houghp_device(const uint8_t* d_image, size_t step, int width, int height, int threshold, int line_length,
                          int line_gap, int32_t* lines, int cap, int* n_lines, void* stream);

/* Diagnostics of the HoughLinesP searches (prl::deskew, prl::findAngle, the chain's deskew stage, prl_hip_houghp_device)
 * accumulated process-wide since the last reset - the chain searches on a helper thread, so these are not per thread.
 * The point and segment lists are sized per page from the page's ink before the search: `segment_capacity` is the room the
 * segment lists had, `min_page_headroom` the smallest (capacity - segments found) of any page.  A page that needed more
 * room than it had makes its call fail with PRL_ERR_NOMEM ("HoughLinesP: segment list overflow"): nothing is clipped
 * silently, and a negative headroom is only ever seen together with that error. */
typedef struct prl_deskew_stats {
    uint64_t pages;              /* pages searched */
    uint64_t points;             /* non-zero pixels handed to HoughLinesP */
    uint64_t segments;           /* segments found */
    uint64_t segment_capacity;   /* room of the segment lists */
    uint64_t max_page_points;
    uint64_t max_page_segments;
    int64_t  min_page_headroom;  /* min over pages of capacity - segments */
    uint64_t reserved;
} prl_deskew_stats;
int prl_hip_last_deskew_stats(prl_deskew_stats* out);
int prl_hip_reset_deskew_stats(void);

/*
 * prl::findAngle (src/deskew/deskew.h:62, src/deskew/deskew.cpp:139-205) on 1-channel pages (the thresholded page prl::deskew
 * hands it, :226; any 8-bit page is accepted, its points are the pixels != 255 as after the reference's bitwise_not):
 * HoughLinesP(~page, 1, CV_PI/180, 100, width/8.f, 20), atan2 per segment, first-fit clusters of 0.01 rad, the most
 * populated cluster's first angle in degrees; 0.0 when no segment was found.  angles (host, one per page) is required,
 * n_segments (host, optional) receives the number of segments HoughLinesP found.  Synchronises.
 */
int prl_hip_find_angle_batch_device(int n_pages, const uint8_t* d_image, size_t page_stride, size_t step, int width, int height,
                                    double* angles, int32_t* n_segments, void* stream);
int prl_hip_find_angle_host(const uint8_t* src, size_t src_step, int width, int height, double* angle, int32_t* n_segments);

/*
 * prl::deskew (src/deskew/deskew.cpp:208-251) on n_pages device pages of 1, 3 or 4 channels: gray -> Otsu -> findAngle
 * (HoughLinesP + angle vote) -> prl::rotate.  Page i's result is out_wh[2i] x out_wh[2i+1] pixels (host array):
 * max(width,height)^2 when an angle was found, width x height otherwise.  d_dst pages need room for max(width,height)
 * rows of dst_step >= max(width,height) * channels bytes.  angles (host, optional) receives findAngle's degrees.
 * The orientation step (:238, Leptonica) is a no-op for the page the reference hands it; see DESIGN.md.  Synchronises.
 */
int prl_hip_deskew_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                int32_t* out_wh, double* angles, void* stream);

/* Host-image forms of the two (what the cv::Mat wrappers call): prl_hip_rotate_host's dst holds the size
 * prl_hip_rotate_out_size reports; prl_hip_deskew_host's dst has room for max(width,height)^2 pixels and *out_w x *out_h
 * tells which part was written. */
int prl_hip_rotate_host(int channels, double angle, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                        size_t dst_step);
int prl_hip_deskew_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step,
                        int* out_w, int* out_h, double* angle);

/* ---- perspective crop (prl::warpCrop, src/warp.cpp:32-102, src/warp.h:49-73) -------------------------- */

/*
 * prl::warpCrop(in, out, x0, y0, ..., x3, y3, ratio, borderMode, borderValue) takes four corners (top left, top right, bottom
 * right, bottom left) and returns the quadrilateral as a rectangle: a size rule, cv::getPerspectiveTransform and
 * cv::warpPerspective(INTER_LINEAR).  The canonical arithmetic, float64 throughout with one rounding per written operation;
 * [upstream] marks what is OpenCV's (3.4.4+ / 4.x: imgwarp.cpp, matrix_operations.cpp, the hal LU), as restated in
 * tests/warp_ref.py.  Parity with an installed OpenCV is not pinned.
 *
 * Size (warp.cpp:42-53).  side1 = sqrt((x1-x0)^2 + (y1-y0)^2), side2 over corners 2, 3, side3 over 0, 3, side4 over 1, 2: the
 * argument is the reference's `int` expression (it wraps like 32-bit two's complement; a negative one gives a NaN) converted to
 * double.  W = cvRound(max(side1, side2)), H = cvRound(max(side3, side4)); if ratio > 0, W = cvRound(H / ratio).  max(a, b) is
 * a < b ? b : a; cvRound rounds half to even, and a NaN or a value outside the int range gives INT_MIN [upstream, x86].
 *
 * Matrix [upstream]: cv::getPerspectiveTransform(src, dst) with dst = (0,0), (W,0), (W,H), (0,H).  The corners go through float
 * (the reference's srcBuff / dstBuff), then to double.  For i = 0..3, with (sx, sy) -> (dx, dy):
 *     a[i]   = {sx, sy, 1, 0, 0, 0, -sx*dx, -sy*dx}     b[i]   = dx
 *     a[i+4] = {0, 0, 0, sx, sy, 1, -sx*dy, -sy*dy}     b[i+4] = dy
 * solved by LU with partial pivoting: in column i the FIRST row of largest |a[j][i]| (strict >) is the pivot, the system is
 * singular if that pivot is < 100 * DBL_EPSILON; d = -1 / a[i][i]; for the rows j below, alpha = a[j][i] * d,
 * a[j][k] += alpha * a[i][k] (k > i), b[j] += alpha * b[i]; back substitution s = b[i], s -= a[i][k] * x[k] (k > i ascending),
 * x[i] = s / a[i][i].  M = {x0 .. x7, 1}.  (OpenCV before 3.4.4 solved the system by SVD: not this.)
 *
 * Inversion [upstream]: cv::warpPerspective without WARP_INVERSE_MAP inverts M by cv::invert's closed form for 3 x 3:
 *     det = m00*(m11*m22 - m12*m21) - m01*(m10*m22 - m12*m20) + m02*(m10*m21 - m11*m20),   d = 1 / det,
 *     t = {(m11*m22 - m12*m21)*d, (m02*m21 - m01*m22)*d, (m01*m12 - m02*m11)*d,
 *          (m12*m20 - m10*m22)*d, (m00*m22 - m02*m20)*d, (m02*m10 - m00*m12)*d,
 *          (m10*m21 - m11*m20)*d, (m01*m20 - m00*m21)*d, (m00*m11 - m01*m10)*d}.
 *
 * Per pixel (x, y) of the ow x oh result [upstream], M now the inverted matrix.  OpenCV walks the result in blocks and the
 * block width enters the arithmetic: bh = min(16, oh), bw = min(1024 / bh, ow) (integer division), xb = (x / bw) * bw,
 * x1 = x - xb.  Per row of a block, each sum left to right:
 *     X0 = M[0]*xb + M[1]*y + M[2]      Y0 = M[3]*xb + M[4]*y + M[5]      W0 = M[6]*xb + M[7]*y + M[8]
 * and per pixel
 *     W = W0 + M[6]*x1;  W = W ? 32.0 / W : 0
 *     fX = max(-2^31, min(2^31 - 1, (X0 + M[0]*x1) * W))      fY likewise      (min(a, b) is b < a ? b : a: a NaN gives 2^31 - 1)
 *     X = fX rounded half to even, Y likewise;  sx = clamp(X >> 5, -32768, 32767), sy likewise;  fx = X & 31, fy = Y & 31
 * then the four taps (sx, sy), (sx+1, sy), (sx, sy+1), (sx+1, sy+1) with the weights 32(32-fx)(32-fy), 32 fx (32-fy),
 * 32(32-fx) fy, 32 fx fy and out = (sum v*w + 2^14) >> 15 per channel.  A tap is inside iff 0 <= its x < width and
 * 0 <= its y < height, tested per tap.  PRL_BORDER_CONSTANT: an outside tap takes saturate_cast<uchar>(border_value[c]) =
 * clamp(cvRound(border_value[c]), 0, 255); PRL_BORDER_REPLICATE: the tap's coordinates are clamped to the page.  Any other border
 * mode is PRL_ERR_UNSUPPORTED.
 *
 * Limits, all PRL_ERR_BAD_ARG (the reference has none of them): page or result sides above 32767; W <= 0 or H <= 0 after the
 * rounding; a singular 8 x 8 system or det == 0; an entry of the given or of the inverted matrix that is not finite or exceeds
 * 2^500 in magnitude (no intermediate value can then become a NaN).
 */
#define PRL_BORDER_CONSTANT 0    /* cv::BORDER_CONSTANT */
#define PRL_BORDER_REPLICATE 1   /* cv::BORDER_REPLICATE */

/* The size rule alone: what a caller sizes its destination with.  Host code, no device needed.  PRL_ERR_BAD_ARG for a null
 * pointer and for a size outside 1..32767 (nothing is written then). */
int prl_hip_warp_crop_size(const int32_t quad[8], double ratio, int* out_w, int* out_h);

/* cv::getPerspectiveTransform as stated above: four (x, y) pairs each way, M = 9 doubles in row order.  Host code, no device
 * needed.  PRL_ERR_BAD_ARG for a null pointer or a singular system (M is not written then). */
int prl_hip_perspective_transform(const double src_xy[8], const double dst_xy[8], double M[9]);

/*
 * cv::warpPerspective(src, dst, M_i, Size(out_wh[2i], out_wh[2i+1]), INTER_LINEAR [| WARP_INVERSE_MAP], border_mode,
 * border_value) per page: `matrices` is a host array of 9 * n_pages doubles, inverse_map != 0 says they already map result ->
 * source, out_wh a host array (INPUT) of 2 * n_pages sizes.  1..4 channels.  d_dst pages need room for the largest result, rows of
 * dst_step bytes; bytes of a destination page outside its ow x oh are not written.  border_value: 4 doubles or NULL (zeros).
 * In place is not allowed.  Enqueues on `stream` and returns: nothing is waited for but the previous call's record copy.
 * Checked in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_CHANNELS;
 * PRL_ERR_UNSUPPORTED (border mode); PRL_ERR_BAD_ARG (null pointer, negative n_pages, d_src == d_dst, step < row bytes, then
 * the limits above per page).
 */
int prl_hip_warp_perspective_batch_device(int n_pages, int channels, const double* matrices, int inverse_map, const uint8_t* d_src,
                                          size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                          size_t dst_page_stride, size_t dst_step, const int32_t* out_wh, int border_mode,
                                          const double* border_value, void* stream);

/* prl::warpCrop per page: `quads` is a host array of 8 * n_pages ints (x0, y0, ..., x3, y3), one `ratio` for the call; sizes and
 * matrices as stated above; out_wh (host, OUTPUT, written on success) receives every page's W x H.  A caller sizes the destination
 * beforehand with prl_hip_warp_crop_size.  Otherwise as prl_hip_warp_perspective_batch_device. */
int prl_hip_warp_crop_batch_device(int n_pages, int channels, const int32_t* quads, double ratio, const uint8_t* d_src,
                                   size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                   size_t dst_page_stride, size_t dst_step, int32_t* out_wh, int border_mode,
                                   const double* border_value, void* stream);

/* One host image (what the cv::Mat wrapper calls); dst holds the size prl_hip_warp_crop_size reports.  Synchronises. */
int prl_hip_warp_crop_host(int channels, const int32_t quad[8], double ratio, const uint8_t* src, size_t src_step, int width,
                           int height, uint8_t* dst, size_t dst_step, int border_mode, const double* border_value);

/* ---- pyramid, edge map, resize (cv::pyrDown, cv::Canny, the edge map of prl::documentContour, prl::resize) ------------------ */

/*
 * The two OpenCV primitives the border detector and prl::resize start from (src/resize.cpp:29-62,
 * src/border_detection/autoCrop.cpp:67-101), for 8-bit pages in device memory.  Integer arithmetic throughout, so every byte is
 * held; [upstream] marks what is OpenCV's, as restated in tests/edges_ref.py.  Parity with an installed OpenCV is not pinned
 * (DESIGN.md §2).  Pages and rows may be strided; a destination has another size than its source and never shares a byte with it.
 *
 * cv::pyrDown [upstream], BORDER_REFLECT_101, 1..4 channels, result (W+1)/2 x (H+1)/2.  Per channel
 *     r(x, j) = s(2x-2, j) + 4 s(2x-1, j) + 6 s(2x, j) + 4 s(2x+1, j) + s(2x+2, j)          columns through R(., W)
 *     v       = r(x, 2y-2) + 4 r(x, 2y-1) + 6 r(x, 2y) + 4 r(x, 2y+1) + r(x, 2y+2)          rows through R(., H)
 *     dst     = (v + 128) >> 8
 * R(p, len) is cv::borderInterpolate: p if 0 <= p < len; 0 if len == 1; else p = -p (p < 0) or 2 len - 2 - p, repeated until
 * inside (a side of 2 or 3 folds more than once).  `levels` in 1..16 applies the step that many times in one call; the levels
 * between live in the cached workspace, ordered by the stream alone.
 *
 * cv::Canny(src, dst, threshold1, threshold2) [upstream] with apertureSize 3 and L2gradient false, 8UC1 only: a colour page is
 * PRL_ERR_BAD_CHANNELS (OpenCV takes the channel of largest magnitude per pixel, which is not provided).  threshold1 > threshold2:
 * swapped.  low = floor(threshold1), high = floor(threshold2), each clamped to [-1, 2041] (every magnitude lies in 0..2040, so no
 * comparison changes); a NaN is PRL_ERR_BAD_ARG.  With coordinates clamped to the page (BORDER_REPLICATE):
 *     dx = [p(x+1,y-1) + 2 p(x+1,y) + p(x+1,y+1)] - [p(x-1,y-1) + 2 p(x-1,y) + p(x-1,y+1)]
 *     dy = [p(x-1,y+1) + 2 p(x,y+1) + p(x+1,y+1)] - [p(x-1,y-1) + 2 p(x,y-1) + p(x+1,y-1)]
 *     m  = |dx| + |dy|, and m = 0 outside the page
 * ax = |dx|, ay = |dy| * 2^15, t = ax * 13573.  A pixel is a local maximum iff m > low and
 *     ay < t:               m > m(x-1,y) and m >= m(x+1,y)
 *     ay > t + ax * 2^16:   m > m(x,y-1) and m >= m(x,y+1)
 *     else:                 m > m(x-s,y-1) and m > m(x+s,y+1),  s = -1 if (dx ^ dy) < 0, else +1
 * Class 2: a local maximum with m > high; class 0: any other local maximum; class 1: the rest (OpenCV's map codes).  The result is
 * 255 for class 2 and for every class-0 pixel that reaches a class-2 pixel through 8-connected class-0 pixels, 0 elsewhere: a
 * closure that does not depend on the visiting order, so the parallel fixpoint equals OpenCV's stack walk.  The passes repeat
 * until no page changes, without a cap; the calls that link wait for the stream (they read the per-page flags back).
 *
 * The edge map of prl::documentContour (autoCrop.cpp:67-101), pages of 1, 3 or 4 channels: pyrDown while longSide / 2 >= 256
 * (longSide from the reduced size each time; 511 gives no level), the channel with the first maximum of cv::meanStdDev's
 * standard deviations, cv::Canny(25, 50) on it.  The deviations come from the last level's per-channel histograms, on the host in
 * float64: mean = sum(h v) / N, stddev = sqrt(max(sum(h v^2) / N - mean^2, 0)), both sums exact integers: ONE small read-back
 * (the bins) per chunk of pages, before the edge map.  Gray pages skip it.  The quad search on this map and the retry of
 * autoCrop.cpp:118-125 are the next section ("document contour").
 *
 * prl::resize (resize.cpp:29-62).  Pyramid path (scaleX or scaleY not positive): pyrDown while the long side exceeds maxSize;
 * maxSize < 1 never ends in the reference and is PRL_ERR_BAD_ARG here.  Scale path: cv::resize(INTER_AREA) to cols * scaleX x
 * rows * scaleY with integer factors >= 1 is an enlargement, which OpenCV [upstream] runs through its bilinear routine with the
 * coefficient fx = (dx + 1) - (sx + 1) * scaleX, sx = floor(dx * (1.0 / scaleX)) in float64: fx is an integer, its fraction 0, so
 * dst(dy, dx) = src(min(sy(dy), rows - 1), min(sx(dx), cols - 1)).  The tables come from the product, not from dx / scaleX: at
 * scaleX = 49 the product 49 * (1.0 / 49) lies below 1 and column 49 copies source column 0.  A result side above 32768 is
 * PRL_ERR_BAD_ARG.
 *
 * Every entry checks in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_CHANNELS;
 * PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row bytes, levels / factors / thresholds / maxSize as above, sides above
 * 32768, source and destination sharing a byte).  The *_host entries take one page in host memory and synchronise.
 */

/* the size after `levels` pyramid levels; host code, no device needed */
int prl_hip_pyr_down_size(int width, int height, int levels, int* out_w, int* out_h);
/* d_dst pages hold the last level: prl_hip_pyr_down_size.  Enqueues only. */
int prl_hip_pyr_down_batch_device(int n_pages, int channels, int levels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                  int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_pyr_down_host(int channels, int levels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                          size_t dst_step);

/* stage 1 alone: the class of every pixel (0, 1, 2) as bytes.  Enqueues only. */
int prl_hip_canny_classes_batch_device(int n_pages, int channels, double threshold1, double threshold2, const uint8_t* d_src,
                                       size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                       size_t dst_page_stride, size_t dst_step, void* stream);
/* stage 2 alone on a byte class map (2 = edge, 0 = candidate, anything else = no edge) -> 0 / 255.  out_passes (host, n_pages
 * entries, or NULL) receives the number of linking passes each page took part in; the last of them changed nothing.  Waits for
 * the stream. */
int prl_hip_edge_link_batch_device(int n_pages, const uint8_t* d_classes, size_t src_page_stride, size_t src_step, int width, int height,
                                   uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, int32_t* out_passes, void* stream);
/* cv::Canny: stage 1 writes two bit planes (strong, candidate), stage 2 links on them, the strong plane leaves as 0 / 255 bytes;
 * no byte class map is written.  Waits for the stream. */
int prl_hip_canny_batch_device(int n_pages, int channels, double threshold1, double threshold2, const uint8_t* d_src, size_t src_page_stride,
                               size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_canny_host(int channels, double threshold1, double threshold2, const uint8_t* src, size_t src_step, int width, int height,
                       uint8_t* dst, size_t dst_step);

/* the pyramid levels prl::documentContour takes and the size of its edge map; host code, no device needed */
int prl_hip_document_edges_geometry(int width, int height, int* levels, int* out_w, int* out_h);
/* d_dst: one 8UC1 map per page of the size prl_hip_document_edges_geometry reports; out_channel (host, n_pages entries): the
 * channel each page's map was made from.  Reads the bins back once per chunk of pages and waits for the stream. */
int prl_hip_document_edges_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                        int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, int32_t* out_channel,
                                        void* stream);
int prl_hip_document_edges_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step,
                                int32_t* out_channel);

/* prl::resize, pyramid path: how many levels the reference takes and the size it ends with; host code, no device needed */
int prl_hip_resize_pyramid_levels(int width, int height, int max_size, int* levels, int* out_w, int* out_h);
/* prl::resize, scale path: dst is width * scale_x x height * scale_y; factors (1, 1) are a copy.  Enqueues only: nothing is waited
 * for but the previous call's table copy. */
int prl_hip_resize_replicate_batch_device(int n_pages, int channels, int scale_x, int scale_y, const uint8_t* d_src, size_t src_page_stride,
                                          size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                          void* stream);
int prl_hip_resize_replicate_host(int channels, int scale_x, int scale_y, const uint8_t* src, size_t src_step, int width, int height,
                                  uint8_t* dst, size_t dst_step);

/* ---- document contour (prl::documentContour, prl::autoCrop: autoCrop.cpp:43-175, autoCropUtils.cpp:40-55, 141-348) ---------- */

/*
 * prl::documentContour finds the page in a photograph as four corners: the edge map above, findDocumentContour on it, one retry
 * after a closing, scaleContour and cropVerticesOrdering.  The pixel work runs on the device; the search runs on the host, per
 * page, on a map of at most 511 x 511 pixels, in the arithmetic below ([upstream]: OpenCV's contours.cpp, approx.cpp, shapedescr.cpp,
 * convhull.cpp of 3.4 / 4.x before the 4.10 rewrite of findContours), as restated in tests/contour_ref.py.  Parity with an
 * installed OpenCV is not pinned.
 *
 * cv::findContours(map, RETR_CCOMP, CHAIN_APPROX_SIMPLE) [upstream: Suzuki-Abe].  Non-zero is foreground (value 1).  The page is
 * surrounded by one pixel of background and keeps its own border pixels.  The page's pixels are scanned in raster order, `prev`
 * being the value to the left (0 at a row's start) and `p` the pixel's own:
 *     an outer border starts at a pixel with p == 1 (foreground, unmarked) and prev == 0;
 *     a hole border starts at the pixel to the LEFT of a page pixel with p == 0 whose own value is 1 or 2, that is foreground and
 *     not marked as a right-hand end (so the scan never starts a hole border from the last column's right side);
 *     after a border the scan goes on from the same pixel with the value it has now.
 * Directions: 0 = (+1, 0), 1 = (+1, -1), 2 = (0, -1), 3 = (-1, -1), 4 = (-1, 0), 5 = (-1, +1), 6 = (0, +1), 7 = (+1, +1).  From the
 * start pixel i0 the first neighbour i1 is searched clockwise, s = 3, 2, 1, 0, 7, 6, 5 for an outer border (from 4) and
 * s = 7, 6, ..., 1 for a hole border (from 0); none: an isolated pixel, marked as a right-hand end, one point.  Else, with i3 = i0 and
 * the arrival direction s: the next neighbour i4 is the first non-zero one counter-clockwise from s + 1 (s + 1, s + 2, ... mod 8);
 * with s' its direction, i3 is marked as a right-hand end (-126) if (unsigned)(s' - 1) < (unsigned)s, else 2 if it still was 1;
 * the point i3 is emitted iff s' differs from the direction of the step before (initially the first s with bit 2 flipped, s ^ 4);
 * the walk ends when i4 == i0 and i3 == i1, else i3 = i4, s = (s' + 4) mod 8.  Points are page coordinates.
 * Order of the result: outer borders from the last discovered to the first, each followed by the hole borders of its 8-connected
 * component, last discovered first (OpenCV hangs a hole on the outer border that surrounds it, which is that one).  Both kinds are
 * candidates; the order decides ties only.
 *
 * cv::approxPolyDP(points, eps, closed = true) on integer points [upstream], eps2 = eps * eps, all distances in float64:
 *     1. three rounds: from the current start (first: point 0) the point of largest squared distance, the first of equals; the next
 *        round starts there.  If the last round's largest squared distance is <= eps2 the result is that round's start alone.
 *     2. else the slices (start, far) and (far, start) of the last round go on a stack, the first on top.
 *     3. a slice (a, b) is popped; with chord d = P[b] - P[a], the point between them of largest |(y - ya) dx - (x - xa) dy|, first
 *        of equals; if there is none, or that value squared is <= eps2 * (dx^2 + dy^2), P[a] is written, else (far, b) and then
 *        (a, far) are pushed.
 *     4. clean-up over the written points, cyclically from the last one (start S), P the next, E the one after: with d = E - S,
 *        P is dropped iff |(Px - Sx) dy - (Py - Sy) dx|^2 <= 0.5 eps2 (dx^2 + dy^2) and dx != 0 and dy != 0 and
 *        (P - S).(E - P) >= 0; then S = E and the walk skips one; else S = P.  It stops at two points.
 * The reference feeds each result back in with eps = 1, 2, 3, ... until at most 4 points remain (autoCropUtils.cpp:186-191).
 *
 * A polygon of exactly four points p0..p3 is a candidate iff (autoCropUtils.cpp:193-235), in float64:
 *     area = |sum(x[i-1] y[i] - x[i] y[i-1])| / 2, i from 0 with i - 1 = 3 first             (cv::contourArea)
 *     side1..4 = |p0 p1|, |p1 p2|, |p2 p3|, |p3 p0|, sqrt of the float64 sum of squares       (cv::norm)
 *     min(side1, side3) / max(side1, side3) >= 0.85 and likewise for sides 2, 4 (stated as "not < 0.85": a NaN passes)
 *     angle(p0, p1, p2, p3) >= 160 and angle(p1, p2, p3, p0) >= 160, where angle(a, b, c, d) =
 *         r = (atan2(cy - dy, cx - dx) - atan2(ay - by, ax - bx)) * 180.0 / 3.14;  r < 0: r += 360;  r > 180: r = 360 - r
 *     area <= cols * rows (an int product) and area >= minArea, minArea = 0.05 * cols * rows at first
 * and it replaces the kept one iff area > minArea (strictly), which then becomes minArea.  The kept polygon is the answer iff
 * cv::convexHull of its points has four vertices, that is iff the four are in strictly convex position: decided in exact integers.
 * The corners leave in the polygon's own order.
 *
 * scaleContour, cropVerticesOrdering (autoCropUtils.cpp:269-348): xScale = (float)src_w / (float)map_w, likewise y, where
 * map_w x map_h is cols / 2^levels x rows / 2^levels (autoCrop.cpp:83, integer division: 1027 gives 513 at one level while the
 * pyramid's map is 514 wide); x *= xScale, y *= yScale in float.  The hull's cycle is taken with
 * sum(x[i] y[i+1] - x[i+1] y[i]) > 0 (top left -> top right -> bottom right -> bottom left on the screen), starting at the corner of
 * smallest x, then smallest y: both decided on the integer corners, which a positive scale does not reorder.  The cycle is then
 * rotated to the first corner of strictly smallest x * x + y * y, each product and the sum rounded to float, as written.
 *
 * The retry (autoCrop.cpp:105-128): a page without a quad gets cv::dilate, then cv::erode, of its map with the 2 x 2 rectangle,
 * default anchor, iterations = 2, which is prl_hip_morphology_ex's CLOSE; then the search again.  `try` is 0 for a page found at
 * once and 1 for every other page, found or not.  The reference closes the map once more after the second search (iterations = 3)
 * and then returns without looking at it: that closing changes nothing observable and is not run.
 * Positive scaleX, scaleY take cv::resize(INTER_AREA) in general position: not in the C ABI; the C++ layer throws
 * cv::Exception(StsNotImplemented).
 */

/* cv::findContours as above, host code, no device needed.  points: x, y per point, the borders one after the other; contours: per
 * border its number of points and 1 for a hole border.  n_points / n_contours always receive the totals; the arrays are written
 * only if both have room (max_points points, max_contours borders).  PRL_ERR_EMPTY, then PRL_ERR_BAD_ARG (null, step < width). */
int prl_hip_find_contours(const uint8_t* map, size_t step, int width, int height, int32_t* points, int max_points, int32_t* contours,
                          int max_contours, int* n_points, int* n_contours);
/* cv::approxPolyDP(closed) as above; out_points has room for n_points points.  Host code. */
int prl_hip_approx_poly_closed(const int32_t* points, int n_points, double epsilon, int32_t* out_points, int* n_out);
/* findDocumentContour on an 8UC1 map: *found = 1 and the four corners in the polygon's own order, or *found = 0 and zeros.  Host
 * code, no device needed.  PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_ARG (null, step < width, a side above 32768). */
int prl_hip_document_quad(const uint8_t* map, size_t step, int width, int height, int32_t quad[8], int* found);
/* scaleContour, then cropVerticesOrdering.  Host code.  PRL_ERR_BAD_ARG for corners that are not in strictly convex position (the
 * reference reads past its hull there); nothing is written then. */
int prl_hip_document_quad_finish(const int32_t quad[8], int map_width, int map_height, int src_width, int src_height, float out[8]);

/* prl::documentContour(page, -1, -1, contour) per page of 1, 3 or 4 channels in device memory.  quads (host, 8 floats per page: the
 * ordered corners, zeros without a quad), found (host, 0 / 1 per page), out_try (host or NULL) as above.  Per chunk of pages: the
 * edge maps, ONE copy of them to pinned host memory, the search per page on the library's host thread pool (the pool of the
 * host-list entries: PRL_HIP_HOST_COPY_THREADS), the closing on the pages without a quad alone, as a table of pages, their copy
 * and second search.  Waits for the stream.  Checked as the edge entries are: PRL_ERR_EMPTY; PRL_ERR_BAD_CHANNELS;
 * PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row bytes, a side above 32768). */
int prl_hip_document_contour_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                          int height, float* quads, int32_t* found, int32_t* out_try, void* stream);
int prl_hip_document_contour_host(int channels, const uint8_t* src, size_t src_step, int width, int height, float quad[8], int32_t* found,
                                  int32_t* out_try);

/* ---- Hough lines (cv::HoughLines; prl::findHoughLineContour: houghLine.cpp:16-256, imageLibCommon.cpp:821-833, 929-941,
 *      autoCropUtils.cpp:350-366) ------------------------------------------------------------------------------------------------- */

/*
 * prl::findHoughLineContour is the reference's second border detector: where a page's outline is broken, contour following fails
 * and voting lines succeed.  Edge map, votes and peaks run on the device; the line filter and the quad search run on the host, per
 * page, on at most a few hundred lines.  The arithmetic below is restated in tests/houghline_ref.py; what is marked [upstream] is
 * OpenCV's (hough.cpp HoughLinesStandard, canny.cpp, shapedescr.cpp, convhull.cpp of 3.4 / 4.x).  Parity with an installed OpenCV is
 * not pinned.
 *
 * cv::HoughLines(map, lines, rho = 1, theta = (float)(CV_PI / 180), threshold), the standard transform [upstream], on an 8UC1 map of
 * W x H pixels:
 *     numangle = cvRound(CV_PI / theta) = 180: the rule of 3.4 and of 4.x up to the release that changed it.  Later 4.x releases
 *         take cvFloor(CV_PI / theta) + 1 = 181 rows (an extra angle just below pi); that rule is NOT the one taken here.
 *     numrho = cvRound(((W + H) * 2 + 1) / rho) = 2 (W + H) + 1.
 *     the table, on the host with libm: float ang = 0; for n = 0..179: tabSin[n] = (float)(sin((double)ang) * 1.f), tabCos[n] likewise,
 *         ang += theta in float32.  The device never evaluates sin or cos.
 *     every non-zero pixel (x = column, y = row) votes once per n: r = cvRound(x * tabCos[n] + y * tabSin[n]) + (numrho - 1) / 2,
 *         two float32 products and one float32 sum, each rounded on its own (no contraction), the sum rounded to the nearest integer,
 *         ties to even; cell (n + 1, r + 1) of an accumulator of (numangle + 2) x (numrho + 2) int32 is incremented.  The accumulator
 *         is an integer histogram: the order of the votes does not matter.
 *         Denormals cannot matter: the table's only zero is tabSin[0]; its smallest other magnitude is |tabCos[90]| = 1.1165949e-06
 *         (the float32 angle after 90 additions misses pi / 2 by that much), so every non-zero product, x and y being integers >= 1,
 *         is at least 1.1e-06, far above the smallest normal float32 (1.2e-38), and the sum of two such products is zero or at
 *         least one unit in the last place of the smaller one, 1.3e-13: normal as well.
 *     cell (n, r), 0 <= n < 180, 0 <= r < numrho, with count a, is a peak iff a > threshold and a > left and a >= right and a > up
 *         and a >= down: left / right are r -+ 1, up / down are n -+ 1; the frame cells (row 0, row 181, column 0, column numrho + 1)
 *         are zero.
 *     the peaks are ordered by count, descending, then by cell index (n + 1) * (numrho + 2) + r + 1, ascending.
 *     a peak leaves as rho = (r - (numrho - 1) * 0.5f) * 1.f, theta = n * theta, both float32.
 * Other rho / theta steps and the multi-scale variant are not offered.
 *
 * The edge map of prl::findHoughLineContour (houghLine.cpp:198-218) on a page of 1, 3 or 4 channels: cv::medianBlur(3) three times,
 * cv::medianBlur(5) three times (prl_hip_median_batch_device's arithmetic, per channel), then cv::Canny(25, 50), apertureSize 3, L1
 * magnitude, as stated under "pyramid, edge map, resize", with one rule more for colour pages [upstream]: per pixel, dx, dy and the
 * magnitude |dx| + |dy| are those of the channel whose magnitude is largest, the first of equals (a fourth channel takes part as
 * any other).  Non-maximum suppression, the thresholds and the linking then see one gradient per pixel.  Only these entries reach
 * the colour rule: prl_hip_canny_* keep refusing colour pages.  The reference's three cv::imwrite("after_*.jpg") calls are debugging
 * leftovers: no file is written here.
 *
 * The line filter and the quad search (houghLine.cpp:16-175, 231-255) on the lines in cv::HoughLines' order:
 *     fewer than four lines: no quad (before the filter).
 *     fromVec2f(rho, theta): a = cosf(theta), b = sinf(theta) (std::cos / std::sin of a float are the float overloads) widened to
 *         float64; x0 = a * rho, y0 = b * rho; the line's two ends are (cvRound(x0 - 1000 b), cvRound(y0 + 1000 a)) and
 *         (cvRound(x0 + 1000 b), cvRound(y0 - 1000 a)), stored as float32: integers.
 *     distanceToLine(start, end, p) takes the ends as integer points: |(px - sx)(ey - sy) - (py - sy)(ex - sx)| as an int, widened,
 *         over hypot(ex - sx, ey - sy).
 *     deleteSimilarLines(lines, minDist = 5, step = 5, maxLines = 20): while more than 20 lines remain, one round: in order, every
 *         line not yet dropped is kept and drops every later line j whose distance is < minDist, the distance of two lines being the
 *         smallest of the four end-to-line distances.  A round that keeps fewer than four lines ends the filter: the round's INPUT is
 *         cut to its first 20 lines and kept.  Else the kept lines are the next round's input and minDist grows by 5.
 *     intersection(o1, p1, o2, p2) (autoCropUtils.cpp:350-366) in float32: x = o2 - o1, d1 = p1 - o1, d2 = p2 - o2,
 *         cross = d1.x * d2.y - d1.y * d2.x; |cross| <= 1e-7 (as float64): none.  t1 = (x.x * d2.y - x.y * d2.x) / cross, a float32
 *         quotient widened to float64; the point is o1 + (float)(d1 * t1), the product in float64, the sum in float32.
 *     findMaxValidContour: for every ordered choice (i, j, k, m) of four different lines, the corners are intersection(j, i),
 *         intersection(k, j), intersection(m, k), intersection(i, m), the first line's ends given first; a choice with a missing
 *         intersection is skipped, as is one with a corner outside 0 <= x <= width, 0 <= y <= height (the reference's flag for
 *         "outside" is named validCoord, and the comparison is strict: a corner ON x == width is kept).  The choice replaces the kept
 *         one iff cv::isContourConvex [upstream: every turn dy * dx0 > dx * dy0 of one strict sign, in float32, a zero turn fails] and
 *         IsQuadrangularConvex (cv::convexHull of the four points has four vertices) hold and cv::contourArea [upstream: float64 sum
 *         of prev.x * y - prev.y * x, halved, absolute] is > the kept area, which starts at 0: of equal areas the first choice wins.
 *         The hull test is decided here as "each corner lies strictly outside the triangle of the other three", on float64 cross
 *         products of the float32 corners; after isContourConvex has passed it can differ from OpenCV's float32 scan only where a
 *         turn's sign depends on the last bit of a float32 product.
 *     the four corners leave truncated towards zero, static_cast<int>, in the choice's order; the C++ layer APPENDS them to the
 *         caller's vector as the reference does.
 * splitPage (a stub in the reference), a chain stage and host-list entries are not offered.
 *
 * Every entry checks in this order, before any device is touched: PRL_ERR_EMPTY (width or height <= 0); PRL_ERR_BAD_CHANNELS (the
 * edge and contour entries: not 1, 3 or 4); PRL_ERR_BAD_ARG (null pointer, negative n_pages, step < row bytes, a side above 32768,
 * threshold < 0, max_lines < 0, an accumulator page stride below the accumulator's bytes or not a multiple of 4, source and
 * destination of the edge map sharing a byte).
 */

/* numangle (180) and numrho of a width x height map; host code, no device needed */
int prl_hip_hough_lines_geometry(int width, int height, int* numangle, int* numrho);
/* The voting stage alone: page i's framed accumulator, (numangle + 2) x (numrho + 2) int32 in row-major order, at
 * d_accum + i * accum_page_stride bytes (device memory, every cell written).  Enqueues only. */
int prl_hip_hough_accumulator_batch_device(int n_pages, const uint8_t* d_map, size_t page_stride, size_t step, int width, int height,
                                           int32_t* d_accum, size_t accum_page_stride, void* stream);
/* cv::HoughLines per page of a batch of 8UC1 device maps.  lines (host): page i's lines as (rho, theta) pairs from
 * lines + 2 * max_lines * i, in OpenCV's order; n_lines (host, n_pages entries) always receives the number found, which may exceed
 * max_lines: then the first max_lines of the order were written and the caller sees that it has to call again with room (nothing
 * is clipped silently; max_lines = 0 with lines = NULL asks for the counts alone).  Per chunk of pages the counts and the peak
 * lists come down once and are sorted on the host.  Waits for the stream. */
int prl_hip_hough_lines_batch_device(int n_pages, const uint8_t* d_map, size_t page_stride, size_t step, int width, int height, int threshold,
                                     float* lines, int max_lines, int32_t* n_lines, void* stream);
int prl_hip_hough_lines_host(const uint8_t* map, size_t step, int width, int height, int threshold, float* lines, int max_lines,
                             int32_t* n_lines);
/* the edge map above as 0 / 255 bytes, one 8UC1 map of the page's size per page.  Waits for the stream. */
int prl_hip_hough_edges_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                     int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream);
int prl_hip_hough_edges_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step);
/* The line filter and the quad search on n_lines (rho, theta) pairs in cv::HoughLines' order, for a map of width x height: *found = 1
 * and the four corners (x, y) in quad, or *found = 0 and zeros.  Host code, no device needed. */
int prl_hip_hough_line_quad(const float* lines, int n_lines, int width, int height, int32_t quad[8], int* found);
/* prl::findHoughLineContour per page of 1, 3 or 4 channels in device memory: found (host, 0 / 1 per page), quads (host, 8 ints per
 * page: the four corners, zeros without a quad), out_lines (host or NULL): the lines cv::HoughLines(threshold 50) found on the page.
 * Per chunk of pages: the edge maps, the votes and the peaks on the device, ONE read-back of the line lists, the filter and the search
 * per page on the library's host thread pool.  Waits for the stream. */
int prl_hip_hough_line_contour_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                            int width, int height, int32_t* quads, int32_t* found, int32_t* out_lines, void* stream);
int prl_hip_hough_line_contour_host(int channels, const uint8_t* src, size_t src_step, int width, int height, int32_t quad[8], int32_t* found,
                                    int32_t* out_lines);

#ifdef __cplusplus
}
#endif
#endif /* PRL_HIP_H_ */
