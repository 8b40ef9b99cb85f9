/* gfdm_hip.h -- C-ABI of the MI355X (gfx950) GFDM modulator / receiver / IC-receiver kernels.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Each entry point names the gr-gfdm interface it replaces (paths relative to
 * the gr-gfdm checkout).  The GR-free C++ classes of gr-gfdm_amd/cpp/ and the
 * pybind11 module `gfdm_python` are thin wrappers over these functions; see
 * INTEGRATION.md for the reference-side binding.
 *
 * Conventions
 *   - samples are interleaved float32 (re, im) == std::complex<float> == gr_complex
 *     (include/gfdm/gfdm_kernel_utils.h:40).  One GFDM block = timeslots*subcarriers
 *     samples; batched calls take `nblocks` blocks back to back (block stride = block_size),
 *     exactly the stream layout the GNU Radio wrappers feed one block at a time
 *     (lib/simple_receiver_cc_impl.cc:70-74, lib/advanced_receiver_sb_cc_impl.cc:98-113).
 *   - `*_host` calls take host pointers and return when the result is in `out` (the reference's
 *     synchronous generic_work contract); see "the host-buffer batch path" below for how the bytes move.
 *   - `*_device` calls take device pointers on the handle's device and only ENQUEUE work on
 *     `stream` (a hipStream_t passed as void*, NULL = default stream).  No synchronisation,
 *     no allocation: they are hipGraph-capturable.  Buffers must not alias.
 *   - every function returns GFDM_HIP_OK (0) or a negative gfdm_hip_status; the text of the
 *     last failure on the calling thread is available from gfdm_hip_last_error().
 *   - a handle is not thread-safe (neither are the reference kernels, which own scratch
 *     buffers: include/gfdm/receiver_kernel_cc.h:103-118); use one handle per thread/stream.
 *   - there is NO CPU fallback: without a usable gfx950 device creation fails with
 *     GFDM_HIP_ENODEV.
 */
#ifndef GFDM_HIP_H
#define GFDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gfdm_hip_status {
    GFDM_HIP_OK = 0,
    GFDM_HIP_EINVAL_TAPS = -1,     /* std::invalid_argument: taps.size() != timeslots*overlap
                                      (lib/modulator_kernel_cc.cc:39-46, lib/receiver_kernel_cc.cc:40-47) */
    GFDM_HIP_EINVAL_OVERLAP = -2,  /* std::invalid_argument: receiver overlap < 2 (lib/receiver_kernel_cc.cc:48-52) */
    GFDM_HIP_EINVAL = -3,          /* any other bad argument (NULL pointer, negative size, bad subcarrier index ...) */
    GFDM_HIP_ENODEV = -4,          /* no usable HIP device */
    GFDM_HIP_EHIP = -5,            /* a HIP runtime call failed */
    GFDM_HIP_ENOMEM = -6,
    GFDM_HIP_EUNSUPPORTED = -7     /* beyond the device: timeslots * subcarriers > 2^24, or 2 * timeslots + subcarriers above ~20 000 */
} gfdm_hip_status;

/* how hard decisions are taken in the IC loop (gr::digital::constellation::decision_maker,
 * called at lib/advanced_receiver_kernel_cc.cc:119) */
typedef enum gfdm_hip_decision {
    GFDM_HIP_DECIDE_AUTO = -1,     /* QPSK/BPSK sign tests when the points match those constellations, else NEAREST */
    GFDM_HIP_DECIDE_NEAREST = 0,   /* minimum Euclidean distance, first minimum wins */
    GFDM_HIP_DECIDE_QPSK = 1,      /* index = 2*(im > 0) + (re > 0)   (constellation_qpsk) */
    GFDM_HIP_DECIDE_BPSK = 2       /* index = (re > 0)                (constellation_bpsk) */
    /* QPSK / BPSK name the sign tests of GNU Radio's unit constellations, points (+-1 +-j)/sqrt 2 in the order --, +-, -+, ++ and -1, +1.
     * Given with other points (scaled, rotated) a handle decides by NEAREST over the points as given -- for a scaled QPSK / BPSK the same
     * regions and the same tie rule (zero -> the first, all-negative point). */
} gfdm_hip_decision;

typedef struct gfdm_hip_modulator gfdm_hip_modulator;
typedef struct gfdm_hip_receiver gfdm_hip_receiver;
typedef struct gfdm_hip_advanced_receiver gfdm_hip_advanced_receiver;

const char* gfdm_hip_strerror(int status);
const char* gfdm_hip_last_error(void);
int gfdm_hip_device_count(void);
/* TEST HOOK, not part of the drop-in surface: handles created while `enable` is non-zero use the generic kernel family even
 * for shapes the tuned row-lane family serves, so that the tests can run both families on the same shape.  Returns the previous
 * setting.  Nothing else (no environment variable) changes the kernel family of a handle. */
int gfdm_hip_force_generic_family_for_testing(int enable);
/* Run-time instantiation of the tuned (row-lane) kernels for shapes outside the library's compiled list: a handle for a shape with
 * a power-of-two number of subcarriers (4 .. 1024) or one up to 1024 that is a product of two or three factors <= 32 (12, 20, 34, 48, 96, 100, 240, 384, 600, 1000 ...),
 * 3 .. 48 timeslots and overlap 2 .. 8 -- as far as the block fits the CU's 160 KB LDS (every shape up to 512 subcarriers does; 1024 x 17) -- gets the kernels compiled for exactly that
 * shape through hiprtc (1-70 s per part, growing with the number of timeslots; a handle compiles only the parts of its kind -- a modulator
 * the modulator kernels, a receiver the receive kernels, ... -- the rest at first use; the code objects are cached under
 * $GFDM_HIP_CACHE_DIR, else $XDG_CACHE_HOME/gfdm_hip, else ~/.cache/gfdm_hip -- a directory of this user that nobody else can write, or no
 * cache at all -- so this happens once per shape and machine) and reports kernel_name "rowlane_jit".
 * gfdm_hip_set_jit(mode) says WHEN the compile happens for handles created afterwards (returns the previous mode):
 *   0  never: such shapes use the generic kernel family (no compile step, several times slower kernels);
 *   1  inside the constructor, which then takes as long as the compile;
 *   2  on a background thread: the constructor returns at once, the handle runs on the generic family (same results, kernel_name
 *      "generic_lds") and switches to the tuned kernels -- kernel_name "rowlane_jit" -- at the first call after the build has finished;
 *   3  (default) like 1 when the code objects are already in the disk cache or the shape compiles within seconds (timeslots <= 16),
 *      like 2 otherwise: no constructor blocks for longer than a few seconds.
 * If hiprtc is unavailable the generic family is used.  gfdm_hip_precompile fills the disk cache ahead of time. */
int gfdm_hip_set_jit(int mode);
/* Deployment step: compile the tuned kernels of a shape into the disk cache WITHOUT creating a handle (no GPU needed), so that the first
 * flowgraph using the shape starts with them.  parts: bit 0 receive, 1 receive + IC, 2 preamble-equalised receive, 3 modulate,
 * 4 estimator, 5 preamble-equalised receive straight from a capture (demodulate_bursts) (0 = all).  Returns GFDM_HIP_OK also for shapes that are compiled into the library; GFDM_HIP_EUNSUPPORTED for shapes only
 * the generic family serves.  Command line: python -m gfdm_amd.precompile <timeslots> <subcarriers> <overlap> [...]. */
int gfdm_hip_precompile(int timeslots, int subcarriers, int overlap, unsigned parts);
/* Stops the background builds of gfdm_hip_set_jit modes 2 / 3: what is still queued is dropped (those handles stay on the generic kernels), the
 * builds in flight finish their compile (the code object still reaches the disk cache) without touching the GPU, and the call returns when the
 * two pool threads are idle -- at most one compile (10-70 s) later.  The library does this by itself when it is unloaded; an application that
 * tears the HIP runtime down before that (an interpreter at exit: the Python package registers it with atexit) calls it first.  Later requests
 * start the pool again. */
void gfdm_hip_quiesce(void);
/* The interference-cancellation rounds of the advanced receiver (lib/advanced_receiver_kernel_cc.cc:56-76, lib/receiver_kernel_cc.cc:274-299)
 * can run on the matrix cores (v_mfma_f32_16x16x32_f16; the QPSK decisions are exact in f16, the IC taps enter as a three-term f16 split with
 * 33 significant bits, sums in f32) where that form applies: QPSK sign decisions, a real even IC kernel (any real, even prototype filter),
 * no phase compensation, 4 .. 16 timeslots and a power-of-two number of subcarriers >= 16 on the row-lane kernels.  Mode of the handles
 * created afterwards (returns the previous mode): 0 = vector ALU only (f32 throughout), 1 (default) = matrix cores where they are the
 * faster form (blocks of two or more wavefronts: subcarriers >= 128), 2 = matrix cores wherever the form applies. */
int gfdm_hip_set_ic_matrix_cores(int mode);
/* The timeslot-axis transforms of the generic kernel family (shapes outside the tuned row-lane families: more than 48 timeslots, a number of
 * subcarriers with a prime factor above 31 or above 1024; lib/modulator_kernel_cc.cc:109-110,137-140, lib/receiver_kernel_cc.cc:211-225,
 * 274-299, 304-305) are direct sums; from 32 timeslots on they can run on the matrix cores as products of the constant cosine / sine matrices
 * with the block's samples (v_mfma_f32_16x16x4_f32: f32 operands, f32 sums -- no reduced precision).  Mode of the handles created afterwards
 * (returns the previous mode): 0 = vector ALU only, 1 (default) = matrix cores where they are the faster form (the 16 x 16 x 4 operand tiles
 * well filled, at least four of them per block, and the operand scratch does not cost the CU its second workgroup), 2 = wherever the form fits.
 * In mode 1 the reference's own QA shape -- 127 timeslots, 16 subcarriers (python/qa_simple_receiver_cc.py:58-83) -- does not use dense
 * transforms at all for plain blocks (modulate, fft_[equalize_]filter_downsample, generic_work[_equalize], the advanced receiver's cancellation
 * rounds): its 127-point transforms are Rader transforms, cyclic convolutions of length 126 = 9 x 14 through prime-factor FFTs
 * (csrc/gfdm_rader.hip; kernel_name "generic_rader"); frames / demapper and the self-estimating receivers of that shape stay on the generic
 * kernels.  Modes 0 and 2 keep the dense forms for that shape too (A/B, tests). */
int gfdm_hip_set_dft_matrix_cores(int mode);
/* The row-lane kernels of 64 subcarriers move the samples of plain, packed blocks (modulator_work, the receivers without frame offset) two at a
 * time -- 16-byte accesses -- when every device pointer of the call lies on a 16-byte boundary; a call with any pointer that is only 8-byte
 * aligned runs the 8-byte form, with bit-identical results.  enable = 0 keeps every later call on the 8-byte form (tests, A/B runs),
 * 1 (default) restores the choice per call.  Process-wide, takes effect at the next launch; returns the previous setting.  A process started
 * with GFDM_HIP_WIDE_ACCESS=0 in its environment begins with 0. */
int gfdm_hip_set_wide_access(int enable);
/* TEST HOOK: compile (or find in the disk cache) part 0..4 (receive, receive + IC, preamble-equalised receive, modulate, estimator; the
 * sixth part, the receive kernels of demodulate_bursts, builds through gfdm_hip_precompile, bit 5) of
 * the row-lane kernels for a shape through hiprtc WITHOUT loading it --
 * needs no GPU, so the CPU-side tests can check that the embedded kernel sources build. */
int gfdm_hip_jit_build_for_testing(int timeslots, int subcarriers, int overlap, int part);
const char* gfdm_hip_version(void);
/* 16 hex digits: hash of the kernel / C-ABI sources and compiler flags this library was built from.  The rocprofv3 summaries under
 * profiles/ name the build they were measured with; bench.py only quotes counters whose build id equals the loaded library's. */
const char* gfdm_hip_build_id(void);

/* ---- the host-buffer batch path (*_host entry points) -------------------------------------------------------------------------
 * The reference's callers hand HOST pointers and advance them block by block (lib/simple_receiver_cc_impl.cc:61-77,
 * lib/advanced_receiver_sb_cc_impl.cc:86-123 -- in, f_eq and out --, lib/transmitter_cc_impl.cc:165-177); a *_host call takes the
 * whole run of a scheduler call.  How its bytes cross the PCIe link:
 *   - buffers the GPU can address -- registered with gfdm_hip_register_host, allocated with hipHostMalloc, or device memory -- are
 *     used IN PLACE: the kernels run on the caller's memory, bound by the link (~57 GB/s each way on the MI355X boxes);
 *   - ordinary pageable buffers are bounced through pinned staging sets in chunks: the kernel of chunk c works across the link
 *     while the calling thread and a small pool of copy threads move chunk c + 1 in and chunk c - 1 out.  A call that fits one
 *     chunk (<= 512 KiB, e.g. the one block per call of an unchanged GNU Radio wrapper) is copy in, one launch, completion ticket, copy out.
 *   Measured (MI355X box, K=64 M=9, profiles/r04/bench_default.json): pageable 6.4 M blocks/s matched filter, 4.3 M ZF + 2 IC at 65 536 blocks
 *   per call; registered 9.6 M / 6.0 M (88 / 82 GB/s over the link, both directions together); one block per call 13-16 us either way.
 * Results do not depend on the route (same kernels, same blocks).  The call returns when `out` is complete.
 *
 * gfdm_hip_register_host: pin a long-lived buffer (a GNU Radio circular buffer, an application's frame store) and map it for every GPU,
 * ~16 us per MiB once; later *_host calls on any part of it skip the bounce.  The range must be WHOLE PAGES the caller owns -- start and size
 * multiples of the page size (mmap'ed buffers, aligned_alloc / posix_memalign with a page-multiple size), GFDM_HIP_EINVAL otherwise: pinning is
 * per page, and a page shared with other objects must not be pinned and unpinned under them.  Unregister before the memory is freed. */
int gfdm_hip_register_host(void* ptr, size_t bytes);
int gfdm_hip_unregister_host(void* ptr);
/* Process-wide tuning of the bounce (negative = leave unchanged).  mode = how the bytes cross the link: 0 (default) under the kernels' own
 * accesses to the pinned staging memory, 1 copy engines (H2D / kernel / D2H on three streams, device staging), 2 inputs under the kernel's
 * reads and outputs by copy engine, 3 the reverse -- 1 .. 3 are kept for A/B measurements (profiles/r04/host_path_sweep.txt: mode 0 wins
 * or ties everywhere but the largest matched-filter calls); chunk_bytes = staged bytes per chunk over all operands, 0 = automatic (one chunk
 * up to 512 KiB, else about sqrt(1.3 x MiB staged) chunks, at least two, of at most 16 MiB: profiles/r04/host_chunk_sweep.txt); depth = staging
 * sets (1 .. 4, default 3); copy_threads = pool threads that help the calling thread with the bounce copies of chunks >= 1 MiB (0 .. 16,
 * default 3); kernel_streams = 2 (default): the chunks alternate
 * between two streams (a kernel reads its blocks, then writes them, i.e. uses one direction of the link at a time; with two streams the
 * reads of one chunk can run under the writes of another), 1 = a single stream. */
int gfdm_hip_set_host_pipeline(int mode, int64_t chunk_bytes, int depth, int copy_threads, int kernel_streams);
int gfdm_hip_get_host_pipeline(int* mode, int64_t* chunk_bytes, int* depth, int* copy_threads, int* kernel_streams);
/* What the last *_host call of the calling thread did (any pointer may be NULL): kernel launches, blocks per chunk, bytes bounced,
 * bit i of direct_mask = operand i was used in place (operands in signature order: outputs first, then inputs), route, pool threads used. */
int gfdm_hip_host_call_stats(int64_t* chunks, int64_t* chunk_blocks, int64_t* staged_bytes, unsigned* direct_mask, int* mode, int* copy_threads);
/* ... and where the calling thread spent it, nanoseconds: ns5[0] sorting the operands and sizing the staging, [1] bounce copies, [2] enqueueing
 * the kernels, [3] posting completion tickets, [4] waiting for them.  (A one-block call on the MI355X box: 0.3 / 0.4 / 3.8 / 3.1 / 5.1 us.) */
int gfdm_hip_host_call_times(int64_t* ns5);
/* TEST / MEASUREMENT HOOK: the bounce copies of calls that stage 2 MiB or more use non-temporal (streaming) stores; 0 = plain memcpy everywhere
 * (A/B).  Returns the previous setting. */
int gfdm_hip_set_host_streaming_copies_for_testing(int enable);

/* ---- modulator_kernel_cc (include/gfdm/modulator_kernel_cc.h:41-51) -------------------- */

/* ctor, lib/modulator_kernel_cc.cc:30-66.  taps: ntaps interleaved complex; device: HIP ordinal. */
int gfdm_hip_modulator_create(gfdm_hip_modulator** out, int timeslots, int subcarriers, int overlap,
                              const float* taps, int ntaps, int device);
int gfdm_hip_modulator_destroy(gfdm_hip_modulator* m);
int gfdm_hip_modulator_block_size(const gfdm_hip_modulator* m);                 /* block_size(), .h:50 */
int gfdm_hip_modulator_filter_taps(const gfdm_hip_modulator* m, float* out);    /* filter_taps(), .cc:92-95; overlap*timeslots complex */
const char* gfdm_hip_modulator_kernel_name(const gfdm_hip_modulator* m);        /* which HIP kernel family serves this shape */
/* generic_work(out, in), lib/modulator_kernel_cc.cc:98-141, over nblocks blocks */
int gfdm_hip_modulator_work_host(gfdm_hip_modulator* m, float* out, const float* in, int64_t nblocks);
int gfdm_hip_modulator_work_device(gfdm_hip_modulator* m, void* out, const void* in, int64_t nblocks, void* stream);

/* ---- receiver_kernel_cc (include/gfdm/receiver_kernel_cc.h:52-89) ---------------------- */

/* ctor, lib/receiver_kernel_cc.cc:31-88 */
int gfdm_hip_receiver_create(gfdm_hip_receiver** out, int timeslots, int subcarriers, int overlap,
                             const float* taps, int ntaps, int device);
int gfdm_hip_receiver_destroy(gfdm_hip_receiver* r);
int gfdm_hip_receiver_block_size(const gfdm_hip_receiver* r);
int gfdm_hip_receiver_timeslots(const gfdm_hip_receiver* r);
int gfdm_hip_receiver_subcarriers(const gfdm_hip_receiver* r);
int gfdm_hip_receiver_overlap(const gfdm_hip_receiver* r);
int gfdm_hip_receiver_filter_taps(const gfdm_hip_receiver* r, float* out);      /* .cc:120-123 */
int gfdm_hip_receiver_ic_filter_taps(const gfdm_hip_receiver* r, float* out);   /* .cc:125-128; timeslots complex */
const char* gfdm_hip_receiver_kernel_name(const gfdm_hip_receiver* r);

/* generic_work (f_eq == NULL, .cc:322-326) / generic_work_equalize (f_eq != NULL, .cc:328-334);
 * f_eq holds one block_size vector PER BLOCK (lib/advanced_receiver_sb_cc_impl.cc:98-104)
 *
 * Zero, infinite and non-finite data (every receiver entry point: *_demodulate_*, *_fft_filter_downsample_*, the advanced receiver's *_work_*,
 * the *_frames_*, *_estimated_* and *_bursts_* forms, and the modulator / transmitter likewise).  A non-finite result is confined to the block,
 * frame or burst whose input, equaliser or preamble caused it: every other block of the launch is bit-identical to the launch without it.  The
 * equaliser is the reference's division X / f_eq (volk_32fc_x2_divide_32fc, lib/receiver_kernel_cc.cc:315-316) computed as
 * X conj(e) / |e|^2, and what it yields spreads exactly as far as the arithmetic carries it: a bin at subcarrier row j0, column m0 of a block
 * reaches column m0 of the rows k in [j0 - overlap + 1 + overlap/2, j0 + overlap/2] mod subcarriers of fft_equalize_filter_downsample and these
 * rows in full of generic_work_equalize; the advanced receiver decides a NaN like a zero (a finite constellation point), so the same rows stay
 * non-finite, the rows within ic_iter of them may differ from the unpoisoned result and stay finite, and all other rows are bit-identical.
 *   f_eq bin = 0 or NaN:  NaN in the elements named above, as numpy and C99 division give non-finite values there.
 *   f_eq bin infinite:    DEVIATION: NaN in the same elements, on every kernel family (row-lane compiled and run-time instantiated, generic
 *                         in LDS and in global scratch, with vector-ALU and matrix-core transforms and cancellation rounds, Rader), for
 *                         +inf as for inf + inf j -- |e|^2 is inf and inf / inf is NaN -- where numpy and C99 give the quotient 0 for a
 *                         finite X over a real +inf (observed by tests/test_poison_gpu.py::test_equaliser_bin_stays_in_its_rows_and_block).
 *   One NaN or infinite input sample makes its whole block non-finite, one NaN symbol its whole modulated block (the transmitter's frame
 *   behind the preamble); an all-zero received preamble (estimate 0) or one NaN preamble sample makes its whole block non-finite in the
 *   *_estimated_* and *_bursts_* calls, and estimate_frame returns zeros resp. a wholly non-finite estimate for that frame alone.
 *   Samples outside the part a call is documented to read -- a frame outside [cp_len, cp_len + block_size), the gap between two preambles
 *   preamble_stride apart, the capture outside a burst's two windows -- are not read: NaN there changes no bit of the output, and with a
 *   truncating noutput_size nothing is written outside [b noutput_size, (b + 1) noutput_size) of `out` (tests/test_poison_gpu.py). */
int gfdm_hip_receiver_demodulate_host(gfdm_hip_receiver* r, float* out, const float* in, const float* f_eq, int64_t nblocks);
int gfdm_hip_receiver_demodulate_device(gfdm_hip_receiver* r, void* out, const void* in, const void* f_eq, int64_t nblocks, void* stream);
/* fft_filter_downsample (.cc:301-307) / fft_equalize_filter_downsample (.cc:309-320); zero, infinite and NaN f_eq bins: see above */
int gfdm_hip_receiver_fft_filter_downsample_host(gfdm_hip_receiver* r, float* out, const float* in, const float* f_eq, int64_t nblocks);
int gfdm_hip_receiver_fft_filter_downsample_device(gfdm_hip_receiver* r, void* out, const void* in, const void* f_eq, int64_t nblocks, void* stream);
/* transform_subcarriers_to_td (.cc:211-225) */
int gfdm_hip_receiver_transform_subcarriers_to_td_host(gfdm_hip_receiver* r, float* out, const float* in, int64_t nblocks);
int gfdm_hip_receiver_transform_subcarriers_to_td_device(gfdm_hip_receiver* r, void* out, const void* in, int64_t nblocks, void* stream);
/* cancel_sc_interference(out, td_in, fd_in) (.cc:274-299) */
int gfdm_hip_receiver_cancel_sc_interference_host(gfdm_hip_receiver* r, float* out, const float* td_in, const float* fd_in, int64_t nblocks);
int gfdm_hip_receiver_cancel_sc_interference_device(gfdm_hip_receiver* r, void* out, const void* td_in, const void* fd_in, int64_t nblocks, void* stream);

/* ---- advanced_receiver_kernel_cc (include/gfdm/advanced_receiver_kernel_cc.h:37-78) ---- */

/* ctor, lib/advanced_receiver_kernel_cc.cc:32-52.  The gr::digital::constellation_sptr argument of the
 * reference is passed as its points() array plus the decision rule. */
int gfdm_hip_advanced_receiver_create(gfdm_hip_advanced_receiver** out, int timeslots, int subcarriers, int overlap,
                                      const float* taps, int ntaps,
                                      const int* subcarrier_map, int n_subcarrier_map,
                                      int ic_iter,
                                      const float* constellation_points, int n_points, int decision,
                                      int do_phase_compensation, int device);
int gfdm_hip_advanced_receiver_destroy(gfdm_hip_advanced_receiver* a);
int gfdm_hip_advanced_receiver_block_size(const gfdm_hip_advanced_receiver* a);
int gfdm_hip_advanced_receiver_set_ic(gfdm_hip_advanced_receiver* a, int ic_iter);                 /* .h:57 */
int gfdm_hip_advanced_receiver_get_ic(const gfdm_hip_advanced_receiver* a);                        /* .h:58 */
int gfdm_hip_advanced_receiver_set_phase_compensation(gfdm_hip_advanced_receiver* a, int enable);  /* .h:60-63 */
int gfdm_hip_advanced_receiver_get_phase_compensation(const gfdm_hip_advanced_receiver* a);        /* .h:64 */
const char* gfdm_hip_advanced_receiver_kernel_name(const gfdm_hip_advanced_receiver* a);
/* the decision rule the handle RUNS (a gfdm_hip_decision, never AUTO): QPSK / BPSK -- the sign tests, and with a real even IC kernel the
 * matrix-core rounds -- only for GNU Radio's unit constellations (every component within 6 * FLT_EPSILON relative of (+-1 +-j)/sqrt 2 resp. -1, +1 -- this admits gr::digital's 0.707107 literal -- in
 * that order); any other points, also when created with an explicit QPSK / BPSK, are decided by NEAREST over the points as given */
int gfdm_hip_advanced_receiver_decision(const gfdm_hip_advanced_receiver* a);
/* generic_work (f_eq == NULL, .cc:93-98) / generic_work_equalize (f_eq != NULL, .cc:100-107); zero, infinite and NaN f_eq bins, samples: as
 * described at gfdm_hip_receiver_demodulate_* (the affected rows stay non-finite through the cancellation rounds, a halo of ic_iter rows may change) */
int gfdm_hip_advanced_receiver_work_host(gfdm_hip_advanced_receiver* a, float* out, const float* in, const float* f_eq, int64_t nblocks);
int gfdm_hip_advanced_receiver_work_device(gfdm_hip_advanced_receiver* a, void* out, const void* in, const void* f_eq, int64_t nblocks, void* stream);

/* ---- receivers on raw frames with demapped output -----------------------------------
 * In the reference flowgraph the receiver sits between remove_prefix (add_cyclic_prefix_cc::remove_cyclic_prefix,
 * lib/add_cyclic_prefix_cc.cc:100-104) and the resource demapper (resource_mapper_kernel_cc::demap_from_resources,
 * lib/resource_mapper_kernel_cc.cc:91-106,136-163).  Here both are the receiver kernel's load / store stage:
 * configure_frames declares the frame layout once, the *_frames_* calls then read frames of frame_len samples (the block
 * starts cp_len samples in) and write only the active subcarriers' symbols in mapper order, noutput_size per frame
 * (<= 0: all of them).  n_subcarrier_map == 0 keeps the plain [k][m] block output.  f_eq stays one block_size vector per frame.
 * The demapper walks the SORTED map, as the reference constructor does. */
int gfdm_hip_receiver_configure_frames(gfdm_hip_receiver* r, int frame_len, int cp_len, const int* subcarrier_map, int n_subcarrier_map,
                                       int per_timeslot);
int gfdm_hip_receiver_demodulate_frames_host(gfdm_hip_receiver* r, float* out, const float* in, const float* f_eq, int noutput_size,
                                             int64_t nblocks);
int gfdm_hip_receiver_demodulate_frames_device(gfdm_hip_receiver* r, void* out, const void* in, const void* f_eq, int noutput_size,
                                               int64_t nblocks, void* stream);
int gfdm_hip_advanced_receiver_configure_frames(gfdm_hip_advanced_receiver* a, int frame_len, int cp_len, const int* subcarrier_map,
                                                int n_subcarrier_map, int per_timeslot);
int gfdm_hip_advanced_receiver_work_frames_host(gfdm_hip_advanced_receiver* a, float* out, const float* in, const float* f_eq,
                                                int noutput_size, int64_t nblocks);
int gfdm_hip_advanced_receiver_work_frames_device(gfdm_hip_advanced_receiver* a, void* out, const void* in, const void* f_eq,
                                                  int noutput_size, int64_t nblocks, void* stream);

/* ---- transmitter_kernel (include/gfdm/transmitter_kernel.h:43-85) -------------
 * resource mapper -> modulator -> cyclic prefix / suffix with cyclic shift + window ramp -> preamble, FUSED into one HIP kernel:
 * the mapper is the modulator's load stage, prefix/suffix/ramp/preamble its store stage, for all cyclic shifts ("ports") at once. */
typedef struct gfdm_hip_transmitter gfdm_hip_transmitter;

/* ctor, lib/transmitter_kernel.cc:33-73 (which constructs resource_mapper_kernel_cc, modulator_kernel_cc, add_cyclic_prefix_cc).
 * window_taps: n_window_taps complex (the whole window block+cp+cs, or 2*ramp_len); preambles: [n_cyclic_shifts][preamble_len] complex.
 * Argument errors of the three reference constructors are reported as GFDM_HIP_EINVAL / GFDM_HIP_EINVAL_TAPS with their messages. */
int gfdm_hip_transmitter_create(gfdm_hip_transmitter** out, int timeslots, int subcarriers, int active_subcarriers, int cp_len,
                                int cs_len, int ramp_len, const int* subcarrier_map, int n_subcarrier_map, int per_timeslot, int overlap,
                                const float* taps, int ntaps, const float* window_taps, int n_window_taps, const int* cyclic_shifts,
                                int n_cyclic_shifts, const float* preambles, int preamble_len, int device);
int gfdm_hip_transmitter_destroy(gfdm_hip_transmitter* t);
int gfdm_hip_transmitter_input_vector_size(const gfdm_hip_transmitter* t);    /* .h:63, active_subcarriers * timeslots */
int gfdm_hip_transmitter_output_vector_size(const gfdm_hip_transmitter* t);   /* .h:64, preamble + cp + block + cs */
int gfdm_hip_transmitter_block_size(const gfdm_hip_transmitter* t);
int gfdm_hip_transmitter_n_cyclic_shifts(const gfdm_hip_transmitter* t);
int gfdm_hip_transmitter_cyclic_shift(const gfdm_hip_transmitter* t, int port); /* cyclic_shifts()[port], .h:69 */
const char* gfdm_hip_transmitter_kernel_name(const gfdm_hip_transmitter* t);
/* generic_work (lib/transmitter_kernel.cc:100-106) generalised to the first n_outs cyclic shifts, i.e. what
 * transmitter_cc_impl::general_work does per frame (lib/transmitter_cc_impl.cc:165-177).  in: nblocks x ninput_size symbols,
 * outs[i]: nblocks x output_vector_size samples for cyclic_shifts[i]. */
int gfdm_hip_transmitter_work_host(gfdm_hip_transmitter* t, float* const* outs, int n_outs, const float* in, int ninput_size, int64_t nblocks);
int gfdm_hip_transmitter_work_device(gfdm_hip_transmitter* t, void* const* outs, int n_outs, const void* in, int ninput_size,
                                     int64_t nblocks, void* stream);
/* modulate (lib/transmitter_kernel.cc:78-84): mapper + modulator, out = bare blocks */
int gfdm_hip_transmitter_modulate_host(gfdm_hip_transmitter* t, float* out, const float* in, int ninput_size, int64_t nblocks);
int gfdm_hip_transmitter_modulate_device(gfdm_hip_transmitter* t, void* out, const void* in, int ninput_size, int64_t nblocks, void* stream);
/* add_frame (lib/transmitter_kernel.cc:92-98): preamble of `cyclic_shift` + cyclic prefix/suffix + ramp of modulated blocks */
int gfdm_hip_transmitter_add_frame_host(gfdm_hip_transmitter* t, float* out, const float* in, int cyclic_shift, int64_t nblocks);
int gfdm_hip_transmitter_add_frame_device(gfdm_hip_transmitter* t, void* out, const void* in, int cyclic_shift, int64_t nblocks, void* stream);

/* ---- preamble_channel_estimator_cc (include/gfdm/preamble_channel_estimator_cc.h:45-78) ----
 * Received preamble (2 * fft_len samples) -> frequency-domain channel estimate of a whole frame (timeslots * fft_len bins), the
 * f_eq input of the receivers above.  One HIP kernel per call, one workgroup per preamble, every stage LDS-resident;
 * `nframes` preambles / estimates back to back. */
typedef struct gfdm_hip_channel_estimator gfdm_hip_channel_estimator;

/* ctor, lib/preamble_channel_estimator_cc.cc:32-76.  preamble: n_preamble >= 2 * fft_len complex (the known core preamble). */
int gfdm_hip_channel_estimator_create(gfdm_hip_channel_estimator** out, int timeslots, int fft_len, int active_subcarriers, int is_dc_free,
                                      int which_estimator, const float* preamble, int n_preamble, int device);
int gfdm_hip_channel_estimator_destroy(gfdm_hip_channel_estimator* c);
int gfdm_hip_channel_estimator_timeslots(const gfdm_hip_channel_estimator* c);            /* .h:58 */
int gfdm_hip_channel_estimator_fft_len(const gfdm_hip_channel_estimator* c);              /* .h:57 */
int gfdm_hip_channel_estimator_active_subcarriers(const gfdm_hip_channel_estimator* c);   /* .h:60 */
int gfdm_hip_channel_estimator_frame_len(const gfdm_hip_channel_estimator* c);            /* .h:59, timeslots * fft_len */
int gfdm_hip_channel_estimator_is_dc_free(const gfdm_hip_channel_estimator* c);           /* .h:61 */
int gfdm_hip_channel_estimator_filtered_len(const gfdm_hip_channel_estimator* c);         /* active_subcarriers + is_dc_free */
const char* gfdm_hip_channel_estimator_kernel_name(const gfdm_hip_channel_estimator* c);  /* kernel family of estimate_frame */
int gfdm_hip_channel_estimator_preamble_filter_taps(const gfdm_hip_channel_estimator* c, float* out);   /* .h:62, 9 floats; returns 9 */
/* estimate_frame (lib/preamble_channel_estimator_cc.cc:284-295): the three stages below fused.  Bins the reference leaves
 * unwritten when not dc-free ([(A/2 - 1) M, (A/2) M)) carry the value of the constant region next to them. */
int gfdm_hip_channel_estimator_estimate_frame_host(gfdm_hip_channel_estimator* c, float* frame_estimate, const float* rx_preamble, int64_t nframes);
int gfdm_hip_channel_estimator_estimate_frame_device(gfdm_hip_channel_estimator* c, void* frame_estimate, const void* rx_preamble,
                                                     int64_t nframes, void* stream);
/* estimate_preamble_channel (:118-145): rx preamble -> fft_len bins */
int gfdm_hip_channel_estimator_estimate_preamble_channel_host(gfdm_hip_channel_estimator* c, float* fd_preamble_channel, const float* rx_preamble,
                                                              int64_t nframes);
int gfdm_hip_channel_estimator_estimate_preamble_channel_device(gfdm_hip_channel_estimator* c, void* fd_preamble_channel, const void* rx_preamble,
                                                                int64_t nframes, void* stream);
/* filter_preamble_estimate (:147-187): fft_len bins -> filtered_len smoothed bins (fftshift order) */
int gfdm_hip_channel_estimator_filter_preamble_estimate_host(gfdm_hip_channel_estimator* c, float* filtered, const float* estimate, int64_t nframes);
int gfdm_hip_channel_estimator_filter_preamble_estimate_device(gfdm_hip_channel_estimator* c, void* filtered, const void* estimate, int64_t nframes,
                                                               void* stream);
/* interpolate_frame (:238-273): filtered_len bins -> frame_len bins */
int gfdm_hip_channel_estimator_interpolate_frame_host(gfdm_hip_channel_estimator* c, float* frame_estimate, const float* filtered, int64_t nframes);
int gfdm_hip_channel_estimator_interpolate_frame_device(gfdm_hip_channel_estimator* c, void* frame_estimate, const void* filtered, int64_t nframes,
                                                        void* stream);
/* prepare_for_zf (:275-281): conj(1 / frame_estimate) */
int gfdm_hip_channel_estimator_prepare_for_zf_host(gfdm_hip_channel_estimator* c, float* transformed_frame, const float* frame_estimate,
                                                   int64_t nframes);
int gfdm_hip_channel_estimator_prepare_for_zf_device(gfdm_hip_channel_estimator* c, void* transformed_frame, const void* frame_estimate,
                                                     int64_t nframes, void* stream);
/* estimate_snr (:189-236): snr_lin[nframes] (the return value), cnrs[nframes][active_subcarriers] (the std::vector argument) */
int gfdm_hip_channel_estimator_estimate_snr_host(gfdm_hip_channel_estimator* c, float* snr_lin, float* cnrs, const float* rx_preamble, int64_t nframes);
int gfdm_hip_channel_estimator_estimate_snr_device(gfdm_hip_channel_estimator* c, float* snr_lin, float* cnrs, const void* rx_preamble,
                                                   int64_t nframes, void* stream);

/* ---- receivers that estimate the channel themselves (second half) ----
 * The chain  channel_estimator_cc -> (f_eq input of) simple_receiver_cc / advanced_receiver_sb_cc  of
 * examples/hier_gfdm_receiver.grc in ONE kernel: the receiver kernel runs estimate_frame on its block's received preamble
 * and applies the result as its one-tap equaliser; the N-bin estimate never exists in HBM (the preamble's 2 * fft_len samples
 * are read instead of N equaliser bins).  Results equal estimate_frame followed by generic_work_equalize.
 * set_channel_estimator: the estimator handle must match (timeslots, subcarriers, device) and outlive its use; NULL detaches.  (A receiver on
 *   run-time instantiated kernels loads its preamble-equalised kernels here: at once when they are cached or quick to build, otherwise on the
 *   background pool -- the estimated calls run on the generic kernel family, same results, until they are there.)
 * rx_preamble: preamble of block b at rx_preamble + b * preamble_stride complex (0 = packed, 2 * fft_len) -- a burst buffer
 *   holding preamble and frame back to back is passed as `in` and, offset to the core preamble, as `rx_preamble`.
 * The block I/O follows configure_frames when that was called (frames in, demapped symbols out, noutput_size as there),
 * else plain blocks in and out (noutput_size must then be <= 0 or block_size). */
/* Buffer sizes of ONE *_frames_* (estimated == 0) or *_estimated_* (estimated != 0) call with this noutput_size, in complex samples
 * per frame / block: n_in read from `in`, n_out written to `out`, and the attached estimator's fft_len (0 = none).  The library is
 * the authority on these sizes (a caller that derives them itself can under-allocate `out`): EINVAL where the call itself would
 * fail -- no configure_frames / estimator, noutput_size above active_subcarriers * timeslots
 * (lib/resource_mapper_kernel_cc.cc:95-99), or noutput_size given without a subcarrier map (the block is written whole). */
int gfdm_hip_receiver_io_layout(const gfdm_hip_receiver* r, int estimated, int noutput_size, int* n_in, int* n_out, int* est_fft_len);
int gfdm_hip_advanced_receiver_io_layout(const gfdm_hip_advanced_receiver* a, int estimated, int noutput_size, int* n_in, int* n_out,
                                         int* est_fft_len);
int gfdm_hip_receiver_set_channel_estimator(gfdm_hip_receiver* r, const gfdm_hip_channel_estimator* c);
int gfdm_hip_advanced_receiver_set_channel_estimator(gfdm_hip_advanced_receiver* a, const gfdm_hip_channel_estimator* c);
int gfdm_hip_receiver_demodulate_estimated_host(gfdm_hip_receiver* r, float* out, const float* in, const float* rx_preamble, int preamble_stride,
                                                int noutput_size, int64_t nblocks);
int gfdm_hip_receiver_demodulate_estimated_device(gfdm_hip_receiver* r, void* out, const void* in, const void* rx_preamble, int preamble_stride,
                                                  int noutput_size, int64_t nblocks, void* stream);
int gfdm_hip_advanced_receiver_work_estimated_host(gfdm_hip_advanced_receiver* a, float* out, const float* in, const float* rx_preamble,
                                                   int preamble_stride, int noutput_size, int64_t nblocks);
int gfdm_hip_advanced_receiver_work_estimated_device(gfdm_hip_advanced_receiver* a, void* out, const void* in, const void* rx_preamble,
                                                     int preamble_stride, int noutput_size, int64_t nblocks, void* stream);

/* ---- receivers that read detected bursts straight from the capture ----
 * The chain  burst_extractor -> *_estimated_*  in ONE kernel: the extractor's fetch (offset per burst, zero outside the stream, per-sample
 * CFO rotation) is the receiver kernel's load stage, so the extracted burst buffer never exists in memory.  The handle needs a frame
 * layout (frame_len, cp_len) from configure_frames and an attached channel estimator.  For burst b < n_bursts define the virtual burst
 *     e_b[n] = s[off_b - backoff + n] * rho_b^n          0 <= n < frame_len      (n counted from the burst start, as the extractor below)
 *     s[i]   = 0 for i < 0 or i >= stream_len            (the extractor's rule, including its extension past the end)
 *     rho_b  = conj(r_b) / |r_b|;  rho_b = 1 when sc_rot is NULL, r_b == 0 or cfo_correction == 0
 * The result for burst b is what the *_estimated_* call above returns for in = e_b and rx_preamble = e_b + preamble_offset: the same
 * demapping, noutput_size, IC iterations, decision rule and phase compensation; per burst the buffer sizes are those of
 * *_io_layout(estimated = 1, noutput_size).  Only the samples the kernel needs are read: n in [cp_len, cp_len + block_size) and
 * n in [preamble_offset, preamble_offset + 2 fft_len).  Both paths fetch through one device function; their results differ by the
 * compiler's contraction of the rotation only (tested: within 1e-5 relative).
 * There is no `scale` argument: the preamble equaliser divides any per-burst gain out.
 * count: NULL, or one int64 (the detector's `count` output).  live = count ? clamp(*count, 0, n_bursts) : n_bursts; output rows
 * b >= live are written as zeros and their workgroups read nothing from the capture -- the detector's spare slots (frame_start = -1)
 * are exactly those rows, so detect(max_bursts = n) followed by this call is a fixed-shape chain.
 * *_device: samples, offsets (int64[n_bursts]), sc_rot (complex[n_bursts] or NULL) and count are device arrays -- the synchroniser's and
 * the detector's outputs as they are; the call neither allocates nor synchronises and is hipGraph-capturable.  (A receiver on run-time
 * instantiated kernels requests this call's kernels in set_channel_estimator -- at once when they are cached or quick to build, otherwise
 * on the background pool -- under a state of their own: until they are there, or if they fail to build, THIS call runs on the generic
 * kernel family, same results; what the *_estimated_* calls launch, and whether set_channel_estimator succeeds, does not depend on them.)
 * *_host: a convenience, not a pipeline: copies the capture and the arrays to the device, makes one launch and copies the result back.
 * GFDM_HIP_EINVAL (message in gfdm_hip_last_error()): no configure_frames; no estimator attached; preamble_offset < 0 or
 * preamble_offset + 2 fft_len > frame_len; backoff < 0; stream_len < 0; n_bursts < 0; noutput_size as the *_estimated_* calls refuse it.
 * n_bursts == 0 returns GFDM_HIP_OK without a launch. */
int gfdm_hip_receiver_demodulate_bursts_device(gfdm_hip_receiver* r, void* out, const void* samples, int64_t stream_len, const void* offsets,
                                               const void* sc_rot, const void* count, int backoff, int preamble_offset, int cfo_correction,
                                               int noutput_size, int64_t n_bursts, void* stream);
int gfdm_hip_receiver_demodulate_bursts_host(gfdm_hip_receiver* r, float* out, const float* samples, int64_t stream_len, const int64_t* offsets,
                                             const float* sc_rot, const int64_t* count, int backoff, int preamble_offset, int cfo_correction,
                                             int noutput_size, int64_t n_bursts);
int gfdm_hip_advanced_receiver_work_bursts_device(gfdm_hip_advanced_receiver* a, void* out, const void* samples, int64_t stream_len, const void* offsets,
                                                  const void* sc_rot, const void* count, int backoff, int preamble_offset, int cfo_correction,
                                                  int noutput_size, int64_t n_bursts, void* stream);
int gfdm_hip_advanced_receiver_work_bursts_host(gfdm_hip_advanced_receiver* a, float* out, const float* samples, int64_t stream_len,
                                                const int64_t* offsets, const float* sc_rot, const int64_t* count, int backoff, int preamble_offset,
                                                int cfo_correction, int noutput_size, int64_t n_bursts);

/* ---- resource_mapper_kernel_cc (include/gfdm/resource_mapper_kernel_cc.h:38-60, lib/resource_mapper_kernel_cc.cc) -----------------
 * The stand-alone form of the mapper / demapper that the transmitter and the *_frames_* receivers above have fused into their
 * kernels: data symbols <-> the [subcarriers][timeslots] grid the modulator reads and the receivers
 * write.  Blocks back to back: map reads ninput_size symbols per block and writes frame_size; demap reads frame_size and writes
 * noutput_size.  Errors as the reference constructor / methods throw them (:44-69, :78-82, :95-99), as GFDM_HIP_EINVAL with the
 * message in gfdm_hip_last_error().  Two deliberate differences: a subcarrier index EQUAL to `subcarriers` is refused (the reference
 * tests '>' at :65 and then writes past the grid), and the per-subcarrier demapper writes exactly noutput_size symbols (the reference
 * loop :150-161 writes one more when noutput_size < block_size). */
typedef struct gfdm_hip_resource_mapper gfdm_hip_resource_mapper;
int gfdm_hip_resource_mapper_create(gfdm_hip_resource_mapper** out, int timeslots, int subcarriers, int active_subcarriers,
                                    const int* subcarrier_map, int n_subcarrier_map, int per_timeslot, int device);
int gfdm_hip_resource_mapper_destroy(gfdm_hip_resource_mapper* m);
int gfdm_hip_resource_mapper_block_size(const gfdm_hip_resource_mapper* m);      /* timeslots * active_subcarriers   (.h:47) */
int gfdm_hip_resource_mapper_frame_size(const gfdm_hip_resource_mapper* m);      /* timeslots * subcarriers          (.h:46) */
/* map_to_resources (.h:50-52, .cc:74-89): grid zeroed, the first ninput_size symbols placed, the rest of the grid stays zero */
int gfdm_hip_resource_mapper_map_host(gfdm_hip_resource_mapper* m, float* out, const float* in, int ninput_size, int64_t nblocks);
int gfdm_hip_resource_mapper_map_device(gfdm_hip_resource_mapper* m, void* out, const void* in, int ninput_size, int64_t nblocks, void* stream);
/* demap_from_resources (.h:53-55, .cc:91-106) */
int gfdm_hip_resource_mapper_demap_host(gfdm_hip_resource_mapper* m, float* out, const float* in, int noutput_size, int64_t nblocks);
int gfdm_hip_resource_mapper_demap_device(gfdm_hip_resource_mapper* m, void* out, const void* in, int noutput_size, int64_t nblocks, void* stream);

/* ---- add_cyclic_prefix_cc (include/gfdm/add_cyclic_prefix_cc.h:40-60, lib/add_cyclic_prefix_cc.cc) -------------------------------
 * Cyclic prefix + suffix with cyclic shift and the block-pinching window ramps, and prefix removal; the stand-alone form of the
 * transmitter's store stage / the frame receivers' load offset.  window_taps: either the whole window (block_len + cp_len + cs_len
 * taps) or only its 2 * ramp_len ramp taps (.cc:42-56).  add: block_len samples in, frame_size = block_len + cp_len + cs_len out;
 * remove: the reverse (frame[cp_len : cp_len + block_len], .cc:100-104).  cyclic_shift must lie in [0, cs_len] with cp_len + shift
 * <= block_len (the reference reads outside its input otherwise). */
typedef struct gfdm_hip_cyclic_prefixer gfdm_hip_cyclic_prefixer;
int gfdm_hip_cyclic_prefixer_create(gfdm_hip_cyclic_prefixer** out, int block_len, int cp_len, int cs_len, int ramp_len, const float* window_taps,
                                    int n_window_taps, int cyclic_shift, int device);
int gfdm_hip_cyclic_prefixer_destroy(gfdm_hip_cyclic_prefixer* c);
int gfdm_hip_cyclic_prefixer_block_size(const gfdm_hip_cyclic_prefixer* c);
int gfdm_hip_cyclic_prefixer_frame_size(const gfdm_hip_cyclic_prefixer* c);
int gfdm_hip_cyclic_prefixer_cyclic_shift(const gfdm_hip_cyclic_prefixer* c);
/* add_cyclic_prefix(out, in, cyclic_shift) (.cc:66-98); generic_work = the constructor's shift */
int gfdm_hip_cyclic_prefixer_add_host(gfdm_hip_cyclic_prefixer* c, float* out, const float* in, int cyclic_shift, int64_t nblocks);
int gfdm_hip_cyclic_prefixer_add_device(gfdm_hip_cyclic_prefixer* c, void* out, const void* in, int cyclic_shift, int64_t nblocks, void* stream);
int gfdm_hip_cyclic_prefixer_remove_host(gfdm_hip_cyclic_prefixer* c, float* out, const float* in, int64_t nblocks);
int gfdm_hip_cyclic_prefixer_remove_device(gfdm_hip_cyclic_prefixer* c, void* out, const void* in, int64_t nblocks, void* stream);

/* ---- burst acquisition: timing / CFO synchronisation and burst extraction ------------------------------------------------------
 * The two steps in front of the receivers above, on device-resident capture buffers: find each burst's core preamble and CFO, then
 * cut the bursts out, scaled and CFO-corrected.  The synchroniser's outputs feed the extractor's device entry point as they are.
 *
 * gfdm_hip_burst_sync: pygfdm's find_frame_start(s, preamble, K, cp_len) (python/pygfdm/synchronization.py:154-263) on every window
 * s = stream[start_b : start_b + W] of a regular grid start_b = first + b * stride, b < n_windows (W = window_len; a window running past
 * stream_len is GFDM_HIP_EINVAL).  With p the core preamble scaled to unit average energy (initialize_sync_algorithm, :225-236):
 *   ac[i]  = 2 sum_{n<K} conj(s[i+n]) s[i+n+K] / sum_{n<2K} |s[i+n]|^2      i < W - 2K   (auto_correlate_signal, :127-137)
 *            DEVIATION: ac = 0 where the energy is 0; pygfdm yields NaN there
 *   ic[n]  = mean(|ac|[n - cp_len .. n]) for n >= cp_len, else 0                          (abs_integrate, :146-151)
 *   nm     = argmax(ic);  cfo = angle(ac[nm]) / 2 pi, in subcarrier spacings           (auto_correlation_sync, :154-163)
 *   s'[n]  = s[n] exp(j pi cfo n / K): the correction pygfdm applies (:255 with :187-190).  It is not the physical one (half the rate,
 *            opposite sign); it only changes |pcc| and is kept for parity.  It leaves 1.5x the CFO in the signal: beyond about
 *            |cfo| = 0.3 the fine timing can lock to a +-K side peak of the two-half preamble, as pygfdm's does.
 *   pcc[i] = sum_{n<2K} s'[i+n] conj(p[n]) / 2K;  nc = argmax(|pcc[i]| ic[i]) over i < W - 2K   (improved_cross_correlation_peak, :175-187)
 *   every argmax takes the first index of equal values.
 * Outputs per window: frame_start = start_b + nc (int64), coarse = start_b + nm (int64), cfo (float), metric = ic[nm] (float: a window
 * without a burst has a low one), sc_rot = exp(j angle(ac[nm]) / K) (complex: the per-sample rotation present in the signal, in
 * extract_burst_cc's tag convention).  Every position's sums are computed on their own (no running sums), in fp32.
 * auto_correlate: the first stage alone, ac (complex) and ic (float), W - 2K values each per window (either may be NULL, not both).
 * create: EINVAL for n_preamble != 2 fft_len, fft_len outside [2, 1024], cp_len < 0, window_len < 2 fft_len + cp_len + 1.
 * Tested range (against pygfdm fixtures and a float64 restatement of the above: ac and ic within 1e-5, argmax positions exact):
 * fft_len 2, 15, 16, 31, 32, 64, 93, 128, 256, 589 and 1024; cp_len 0 to 600, among them 255, 256 and 257 (either side of the kernels'
 * 256-position tile) and values above 2 fft_len; windows from the smallest, 2 fft_len + cp_len + 1 (one live position), to about
 * 16 million samples (the stream as one window in the detector's tests); up to 32768 + 37 windows per call (beyond 32768 a workgroup
 * takes several), for the regular grid and the start array alike; detect with min_distance up to 2100 at cp_len 600.  The
 * extractor: burst_len 1 to 65536,
 * up to 32768 + 7 bursts per call. */
typedef struct gfdm_hip_burst_sync gfdm_hip_burst_sync;
int gfdm_hip_burst_sync_create(gfdm_hip_burst_sync** out, int fft_len, int cp_len, const float* core_preamble, int n_preamble, int64_t window_len,
                               int device);
int gfdm_hip_burst_sync_destroy(gfdm_hip_burst_sync* s);
int gfdm_hip_burst_sync_fft_len(const gfdm_hip_burst_sync* s);
int gfdm_hip_burst_sync_cp_len(const gfdm_hip_burst_sync* s);
int64_t gfdm_hip_burst_sync_window_len(const gfdm_hip_burst_sync* s);
int64_t gfdm_hip_burst_sync_corr_len(const gfdm_hip_burst_sync* s);          /* window_len - 2 fft_len: ac / ic values per window */
int gfdm_hip_burst_sync_find_frame_start_host(gfdm_hip_burst_sync* s, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                              const float* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows);
int gfdm_hip_burst_sync_find_frame_start_device(gfdm_hip_burst_sync* s, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                                const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows, void* stream);
int gfdm_hip_burst_sync_auto_correlate_host(gfdm_hip_burst_sync* s, float* ac, float* ic, const float* samples, int64_t stream_len, int64_t first,
                                            int64_t stride, int64_t n_windows);
int gfdm_hip_burst_sync_auto_correlate_device(gfdm_hip_burst_sync* s, void* ac, void* ic, const void* samples, int64_t stream_len, int64_t first,
                                              int64_t stride, int64_t n_windows, void* stream);

/* find_frame_start_at: the same five outputs on windows at arbitrary starts.  starts is int64[n_windows] (a device array in the device
 * flavour); window w is stream[st_w : st_w + W] with st_w = clamp(starts[w], 0, stream_len - W) -- clamped, not refused, because starts
 * that live on the device cannot be checked on the host.  The kernels are those of the regular-grid call, so a window's results are
 * bit-equal to find_frame_start(first = st_w, n_windows = 1).  stream_len < W is GFDM_HIP_EINVAL. */
int gfdm_hip_burst_sync_find_frame_start_at_host(gfdm_hip_burst_sync* s, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                                 const float* samples, int64_t stream_len, const int64_t* starts, int64_t n_windows);
int gfdm_hip_burst_sync_find_frame_start_at_device(gfdm_hip_burst_sync* s, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                                   const void* samples, int64_t stream_len, const void* starts, int64_t n_windows, void* stream);

/* detect: every burst of a stream, without the caller knowing where they are (the job of the external detector in front of
 * extract_burst_cc in the reference's flowgraphs; pygfdm's pieces are auto_correlate_signal, abs_integrate and
 * calculate_threshold_factor, python/pygfdm/synchronization.py:132-151, :239-243).
 * Definitions: ac[i] and ic[i] as above over the WHOLE stream as one window: P = stream_len - 2K positions, ac = 0 where the energy
 * is 0, ic[n] = 0 for n < cp_len.  With R = min_distance, position i is a peak when
 *     ic[i] >= threshold,   ic[j] < ic[i] for every j in [i - R, i),   ic[j] <= ic[i] for every j in (i, i + R]
 * (ranges cut at the stream ends): non-maximum suppression in which the first index of equal values wins.  The rule is local, so
 * the result does not depend on how the stream is tiled or batched, and any R + 1 consecutive positions hold at most one peak.
 * Each peak d gets the window start st = clamp(d - lead, 0, stream_len - W); its five outputs are those of find_frame_start on
 * stream[st : st + W] (bit-equal to find_frame_start_at on that start).
 * Arguments, each GFDM_HIP_EINVAL otherwise:  cp_len <= lead <= R;  W - 2K - lead - 1 <= R;  threshold > 0;  max_bursts >= 0;
 * W <= stream_len <= 2^29 (the scan indexes positions in 32 bits; split a longer capture into spans that overlap by W + 2 R);
 * R <= 2^16 (every tile of 1024 to 4096 positions also computes ic over R positions on either side of it, so the scan's work is
 * about 1 + 2 R / tile times that of one pass over the stream: half a burst length is the intended order of magnitude).
 * Why coarse == d away from a clamped edge: the window's positions are the stream's st .. st + W - 2K - 1, and each ac is a function
 * of its own 2K samples only, so window ac == stream ac.  The window's ic at local n >= cp_len sums the same cp_len + 1 magnitudes as
 * the stream's ic at st + n (same order: bit-equal in fp32 too), and is 0 for n < cp_len, where the stream's is >= 0.  The peak sits
 * at local n = lead >= cp_len, so it is present with its full value; every other window position lies within
 * [d - lead, d + W - 2K - lead - 1], i.e. within R of d on either side, where the stream's ic is < ic[d] before d and <= ic[d] after
 * it -- and the window's ic is at most the stream's.  The window's first-index argmax is therefore d.
 * Output: detections in ascending position.  count (one int64; on the device in the device flavour) is the total number of peaks
 * found, also when it exceeds max_bursts.  Slots [0, min(count, max_bursts)) hold the lowest-position detections; the slots after
 * them, up to max_bursts, hold frame_start = coarse = -1, cfo = metric = 0, sc_rot = 0 (the extractor does not rotate those).
 * The device entry point neither allocates nor synchronises (hipGraph-capturable): its scratch -- per-tile peak counts and lists for
 * the ordered compaction, and the window starts -- is the caller's `workspace` of detect_workspace_bytes(s, stream_len) bytes
 * (device memory, 16-byte aligned; its content need not be preserved between calls).  The stream is read once plus a halo of
 * 2 R + cp_len per tile; ic never exists in HBM and nothing is written per position.
 * detect_check: the argument table alone, without a handle or a device. */
int gfdm_hip_burst_sync_detect_check(int fft_len, int cp_len, int64_t window_len, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead,
                                     int64_t max_bursts);
int64_t gfdm_hip_burst_sync_detect_workspace_bytes(const gfdm_hip_burst_sync* s, int64_t stream_len);
int gfdm_hip_burst_sync_detect_host(gfdm_hip_burst_sync* s, int64_t* count, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                    const float* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts);
int gfdm_hip_burst_sync_detect_device(gfdm_hip_burst_sync* s, void* count, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                      const void* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts,
                                      void* workspace, void* stream);

/* gfdm_hip_burst_extractor: extract_burst_cc (lib/extract_burst_cc_impl.cc:72-242) for n bursts given by their tag offsets:
 *   out[b][n] = scale_b * s[off_b - tag_backoff + n] * (conj(r_b) / |r_b|)^n,   n < burst_len   (n counted from the burst start)
 * scale NULL = 1; sc_rot (complex r_b) NULL, |r_b| = 0 or CFO correction off = no rotation.  Samples before 0 read as zero (the
 * reference's prepend); samples at or after stream_len read as zero too -- an EXTENSION: the device entry point takes offsets,
 * scale and sc_rot as device arrays (e.g. the synchroniser's outputs) and cannot check them on the host.  The phase of sample n is
 * reduced in fp64: within 2e-5 of a float64 rotation for any burst_len. */
typedef struct gfdm_hip_burst_extractor gfdm_hip_burst_extractor;
int gfdm_hip_burst_extractor_create(gfdm_hip_burst_extractor** out, int burst_len, int tag_backoff, int activate_cfo_correction, int device);
int gfdm_hip_burst_extractor_destroy(gfdm_hip_burst_extractor* e);
int gfdm_hip_burst_extractor_burst_len(const gfdm_hip_burst_extractor* e);
int gfdm_hip_burst_extractor_tag_backoff(const gfdm_hip_burst_extractor* e);
int gfdm_hip_burst_extractor_set_cfo_correction(gfdm_hip_burst_extractor* e, int activate);   /* activate_cfo_compensation, :100-104 */
int gfdm_hip_burst_extractor_get_cfo_correction(const gfdm_hip_burst_extractor* e);
int gfdm_hip_burst_extractor_extract_host(gfdm_hip_burst_extractor* e, float* out, const float* samples, int64_t stream_len, const int64_t* offsets,
                                          const float* scale, const float* sc_rot, int64_t n_bursts);
int gfdm_hip_burst_extractor_extract_device(gfdm_hip_burst_extractor* e, void* out, const void* samples, int64_t stream_len, const void* offsets,
                                            const void* scale, const void* sc_rot, int64_t n_bursts, void* stream);

/* ---- sc16 captures: interleaved int16 I/Q as UHD streams and capture files deliver it --------------------------------------------
 * Every call above that reads a capture has a *_sc16_* twin.  An sc16 capture of n samples is 2 n int16 values I0, Q0, I1, Q1, ... in
 * native byte order; sample i is (float)I_i + j (float)Q_i, UNSCALED (pygfdm's convert_from_sc16).  stream_len, first, stride, starts
 * and offsets count samples, not int16 values.  `samples` is const int16_t* in the host flavours and a device pointer (const void*) in
 * the device flavours; it needs the alignment of one sample, 4 bytes, and no more (a capture may start at an odd sample of a larger
 * buffer).  Everything else -- the other arguments, checks, error codes, limits, detect_workspace_bytes, count and the spare-slot
 * sentinels, all outputs (complex64 / float32 / int64) -- is that of the call without _sc16.
 * CONTRACT: a *_sc16_* call returns, bit for bit, what its twin returns on the same capture widened to complex64.  int16 -> fp32 is
 * exact, the kernels are the same ones with the sample format as a launch-uniform field, and nothing behind the load depends on it.
 * There is no full-scale argument: ac, ic, cfo, metric and the peak positions do not depend on the scale (an all-zero stretch gives
 * ac = 0 as above), and the preamble equaliser divides any gain out of the receivers; the extractor keeps its per-burst `scale`
 * (1 / 32768 there gives unit full scale).
 * The device flavours neither allocate nor synchronise and are hipGraph-capturable, like their twins.  The host flavours upload the
 * int16 data as it is -- half the bytes of the complex64 copy -- and never widen it on the host. */
int gfdm_hip_burst_sync_find_frame_start_sc16_host(gfdm_hip_burst_sync* s, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                                   const int16_t* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows);
int gfdm_hip_burst_sync_find_frame_start_sc16_device(gfdm_hip_burst_sync* s, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                                     const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows,
                                                     void* stream);
int gfdm_hip_burst_sync_auto_correlate_sc16_host(gfdm_hip_burst_sync* s, float* ac, float* ic, const int16_t* samples, int64_t stream_len, int64_t first,
                                                 int64_t stride, int64_t n_windows);
int gfdm_hip_burst_sync_auto_correlate_sc16_device(gfdm_hip_burst_sync* s, void* ac, void* ic, const void* samples, int64_t stream_len, int64_t first,
                                                   int64_t stride, int64_t n_windows, void* stream);
int gfdm_hip_burst_sync_find_frame_start_at_sc16_host(gfdm_hip_burst_sync* s, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric,
                                                      float* sc_rot, const int16_t* samples, int64_t stream_len, const int64_t* starts, int64_t n_windows);
int gfdm_hip_burst_sync_find_frame_start_at_sc16_device(gfdm_hip_burst_sync* s, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                                        const void* samples, int64_t stream_len, const void* starts, int64_t n_windows, void* stream);
int gfdm_hip_burst_sync_detect_sc16_host(gfdm_hip_burst_sync* s, int64_t* count, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric,
                                         float* sc_rot, const int16_t* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead,
                                         int64_t max_bursts);
int gfdm_hip_burst_sync_detect_sc16_device(gfdm_hip_burst_sync* s, void* count, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                           const void* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts,
                                           void* workspace, void* stream);
int gfdm_hip_burst_extractor_extract_sc16_host(gfdm_hip_burst_extractor* e, float* out, const int16_t* samples, int64_t stream_len, const int64_t* offsets,
                                               const float* scale, const float* sc_rot, int64_t n_bursts);
int gfdm_hip_burst_extractor_extract_sc16_device(gfdm_hip_burst_extractor* e, void* out, const void* samples, int64_t stream_len, const void* offsets,
                                                 const void* scale, const void* sc_rot, int64_t n_bursts, void* stream);
int gfdm_hip_receiver_demodulate_bursts_sc16_host(gfdm_hip_receiver* r, float* out, const int16_t* samples, int64_t stream_len, const int64_t* offsets,
                                                  const float* sc_rot, const int64_t* count, int backoff, int preamble_offset, int cfo_correction,
                                                  int noutput_size, int64_t n_bursts);
int gfdm_hip_receiver_demodulate_bursts_sc16_device(gfdm_hip_receiver* r, void* out, const void* samples, int64_t stream_len, const void* offsets,
                                                    const void* sc_rot, const void* count, int backoff, int preamble_offset, int cfo_correction,
                                                    int noutput_size, int64_t n_bursts, void* stream);
int gfdm_hip_advanced_receiver_work_bursts_sc16_host(gfdm_hip_advanced_receiver* a, float* out, const int16_t* samples, int64_t stream_len,
                                                     const int64_t* offsets, const float* sc_rot, const int64_t* count, int backoff, int preamble_offset,
                                                     int cfo_correction, int noutput_size, int64_t n_bursts);
int gfdm_hip_advanced_receiver_work_bursts_sc16_device(gfdm_hip_advanced_receiver* a, void* out, const void* samples, int64_t stream_len,
                                                       const void* offsets, const void* sc_rot, const void* count, int backoff, int preamble_offset,
                                                       int cfo_correction, int noutput_size, int64_t n_bursts, void* stream);

/* ---- gfdm_hip_burst_shaper: scaled frames in a TX stream, complex64 or sc16 ---------------------------------------------------------
 * The stage between the transmitter's dense [n_bursts][frame_len] array and what a radio or a capture file takes: silence around each
 * burst, the amplitude scale, frames at given sample positions of a continuous stream, conversion to int16 I/Q.  `shape` is gr-gfdm's
 * short_burst_shaper (lib/short_burst_shaper_impl.cc:161-182: zero pre-padding, scale * in, zero post-padding), batched; `place` is the
 * dual of find_frame_start_at / detect.  One handle serves one port; the block's timed commands and tx_time tags are not here.
 * With F = frame_len and the complex `scale` of create:  y_b[n] = scale * frame_b[n], one fp32 complex product
 *     (re = fma(sr, xr, -(si xi)), im = fma(sr, xi, si xr): exact products for a real scale, within 4 * 2^-24 |scale| |x| otherwise).
 * shape: n_bursts frames -> n_bursts * S samples, S = pre_padding + F + post_padding:
 *     out[b S + n] = 0 for n < pre_padding,  y_b[n - pre_padding] for the next F samples,  0 for the rest of the slot.
 * place: the stream has out_len samples and EVERY one of them is written exactly once.  starts is int64[n_bursts], ascending (a device
 *   array in the device flavour); count an optional int64 (on the device in the device flavour; NULL = n_bursts -- detect's count as it
 *   is).  With n_live = clamp(*count, 0, n_bursts) and starts[n_live] := out_len:
 *     out[i] = y_b[i - starts[b]]   where b is the live burst with starts[b] <= i < starts[b + 1], if i - starts[b] < F
 *     out[i] = 0                    everywhere else (before the first start, behind a frame, all of it when n_live = 0).
 *   So a frame that runs into its successor or past out_len is cut there, the part of a frame before sample 0 is dropped, and the frames
 *   from n_live on never appear.  The host flavour refuses what it can see with GFDM_HIP_EINVAL, over the live bursts: starts[0] < 0,
 *   starts that do not ascend, starts[b] + F > starts[b + 1], a last frame running past out_len.  The device flavour cannot check the
 *   starts; the cutting rule keeps it memory-safe (as the clamped window starts do in find_frame_start_at): for starts that do not
 *   ascend the CONTENT of out is unspecified (each sample is 0 or some in-range sample of some live frame), but even then all of
 *   out[0, out_len) and nothing outside it is written, and nothing outside frames[0, n_live * F) is read.
 * Output format: each call has a complex64 flavour and a *_sc16_* twin that writes interleaved int16 I, Q (the format the *_sc16_*
 *   calls above read).  The sc16 value is q(y * g) per component, the product in fp32; q truncates toward zero and saturates to
 *   [-32768, 32767], NaN gives 0.  peak == 0: g = 1, the caller's scale carries the gain.  peak in (0, 32767]: normalised as pygfdm's
 *   convert_to_sc16 does: top = the largest |re| or |im| of y over the live frames of THIS call (whole frames, cut or not), found on
 *   the device, g = (float)((double)peak / (double)top), g = 1 for top == 0.  Each call, and so each port, normalises on its own:
 *   ports that must share one gain take peak = 0 and a common scale.  Non-finite input under normalisation: the values are
 *   unspecified, the call still returns 0.  Against to_sc16 (float64 throughout) a component differs by at most 1 LSB.
 * *_device: out, frames, starts and count are device arrays; out needs the alignment of one sample (8 bytes, sc16: 4 bytes) and no
 *   more -- a stream may start at an odd sample of a larger buffer.  The call neither allocates nor synchronises and is
 *   hipGraph-capturable.  Its scratch (the partial maxima and the gain of a normalised call) is the caller's `workspace` of
 *   workspace_bytes(s, n_bursts, out_len) bytes: device memory, 16-byte aligned, content not preserved between calls and never
 *   assumed; it may be NULL for complex64 and for peak == 0.  When a normalised call has run, its first two floats are g and top (for
 *   the caller's records; nothing reads them back).  No memset fills the gaps: the kernel that writes the frames writes the
 *   zeros.  The stream is written in 16-byte stores aligned in memory whatever pre_padding and the starts are (the first and last
 *   samples of a stream that is itself unaligned go out one by one); byte offsets are 64-bit.
 * *_host: a convenience, not a pipeline: uploads the frames (and starts, count), runs the device call, downloads the stream.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device) and from every call: frame_len < 1; negative
 *   paddings; peak outside {0} and (0, 32767]; n_bursts < 0; out_len < 0; byte sizes (8 n_bursts frame_len, 8 out_len, for shape
 *   8 n_bursts S) that overflow int64.  Also: a NULL buffer that the call would touch.  out_len == 0 returns GFDM_HIP_OK without a
 *   launch; n_bursts == 0 with out_len > 0 writes out_len zeros.
 * Tested range (against a numpy restatement of the above: complex64 and fixed-gain sc16 equal, normalised sc16 equal with top compared
 *   exactly): frame_len 1, 3, 5, 255, 256, 257, 721, 738; paddings 0, 1, 5; 1, 7, 5000 (of 3 samples) and 32768 + 7 (of 5 samples)
 *   bursts per call (bursts are not a grid dimension: a workgroup takes 16 KiB of the stream, whatever lies there); output buffers at
 *   every alignment of one sample.  Streams beyond 2^31 bytes are computed for (64-bit offsets throughout) but not part of the tests. */
typedef struct gfdm_hip_burst_shaper gfdm_hip_burst_shaper;
int gfdm_hip_burst_shaper_create(gfdm_hip_burst_shaper** out, int frame_len, int pre_padding, int post_padding, float scale_re, float scale_im, int device);
int gfdm_hip_burst_shaper_destroy(gfdm_hip_burst_shaper* s);
int gfdm_hip_burst_shaper_frame_len(const gfdm_hip_burst_shaper* s);
int gfdm_hip_burst_shaper_pre_padding(const gfdm_hip_burst_shaper* s);
int gfdm_hip_burst_shaper_post_padding(const gfdm_hip_burst_shaper* s);
int gfdm_hip_burst_shaper_scale(const gfdm_hip_burst_shaper* s, float* scale);          /* scale[0] = re, scale[1] = im */
int gfdm_hip_burst_shaper_check(int frame_len, int pre_padding, int post_padding, double peak, int64_t n_bursts, int64_t out_len);
int64_t gfdm_hip_burst_shaper_workspace_bytes(const gfdm_hip_burst_shaper* s, int64_t n_bursts, int64_t out_len);
int gfdm_hip_burst_shaper_shape_host(gfdm_hip_burst_shaper* s, float* out, const float* frames, int64_t n_bursts);
int gfdm_hip_burst_shaper_shape_device(gfdm_hip_burst_shaper* s, void* out, const void* frames, int64_t n_bursts, void* workspace, void* stream);
int gfdm_hip_burst_shaper_shape_sc16_host(gfdm_hip_burst_shaper* s, int16_t* out, const float* frames, int64_t n_bursts, double peak);
int gfdm_hip_burst_shaper_shape_sc16_device(gfdm_hip_burst_shaper* s, void* out, const void* frames, int64_t n_bursts, double peak, void* workspace,
                                            void* stream);
int gfdm_hip_burst_shaper_place_host(gfdm_hip_burst_shaper* s, float* out, int64_t out_len, const float* frames, const int64_t* starts,
                                     const int64_t* count, int64_t n_bursts);
int gfdm_hip_burst_shaper_place_device(gfdm_hip_burst_shaper* s, void* out, int64_t out_len, const void* frames, const void* starts, const void* count,
                                       int64_t n_bursts, void* workspace, void* stream);
int gfdm_hip_burst_shaper_place_sc16_host(gfdm_hip_burst_shaper* s, int16_t* out, int64_t out_len, const float* frames, const int64_t* starts,
                                          const int64_t* count, int64_t n_bursts, double peak);
int gfdm_hip_burst_shaper_place_sc16_device(gfdm_hip_burst_shaper* s, void* out, int64_t out_len, const void* frames, const void* starts,
                                            const void* count, int64_t n_bursts, double peak, void* workspace, void* stream);

/* ---- gfdm_hip_symbol_mapper: payload bytes to symbols and back, and soft bits -------------------------------------------------------
 * The two ends of the chain: in front of the transmitter GNU Radio's repack_bits_bb (8 -> k bits, GR_MSB_FIRST) + chunks_to_symbols
 * (symbol_table = constellation.points()), behind the receivers constellation_decoder_cb (decision_maker) + repack_bits_bb (k -> 8,
 * GR_MSB_FIRST); pygfdm's bits2symbols / symbols2bits (python/pygfdm/symbolmapping.py).  All calls are batched over ROWS: a row is one
 * frame's or one burst's symbols -- the [n_frames][input_vector_size] the transmitter takes, the [n_bursts][noutput_size] the
 * demodulate_frames / _estimated / _bursts calls return, with detect's count.
 * Constellation: n_points = 2^k complex64 points, 1 <= k <= 8 (anything else is GFDM_HIP_EINVAL); duplicate points are allowed.
 *   `decision` is a gfdm_hip_decision with the meaning it has for gfdm_hip_advanced_receiver_create: AUTO resolves to the sign tests only
 *   for GNU Radio's unit QPSK / BPSK points (every component within 6 * FLT_EPSILON relative, the one rule both constructors share) and
 *   to NEAREST otherwise; an explicit QPSK / BPSK over other points runs as NEAREST; a rule that does not fit n_points is EINVAL.
 *   gfdm_hip_symbol_mapper_decision reports the rule the handle runs (never AUTO).
 * Bit order: a symbol's value is its point index; bit j of a symbol is bit k-1-j of the index (j = 0 is the most significant).  A row of
 *   n_sym symbols is n_sym k bits, packed MSB-first into row_bytes = ceil(n_sym k / 8) bytes; every row starts on a byte; the unused low
 *   bits of a row's last byte are written as 0 by decode and ignored by map.  (repack_bits_bb(..., GR_MSB_FIRST) with align_output;
 *   np.packbits / np.unpackbits; pygfdm's pack_bits.)
 * map:    bytes [n_rows][row_bytes] -> symbols [n_rows][n_sym]:  out[r][i] = points[index], a bit copy of the point as given to create.
 * decode: symbols [n_rows][n_sym] -> bytes [n_rows][row_bytes].  The index of a symbol x, in fp32:
 *     QPSK     index = 2 * (im > 0) + (re > 0)
 *     BPSK     index = (re > 0)
 *     NEAREST  the first i that minimises d_i = (x.re - p_i.re)^2 + (x.im - p_i.im)^2; the comparison is strict and starts from +inf.
 *   From these formulas: NaN decodes to index 0 under every rule; an infinite component decodes to index 0 under NEAREST (no d_i is
 *   below +inf) and by its sign under the sign tests.
 * soft:   symbols [n_rows][n_sym] -> float32 [n_rows][n_sym k], max-log: for bit j of a symbol of row r
 *     llr = s_r * (min over i with bit_j(i) = 1 of d_i  -  min over i with bit_j(i) = 0 of d_i),
 *   d_i the squared distance in the direct form above (never the expanded |x|^2 - 2 Re(x conj p) + |p|^2, which cancels), all in fp32:
 *   positive means bit 0.  `scale` is an optional float32 [n_rows] holding s_r, typically 1 / sigma^2 per burst (NULL: 1; a device array
 *   in the device flavour).  The rule of `decision` plays no part.  A non-finite input symbol makes that symbol's k values unspecified,
 *   and only those.  Against the same formula in float64 a value differs by at most 8 * 2^-24 |s_r| (d0 + d1), d0 and d1 the two minima.
 * count: an optional int64 (on the device in the device flavour; NULL = n_rows -- detect's count as it is).  With
 *   n_live = clamp(*count, 0, n_rows) the rows from n_live on are written as zeros (decode: zero bytes, soft: 0.0f, map: 0 + 0j) and
 *   their input is never read.  Every output element of the n_rows rows is written exactly once whatever count is, by the one kernel of
 *   the call: there is no memset in front, so a graph replay with a changed count is correct.
 * *_device: every array is a device array.  The call neither allocates nor synchronises, needs no workspace and is hipGraph-capturable
 *   (one kernel).  Buffers need the alignment of one element and no more -- 8 bytes for symbols, 1 byte for packed bytes, 4 bytes for LLRs
 *   and scale -- so a block of rows may start anywhere inside a larger buffer; byte offsets are 64-bit.  The grid depends on the total
 *   size, never on n_rows: many short rows and one long row spread alike.
 * *_host: a convenience, not a pipeline: uploads the rows (and scale, count), runs the device call, downloads the result.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device) and from every call: n_points not 2^1 .. 2^8;
 *   n_sym < 1; n_rows < 0; byte sizes (8 n_rows n_sym, 4 k n_rows n_sym) that overflow int64.  Also: a NULL buffer that the call would
 *   touch.  n_rows == 0 returns GFDM_HIP_OK without a launch.
 * Tested range (against a numpy restatement of the above in float64 on the float32 inputs, and pygfdm's own bits2symbols / symbols2bits):
 *   k = 1, 2, 3, 4, 6, 8; n_sym 1, 3, 5, 7, 8, 63, 64, 65, 257, 468, 4097; 1, 7, 5000 (of 3 symbols) and 32768 + 7 (of 5 symbols) rows per
 *   call; buffers at every alignment of one element; count below, at and beyond n_rows. */
typedef struct gfdm_hip_symbol_mapper gfdm_hip_symbol_mapper;
int gfdm_hip_symbol_mapper_create(gfdm_hip_symbol_mapper** out, const float* points, int n_points, int decision, int device);
int gfdm_hip_symbol_mapper_destroy(gfdm_hip_symbol_mapper* m);
int gfdm_hip_symbol_mapper_bits_per_symbol(const gfdm_hip_symbol_mapper* m);
int gfdm_hip_symbol_mapper_n_points(const gfdm_hip_symbol_mapper* m);
int gfdm_hip_symbol_mapper_decision(const gfdm_hip_symbol_mapper* m);
int gfdm_hip_symbol_mapper_points(const gfdm_hip_symbol_mapper* m, float* points);          /* 2 n_points floats: re, im */
int64_t gfdm_hip_symbol_mapper_row_bytes(const gfdm_hip_symbol_mapper* m, int64_t n_sym);
int gfdm_hip_symbol_mapper_check(int n_points, int64_t n_sym, int64_t n_rows);
int gfdm_hip_symbol_mapper_map_host(gfdm_hip_symbol_mapper* m, float* out, const uint8_t* data, const int64_t* count, int64_t n_sym, int64_t n_rows);
int gfdm_hip_symbol_mapper_map_device(gfdm_hip_symbol_mapper* m, void* out, const void* data, const void* count, int64_t n_sym, int64_t n_rows,
                                      void* stream);
int gfdm_hip_symbol_mapper_decode_host(gfdm_hip_symbol_mapper* m, uint8_t* out, const float* symbols, const int64_t* count, int64_t n_sym,
                                       int64_t n_rows);
int gfdm_hip_symbol_mapper_decode_device(gfdm_hip_symbol_mapper* m, void* out, const void* symbols, const void* count, int64_t n_sym, int64_t n_rows,
                                         void* stream);
int gfdm_hip_symbol_mapper_soft_host(gfdm_hip_symbol_mapper* m, float* out, const float* symbols, const float* scale, const int64_t* count,
                                     int64_t n_sym, int64_t n_rows);
int gfdm_hip_symbol_mapper_soft_device(gfdm_hip_symbol_mapper* m, void* out, const void* symbols, const void* scale, const void* count,
                                       int64_t n_sym, int64_t n_rows, void* stream);

/* ---- gfdm_hip_channel_model: multipath, frequency offset and noise on a stream, complex64 or sc16 out ------------------------------
 * The link between the burst shaper's TX stream and the synchroniser's capture: GNU Radio's channels.channel_model(noise_voltage,
 * frequency_offset, epsilon, taps, noise_seed) as the reference's end-to-end flowgraph places it (examples/gfdm_simulation_demo.grc),
 * with epsilon = 1 (the demo's value; resampling is not part of this: gfdm_hip_resampler below).  Order as in GNU Radio: FIR, then mixer, then noise.  The taps
 * are fixed at create; frequency_offset, noise_voltage and seed are host state with setters, read when a call is enqueued -- a captured
 * graph keeps the values it was captured with.
 * With T = n_taps, h the taps as given (complex64), f = frequency_offset in cycles per sample, s = noise_voltage, a = offset + i the
 * ABSOLUTE index of sample i of the call, for 0 <= i < n:
 *     x[j] = in[j] for -history <= j < n,  0 for j < -history
 *     v[i] = sum_{t < T} h[t] * x[i - t]
 *     r[i] = v[i] * exp(j 2 pi frac(f * a))
 *     y[i] = r[i] + (s / sqrt 2) * w(a)
 * history: `in` points at sample 0 and the `history` samples in front of it are readable (GNU Radio's FIR history, which starts as
 *   zeros: the first call of a stream takes history = 0, the later ones min(T - 1, samples so far)).
 * v[i]: fp32, the first term a complex product, then one complex fma per tap with t ascending -- the same chain for every i.  Where every
 *   tap has imaginary part 0 the products with it are left out, so T = 1, h = 1 copies x bit for bit.
 * r[i]: p = f * (double)a rounded to fp64 once, frac = p - rint(p) (exact), then sincospi of (float)(2 frac) and one fp32 complex
 *   product.  f == 0 leaves r = v bit for bit.  (Beyond a = 2^53 / f the fp64 product itself is coarser than the phase; the contract is
 *   this formula, not the real-number one.)
 * y[i]: re = fma(sigma, w.re, r.re) with sigma = (float)(s / sqrt 2), im alike.  s == 0 leaves y = r bit for bit.
 * w(a) is a pure function of (seed, a), so a stream cut into calls at any point gives the same samples:
 *     Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) on the counter
 *     (lo32(a >> 1), hi32(a >> 1), 0, 0) under the key (lo32(seed), hi32(seed)); even a takes output words (0, 1), odd a words (2, 3),
 *     as (k0, k1);  u = ((k0 >> 8) + 0.5) * 2^-24,  t = (k1 >> 8) * 2^-24,  w = sqrt(-2 ln u) * (cos 2 pi t, sin 2 pi t),
 *   with the accurate logf, sqrtf and sincospif.  t is exact in fp32; u has 25 significant bits from 0.5 on, so ln u is taken as
 *   ln(fl32(u)) + (u - fl32(u)) / fl32(u), the residual formed exactly.  E|w|^2 = 2, so the noise power is s^2; |w| <= 5.89.
 * sc16 twin: interleaved int16 q(y.re * gain), q(y.im * gain), the products in fp32, q the burst shaper's rule (truncate toward zero,
 *   saturate, NaN -> 0).
 * Error budget against the same formulas in float64 on the same complex64 inputs, with S_i = sum_t |h[t]| |x[i - t]|:
 *     |y - y64| <= (T + 10) * 2^-23 * S_i  +  2^-20 * (s / sqrt 2) * |w(a)|  +  2^-23 * |y64|
 *   (the length-T complex fma chain; the fp32 cast of the reduced phase, <= 2 ulp sincospi and one complex product, < 2^-20 relative;
 *   <= 2 ulp log, one sqrt, <= 2 ulp sincospi and two products; the final fma).  Derived, not measured.
 * *_device: in and out are device arrays with the alignment of one element and no more (8 bytes, sc16 out 4 bytes); byte offsets are
 *   64-bit.  out overlapping [in - history, in + n) is GFDM_HIP_EINVAL: the FIR reads neighbours, there is no in-place call.  No
 *   workspace, no allocation, no synchronisation: one kernel, hipGraph-capturable.  Every input sample is read from memory once per
 *   tile of 2044 output samples (plus the T samples in front of the tile); the stream is written in 16-byte stores aligned in memory
 *   whatever the alignment of out and the parity of offset are, the first and last samples of an unaligned stream one by one.
 * *_host: a convenience, not a pipeline: uploads history + n samples, runs the device call, downloads n.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device), from create, the setters and every call: n_taps
 *   outside 1 .. 64; a non-finite tap (create), frequency_offset, noise_voltage or gain; |frequency_offset| > 0.5; noise_voltage < 0;
 *   n, history or offset negative; offset + n > 2^62; a byte size (8 (history + n)) that overflows int64.  Also: a NULL buffer that the
 *   call would touch.  n == 0 returns GFDM_HIP_OK without a launch.
 * Tested range (against a float64 numpy restatement of the above with its own Philox, held to the generator's published known answers):
 *   T 1, 2, 3, 8, 64; n 1, 2, 3, 255, 256, 257, 4097, 65539 and 2^20; history 0, 1, T - 2, T - 1, T + 5; f 0, 0.002, 1/3, 0.4999,
 *   -0.5; s 0, 1; offset 0, 1, 2^31 - 1, 2^33 - 3, 2^40 + 1; in and out at every alignment of one element.  Worst measured share of
 *   the error budget: 0.22 (T = 3 with mixer and noise), 0.21 on 2^20 samples of noise alone, 0.15 over the table of shapes; sc16 differs
 *   from q of the float64 value only inside gain * budget of a step of q (at most 0.6 % of the components of a tested case), by one LSB. */
typedef struct gfdm_hip_channel_model gfdm_hip_channel_model;
int gfdm_hip_channel_model_create(gfdm_hip_channel_model** out, const float* taps, int n_taps, double frequency_offset, double noise_voltage,
                                  uint64_t seed, int device);          /* taps: 2 n_taps floats: re, im */
int gfdm_hip_channel_model_destroy(gfdm_hip_channel_model* c);
int gfdm_hip_channel_model_n_taps(const gfdm_hip_channel_model* c);
int gfdm_hip_channel_model_taps(const gfdm_hip_channel_model* c, float* taps);
int gfdm_hip_channel_model_frequency_offset(const gfdm_hip_channel_model* c, double* frequency_offset);
int gfdm_hip_channel_model_noise_voltage(const gfdm_hip_channel_model* c, double* noise_voltage);
int gfdm_hip_channel_model_seed(const gfdm_hip_channel_model* c, uint64_t* seed);
int gfdm_hip_channel_model_set_frequency_offset(gfdm_hip_channel_model* c, double frequency_offset);
int gfdm_hip_channel_model_set_noise_voltage(gfdm_hip_channel_model* c, double noise_voltage);
int gfdm_hip_channel_model_set_seed(gfdm_hip_channel_model* c, uint64_t seed);
int gfdm_hip_channel_model_check(int n_taps, double frequency_offset, double noise_voltage, int64_t n, int64_t history, int64_t offset, double gain);
int gfdm_hip_channel_model_apply_host(gfdm_hip_channel_model* c, float* out, const float* in, int64_t n, int64_t history, int64_t offset);
int gfdm_hip_channel_model_apply_device(gfdm_hip_channel_model* c, void* out, const void* in, int64_t n, int64_t history, int64_t offset, void* stream);
int gfdm_hip_channel_model_apply_sc16_host(gfdm_hip_channel_model* c, int16_t* out, const float* in, int64_t n, int64_t history, int64_t offset,
                                           double gain);
int gfdm_hip_channel_model_apply_sc16_device(gfdm_hip_channel_model* c, void* out, const void* in, int64_t n, int64_t history, int64_t offset,
                                             double gain, void* stream);

/* ---- gfdm_hip_resampler: fractional-rate resampling of a stream, complex64 or sc16 in, complex64 out -------------------------------
 * The stage the channel model above leaves out (GNU Radio's channels.channel_model starts with a fractional resampler driven by
 * epsilon), and the conversion of a capture taken at a radio's rate to the GFDM rate in front of detect: place -> resample -> apply,
 * capture -> resample -> detect.  A polyphase interpolator that does the work of GNU Radio's mmse_resampler_cc /
 * pfb_arb_resampler_ccf.  Positions are integers (unsigned Q32.32), so every result is a pure function of its arguments and a stream
 * cut into calls at any point gives the same samples to the bit.  Bit-compatibility with GNU Radio's MMSE tap table is unpinned: the
 * table is the caller's (gfdm_amd.resampler_taps builds a Kaiser-windowed sinc).
 * create: T = n_taps in 1 .. 64; L = n_phases a power of two in 1 .. 1024, lg = log2 L; taps: (L + 1) * T real fp32 values, row p, tap
 *   t, h[p][t] = taps[p * T + t], row L being row 0 moved by one sample as in GNU Radio's table; (L + 1) * T <= 8256; interp 0 (the
 *   nearest row, GNU Radio's mmse rule) or 1 (linear between neighbouring rows); step = the input advance per output sample as unsigned
 *   Q32.32, 2^29 <= step <= 2^35 (1/8 .. 8).  Table and interp are fixed at create; step is host state with a setter, read when a call
 *   is enqueued -- a captured graph keeps the value it was captured with.
 * With D = (T - 1) / 2 in integer division and pos the Q32.32 position of output 0 relative to in[0], for 0 <= i < n_out:
 *     P(i)   = pos + i * step                 an exact integer below 2^94: the product from mul-hi / mul-lo, there is no float
 *     idx    = P >> 32,   frac = P & (2^32 - 1)
 *     interp 0:  p = (frac + 2^(31 - lg)) >> (32 - lg)  in 0 .. L     (in 64 bits, so that L = 1 shifts by 32: p = frac >> 31),
 *                c[t] = h[p][t]
 *     interp 1:  q = frac >> (32 - lg)  in 0 .. L - 1                   (in 64 bits; L = 1: q = 0),
 *                w = fp32 of ((frac << lg) mod 2^32) >> 8, times 2^-24   (the next 24 bits of frac below q's bits -- for lg > 8 the
 *                    last lg - 8 of them lie below frac's end and are zeros; exact; L = 1: the top 24 bits of frac),
 *                c[t] = fmaf(w, d[q][t], h[q][t]),   d[q][t] = fp32(h[q + 1][t] - h[q][t])   (one rounding; the kernel forms it from
 *                    the two rows where it needs it, which is that same rounding, so there is no second table)
 *     x[j]   = in[j] for -history <= j < n_in,  0 elsewhere              (as the extractor reads zeros past the capture)
 *     y[i]   = sum_{t < T} c[t] * x[idx - D + t]      fp32 per component: the first term a product, then one fma per tap, t ascending
 *   So T = 1, h = 1, step = 2^32, pos = 0 copies x bit for bit, and a table whose row 0 is the unit impulse at tap D copies every
 *   finite non-zero component bit for bit at step = 2^32, pos = 0 (a zero component may come out as +0: the chain starts from 0 * x).
 * plan(step, n_taps, pos, n_in, flush, &n_out, &advance, &next_pos): host arithmetic alone, no handle and no device.  n_out = the
 *   number of i >= 0 with idx(i) - D + T - 1 < n_in (every sample of the window is there), with flush != 0 with idx(i) < n_in (the last
 *   piece: zeros lie behind the end); advance = min(n_in, idx(n_out)); next_pos = pos + n_out * step - advance * 2^32.  The next piece
 *   passes in + advance, next_pos and history = min(D, samples in front of it).  Any of the three result pointers may be NULL.
 * resample_*: `in` points at sample 0; the `history` samples in front of it are readable.  The sc16 twins read interleaved int16 I/Q,
 *   widened exactly, one 4-byte load per sample: bit-equal to the complex64 call on the widened capture.  Output is always complex64.
 * *_device: element alignment only (out 8 bytes; in 8, sc16 4) with 64-bit byte offsets; out overlapping [in - history, in + n_in) is
 *   GFDM_HIP_EINVAL; n_out == 0 returns GFDM_HIP_OK without a launch; no workspace, no allocation, no synchronisation: one kernel,
 *   hipGraph-capturable.  A workgroup owns tiles of consecutive outputs cut at 16-byte boundaries of memory; per tile the input span
 *   [idx(first) - D, idx(last) - D + T) goes to LDS once (zeros and the widening applied there), the table once per workgroup; the
 *   stream is written in 16-byte stores aligned in memory whatever the alignment of out, its first and last sample alone if need be.
 * *_host: a convenience, not a pipeline: uploads history + n_in samples, runs the device call, downloads n_out.
 * Error budget against the same formulas with Python integers for P, idx, frac, p, q, w and float64 for c and the sum, on the same
 *   fp32 table and samples, with S_i = sum_t |c[t]| |x[idx - D + t]|:
 *     |y - y64| <= (T + 4) * 2^-23 * S_i       (one fma for c, the length-T chain, the final rounding).  Derived, not measured.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device), from create, set_step, plan and every call:
 *   n_taps outside 1 .. 64; n_phases no power of two in 1 .. 1024; (L + 1) * T > 8256; interp not 0 or 1; step outside 2^29 .. 2^35; a
 *   non-finite tap (create); n_out, n_in, history or pos negative; pos >= 2^62; pos + n_out * step >= 2^94; a byte size (8 n_out,
 *   8 (history + n_in)) that overflows int64 -- in plan: an n_out whose 8 n_out would.  Also: a NULL buffer that the call would touch
 *   (`in` may be NULL when history + n_in == 0: every x is zero).
 * Tested range (against the restatement of tests/resampler_ref.py): T 1, 2, 3, 8, 16, 64; L 1, 2, 128, 1024 within the cap; both
 *   interp; n_out 1, 2, 3, 255, 256, 257, 4097, 65539; step 2^29, 2^32, 2^32 + 1, round(1.0001 * 2^32), 3 * 2^31, 2^35; pos with
 *   fraction 0, 2^31, 2^32 - 1 and integer part 0 and 5; history 0, 1, D - 1, D, D + 5; n_in short of the last windows; in and out at
 *   every alignment of one element, complex64 and sc16 in -- 24 cases per T that go round these values with the case number, not their
 *   cross product: every value occurs with every T, not with every other value.  End to end: a clock offset of 100 ppm with half a
 *   sample of static offset between place and apply, and a 4/5 - 5/4 rate change around apply (8 taps, complex64 and sc16 between).
 *   Accuracy of the default table (gfdm_amd.resampler_taps) on a tone, measured on the restatement: linear is never worse than nearest,
 *   and T = 16 is not worse than T = 8 with linear; with the nearest row the error is the row's position error, about pi f / L whatever
 *   T is, and T = 16 measured 0.07 % ABOVE T = 8 at L = 32 (1.0801e-2 against 1.0794e-2): "more taps are not worse" is tested for linear
 *   alone, and nearest is held to pi f / L + the linear error instead.  Worst measured share of the error budget: 0.163 over the table of shapes (T = 1;
 *   0.157, 0.138, 0.106, 0.064, 0.021 for T = 2, 3, 8, 16, 64), 0.113 on sc16 input (profiles/r19/resampler_accuracy.json). */
typedef struct gfdm_hip_resampler gfdm_hip_resampler;
int gfdm_hip_resampler_create(gfdm_hip_resampler** out, const float* taps, int n_taps, int n_phases, int interp, uint64_t step, int device);
int gfdm_hip_resampler_destroy(gfdm_hip_resampler* c);
int gfdm_hip_resampler_n_taps(const gfdm_hip_resampler* c);
int gfdm_hip_resampler_n_phases(const gfdm_hip_resampler* c);
int gfdm_hip_resampler_interp(const gfdm_hip_resampler* c);
int gfdm_hip_resampler_taps(const gfdm_hip_resampler* c, float* taps);          /* (n_phases + 1) * n_taps floats */
int gfdm_hip_resampler_step(const gfdm_hip_resampler* c, uint64_t* step);
int gfdm_hip_resampler_set_step(gfdm_hip_resampler* c, uint64_t step);
int gfdm_hip_resampler_check(int n_taps, int n_phases, int interp, uint64_t step, int64_t n_out, int64_t n_in, int64_t history, int64_t pos);
int gfdm_hip_resampler_plan(uint64_t step, int n_taps, int64_t pos, int64_t n_in, int flush, int64_t* n_out, int64_t* advance, int64_t* next_pos);
int gfdm_hip_resampler_resample_host(gfdm_hip_resampler* c, float* out, const float* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos);
int gfdm_hip_resampler_resample_device(gfdm_hip_resampler* c, void* out, const void* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos,
                                       void* stream);
int gfdm_hip_resampler_resample_sc16_host(gfdm_hip_resampler* c, float* out, const int16_t* in, int64_t n_out, int64_t n_in, int64_t history,
                                          int64_t pos);
int gfdm_hip_resampler_resample_sc16_device(gfdm_hip_resampler* c, void* out, const void* in, int64_t n_out, int64_t n_in, int64_t history,
                                            int64_t pos, void* stream);

/* ---- gfdm_hip_fading_model: time-varying multipath on a stream, complex64 or sc16 out ------------------------------------------------
 * The channel that changes from burst to burst, in front of the channel model above (whose FIR is fixed at create and which keeps the
 * frequency offset and the noise): place -> [resample] -> fade -> apply(taps = [1], f, noise) -> detect.  What GNU Radio's
 * channels.fading_model / channels.selective_fading_model do in a flowgraph: P paths, each a real delay line (a fractional delay times
 * a magnitude) times a complex gain that is a sum of sinusoids (Clarke's model, a line-of-sight term being one more sinusoid).  The
 * phases are 64-bit integers, so every output is a pure function of the tables and the ABSOLUTE sample index and a stream cut into calls
 * at any point gives the same samples to the bit.  Bit-compatibility with GNU Radio's fader is unpinned: its arrival angles walk
 * randomly from sample to sample and so cannot be a function of the index; the tables are the caller's (gfdm_amd.fading_taps and
 * gfdm_amd.fading_sinusoids build a stratified Monte-Carlo Clarke model from a seed).
 * create: P = n_paths in 1 .. 8, S = n_sinusoids in 1 .. 17, T = n_taps in 1 .. 64; four tables, fixed at create, copied to the device
 *   there, read back by the getters bit for bit:
 *     c   [P][T] fp32      real delay-line coefficients of path p
 *     A   [P][S] fp32      amplitude of sinusoid s of path p
 *     F   [P][S] int64     frequency, signed, in units of 2^-64 cycles per sample
 *     Ph0 [P][S] uint64    start phase in units of 2^-64 turns
 *   There are no setters: another Doppler is another handle.
 * With a = offset + i the ABSOLUTE index of sample i of the call, for 0 <= i < n:
 *     x[j]         = in[j] for -history <= j < n,  0 for j < -history           (history as in the channel model)
 *     Phi[p][s](a) = (F[p][s] * a + Ph0[p][s]) mod 2^64                         64-bit wrap-around integers, exact
 *     e[p][s](a)   = exp(j 2 pi (Phi >> 32) / 2^32)                             the top 32 bits are the phase
 *     g[p](a)      = sum_s A[p][s] * e[p][s](a)
 *     v[p][i]      = sum_{k < T} c[p][k] * x[i - k]
 *     y[i]         = sum_p g[p](a) * v[p][i]
 * In fp32, no fp64 on the device.  The phasors are formed per aligned run of eight absolute indices 8 r .. 8 r + 7: at 8 r from the
 *   integer phase (its nearest 24 bits through sincospif, whose argument is then exact, the remaining 8 by a first-order turn), times A;
 *   at 8 r + m by at most three complex products with exp(j 2 pi F m' / 2^64), m' = 1, 2, 4, which create tabulates from fp64.  The runs
 *   are aligned in a, not in i, so the value of a sample does not depend on where a call or a tile begins.  g sums s ascending from 0;
 *   v is one fma per tap and component, k ascending from 0; y sums p ascending from 0, two fmas per component.  Every step is linear in x,
 *   so scaling x by a power of two scales y exactly; A = 1, F = 0, Ph0 = 0, c = 1 returns x equal in every finite component.
 * sc16 twin: interleaved int16 q(y.re * gain), q(y.im * gain), the products in fp32 from the same fp32 y as the complex64 call, q the
 *   burst shaper's rule (truncate toward zero, saturate, NaN -> 0).
 * Error budget against the same formulas in float64 on the same complex64 inputs, with Abar_p = sum_s |A[p][s]| and
 *   S_pi = sum_k |c[p][k]| |x[i - k]|:
 *     |y - y64| <= (T + P + 16) * 2^-23 * sum_p Abar_p * S_pi
 *   (the length-T real-by-complex fma chain per path; a phasor per sinusoid -- the phase's last bits, <= 2 ulp sincospi, the product with
 *   A -- with its rotations behind it; the sums over s and p).  Counted from roundings, not from what the kernel gives.
 * *_device: in and out are device arrays with the alignment of one element and no more (8 bytes, sc16 out 4 bytes); byte offsets are
 *   64-bit.  out overlapping [in - history, in + n) is GFDM_HIP_EINVAL: the delay lines read neighbours, there is no in-place call.  No
 *   workspace, no allocation, no synchronisation: one kernel, hipGraph-capturable.  Every input sample is read from memory once per tile
 *   of 2040 output samples (plus the T + 14 samples around the tile); the stream is written in 16-byte stores aligned in memory whatever
 *   the alignment of out and the value of offset are, the first and last samples of an unaligned stream one by one.  At most 2048
 *   workgroups per launch, which stride over the tiles beyond.
 * *_host: a convenience, not a pipeline: uploads history + n samples, runs the device call, downloads n.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device), from create and every call: n_paths outside
 *   1 .. 8, n_sinusoids outside 1 .. 17, n_taps outside 1 .. 64; a NULL table, a non-finite c or A (create); a non-finite gain; n,
 *   history or offset negative; offset + n > 2^62; a byte size (8 (history + n)) that overflows int64.  Also: a NULL buffer that the
 *   call would touch.  n == 0 returns GFDM_HIP_OK without a launch.
 * Tested range (against the float64 numpy restatement of tests/fading_model_ref.py, whose phases are held to Python integers):
 *   (P, S, T) (1, 1, 1), (1, 8, 1), (2, 3, 3), (4, 8, 16), (8, 17, 64); n 1, 2, 7, 8, 9, 255, 256, 257, 4097, 65539; history 0, 1,
 *   T - 2, T - 1, T + 5; offset 0, 1, 7, 2^31 - 1, 2^33 - 3, 2^40 + 1; in and out at every alignment of one element, complex64 and
 *   sc16 -- 20 cases per shape that go round these values with the case number; 2 * 2048 + 3 tiles in one launch.
 *   Bit for bit: a stream in one call against the same stream cut at 1, 7, 8, 9 and at a seeded ragged list of points; sc16 against
 *   q(fp32 y * gain) of the complex64 call; apply(4 x) against 4 apply(x); host flavour against device flavour; a graph replay against
 *   the eager call.  Against the channel model: every F = 0 against its FIR with the taps sum_p g_p c[p][:], and P = S = T = 1 against
 *   its mixer at f = 0.002, 1/3, -0.5 and offsets up to 2^33, within the two budgets added (worst 0.31 of them, at f = 1/3 and 2^33,
 *   where the channel model's float64 product f * a carries 2^-22 of a cycle).  Worst measured share of the error budget: 0.119 over the
 *   table of shapes (P = S = T = 1; 0.074, 0.054, 0.016, 0.006 for the other four shapes in the order above), 0.055 past the bounded
 *   grid, 0.020 on the faded stream of the end-to-end loop; a float32 numpy emulation of the same scheme without fused multiply-adds
 *   reaches 0.134, and its gains alone 1.7 * 2^-23 * Abar of the 12 that the budget grants them.  sc16 differs from q of the float64
 *   value only inside gain * budget of a step of q (at most 0.6 % of the components of a tested case), by one LSB
 *   (profiles/r20/fading_accuracy.json). */
typedef struct gfdm_hip_fading_model gfdm_hip_fading_model;
int gfdm_hip_fading_model_create(gfdm_hip_fading_model** out, const float* c, const float* A, const int64_t* F, const uint64_t* Ph0, int n_paths,
                                 int n_sinusoids, int n_taps, int device);
int gfdm_hip_fading_model_destroy(gfdm_hip_fading_model* m);
int gfdm_hip_fading_model_n_paths(const gfdm_hip_fading_model* m);
int gfdm_hip_fading_model_n_sinusoids(const gfdm_hip_fading_model* m);
int gfdm_hip_fading_model_n_taps(const gfdm_hip_fading_model* m);
int gfdm_hip_fading_model_taps(const gfdm_hip_fading_model* m, float* c);                 /* n_paths * n_taps */
int gfdm_hip_fading_model_amplitudes(const gfdm_hip_fading_model* m, float* A);          /* n_paths * n_sinusoids, as the two below */
int gfdm_hip_fading_model_frequencies(const gfdm_hip_fading_model* m, int64_t* F);
int gfdm_hip_fading_model_phases(const gfdm_hip_fading_model* m, uint64_t* Ph0);
int gfdm_hip_fading_model_check(int n_paths, int n_sinusoids, int n_taps, int64_t n, int64_t history, int64_t offset, double gain);
int gfdm_hip_fading_model_apply_host(gfdm_hip_fading_model* m, float* out, const float* in, int64_t n, int64_t history, int64_t offset);
int gfdm_hip_fading_model_apply_device(gfdm_hip_fading_model* m, void* out, const void* in, int64_t n, int64_t history, int64_t offset, void* stream);
int gfdm_hip_fading_model_apply_sc16_host(gfdm_hip_fading_model* m, int16_t* out, const float* in, int64_t n, int64_t history, int64_t offset,
                                          double gain);
int gfdm_hip_fading_model_apply_sc16_device(gfdm_hip_fading_model* m, void* out, const void* in, int64_t n, int64_t history, int64_t offset,
                                            double gain, void* stream);

/* ---- gfdm_hip_amplifier_model: the transmitter's power amplifier on a stream, complex64 or sc16 out ---------------------------------
 * The stage between the burst shaper (or the resampler) and the fading / channel model: place -> [resample] -> amplify -> [fade] ->
 * apply.  Four kinds, fixed at create; drive is host state with a setter, read when a call is enqueued (a back-off sweep needs one
 * handle; a captured graph keeps the value it was captured with).  Nothing depends on the absolute sample index: there is no offset.
 * With d = (float)drive, for 0 <= i < n:
 *     x[j] = in[j] for -history <= j < n,  0 for j < -history
 *     u[j] = d * x[j] (the fp32 product of each component),  r[j] = |u[j]|^2
 *   kind    params            y[i]
 *   CLIP    A                 u where r <= A^2, bit for bit; else u * A / sqrt(r)
 *   RAPP    g, A, p           g u (1 + t^p)^(-1 / (2 p)),  t = g^2 r / A^2
 *   SALEH   aa, ba, ap, bp    u * aa / (1 + ba r) * exp(j ap r / (1 + bp r))
 *   POLY    none              sum_{q < Q} sum_{k < K} c[q][k] u[i - q] r[i - q]^k      (the odd orders 1, 3, .. 2 K - 1)
 * params are doubles that create rounds to fp32: the formulas hold for the rounded values, and the getter returns those.  POLY takes
 *   Q = n_delays, K = n_orders and 2 Q K floats (re, im of c[q][k], k fastest) instead; the other kinds take n_delays = n_orders = 0.
 * Arithmetic: fp32 without contraction, every fused multiply-add written out, correctly rounded division and sqrtf, the accurate powf
 *   and sincosf.  r = fma(u.re, u.re, u.im * u.im).  CLIP compares r with fl32(A^2), s = A / sqrt(r), y = u * s.  RAPP: t = fl32(g^2 /
 *   A^2) * r; where t <= 1, s = g * powf(1 + powf(t, p), -h) with h = fl32(1 / (2 p)); else s = (A / sqrt(r)) * powf(1 + powf(t, -p), -h)
 *   -- the same curve from its saturated end, which holds for every finite r where t^p would overflow; y = u * s.  SALEH: am = aa /
 *   fma(ba, r, 1), phi = (ap * r) / fma(bp, r, 1), sincosf(phi), y = (u * am) times the phasor, one complex product.  POLY: q ascending;
 *   per delay G = c[q][K - 1], then G = fma(G, r, c[q][k]) for k = K - 2 .. 0, then y += G * u by fma (re: G.re u.re, then -G.im u.im;
 *   im: G.re u.im, then G.im u.re), starting from y = 0; where every coefficient has imaginary part 0 the products with it are left out.
 *   A sample is a pure function of its 1 (POLY: Q) input samples: a stream cut into calls at any point (each piece passing history =
 *   min(Q - 1, samples before it)), or written to an `out` of another alignment, gives the same bits.
 * A non-finite input sample spoils its own output sample (POLY: the Q outputs that read it) and nothing else.
 * sc16 twin: interleaved int16 q(y.re * gain), q(y.im * gain), the products in fp32, q the burst shaper's rule.
 * Error budget against the same formulas in float64 on the same complex64 inputs (u the exact product d * x there):
 *     CLIP, RAPP   |y - y64| <= 8 * 2^-23 * |y64|          SALEH   |y - y64| <= 16 * 2^-23 * |y64|  while |phi| <= pi
 *     POLY         |y - y64| <= (4 K + Q + 8) * 2^-23 * S_i,  S_i = sum_q sum_k |c[q][k]| |u[i - q]|^(2 k + 1)
 *   (RAPP: the outer root 1 / (2 p) cancels the p-fold amplification of t's error.  POLY: the roundings of Horner, of r, of the product
 *   and of the sum over q.)  Derived, not measured.
 * *_device: in and out are device arrays with the alignment of one element and no more (8 bytes, sc16 out 4 bytes); byte offsets are
 *   64-bit.  out overlapping [in - history, in + n) is GFDM_HIP_EINVAL for every kind: there is no in-place call.  No workspace, no
 *   allocation, no synchronisation: one kernel, hipGraph-capturable.  The stream is written in 16-byte stores aligned in memory whatever
 *   the alignment of out is, the first and last samples of an unaligned stream one by one; the memoryless kinds read 16 bytes a load
 *   where `in` is aligned under an output vector and 8 where it is not, POLY reads every input sample once per tile of 2048 output
 *   samples (plus the Q - 1 in front of the tile).  At most 2048 workgroups per launch, which stride over the tiles beyond.
 * *_host: a convenience, not a pipeline: uploads history + n samples, runs the device call, downloads n.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device), from create, set_drive and every call: kind
 *   outside the enum; n_params other than 1 / 3 / 4 / 0 for the kind; a param that is not finite in fp32; A <= 0, g <= 0, p outside
 *   0.5 .. 16, fl32(g^2 / A^2) zero or not finite, ba < 0, bp < 0; n_delays outside 1 .. 16 or n_orders outside 1 .. 5 (POLY), either non-zero (the others); a NULL or
 *   non-finite coefficient table (create); drive negative or not finite in fp32; a non-finite gain; n or history negative; n > 2^62; a
 *   byte size (8 (history + n)) that overflows int64.  Also: a NULL buffer that the call would touch.  n == 0 returns GFDM_HIP_OK
 *   without a launch.
 * Not here: AM/PM for Rapp, even orders and cross terms (the generalised memory polynomial), sc16 input, setters other than drive,
 *   digital predistortion, fusing into place or apply.
 * Tested range and measured shares of the budgets: tests/amplifier_model_ref.py, profiles/r23/amplifier_accuracy.json. */
typedef enum gfdm_hip_amplifier_kind {
    GFDM_HIP_AMPLIFIER_CLIP = 0,
    GFDM_HIP_AMPLIFIER_RAPP = 1,
    GFDM_HIP_AMPLIFIER_SALEH = 2,
    GFDM_HIP_AMPLIFIER_POLY = 3
} gfdm_hip_amplifier_kind;
typedef struct gfdm_hip_amplifier_model gfdm_hip_amplifier_model;
int gfdm_hip_amplifier_model_create(gfdm_hip_amplifier_model** out, int kind, const double* params, int n_params, const float* coefficients,
                                    int n_delays, int n_orders, double drive, int device);
int gfdm_hip_amplifier_model_destroy(gfdm_hip_amplifier_model* m);
int gfdm_hip_amplifier_model_kind(const gfdm_hip_amplifier_model* m);
int gfdm_hip_amplifier_model_n_params(const gfdm_hip_amplifier_model* m);
int gfdm_hip_amplifier_model_n_delays(const gfdm_hip_amplifier_model* m);
int gfdm_hip_amplifier_model_n_orders(const gfdm_hip_amplifier_model* m);
int gfdm_hip_amplifier_model_params(const gfdm_hip_amplifier_model* m, double* params);               /* n_params */
int gfdm_hip_amplifier_model_coefficients(const gfdm_hip_amplifier_model* m, float* coefficients);     /* 2 * n_delays * n_orders */
int gfdm_hip_amplifier_model_drive(const gfdm_hip_amplifier_model* m, double* drive);
int gfdm_hip_amplifier_model_set_drive(gfdm_hip_amplifier_model* m, double drive);
int gfdm_hip_amplifier_model_check(int kind, const double* params, int n_params, int n_delays, int n_orders, double drive, int64_t n,
                                   int64_t history, double gain);
int gfdm_hip_amplifier_model_apply_host(gfdm_hip_amplifier_model* m, float* out, const float* in, int64_t n, int64_t history);
int gfdm_hip_amplifier_model_apply_device(gfdm_hip_amplifier_model* m, void* out, const void* in, int64_t n, int64_t history, void* stream);
int gfdm_hip_amplifier_model_apply_sc16_host(gfdm_hip_amplifier_model* m, int16_t* out, const float* in, int64_t n, int64_t history, double gain);
int gfdm_hip_amplifier_model_apply_sc16_device(gfdm_hip_amplifier_model* m, void* out, const void* in, int64_t n, int64_t history, double gain,
                                               void* stream);

/* ---- gfdm_hip_link_meter: which burst a detection is, bit errors and error-vector power per row, counters on the device ------------
 * Behind the receivers and beside the symbol mapper's decode: what a BER or EVM curve point needs so that it is one fixed-shape,
 * hipGraph-capturable sequence of launches with one 96-byte read at the end.  Rows are bursts or frames as for the symbol mapper.
 * create takes the constellation and the decision exactly as gfdm_hip_symbol_mapper_create does (same EINVAL table, same resolution
 *   of AUTO); bits_per_symbol, n_points, decision and row_bytes are the mapper's.  The decisions of measure are those of the mapper's
 *   decode for the same points and rule, from the same device function: an error counted here is an error in decode's bytes.
 * totals: the handle owns int64[12] on the device, zero at create:
 *     0 rows  1 symbols  2 bits  3 bit_errors  4 symbol_errors  5 row_errors (rows with at least one bit error)
 *     6 detections  7 matched  8 missed  9 false_alarms  10, 11 reserved (stay 0)
 *   totals_device returns its device pointer; reset enqueues its zeroing on `stream` (one kernel, capturable); totals synchronises
 *   `stream` and copies the 96 bytes to the host.  Every match and measure ADDS to totals with 64-bit integer atomics: exact, and
 *   independent of arrival order.  Calls that add to one handle's totals are ordered by the caller's streams: the *_host flavours run
 *   on the handle's own stream, so a reset or *_device call on another stream must have completed before one of them is made.
 * match: frame_start int64[n_rows] and the optional count as detect writes them (n_live = clamp(*count, 0, n_rows)); sent_pos
 *   int64[n_sent], ascending; e_j = sent_pos[j] + offset (offset: e.g. the preamble's cyclic prefix where sent_pos are place's starts);
 *   tol >= 0.  Row d is a DETECTION when d < n_live and frame_start[d] >= 0.  A detection d PROPOSES the j that minimises
 *   |frame_start[d] - e_j|, the lower j on a tie, if that distance is <= tol.  Among the detections that propose j the one with the
 *   smallest (distance, d) in lexicographic order WINS.  Outputs, each optional: ref_row int64[n_rows] = j for a winner, -1 for every
 *   other row (rows from n_live on included; their input is never read); sent_row int64[n_sent] = the winner d, or -1.  totals:
 *   detections += detections, matched += winners, missed += n_sent - winners, false_alarms += detections - winners.  The rule is
 *   symmetric and order-free; frame_start need not be ascending.  n_sent == 0: every detection is a false alarm; n_rows == 0: every
 *   sent burst is missed.  A sent_pos that is not ascending gives unspecified matches and no access outside the arrays.
 *   workspace: match_workspace_bytes(n_sent) bytes (one 64-bit key per sent burst), 8-byte aligned.  At most three small kernels.
 *   GFDM_HIP_EINVAL: tol < 0 or >= 2^31; n_rows or n_sent negative or >= 2^31; a NULL buffer the call would touch.
 * measure: symbols complex64 [n_rows][n_sym]; payload optional uint8 [n_ref][row_bytes], packed as the symbol mapper says (the spare
 *   low bits of a row's last byte are ignored); ref_row optional int64[n_rows], NULL = the identity; count optional.
 *   Row r is MEASURED when r < n_live and ref(r) >= 0 -- and, with a payload, ref(r) < n_ref.  For a measured row and symbol i:
 *     idx_i  the mapper's decision of x_i under the handle's rule (NaN -> 0, as there);
 *     data-aided (payload given):   s_i = the sent index in the payload bits of row ref(r), p_i = points[s_i];
 *     decision-directed (payload NULL): p_i = points[idx_i]; bit_errors must be NULL (EINVAL otherwise).
 *   Outputs, each optional, one element per row:        measured row                       unmeasured row
 *     bit_errors int32                                  sum_i popcount(idx_i XOR s_i)      -1
 *     err_power  float32                                sum_i |x_i - p_i|^2                 0
 *     ref_power  float32                                sum_i |p_i|^2                       0
 *   EVM rms of a measured row is sqrt(err_power / ref_power); err_power / n_sym of a decision-directed call is the noise estimate the
 *   mapper's soft() takes as scale = n_sym / err_power.  The symbols of an unmeasured row are never read.  Every output element is
 *   written exactly once by the call's own kernels whatever count and ref_row are: no memset in front, so a graph replay with a changed
 *   count or ref_row is correct.  totals, data-aided: rows, symbols, bits (= symbols * k), bit_errors, symbol_errors (idx_i != s_i),
 *   row_errors; decision-directed: rows and symbols only.
 *   Arithmetic: |x - p|^2 is the mapper's direct form d_i in fp32, |p|^2 = re^2 + im^2 in fp32.  The flat symbol array is cut into tiles
 *   of 2048 symbols; inside a tile a row's terms are summed in fp32 in a fixed order (up to 8 in sequence in a lane, then a tree over
 *   the 256 lanes); the parts of a row that crosses tile boundaries are summed in fp64 in ascending tile order and rounded to fp32
 *   once.  No float atomics: two calls on the same inputs give bit-equal outputs, and the result does not depend on the alignment of
 *   the buffers.  A non-finite symbol makes err_power of ITS row non-finite and touches no other row (ref_power is a sum over points and
 *   stays finite); the integer outputs and totals are never affected.
 *   Error budget against the same formulas in float64 on the same float32 inputs, for both powers: |got - ref| <= 2^-19 * ref.  All
 *   terms are non-negative, so every rounding is a relative error of at most 2^-24 of the running sum: four roundings per term (two
 *   differences, a product, a fused or unfused sum), at most 8 lane-sequential additions, 6 levels of the wave's scan + at most 3 joins
 *   of wave totals + 1 join of the carry, the fp64 sum across tiles (below 2^-40 for any row that fits in memory) and the final
 *   rounding: 4 + 8 + 10 + 1 = 23 roundings < 32 = 2^-19 / 2^-24.  Derived, not measured.
 *   workspace: measure_workspace_bytes(n_sym, n_rows) bytes, 16-byte aligned; its content need not survive between calls.  Two kernels:
 *   the tiles, then one lane per tile boundary for the rows that cross one.  No kernel waits for another workgroup.
 *   GFDM_HIP_EINVAL: the symbol mapper's table; n_sym * k > 2^31 - 1 (the per-row count is an int32); n_ref < 0; bit_errors without a
 *   payload; a NULL buffer the call would touch.  n_rows == 0 returns GFDM_HIP_OK without a launch.
 * *_device: every array is a device array with the alignment of one element and no more (symbols 8 bytes, payload 1, int32 / float32
 *   outputs 4, int64 arrays 8); byte offsets are 64-bit.  The calls neither allocate nor synchronise and are hipGraph-capturable; the
 *   grid of measure depends on the total size, never on n_rows.
 * *_host: a convenience, not a pipeline: upload, the device call on the handle's stream, download.
 * Tested range (against the mapper's decode on the same device tensor, exactly, and a numpy restatement of the above in float64):
 *   k = 1, 2, 3, 4, 6, 8; n_sym 1, 3, 5, 7, 8, 63, 64, 65, 257, 468, 4097 (more than two tiles of 2048); 1, 7, 5000 (of 3 symbols) and
 *   32768 + 7 (of 5 symbols) rows per call; ref_row permuted, repeated, -1 and beyond n_ref; count below, at and beyond n_rows; buffers
 *   at every alignment of one element; match on known answers and on 320 detections against 300 sent bursts.  Worst measured share of
 *   the 2^-19 budget over all of these: 0.11. */
typedef struct gfdm_hip_link_meter gfdm_hip_link_meter;
int gfdm_hip_link_meter_create(gfdm_hip_link_meter** out, const float* points, int n_points, int decision, int device);
int gfdm_hip_link_meter_destroy(gfdm_hip_link_meter* m);
int gfdm_hip_link_meter_bits_per_symbol(const gfdm_hip_link_meter* m);
int gfdm_hip_link_meter_n_points(const gfdm_hip_link_meter* m);
int gfdm_hip_link_meter_decision(const gfdm_hip_link_meter* m);
int64_t gfdm_hip_link_meter_row_bytes(const gfdm_hip_link_meter* m, int64_t n_sym);
void* gfdm_hip_link_meter_totals_device(gfdm_hip_link_meter* m);                             /* int64[12] on the device */
int gfdm_hip_link_meter_reset(gfdm_hip_link_meter* m, void* stream);
int gfdm_hip_link_meter_totals(gfdm_hip_link_meter* m, int64_t* out, void* stream);          /* out: int64[12] on the host */
int64_t gfdm_hip_link_meter_match_workspace_bytes(int64_t n_sent);
int64_t gfdm_hip_link_meter_measure_workspace_bytes(int64_t n_sym, int64_t n_rows);
int gfdm_hip_link_meter_match_host(gfdm_hip_link_meter* m, int64_t* ref_row, int64_t* sent_row, const int64_t* frame_start, const int64_t* count,
                                   int64_t n_rows, const int64_t* sent_pos, int64_t n_sent, int64_t offset, int64_t tol);
int gfdm_hip_link_meter_match_device(gfdm_hip_link_meter* m, void* ref_row, void* sent_row, const void* frame_start, const void* count, int64_t n_rows,
                                     const void* sent_pos, int64_t n_sent, int64_t offset, int64_t tol, void* workspace, void* stream);
int gfdm_hip_link_meter_measure_host(gfdm_hip_link_meter* m, int32_t* bit_errors, float* err_power, float* ref_power, const float* symbols,
                                     const uint8_t* payload, int64_t n_ref, const int64_t* ref_row, const int64_t* count, int64_t n_sym, int64_t n_rows);
int gfdm_hip_link_meter_measure_device(gfdm_hip_link_meter* m, void* bit_errors, void* err_power, void* ref_power, const void* symbols,
                                       const void* payload, int64_t n_ref, const void* ref_row, const void* count, int64_t n_sym, int64_t n_rows,
                                       void* workspace, void* stream);

/* ---- gfdm_hip_conv_code: convolutional code, encode and soft- / hard-input Viterbi decode ------------------------------------------
 * The forward error correction pair of the chain: encode in front of gfdm_hip_symbol_mapper_map, decode behind ..._soft (decode_hard
 * behind ..._decode).  Constraint length 7, rate 1/2 and nothing else; the default generators are 171 / 133 octal, GNU Radio's
 * fec.cc_encoder / cc_decoder default polys = [109, 79].  GNU Radio is not part of this project's test bed: the code is DEFINED by the
 * formulas below, and bit-compatibility with GNU Radio's blocks is unpinned.  All arithmetic is integer, so every result is exact.
 * Encoder: g0, g1 are the generators, 1 <= |g_i| <= 127; a negative g_i complements that output (Karn's convention).  With u_t the
 *   input bits, t = 0 .. T-1, u_t = 0 for t < 0 and for the tail:
 *     R_t = sum_{d=0..6} u_{t-d} << d                    (the newest bit is bit 0)
 *     c_{t,i} = parity(R_t & |g_i|) XOR (g_i < 0)
 *   and the coded row is c_{0,0} c_{0,1} c_{1,0} c_{1,1} ...: coded_bits = 2 T.
 * Modes: GFDM_HIP_CC_TERMINATED: six zero bits follow the n_info information bits, T = steps = n_info + 6, the trellis ends in state 0.
 *   GFDM_HIP_CC_TRUNCATED: T = n_info, the final state is free.  T <= 2^20.
 * Packing is the symbol mapper's: MSB first, every row starts on a byte.  An information row is info_bytes = ceil(n_info / 8) bytes; the
 *   spare low bits of its last byte are ignored by encode and written as 0 by decode.  A coded row is coded_bytes = ceil(2 T / 8) bytes.
 * encode: bytes [n_rows][info_bytes] -> bytes [n_rows][out_row_bytes], out_row_bytes >= coded_bytes; everything behind the 2 T coded bits
 *   of a row is written as 0, so a row may have the width gfdm_hip_symbol_mapper_row_bytes(n_sym) and go straight into map.
 * decode: float32 LLRs [n_rows][llr_stride], llr_stride >= coded_bits (the floats behind the coded bits are never read: soft's
 *   [n_rows][n_sym k] goes in as it is) -> bytes [n_rows][info_bytes] and, where path_metric is not NULL, int32 [n_rows].
 *   Soft value of a coded bit: q = clamp(rintf(llr * gain), -127, 127) -- one fp32 product, rintf rounds half to even, NaN gives 0, +-inf
 *   gives +-127; positive means bit 0 (soft's sign); gain is a finite float > 0.  decode_hard reads a packed coded row
 *   [n_rows][in_row_bytes], in_row_bytes >= coded_bytes (encode's output, gfdm_hip_symbol_mapper_decode's bytes): q = +1 for a 0 bit, -1
 *   for a 1 bit.
 *   Path metrics are int32: PM_{-1}[0] = 0, PM_{-1}[s] = -(1 << 30) for s != 0.  At step t state s has the predecessors
 *   p_b = (s >> 1) + 32 b, b in {0, 1}, over the register value R = s | (b << 6):
 *     m_b = PM_{t-1}[p_b] + sum_i (1 - 2 c_i(R)) q_{t,i},     d_t[s] = (m_1 > m_0)  (strict: a tie keeps b = 0),     PM_t[s] = max(m_0, m_1).
 *   No normalisation: 2^20 * 254 < 2^30 - 2^28 keeps every metric inside int32.
 *   Traceback: start state s = 0 (terminated) or the first state of maximal PM_{T-1} (truncated); for t = T-1 .. 0: u_t = s & 1, then
 *   s = (s >> 1) | (d_t[s] << 5).  The output is u_0 .. u_{n_info-1}; path_metric is PM_{T-1} at the start state.  An all-zero row of
 *   LLRs (erasures) therefore decodes to zero bits with metric 0.
 * Workspace: the survivor decisions of a row are 8 T bytes.  Rows of at most GFDM_HIP_CC_LDS_STEPS steps keep them in LDS and
 *   decode_workspace_bytes is 0 (workspace may be NULL); longer rows need decode_workspace_bytes(c, n_info, n_rows) bytes of device
 *   memory, 16-byte aligned, whose content is not preserved between calls.  It grows with n_rows only up to the 2048 rows a launch
 *   keeps in flight.
 * count, *_device, *_host: as for gfdm_hip_symbol_mapper.  Rows from n_live = clamp(*count, 0, n_rows) on are written as zeros
 *   (path_metric 0) and their input is never read; every output element is written exactly once by the one kernel of the call, with
 *   no memset in front, so a graph replay with a changed count is correct.  The device flavours neither allocate nor synchronise and
 *   are hipGraph-capturable.  Buffers need the alignment of one element and no more: 1 byte for bytes, 4 bytes for LLRs and
 *   path_metric (8 for count); byte offsets are 64-bit.  The host flavours upload, run the device call with a workspace of their own,
 *   and download: a convenience, not a pipeline.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device) and from every call: a generator of 0 or with
 *   |g| > 127; an unknown mode; n_info < 1; T > 2^20; n_rows < 0; byte sizes that overflow int64.  From the calls also: a stride or row
 *   width below the minimum; gain non-finite or <= 0; a NULL buffer the call would touch (the workspace where one is needed).
 *   n_rows == 0 returns GFDM_HIP_OK without a launch.  The size getters return int64, negative values are status codes; poly returns
 *   0 for a bad handle or index.
 * Not here: tail-biting and streaming modes, other constraint lengths or mother-code rates, int8 LLR input.  Puncturing (rates above
 *   1/2: a depunctured position is an LLR of 0) and interleaving are gfdm_hip_rate_matcher's, below.
 * Tested range (bit for bit, path_metric included, against the numpy restatement of the above in tests/conv_code_ref.py): both modes;
 *   n_info 1, 2, 5, 6, 7, 8, 57, 58, 59, 122, 456, the last three that keep T <= GFDM_HIP_CC_LDS_STEPS and the two after, one row of
 *   2^16 + 3; 1, 3, 4, 5, 7, 5000 (n_info 3) and 32768 + 7 (n_info 2) rows per call; polys (109, 79), (109, -79), (91, 121), (55, 79);
 *   saturating, half-way, NaN, infinite and all-zero LLRs; llr_stride coded_bits + 0, 1, 12; buffers at every alignment of one
 *   element; count below, at and beyond n_rows. */
typedef enum gfdm_hip_cc_mode {
    GFDM_HIP_CC_TERMINATED = 0,
    GFDM_HIP_CC_TRUNCATED = 1
} gfdm_hip_cc_mode;
#define GFDM_HIP_CC_LDS_STEPS 2048 /* rows of up to this many trellis steps keep their decisions in LDS (16 KiB per row) */
typedef struct gfdm_hip_conv_code gfdm_hip_conv_code;
int gfdm_hip_conv_code_create(gfdm_hip_conv_code** out, int poly0, int poly1, int mode, int device);
int gfdm_hip_conv_code_destroy(gfdm_hip_conv_code* c);
int gfdm_hip_conv_code_poly(const gfdm_hip_conv_code* c, int i);
int gfdm_hip_conv_code_mode(const gfdm_hip_conv_code* c);
int64_t gfdm_hip_conv_code_steps(const gfdm_hip_conv_code* c, int64_t n_info);
int64_t gfdm_hip_conv_code_coded_bits(const gfdm_hip_conv_code* c, int64_t n_info);
int64_t gfdm_hip_conv_code_coded_bytes(const gfdm_hip_conv_code* c, int64_t n_info);
int64_t gfdm_hip_conv_code_info_bytes(const gfdm_hip_conv_code* c, int64_t n_info);
int64_t gfdm_hip_conv_code_decode_workspace_bytes(const gfdm_hip_conv_code* c, int64_t n_info, int64_t n_rows);
int gfdm_hip_conv_code_check(int poly0, int poly1, int mode, int64_t n_info, int64_t n_rows);
int gfdm_hip_conv_code_encode_host(gfdm_hip_conv_code* c, uint8_t* out, const uint8_t* data, const int64_t* count, int64_t n_info,
                                   int64_t out_row_bytes, int64_t n_rows);
int gfdm_hip_conv_code_encode_device(gfdm_hip_conv_code* c, void* out, const void* data, const void* count, int64_t n_info, int64_t out_row_bytes,
                                     int64_t n_rows, void* stream);
int gfdm_hip_conv_code_decode_host(gfdm_hip_conv_code* c, uint8_t* out, int32_t* path_metric, const float* llr, const int64_t* count, int64_t n_info,
                                   int64_t llr_stride, float gain, int64_t n_rows);
int gfdm_hip_conv_code_decode_device(gfdm_hip_conv_code* c, void* out, void* path_metric, const void* llr, const void* count, int64_t n_info,
                                     int64_t llr_stride, float gain, int64_t n_rows, void* workspace, void* stream);
int gfdm_hip_conv_code_decode_hard_host(gfdm_hip_conv_code* c, uint8_t* out, int32_t* path_metric, const uint8_t* coded, const int64_t* count,
                                        int64_t n_info, int64_t in_row_bytes, int64_t n_rows);
int gfdm_hip_conv_code_decode_hard_device(gfdm_hip_conv_code* c, void* out, void* path_metric, const void* coded, const void* count, int64_t n_info,
                                          int64_t in_row_bytes, int64_t n_rows, void* workspace, void* stream);

/* ---- gfdm_hip_rate_matcher: puncture and interleave coded bits, depuncture and deinterleave LLRs --------------------------------------
 * Between gfdm_hip_conv_code_encode and gfdm_hip_symbol_mapper_map on the transmit side (match), between ..._soft and
 * gfdm_hip_conv_code_decode (unmatch), or between ..._symbol_mapper_decode and ..._conv_code_decode (unmatch_hard), on the receive side.
 * Everything is integer index arithmetic, so every result is exact.  With c_0 .. c_{n_coded-1} the bits of a mother-code row
 * (n_coded = gfdm_hip_conv_code_coded_bits; 1 <= n_coded <= 2^21, the code's T <= 2^20):
 *   Puncturing: keep[0 .. period-1] is a pattern of bytes, 1 <= period <= 4096; bit i of the coded row is transmitted iff
 *     keep[i mod period] != 0.  The kept positions in ascending order are k_0 < ... < k_{n_tx-1}; n_tx >= 1 is required
 *     (tx_bits_of gives n_tx without a handle).  The punctured sequence is p_a = c[k_a].
 *   Interleaving: perm[0 .. n_tx-1] is a permutation of 0 .. n_tx-1, NULL for the identity (n_perm is then ignored).  The gather
 *     convention: transmitted bit j is t_j = p[perm[j]] = c[src[j]] with src[j] = k_{perm[j]}.
 *   create composes both on the host into src (n_tx entries; source_index copies it out) and its inverse inv (n_coded entries, -1 at
 *   the punctured positions) and keeps the two tables on the device.  A handle serves one (n_coded, keep, perm).
 *   The patterns in use for the 171 / 133 code over c_{0,0} c_{0,1} c_{1,0} c_{1,1} ... are [1,1] (rate 1/2), [1,1,1,0] (2/3),
 *   [1,1,1,0,0,1] (3/4) and [1,1,1,0,0,1,1,0,0,1] (5/6): those of IEEE 802.11a.  That standard is not part of this project's test
 *   bed; bit-compatibility with it is unpinned.
 * Packing is the symbol mapper's: MSB first, every row starts on a byte.  tx_bytes = ceil(n_tx / 8).
 * match: coded bytes [n_rows][in_row_bytes], in_row_bytes >= ceil(n_coded / 8) (encode's output at any width; what lies behind the
 *   n_coded bits of a row is never looked at) -> transmitted bytes [n_rows][out_row_bytes], out_row_bytes >= tx_bytes.  Everything behind
 *   the n_tx bits of a row is written as 0, so a row may have the width gfdm_hip_symbol_mapper_row_bytes(n_sym) and go straight into map.
 * unmatch: float32 LLRs [n_rows][in_stride], in_stride >= n_tx (the floats behind n_tx are never read: soft's rows go in as they are)
 *   -> float32 [n_rows][out_stride], out_stride >= n_coded: out[i] = in[inv[i]] as a BIT copy (NaN payloads and the sign of zero are
 *   preserved), +0.0f where inv[i] < 0 and in the floats behind n_coded.  The output is what gfdm_hip_conv_code_decode takes, with
 *   llr_stride = out_stride.
 * unmatch_hard: transmitted bytes [n_rows][in_row_bytes], in_row_bytes >= tx_bytes (gfdm_hip_symbol_mapper_decode's output) -> float32
 *   rows laid out as unmatch's: +1.0f for a 0 bit, -1.0f for a 1 bit, +0.0f at the punctured positions and behind n_coded.  Fed to
 *   gfdm_hip_conv_code_decode with gain 1 this is q = +1 / -1 / 0: decode_hard's metric with erasures, which decode_hard cannot express.
 * count, *_device, *_host: as for gfdm_hip_conv_code.  Rows from n_live = clamp(*count, 0, n_rows) on are written as zeros and their
 *   input is never read; every output element is written exactly once by the one kernel of the call, with no memset in front, so a
 *   graph replay with a changed count is correct.  The device flavours neither allocate nor synchronise and are hipGraph-capturable.
 *   Buffers need the alignment of one element and no more: 1 byte for bytes, 4 bytes for floats (8 for count); byte offsets are 64-bit.
 *   The host flavours upload, run the device call and download: a convenience, not a pipeline.
 * Rows of at most GFDM_HIP_RM_LDS_BITS coded bits have their table copied into LDS once per workgroup; longer rows read it through the
 *   cache.  The results are the same.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device), from create (before any device is touched) and
 *   where it applies from tx_bits_of: n_coded < 1 or > 2^21; period < 1 or > 4096; a NULL keep; a pattern that keeps no bit within
 *   n_coded; with a perm, n_perm != n_tx or a perm that is not a permutation of 0 .. n_tx-1; n_rows < 0; byte sizes that overflow int64.
 *   From the calls: a NULL handle; n_rows < 0; a width or stride below the minimum; byte sizes that overflow int64; a NULL buffer the
 *   call would touch.  n_rows == 0 returns GFDM_HIP_OK without a launch.  The size getters return int64, negative values are status
 *   codes.
 * Not here: fusing unmatch into decode's LLR fetch (it would change the decode kernel; profiles/r17/rate_matcher_kernel_durations.txt
 *   is the measurement to decide it by), per-row patterns, repetition (rates below 1/2).
 * Tested range (bit for bit against the numpy restatement of the above in tests/rate_match_ref.py): n_coded 1, 2, 7, 8, 9, 15, 16, 17,
 *   63, 64, 65, 127, 128, 129, 924, 1388, GFDM_HIP_RM_LDS_BITS + 0, 1, 2, one row of 2^17 + 6; the patterns all ones, the four rates
 *   above, [0,1], the period-7 pattern [1,0,1,1,0,1,1], a period above n_coded, one kept bit; perm identity, reversal, block
 *   interleavers of 18 and n_tx columns, a random permutation; 1, 3, 4, 5, 7, 5000 (n_coded 6) and 32768 + 7 (n_coded 4) rows per
 *   call; widths and strides of the minimum + 0, 1, 12; buffers at every alignment of one element; NaN payloads, infinities, -0.0 and
 *   denormals; count below, at and beyond n_rows. */
#define GFDM_HIP_RM_LDS_BITS 8192 /* rows of up to this many coded bits keep their index table in LDS (32 KiB per workgroup) */
typedef struct gfdm_hip_rate_matcher gfdm_hip_rate_matcher;
int gfdm_hip_rate_matcher_create(gfdm_hip_rate_matcher** out, int64_t n_coded, const uint8_t* keep, int period, const int32_t* perm, int64_t n_perm,
                                 int device);
int gfdm_hip_rate_matcher_destroy(gfdm_hip_rate_matcher* r);
int64_t gfdm_hip_rate_matcher_coded_bits(const gfdm_hip_rate_matcher* r);
int64_t gfdm_hip_rate_matcher_tx_bits(const gfdm_hip_rate_matcher* r);
int64_t gfdm_hip_rate_matcher_tx_bytes(const gfdm_hip_rate_matcher* r);
int gfdm_hip_rate_matcher_source_index(const gfdm_hip_rate_matcher* r, int32_t* src);
int64_t gfdm_hip_rate_matcher_tx_bits_of(int64_t n_coded, const uint8_t* keep, int period);
int gfdm_hip_rate_matcher_check(int64_t n_coded, const uint8_t* keep, int period, const int32_t* perm, int64_t n_perm, int64_t n_rows);
int gfdm_hip_rate_matcher_match_host(gfdm_hip_rate_matcher* r, uint8_t* out, const uint8_t* coded, const int64_t* count, int64_t in_row_bytes,
                                     int64_t out_row_bytes, int64_t n_rows);
int gfdm_hip_rate_matcher_match_device(gfdm_hip_rate_matcher* r, void* out, const void* coded, const void* count, int64_t in_row_bytes,
                                       int64_t out_row_bytes, int64_t n_rows, void* stream);
int gfdm_hip_rate_matcher_unmatch_host(gfdm_hip_rate_matcher* r, float* out, const float* llr, const int64_t* count, int64_t in_stride,
                                       int64_t out_stride, int64_t n_rows);
int gfdm_hip_rate_matcher_unmatch_device(gfdm_hip_rate_matcher* r, void* out, const void* llr, const void* count, int64_t in_stride,
                                         int64_t out_stride, int64_t n_rows, void* stream);
int gfdm_hip_rate_matcher_unmatch_hard_host(gfdm_hip_rate_matcher* r, float* out, const uint8_t* tx, const int64_t* count, int64_t in_row_bytes,
                                            int64_t out_stride, int64_t n_rows);
int gfdm_hip_rate_matcher_unmatch_hard_device(gfdm_hip_rate_matcher* r, void* out, const void* tx, const void* count, int64_t in_row_bytes,
                                              int64_t out_stride, int64_t n_rows, void* stream);

/* ---- gfdm_hip_frame_check: CRC-32 and whitening of payload rows, attach before the code and verify behind it --------------------------
 * The two ends of the chain: attach in front of gfdm_hip_conv_code_encode, verify behind gfdm_hip_conv_code_decode -- the receiver's
 * verdict on a row (keep or drop) without the payload that was sent.  GNU Radio's digital.crc32_bb / crc_append / crc_check and
 * digital.additive_scrambler_bb do the same work; GNU Radio is not part of this project's test bed: the pair is DEFINED by the formulas
 * below, and bit-compatibility with GNU Radio's blocks is unpinned.  All arithmetic is integer, so every result is exact.
 * Frame: a payload row is n_payload bytes, 1 <= n_payload <= 2^17 - 4.  A frame row is frame_bytes = n_payload + 4 bytes: the payload,
 *   then the CRC, least significant byte first.  frame_bits = 8 frame_bytes is what goes into gfdm_hip_conv_code_encode as n_info; 2^17
 *   bytes keeps it at the code's T <= 2^20.
 * CRC: CRC-32 of IEEE 802.3, by the bitwise formula: r = 0xFFFFFFFF; for every byte b of the payload, in order: r ^= b, then eight times
 *   r = (r >> 1) ^ (r & 1 ? 0xEDB88320 : 0); the CRC is r ^ 0xFFFFFFFF.  This is zlib's crc32; its value for "123456789" is 0xCBF43926.
 * Whitening: an additive sequence from a Fibonacci LFSR.  degree d is 0 (no whitening; mask and seed are ignored) or 1 .. 32, with
 *   1 <= mask < 2^d and 1 <= seed < 2^d.  s_0 = seed; whitening bit w_i = s_i & 1; s_{i+1} = (s_i >> 1) | (parity(s_i & mask) << (d - 1)),
 *   so w_{i+d} = XOR over the set bits j of mask of w_{i+j}; d = 7, mask = 0x11 is x^7 + x^4 + 1.  Bit i of the sequence is XORed onto
 *   bit i of the frame row in the symbol mapper's order (MSB first), over all frame_bits, CRC included; every row starts at s_0.  create
 *   computes the packed sequence (frame_bytes bytes) on the host and keeps it on the device; whitening copies it out.
 * attach: payload bytes [n_rows][in_row_bytes], in_row_bytes >= n_payload (the bytes behind the payload are never read) -> frame bytes
 *   [n_rows][out_row_bytes], out_row_bytes >= frame_bytes: the payload, then the CRC of the unwhitened payload, the whitening over both,
 *   and zeros behind frame_bytes.
 * verify: frame bytes [n_rows][in_row_bytes], in_row_bytes >= frame_bytes (decode's output at n_info = frame_bits, as it is) ->
 *   payload [n_rows][out_row_bytes], out_row_bytes >= n_payload: the dewhitened payload of every live row, good or not, and zeros
 *   behind it; ok uint8 [n_rows]: 1 where the CRC of the dewhitened payload equals the dewhitened four bytes behind it, else 0;
 *   good_row int64 [n_rows]: the indices of the rows with ok = 1 in ascending order, then -1; n_good: one int64.  payload may be NULL
 *   (check only; out_row_bytes is then ignored); good_row and n_good may both be NULL.  verify never looks at anything but the frame.
 * count, *_device, *_host: as for gfdm_hip_rate_matcher.  Rows from n_live = clamp(*count, 0, n_rows) on are written as zeros (ok 0,
 *   not in good_row) and their input is never read; every output element is written exactly once per call with no memset in front, so
 *   a graph replay with a changed count is correct.  A call is one kernel, and a second, small one where good_row is asked for; no
 *   workspace.  The device flavours neither allocate nor synchronise and are hipGraph-capturable.  Buffers need the alignment of one
 *   element and no more: 1 byte for bytes, 8 bytes for good_row, n_good and count; byte offsets are 64-bit.  The host flavours upload,
 *   run the device call and download: a convenience, not a pipeline.
 * GFDM_HIP_EINVAL from check (the argument table alone, without a handle or a device), from create (before any device is touched) and
 *   from every call: n_payload out of range; degree outside 0 .. 32; a mask or seed of 0 or >= 2^d when d > 0; n_rows < 0; byte sizes
 *   that overflow int64.  From the calls also: a NULL handle; a width below the minimum; a NULL buffer the call would touch; exactly
 *   one of good_row / n_good.  n_rows == 0 returns GFDM_HIP_OK without a launch.  The size getters return int64, negative values are
 *   status codes.
 * Not here: a per-row seed (802.11's random scrambler initialisation); other CRC polynomials or widths; moving the good rows' payloads
 *   to the front (good_row is the index list such a gather would take); fusing verify into decode's traceback.
 * Tested range (bit for bit against the numpy restatement of the above in tests/frame_check_ref.py): n_payload 1, 2, 11, 12, 13, 27, 28,
 *   29, 57, 60, 61, 124, 1019, 1020, 1021, 1024, 2044, 2045 and one row of 2^17 - 4; 1, 3, 4, 5, 7, 63, 64, 65 rows per call at every
 *   group size, 5000, 32768 + 7, 65536 + 5 and 2^20 + 4101 short rows, 8197 rows of 1025 bytes; widths of the minimum + 0, 1, 12; buffers
 *   at every byte alignment; whitening off, (7, 0x11, 0x7F) and a degree-32 mask; single-bit errors in the payload, the CRC and the last
 *   byte, all rows good, no row good; count below, at and beyond n_rows; decode -> verify in a captured graph. */
typedef struct gfdm_hip_frame_check gfdm_hip_frame_check;
int gfdm_hip_frame_check_create(gfdm_hip_frame_check** out, int64_t n_payload, uint64_t mask, uint64_t seed, int degree, int device);
int gfdm_hip_frame_check_destroy(gfdm_hip_frame_check* c);
int64_t gfdm_hip_frame_check_payload_bytes(const gfdm_hip_frame_check* c);
int64_t gfdm_hip_frame_check_frame_bytes(const gfdm_hip_frame_check* c);
int64_t gfdm_hip_frame_check_frame_bits(const gfdm_hip_frame_check* c);
int gfdm_hip_frame_check_whitening(const gfdm_hip_frame_check* c, uint8_t* seq);
int gfdm_hip_frame_check_check(int64_t n_payload, uint64_t mask, uint64_t seed, int degree, int64_t n_rows);
int gfdm_hip_frame_check_attach_host(gfdm_hip_frame_check* c, uint8_t* out, const uint8_t* payload, const int64_t* count, int64_t in_row_bytes,
                                     int64_t out_row_bytes, int64_t n_rows);
int gfdm_hip_frame_check_attach_device(gfdm_hip_frame_check* c, void* out, const void* payload, const void* count, int64_t in_row_bytes,
                                       int64_t out_row_bytes, int64_t n_rows, void* stream);
int gfdm_hip_frame_check_verify_host(gfdm_hip_frame_check* c, uint8_t* payload, uint8_t* ok, int64_t* good_row, int64_t* n_good, const uint8_t* frames,
                                     const int64_t* count, int64_t in_row_bytes, int64_t out_row_bytes, int64_t n_rows);
int gfdm_hip_frame_check_verify_device(gfdm_hip_frame_check* c, void* payload, void* ok, void* good_row, void* n_good, const void* frames,
                                       const void* count, int64_t in_row_bytes, int64_t out_row_bytes, int64_t n_rows, void* stream);

/* ---- gfdm_hip_spectrum_meter: Welch PSD and power statistics (PAPR, CCDF) of a stream or of the bursts of a capture ------------------
 * The third meter beside the shaper's peak and the link meter: what the waveform looks like on the air.  Two independent accumulators
 * in totals that stay on the device; a curve point is a fixed-shape, hipGraph-capturable sequence of launches and one read at the end.
 * create: window real float32[nfft], fixed at create (no setter, neither for the hop); nfft = 2^a, 4 <= a <= 12; 1 <= hop <= nfft.
 *   GFDM_HIP_EINVAL: any other nfft or hop; a NULL window; a window value that is not finite.  Getters: nfft, hop, window (bit for bit).
 * totals: the handle owns, on the device, zero at create, contiguous in this order (totals_bytes() = 8 (8 + 1 + nfft + 512) bytes):
 *     head      int64[8]      0 segments  1 bad_segments  2 samples  3 bad_samples  4 peak_bits  5 .. 7 reserved (stay 0)
 *     power_sum float64       sum of the counted sample powers
 *     psd_sum   float64[nfft] FFT order, DC at 0
 *     hist      int64[512]    power histogram
 *   totals_device returns the pointer; reset enqueues the zeroing on `stream` (one kernel, capturable); read synchronises `stream` and
 *   copies the parts out (any of the four outputs may be NULL).  Calls that add to one handle's totals -- and they share the handle's
 *   partial rows -- are ordered by the caller's streams: the *_host flavours run on the handle's own stream, so a reset or *_device
 *   call on another stream must have completed before one of them is made, and two calls on one handle never run concurrently.
 * PSD accumulator (accumulate, accumulate_at): segment s of accumulate is in[s hop .. s hop + nfft), n_seg = n < nfft ? 0 :
 *   (n - nfft) / hop + 1.  plan(nfft, hop, n, &n_seg, &advance) gives n_seg and advance = n_seg hop, host arithmetic: the next call of a
 *   cut stream starts at in + advance.  n_seg == 0 returns GFDM_HIP_OK without a launch.  Per segment
 *       X_s[k] = sum_n x[n] w[n] exp(-2 pi j n k / nfft),   psd_sum[k] += |X_s[k]|^2
 *   The product x w, the transform and |X|^2 are fp32; the sum over the segments is fp64: a workgroup owns a contiguous run of segments and
 *   keeps its bins in fp64 registers, the at most 1024 workgroups write one partial row each, and a second kernel adds the rows in ascending
 *   order into psd_sum and bumps the counters.  The order is a function of (n_seg, nfft) alone -- not of the alignment of `in`, not of
 *   arrival: no float atomics, two calls on the same input give bit-equal totals.  The handle owns the 1024 x nfft partials (no workspace).
 *   A segment that holds a non-finite sample, or a sample whose fp32 product with its window value is not finite (an overflow), adds
 *   nothing to psd_sum and counts in bad_segments, not in segments: psd_sum stays finite whatever the input; every other segment
 *   counts in segments.  sc16: one 4-byte load per sample, widened unscaled; bit-equal to the complex64 call on the widened capture.
 *   accumulate_at: the dual of place / find_frame_start_at.  starts int64[n_bursts] and the optional count are device arrays exactly as
 *   detect writes them (host arrays in the *_host flavour); segment (b, j), j < seg_per_burst, starts at o = starts[b] + first + j hop
 *   and is LIVE iff b < clamp(*count, 0, n_bursts), 0 <= starts[b] <= 2^61, o >= 0 and o + nfft <= stream_len.  Other segments are
 *   skipped, never read and not counted.  The shape is fixed by (seg_per_burst, n_bursts): graph-capturable, a replay follows starts and
 *   count.  The same kernel with another origin map.
 *   GFDM_HIP_EINVAL: n < 0 or > 2^61; stream_len outside 0 .. 2^61; |first| > 2^60; seg_per_burst or n_bursts < 0; seg_per_burst *
 *   n_bursts > 2^40; a NULL buffer the call would touch; a buffer without the alignment of one element (8 bytes complex64, 4 sc16,
 *   8 int64).
 * Power accumulator (power): over every sample once, p = fadd_rn(fmul_rn(re, re), fmul_rn(im, im)) in fp32, no contraction (numpy's
 *   float32 reproduces it to the bit).  A non-finite p (an overflow included) counts in bad_samples and nowhere else.  A finite p:
 *     samples += 1;  peak_bits = max(peak_bits, bits(p)) (p >= +0: floats order as their bits; exact);  power_sum += p;
 *     hist[clamp((bits(p) >> 20) - 760, 0, 511)] += 1: eight bins per octave from 2^-32 to 2^32, bin 0 also takes everything below
 *     (zero and denormals: the flush mode cannot matter), bin 511 everything above; the lower edge of bin i is
 *     (1 + (i mod 8) / 8) 2^(floor(i / 8) - 32): the bins are pure integer rules on the bits of p.
 *   hist, samples, bad_samples: 64-bit integer atomics (exact, order-free); peak_bits: one atomic max; power_sum: fp64 partials per
 *   workgroup in tile order (tiles of 2048 samples), then the ordered sum pass.  No float atomics.
 * Error budget (derived, not measured) against the same formulas in float64 on the same float32 inputs, after any sequence of calls:
 *     |psd_sum[k] - ref[k]| <= sum_s (2 |X_s[k]| d_s + d_s^2) + 2^-40 ref[k],   d_s = (8 log2 nfft + 8) 2^-24 sqrt(nfft E_s),
 *     E_s = sum_n |x_n|^2 w_n^2    (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2, at 6.7 eps per radix-2 stage, widened
 *     for the window product and the squared magnitude; the last term covers the fp64 sums)
 *     |power_sum - ref| <= (tiles + 32) 2^-53 ref, tiles = ceil(n / 2048) summed over the calls (all terms are non-negative)
 *   segments, bad_segments, samples, bad_samples, peak_bits and hist are exact.
 * *_device: `in` has the alignment of one sample and no more; the calls neither allocate nor synchronise and are hipGraph-capturable.
 * *_host: a convenience, not a pipeline: upload, the device call on the handle's stream, one synchronise.
 * Not here: nfft that is no power of two or above 4096; cross-spectra and coherence; a spectrogram (the PSD is averaged only); a PA
 *   non-linearity to drive the meter with; per-burst PAPR (power on shaped frames gives the ensemble); setters for window or hop.
 * Tested range (tests/test_spectrum_meter_gpu.py against the numpy restatement of tests/spectrum_meter_ref.py): every nfft 16 .. 4096
 *   with a Hann window; hop 1, 3, nfft / 2, nfft - 1, nfft at nfft 16 and 64; n = nfft - 1, nfft, nfft + hop - 1; `in` at every alignment
 *   of one sample; sc16 against the widened call; repeated and cut streams; a NaN segment; accumulate_at with permuted starts, -1, a burst
 *   past stream_len and count below, at and beyond n_bursts; a window value of 3e38; power on 100 003 samples spanning 2^-40 .. 2^40; one graph replay;
 *   2 G + 3 trips past the bounded grid (tests/test_spectrum_grid_bound_gpu.py). */
typedef struct gfdm_hip_spectrum_meter gfdm_hip_spectrum_meter;
int gfdm_hip_spectrum_meter_create(gfdm_hip_spectrum_meter** out, const float* window, int nfft, int64_t hop, int device);
int gfdm_hip_spectrum_meter_destroy(gfdm_hip_spectrum_meter* m);
int gfdm_hip_spectrum_meter_nfft(const gfdm_hip_spectrum_meter* m);
int64_t gfdm_hip_spectrum_meter_hop(const gfdm_hip_spectrum_meter* m);
int gfdm_hip_spectrum_meter_window(const gfdm_hip_spectrum_meter* m, float* window);
int gfdm_hip_spectrum_meter_plan(int nfft, int64_t hop, int64_t n, int64_t* n_seg, int64_t* advance);
void* gfdm_hip_spectrum_meter_totals_device(gfdm_hip_spectrum_meter* m);
int64_t gfdm_hip_spectrum_meter_totals_bytes(const gfdm_hip_spectrum_meter* m);
int gfdm_hip_spectrum_meter_reset(gfdm_hip_spectrum_meter* m, void* stream);
int gfdm_hip_spectrum_meter_read(gfdm_hip_spectrum_meter* m, int64_t* head, double* power_sum, double* psd_sum, int64_t* hist, void* stream);
int gfdm_hip_spectrum_meter_accumulate_host(gfdm_hip_spectrum_meter* m, const float* in, int64_t n);
int gfdm_hip_spectrum_meter_accumulate_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream);
int gfdm_hip_spectrum_meter_accumulate_sc16_host(gfdm_hip_spectrum_meter* m, const int16_t* in, int64_t n);
int gfdm_hip_spectrum_meter_accumulate_sc16_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream);
int gfdm_hip_spectrum_meter_accumulate_at_host(gfdm_hip_spectrum_meter* m, const float* in, int64_t stream_len, const int64_t* starts, const int64_t* count,
                                               int64_t first, int64_t seg_per_burst, int64_t n_bursts);
int gfdm_hip_spectrum_meter_accumulate_at_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t stream_len, const void* starts, const void* count,
                                                 int64_t first, int64_t seg_per_burst, int64_t n_bursts, void* stream);
int gfdm_hip_spectrum_meter_accumulate_at_sc16_host(gfdm_hip_spectrum_meter* m, const int16_t* in, int64_t stream_len, const int64_t* starts,
                                                    const int64_t* count, int64_t first, int64_t seg_per_burst, int64_t n_bursts);
int gfdm_hip_spectrum_meter_accumulate_at_sc16_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t stream_len, const void* starts, const void* count,
                                                      int64_t first, int64_t seg_per_burst, int64_t n_bursts, void* stream);
int gfdm_hip_spectrum_meter_power_host(gfdm_hip_spectrum_meter* m, const float* in, int64_t n);
int gfdm_hip_spectrum_meter_power_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream);
int gfdm_hip_spectrum_meter_power_sc16_host(gfdm_hip_spectrum_meter* m, const int16_t* in, int64_t n);
int gfdm_hip_spectrum_meter_power_sc16_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GFDM_HIP_H */
