// bbme_device.hip -- context, launch sequence and the GPU half of the C-ABI (include/bbme.h).
// Replaces the MF object of the reference (motion_framework.h:9-54): bbme_create + bbme_set_frames_*
// are MF::MF, bbme_estimate is MF::calcMotionBlockMatching.  gfx950 only; no CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "bbme_internal.hpp"
#include "guard_layout.hpp"
#include "bbme_kernels.hpp"
#include "launch_plan.hpp"

using namespace bbme;

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return bbme::fail(BBME_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                              __FILE__, __LINE__);                                             \
    } while (0)

namespace {

// TEST HOOKS of the device allocations (guard_layout.hpp; include/bbme.h, "test hooks").  Both knobs are read at every allocation
// -- allocations are rare and the steady state makes none --, so a test can set them for one context.  With neither set the
// allocation path is what it was: one hipMalloc of the caller's bytes, nothing registered, nothing filled.
// BBME_TEST_GUARD: every allocation gets a guard band on either side; the registry below knows every live one, and a band is
// scanned by bbme_test_guard_check and when its buffer is freed or replaced, where damage goes into a sticky record.
// BBME_TEST_POISON: a fresh DATA buffer (Fill::poison) is filled with kPoisonByte.
enum class Fill {
    none,       // index lists, whose valid length is a counter's (an address derived from poison must not be possible), and probes
    poison      // data: grids, planes' upload buffer, colour store, staging, statistics partials, scratch
};

struct GuardRegistry {
    struct Entry { uint8_t *base; size_t payload; int device; std::string what; };
    std::mutex mu;
    std::vector<Entry> live;
    unsigned long long sticky = 0;                // damaged bands of buffers that are gone
    std::string sticky_first;
};
GuardRegistry &guard_registry() { static GuardRegistry r; return r; }

// Downloads and scans the two bands of `e`; appends to *violations and, while it is empty, describes the first damage in *first.
void guard_scan(const GuardRegistry::Entry &e, unsigned long long *violations, std::string *first)
{
    std::vector<uint8_t> band(kGuardBytes);
    for (int back = 0; back < 2; ++back) {
        const uint8_t *src = e.base + (back ? kGuardBytes + e.payload : 0);
        char text[256];
        if (hipMemcpy(band.data(), src, kGuardBytes, hipMemcpyDeviceToHost) != hipSuccess) {
            snprintf(text, sizeof text, "%s: the %s guard could not be read", e.what.c_str(), back ? "back" : "front");
        } else {
            const GuardDamage d = scan_guard(band.data(), kGuardBytes, back != 0);
            if (!d.count) continue;
            snprintf(text, sizeof text, "%s (%zu bytes): %s guard, offset %zu from the payload's edge holds 0x%02x (%zu damaged bytes, the "
                     "farthest at offset %zu)", e.what.c_str(), e.payload, back ? "back" : "front", d.first, (unsigned)d.first_byte,
                     d.count, d.last);
        }
        ++*violations;
        if (first->empty()) *first = text;
    }
}

void guard_register(uint8_t *base, size_t payload, const char *what)
{
    int device = 0;
    (void)hipGetDevice(&device);
    GuardRegistry &r = guard_registry();
    std::lock_guard<std::mutex> lock(r.mu);
    r.live.push_back({base, payload, device, what});
}

// A guarded buffer goes (freed, or replaced by ensure): whatever wrote near it has finished after the synchronisation
void guard_release(uint8_t *base)
{
    GuardRegistry &r = guard_registry();
    std::lock_guard<std::mutex> lock(r.mu);
    for (size_t i = 0; i < r.live.size(); ++i)
        if (r.live[i].base == base) {
            (void)hipDeviceSynchronize();
            guard_scan(r.live[i], &r.sticky, &r.sticky_first);
            r.live.erase(r.live.begin() + (long)i);
            return;
        }
}

// Owning handles of device memory and of events: whoever holds one releases it, so an early return leaks nothing.
// DevBuf is move-only, its sizes are in elements of T; every size expression and its slack stays with the caller (they are
// contracts with the kernels).  Errors are the library's codes: "allocating <what>: <HIP's text>".  The caller says what kind
// of buffer it is (Fill); alloc_zero and upload fill their own part.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_), guarded_(o.guarded_) { o.p_ = nullptr; o.bytes_ = 0; o.guarded_ = false; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t size() const { return bytes_ / sizeof(T); }
    int alloc(size_t n, const char *what, Fill fill) { return alloc_bytes(n * sizeof(T), what, fill, 0); }
    int alloc_zero(size_t n, const char *what)
    {
        if (int rc = alloc(n, what, Fill::none)) return rc;
        return check(hipMemset(p_, 0, bytes_), what);
    }
    // the vector's bytes, and `slack_bytes` behind them that a kernel may load (and mask) but that hold nothing (poisoned in a test)
    template <class U>
    int upload(const std::vector<U> &v, const char *what, size_t slack_bytes = 0)
    {
        if (int rc = alloc_bytes(v.size() * sizeof(U) + slack_bytes, what, Fill::poison, v.size() * sizeof(U))) return rc;
        return check(hipMemcpy(p_, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice), what);
    }
    // scratch: allocated on first use, replaced when more is asked for (the caller orders that against whoever reads it)
    int ensure(size_t n, const char *what, Fill fill) { return n * sizeof(T) <= bytes_ ? BBME_OK : alloc(n, what, fill); }

private:
    static int check(hipError_t e, const char *what)
    {
        return e == hipSuccess ? BBME_OK : bbme::fail(BBME_ERR_HIP, "allocating %s: %s", what, hipGetErrorString(e));
    }
    uint8_t *base() const { return reinterpret_cast<uint8_t *>(p_) - (guarded_ ? kGuardBytes : 0); }
    void release()
    {
        if (!p_) return;
        if (guarded_) guard_release(base());
        (void)hipFree(base());
        p_ = nullptr;
        bytes_ = 0;
        guarded_ = false;
    }
    // `poison_from`: the first payload byte that Fill::poison covers (upload overwrites what lies in front of it)
    int alloc_bytes(size_t bytes, const char *what, Fill fill, size_t poison_from)
    {
        release();
        const bool guarded = test_knob_on(getenv("BBME_TEST_GUARD"));
        const bool poison = fill == Fill::poison && test_knob_on(getenv("BBME_TEST_POISON")) && poison_from < bytes;
        const GuardLayout g = guard_layout(bytes, guarded);
        void *raw = nullptr;
        if (int rc = check(hipMalloc(&raw, g.total()), what)) return rc;
        uint8_t *b = static_cast<uint8_t *>(raw);
        if (guarded || poison) {
            // the fills run on the null stream, which the context's streams do not wait for: finished before anything is enqueued
            hipError_t e = hipSuccess;
            if (guarded) e = hipMemset(b, kGuardByte, g.front);
            if (guarded && e == hipSuccess) e = hipMemset(b + g.back_offset(), kGuardByte, g.back);
            if (poison && e == hipSuccess) e = hipMemset(b + g.payload_offset() + poison_from, kPoisonByte, bytes - poison_from);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) { (void)hipFree(raw); return check(e, what); }
        }
        if (guarded) guard_register(b, bytes, what);
        p_ = reinterpret_cast<T *>(b + g.payload_offset());
        bytes_ = bytes;
        guarded_ = guarded;
        return BBME_OK;
    }
    T *p_ = nullptr;
    size_t bytes_ = 0;
    bool guarded_ = false;
};

// Statistics scratch of a gather stage (k_motion_compensate .. k_temporal_filter_bgr): `slots` result quadruples (one per pair or
// frame, filled by k_mc_reduce), then the kernel's partials, four words per workgroup -- `groups` per pair or frame --, of a launch
// over everything the context holds (`all` pairs or frames), then those of a caller's launch over `caller` more.  The layout is
// the stage's (layout() names the same one at every call); how the buffer may grow is its caller's business.
struct StatsScratch {
    void layout(int slots, long long groups, int all) { slots_ = slots; groups_ = groups; all_ = all; }
    size_t words(int caller) const { return (size_t)4 * (slots_ + groups_ * (all_ + caller)); }
    size_t size() const { return buf_.size(); }
    int ensure(int caller, const char *what) { return buf_.ensure(words(caller), what, Fill::poison); }
    int ensure(int slots, long long groups, int all, int caller, const char *what)
    {
        layout(slots, groups, all);
        return ensure(caller, what);
    }
    unsigned long long *results() const { return buf_; }
    unsigned long long *partials_all() const { return buf_ + (size_t)4 * slots_; }
    unsigned long long *partials_caller() const { return buf_ + words(0); }

private:
    DevBuf<unsigned long long> buf_;
    int slots_ = 0, all_ = 0;
    long long groups_ = 0;
};

struct DevEvent {
    hipEvent_t ev = nullptr;
    DevEvent() = default;
    DevEvent(DevEvent &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    ~DevEvent() { if (ev) (void)hipEventDestroy(ev); }
    operator hipEvent_t() const { return ev; }
};

struct Level : PlanLevel {                        // width, height, block, range and what the search plans give (launch_plan.hpp)
    int search = 0;
    // Every padded plane of the level (pitch == width), one plane_stride apart, in ONE allocation.  A pair or batch context: the
    // image-1 planes of its pairs, then, from frame_step on, their image-2 planes.  A chain context: its pairs + 1 frame slots.
    // Either way pair p reads img1 + p * plane_stride and img2 + p * plane_stride, and the slack behind every plane is zero.
    DevBuf<uint8_t> img1;
    uint8_t *img2 = nullptr;                      // img1 + frame_step
    size_t frame_step = 0;                        // bytes from a pair's image 1 to its image 2: on a chain one plane_stride
    // MV grids.  small[]: grids at the level's own block size B (the search writes small[0]; the two sweeps at B go
    // small[0] -> small[1] -> small[0], which then stays untouched until the level's next search: the speculative search
    // of the next finer level predicts from it).  big[]: grids at b < B (capacity (H/2)*(W/2)), ping-pong; zeroed at creation,
    // since a speculative search may read them before any sweep has written them (newest_coarse_grid, bbme_kernels.hpp).
    DevBuf<mv_t> small[2];
    DevBuf<mv_t> big[2];
    mv_t *cur_grid = nullptr;                     // the grid that holds the current field
    int cur_block = 0;                            // its block size (0 = nothing yet)
    DevBuf<mv_t> pred;                            // per block: the coarse MV a speculative search started from
    DevBuf<uint32_t> fix_list, fix_count;         // blocks to search again after a speculative search
    // as the coarse side of a speculative search: the sweeps behind the fork that are complete (RegArgs::publish; 64 bytes per pair)
    DevBuf<uint32_t> publish;
    mv_t *final_grid() const { return block == 2 ? small[0] : big[1]; }   // where two sweeps per block size leave the 2x2 cells
    DevBuf<uint32_t> spiral;                      // rank -> packed (dx, dy)
    int ncand = 0;
    int pitch_dw = 0;
    // fast search kernel (block 8 / 16 / 32)
    DevBuf<uint16_t> rank_of;
    int rank_pitch = 0;
    DevBuf<uint32_t> tasks, rounds;
    int nrounds = 0;
    DevBuf<uint32_t> tasks2, rounds2;                 // the plan for two waves per macroblock (levels of few blocks)
    int nrounds2 = 0;
    DevBuf<uint2> lane_ranks, lane_ranks2;            // per plan: the ranks of every lane's candidates (FastSearchArgs::lane_ranks)
    // batch: every per-pair buffer holds ctx->batch copies, pair p at p * stride elements (multiples of 64 elements)
    uint32_t plane_stride = 0;                        // img1 / img2, bytes (frame_step and every product with it: size_t)
    uint32_t small_stride = 0;                        // small[], pred, fix_list: words
    uint32_t big_stride = 0;                          // big[]: words
    uint32_t grid_stride(const mv_t *g) const { return (g == small[0] || g == small[1]) ? small_stride : big_stride; }
    mv_t *grid(GridId g) const { return g == kSmall0 ? small[0] : g == kSmall1 ? small[1] : g == kBig0 ? big[0] : big[1]; }
    GridId grid_id(const mv_t *g) const { return g == small[0] ? kSmall0 : g == small[1] ? kSmall1 : g == big[0] ? kBig0 : kBig1; }
};

}  // namespace

struct bbme_ctx {
    bbme_params params{};
    Geometry geom{};
    int device = 0;
    int batch = 1;                                // independent frame pairs this context holds (blockIdx.y of every kernel)
    Tuning tune;
    size_t flow_stride = 0;                       // floats from pair to pair in `flow`
    uint32_t list_stride = 0, own_stride = 0;     // words from pair to pair in list[] / own
    size_t raw_stride = 0;                        // bytes from slot to slot in raw
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<Level> lv;
    DevBuf<float> flow;                           // dense padded H0 x W0 float2
    DevBuf<uint32_t> list[2];
    DevBuf<uint8_t> flags[2];                     // dirty flags of the regulariser, one byte per block, all zero between sweeps
    size_t flag_bytes = 0;
    DevBuf<uint32_t> own;                         // ownership counters of the solver, one word per block
    uint32_t own_pitch = 0;                       // transposed layout: 32 residue classes of own_pitch words
    DevBuf<uint32_t> counters;                    // 64 words (RegArgs::counters)
    // SAD memo of the regulariser's chain form (bbme_kernels.hpp, "SAD memo"): nine (MV, SAD) words per block at b >= 8
    DevBuf<unsigned long long> memo;
    uint32_t memo_stride = 0;                     // words from pair to pair
    size_t memo_blocks = 0;                       // blocks per pair it has room for
    int memo_level = -1, memo_block = 0;          // the (level, block size) its slots describe; block 0 = nothing
    // FRAME SLOTS: every frame the context holds has one number, used for its planes (Level::img1), the upload buffer, the colour
    // store and the two vectors of flags below.  A pair or batch context holds 2 batch frames, frame `which` of pair p in slot
    // which * batch + p; a chain context (bbme_create_chain) holds batch + 1, pair p reading slots p and p + 1.
    bool chain = false;
    int frames() const { return chain ? batch + 1 : 2 * batch; }
    int slot(int pair, int which) const { return chain ? pair + which : which * batch + pair; }
    std::vector<uint8_t> slot_set;                // per slot: it has planes (bbme_estimate needs every slot's)
    bool frames_set() const { return std::find(slot_set.begin(), slot_set.end(), 0) == slot_set.end(); }
    bool jacobi = false;                          // opt-in, not bit-exact: Jacobi sweeps (pass 1 only); bbme_set_regularizer_mode
    bool raster_search = false;                   // MF::find_min_block (:246-294) instead of the spiral search; bbme_set_search_mode
    bool relax = true;                            // relaxation launches (k_reg_iter) on large grids of small blocks; bbme_set_relaxation
    hipStream_t side_stream = nullptr;            // the speculative searches
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipGraphExec_t graph_exec[2] = {nullptr, nullptr};   // the captured launch sequence of each direction, captured on first use
    // bbme_set_direction: BBME_DIR_BACKWARD exchanges the two plane bases in the arguments of every kernel that reads planes for
    // an estimate or a result (plane1 / plane2 below); setters, the chain roll and the plane accessors stay physical
    int direction = 0;
    // A context keeps ONE graph with the speculative search's forked branch: a second forked graph on the same context replays
    // 0.9 ms slower at 4K whichever direction it is (2.4 ms against 1.43-1.47; 1.57 unforked; profiles/r08_bidirectional.txt).
    // FORWARD's graph always speculates; BACKWARD's only while the context has no FORWARD graph, and capturing FORWARD drops a
    // forked BACKWARD graph (captured again, unforked, on its next use).  Tuning::fork_both: both forked (measurements).
    bool graph_forked[2] = {false, false};
    // bit l: level l's search is speculative in the launch sequence of that direction (enqueue_pyramid), and in the last
    // estimate (bbme_fixup_counts)
    uint32_t spec_levels[2] = {0, 0}, last_spec_levels = 0;
    const uint8_t *plane1(const Level &L) const { return direction ? L.img2 : L.img1.get(); }
    const uint8_t *plane2(const Level &L) const { return direction ? L.img1.get() : L.img2; }
    // bbme_estimate_bidirectional: level 0's final grid of the backward half, every pair (bwd_stride words apart), and whether
    // it and the forward grid still describe the frames the context holds
    DevBuf<mv_t> bwd_cells;
    uint32_t bwd_stride = 0;
    bool fields_valid = false;
    bool profiling = false;
    float t_total = 0, t_search = 0, t_reg = 0, t_expand = 0, t_search0 = 0;
    hipEvent_t ev_sub = nullptr;                  // stream_behind_ctx: orders a caller's stream behind the ctx stream
    // scratch of single entry points, allocated on their first use (DevBuf::ensure)
    DevBuf<double> epe_scratch;                   // partial sums + counts of bbme_calculate_mse_device
    // STAGING AREA of the host getters (bbme_get_*_host): the packed product before its download (download_staged).  Every host
    // getter waits for the context's stream before it returns, so the area is free on entry: one area serves them all, and it
    // only grows (on the context's device) -- to the largest product asked for so far.
    DevBuf<uint8_t> staging;
    template <class T>
    int staged(size_t n, const char *what, T **p)      // room for n elements of T, at least
    {
        if (n * sizeof(T) > staging.size()) {
            HIP_TRY(hipSetDevice(device));
            if (int rc = staging.ensure(n * sizeof(T), what, Fill::poison)) return rc;
        }
        *p = reinterpret_cast<T *>(staging.get());
        return BBME_OK;
    }
    StatsScratch fb_stats;                        // bbme_consistency_stats (every pair) and bbme_cells_consistency_device (one pair)
    DevBuf<uint8_t> raw;                          // the host setters' upload buffer: one unpadded grey frame per slot
    StatsScratch mc_stats;                        // bbme_compensation_error (every pair)
    StatsScratch ip_stats;                        // bbme_interpolation_stats (every pair) and bbme_cells_interpolate_device (one pair,
                                                  // every phase): grows with the phases
    DevBuf<uint32_t> color_range;                 // colour coding: the key words of every slot (pair 0 .. batch - 1, then the slot of
                                                  // bbme_cells_color_device; k_color_range), then five floats per slot
    // COLOUR STORE (include/bbme.h): one packed B,G,R frame (pitch 3 width) per slot, bgr_stride bytes apart, allocated by the
    // first *_bgr setter.  bgr_set[slot]: the slot's colour is what its luma plane was made from (cleared by every grey setter
    // of that frame).
    DevBuf<uint8_t> bgr;
    size_t bgr_stride = 0;
    std::vector<uint8_t> bgr_set;
    StatsScratch tf_stats;                        // bbme_temporal_filter_stats (every frame) and bbme_cells_temporal_filter_device (one)
    StatsScratch tf_bgr_stats;                    // the same of bbme_temporal_filter_bgr_stats and bbme_cells_temporal_filter_bgr_device
    int src_scale = 1;                            // 4 after a setter of frames to up-sample (bbme_set_frames_*_x4, scale 4 of a chain), else 1
    StatsScratch sp_stats;                        // bbme_subpel_stats (every pair) and bbme_cells_subpel_device (one pair)
    DevBuf<mv_t> sc_q4;                           // the quarter-pel cells the context's own sub-pel compensation reads: a packed
                                                  // grid per pair, allocated at first use (enqueue_own_sc)
    StatsScratch sc_stats;                        // bbme_subpel_compensation_error (every pair) and
                                                  // bbme_cells_subpel_compensate_device (one pair)
    DevBuf<mv_t> si_q4;                           // the quarter-pel cells the context's own sub-pel interpolation reads: the packed
                                                  // forward grids of every pair, then their backward grids, allocated at first use
                                                  // (enqueue_own_si)
    StatsScratch si_stats;                        // bbme_subpel_interpolation_stats (every pair) and
                                                  // bbme_cells_subpel_interpolate_device (one pair, `count` phases)
    DevBuf<mv_t> tfs_q4;                          // the quarter-pel cells the context's own sub-pel temporal filters read, grey and
                                                  // colour (both refine the same cells on the same luma planes): the packed forward
                                                  // grids of every pair, then their backward grids, allocated at first use
                                                  // (TfSubpel::prepare)
    StatsScratch tfs_stats;                       // bbme_subpel_temporal_filter_stats (every frame) and
                                                  // bbme_cells_subpel_temporal_filter_device (one)
    StatsScratch tfsb_stats;                      // bbme_subpel_temporal_filter_bgr_stats (every frame) and
                                                  // bbme_cells_subpel_temporal_filter_bgr_device (one)
    StatsScratch cmp_stats;                       // bbme_cells_compose_device: one result quadruple and one launch's partials
    DevBuf<mv_t> wide_cells, wide_q4;             // a chain's wide temporal filter: the composed integer cells into slot f + 2 of
                                                  // every slot f, then those into slot f - 2, packed; and the same refined to
                                                  // quarter pels.  Allocated at first use (wide_prepare)
    StatsScratch wide_stats;                      // bbme_wide_temporal_filter_stats (two quadruples per slot) and
                                                  // bbme_cells_wide_temporal_filter_device (two more)
    StatsScratch wide_bgr_stats;                  // the same of bbme_wide_temporal_filter_bgr_stats and
                                                  // bbme_cells_wide_temporal_filter_bgr_device
    // GLOBAL MOTION RULE, all allocated at first use
    DevBuf<unsigned long long> gm_words;          // sixteen result words per pair (BBME_MAX_BATCH of them), then K17's partials of a
                                                  // launch over every pair, then those of a caller's launch (gm_scratch)
    DevBuf<uint32_t> gm_hist;                     // bbme_global_motion: the two histograms of every pair
    DevBuf<int32_t> gm_models;                    // the device table of models, six words per pair
    DevBuf<mv_t> gm_q4;                           // with subpel = 1: the refined cells of every pair, packed
    DevBuf<uint8_t> gm_mask;                      // with mask_tol >= 0: the consistency mask of every pair, packed
    StatsScratch gc_stats;                        // bbme_global_compensation_error (every pair) and
                                                  // bbme_cells_global_compensate_device (one pair)
    // BGR GLOBAL COMPENSATION RULE, allocated at first use and at one size, so neither is replaced under a launch that reads it
    StatsScratch gcb_stats;                       // bbme_global_compensation_error_bgr (every pair) and
                                                  // bbme_cells_global_compensate_bgr_device (BBME_GC_MAX_FRAMES frames)
    DevBuf<int32_t> gcb_models;                   // the device tables of models, six words per frame: every pair's of the context's own
                                                  // calls (BBME_MAX_BATCH), then a caller's run (BBME_GC_MAX_FRAMES)
    StatsScratch cb_stats;                        // bbme_compensation_error_bgr (every pair) and bbme_cells_compensate_bgr_device
                                                  // (one pair)
};

namespace {

int check_ctx(const bbme_ctx *c)
{
    if (!c) return bbme::fail(BBME_ERR_INVALID, "ctx is null");
    return BBME_OK;
}

// The stage-by-stage entry points, the plane injection, the sweep counters, the device-side EPE and the RCCL gather address ONE
// pair: on a batched context (bbme_create_batch with pairs > 1) they are refused rather than silently applied to pair 0.
int single_pair_only(const bbme_ctx *c, const char *what)
{
    if (int rc = check_ctx(c)) return rc;
    if (c->batch > 1)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s addresses one pair: not available on a batched context (%d pairs)", what, c->batch);
    return BBME_OK;
}

// The pair setters write both planes of a pair; in a chain context a plane belongs to two pairs and is set by slot.
int pair_context_only(const bbme_ctx *c, const char *what)
{
    if (int rc = check_ctx(c)) return rc;
    if (c->chain)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s sets the two frames of a pair: a chain context (%d pairs over %d frame slots) "
                                                "is fed with bbme_set_chain_frames_*", what, c->batch, c->batch + 1);
    return BBME_OK;
}

int chain_context_only(const bbme_ctx *c, const char *what)
{
    if (int rc = check_ctx(c)) return rc;
    if (!c->chain) return bbme::fail(BBME_ERR_UNSUPPORTED, "%s needs a chain context (bbme_create_chain)", what);
    return BBME_OK;
}

// Calls that read planes on a chain context between bbme_chain_advance and the setting of the last slot
int chain_slots_ready(const bbme_ctx *c, const char *what)
{
    if (c->chain && !c->frames_set())
        return bbme::fail(BBME_ERR_STATE, "%s: not every frame slot of the chain context is set", what);
    return BBME_OK;
}

int check_level(const bbme_ctx *c, int level)
{
    if (int rc = check_ctx(c)) return rc;
    if (level < 0 || level >= (int)c->lv.size())
        return bbme::fail(BBME_ERR_INVALID, "level %d out of range 0..%d", level, (int)c->lv.size() - 1);
    return BBME_OK;
}

void drop_graph(bbme_ctx *c)
{
    for (hipGraphExec_t &g : c->graph_exec)
        if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    c->graph_forked[0] = c->graph_forked[1] = false;
}

// What every setter does that changes the launch sequence (other kernels, another stream): the graphs may still be running
int settle_and_drop_graphs(bbme_ctx *c)
{
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_graph(c);
    return BBME_OK;
}

// The stream an entry point enqueues on: the context's own for a null `hip_stream`, else the caller's, ordered behind whatever
// the context's stream holds at this point
int stream_behind_ctx(bbme_ctx *c, void *hip_stream, hipStream_t *stream)
{
    *stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if (*stream == c->stream) return BBME_OK;
    if (!c->ev_sub) HIP_TRY(hipEventCreateWithFlags(&c->ev_sub, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_sub, c->stream));
    HIP_TRY(hipStreamWaitEvent(*stream, c->ev_sub, 0));
    return BBME_OK;
}

// An optional window {x0, y0, w, h} inside limit_w x limit_h: the plane of `level`, or (level < 0) a grid of cells.  Touches no device.
int check_window(const int *window, int limit_w, int limit_h, const char *what, int level)
{
    if (!window || (window[0] >= 0 && window[1] >= 0 && window[2] >= 1 && window[3] >= 1 &&
                    (long long)window[0] + window[2] <= limit_w && (long long)window[1] + window[3] <= limit_h))
        return BBME_OK;
    char where[32] = "cells";
    if (level >= 0) snprintf(where, sizeof where, "plane of level %d", level);
    return bbme::fail(BBME_ERR_INVALID, "%s: window (%d, %d, %d, %d) is not inside the %dx%d %s", what, window[0], window[1],
                      window[2], window[3], limit_w, limit_h, where);
}

// wx0 .. wy1 of McArgs / FbArgs: the window, or the whole full_w x full_h
template <class Args>
void set_window(Args &a, const int *window, int full_w, int full_h)
{
    a.wx0 = window ? window[0] : 0; a.wy0 = window ? window[1] : 0;
    a.wx1 = window ? window[0] + window[2] : full_w; a.wy1 = window ? window[1] + window[3] : full_h;
}

// The regulariser's waves leave at a round cap instead of spinning for ever (RegArgs::round_cap); a sweep that hit
// it has not reached the fixed point and its field must not be handed out as a result.  Waits for the stream.  On
// that path the solver's ownership words and counters are stale too: cleared, so that the context stays usable.
int check_converged(bbme_ctx *c)
{
    std::vector<uint32_t> flags((size_t)c->batch, 0u);    // counters[5] of every pair (64 words apart)
    HIP_TRY(hipMemcpy2DAsync(flags.data(), sizeof(uint32_t), c->counters + 5, 64 * sizeof(uint32_t), sizeof(uint32_t),
                             (size_t)c->batch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bool flag = false;
    for (uint32_t f : flags) flag = flag || f != 0;
    if (!flag) return BBME_OK;
    HIP_TRY(hipMemsetAsync(c->own, 0, (size_t)c->own_stride * 4 * c->batch, c->stream));
    HIP_TRY(hipMemsetAsync(c->counters, 0, (size_t)256 * c->batch, c->stream));
    HIP_TRY(hipMemsetAsync(c->flags[0], 0, c->flag_bytes * c->batch, c->stream));
    HIP_TRY(hipMemsetAsync(c->flags[1], 0, c->flag_bytes * c->batch, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return bbme::fail(BBME_ERR_STATE, "a regulariser sweep hit its round cap without converging: the motion field is not "
                                      "the reference's and has been discarded");
}

// What every probe starts with.  They own their buffers and events (DevBuf, DevEvent): an error return releases them.
const char *const kProbe = "probe buffers";

int probe_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return bbme::fail(BBME_ERR_HIP, "no HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    return BBME_OK;
}

// launch(0), launch(1) on the null stream: the milliseconds the second one took
template <class Launch>
int time_second_launch(Launch &&launch, float *ms)
{
    DevEvent e0, e1;
    HIP_TRY(hipEventCreate(&e0.ev));
    HIP_TRY(hipEventCreate(&e1.ev));
    for (int rep = 0; rep < 2; ++rep) {
        HIP_TRY(hipEventRecord(e0, 0));
        launch(rep);
        HIP_TRY(hipEventRecord(e1, 0));
        HIP_TRY(hipEventSynchronize(e1));
    }
    HIP_TRY(hipEventElapsedTime(ms, e0, e1));
    return BBME_OK;
}

// ---- launches ---------------------------------------------------------------------------

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a kernel, not to a context: every context of the process that launches
// the kernel on the device depends on it.  So it is only ever raised, to the most any context has asked of it there; a context
// created later with a smaller window must not lower it under one that is still alive.
int raise_lds_limit(int device, const void *kernel, size_t bytes)
{
    if (bytes <= 48 * 1024) return BBME_OK;                 // what every kernel may use without the attribute
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> granted;
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = granted[{device, kernel}];
    if (bytes <= cur) return BBME_OK;
    const hipError_t err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return bbme::fail(BBME_ERR_HIP, "%zu bytes of LDS for a search kernel: %s", bytes, hipGetErrorString(err));
    cur = bytes;
    return BBME_OK;
}

// The one place a run-time block size becomes a template argument: f(std::integral_constant<int, B>) for the B of `Bs` that
// equals `b`, and its return code.
template <int... Bs, class F>
int with_block(int b, F &&f)
{
    int rc = BBME_OK;
    const bool hit = ((b == Bs && ((rc = f(std::integral_constant<int, Bs>{})), true)) || ...);
    return hit ? rc : bbme::fail(BBME_ERR_UNSUPPORTED, "block size %d", b);
}

// Where the search of `level` takes its predictions from (copyMVs, :828-843), by mode:
//   plain / fix-up : the coarser level's final 2x2-cell grid (it must have been regularised down to 2x2);
//   speculative    : the coarser level's grid as the sweeps at its own block size have left it when the search is forked
//                    (Level::small[0] behind the second of them); the fast kernel's blocks may take a newer one (set_late_grids).
template <class Args>
int set_prediction_source(bbme_ctx *c, int level, int mode, Args &a)
{
    Level &L = c->lv[level];
    a.mode = mode;
    a.pred = L.pred;
    a.coarse = nullptr;
    a.s_plane = L.plane_stride; a.s_pred = L.small_stride; a.s_out = L.small_stride; a.s_coarse = 0;
    if (level + 1 >= (int)c->lv.size()) return BBME_OK;
    Level &C = c->lv[level + 1];
    a.coarse_block = C.block;
    if (mode == kSearchSpeculative) {
        if (C.cur_block != C.block || (C.cur_grid != C.small[0] && C.cur_grid != C.small[1]))
            return bbme::fail(BBME_ERR_STATE, "level %d is not behind a sweep at its own block size", level + 1);
        a.coarse = C.cur_grid;
        a.coarse_cell_shift = 0;
        while ((1 << a.coarse_cell_shift) < C.block) ++a.coarse_cell_shift;
    } else {
        if (C.cur_block != 2)
            return bbme::fail(BBME_ERR_STATE, "level %d has not been regularised down to 2x2 blocks", level + 1);
        a.coarse = C.cur_grid;
        a.coarse_cell_shift = 1;
    }
    a.coarse_cols = C.width >> a.coarse_cell_shift;
    a.s_coarse = C.grid_stride(a.coarse);
    return BBME_OK;
}

// What the launch plan decides from (launch_plan.hpp): the levels' numbers, the context's modes and its knobs
PlanInputs plan_inputs(const bbme_ctx *c)
{
    PlanInputs in;
    in.lv.assign(c->lv.begin(), c->lv.end());
    in.pairs = c->batch;
    in.jacobi = c->jacobi; in.raster_search = c->raster_search; in.relax = c->relax;
    in.tune = c->tune;
    in.memo_blocks = c->memo_blocks;
    return in;
}

static_assert(kPredictPlain == kSearchPlain && kPredictSpeculative == kSearchSpeculative && kPredictFixup == kSearchFixup, "prediction modes");

// FastSearchArgs::late of the speculative launch of `level`: the coarser level's grids in the order the sweeps behind the fork
// leave them (entry 0 is a.coarse, set_prediction_source), and the word those sweeps publish their number in (enqueue_pyramid).
void set_late_grids(bbme_ctx *c, const SearchLaunch &s, FastSearchArgs &a)
{
    a.late_word = nullptr; a.late_n = 0; a.late_force = 0;
    if (!s.late) return;
    const Level &C = c->lv[s.level + 1];
    a.late_n = fill_coarse_grids(a.late, C.width, C.block, a.coarse == C.small[1], C.small[0], C.small[1], C.small_stride,
                                 C.big[0], C.big[1], C.big_stride);
    a.late_word = C.publish;
    a.late_force = s.late_force;
}

// Level::tasks2 ..: the plan whose rounds have 128 strips, for two waves per macroblock
void use_two_wave_plan(FastSearchArgs &a, const Level &L)
{
    a.tasks = L.tasks2; a.rounds = L.rounds2; a.nrounds = L.nrounds2; a.lane_ranks = L.lane_ranks2;
    a.stage_rpp = 128u / ((uint32_t)(L.fast_pitch_dw + 3) / 4);
}

int launch_search_fast(bbme_ctx *c, const SearchLaunch &s, hipStream_t stream)
{
    Level &L = c->lv[s.level];
    FastSearchArgs a{};
    a.image1 = c->plane1(L); a.image2 = c->plane2(L);
    a.width = L.width; a.height = L.height;
    a.range = L.range; a.spiral = L.spiral;
    a.rank_of = L.rank_of; a.rank_pitch = L.rank_pitch;
    a.tasks = L.tasks; a.rounds = L.rounds; a.nrounds = L.nrounds; a.lane_ranks = L.lane_ranks;
    {
        const uint32_t nch = (uint32_t)(L.fast_pitch_dw + 3) / 4;
        a.stage_magic = (65536u + nch - 1) / nch;
        a.stage_rpp = 64u / nch;
    }
    if (int rc = set_prediction_source(c, s.level, s.mode, a)) return rc;
    set_late_grids(c, s, a);
    a.out = L.small[0];
    a.cols = L.width / L.block;
    a.pitch_dw = L.fast_pitch_dw;
    const int nblocks = L.blocks_at(L.block);
    a.nblocks = nblocks;
    a.cols_magic = (uint64_t)nblocks * (uint64_t)a.cols < (1ull << 32) ? (uint32_t)(((1ull << 32) + (uint64_t)a.cols - 1) / (uint64_t)a.cols) : 0u;
    a.xcd_remap = c->tune.xcd_remap;
    a.fix_count = L.fix_count;
    a.s_fix_list = L.small_stride;
    const unsigned P = (unsigned)c->batch;
    const bool list = s.kernel == SearchKernel::List;
    if (list) {
        a.mode = kSearchPlain;                               // k_search_list searches what k_fixup_list has compared and listed
        hipLaunchKernelGGL(k_fixup_list, dim3(s.list_grid, P), dim3(256), 0, stream, a, L.block, L.fix_count.get(), L.fix_list.get());
    }
    if (s.waves == 2) use_two_wave_plan(a, L);
    // the one launch site: the listed blocks (k_search_list) or the whole level (k_search_fast), W waves per block
    return with_block<8, 16, 32>(L.block, [&](auto B) {
        auto launch = [&](auto W) {
            constexpr int kB = decltype(B)::value, kW = decltype(W)::value;
            if (list) hipLaunchKernelGGL((k_search_list<kB, kW>), dim3(s.grid, P), dim3(64 * kW), s.lds, stream, a, L.fix_count.get(), L.fix_list.get());
            else hipLaunchKernelGGL((k_search_fast<kB, kW>), dim3(s.grid, P), dim3(64 * kW), s.lds, stream, a);
        };
        if (s.waves == 2) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 1>{});
        HIP_TRY(hipGetLastError());
        return (int)BBME_OK;
    });
}

int launch_search(bbme_ctx *c, const SearchLaunch &s)
{
    Level &L = c->lv[s.level];
    const hipStream_t stream = s.side_stream ? c->side_stream : c->stream;
    int rc;
    if (s.kernel != SearchKernel::Generic) {
        rc = launch_search_fast(c, s, stream);
    } else {
        SearchArgs a{};
        a.image1 = c->plane1(L); a.image2 = c->plane2(L);
        a.width = L.width; a.height = L.height;
        a.range = L.range; a.ncand = L.ncand; a.spiral = L.spiral;
        a.raster = c->raster_search ? 1 : 0;
        if ((rc = set_prediction_source(c, s.level, s.mode, a))) return rc;
        a.out = L.small[0];
        a.cols = L.width / L.block;
        a.pitch_dw = L.pitch_dw;
        rc = with_block<2, 4, 8, 16, 32, 64>(L.block, [&](auto B) {
            hipLaunchKernelGGL(k_search_generic<B()>, dim3(s.grid, c->batch), dim3(64), s.lds, stream, a);
            HIP_TRY(hipGetLastError());
            return (int)BBME_OK;
        });
    }
    if (rc == BBME_OK && s.mode != kSearchSpeculative) { L.cur_grid = L.small[0]; L.cur_block = L.block; }
    return rc;
}

template <int BS>
void launch_sweep_t(RegArgs a, const SweepLaunch &s, uint8_t *const (&flags)[2], unsigned P, hipStream_t st)
{
    // pass 1 marks flags[0]; relaxation step i consumes flags[i & 1] and marks the other; the solver
    // consumes what the last step marked.  Every flag is zero again afterwards.
    a.flag_cur = nullptr; a.flag_next = s.solve ? flags[0] : nullptr;
    a.lazy = s.lazy ? 1 : 0;
    const dim3 grid1(s.pass1_grid, P);
    switch (s.pass1) {
    case Pass1::ChainMemo:
        if constexpr (BS >= 8) hipLaunchKernelGGL((k_reg_pass1_lanes<BS, true>), grid1, dim3(256), 0, st, a);
        break;
    case Pass1::Chain: hipLaunchKernelGGL(k_reg_pass1_lanes<BS>, grid1, dim3(256), 0, st, a); break;
    case Pass1::Strip:
        if constexpr (BS <= 4) hipLaunchKernelGGL(k_reg_pass1_strip<BS>, grid1, dim3(256), 0, st, a);
        break;
    case Pass1::Plain: hipLaunchKernelGGL(k_reg_pass1<BS>, grid1, dim3(256), 0, st, a); break;
    }
    if (!s.solve) return;
    int cur = 0;
    for (int i = 0; i < s.relax_steps; ++i, cur ^= 1) {
        a.flag_cur = flags[cur]; a.flag_next = flags[cur ^ 1];
        hipLaunchKernelGGL(k_reg_iter<BS>, dim3(s.relax_tiles, P), dim3(256), 0, st, a);
    }
    a.flag_cur = flags[cur]; a.flag_next = nullptr;
    a.memo_init = 0;                                       // pass 1 has written every slot
    const dim3 grid2(s.solve_grid, P), waves(64 * s.solve_waves);
    a.flood = s.flood;
    auto solve = [&](auto SEG) {
        auto launch = [&](auto MEMO) {
            if (s.flood > 0) hipLaunchKernelGGL((k_reg_solve<BS, SEG(), MEMO(), true>), grid2, waves, 0, st, a);
            else hipLaunchKernelGGL((k_reg_solve<BS, SEG(), MEMO()>), grid2, waves, 0, st, a);
        };
        if constexpr (BS >= 8) {
            if (s.memo) { launch(std::true_type{}); return; }
        }
        launch(std::false_type{});
    };
    if (s.solve_segment == 4) solve(std::integral_constant<int, 4>{});
    else solve(std::integral_constant<int, 16>{});
}

// One sweep on the level's current grid, which must be the one the entry was planned on
int launch_sweep(bbme_ctx *c, const SweepLaunch &s, bool stats = false)
{
    const int level = s.level, b = s.block;
    Level &L = c->lv[level];
    if (L.cur_block != b << s.old_shift || L.cur_grid != L.grid(s.from))
        return bbme::fail(BBME_ERR_STATE, "level %d grid is at block size %d, cannot sweep at %d",
                          level, L.cur_block, b);
    RegArgs a{};
    a.old_shift = s.old_shift;
    a.image1 = c->plane1(L); a.image2 = c->plane2(L);
    a.width = L.width; a.height = L.height;
    a.rows = L.height / b; a.cols = L.width / b;
    a.old_grid = L.cur_grid;
    a.old_cols = a.cols >> a.old_shift;
    a.est = L.grid(s.to);
    a.lambda_mult = s.lambda_mult;
    a.list0 = c->list[0]; a.list1 = c->list[1];
    a.own = c->own;
    a.own_pitch = c->own_pitch;
    a.s_plane = L.plane_stride; a.s_old = L.grid_stride(a.old_grid); a.s_est = L.grid_stride(a.est);
    a.s_list = c->list_stride; a.s_own = c->own_stride; a.s_flag = (uint32_t)c->flag_bytes;
    a.local_rounds = c->tune.local_rounds;
    a.wide_threshold = (uint32_t)c->tune.wide_threshold;
    a.round_cap = s.round_cap;
    a.counters = c->counters;
    a.stats = stats ? 1 : 0;
    a.share = c->tune.solve_share ? 1 : 0;
    a.publish = s.publish >= 0 ? L.publish.get() : nullptr; a.publish_value = s.publish >= 0 ? (uint32_t)s.publish : 0u;
    if (s.memo) {
        a.memo = c->memo;
        a.s_memo = c->memo_stride;
        a.memo_init = !(c->memo_level == level && c->memo_block == b);
        a.memo_forward = c->tune.memo_forward ? 1 : 0;
        c->memo_level = level; c->memo_block = b;
    }
    uint8_t *const flags[2] = {c->flags[0], c->flags[1]};
    if (int rc = with_block<2, 4, 8, 16, 32, 64>(b, [&](auto B) {
            launch_sweep_t<B()>(a, s, flags, (unsigned)c->batch, c->stream);
            HIP_TRY(hipGetLastError());
            return (int)BBME_OK;
        })) return rc;
    L.cur_grid = a.est;
    L.cur_block = b;
    return BBME_OK;
}

int launch_expand(bbme_ctx *c)
{
    Level &L = c->lv[0];
    if (L.cur_block != 2) return bbme::fail(BBME_ERR_STATE, "level 0 has not been regularised down to 2x2 blocks");
    const int cc = L.width / 2, cr = L.height / 2;
    const long long threads = (long long)cc * cr * 2;
    hipLaunchKernelGGL(k_expand, dim3((unsigned)((threads + 255) / 256), (unsigned)c->batch), dim3(256), 0, c->stream,
                       L.cur_grid, cc, cr, c->flow, L.width, L.grid_stride(L.cur_grid), c->flow_stride);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

// Enqueues plan_pyramid's steps (launch_plan.hpp) on the context's streams.  `section(kind, level)` is called behind every search
// (kind 0), behind the last sweep of every level (1) and behind the expansion (2): the profiled path marks its events there.
// `spec_levels`: the levels whose search the sequence speculates (bbme_ctx::spec_levels).
template <class Section>
int walk_pyramid(bbme_ctx *c, bool speculate, uint32_t *spec_levels, Section &&section)
{
    const PlanInputs in = plan_inputs(c);
    const PyramidPlan plan = plan_pyramid(in, speculate);
    if (speculate && in.lv.size() > 1 && !c->side_stream) {   // only contexts that speculate hold a second stream (hardware queue)
        // lowest dispatch priority: the regulariser's workgroups on the main stream go first whenever both have some ready
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, lo));
    }
    c->memo_block = 0;                                  // a captured launch sequence must not depend on what ran before it
    *spec_levels = plan.spec_levels;
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const Step &s = plan.steps[i];
        Level &L = c->lv[s.level];
        switch (s.kind) {
        case Step::JoinFixup:
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
            [[fallthrough]];
        case Step::Search:
            if (int rc = launch_search(c, s.search)) return rc;
            if (int rc = section(0, s.level)) return rc;
            break;
        case Step::ForkSearch:
            HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
            HIP_TRY(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
            if (int rc = launch_search(c, s.search)) return rc;
            HIP_TRY(hipEventRecord(c->ev_join, c->side_stream));
            break;
        case Step::Sweep: {
            const SweepLaunch &w = s.sweep;
            if (int rc = launch_sweep(c, w)) return rc;
            if (w.publish >= 0) {                       // what set_late_grids hands the search: checked against the sweeps
                CoarseGrid table[kMaxCoarseGrids];
                const int n = fill_coarse_grids(table, L.width, L.block, fork_mult(c->tune) == 1, L.small[0], L.small[1], L.small_stride,
                                                L.big[0], L.big[1], L.big_stride);
                if (w.publish >= n || L.cur_grid != table[w.publish].grid || L.cur_block != 1 << table[w.publish].cell_shift)
                    return bbme::fail(BBME_ERR_STATE, "level %d: sweep %u behind the fork is not entry %u of the coarse grid table", s.level, (unsigned)w.publish, (unsigned)w.publish);
            }
            if (plan.steps[i + 1].kind != Step::Sweep && plan.steps[i + 1].kind != Step::ForkSearch)
                if (int rc = section(1, s.level)) return rc;
            break;
        }
        case Step::Expand:
            if (int rc = launch_expand(c)) return rc;
            if (int rc = section(2, 0)) return rc;
            break;
        }
    }
    return BBME_OK;
}

int enqueue_pyramid(bbme_ctx *c, bool speculate)
{
    return walk_pyramid(c, speculate, &c->spec_levels[c->direction], [](int, int) { return (int)BBME_OK; });
}

int profiled_pyramid(bbme_ctx *c)
{
    // eager launches, speculation off, with events between sections (rank-0 diagnostics; not the timed bench path)
    std::vector<DevEvent> ev;
    std::vector<int> kind;   // 0 search, 1 reg, 2 expand ; section i lies between ev[i] and ev[i+1]
    std::vector<int> lvl;
    auto mark = [&](int k, int l) -> int {
        ev.emplace_back();
        HIP_TRY(hipEventCreate(&ev.back().ev));
        HIP_TRY(hipEventRecord(ev.back(), c->stream));
        if (k >= 0) { kind.push_back(k); lvl.push_back(l); }
        return BBME_OK;
    };
    if (int rc = mark(-1, 0)) return rc;
    uint32_t none = 0;
    if (int rc = walk_pyramid(c, false, &none, mark)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->t_search = c->t_reg = c->t_expand = c->t_search0 = 0;
    for (size_t i = 0; i < kind.size(); ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        if (kind[i] == 0) { c->t_search += ms; if (lvl[i] == 0) c->t_search0 = ms; }
        else if (kind[i] == 1) c->t_reg += ms;
        else c->t_expand += ms;
    }
    HIP_TRY(hipEventElapsedTime(&c->t_total, ev.front(), ev.back()));
    return BBME_OK;
}

}  // namespace

// =========================================================================================
// C-ABI
// =========================================================================================
extern "C" {

int bbme_create(const bbme_params *params, int width, int height, int device, bbme_ctx **out)
{
    return bbme_create_batch(params, width, height, device, 1, out);
}

static int create_context(const bbme_params *params, int width, int height, int device, int pairs, bool chain, bbme_ctx **out)
{
    if (!params || !out) return bbme::fail(BBME_ERR_INVALID, "bbme_create: null argument");
    *out = nullptr;
    if (pairs < 1 || pairs > BBME_MAX_BATCH) return bbme::fail(BBME_ERR_INVALID, "batch of %d pairs (1..%d)", pairs, BBME_MAX_BATCH);
    if (int rc = validate_params(*params)) return rc;
    Geometry g;
    if (int rc = plan_padding(width, height, *params, g)) return rc;
    const int nl = params->num_levels;
    // grids with fewer than two blocks in a dimension make regularize_MVs read outside the
    // flow field in the reference (motion_framework.cpp:452-522): undefined there, refused here
    for (int l = 0; l < nl; ++l) {
        const int w = g.padded_width >> l, h = g.padded_height >> l, b = params->block_size[l];
        if (w / b < 2 || h / b < 2)
            return bbme::fail(BBME_ERR_DEGENERATE,
                              "level %d is %dx%d with %dx%d blocks: fewer than two blocks in a dimension "
                              "is undefined behaviour in the reference", l, w, h, b, b);
    }
    // the kernels move level rows as dwords (pitch == level width): with blocks of 4 x 4 and more every level width is a multiple
    // of four by construction, with 2 x 2 blocks it need not be
    for (int l = 0; l < nl; ++l)
        if ((g.padded_width >> l) % 4 != 0)
            return bbme::fail(BBME_ERR_UNSUPPORTED, "level %d is %d pixels wide: the kernels need level widths that are multiples of 4 "
                                                     "(2x2 blocks on a frame this narrow)", l, g.padded_width >> l);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return bbme::fail(BBME_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return bbme::fail(BBME_ERR_INVALID, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));

    // every return below destroys the half-built context, by the one path that sets the device first
    std::unique_ptr<bbme_ctx, int (*)(bbme_ctx *)> guard(new bbme_ctx(), bbme_destroy);
    bbme_ctx *c = guard.get();
    c->params = *params; c->geom = g; c->device = device;
    c->batch = pairs;
    c->chain = chain;
    c->slot_set.assign(c->frames(), 0);
    c->bgr_set.assign(c->frames(), 0);
    c->raw_stride = ((size_t)g.width * g.height + 64 + 255) / 256 * 256;
    c->tune = read_tuning(pairs);
    const size_t P = (size_t)pairs;
    auto round64 = [](size_t n) { return (n + 63) / 64 * 64; };
    c->lv.resize(nl);
    hipError_t err = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (err != hipSuccess) return bbme::fail(BBME_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(err));
    c->own_stream = true;
    if ((err = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess ||
        (err = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming)) != hipSuccess)
        return bbme::fail(BBME_ERR_HIP, "creating the side stream: %s", hipGetErrorString(err));
    size_t max_blocks = 0, max_plane = 0;
    for (int l = 0; l < nl; ++l) {
        Level &L = c->lv[l];
        char what[48], what_plan[48];                      // "allocating level 2: out of memory"
        snprintf(what, sizeof what, "level %d", l);
        snprintf(what_plan, sizeof what_plan, "search plan of level %d", l);
        L.width = g.padded_width >> l; L.height = g.padded_height >> l;
        L.block = params->block_size[l]; L.search = params->search_size[l];
        SpiralTable sp = build_spiral(L.search, L.block);
        L.range = sp.range; L.ncand = (int)sp.dx.size();
        L.pitch_dw = generic_pitch_dw(L.block, L.range);
        L.lds_bytes = generic_lds_bytes(L.block, L.range);
        const size_t plane = round64((size_t)L.width * L.height + 64) + 192;   // slack: row_sad may touch 3 bytes past the end
        const size_t cells = round64((size_t)(L.width / 2) * (L.height / 2));
        const size_t own_blocks = round64((size_t)(L.width / L.block) * (L.height / L.block));
        max_plane = std::max(max_plane, plane);             // (before the stride's cast: what s_plane is set from)
        L.plane_stride = (uint32_t)plane; L.small_stride = (uint32_t)own_blocks; L.big_stride = (uint32_t)cells;
        max_blocks = std::max(max_blocks, cells);
        std::vector<uint32_t> packed(sp.dx.size());
        for (size_t i = 0; i < sp.dx.size(); ++i)
            packed[i] = ((uint32_t)(uint16_t)sp.dx[i]) | ((uint32_t)(uint16_t)sp.dy[i] << 16);
        // a chain context: P + 1 frame slots, image 2 of pair p = image 1 of pair p + 1.  Otherwise the P image-1 planes, then the
        // P image-2 planes from the next multiple of 4 KiB on (the alignment an allocation of their own would give them)
        L.frame_step = chain ? plane : (P * plane + 4095) / 4096 * 4096;
        if (int rc = L.img1.alloc_zero(chain ? (P + 1) * plane : L.frame_step + P * plane, what)) return rc;
        L.img2 = L.img1 + L.frame_step;
        for (DevBuf<mv_t> *grid : {&L.small[0], &L.small[1], &L.pred})
            if (int rc = grid->alloc(P * own_blocks, what, Fill::poison)) return rc;
        if (int rc = L.fix_list.alloc(P * own_blocks, what, Fill::none)) return rc;
        if (int rc = L.fix_count.alloc_zero(P * 64 / sizeof(uint32_t), what)) return rc;    // 64 bytes per pair
        if (int rc = L.publish.alloc_zero(P * 64 / sizeof(uint32_t), what)) return rc;
        if (int rc = L.big[0].alloc_zero(P * cells, what)) return rc;
        if (int rc = L.big[1].alloc_zero(P * cells, what)) return rc;
        if (int rc = L.spiral.upload(packed, what)) return rc;
        // a speculative search of this level runs beside the sweeps of the next coarser one and pads its workgroups (search_lds_bytes)
        const int coarser_block = l + 1 < nl ? params->block_size[l + 1] : 0;
        if (!fast_kernel_serves(L.block, L.range)) {
            // the generic kernel (block 4 / 64, or a range beyond the strip kernel's packed keys): its window may need more LDS
            // than a kernel gets by default (raise_lds_limit below)
            if (L.lds_bytes > 160 * 1024)
                return bbme::fail(BBME_ERR_UNSUPPORTED, "level %d: a %dx%d block with range %d needs %zu bytes of LDS", l,
                                  L.block, L.block, L.range, L.lds_bytes);
        } else {
            // the strip kernel reads rank rows dy0 .. dy0+S-1 as 4 x u16 per column group
            SearchPlan plan = plan_search(L.range, L.block, L.block == 32 ? 8 : 16, 64, c->tune.loose_plan);
            L.fast = true;
            L.rank_pitch = sp.rank_pitch;
            L.nrounds = (int)plan.rounds.size();
            L.fast_pitch_dw = plan.pitch_dw;
            L.fast_lds_bytes = fast_lds_bytes(L.block, L.range, plan.pitch_dw);
            if (int rc = with_block<8, 16, 32>(L.block, [&](auto B) {
                    return raise_lds_limit(device, reinterpret_cast<const void *>(&k_search_fast<B(), 1>), search_lds_bytes(c->tune, L, true, l, coarser_block));
                })) return rc;
            // the device copy of a plan's round codes carries, for strip rounds, where the round's rank entries start in
            // lane_ranks (<< 16, in rows of T entries); lane_ranks itself: per strip round and lane the S entries of 4 ranks
            auto upload_plan = [&](const SearchPlan &p, int T, DevBuf<uint32_t> &d_tasks, DevBuf<uint32_t> &d_rounds, DevBuf<uint2> &d_ranks) -> int {
                std::vector<uint32_t> codes(p.rounds);
                std::vector<uint16_t> ranks;
                uint32_t cum = 0;
                for (size_t rd = 0; rd < p.rounds.size(); ++rd) {
                    if ((p.rounds[rd] >> 8) != 0) continue;
                    const uint32_t S = p.rounds[rd] & 0xffu;
                    if (cum > 0xffffu) return bbme::fail(BBME_ERR_STATE, "search plan of level %d: too many strip rows", l);
                    codes[rd] |= cum << 16;
                    for (int t = 0; t < T; ++t) {
                        const uint32_t task = p.tasks[rd * (size_t)T + t];
                        for (uint32_t d = 0; d < S; ++d)
                            for (int cc = 0; cc < 4; ++cc) {
                                uint16_t r = 0xffffu;                     // idle lane / padding column: masked in the kernel
                                if (task != 0xffffffffu) {
                                    const int dxi = 4 * (int)(task & 0xffu) + cc, dyi = (int)((task >> 8) & 0xffu) + (int)d;
                                    if (dyi > 2 * L.range)
                                        return bbme::fail(BBME_ERR_STATE, "search plan of level %d: a strip leaves the candidate square", l);
                                    if (dxi < sp.rank_pitch) r = sp.rank_of[(size_t)dyi * sp.rank_pitch + dxi];
                                }
                                ranks.push_back(r);
                            }
                    }
                    cum += S;
                }
                if (ranks.empty()) ranks.assign(4, 0xffffu);
                if (int rc = d_tasks.upload(p.tasks, what_plan)) return rc;
                if (int rc = d_rounds.upload(codes, what_plan)) return rc;
                return d_ranks.upload(ranks, what_plan, 64);
            };
            if (int rc = L.rank_of.upload(sp.rank_of, what_plan, 64)) return rc;
            if (int rc = upload_plan(plan, 64, L.tasks, L.rounds, L.lane_ranks)) return rc;
            // shorter strips, so that the 128 lanes of two waves have a full round of them
            SearchPlan plan2 = plan_search(L.range, L.block, 8, 128, c->tune.loose_plan);
            L.nrounds2 = (int)plan2.rounds.size();
            L.split_pays = split_shortens_walk(plan.rounds, plan2.rounds, L.block);
            if (plan2.pitch_dw != plan.pitch_dw) return bbme::fail(BBME_ERR_STATE, "search plans disagree on the window pitch");
            if (int rc = upload_plan(plan2, 128, L.tasks2, L.rounds2, L.lane_ranks2)) return rc;
        }
        // k_search_generic serves the levels above, and every level in raster mode or under BBME_GENERIC_SEARCH
        if (int rc = with_block<2, 4, 8, 16, 32, 64>(L.block, [&](auto B) {
                return raise_lds_limit(device, reinterpret_cast<const void *>(&k_search_generic<B()>), search_lds_bytes(c->tune, L, false, l, coarser_block));
            })) return rc;
    }
    c->memo_blocks = memo_room(c->tune, std::vector<PlanLevel>(c->lv.begin(), c->lv.end()));
    // pitch = 33 (mod 64) words: consecutive blocks land 132 bytes (mod 256) apart
    c->own_pitch = (uint32_t)(((max_blocks + 31) / 32 + 63) / 64 * 64 + 33);
    const size_t bit_words = (size_t)c->own_pitch * 32;
    c->flag_bytes = (max_blocks + 2047) / 2048 * 2048 + 2048;             // whole 16-flag segments (k_reg_solve), zero beyond the grid
    c->flow_stride = (size_t)g.padded_width * g.padded_height * 2;        // floats
    c->list_stride = (uint32_t)max_blocks; c->own_stride = (uint32_t)bit_words;
    // k_reg_solve addresses a pair's planes, grids, ownership words and flags with 32-bit byte offsets on the pair's 64-bit base
    // and multiplies rows by pitches in 24 bits (SolverArgs): every one of those buffers must end below 4 GiB per pair, every
    // dimension lie below 2^23 and the ownership map's pitch below 2^24
    {
        const size_t most = std::max(std::max(max_plane, max_blocks * sizeof(mv_t)), std::max(bit_words * sizeof(uint32_t), c->flag_bytes));
        if (most >= (1ull << 32) || c->lv[0].width >= (1 << 23) || c->lv[0].height >= (1 << 23) || c->own_pitch >= (1u << 24))
            return bbme::fail(BBME_ERR_UNSUPPORTED, "a %d x %d frame needs a per-pair buffer of %zu bytes: the solver's offsets are 32-bit",
                              c->lv[0].width, c->lv[0].height, most);
    }
    const char *work = "work buffers";
    if (int rc = c->flow.alloc_zero(P * c->flow_stride, work)) return rc;
    if (int rc = c->list[0].alloc(P * max_blocks, work, Fill::none)) return rc;
    if (int rc = c->list[1].alloc(P * max_blocks, work, Fill::none)) return rc;
    if (int rc = c->flags[0].alloc_zero(P * c->flag_bytes, work)) return rc;
    if (int rc = c->flags[1].alloc_zero(P * c->flag_bytes, work)) return rc;
    if (int rc = c->own.alloc_zero(P * bit_words, work)) return rc;
    if (int rc = c->counters.alloc_zero(P * 64, work)) return rc;
    if (c->memo_blocks) {
        c->memo_stride = (uint32_t)round64(c->memo_blocks << kMemoSlotShift);
        // every slot starts as "nothing known" (the MV half of the word is what counts: 0x80008000 is never a motion vector)
        if (int rc = c->memo.alloc(P * c->memo_stride, "the SAD memo", Fill::poison)) return rc;
        err = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(c->memo.get()), (int)kMemoNoMv, P * c->memo_stride * 2);
        if (err != hipSuccess) return bbme::fail(BBME_ERR_HIP, "allocating the SAD memo: %s", hipGetErrorString(err));
    }
    HIP_TRY(hipDeviceSynchronize());
    bbme::clear_error();
    *out = guard.release();
    return BBME_OK;
}

int bbme_create_batch(const bbme_params *params, int width, int height, int device, int pairs, bbme_ctx **out)
{
    return create_context(params, width, height, device, pairs, false, out);
}

int bbme_create_chain(const bbme_params *params, int width, int height, int device, int pairs, bbme_ctx **out)
{
    return create_context(params, width, height, device, pairs, true, out);
}

int bbme_destroy(bbme_ctx *c)
{
    if (!c) return BBME_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    drop_graph(c);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    for (hipEvent_t e : {c->ev_sub, c->ev_fork, c->ev_join})
        if (e) (void)hipEventDestroy(e);
    delete c;                                        // the buffers go with it (DevBuf)
    return BBME_OK;
}

int bbme_set_stream(bbme_ctx *c, void *hip_stream)
{
    if (int rc = check_ctx(c)) return rc;
    if (int rc = settle_and_drop_graphs(c)) return rc;
    if (c->own_stream) { (void)hipStreamDestroy(c->stream); c->own_stream = false; }
    c->stream = (hipStream_t)hip_stream;
    if (!c->stream) {
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return BBME_OK;
}

int bbme_set_search_mode(bbme_ctx *c, int mode)
{
    if (int rc = check_ctx(c)) return rc;
    if (mode != BBME_SEARCH_SPIRAL && mode != BBME_SEARCH_RASTER) return bbme::fail(BBME_ERR_INVALID, "search mode %d", mode);
    if (c->raster_search == (mode == BBME_SEARCH_RASTER)) return BBME_OK;
    if (int rc = settle_and_drop_graphs(c)) return rc;
    c->raster_search = mode == BBME_SEARCH_RASTER;
    return BBME_OK;
}

int bbme_set_regularizer_mode(bbme_ctx *c, int mode)
{
    if (int rc = check_ctx(c)) return rc;
    if (mode != BBME_REG_EXACT && mode != BBME_REG_JACOBI) return bbme::fail(BBME_ERR_INVALID, "regulariser mode %d", mode);
    if (c->jacobi == (mode == BBME_REG_JACOBI)) return BBME_OK;
    if (int rc = settle_and_drop_graphs(c)) return rc;
    c->jacobi = mode == BBME_REG_JACOBI;
    return BBME_OK;
}

int bbme_set_speculation(bbme_ctx *c, int enabled)
{
    if (int rc = check_ctx(c)) return rc;
    if (c->tune.speculate == (enabled != 0)) return BBME_OK;
    if (int rc = settle_and_drop_graphs(c)) return rc;
    c->tune.speculate = enabled != 0;
    if (!c->tune.speculate && c->side_stream) { (void)hipStreamDestroy(c->side_stream); c->side_stream = nullptr; }
    return BBME_OK;
}

int bbme_set_relaxation(bbme_ctx *c, int enabled)
{
    if (int rc = check_ctx(c)) return rc;
    if (c->relax == (enabled != 0)) return BBME_OK;
    if (int rc = settle_and_drop_graphs(c)) return rc;
    c->relax = enabled != 0;
    return BBME_OK;
}

int bbme_wait_for_stream(bbme_ctx *c, void *producer_stream)
{
    if (int rc = check_ctx(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(producer_stream));
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
    (void)hipEventDestroy(ev);                      // released once the recorded work has completed
    if (e != hipSuccess) return bbme::fail(BBME_ERR_HIP, "bbme_wait_for_stream: %s", hipGetErrorString(e));
    return BBME_OK;
}

int bbme_get_stream(bbme_ctx *c, void **hip_stream)
{
    if (int rc = check_ctx(c)) return rc;
    if (!hip_stream) return bbme::fail(BBME_ERR_INVALID, "null output");
    *hip_stream = c->stream;
    return BBME_OK;
}

int bbme_get_geometry(const bbme_ctx *c, int *pw, int *ph, int *px, int *py)
{
    if (int rc = check_ctx(c)) return rc;
    if (pw) *pw = c->geom.padded_width;
    if (ph) *ph = c->geom.padded_height;
    if (px) *px = c->geom.pad_x;
    if (py) *py = c->geom.pad_y;
    return BBME_OK;
}

int bbme_level_geometry(const bbme_ctx *c, int level, int *w, int *h, int *b, int *s)
{
    if (int rc = check_level(c, level)) return rc;
    const Level &L = c->lv[level];
    if (w) *w = L.width;
    if (h) *h = L.height;
    if (b) *b = L.block;
    if (s) *s = L.search;
    return BBME_OK;
}

// ---- frame setters: one check, one upload, one preparation path for every kind of context and of frame --------------------

namespace {

// WHICH FRAMES a setter writes: `count` slots from `first` on, `step` slots apart (bbme_ctx, "frame slots").  The two frames
// of a pair are a run of two with the step of a whole batch; a run of a chain context's slots has step 1.  At every level
// the set's first plane is img1 + first * plane_stride and its planes lie frame_step apart: that is what frame_step is.
struct FrameSet {
    int first, count, step;
    int slot(int i) const { return first + i * step; }
    uint8_t *planes(const Level &L) const { return L.img1 + (size_t)first * L.plane_stride; }
};
FrameSet frames_of_pair(const bbme_ctx *c, int pair) { return {pair, 2, c->batch}; }
FrameSet frames_of_run(int first, int count) { return {first, count, 1}; }

// What the frames of a setter are made of.  kNoFormat: a chain setter's `scale` that is neither 1 nor 4.
enum FrameFormat { kGrey, kGreyX4, kBgr, kNoFormat };
FrameFormat grey_format(int scale) { return scale == 1 ? kGrey : scale == 4 ? kGreyX4 : kNoFormat; }

// The arguments of every frame setter.  by_slot: a chain setter (`first`, `count` are slots of a chain context), else a pair
// setter (`first` is the pair, count 2).  Touches no device.
int check_frames(const bbme_ctx *c, bool by_slot, int first, int count, const uint8_t *const *frames, int pitch, FrameFormat fmt,
                 const char *what)
{
    if (int rc = by_slot ? chain_context_only(c, what) : pair_context_only(c, what)) return rc;
    const Geometry &g = c->geom;
    if (fmt == kNoFormat) return bbme::fail(BBME_ERR_INVALID, "%s: scale is neither 1 nor 4", what);
    if (fmt == kGreyX4 && (g.width % 4 || g.height % 4))
        return bbme::fail(BBME_ERR_INVALID, "%s: the context's frame (%dx%d) is not a multiple of 4 in both dimensions", what,
                          g.width, g.height);
    if (by_slot && (first < 0 || count < 1 || first > c->batch || count > c->batch + 1 - first))
        return bbme::fail(BBME_ERR_INVALID, "%s: slots %d .. %d of %d", what, first, first + count - 1, c->batch + 1);
    if (!by_slot && (first < 0 || first >= c->batch)) return bbme::fail(BBME_ERR_INVALID, "%s: pair %d of %d", what, first, c->batch);
    if (!frames) return bbme::fail(BBME_ERR_INVALID, "%s: null frame table", what);
    for (int i = 0; i < count; ++i)
        if (!frames[i]) return bbme::fail(BBME_ERR_INVALID, "%s: frame %d of the %s is null", what, i, by_slot ? "run" : "pair");
    const long long row = fmt == kBgr ? 3LL * g.width : fmt == kGreyX4 ? g.width / 4 : g.width;
    if (pitch < row) return bbme::fail(BBME_ERR_INVALID, "%s: pitch %d < %lld bytes of a frame's row", what, pitch, row);
    return BBME_OK;
}

// k_pyr_down4_run makes four output pixels per thread from 16-byte loads: the SOURCE level of a pyrDown must be a multiple of
// 8 pixels wide.  create_context refuses every level width that is not a multiple of 4, and a source level is twice the level
// below it, so this holds for every context there is; a geometry that broke it must fail here, not compute something.
int check_pyr_down_source(const Level &P, size_t level)
{
    if (P.width % 8 != 0)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "level %zu is %d pixels wide: pyrDown needs a source width that is a multiple of 8",
                          level, P.width);
    return BBME_OK;
}

// The frames of `set` from `src` in HBM (rows `pitch` bytes apart) into their planes of every level, one launch per level with
// every frame of the set in it (blockIdx.y): zero border -- with the x4 up-sampling (main_class.cpp:32-33; sources of a quarter
// of the frame) or the luma conversion fused in -- then MF::MF's pyrDown cascade (motion_framework.cpp:86-106).  kBgr with
// `keep`: the sources are a caller's and are copied into the set's slots of the colour store in the same pass; without, they
// ARE those slots.  And the bookkeeping of every frame setter.  No host wait: upload, border, pyramid and an estimate behind
// them overlap whatever the host does next.
int prepare_frames(bbme_ctx *c, FrameSet set, const FrameRun &src, int pitch, FrameFormat fmt, bool keep = false)
{
    const Geometry &g = c->geom;
    Level &L0 = c->lv[0];
    c->src_scale = fmt == kGreyX4 ? 4 : 1;
    const long long chunks = (long long)((L0.width + 15) / 16) * L0.height;
    const dim3 grid0((unsigned)((chunks + 255) / 256), (unsigned)set.count);
    if (fmt == kBgr)
        hipLaunchKernelGGL(k_bgr_pad_run, grid0, dim3(256), 0, c->stream, src, set.planes(L0), L0.frame_step,
                           keep ? c->bgr + (size_t)set.first * c->bgr_stride : nullptr, (size_t)set.step * c->bgr_stride, g.width,
                           g.height, pitch, g.pad_x, g.pad_y, L0.width, L0.height);
    else if (fmt == kGreyX4)
        hipLaunchKernelGGL(k_resize_x4_pad_run, grid0, dim3(256), 0, c->stream, src, set.planes(L0), L0.frame_step, g.width / 4,
                           g.height / 4, pitch, g.pad_x, g.pad_y, L0.width, L0.height);
    else
        hipLaunchKernelGGL(k_pad_zero_run, grid0, dim3(256), 0, c->stream, src, set.planes(L0), L0.frame_step, g.width, g.height,
                           pitch, g.pad_x, g.pad_y, L0.width, L0.height);
    for (size_t l = 1; l < c->lv.size(); ++l) {
        Level &P = c->lv[l - 1], &L = c->lv[l];
        if (int rc = check_pyr_down_source(P, l - 1)) return rc;
        const long long n = (long long)(L.width / 4) * L.height;
        hipLaunchKernelGGL(k_pyr_down4_run, dim3((unsigned)((n + 255) / 256), (unsigned)set.count), dim3(256), 0, c->stream,
                           set.planes(P), P.frame_step, set.planes(L), L.frame_step, P.width, P.height);
    }
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < set.count; ++i) {
        c->slot_set[set.slot(i)] = 1;
        c->bgr_set[set.slot(i)] = fmt == kBgr;
    }
    c->memo_block = 0;                                  // new planes: what the SAD memo holds is no longer true
    c->fields_valid = false;
    return BBME_OK;
}

// the colour store, allocated on first use: one packed frame per slot
int bgr_store(bbme_ctx *c)
{
    if (c->bgr.get()) return BBME_OK;
    c->bgr_stride = ((size_t)3 * c->geom.width * c->geom.height + 255) / 256 * 256;
    return c->bgr.alloc(c->bgr_stride * (size_t)c->frames(), "the colour store", Fill::poison);
}

// A device setter: frames in HBM.  B,G,R frames are kept (copied into the colour store).
int set_frames_device(bbme_ctx *c, bool by_slot, int first, int count, const uint8_t *const *d_frames, int pitch, FrameFormat fmt,
                      const char *what)
{
    if (int rc = check_frames(c, by_slot, first, count, d_frames, pitch, fmt, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (fmt == kBgr) if (int rc = bgr_store(c)) return rc;
    FrameRun run{};
    for (int i = 0; i < count; ++i) run.src[i] = d_frames[i];
    return prepare_frames(c, by_slot ? frames_of_run(first, count) : frames_of_pair(c, first), run, pitch, fmt, fmt == kBgr);
}

// A host setter: every frame crosses PCIe once, packed, on the context's stream -- grey frames as they are into their slots of
// the upload buffer (room for the context's frame size; x4 sources are a sixteenth of that), B,G,R frames straight into their
// slots of the colour store, where the conversion reads them and where they stay.  Border and cascade run in HBM (the same
// integers as bbme_pad_zero_host / bbme_pyr_down_host, without 18 ms of single-threaded host filtering at 4K).  The caller's
// buffers must stay untouched until the context's stream has passed this point.
int set_frames_host(bbme_ctx *c, bool by_slot, int first, int count, const uint8_t *const *frames, int pitch, FrameFormat fmt,
                    const char *what)
{
    if (int rc = check_frames(c, by_slot, first, count, frames, pitch, fmt, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const FrameSet set = by_slot ? frames_of_run(first, count) : frames_of_pair(c, first);
    const Geometry &g = c->geom;
    const int scale = fmt == kGreyX4 ? 4 : 1;
    const size_t row = (size_t)(fmt == kBgr ? 3 : 1) * (g.width / scale), rows = (size_t)(g.height / scale);
    if (int rc = fmt == kBgr ? bgr_store(c) : c->raw.ensure(c->raw_stride * (size_t)c->frames(), "the upload buffer", Fill::poison)) return rc;
    FrameRun run{};
    for (int i = 0; i < count; ++i) {
        uint8_t *d = fmt == kBgr ? c->bgr + (size_t)set.slot(i) * c->bgr_stride : c->raw + (size_t)set.slot(i) * c->raw_stride;
        c->bgr_set[set.slot(i)] = 0;                        // the store's slot, or the plane it described, is being overwritten
        HIP_TRY(hipMemcpy2DAsync(d, row, frames[i], (size_t)pitch, row, rows, hipMemcpyHostToDevice, c->stream));
        run.src[i] = d;
    }
    return prepare_frames(c, set, run, (int)row, fmt);
}

// The blocking form of a host setter: on return the caller may re-use its buffers
int then_wait(bbme_ctx *c, int rc)
{
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BBME_OK;
}

}  // namespace

int bbme_set_frames_device_pair(bbme_ctx *c, int pair, const uint8_t *d_image1, const uint8_t *d_image2, int pitch)
{
    const uint8_t *const frames[2] = {d_image1, d_image2};
    return set_frames_device(c, false, pair, 2, frames, pitch, kGrey, "bbme_set_frames_device");
}

int bbme_set_frames_device(bbme_ctx *c, const uint8_t *d_image1, const uint8_t *d_image2, int pitch)
{
    return bbme_set_frames_device_pair(c, 0, d_image1, d_image2, pitch);
}

int bbme_set_frames_host_async(bbme_ctx *c, int pair, const uint8_t *image1, const uint8_t *image2, int pitch)
{
    const uint8_t *const frames[2] = {image1, image2};
    return set_frames_host(c, false, pair, 2, frames, pitch, kGrey, "bbme_set_frames_host");
}

int bbme_set_frames_host_pair(bbme_ctx *c, int pair, const uint8_t *image1, const uint8_t *image2, int pitch)
{
    return then_wait(c, bbme_set_frames_host_async(c, pair, image1, image2, pitch));
}

int bbme_set_frames_host(bbme_ctx *c, const uint8_t *image1, const uint8_t *image2, int pitch)
{
    return bbme_set_frames_host_pair(c, 0, image1, image2, pitch);
}

int bbme_set_frames_device_x4(bbme_ctx *c, int pair, const uint8_t *d_image1, const uint8_t *d_image2, int pitch)
{
    const uint8_t *const frames[2] = {d_image1, d_image2};
    return set_frames_device(c, false, pair, 2, frames, pitch, kGreyX4, "bbme_set_frames_device_x4");
}

int bbme_set_frames_host_x4_async(bbme_ctx *c, int pair, const uint8_t *image1, const uint8_t *image2, int pitch)
{
    const uint8_t *const frames[2] = {image1, image2};
    return set_frames_host(c, false, pair, 2, frames, pitch, kGreyX4, "bbme_set_frames_host_x4");
}

int bbme_set_frames_host_x4(bbme_ctx *c, int pair, const uint8_t *image1, const uint8_t *image2, int pitch)
{
    return then_wait(c, bbme_set_frames_host_x4_async(c, pair, image1, image2, pitch));
}

int bbme_set_frames_device_bgr(bbme_ctx *c, int pair, const uint8_t *d_image1, const uint8_t *d_image2, int pitch)
{
    const uint8_t *const frames[2] = {d_image1, d_image2};
    return set_frames_device(c, false, pair, 2, frames, pitch, kBgr, "bbme_set_frames_device_bgr");
}

int bbme_set_frames_host_bgr_async(bbme_ctx *c, int pair, const uint8_t *image1, const uint8_t *image2, int pitch)
{
    const uint8_t *const frames[2] = {image1, image2};
    return set_frames_host(c, false, pair, 2, frames, pitch, kBgr, "bbme_set_frames_host_bgr");
}

int bbme_set_frames_host_bgr(bbme_ctx *c, int pair, const uint8_t *image1, const uint8_t *image2, int pitch)
{
    return then_wait(c, bbme_set_frames_host_bgr_async(c, pair, image1, image2, pitch));
}

int bbme_set_chain_frames_device(bbme_ctx *c, int first, int count, const uint8_t *const *d_frames, int pitch, int scale)
{
    return set_frames_device(c, true, first, count, d_frames, pitch, grey_format(scale), "bbme_set_chain_frames_device");
}

int bbme_set_chain_frames_host_async(bbme_ctx *c, int first, int count, const uint8_t *const *frames, int pitch, int scale)
{
    return set_frames_host(c, true, first, count, frames, pitch, grey_format(scale), "bbme_set_chain_frames_host");
}

int bbme_set_chain_frames_host(bbme_ctx *c, int first, int count, const uint8_t *const *frames, int pitch, int scale)
{
    return then_wait(c, bbme_set_chain_frames_host_async(c, first, count, frames, pitch, scale));
}

int bbme_set_chain_frames_device_bgr(bbme_ctx *c, int first, int count, const uint8_t *const *d_frames, int pitch)
{
    return set_frames_device(c, true, first, count, d_frames, pitch, kBgr, "bbme_set_chain_frames_device_bgr");
}

int bbme_set_chain_frames_host_bgr_async(bbme_ctx *c, int first, int count, const uint8_t *const *frames, int pitch)
{
    return set_frames_host(c, true, first, count, frames, pitch, kBgr, "bbme_set_chain_frames_host_bgr");
}

int bbme_set_chain_frames_host_bgr(bbme_ctx *c, int first, int count, const uint8_t *const *frames, int pitch)
{
    return then_wait(c, bbme_set_chain_frames_host_bgr_async(c, first, count, frames, pitch));
}

// ---- chain contexts: frames by slot, rolled forward through a video ----------------------------------------------------

int bbme_chain_frames(const bbme_ctx *c, int *frames)
{
    if (int rc = check_ctx(c)) return rc;
    if (!frames) return bbme::fail(BBME_ERR_INVALID, "null output");
    *frames = c->chain ? c->batch + 1 : 0;
    return BBME_OK;
}

int bbme_chain_advance(bbme_ctx *c)
{
    if (int rc = chain_context_only(c, "bbme_chain_advance")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the planes of the last slot, all levels, become slot 0: one copy launch behind whatever still reads the slots
    ChainRoll r{};
    uint32_t most = 0;
    for (size_t l = 0; l < c->lv.size(); ++l) {
        Level &L = c->lv[l];
        r.src[l] = reinterpret_cast<const uint4 *>(L.img1 + (size_t)c->batch * L.plane_stride);
        r.dst[l] = reinterpret_cast<uint4 *>(L.img1.get());
        r.n16[l] = L.plane_stride / 16;
        most = std::max(most, r.n16[l]);
    }
    const unsigned wgs = std::max(1u, std::min(2048u, (most + 255u) / 256u));
    hipLaunchKernelGGL(k_chain_roll, dim3(wgs, (unsigned)c->lv.size()), dim3(256), 0, c->stream, r);
    HIP_TRY(hipGetLastError());
    // slot 0 takes the last slot's flags (it is as set as the slot it came from), the rest are cleared
    const uint8_t had_last = c->slot_set[c->batch], had_bgr = c->bgr_set[c->batch];
    c->slot_set.assign(c->slot_set.size(), 0);
    c->bgr_set.assign(c->bgr_set.size(), 0);
    c->slot_set[0] = had_last;
    c->memo_block = 0;
    c->fields_valid = false;
    if (had_bgr) {                                      // the last slot's colour goes with its planes; slot 0 has colour once the copy is enqueued
        HIP_TRY(hipMemcpyAsync(c->bgr.get(), c->bgr + (size_t)c->batch * c->bgr_stride, c->bgr_stride, hipMemcpyDeviceToDevice,
                               c->stream));
        c->bgr_set[0] = 1;
    }
    return BBME_OK;
}

int bbme_get_chain_plane_host(bbme_ctx *c, int level, int slot, uint8_t *image)
{
    const char *what = "bbme_get_chain_plane_host";
    if (int rc = chain_context_only(c, what)) return rc;
    if (int rc = check_level(c, level)) return rc;
    if (slot < 0 || slot > c->batch) return bbme::fail(BBME_ERR_INVALID, "%s: slot %d of %d", what, slot, c->batch + 1);
    if (!image) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    HIP_TRY(hipSetDevice(c->device));
    const Level &L = c->lv[level];
    HIP_TRY(hipMemcpyAsync(image, L.img1 + (size_t)slot * L.plane_stride, (size_t)L.width * L.height, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BBME_OK;
}

int bbme_level_planes_device(bbme_ctx *c, int level, uint8_t **d1, uint8_t **d2)
{
    if (int rc = single_pair_only(c, "bbme_level_planes_device")) return rc;
    if (int rc = check_level(c, level)) return rc;
    if (d1) *d1 = c->lv[level].img1.get();
    if (d2) *d2 = c->lv[level].img2;
    c->slot_set[0] = c->slot_set[1] = 1;    // the caller fills them in place (the one pair's frames are slots 0 and 1 on either kind of context)
    c->memo_block = 0;
    return BBME_OK;
}

int bbme_set_level_planes_host(bbme_ctx *c, int level, const uint8_t *image1, const uint8_t *image2)
{
    if (int rc = single_pair_only(c, "bbme_set_level_planes_host")) return rc;
    if (int rc = check_level(c, level)) return rc;
    if (!image1 || !image2) return bbme::fail(BBME_ERR_INVALID, "null plane");
    HIP_TRY(hipSetDevice(c->device));
    Level &L = c->lv[level];
    HIP_TRY(hipMemcpyAsync(L.img1, image1, (size_t)L.width * L.height, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(L.img2, image2, (size_t)L.width * L.height, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->slot_set[0] = c->slot_set[1] = 1;                // the one pair's frames: slots 0 and 1 on either kind of context
    c->bgr_set[0] = c->bgr_set[1] = 0;
    c->memo_block = 0;
    c->fields_valid = false;
    return BBME_OK;
}

int bbme_get_level_planes_host(bbme_ctx *c, int level, uint8_t *image1, uint8_t *image2)
{
    if (int rc = single_pair_only(c, "bbme_get_level_planes_host")) return rc;
    if (int rc = check_level(c, level)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Level &L = c->lv[level];
    if (image1) HIP_TRY(hipMemcpyAsync(image1, L.img1, (size_t)L.width * L.height, hipMemcpyDeviceToHost, c->stream));
    if (image2) HIP_TRY(hipMemcpyAsync(image2, L.img2, (size_t)L.width * L.height, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BBME_OK;
}

// bbme_estimate in the context's current direction (one captured graph per direction)
static int run_pyramid(bbme_ctx *c)
{
    c->last_spec_levels = 0;
    if (c->profiling) { const int rc = profiled_pyramid(c); c->memo_block = 0; return rc; }
    if (!c->tune.use_graph) {
        const int rc = enqueue_pyramid(c, c->tune.speculate);
        c->memo_block = 0;
        c->last_spec_levels = c->spec_levels[c->direction];
        return rc;
    }
    hipGraphExec_t &exec = c->graph_exec[c->direction];
    if (!exec) {
        // the launch sequence is fixed (no host decisions inside), so capture it once
        hipGraph_t graph = nullptr;
        bool fork = c->tune.speculate;                      // (see bbme_ctx::graph_forked)
        if (!c->tune.fork_both) {
            if (c->direction == BBME_DIR_BACKWARD && c->graph_exec[BBME_DIR_FORWARD]) fork = false;
            if (c->direction == BBME_DIR_FORWARD && c->graph_exec[BBME_DIR_BACKWARD] && c->graph_forked[BBME_DIR_BACKWARD]) {
                HIP_TRY(hipStreamSynchronize(c->stream));          // once per context: the graph may still be running
                (void)hipGraphExecDestroy(c->graph_exec[BBME_DIR_BACKWARD]);
                c->graph_exec[BBME_DIR_BACKWARD] = nullptr;
                c->graph_forked[BBME_DIR_BACKWARD] = false;
            }
        }
        c->graph_forked[c->direction] = fork;
        HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        int rc = enqueue_pyramid(c, fork);
        hipError_t e = hipStreamEndCapture(c->stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) return bbme::fail(BBME_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { exec = nullptr; return bbme::fail(BBME_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
    } else {
        // keep the host-side grid bookkeeping in step with what the graph replays
        for (Level &L : c->lv) { L.cur_grid = L.final_grid(); L.cur_block = 2; }
    }
    HIP_TRY(hipGraphLaunch(exec, c->stream));
    c->last_spec_levels = c->spec_levels[c->direction];
    // after a pyramid the memo describes level 0 at its last memoised block size; a later stage call starts afresh
    c->memo_block = 0;
    return BBME_OK;
}

int bbme_estimate(bbme_ctx *c)
{
    if (int rc = check_ctx(c)) return rc;
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "bbme_estimate: no frames set (every pair of a batch needs its frames)");
    HIP_TRY(hipSetDevice(c->device));
    c->fields_valid = false;
    return run_pyramid(c);
}

// The grids and the SAD memo describe one direction's problem: the other direction starts as after bbme_create.
static void switch_direction(bbme_ctx *c, int dir)
{
    if (c->direction == dir) return;
    c->direction = dir;
    for (Level &L : c->lv) { L.cur_grid = nullptr; L.cur_block = 0; }
    c->memo_block = 0;
    c->fields_valid = false;
}

int bbme_set_direction(bbme_ctx *c, int dir)
{
    if (int rc = check_ctx(c)) return rc;
    if (dir != BBME_DIR_FORWARD && dir != BBME_DIR_BACKWARD) return bbme::fail(BBME_ERR_INVALID, "direction %d (0 or 1)", dir);
    switch_direction(c, dir);
    return BBME_OK;
}

int bbme_get_direction(const bbme_ctx *c, int *dir)
{
    if (int rc = check_ctx(c)) return rc;
    if (!dir) return bbme::fail(BBME_ERR_INVALID, "null output");
    *dir = c->direction;
    return BBME_OK;
}

int bbme_estimate_bidirectional(bbme_ctx *c)
{
    if (int rc = check_ctx(c)) return rc;
    if (!c->frames_set())
        return bbme::fail(BBME_ERR_STATE, "bbme_estimate_bidirectional: no frames set (every pair of a batch needs its frames)");
    HIP_TRY(hipSetDevice(c->device));
    const Level &L0 = c->lv[0];
    const uint32_t stride = L0.grid_stride(L0.final_grid());
    if (int rc = c->bwd_cells.ensure((size_t)stride * c->batch, "the backward cells", Fill::poison)) return rc;
    c->bwd_stride = stride;
    // backward pyramid, its final grid of every pair into the backward cells, forward pyramid: all on the ctx stream, in order
    switch_direction(c, BBME_DIR_BACKWARD);
    int rc = run_pyramid(c);
    if (rc == BBME_OK) {
        hipError_t e = hipMemcpyAsync(c->bwd_cells, L0.final_grid(), (size_t)stride * c->batch * sizeof(mv_t), hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) rc = bbme::fail(BBME_ERR_HIP, "copying the backward cells: %s", hipGetErrorString(e));
    }
    switch_direction(c, BBME_DIR_FORWARD);
    if (rc) return rc;
    if ((rc = run_pyramid(c))) return rc;
    c->fields_valid = true;
    return BBME_OK;
}

int bbme_synchronize(bbme_ctx *c)
{
    if (int rc = check_ctx(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return check_converged(c);
}

int bbme_batch_size(const bbme_ctx *c, int *pairs)
{
    if (int rc = check_ctx(c)) return rc;
    if (!pairs) return bbme::fail(BBME_ERR_INVALID, "null output");
    *pairs = c->batch;
    return BBME_OK;
}

static int check_pair(const bbme_ctx *c, int pair)
{
    if (int rc = check_ctx(c)) return rc;
    if (pair < 0 || pair >= c->batch) return bbme::fail(BBME_ERR_INVALID, "pair %d of a batch of %d", pair, c->batch);
    return BBME_OK;
}

int bbme_flow_device(bbme_ctx *c, const float **d_flow) { return bbme_flow_device_pair(c, 0, d_flow); }

int bbme_flow_device_pair(bbme_ctx *c, int pair, const float **d_flow)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (!d_flow) return bbme::fail(BBME_ERR_INVALID, "null output");
    *d_flow = c->flow + (size_t)pair * c->flow_stride;
    return BBME_OK;
}

int bbme_get_flow_host(bbme_ctx *c, float *flow) { return bbme_get_flow_host_pair(c, 0, flow); }

int bbme_get_flow_host_pair(bbme_ctx *c, int pair, float *flow)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (!flow) return bbme::fail(BBME_ERR_INVALID, "null output");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(flow, c->flow + (size_t)pair * c->flow_stride, c->flow_stride * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return check_converged(c);
}

int bbme_get_cells_host(bbme_ctx *c, int16_t *cells) { return bbme_get_cells_host_pair(c, 0, cells); }

int bbme_get_cells_host_pair(bbme_ctx *c, int pair, int16_t *cells)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (!cells) return bbme::fail(BBME_ERR_INVALID, "null output");
    Level &L = c->lv[0];
    if (L.cur_block != 2) return bbme::fail(BBME_ERR_STATE, "level 0 is not at 2x2 cells");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)(L.width / 2) * (L.height / 2);
    HIP_TRY(hipMemcpyAsync(cells, L.cur_grid + (size_t)pair * L.grid_stride(L.cur_grid), n * sizeof(mv_t), hipMemcpyDeviceToHost, c->stream));
    return check_converged(c);
}

int bbme_cells_device(bbme_ctx *c, const int16_t **d_cells) { return bbme_cells_device_pair(c, 0, d_cells); }

int bbme_cells_device_pair(bbme_ctx *c, int pair, const int16_t **d_cells)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (!d_cells) return bbme::fail(BBME_ERR_INVALID, "null output");
    // two sweeps per block size always leave the final field of a level in the same buffer (Level::final_grid)
    const Level &L = c->lv[0];
    *d_cells = reinterpret_cast<const int16_t *>(L.final_grid() + (size_t)pair * L.grid_stride(L.final_grid()));
    return BBME_OK;
}

int bbme_expand_cells_device(bbme_ctx *c, const int16_t *d_cells, float *d_flow)
{
    return bbme_expand_cells_device_on(c, d_cells, d_flow, nullptr);
}

int bbme_expand_cells_device_on(bbme_ctx *c, const int16_t *d_cells, float *d_flow, void *hip_stream)
{
    if (int rc = check_ctx(c)) return rc;
    if (!d_cells || !d_flow) return bbme::fail(BBME_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(c->device));
    Level &L = c->lv[0];
    const int cc = L.width / 2, cr = L.height / 2;
    const long long threads = (long long)cc * cr * 2;
    hipLaunchKernelGGL(k_expand, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream,
                       reinterpret_cast<const mv_t *>(d_cells), cc, cr, d_flow, L.width, 0u, (size_t)0);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

int bbme_calculate_mse_device(bbme_ctx *c, const float *d_gtruth, int gt_width, int gt_height, int scale, double *out)
{
    if (int rc = single_pair_only(c, "bbme_calculate_mse_device")) return rc;
    if (int rc = check_ctx(c)) return rc;
    if (!d_gtruth || !out || gt_width < 1 || gt_height < 1 || scale < 1)
        return bbme::fail(BBME_ERR_INVALID, "bbme_calculate_mse_device: bad arguments");
    Level &L = c->lv[0];
    if (L.cur_block != 2) return bbme::fail(BBME_ERR_STATE, "level 0 has not been regularised down to 2x2 blocks");
    if ((long long)(gt_width - 1) * scale >= c->geom.width || (long long)(gt_height - 1) * scale >= c->geom.height)
        return bbme::fail(BBME_ERR_INVALID, "ground truth %dx%d at scale %d does not fit the %dx%d frame",
                          gt_width, gt_height, scale, c->geom.width, c->geom.height);
    HIP_TRY(hipSetDevice(c->device));
    constexpr int kMaxGroups = 512;
    const long long n = (long long)gt_width * gt_height;
    const int groups = (int)std::min<long long>(kMaxGroups, (n + 255) / 256);
    static_assert(sizeof(double) == sizeof(unsigned long long), "sums and counts share the scratch");
    if (int rc = c->epe_scratch.ensure(2 * kMaxGroups, "the EPE scratch", Fill::poison)) return rc;
    double *d_sum = c->epe_scratch;
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(d_sum + kMaxGroups);
    hipLaunchKernelGGL(k_epe, dim3(groups), dim3(256), 0, c->stream, L.cur_grid, L.width / 2,
                       c->geom.pad_x, c->geom.pad_y, scale, d_gtruth, gt_width, gt_height, d_sum, d_cnt);
    std::vector<double> h_sum(kMaxGroups);
    std::vector<unsigned long long> h_cnt(kMaxGroups);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(h_sum.data(), d_sum, groups * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h_cnt.data(), d_cnt, groups * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (err != hipSuccess) return bbme::fail(BBME_ERR_HIP, "bbme_calculate_mse_device: %s", hipGetErrorString(err));
    if (int rc = check_converged(c)) return rc;
    double error = 0;
    unsigned long long count = 0;
    for (int i = 0; i < groups; ++i) { error += h_sum[i]; count += h_cnt[i]; }
    *out = error / (double)count;                     // 0/0 = NaN when no pixel is known, as in the reference (:330)
    return BBME_OK;
}

// main_class.cpp:58-70 from the cell grid: the ceil(W/s) x ceil(H/s) field at every s-th pixel of the unpadded frame, / s
static int enqueue_subsample(bbme_ctx *c, int pair, int scale, float *d_out, int out_pitch, void *hip_stream, const char *what)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (!d_out || scale < 1) return bbme::fail(BBME_ERR_INVALID, "%s: null output or scale %d < 1", what, scale);
    const int ow = (c->geom.width + scale - 1) / scale, oh = (c->geom.height + scale - 1) / scale;
    if (out_pitch < ow) return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < width %d", what, out_pitch, ow);
    const Level &L = c->lv[0];
    if (L.cur_block != 2) return bbme::fail(BBME_ERR_STATE, "%s: level 0 has not been regularised down to 2x2 blocks", what);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    const long long n = (long long)ow * oh;
    hipLaunchKernelGGL(k_subsample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       L.cur_grid + (size_t)pair * L.grid_stride(L.cur_grid), L.width / 2, c->geom.pad_x, c->geom.pad_y, scale,
                       d_out, ow, oh, out_pitch, 0u, (size_t)0);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

int bbme_subsampled_flow_device(bbme_ctx *c, int pair, int scale, float *d_out, int out_pitch_pixels, void *hip_stream)
{
    if (int rc = check_ctx(c)) return rc;
    return enqueue_subsample(c, pair, scale, d_out, out_pitch_pixels, hip_stream, "bbme_subsampled_flow_device");
}

}  // extern "C": the stages from here on share templates, which need C++ linkage; their entry points have C linkage from bbme.h

// ---- what the gather stages share (bbme_kernels.hpp: compensation, K6 consistency, K7 / K7b interpolation, K9 / K9b temporal filter, K11 .. K15) ----
// Every stage is one launch in which a lane takes runs of 4 units (pixels or cells) along a row, over (workgroups, pairs, phases
// or frames), with optional statistics: the kernel's partials, then k_mc_reduce.  One run split, one launch path, one scratch
// layout, one pair of output checks and one pair of download helpers serve all of them.

// workgroups of a launch whose lanes take up to runs_per_lane runs each
static long long gather_groups(int units_per_row, int rows, int runs_per_lane)
{
    return ((long long)(units_per_row + 3) / 4 * rows + 256 * runs_per_lane - 1) / (256 * runs_per_lane);
}

// the stages on level 0's 2x2 cells
static long long cell_groups(const bbme_ctx *c, int runs_per_lane)
{
    return gather_groups(c->lv[0].width / 2, c->lv[0].height / 2, runs_per_lane);
}

template <class Args>
static void set_runs(Args &a, int units_per_row, int rows)
{
    a.runs_per_row = (units_per_row + 3) / 4;
    a.runs = (long long)a.runs_per_row * rows;
}

// `kernel` over (groups, pairs, count) and, with d_stats, k_mc_reduce of its partials at `partial` into d_stats[4 (y count + z) ..]
// (k_interpolate: 4 (z pairs + y))
template <class Args>
static int launch_gather(void (*kernel)(Args), Args &a, long long groups, int pairs, int count, unsigned long long *partial,
                         unsigned long long *d_stats, hipStream_t stream)
{
    a.partial = d_stats ? partial : nullptr;
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups, (unsigned)pairs, (unsigned)count), dim3(256), 0, stream, a);
    if (d_stats) hipLaunchKernelGGL(k_mc_reduce, dim3((unsigned)(pairs * count)), dim3(256), 0, stream, a.partial, (int)groups, d_stats);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

// A frame or map that a caller brings: pitch at least a row; with more than one frame, stride at least a frame.  Touches no device.
static int check_frames(int count, int pitch, size_t stride, int min_pitch, int rows, const char *what, const char *which)
{
    if (pitch < min_pitch) return bbme::fail(BBME_ERR_INVALID, "%s: %s pitch %d < %d", what, which, pitch, min_pitch);
    if (count > 1 && stride < (size_t)pitch * rows)
        return bbme::fail(BBME_ERR_INVALID, "%s: %s stride %zu < one frame of %d rows of %d bytes", what, which, stride, rows, pitch);
    return BBME_OK;
}

// the same of B,G,R frames of the context's size
static int check_bgr_frames(const bbme_ctx *c, int count, int pitch, size_t stride, const char *what)
{
    if ((long long)pitch < 3LL * c->geom.width)
        return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < 3 x frame width %d", what, pitch, c->geom.width);
    return check_frames(count, pitch, stride, pitch, c->geom.height, what, "output");
}

// A frame is written while other lanes still gather from the inputs: an output inside an input is a race, not a result.
// Frames of `rows` rows of row_bytes, the output's out_pitch and the inputs' in_pitch bytes apart; a null input is absent.
static bool overlaps_input(const uint8_t *d_out, int out_pitch, std::initializer_list<const uint8_t *> inputs, int in_pitch,
                           int row_bytes, int rows)
{
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + (size_t)out_pitch * (rows - 1) + (size_t)row_bytes;
    for (const uint8_t *in : inputs) {
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + (size_t)in_pitch * (rows - 1) + (size_t)row_bytes;
        if (in && o0 < i1 && i0 < o1) return true;
    }
    return false;
}

// the forward and the backward 2x2 cells of `pair` of the context's own bidirectional estimate
static void own_fields(const bbme_ctx *c, int pair, const mv_t **f, const mv_t **b)
{
    const Level &L = c->lv[0];
    *f = L.final_grid() + (size_t)pair * L.grid_stride(L.final_grid());
    *b = c->bwd_cells + (size_t)pair * c->bwd_stride;
}

// One more device-to-host copy that rides on a host getter's wait (bbme_get_flow_color_host: the five range floats)
struct ExtraCopy { void *dst = nullptr; const void *src = nullptr; size_t bytes = 0; };

// What the host getters share: n elements of T in the context's staging area, filled by enqueue(T *, scratch) on the context's
// stream and copied down to `out`; waits.  `scratch` is a second region of scratch_bytes at a 256-byte-aligned offset behind
// them, for a product made in two steps.  n = 0: nothing is staged or copied and enqueue gets null.
template <class T, class Enqueue>
static int download_staged_with_scratch(bbme_ctx *c, size_t n, const char *what, T *out, size_t scratch_bytes, Enqueue enqueue,
                                        ExtraCopy extra = {})
{
    const size_t bytes = n * sizeof(T), scratch_at = (bytes + 255) / 256 * 256;
    uint8_t *area;
    if (int rc = c->staged(scratch_bytes ? scratch_at + scratch_bytes : bytes, what, &area)) return rc;
    T *d = n ? reinterpret_cast<T *>(area) : nullptr;
    if (int rc = enqueue(d, area + scratch_at)) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream));
    if (extra.bytes) HIP_TRY(hipMemcpyAsync(extra.dst, extra.src, extra.bytes, hipMemcpyDeviceToHost, c->stream));
    return check_converged(c);
}

template <class T, class Enqueue>
static int download_staged(bbme_ctx *c, size_t n, const char *what, T *out, Enqueue enqueue, ExtraCopy extra = {})
{
    return download_staged_with_scratch(c, n, what, out, 0, [&](T *d, uint8_t *) { return enqueue(d); }, extra);
}

// What the statistics calls share: enqueue() on the context's stream, the first n result quadruples of `s` copied down; waits.
template <class Enqueue>
static int download_stats(bbme_ctx *c, const StatsScratch &s, int n, unsigned long long *stats, Enqueue enqueue)
{
    if (int rc = enqueue()) return rc;
    HIP_TRY(hipMemcpyAsync(stats, s.results(), (size_t)4 * sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
    return check_converged(c);
}

int bbme_get_subsampled_flow_host(bbme_ctx *c, int pair, int scale, float *out)
{
    const char *what = "bbme_get_subsampled_flow_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (!out || scale < 1) return bbme::fail(BBME_ERR_INVALID, "%s: null output or scale %d < 1", what, scale);
    if (c->lv[0].cur_block != 2) return bbme::fail(BBME_ERR_STATE, "%s: level 0 has not been regularised down to 2x2 blocks", what);
    const int ow = (c->geom.width + scale - 1) / scale, oh = (c->geom.height + scale - 1) / scale;
    return download_staged(c, (size_t)ow * oh * 2, "the subsampled field", out, [&](float *d) {
        return enqueue_subsample(c, pair, scale, d, ow, nullptr, what);
    });
}

// ---- motion compensation: MF::draw_MVimage (motion_framework.cpp:887-905) and its residual statistics ---------------------

// The arguments every motion-compensation entry point shares (include/bbme.h): level, block size, fill and window are valid,
// and the level has a grid.  Touches no device.
static int check_mc(const bbme_ctx *c, int level, int block, int fill, const int *window, const char *what)
{
    if (int rc = check_level(c, level)) return rc;
    const Level &L = c->lv[level];
    if (block < 1 || block > L.block || (block & (block - 1)))
        return bbme::fail(BBME_ERR_INVALID, "%s: block %d is not a power of two in 1..%d", what, block, L.block);
    if (fill < 0 || fill > 255) return bbme::fail(BBME_ERR_INVALID, "%s: fill %d outside 0..255", what, fill);
    return check_window(window, L.width, L.height, what, level);
}

static int check_mc_state(const bbme_ctx *c, int level, const char *what)
{
    if (int rc = chain_slots_ready(c, what)) return rc;
    if (c->lv[level].cur_block == 0) return bbme::fail(BBME_ERR_STATE, "%s: level %d has no MV grid yet", what, level);
    return BBME_OK;
}

static long long mc_groups(const Level &L) { return gather_groups(L.width, L.height, kMcRunsPerLane); }

// k_motion_compensate over `pairs` pairs from `pair0` on: the frame into d_out (one pair only) and/or, with d_stats, the
// statistics (partials in c->mc_stats)
static int enqueue_mc(bbme_ctx *c, int pair0, int pairs, int level, int block, int fill, const int *window, uint8_t *d_out,
                      int out_pitch, unsigned long long *d_stats, hipStream_t stream)
{
    const Level &L = c->lv[level];
    McArgs a{};
    a.plane_stride = L.plane_stride;
    a.grid_stride = L.grid_stride(L.cur_grid);
    a.img1 = c->plane1(L) + (size_t)pair0 * a.plane_stride;
    a.img2 = c->plane2(L) + (size_t)pair0 * a.plane_stride;
    a.grid = L.cur_grid + (size_t)pair0 * a.grid_stride;
    a.out = d_out;
    a.width = L.width; a.height = L.height;
    a.gcols = L.width / L.cur_block;
    a.lcb = __builtin_ctz((unsigned)L.cur_block);
    a.lb = __builtin_ctz((unsigned)block);
    a.fill = fill; a.out_pitch = out_pitch;
    set_window(a, window, L.width, L.height);
    set_runs(a, L.width, L.height);
    return launch_gather(k_motion_compensate, a, mc_groups(L), pairs, 1, c->mc_stats.partials_all(), d_stats, stream);
}

int bbme_motion_compensate_device(bbme_ctx *c, int pair, int level, int block, int fill, uint8_t *d_out, int out_pitch,
                                  void *hip_stream)
{
    const char *what = "bbme_motion_compensate_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_mc(c, level, block, fill, nullptr, what)) return rc;
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (out_pitch < c->lv[level].width)
        return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < level width %d", what, out_pitch, c->lv[level].width);
    if (int rc = check_mc_state(c, level, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_mc(c, pair, 1, level, block, fill, nullptr, d_out, out_pitch, nullptr, stream);
}

int bbme_get_motion_compensated_host(bbme_ctx *c, int pair, int level, int block, int fill, uint8_t *out)
{
    const char *what = "bbme_get_motion_compensated_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_mc(c, level, block, fill, nullptr, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_mc_state(c, level, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const Level &L = c->lv[level];
    return download_staged(c, (size_t)L.width * L.height, "the compensated plane", out, [&](uint8_t *d) {
        return enqueue_mc(c, pair, 1, level, block, fill, nullptr, d, L.width, nullptr, c->stream);
    });
}

int bbme_compensation_error(bbme_ctx *c, int level, int block, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_compensation_error";
    if (int rc = check_mc(c, level, block, 0, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_mc_state(c, level, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // one partial per pair and workgroup of level 0 (the largest plane); no caller's launch has statistics
    if (int rc = c->mc_stats.ensure(BBME_MAX_BATCH, mc_groups(c->lv[0]), c->batch, 0, "the compensation statistics")) return rc;
    return download_stats(c, c->mc_stats, c->batch, stats, [&] {
        return enqueue_mc(c, 0, c->batch, level, block, 0, window, nullptr, 0, c->mc_stats.results(), c->stream);
    });
}

// ---- forward-backward consistency of two cell grids (the rule of include/bbme.h; k_fb_consistency) -----------------------------

int bbme_backward_cells_device_pair(bbme_ctx *c, int pair, const int16_t **d_cells)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (!d_cells) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (!c->fields_valid) return bbme::fail(BBME_ERR_STATE, "bbme_backward_cells_device_pair: no valid bidirectional estimate");
    *d_cells = reinterpret_cast<const int16_t *>(c->bwd_cells + (size_t)pair * c->bwd_stride);
    return BBME_OK;
}

int bbme_get_backward_cells_host_pair(bbme_ctx *c, int pair, int16_t *cells)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (!cells) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (!c->fields_valid) return bbme::fail(BBME_ERR_STATE, "bbme_get_backward_cells_host_pair: no valid bidirectional estimate");
    HIP_TRY(hipSetDevice(c->device));
    const Level &L = c->lv[0];
    const size_t n = (size_t)(L.width / 2) * (L.height / 2);
    HIP_TRY(hipMemcpyAsync(cells, c->bwd_cells + (size_t)pair * c->bwd_stride, n * sizeof(mv_t), hipMemcpyDeviceToHost, c->stream));
    return check_converged(c);
}

// tolerance and window {cx0, cy0, cw, ch} in cells of a cells_w x cells_h grid.  Touches no device.
static int check_fb(int cells_w, int cells_h, int tol, const int *window, const char *what)
{
    if (tol < 0) return bbme::fail(BBME_ERR_INVALID, "%s: tolerance %d < 0", what, tol);
    return check_window(window, cells_w, cells_h, what, -1);
}

static int fb_scratch(bbme_ctx *c)
{
    return c->fb_stats.ensure(BBME_MAX_BATCH, cell_groups(c, kFbRunsPerLane), c->batch, 1, "the consistency statistics");
}

// k_fb_consistency over `pairs` pairs: the mask (rows mask_pitch, pairs s_mask bytes apart) and / or, with d_stats, the statistics
static int enqueue_fb(bbme_ctx *c, const mv_t *d_a, uint32_t s_a, const mv_t *d_b, uint32_t s_b, int pairs, int tol, const int *window,
                      uint8_t *d_mask, int mask_pitch, unsigned long long *partial, unsigned long long *d_stats, hipStream_t stream)
{
    const Level &L = c->lv[0];
    FbArgs a{};
    a.a = d_a; a.b = d_b; a.s_a = s_a; a.s_b = s_b;
    a.mask = d_mask; a.mask_pitch = mask_pitch; a.s_mask = 0;
    a.cw = L.width / 2; a.ch = L.height / 2; a.tol = tol;
    set_window(a, window, a.cw, a.ch);
    set_runs(a, a.cw, a.ch);
    return launch_gather(k_fb_consistency, a, cell_groups(c, kFbRunsPerLane), pairs, 1, partial, d_stats, stream);
}

int bbme_cells_consistency_device(bbme_ctx *c, const int16_t *d_a, const int16_t *d_b, int tol, const int *window, uint8_t *d_mask,
                                  int mask_pitch, unsigned long long *d_stats4, void *hip_stream)
{
    const char *what = "bbme_cells_consistency_device";
    if (int rc = check_ctx(c)) return rc;
    const Level &L = c->lv[0];
    if (!d_a || !d_b || (!d_mask && !d_stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_fb(L.width / 2, L.height / 2, tol, window, what)) return rc;
    if (d_mask && mask_pitch < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: mask pitch %d < %d cells per row", what, mask_pitch, L.width / 2);
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats4) if (int rc = fb_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_fb(c, reinterpret_cast<const mv_t *>(d_a), 0, reinterpret_cast<const mv_t *>(d_b), 0, 1, tol, window, d_mask,
                      mask_pitch, c->fb_stats.partials_caller(), d_stats4, stream);
}

// A = the forward cells, B = the backward cells of `which` = BBME_DIR_FORWARD, the other way round for BBME_DIR_BACKWARD
static int check_fb_ctx(const bbme_ctx *c, int which, int tol, const int *window, const char *what)
{
    if (int rc = check_ctx(c)) return rc;
    if (which != BBME_DIR_FORWARD && which != BBME_DIR_BACKWARD) return bbme::fail(BBME_ERR_INVALID, "%s: which = %d (0 or 1)", what, which);
    return check_fb(c->lv[0].width / 2, c->lv[0].height / 2, tol, window, what);
}

int bbme_get_consistency_host(bbme_ctx *c, int pair, int which, int tol, uint8_t *mask)
{
    const char *what = "bbme_get_consistency_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_fb_ctx(c, which, tol, nullptr, what)) return rc;
    if (!mask) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (!c->fields_valid) return bbme::fail(BBME_ERR_STATE, "%s: no valid bidirectional estimate", what);
    HIP_TRY(hipSetDevice(c->device));
    const int cw = c->lv[0].width / 2, ch = c->lv[0].height / 2;
    const mv_t *f, *b;
    own_fields(c, pair, &f, &b);
    return download_staged(c, (size_t)cw * ch, "the consistency mask", mask, [&](uint8_t *d) {
        return enqueue_fb(c, which ? b : f, 0, which ? f : b, 0, 1, tol, nullptr, d, cw, nullptr, nullptr, c->stream);
    });
}

int bbme_consistency_stats(bbme_ctx *c, int which, int tol, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_consistency_stats";
    if (int rc = check_fb_ctx(c, which, tol, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (!c->fields_valid) return bbme::fail(BBME_ERR_STATE, "%s: no valid bidirectional estimate", what);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = fb_scratch(c)) return rc;
    const Level &L = c->lv[0];
    const uint32_t s_f = L.grid_stride(L.final_grid()), s_b = c->bwd_stride;
    const mv_t *f = L.final_grid(), *b = c->bwd_cells;
    return download_stats(c, c->fb_stats, c->batch, stats, [&] {
        return enqueue_fb(c, which ? b : f, which ? s_b : s_f, which ? f : b, which ? s_f : s_b, c->batch, tol, window, nullptr, 0,
                          c->fb_stats.partials_all(), c->fb_stats.results(), c->stream);
    });
}

// ---- colour coding of a cell grid: Flow::MotionToColor of the subsampled field (the colour rule of include/bbme.h) ----------

// slots of bbme_ctx::color_range: one per pair, and one for the grids a caller brings (bbme_cells_color_device)
constexpr int kColorSlots = BBME_MAX_BATCH + 1;

// scale and the image it gives; with an image, its pitch.  Touches no device.
static int check_color(const bbme_ctx *c, int scale, const uint8_t *d_bgr, int pitch, const char *what, int *ow, int *oh)
{
    if (scale < 1) return bbme::fail(BBME_ERR_INVALID, "%s: scale %d < 1", what, scale);
    *ow = (int)(((long long)c->geom.width + scale - 1) / scale);
    *oh = (int)(((long long)c->geom.height + scale - 1) / scale);
    if (d_bgr && pitch < 3 * *ow) return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < 3 x %d bytes", what, pitch, *ow);
    return BBME_OK;
}

// the cells `which` names, every pair of them `*stride` words apart
static int color_source(const bbme_ctx *c, int which, const char *what, const mv_t **cells, uint32_t *stride)
{
    const Level &L = c->lv[0];
    if (which == BBME_DIR_BACKWARD) {
        if (!c->fields_valid) return bbme::fail(BBME_ERR_STATE, "%s: no valid bidirectional estimate", what);
        *cells = c->bwd_cells;
        *stride = c->bwd_stride;
    } else {
        if (L.cur_block != 2) return bbme::fail(BBME_ERR_STATE, "%s: level 0 has not been regularised down to 2x2 blocks", what);
        *cells = L.cur_grid;
        *stride = L.grid_stride(L.cur_grid);
    }
    return BBME_OK;
}

// Range pass over `pairs` grids (s_cells words apart) into slots slot .. slot + pairs - 1, when somebody reads it -- the caller
// (want_range; d_range: also there) or the image, which needs the max radius unless maxmotion overrides it --, then the image of
// the first grid into d_bgr, if any.  All on `stream`, no host wait.
static int enqueue_color(bbme_ctx *c, const mv_t *cells, uint32_t s_cells, int pairs, int slot, int scale, float maxmotion,
                         uint8_t *d_bgr, int pitch, bool want_range, float *d_range, hipStream_t stream)
{
    const Level &L = c->lv[0];
    ColorArgs a{};
    a.cells = cells; a.s_cells = s_cells; a.cell_cols = L.width / 2;
    a.pad_x = c->geom.pad_x; a.pad_y = c->geom.pad_y; a.scale = scale;
    a.ow = (int)(((long long)c->geom.width + scale - 1) / scale);
    a.oh = (int)(((long long)c->geom.height + scale - 1) / scale);
    a.ncx = scale == 1 ? ((a.pad_x + c->geom.width - 1) >> 1) - (a.pad_x >> 1) + 1 : a.ow;
    a.ncy = scale == 1 ? ((a.pad_y + c->geom.height - 1) >> 1) - (a.pad_y >> 1) + 1 : a.oh;
    uint32_t *keys = c->color_range + (size_t)slot * kColorKeyCopies * kColorKeyStride;
    float *range = reinterpret_cast<float *>(c->color_range + (size_t)kColorSlots * kColorKeyCopies * kColorKeyStride) + 5 * slot;
    if (want_range || d_range || !(maxmotion > 0)) {
        a.keys = keys;
        a.tiles_x = (a.ncx + 256 * kColorCellsPerLane - 1) / (256 * kColorCellsPerLane);
        const long long groups = (long long)a.tiles_x * a.ncy;
        hipLaunchKernelGGL(k_color_range_init, dim3((unsigned)pairs), dim3(256), 0, stream, keys);
        hipLaunchKernelGGL(k_color_range, dim3((unsigned)groups, (unsigned)pairs), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(k_color_range_finish, dim3((unsigned)pairs), dim3(64), 0, stream, keys, range, d_range);
    }
    if (d_bgr) {
        a.range = range; a.maxmotion = maxmotion; a.out = d_bgr; a.pitch = pitch;
        a.tiles_x = (a.ncx + 63) / 64;
        const long long tiles = (long long)a.tiles_x * ((a.ncy + 4 * kColorRowsPerWave - 1) / (4 * kColorRowsPerWave));
        hipLaunchKernelGGL(k_color_image, dim3((unsigned)tiles), dim3(256), 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

// the five floats of every slot, behind the slots' key words
static const float *color_floats(const bbme_ctx *c)
{
    return reinterpret_cast<const float *>(c->color_range + (size_t)kColorSlots * kColorKeyCopies * kColorKeyStride);
}

static int color_scratch(bbme_ctx *c)
{
    return c->color_range.ensure((size_t)kColorSlots * (kColorKeyCopies * kColorKeyStride + 5), "the colour ranges", Fill::poison);
}

int bbme_cells_color_device(bbme_ctx *c, const int16_t *d_cells, int scale, float maxmotion, uint8_t *d_bgr, int out_pitch_bytes,
                            float *d_range, void *hip_stream)
{
    const char *what = "bbme_cells_color_device";
    if (int rc = check_ctx(c)) return rc;
    if (!d_cells || (!d_bgr && !d_range)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    int ow, oh;
    if (int rc = check_color(c, scale, d_bgr, out_pitch_bytes, what, &ow, &oh)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = color_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_color(c, reinterpret_cast<const mv_t *>(d_cells), 0, 1, BBME_MAX_BATCH, scale, maxmotion, d_bgr, out_pitch_bytes,
                         false, d_range, stream);
}

int bbme_flow_color_device(bbme_ctx *c, int pair, int which, int scale, float maxmotion, uint8_t *d_bgr, int out_pitch_bytes,
                           float *d_range, void *hip_stream)
{
    const char *what = "bbme_flow_color_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (which != BBME_DIR_FORWARD && which != BBME_DIR_BACKWARD) return bbme::fail(BBME_ERR_INVALID, "%s: which = %d (0 or 1)", what, which);
    if (!d_bgr && !d_range) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    int ow, oh;
    if (int rc = check_color(c, scale, d_bgr, out_pitch_bytes, what, &ow, &oh)) return rc;
    const mv_t *cells;
    uint32_t stride;
    if (int rc = color_source(c, which, what, &cells, &stride)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = color_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_color(c, cells + (size_t)pair * stride, 0, 1, pair, scale, maxmotion, d_bgr, out_pitch_bytes, false, d_range, stream);
}

int bbme_get_flow_color_host(bbme_ctx *c, int pair, int which, int scale, float maxmotion, uint8_t *bgr, float *range5)
{
    const char *what = "bbme_get_flow_color_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (which != BBME_DIR_FORWARD && which != BBME_DIR_BACKWARD) return bbme::fail(BBME_ERR_INVALID, "%s: which = %d (0 or 1)", what, which);
    if (!bgr && !range5) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    int ow, oh;
    if (int rc = check_color(c, scale, nullptr, 0, what, &ow, &oh)) return rc;
    const mv_t *cells;
    uint32_t stride;
    if (int rc = color_source(c, which, what, &cells, &stride)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = color_scratch(c)) return rc;
    return download_staged(c, bgr ? (size_t)ow * oh * 3 : 0, "the colour image", bgr, [&](uint8_t *d) {
        return enqueue_color(c, cells + (size_t)pair * stride, 0, 1, pair, scale, maxmotion, d, 3 * ow, range5 != nullptr, nullptr,
                             c->stream);
    }, ExtraCopy{range5, color_floats(c) + 5 * pair, range5 ? 5 * sizeof(float) : 0});
}

int bbme_flow_ranges(bbme_ctx *c, int which, int scale, float *ranges)
{
    const char *what = "bbme_flow_ranges";
    if (int rc = check_ctx(c)) return rc;
    if (which != BBME_DIR_FORWARD && which != BBME_DIR_BACKWARD) return bbme::fail(BBME_ERR_INVALID, "%s: which = %d (0 or 1)", what, which);
    if (!ranges) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    int ow, oh;
    if (int rc = check_color(c, scale, nullptr, 0, what, &ow, &oh)) return rc;
    const mv_t *cells;
    uint32_t stride;
    if (int rc = color_source(c, which, what, &cells, &stride)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = color_scratch(c)) return rc;
    if (int rc = enqueue_color(c, cells, stride, c->batch, 0, scale, -1.0f, nullptr, 0, true, nullptr, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(ranges, color_floats(c), (size_t)5 * sizeof(float) * c->batch,
                           hipMemcpyDeviceToHost, c->stream));
    return check_converged(c);
}

// ---- motion-compensated interpolation between the two frames of a pair (the rule of include/bbme.h; k_interpolate) ----------

// phases num0 .. num0 + count - 1 of den, and the window {cx0, cy0, cw, ch} in cells.  Touches no device.
static int check_ip(const bbme_ctx *c, int num0, int count, int den, const int *window, const char *what)
{
    if (den < 2 || den > 256) return bbme::fail(BBME_ERR_INVALID, "%s: den %d outside 2..256", what, den);
    if (num0 < 1 || count < 1 || (long long)num0 + count > den)
        return bbme::fail(BBME_ERR_INVALID, "%s: phases %d .. %d + %d - 1 are not inside 1 .. %d", what, num0, num0, count, den - 1);
    return check_window(window, c->lv[0].width / 2, c->lv[0].height / 2, what, -1);
}

// partials of a launch over every pair, then those of a one-pair launch of `count` phases; grown, behind both streams, when a
// launch of more phases comes
static int phase_scratch(bbme_ctx *c, StatsScratch &s, long long groups, int count, hipStream_t stream, const char *what)
{
    s.layout(BBME_MAX_BATCH, groups, c->batch);
    if (s.words(count) <= s.size()) return BBME_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));             // the old buffer may still be being read
    if (stream != c->stream) HIP_TRY(hipStreamSynchronize(stream));
    return s.ensure(count, what);
}

static int ip_scratch(bbme_ctx *c, int count, hipStream_t stream)
{
    return phase_scratch(c, c->ip_stats, cell_groups(c, kIpRunsPerLane), count, stream, "the interpolation statistics");
}

// what IpArgs and IpBgrArgs share: the planes of `pair0`, the two grids, the output frames, the phases and their division
static void ip_fill(IpCommon &a, const bbme_ctx *c, int pair0, const mv_t *d_f, const mv_t *d_b, int num0, int den, uint8_t *d_out,
                    int out_pitch, size_t out_stride)
{
    const Level &L = c->lv[0];
    a.img1 = c->plane1(L) + (size_t)pair0 * L.plane_stride;
    a.img2 = c->plane2(L) + (size_t)pair0 * L.plane_stride;
    a.fwd = d_f; a.bwd = d_b;
    a.out = d_out; a.out_pitch = out_pitch; a.out_stride = out_stride;
    a.width = L.width; a.height = L.height; a.cw = L.width / 2;
    a.num0 = num0; a.den = den;
    a.magic = (uint32_t)((1ull << 32) / (unsigned)den + 1ull);
    set_runs(a, a.cw, L.height / 2);
}

// k_interpolate over `pairs` pairs from `pair0` on and `count` phases from num0 on: frames and maps (one pair only) and / or, with
// d_stats, the statistics
static int enqueue_ip(bbme_ctx *c, int pair0, int pairs, const mv_t *d_f, uint32_t s_f, const mv_t *d_b, uint32_t s_b, int num0,
                      int count, int den, const int *window, uint8_t *d_out, int out_pitch, size_t out_stride, uint8_t *d_sel,
                      int sel_pitch, size_t sel_stride, unsigned long long *partial, unsigned long long *d_stats, hipStream_t stream)
{
    IpArgs a{};
    ip_fill(a, c, pair0, d_f, d_b, num0, den, d_out, out_pitch, out_stride);
    a.plane_stride = c->lv[0].plane_stride; a.s_f = s_f; a.s_b = s_b;
    a.sel = d_sel; a.sel_pitch = sel_pitch; a.sel_stride = sel_stride;
    a.ch = a.height / 2;
    set_window(a, window, a.cw, a.ch);
    return launch_gather(k_interpolate, a, cell_groups(c, kIpRunsPerLane), pairs, count, partial, d_stats, stream);
}

int bbme_cells_interpolate_device(bbme_ctx *c, int pair, const int16_t *d_fwd, const int16_t *d_bwd, int num0, int count, int den,
                                  const int *window, uint8_t *d_out, int out_pitch, size_t out_stride, uint8_t *d_sel,
                                  int sel_pitch, size_t sel_stride, unsigned long long *d_stats4, void *hip_stream)
{
    const char *what = "bbme_cells_interpolate_device";
    if (int rc = check_pair(c, pair)) return rc;
    const Level &L = c->lv[0];
    if (!d_fwd || (!d_out && !d_sel && !d_stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_ip(c, num0, count, den, window, what)) return rc;
    if (d_out) if (int rc = check_frames(count, out_pitch, out_stride, L.width, L.height, what, "output")) return rc;
    if (d_sel) if (int rc = check_frames(count, sel_pitch, sel_stride, L.width / 2, L.height / 2, what, "selection map")) return rc;
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if (d_stats4) if (int rc = ip_scratch(c, count, stream)) return rc;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_ip(c, pair, 1, reinterpret_cast<const mv_t *>(d_fwd), 0, reinterpret_cast<const mv_t *>(d_bwd), 0, num0, count, den,
                      window, d_out, out_pitch, out_stride, d_sel, sel_pitch, sel_stride, c->ip_stats.partials_caller(), d_stats4, stream);
}

// what the three calls on the context's own two fields share
static int check_ip_ctx(const bbme_ctx *c, int num0, int count, int den, const int *window, const char *what)
{
    if (int rc = check_ctx(c)) return rc;
    return check_ip(c, num0, count, den, window, what);
}

// frames and a valid bidirectional estimate: what interpolation and the temporal filter need of the context's own state
static int check_fields_state(const bbme_ctx *c, const char *what)
{
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    if (!c->fields_valid) return bbme::fail(BBME_ERR_STATE, "%s: no valid bidirectional estimate", what);
    return BBME_OK;
}

// the context's own two fields of `pair`, `count` phases into d_out on `stream`
static int enqueue_own_ip(bbme_ctx *c, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch, size_t out_stride,
                          hipStream_t stream)
{
    const mv_t *f, *b;
    own_fields(c, pair, &f, &b);
    return enqueue_ip(c, pair, 1, f, 0, b, 0, num0, count, den, nullptr, d_out, out_pitch, out_stride, nullptr, 0, 0, nullptr, nullptr, stream);
}

int bbme_interpolate_device(bbme_ctx *c, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch, size_t out_stride,
                            void *hip_stream)
{
    const char *what = "bbme_interpolate_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_ip_ctx(c, num0, count, den, nullptr, what)) return rc;
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_frames(count, out_pitch, out_stride, c->lv[0].width, c->lv[0].height, what, "output")) return rc;
    if (int rc = check_fields_state(c, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_ip(c, pair, num0, count, den, d_out, out_pitch, out_stride, stream);
}

int bbme_get_interpolated_host(bbme_ctx *c, int pair, int num, int den, uint8_t *out)
{
    const char *what = "bbme_get_interpolated_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_ip_ctx(c, num, 1, den, nullptr, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_fields_state(c, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const Level &L = c->lv[0];
    return download_staged(c, (size_t)L.width * L.height, "the interpolated frame", out, [&](uint8_t *d) {
        return enqueue_own_ip(c, pair, num, 1, den, d, L.width, 0, c->stream);
    });
}

int bbme_interpolation_stats(bbme_ctx *c, int num, int den, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_interpolation_stats";
    if (int rc = check_ip_ctx(c, num, 1, den, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_fields_state(c, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ip_scratch(c, 1, c->stream)) return rc;
    const Level &L = c->lv[0];
    return download_stats(c, c->ip_stats, c->batch, stats, [&] {
        return enqueue_ip(c, 0, c->batch, L.final_grid(), L.grid_stride(L.final_grid()), c->bwd_cells, c->bwd_stride, num, 1, den, window,
                          nullptr, 0, 0, nullptr, 0, 0, c->ip_stats.partials_all(), c->ip_stats.results(), c->stream);
    });
}

// ---- colour frames out (the BGR interpolation rule of include/bbme.h; k_interpolate_bgr) -----------------------------------

// the stored colour of `pair` as the current direction reads it (frame 1, frame 2), or BBME_ERR_STATE
static int stored_bgr(const bbme_ctx *c, int pair, const char *what, const uint8_t **bgr1, const uint8_t **bgr2)
{
    const int s1 = c->slot(pair, c->direction ? 1 : 0), s2 = c->slot(pair, c->direction ? 0 : 1);
    if (!c->bgr_set[s1] || !c->bgr_set[s2])
        return bbme::fail(BBME_ERR_STATE, "%s: pair %d has no stored colour (set both frames with a *_bgr setter)", what, pair);
    *bgr1 = c->bgr + (size_t)s1 * c->bgr_stride;
    *bgr2 = c->bgr + (size_t)s2 * c->bgr_stride;
    return BBME_OK;
}

int bbme_bgr_frames_device_pair(bbme_ctx *c, int pair, const uint8_t **d_bgr1, const uint8_t **d_bgr2)
{
    const char *what = "bbme_bgr_frames_device_pair";
    if (int rc = check_pair(c, pair)) return rc;
    if (!d_bgr1 || !d_bgr2) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const uint8_t *a = nullptr, *b = nullptr;
    if (int rc = stored_bgr(c, pair, what, &a, &b)) return rc;
    *d_bgr1 = c->direction ? b : a;                        // physical: image 1 as it was set
    *d_bgr2 = c->direction ? a : b;
    return BBME_OK;
}

// k_interpolate_bgr over `count` phases from num0 on, one pair; bgr1 / bgr2 already in the direction's order.  No statistics, no
// map: its own launch.
static int enqueue_ip_bgr(bbme_ctx *c, int pair, const mv_t *d_f, const mv_t *d_b, const uint8_t *bgr1, const uint8_t *bgr2, int bgr_pitch,
                          int num0, int count, int den, uint8_t *d_out, int out_pitch, size_t out_stride, hipStream_t stream)
{
    const Geometry &g = c->geom;
    IpBgrArgs a{};
    ip_fill(a, c, pair, d_f, d_b, num0, den, d_out, out_pitch, out_stride);
    a.bgr1 = bgr1; a.bgr2 = bgr2; a.bgr_pitch = bgr_pitch;
    a.fw = g.width; a.fh = g.height; a.pad_x = g.pad_x; a.pad_y = g.pad_y;
    hipLaunchKernelGGL(k_interpolate_bgr, dim3((unsigned)cell_groups(c, kIpRunsPerLane), 1, (unsigned)count), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

// phases, output pitch and stride of the colour calls.  Touches no device.
static int check_ip_bgr(const bbme_ctx *c, int num0, int count, int den, const uint8_t *d_out, int out_pitch, size_t out_stride,
                        const char *what)
{
    if (int rc = check_ip(c, num0, count, den, nullptr, what)) return rc;
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    return check_bgr_frames(c, count, out_pitch, out_stride, what);
}

int bbme_cells_interpolate_bgr_device(bbme_ctx *c, int pair, const int16_t *d_fwd, const int16_t *d_bwd, const uint8_t *d_bgr1,
                                      const uint8_t *d_bgr2, int bgr_pitch, int num0, int count, int den, uint8_t *d_out,
                                      int out_pitch, size_t out_stride, void *hip_stream)
{
    const char *what = "bbme_cells_interpolate_bgr_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (!d_fwd) return bbme::fail(BBME_ERR_INVALID, "%s: null forward grid", what);
    if (int rc = check_ip_bgr(c, num0, count, den, d_out, out_pitch, out_stride, what)) return rc;
    if ((d_bgr1 == nullptr) != (d_bgr2 == nullptr))
        return bbme::fail(BBME_ERR_INVALID, "%s: one colour frame without the other (both, or neither for the stored colour)", what);
    if (d_bgr1 && (long long)bgr_pitch < 3LL * c->geom.width)
        return bbme::fail(BBME_ERR_INVALID, "%s: colour pitch %d < 3 x frame width %d", what, bgr_pitch, c->geom.width);
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    const uint8_t *bgr1 = c->direction ? d_bgr2 : d_bgr1, *bgr2 = c->direction ? d_bgr1 : d_bgr2;
    if (!d_bgr1) {
        if (int rc = stored_bgr(c, pair, what, &bgr1, &bgr2)) return rc;
        bgr_pitch = 3 * c->geom.width;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_ip_bgr(c, pair, reinterpret_cast<const mv_t *>(d_fwd), reinterpret_cast<const mv_t *>(d_bwd), bgr1, bgr2, bgr_pitch,
                          num0, count, den, d_out, out_pitch, out_stride, stream);
}

// the context's own two fields and stored colour of `pair` on `stream`
static int enqueue_own_ip_bgr(bbme_ctx *c, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch, size_t out_stride,
                              hipStream_t stream, const char *what)
{
    const uint8_t *bgr1 = nullptr, *bgr2 = nullptr;
    if (int rc = stored_bgr(c, pair, what, &bgr1, &bgr2)) return rc;
    const mv_t *f, *b;
    own_fields(c, pair, &f, &b);
    return enqueue_ip_bgr(c, pair, f, b, bgr1, bgr2, 3 * c->geom.width, num0, count, den, d_out, out_pitch, out_stride, stream);
}

int bbme_interpolate_bgr_device(bbme_ctx *c, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch, size_t out_stride,
                                void *hip_stream)
{
    const char *what = "bbme_interpolate_bgr_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_ip_bgr(c, num0, count, den, d_out, out_pitch, out_stride, what)) return rc;
    if (int rc = check_fields_state(c, what)) return rc;
    const uint8_t *bgr1 = nullptr, *bgr2 = nullptr;
    if (int rc = stored_bgr(c, pair, what, &bgr1, &bgr2)) return rc;       // before anything is enqueued
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_ip_bgr(c, pair, num0, count, den, d_out, out_pitch, out_stride, stream, what);
}

int bbme_get_interpolated_bgr_host(bbme_ctx *c, int pair, int num, int den, uint8_t *out)
{
    const char *what = "bbme_get_interpolated_bgr_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_ip(c, num, 1, den, nullptr, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_fields_state(c, what)) return rc;
    const uint8_t *bgr1 = nullptr, *bgr2 = nullptr;
    if (int rc = stored_bgr(c, pair, what, &bgr1, &bgr2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return download_staged(c, (size_t)3 * c->geom.width * c->geom.height, "the interpolated colour frame", out, [&](uint8_t *d) {
        return enqueue_own_ip_bgr(c, pair, num, 1, den, d, 3 * c->geom.width, 0, c->stream, what);
    });
}

// ---- motion-compensated temporal filter of a frame with its neighbours (the temporal filter rules of include/bbme.h) --------------
// Written once over a flavour: TfGrey filters the level-0 planes (k_temporal_filter), TfBgr the B,G,R frames (k_temporal_filter_bgr),
// TfSubpel (further down, behind the refinement it needs) the level-0 planes along quarter-pel grids (k_subpel_temporal_filter),
// TfSubpelBgr (beside it) the B,G,R frames along quarter-pel grids (k_subpel_temporal_filter_bgr).

constexpr int kTfMaxFrames = 2 * BBME_MAX_BATCH;          // a batch holds 2 batch frames, a chain batch + 1

// BBME_ERR_STATE unless the slots lo .. hi of the colour store (clamped to the context's) all have colour
static int check_tf_bgr_colour(const bbme_ctx *c, int lo, int hi, const char *what)
{
    for (int s = std::max(lo, 0); s <= std::min(hi, c->frames() - 1); ++s)
        if (!c->bgr_set[s])
            return bbme::fail(BBME_ERR_STATE, "%s: frame slot %d has no stored colour (set it with a *_bgr setter)", what, s);
    return BBME_OK;
}

// BBME_ERR_STATE unless frame `which` of `pair` and the neighbours the rule gives it have colour
static int check_tf_bgr_frame_colour(const bbme_ctx *c, int pair, int which, const char *what)
{
    if (c->chain) return check_tf_bgr_colour(c, pair + which - 1, pair + which + 1, what);
    for (int w = 0; w < 2; ++w)
        if (!c->bgr_set[c->slot(pair, w)])
            return bbme::fail(BBME_ERR_STATE, "%s: pair %d has no stored colour (set both frames with a *_bgr setter)", what, pair);
    return BBME_OK;
}

// A flavour names the argument type and kernel, the size of a frame (`rows` rows of row_bytes), the statistics scratch, what the
// arguments hold beyond TfArgs, and the context's own frames: their base, s_pair bytes from pair to pair and s_frame from a frame
// to its next neighbour.  What only colour checks hangs on `bgr` in the bodies below, the pitch of a caller's quarter-pel grids on
// `subpel`.  check_own is what the context-level calls check beyond the integer filter's; prepare runs on the stream before a
// launch on the context's own frames (pairs pair0 .. along y, frames first .. along z) and may replace the grids in the arguments.
struct TfNoPrepare {
    static constexpr bool subpel = false;
    static int check_own(const bbme_ctx *, const char *) { return BBME_OK; }
    template <class Args>
    static int prepare(bbme_ctx *, Args &, int, int, int, int, hipStream_t, const char *) { return BBME_OK; }
};

struct TfGrey : TfNoPrepare {
    using Args = TfArgs;
    static constexpr bool bgr = false;
    static constexpr const char *input = "plane", *staging_what = "the filtered frame", *stats_what = "the temporal filter statistics";
    static auto kernel() { return k_temporal_filter; }
    static int row_bytes(const bbme_ctx *c) { return c->lv[0].width; }
    static int rows(const bbme_ctx *c) { return c->lv[0].height; }
    static StatsScratch &stats(bbme_ctx *c) { return c->tf_stats; }
    static void geometry(const bbme_ctx *, TfArgs &) {}
    static const uint8_t *own(const bbme_ctx *c, long long *s_pair, long long *s_frame)
    {
        const Level &L = c->lv[0];
        *s_pair = L.plane_stride;
        *s_frame = c->chain ? (long long)L.plane_stride : (long long)L.frame_step;
        return L.img1;
    }
};

struct TfBgr : TfNoPrepare {
    using Args = TfBgrArgs;
    static constexpr bool bgr = true;
    static constexpr const char *input = "frame", *staging_what = "the filtered colour frame",
                                *stats_what = "the colour temporal filter statistics";
    static auto kernel() { return k_temporal_filter_bgr; }
    static int row_bytes(const bbme_ctx *c) { return 3 * c->geom.width; }
    static int rows(const bbme_ctx *c) { return c->geom.height; }
    static StatsScratch &stats(bbme_ctx *c) { return c->tf_bgr_stats; }
    static void geometry(const bbme_ctx *c, TfBgrArgs &a)      // the frame inside the padded view
    {
        a.fw = c->geom.width; a.fh = c->geom.height; a.pad_x = c->geom.pad_x; a.pad_y = c->geom.pad_y;
        a.bgr_pitch = 3 * c->geom.width;
    }
    // the colour store's slots (chain: slot; pair or batch: which x batch + pair).  In 64 bits: a deep chain's store exceeds 4 GB.
    static const uint8_t *own(const bbme_ctx *c, long long *s_pair, long long *s_frame)
    {
        *s_pair = (long long)c->bgr_stride;
        *s_frame = c->chain ? *s_pair : *s_pair * c->batch;
        return c->bgr;
    }
};

// pitch and, with more than one frame, stride of a caller's output frames
template <class F>
static int check_tf_out(const bbme_ctx *c, int count, int pitch, size_t stride, const char *what)
{
    if (F::bgr) return check_bgr_frames(c, count, pitch, stride, what);
    return check_frames(count, pitch, stride, F::row_bytes(c), F::rows(c), what, "output");
}

static long long tf_groups(const bbme_ctx *c) { return cell_groups(c, kTfRunsPerLane); }

// result words of every frame, partials of a launch over every frame, then those of a one-frame launch: one size per context, so
// it is never replaced under a launch that reads it
template <class F>
static int tf_scratch(bbme_ctx *c)
{
    return F::stats(c).ensure(kTfMaxFrames, tf_groups(c), c->frames(), 1, F::stats_what);
}

static int check_tf(const bbme_ctx *c, int thr, const int *window, const char *what)
{
    if (thr < 1 || thr > 1021) return bbme::fail(BBME_ERR_INVALID, "%s: strength %d outside 1..1021", what, thr);
    return check_window(window, c->lv[0].width / 2, c->lv[0].height / 2, what, -1);
}

// what both flavours' arguments share: geometry, strength, the magics of both divisions and the window
static void tf_fill(TfArgs &a, const bbme_ctx *c, int thr, const int *window)
{
    const Level &L = c->lv[0];
    a.width = L.width; a.height = L.height; a.cw = L.width / 2; a.ch = L.height / 2;
    a.thr = thr;
    a.magic_thr = thr > 1 ? (uint32_t)((1ull << 32) / (unsigned)thr + 1ull) : 0u;      // thr = 1: the kernels do not divide
    for (int S = 8; S <= 24; ++S) a.magic_s[S - 8] = (uint32_t)((1ull << 32) / (unsigned)S + 1ull);
    set_window(a, window, a.cw, a.ch);
    set_runs(a, a.cw, a.ch);
}

template <class F>
static typename F::Args tf_args(const bbme_ctx *c, int thr, const int *window)
{
    typename F::Args a{};
    tf_fill(a, c, thr, window);
    F::geometry(c, a);
    return a;
}

// the flavour's kernel over `pairs` x `count` frames (blockIdx.y, blockIdx.z)
template <class F>
static int enqueue_tf(bbme_ctx *c, typename F::Args &a, int pairs, int count, unsigned long long *partial, unsigned long long *d_stats,
                      hipStream_t stream)
{
    return launch_gather(F::kernel(), a, tf_groups(c), pairs, count, partial, d_stats, stream);
}

// The context's own frames as the kernels address them.  Chain: slots first .. first + count - 1 along z, neighbours one slot to
// either side, into-previous = backward cells of pair slot - 1, into-next = forward cells of pair slot.  Pair or batch: image 1
// and image 2 of pairs pair0 .. along z = which (from which0 on), image 1 with its next neighbour only and image 2 with its
// previous one.  A base that a launch never dereferences (the first slot's previous frame, ...) is address arithmetic only.
static void tf_own_fill(TfArgs &a, const bbme_ctx *c, const uint8_t *frames, long long s_pair, long long s_frame, int pair0, int first,
                        int count)
{
    const Level &L = c->lv[0];
    const long long s_f = L.grid_stride(L.final_grid()), s_b = c->bwd_stride;
    const uintptr_t f = reinterpret_cast<uintptr_t>(L.final_grid()), b = reinterpret_cast<uintptr_t>(c->bwd_cells.get());
    const uintptr_t cur = reinterpret_cast<uintptr_t>(frames) + (c->chain ? 0 : pair0 * s_pair) + first * s_frame;   // chain: `first` is a slot
    a.cur = reinterpret_cast<const uint8_t *>(cur);
    a.prev = reinterpret_cast<const uint8_t *>(cur - s_frame);
    a.next = reinterpret_cast<const uint8_t *>(cur + s_frame);
    a.cur_z = a.prev_z = a.next_z = s_frame;
    a.first_prev = first > 0;                             // pair or batch: image 2 has image 1 behind it
    if (c->chain) {
        a.gp = reinterpret_cast<const mv_t *>(b + (first - 1) * s_b * (long long)sizeof(mv_t));
        a.gn = reinterpret_cast<const mv_t *>(f + first * s_f * (long long)sizeof(mv_t));
        a.gp_z = s_b; a.gn_z = s_f;
        a.last_next = first + count - 1 < c->batch;
    } else {
        a.cur_y = a.prev_y = a.next_y = s_pair;
        a.gp = reinterpret_cast<const mv_t *>(b + pair0 * s_b * (long long)sizeof(mv_t));
        a.gn = reinterpret_cast<const mv_t *>(f + pair0 * s_f * (long long)sizeof(mv_t));
        a.gp_y = s_b; a.gn_y = s_f;
        a.last_next = first + count - 1 < 1;              // image 1 has image 2 ahead
    }
}

template <class F>
static typename F::Args tf_own_frames(const bbme_ctx *c, int thr, const int *window, int pair0, int first, int count)
{
    typename F::Args a = tf_args<F>(c, thr, window);
    long long s_pair, s_frame;
    const uint8_t *frames = F::own(c, &s_pair, &s_frame);
    tf_own_fill(a, c, frames, s_pair, s_frame, pair0, first, count);
    return a;
}

// bbme_cells_temporal_filter_device and its colour twin: a caller's frames (rows in_pitch bytes apart) and grids
template <class F>
static int tf_cells(bbme_ctx *c, const char *what, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next, int in_pitch,
                    const int16_t *d_to_prev, const int16_t *d_to_next, int thr, const int *window, uint8_t *d_out, int out_pitch,
                    uint8_t *d_weights, int weights_pitch, unsigned long long *d_stats4, void *hip_stream, int q4_pitch = 0)
{
    if (int rc = check_ctx(c)) return rc;
    const Level &L = c->lv[0];
    if (!d_cur || (!d_out && !d_weights && !d_stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (F::subpel && q4_pitch < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch, L.width / 2);
    if ((d_prev == nullptr) != (d_to_prev == nullptr) || (d_next == nullptr) != (d_to_next == nullptr))
        return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its %s and its grid", what, F::input);
    if (!d_prev && !d_next) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (int rc = check_tf(c, thr, window, what)) return rc;
    if (F::bgr && (long long)in_pitch < 3LL * c->geom.width)
        return bbme::fail(BBME_ERR_INVALID, "%s: colour pitch %d < 3 x frame width %d", what, in_pitch, c->geom.width);
    if (d_out) if (int rc = check_tf_out<F>(c, 1, out_pitch, 0, what)) return rc;
    if (d_weights && weights_pitch < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: weight map pitch %d < %d cells per row", what, weights_pitch, L.width / 2);
    if (d_out && overlaps_input(d_out, out_pitch, {d_prev, d_cur, d_next}, in_pitch, F::row_bytes(c), F::rows(c)))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input %s", what, F::input);
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats4) if (int rc = tf_scratch<F>(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    typename F::Args a = tf_args<F>(c, thr, window);
    a.cur = d_cur; a.prev = d_prev; a.next = d_next;
    if constexpr (F::bgr) a.bgr_pitch = in_pitch;
    if constexpr (F::subpel) a.q4_pitch = q4_pitch;
    a.gp = reinterpret_cast<const mv_t *>(d_to_prev); a.gn = reinterpret_cast<const mv_t *>(d_to_next);
    a.first_prev = a.last_next = 1;
    a.out = d_out; a.out_pitch = out_pitch;
    a.wmap = d_weights; a.wmap_pitch = weights_pitch;
    return enqueue_tf<F>(c, a, 1, 1, F::stats(c).partials_caller(), d_stats4, stream);
}

// frame `which` of `pair` of the context's own, into d_out on `stream`
template <class F>
static int enqueue_own_tf(bbme_ctx *c, const char *what, int pair, int which, int thr, uint8_t *d_out, int out_pitch, hipStream_t stream)
{
    const int pair0 = c->chain ? 0 : pair, first = c->chain ? pair + which : which;
    typename F::Args a = tf_own_frames<F>(c, thr, nullptr, pair0, first, 1);
    if (int rc = F::prepare(c, a, pair0, 1, first, 1, stream, what)) return rc;
    a.out = d_out; a.out_pitch = out_pitch;
    return enqueue_tf<F>(c, a, 1, 1, nullptr, nullptr, stream);
}

// pair, which and strength, a non-null output, the context's state and that frame `which` of `pair` and the neighbours the rule
// gives it are there
template <class F>
static int check_tf_frame(const bbme_ctx *c, int pair, int which, int thr, const uint8_t *out, const int *out_pitch, const char *what)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (which != 0 && which != 1) return bbme::fail(BBME_ERR_INVALID, "%s: which = %d (0 or 1)", what, which);
    if (int rc = check_tf(c, thr, nullptr, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (out_pitch) if (int rc = check_tf_out<F>(c, 1, *out_pitch, 0, what)) return rc;
    if (int rc = F::check_own(c, what)) return rc;
    if (int rc = check_fields_state(c, what)) return rc;
    return F::bgr ? check_tf_bgr_frame_colour(c, pair, which, what) : BBME_OK;
}

template <class F>
static int tf_device(bbme_ctx *c, const char *what, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream)
{
    if (int rc = check_tf_frame<F>(c, pair, which, thr, d_out, &out_pitch, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_tf<F>(c, what, pair, which, thr, d_out, out_pitch, stream);
}

template <class F>
static int tf_chain(bbme_ctx *c, const char *what, int first, int count, int thr, uint8_t *d_out, int out_pitch, size_t out_stride,
                    void *hip_stream)
{
    if (int rc = chain_context_only(c, what)) return rc;
    if (first < 0 || count < 1 || (long long)first + count > c->batch + 1)
        return bbme::fail(BBME_ERR_INVALID, "%s: slots %d .. %d + %d - 1 are not inside 0 .. %d", what, first, first, count, c->batch);
    if (int rc = check_tf(c, thr, nullptr, what)) return rc;
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_tf_out<F>(c, count, out_pitch, out_stride, what)) return rc;
    if (int rc = F::check_own(c, what)) return rc;
    if (int rc = check_fields_state(c, what)) return rc;
    if (F::bgr) if (int rc = check_tf_bgr_colour(c, first - 1, first + count, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    typename F::Args a = tf_own_frames<F>(c, thr, nullptr, 0, first, count);
    if (int rc = F::prepare(c, a, 0, 1, first, count, stream, what)) return rc;
    a.out = d_out; a.out_pitch = out_pitch; a.out_stride = out_stride;
    return enqueue_tf<F>(c, a, 1, count, nullptr, nullptr, stream);
}

template <class F>
static int tf_host(bbme_ctx *c, const char *what, int pair, int which, int thr, uint8_t *out)
{
    if (int rc = check_tf_frame<F>(c, pair, which, thr, out, nullptr, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return download_staged(c, (size_t)F::row_bytes(c) * F::rows(c), F::staging_what, out, [&](uint8_t *d) {
        return enqueue_own_tf<F>(c, what, pair, which, thr, d, F::row_bytes(c), c->stream);
    });
}

template <class F>
static int tf_stats(bbme_ctx *c, const char *what, int thr, const int *window, unsigned long long *stats)
{
    if (int rc = check_ctx(c)) return rc;
    if (int rc = check_tf(c, thr, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = F::check_own(c, what)) return rc;
    if (int rc = check_fields_state(c, what)) return rc;
    if (F::bgr) if (int rc = check_tf_bgr_colour(c, 0, c->frames() - 1, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = tf_scratch<F>(c)) return rc;
    // chain: one pair row, every slot along z; otherwise every pair along y, which along z: frame y gridDim.z + z either way
    const int pairs = c->chain ? 1 : c->batch, count = c->chain ? c->batch + 1 : 2;
    typename F::Args a = tf_own_frames<F>(c, thr, window, 0, 0, count);
    return download_stats(c, F::stats(c), c->frames(), stats, [&] {
        if (int rc = F::prepare(c, a, 0, pairs, 0, count, c->stream, what)) return rc;
        return enqueue_tf<F>(c, a, pairs, count, F::stats(c).partials_all(), F::stats(c).results(), c->stream);
    });
}

int bbme_cells_temporal_filter_device(bbme_ctx *c, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next,
                                      const int16_t *d_to_prev, const int16_t *d_to_next, int thr, const int *window, uint8_t *d_out,
                                      int out_pitch, uint8_t *d_weights, int weights_pitch, unsigned long long *d_stats4,
                                      void *hip_stream)
{
    return tf_cells<TfGrey>(c, "bbme_cells_temporal_filter_device", d_prev, d_cur, d_next, c ? c->lv[0].width : 0, d_to_prev, d_to_next,
                            thr, window, d_out, out_pitch, d_weights, weights_pitch, d_stats4, hip_stream);
}

int bbme_temporal_filter_device(bbme_ctx *c, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream)
{
    return tf_device<TfGrey>(c, "bbme_temporal_filter_device", pair, which, thr, d_out, out_pitch, hip_stream);
}

int bbme_temporal_filter_chain_device(bbme_ctx *c, int first, int count, int thr, uint8_t *d_out, int out_pitch, size_t out_stride,
                                      void *hip_stream)
{
    return tf_chain<TfGrey>(c, "bbme_temporal_filter_chain_device", first, count, thr, d_out, out_pitch, out_stride, hip_stream);
}

int bbme_get_temporal_filtered_host(bbme_ctx *c, int pair, int which, int thr, uint8_t *out)
{
    return tf_host<TfGrey>(c, "bbme_get_temporal_filtered_host", pair, which, thr, out);
}

int bbme_temporal_filter_stats(bbme_ctx *c, int thr, const int *window, unsigned long long *stats)
{
    return tf_stats<TfGrey>(c, "bbme_temporal_filter_stats", thr, window, stats);
}

int bbme_cells_temporal_filter_bgr_device(bbme_ctx *c, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next, int bgr_pitch,
                                          const int16_t *d_to_prev, const int16_t *d_to_next, int thr, const int *window,
                                          uint8_t *d_out, int out_pitch, uint8_t *d_weights, int weights_pitch,
                                          unsigned long long *d_stats4, void *hip_stream)
{
    return tf_cells<TfBgr>(c, "bbme_cells_temporal_filter_bgr_device", d_prev, d_cur, d_next, bgr_pitch, d_to_prev, d_to_next, thr, window,
                           d_out, out_pitch, d_weights, weights_pitch, d_stats4, hip_stream);
}

int bbme_temporal_filter_bgr_device(bbme_ctx *c, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream)
{
    return tf_device<TfBgr>(c, "bbme_temporal_filter_bgr_device", pair, which, thr, d_out, out_pitch, hip_stream);
}

int bbme_temporal_filter_bgr_chain_device(bbme_ctx *c, int first, int count, int thr, uint8_t *d_out, int out_pitch, size_t out_stride,
                                          void *hip_stream)
{
    return tf_chain<TfBgr>(c, "bbme_temporal_filter_bgr_chain_device", first, count, thr, d_out, out_pitch, out_stride, hip_stream);
}

int bbme_get_temporal_filtered_bgr_host(bbme_ctx *c, int pair, int which, int thr, uint8_t *out)
{
    return tf_host<TfBgr>(c, "bbme_get_temporal_filtered_bgr_host", pair, which, thr, out);
}

int bbme_temporal_filter_bgr_stats(bbme_ctx *c, int thr, const int *window, unsigned long long *stats)
{
    return tf_stats<TfBgr>(c, "bbme_temporal_filter_bgr_stats", thr, window, stats);
}

// ---- quarter-pel refinement of a cell grid (the SUBPEL RULE of include/bbme.h; K10 k_subpel_refine) ------------------------------

static int sp_tiles_x(const bbme_ctx *c) { return (c->lv[0].width / 2 + kSpTileW - 1) / kSpTileW; }
static long long sp_groups(const bbme_ctx *c) { return (long long)sp_tiles_x(c) * ((c->lv[0].height / 2 + kSpTileH - 1) / kSpTileH); }

// result words of every pair, partials of a launch over every pair, then those of a caller's launch: one size per context
static int sp_scratch(bbme_ctx *c)
{
    return c->sp_stats.ensure(BBME_MAX_BATCH, sp_groups(c), c->batch, 1, "the subpel statistics");
}

// geometry and window.  Touches no device.
static int check_sp(const bbme_ctx *c, const int *window, const char *what)
{
    const Level &L = c->lv[0];
    if (L.width > 8188 || L.height > 8188)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: a %dx%d plane is beyond 8188 (quarter-pel vectors would not fit 16 bits)", what,
                          L.width, L.height);
    return check_window(window, L.width / 2, L.height / 2, what, -1);
}

static int check_which(int which, const char *what)
{
    if (which != 0 && which != 1) return bbme::fail(BBME_ERR_INVALID, "%s: which = %d (0 or 1)", what, which);
    return BBME_OK;
}

// The context's own planes and grid of `which`, pairs s_plane bytes and *s_grid words apart: 0 = the current level-0 cells against
// (image 1, image 2) of the context's direction, 1 = the backward cells against (image 2, image 1).
static int sp_source(const bbme_ctx *c, int which, const char *what, const uint8_t **img1, const uint8_t **img2, const mv_t **grid,
                     uint32_t *s_grid)
{
    const Level &L = c->lv[0];
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    if (int rc = color_source(c, which, what, grid, s_grid)) return rc;
    *img1 = which ? L.img2 : c->plane1(L);
    *img2 = which ? L.img1.get() : c->plane2(L);
    return BBME_OK;
}

// k_subpel_refine over `pairs` pairs: the grid (rows out_pitch, pairs s_out cells apart) and / or, with d_stats, the statistics
static int enqueue_sp(bbme_ctx *c, const uint8_t *img1, const uint8_t *img2, size_t s_plane, const mv_t *grid, size_t s_grid, int pairs,
                      const int *window, mv_t *d_out, int out_pitch, size_t s_out, unsigned long long *partial,
                      unsigned long long *d_stats, hipStream_t stream)
{
    const Level &L = c->lv[0];
    SpArgs a{};
    a.img1 = img1; a.img2 = img2; a.grid = grid; a.out = d_out;
    a.s_plane = s_plane; a.s_grid = s_grid; a.s_out = s_out;
    a.width = L.width; a.height = L.height; a.cw = L.width / 2; a.ch = L.height / 2;
    a.out_pitch = out_pitch; a.tiles_x = sp_tiles_x(c);
    set_window(a, window, a.cw, a.ch);
    return launch_gather(k_subpel_refine, a, sp_groups(c), pairs, 1, partial, d_stats, stream);
}

static int enqueue_own_sp(bbme_ctx *c, int pair, int which, mv_t *d_out, int out_pitch, hipStream_t stream, const char *what)
{
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
    const size_t s_plane = c->lv[0].plane_stride;
    return enqueue_sp(c, i1 + pair * s_plane, i2 + pair * s_plane, 0, grid + (size_t)pair * s_grid, 0, 1, nullptr, d_out, out_pitch, 0,
                      nullptr, nullptr, stream);
}

int bbme_cells_subpel_device(bbme_ctx *c, const uint8_t *d_image1, const uint8_t *d_image2, const int16_t *d_cells, const int *window,
                             int16_t *d_q4, int q4_pitch_cells, unsigned long long *d_stats4, void *hip_stream)
{
    const char *what = "bbme_cells_subpel_device";
    if (int rc = check_ctx(c)) return rc;
    const Level &L = c->lv[0];
    const int cw = L.width / 2, ch = L.height / 2;
    if (!d_image1 || !d_image2 || !d_cells || (!d_q4 && !d_stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_sp(c, window, what)) return rc;
    if (d_q4 && q4_pitch_cells < cw) return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < %d cells per row", what, q4_pitch_cells, cw);
    if (d_q4 && overlaps_input(reinterpret_cast<const uint8_t *>(d_q4), q4_pitch_cells * 4, {reinterpret_cast<const uint8_t *>(d_cells)},
                               cw * 4, cw * 4, ch))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps the input grid", what);
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats4) if (int rc = sp_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_sp(c, d_image1, d_image2, 0, reinterpret_cast<const mv_t *>(d_cells), 0, 1, window, reinterpret_cast<mv_t *>(d_q4),
                      q4_pitch_cells, 0, c->sp_stats.partials_caller(), d_stats4, stream);
}

int bbme_subpel_device(bbme_ctx *c, int pair, int which, int16_t *d_q4, int q4_pitch_cells, void *hip_stream)
{
    const char *what = "bbme_subpel_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (!d_q4) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_sp(c, nullptr, what)) return rc;
    if (q4_pitch_cells < c->lv[0].width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < %d cells per row", what, q4_pitch_cells, c->lv[0].width / 2);
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;       // the state, before anything is enqueued
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_sp(c, pair, which, reinterpret_cast<mv_t *>(d_q4), q4_pitch_cells, stream, what);
}

static int check_sp_get(const bbme_ctx *c, int pair, int which, const void *out, const char *what)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    return check_sp(c, nullptr, what);
}

int bbme_get_subpel_cells_host(bbme_ctx *c, int pair, int which, int16_t *q4)
{
    const char *what = "bbme_get_subpel_cells_host";
    if (int rc = check_sp_get(c, pair, which, q4, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int cw = c->lv[0].width / 2, ch = c->lv[0].height / 2;
    return download_staged(c, (size_t)cw * ch, "the quarter-pel cells", reinterpret_cast<mv_t *>(q4), [&](mv_t *d) {
        return enqueue_own_sp(c, pair, which, d, cw, c->stream, what);
    });
}

int bbme_subpel_stats(bbme_ctx *c, int which, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_subpel_stats";
    if (int rc = check_ctx(c)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (int rc = check_sp(c, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = sp_scratch(c)) return rc;
    return download_stats(c, c->sp_stats, c->batch, stats, [&] {
        return enqueue_sp(c, i1, i2, c->lv[0].plane_stride, grid, s_grid, c->batch, window, nullptr, 0, 0, c->sp_stats.partials_all(),
                          c->sp_stats.results(), c->stream);
    });
}

int bbme_get_subpel_flow_host(bbme_ctx *c, int pair, int which, float *flow)
{
    const char *what = "bbme_get_subpel_flow_host";
    if (int rc = check_sp_get(c, pair, which, flow, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int cw = c->lv[0].width / 2, ch = c->lv[0].height / 2;
    const int scale = c->src_scale, ow = (c->geom.width + scale - 1) / scale, oh = (c->geom.height + scale - 1) / scale;
    // the field in the area's first region, the packed quarter-pel cells it is expanded from in the second
    return download_staged_with_scratch(c, (size_t)ow * oh * 2, "the quarter-pel field", flow, (size_t)cw * ch * sizeof(mv_t),
                                        [&](float *d, uint8_t *scratch) {
        mv_t *q4 = reinterpret_cast<mv_t *>(scratch);
        if (int rc = enqueue_own_sp(c, pair, which, q4, cw, c->stream, what)) return rc;
        hipLaunchKernelGGL(k_subsample_q4, dim3((unsigned)(((long long)ow * oh + 255) / 256)), dim3(256), 0, c->stream, q4, cw,
                           c->geom.pad_x, c->geom.pad_y, scale, d, ow, oh);
        HIP_TRY(hipGetLastError());
        return (int)BBME_OK;
    });
}

// ---- motion compensation along a quarter-pel grid (the SUBPEL COMPENSATION RULE of include/bbme.h; K11 k_subpel_compensate) -------

static long long sc_groups(const bbme_ctx *c) { return cell_groups(c, kScRunsPerLane); }

// result words of every pair, partials of a launch over every pair, then those of a caller's launch: one size per context
static int sc_scratch(bbme_ctx *c)
{
    return c->sc_stats.ensure(BBME_MAX_BATCH, sc_groups(c), c->batch, 1, "the subpel compensation statistics");
}

static int check_fill(int fill, const char *what)
{
    if (fill < 0 || fill > 255) return bbme::fail(BBME_ERR_INVALID, "%s: fill %d outside 0..255", what, fill);
    return BBME_OK;
}

// k_subpel_compensate over `pairs` pairs (planes s_plane bytes, grids s_q4 words apart): the frame into d_out (one pair only)
// and / or, with d_stats, the statistics over `window` in pixels
static int enqueue_sc(bbme_ctx *c, const uint8_t *img1, const uint8_t *img2, size_t s_plane, const mv_t *q4, int q4_pitch, size_t s_q4,
                      int pairs, int fill, const int *window, uint8_t *d_out, int out_pitch, unsigned long long *partial,
                      unsigned long long *d_stats, hipStream_t stream)
{
    const Level &L = c->lv[0];
    ScArgs a{};
    a.img1 = img1; a.img2 = img2; a.q4 = q4; a.out = d_out;
    a.s_plane = s_plane; a.s_q4 = s_q4;
    a.width = L.width; a.height = L.height; a.cw = L.width / 2;
    a.q4_pitch = q4_pitch; a.fill = fill; a.out_pitch = out_pitch;
    set_window(a, window, L.width, L.height);
    set_runs(a, L.width / 2, L.height / 2);
    return launch_gather(k_subpel_compensate, a, sc_groups(c), pairs, 1, partial, d_stats, stream);
}

// The context's own: the cells of `which` of `pairs` pairs from pair0 on refined into the context's quarter-pel buffer (one packed
// grid per pair, allocated here at first use), then compensated from it
static int enqueue_own_sc(bbme_ctx *c, int pair0, int pairs, int which, int fill, const int *window, uint8_t *d_out, int out_pitch,
                          unsigned long long *d_stats, hipStream_t stream, const char *what)
{
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
    const Level &L = c->lv[0];
    const int cw = L.width / 2;
    const size_t cells = (size_t)cw * (L.height / 2), s_plane = L.plane_stride;
    if (int rc = c->sc_q4.ensure(cells * c->batch, "the quarter-pel cells of the compensation", Fill::poison)) return rc;
    i1 += pair0 * s_plane; i2 += pair0 * s_plane;
    mv_t *q4 = c->sc_q4 + pair0 * cells;
    if (int rc = enqueue_sp(c, i1, i2, s_plane, grid + (size_t)pair0 * s_grid, s_grid, pairs, nullptr, q4, cw, cells, nullptr, nullptr,
                            stream))
        return rc;
    return enqueue_sc(c, i1, i2, s_plane, q4, cw, cells, pairs, fill, window, d_out, out_pitch, c->sc_stats.partials_all(), d_stats,
                      stream);
}

int bbme_cells_subpel_compensate_device(bbme_ctx *c, const uint8_t *d_image1, const uint8_t *d_image2, const int16_t *d_q4,
                                        int q4_pitch_cells, int fill, const int *window, uint8_t *d_out, int out_pitch,
                                        unsigned long long *d_stats4, void *hip_stream)
{
    const char *what = "bbme_cells_subpel_compensate_device";
    if (int rc = check_ctx(c)) return rc;
    const Level &L = c->lv[0];
    if (!d_image2 || !d_q4 || (!d_out && !d_stats4) || (d_stats4 && !d_image1))
        return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_fill(fill, what)) return rc;
    if (int rc = check_window(window, L.width, L.height, what, 0)) return rc;
    if (q4_pitch_cells < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch_cells, L.width / 2);
    if (d_out && out_pitch < L.width) return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < width %d", what, out_pitch, L.width);
    if (d_out && overlaps_input(d_out, out_pitch, {d_image1, d_image2}, L.width, L.width, L.height))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input plane", what);
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats4) if (int rc = sc_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_sc(c, d_image1, d_image2, 0, reinterpret_cast<const mv_t *>(d_q4), q4_pitch_cells, 0, 1, fill, window, d_out, out_pitch,
                      c->sc_stats.partials_caller(), d_stats4, stream);
}

// what bbme_subpel_compensate_device and bbme_get_subpel_compensated_host check alike.  Touches no device.
static int check_sc_own(const bbme_ctx *c, int pair, int which, int fill, const void *out, const char *what)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (int rc = check_fill(fill, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    return check_sp(c, nullptr, what);
}

int bbme_subpel_compensate_device(bbme_ctx *c, int pair, int which, int fill, uint8_t *d_out, int out_pitch, void *hip_stream)
{
    const char *what = "bbme_subpel_compensate_device";
    if (int rc = check_sc_own(c, pair, which, fill, d_out, what)) return rc;
    if (out_pitch < c->lv[0].width)
        return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < width %d", what, out_pitch, c->lv[0].width);
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;       // the state, before anything is enqueued
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_sc(c, pair, 1, which, fill, nullptr, d_out, out_pitch, nullptr, stream, what);
}

int bbme_get_subpel_compensated_host(bbme_ctx *c, int pair, int which, int fill, uint8_t *out)
{
    const char *what = "bbme_get_subpel_compensated_host";
    if (int rc = check_sc_own(c, pair, which, fill, out, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const Level &L = c->lv[0];
    return download_staged(c, (size_t)L.width * L.height, "the quarter-pel compensated plane", out, [&](uint8_t *d) {
        return enqueue_own_sc(c, pair, 1, which, fill, nullptr, d, L.width, nullptr, c->stream, what);
    });
}

int bbme_subpel_compensation_error(bbme_ctx *c, int which, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_subpel_compensation_error";
    if (int rc = check_ctx(c)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (int rc = check_sp(c, nullptr, what)) return rc;
    if (int rc = check_window(window, c->lv[0].width, c->lv[0].height, what, 0)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = sc_scratch(c)) return rc;
    return download_stats(c, c->sc_stats, c->batch, stats, [&] {
        return enqueue_own_sc(c, 0, c->batch, which, 0, window, nullptr, 0, c->sc_stats.results(), c->stream, what);
    });
}

// ---- interpolation at quarter-pel positions (the SUBPEL INTERPOLATION RULE of include/bbme.h; K12 k_subpel_interpolate) ----------

// as ip_scratch, of the context's own buffer for this rule
static int si_scratch(bbme_ctx *c, int count, hipStream_t stream)
{
    return phase_scratch(c, c->si_stats, cell_groups(c, kSiRunsPerLane), count, stream, "the subpel interpolation statistics");
}

// k_subpel_interpolate over `pairs` pairs from `pair0` on (grids s_q4 words apart) and `count` phases from num0 on: frames and maps
// (one pair only) and / or, with d_stats, the statistics
static int enqueue_si(bbme_ctx *c, int pair0, int pairs, const mv_t *d_qf, const mv_t *d_qb, int q4_pitch, size_t s_q4, int num0,
                      int count, int den, const int *window, uint8_t *d_out, int out_pitch, size_t out_stride, uint8_t *d_sel,
                      int sel_pitch, size_t sel_stride, unsigned long long *partial, unsigned long long *d_stats, hipStream_t stream)
{
    const Level &L = c->lv[0];
    SiArgs a{};
    a.img1 = c->plane1(L) + (size_t)pair0 * L.plane_stride;
    a.img2 = c->plane2(L) + (size_t)pair0 * L.plane_stride;
    a.qf = d_qf; a.qb = d_qb; a.q4_pitch = q4_pitch;
    a.s_plane = L.plane_stride; a.s_q4 = s_q4;
    a.out = d_out; a.out_pitch = out_pitch; a.out_stride = out_stride;
    a.sel = d_sel; a.sel_pitch = sel_pitch; a.sel_stride = sel_stride;
    a.width = L.width; a.height = L.height; a.cw = L.width / 2;
    a.num0 = num0; a.den = den;
    a.magic = (uint32_t)((1ull << 32) / (unsigned)den + 1ull);
    set_window(a, window, a.cw, L.height / 2);
    set_runs(a, a.cw, L.height / 2);
    return launch_gather(k_subpel_interpolate, a, cell_groups(c, kSiRunsPerLane), pairs, count, partial, d_stats, stream);
}

int bbme_cells_subpel_interpolate_device(bbme_ctx *c, int pair, const int16_t *d_qf, const int16_t *d_qb, int q4_pitch_cells,
                                         int num0, int count, int den, const int *window, uint8_t *d_out, int out_pitch,
                                         size_t out_stride, uint8_t *d_sel, int sel_pitch, size_t sel_stride,
                                         unsigned long long *d_stats4, void *hip_stream)
{
    const char *what = "bbme_cells_subpel_interpolate_device";
    if (int rc = check_pair(c, pair)) return rc;
    const Level &L = c->lv[0];
    if (!d_qf || (!d_out && !d_sel && !d_stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_ip(c, num0, count, den, window, what)) return rc;
    if (q4_pitch_cells < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch_cells, L.width / 2);
    if (d_out) if (int rc = check_frames(count, out_pitch, out_stride, L.width, L.height, what, "output")) return rc;
    if (d_sel) if (int rc = check_frames(count, sel_pitch, sel_stride, L.width / 2, L.height / 2, what, "selection map")) return rc;
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if (d_stats4) if (int rc = si_scratch(c, count, stream)) return rc;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_si(c, pair, 1, reinterpret_cast<const mv_t *>(d_qf), reinterpret_cast<const mv_t *>(d_qb), q4_pitch_cells, 0, num0,
                      count, den, window, d_out, out_pitch, out_stride, d_sel, sel_pitch, sel_stride, c->si_stats.partials_caller(),
                      d_stats4, stream);
}

// The context's own two fields of `pairs` pairs from pair0 on refined into the context's quarter-pel buffer (the packed forward
// grids of every pair, then the backward ones; allocated here at first use): q4[0] and q4[1] are pair0's, later pairs' `*cells`
// words on, rows *cw cells apart.  Shared by the grey and the colour interpolation.
static int refine_own_si(bbme_ctx *c, int pair0, int pairs, hipStream_t stream, const char *what, mv_t *(&q4)[2], int *cw_out,
                         size_t *cells_out)
{
    const Level &L = c->lv[0];
    const int cw = L.width / 2;
    const size_t cells = (size_t)cw * (L.height / 2), s_plane = L.plane_stride;
    if (int rc = c->si_q4.ensure(2 * cells * c->batch, "the quarter-pel cells of the interpolation", Fill::poison)) return rc;
    q4[0] = c->si_q4 + pair0 * cells;
    q4[1] = c->si_q4 + ((size_t)c->batch + pair0) * cells;
    for (int which = 0; which < 2; ++which) {
        const uint8_t *i1, *i2;
        const mv_t *grid;
        uint32_t s_grid;
        if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
        if (int rc = enqueue_sp(c, i1 + pair0 * s_plane, i2 + pair0 * s_plane, s_plane, grid + (size_t)pair0 * s_grid, s_grid, pairs,
                                nullptr, q4[which], cw, cells, nullptr, nullptr, stream))
            return rc;
    }
    *cw_out = cw;
    *cells_out = cells;
    return BBME_OK;
}

// The context's own: both fields refined (refine_own_si), then interpolated from the quarter-pel buffer
static int enqueue_own_si(bbme_ctx *c, int pair0, int pairs, int num0, int count, int den, const int *window, uint8_t *d_out,
                          int out_pitch, size_t out_stride, unsigned long long *partial, unsigned long long *d_stats, hipStream_t stream,
                          const char *what)
{
    mv_t *q4[2];
    int cw;
    size_t cells;
    if (int rc = refine_own_si(c, pair0, pairs, stream, what, q4, &cw, &cells)) return rc;
    return enqueue_si(c, pair0, pairs, q4[0], q4[1], cw, cells, num0, count, den, window, d_out, out_pitch, out_stride, nullptr, 0, 0,
                      partial, d_stats, stream);
}

// what the three calls on the context's own two fields share.  Touches no device.
static int check_si_own(const bbme_ctx *c, int num0, int count, int den, const int *window, const void *out, const char *what)
{
    if (int rc = check_ip_ctx(c, num0, count, den, window, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_sp(c, nullptr, what)) return rc;
    return check_fields_state(c, what);
}

int bbme_subpel_interpolate_device(bbme_ctx *c, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch, size_t out_stride,
                                   void *hip_stream)
{
    const char *what = "bbme_subpel_interpolate_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (d_out) if (int rc = check_frames(count, out_pitch, out_stride, c->lv[0].width, c->lv[0].height, what, "output")) return rc;
    if (int rc = check_si_own(c, num0, count, den, nullptr, d_out, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_si(c, pair, 1, num0, count, den, nullptr, d_out, out_pitch, out_stride, nullptr, nullptr, stream, what);
}

int bbme_get_subpel_interpolated_host(bbme_ctx *c, int pair, int num, int den, uint8_t *out)
{
    const char *what = "bbme_get_subpel_interpolated_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_si_own(c, num, 1, den, nullptr, out, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const Level &L = c->lv[0];
    return download_staged(c, (size_t)L.width * L.height, "the quarter-pel interpolated frame", out, [&](uint8_t *d) {
        return enqueue_own_si(c, pair, 1, num, 1, den, nullptr, d, L.width, 0, nullptr, nullptr, c->stream, what);
    });
}

int bbme_subpel_interpolation_stats(bbme_ctx *c, int num, int den, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_subpel_interpolation_stats";
    if (int rc = check_si_own(c, num, 1, den, window, stats, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = si_scratch(c, 1, c->stream)) return rc;
    return download_stats(c, c->si_stats, c->batch, stats, [&] {
        return enqueue_own_si(c, 0, c->batch, num, 1, den, window, nullptr, 0, 0, c->si_stats.partials_all(), c->si_stats.results(),
                              c->stream, what);
    });
}

// ---- colour frames at quarter-pel positions (the BGR SUBPEL INTERPOLATION RULE of include/bbme.h; K12b k_subpel_interpolate_bgr) ----

// k_subpel_interpolate_bgr over `count` phases from num0 on, one pair; bgr1 / bgr2 already in the direction's order.  No
// statistics, no map: its own launch.
static int enqueue_si_bgr(bbme_ctx *c, int pair, const mv_t *d_qf, const mv_t *d_qb, int q4_pitch, const uint8_t *bgr1,
                          const uint8_t *bgr2, int bgr_pitch, int num0, int count, int den, uint8_t *d_out, int out_pitch,
                          size_t out_stride, hipStream_t stream)
{
    const Level &L = c->lv[0];
    const Geometry &g = c->geom;
    SiBgrArgs a{};
    a.img1 = c->plane1(L) + (size_t)pair * L.plane_stride;
    a.img2 = c->plane2(L) + (size_t)pair * L.plane_stride;
    a.qf = d_qf; a.qb = d_qb; a.q4_pitch = q4_pitch;
    a.bgr1 = bgr1; a.bgr2 = bgr2; a.bgr_pitch = bgr_pitch;
    a.out = d_out; a.out_pitch = out_pitch; a.out_stride = out_stride;
    a.width = L.width; a.height = L.height; a.cw = L.width / 2;
    a.fw = g.width; a.fh = g.height; a.pad_x = g.pad_x; a.pad_y = g.pad_y;
    a.num0 = num0; a.den = den;
    a.magic = (uint32_t)((1ull << 32) / (unsigned)den + 1ull);
    set_runs(a, a.cw, L.height / 2);
    hipLaunchKernelGGL(k_subpel_interpolate_bgr<kSiRunsPerLane>, dim3((unsigned)cell_groups(c, kSiRunsPerLane), 1, (unsigned)count), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

int bbme_cells_subpel_interpolate_bgr_device(bbme_ctx *c, int pair, const int16_t *d_qf, const int16_t *d_qb, int q4_pitch_cells,
                                             const uint8_t *d_bgr1, const uint8_t *d_bgr2, int bgr_pitch, int num0, int count,
                                             int den, uint8_t *d_out, int out_pitch, size_t out_stride, void *hip_stream)
{
    const char *what = "bbme_cells_subpel_interpolate_bgr_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (!d_qf) return bbme::fail(BBME_ERR_INVALID, "%s: null forward grid", what);
    if (int rc = check_ip_bgr(c, num0, count, den, d_out, out_pitch, out_stride, what)) return rc;
    if (q4_pitch_cells < c->lv[0].width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch_cells, c->lv[0].width / 2);
    if ((d_bgr1 == nullptr) != (d_bgr2 == nullptr))
        return bbme::fail(BBME_ERR_INVALID, "%s: one colour frame without the other (both, or neither for the stored colour)", what);
    if (d_bgr1 && (long long)bgr_pitch < 3LL * c->geom.width)
        return bbme::fail(BBME_ERR_INVALID, "%s: colour pitch %d < 3 x frame width %d", what, bgr_pitch, c->geom.width);
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    const uint8_t *bgr1 = c->direction ? d_bgr2 : d_bgr1, *bgr2 = c->direction ? d_bgr1 : d_bgr2;
    if (!d_bgr1) {
        if (int rc = stored_bgr(c, pair, what, &bgr1, &bgr2)) return rc;
        bgr_pitch = 3 * c->geom.width;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_si_bgr(c, pair, reinterpret_cast<const mv_t *>(d_qf), reinterpret_cast<const mv_t *>(d_qb), q4_pitch_cells, bgr1, bgr2,
                          bgr_pitch, num0, count, den, d_out, out_pitch, out_stride, stream);
}

// what the two calls on the context's own two fields and stored colour share; before anything is enqueued.  Touches no device.
static int check_si_bgr_own(const bbme_ctx *c, int pair, int num0, int count, int den, const uint8_t *d_out, int out_pitch,
                            size_t out_stride, const char *what)
{
    if (int rc = check_ip_bgr(c, num0, count, den, d_out, out_pitch, out_stride, what)) return rc;
    if (int rc = check_sp(c, nullptr, what)) return rc;
    if (int rc = check_fields_state(c, what)) return rc;
    const uint8_t *bgr1 = nullptr, *bgr2 = nullptr;
    return stored_bgr(c, pair, what, &bgr1, &bgr2);
}

// the context's own two fields of `pair` refined (refine_own_si) and its stored colour, on `stream`
static int enqueue_own_si_bgr(bbme_ctx *c, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch, size_t out_stride,
                              hipStream_t stream, const char *what)
{
    const uint8_t *bgr1 = nullptr, *bgr2 = nullptr;
    if (int rc = stored_bgr(c, pair, what, &bgr1, &bgr2)) return rc;
    mv_t *q4[2];
    int cw;
    size_t cells;
    if (int rc = refine_own_si(c, pair, 1, stream, what, q4, &cw, &cells)) return rc;
    return enqueue_si_bgr(c, pair, q4[0], q4[1], cw, bgr1, bgr2, 3 * c->geom.width, num0, count, den, d_out, out_pitch, out_stride,
                          stream);
}

int bbme_subpel_interpolate_bgr_device(bbme_ctx *c, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch,
                                       size_t out_stride, void *hip_stream)
{
    const char *what = "bbme_subpel_interpolate_bgr_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_si_bgr_own(c, pair, num0, count, den, d_out, out_pitch, out_stride, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_si_bgr(c, pair, num0, count, den, d_out, out_pitch, out_stride, stream, what);
}

int bbme_get_subpel_interpolated_bgr_host(bbme_ctx *c, int pair, int num, int den, uint8_t *out)
{
    const char *what = "bbme_get_subpel_interpolated_bgr_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_si_bgr_own(c, pair, num, 1, den, out, 3 * c->geom.width, 0, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return download_staged(c, (size_t)3 * c->geom.width * c->geom.height, "the quarter-pel interpolated colour frame", out,
                           [&](uint8_t *d) {
        return enqueue_own_si_bgr(c, pair, num, 1, den, d, 3 * c->geom.width, 0, c->stream, what);
    });
}

// ---- temporal filter along quarter-pel grids (the SUBPEL TEMPORAL FILTER RULE of include/bbme.h; K13 k_subpel_temporal_filter) ----
// The third flavour of the temporal filter's one path (tf_cells .. tf_stats above): the grey flavour's planes and frames, the
// grids quarter-pel.  On the context's own frames the integer cells a launch reads are refined first (prepare).
struct TfSubpel : TfGrey {
    using Args = TfSpArgs;
    static constexpr bool subpel = true;
    static constexpr const char *staging_what = "the quarter-pel filtered frame", *stats_what = "the subpel temporal filter statistics";
    static auto kernel() { return k_subpel_temporal_filter<kTfRunsPerLane>; }
    static StatsScratch &stats(bbme_ctx *c) { return c->tfs_stats; }
    static void geometry(const bbme_ctx *c, TfSpArgs &a) { a.q4_pitch = c->lv[0].width / 2; }
    static int check_own(const bbme_ctx *c, const char *what) { return check_sp(c, nullptr, what); }
    // The forward cells of every pair the launch reads as a grid into a next frame and the backward cells of every pair it reads
    // as a grid into a previous one, each set refined by one k_subpel_refine launch into the context's quarter-pel buffer (the
    // packed forward grids of every pair, then the backward ones); then the arguments' grids are those, addressed as tf_own_fill
    // addresses the integer ones.
    template <class Args>
    static int prepare(bbme_ctx *c, Args &a, int pair0, int pairs, int first, int count, hipStream_t stream, const char *what)
    {
        const Level &L = c->lv[0];
        const int cw = L.width / 2, last = first + count - 1;
        const long long cells = (long long)cw * (L.height / 2);
        const size_t s_plane = L.plane_stride;
        if (int rc = c->tfs_q4.ensure(2 * (size_t)cells * c->batch, "the quarter-pel cells of the temporal filter", Fill::poison)) return rc;
        mv_t *q4[2] = {c->tfs_q4.get(), c->tfs_q4 + (size_t)c->batch * cells};
        // chain: slot s reads forward pair s (s < batch) and backward pair s - 1 (s > 0); pair or batch: image 1 forward, image 2 backward
        const int p0[2] = {c->chain ? first : pair0, c->chain ? std::max(first, 1) - 1 : pair0};
        const int n[2] = {c->chain ? std::min(last, c->batch - 1) - p0[0] + 1 : (first == 0 ? pairs : 0),
                          c->chain ? last - 1 - p0[1] + 1 : (last >= 1 ? pairs : 0)};
        for (int which = 0; which < 2; ++which) {
            if (n[which] < 1) continue;
            const uint8_t *i1, *i2;
            const mv_t *grid;
            uint32_t s_grid;
            if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
            if (int rc = enqueue_sp(c, i1 + p0[which] * s_plane, i2 + p0[which] * s_plane, s_plane, grid + (size_t)p0[which] * s_grid, s_grid,
                                    n[which], nullptr, q4[which] + (size_t)p0[which] * cells, cw, (size_t)cells, nullptr, nullptr, stream))
                return rc;
        }
        const uintptr_t f = reinterpret_cast<uintptr_t>(q4[0]), b = reinterpret_cast<uintptr_t>(q4[1]);
        const long long prev_pair = c->chain ? first - 1 : pair0, next_pair = c->chain ? first : pair0;
        a.gp = reinterpret_cast<const mv_t *>(b + prev_pair * cells * (long long)sizeof(mv_t));
        a.gn = reinterpret_cast<const mv_t *>(f + next_pair * cells * (long long)sizeof(mv_t));
        a.gp_y = a.gn_y = c->chain ? 0 : cells;
        a.gp_z = a.gn_z = c->chain ? cells : 0;
        return BBME_OK;
    }
};

int bbme_cells_subpel_temporal_filter_device(bbme_ctx *c, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next,
                                             const int16_t *d_q_to_prev, const int16_t *d_q_to_next, int q4_pitch_cells, int thr,
                                             const int *window, uint8_t *d_out, int out_pitch, uint8_t *d_weights, int weights_pitch,
                                             unsigned long long *d_stats4, void *hip_stream)
{
    return tf_cells<TfSubpel>(c, "bbme_cells_subpel_temporal_filter_device", d_prev, d_cur, d_next, c ? c->lv[0].width : 0, d_q_to_prev,
                              d_q_to_next, thr, window, d_out, out_pitch, d_weights, weights_pitch, d_stats4, hip_stream, q4_pitch_cells);
}

int bbme_subpel_temporal_filter_device(bbme_ctx *c, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream)
{
    return tf_device<TfSubpel>(c, "bbme_subpel_temporal_filter_device", pair, which, thr, d_out, out_pitch, hip_stream);
}

int bbme_subpel_temporal_filter_chain_device(bbme_ctx *c, int first, int count, int thr, uint8_t *d_out, int out_pitch, size_t out_stride,
                                             void *hip_stream)
{
    return tf_chain<TfSubpel>(c, "bbme_subpel_temporal_filter_chain_device", first, count, thr, d_out, out_pitch, out_stride, hip_stream);
}

int bbme_get_subpel_temporal_filtered_host(bbme_ctx *c, int pair, int which, int thr, uint8_t *out)
{
    return tf_host<TfSubpel>(c, "bbme_get_subpel_temporal_filtered_host", pair, which, thr, out);
}

int bbme_subpel_temporal_filter_stats(bbme_ctx *c, int thr, const int *window, unsigned long long *stats)
{
    return tf_stats<TfSubpel>(c, "bbme_subpel_temporal_filter_stats", thr, window, stats);
}

// ---- the same on the B,G,R frames (the BGR SUBPEL TEMPORAL FILTER RULE of include/bbme.h; K13b k_subpel_temporal_filter_bgr) ----
// The fourth flavour: the colour flavour's frames, colour checks and output checks, the quarter-pel flavour's refusals and
// refinement.  The cells are refined on the LUMA planes, into the quarter-pel buffer the grey flavour uses (the same cells of the
// same planes give the same vectors); the filter launch then reads only colour.
struct TfSubpelBgr : TfBgr {
    using Args = TfSpBgrArgs;
    static constexpr bool subpel = true;
    static constexpr const char *staging_what = "the quarter-pel filtered colour frame",
                                *stats_what = "the colour subpel temporal filter statistics";
    static auto kernel() { return k_subpel_temporal_filter_bgr<kTfRunsPerLane>; }
    static StatsScratch &stats(bbme_ctx *c) { return c->tfsb_stats; }
    static void geometry(const bbme_ctx *c, TfSpBgrArgs &a) { TfBgr::geometry(c, a); a.q4_pitch = c->lv[0].width / 2; }
    static int check_own(const bbme_ctx *c, const char *what) { return check_sp(c, nullptr, what); }
    static int prepare(bbme_ctx *c, TfSpBgrArgs &a, int pair0, int pairs, int first, int count, hipStream_t stream, const char *what)
    {
        return TfSubpel::prepare(c, a, pair0, pairs, first, count, stream, what);
    }
};

int bbme_cells_subpel_temporal_filter_bgr_device(bbme_ctx *c, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next,
                                                 int bgr_pitch, const int16_t *d_q_to_prev, const int16_t *d_q_to_next, int q4_pitch_cells,
                                                 int thr, const int *window, uint8_t *d_out, int out_pitch, uint8_t *d_weights,
                                                 int weights_pitch, unsigned long long *d_stats4, void *hip_stream)
{
    return tf_cells<TfSubpelBgr>(c, "bbme_cells_subpel_temporal_filter_bgr_device", d_prev, d_cur, d_next, bgr_pitch, d_q_to_prev,
                                 d_q_to_next, thr, window, d_out, out_pitch, d_weights, weights_pitch, d_stats4, hip_stream, q4_pitch_cells);
}

int bbme_subpel_temporal_filter_bgr_device(bbme_ctx *c, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream)
{
    return tf_device<TfSubpelBgr>(c, "bbme_subpel_temporal_filter_bgr_device", pair, which, thr, d_out, out_pitch, hip_stream);
}

int bbme_subpel_temporal_filter_bgr_chain_device(bbme_ctx *c, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                                 size_t out_stride, void *hip_stream)
{
    return tf_chain<TfSubpelBgr>(c, "bbme_subpel_temporal_filter_bgr_chain_device", first, count, thr, d_out, out_pitch, out_stride, hip_stream);
}

int bbme_get_subpel_temporal_filtered_bgr_host(bbme_ctx *c, int pair, int which, int thr, uint8_t *out)
{
    return tf_host<TfSubpelBgr>(c, "bbme_get_subpel_temporal_filtered_bgr_host", pair, which, thr, out);
}

int bbme_subpel_temporal_filter_bgr_stats(bbme_ctx *c, int thr, const int *window, unsigned long long *stats)
{
    return tf_stats<TfSubpelBgr>(c, "bbme_subpel_temporal_filter_bgr_stats", thr, window, stats);
}

// ---- composition of two cell grids (the CELL COMPOSITION RULE of include/bbme.h; K14 k_compose_cells) ----------------------------

// k_compose_cells over `count` frames (blockIdx.z) and, with d_results, k_mc_reduce of its partials into d_results[4 z ..]
static int enqueue_cmp(bbme_ctx *c, CmpArgs &a, int count, const int *window, unsigned long long *partial,
                       unsigned long long *d_results, hipStream_t stream)
{
    a.cw = c->lv[0].width / 2; a.ch = c->lv[0].height / 2;
    set_window(a, window, a.cw, a.ch);
    set_runs(a, a.cw, a.ch);
    return launch_gather(k_compose_cells<kCmpRunsPerLane>, a, cell_groups(c, kCmpRunsPerLane), 1, count, partial, d_results, stream);
}

int bbme_cells_compose_device(bbme_ctx *c, const int16_t *d_a, int a_pitch_cells, const int16_t *d_b, int b_pitch_cells, int unit_shift,
                              const int *window, int16_t *d_out, int out_pitch_cells, unsigned long long *d_stats2, void *hip_stream)
{
    const char *what = "bbme_cells_compose_device";
    if (int rc = check_ctx(c)) return rc;
    const int cw = c->lv[0].width / 2, ch = c->lv[0].height / 2;
    if (!d_a || !d_b || (!d_out && !d_stats2)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (a_pitch_cells < cw || b_pitch_cells < cw || (d_out && out_pitch_cells < cw))
        return bbme::fail(BBME_ERR_INVALID, "%s: a grid pitch < %d cells per row", what, cw);
    if (unit_shift != 0 && unit_shift != 2) return bbme::fail(BBME_ERR_INVALID, "%s: unit shift %d (0 or 2)", what, unit_shift);
    if (int rc = check_window(window, cw, ch, what, -1)) return rc;
    const uint8_t *o = reinterpret_cast<const uint8_t *>(d_out);
    if (d_out && (overlaps_input(o, out_pitch_cells * 4, {reinterpret_cast<const uint8_t *>(d_a)}, a_pitch_cells * 4, cw * 4, ch) ||
                  overlaps_input(o, out_pitch_cells * 4, {reinterpret_cast<const uint8_t *>(d_b)}, b_pitch_cells * 4, cw * 4, ch)))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input grid", what);
    HIP_TRY(hipSetDevice(c->device));
    // one result quadruple, then one launch's partials: one size per context
    if (d_stats2) if (int rc = c->cmp_stats.ensure(1, cell_groups(c, kCmpRunsPerLane), 0, 1, "the composition statistics")) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    CmpArgs a{};
    a.a = reinterpret_cast<const mv_t *>(d_a); a.b = reinterpret_cast<const mv_t *>(d_b); a.out = reinterpret_cast<mv_t *>(d_out);
    a.a_pitch = a_pitch_cells; a.b_pitch = b_pitch_cells; a.out_pitch = out_pitch_cells; a.ushift = unit_shift;
    if (int rc = enqueue_cmp(c, a, 1, window, c->cmp_stats.partials_caller(), d_stats2 ? c->cmp_stats.results() : nullptr, stream)) return rc;
    if (d_stats2)      // the first two words of the quadruple
        HIP_TRY(hipMemcpyAsync(d_stats2, c->cmp_stats.results(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
    return BBME_OK;
}

// The chain's own: for slots lo .. lo + n - 1 the integer grid into slot + 2 (side > 0: the forward cells of pair slot, then those
// of pair slot + 1) or into slot - 2 (the backward cells of pair slot - 1, then those of pair slot - 2), one launch
static int enqueue_cmp_chain(bbme_ctx *c, int lo, int n, int side, mv_t *d_out, int out_pitch, size_t out_stride, hipStream_t stream)
{
    const Level &L = c->lv[0];
    CmpArgs a{};
    if (side > 0) {
        a.a_z = a.b_z = L.grid_stride(L.final_grid());
        a.a = L.final_grid() + lo * a.a_z; a.b = a.a + a.a_z;
    } else {
        a.a_z = a.b_z = c->bwd_stride;
        a.a = c->bwd_cells.get() + (lo - 1) * a.a_z; a.b = a.a - a.a_z;
    }
    a.out = d_out; a.out_pitch = out_pitch; a.out_stride = out_stride;
    a.a_pitch = a.b_pitch = L.width / 2;
    return enqueue_cmp(c, a, n, nullptr, nullptr, nullptr, stream);
}

int bbme_compose_chain_device(bbme_ctx *c, int first, int count, int side, int16_t *d_out, int out_pitch_cells, size_t out_stride_cells,
                              void *hip_stream)
{
    const char *what = "bbme_compose_chain_device";
    if (int rc = chain_context_only(c, what)) return rc;
    const int cw = c->lv[0].width / 2, ch = c->lv[0].height / 2;
    if (side != 1 && side != -1) return bbme::fail(BBME_ERR_INVALID, "%s: side %d (+1 or -1)", what, side);
    const int lo = side > 0 ? 0 : 2, hi = side > 0 ? c->batch - 2 : c->batch;
    if (count < 1 || first < lo || (long long)first + count - 1 > hi)
        return bbme::fail(BBME_ERR_INVALID, "%s: slots %d .. %d + %d - 1 are not inside %d .. %d, the slots with a slot two %s", what,
                          first, first, count, lo, hi, side > 0 ? "on" : "back");
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (out_pitch_cells < cw) return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < %d cells per row", what, out_pitch_cells, cw);
    if (count > 1 && out_stride_cells < (size_t)out_pitch_cells * ch)
        return bbme::fail(BBME_ERR_INVALID, "%s: output stride %zu < one grid of %d rows of %d cells", what, out_stride_cells, ch,
                          out_pitch_cells);
    if (int rc = check_fields_state(c, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_cmp_chain(c, first, count, side, reinterpret_cast<mv_t *>(d_out), out_pitch_cells, out_stride_cells, stream);
}

// ---- temporal filter over two frames on each side (the WIDE TEMPORAL FILTER RULE of include/bbme.h; K15 k_wide_temporal_filter) ----
// A path of its own beside the temporal filter's flavours: four neighbours, six statistics and chain contexts only.

// Statistics scratch: two result quadruples per slot ({w_k > 0}, {weights, |out - C|, 0, 0}), two more for a caller's launch,
// then the partials of a launch over every slot and those of a caller's: one size per context
static int wide_scratch(bbme_ctx *c, StatsScratch &s, const char *what = "the wide temporal filter statistics")
{
    return s.ensure(2 * kTfMaxFrames + 2, tf_groups(c), 2 * c->frames(), 2, what);
}

static int wide_scratch(bbme_ctx *c) { return wide_scratch(c, c->wide_stats); }

static unsigned long long *wide_results_caller(StatsScratch &s) { return s.results() + (size_t)4 * 2 * kTfMaxFrames; }
static unsigned long long *wide_results_caller(bbme_ctx *c) { return wide_results_caller(c->wide_stats); }

static WtfArgs wide_args(const bbme_ctx *c, int thr, const int *window)
{
    const Level &L = c->lv[0];
    WtfArgs a{};
    a.width = L.width; a.height = L.height; a.cw = L.width / 2; a.ch = L.height / 2;
    a.thr = thr;
    a.magic_thr = thr > 1 ? (uint32_t)((1ull << 32) / (unsigned)thr + 1ull) : 0u;      // thr = 1: the kernel does not divide
    for (int S = 8; S <= 40; ++S) a.magic_s[S - 8] = (uint32_t)((1ull << 32) / (unsigned)S + 1ull);
    a.q4_pitch = a.cw;
    set_window(a, window, a.cw, a.ch);
    set_runs(a, a.cw, a.ch);
    return a;
}

static auto wide_kernel(const WtfArgs &) { return k_wide_temporal_filter<kTfRunsPerLane>; }
static auto wide_kernel(const WtfBgrArgs &) { return k_wide_temporal_filter_bgr<kTfRunsPerLane>; }

// k_wide_temporal_filter (WtfArgs) or k_wide_temporal_filter_bgr (WtfBgrArgs) over `count` frames and, with d_results, k_mc_reduce
// of its partials into d_results[8 z ..]
template <class Args>
static int enqueue_wide(bbme_ctx *c, Args &a, int count, unsigned long long *partial, unsigned long long *d_results, hipStream_t stream)
{
    const long long groups = tf_groups(c);
    a.partial = d_results ? partial : nullptr;
    hipLaunchKernelGGL(wide_kernel(a), dim3((unsigned)groups, 1u, (unsigned)count), dim3(256), 0, stream, a);
    if (d_results) hipLaunchKernelGGL(k_mc_reduce, dim3(2u * (unsigned)count), dim3(256), 0, stream, a.partial, (int)groups, d_results);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

int bbme_cells_wide_temporal_filter_device(bbme_ctx *c, const uint8_t *const d_planes[4], const uint8_t *d_cur,
                                           const int16_t *const d_grids[4], int q4_pitch_cells, int thr, const int *window, uint8_t *d_out,
                                           int out_pitch, uint16_t *d_weights, int weights_pitch, unsigned long long *d_stats6,
                                           void *hip_stream)
{
    const char *what = "bbme_cells_wide_temporal_filter_device";
    if (int rc = check_ctx(c)) return rc;
    const Level &L = c->lv[0];
    if (!d_planes || !d_grids || !d_cur || (!d_out && !d_weights && !d_stats6)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (q4_pitch_cells < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch_cells, L.width / 2);
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if ((d_planes[k] == nullptr) != (d_grids[k] == nullptr))
            return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its plane and its grid", what);
        any = any || d_planes[k];
    }
    if (!any) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (int rc = check_tf(c, thr, window, what)) return rc;
    if (d_out) if (int rc = check_frames(1, out_pitch, 0, L.width, L.height, what, "output")) return rc;
    if (d_weights && weights_pitch < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: weight map pitch %d < %d cells per row", what, weights_pitch, L.width / 2);
    if (d_out && overlaps_input(d_out, out_pitch, {d_cur, d_planes[0], d_planes[1], d_planes[2], d_planes[3]}, L.width, L.width, L.height))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input plane", what);
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats6) if (int rc = wide_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    WtfArgs a = wide_args(c, thr, window);
    a.cur = d_cur;
    for (int k = 0; k < 4; ++k) { a.x[k] = d_planes[k]; a.g[k] = reinterpret_cast<const mv_t *>(d_grids[k]); }
    a.q4_pitch = q4_pitch_cells;
    a.first_prev = a.last_next = 2;
    a.out = d_out; a.out_pitch = out_pitch;
    a.wmap = d_weights; a.wmap_pitch = weights_pitch;
    if (int rc = enqueue_wide(c, a, 1, c->wide_stats.partials_caller(), d_stats6 ? wide_results_caller(c) : nullptr, stream)) return rc;
    if (d_stats6)      // the first six words of the two quadruples
        HIP_TRY(hipMemcpyAsync(d_stats6, wide_results_caller(c), 6 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
    return BBME_OK;
}

// The chain's slots first .. first + count - 1 as the kernel addresses them, every grid a launch reads made on `stream` first:
// the +-1 grids are the subpel temporal filter's, refined into its buffer by its own prepare (at most two K10 launches); the +-2
// grids are composed (one K14 launch a side) into wide_cells and refined against (slot, slot +- 2) into wide_q4 (one K10 launch a
// side).  Both buffers hold, packed, the grids into slot f - 2 of every slot f, then those into slot f + 2.
static int wide_prepare(bbme_ctx *c, WtfArgs &a, int first, int count, hipStream_t stream, const char *what)
{
    const Level &L = c->lv[0];
    const int cw = L.width / 2, slots = c->batch + 1, last = first + count - 1;
    const long long cells = (long long)cw * (L.height / 2), s_plane = L.plane_stride;
    TfSpArgs adj{};
    if (int rc = TfSubpel::prepare(c, adj, 0, 1, first, count, stream, what)) return rc;
    if (int rc = c->wide_cells.ensure(2 * (size_t)cells * slots, "the composed cells of the wide temporal filter", Fill::poison)) return rc;
    if (int rc = c->wide_q4.ensure(2 * (size_t)cells * slots, "the quarter-pel cells of the wide temporal filter", Fill::poison)) return rc;
    const uintptr_t cur = reinterpret_cast<uintptr_t>(L.img1.get()) + first * s_plane;
    a.cur = reinterpret_cast<const uint8_t *>(cur);
    a.plane_z = s_plane; a.g_z = cells;
    a.first_prev = std::min(first, 2); a.last_next = std::min(slots - 1 - last, 2);
    a.g[0] = adj.gp; a.g[1] = adj.gn;
    for (int k = 0; k < 4; ++k) {
        const long long step = (k & 1 ? 1 : -1) * (1 + (k >> 1));                    // slots from C to the neighbour
        a.x[k] = reinterpret_cast<const uint8_t *>(cur + step * s_plane);            // never read where the chain has no such slot
    }
    for (int side = 0; side < 2; ++side) {                                           // 0: into slot - 2 (P2), 1: into slot + 2 (N2)
        const int lo = side ? first : std::max(first, 2), hi = side ? std::min(last, slots - 3) : last;
        mv_t *cmp = c->wide_cells.get() + (size_t)side * slots * cells, *q4 = c->wide_q4.get() + (size_t)side * slots * cells;
        if (hi >= lo) {
            const uint8_t *i1 = L.img1.get() + (size_t)lo * s_plane, *i2 = L.img1.get() + (size_t)(lo + (side ? 2 : -2)) * s_plane;
            if (int rc = enqueue_cmp_chain(c, lo, hi - lo + 1, side ? 1 : -1, cmp + (size_t)lo * cells, cw, (size_t)cells, stream)) return rc;
            if (int rc = enqueue_sp(c, i1, i2, (size_t)s_plane, cmp + (size_t)lo * cells, (size_t)cells, hi - lo + 1, nullptr,
                                    q4 + (size_t)lo * cells, cw, (size_t)cells, nullptr, nullptr, stream))
                return rc;
        }
        a.g[2 + side] = q4 + (size_t)first * cells;
    }
    return BBME_OK;
}

// what the context-level calls of the wide filter share: a chain, the strength and window, 8188, the context's state
static int check_wide_own(const bbme_ctx *c, int thr, const int *window, const char *what)
{
    if (int rc = chain_context_only(c, what)) return rc;
    if (int rc = check_tf(c, thr, window, what)) return rc;
    if (int rc = check_sp(c, nullptr, what)) return rc;
    return check_fields_state(c, what);
}

static int enqueue_own_wide(bbme_ctx *c, const char *what, int first, int count, int thr, uint8_t *d_out, int out_pitch, size_t out_stride,
                            hipStream_t stream)
{
    WtfArgs a = wide_args(c, thr, nullptr);
    if (int rc = wide_prepare(c, a, first, count, stream, what)) return rc;
    a.out = d_out; a.out_pitch = out_pitch; a.out_stride = out_stride;
    return enqueue_wide(c, a, count, nullptr, nullptr, stream);
}

int bbme_wide_temporal_filter_chain_device(bbme_ctx *c, int first, int count, int thr, uint8_t *d_out, int out_pitch, size_t out_stride,
                                           void *hip_stream)
{
    const char *what = "bbme_wide_temporal_filter_chain_device";
    if (int rc = chain_context_only(c, what)) return rc;
    if (first < 0 || count < 1 || (long long)first + count > c->batch + 1)
        return bbme::fail(BBME_ERR_INVALID, "%s: slots %d .. %d + %d - 1 are not inside 0 .. %d", what, first, first, count, c->batch);
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_frames(count, out_pitch, out_stride, c->lv[0].width, c->lv[0].height, what, "output")) return rc;
    if (int rc = check_wide_own(c, thr, nullptr, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_wide(c, what, first, count, thr, d_out, out_pitch, out_stride, stream);
}

int bbme_get_wide_temporal_filtered_host(bbme_ctx *c, int slot, int thr, uint8_t *out)
{
    const char *what = "bbme_get_wide_temporal_filtered_host";
    if (int rc = chain_context_only(c, what)) return rc;
    if (slot < 0 || slot > c->batch) return bbme::fail(BBME_ERR_INVALID, "%s: slot %d is not inside 0 .. %d", what, slot, c->batch);
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_wide_own(c, thr, nullptr, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int w = c->lv[0].width;
    return download_staged(c, (size_t)w * c->lv[0].height, "the wide filtered frame", out, [&](uint8_t *d) {
        return enqueue_own_wide(c, what, slot, 1, thr, d, w, 0, c->stream);
    });
}

int bbme_wide_temporal_filter_stats(bbme_ctx *c, int thr, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_wide_temporal_filter_stats";
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_wide_own(c, thr, window, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = wide_scratch(c)) return rc;
    const int slots = c->batch + 1;
    std::vector<unsigned long long> s((size_t)8 * slots);
    WtfArgs a = wide_args(c, thr, window);
    if (int rc = download_stats(c, c->wide_stats, 2 * slots, s.data(), [&] {
            if (int rc = wide_prepare(c, a, 0, slots, c->stream, what)) return rc;
            return enqueue_wide(c, a, slots, c->wide_stats.partials_all(), c->wide_stats.results(), c->stream);
        }))
        return rc;
    for (int f = 0; f < slots; ++f)
        for (int k = 0; k < 6; ++k) stats[6 * f + k] = s[8 * f + k];
    return BBME_OK;
}

// ---- the same on the B,G,R frames (the BGR WIDE TEMPORAL FILTER RULE of include/bbme.h; K15b k_wide_temporal_filter_bgr) ---------
// The wide path's arguments, grids and launch (wide_args, wide_prepare, enqueue_wide) with the colour flavour's frames, colour
// checks and output checks.  The grids are made on the LUMA planes into the buffers the grey wide calls use (the same cells of the
// same planes give the same vectors); the filter launch then reads only colour.

static WtfBgrArgs wide_bgr_args(const bbme_ctx *c, int thr, const int *window)
{
    WtfBgrArgs a{};
    static_cast<WtfArgs &>(a) = wide_args(c, thr, window);
    a.fw = c->geom.width; a.fh = c->geom.height; a.pad_x = c->geom.pad_x; a.pad_y = c->geom.pad_y;
    a.bgr_pitch = 3 * c->geom.width;
    return a;
}

int bbme_cells_wide_temporal_filter_bgr_device(bbme_ctx *c, const uint8_t *const d_frames[4], const uint8_t *d_cur, int bgr_pitch,
                                               const int16_t *const d_grids[4], int q4_pitch_cells, int thr, const int *window,
                                               uint8_t *d_out, int out_pitch, uint16_t *d_weights, int weights_pitch,
                                               unsigned long long *d_stats6, void *hip_stream)
{
    const char *what = "bbme_cells_wide_temporal_filter_bgr_device";
    if (int rc = check_ctx(c)) return rc;
    const Level &L = c->lv[0];
    if (!d_frames || !d_grids || !d_cur || (!d_out && !d_weights && !d_stats6)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (q4_pitch_cells < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch_cells, L.width / 2);
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if ((d_frames[k] == nullptr) != (d_grids[k] == nullptr))
            return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its frame and its grid", what);
        any = any || d_frames[k];
    }
    if (!any) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (int rc = check_tf(c, thr, window, what)) return rc;
    if ((long long)bgr_pitch < 3LL * c->geom.width)
        return bbme::fail(BBME_ERR_INVALID, "%s: colour pitch %d < 3 x frame width %d", what, bgr_pitch, c->geom.width);
    if (d_out) if (int rc = check_bgr_frames(c, 1, out_pitch, 0, what)) return rc;
    if (d_weights && weights_pitch < L.width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: weight map pitch %d < %d cells per row", what, weights_pitch, L.width / 2);
    if (d_out && overlaps_input(d_out, out_pitch, {d_cur, d_frames[0], d_frames[1], d_frames[2], d_frames[3]}, bgr_pitch,
                                3 * c->geom.width, c->geom.height))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input frame", what);
    HIP_TRY(hipSetDevice(c->device));
    StatsScratch &scratch = c->wide_bgr_stats;
    if (d_stats6) if (int rc = wide_scratch(c, scratch, "the colour wide temporal filter statistics")) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    WtfBgrArgs a = wide_bgr_args(c, thr, window);
    a.cur = d_cur; a.bgr_pitch = bgr_pitch;
    for (int k = 0; k < 4; ++k) { a.x[k] = d_frames[k]; a.g[k] = reinterpret_cast<const mv_t *>(d_grids[k]); }
    a.q4_pitch = q4_pitch_cells;
    a.first_prev = a.last_next = 2;
    a.out = d_out; a.out_pitch = out_pitch;
    a.wmap = d_weights; a.wmap_pitch = weights_pitch;
    if (int rc = enqueue_wide(c, a, 1, scratch.partials_caller(), d_stats6 ? wide_results_caller(scratch) : nullptr, stream)) return rc;
    if (d_stats6)      // the first six words of the two quadruples
        HIP_TRY(hipMemcpyAsync(d_stats6, wide_results_caller(scratch), 6 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
    return BBME_OK;
}

// wide_prepare's grids for slots first .. first + count - 1, then the frames those slots have in the colour store (slots
// bgr_stride bytes apart, in 64 bits: a deep chain's store exceeds 4 GB).  A base the launch never dereferences is address
// arithmetic only.
static int wide_bgr_prepare(bbme_ctx *c, WtfBgrArgs &a, int first, int count, hipStream_t stream, const char *what)
{
    if (int rc = wide_prepare(c, a, first, count, stream, what)) return rc;
    const long long s_slot = (long long)c->bgr_stride;
    const uintptr_t cur = reinterpret_cast<uintptr_t>(c->bgr.get()) + first * s_slot;
    a.cur = reinterpret_cast<const uint8_t *>(cur);
    a.plane_z = s_slot;
    for (int k = 0; k < 4; ++k) {
        const long long step = (k & 1 ? 1 : -1) * (1 + (k >> 1));                    // slots from C to the neighbour
        a.x[k] = reinterpret_cast<const uint8_t *>(cur + step * s_slot);
    }
    return BBME_OK;
}

// what the context-level calls of the colour wide filter share: check_wide_own, and stored colour in every slot that the slots
// first .. first + count - 1 read
static int check_wide_bgr_own(const bbme_ctx *c, int first, int count, int thr, const int *window, const char *what)
{
    if (int rc = check_wide_own(c, thr, window, what)) return rc;
    return check_tf_bgr_colour(c, first - 2, first + count + 1, what);
}

static int enqueue_own_wide_bgr(bbme_ctx *c, const char *what, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                size_t out_stride, hipStream_t stream)
{
    WtfBgrArgs a = wide_bgr_args(c, thr, nullptr);
    if (int rc = wide_bgr_prepare(c, a, first, count, stream, what)) return rc;
    a.out = d_out; a.out_pitch = out_pitch; a.out_stride = out_stride;
    return enqueue_wide(c, a, count, nullptr, nullptr, stream);
}

int bbme_wide_temporal_filter_bgr_chain_device(bbme_ctx *c, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                               size_t out_stride, void *hip_stream)
{
    const char *what = "bbme_wide_temporal_filter_bgr_chain_device";
    if (int rc = chain_context_only(c, what)) return rc;
    if (first < 0 || count < 1 || (long long)first + count > c->batch + 1)
        return bbme::fail(BBME_ERR_INVALID, "%s: slots %d .. %d + %d - 1 are not inside 0 .. %d", what, first, first, count, c->batch);
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_bgr_frames(c, count, out_pitch, out_stride, what)) return rc;
    if (int rc = check_wide_bgr_own(c, first, count, thr, nullptr, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_wide_bgr(c, what, first, count, thr, d_out, out_pitch, out_stride, stream);
}

int bbme_get_wide_temporal_filtered_bgr_host(bbme_ctx *c, int slot, int thr, uint8_t *out)
{
    const char *what = "bbme_get_wide_temporal_filtered_bgr_host";
    if (int rc = chain_context_only(c, what)) return rc;
    if (slot < 0 || slot > c->batch) return bbme::fail(BBME_ERR_INVALID, "%s: slot %d is not inside 0 .. %d", what, slot, c->batch);
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_wide_bgr_own(c, slot, 1, thr, nullptr, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int row = 3 * c->geom.width;
    return download_staged(c, (size_t)row * c->geom.height, "the wide filtered colour frame", out, [&](uint8_t *d) {
        return enqueue_own_wide_bgr(c, what, slot, 1, thr, d, row, 0, c->stream);
    });
}

int bbme_wide_temporal_filter_bgr_stats(bbme_ctx *c, int thr, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_wide_temporal_filter_bgr_stats";
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = chain_context_only(c, what)) return rc;
    if (int rc = check_wide_bgr_own(c, 0, c->batch + 1, thr, window, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    StatsScratch &scratch = c->wide_bgr_stats;
    if (int rc = wide_scratch(c, scratch, "the colour wide temporal filter statistics")) return rc;
    const int slots = c->batch + 1;
    std::vector<unsigned long long> s((size_t)8 * slots);
    WtfBgrArgs a = wide_bgr_args(c, thr, window);
    if (int rc = download_stats(c, scratch, 2 * slots, s.data(), [&] {
            if (int rc = wide_bgr_prepare(c, a, 0, slots, c->stream, what)) return rc;
            return enqueue_wide(c, a, slots, scratch.partials_all(), scratch.results(), c->stream);
        }))
        return rc;
    for (int f = 0; f < slots; ++f)
        for (int k = 0; k < 6; ++k) stats[6 * f + k] = s[8 * f + k];
    return BBME_OK;
}

// ---- global motion and global compensation (the GLOBAL MOTION RULE and the GLOBAL COMPENSATION RULE of include/bbme.h; K16 k_vector_histogram,
// K17 k_global_moments, K18 k_global_compensate) ------------------------------------------------------------------------------

// a grid and, optionally, its exclusion mask, of `pairs` pairs s_cells words / s_excl bytes apart
struct GmGrid {
    const mv_t *cells = nullptr;
    size_t s_cells = 0;
    int pitch = 0;
    const uint8_t *excl = nullptr;
    size_t s_excl = 0;
    int excl_pitch = 0;
};

static long long vh_groups(const bbme_ctx *c) { return std::min<long long>(cell_groups(c, 1), kVhMaxGroups); }
static long long gm_groups(const bbme_ctx *c) { return cell_groups(c, kGmRunsPerLane); }
static long long gc_groups(const bbme_ctx *c) { return gather_groups(c->lv[0].width, c->lv[0].height, kGcRunsPerLane); }

// gm_words: sixteen result words of every pair, K17's partials of a launch over every pair, then those of a caller's launch
static int gm_scratch(bbme_ctx *c)
{
    return c->gm_words.ensure((size_t)16 * (BBME_MAX_BATCH + gm_groups(c) * (c->batch + 1)), "the global motion moments", Fill::poison);
}
static unsigned long long *gm_partials_all(const bbme_ctx *c) { return c->gm_words + (size_t)16 * BBME_MAX_BATCH; }
static unsigned long long *gm_partials_caller(const bbme_ctx *c) { return gm_partials_all(c) + (size_t)16 * gm_groups(c) * c->batch; }

static int gc_scratch(bbme_ctx *c)
{
    return c->gc_stats.ensure(BBME_MAX_BATCH, gc_groups(c), c->batch, 1, "the global compensation statistics");
}

// geometry and a window in cells.  Touches no device.
static int check_gm(const bbme_ctx *c, const int *window, const char *what)
{
    const Level &L = c->lv[0];
    if (L.width > 8188 || L.height > 8188)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: a %dx%d plane is beyond 8188 (the moments would not stay exact)", what, L.width, L.height);
    return check_window(window, L.width / 2, L.height / 2, what, -1);
}

static int check_gm_tol(long long tol_q16, const char *what)
{
    if (tol_q16 < 0 || tol_q16 > (1LL << 40)) return bbme::fail(BBME_ERR_INVALID, "%s: tolerance %lld outside 0..2^40", what, tol_q16);
    return BBME_OK;
}

// a caller's grid and mask.  Touches no device.
static int check_gm_cells(const bbme_ctx *c, const int16_t *d_cells, int cells_pitch_cells, const uint8_t *d_exclude, int exclude_pitch,
                          const char *what, GmGrid *g)
{
    const int cw = c->lv[0].width / 2;
    if (!d_cells) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (cells_pitch_cells < cw) return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, cells_pitch_cells, cw);
    if (d_exclude && exclude_pitch < cw)
        return bbme::fail(BBME_ERR_INVALID, "%s: exclusion mask pitch %d < %d cells per row", what, exclude_pitch, cw);
    g->cells = reinterpret_cast<const mv_t *>(d_cells); g->pitch = cells_pitch_cells;
    g->excl = d_exclude; g->excl_pitch = exclude_pitch;
    return BBME_OK;
}

// the table zeroed, then k_vector_histogram over `pairs` pairs into it (2 BBME_GM_BINS words per pair)
static int enqueue_vh(bbme_ctx *c, const GmGrid &g, int pairs, const int *window, uint32_t *d_hist, hipStream_t stream)
{
    const Level &L = c->lv[0];
    VhArgs a{};
    a.cells = g.cells; a.s_cells = g.s_cells; a.pitch = g.pitch;
    a.excl = g.excl; a.s_excl = g.s_excl; a.excl_pitch = g.excl_pitch;
    a.hist = d_hist; a.cw = L.width / 2;
    set_window(a, window, L.width / 2, L.height / 2);
    set_runs(a, L.width / 2, L.height / 2);
    HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)pairs * 2 * BBME_GM_BINS * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_vector_histogram<BBME_GM_BINS>, dim3((unsigned)vh_groups(c), (unsigned)pairs), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

// k_global_moments over `pairs` pairs under the models of the device table d_models (six words per pair) or, without one, under
// `model`: the map (rows map_pitch, pairs s_map bytes apart) and / or, with d_words, the sixteen words of every pair
static int enqueue_gm(bbme_ctx *c, const GmGrid &g, int pairs, const int32_t *d_models, const int32_t *model, long long tol_q16,
                      const int *window, uint8_t *d_map, int map_pitch, size_t s_map, unsigned long long *partial,
                      unsigned long long *d_words, hipStream_t stream)
{
    const Level &L = c->lv[0];
    GmArgs a{};
    a.cells = g.cells; a.s_cells = g.s_cells; a.pitch = g.pitch;
    a.excl = g.excl; a.s_excl = g.s_excl; a.excl_pitch = g.excl_pitch;
    a.map = d_map; a.map_pitch = map_pitch; a.s_map = s_map;
    a.partial = d_words ? partial : nullptr;
    a.models = d_models;
    if (model) std::copy(model, model + 6, a.model);
    a.tol = tol_q16;
    a.cw = L.width / 2; a.ch = L.height / 2;
    set_window(a, window, a.cw, a.ch);
    set_runs(a, a.cw, a.ch);
    const long long groups = gm_groups(c);
    hipLaunchKernelGGL(k_global_moments<kGmRunsPerLane>, dim3((unsigned)groups, (unsigned)pairs), dim3(256), 0, stream, a);
    if (d_words) hipLaunchKernelGGL(k_reduce_words<16>, dim3((unsigned)pairs), dim3(256), 0, stream, a.partial, (int)groups, d_words);
    HIP_TRY(hipGetLastError());
    return BBME_OK;
}

// k_global_compensate over `pairs` pairs (planes s_plane bytes apart), models as for enqueue_gm: the frame into d_out (one pair
// only) and / or, with d_stats, the statistics over `window` in pixels
static int enqueue_gc(bbme_ctx *c, const uint8_t *img1, const uint8_t *img2, size_t s_plane, int pairs, const int32_t *d_models,
                      const int32_t *model, int unit, int fill, const int *window, uint8_t *d_out, int out_pitch,
                      unsigned long long *partial, unsigned long long *d_stats, hipStream_t stream)
{
    const Level &L = c->lv[0];
    GcArgs a{};
    a.img1 = img1; a.img2 = img2; a.out = d_out; a.s_plane = s_plane;
    a.models = d_models;
    if (model) std::copy(model, model + 6, a.model);
    a.width = L.width; a.height = L.height; a.mul = 4 / unit; a.fill = fill; a.out_pitch = out_pitch;
    set_window(a, window, L.width, L.height);
    set_runs(a, L.width, L.height);
    return launch_gather(k_global_compensate<kGcRunsPerLane>, a, gc_groups(c), pairs, 1, partial, d_stats, stream);
}

int bbme_cells_vector_histogram_device(bbme_ctx *c, const int16_t *d_cells, int cells_pitch_cells, const uint8_t *d_exclude,
                                       int exclude_pitch, const int *window, uint32_t *d_hist, void *hip_stream)
{
    const char *what = "bbme_cells_vector_histogram_device";
    if (int rc = check_ctx(c)) return rc;
    GmGrid g;
    if (int rc = check_gm_cells(c, d_cells, cells_pitch_cells, d_exclude, exclude_pitch, what, &g)) return rc;
    if (!d_hist) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_gm(c, window, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_vh(c, g, 1, window, d_hist, stream);
}

int bbme_cells_global_moments_device(bbme_ctx *c, const int16_t *d_cells, int cells_pitch_cells, const uint8_t *d_exclude,
                                     int exclude_pitch, const int32_t *model, long long tol_q16, const int *window, uint8_t *d_map,
                                     int map_pitch, long long *d_words16, void *hip_stream)
{
    const char *what = "bbme_cells_global_moments_device";
    if (int rc = check_ctx(c)) return rc;
    GmGrid g;
    if (int rc = check_gm_cells(c, d_cells, cells_pitch_cells, d_exclude, exclude_pitch, what, &g)) return rc;
    if (!model || (!d_map && !d_words16)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_gm_tol(tol_q16, what)) return rc;
    if (int rc = check_gm(c, window, what)) return rc;
    if (d_map && map_pitch < c->lv[0].width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: map pitch %d < %d cells per row", what, map_pitch, c->lv[0].width / 2);
    HIP_TRY(hipSetDevice(c->device));
    if (d_words16) if (int rc = gm_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_gm(c, g, 1, nullptr, model, tol_q16, window, d_map, map_pitch, 0, d_words16 ? gm_partials_caller(c) : nullptr,
                      reinterpret_cast<unsigned long long *>(d_words16), stream);
}

// What bbme_global_motion and bbme_get_global_motion_map_host check alike: the arguments, then the state.  Touches no device.
static int check_gm_own(const bbme_ctx *c, int which, int subpel, int mask_tol, long long tol_q16, const int *window, const char *what)
{
    if (int rc = check_ctx(c)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (subpel != 0 && subpel != 1) return bbme::fail(BBME_ERR_INVALID, "%s: subpel = %d (0 or 1)", what, subpel);
    if (int rc = check_gm_tol(tol_q16, what)) return rc;
    if (int rc = check_gm(c, window, what)) return rc;
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
    if (mask_tol >= 0 && !c->fields_valid) return bbme::fail(BBME_ERR_STATE, "%s: no valid bidirectional estimate for the mask", what);
    return BBME_OK;
}

// The cells the context's own calls fit, of `pairs` pairs from pair0 on: the cells of `which`, refined into gm_q4 with subpel,
// and with mask_tol >= 0 their consistency mask in gm_mask -- both made on `stream` first.  After check_gm_own.
static int gm_prepare(bbme_ctx *c, int pair0, int pairs, int which, int subpel, int mask_tol, hipStream_t stream, const char *what,
                      GmGrid *g)
{
    const Level &L = c->lv[0];
    const int cw = L.width / 2;
    const size_t cells = (size_t)cw * (L.height / 2), s_plane = L.plane_stride;
    const uint8_t *i1, *i2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
    g->cells = grid + (size_t)pair0 * s_grid; g->s_cells = s_grid; g->pitch = cw;
    if (subpel) {
        if (int rc = c->gm_q4.ensure(cells * c->batch, "the quarter-pel cells of the global motion", Fill::poison)) return rc;
        mv_t *q4 = c->gm_q4 + pair0 * cells;
        if (int rc = enqueue_sp(c, i1 + pair0 * s_plane, i2 + pair0 * s_plane, s_plane, g->cells, s_grid, pairs, nullptr, q4, cw, cells,
                                nullptr, nullptr, stream))
            return rc;
        g->cells = q4; g->s_cells = cells;
    }
    if (mask_tol >= 0) {
        if (int rc = c->gm_mask.ensure(cells * c->batch, "the consistency mask of the global motion", Fill::poison)) return rc;
        const uint32_t s_f = L.grid_stride(L.final_grid()), s_b = c->bwd_stride;
        const mv_t *f = L.final_grid() + (size_t)pair0 * s_f, *b = c->bwd_cells + (size_t)pair0 * s_b;
        FbArgs a{};
        a.a = which ? b : f; a.s_a = which ? s_b : s_f;
        a.b = which ? f : b; a.s_b = which ? s_f : s_b;
        a.mask = c->gm_mask + pair0 * cells; a.mask_pitch = cw; a.s_mask = cells;
        a.cw = cw; a.ch = L.height / 2; a.tol = mask_tol;
        set_window(a, nullptr, a.cw, a.ch);
        set_runs(a, a.cw, a.ch);
        if (int rc = launch_gather(k_fb_consistency, a, cell_groups(c, kFbRunsPerLane), pairs, 1, nullptr, nullptr, stream)) return rc;
        g->excl = a.mask; g->s_excl = cells; g->excl_pitch = cw;
    }
    return BBME_OK;
}

int bbme_global_motion(bbme_ctx *c, int which, int subpel, int kind, long long tol_q16, int iterations, int mask_tol, const int *window,
                       int32_t *models, long long *words)
{
    const char *what = "bbme_global_motion";
    if (int rc = check_gm_own(c, which, subpel, mask_tol, tol_q16, window, what)) return rc;
    if (kind != BBME_GM_TRANSLATION && kind != BBME_GM_AFFINE) return bbme::fail(BBME_ERR_INVALID, "%s: kind = %d (0 or 1)", what, kind);
    if (iterations < 0 || iterations > 8) return bbme::fail(BBME_ERR_INVALID, "%s: %d iterations (0..8)", what, iterations);
    if (!models || !words) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    HIP_TRY(hipSetDevice(c->device));
    const int P = c->batch;
    if (int rc = gm_scratch(c)) return rc;
    if (int rc = c->gm_hist.ensure((size_t)P * 2 * BBME_GM_BINS, "the global motion histograms", Fill::poison)) return rc;
    if (int rc = c->gm_models.ensure((size_t)6 * BBME_MAX_BATCH, "the global motion models", Fill::poison)) return rc;
    GmGrid g;
    if (int rc = gm_prepare(c, 0, P, which, subpel, mask_tol, c->stream, what, &g)) return rc;
    // step 1: the histograms of every pair, 16 KB each, and their medians
    std::vector<uint32_t> hist((size_t)P * 2 * BBME_GM_BINS);
    if (int rc = enqueue_vh(c, g, P, window, c->gm_hist, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(hist.data(), c->gm_hist, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (int rc = check_converged(c)) return rc;
    std::vector<uint8_t> done((size_t)P, 0);
    for (int p = 0; p < P; ++p) {
        const uint32_t *h = hist.data() + (size_t)p * 2 * BBME_GM_BINS;
        unsigned long long n = 0;
        for (int b = 0; b < BBME_GM_BINS; ++b) n += h[b];
        int32_t *m = models + 6 * p;
        std::fill(m, m + 6, 0);
        m[0] = bbme::global_median(h, n) * 65536;
        m[3] = bbme::global_median(h + BBME_GM_BINS, n) * 65536;
        done[p] = n == 0;
    }
    // steps 2 .. : a moments pass over every pair under the table of models, 128 bytes per pair down, the solve on the host; a pair
    // that is done (no cell, or no inlier) keeps its model and its words of these passes are not read.  The last pass is the result.
    for (int it = 0; it <= iterations; ++it) {
        const bool last = it == iterations || std::find(done.begin(), done.end(), 0) == done.end();
        HIP_TRY(hipMemcpyAsync(c->gm_models, models, (size_t)6 * P * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if (int rc = enqueue_gm(c, g, P, c->gm_models, nullptr, tol_q16, window, nullptr, 0, 0, gm_partials_all(c), c->gm_words, c->stream))
            return rc;
        HIP_TRY(hipMemcpyAsync(words, c->gm_words, (size_t)16 * P * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (last) break;
        for (int p = 0; p < P; ++p) {
            if (done[p]) continue;
            if (words[16 * p] == 0) { done[p] = 1; continue; }
            if (int rc = bbme_global_motion_solve_host(words + 16 * p, kind, models + 6 * p)) return rc;
        }
    }
    return BBME_OK;
}

int bbme_get_global_motion_map_host(bbme_ctx *c, int pair, int which, int subpel, int mask_tol, const int32_t *model, long long tol_q16,
                                    uint8_t *map)
{
    const char *what = "bbme_get_global_motion_map_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_gm_own(c, which, subpel, mask_tol, tol_q16, nullptr, what)) return rc;
    if (!model || !map) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    HIP_TRY(hipSetDevice(c->device));
    const int cw = c->lv[0].width / 2, ch = c->lv[0].height / 2;
    return download_staged(c, (size_t)cw * ch, "the global motion map", map, [&](uint8_t *d) {
        GmGrid g;
        if (int rc = gm_prepare(c, pair, 1, which, subpel, mask_tol, c->stream, what, &g)) return rc;
        return enqueue_gm(c, g, 1, nullptr, model, tol_q16, nullptr, d, cw, 0, nullptr, nullptr, c->stream);
    });
}

// unit, fill and a window in pixels.  Touches no device.
static int check_gc(const bbme_ctx *c, const int32_t *model, int unit, int fill, const int *window, const char *what)
{
    const Level &L = c->lv[0];
    if (!model) return bbme::fail(BBME_ERR_INVALID, "%s: null model", what);
    if (unit != 1 && unit != 4) return bbme::fail(BBME_ERR_INVALID, "%s: unit %d (1 or 4)", what, unit);
    if (int rc = check_fill(fill, what)) return rc;
    if (L.width > 8188 || L.height > 8188)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: a %dx%d plane is beyond 8188", what, L.width, L.height);
    return check_window(window, L.width, L.height, what, 0);
}

int bbme_cells_global_compensate_device(bbme_ctx *c, const uint8_t *d_image1, const uint8_t *d_image2, const int32_t *model, int unit,
                                        int fill, const int *window, uint8_t *d_out, int out_pitch, unsigned long long *d_stats4,
                                        void *hip_stream)
{
    const char *what = "bbme_cells_global_compensate_device";
    if (int rc = check_ctx(c)) return rc;
    const Level &L = c->lv[0];
    if (!d_image2 || (!d_out && !d_stats4) || (d_stats4 && !d_image1)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_gc(c, model, unit, fill, window, what)) return rc;
    if (d_out && out_pitch < L.width) return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < width %d", what, out_pitch, L.width);
    if (d_out && overlaps_input(d_out, out_pitch, {d_image1, d_image2}, L.width, L.width, L.height))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input plane", what);
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats4) if (int rc = gc_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_gc(c, d_image1, d_image2, 0, 1, nullptr, model, unit, fill, window, d_out, out_pitch, c->gc_stats.partials_caller(),
                      d_stats4, stream);
}

// the context's own planes of `which`, as sp_source names them: 0 predicts image 1 from image 2 of the context's direction, 1
// image 2 from image 1 (the planes the backward cells lie on)
static int gc_source(const bbme_ctx *c, int which, const char *what, const uint8_t **img1, const uint8_t **img2)
{
    const Level &L = c->lv[0];
    if (int rc = check_which(which, what)) return rc;
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    *img1 = which ? L.img2 : c->plane1(L);
    *img2 = which ? L.img1.get() : c->plane2(L);
    return BBME_OK;
}

int bbme_global_compensate_device(bbme_ctx *c, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *d_out,
                                  int out_pitch, void *hip_stream)
{
    const char *what = "bbme_global_compensate_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_gc(c, model, unit, fill, nullptr, what)) return rc;
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (out_pitch < c->lv[0].width) return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < width %d", what, out_pitch, c->lv[0].width);
    const uint8_t *i1, *i2;
    if (int rc = gc_source(c, which, what, &i1, &i2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    const size_t at = (size_t)pair * c->lv[0].plane_stride;
    return enqueue_gc(c, i1 + at, i2 + at, 0, 1, nullptr, model, unit, fill, nullptr, d_out, out_pitch, nullptr, nullptr, stream);
}

int bbme_get_global_compensated_host(bbme_ctx *c, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *out)
{
    const char *what = "bbme_get_global_compensated_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_gc(c, model, unit, fill, nullptr, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const uint8_t *i1, *i2;
    if (int rc = gc_source(c, which, what, &i1, &i2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const Level &L = c->lv[0];
    const size_t at = (size_t)pair * L.plane_stride;
    return download_staged(c, (size_t)L.width * L.height, "the globally compensated plane", out, [&](uint8_t *d) {
        return enqueue_gc(c, i1 + at, i2 + at, 0, 1, nullptr, model, unit, fill, nullptr, d, L.width, nullptr, nullptr, c->stream);
    });
}

int bbme_global_compensation_error(bbme_ctx *c, int which, const int32_t *models, int unit, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_global_compensation_error";
    if (int rc = check_ctx(c)) return rc;
    if (int rc = check_gc(c, models, unit, 0, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const uint8_t *i1, *i2;
    if (int rc = gc_source(c, which, what, &i1, &i2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = gc_scratch(c)) return rc;
    if (int rc = c->gm_models.ensure((size_t)6 * BBME_MAX_BATCH, "the global motion models", Fill::poison)) return rc;
    return download_stats(c, c->gc_stats, c->batch, stats, [&] {
        HIP_TRY(hipMemcpyAsync(c->gm_models, models, (size_t)6 * c->batch * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        return enqueue_gc(c, i1, i2, c->lv[0].plane_stride, c->batch, c->gm_models, nullptr, unit, 0, window, nullptr, 0,
                          c->gc_stats.partials_all(), c->gc_stats.results(), c->stream);
    });
}

// ---- the same on the B,G,R frames (the BGR GLOBAL COMPENSATION RULE of include/bbme.h; K18b k_global_compensate_bgr) ----------

static long long gcb_groups(const bbme_ctx *c) { return gather_groups(c->geom.width, c->geom.height, kGcBgrRunsPerLane); }

// result words of every pair, partials of a launch over every pair, then those of a caller's longest run: one size per context
static int gcb_scratch(bbme_ctx *c)
{
    return c->gcb_stats.ensure(BBME_MAX_BATCH, gcb_groups(c), c->batch, BBME_GC_MAX_FRAMES, "the colour global compensation statistics");
}

static int gcb_tables(bbme_ctx *c)
{
    return c->gcb_models.ensure((size_t)6 * (BBME_MAX_BATCH + BBME_GC_MAX_FRAMES), "the colour global compensation models", Fill::poison);
}
static int32_t *gcb_table_caller(const bbme_ctx *c) { return c->gcb_models + (size_t)6 * BBME_MAX_BATCH; }

// unit, fill, the padded plane's limit and a window in pixels of the FRAME.  Touches no device.
static int check_gcb(const bbme_ctx *c, const int32_t *model, int unit, int fill, const int *window, const char *what)
{
    const Level &L = c->lv[0];
    if (!model) return bbme::fail(BBME_ERR_INVALID, "%s: null model", what);
    if (unit != 1 && unit != 4) return bbme::fail(BBME_ERR_INVALID, "%s: unit %d (1 or 4)", what, unit);
    if (int rc = check_fill(fill, what)) return rc;
    if (L.width > 8188 || L.height > 8188)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: a %dx%d plane is beyond 8188", what, L.width, L.height);
    if (!window || (window[0] >= 0 && window[1] >= 0 && window[2] >= 1 && window[3] >= 1 &&
                    (long long)window[0] + window[2] <= c->geom.width && (long long)window[1] + window[3] <= c->geom.height))
        return BBME_OK;
    return bbme::fail(BBME_ERR_INVALID, "%s: window (%d, %d, %d, %d) is not inside the %dx%d frame", what, window[0], window[1],
                      window[2], window[3], c->geom.width, c->geom.height);
}

// k_global_compensate_bgr over `count` frames (frame_stride bytes apart in both inputs, out_stride in the output) under the models
// of the device table d_models (six words per frame) or, without one, under `model`: the frames into d_out and / or, with
// d_stats, the statistics of every frame over `window` in frame pixels
static int enqueue_gcb(bbme_ctx *c, const uint8_t *bgr1, const uint8_t *bgr2, int bgr_pitch, size_t frame_stride, int count,
                       const int32_t *d_models, const int32_t *model, int unit, int fill, const int *window, uint8_t *d_out,
                       int out_pitch, size_t out_stride, unsigned long long *partial, unsigned long long *d_stats, hipStream_t stream)
{
    GcBgrArgs a{};
    a.bgr1 = bgr1; a.bgr2 = bgr2; a.out = d_out;
    a.models = d_models;
    if (model) std::copy(model, model + 6, a.model);
    a.frame_stride = frame_stride; a.out_stride = out_stride;
    a.fw = c->geom.width; a.fh = c->geom.height; a.pad_x = c->geom.pad_x; a.pad_y = c->geom.pad_y;
    a.bgr_pitch = bgr_pitch; a.out_pitch = out_pitch; a.mul = 4 / unit; a.fill = fill;
    set_window(a, window, a.fw, a.fh);
    set_runs(a, a.fw, a.fh);
    return launch_gather(k_global_compensate_bgr<kGcBgrRunsPerLane>, a, gcb_groups(c), count, 1, partial, d_stats, stream);
}

int bbme_cells_global_compensate_bgr_device(bbme_ctx *c, const uint8_t *d_bgr1, const uint8_t *d_bgr2, int bgr_pitch, size_t frame_stride,
                                            int count, const int32_t *models, int unit, int fill, const int *window, uint8_t *d_out,
                                            int out_pitch, size_t out_stride, unsigned long long *d_stats4, void *hip_stream)
{
    const char *what = "bbme_cells_global_compensate_bgr_device";
    if (int rc = check_ctx(c)) return rc;
    const int fw = c->geom.width, fh = c->geom.height;
    if (!d_bgr2 || (!d_out && !d_stats4) || (d_stats4 && !d_bgr1)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (count < 1 || count > BBME_GC_MAX_FRAMES)
        return bbme::fail(BBME_ERR_INVALID, "%s: %d frames (1..%d)", what, count, (int)BBME_GC_MAX_FRAMES);
    if (int rc = check_gcb(c, models, unit, fill, window, what)) return rc;
    if (int rc = check_frames(count, bgr_pitch, frame_stride, 3 * fw, fh, what, "colour")) return rc;
    if (d_out) if (int rc = check_bgr_frames(c, count, out_pitch, out_stride, what)) return rc;
    if (d_out) {                                            // the run of output frames against each run of input frames
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out),
                        o1 = o0 + (size_t)(count - 1) * out_stride + (size_t)out_pitch * (fh - 1) + (size_t)3 * fw;
        for (const uint8_t *in : {d_bgr1, d_bgr2}) {
            const uintptr_t i0 = reinterpret_cast<uintptr_t>(in),
                            i1 = i0 + (size_t)(count - 1) * frame_stride + (size_t)bgr_pitch * (fh - 1) + (size_t)3 * fw;
            if (in && o0 < i1 && i0 < o1) return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input frame", what);
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats4) if (int rc = gcb_scratch(c)) return rc;
    if (count > 1) if (int rc = gcb_tables(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    const int32_t *table = nullptr;
    if (count > 1) {                                        // one frame: its model travels in the arguments
        HIP_TRY(hipMemcpyAsync(gcb_table_caller(c), models, (size_t)6 * count * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        table = gcb_table_caller(c);
    }
    return enqueue_gcb(c, d_bgr1, d_bgr2, bgr_pitch, frame_stride, count, table, table ? nullptr : models, unit, fill, window, d_out,
                       out_pitch, out_stride, d_stats4 ? c->gcb_stats.partials_caller() : nullptr, d_stats4, stream);
}

// The stored colour of `which`, pairs bgr_stride bytes apart, as gc_source names the planes: 0 predicts frame 1 from frame 2 of
// the context's direction, 1 frame 2 from frame 1 as they were set.  Pairs pair0 .. pair0 + pairs - 1 need their colour.
static int gcb_source(const bbme_ctx *c, int which, int pair0, int pairs, const char *what, const uint8_t **bgr1, const uint8_t **bgr2)
{
    if (int rc = check_which(which, what)) return rc;
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "%s: no frames set", what);
    const int w1 = which ? 1 : c->direction ? 1 : 0, w2 = 1 - w1;
    for (int p = pair0; p < pair0 + pairs; ++p)
        if (!c->bgr.get() || !c->bgr_set[c->slot(p, 0)] || !c->bgr_set[c->slot(p, 1)])
            return bbme::fail(BBME_ERR_STATE, "%s: pair %d has no stored colour (set both frames with a *_bgr setter)", what, p);
    *bgr1 = c->bgr + (size_t)c->slot(pair0, w1) * c->bgr_stride;
    *bgr2 = c->bgr + (size_t)c->slot(pair0, w2) * c->bgr_stride;
    return BBME_OK;
}

int bbme_global_compensate_bgr_device(bbme_ctx *c, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *d_out,
                                      int out_pitch, void *hip_stream)
{
    const char *what = "bbme_global_compensate_bgr_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_gcb(c, model, unit, fill, nullptr, what)) return rc;
    if (!d_out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_bgr_frames(c, 1, out_pitch, 0, what)) return rc;
    const uint8_t *b1, *b2;
    if (int rc = gcb_source(c, which, pair, 1, what, &b1, &b2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_gcb(c, b1, b2, 3 * c->geom.width, 0, 1, nullptr, model, unit, fill, nullptr, d_out, out_pitch, 0, nullptr, nullptr,
                       stream);
}

int bbme_get_global_compensated_bgr_host(bbme_ctx *c, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *out)
{
    const char *what = "bbme_get_global_compensated_bgr_host";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_gcb(c, model, unit, fill, nullptr, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const uint8_t *b1, *b2;
    if (int rc = gcb_source(c, which, pair, 1, what, &b1, &b2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int row = 3 * c->geom.width;
    return download_staged(c, (size_t)row * c->geom.height, "the globally compensated colour frame", out, [&](uint8_t *d) {
        return enqueue_gcb(c, b1, b2, row, 0, 1, nullptr, model, unit, fill, nullptr, d, row, 0, nullptr, nullptr, c->stream);
    });
}

int bbme_global_compensation_error_bgr(bbme_ctx *c, int which, const int32_t *models, int unit, const int *window,
                                       unsigned long long *stats)
{
    const char *what = "bbme_global_compensation_error_bgr";
    if (int rc = check_ctx(c)) return rc;
    if (int rc = check_gcb(c, models, unit, 0, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const uint8_t *b1, *b2;
    if (int rc = gcb_source(c, which, 0, c->batch, what, &b1, &b2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = gcb_scratch(c)) return rc;
    if (int rc = gcb_tables(c)) return rc;
    return download_stats(c, c->gcb_stats, c->batch, stats, [&] {
        HIP_TRY(hipMemcpyAsync(c->gcb_models, models, (size_t)6 * c->batch * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        return enqueue_gcb(c, b1, b2, 3 * c->geom.width, c->bgr_stride, c->batch, c->gcb_models, nullptr, unit, 0, window, nullptr, 0, 0,
                           c->gcb_stats.partials_all(), c->gcb_stats.results(), c->stream);
    });
}

// ---- motion compensation of the B,G,R frames along a cell grid (the BGR COMPENSATION RULE of include/bbme.h; K11b k_compensate_bgr) ----

static long long cb_groups(const bbme_ctx *c) { return cell_groups(c, kCbRunsPerLane); }

// result words of every pair, partials of a launch over every pair, then those of a caller's launch: one size per context
static int cb_scratch(bbme_ctx *c)
{
    return c->cb_stats.ensure(BBME_MAX_BATCH, cb_groups(c), c->batch, 1, "the colour compensation statistics");
}

// unit, fill and a window in pixels of the FRAME.  Touches no device.
static int check_cb(const bbme_ctx *c, int unit, int fill, const int *window, const char *what)
{
    if (unit != 1 && unit != 4) return bbme::fail(BBME_ERR_INVALID, "%s: unit %d (1 or 4)", what, unit);
    if (int rc = check_fill(fill, what)) return rc;
    if (!window || (window[0] >= 0 && window[1] >= 0 && window[2] >= 1 && window[3] >= 1 &&
                    (long long)window[0] + window[2] <= c->geom.width && (long long)window[1] + window[3] <= c->geom.height))
        return BBME_OK;
    return bbme::fail(BBME_ERR_INVALID, "%s: window (%d, %d, %d, %d) is not inside the %dx%d frame", what, window[0], window[1],
                      window[2], window[3], c->geom.width, c->geom.height);
}

// k_compensate_bgr over `pairs` pairs (colour frames frame_stride bytes, grids s_grid words apart): the frame into d_out (one pair
// only) and / or, with d_stats, the statistics over `window` in frame pixels
static int enqueue_cb(bbme_ctx *c, const uint8_t *bgr1, const uint8_t *bgr2, int bgr_pitch, size_t frame_stride, const mv_t *grid,
                      int grid_pitch, size_t s_grid, int pairs, int unit, int fill, const int *window, uint8_t *d_out, int out_pitch,
                      unsigned long long *partial, unsigned long long *d_stats, hipStream_t stream)
{
    const Level &L = c->lv[0];
    CbArgs a{};
    a.bgr1 = bgr1; a.bgr2 = bgr2; a.grid = grid; a.out = d_out;
    a.frame_stride = frame_stride; a.s_grid = s_grid;
    a.fw = c->geom.width; a.fh = c->geom.height; a.pad_x = c->geom.pad_x; a.pad_y = c->geom.pad_y;
    a.cw = L.width / 2; a.grid_pitch = grid_pitch; a.bgr_pitch = bgr_pitch; a.out_pitch = out_pitch;
    a.mul = 4 / unit; a.fill = fill;
    set_window(a, window, a.fw, a.fh);
    set_runs(a, L.width / 2, L.height / 2);
    return launch_gather(k_compensate_bgr<kCbRunsPerLane>, a, cb_groups(c), pairs, 1, partial, d_stats, stream);
}

int bbme_cells_compensate_bgr_device(bbme_ctx *c, const uint8_t *d_bgr1, const uint8_t *d_bgr2, int bgr_pitch, const int16_t *d_grid,
                                     int pitch_cells, int unit, int fill, const int *window, uint8_t *d_out, int out_pitch,
                                     unsigned long long *d_stats4, void *hip_stream)
{
    const char *what = "bbme_cells_compensate_bgr_device";
    if (int rc = check_ctx(c)) return rc;
    const int fw = c->geom.width, fh = c->geom.height;
    if (!d_bgr2 || !d_grid || (!d_out && !d_stats4) || (d_stats4 && !d_bgr1)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = check_cb(c, unit, fill, window, what)) return rc;
    if (int rc = check_frames(1, bgr_pitch, 0, 3 * fw, fh, what, "colour")) return rc;
    if (pitch_cells < c->lv[0].width / 2)
        return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, pitch_cells, c->lv[0].width / 2);
    if (d_out) if (int rc = check_bgr_frames(c, 1, out_pitch, 0, what)) return rc;
    if (d_out && (overlaps_input(d_out, out_pitch, {d_bgr1, d_bgr2}, bgr_pitch, 3 * fw, fh)))
        return bbme::fail(BBME_ERR_INVALID, "%s: the output overlaps an input frame", what);
    HIP_TRY(hipSetDevice(c->device));
    if (d_stats4) if (int rc = cb_scratch(c)) return rc;
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_cb(c, d_bgr1, d_bgr2, bgr_pitch, 0, reinterpret_cast<const mv_t *>(d_grid), pitch_cells, 0, 1, unit, fill, window,
                      d_out, out_pitch, c->cb_stats.partials_caller(), d_stats4, stream);
}

// The state the context's own calls need, before anything is enqueued: planes and cells as bbme_subpel_device's `which` names them,
// and the stored colour of pairs pair0 .. pair0 + pairs - 1.  Touches no device.
static int cb_state(const bbme_ctx *c, int which, int pair0, int pairs, const char *what)
{
    const uint8_t *p1, *p2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &p1, &p2, &grid, &s_grid)) return rc;
    return gcb_source(c, which, pair0, pairs, what, &p1, &p2);
}

// The context's own: the integer cells of `which` of `pairs` pairs from pair0 on (unit 1) or, with unit 4, those cells refined on
// the luma planes into the context's quarter-pel buffer as enqueue_own_sc refines them, then the stored colour compensated along them
static int enqueue_own_cb(bbme_ctx *c, int pair0, int pairs, int which, int unit, int fill, const int *window, uint8_t *d_out,
                          int out_pitch, unsigned long long *d_stats, hipStream_t stream, const char *what)
{
    const uint8_t *i1, *i2, *b1, *b2;
    const mv_t *grid;
    uint32_t s_grid;
    if (int rc = sp_source(c, which, what, &i1, &i2, &grid, &s_grid)) return rc;
    if (int rc = gcb_source(c, which, pair0, pairs, what, &b1, &b2)) return rc;
    const Level &L = c->lv[0];
    const int cw = L.width / 2;
    const size_t cells = (size_t)cw * (L.height / 2), s_plane = L.plane_stride;
    grid += (size_t)pair0 * s_grid;
    size_t s_cells = s_grid;
    if (unit == 4) {
        if (int rc = c->sc_q4.ensure(cells * c->batch, "the quarter-pel cells of the compensation", Fill::poison)) return rc;
        mv_t *q4 = c->sc_q4 + pair0 * cells;
        if (int rc = enqueue_sp(c, i1 + pair0 * s_plane, i2 + pair0 * s_plane, s_plane, grid, s_grid, pairs, nullptr, q4, cw, cells, nullptr,
                                nullptr, stream))
            return rc;
        grid = q4; s_cells = cells;
    }
    return enqueue_cb(c, b1, b2, 3 * c->geom.width, c->bgr_stride, grid, cw, s_cells, pairs, unit, fill, window, d_out, out_pitch,
                      c->cb_stats.partials_all(), d_stats, stream);
}

// what bbme_compensate_bgr_device and bbme_get_compensated_bgr_host check alike.  Touches no device.
static int check_cb_own(const bbme_ctx *c, int pair, int which, int unit, int fill, const void *out, const char *what)
{
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (int rc = check_cb(c, unit, fill, nullptr, what)) return rc;
    if (!out) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_sp(c, nullptr, what)) return rc;
    return cb_state(c, which, pair, 1, what);
}

int bbme_compensate_bgr_device(bbme_ctx *c, int pair, int which, int unit, int fill, uint8_t *d_out, int out_pitch, void *hip_stream)
{
    const char *what = "bbme_compensate_bgr_device";
    if (int rc = check_cb_own(c, pair, which, unit, fill, d_out, what)) return rc;
    if (int rc = check_bgr_frames(c, 1, out_pitch, 0, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream;
    if (int rc = stream_behind_ctx(c, hip_stream, &stream)) return rc;
    return enqueue_own_cb(c, pair, 1, which, unit, fill, nullptr, d_out, out_pitch, nullptr, stream, what);
}

int bbme_get_compensated_bgr_host(bbme_ctx *c, int pair, int which, int unit, int fill, uint8_t *out)
{
    const char *what = "bbme_get_compensated_bgr_host";
    if (int rc = check_cb_own(c, pair, which, unit, fill, out, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int row = 3 * c->geom.width;
    return download_staged(c, (size_t)row * c->geom.height, "the compensated colour frame", out, [&](uint8_t *d) {
        return enqueue_own_cb(c, pair, 1, which, unit, fill, nullptr, d, row, nullptr, c->stream, what);
    });
}

int bbme_compensation_error_bgr(bbme_ctx *c, int which, int unit, const int *window, unsigned long long *stats)
{
    const char *what = "bbme_compensation_error_bgr";
    if (int rc = check_ctx(c)) return rc;
    if (int rc = check_which(which, what)) return rc;
    if (int rc = check_cb(c, unit, 0, window, what)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    if (int rc = check_sp(c, nullptr, what)) return rc;
    if (int rc = cb_state(c, which, 0, c->batch, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = cb_scratch(c)) return rc;
    return download_stats(c, c->cb_stats, c->batch, stats, [&] {
        return enqueue_own_cb(c, 0, c->batch, which, unit, 0, window, nullptr, 0, c->cb_stats.results(), c->stream, what);
    });
}

extern "C" {

int bbme_frame_plane_device(bbme_ctx *c, int pair, int which, int level, const uint8_t **d_plane)
{
    const char *what = "bbme_frame_plane_device";
    if (int rc = check_pair(c, pair)) return rc;
    if (int rc = check_level(c, level)) return rc;
    if (which != 0 && which != 1) return bbme::fail(BBME_ERR_INVALID, "%s: which = %d (0 or 1)", what, which);
    if (!d_plane) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    const Level &L = c->lv[level];
    *d_plane = L.img1 + (size_t)pair * L.plane_stride + (size_t)which * L.frame_step;
    return BBME_OK;
}

int bbme_stage_search(bbme_ctx *c, int level)
{
    if (int rc = single_pair_only(c, "bbme_stage_search")) return rc;
    if (int rc = check_level(c, level)) return rc;
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "no frames set");
    HIP_TRY(hipSetDevice(c->device));
    c->memo_block = 0;             // a stage sequence at a level starts here: the planes may have been refilled in place since
    c->fields_valid = false;
    return launch_search(c, plan_search_launch(plan_inputs(c), level, kPredictPlain));
}

int bbme_stage_regularize(bbme_ctx *c, int level, int block, int mult)
{
    if (int rc = single_pair_only(c, "bbme_stage_regularize")) return rc;
    if (int rc = check_level(c, level)) return rc;
    if (!c->frames_set()) return bbme::fail(BBME_ERR_STATE, "no frames set");
    HIP_TRY(hipSetDevice(c->device));
    c->fields_valid = false;
    Level &L = c->lv[level];
    if (mult < 1) return bbme::fail(BBME_ERR_INVALID, "lambda multiplier %d", mult);
    if (block < 2 || block > L.block || (block & (block - 1)))
        return bbme::fail(BBME_ERR_INVALID, "block %d is not a power of two in 2..%d", block, L.block);
    // on the grid the level holds, with the solver's counters (bbme_sweep_stats)
    return launch_sweep(c, plan_sweep(plan_inputs(c), level, block, mult, L.grid_id(L.cur_grid), L.cur_block), true);
}

int bbme_stage_get_mvs(bbme_ctx *c, int level, int block, int16_t *mvs)
{
    if (int rc = single_pair_only(c, "bbme_stage_get_mvs")) return rc;
    if (int rc = check_level(c, level)) return rc;
    Level &L = c->lv[level];
    if (!mvs) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (L.cur_block == 0) return bbme::fail(BBME_ERR_STATE, "level %d has no MV grid yet", level);
    if (block < 1 || block > L.cur_block || (L.cur_block % block))
        return bbme::fail(BBME_ERR_INVALID, "block %d does not divide the grid's block size %d", block, L.cur_block);
    HIP_TRY(hipSetDevice(c->device));
    const int rows = L.height / L.cur_block, cols = L.width / L.cur_block;
    std::vector<mv_t> host((size_t)rows * cols);
    HIP_TRY(hipMemcpyAsync(host.data(), L.cur_grid, host.size() * sizeof(mv_t), hipMemcpyDeviceToHost, c->stream));
    if (int rc = check_converged(c)) return rc;
    // divide_blocks (:845-862) repeated: every finer block inherits its parent's MV
    const int f = L.cur_block / block, orows = rows * f, ocols = cols * f;
    for (int r = 0; r < orows; ++r)
        for (int q = 0; q < ocols; ++q) {
            const mv_t m = host[(size_t)(r / f) * cols + q / f];
            mvs[2 * ((size_t)r * ocols + q)] = (int16_t)(m & 0xffffu);
            mvs[2 * ((size_t)r * ocols + q) + 1] = (int16_t)(m >> 16);
        }
    return BBME_OK;
}

int bbme_stage_set_mvs(bbme_ctx *c, int level, int block, const int16_t *mvs)
{
    if (int rc = single_pair_only(c, "bbme_stage_set_mvs")) return rc;
    if (int rc = check_level(c, level)) return rc;
    Level &L = c->lv[level];
    if (!mvs) return bbme::fail(BBME_ERR_INVALID, "null input");
    if (block < 2 || block > L.block || (block & (block - 1)))
        return bbme::fail(BBME_ERR_INVALID, "block %d is not a power of two in 2..%d", block, L.block);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)(L.height / block) * (L.width / block);
    std::vector<mv_t> host(n);
    for (size_t i = 0; i < n; ++i) host[i] = ((uint32_t)(uint16_t)mvs[2 * i]) | ((uint32_t)(uint16_t)mvs[2 * i + 1] << 16);
    L.cur_grid = block == L.block ? L.small[0] : L.big[0];
    L.cur_block = block;
    c->memo_block = 0;             // as bbme_stage_search: the planes may have been refilled in place since
    c->fields_valid = false;
    HIP_TRY(hipMemcpyAsync(L.cur_grid, host.data(), n * sizeof(mv_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BBME_OK;
}

int bbme_stage_expand(bbme_ctx *c)
{
    if (int rc = single_pair_only(c, "bbme_stage_expand")) return rc;
    if (int rc = check_ctx(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launch_expand(c);
}

int bbme_last_sweep_passes(bbme_ctx *c, int *passes)
{
    if (int rc = single_pair_only(c, "bbme_last_sweep_passes")) return rc;
    if (int rc = check_ctx(c)) return rc;
    if (!passes) return bbme::fail(BBME_ERR_INVALID, "null output");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t host[8];
    HIP_TRY(hipMemcpyAsync(host, c->counters, sizeof host, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    passes[0] = (int)host[3];
    passes[1] = (int)host[4];
    if (host[5]) return bbme::fail(BBME_ERR_STATE, "a regulariser sweep hit its pass cap without converging");
    return BBME_OK;
}

int bbme_fixup_counts(bbme_ctx *c, int pair, unsigned *counts, int n)
{
    if (int rc = check_ctx(c)) return rc;
    if (!counts || n < 0) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (pair < 0 || pair >= c->batch) return bbme::fail(BBME_ERR_INVALID, "pair %d of %d", pair, c->batch);
    HIP_TRY(hipSetDevice(c->device));
    for (int l = 0; l < n; ++l) counts[l] = 0;
    for (int l = 0; l < n && l < (int)c->lv.size(); ++l)
        if (c->last_spec_levels >> l & 1u)
            HIP_TRY(hipMemcpyAsync(&counts[l], c->lv[l].fix_count.get() + (size_t)pair * 16, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BBME_OK;
}

int bbme_sweep_stats(bbme_ctx *c, unsigned *stats)
{
    if (int rc = single_pair_only(c, "bbme_sweep_stats")) return rc;
    if (int rc = check_ctx(c)) return rc;
    if (!stats) return bbme::fail(BBME_ERR_INVALID, "null output");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(stats, c->counters, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BBME_OK;
}

int bbme_set_profiling(bbme_ctx *c, int enabled)
{
    if (int rc = check_ctx(c)) return rc;
    c->profiling = enabled != 0;
    return BBME_OK;
}

int bbme_get_timings(bbme_ctx *c, float *total, float *search, float *reg, float *expand, float *search0)
{
    if (int rc = check_ctx(c)) return rc;
    if (total) *total = c->t_total;
    if (search) *search = c->t_search;
    if (reg) *reg = c->t_reg;
    if (expand) *expand = c->t_expand;
    if (search0) *search0 = c->t_search0;
    return BBME_OK;
}

int bbme_probe_rates(int device, double *gops)
{
    if (!gops) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (int rc = probe_device(device)) return rc;
    DevBuf<uint32_t> out;
    if (int rc = out.alloc(16, kProbe, Fill::none)) return rc;
    const int iters = 4096, grid = 256 * 8;          // 8 workgroups of 4 waves per CU: 8 waves per SIMD
    void (*const kernels[4])(uint32_t *, int, uint32_t) = {k_probe_rate<0>, k_probe_rate<1>, k_probe_rate<2>, k_probe_rate<5>};
    for (int which = 0; which < 4; ++which) {
        float ms = 0;
        if (int rc = time_second_launch([&](int rep) { kernels[which]<<<dim3(grid), dim3(256), 0, 0>>>(out, iters, 7u + rep); }, &ms)) return rc;
        // wave-instructions per second over the whole chip, in units of 1e9 (mixed runs: QSADs only)
        gops[which] = (double)grid * 4 * iters * 8 / (ms * 1e-3) / 1e9;
    }
    return BBME_OK;
}

int bbme_probe_search_loops(int device, double *tabs2)
{
    if (!tabs2) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (int rc = probe_device(device)) return rc;
    DevBuf<uint32_t> out;
    if (int rc = out.alloc(16, kProbe, Fill::none)) return rc;
    const int passes = 128, grid = 32768;
    for (int which = 0; which < 2; ++which) {
        float ms = 0;
        if (int rc = time_second_launch([&](int rep) {
                if (which == 0) hipLaunchKernelGGL(k_probe_search_loop<false>, dim3(grid), dim3(64), 6912 + 21 * 32 * 4, 0, out.get(), passes, 3u + rep);
                else hipLaunchKernelGGL(k_probe_search_loop<true>, dim3(grid), dim3(64), 27648 + 16 * 5 * 32 + 16 * 5 * 31, 0, out.get(), passes, 3u + rep);
            }, &ms)) return rc;
        // abs-diffs: per lane and pass 16 x 16 x 4 instructions of 16 (QSAD: four dx at once) or 4 (v_sad_u8) abs-diffs
        const double absdiff = (double)grid * 64 * passes * 1024 * (which == 0 ? 16 : 4);
        tabs2[which] = absdiff / (ms * 1e-3) / 1e12;
    }
    return BBME_OK;
}

int bbme_probe_latency(int device, unsigned long long *out9)
{
    if (!out9) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (int rc = probe_device(device)) return rc;
    const uint32_t nwords = 1u << 18;                       // 1 MiB: beyond L1, inside an L2
    std::vector<uint32_t> host(nwords);
    uint32_t x = 12345;
    for (uint32_t i = 0; i < nwords; ++i) { x = x * 1664525u + 1013904223u; host[i] = x; }
    DevBuf<uint32_t> buf;
    DevBuf<unsigned long long> out;
    if (int rc = buf.upload(host, kProbe)) return rc;
    if (int rc = out.alloc(9, kProbe, Fill::none)) return rc;
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k_probe_latency, dim3(1), dim3(64), 0, 0, buf.get(), nwords, out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out9, out, 9 * 8, hipMemcpyDeviceToHost));
    return BBME_OK;
}

int bbme_probe_xcd(int device, int *xcds_seen, int *violations)
{
    if (!xcds_seen || !violations) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (int rc = probe_device(device)) return rc;
    const int n = 4096;
    std::vector<uint32_t> host(n);
    DevBuf<uint32_t> d;
    if (int rc = d.alloc(n, kProbe, Fill::none)) return rc;
    hipLaunchKernelGGL(k_probe_xcc, dim3(n), dim3(64), 0, 0, d.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(host.data(), d, n * 4, hipMemcpyDeviceToHost));
    uint32_t seen = 0;
    *violations = 0;
    for (int b = 0; b < n; ++b) {
        seen |= 1u << host[b];
        if (host[b] != host[b & 7]) ++*violations;
    }
    *xcds_seen = __builtin_popcount(seen);
    return BBME_OK;
}

int bbme_calibrate_read(int device, unsigned mbytes, int repeats)
{
    if (int rc = probe_device(device)) return rc;
    if (mbytes == 0 || mbytes > 16384 || repeats < 1) return bbme::fail(BBME_ERR_INVALID, "bbme_calibrate_read: bad size");
    const size_t bytes = (size_t)mbytes << 20, n = bytes / 4;
    DevBuf<uint32_t> buf, out;
    if (int rc = buf.alloc(n, kProbe, Fill::none)) return rc;
    if (int rc = out.alloc(16, kProbe, Fill::none)) return rc;
    HIP_TRY(hipMemset(buf, 1, bytes));
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < repeats; ++i)
        hipLaunchKernelGGL(k_calib_read_dword, dim3(256 * 8), dim3(256), 0, 0, buf.get(), n, out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return BBME_OK;
}

int bbme_selftest_isa(int device, int *mismatches)
{
    if (!mismatches) return bbme::fail(BBME_ERR_INVALID, "null output");
    if (int rc = probe_device(device)) return rc;
    const int n = 1 << 16;
    std::vector<uint32_t> a(n), b(n), cc(n), sad(n), al(n), s16(n);
    std::vector<unsigned long long> qs(n);
    uint32_t x = 0x12345678u;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (int i = 0; i < n; ++i) { a[i] = rnd(); b[i] = rnd(); cc[i] = rnd(); }
    DevBuf<uint32_t> da, db, dc, dsad, dal, ds16;
    DevBuf<unsigned long long> dqs;
    if (int rc = da.upload(a, kProbe)) return rc;
    if (int rc = db.upload(b, kProbe)) return rc;
    if (int rc = dc.upload(cc, kProbe)) return rc;
    for (DevBuf<uint32_t> *d : {&dsad, &dal, &ds16})
        if (int rc = d->alloc(n, kProbe, Fill::none)) return rc;
    if (int rc = dqs.alloc(n, kProbe, Fill::none)) return rc;
    hipLaunchKernelGGL(k_probe_sad, dim3(n / 256), dim3(256), 0, 0, da.get(), db.get(), dc.get(), dsad.get(), dqs.get(), dal.get(), ds16.get(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(sad.data(), dsad, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(al.data(), dal, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s16.data(), ds16, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(qs.data(), dqs, n * 8, hipMemcpyDeviceToHost));
    auto absd = [](int p, int q) { return p > q ? p - q : q - p; };
    mismatches[0] = mismatches[1] = mismatches[2] = mismatches[3] = mismatches[4] = 0;
    {   // unaligned dword / x2 / x4 global loads (score_block relies on them)
        const int m = 4096;
        std::vector<uint8_t> bytes(5 * m + 64);
        for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = (uint8_t)rnd();
        std::vector<uint32_t> got(7 * m);
        DevBuf<uint8_t> dp;
        DevBuf<uint32_t> dout;
        if (int rc = dp.upload(bytes, kProbe)) return rc;
        if (int rc = dout.alloc(got.size(), kProbe, Fill::none)) return rc;
        hipLaunchKernelGGL(k_probe_unaligned, dim3(m / 256), dim3(256), 0, 0, dp.get(), dout.get(), m);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(got.data(), dout, got.size() * 4, hipMemcpyDeviceToHost));
        auto rd = [&](size_t o) { return (uint32_t)bytes[o] | ((uint32_t)bytes[o + 1] << 8) | ((uint32_t)bytes[o + 2] << 16) | ((uint32_t)bytes[o + 3] << 24); };
        for (int i = 0; i < m; ++i) {
            const size_t o = 5 * (size_t)i + (i & 3);
            bool ok = got[7 * i] == rd(o) && got[7 * i + 1] == rd(o + 1) && got[7 * i + 2] == rd(o + 5);
            for (int k = 0; k < 4; ++k) ok = ok && got[7 * i + 3 + k] == rd(o + 2 + 4 * k);
            if (!ok) ++mismatches[4];
        }
    }
    for (int i = 0; i < n; ++i) {
        uint32_t e = cc[i];
        for (int k = 0; k < 4; ++k) e += absd((a[i] >> (8 * k)) & 255, (b[i] >> (8 * k)) & 255);
        if (e != sad[i]) ++mismatches[0];
        const unsigned long long w = ((unsigned long long)b[i] << 32) | a[i];
        if ((uint32_t)(w >> (8 * (cc[i] & 3))) != al[i]) ++mismatches[1];
        // v_qsad_pk_u16_u8: four SADs of src1's 4 bytes against src0 shifted by 0..3 bytes,
        // each added to the matching 16-bit lane of the accumulator
        const uint32_t ref = cc[i] ^ a[i];
        const unsigned long long acc = ((unsigned long long)(cc[i] & 0x00ff00ffu) << 32) | (cc[i] & 0x0f0f0f0fu);
        unsigned long long eq = 0;
        for (int k = 0; k < 4; ++k) {
            const uint32_t win = (uint32_t)(w >> (8 * k));
            uint32_t s = (uint32_t)((acc >> (16 * k)) & 0xffff);
            for (int q = 0; q < 4; ++q) s += absd((win >> (8 * q)) & 255, (ref >> (8 * q)) & 255);
            eq |= (unsigned long long)(s & 0xffff) << (16 * k);
        }
        if (eq != qs[i]) ++mismatches[2];
        const uint32_t e16 = (cc[i] & 0xffffu) + absd(a[i] & 0xffff, b[i] & 0xffff) + absd(a[i] >> 16, b[i] >> 16);
        if (e16 != s16[i]) ++mismatches[3];
    }
    return BBME_OK;
}

// ---- test hooks: the guard bands of BBME_TEST_GUARD (DevBuf, guard_layout.hpp) ---------------------------------------------
int bbme_test_guard_check(unsigned long long *live, unsigned long long *violations, char *first, int first_len)
{
    if (!live || !violations || first_len < 0 || (first_len > 0 && !first))
        return bbme::fail(BBME_ERR_INVALID, "bbme_test_guard_check: bad arguments");
    GuardRegistry &r = guard_registry();
    std::lock_guard<std::mutex> lock(r.mu);
    int before = 0;
    const bool have_device = hipGetDevice(&before) == hipSuccess;
    unsigned long long found = r.sticky;
    std::string text = r.sticky_first;
    int synced = -1;
    for (const GuardRegistry::Entry &e : r.live) {
        if (e.device != synced) {                            // whatever any stream of that device still runs has finished
            HIP_TRY(hipSetDevice(e.device));
            HIP_TRY(hipDeviceSynchronize());
            synced = e.device;
        }
        guard_scan(e, &found, &text);
    }
    if (have_device && synced >= 0) (void)hipSetDevice(before);
    *live = r.live.size();
    *violations = found;
    if (first_len > 0) snprintf(first, (size_t)first_len, "%s", text.c_str());
    return BBME_OK;
}

int bbme_test_guard_reset(void)
{
    GuardRegistry &r = guard_registry();
    std::lock_guard<std::mutex> lock(r.mu);
    r.sticky = 0;
    r.sticky_first.clear();
    return BBME_OK;
}

int bbme_test_guard_find(const char *what, int back, void **guard_address)
{
    if (!what || !guard_address) return bbme::fail(BBME_ERR_INVALID, "bbme_test_guard_find: null argument");
    *guard_address = nullptr;
    if (!test_knob_on(getenv("BBME_TEST_GUARD")))
        return bbme::fail(BBME_ERR_UNSUPPORTED, "bbme_test_guard_find: BBME_TEST_GUARD is not set");
    GuardRegistry &r = guard_registry();
    std::lock_guard<std::mutex> lock(r.mu);
    for (const GuardRegistry::Entry &e : r.live)
        if (e.what == what) {
            *guard_address = e.base + (back ? kGuardBytes + e.payload : 0);
            return BBME_OK;
        }
    return bbme::fail(BBME_ERR_INVALID, "bbme_test_guard_find: no live guarded buffer \"%s\"", what);
}

}  // extern "C"
