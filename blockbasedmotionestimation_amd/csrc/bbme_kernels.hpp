// bbme_kernels.hpp -- HIP kernels for gfx950 (CDNA4, wave64).  Included by bbme_device.hip only.
//
// Data layout in HBM (per pyramid level l, all owned by the context):
//   image1/image2 : uint8 planes, pitch == level width W_l (a multiple of 4).
//   MV grids      : one uint32 per block, (dx & 0xffff) | (dy << 16), int16 halves, row-major
//                   (H_l/b) x (W_l/b) for the block size b currently being regularised.  Two
//                   buffers per level, ping-ponged between "old" (read-only in a sweep) and
//                   "est" (being solved).  The reference instead keeps a dense CV_32FC2 field
//                   and a CV_32SC4 SAD cache per pixel (pyramid_level.h:10, motion_framework.h:46).
//   dense flow    : float2 per pixel of level 0 (the cv::Mat calcMotionBlockMatching returns).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "spec_grids.hpp"

namespace bbme {

typedef uint32_t mv_t;   // packed int16 (dx, dy)

__device__ __forceinline__ int mv_x(mv_t m) { return (int)(int16_t)(m & 0xffffu); }
__device__ __forceinline__ int mv_y(mv_t m) { return (int)(int16_t)(m >> 16); }
__device__ __forceinline__ mv_t mv_pack(int x, int y) { return ((uint32_t)x & 0xffffu) | ((uint32_t)y << 16); }

// 2 .. 16 bytes at any byte address (gfx950 global loads need no alignment; bbme_selftest_isa checks it)
struct __attribute__((packed, aligned(1))) ua_u16 { uint16_t v; };
struct __attribute__((packed, aligned(1))) ua_u32 { uint32_t v; };
struct __attribute__((packed, aligned(1))) ua_u32x2 { uint32_t v[2]; };
struct __attribute__((packed, aligned(1))) ua_u32x4 { uint32_t v[4]; };
struct __attribute__((packed, aligned(1))) ua_u64 { uint64_t v; };
struct __attribute__((packed, aligned(1))) ua_u128 { uint32_t v[4]; };

// DPP move within a row of 16 lanes (CTRL: quad_perm 0x00-0xff, row_mirror 0x140, row_half_mirror 0x141,
// row_newbcast:n 0x150+n).  All 16 lanes of a row must be active.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_row(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}


// =======================================================================================
// K1 (generic form): MF::copyMVs + MF::calcLevelBM + MF::find_min_block_spiral
// (motion_framework.cpp:828-843, 226-244, 296-422).  One wavefront per macroblock.
// The (B+2R)^2 search window of image2 and the BxB block of image1 are staged in LDS; each
// lane walks the spiral ranks lane, lane+64, ... (so inside a lane the first strict minimum
// is the lowest rank), then the wave reduces (SAD, rank) lexicographically.
// =======================================================================================
struct SearchArgs {
    const uint8_t *image1, *image2;
    int width, height;          // level size
    int range;                  // R
    int ncand;                  // (2R+1)^2
    const uint32_t *spiral;     // rank -> (dx & 0xffff) | (dy << 16)
    const mv_t *coarse;         // MV grid of level l+1 at cells of 1 << coarse_cell_shift pixels, or nullptr (coarsest level)
    int coarse_cols;            // its row length = W_{l+1} >> coarse_cell_shift
    int coarse_block;           // B_{l+1}
    int coarse_cell_shift;      // 1: the final 2x2-cell grid; log2(B_{l+1}): the grid after the sweeps at B_{l+1} (speculation)
    int mode;                   // kSearchPlain / kSearchSpeculative / kSearchFixup (see search_prediction)
    int raster;                 // 1: MF::find_min_block (:246-294) instead of find_min_block_spiral
    mv_t *pred;                 // per block of this level: the coarse MV a speculative search started from
    mv_t *out;                  // (H/B) x (W/B)
    int cols;                   // W / B
    int pitch_dw;               // LDS window pitch in dwords
    // batch: a context may hold several independent frame pairs (blockIdx.y = pair); every per-pair buffer of pair p starts
    // p * stride elements after pair 0's (shift_pair, first statement of every kernel)
    uint32_t s_plane, s_coarse, s_pred, s_out;
};
__device__ __forceinline__ void shift_pair(SearchArgs &a, uint32_t p)
{
    a.image1 += (size_t)p * a.s_plane; a.image2 += (size_t)p * a.s_plane;
    if (a.coarse) a.coarse += (size_t)p * a.s_coarse;
    a.pred += (size_t)p * a.s_pred; a.out += (size_t)p * a.s_out;
}

// copyMVs (:828-843) as the search kernels see it: the MV of the coarse block covering pixel (i, j) of this level.
// A block's search result depends on its prediction alone, which is what makes the search of level l speculable:
//   kSearchSpeculative  runs beside the late sweeps of level l+1 (second stream), predicting from the grid as the two
//                       sweeps at B_{l+1} left it -- or from a newer one (newest_coarse_grid) -- and records the coarse MV it used;
//   kSearchFixup        after level l+1 is final: a block whose recorded MV equals the final one (the top-left 2x2 cell
//                       of the coarse block, which is all copyMVs reads) keeps its result, the others are searched again.
// Either way every block ends with the result of a search from the final prediction: bit-exact by construction.
enum { kSearchPlain = 0, kSearchSpeculative = 1, kSearchFixup = 2 };
// LIVE: the grid may be written while this launch runs (newest_coarse_grid): one lane of the (one-wave) workgroup reads the cell
// once, past the caches another XCD's sweep does not reach, and the wave goes on with that value.
template <bool LIVE = false, class Args>
__device__ __forceinline__ bool search_prediction(const Args &a, int i, int j, uint32_t bid, mv_t &m)
{
    m = 0;
    if (a.coarse) {
        const int lg = 31 - __builtin_clz((unsigned)a.coarse_block);      // block sizes are powers of two (validate_params): no division
        const int ci = (i >> (lg + 1)) << lg;                              // (i / (2 B_{l+1})) * B_{l+1}, i >= 0
        const int cj = (j >> (lg + 1)) << lg;
        const mv_t *cell = a.coarse + (size_t)(ci >> a.coarse_cell_shift) * a.coarse_cols + (cj >> a.coarse_cell_shift);
        if constexpr (LIVE) {
            if (threadIdx.x == 0) m = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            m = (mv_t)__builtin_amdgcn_readfirstlane((int)m);
        } else
            m = *cell;
    }
    if (a.mode == kSearchFixup && a.pred[bid] == m) return false;       // searched from this prediction already
    if (a.mode == kSearchSpeculative && threadIdx.x == 0) a.pred[bid] = m;
    return true;
}

template <int B>
__global__ __launch_bounds__(64) void k_search_generic(SearchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    shift_pair(a, blockIdx.y);
    constexpr int BW = B / 4;
    const int lane = threadIdx.x;
    const int bc = blockIdx.x % a.cols, br = blockIdx.x / a.cols;
    const int i = br * B, j = bc * B;                     // block origin (row, col)

    // copyMVs: the coarse block covering pixel (i, j) of this level, MV doubled (:836-840)
    mv_t m;
    if (!search_prediction(a, i, j, blockIdx.x, m)) return;
    const int u = 2 * mv_x(m), v = 2 * mv_y(m);
    const int px = j + u, py = i + v;                      // :233-234
    mv_t *dst = a.out + (size_t)br * a.cols + bc;
    if (!a.raster && (px < 0 || py < 0 || px + B > a.width || py + B > a.height)) {   // :304-310 -> zero MV
        if (lane == 0) *dst = 0;
        return;
    }
    const int R = a.range;
    const int wrows = B + 2 * R;
    const int wx0 = px - R, wy0 = py - R;
    const int ax0 = wx0 & ~3;                              // dword-aligned left edge
    const int sh0 = wx0 - ax0;
    uint32_t *win = smem;
    uint32_t *cur = smem + wrows * a.pitch_dw;

    for (int idx = lane; idx < wrows * a.pitch_dw; idx += 64) {
        const int row = idx / a.pitch_dw, k = idx - row * a.pitch_dw;
        const int y = wy0 + row, x = ax0 + 4 * k;
        uint32_t w = 0;
        if (y >= 0 && y < a.height && x >= 0 && x + 4 <= a.width)
            w = *reinterpret_cast<const uint32_t *>(a.image2 + (size_t)y * a.width + x);
        win[idx] = w;
    }
    if constexpr (B >= 4) {
        for (int idx = lane; idx < B * BW; idx += 64) {
            const int row = idx / BW, k = idx - row * BW;
            cur[idx] = *reinterpret_cast<const uint32_t *>(a.image1 + (size_t)(i + row) * a.width + j + 4 * k);
        }
    } else {
        // 2 x 2 blocks (r04): the block is one dword, row 0 in the low half and row 1 in the high half
        if (lane == 0)
            cur[0] = (uint32_t)*reinterpret_cast<const uint16_t *>(a.image1 + (size_t)i * a.width + j) |
                     (uint32_t)*reinterpret_cast<const uint16_t *>(a.image1 + (size_t)(i + 1) * a.width + j) << 16;
    }
    __syncthreads();

    // SAD of the candidate at offset (dx, dy) from the prediction (its block lies inside the image)
    auto candidate_sad = [&](int dx, int dy) {
        const int ox = dx + R + sh0;                       // byte offset inside an LDS row
        const int k0 = ox >> 2, sh = ox & 3;
        const uint32_t *wrow = win + (dy + R) * a.pitch_dw + k0;
        uint32_t sad = 0;
        if constexpr (B == 2) {
            const uint32_t r0 = __builtin_amdgcn_alignbyte(wrow[1], wrow[0], sh) & 0xffffu;
            const uint32_t r1 = __builtin_amdgcn_alignbyte(wrow[a.pitch_dw + 1], wrow[a.pitch_dw], sh) << 16;
            return __builtin_amdgcn_sad_u8(cur[0], r0 | r1, 0u);
        }
#pragma unroll 2
        for (int r = 0; r < B; ++r) {
            uint32_t lo = wrow[0];
#pragma unroll
            for (int q = 0; q < BW; ++q) {
                const uint32_t hi = wrow[q + 1];
                const uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, sh);
                sad = __builtin_amdgcn_sad_u8(cur[r * BW + q], w, sad);
                lo = hi;
            }
            wrow += a.pitch_dw;
        }
        return sad;
    };
    if (a.raster) {
        // MF::find_min_block (:246-294): every candidate of [-R, R]^2 whose block lies inside the image (the clamped loops
        // of :260,262), no special case for a prediction outside it; winner = lowest SAD, then the smaller L1 distance
        // to the block's own position (:276-281), then raster order (strict comparisons): one 64-bit key
        const int side = 2 * R + 1;
        unsigned long long best = ~0ull;
        for (int idx = lane; idx < side * side; idx += 64) {
            const int dy = idx / side - R, dx = idx % side - R;
            const int cx = px + dx, cy = py + dy;
            if (cx < 0 || cy < 0 || cx + B > a.width || cy + B > a.height) continue;
            const uint32_t l1 = (uint32_t)(abs(cx - j) + abs(cy - i));
            const unsigned long long key = ((unsigned long long)candidate_sad(dx, dy) << 32) | (l1 << 16) | (uint32_t)idx;
            best = key < best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        if (lane == 0) {
            // no candidate inside the image: min_x, min_y keep the prediction (:251-252)
            int dx = 0, dy = 0;
            if (best != ~0ull) { const int idx = (int)(best & 0xffffu); dy = idx / side - R; dx = idx % side - R; }
            *dst = mv_pack(u + dx, v + dy);
        }
        return;
    }

    uint32_t best_sad = 0xffffffffu, best_rank = 0xffffffffu;
    for (int rank = lane; rank < a.ncand; rank += 64) {
        const uint32_t s = a.spiral[rank];
        const int dx = (int)(int16_t)(s & 0xffffu), dy = (int)(int16_t)(s >> 16);
        const int cx = px + dx, cy = py + dy;
        if (cx < 0 || cy < 0 || cx + B > a.width || cy + B > a.height) continue;   // :335 skipped
        const uint32_t sad = candidate_sad(dx, dy);
        if (sad < best_sad) { best_sad = sad; best_rank = (uint32_t)rank; }         // strict :339
    }
    // wave reduction of (sad, rank), lexicographic
    unsigned long long key = ((unsigned long long)best_sad << 32) | best_rank;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    if (lane == 0) {
        const uint32_t s = a.spiral[(uint32_t)key];
        *dst = mv_pack(u + (int)(int16_t)(s & 0xffffu), v + (int)(int16_t)(s >> 16));   // :238-239
    }
}

// =======================================================================================
// K1 (fast form, B = 8, 16 or 32): same function, same results, built around v_qsad_pk_u16_u8.
//
// One wavefront per macroblock.  The (B+2R)^2 window of image2 is staged in LDS re-aligned so
// that candidate column dx = -R starts on a dword; the BxB block of image1 sits in SGPRs (its
// address is wave-uniform).  Candidates are handled four at a time: a "column group" g covers
// dx indices 4g..4g+3, and one v_qsad_pk_u16_u8 adds |cur dword - window bytes| for all four
// byte shifts to four packed u16 sums (255 * 16 * 16 < 2^16, so the sums never carry).  A lane
// owns one column group and a vertical STRIP of S consecutive candidate rows, so each window
// row it reads from LDS (B/4 + 1 dwords) feeds up to S * B/4 QSADs.  The odd (2R+1)^2 candidate
// square is cut by the host into "rounds" of up to 64 equal-height strips (S in 16,8,4,2,1) so
// that lanes stay busy; `tasks` holds one word per lane and round: strip rounds g | dy0 << 8, and for the rim rounds of
// the tight plan (even ranges; plan_search in bbme_host.cpp) g | dy << 8 | part << 16 (the last candidate row, four lanes
// of a quad per (group, row), a quarter of the block's rows each) or a bare dy (the last candidate column, dx = +R).
// Winner = min over (SAD << 16) | spiral_rank, i.e. lowest SAD, ties by the reference's visiting
// order (motion_framework.cpp:326-411, strict < at :339); the rank of every (dx, dy) comes from a
// table the host builds by walking that loop.  Candidates whose block leaves the image (:335) and
// the padding columns of the last group get SAD 0xffff and can never win (the centre is valid).
// LDS pitch is an odd number of dwords: the four strips of a full round then hit disjoint banks.
// =======================================================================================
struct FastSearchArgs {
    const uint8_t *image1, *image2;
    int width, height;
    int range;                  // R
    const uint32_t *spiral;     // rank -> (dx & 0xffff) | (dy << 16)
    const uint16_t *rank_of;    // [(dy+R) * rank_pitch + (dx+R)] -> rank, 0xffff where dx > R
    int rank_pitch;             // multiple of 4
    const uint32_t *tasks;      // nrounds * 64 entries by round kind (rounds[] >> 8 & 0xff): 0 strips g | dy0 << 8; 1 last row
                                // g | dy << 8 | part << 16; 2 last column dy; 0xffffffff = idle lane
    const uint32_t *rounds;     // nrounds entries: strip height S | kind << 8 | (strip rounds) first row of the round in lane_ranks << 16
    int nrounds;
    const uint2 *lane_ranks;    // strip rounds: the ranks of a lane's candidates, S entries of 4 x u16 (columns 4g..4g+3 of row dy0 + d),
                                // contiguous per lane: entry ((code >> 16) * T + tid * S + d), T = 64 x waves per block
    uint32_t cols_magic;        // ceil(2^32 / cols) when nblocks * cols < 2^32 (then bid / cols == mulhi(bid, magic)), else 0
    uint32_t stage_magic;       // ceil(65536 / nch), nch = ceil(pitch_dw / 4): tid / nch == (tid * magic) >> 16 for tid < 256
    uint32_t stage_rpp;         // T / nch: window rows one staging pass covers
    const mv_t *coarse;         // prediction source, as in SearchArgs
    int coarse_cols, coarse_block, coarse_cell_shift;
    int mode;
    mv_t *pred;
    uint32_t *fix_count;        // length of the fix-up list (zeroed by the speculative launch)
    // speculative launch only (newest_coarse_grid): the coarser level's grids in the order its sweeps leave them (late[0] is
    // `coarse`), the word in which its solver publishes how many of them are complete, and the test setting that takes the last
    // entry whatever the word says.  late_n <= 1: every block predicts from `coarse`.
    const uint32_t *late_word;
    int late_n, late_force;
    CoarseGrid late[kMaxCoarseGrids];
    mv_t *out;
    int cols;
    int pitch_dw;               // LDS window pitch in dwords (odd)
    int nblocks;                // macroblocks of the level
    int xcd_remap;              // 1 = XCD-aware block order
    uint32_t s_plane, s_coarse, s_pred, s_out, s_fix_list;   // element strides from pair to pair (see SearchArgs); fix_count: 16 words
};
__device__ __forceinline__ void shift_pair(FastSearchArgs &a, uint32_t p)
{
    a.image1 += (size_t)p * a.s_plane; a.image2 += (size_t)p * a.s_plane;
    if (a.coarse) a.coarse += (size_t)p * a.s_coarse;
    a.pred += (size_t)p * a.s_pred; a.out += (size_t)p * a.s_out;
    a.fix_count += (size_t)p * 16u;
    if (a.late_word) a.late_word += (size_t)p * 16u;
}

// A speculative search's block picks its prediction source when it STARTS: the newest grid of the coarser level that is
// complete by then.  The level's solver stores k in late_word (release, agent scope) once the k-th sweep behind the fork is
// done (RegArgs::publish; the sweep in front of the fork stores 0, so a replay never sees the previous step's count), one lane
// reads the word once and the wave takes late[min(k, late_n - 1)].  No wait and no second look: whatever the block reads,
// k_fixup_list compares the recorded MV with the final one and k_search_list searches the block again if they differ, so the
// level ends as the search from the final prediction either way.  Why ANY outcome of the two reads is harmless:
//   - an MV is one aligned dword: a load beside a store sees the old or the new value, never a mixture;
//   - late[k] indexes inside its buffer whatever the buffer holds at that moment: small[0] holds (H/B)(W/B) cells and is read
//     at that geometry only; big[] are sized for the level's finest grid, (H/2)(W/2) cells, and an entry of cell size 2^s
//     reads below (H >> s)(W >> s) (fill_coarse_grids; tests/cpp/spec_grids_test.cpp).  They are zeroed at creation, so a grid
//     no sweep has written yet reads as zero vectors;
//   - whatever a grid buffer holds is an MV of this level or zero, and search_block_fast takes any MV: a prediction whose block
//     leaves the image gives the zero vector (:304-310), every other window is staged with its bounds checked;
//   - so a stale grid, one that a later sweep is rewriting (big[] ping-pong: entry k's buffer is written again by sweep
//     k + 2, at half the cell size) or a word that lags can only put more blocks on the fix-up list.
// The fix-up's comparison is the only correctness gate, and it is the one the search had before.
// (`table`: the kernel's argument itself, which nothing writes -- the entry is then a scalar load at a run-time offset of the
// argument segment; taken from the kernel's working copy `a` the table would live in scratch)
__device__ __forceinline__ void newest_coarse_grid(FastSearchArgs &a, const FastSearchArgs &table, uint32_t pair)
{
    uint32_t k = 0;
    if (threadIdx.x == 0) k = __hip_atomic_load(a.late_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    const uint32_t last = (uint32_t)a.late_n - 1u;
    k = a.late_force ? last : min(k, last);
    const CoarseGrid g = table.late[k];
    a.coarse = g.grid + (size_t)pair * g.stride;
    a.coarse_cols = g.cols;
    a.coarse_cell_shift = g.cell_shift;
}

// bid / cols without the (floating-point reciprocal) division sequence: one scalar multiply for a uniform bid
__device__ __forceinline__ uint32_t block_row(const FastSearchArgs &a, uint32_t bid)
{
    return a.cols_magic ? __umulhi(bid, a.cols_magic) : bid / (uint32_t)a.cols;
}

// minimum over the wave, in every lane: four DPP steps inside the rows of 16 lanes, then the four row minima through scalar registers
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x)
{
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0xB1, 0xf, 0xf, false));     // quad_perm [1,0,3,2]
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x4E, 0xf, 0xf, false));     // quad_perm [2,3,0,1]
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x141, 0xf, 0xf, false));    // row_half_mirror
    x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x140, 0xf, 0xf, false));    // row_mirror
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    return min(min(r0, r1), min(r2, r3));
}

// Current block operand: B <= 16 keeps the whole block in SGPRs; B = 32 keeps its address, and search_strip brings the block
// through the SGPRs eight rows at a time.
template <int B> struct CurBlock {
    uint32_t sg[B <= 16 ? B : 1][B <= 16 ? B / 4 : 1];
    uint64_t base;              // B = 32: image1 (wave-uniform) and the byte offset of the block's first pixel: the strip
    uint32_t off0, width;       // function loads the block eight rows at a time into SGPRs
    __device__ __forceinline__ uint32_t at(int row, int q) const { return sg[row][q]; }
};

template <int B, int S>
__device__ __forceinline__ uint32_t search_strip(const uint32_t *win, int P, const CurBlock<B> &cur,
                                                 uint32_t task, const FastSearchArgs &a, uint32_t best,
                                                 bool border, int xlo, int xhi, int ylo, int yhi,
                                                 const char *rk, uint32_t rk_off)
{
    constexpr int BW = B / 4;
    // packed u16 sums hold at most 256 pixels (255 * 256 < 2^16): B = 32 flushes them into 32-bit sums after every 8 block rows
    constexpr bool WIDE = B > 16;
    const bool idle = task == 0xffffffffu;
    const int g = idle ? 0 : (int)(task & 0xffu);
    const int dy0 = idle ? 0 : (int)((task >> 8) & 0xffu);
    unsigned long long acc[S];
    uint32_t acc32[WIDE ? S : 1][4];
#pragma unroll
    for (int d = 0; d < S; ++d) acc[d] = 0;
    if constexpr (WIDE) {
#pragma unroll
        for (int d = 0; d < S; ++d)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc32[d][c] = 0;
    }
    struct __attribute__((packed, aligned(4))) pair_w { unsigned long long v; };
    if constexpr (WIDE) {
        // B = 32: the block does not fit the scalar registers (256 dwords), and read from LDS at every use it cost an LDS read
        // per QSAD and -- fully unrolled over 39 window rows -- 512 registers plus scratch.  So the block goes through the
        // SGPRs in four bands of eight rows (64 dwords, as a whole 16 x 16 block does): per band the strip walks the
        // 8 + S - 1 window rows that meet it, the packed u16 sums (8 x 32 pixels: 255 * 256 < 2^16) are flushed into the
        // 32-bit sums, and the next band is loaded.
        typedef const uint32_t __attribute__((address_space(4))) *cptr_t;
#pragma unroll 1
        for (int band = 0; band < B / 8; ++band) {
            uint32_t cb[8][BW];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                cptr_t c1 = (cptr_t)(cur.base + cur.off0 + (uint32_t)(band * 8 + r) * cur.width);
#pragma unroll
                for (int q = 0; q < BW; ++q) cb[r][q] = c1[q];
            }
            const uint32_t *wrow = win + (dy0 + band * 8) * P + g;
            unsigned long long wn[BW];
#pragma unroll
            for (int q = 0; q < BW; ++q) wn[q] = reinterpret_cast<const pair_w *>(wrow + q)->v;
            wrow += P;
#pragma unroll
            for (int yy = 0; yy < 8 + S - 1; ++yy) {
                unsigned long long w[BW];
#pragma unroll
                for (int q = 0; q < BW; ++q) w[q] = wn[q];
                if (yy + 1 < 8 + S - 1) {
#pragma unroll
                    for (int q = 0; q < BW; ++q) wn[q] = reinterpret_cast<const pair_w *>(wrow + q)->v;
                    wrow += P;
                }
                asm volatile("" ::: "memory");
#pragma unroll
                for (int d = 0; d < S; ++d) {
                    const int brow = yy - d;                   // row of the band this window row meets
                    if (brow < 0 || brow >= 8) continue;
#pragma unroll
                    for (int q = 0; q < BW; ++q)
                        acc[d] = __builtin_amdgcn_qsad_pk_u16_u8(w[q], cb[brow][q], acc[d]);
                    asm volatile("" : "+v"(acc[d]));
                }
            }
#pragma unroll
            for (int d = 0; d < S; ++d) {
                const uint32_t lo = (uint32_t)acc[d], hi = (uint32_t)(acc[d] >> 32);
                acc32[d][0] += lo & 0xffffu; acc32[d][1] += lo >> 16;
                acc32[d][2] += hi & 0xffffu; acc32[d][3] += hi >> 16;
                acc[d] = 0;
            }
        }
    }
    // One window row ahead is kept in flight.  The QSAD chains are pure, so the optimiser would
    // sink all of them below all of the LDS reads (150+ live VGPRs, occupancy gone); the empty asm
    // statements pin the order: reads of row yy+1, then the QSADs of row yy, row after row.
    // QSAD's first operand is the 8 window bytes at dword q of the row: dwords (q, q + 1) in one register pair.  Adjacent
    // operands overlap by a dword, so building them from BW + 1 loaded dwords costs a register copy each; loading every
    // pair on its own (ds_read2_b32 q, q + 1 straight into the pair) costs LDS reads instead, which are not the limit.
    if constexpr (!WIDE) {
        const uint32_t *wrow = win + dy0 * P + g;
        unsigned long long wn[BW];
#pragma unroll
        for (int q = 0; q < BW; ++q) wn[q] = reinterpret_cast<const pair_w *>(wrow + q)->v;
        wrow += P;
#pragma unroll
        for (int yy = 0; yy < B + S - 1; ++yy) {
            unsigned long long w[BW];
#pragma unroll
            for (int q = 0; q < BW; ++q) w[q] = wn[q];
            if (yy + 1 < B + S - 1) {
#pragma unroll
                for (int q = 0; q < BW; ++q) wn[q] = reinterpret_cast<const pair_w *>(wrow + q)->v;
                wrow += P;
            }
            asm volatile("" ::: "memory");
#pragma unroll
            for (int d = 0; d < S; ++d) {
                const int brow = yy - d;                   // row of the current block this window row meets
                if (brow < 0 || brow >= B) continue;
#pragma unroll
                for (int q = 0; q < BW; ++q)
                    acc[d] = __builtin_amdgcn_qsad_pk_u16_u8(w[q], cur.at(brow, q), acc[d]);
                asm volatile("" : "+v"(acc[d]));
            }
        }
    }
    // column validity: padding columns of the last group, and (near the image border) blocks leaving the image
    unsigned long long colmask = idle ? ~0ull : 0ull;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int dxi = 4 * g + c;
        if (dxi > 2 * a.range || (border && (dxi < xlo || dxi > xhi))) colmask |= 0xffffull << (16 * c);
    }
    // the ranks of this lane's 4 S candidates: S entries of 8 bytes, contiguous (FastSearchArgs::lane_ranks) -- `rk` is the
    // round's uniform base, rk_off the lane's byte offset, the entries follow at constant offsets
    if constexpr (!WIDE) {
        // away from the image border, in a round without idle lanes or padding columns (every strip round of the tight plan),
        // no candidate needs masking: four v_perm and the minimum per candidate row, nothing else
        if (!border && !__ballot(colmask != 0ull)) {
            constexpr int CH = S < 8 ? S : 8;               // rank rows in flight at a time (registers: the sums are live too)
#pragma unroll
            for (int d0 = 0; d0 < S; d0 += CH) {
                uint2 r4[CH];
#pragma unroll
                for (int d = 0; d < CH; ++d) r4[d] = *reinterpret_cast<const uint2 *>(rk + rk_off + 8 * (d0 + d));
#pragma unroll
                for (int d = 0; d < CH; ++d) {
                    const uint32_t lo = (uint32_t)acc[d0 + d], hi = (uint32_t)(acc[d0 + d] >> 32);
                    const uint32_t k0 = __builtin_amdgcn_perm(lo, r4[d].x, 0x05040100u);
                    const uint32_t k1 = __builtin_amdgcn_perm(lo, r4[d].x, 0x07060302u);
                    const uint32_t k2 = __builtin_amdgcn_perm(hi, r4[d].y, 0x05040100u);
                    const uint32_t k3 = __builtin_amdgcn_perm(hi, r4[d].y, 0x07060302u);
                    best = min(min(best, k0), k1);                 // two v_min3_u32
                    best = min(min(best, k2), k3);
                }
                asm volatile("" ::: "memory");
            }
            return best;
        }
    }
#pragma unroll
    for (int d = 0; d < S; ++d) {
        const uint2 r4 = *reinterpret_cast<const uint2 *>(rk + rk_off + 8 * d);
        const bool row_bad = border && (dy0 + d < ylo || dy0 + d > yhi);
        if constexpr (!WIDE) {
            unsigned long long v = acc[d] | colmask;
            if (row_bad) v = ~0ull;
            const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
            // key = (sad << 16) | rank, assembled bytewise: v_perm_b32(S0 = sums, S1 = ranks)
            const uint32_t k0 = __builtin_amdgcn_perm(lo, r4.x, 0x05040100u);
            const uint32_t k1 = __builtin_amdgcn_perm(lo, r4.x, 0x07060302u);
            const uint32_t k2 = __builtin_amdgcn_perm(hi, r4.y, 0x05040100u);
            const uint32_t k3 = __builtin_amdgcn_perm(hi, r4.y, 0x07060302u);
            best = min(best, min(min(k0, k1), min(k2, k3)));
        } else {
            // key = (sad << 14) | rank: sad <= 255 * 32 * 32 < 2^18 - 1, rank < (2 * 63 + 1)^2 < 2^14 (range <= 63),
            // so a valid key stays below the 0xffffffff of an invalid candidate
            const uint32_t rank[4] = {r4.x & 0xffffu, r4.x >> 16, r4.y & 0xffffu, r4.y >> 16};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool bad = row_bad || ((colmask >> (16 * c)) & 1ull);
                const uint32_t key = bad ? 0xffffffffu : ((acc32[d][c] << 14) | rank[c]);
                best = min(best, key);
            }
        }
    }
    return best;
}

// The rim of the candidate square in the tight plan (plan_search, n = 2R + 1 = 4 G' + 1), B <= 16.
// Kind 1: candidate row `dyi` of a full column group, four lanes of a quad per (group, row), lane `part` takes a quarter of the
// block's rows -- the block operand differs from lane to lane, so it comes from the copy of the block in LDS (cur_lds), not
// from the SGPRs -- and the four packed partial sums meet by two DPP quad moves (u16 halves cannot carry: totals stay below
// 255 * B * B < 2^16).  Every lane of the wave calls it (DPP needs whole rows of 16 lanes active); idle lanes and parts
// 1..3 leave `best` alone.
template <int B>
__device__ __forceinline__ uint32_t search_row_parts(const uint32_t *win, const uint32_t *cur_lds, int P, uint32_t task,
                                                     const FastSearchArgs &a, uint32_t best, bool border,
                                                     int xlo, int xhi, int ylo, int yhi)
{
    constexpr int BW = B / 4, RP = B / 4;                      // dwords per block row, block rows per part
    struct __attribute__((packed, aligned(4))) pair_w { unsigned long long v; };
    const bool idle = task == 0xffffffffu;
    const int g = idle ? 0 : (int)(task & 0xffu);
    const int dyi = idle ? 0 : (int)((task >> 8) & 0xffu);
    const int part = idle ? 0 : (int)((task >> 16) & 3u);
    const uint32_t *wrow = win + (dyi + part * RP) * P + g;
    const uint32_t *crow = cur_lds + part * RP * BW;
    unsigned long long acc = 0;
#pragma unroll
    for (int r = 0; r < RP; ++r) {
#pragma unroll
        for (int q = 0; q < BW; ++q)
            acc = __builtin_amdgcn_qsad_pk_u16_u8(reinterpret_cast<const pair_w *>(wrow + q)->v, crow[r * BW + q], acc);
        wrow += P;
    }
    uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
    lo += dpp_row<0xB1>(lo); hi += dpp_row<0xB1>(hi);           // partner in the pair
    lo += dpp_row<0x4E>(lo); hi += dpp_row<0x4E>(hi);           // the other pair of the quad
    if (idle || part != 0) return best;
    const uint2 r4 = *reinterpret_cast<const uint2 *>(a.rank_of + (size_t)dyi * a.rank_pitch + 4 * g);
    if (border) {
        asm volatile("" ::: "memory");                          // a real branch: the interior path must not pay for the masking
        if (dyi < ylo || dyi > yhi) return best;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int dxi = 4 * g + c;
            if (dxi < xlo || dxi > xhi) { if (c < 2) lo |= 0xffffu << (16 * c); else hi |= 0xffffu << (16 * (c - 2)); }
        }
    }
    const uint32_t k0 = __builtin_amdgcn_perm(lo, r4.x, 0x05040100u);
    const uint32_t k1 = __builtin_amdgcn_perm(lo, r4.x, 0x07060302u);
    const uint32_t k2 = __builtin_amdgcn_perm(hi, r4.y, 0x05040100u);
    const uint32_t k3 = __builtin_amdgcn_perm(hi, r4.y, 0x07060302u);
    return min(best, min(min(k0, k1), min(k2, k3)));
}

// Kind 2: candidate column dx = +R, one candidate (row `dyi`) per lane.  Its window bytes start on a dword (the staged window
// starts at dx = -R on a dword and 2R is a multiple of 4), so the plain v_sad_u8 applies: block dword from the SGPRs, window
// dword from LDS, four absolute differences per lane-instruction at four times the QSAD's issue rate -- the same cost per
// candidate as a QSAD column group with four live columns, instead of one live column in four.
template <int B>
__device__ __forceinline__ uint32_t search_aligned_column(const uint32_t *win, int P, const CurBlock<B> &cur, uint32_t task,
                                                          const FastSearchArgs &a, uint32_t best, bool border,
                                                          int xlo, int xhi, int ylo, int yhi)
{
    constexpr int BW = B / 4;
    const bool idle = task == 0xffffffffu;
    const int dyi = idle ? 0 : (int)(task & 0xffu);
    const int dxi = 2 * a.range;
    const uint32_t *wrow = win + dyi * P + (dxi >> 2);
    uint32_t s0 = 0, s1 = 0;                                   // two chains: a v_sad_u8 result feeds the next one
#pragma unroll
    for (int r = 0; r < B; ++r) {
#pragma unroll
        for (int q = 0; q < BW; ++q) {
            if ((r + q) & 1) s1 = __builtin_amdgcn_sad_u8(wrow[q], cur.at(r, q), s1);
            else s0 = __builtin_amdgcn_sad_u8(wrow[q], cur.at(r, q), s0);
        }
        wrow += P;
    }
    const bool bad = idle || (border && (dxi < xlo || dxi > xhi || dyi < ylo || dyi > yhi));
    const uint32_t rank = a.rank_of[(size_t)dyi * a.rank_pitch + dxi];
    const uint32_t key = bad ? 0xffffffffu : (((s0 + s1) << 16) | rank);
    return min(best, key);
}

// The search of macroblock `bid` from the coarse MV `m` (one wave; smem = the workgroup's dynamic LDS).
// W waves share the macroblock (W = 2 on levels too small to give every SIMD two waves): they stage the window together,
// each keeps the block in its own SGPRs, wave w takes tasks [64 w, 64 w + 64) of every round, and the W minima meet in LDS.
template <int B, int W = 1>
__device__ __forceinline__ void search_block_fast(const FastSearchArgs &a, uint32_t bid, mv_t m, uint32_t *smem)
{
    constexpr int BW = B / 4;
    constexpr int T = 64 * W;                                // threads staging the window
    const int lane = threadIdx.x & 63;
    const int tid = W == 1 ? lane : (int)threadIdx.x;
    const int br = (int)block_row(a, bid), bc = (int)bid - br * a.cols;
    const int i = br * B, j = bc * B;
    const int u = 2 * mv_x(m), v = 2 * mv_y(m);             // copyMVs doubles the coarse MV (:836)
    // :233-234; the whole workgroup searches one block from one prediction: said so, the window geometry, the border tests
    // and the staging base address below stay in scalar registers
    const int px = __builtin_amdgcn_readfirstlane(j + u), py = __builtin_amdgcn_readfirstlane(i + v);
    mv_t *dst = a.out + (size_t)br * a.cols + bc;
    if (px < 0 || py < 0 || px + B > a.width || py + B > a.height) {    // :304-310 (workgroup-uniform)
        if (tid == 0) *dst = 0;
        return;
    }
    const int R = a.range, P = a.pitch_dw;
    const int wrows = B + 2 * R;
    const int wx0 = px - R, wy0 = py - R;
    const int ax0 = wx0 & ~3, sh0 = wx0 & 3;

    // stage the window.  Inside the image (the common case): 16-byte loads straight from the unaligned address wx0 --
    // gfx950 global loads take any byte address, so the re-alignment costs nothing -- a lane owns a 4-dword chunk of a
    // row, and the chunks of up to 8 passes are in flight together: the whole window in one memory trip.
    const int wbytes = 4 * P;
    if (wx0 >= 0 && wx0 + wbytes <= a.width && wy0 >= 0 && wy0 + wrows <= a.height) {
        const int nch = (P + 3) >> 2;                        // chunks per row, the last one partial
        const int rpp = (int)a.stage_rpp;                    // rows per pass: T / nch
        const int rr = (int)(((uint32_t)tid * a.stage_magic) >> 16), ch = tid - rr * nch;      // tid / nch, tid % nch
        const int nd = min(4, P - 4 * ch);                   // dwords of this lane's chunk that belong to the row
        // uniform base (scalar registers, advanced there from pass to pass) + one 32-bit byte offset per lane
        const uint8_t *ubase = a.image2 + ((size_t)wy0 * (size_t)a.width + (size_t)wx0);
        const uint32_t loff = (uint32_t)rr * (uint32_t)a.width + 16u * (uint32_t)ch;
        uint32_t *dstw = smem + rr * P + 4 * ch;
        const uint32_t sstep = (uint32_t)rpp * (uint32_t)a.width;
        const int dstep = rpp * P;
        constexpr int U = 8;
        for (int row0 = rr; row0 < wrows; row0 += rpp * U) {
            ua_u128 v[U];
#pragma unroll
            for (int t = 0; t < U; ++t)
                if (rr < rpp && row0 + t * rpp < wrows) v[t] = *reinterpret_cast<const ua_u128 *>(ubase + (size_t)((uint32_t)t * sstep) + loff);
#pragma unroll
            for (int t = 0; t < U; ++t)
                if (rr < rpp && row0 + t * rpp < wrows) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nd) dstw[t * dstep + q] = v[t].v[q];
                }
            ubase += (size_t)U * sstep;
            dstw += U * dstep;
        }
    } else {
        // near the image border: lane (rr, k) produces dword k of rows rr, rr + RPI, ... re-aligned by sh0 bytes, zeros outside
        const int rpi = T / P;                               // rows per pass
        const int rr = tid / P, k = tid - rr * P;
        if (rr < rpi) {
            const int x = ax0 + 4 * k;
            const bool x_lo_ok = x >= 0 && x + 4 <= a.width;
            const bool x_hi_ok = sh0 != 0 && x + 4 >= 0 && x + 8 <= a.width;
            for (int row = rr; row < wrows; row += rpi) {
                const int y = wy0 + row;
                uint32_t lo = 0, hi = 0;
                if (y >= 0 && y < a.height) {
                    const uint8_t *src = a.image2 + (size_t)y * a.width + x;
                    if (x_lo_ok) lo = *reinterpret_cast<const uint32_t *>(src);
                    if (x_hi_ok) hi = *reinterpret_cast<const uint32_t *>(src + 4);
                }
                smem[row * P + k] = __builtin_amdgcn_alignbyte(hi, lo, sh0);
            }
        }
    }
    // the current block: wave-uniform addresses of read-only data -> through the constant address space these are scalar
    // loads (s_load_dwordx4 / x8 per block row) instead of a vector load + v_readfirstlane per dword.  B <= 16: the whole block
    // lives in SGPRs from here on; B = 32: search_strip loads it band by band
    CurBlock<B> cur;
    {
        typedef const uint32_t __attribute__((address_space(4))) *cptr_t;
        const uint64_t base = (uint64_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uintptr_t)a.image1 >> 32)) << 32 |
                              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)a.image1);
        const uint32_t off0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)i * (uint32_t)a.width + (uint32_t)j));
        cur.base = base; cur.off0 = off0; cur.width = (uint32_t)a.width;
        if constexpr (B <= 16) {
#pragma unroll
            for (int r = 0; r < B; ++r) {
                cptr_t c1 = (cptr_t)(base + off0 + (uint32_t)r * (uint32_t)a.width);
#pragma unroll
                for (int q = 0; q < BW; ++q) cur.sg[r][q] = c1[q];
            }
        }
    }
    // B <= 16: a copy of the block behind the window in LDS, for the rounds whose lanes need different block rows (search_row_parts)
    uint32_t *cur_lds = smem + ((wrows * P + 3) & ~3);
    if constexpr (B <= 16) {
        if (tid < B * BW)
            cur_lds[tid] = *reinterpret_cast<const uint32_t *>(a.image1 + (size_t)(i + tid / BW) * a.width + j + 4 * (tid % BW));
    }
    __syncthreads();

    // candidate (dxi, dyi) in [0, 2R]^2 is valid iff its block lies inside the image (:335)
    const bool border = wx0 < 0 || wy0 < 0 || wx0 + wrows > a.width || wy0 + wrows > a.height;
    const int xlo = max(0, -wx0), xhi = min(2 * R, a.width - B - wx0);
    const int ylo = max(0, -wy0), yhi = min(2 * R, a.height - B - wy0);

    uint32_t best = 0xffffffffu;
    for (int rd = 0; rd < a.nrounds; ++rd) {
        const uint32_t code = a.rounds[rd];                 // strip height S | kind << 8 (plan_search)
        const uint32_t S = code & 0xffu;
        const uint32_t task = a.tasks[rd * T + tid];
        const uint32_t kind = (code >> 8) & 0xffu;
        if (kind) {
            if constexpr (B <= 16) {
                if (kind == 1u) best = search_row_parts<B>(smem, cur_lds, P, task, a, best, border, xlo, xhi, ylo, yhi);
                else best = search_aligned_column<B>(smem, P, cur, task, a, best, border, xlo, xhi, ylo, yhi);
            }
            continue;
        }
        // the round's rank entries: uniform base + this lane's S entries of 8 bytes
        const char *rk = reinterpret_cast<const char *>(a.lane_ranks) + (size_t)((code >> 16) * (uint32_t)T) * 8u;
        const uint32_t rk_off = (uint32_t)tid * S * 8u;
        switch (S) {
        case 16: if constexpr (B <= 16) { best = search_strip<B, 16>(smem, P, cur, task, a, best, border, xlo, xhi, ylo, yhi, rk, rk_off); } break;
        case 8:  best = search_strip<B, 8>(smem, P, cur, task, a, best, border, xlo, xhi, ylo, yhi, rk, rk_off); break;
        case 4:  best = search_strip<B, 4>(smem, P, cur, task, a, best, border, xlo, xhi, ylo, yhi, rk, rk_off); break;
        case 2:  best = search_strip<B, 2>(smem, P, cur, task, a, best, border, xlo, xhi, ylo, yhi, rk, rk_off); break;
        default: best = search_strip<B, 1>(smem, P, cur, task, a, best, border, xlo, xhi, ylo, yhi, rk, rk_off); break;
        }
    }
    best = wave_min_u32(best);
    if constexpr (W > 1) {
        __shared__ uint32_t wave_best[W];
        if (lane == 0) wave_best[threadIdx.x >> 6] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < W; ++w) best = min(best, wave_best[w]);
    }
    if (tid == 0) {
        const uint32_t sp = a.spiral[best & (B > 16 ? 0x3fffu : 0xffffu)];
        *dst = mv_pack(u + (int)(int16_t)(sp & 0xffffu), v + (int)(int16_t)(sp >> 16));   // :238-239
    }
}

template <int B, int W>
__global__ __launch_bounds__(64 * W, (W == 1 && B <= 16 ? 5 : 1)) void k_search_fast(const FastSearchArgs args)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    FastSearchArgs a = args;
    shift_pair(a, blockIdx.y);
    // Workgroups are dealt round-robin over the 8 XCDs, each with a private L2.  Give every XCD a
    // contiguous eighth of the raster so that neighbouring macroblocks -- whose windows overlap by
    // 80 % -- meet in the same L2.  Pure speed: any placement gives the same result.
    const uint32_t chunk = (uint32_t)(a.nblocks + 7) / 8;
    const uint32_t bid = a.xcd_remap ? (blockIdx.x & 7u) * chunk + (blockIdx.x >> 3) : blockIdx.x;
    if (a.mode == kSearchSpeculative && blockIdx.x == 0 && threadIdx.x == 0) *a.fix_count = 0;   // for the fix-up behind this launch
    if (bid >= (uint32_t)a.nblocks) return;
    mv_t m;                                                 // copyMVs (:828-843)
    const uint32_t brow = block_row(a, bid);
    const int i = (int)brow * B, j = (int)(bid - brow * (uint32_t)a.cols) * B;
    bool live = false;
    if constexpr (W == 1) live = a.mode == kSearchSpeculative && a.late_n > 1;     // (a speculative launch has one wave per block)
    if (live) {
        newest_coarse_grid(a, args, blockIdx.y);
        (void)search_prediction<true>(a, i, j, bid, m);
    } else if (!search_prediction(a, i, j, bid, m)) return;
    search_block_fast<B, W>(a, bid, m, smem);
}

// The fix-up behind a speculative search, in two launches (one workgroup per macroblock that mostly returns at once costs
// more in dispatch than the searches that remain): k_fixup_list compares every block's final prediction with the one the
// speculative search used and appends the blocks that differ to a list (one atomic per workgroup); k_search_list searches
// the listed blocks, workgroup w taking entries w, w + gridDim.x, ...  The speculative launch zeroes the list's counter.
__global__ __launch_bounds__(256) void k_fixup_list(FastSearchArgs a, int block, uint32_t *count, uint32_t *list)
{
    __shared__ uint32_t s_n, s_base;
    shift_pair(a, blockIdx.y);
    count = a.fix_count;
    list += (size_t)blockIdx.y * a.s_fix_list;
    const uint32_t bid = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    bool redo = false;
    if (bid < (uint32_t)a.nblocks) {
        const int i = (int)(bid / (uint32_t)a.cols) * block, j = (int)(bid % (uint32_t)a.cols) * block;
        const int ci = (i / (2 * a.coarse_block)) * a.coarse_block, cj = (j / (2 * a.coarse_block)) * a.coarse_block;
        const mv_t m = a.coarse[(size_t)(ci >> a.coarse_cell_shift) * a.coarse_cols + (cj >> a.coarse_cell_shift)];
        redo = a.pred[bid] != m;
    }
    uint32_t slot = 0;
    if (redo) slot = atomicAdd(&s_n, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) s_base = atomicAdd(count, s_n);
    __syncthreads();
    if (redo) list[s_base + slot] = bid;
}

// (five waves per SIMD, 96 registers: a fix-up list of ~5 000 blocks at 4K then fits the chip's 5 120 wave slots in ONE generation instead
// of a full one and a nearly empty one -- 64 -> 4x us at level 0)
template <int B, int W = 1>
__global__ __launch_bounds__(64 * W, (W == 1 && B <= 16 ? 5 : 1)) void k_search_list(FastSearchArgs a, const uint32_t *count, const uint32_t *list)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    shift_pair(a, blockIdx.y);
    list += (size_t)blockIdx.y * a.s_fix_list;
    const uint32_t n = *a.fix_count;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {               // wave-uniform
        const uint32_t bid = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[e]);
        const uint32_t brow = block_row(a, bid);
        mv_t m;
        (void)search_prediction(a, (int)brow * B, (int)(bid - brow * (uint32_t)a.cols) * B, bid, m);   // a.mode == kSearchPlain
        search_block_fast<B, W>(a, bid, m, smem);
        __syncthreads();                                                   // the window in LDS is re-used
    }
}

// =======================================================================================
// K2: MF::regularize_MVs / find_min_candidate / calculate_smoothness / min_energy_candidate
// (motion_framework.cpp:424-662), solved as a fixed point instead of an in-place raster sweep.
//
// The raster sweep computes new[r][c] = F(old[C,R,DR,D,DL], new[L,UL,U,UR]) -- block (r,c)
// sees the already-updated values of its left / upper neighbours and the old values of itself
// and its right / lower neighbours.  The dependency graph of `new` is acyclic, so the field
// is the unique fixed point of that system.  We reach it by:
//   pass 1   every block evaluated with new := old; a block that comes out different from its old
//            value marks its dependants R, DR, D, DL in a byte map         (k_reg_pass1)
//   relax    (0-2 launches, large grids only) the marked blocks re-evaluated in place, chip-wide,
//            plain loads and stores; changes mark dependants again          (k_reg_iter)
//   solve    the marked blocks are queued and re-evaluated; a block that changes claims its
//            dependants -- asynchronously, each wave following its own chains (k_reg_solve)
// until no block is queued.  Two to four launches per sweep, no host synchronisation.  Energies are float32 exactly as the reference's
// (SAD + lambda * mult * Smoothness, FLT_MAX for out-of-image candidates, first strict min).
//
// BS x BS blocks; LPB lanes cooperate on one block, one image row per lane.
// =======================================================================================
struct RegArgs {
    const uint8_t *image1, *image2;
    int width, height;
    int rows, cols;             // grid at this block size
    const mv_t *old_grid;       // values before the sweep
    int old_shift;              // 1 when old_grid is the parent grid (divide_blocks fused), else 0
    int old_cols;
    mv_t *est;                  // rows x cols, the field being solved
    float lambda_mult;          // lambda * (float)lambda_multiplier, computed as the reference does
    // work lists
    uint32_t *list0, *list1;    // overflow lists of the solver (block indices)
    uint32_t *own;              // ownership counters, one word per block (see "work-list state" below)
    uint32_t own_pitch;         // words per residue class of the transposed layout (own_slot)
    // dirty flags, one byte per block: a kernel consumes (and zeroes) flag_cur and marks flag_next.  A block is
    // marked when one of its already-updated inputs (L, UL, UR, U) has just been changed.
    uint8_t *flag_cur, *flag_next;
    int local_rounds;           // k_reg_iter: rounds a workgroup runs on its tile within one launch
    uint32_t wide_threshold;    // solver: queue length above which a round uses the throughput form
    uint32_t round_cap;         // most rounds / idle spins of one wave before it gives up and raises counters[5]
    uint32_t *counters;         // [0..2] overflow list lengths (rotating), [3] safety-net passes, [4] blocks re-evaluated,
                                // [5] sticky: a sweep hit a cap without converging, [6] solver ticket, [7] most rounds of
                                // one wave, [8] rounds summed, [9..15] phase profile
    // SAD memo (see "SAD memo" below): nine (MV, SAD) pairs per block, or nullptr when the sweep runs without one
    unsigned long long *memo;
    int memo_init;              // 1: the memo holds nothing for this (level, block size) yet -- pass 1 writes every slot and reads none
    int memo_forward;           // 1: a block that changes leaves its dependants' SADs of the new value in their slots (forward_sads)
    int lazy;                   // k_reg_pass1_strip, when a relaxation launch follows: blocks that need their images are not evaluated
                                // but flagged (estimate = old value meanwhile) -- the relaxation's first round evaluates them, densely
    int share;                  // solver: a wave whose queue holds more than a round takes hands the surplus to idle waves of its workgroup
    // the solver's last workgroup stores publish_value here when the sweep is complete (nullptr: nothing is stored): the
    // speculative search beside the level's late sweeps picks its prediction source by it (newest_coarse_grid)
    uint32_t *publish;          // pair 0's word, the others 16 words apart (not shifted by shift_pair: read once, in the solver's epilogue)
    uint32_t publish_value;
    int stats;                  // 1: the solver's waves add their counts to counters[4], [7..12] -- stage calls only: several hundred
                                // waves adding to the same few words is a queue at the memory side that the pyramid need not stand in
    // batch (blockIdx.y = pair): element strides from pair to pair of the per-pair buffers; counters: 64 words
    uint32_t s_plane, s_old, s_est, s_list, s_own, s_flag, s_memo;
    int flood;                  // k_reg_solve<.., true>: blocks a flood claims ahead of itself (1..3); counters[15] (with `stats`): how
                                // many speculative evaluations counted
};
__device__ __forceinline__ void shift_pair(RegArgs &a, uint32_t p)
{
    a.image1 += (size_t)p * a.s_plane; a.image2 += (size_t)p * a.s_plane;
    a.old_grid += (size_t)p * a.s_old; a.est += (size_t)p * a.s_est;
    a.list0 += (size_t)p * a.s_list; a.list1 += (size_t)p * a.s_list;
    a.own += (size_t)p * a.s_own;
    if (a.flag_cur) a.flag_cur += (size_t)p * a.s_flag;
    if (a.flag_next) a.flag_next += (size_t)p * a.s_flag;
    if (a.memo) a.memo += (size_t)p * a.s_memo;
    a.counters += (size_t)p * 64u;
}

// The solver's copy of the arguments (k_reg_solve, "HOT AND COLD ARGUMENTS"): the same fields, and a promise -- checked where the
// context is created -- that every per-pair buffer ends below 4 GiB and every dimension below 2^23.  The helpers a chain round
// inlines take it as a licence to index grids, ownership words and image rows with 32-bit offsets on the pair's 64-bit base (the
// scalar-base form of a global access, 24-bit multiplies); given a RegArgs they are, instruction for instruction, what they were.
// (The memo needs no such form: memo_load / memo_store go through a buffer descriptor, whose offsets are 32-bit already.)
struct SolverArgs : RegArgs {};
// Pass 1's copy (pass1_hot_args): the same promise, and the fields pass 1 reads -- the pair's shift is applied to those alone.
// It reaches further than the solver's: eval_block, score_block and mark_dependants, which the solver's throughput rounds
// call as they always did, take the 32-bit form for a Pass1Args only (kPass1Args).
struct Pass1Args : RegArgs {};
template <class A> constexpr bool kPass1Args = std::is_same<A, Pass1Args>::value;
template <class A> constexpr bool kOffsets32 = std::is_same<A, SolverArgs>::value || kPass1Args<A>;
// element at a 32-bit byte offset from a (scalar) 64-bit base: the scalar-base form of a global access
template <class T>
__device__ __forceinline__ T *at32(T *base, uint32_t bytes)
{
    using byte_t = typename std::conditional<std::is_const<T>::value, const char, char>::type;
    return reinterpret_cast<T *>(reinterpret_cast<byte_t *>(base) + bytes);
}

template <int BS> struct RegCfg {
    static constexpr int LPB = BS >= 4 ? (BS > 64 ? 64 : BS) : 1;   // lanes per block
    static constexpr int ROWS_PER_LANE = BS / LPB;                  // 2 for BS == 2, else 1
};

// candidate order of motion_framework.cpp:441-449: C, L, R, DR, UL, UR, U, D, DL as (drow, dcol)
static constexpr int kNbRow[9] = {0, 0, 0, 1, -1, -1, -1, 1, 1};
static constexpr int kNbCol[9] = {0, -1, 1, 1, -1, 1, 0, 0, -1};
// which of them a raster sweep has already updated when it reaches the block
#define BBME_NEW_MASK ((1u << 1) | (1u << 4) | (1u << 5) | (1u << 6))

template <bool COHERENT>
__device__ __forceinline__ mv_t load_est(const mv_t *p)
{
    if constexpr (COHERENT)   // tail kernel: written by other waves of this workgroup a pass ago
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        return *p;
}

// Score the (up to nine) candidates of block (bx, by) and return the winner: find_min_candidate,
// calculate_smoothness, min_energy_candidate (motion_framework.cpp:532-662).  All LPB lanes of the
// block's group call it; `sub` is the lane's row inside the block; `present` marks the neighbours
// that exist in the grid.  Every image row of every candidate is loaded in ONE memory trip: loads are
// unconditional -- out-of-image candidates read a clamped, harmless address and are masked afterwards
// -- because a load inside a divergent `if` costs its own round trip.
template <int BS, bool DEDUP = false, class A = RegArgs>
__device__ __forceinline__ mv_t score_block(const A &a, const mv_t (&cand)[9], uint32_t present,
                                            int bx, int by, int sub)
{
#pragma clang fp contract(off)
    constexpr int LPB = RegCfg<BS>::LPB;
    constexpr int NW = BS >= 4 ? BS / 4 : 1;              // dwords per image row segment
    constexpr int RPL = BS >= 4 ? BS / LPB : 2;           // rows per lane
    // A row segment is fetched with ONE unaligned vector load (gfx950 global loads take any byte
    // address; bbme_selftest_isa checks it): the cost of this function is the number of load
    // instructions a wave issues, since each one walks up to 64 different cache lines.
    struct __attribute__((packed, aligned(1))) row_t { uint32_t v[NW]; };
    constexpr uint32_t kMask = BS >= 4 ? 0xffffffffu : 0x0000ffffu;   // 2-pixel rows: low half of the dword
    uint32_t inside = 0;
    row_t cur[RPL];
    row_t win[9][RPL];
#pragma unroll
    for (int i = 0; i < RPL; ++i)
        if constexpr (kPass1Args<A>)   // (rows and widths below 2^23, planes below 4 GiB: see Pass1Args)
            cur[i] = *reinterpret_cast<const row_t *>(at32(a.image1, __umul24((uint32_t)(by + sub + i * LPB), (uint32_t)a.width) + (uint32_t)bx));
        else
            cur[i] = *reinterpret_cast<const row_t *>(a.image1 + (size_t)(by + sub + i * LPB) * a.width + bx);
    // DEDUP (throughput kernels): neighbouring blocks mostly carry the same MV, so a candidate whose
    // MV already occurred earlier in the list re-uses that candidate's SAD instead of gathering the same
    // image rows again.  first[k] = index of the first present candidate with the same MV.
    int first[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        first[k] = k;
        if constexpr (DEDUP) {
#pragma unroll
            for (int m = k - 1; m >= 0; --m)
                if (((present >> m) & 1u) && cand[m] == cand[k]) first[k] = m;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        int x2 = bx + mv_x(cand[k]), y2 = by + mv_y(cand[k]);
        const bool ok = ((present >> k) & 1u) &&
                        !(x2 < 0 || x2 > a.width - BS || y2 < 0 || y2 > a.height - BS);   // :578
        if (ok) inside |= 1u << k;
        else { x2 = bx; y2 = by; }                          // harmless address; result is discarded
        if (!DEDUP || first[k] == k) {
#pragma unroll
            for (int i = 0; i < RPL; ++i) {
                if constexpr (kPass1Args<A>)   // (x2, y2 lie inside the image here)
                    win[k][i] = *reinterpret_cast<const row_t *>(at32(a.image2, __umul24((uint32_t)(y2 + sub + i * LPB), (uint32_t)a.width) + (uint32_t)x2));
                else
                    win[k][i] = *reinterpret_cast<const row_t *>(a.image2 + (size_t)(y2 + sub + i * LPB) * a.width + x2);
            }
        } else {                                            // duplicate: loads skipped under the exec mask
#pragma unroll
            for (int i = 0; i < RPL; ++i)
#pragma unroll
                for (int q = 0; q < NW; ++q) win[k][i].v[q] = 0;
        }
    }
    // ---- SADs, reduced over the block's lanes ---------------------------------------------------
    float energy[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        uint32_t sad = 0;
#pragma unroll
        for (int i = 0; i < RPL; ++i)
#pragma unroll
            for (int q = 0; q < NW; ++q)
                sad = __builtin_amdgcn_sad_u8(cur[i].v[q] & kMask, win[k][i].v[q] & kMask, sad);
        // sum over the block's LPB lanes (aligned groups inside a DPP row of 16): partner in the pair, in the quad, in the
        // half row, in the row -- VALU moves instead of LDS shuffles -- and across rows for the larger blocks
        if constexpr (LPB >= 2) sad += dpp_row<0xB1>(sad);
        if constexpr (LPB >= 4) sad += dpp_row<0x4E>(sad);
        if constexpr (LPB >= 8) sad += dpp_row<0x141>(sad);
        if constexpr (LPB >= 16) sad += dpp_row<0x140>(sad);
        if constexpr (LPB >= 32) sad += __shfl_xor(sad, 16);
        if constexpr (LPB >= 64) sad += __shfl_xor(sad, 32);
        energy[k] = (float)sad;
    }
    if constexpr (DEDUP) {
#pragma unroll
        for (int k = 1; k < 9; ++k) {
            float e = energy[k];
#pragma unroll
            for (int m = 0; m < k; ++m) if (first[k] == m) e = energy[m];
            energy[k] = e;
        }
    }
    // calculate_smoothness (:623-644) with v_sad_u16 on bias-shifted halves: |u_m-u_k| + |v_m-v_k|
    int best = -1;
    float best_e = 0.f;
    if (present == 0x1ffu) {
        // away from the grid's border (nearly every block): all nine candidates exist -- 81 unconditional terms
        uint32_t cb[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) cb[k] = cand[k] ^ 0x80008000u;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            uint32_t smooth = 0;
#pragma unroll
            for (int m = 0; m < 9; ++m)
                if (m != k) smooth = __builtin_amdgcn_sad_u16(cb[m], cb[k], smooth);
            const float t = a.lambda_mult * (float)smooth;
            float e = energy[k] + t;                                             // :607
            if (!((inside >> k) & 1u)) e = 3.402823466e+38f;                     // FLT_MAX :580
            if (k == 0 || e < best_e) { best = k; best_e = e; }                 // first strict min :648-660
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (!((present >> k) & 1u)) continue;
            float e = 3.402823466e+38f;                                          // FLT_MAX :580
            if ((inside >> k) & 1u) {
                const uint32_t ck = cand[k] ^ 0x80008000u;
                uint32_t smooth = 0;
#pragma unroll
                for (int m = 0; m < 9; ++m)
                    if ((present >> m) & 1u)
                        smooth = __builtin_amdgcn_sad_u16(cand[m] ^ 0x80008000u, ck, smooth);
                const float t = a.lambda_mult * (float)smooth;
                e = energy[k] + t;                                               // :607
            }
            if (best < 0 || e < best_e) { best = k; best_e = e; }               // first strict min :648-660
        }
    }
    mv_t res = cand[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) if (best == k) res = cand[k];
    return res;
}

// Evaluate block (r, c) with its candidates read from global memory (one trip for all nine):
// use_new = bit mask of the candidates read from `est` instead of `old_grid`.  `own`, if given, takes candidate 0 as it was loaded.
template <int BS, bool COHERENT, bool DEDUP = false, class A = RegArgs>
__device__ __forceinline__ mv_t eval_block(const A &a, int r, int c, int sub, uint32_t use_new, mv_t *own = nullptr)
{
    mv_t cand[9];
    uint32_t present = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int rr = r + kNbRow[k], cc = c + kNbCol[k];
        if (rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols) present |= 1u << k;
        const int rs = min(max(rr, 0), a.rows - 1), cs = min(max(cc, 0), a.cols - 1);
        if constexpr (kPass1Args<A>) {
            if ((use_new >> k) & 1u)
                cand[k] = load_est<COHERENT>(at32(a.est, (__umul24((uint32_t)rs, (uint32_t)a.cols) + (uint32_t)cs) << 2));
            else
                cand[k] = *at32(a.old_grid, (__umul24((uint32_t)(rs >> a.old_shift), (uint32_t)a.old_cols) + (uint32_t)(cs >> a.old_shift)) << 2);
        } else {
            if ((use_new >> k) & 1u)
                cand[k] = load_est<COHERENT>(a.est + (size_t)rs * a.cols + cs);
            else
                cand[k] = a.old_grid[(size_t)(rs >> a.old_shift) * a.old_cols + (cs >> a.old_shift)];
        }
    }
    if (own) *own = cand[0];
    // All candidates equal (the common case inside a moving region): they have the same SAD and the same smoothness
    // (or all lie outside the image: FLT_MAX), so the first one -- the block's own old MV -- stays (:648-660).
    // No image row is touched; whole waves leave here where the field is locally constant.
    bool uniform = true;
#pragma unroll
    for (int k = 1; k < 9; ++k) uniform &= !((present >> k) & 1u) || cand[k] == cand[0];
    if (uniform) return cand[0];
    return score_block<BS, DEDUP>(a, cand, present, c * BS, r * BS, sub);
}

// Latency form of the evaluation, used where one wave walks a dependency chain (k_reg_solve and the
// safety net): a lone wave issues about one instruction per four cycles, so the ~1000 instructions
// of the nine-candidates-per-lane form above ARE the round time.  Here a block is handled by a group
// of 16 lanes and lane k < 9 owns candidate k: its address arithmetic, its image rows, its SAD, its
// smoothness term (the other candidates arrive by shuffle) and its energy -- the same float expression
// as in score_block, so the same winner: lowest energy, ties to the lowest k (:648-660).
// Phase profile of a LANES round (development aid, compiled only with -DBBME_PHASE_PROFILE): shader-clock
// stamps, each after every outstanding memory operation has returned, summed per phase in counters[9..15].
#ifdef BBME_PHASE_PROFILE
struct PhaseProf { uint32_t ph[7]; unsigned long long last; };
__device__ __forceinline__ void phase_stamp(PhaseProf *p, int i)
{
    if (!p) return;
    unsigned long long t;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    if (i >= 0) p->ph[i] += (uint32_t)(t - p->last);
    p->last = t;
}
#define BBME_PHASE(p, i) phase_stamp(p, i)
#else
struct PhaseProf;
#define BBME_PHASE(p, i) ((void)0)
#endif

// Which estimate lane k16 of a 16-lane group reads for block (r, c): candidate k = k16 (lanes 9..15
// shadow candidate 0 and are ignored).
struct LaneCand {
    const mv_t *src;            // where the candidate's MV lives (est for the already-updated inputs, else old_grid)
    bool present;               // k16 < 9 and the neighbour exists
};
// The part of lanes_candidate that depends on the lane only (a chain walker computes it once, not every round): the
// neighbour's offset, and where its MV lives -- `est` for the inputs a raster sweep has already updated, else `old_grid`.
struct LaneGeom {
    const mv_t *base;
    int drow, dcol, pitch, shift;
    bool cand;                  // k16 < 9
};
__device__ __forceinline__ LaneGeom lanes_geometry(const RegArgs &a, int k16, uint32_t use_new)
{
    constexpr uint32_t kRowCode = 1u | 1u << 2 | 1u << 4 | 2u << 6 | 0u << 8 | 0u << 10 | 0u << 12 | 2u << 14 | 2u << 16;
    constexpr uint32_t kColCode = 1u | 0u << 2 | 2u << 4 | 2u << 6 | 0u << 8 | 2u << 10 | 1u << 12 | 1u << 14 | 0u << 16;
    const int k = k16 < 9 ? k16 : 0;
    LaneGeom lg;
    lg.cand = k16 < 9;
    lg.drow = (int)((kRowCode >> (2 * k)) & 3u) - 1;
    lg.dcol = (int)((kColCode >> (2 * k)) & 3u) - 1;
    const bool is_new = (use_new >> k) & 1u;
    lg.base = is_new ? a.est : a.old_grid;
    lg.pitch = is_new ? a.cols : a.old_cols;
    lg.shift = is_new ? 0 : a.old_shift;
    return lg;
}
template <class A>
__device__ __forceinline__ LaneCand lanes_candidate(const A &a, const LaneGeom &lg, int r, int c)
{
    const int rr = r + lg.drow, cc = c + lg.dcol;
    LaneCand lc;
    lc.present = lg.cand && (uint32_t)rr < (uint32_t)a.rows && (uint32_t)cc < (uint32_t)a.cols;
    const int rs = min(max(rr, 0), a.rows - 1), cs = min(max(cc, 0), a.cols - 1);
    if constexpr (kOffsets32<A>) lc.src = lg.base + (uint32_t)(__mul24(rs >> lg.shift, lg.pitch) + (cs >> lg.shift));
    else lc.src = lg.base + (size_t)((rs >> lg.shift) * lg.pitch + (cs >> lg.shift));
    return lc;
}
__device__ __forceinline__ LaneCand lanes_candidate(const RegArgs &a, int r, int c, int k16, uint32_t use_new)
{
    // (drow + 1) and (dcol + 1) of candidate k, two bits each, order C,L,R,DR,UL,UR,U,D,DL (:441-449)
    constexpr uint32_t kRowCode = 1u | 1u << 2 | 1u << 4 | 2u << 6 | 0u << 8 | 0u << 10 | 0u << 12 | 2u << 14 | 2u << 16;
    constexpr uint32_t kColCode = 1u | 0u << 2 | 2u << 4 | 2u << 6 | 0u << 8 | 2u << 10 | 1u << 12 | 1u << 14 | 0u << 16;
    const int k = k16 < 9 ? k16 : 0;
    const int rr = r + (int)((kRowCode >> (2 * k)) & 3u) - 1, cc = c + (int)((kColCode >> (2 * k)) & 3u) - 1;
    LaneCand lc;
    lc.present = k16 < 9 && rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols;
    const int rs = min(max(rr, 0), a.rows - 1), cs = min(max(cc, 0), a.cols - 1);
    // one load instruction for all lanes (a divergent if / else would cost two memory trips): the
    // already-updated inputs come from `est`, the others from `old_grid`, all through the coherent path
    lc.src = ((use_new >> k) & 1u) ? a.est + (size_t)rs * a.cols + cs
                                   : a.old_grid + (size_t)(rs >> a.old_shift) * a.old_cols + (cs >> a.old_shift);
    return lc;
}

// pass 1's form: every candidate comes from the old grid (use_new = 0), at a 32-bit byte offset from its base
__device__ __forceinline__ LaneCand lanes_candidate(const Pass1Args &a, int r, int c, int k16, uint32_t)
{
    constexpr uint32_t kRowCode = 1u | 1u << 2 | 1u << 4 | 2u << 6 | 0u << 8 | 0u << 10 | 0u << 12 | 2u << 14 | 2u << 16;
    constexpr uint32_t kColCode = 1u | 0u << 2 | 2u << 4 | 2u << 6 | 0u << 8 | 2u << 10 | 1u << 12 | 1u << 14 | 0u << 16;
    const int k = k16 < 9 ? k16 : 0;
    const int rr = r + (int)((kRowCode >> (2 * k)) & 3u) - 1, cc = c + (int)((kColCode >> (2 * k)) & 3u) - 1;
    LaneCand lc;
    lc.present = k16 < 9 && (uint32_t)rr < (uint32_t)a.rows && (uint32_t)cc < (uint32_t)a.cols;
    const int rs = min(max(rr, 0), a.rows - 1), cs = min(max(cc, 0), a.cols - 1);
    lc.src = at32(a.old_grid, (__umul24((uint32_t)(rs >> a.old_shift), (uint32_t)a.old_cols) + (uint32_t)(cs >> a.old_shift)) << 2);
    return lc;
}

// ---- SAD memo -------------------------------------------------------------------------------
// The reference memoises block SADs in `fast_array` (motion_framework.h:46, .cpp:594-602: a hit returns what :599 would
// recompute).  Here, for the block sizes whose SAD is worth keeping (b >= 8), every block owns one slot per candidate:
// (MV, SAD(block, MV)) of that candidate at its last evaluation.  SAD(block, MV) is a pure function of the two level planes
// and the block size, so a slot is a FACT, not state: whoever wrote it and whenever, a slot whose MV equals the
// candidate's MV carries that candidate's SAD.  That is what makes the memo safe under the solver's asynchrony -- slots
// are single 8-byte words (never torn), a stale or overwritten slot is still true (so the words need no coherence beyond
// the XCD's L2), and the only obligation is that no slot survives a change of (planes, block size): the first pass 1 at a
// block size (RegArgs::memo_init) rewrites every slot, and kernel boundaries write every L2 back.
// A chain round on a lone wave costs what it ISSUES (~5 cycles an instruction) plus its dependent memory trips, so the memo
// is used the cheapest way: candidate k looks at slot k only (one compare), else at slot 0 (the block's own vector: in a
// region about to be flooded all the other candidates equal it); what is still unknown is summed by the lane group, one
// image row per lane; and a block that changes leaves SAD(dependant, new MV) in the slot through which each of its
// dependants R, DR, D, DL will see the new value (forward_sads) -- computed while its own store drains, so that the
// re-evaluation the change triggers, the next link of the chain, touches no image row at all.
constexpr uint32_t kMemoNoMv = 0x80008000u;       // (-32768, -32768): never a motion vector
constexpr uint32_t kMemoNoSad = 0xffffffffu;      // "not known": every real SAD is below 255 * 64 * 64
constexpr int kMemoSlotShift = 4;                  // 16 words (one 128-byte line) per block, nine used
// what the solver's chain rounds found in the memo (wave-uniform sums; bbme_sweep_stats words 9..12, unless the build is a
// phase-profile build, which keeps its cycle counts there)
struct MemoStats { uint32_t lookups = 0, misses = 0, passes = 0, forwards = 0; };

// Memo words are read and written through a raw buffer descriptor, which is what carries the cache policy wanted here:
// the solver's loads miss the (per-CU, incoherent) L1 and are served by the XCD's L2 (sc0), stores are plain write-throughs
// to that L2.  Nothing is forced out to the memory side as the estimates are: the solver deals a band of the raster to each
// XCD, so a block's slots are read where they were written; a wave of another XCD sees older words -- still facts -- and a
// store that had to complete at the memory side (sc1) would sit in front of the round's atomics on the in-order counter.
typedef uint32_t memo_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t memo_rsrc(const RegArgs &a)
{
    return __builtin_amdgcn_make_buffer_rsrc(a.memo, 0, 0x7fffffff, 0x00020000);
}
template <bool COHERENT>
__device__ __forceinline__ uint2 memo_load(const RegArgs &a, uint32_t word)
{
    const memo_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(memo_rsrc(a), (int)(word * 8u), 0, COHERENT ? 1 : 0);
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void memo_store(const RegArgs &a, uint32_t word, uint32_t mv, uint32_t sad)
{
    const memo_u32x2 v = {mv, sad};
    __builtin_amdgcn_raw_buffer_store_b64(v, memo_rsrc(a), (int)(word * 8u), 0, 0);
}

// LPM lanes of a 16-lane group share the pixels of one BS x BS block (and one motion vector): 16 / LPM blocks at a time.
// A lane takes whole rows (sub, sub + LPM, ...) or, with more lanes than rows (b = 8 on 16 lanes), one part of a row.
template <int BS, int LPM> struct GroupSad {
    static_assert(LPM == 4 || LPM == 8 || LPM == 16, "lanes per block");
    static constexpr int PARTS = LPM > BS ? LPM / BS : 1;      // lanes per row
    static constexpr int RPL = LPM > BS ? 1 : BS / LPM;        // rows per lane
    static constexpr int NW = BS / 4 / PARTS;                  // dwords per lane and row
    static_assert(NW >= 1, "a lane needs at least a dword");
    struct __attribute__((packed, aligned(1))) row_t { uint32_t v[NW]; };
    static __device__ __forceinline__ void load(const uint8_t *img, int width, int x, int y, int sub, row_t (&rows)[RPL])
    {
        const int row = PARTS > 1 ? sub / PARTS : sub, col = PARTS > 1 ? (sub % PARTS) * 4 * NW : 0;
        const uint8_t *p = img + (uint32_t)((y + row) * width + x + col);
#pragma unroll
        for (int i = 0; i < RPL; ++i) rows[i] = *reinterpret_cast<const row_t *>(p + (uint32_t)(i * LPM * width));
    }
    // sum of absolute differences of the lane's pixels, reduced over the LPM lanes: every one of them returns the block's SAD
    static __device__ __forceinline__ uint32_t reduce(const row_t (&u)[RPL], const row_t (&w)[RPL])
    {
        uint32_t s0 = 0, s1 = 0;
#pragma unroll
        for (int i = 0; i < RPL; ++i)
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                if ((i + q) & 1) s1 = __builtin_amdgcn_sad_u8(u[i].v[q], w[i].v[q], s1);
                else s0 = __builtin_amdgcn_sad_u8(u[i].v[q], w[i].v[q], s0);
            }
        uint32_t s = s0 + s1;
        s += dpp_row<0xB1>(s);
        s += dpp_row<0x4E>(s);
        if constexpr (LPM >= 8) s += dpp_row<0x141>(s);
        if constexpr (LPM >= 16) s += dpp_row<0x140>(s);
        return s;
    }
};

// SADs of the candidates the memo does not know, summed by the group, one vector per pass: the lowest lane in need names it
// (a row minimum of lane << 28 | vector, four DPP steps -- vectors are below 2^13 in magnitude wherever the memo is used,
// which the host checks), the 16 lanes take a row (or several) each, every lane holding that vector takes the sum.  The
// loop is wave-uniform and ends when no lane of the wave needs one.
template <int BS>
__device__ __forceinline__ uint32_t group_sads(const RegArgs &a, int bx, int by, int k16, bool need, mv_t mv, uint32_t sad,
                                               MemoStats *stats = nullptr)
{
    using G = GroupSad<BS, 16>;
    typename G::row_t cur[G::RPL];
    G::load(a.image1, a.width, bx, by, k16, cur);
    const uint32_t packed = (mv & 0x3fffu) | ((mv >> 2) & 0x0fffc000u);      // 14 bits of dx, 14 bits of dy
    do {
        uint32_t key = need ? ((uint32_t)k16 << 28) | packed : 0xffffffffu;
        key = min(key, dpp_row<0xB1>(key)); key = min(key, dpp_row<0x4E>(key));
        key = min(key, dpp_row<0x141>(key)); key = min(key, dpp_row<0x140>(key));
        const bool mine = need && ((key ^ packed) & 0x0fffffffu) == 0u;
        // a group without a lane in need (key = -1) reads the block's own position: dx = dy = 0 after the mask below
        const bool any = key != 0xffffffffu;
        const int dx = any ? ((int)(key << 18) >> 18) : 0, dy = any ? ((int)(key << 4) >> 18) : 0;
        typename G::row_t win[G::RPL];
        G::load(a.image2, a.width, bx + dx, by + dy, k16, win);
        const uint32_t s = G::reduce(cur, win);
        if (mine) { sad = s; need = false; }
        if (stats) stats->passes += 1;
    } while (__ballot(need));
    return sad;
}

// A block took the value `res`: leave SAD(dependant, res) in the slot through which each of its dependants R, DR, D, DL
// will see it (candidate L, UL, U, UR of theirs).  Called between the estimate's store and the wait for it: the image
// rows travel while the store drains.  `go`: the group's block changed (group-uniform); r, c, res are the group's.
// b <= 16: the four quads of the group take one dependant each, a quarter of its rows per lane -- one pass.
template <int BS>
__device__ __forceinline__ void forward_sads(const RegArgs &a, int r, int c, int k16, bool go, mv_t res)
{
    constexpr int LPM = BS <= 16 ? 4 : 16;
    using G = GroupSad<BS, LPM>;
    constexpr int PER = 16 / LPM;                                          // dependants per pass
#pragma unroll
    for (int d0 = 0; d0 < 4; d0 += PER) {
        const int d = d0 + (PER == 4 ? (k16 >> 2) : 0);                    // (0,+1) (+1,+1) (+1,0) (+1,-1)
        const int tr = r + (d != 0), tc = c + (d < 2 ? 1 : 2 - d);
        const int bx = tc * BS, by = tr * BS;
        const int x2 = bx + mv_x(res), y2 = by + mv_y(res);
        const bool ok = go && tr < a.rows && tc >= 0 && tc < a.cols &&
                        !(x2 < 0 || x2 > a.width - BS || y2 < 0 || y2 > a.height - BS);
        typename G::row_t u[G::RPL], w[G::RPL];
        G::load(a.image1, a.width, ok ? bx : 0, ok ? by : 0, k16 & (LPM - 1), u);
        G::load(a.image2, a.width, ok ? x2 : 0, ok ? y2 : 0, k16 & (LPM - 1), w);
        const uint32_t s = G::reduce(u, w);
        const uint32_t slot = d == 0 ? 1u : d == 1 ? 4u : d == 2 ? 6u : 5u;   // R sees it as L, DR as UL, D as U, DL as UR
        if (ok && (k16 & (LPM - 1)) == 0)
            memo_store(a, (((uint32_t)(tr * a.cols + tc)) << kMemoSlotShift) | slot, res, s);
    }
}

// SAD of this lane's candidate, every row walked by the lane itself (no memo): the rows are independent loads, issued
// back to back
template <int BS, class A>
__device__ __forceinline__ uint32_t lane_sad(const A &a, int bx, int by, int x2, int y2)
{
    constexpr int NW = BS >= 4 ? BS / 4 : 1;
    struct __attribute__((packed, aligned(1))) row_t { uint32_t v[NW]; };
    constexpr uint32_t kMask = BS >= 4 ? 0xffffffffu : 0x0000ffffu;
    uint32_t sad0 = 0, sad1 = 0;                              // two chains: v_sad_u8 results feed the next one
    if constexpr (kOffsets32<A> && BS <= 16) {
        // every row at a 32-bit offset from the plane's (scalar) base: one 32-bit add a row
        const uint32_t w = (uint32_t)a.width;
        uint32_t o1 = __umul24((uint32_t)by, w) + (uint32_t)bx, o2 = __umul24((uint32_t)y2, w) + (uint32_t)x2;
        row_t u[BS], v[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            u[i] = *reinterpret_cast<const row_t *>(a.image1 + o1);
            v[i] = *reinterpret_cast<const row_t *>(a.image2 + o2);
            o1 += w; o2 += w;
        }
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                if ((i + q) & 1) sad1 = __builtin_amdgcn_sad_u8(u[i].v[q] & kMask, v[i].v[q] & kMask, sad1);
                else sad0 = __builtin_amdgcn_sad_u8(u[i].v[q] & kMask, v[i].v[q] & kMask, sad0);
            }
        return sad0 + sad1;
    }
    const uint8_t *p1 = a.image1 + (size_t)by * a.width + bx;
    const uint8_t *p2 = a.image2 + (size_t)y2 * a.width + x2;
    // b <= 16: every row in flight at once.  b >= 32: eight rows at a time -- 2 x 32 rows of 8+ dwords do not fit the 256
    // architectural registers, and the accumulation registers the compiler parks them in cost a copy each way
    constexpr int CHUNK = BS >= 32 ? 8 : BS;
    for (int row0 = 0; row0 < BS; row0 += CHUNK) {
        row_t u[CHUNK], w[CHUNK];
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) {
            u[i] = *reinterpret_cast<const row_t *>(p1 + (size_t)(row0 + i) * a.width);
            w[i] = *reinterpret_cast<const row_t *>(p2 + (size_t)(row0 + i) * a.width);
        }
#pragma unroll
        for (int i = 0; i < CHUNK; ++i)
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                if ((i + q) & 1) sad1 = __builtin_amdgcn_sad_u8(u[i].v[q] & kMask, w[i].v[q] & kMask, sad1);
                else sad0 = __builtin_amdgcn_sad_u8(u[i].v[q] & kMask, w[i].v[q] & kMask, sad0);
            }
        if constexpr (BS >= 32) asm volatile("" ::: "memory");   // keep the chunks apart
    }
    return sad0 + sad1;
}

// Second half: lane k16 of the group holds candidate k16's MV `mv`; every lane of the group returns the winner.
// MEMO: `memo` is what the lane's slot held (slot k16; lanes 9..15 shadow slot 0) and `slot` where it lives.
template <int BS, bool MEMO = false, bool COHERENT = false, bool GROUP = ((COHERENT && BS >= 16) || BS >= 32), class A>
__device__ __forceinline__ mv_t lanes_score(const A &a, int r, int c, int k16, bool present, mv_t mv,
                                            PhaseProf *prof = nullptr, uint2 memo = make_uint2(0, 0),
                                            uint32_t slot = 0, MemoStats *stats = nullptr)
{
#pragma clang fp contract(off)
    const int bx = c * BS, by = r * BS;
    int x2 = bx + mv_x(mv), y2 = by + mv_y(mv);
    const bool inside = present && !(x2 < 0 || x2 > a.width - BS || y2 < 0 || y2 > a.height - BS);   // :578
    if (!inside) { x2 = bx; y2 = by; }
    uint32_t sad;
    if constexpr (MEMO) {
        // slot k knows candidate k's SAD if it holds candidate k's vector; else slot 0 may (the block's own vector)
        sad = memo.x == mv ? memo.y : kMemoNoSad;
        {
            const uint32_t m0 = dpp_row<0x150>(memo.x), s0 = dpp_row<0x150>(memo.y);
            sad = (sad == kMemoNoSad && m0 == mv) ? s0 : sad;
        }
        const bool need = inside && sad == kMemoNoSad;
        const unsigned long long nball = __ballot(need);
        if (stats) { stats->lookups += (uint32_t)__popcll(__ballot(inside)); stats->misses += (uint32_t)__popcll(nball); }
        if (nball) {
            if constexpr (GROUP) sad = group_sads<BS>(a, bx, by, k16, need, mv, sad, stats);
            else if (need) sad = lane_sad<BS>(a, bx, by, x2, y2);           // pass 1 at b <= 16, and b = 8 everywhere: the lanes in need walk
                                                                            // their own rows -- any number of different vectors in one trip
        }
        // the slot now describes this lane's candidate (or nothing, if it has no SAD); written only when that is news
        const uint32_t nmv = inside ? mv : kMemoNoMv, nsad = inside ? sad : 0u;
        if (k16 < 9 && (a.memo_init || nmv != memo.x || nsad != memo.y)) memo_store(a, slot, nmv, nsad);
    } else {
        sad = lane_sad<BS>(a, bx, by, x2, y2);
    }
    BBME_PHASE(prof, 1);                                      // row loads + SAD
    // smoothness: sum over the present candidates of |u_m - u_k| + |v_m - v_k| (:637-641).  The group is
    // one DPP row of 16 lanes: candidate m reaches every lane by row_newbcast (a VALU move, no LDS trip)
    const int lane = (int)(threadIdx.x & 63u);
    const int base = lane & ~15;
    const unsigned long long pball = __ballot(present);
    const uint32_t mine = mv ^ 0x80008000u;
    uint32_t smooth = 0;
    // (lanes 9..15 of a group are never present: a group away from the grid's border shows 0x01ff in its 16 bits)
    const unsigned long long aball = __ballot(true);          // the active groups, 16 lanes each
    if (pball == (aball & 0x01ff01ff01ff01ffull)) {
        // no block of the round touches the border of the grid -- nearly always: nine unconditional terms
#define BBME_SMOOTH_TERM(m) smooth = __builtin_amdgcn_sad_u16(dpp_row<0x150 + (m)>(mine), mine, smooth);
        BBME_SMOOTH_TERM(0) BBME_SMOOTH_TERM(1) BBME_SMOOTH_TERM(2) BBME_SMOOTH_TERM(3) BBME_SMOOTH_TERM(4)
        BBME_SMOOTH_TERM(5) BBME_SMOOTH_TERM(6) BBME_SMOOTH_TERM(7) BBME_SMOOTH_TERM(8)
#undef BBME_SMOOTH_TERM
    } else {
        const uint32_t pmask = (uint32_t)(pball >> base) & 0x1ffu;
#define BBME_SMOOTH_TERM(m) \
    { const uint32_t other = dpp_row<0x150 + (m)>(mine); if ((pmask >> (m)) & 1u) smooth = __builtin_amdgcn_sad_u16(other, mine, smooth); }
        BBME_SMOOTH_TERM(0) BBME_SMOOTH_TERM(1) BBME_SMOOTH_TERM(2) BBME_SMOOTH_TERM(3) BBME_SMOOTH_TERM(4)
        BBME_SMOOTH_TERM(5) BBME_SMOOTH_TERM(6) BBME_SMOOTH_TERM(7) BBME_SMOOTH_TERM(8)
#undef BBME_SMOOTH_TERM
    }
    float e = 3.402823466e+38f;                                                 // FLT_MAX :580
    if (inside) {
        const float t = a.lambda_mult * (float)smooth;
        e = (float)sad + t;                                                     // :607
    }
    // energies are >= 0, so their bit patterns order like the floats; absent lanes sort last.  Three all-reduces over the
    // row of 16 lanes (partner in the pair, in the quad, in the half row, in the row), each a single DPP-fused instruction per
    // step: the lowest energy; the lowest candidate index that has it (first strict minimum, :648-660); that candidate's MV
    const uint32_t ebits = present ? __float_as_uint(e) : 0xffffffffu;
    uint32_t emin = ebits;
#define BBME_ROW_ALLREDUCE(var, op) \
    var = op(var, dpp_row<0xB1>(var)); var = op(var, dpp_row<0x4E>(var)); var = op(var, dpp_row<0x141>(var)); var = op(var, dpp_row<0x140>(var));
    BBME_ROW_ALLREDUCE(emin, min)
    uint32_t who = ebits == emin ? (uint32_t)k16 : 15u;      // candidate 0 is always present, so emin belongs to a present one
    BBME_ROW_ALLREDUCE(who, min)
    uint32_t wmv = (uint32_t)k16 == who ? mv : 0u;
#define BBME_OR(a, b) ((a) | (b))
    BBME_ROW_ALLREDUCE(wmv, BBME_OR)
#undef BBME_OR
#undef BBME_ROW_ALLREDUCE
    const mv_t winner = wmv;
    BBME_PHASE(prof, 2);                                      // smoothness + energy + argmin
    return winner;
}

template <int BS, bool COHERENT, bool MEMO = false, class A>
__device__ __forceinline__ mv_t eval_block_lanes(const A &a, int r, int c, int k16, uint32_t use_new,
                                                 PhaseProf *prof = nullptr, const LaneGeom *lg = nullptr, MemoStats *stats = nullptr,
                                                 mv_t *own_out = nullptr)
{
    const LaneCand lc = lg ? lanes_candidate(a, *lg, r, c) : lanes_candidate(a, r, c, k16, use_new);
    uint32_t slot = 0;                                        // the lane's memo word (index into RegArgs::memo)
    uint2 memo = make_uint2(kMemoNoMv, 0u);
    if constexpr (MEMO) {
        // the memo slot rides in the candidates' memory trip
        slot = (((uint32_t)(r * a.cols + c)) << kMemoSlotShift) | (uint32_t)(k16 < 9 ? k16 : 0);
        if (!a.memo_init) memo = memo_load<COHERENT>(a, slot);
    }
    const mv_t mv = load_est<COHERENT>(lc.src);
    BBME_PHASE(prof, 0);                                      // queue pop + address arithmetic + gather trip
    // every block of the round has nine equal candidates (behind a flood that has passed): equal SADs, equal smoothness, the
    // first one -- the block's own MV -- stays (:648-660), as in eval_block; no image row is touched
    const mv_t own = dpp_row<0x150>(mv);
    if (own_out) *own_out = own;                              // candidate 0 as the group's first lane loaded it
    if (!__ballot(lc.present && mv != own)) {
        if constexpr (MEMO) {
            if (a.memo_init && k16 < 9) memo_store(a, slot, kMemoNoMv, 0u);   // nothing known yet
        }
        return own;
    }
    return lanes_score<BS, MEMO, COHERENT>(a, r, c, k16, lc.present, mv, prof, memo, slot, stats);
}

// ---- work-list state ---------------------------------------------------------------------
// One counter word per block in `own`, agent-scope atomics only:
//   0      nobody is responsible for the block;
//   >= 1   exactly one wave OWNS it: it sits in that wave's LDS queue (or on a global list) or is
//          being evaluated by it.  Only the owner ever evaluates the block and stores its estimate;
//   >= 2   an input changed after the owner took it: the owner must evaluate it once more.
// claim  fetch_add(1) -- issued by a wave that changed one of the block's inputs, AFTER that
//        store has completed (and by the scan for blocks pass 1 left stale).  Old value 0: the
//        caller becomes the owner and queues the block; its input loads come after this atomic,
//        so they see every change made before it.  Old value > 0: the owner will redo it.
// release after the owner's own store has completed: exchange with 0.  Old value >= 2: claim again.
// Every change is followed by a claim on each dependant, every claimed block is evaluated with
// inputs loaded after the claim, and no two waves evaluate one block at the same time; when every
// queue is empty the field is the fixed point.
// Layout: block x lives in word (x mod 32) * pitch + x / 32, pitch = 33 mod 64.  Neighbouring blocks
// -- the ones a chain, or a cluster of stale blocks, claims at the same time -- are thus 132 bytes
// (mod 256) apart: different cache lines on different L2 channels, instead of 32 atomics queueing
// on one line.
__device__ __forceinline__ uint32_t own_slot(const RegArgs &a, uint32_t x) { return (x & 31u) * a.own_pitch + (x >> 5); }
template <class A>
__device__ __forceinline__ uint32_t *own_word(const A &a, uint32_t x)
{
    if constexpr (kOffsets32<A>)
        return reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(a.own) + ((__umul24(x & 31u, a.own_pitch) + (x >> 5)) << 2));
    else
        return &a.own[own_slot(a, x)];
}
template <class A>
__device__ __forceinline__ uint32_t own_claim(const A &a, uint32_t x)    // returns the old counter
{
    return atomicAdd(own_word(a, x), 1u);
}
template <class A>
__device__ __forceinline__ uint32_t own_release(const A &a, uint32_t x)  // returns the old counter
{
    return atomicExch(own_word(a, x), 0u);
}
#define BBME_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// block (r, c) has a new estimate: its dependants R, DR, D, DL must be looked at again (idempotent byte stores)
template <class A>
__device__ __forceinline__ void mark_dependants(const A &a, uint8_t *flags, int r, int c)
{
    const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 1, 0, -1};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int rr = r + dr[d], cc = c + dc[d];
        if (rr < a.rows && cc >= 0 && cc < a.cols) {
            if constexpr (kPass1Args<A>) *at32(flags, __umul24((uint32_t)rr, (uint32_t)a.cols) + (uint32_t)cc) = 1;
            else flags[(size_t)rr * a.cols + cc] = 1;
        }
    }
}

// PASS 1'S HEAD (the three kernels below).  A pass-1 launch on a small grid lasts as long as one wave's way to its first and
// last memory trip, and one on a large grid of small blocks as long as 32 waves a SIMD take to issue theirs, so what stands in front
// of the candidates' load is the launch.  Hence: thread, block, row and column in 32 bits (the context promises every dimension
// below 2^23 and every per-pair buffer below 4 GiB, see Pass1Args; the block index is formed per group, blockIdx.x * groups + group, and
// stays below blocks + 256), one unsigned 32-bit division by `cols`; every grid, flag and image access at a 32-bit byte offset from
// the pair's base; the pair's shift on the pointers pass 1 reads and no others; what the straight path reads asked for in one
// group of scalar loads at entry (pass1_pin: it pins the VALUES -- the kernel-argument pointer stays the compiler's); the counters
// zeroed behind the evaluation, not in front of it; and the block's old value taken from the candidates' trip, where it is
// candidate 0, instead of from a load of its own behind the estimate's store.
__device__ __forceinline__ Pass1Args pass1_hot_args(const RegArgs &k, uint32_t p)
{
    Pass1Args a{};
    a.image1 = k.image1 + (size_t)p * k.s_plane; a.image2 = k.image2 + (size_t)p * k.s_plane;
    a.width = k.width; a.height = k.height; a.rows = k.rows; a.cols = k.cols;
    a.old_grid = k.old_grid + (size_t)p * k.s_old; a.old_shift = k.old_shift; a.old_cols = k.old_cols;
    a.est = k.est + (size_t)p * k.s_est;
    a.lambda_mult = k.lambda_mult;
    // (the strides are read whether or not the pointer is null: a load under the test would be a second wait)
    uint8_t *const flag_next = k.flag_next + (size_t)p * k.s_flag;
    a.flag_next = k.flag_next ? flag_next : nullptr;                              // no map: the Jacobi fast mode
    unsigned long long *const memo = k.memo + (size_t)p * k.s_memo;
    a.memo = k.memo ? memo : nullptr; a.memo_init = k.memo_init;
    a.lazy = k.lazy;
    return a;
}
// everything the straight path reads is in scalar registers from here on: the loads stand together at the kernel's entry.
// (Not in the strip form: it lives at the SGPR limit, the pinned values were spilled at once and its first load moved back;
// without the pin the compiler groups its loads by itself.)
template <bool MEMO = false>
__device__ __forceinline__ void pass1_pin(const Pass1Args &a)
{
    asm volatile("" :: "s"(a.image1), "s"(a.image2), "s"(a.width), "s"(a.height), "s"(a.rows), "s"(a.cols), "s"(a.old_grid),
                 "s"(a.old_shift), "s"(a.old_cols), "s"(a.est), "s"(a.lambda_mult), "s"(a.flag_next));
    if constexpr (MEMO) asm volatile("" :: "s"(a.memo), "s"(a.memo_init));
}
// the solver's counters (nothing else touches them before this sweep's solver launch): the launch's first 16 threads, [5] stays
__device__ __forceinline__ void pass1_zero_counters(const RegArgs &k)
{
    if (blockIdx.x == 0 && threadIdx.x < 16 && threadIdx.x != 5) k.counters[(size_t)blockIdx.y * 64u + threadIdx.x] = 0;
}

template <int BS>
__global__ __launch_bounds__(256) void k_reg_pass1(const RegArgs args)
{
    constexpr int LPB = RegCfg<BS>::LPB;
    __builtin_amdgcn_s_setprio(2);                 // latency-bound: ahead of a speculative search sharing the SIMD
    const Pass1Args a = pass1_hot_args(args, blockIdx.y);
    pass1_pin(a);
    const uint32_t g = blockIdx.x * (256u / LPB) + threadIdx.x / LPB;
    const int sub = (int)(threadIdx.x % LPB);
    if (g >= (uint32_t)a.rows * (uint32_t)a.cols) {  // whole groups drop out together (LPB | 256)
        pass1_zero_counters(args);                 // (a grid of fewer than 16 blocks)
        return;
    }
    const int r = (int)(g / (uint32_t)a.cols), c = (int)(g - (uint32_t)r * (uint32_t)a.cols);
    mv_t res, old;
    if (r >= 1 && r + 1 < a.rows && c >= 1 && c + 1 < a.cols) {
        // away from the border all nine candidates exist and come from the old grid: three 12-byte loads (or, when the old
        // grid is the parent grid, the 2 x 2 parent cells around the block: two 8-byte loads) instead of nine
        mv_t cand[9];
        if (a.old_shift == 0) {
            struct __attribute__((packed, aligned(1))) tri_t { uint32_t v[3]; };
            const uint32_t pitch = (uint32_t)a.old_cols << 2, o = (__umul24((uint32_t)(r - 1), (uint32_t)a.old_cols) + (uint32_t)(c - 1)) << 2;
            tri_t row[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) row[i] = *reinterpret_cast<const tri_t *>(at32(a.old_grid, o + (uint32_t)i * pitch));
#pragma unroll
            for (int k = 0; k < 9; ++k) cand[k] = row[1 + kNbRow[k]].v[1 + kNbCol[k]];
        } else {
            struct __attribute__((packed, aligned(1))) duo_t { uint32_t v[2]; };
            const int pr0 = (r - 1) >> 1, pc0 = (c - 1) >> 1;                // (r + 1) >> 1 == pr0 + 1, (c + 1) >> 1 == pc0 + 1
            const uint32_t o = (__umul24((uint32_t)pr0, (uint32_t)a.old_cols) + (uint32_t)pc0) << 2;
            const duo_t w0 = *reinterpret_cast<const duo_t *>(at32(a.old_grid, o));
            const duo_t w1 = *reinterpret_cast<const duo_t *>(at32(a.old_grid, o + ((uint32_t)a.old_cols << 2)));
            const int ro = r & 1, co = c & 1;                                 // odd row: rows r-1, r in parent row pr0, r+1 in pr0 + 1
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                // neighbour row r + d lies in parent row pr0 + ((r + d) >> 1) - pr0: d = -1 -> 0, d = +1 -> 1, d = 0 -> 1 - (r & 1)
                const int pr = kNbRow[k] < 0 ? 0 : kNbRow[k] > 0 ? 1 : 1 - ro;
                const int pc = kNbCol[k] < 0 ? 0 : kNbCol[k] > 0 ? 1 : 1 - co;
                const mv_t lo = pc ? w0.v[1] : w0.v[0], hi = pc ? w1.v[1] : w1.v[0];
                cand[k] = pr ? hi : lo;
            }
        }
        old = cand[0];
        bool uniform = true;
#pragma unroll
        for (int k = 1; k < 9; ++k) uniform &= cand[k] == cand[0];
        res = uniform ? cand[0] : score_block<BS, true>(a, cand, 0x1ffu, c * BS, r * BS, sub);
    } else {
        res = eval_block<BS, false, true>(a, r, c, sub, 0u, &old);            // (candidate 0 is the block's old value)
    }
    if (sub == 0) {
        *at32(a.est, g << 2) = res;
        // the blocks that read this one as an already-updated input assumed the old value
        if (a.flag_next && res != old) mark_dependants(a, a.flag_next, r, c);     // no map: the Jacobi fast mode stops here
    }
    pass1_zero_counters(args);
}

// Pass 1 on the large grids of small blocks (b = 2, 4; hundreds of thousands to millions of blocks), r04.  Measured with the image
// path switched off, 70 % of k_reg_pass1 there is the test "are the nine candidates equal?" -- three 12-byte loads, eight compares and a
// 4-byte store per block, one block per lane (b = 2) or per four lanes (b = 4) -- and the rest is the evaluations of the few blocks that
// fail it, run by whole waves for a handful of live lanes.  Here a lane tests a STRIP of four blocks of a row from a 3 x 6 window (six
// loads for four blocks instead of twelve, one 16-byte store), and the blocks that need their images are not evaluated where they
// were found: the wave lists them (ballots, no barrier) and works the list off densely, 64 / LPB blocks per pass -- blocks that need
// their images come in clusters (motion boundaries), so one dense pass replaces what were several sparse ones.
template <int BS>
__global__ __launch_bounds__(256) void k_reg_pass1_strip(const RegArgs args)
{
    constexpr int LPB = RegCfg<BS>::LPB;                       // 1 (b = 2) or 4 (b = 4): lanes per block on the image path
    static_assert(BS == 2 || BS == 4, "small blocks");
    __shared__ uint32_t s_list[4][256];                       // per wave: the blocks of its 64 strips that need their images
    __builtin_amdgcn_s_setprio(2);
    const Pass1Args a = pass1_hot_args(args, blockIdx.y);
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t *list = s_list[threadIdx.x >> 6];
    const uint32_t spr = (uint32_t)a.cols >> 2;                // strips per row (the host takes this form only when 4 | cols)
    const uint32_t nstrips = spr * (uint32_t)a.rows;
    const bool valid = t < nstrips;
    const uint32_t ts = valid ? t : nstrips - 1;
    const int r = (int)(ts / spr), c0 = (int)(ts - (uint32_t)r * spr) * 4;
    const uint32_t cell0 = (uint32_t)r * (uint32_t)a.cols + (uint32_t)c0;
    uint32_t need = valid ? 0xfu : 0u;                         // bit j: block c0 + j takes the image path (border strips: all four)
    if (valid && r >= 1 && r + 1 < a.rows && c0 >= 4 && c0 + 4 < a.cols) {
        mv_t own[4];
        need = 0;
        if (a.old_shift == 0) {
            struct __attribute__((packed, aligned(1))) hex_t { uint32_t v[6]; };
            const uint32_t pitch = (uint32_t)a.old_cols << 2, o = (__umul24((uint32_t)(r - 1), (uint32_t)a.old_cols) + (uint32_t)(c0 - 1)) << 2;
            hex_t row[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) row[i] = *reinterpret_cast<const hex_t *>(at32(a.old_grid, o + (uint32_t)i * pitch));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                own[j] = row[1].v[j + 1];
                bool uniform = true;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int d = 0; d < 3; ++d) uniform &= row[i].v[j + d] == own[j];
                if (!uniform) need |= 1u << j;
            }
        } else {
            // the old grid is the parent grid: columns c0 - 1 .. c0 + 4 lie in parent columns c0 / 2 - 1 .. c0 / 2 + 2, rows r - 1 .. r + 1
            // in parent rows (r - 1) >> 1 and that + 1
            struct __attribute__((packed, aligned(1))) quad_t { uint32_t v[4]; };
            const int pr0 = (r - 1) >> 1, pc0 = (c0 >> 1) - 1;
            const uint32_t o = (__umul24((uint32_t)pr0, (uint32_t)a.old_cols) + (uint32_t)pc0) << 2;
            const quad_t w0 = *reinterpret_cast<const quad_t *>(at32(a.old_grid, o));
            const quad_t w1 = *reinterpret_cast<const quad_t *>(at32(a.old_grid, o + ((uint32_t)a.old_cols << 2)));
            const bool mid_hi = !(r & 1);                                     // row r itself: parent row pr0 (r odd) or pr0 + 1 (r even)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // column c0 + k (c0 a multiple of 4) lies in parent column c0 / 2 + (k >> 1) = pc0 + 1 + (k >> 1); k = -1: pc0
                own[j] = mid_hi ? w1.v[(j >> 1) + 1] : w0.v[(j >> 1) + 1];
                bool uniform = true;
#pragma unroll
                for (int dc = -1; dc <= 1; ++dc) {
                    const int k = j + dc, pc = k < 0 ? 0 : (k >> 1) + 1;
                    uniform &= w0.v[pc] == own[j];                            // row r - 1: always parent row pr0
                    uniform &= w1.v[pc] == own[j];                            // row r + 1: always parent row pr0 + 1
                    // (row r is one of the two)
                }
                if (!uniform) need |= 1u << j;
            }
        }
        // nine equal candidates: the block keeps its vector (:648-660); the others get theirs below, this is their old value meanwhile
        struct __attribute__((aligned(16))) out_t { uint32_t v[4]; };
        *reinterpret_cast<out_t *>(at32(a.est, cell0 << 2)) = out_t{{own[0], own[1], own[2], own[3]}};
    }
    pass1_zero_counters(args);                                // as k_reg_pass1: behind the strip test
    if (a.lazy) {
        // a relaxation launch follows: it evaluates flagged blocks tile by tile with every lane busy, so the blocks that need their
        // images are handed to it as they are -- old value as the estimate, flag set.  The field the sweep converges to is the same:
        // every block that is not flagged has nine equal candidates (its estimate is final unless a neighbour changes, which marks it),
        // every other block is evaluated at least once.
        if (valid && need) {
            const bool interior = need != 0xfu || (r >= 1 && r + 1 < a.rows && c0 >= 4 && c0 + 4 < a.cols);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((need >> j) & 1u) {
                    if (!interior)
                        *at32(a.est, (cell0 + j) << 2) =
                            *at32(a.old_grid, (__umul24((uint32_t)(r >> a.old_shift), (uint32_t)a.old_cols) + (uint32_t)((c0 + j) >> a.old_shift)) << 2);
                    *at32(a.flag_next, cell0 + j) = 1;
                }
        }
        return;
    }
    // the wave's list of blocks for the image path: ranks from four ballots
    uint32_t total = 0;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long m = __ballot((need >> j) & 1u);
        if ((need >> j) & 1u) list[total + (uint32_t)__popcll(m & lt_mask)] = cell0 + (uint32_t)j;
        total += (uint32_t)__popcll(m);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the wave's own LDS writes, before its own reads
    constexpr int PER = 64 / LPB;                             // blocks per pass
    const int sub = lane & (LPB - 1);
    for (uint32_t base = 0; base < total; base += PER) {      // wave-uniform
        const uint32_t idx = base + (uint32_t)(lane / LPB);
        if (idx < total) {                                     // whole groups
            const uint32_t cell = list[idx];
            const int rr = (int)(cell / (uint32_t)a.cols), cc = (int)(cell - (uint32_t)rr * (uint32_t)a.cols);
            mv_t old;                                          // candidate 0 of the evaluation
            const mv_t res = eval_block<BS, false, true>(a, rr, cc, sub, 0u, &old);
            if (sub == 0) {
                *at32(a.est, cell << 2) = res;
                if (a.flag_next && res != old) mark_dependants(a, a.flag_next, rr, cc);
            }
        }
    }
}

// Relaxation over the marked blocks, the whole chip at once, before the solver.  The grid is cut into tiles of
// T x T blocks, one workgroup each.  A workgroup keeps the estimates of its tile (+ the ring of neighbours it reads:
// one column left and right, one row above) in LDS, evaluates the marked blocks of the tile, and when a block
// changes, queues its dependants R, DR, D, DL: those inside the tile for the workgroup's next LOCAL round (same
// launch, a barrier apart), those outside in the byte map flag_next for the next launch.  After `local_rounds`
// rounds whatever is still queued goes to flag_next too.  Plain loads and stores.  An estimate outside the tile is
// read once, at the start; if its owner changes it during this launch, that owner marks the reader in flag_next.
// Pass 1 in the chain form (16 lanes per block, lane k = candidate k), for grids too small to fill the chip: there the launch
// lasts as long as one wave's instruction stream does, and the chain form's is a third as long as eval_block's.
template <int BS, bool MEMO = false>
__global__ __launch_bounds__(256) void k_reg_pass1_lanes(const RegArgs args)
{
    __builtin_amdgcn_s_setprio(2);
    const Pass1Args a = pass1_hot_args(args, blockIdx.y);
    pass1_pin<MEMO>(a);
    const uint32_t g = blockIdx.x * 16u + (threadIdx.x >> 4);
    const int k16 = (int)(threadIdx.x & 15u);
    if (g >= (uint32_t)a.rows * (uint32_t)a.cols) return;     // whole groups drop out together (never the launch's first: it zeroes the counters)
    const int r = (int)(g / (uint32_t)a.cols), c = (int)(g - (uint32_t)r * (uint32_t)a.cols);
    mv_t old;                                                  // candidate 0 as the group's first lane loaded it
    const mv_t res = eval_block_lanes<BS, false, MEMO>(a, r, c, k16, 0u, nullptr, nullptr, nullptr, &old);
    if (k16 == 0) {
        *at32(a.est, g << 2) = res;
        if (a.flag_next && res != old) mark_dependants(a, a.flag_next, r, c);
    }
    pass1_zero_counters(args);                                // as k_reg_pass1
}

// This is asynchronous fixed-point iteration: any number of rounds or launches, followed by k_reg_solve, ends at
// the same (unique) field.  It takes the first, heavy generations of a sweep -- thousands of stale blocks at once --
// away from the solver, whose coherent traffic and memory-side atomics queue up under that load.
template <int BS> struct RegIter {
    static constexpr int T = BS <= 4 ? 32 : (BS == 8 ? 16 : 8);       // tile edge in blocks
};
template <int BS>
__global__ __launch_bounds__(256) void k_reg_iter(RegArgs a)
{
    constexpr int LPB = RegCfg<BS>::LPB;
    constexpr int T = RegIter<BS>::T;
    constexpr int TP = T + 2;                                 // pitch of the LDS tile: halo column left and right
    __shared__ mv_t tile[(T + 1) * TP];                       // row 0 = halo row above
    __shared__ uint32_t list[2][T * T];
    __shared__ uint32_t n_list[2];
    __shared__ uint32_t queued[(T * T + 31) / 32];
    __builtin_amdgcn_s_setprio(2);
    shift_pair(a, blockIdx.y);
    const int t = threadIdx.x;
    const int tiles_x = (a.cols + T - 1) / T;
    const int r0 = ((int)blockIdx.x / tiles_x) * T, c0 = ((int)blockIdx.x % tiles_x) * T;
    if (t < 2) n_list[t] = 0;
    for (int i = t; i < (T + 1) * TP; i += 256) {
        const int rr = r0 - 1 + i / TP, cc = c0 - 1 + i % TP;
        tile[i] = (rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols) ? a.est[(size_t)rr * a.cols + cc] : 0u;
    }
    __syncthreads();
    for (int i = t; i < T * T; i += 256) {                    // consume the tile's marks
        const int lr = i / T, lc = i % T, rr = r0 + lr, cc = c0 + lc;
        if (rr < a.rows && cc < a.cols) {
            uint8_t *f = a.flag_cur + (size_t)rr * a.cols + cc;
            if (*f) { *f = 0; list[0][atomicAdd(&n_list[0], 1u)] = (uint32_t)(lr * T + lc); }
        }
    }
    const int sub = t % LPB;
    int cur = 0, heavy = 0;
    // a block changed: its dependants go on the tile's next list (once) or, outside the tile, into the byte map
    auto propagate = [&](int lr, int lc, int r, int c, bool last) {
        const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 1, 0, -1};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int lr2 = lr + dr[d], lc2 = lc + dc[d], rr = r + dr[d], cc = c + dc[d];
            if (rr >= a.rows || cc < 0 || cc >= a.cols) continue;
            if (!last && lr2 < T && lc2 >= 0 && lc2 < T) {
                const uint32_t bit = (uint32_t)(lr2 * T + lc2);
                if (!(atomicOr(&queued[bit >> 5], 1u << (bit & 31u)) & (1u << (bit & 31u))))
                    list[cur ^ 1][atomicAdd(&n_list[cur ^ 1], 1u)] = bit;
            } else {
                a.flag_next[(size_t)rr * a.cols + cc] = 1;
            }
        }
    };
    for (int round = 0;; ++round) {
        __syncthreads();
        const uint32_t cnt = n_list[cur];
        if (cnt == 0) break;                                  // uniform
        // rounds with many blocks keep one CU busy while the chip waits: only `local_rounds` of them; rounds with
        // up to 16 blocks are a chain being walked, which is cheapest right here (estimates in LDS, no atomics)
        const bool chain = cnt <= 16u;
        if (!chain) ++heavy;
        const bool last = heavy >= a.local_rounds || round + 1 >= 96;
        __syncthreads();
        if (t == 0) n_list[cur ^ 1] = 0;
        for (int i = t; i < (T * T + 31) / 32; i += 256) queued[i] = 0;
        __syncthreads();
        if (chain) {
            // 16 lanes per block, lane k = candidate k (see eval_block_lanes)
            const int g = t >> 4, k16 = t & 15;
            if ((uint32_t)g < cnt) {
                const int lr = (int)(list[cur][g] / T), lc = (int)(list[cur][g] % T);
                const int r = r0 + lr, c = c0 + lc;
                const int k = k16 < 9 ? k16 : 0;
                const int rr = r + kNbRow[k], cc = c + kNbCol[k];
                const bool present = k16 < 9 && rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols;
                const int rs = min(max(rr, 0), a.rows - 1), cs = min(max(cc, 0), a.cols - 1);
                mv_t mv;
                if ((BBME_NEW_MASK >> k) & 1u) mv = tile[(lr + kNbRow[k] + 1) * TP + lc + kNbCol[k] + 1];
                else mv = a.old_grid[(size_t)(rs >> a.old_shift) * a.old_cols + (cs >> a.old_shift)];
                const mv_t res = lanes_score<BS>(a, r, c, k16, present, mv);
                if (k16 == 0 && res != tile[(lr + 1) * TP + lc + 1]) {
                    tile[(lr + 1) * TP + lc + 1] = res;
                    a.est[(size_t)r * a.cols + c] = res;
                    propagate(lr, lc, r, c, last);
                }
            }
        } else {
            for (uint32_t idx = t / LPB; idx < cnt; idx += 256 / LPB) {
                const int lr = (int)(list[cur][idx] / T), lc = (int)(list[cur][idx] % T);
                const int r = r0 + lr, c = c0 + lc;
                mv_t cand[9];
                uint32_t present = 0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int rr = r + kNbRow[k], cc = c + kNbCol[k];
                    if (rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols) present |= 1u << k;
                    const int rs = min(max(rr, 0), a.rows - 1), cs = min(max(cc, 0), a.cols - 1);
                    if ((BBME_NEW_MASK >> k) & 1u) cand[k] = tile[(lr + kNbRow[k] + 1) * TP + lc + kNbCol[k] + 1];
                    else cand[k] = a.old_grid[(size_t)(rs >> a.old_shift) * a.old_cols + (cs >> a.old_shift)];
                }
                bool uniform = true;
#pragma unroll
                for (int k = 1; k < 9; ++k) uniform &= !((present >> k) & 1u) || cand[k] == cand[0];
                mv_t res = cand[0];
                if (!uniform) res = score_block<BS, false>(a, cand, present, c * BS, r * BS, sub);
                if (sub == 0 && res != tile[(lr + 1) * TP + lc + 1]) {
                    tile[(lr + 1) * TP + lc + 1] = res;
                    a.est[(size_t)r * a.cols + c] = res;
                    propagate(lr, lc, r, c, last);
                }
            }
        }
        if (last) break;                                      // uniform
        cur ^= 1;
    }
}

// One work-list pass of the safety net (see k_reg_solve's epilogue): `nthreads` threads of one
// workgroup, lists in global memory that cannot overflow (a block is on a list at most once).
template <int BS>
__device__ __forceinline__ void drain_lists(const RegArgs &a, int t, int nthreads)
{
    constexpr int LPB = 16;                      // lane k of a group = candidate k (eval_block_lanes)
    const int group = t / LPB, ngroups = nthreads / LPB, sub = t % LPB;
    // pass p reads list[p&1] (length counters[p%3]), appends to list[(p+1)&1] (counters[(p+1)%3])
    // and zeroes counters[(p+2)%3]; the overflow list of the solver is list0 / counters[1] -> p = 4.
    int p = 4;
    // a change can only travel along the raster dependency chain, whose length is below
    // 2*rows + cols; the cap is an exit every wave reaches even if that reasoning were wrong
    const int p_max = p + 2 * a.rows + a.cols + 16;
    for (;;) {
        const uint32_t n = __hip_atomic_load(&a.counters[p % 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == 0) break;
        if (p > p_max) { if (t == 0) a.counters[5] = 1; break; }      // reported by bbme_last_sweep_passes
        __syncthreads();                              // everyone has read n before it can be reused
        if (t == 0) {
            __hip_atomic_store(&a.counters[(p + 2) % 3], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.counters[3] += 1;
        }
        const uint32_t *lcur = (p & 1) ? a.list1 : a.list0;
        uint32_t *lnext = (p & 1) ? a.list0 : a.list1;
        uint32_t *cnext = &a.counters[(p + 1) % 3];
        for (uint32_t idx = group; idx < n; idx += ngroups) {
            const uint32_t x = __hip_atomic_load(&lcur[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int r = (int)(x / a.cols), c = (int)(x % a.cols);
            if (sub == 0) own_release(a, x);                                  // the list owned it
            BBME_DRAIN();
            const mv_t res = eval_block_lanes<BS, true>(a, r, c, sub, BBME_NEW_MASK);
            if (sub == 0 && res != load_est<true>(a.est + x)) {
                __hip_atomic_store(a.est + x, res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                BBME_DRAIN();
                const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 1, 0, -1};
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int rr = r + dr[d], cc = c + dc[d];
                    if (rr >= a.rows || cc < 0 || cc >= a.cols) continue;
                    const uint32_t xd = (uint32_t)rr * a.cols + cc;
                    if (own_claim(a, xd) == 0)
                        __hip_atomic_store(&lnext[atomicAdd(cnext, 1u)], xd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        BBME_DRAIN();
        __syncthreads();
        ++p;
    }
}

// HOT AND COLD ARGUMENTS (k_reg_solve).  A round reads the images, the two grids, the ownership words, the memo, the geometry,
// lambda and its own switches, a scan step the flag map: those are copied once, with the pair's shift applied, into the SolverArgs
// the helpers are given (solver_hot_args) and live in scalar registers.  Everything else -- the overflow lists, the counters, the publish word, the switches of the epilogue -- is read
// from the kernel-argument segment where it is used (BBME_SOLVER_COLD): a scalar load on a path that is not a round's, instead of a
// register (or a spill slot in a VGPR lane, reloaded inside the rounds) for the whole launch.  The loads are written against the
// segment's pointer and not against the parameter: the compiler gathers a parameter's loads at the kernel's entry, these it leaves
// where they stand.  (Hiding the pointer behind an empty asm statement is no way to pin them: the statement's result counts as
// divergent, and the round loop's control flow -- head, tail, the branches -- turns into vector code.)
// THE SEGMENT'S POINTER IS TAKEN IN THE KERNEL'S OWN BODY AND HANDED DOWN (SolverKernarg): __builtin_amdgcn_kernarg_segment_ptr()
// is the segment only inside a kernel -- in a function that the inliner leaves out of line (solver_wait_idle is one) the backend
// lowers it to a null pointer, without a word.  So no helper calls the builtin: whoever needs a cold argument is given the pointer,
// which is right inlined or not.  The other condition is stated where k_reg_solve takes the pointer: the kernel's only parameter
// is the RegArgs, so the segment begins with it.
typedef const __attribute__((address_space(4))) char *SolverKernarg;
template <class T>
__device__ __forceinline__ T solver_cold_arg(SolverKernarg kp, size_t offset)
{
    return *reinterpret_cast<const __attribute__((address_space(4))) T *>(kp + offset);
}
#define BBME_SOLVER_COLD(kp, field) solver_cold_arg<decltype(RegArgs::field)>(kp, offsetof(RegArgs, field))
__device__ __forceinline__ uint32_t *solver_counters(SolverKernarg kp) { return BBME_SOLVER_COLD(kp, counters) + (size_t)blockIdx.y * 64u; }
__device__ __forceinline__ uint32_t *solver_overflow_list(SolverKernarg kp)
{
    return BBME_SOLVER_COLD(kp, list0) + (size_t)blockIdx.y * BBME_SOLVER_COLD(kp, s_list);
}

// k_reg_solve, a wave with nothing left: announce it, wait for a sibling's surplus (returns how many blocks arrived in the wave's
// mailbox) or for the last wave to fall idle (returns 0).  Kept out of line: inlined, its spin loop sits inside the solver's round loop
// as far as the register allocator is concerned and costs the rounds 30 scalar spills.
__device__ __attribute__((noinline)) uint32_t solver_wait_idle(uint32_t *mail, uint32_t *idle_mask, uint32_t *done, uint32_t wave, uint32_t wpw,
                                                               uint32_t *error_flag)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bit = 1u << wave, full = (1u << wpw) - 1u;
    uint32_t old = 0;
    if (lane == 0) old = __hip_atomic_fetch_or(idle_mask, bit, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = __builtin_amdgcn_readfirstlane(old);
    if ((old | bit) == full) {
        if (lane == 0) __hip_atomic_store(done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        return 0;
    }
    for (uint32_t spin = 0;; ++spin) {
        const uint32_t got = __builtin_amdgcn_readfirstlane(__hip_atomic_load(mail, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (got) return got;
        if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP))) return 0;
        if (spin > (1u << 23)) {                                      // (~1 s) an exit every wave reaches: reported, and everyone leaves
            if (lane == 0) { *error_flag = 1; __hip_atomic_store(done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
            return 0;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Asynchronous solver.  Every wave owns a private LDS queue.  It scans its share of the dirty flags
// (blocks one of whose already-updated inputs was changed by pass 1 or by the last relaxation step),
// claims and queues the marked blocks, and whatever its own changes make stale it queues locally too
// and evaluates itself, round after round, without any grid-wide step: fixed-point iteration
// tolerates any evaluation order.  A wave whose queue is empty and which has scanned its share simply
// exits.  If a local queue is full the surplus goes to a global overflow list; the workgroup that
// finishes last (ticket counter) drains that list on its own, so the launch always ends at the fixed
// point.
//
// The scan: the flag map is cut into SEGMENTS of 16 flags (one 16-byte load).  XCD j owns the j-th band
// of the raster (workgroups go round-robin to the 8 XCDs, each with its own L2: the estimates and
// ownership words of a band are then read, written and claimed through one L2); inside a band segment
// s belongs to wave s mod W of that XCD, so that a cluster of stale blocks is spread over many waves
// instead of queueing up behind one, and a wave looks at 64 of its segments -- 1024 flags -- per memory
// trip: a sweep that left nothing stale costs two trips at 2 M blocks, not 127.
//
// FLOOD (k_reg_solve<.., true>; never part of the other instantiations' instruction stream): the chain rounds speculate along floods.
// Nine of ten changes that a neighbour's change triggers adopt that neighbour's new value, so a block that has just taken
// the value of one of its updated inputs L, UL, U, UR claims, besides its four dependants, up to RegArgs::flood further
// blocks along that direction and queues them, marked, right behind the dependant that leads them.  A marked entry that
// is popped into the 16-lane group behind its predecessor is evaluated in the SAME round, with the predecessor's estimate
// replaced in registers by the value the flood is expected to leave there; the evaluation counts if the predecessor's
// evaluation counted and gave exactly that value, and then the predecessor does not claim the block again.  The block
// was claimed before the round, so its other inputs were loaded after its claim, and the estimate it was given is the one
// the same wave stores before any of the round's claims and releases go out: a kept evaluation is an ordinary owned
// evaluation, and "work-list state" holds as it stands.  Any other outcome leaves the entry where it was, owned and queued,
// for an ordinary evaluation.  Marked entries exist in the LDS queues and mailboxes only; the overflow list holds plain indices.
constexpr uint32_t kFloodEntry = 0x80000000u;   // queue entry: claimed on speculation, behind its predecessor along a flood

__device__ __forceinline__ SolverArgs solver_hot_args(const RegArgs &k, uint32_t p)
{
    SolverArgs a{};
    a.image1 = k.image1 + (size_t)p * k.s_plane; a.image2 = k.image2 + (size_t)p * k.s_plane;
    a.width = k.width; a.height = k.height; a.rows = k.rows; a.cols = k.cols;
    a.old_grid = k.old_grid + (size_t)p * k.s_old; a.old_shift = k.old_shift; a.old_cols = k.old_cols;
    a.est = k.est + (size_t)p * k.s_est;
    a.lambda_mult = k.lambda_mult;
    a.own = k.own + (size_t)p * k.s_own; a.own_pitch = k.own_pitch;
    a.flag_cur = k.flag_cur + (size_t)p * k.s_flag;                 // (the scan steps: never null in a solver launch)
    a.wide_threshold = k.wide_threshold; a.round_cap = k.round_cap; a.share = k.share;
    a.memo = k.memo ? k.memo + (size_t)p * k.s_memo : nullptr; a.memo_init = k.memo_init; a.memo_forward = k.memo_forward;
    return a;
}
// the epilogue's safety net runs on the whole set (drain_lists): the hot ones and the lists and counters
__device__ __forceinline__ RegArgs solver_all_args(const SolverArgs &hot, SolverKernarg kp)
{
    RegArgs a = hot;
    const uint32_t s_list = BBME_SOLVER_COLD(kp, s_list);
    a.list0 = BBME_SOLVER_COLD(kp, list0) + (size_t)blockIdx.y * s_list; a.list1 = BBME_SOLVER_COLD(kp, list1) + (size_t)blockIdx.y * s_list;
    a.counters = solver_counters(kp);
    return a;
}

template <int BS, int SEG = 16, bool MEMO = false, bool FLOOD = false>
__global__ __launch_bounds__(256) void k_reg_solve(const RegArgs args)
{
    static_assert(SEG == 16 || SEG == 4, "flags per scan segment");
    // two forms of a round: WIDE (eval_block: LPBW lanes per block, 64/LPBW blocks per round) when
    // the queue is long and throughput counts, LANES (eval_block_lanes: 16 lanes per block, lane k =
    // candidate k, 4 blocks per round) when it is short and the wave is walking a chain
    constexpr int LPBW = RegCfg<BS>::LPB;
    constexpr int NBW = 64 / LPBW;
    constexpr int NBL = 4;
    constexpr uint32_t QCAP = 1024;
    constexpr uint32_t MAILCAP = 64;
    // Handing surplus blocks to idle sibling waves (below).  (A compile-time switch for experiments: with the rounds in a flat loop the
    // code's mere presence cost the b = 8 launches 1-3 us each; with the rounds in an inner loop of their own it costs nothing.)
    constexpr bool SHARE = true;
    // (four waves, 17.4 KB of LDS: eight waves -- 34 KB -- shared no better, and a workgroup of that size no longer fits the holes that
    // the 20 KB workgroups of a speculative search leave: measured, the step lost its whole overlap)
    constexpr int MAXW = 4;                                // most waves of a workgroup
    __shared__ uint32_t qmem[MAXW][QCAP];
    __shared__ uint32_t s_mail[MAXW][MAILCAP + 1];            // [w][0]: blocks handed to wave w, [w][1..]: their indices
    __shared__ uint32_t s_idle, s_done;                    // bit w: wave w has nothing to do and may be handed blocks; all waves idle
    __shared__ uint32_t s_ticket;
    __builtin_amdgcn_s_setprio(2);
    // (the segment begins with the kernel's first parameter, and the RegArgs is its only one)
    const SolverKernarg kp = (SolverKernarg)__builtin_amdgcn_kernarg_segment_ptr();
    const SolverArgs a = solver_hot_args(args, blockIdx.y);   // what the rounds read; the rest: BBME_SOLVER_COLD where it is used
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform, and the compiler is told so: it steers branches)
    uint32_t *q = qmem[wave];
    const uint32_t nblocks = (uint32_t)a.rows * a.cols;
    const uint32_t xcd = blockIdx.x & 7u;                  // the launch has a multiple of 8 workgroups
    const uint32_t wpw = blockDim.x >> 6;                  // waves per workgroup (1, 2 or 4)
    const uint32_t wx = (blockIdx.x >> 3) * wpw + wave, Wx = (gridDim.x >> 3) * wpw;
    const uint32_t nseg = (nblocks + (uint32_t)SEG - 1u) / (uint32_t)SEG, band = (nseg + 7u) / 8u;
    const uint32_t seg_begin = min(xcd * band, nseg), seg_end = min(seg_begin + band, nseg);
    // The first scan step's flags are asked for before anything else: the mailboxes with their barrier, the lanes' geometry and the
    // rest of the set-up below run while that trip is under way (most launches of a pyramid find nothing in it, and it is all they do)
    auto load_flags = [&](uint32_t sg) {
        uint4 f = make_uint4(0, 0, 0, 0);
        const uint8_t *fp = a.flag_cur + (size_t)sg * SEG;                                 // the map is padded to whole 16-flag segments
        if (sg < seg_end) {
            if constexpr (SEG == 16) f = *reinterpret_cast<const uint4 *>(fp);
            else f.x = *reinterpret_cast<const uint32_t *>(fp);
        }
        return f;
    };
    uint4 f_first = make_uint4(0, 0, 0, 0);
    if (seg_begin + wx < seg_end) f_first = load_flags(seg_begin + (uint32_t)lane * Wx + wx);
    if (SHARE && a.share && blockDim.x > 64) {             // (uniform over the launch)
        if (threadIdx.x < MAXW) s_mail[threadIdx.x][0] = 0;
        if (threadIdx.x == 0) { s_idle = 0; s_done = 0; }
        __syncthreads();
    }
    auto est_at = [&](uint32_t x) { return reinterpret_cast<mv_t *>(reinterpret_cast<char *>(a.est) + (x << 2)); };   // (32-bit offset, scalar base)
    uint32_t head = 0, tail = 0;                  // wave-uniform, free-running
    uint32_t evaluated = 0, rounds = 0, backlog = 0;       // backlog: rounds that left queued blocks waiting
#ifdef BBME_PHASE_PROFILE
    PhaseProf prof_s = {};
    PhaseProf *prof = nullptr;
#else
    PhaseProf *prof = nullptr;
#endif
    // every round either empties part of the queue or follows a real change; the cap is only an
    // exit that every wave reaches should that reasoning ever be wrong (reported via counters[5])
    const uint32_t round_cap = a.round_cap;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    // enqueue `flag`ged lanes' value v on the wave's queue (or the overflow list when full)
    auto enqueue = [&](bool flag, uint32_t v) {
        const unsigned long long m = __ballot(flag);
        const uint32_t total = (uint32_t)__popcll(m);
        if (total == 0) return;
        if (tail - head + total <= QCAP) {
            if (flag) q[(tail + (uint32_t)__popcll(m & lt_mask)) % QCAP] = v;
            tail = __builtin_amdgcn_readfirstlane(tail + total);
        } else if (flag) {                                  // stays QUEUED; drained in the epilogue
            if constexpr (FLOOD) v &= ~kFloodEntry;
            uint32_t *ovf_list = solver_overflow_list(kp), *ovf_count = solver_counters(kp) + 1;
            __hip_atomic_store(&ovf_list[atomicAdd(ovf_count, 1u)], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    // FLOOD: blocks a flood may claim ahead of itself -- a round has four groups, the dependant that leads them takes one; the
    // direction is told from the distance of two entries, which needs a grid at least four blocks wide
    const uint32_t flood_depth = FLOOD && a.cols >= 4 ? min((uint32_t)args.flood, (uint32_t)(NBL - 1)) : 0u;
    uint32_t kept = 0;                                     // speculative evaluations that counted (bbme_sweep_stats [15])

    const LaneGeom lgeom = lanes_geometry(a, lane & 15, BBME_NEW_MASK);      // chain form: lane k of a group = candidate k
    MemoStats mstats;

    // Outer loop: with the queue empty, a scan step, or -- the scan finished -- a wait for a sibling's surplus; then rounds until the
    // queue is empty again (an inner loop of their own: measured 1-3 us per launch ahead of one flat loop at b = 8).
    uint32_t k = 0;
    for (;;) {
        if (head == tail) {
            if (seg_begin + k * 64u * Wx + wx < seg_end) {
                const uint32_t sg = seg_begin + (k * 64u + (uint32_t)lane) * Wx + wx;
                // SEG = 4 on small grids: a cluster of stale blocks in a row is dealt to four times as many waves
                const uint4 f = k == 0 ? f_first : load_flags(sg);
                uint8_t *fp = a.flag_cur + (size_t)sg * SEG;
                ++k;
                const bool any = (f.x | f.y | f.z | f.w) != 0;
                if (__ballot(any)) {
                    if (any) {
                        if constexpr (SEG == 16) *reinterpret_cast<uint4 *>(fp) = make_uint4(0, 0, 0, 0);
                        else *reinterpret_cast<uint32_t *>(fp) = 0u;
                    }
                    const uint32_t fw[4] = {f.x, f.y, f.z, f.w};
                    // every claim of the step in flight at once (one memory trip), then the queue
                    uint32_t was[SEG];
#pragma unroll
                    for (int j = 0; j < SEG; ++j) {
                        was[j] = 1;
                        if ((fw[j >> 2] >> (8 * (j & 3))) & 0xffu) was[j] = own_claim(a, sg * (uint32_t)SEG + (uint32_t)j);
                    }
#pragma unroll
                    for (int j = 0; j < SEG; ++j) enqueue(was[j] == 0, sg * (uint32_t)SEG + (uint32_t)j);
                }
                continue;
            }
            // Nothing left of its own.  Alone in the workgroup (or sharing off) the wave leaves; otherwise it announces itself idle
            // and waits for a sibling's surplus -- a flood's whole frontier is claimed by the wave that follows it, and the siblings
            // that scanned the quiet segments beside it would otherwise have left long ago.  The last wave to fall idle ends all.
            if (!SHARE || !a.share || wpw == 1) break;
            // (every value that steers the loop is made wave-uniform by hand: a function's result, an LDS load are divergent to the
            // compiler, and one divergent exit turns the whole loop's control flow -- head, tail, the branches -- into vector code)
            const uint32_t got = __builtin_amdgcn_readfirstlane(solver_wait_idle(&s_mail[wave][0], &s_idle, &s_done, (uint32_t)wave, wpw, solver_counters(kp) + 5));
            if (!got) break;
            // the donor cleared this wave's idle bit before it wrote the mailbox: the blocks are this wave's now (owned since claimed)
            if ((uint32_t)lane < got) q[(tail + (uint32_t)lane) % QCAP] = s_mail[wave][1 + lane];
            tail = __builtin_amdgcn_readfirstlane(tail + got);
            if (lane == 0) __hip_atomic_store(&s_mail[wave][0], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            continue;
        }
        while (head != tail) {
            if (++rounds > round_cap) { if (lane == 0) solver_counters(kp)[5] = 1; head = tail; continue; }
            const bool wide = NBW > NBL && tail - head > a.wide_threshold;   // wave-uniform
            if (__builtin_expect(SHARE && a.share && wpw > 1 && tail - head > (uint32_t)(wide ? NBW : NBL), 0)) {
                // more queued than this round takes: deal the surplus to the idle siblings (at most MAILCAP each)
                uint32_t idle = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&s_idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                uint32_t surplus = tail - head - (uint32_t)(wide ? NBW : NBL);
                while (idle && surplus) {
                    const uint32_t j = (uint32_t)__builtin_ctz(idle);
                    idle &= idle - 1u;
                    uint32_t was_idle = 0;
                    if (lane == 0) was_idle = __hip_atomic_fetch_and(&s_idle, ~(1u << j), __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
                    was_idle = __builtin_amdgcn_readfirstlane(was_idle);
                    if (!((was_idle >> j) & 1u)) continue;                    // another sibling was quicker
                    const uint32_t share = min(MAILCAP, (surplus + (uint32_t)__popc(idle) + 1u) / ((uint32_t)__popc(idle) + 2u));
                    // the NEWEST blocks go: the oldest stay in this round's reach
                    if ((uint32_t)lane < share) s_mail[j][1 + lane] = q[(tail - share + (uint32_t)lane) % QCAP];
                    tail = __builtin_amdgcn_readfirstlane(tail - share);
                    surplus -= share;
                    if (lane == 0) __hip_atomic_store(&s_mail[j][0], share, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
#ifdef BBME_PHASE_PROFILE
            prof = wide ? nullptr : &prof_s;
            if (prof) prof_s.ph[6]++;
            BBME_PHASE(prof, -1);
#endif
            if constexpr (FLOOD) {
                if (!wide) {
                    // ---- a chain round that speculates along floods (see the kernel's head) ----
                    const int g = lane >> 4, sub = lane & 15;
                    const uint32_t cnt = min((uint32_t)NBL, tail - head);
                    backlog += (tail - head > cnt) ? 1u : 0u;
                    const bool active = (uint32_t)g < cnt;
                    const uint32_t e = active ? q[(head + g) % QCAP] : 0u;    // owned since it was claimed
                    head = __builtin_amdgcn_readfirstlane(head + cnt);
                    const uint32_t x = e & ~kFloodEntry;
                    const int r = (int)(x / a.cols), c = (int)(x % a.cols);
                    const uint32_t cols = (uint32_t)a.cols;
                    const bool leader = active && sub == 0;
                    // the candidates' trip, as eval_block_lanes: asked for first -- no load needs the links, which are worked out under it
                    const LaneCand lc = lanes_candidate(a, lgeom, r, c);
                    uint32_t slot = 0;
                    uint2 memo = make_uint2(kMemoNoMv, 0u);
                    mv_t prev = 0, mv = 0;
                    if (active) {
                        if constexpr (MEMO) {
                            slot = (x << kMemoSlotShift) | (uint32_t)(sub < 9 ? sub : 0);
                            if (!a.memo_init) memo = memo_load<true>(a, slot);
                        }
                        if (leader) prev = load_est<true>(est_at(x));
                        mv = load_est<true>(lc.src);
                    }
                    // links: a marked entry whose predecessor along R, DR, D or DL sits in the group before it reads that block as
                    // its candidate kd = L, UL, U or UR (every steering value wave-uniform: one readlane per group)
                    const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)e, 0), e1 = (uint32_t)__builtin_amdgcn_readlane((int)e, 16),
                                   e2 = (uint32_t)__builtin_amdgcn_readlane((int)e, 32);
                    const uint32_t dist = x - ((g == 1 ? e0 : g == 2 ? e1 : e2) & ~kFloodEntry);
                    uint32_t kd = 0;
                    if (active && g >= 1 && (e & kFloodEntry))
                        kd = (dist == 1u && c >= 1) ? 1u : (dist == cols + 1u && c >= 1) ? 4u : dist == cols ? 6u
                             : (dist == cols - 1u && (uint32_t)c + 1u < cols) ? 5u : 0u;
                    const uint32_t k1 = (uint32_t)__builtin_amdgcn_readlane((int)kd, 16), k2 = (uint32_t)__builtin_amdgcn_readlane((int)kd, 32),
                                   k3 = (uint32_t)__builtin_amdgcn_readlane((int)kd, 48);
                    BBME_PHASE(prof, 0);
                    // A run of linked groups expects the value that its first, unlinked group read from the flood's direction:
                    // h1, h2, h3 = what group 1, 2, 3 is given in place of its predecessor's estimate
                    const uint32_t v0 = (uint32_t)__builtin_amdgcn_readlane((int)mv, (int)k1), v1 = (uint32_t)__builtin_amdgcn_readlane((int)mv, (int)(16u + k2)),
                                   v2 = (uint32_t)__builtin_amdgcn_readlane((int)mv, (int)(32u + k3));
                    const uint32_t h1 = v0, h2 = k1 ? h1 : v1, h3 = k2 ? h2 : v2;
                    if (kd != 0u && (uint32_t)sub == kd) mv = g == 1 ? h1 : g == 2 ? h2 : h3;
                    mv_t res = 0;
                    if (active) {
                        const mv_t own = dpp_row<0x150>(mv);
                        if (!__ballot(lc.present && mv != own)) {
                            if constexpr (MEMO) {
                                if (a.memo_init && sub < 9) memo_store(a, slot, kMemoNoMv, 0u);
                            }
                            res = own;
                        } else {
                            res = lanes_score<BS, MEMO, true>(a, r, c, sub, lc.present, mv, prof, memo, slot, MEMO ? &mstats : nullptr);
                        }
                    }
                    // an evaluation counts if the group is not linked, or if its predecessor's counted and gave what was expected
                    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)res, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)res, 16),
                                   r2 = (uint32_t)__builtin_amdgcn_readlane((int)res, 32);
                    const bool ok1 = !k1 || r0 == h1, ok2 = !k2 || (ok1 && r1 == h2), ok3 = !k3 || (ok2 && r2 == h3);
                    const bool valid = g == 0 || (g == 1 ? ok1 : g == 2 ? ok2 : ok3);
                    const bool changed = leader && valid && res != prev;
                    if (changed) __hip_atomic_store(est_at(x), res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    evaluated += cnt;
                    kept += (uint32_t)__popcll(__ballot(leader && kd != 0u && valid));   // (counted whether asked for or not: a test of RegArgs::stats costs as much)
                    if (__ballot(changed)) BBME_DRAIN();                       // the stores have completed
                    BBME_PHASE(prof, 3);
                    // release, and the claims: lanes 0..3 one dependant each, as in the plain round -- but not the block that was
                    // evaluated behind this one in this very round (nk: the next group's link) -- and, where the block took the
                    // value of an updated input (fk: the first of L, UL, U, UR that holds it) while the queue is short, lanes 4.. the
                    // blocks 2, 3, .. steps along that direction
                    uint32_t wasx = 0;
                    if (leader && valid) wasx = own_release(a, x);
                    const bool g_changed = dpp_row<0x150>((uint32_t)changed) != 0;
                    const uint32_t nk = g == 0 ? k1 : g == 1 ? k2 : g == 2 ? k3 : 0u;
                    const uint32_t took = (uint32_t)(__ballot(active && lc.present && mv == res) >> (lane & 48)) & 0xffffu;
                    const uint32_t fk = (took & 2u) ? 1u : (took & 16u) ? 4u : (took & 64u) ? 6u : (took & 32u) ? 5u : 0u;
                    const bool grow = g_changed && nk == 0u && fk != 0u && tail - head < (uint32_t)NBL;
                    // candidate L, UL, U, UR is read by the dependant R, DR, D, DL: lane 0, 1, 2, 3
                    const int nd = nk == 1u ? 0 : nk == 4u ? 1 : nk == 6u ? 2 : 3, fd = fk == 1u ? 0 : fk == 4u ? 1 : fk == 6u ? 2 : 3;
                    const bool ahead = grow && sub >= 4 && (uint32_t)sub < 4u + flood_depth;
                    const int d = sub < 4 ? sub : fd, steps = sub < 4 ? 1 : sub - 2;
                    const int tr = r + steps * (d != 0), tc = c + steps * (d < 2 ? 1 : 2 - d);   // (0,+1) (+1,+1) (+1,0) (+1,-1)
                    const bool want = g_changed && (sub < 4 ? !(nk != 0u && sub == nd) : ahead) && tr < a.rows && tc >= 0 && tc < a.cols;
                    const uint32_t tx = (uint32_t)tr * cols + (uint32_t)tc;
                    uint32_t was = 1;
                    if (want) was = own_claim(a, tx);
                    BBME_PHASE(prof, 4);
                    // the flood's next blocks, and the entries whose evaluation did not count, go to the FRONT of the queue, in
                    // order: the next round takes them side by side; the other dependants go to its end
                    const bool won = want && was == 0u;
                    const bool requeue = leader && !valid;
                    const bool front = requeue || (won && grow && (sub >= 4 || sub == fd));
                    const uint32_t fval = requeue ? e : sub >= 4 ? tx | kFloodEntry : tx;
                    const unsigned long long fm = __ballot(front);
                    const uint32_t nf = (uint32_t)__popcll(fm);
                    if (nf != 0u) {
                        if (tail - head + nf <= QCAP) {
                            if (front) q[(head - nf + (uint32_t)__popcll(fm & lt_mask)) % QCAP] = fval;
                            head = __builtin_amdgcn_readfirstlane(head - nf);
                        } else {
                            enqueue(front, fval);
                        }
                    }
                    enqueue(won && !front, tx);
                    if (__ballot(leader && wasx >= 2)) {                    // an input changed while we held x: take it again
                        bool again = false;
                        if (leader && wasx >= 2) again = own_claim(a, x) == 0;
                        enqueue(again, x);
                    }
                    if (wasx >= 0x80000000u) solver_counters(kp)[5] = 1;            // counter close to overflow: report
                    BBME_PHASE(prof, 5);
                    continue;
                }
            }
            const int gl = wide ? LPBW : 16;                             // lanes per block this round
            const int g = lane / gl, sub = lane % gl;
            const uint32_t cnt = min((uint32_t)(wide ? NBW : NBL), tail - head);
            backlog += (tail - head > cnt) ? 1u : 0u;
            const bool active = (uint32_t)g < cnt;
            uint32_t x = active ? q[(head + g) % QCAP] : 0u;            // owned since it was claimed
            if constexpr (FLOOD) x &= ~kFloodEntry;                     // (a throughput round takes a marked entry as any other)
            head = __builtin_amdgcn_readfirstlane(head + cnt);
            const bool leader = active && sub == 0;
            bool changed = false;
            int r = 0, c = 0;
            if (active) {
                r = (int)(x / a.cols); c = (int)(x % a.cols);
                mv_t prev = 0;
                if (leader) prev = load_est<true>(est_at(x));          // issued with the candidate loads
                mv_t res;
                if (wide) res = eval_block<BS, true>(a, r, c, sub, BBME_NEW_MASK);
                else res = eval_block_lanes<BS, true, MEMO>(a, r, c, sub, BBME_NEW_MASK, prof, &lgeom, MEMO ? &mstats : nullptr);
                changed = leader && res != prev;
                if (changed) __hip_atomic_store(est_at(x), res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if constexpr (MEMO) {
                    // the dependants' SADs of the new value, while the store drains
                    if (!wide && a.memo_forward) {
                        const unsigned long long cb = __ballot(changed);
                        if (cb) {
                            forward_sads<BS>(a, r, c, sub, dpp_row<0x150>((uint32_t)changed) != 0, res);
                            mstats.forwards += (uint32_t)__popcll(cb);
                        }
                    }
                }
            }
            evaluated += cnt;
            if (__ballot(changed)) BBME_DRAIN();                       // the stores have completed
            BBME_PHASE(prof, 3);                                        // store + drain
            if (!wide) {
                // chain form: lanes 0..3 of a block's group claim one dependant each (R, DR, D, DL) -- one atomic instruction,
                // one ballot and one queue write per round instead of four of each, on a path where a lone wave pays
                // about five cycles for every instruction; the release goes out first, in the same trip
                uint32_t wasx = 0;
                if (leader) wasx = own_release(a, x);
                const bool g_changed = dpp_row<0x150>((uint32_t)changed) != 0;
                const int tr = r + (sub != 0), tc = c + (sub < 2 ? 1 : 2 - sub);      // (0,+1) (+1,+1) (+1,0) (+1,-1)
                const bool want = g_changed && sub < 4 && tr < a.rows && tc >= 0 && tc < a.cols;
                const uint32_t tx = (uint32_t)tr * a.cols + tc;
                uint32_t was = 1;
                if (want) was = own_claim(a, tx);
                BBME_PHASE(prof, 4);                                    // claim dependants + release
                enqueue(want && was == 0, tx);
                if (__ballot(leader && wasx >= 2)) {                    // an input changed while we held x: take it again
                    bool again = false;
                    if (leader && wasx >= 2) again = own_claim(a, x) == 0;
                    enqueue(again, x);
                }
                if (wasx >= 0x80000000u) solver_counters(kp)[5] = 1;            // counter close to overflow: report
                BBME_PHASE(prof, 5);                                    // enqueue + re-claim
                continue;
            }
            // one trip for all five atomics: claim the dependants R, DR, D, DL and release x
            const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 1, 0, -1};
            uint32_t xd[4], was[4];
            bool want[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int rr = r + dr[d], cc = c + dc[d];
                want[d] = changed && rr < a.rows && cc >= 0 && cc < a.cols;
                xd[d] = want[d] ? (uint32_t)rr * a.cols + cc : 0u;
                was[d] = 1;
                if (want[d]) was[d] = own_claim(a, xd[d]);
            }
            uint32_t wasx = 0;
            if (leader) wasx = own_release(a, x);
            BBME_PHASE(prof, 4);                                        // claim dependants + release
            // the newly owned dependants go on the queue: the four ballots first, then the stores, so
            // that the round does not wait on four enqueues in a row
            {
                unsigned long long m[4];
                uint32_t tot[4], total = 0;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    m[d] = __ballot(want[d] && was[d] == 0);
                    tot[d] = (uint32_t)__popcll(m[d]);
                    total += tot[d];
                }
                if (total != 0 && tail - head + total <= QCAP) {
                    uint32_t off = tail;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        if (want[d] && was[d] == 0) q[(off + (uint32_t)__popcll(m[d] & lt_mask)) % QCAP] = xd[d];
                        off += tot[d];
                    }
                    tail = __builtin_amdgcn_readfirstlane(tail + total);
                } else if (total != 0) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) enqueue(want[d] && was[d] == 0, xd[d]);
                }
            }
            // an input changed while we held x: take it again (unless somebody else just did)
            if (__ballot(leader && wasx >= 2)) {
                bool again = false;
                if (leader && wasx >= 2) again = own_claim(a, x) == 0;
                enqueue(again, x);
            }
            if (wasx >= 0x80000000u) solver_counters(kp)[5] = 1;                // counter close to overflow: report
            BBME_PHASE(prof, 5);                                        // enqueue + re-claim
        }
    }
#ifdef BBME_PHASE_PROFILE
    if (lane == 0 && prof_s.ph[6])
        for (int i = 0; i < 7; ++i) atomicAdd(&solver_counters(kp)[9 + i], prof_s.ph[i]);
#endif
    if (BBME_SOLVER_COLD(kp, stats) && lane == 0 && evaluated) {
        uint32_t *counters = solver_counters(kp);
        atomicAdd(&counters[4], evaluated); atomicMax(&counters[7], rounds); atomicAdd(&counters[8], rounds);
#ifndef BBME_PHASE_PROFILE
        atomicMax(&counters[13], rounds << 16 | min(backlog, 0xffffu)); atomicAdd(&counters[14], backlog);
        if constexpr (FLOOD) { if (kept) atomicAdd(&counters[15], kept); }
        if constexpr (MEMO) {
            if (mstats.lookups) {
                atomicAdd(&counters[9], mstats.lookups); atomicAdd(&counters[10], mstats.misses);
                atomicAdd(&counters[11], mstats.passes); atomicAdd(&counters[12], mstats.forwards);
            }
        }
#endif
    }

    // epilogue: the workgroup that takes the last ticket knows every other one has finished (their
    // stores were drained before they took theirs) and empties the overflow list, if there is one
    BBME_DRAIN();
    __syncthreads();
    if (threadIdx.x == 0) s_ticket = atomicAdd(&solver_counters(kp)[6], 1u);
    __syncthreads();
    if (s_ticket != gridDim.x - 1) return;
    drain_lists<BS>(solver_all_args(a, kp), threadIdx.x, (int)blockDim.x);
    uint32_t *publish = BBME_SOLVER_COLD(kp, publish);
    if (publish) {                                            // the sweep is complete: every workgroup's stores were drained before its ticket
        BBME_DRAIN();
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(publish + (size_t)blockIdx.y * 16u, BBME_SOLVER_COLD(kp, publish_value), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// =======================================================================================
// K5: MF::copy_to_all_pixels after the last divide (motion_framework.cpp:205-206, 815-826):
// every pixel of level 0 takes the MV of its 2x2 cell, as float2.  One thread per cell row pair.
// =======================================================================================
__global__ __launch_bounds__(256) void k_expand(const mv_t *cells, int cell_cols, int cell_rows,
                                                float *flow, int width, uint32_t s_cells, size_t s_flow)
{
    cells += (size_t)blockIdx.y * s_cells;                            // batch: blockIdx.y = pair
    flow += (size_t)blockIdx.y * s_flow;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)cell_cols * cell_rows * 2;     // two pixel rows per cell row
    if (t >= total) return;
    const int cx = (int)(t % cell_cols);
    const int y = (int)(t / cell_cols);                               // pixel row
    const mv_t m = cells[(size_t)(y >> 1) * cell_cols + cx];
    const float u = (float)mv_x(m), v = (float)mv_y(m);
    float4 o = make_float4(u, v, u, v);
    *reinterpret_cast<float4 *>(flow + 2 * ((size_t)y * width + 2 * cx)) = o;
}

// =======================================================================================
// Flow::CalculateMSE (rw_flow.cpp:309-332) fused with the driver's subsampling (main_class.cpp:58-70): end-point
// error between a ground-truth field and the result at every `scale`-th pixel of the unpadded frame, divided by
// `scale`, straight from the 2x2-cell grid.  float arithmetic per pixel as in the reference's expression, double
// sums; every workgroup leaves one partial sum and one count, the host adds them in index order.
// =======================================================================================
__global__ __launch_bounds__(256) void k_epe(const mv_t *cells, int cell_cols, int pad_x, int pad_y, int scale,
                                             const float *gtruth, int gt_width, int gt_height,
                                             double *partial_sum, unsigned long long *partial_cnt)
{
#pragma clang fp contract(off)
    __shared__ double s_sum[256];
    __shared__ unsigned long long s_cnt[256];
    const long long n = (long long)gt_width * gt_height;
    double sum = 0;
    unsigned long long cnt = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float gu = gtruth[2 * i], gv = gtruth[2 * i + 1];
        if (fabsf(gu) > 1e9f || fabsf(gv) > 1e9f || isnan(gu) || isnan(gv)) continue;     // unknown_flow :39-43
        const int y = pad_y + scale * (int)(i / gt_width), x = pad_x + scale * (int)(i % gt_width);
        const mv_t m = cells[(size_t)(y >> 1) * cell_cols + (x >> 1)];
        const float eu = (float)mv_x(m) / (float)scale, ev = (float)mv_y(m) / (float)scale;
        const float du = gu - eu, dv = gv - ev;
        const float sq = du * du + dv * dv;
        sum += (double)sqrtf(sq);
        ++cnt;
    }
    s_sum[threadIdx.x] = sum; s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s_sum[threadIdx.x] += s_sum[threadIdx.x + o]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial_sum[blockIdx.x] = s_sum[0]; partial_cnt[blockIdx.x] = s_cnt[0]; }
}

// =======================================================================================
// The driver's subsampling (main_class.cpp:58-70) straight from the 2x2-cell grid, with k_epe's indexing:
// out(y, x) = cell((pad_y + s y) >> 1, (pad_x + s x) >> 1) / s for the ceil(W/s) x ceil(H/s) field of the unpadded
// W x H frame; rows out_pitch float2 apart.  s = 4: what bbme_subsample_div4 makes of the dense field; s = 1: the
// unpadded window.  One output pixel per thread; batch as k_expand (blockIdx.y = pair).
// =======================================================================================
__global__ __launch_bounds__(256) void k_subsample(const mv_t *cells, int cell_cols, int pad_x, int pad_y, int scale,
                                                   float *out, int out_width, int out_height, int out_pitch,
                                                   uint32_t s_cells, size_t s_out)
{
    cells += (size_t)blockIdx.y * s_cells;
    out += (size_t)blockIdx.y * s_out;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)out_width * out_height) return;
    const int x = (int)(t % out_width), y = (int)(t / out_width);
    const mv_t m = cells[(size_t)((pad_y + scale * y) >> 1) * cell_cols + ((pad_x + scale * x) >> 1)];
    const float s = (float)scale;
    *reinterpret_cast<float2 *>(out + 2 * ((size_t)y * out_pitch + x)) = make_float2((float)mv_x(m) / s, (float)mv_y(m) / s);
}

// =======================================================================================
// Flow::MotionToColor (rw_flow.cpp:202-275) of the subsampled field, straight from the 2x2-cell grid (the colour rule of
// include/bbme.h).  Pixel (x, y) of the ow x oh image samples cell ((pad_y + s y) >> 1, (pad_x + s x) >> 1), so the field has
// one value per SAMPLED cell: ncx x ncy of them, sampled column i being cell column (pad_x >> 1) + i at s = 1 (a cell then
// covers up to 2x2 pixels) and (pad_x + s i) >> 1 = pixel column i at s >= 2.  Both passes evaluate sampled cells, not pixels.
//   k_color_range_init    the five words of every pair <- the keys of the reference's sentinels -1, 999, -999, 999, -999
//   k_color_range         max radius, min / max u, min / max v over the sampled cells: a workgroup takes 256 kColorCellsPerLane
//                         consecutive cells of one sampled row, a lane folds its cells, a wave its lanes by shuffles, the
//                         workgroup its four waves through LDS, and five lanes issue one atomic max / min each on the pair's
//                         words.  The words hold float_key(), an order-preserving map of float bits to unsigned integers, so
//                         the result is the exact max / min whatever the schedule.  The five words exist kColorKeyCopies times
//                         per pair, 128 bytes apart, and workgroup g adds to copy g mod kColorKeyCopies: two thousand
//                         workgroups adding to ONE line took 50 us per 4K pair, the line's atomics being served one after the
//                         other (profiles/r10_flow_color.txt).
//   k_color_range_finish  folds the copies and turns keys into floats (the context's copy that k_color_image reads, the caller's)
//   k_color_image         a workgroup takes 64 sampled columns x 4 kColorRowsPerWave sampled rows, one wave per row (every fourth
//                         row of them, one after the other): every lane colours one cell (B | G << 8 | R << 16) into LDS,
//                         then the wave writes the pixel row(s) its cells cover: the bytes of
//                         the row segment as whole dwords at 4-byte aligned addresses, each funnel-shifted from the two pixels
//                         it straddles, and single bytes only for the up to 3 + 3 bytes in front of the first and behind the
//                         last aligned dword (none when the caller's rows are dword-aligned and s >= 2 or pad_x is even: a
//                         tile's segment is then 192 or 384 bytes from a multiple of 192 or 384).
// The reference's float / double expression order is kept and nothing is contracted into an FMA; the hue angle is the double
// atan2 rounded to float (include/bbme.h says why).  The 55 x 3 wheel, already divided by 255.0f, is constant memory copied to LDS.
// =======================================================================================
struct ColorWheelTable {
    float c[55 * 3];                                       // entry k, channel b (R, G, B) -> (float)level / 255.0f
    constexpr ColorWheelTable() : c{}
    {
        const int len[6] = {15, 6, 4, 11, 13, 6};          // RY YG GC CB BM MR (makecolorwheel, rw_flow.cpp:277-300)
        const int moving[6] = {1, 0, 2, 1, 0, 2};          // channel that changes
        const int rising[6] = {1, 0, 1, 0, 1, 0};          // ... upwards or downwards
        const int base[6][3] = {{255, 0, 0}, {255, 255, 0}, {0, 255, 0}, {0, 255, 255}, {0, 0, 255}, {255, 0, 255}};
        int k = 0;
        for (int t = 0; t < 6; ++t)
            for (int i = 0; i < len[t]; ++i, ++k) {
                const int step = 255 * i / len[t];
                for (int b = 0; b < 3; ++b) {
                    const int level = b != moving[t] ? base[t][b] : rising[t] ? step : 255 - step;
                    c[3 * k + b] = (float)level / 255.0f;
                }
            }
    }
};
__constant__ ColorWheelTable d_color_wheel{};

struct ColorArgs {
    const mv_t *cells;                    // cell_cols entries per row
    uint32_t s_cells;                     // words from pair to pair (k_color_range: blockIdx.y = pair)
    int cell_cols, pad_x, pad_y, scale;
    int ow, oh;                           // the image: ceil(W / scale) x ceil(H / scale)
    int ncx, ncy;                         // sampled cells per row, rows of them
    uint32_t *keys;                       // k_color_range: kColorKeyCopies x kColorKeyStride words per pair
    const float *range;                   // k_color_image: the pair's five floats ([0] = max radius)
    float maxmotion;
    uint8_t *out;                         // B, G, R per pixel, rows pitch bytes apart
    int pitch;
    int tiles_x;                          // k_color_image: ceil(ncx / 64); k_color_range: ceil(ncx / (256 kColorCellsPerLane))
};

constexpr int kColorCellsPerLane = 4;
constexpr int kColorKeyCopies = 32;       // copies of a pair's five words ...
constexpr int kColorKeyStride = 32;       // ... this many words apart (one 128-byte line each)

__device__ __forceinline__ uint32_t float_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k)
{
    return __uint_as_float(k ^ (((k >> 31) - 1u) | 0x80000000u));
}
// (float)d / (float)scale.  For scale = 2^k the quotient is d times the exactly representable 2^-k, the same bits for every
// int16 d without the dozen instructions of a correctly rounded division (scale 1, 2 and 4 are what callers use)
__device__ __forceinline__ float color_component(int d, int scale)
{
    if ((scale & (scale - 1)) == 0) return (float)d * (1.0f / (float)scale);
    return (float)d / (float)scale;
}
__device__ __forceinline__ int color_cell_col(const ColorArgs &a, int i) { return a.scale == 1 ? (a.pad_x >> 1) + i : (a.pad_x + a.scale * i) >> 1; }
__device__ __forceinline__ int color_cell_row(const ColorArgs &a, int j) { return a.scale == 1 ? (a.pad_y >> 1) + j : (a.pad_y + a.scale * j) >> 1; }

// one workgroup per pair
__global__ __launch_bounds__(256) void k_color_range_init(uint32_t *keys)
{
    const int copy = threadIdx.x >> 3, k = threadIdx.x & 7;
    if (k < 5) keys[((size_t)blockIdx.x * kColorKeyCopies + copy) * kColorKeyStride + k] = float_key(k == 0 ? -1.0f : (k & 1) ? 999.0f : -999.0f);
}

__global__ __launch_bounds__(64) void k_color_range_finish(const uint32_t *keys, float *range, float *user_range)
{
    const int k = threadIdx.x;
    if (k >= 5) return;
    const uint32_t *word = keys + (size_t)blockIdx.x * kColorKeyCopies * kColorKeyStride + k;
    uint32_t key = word[0];
    for (int c = 1; c < kColorKeyCopies; ++c) {
        const uint32_t other = word[c * kColorKeyStride];
        key = (k == 1 || k == 3) ? min(key, other) : max(key, other);
    }
    const float f = key_float(key);
    range[5 * blockIdx.x + k] = f;
    if (user_range) user_range[5 * blockIdx.x + k] = f;
}

__global__ __launch_bounds__(256) void k_color_range(ColorArgs a)
{
#pragma clang fp contract(off)
    const mv_t *cells = a.cells + (size_t)blockIdx.y * a.s_cells;
    float r[5] = {-1.0f, 999.0f, -999.0f, 999.0f, -999.0f};                // max radius, min u, max u, min v, max v
    const int j = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int i0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * (256 * kColorCellsPerLane) + (int)threadIdx.x;
    const mv_t *row = cells + (size_t)color_cell_row(a, j) * a.cell_cols;
#pragma unroll
    for (int k = 0; k < kColorCellsPerLane; ++k) {
        const int i = i0 + 256 * k;
        if (i >= a.ncx) break;
        const mv_t m = row[color_cell_col(a, i)];
        const float u = color_component(mv_x(m), a.scale), v = color_component(mv_y(m), a.scale);
        const float rad = sqrtf(u * u + v * v);
        r[0] = r[0] > rad ? r[0] : rad;
        r[1] = r[1] < u ? r[1] : u;
        r[2] = r[2] > u ? r[2] : u;
        r[3] = r[3] < v ? r[3] : v;
        r[4] = r[4] > v ? r[4] : v;
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float other = __shfl_xor(r[k], o);
            r[k] = (k == 1 || k == 3) ? (r[k] < other ? r[k] : other) : (r[k] > other ? r[k] : other);
        }
    }
    __shared__ float part[4][5];
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 5; ++k) part[threadIdx.x >> 6][k] = r[k];
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        const bool is_min = k == 1 || k == 3;
        float f = part[0][k];
        for (int w = 1; w < 4; ++w) f = is_min ? (f < part[w][k] ? f : part[w][k]) : (f > part[w][k] ? f : part[w][k]);
        uint32_t *word = a.keys + ((size_t)blockIdx.y * kColorKeyCopies + blockIdx.x % kColorKeyCopies) * kColorKeyStride + k;
        if (is_min) atomicMin(word, float_key(f));
        else atomicMax(word, float_key(f));
    }
}

// computeColor (rw_flow.cpp:251-275) of (fx, fy) -> B | G << 8 | R << 16; wheel = the table above in LDS
__device__ __forceinline__ uint32_t color_of(float fx, float fy, const float *wheel)
{
#pragma clang fp contract(off)
    const int ncols = 55;
    const float rad = sqrtf(fx * fx + fy * fy);
    const float angle = (float)atan2((double)-fy, (double)-fx);        // the rule's angle: double atan2, rounded to float
    const float an = (float)((double)angle / 3.14159265358979323846);
    const float fk = (an + 1.0f) / 2.0f * (float)(ncols - 1);
    int k0 = (int)fk;
    k0 = k0 < 0 ? 0 : k0 > ncols - 1 ? ncols - 1 : k0;                  // (no finite input leaves 0 .. 54; keeps the LDS index in range)
    const int k1 = k0 + 1 == ncols ? 0 : k0 + 1;
    const float f = fk - (float)k0;
    uint32_t packed = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float col0 = wheel[3 * k0 + b], col1 = wheel[3 * k1 + b];
        float col = (1 - f) * col0 + f * col1;
        if (rad <= 1) col = 1 - rad * (1 - col);
        else col = (float)(col * .75);
        packed |= ((uint32_t)(int)(255.0 * col) & 255u) << (8 * (2 - b));
    }
    return packed;
}

// sampled rows a wave of k_color_image colours, one after the other.  More than one (all cells loaded up front, the wheel copied
// once) measured no faster at 4K (26.5 against 25.8 us with 4) and slower on a 960 x 540 picture (7.8 against 6.3 us): the
// kernel is bound by its arithmetic, not by its loads
constexpr int kColorRowsPerWave = 1;

__global__ __launch_bounds__(256) void k_color_image(ColorArgs a)
{
#pragma clang fp contract(off)
    __shared__ float s_wheel[55 * 3];
    __shared__ uint32_t s_col[4][68];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * 64;
    const int j0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * (4 * kColorRowsPerWave) + w;      // rows j0, j0 + 4, ...
    // every load the tile needs is under way before the first barrier: the cells of all its rows, the wheel, the max radius
    const int cx = color_cell_col(a, min(i0 + lane, a.ncx - 1));
    mv_t m[kColorRowsPerWave];
#pragma unroll
    for (int t = 0; t < kColorRowsPerWave; ++t)
        m[t] = a.cells[(size_t)color_cell_row(a, min(j0 + 4 * t, a.ncy - 1)) * a.cell_cols + cx];
    if (threadIdx.x < 55 * 3) s_wheel[threadIdx.x] = d_color_wheel.c[threadIdx.x];
    if (lane < 4) s_col[w][64 + lane] = 0;
    float maxrad = a.maxmotion > 0 ? a.maxmotion : a.range[0];
    if (maxrad == 0) maxrad = 1;
    // the pixel columns this tile's cells cover, [px0, px1); pixel p of them -> its cell's slot in s_col[w][]
    const int cx0 = color_cell_col(a, i0);
    int px0 = i0, px1 = min(a.ow, i0 + 64);
    if (a.scale == 1) { px0 = max(0, 2 * cx0 - a.pad_x); px1 = min(a.ow, 2 * (cx0 + 64) - a.pad_x); }
    const int nbytes = 3 * (px1 - px0);
    const int rel0 = a.scale == 1 ? a.pad_x + px0 - 2 * cx0 : 0, sh = a.scale == 1 ? 1 : 0;
    const uint32_t *col = s_col[w];
    for (int t = 0; t < kColorRowsPerWave; ++t) {
        const int j = j0 + 4 * t;
        __syncthreads();                                     // the wheel is there (t = 0); row t - 1 has been read
        const float u = color_component(mv_x(m[t]), a.scale), v = color_component(mv_y(m[t]), a.scale);
        s_col[w][lane] = color_of(u / maxrad, v / maxrad, s_wheel);
        __syncthreads();
        if (j >= a.ncy) continue;                            // (whole waves: the barriers stay uniform)
        int y0 = j, y1 = j + 1;                              // the pixel rows sampled row j covers
        if (a.scale == 1) {
            const int cy = color_cell_row(a, j);
            y0 = max(0, 2 * cy - a.pad_y); y1 = min(a.oh, 2 * cy - a.pad_y + 2);
        }
        // at scale 1 a cell covers two pixel rows: when they are aligned alike, their dwords are assembled once
        const bool twin = y1 - y0 == 2 && (a.pitch & 3) == 0;
        for (int y = y0; y < y1; y += twin ? 2 : 1) {
            uint8_t *row = a.out + (size_t)y * a.pitch + 3 * (size_t)px0;
            const int head = min(nbytes, (int)((4u - (uint32_t)((uintptr_t)row & 3u)) & 3u));
            const int ndw = (nbytes - head) >> 2, tail = nbytes - head - 4 * ndw;
            for (int d = lane; d < ndw; d += 64) {
                const int o = head + 4 * d, p = o / 3, ch = o - 3 * p;
                const unsigned long long v2 = (unsigned long long)col[(rel0 + p) >> sh] | (unsigned long long)col[(rel0 + p + 1) >> sh] << 24;
                *reinterpret_cast<uint32_t *>(row + o) = (uint32_t)(v2 >> (8 * ch));
                if (twin) *reinterpret_cast<uint32_t *>(row + a.pitch + o) = (uint32_t)(v2 >> (8 * ch));
            }
            if (lane < head + tail) {                        // the bytes around the aligned dwords
                const int o = lane < head ? lane : 4 * ndw + lane, p = o / 3, ch = o - 3 * p;
                const uint8_t b = (uint8_t)(col[(rel0 + p) >> sh] >> (8 * ch));
                row[o] = b;
                if (twin) row[a.pitch + o] = b;
            }
        }
    }
}

// =======================================================================================
// Frame preparation.  MF::MF on the GPU (motion_framework.cpp:57-61, 86-106): zero border and pyrDown cascade, with the x4
// up-sampling or the B,G,R -> luma conversion fused into the border pass where the frames come that way.  Bandwidth-bound byte
// work: 16 bytes per thread for the border copy, four output pixels per thread for pyrDown (dword loads, the 5-tap rows as
// v_dot4_u32_u8 on re-aligned dwords).
// The bodies are __device__ functions of one plane.  ONE family of kernels runs them, the *_run kernels: the frames of a SET in
// one launch per step, blockIdx.y = frame of the set.  A set is {first slot address, count, step}: the two frames of a pair (the
// pair's image-1 plane, 2, the distance from image 1 to image 2) or a run of a chain context's slots (the first slot, count, one
// plane stride).  Level 0: frame f is read from run.src[f] (a kernel-argument table: a caller's frames lie anywhere) and written
// to dst + f * s_dst; the cascade reads and writes planes of the context (src + f * s_src -> dst + f * s_dst).  So a setter costs
// num_levels launches whatever the number of frames.  The steps are size_t: a pair's is the image-1 planes of a whole batch.
// =======================================================================================
constexpr int kMaxChainFrames = 65;                    // BBME_MAX_BATCH pairs are one frame more
struct FrameRun { const uint8_t *src[kMaxChainFrames]; };

__device__ __forceinline__ void pad_zero_plane(const uint8_t *src, uint8_t *dst, int width, int height, int pitch,
                                               int pad_x, int pad_y, int pw, int ph)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;    // 16 output bytes (pw is a multiple of 4)
    const int per_row = (pw + 15) / 16;
    if (t >= (long long)per_row * ph) return;
    const int y = (int)(t / per_row), x0 = (int)(t % per_row) * 16;
    const int sy = y - pad_y, sx0 = x0 - pad_x;
    uint32_t w[4] = {0, 0, 0, 0};
    if (sy >= 0 && sy < height) {
        const uint8_t *row = src + (size_t)sy * pitch;
        if (sx0 >= 0 && sx0 + 16 <= width) {                           // inside: one (unaligned) 16-byte load
            const ua_u128 v = *reinterpret_cast<const ua_u128 *>(row + sx0);
            w[0] = v.v[0]; w[1] = v.v[1]; w[2] = v.v[2]; w[3] = v.v[3];
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const int sx = sx0 + b;
                if (sx >= 0 && sx < width) w[b >> 2] |= (uint32_t)row[sx] << (8 * (b & 3));
            }
        }
    }
    uint8_t *o = dst + (size_t)y * pw + x0;
    if (x0 + 16 <= pw && (((uintptr_t)o) & 15u) == 0) {               // the usual case: one 16-byte store
        *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        uint32_t *out = reinterpret_cast<uint32_t *>(o);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + 4 * q < pw) out[q] = w[q];
    }
}

__global__ __launch_bounds__(256) void k_pad_zero_run(FrameRun run, uint8_t *dst, size_t s_dst, int width, int height, int pitch,
                                                      int pad_x, int pad_y, int pw, int ph)
{
    pad_zero_plane(run.src[blockIdx.y], dst + blockIdx.y * s_dst, width, height, pitch, pad_x, pad_y, pw, ph);
}

// =======================================================================================
// cv::resize(..., 4, 4, INTER_LINEAR) of main_class.cpp:32-33 fused with the zero border (motion_framework.cpp:57-61):
// pixel (X, Y) of the padded plane is resize_x4(src)(X - pad_x, Y - pad_y) inside the frame, 0 outside.  Bit for bit
// bbme::resize_x4 (bbme_host.cpp), whose coefficients repeat with period 4: phase p of an output coordinate d = 4k + p
// samples source k - 1 (p = 0, 1) or k (p = 2, 3) with weights (768, 1280), (256, 1792), (1792, 256), (1280, 768).
// Horizontally a first column outside the source resets them to (2048, 0) (output columns 0, 1, 4W-2, 4W-1);
// vertically only the row index is clamped.  16 output bytes per thread, the
// source bytes a thread needs (at most 7 per row) held in one 64-bit word per row.  sw, sh: source size; pw, ph: plane.
// =======================================================================================
__device__ __forceinline__ int resize_x4_w0(int phase)      // weight of the first tap; the second is 2048 minus it
{
    return phase == 0 ? 768 : phase == 1 ? 256 : phase == 2 ? 1792 : 1280;
}

__device__ __forceinline__ void resize_x4_pad_plane(const uint8_t *src, uint8_t *dst, int sw, int sh, int pitch,
                                                    int pad_x, int pad_y, int pw, int ph)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per_row = (pw + 15) / 16;
    if (t >= (long long)per_row * ph) return;
    const int y = (int)(t / per_row), x0 = (int)(t % per_row) * 16;
    const int dw = 4 * sw, dy = y - pad_y, dx0 = x0 - pad_x;
    uint32_t w[4] = {0, 0, 0, 0};
    if (dy >= 0 && dy < 4 * sh) {
        const int py = dy & 3, sy = (dy >> 2) - (py < 2 ? 1 : 0);
        const int y0 = min(max(sy, 0), sh - 1), y1 = min(max(sy + 1, 0), sh - 1);
        const int b0 = resize_x4_w0(py), b1 = 2048 - b0;
        const int kbase = (dx0 >> 2) - 1;                             // first source column any of the 16 bytes reads
        uint64_t r0 = 0, r1 = 0;
        const uint8_t *s0 = src + (size_t)y0 * pitch, *s1 = src + (size_t)y1 * pitch;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sx = kbase + j;
            if (sx >= 0 && sx < sw) { r0 |= (uint64_t)s0[sx] << (8 * j); r1 |= (uint64_t)s1[sx] << (8 * j); }
        }
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int dx = dx0 + b;
            if (dx < 0 || dx >= dw) continue;
            const int px = dx & 3;
            int sx = (dx >> 2) - (px < 2 ? 1 : 0), a0 = resize_x4_w0(px);
            if (sx < 0 || sx >= sw - 1) { sx = min(max(sx, 0), sw - 1); a0 = 2048; }
            const int a1 = 2048 - a0;
            const int i = 8 * (sx - kbase);                           // sx + 1 - kbase <= 7: inside the word
            const int h0 = (int)((r0 >> i) & 0xffu) * a0 + (int)((r0 >> (i + 8)) & 0xffu) * a1;
            const int h1 = (int)((r1 >> i) & 0xffu) * a0 + (int)((r1 >> (i + 8)) & 0xffu) * a1;
            const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
            w[b >> 2] |= (uint32_t)v << (8 * (b & 3));
        }
    }
    uint8_t *o = dst + (size_t)y * pw + x0;
    if (x0 + 16 <= pw && (((uintptr_t)o) & 15u) == 0) {
        *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {                                                          // the row's last chunk, or rows not 16-byte aligned
        uint32_t *out = reinterpret_cast<uint32_t *>(o);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (x0 + 4 * q + 4 <= pw) out[q] = w[q];
            else
                for (int b = 4 * q; b < 4 * q + 4; ++b)               // nothing past the row: it is the next row's
                    if (x0 + b < pw) o[b] = (uint8_t)(w[q] >> (8 * (b & 3)));
        }
    }
}

__global__ __launch_bounds__(256) void k_resize_x4_pad_run(FrameRun run, uint8_t *dst, size_t s_dst, int sw, int sh, int pitch,
                                                           int pad_x, int pad_y, int pw, int ph)
{
    resize_x4_pad_plane(run.src[blockIdx.y], dst + blockIdx.y * s_dst, sw, sh, pitch, pad_x, pad_y, pw, ph);
}

__device__ __forceinline__ int mirror101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// four output pixels per thread.  sw is a multiple of 8 (the host checks it where it launches: a context's level widths are
// multiples of 4, so every level that is pyrDown's source is a multiple of 8 wide).  Output x = 4k + c reads input bytes
// 8k + 2c - 2 .. 8k + 2c + 2, all inside the four dwords at 8k - 4 .. 8k + 11.  h = [1 4 6 4] . bytes[o .. o+3] (v_dot4_u32_u8 on a re-aligned dword)
// + byte[o + 4]; out = (h0 + 4 h1 + 6 h2 + 4 h3 + h4 + 128) >> 8 over the five (mirrored) rows -- the same integers as
// the separable host form, no rounding in between.
__device__ __forceinline__ void pyr_down4_plane(const uint8_t *src, uint8_t *dst, int sw, int sh)
{
    const int dw = sw / 2, dh = sh / 2, per_row = dw / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)per_row * dh) return;
    const int k = (int)(t % per_row), y = (int)(t / per_row);
    const bool left = k == 0, right = 8 * k + 12 > sw;                // sw % 8 == 0: the last thread of a row
    const uint32_t taps = 1u | 4u << 8 | 6u << 16 | 4u << 24;
    uint32_t acc[4] = {128, 128, 128, 128};
    const uint32_t wy[5] = {1, 4, 6, 4, 1};
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
        // the four dwords around input byte 8k in ONE 16-byte load (any byte alignment is fine on gfx950): a quarter of the load
        // instructions of four dword loads.  The first thread of a row starts at the row itself (nothing may be read in front of
        // the plane); the last one reads up to 4 bytes past the row (the next row, or the plane's slack) and ignores them.  On a
        // row of 8 bytes the one thread is both: it starts at the row and reads 8 bytes past it (the slack is 256 bytes at least).
        const uint8_t *row = src + (size_t)mirror101(2 * y + ky - 2, sh) * sw + 8 * k;
        const ua_u128 v = *reinterpret_cast<const ua_u128 *>(row - (left ? 0 : 4));
        uint32_t d[4];
        d[0] = v.v[0]; d[1] = left ? v.v[0] : v.v[1]; d[2] = left ? v.v[1] : v.v[2]; d[3] = left ? v.v[2] : v.v[3];
        // BORDER_REFLECT_101 at the row ends, without divergent byte loops: of d[0] only input bytes -2, -1 (= 2, 1) are
        // used, of d[3] only input byte 8k+8 (= sw, mirrored to sw - 2 = 8k+6)
        if (left) d[0] = (d[1] & 0x00ff0000u) | (d[1] & 0x0000ff00u) << 16;
        if (right) d[3] = (d[2] >> 16) & 0xffu;
        // byte offsets inside d[]: window of output c starts at 2c + 2
        const uint32_t w0 = __builtin_amdgcn_alignbyte(d[1], d[0], 2), w1 = d[1];
        const uint32_t w2 = __builtin_amdgcn_alignbyte(d[2], d[1], 2), w3 = d[2];
        const uint32_t h0 = __builtin_amdgcn_udot4(w0, taps, (d[1] >> 16) & 0xffu, false);
        const uint32_t h1 = __builtin_amdgcn_udot4(w1, taps, d[2] & 0xffu, false);
        const uint32_t h2 = __builtin_amdgcn_udot4(w2, taps, (d[2] >> 16) & 0xffu, false);
        const uint32_t h3 = __builtin_amdgcn_udot4(w3, taps, d[3] & 0xffu, false);
        acc[0] += wy[ky] * h0; acc[1] += wy[ky] * h1; acc[2] += wy[ky] * h2; acc[3] += wy[ky] * h3;
    }
    const uint32_t out = (acc[0] >> 8) | (acc[1] >> 8) << 8 | (acc[2] >> 8) << 16 | (acc[3] >> 8) << 24;
    *reinterpret_cast<uint32_t *>(dst + (size_t)y * dw + 4 * k) = out;
}

__global__ __launch_bounds__(256) void k_pyr_down4_run(const uint8_t *src, size_t s_src, uint8_t *dst, size_t s_dst, int sw, int sh)
{
    pyr_down4_plane(src + blockIdx.y * s_src, dst + blockIdx.y * s_dst, sw, sh);
}

// bbme_chain_advance: the last slot of every level becomes slot 0, all levels in one launch (blockIdx.y = level).  Whole
// plane strides (multiples of 64 bytes; the slack behind a plane is zero in every slot), 16 bytes per thread and step.
struct ChainRoll { const uint4 *src[8]; uint4 *dst[8]; uint32_t n16[8]; };

__global__ __launch_bounds__(256) void k_chain_roll(ChainRoll r)
{
    const uint4 *src = r.src[blockIdx.y];
    uint4 *dst = r.dst[blockIdx.y];
    const uint32_t n = r.n16[blockIdx.y];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) dst[i] = src[i];
}

// =======================================================================================
// Colour frames in (the luma rule of include/bbme.h): B,G,R frames, rows `pitch` >= 3 width bytes apart at any alignment,
// become the zero-bordered level-0 luma planes in ONE pass -- conversion and border, pad_zero_plane's launch shape and stores:
// a thread makes 16 bytes of a plane row from the 48 source bytes under them (three unaligned 16-byte loads inside the frame,
// bytes at its edges).  With `keep` it also writes those 48 bytes to the packed copy (pitch 3 width) the context keeps of a
// caller's frame: every pixel of the frame lies under exactly one thread.  Bandwidth-bound like the grey border copy, on four
// (with keep, seven) bytes per pixel instead of two.  k_bgr_pad_run: the frames of a set, as the kernels of the frame
// preparation above (run.src[f] -> frame f of dst and of keep).
// =======================================================================================

__device__ __forceinline__ uint32_t bgr_luma(uint32_t b, uint32_t g, uint32_t r)
{
    return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;
}

__device__ __forceinline__ void bgr_pad_plane(const uint8_t *src, uint8_t *dst, uint8_t *keep, int width, int height, int pitch,
                                              int pad_x, int pad_y, int pw, int ph)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;    // 16 output bytes (pw is a multiple of 4)
    const int per_row = (pw + 15) / 16;
    if (t >= (long long)per_row * ph) return;
    const int y = (int)(t / per_row), x0 = (int)(t % per_row) * 16;
    const int sy = y - pad_y, sx0 = x0 - pad_x;
    uint32_t w[4] = {0, 0, 0, 0};
    if (sy >= 0 && sy < height) {
        const uint8_t *row = src + (size_t)sy * pitch;
        uint8_t *kept = keep ? keep + (size_t)sy * width * 3 : nullptr;
        uint32_t c[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};       // 16 pixels of B,G,R; 0 outside the frame
        if (sx0 >= 0 && sx0 + 16 <= width) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const ua_u128 v = *reinterpret_cast<const ua_u128 *>(row + 3 * sx0 + 16 * q);
                c[4 * q] = v.v[0]; c[4 * q + 1] = v.v[1]; c[4 * q + 2] = v.v[2]; c[4 * q + 3] = v.v[3];
                if (kept) *reinterpret_cast<ua_u128 *>(kept + 3 * sx0 + 16 * q) = v;
            }
        } else {
#pragma unroll
            for (int b = 0; b < 48; ++b) {
                const int sx = sx0 + b / 3;
                if (sx < 0 || sx >= width) continue;
                const uint8_t v = row[3 * sx + b % 3];
                c[b >> 2] |= (uint32_t)v << (8 * (b & 3));
                if (kept) kept[3 * sx + b % 3] = v;
            }
        }
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const auto ch = [&](int k) { return (c[(3 * b + k) >> 2] >> (8 * ((3 * b + k) & 3))) & 0xffu; };
            w[b >> 2] |= bgr_luma(ch(0), ch(1), ch(2)) << (8 * (b & 3));
        }
    }
    uint8_t *o = dst + (size_t)y * pw + x0;
    if (x0 + 16 <= pw && (((uintptr_t)o) & 15u) == 0) {               // the usual case: one 16-byte store
        *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        uint32_t *out = reinterpret_cast<uint32_t *>(o);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + 4 * q < pw) out[q] = w[q];
    }
}

// keep: the set's first slot of the colour store (its frames s_keep bytes apart), or null
__global__ __launch_bounds__(256) void k_bgr_pad_run(FrameRun run, uint8_t *dst, size_t s_dst, uint8_t *keep, size_t s_keep,
                                                     int width, int height, int pitch, int pad_x, int pad_y, int pw, int ph)
{
    bgr_pad_plane(run.src[blockIdx.y], dst + blockIdx.y * s_dst, keep ? keep + blockIdx.y * s_keep : nullptr, width, height,
                  pitch, pad_x, pad_y, pw, ph);
}

// =======================================================================================
// PMC calibration (bbme_calibrate_read): reads n dwords once with one aligned dword per lane --
// the access shape of the search kernel's window staging -- so that FETCH_SIZE can be scaled by a
// known byte count before it is quoted (MI355X_MICROARCH.md, HBM section).
// =======================================================================================
__global__ __launch_bounds__(256) void k_calib_read_dword(const uint32_t *p, size_t n, uint32_t *out)
{
    const size_t stride = (size_t)gridDim.x * 256;
    uint32_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) acc += p[i];
    if (acc == 0x12345678u) out[0] = acc;            // keeps the loads alive, practically never taken
}

// =======================================================================================
// instruction probes (bbme_selftest_isa)
// =======================================================================================
// issue-rate probes: 8 independent accumulator chains per lane, ITER x 8 instructions per lane
template <int WHICH>
__global__ __launch_bounds__(256) void k_probe_rate(uint32_t *out, int iters, uint32_t seed)
{
    uint32_t x = seed + threadIdx.x;
    if constexpr (WHICH == 0) {
        unsigned long long acc[8];
        for (int i = 0; i < 8; ++i) acc[i] = x + i;
        const unsigned long long pair = ((unsigned long long)(x * 2654435761u) << 32) | (x * 40503u);
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_qsad_pk_u16_u8(pair, x + i, acc[i]);
        unsigned long long r = 0;
        for (int i = 0; i < 8; ++i) r ^= acc[i];
        if (r == 0x123456789abcdefull) out[0] = 1;
    } else if constexpr (WHICH == 1) {
        uint32_t acc[8];
        for (int i = 0; i < 8; ++i) acc[i] = x + i;
        const uint32_t w = x * 2654435761u;
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_sad_u8(w, x + i, acc[i]);
        uint32_t r = 0;
        for (int i = 0; i < 8; ++i) r ^= acc[i];
        if (r == 0x12345678u) out[0] = 1;
    } else {
        // mixed: per iteration 8 QSADs and 8*RATIO SADs, independent chains (do the two overlap?)
        constexpr int RATIO = WHICH - 1;                         // WHICH = 2 -> 1:1, 5 -> 1:4
        unsigned long long qa[8];
        uint32_t sa[8];
        for (int i = 0; i < 8; ++i) { qa[i] = x + i; sa[i] = x * 3 + i; }
        const unsigned long long pair = ((unsigned long long)(x * 2654435761u) << 32) | (x * 40503u);
        const uint32_t w = x * 2246822519u;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                qa[i] = __builtin_amdgcn_qsad_pk_u16_u8(pair, x + i, qa[i]);
#pragma unroll
                for (int k = 0; k < RATIO; ++k) sa[(i + k) & 7] = __builtin_amdgcn_sad_u8(w, x + i + k, sa[(i + k) & 7]);
            }
        }
        unsigned long long r = 0;
        for (int i = 0; i < 8; ++i) r ^= qa[i] ^ sa[i];
        if (r == 0x123456789abcdefull) out[0] = 1;
    }
}

// The two candidate inner loops of the search, stripped to their LDS reads and SAD instructions, at the occupancy their
// LDS footprints allow (bbme_probe_search_loops): one wave per workgroup, a 16 x 16 block against an (16+64)^2 window.
//   QSAD   (what k_search_fast does): window once in LDS (6.7 KB), a lane owns 4 adjacent dx x a strip of 16 rows; per
//          window row 5 dword reads feed 64 v_qsad_pk_u16_u8 (16 abs-diff per lane each).
//   SADU8  (the alternative VERDICT r01 asked to measure): v_sad_u8 issues 5x faster than QSAD but needs its window
//          operand dword-aligned, so the window is kept in four copies shifted by 0..3 bytes (27 KB); a lane owns one dx
//          x a strip of 16 rows; per window row one 16-byte read feeds 64 v_sad_u8 (4 abs-diff per lane each).
// A pass is one strip round of the real kernel: 31 window rows, candidate row d meets block row yy - d (16 x 16 x 4 SAD
// instructions per lane); accumulators are folded into `out`.
template <bool SADU8>
__global__ __launch_bounds__(64) void k_probe_search_loop(uint32_t *out, int passes, uint32_t seed)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int lane = threadIdx.x;
    const int words = SADU8 ? 27 * 256 : 1728;                              // 27 KB / 6.75 KB
    for (int i = lane; i < words; i += 64) smem[i] = (i + seed) * 2654435761u;
    __syncthreads();
    uint32_t cur[16][4];                                                    // the 16 x 16 block, wave-uniform (SGPRs)
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[r][q] = __builtin_amdgcn_readfirstlane((seed + 16 * r + q) * 40503u);
    uint32_t fold = 0;
    for (int p = 0; p < passes; ++p) {
        // one strip round: 31 window rows; candidate row d of the strip meets block row yy - d (as search_strip)
        if constexpr (!SADU8) {
            unsigned long long acc[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) acc[d] = 0;
            const uint32_t *wrow = smem + (lane & 15) + 21 * (p & 31);
#pragma unroll
            for (int yy = 0; yy < 31; ++yy) {
                uint32_t w[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) w[q] = wrow[q];
                wrow += 21;
                asm volatile("" ::: "memory");
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    const int brow = yy - d;
                    if (brow < 0 || brow >= 16) continue;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc[d] = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)w[q + 1] << 32) | w[q], cur[brow][q], acc[d]);
                    asm volatile("" : "+v"(acc[d]));
                }
            }
#pragma unroll
            for (int d = 0; d < 16; ++d) fold ^= (uint32_t)acc[d] ^ (uint32_t)(acc[d] >> 32);
        } else {
            uint32_t acc[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) acc[d] = 0;
            const uint4 *wrow = reinterpret_cast<const uint4 *>(smem) + (lane & 3) * 432 + (lane >> 2) + 5 * (p & 31);
#pragma unroll
            for (int yy = 0; yy < 31; ++yy) {
                const uint4 w = wrow[5 * yy];
                asm volatile("" ::: "memory");
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    const int brow = yy - d;
                    if (brow < 0 || brow >= 16) continue;
                    acc[d] = __builtin_amdgcn_sad_u8(w.x, cur[brow][0], acc[d]);
                    acc[d] = __builtin_amdgcn_sad_u8(w.y, cur[brow][1], acc[d]);
                    acc[d] = __builtin_amdgcn_sad_u8(w.z, cur[brow][2], acc[d]);
                    acc[d] = __builtin_amdgcn_sad_u8(w.w, cur[brow][3], acc[d]);
                    asm volatile("" : "+v"(acc[d]));
                }
            }
#pragma unroll
            for (int d = 0; d < 16; ++d) fold ^= acc[d];
        }
    }
    if (fold == 0x12345678u) out[0] = fold;                                  // keeps the work alive
}

// dependent-chain latencies of the memory operations the solver round is made of (one wave, one lane
// active, otherwise idle chip): cycles (s_memtime) and 10 ns ticks (s_memrealtime) per operation
__global__ void k_probe_latency(uint32_t *buf, uint32_t nwords, unsigned long long *out)
{
    if (threadIdx.x != 0) return;
    const int N = 256;
    uint32_t idx = 1;
    unsigned long long c0, c1, r0, r1;
    // (0) plain load chain (pointer chasing over a buffer larger than L1, smaller than L2)
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < N; ++i) idx = buf[idx % nwords];
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    out[0] = (c1 - c0) / N; out[1] = (r1 - r0);
    // (1) agent-scope (sc1) load chain
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < N; ++i) idx = __hip_atomic_load(&buf[idx % nwords], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    out[2] = (c1 - c0) / N; out[3] = (r1 - r0);
    // (2) returning atomic chain
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < N; ++i) idx = atomicAdd(&buf[(idx * 2654435761u) % nwords], 0u) + i;
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    out[4] = (c1 - c0) / N; out[5] = (r1 - r0);
    // (3) agent-scope store + drain
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < N; ++i) {
        __hip_atomic_store(&buf[(idx + 64 * i) % nwords], idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    out[6] = (c1 - c0) / N; out[7] = (r1 - r0);
    out[8] = idx;
}

// Which XCD a workgroup runs on (HW_REG_XCC_ID, bits 3:0).  The kernels only ASSUME that workgroups b and b + 8 share an
// XCD (round-robin dispatch) when they give every residue class of blockIdx.x mod 8 a contiguous part of the raster;
// bbme_probe_xcd checks that assumption on the device.  Speed only: no result depends on it.
__global__ void k_probe_xcc(uint32_t *out)
{
    if (threadIdx.x == 0) out[blockIdx.x] = (uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu;
}

// unaligned global loads: dword / dwordx2 / dwordx4 at arbitrary byte addresses
__global__ void k_probe_unaligned(const uint8_t *p, uint32_t *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *q = p + 5 * i + (i & 3);                  // every byte alignment occurs
    const uint32_t a = reinterpret_cast<const ua_u32 *>(q)->v;
    const ua_u32x2 b = *reinterpret_cast<const ua_u32x2 *>(q + 1);
    const ua_u32x4 c = *reinterpret_cast<const ua_u32x4 *>(q + 2);
    out[7 * i + 0] = a;
    out[7 * i + 1] = b.v[0]; out[7 * i + 2] = b.v[1];
    out[7 * i + 3] = c.v[0]; out[7 * i + 4] = c.v[1]; out[7 * i + 5] = c.v[2]; out[7 * i + 6] = c.v[3];
}

__global__ void k_probe_sad(const uint32_t *a, const uint32_t *b, const uint32_t *c,
                            uint32_t *sad_out, unsigned long long *qsad_out, uint32_t *align_out,
                            uint32_t *sad16_out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sad_out[i] = __builtin_amdgcn_sad_u8(a[i], b[i], c[i]);
    const unsigned long long src0 = ((unsigned long long)b[i] << 32) | a[i];
    const unsigned long long acc = ((unsigned long long)(c[i] & 0x00ff00ffu) << 32) | (c[i] & 0x0f0f0f0fu);
    qsad_out[i] = __builtin_amdgcn_qsad_pk_u16_u8(src0, c[i] ^ a[i], acc);
    align_out[i] = __builtin_amdgcn_alignbyte(b[i], a[i], c[i] & 3u);
    sad16_out[i] = __builtin_amdgcn_sad_u16(a[i], b[i], c[i] & 0xffffu);
}

// =======================================================================================
// What the gather kernels share: k_motion_compensate, K6 k_fb_consistency, K7 k_interpolate, K7b k_interpolate_bgr, K9
// k_temporal_filter, K9b k_temporal_filter_bgr, K11 k_subpel_compensate, K12 k_subpel_interpolate, K12b k_subpel_interpolate_bgr, K13
// k_subpel_temporal_filter, K13b k_subpel_temporal_filter_bgr, K14 k_compose_cells, K15 k_wide_temporal_filter, K15b
// k_wide_temporal_filter_bgr and K11b k_compensate_bgr.  Each is a memory-bound gather in which a lane takes up to k*RunsPerLane runs of 4
// consecutive units (pixels or 2x2 cells) of one row, blockIdx.x counting workgroups of 256 lanes over the runs_per_row x rows
// runs of a plane and blockIdx.y / z pairs, phases or frames; each has optional statistics of four counters over a window (K14
// two of them, K15 six: two quadruples).  The pieces, each written once below and used by every kernel that has the step:
//   gather_index / gather_split   the run split
//   load_mv4                      a run's four grid words
//   load_cells4                   a run's own four 2x2 cells of a plane (ip_cell's packing)
//   rows_put / store_rows2        a run's two grey pixel rows: a cell into them, the rows to memory
//   bgr_load_rows / bgr_row_get / bgr_row_put / bgr_store_rows
//                                 a run's two colour rows of 24 bytes: the run's own rows, a cell out of a row, a cell into a
//                                 row, the rows to the unpadded frame
//   bgr_run_put / bgr_store_run   a one-row run of 4 colour pixels = 12 bytes: a pixel into it, the run to the unpadded frame
//   store_bytes4                  one map byte per unit
//   store_partial4                the statistics tail
//   tf_frame / tf_cost_weight     the temporal filters' neighbour head and weight tail
// =======================================================================================

// Run split: run r (0 .. RPL - 1) of this lane is run gather_index<RPL>(r) of the plane's runs -- past the last one the lane is
// done, its later runs are past it too --, and run i lies in row `row`, starts at unit x0 and holds the n = 1..4 units of it that
// lie inside the row of `units`.  (One helper with the test inside costs registers: the compiler then no longer sees the loop's
// exit before the division.)
template <int RPL>
__device__ __forceinline__ long long gather_index(int r)
{
    return ((long long)blockIdx.x * RPL + r) * 256 + threadIdx.x;
}

__device__ __forceinline__ void gather_split(long long i, int runs_per_row, int units, int &row, int &x0, int &n)
{
    row = (int)(i / runs_per_row);
    x0 = (int)(i % runs_per_row) * 4;
    n = min(4, units - x0);
}

// The four grid words of a run: one unaligned 16-byte load when the run is whole, word by word otherwise (the others 0).
__device__ __forceinline__ void load_mv4(const mv_t *src, int n, uint32_t (&m)[4])
{
    m[0] = m[1] = m[2] = m[3] = 0;
    if (n == 4) {
        const ua_u32x4 v = *reinterpret_cast<const ua_u32x4 *>(src);
        m[0] = v.v[0]; m[1] = v.v[1]; m[2] = v.v[2]; m[3] = v.v[3];
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < n) m[j] = src[j];
    }
}

// One byte per unit of a run, byte j of v for unit x0 + j: one dword when the run is whole and its address dword-aligned (a
// caller's rows need not be), bytes otherwise.
__device__ __forceinline__ void store_bytes4(uint8_t *o, int n, uint32_t v)
{
    if (n == 4 && ((uintptr_t)o & 3u) == 0) *reinterpret_cast<uint32_t *>(o) = v;
    else for (int j = 0; j < n; ++j) o[j] = (uint8_t)(v >> (8 * j));
}

// the 2x2 cell at (x, y) of a plane as one dword: row y in the low half, row y + 1 in the high half
__device__ __forceinline__ uint32_t ip_cell(const uint8_t *img, int W, int x, int y)
{
    const uint8_t *p = img + (size_t)y * W + x;
    return (uint32_t)reinterpret_cast<const ua_u16 *>(p)->v | (uint32_t)reinterpret_cast<const ua_u16 *>(p + W)->v << 16;
}

// bytes s.x, s.x + 1 and s.x + 1 + x1 of a row of I2 (p = the row's byte s.x) in bits 0-7, 8-15 and 16-23
__device__ __forceinline__ uint32_t sc_row(const uint8_t *p, bool wide, int x1)
{
    if (wide) {
        const uint32_t v = reinterpret_cast<const ua_u32 *>(p)->v;
        return x1 ? v & 0x00ffffffu : (v & 0xffffu) | ((v & 0xff00u) << 8);
    }
    return (uint32_t)reinterpret_cast<const ua_u16 *>(p)->v | (uint32_t)p[1 + x1] << 16;
}

// The 2x2 cell of the SUBPEL RULE's samples of a plane at integer position (ix, iy) with the fractions (fx, fy), every tap of
// non-zero weight inside the plane: row iy's two samples in the low half, row iy + 1's in the high half (as ip_cell)
__device__ __forceinline__ uint32_t si_cell(const uint8_t *img, int W, int ix, int iy, int fx, int fy)
{
    const int x1 = fx != 0, y1 = fy != 0;
    const uint8_t *p = img + (size_t)iy * W + ix;
    const bool wide = ix + 4 <= W;
    const uint32_t t0 = sc_row(p, wide, x1), t1 = sc_row(p + W, wide, x1), t2 = sc_row(p + (size_t)(1 + y1) * W, wide, x1);
    const uint32_t wx = (uint32_t)fx, wy = (uint32_t)fy;
    uint32_t h[3][2];                                         // (4 - fx) P0 + fx P1 of the three rows' two pixels, <= 1020
    h[0][0] = (4u - wx) * (t0 & 0xffu) + wx * ((t0 >> 8) & 0xffu); h[0][1] = (4u - wx) * ((t0 >> 8) & 0xffu) + wx * (t0 >> 16);
    h[1][0] = (4u - wx) * (t1 & 0xffu) + wx * ((t1 >> 8) & 0xffu); h[1][1] = (4u - wx) * ((t1 >> 8) & 0xffu) + wx * (t1 >> 16);
    h[2][0] = (4u - wx) * (t2 & 0xffu) + wx * ((t2 >> 8) & 0xffu); h[2][1] = (4u - wx) * ((t2 >> 8) & 0xffu) + wx * (t2 >> 16);
    uint32_t px = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int m = 0; m < 2; ++m) px |= (((4u - wy) * h[k][m] + wy * h[k + 1][m] + 8u) >> 4) << (16 * k + 8 * m);
    return px;
}

// A run's own four cells of a plane, cells x0 .. x0 + 3 of the cell row whose upper pixel row is oy, each as ip_cell packs it: one
// unaligned 8-byte load per pixel row when the run is whole, ip_cell for each of the n cells otherwise (the others 0).
__device__ __forceinline__ void load_cells4(const uint8_t *img, int W, int oy, int x0, int n, uint32_t (&c)[4])
{
    if (n == 4) {
        const uint8_t *p = img + (size_t)oy * W + 2 * x0;
        const ua_u32x2 t = *reinterpret_cast<const ua_u32x2 *>(p), u = *reinterpret_cast<const ua_u32x2 *>(p + W);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sh = 16 * (j & 1);
            c[j] = ((t.v[j >> 1] >> sh) & 0xffffu) | ((u.v[j >> 1] >> sh) << 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = j < n ? ip_cell(img, W, 2 * (x0 + j), oy) : 0u;
    }
}

// A run's two grey pixel rows, 8 bytes each in two dwords.  rows_put: cell j (ip_cell's packing) into them.  store_rows2: the
// rows to o and o + pitch, each as two dwords when the run is whole and the row's address dword-aligned (a caller's rows need not
// be), its 2 n bytes one by one otherwise.
__device__ __forceinline__ void rows_put(uint32_t (&rows)[2][2], int j, uint32_t px)
{
    rows[0][j >> 1] |= (px & 0xffffu) << (16 * (j & 1));
    rows[1][j >> 1] |= (px >> 16) << (16 * (j & 1));
}

__device__ __forceinline__ void store_rows2(uint8_t *o, int pitch, int n, const uint32_t (&rows)[2][2])
{
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        const uint32_t *row = rows[y];
        uint8_t *q = o + (size_t)y * pitch;
        if (n == 4 && ((uintptr_t)q & 3u) == 0) {
            reinterpret_cast<uint32_t *>(q)[0] = row[0];
            reinterpret_cast<uint32_t *>(q)[1] = row[1];
        } else {
            for (int x = 0; x < 2 * n; ++x) q[x] = (uint8_t)(row[x >> 2] >> (8 * (x & 3)));
        }
    }
}

// A run's two colour rows: 8 pixels = 24 bytes a row in three 64-bit words, cell j's six bytes B,G,R,B,G,R at bytes 6 j .. 6 j + 5
// (bit 48 j: cells 1 and 2 span two words).  The run starts at pixel (fx, fy) of the fw x fh frame and is `whole` when it has four
// cells and its 8 pixels lie inside a frame row; with an odd padding cells straddle the frame's edge.
__device__ __forceinline__ bool bgr_run_whole(int n, int fx, int fw) { return n == 4 && fx >= 0 && fx + 8 <= fw; }

// a whole run's own rows, three unaligned 8-byte loads each (a row outside the frame stays as it is)
__device__ __forceinline__ void bgr_load_rows(const uint8_t *img, int pitch, int fh, int fx, int fy, uint64_t (&rows)[2][3])
{
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        if (fy + y < 0 || fy + y >= fh) continue;
        const uint8_t *q = img + (size_t)(fy + y) * pitch + (size_t)3 * fx;
#pragma unroll
        for (int d = 0; d < 3; ++d) rows[y][d] = reinterpret_cast<const ua_u64 *>(q)[d].v;
    }
}

// cell j's six bytes of a row, from bit 0 up
__device__ __forceinline__ uint64_t bgr_row_get(const uint64_t (&row)[3], int j)
{
    const int bit = 48 * j, wd = bit >> 6, sh = bit & 63;
    uint64_t v = row[wd] >> sh;
    if (sh > 16) v |= row[wd + 1] << (64 - sh);
    return v & 0xffffffffffffull;
}

// six bytes into cell j's place of a row that holds 0 there
__device__ __forceinline__ void bgr_row_put(uint64_t (&row)[3], int j, uint64_t px)
{
    const int bit = 48 * j, wd = bit >> 6, sh = bit & 63;
    row[wd] |= px << sh;
    if (sh > 16) row[wd + 1] |= px >> (64 - sh);
}

// The rows to the unpadded frame (rows `pitch` bytes apart): six dwords a row when the run is whole and the row's address
// dword-aligned (an odd pad_x or a caller's odd pitch breaks that), otherwise byte by byte the pixels of the run's n cells that lie
// inside the frame.  Rows outside the frame are not written.  `whole` is bgr_run_whole's answer: the
// filters hold it for their loads, and found again in here it costs K9b a VGPR (57 against the parent's 56).
__device__ __forceinline__ void bgr_store_rows(uint8_t *frame, int pitch, int fw, int fh, int fx, int fy, int n, bool whole,
                                               const uint64_t (&rows)[2][3])
{
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        if (fy + y < 0 || fy + y >= fh) continue;
        uint8_t *q = frame + (size_t)(fy + y) * pitch + (ptrdiff_t)3 * fx;
        if (whole && ((uintptr_t)q & 3u) == 0) {
            uint32_t *o = reinterpret_cast<uint32_t *>(q);
#pragma unroll
            for (int d = 0; d < 6; ++d) o[d] = (uint32_t)(rows[y][d >> 1] >> (32 * (d & 1)));
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                if (p >= 2 * n || fx + p < 0 || fx + p >= fw) continue;
#pragma unroll
                for (int k = 3 * p; k < 3 * p + 3; ++k) q[k] = (uint8_t)(rows[y][k >> 3] >> (8 * (k & 7)));
            }
        }
    }
}

// A one-row run of 4 colour pixels: 12 bytes in three dwords, pixel j's B,G,R at bytes 3 j .. 3 j + 2 (bit 24 j: pixels 1 and 2
// span two dwords).  bgr_run_put: three bytes into pixel j's place of a run that holds 0 there.  bgr_store_run: the run's n
// pixels to q, three dwords when the run is whole and q dword-aligned (an odd pitch or a caller's odd base breaks that), byte
// by byte otherwise.
__device__ __forceinline__ void bgr_run_put(uint32_t (&run)[3], int j, uint32_t px)
{
    const int bit = 24 * j, wd = bit >> 5, sh = bit & 31;
    run[wd] |= px << sh;
    if (sh > 8) run[wd + 1] |= px >> (32 - sh);
}

__device__ __forceinline__ void bgr_store_run(uint8_t *q, int n, const uint32_t (&run)[3])
{
    if (n == 4 && ((uintptr_t)q & 3u) == 0) {
        uint32_t *o = reinterpret_cast<uint32_t *>(q);
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = run[d];
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) q[k] = (uint8_t)(run[k >> 2] >> (8 * (k & 3)));
    }
}

// The temporal filters' head: frame (y, z) = blockIdx.y / z of a launch reads every input at base + y s_y + z s_z (bytes for
// planes, words for grids).  Along z the first frame has its previous neighbour only with first_prev and the last its next one only
// with last_next, so that one launch serves the frames of a chain (z = slot) as well as the 2 frames of every pair of a batch
// (z = which).  A neighbour that is absent has null pointers.
struct TfFrame { const uint8_t *C, *P, *N; const mv_t *GP, *GN; bool has_p, has_n; };

template <class Args>
__device__ __forceinline__ TfFrame tf_frame(const Args &a)
{
    const long long y = blockIdx.y, z = blockIdx.z;
    TfFrame f;
    f.C = a.cur + y * a.cur_y + z * a.cur_z;
    f.has_p = a.prev && (z > 0 || a.first_prev);
    f.has_n = a.next && (z + 1 < (long long)gridDim.z || a.last_next);
    f.P = f.has_p ? a.prev + y * a.prev_y + z * a.prev_z : nullptr;
    f.N = f.has_n ? a.next + y * a.next_y + z * a.next_z : nullptr;
    f.GP = f.has_p ? a.gp + y * a.gp_y + z * a.gp_z : nullptr;
    f.GN = f.has_n ? a.gn + y * a.gn_y + z * a.gn_z : nullptr;
    return f;
}

// The temporal filters' weight tail: w = 8 (thr - cost) / thr for a cost below thr, 0 otherwise.  The division is a multiply-shift
// (see K9); cost 0 is weight 8 at every thr and all that passes at thr = 1, which has no 32-bit magic, so it is answered without it.
__device__ __forceinline__ uint32_t tf_cost_weight(uint32_t cost, uint32_t thr, uint32_t magic_thr)
{
    if (cost >= thr) return 0u;
    return cost ? __umulhi(8u * (thr - cost), magic_thr) : 8u;
}

// Statistics tail: the lane's four counters summed over its wave, the four waves' sums over the workgroup through `part`, and
// the workgroup's four 64-bit sums stored as the partial of (frame, workgroup) at word 4 (frame gridDim.x + blockIdx.x), for
// k_mc_reduce to add up.  (64-bit atomics into the frame's four words instead: the 2040 workgroups of a 4K plane queue on that
// one cache line, 34 us against 11 us for the same pass writing the frame.)  A wave's 32-bit sums must not overflow: every
// kernel says why its own do not.  `part` is the kernel's: __shared__ inside a helper would be a module-level LDS variable.
__device__ __forceinline__ void store_partial4(unsigned long long *partial, size_t frame, uint32_t (&part)[4][4], uint32_t s0,
                                               uint32_t s1, uint32_t s2, uint32_t s3)
{
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
        s3 += __shfl_xor(s3, o);
    }
    if ((threadIdx.x & 63) == 0) {
        uint32_t *w = part[threadIdx.x >> 6];
        w[0] = s0; w[1] = s1; w[2] = s2; w[3] = s3;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        partial[4 * (frame * gridDim.x + blockIdx.x) + threadIdx.x] =
            (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// =======================================================================================
// MF::draw_MVimage (motion_framework.cpp:887-905) fused with the residual statistics of the compensated frame against
// image1.  b-block (X, Y) = (bx b, by b) takes its MV from grid[Y >> lcb][X >> lcb] (the current grid, cur_block =
// 1 << lcb >= 2) and copies the b x b block of image2 at (X + dx, Y + dy) when that lies inside the plane; a skipped
// block's pixels get `fill`.  A lane takes a run of 4 pixels along x: with b >= 4 the run lies in one block (one grid
// read, one unaligned dword of image2); with b = 2 each half of the run is one block (an unaligned u16 each); with b = 1
// both pixels of a half share a grid cell.  image1 is read (as a dword) only when statistics are asked for.
// Statistics over the window [wx0, wx1) x [wy0, wy1): sse, sad and pixels over compensated pixels, skipped over the
// others.  A lane sums at most kMcRunsPerLane runs in 32 bits and a wave's sum stays below 2^32
// (64 * 4 * 4 * 255^2).  Run split, output store and statistics tail are the shared ones (gather_index / gather_split,
// store_bytes4, store_partial4 with frame = pair) but written out here: through the first and the last this kernel takes 4 more
// SGPRs and 2 more VGPRs, and with store_bytes4 alone its frame-and-statistics pass measured 0.8 % above the written-out text.
// Batch: blockIdx.y = pair (planes plane_stride bytes, grids grid_stride words apart); `out` only with one pair per launch.
// =======================================================================================
struct McArgs {
    const uint8_t *img1, *img2;           // the level's padded planes, pitch = width
    const mv_t *grid;                     // current grid: gcols entries per row
    uint8_t *out;                         // compensated plane (rows out_pitch bytes apart), or null
    unsigned long long *partial;          // per pair and workgroup {sse, sad, pixels, skipped}; or null (no statistics)
    uint32_t plane_stride, grid_stride;
    int width, height, gcols, lcb, lb, fill, out_pitch;
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(width / 4)
    long long runs;                       // runs_per_row * height
};

constexpr int kMcRunsPerLane = 4;

__global__ __launch_bounds__(256) void k_motion_compensate(McArgs a)
{
    const size_t pair = blockIdx.y;
    const uint8_t *img1 = a.img1 + pair * a.plane_stride, *img2 = a.img2 + pair * a.plane_stride;
    const mv_t *grid = a.grid + pair * a.grid_stride;
    const int W = a.width, H = a.height, b = 1 << a.lb;
    uint32_t sse = 0, sad = 0, npix = 0, nskip = 0;
#pragma unroll
    for (int k = 0; k < kMcRunsPerLane; ++k) {
        const long long i = ((long long)blockIdx.x * kMcRunsPerLane + k) * 256 + threadIdx.x;
        if (i >= a.runs) break;
        const int y = (int)(i / a.runs_per_row), x0 = (int)(i % a.runs_per_row) * 4;
        const int Y = y & ~(b - 1), grow = (Y >> a.lcb) * a.gcols, iy = y - Y;
        const int n = min(4, W - x0);                         // pixels of the run inside the row
        uint32_t mc = 0, ok = 0;                              // gathered bytes; bit j: pixel x0 + j was compensated
        if (b >= 4 && n == 4) {
            const int X = x0 & ~(b - 1);
            const mv_t m = grid[grow + (X >> a.lcb)];
            const int sx = X + mv_x(m), sy = Y + mv_y(m);
            if (sx >= 0 && sx <= W - b && sy >= 0 && sy <= H - b) {
                mc = reinterpret_cast<const ua_u32 *>(img2 + (size_t)(sy + iy) * W + sx + (x0 - X))->v;
                ok = 0xfu;
            }
        } else {
            for (int h = 0; h < 2; ++h) {
                const int xh = x0 + 2 * h;
                if (xh >= W) break;
                const mv_t m = grid[grow + ((xh & ~(b - 1)) >> a.lcb)];
                const int dx = mv_x(m), sy = Y + mv_y(m);
                if (sy < 0 || sy > H - b) continue;
                const uint8_t *row = img2 + (size_t)(sy + iy) * W;
                if (b == 2 && xh + 2 <= W) {
                    const int sx = xh + dx;
                    if (sx >= 0 && sx <= W - 2) {
                        mc |= (uint32_t)reinterpret_cast<const ua_u16 *>(row + sx)->v << (16 * h);
                        ok |= 3u << (2 * h);
                    }
                } else {
                    for (int j = 2 * h; j < 2 * h + 2 && j < n; ++j) {
                        const int X = (x0 + j) & ~(b - 1), sx = X + dx;
                        if (sx >= 0 && sx <= W - b) { mc |= (uint32_t)row[sx + (x0 + j - X)] << (8 * j); ok |= 1u << j; }
                    }
                }
            }
        }
        if (a.out) {
            uint32_t keep = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) keep |= ((ok >> j) & 1u) ? 0xffu << (8 * j) : 0u;
            const uint32_t v = (mc & keep) | ((uint32_t)a.fill * 0x01010101u & ~keep);
            uint8_t *o = a.out + (size_t)y * a.out_pitch + x0;
            if (n == 4 && ((uintptr_t)o & 3u) == 0) *reinterpret_cast<uint32_t *>(o) = v;
            else for (int j = 0; j < n; ++j) o[j] = (uint8_t)(v >> (8 * j));
        }
        if (a.partial && y >= a.wy0 && y < a.wy1) {
            const uint8_t *r1 = img1 + (size_t)y * W + x0;
            uint32_t ref = 0;
            if (n == 4) ref = reinterpret_cast<const ua_u32 *>(r1)->v;
            else for (int j = 0; j < n; ++j) ref |= (uint32_t)r1[j] << (8 * j);
            for (int j = 0; j < n; ++j) {
                if (x0 + j < a.wx0 || x0 + j >= a.wx1) continue;
                if ((ok >> j) & 1u) {
                    const int d = (int)((mc >> (8 * j)) & 0xffu) - (int)((ref >> (8 * j)) & 0xffu);
                    sse += (uint32_t)(d * d);
                    sad += (uint32_t)abs(d);
                    ++npix;
                } else {
                    ++nskip;
                }
            }
        }
    }
    if (!a.partial) return;
    for (int o = 32; o > 0; o >>= 1) {
        sse += __shfl_xor(sse, o);
        sad += __shfl_xor(sad, o);
        npix += __shfl_xor(npix, o);
        nskip += __shfl_xor(nskip, o);
    }
    __shared__ uint32_t part[4][4];
    if ((threadIdx.x & 63) == 0) {
        uint32_t *w = part[threadIdx.x >> 6];
        w[0] = sse; w[1] = sad; w[2] = npix; w[3] = nskip;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        a.partial[4 * (pair * gridDim.x + blockIdx.x) + threadIdx.x] =
            (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// One workgroup per pair (blockIdx.x): the `groups` partials of k_motion_compensate into the pair's four words of `out`.
__global__ __launch_bounds__(256) void k_mc_reduce(const unsigned long long *partial, int groups, unsigned long long *out)
{
    const ulonglong2 *p = reinterpret_cast<const ulonglong2 *>(partial + (size_t)4 * groups * blockIdx.x);
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int g = threadIdx.x; g < groups; g += 256) {
        const ulonglong2 lo = p[2 * g], hi = p[2 * g + 1];
        s[0] += lo.x; s[1] += lo.y; s[2] += hi.x; s[3] += hi.y;
    }
    __shared__ unsigned long long red[4][256];
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 4) out[4 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

// =======================================================================================
// K6.  Forward-backward consistency of two 2x2-cell grids (the rule of include/bbme.h): cell (cx, cy) of A with (dx, dy) looks
// at pixel (tx, ty) = (2 cx + dx, 2 cy + dy); outside the 2 CW x 2 CH plane it is class 2, otherwise (ex, ey) =
// B[ty >> 1][tx >> 1], d = |dx + ex| + |dy + ey| and the class is d > tol.  A lane takes a run of 4 consecutive cells of one
// row (the last run of a row holds 2 cells when CW is not a multiple of 4), A arrives as one 16-byte load and the mask leaves as
// one dword; the four reads of B are 4-byte gathers near the lane's own position (fields are piecewise smooth) and are left to L2.
// Statistics over the window [wx0, wx1) x [wy0, wy1) in cells: cells of class 0, 1, 2 and the sum of d over classes 0 and
// 1.  A lane holds at most 4 kFbRunsPerLane = 16 cells, so a wave's 32-bit sum of d stays below 16 * 64 * 131 070 < 2^27.
// Run split, grid words, mask store and statistics tail are the shared ones (gather_index / gather_split, load_mv4, store_bytes4,
// store_partial4 with frame = pair) but written out here: through the helpers the registers stay as they are, but the launches
// with statistics measured 1.3 to 4.3 % above the written-out text.  blockIdx.y = pair; mask and partial are each optional.
// =======================================================================================
struct FbArgs {
    const mv_t *a, *b;                    // cw entries per row, ch rows
    uint8_t *mask;                        // one class byte per cell, rows mask_pitch bytes apart; or null
    unsigned long long *partial;          // per pair and workgroup {consistent, inconsistent, outside, discrepancy}; or null
    uint32_t s_a, s_b;                    // words from pair to pair
    size_t s_mask;                        // bytes from pair to pair
    int cw, ch, tol, mask_pitch;
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

constexpr int kFbRunsPerLane = 4;

__global__ __launch_bounds__(256) void k_fb_consistency(FbArgs a)
{
    const size_t pair = blockIdx.y;
    const mv_t *A = a.a + pair * a.s_a, *B = a.b + pair * a.s_b;
    const int CW = a.cw, PW = 2 * a.cw, PH = 2 * a.ch;
    uint32_t n0 = 0, n1 = 0, n2 = 0, dsum = 0;
#pragma unroll
    for (int k = 0; k < kFbRunsPerLane; ++k) {
        const long long i = ((long long)blockIdx.x * kFbRunsPerLane + k) * 256 + threadIdx.x;
        if (i >= a.runs) break;
        const int cy = (int)(i / a.runs_per_row), x0 = (int)(i % a.runs_per_row) * 4;
        const int n = min(4, CW - x0);                        // cells of the run inside the row (4, or 2 at the row's end)
        const mv_t *src = A + (size_t)cy * CW + x0;
        uint32_t m[4] = {0, 0, 0, 0};
        if (n == 4) {
            const ua_u32x4 v = *reinterpret_cast<const ua_u32x4 *>(src);
            m[0] = v.v[0]; m[1] = v.v[1]; m[2] = v.v[2]; m[3] = v.v[3];
        } else {
            m[0] = src[0];
            if (n > 1) m[1] = src[1];
            if (n > 2) m[2] = src[2];
        }
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint32_t cls = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int dx = mv_x(m[j]), dy = mv_y(m[j]);
            const int tx = 2 * (x0 + j) + dx, ty = 2 * cy + dy;
            uint32_t c = 2u, d = 0;
            if (tx >= 0 && ty >= 0 && tx < PW && ty < PH) {
                const mv_t e = B[(size_t)(ty >> 1) * CW + (tx >> 1)];
                d = (uint32_t)(abs(dx + mv_x(e)) + abs(dy + mv_y(e)));
                c = d > (uint32_t)a.tol ? 1u : 0u;
            }
            cls |= c << (8 * j);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                n0 += c == 0u; n1 += c == 1u; n2 += c == 2u;
                dsum += d;
            }
        }
        if (a.mask) {
            uint8_t *o = a.mask + pair * a.s_mask + (size_t)cy * a.mask_pitch + x0;
            if (n == 4 && ((uintptr_t)o & 3u) == 0) *reinterpret_cast<uint32_t *>(o) = cls;
            else for (int j = 0; j < n; ++j) o[j] = (uint8_t)(cls >> (8 * j));
        }
    }
    if (!a.partial) return;
    for (int o = 32; o > 0; o >>= 1) {
        n0 += __shfl_xor(n0, o);
        n1 += __shfl_xor(n1, o);
        n2 += __shfl_xor(n2, o);
        dsum += __shfl_xor(dsum, o);
    }
    __shared__ uint32_t part[4][4];
    if ((threadIdx.x & 63) == 0) {
        uint32_t *w = part[threadIdx.x >> 6];
        w[0] = n0; w[1] = n1; w[2] = n2; w[3] = dsum;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        a.partial[4 * (pair * gridDim.x + blockIdx.x) + threadIdx.x] =
            (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// =======================================================================================
// K7.  Motion-compensated interpolation at phase num / den from the level-0 planes and the two 2x2-cell grids (the rule of
// include/bbme.h): output cell (cx, cy) tries v = F[cy][cx], v = -B[cy][cx] (when B is given) and v = 0; a hypothesis reads
// the 2x2 cell of I1 at p1 = origin - round(num v / den) and the one of I2 at p2 = p1 + v, is valid when both lie inside the
// plane, and costs their SAD; the cheapest valid one (the earliest of equals) is blended, ((den - num) I1 + num I2 +
// den / 2) / den.  A memory-bound gather: a lane takes a run of 4 consecutive cells of one cell row (fewer at the row's
// end), so that F and B arrive as one 16-byte load each and the zero hypothesis as one 8-byte load per plane row
// (load_cells4's text, kept in ip_load_run); the moved cells are unaligned u16 loads, two per cell and plane, packed into one dword per cell (ip_cell) so
// that v_sad_u8 gives the cost in one instruction.  A lane writes its two output rows by store_rows2 and its selections as one
// dword.
// Divisions by den are multiply-shifts: with magic = floor(2^32 / den) + 1 = (2^32 + e) / den, 0 < e <= den,
// umulhi(n, magic) = floor(n / den) for every n with n e < 2^32.  The blend's numerators stay below 255 * 256 + 128 and the
// shifts', moved to n >= 0 by 32768 den (|num v| < 32768 den), below 2^24, and e <= 256.
// blockIdx.y = pair (planes plane_stride bytes, grids s_f / s_b words apart), blockIdx.z = phase num0 + z (frames out_stride,
// maps sel_stride bytes apart): the planes and grids of one pair are read from L2 by every phase but the first.  `out` and
// `sel` only with one pair per launch.  Statistics over the window [wx0, wx1) x [wy0, wy1) in cells: cells that selected
// k = 0, 1, 2 and the sum of the selected costs; a lane holds at most 4 kIpRunsPerLane cells of cost <= 1020.  The selection map
// leaves by store_bytes4.  Run split, grid words (ip_load_run) and statistics tail are the shared ones (gather_index /
// gather_split, load_mv4, store_partial4 with frame = (phase, pair)) but written out here: through the helpers this kernel or
// k_interpolate_bgr, which shares ip_load_run, takes one more VGPR.
// =======================================================================================
// what k_interpolate and k_interpolate_bgr both take
struct IpCommon {
    const uint8_t *img1, *img2;           // level-0 padded (luma) planes, pitch = width
    const mv_t *fwd, *bwd;                // cw entries per row, height / 2 rows; bwd may be null
    uint8_t *out;                         // frames (rows out_pitch, phases out_stride bytes apart), or null
    size_t out_stride;
    int width, height, cw, num0, den, out_pitch;
    uint32_t magic;                       // floor(2^32 / den) + 1
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * height / 2
};

struct IpArgs : IpCommon {
    uint8_t *sel;                         // one byte k per cell (rows sel_pitch, phases sel_stride bytes apart), or null
    unsigned long long *partial;          // per (phase, pair) and workgroup {k = 0, k = 1, k = 2, cost}; or null
    uint32_t plane_stride, s_f, s_b;
    size_t sel_stride;
    int ch, sel_pitch;
    int wx0, wy0, wx1, wy1;
};

constexpr int kIpRunsPerLane = 2;

// One run of a cell row, cells x0 .. x0 + n - 1 (n = 1..4) of row cy: the grids' entries and the cells of the zero hypothesis
struct IpRun { uint32_t f[4], b[4], z1[4], z2[4]; };

__device__ __forceinline__ IpRun ip_load_run(const uint8_t *img1, const uint8_t *img2, const mv_t *F, const mv_t *B, int W, int CW,
                                             int cy, int x0, int n)
{
    IpRun r;                                                  // load_cells4's text, written out: through it K7b takes 43 VGPRs, not 42
    const int oy = 2 * cy;
    const size_t g0 = (size_t)cy * CW + x0, o0 = (size_t)oy * W + 2 * x0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.f[j] = r.b[j] = 0;
    if (n == 4) {
        const ua_u32x4 v = *reinterpret_cast<const ua_u32x4 *>(F + g0);
        r.f[0] = v.v[0]; r.f[1] = v.v[1]; r.f[2] = v.v[2]; r.f[3] = v.v[3];
        if (B) {
            const ua_u32x4 u = *reinterpret_cast<const ua_u32x4 *>(B + g0);
            r.b[0] = u.v[0]; r.b[1] = u.v[1]; r.b[2] = u.v[2]; r.b[3] = u.v[3];
        }
        const ua_u32x2 t1 = *reinterpret_cast<const ua_u32x2 *>(img1 + o0), u1 = *reinterpret_cast<const ua_u32x2 *>(img1 + o0 + W);
        const ua_u32x2 t2 = *reinterpret_cast<const ua_u32x2 *>(img2 + o0), u2 = *reinterpret_cast<const ua_u32x2 *>(img2 + o0 + W);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sh = 16 * (j & 1);
            r.z1[j] = ((t1.v[j >> 1] >> sh) & 0xffffu) | ((u1.v[j >> 1] >> sh) << 16);
            r.z2[j] = ((t2.v[j >> 1] >> sh) & 0xffffu) | ((u2.v[j >> 1] >> sh) << 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r.z1[j] = r.z2[j] = 0;
            if (j >= n) continue;
            r.f[j] = F[g0 + j];
            if (B) r.b[j] = B[g0 + j];
            r.z1[j] = ip_cell(img1, W, 2 * (x0 + j), oy);
            r.z2[j] = ip_cell(img2, W, 2 * (x0 + j), oy);
        }
    }
    return r;
}

// What the cell with origin (ox, oy) selects: hypothesis k and its cost, its two cells c1 (of I1 at p1) and c2 (of I2 at
// p2 = p1 + v).  Shared by k_interpolate, which blends the cells, and k_interpolate_bgr, which gathers colour at p1 and p2.
struct IpPick { uint32_t c1, c2, k, cost; int p1x, p1y, vx, vy; };

__device__ __forceinline__ IpPick ip_select(const uint8_t *img1, const uint8_t *img2, int W, int H, int ox, int oy, uint32_t f,
                                            uint32_t b, bool has_b, uint32_t z1, uint32_t z2, int num, int half, int bias,
                                            uint32_t magic)
{
    IpPick s{0u, 0u, 2u, ~0u, ox, oy, 0, 0};                  // nothing selected yet
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1 && !has_b) break;
        const int vx = h ? -mv_x(b) : mv_x(f), vy = h ? -mv_y(b) : mv_y(f);
        const int sx = (int)__umulhi((uint32_t)(num * vx + half + bias), magic) - 32768;
        const int sy = (int)__umulhi((uint32_t)(num * vy + half + bias), magic) - 32768;
        const int p1x = ox - sx, p1y = oy - sy, p2x = p1x + vx, p2y = p1y + vy;
        if (p1x < 0 || p2x < 0 || p1x > W - 2 || p2x > W - 2 || p1y < 0 || p2y < 0 || p1y > H - 2 || p2y > H - 2) continue;
        const uint32_t q1 = ip_cell(img1, W, p1x, p1y), q2 = ip_cell(img2, W, p2x, p2y);
        const uint32_t c = __builtin_amdgcn_sad_u8(q1, q2, 0u);
        if (c < s.cost) s = IpPick{q1, q2, (uint32_t)h, c, p1x, p1y, vx, vy};      // strictly cheaper: the earliest of equals stays
    }
    const uint32_t cz = __builtin_amdgcn_sad_u8(z1, z2, 0u);
    if (cz < s.cost) s = IpPick{z1, z2, 2u, cz, ox, oy, 0, 0};
    return s;
}

__global__ __launch_bounds__(256) void k_interpolate(IpArgs a)
{
    const size_t pair = blockIdx.y;
    const uint8_t *img1 = a.img1 + pair * a.plane_stride, *img2 = a.img2 + pair * a.plane_stride;
    const mv_t *F = a.fwd + pair * a.s_f, *B = a.bwd ? a.bwd + pair * a.s_b : nullptr;
    const int W = a.width, H = a.height, CW = a.cw, den = a.den, num = a.num0 + (int)blockIdx.z, half = den >> 1;
    const uint32_t magic = a.magic, w1 = (uint32_t)(den - num), w2 = (uint32_t)num;
    const int bias = 32768 * den;
    uint32_t n0 = 0, n1 = 0, n2 = 0, csum = 0;
#pragma unroll
    for (int r = 0; r < kIpRunsPerLane; ++r) {
        const long long i = ((long long)blockIdx.x * kIpRunsPerLane + r) * 256 + threadIdx.x;
        if (i >= a.runs) break;
        const int cy = (int)(i / a.runs_per_row), x0 = (int)(i % a.runs_per_row) * 4;
        const int n = min(4, CW - x0);                        // cells of the run inside the row
        const int oy = 2 * cy;
        const IpRun run = ip_load_run(img1, img2, F, B, W, CW, cy, x0, n);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint32_t rows[2][2] = {{0, 0}, {0, 0}}, ks = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ox = 2 * (x0 + j);
            const IpPick s = ip_select(img1, img2, W, H, ox, oy, run.f[j], run.b[j], B != nullptr, run.z1[j], run.z2[j], num, half,
                                       bias, magic);
            const uint32_t c1 = s.c1, c2 = s.c2, k = s.k, cost = s.cost;
            uint32_t px = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t v = __umulhi(w1 * ((c1 >> (8 * q)) & 0xffu) + w2 * ((c2 >> (8 * q)) & 0xffu) + (uint32_t)half, magic);
                px |= v << (8 * q);
            }
            rows_put(rows, j, px);
            ks |= k << (8 * j);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                n0 += k == 0u; n1 += k == 1u; n2 += k == 2u;
                csum += cost;
            }
        }
        if (a.out) store_rows2(a.out + blockIdx.z * a.out_stride + (size_t)oy * a.out_pitch + 2 * x0, a.out_pitch, n, rows);
        if (a.sel) store_bytes4(a.sel + blockIdx.z * a.sel_stride + (size_t)cy * a.sel_pitch + x0, n, ks);
    }
    if (!a.partial) return;
    for (int o = 32; o > 0; o >>= 1) {
        n0 += __shfl_xor(n0, o);
        n1 += __shfl_xor(n1, o);
        n2 += __shfl_xor(n2, o);
        csum += __shfl_xor(csum, o);
    }
    __shared__ uint32_t part[4][4];
    if ((threadIdx.x & 63) == 0) {
        uint32_t *w = part[threadIdx.x >> 6];
        w[0] = n0; w[1] = n1; w[2] = n2; w[3] = csum;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        a.partial[4 * (((size_t)blockIdx.z * gridDim.y + pair) * gridDim.x + blockIdx.x) + threadIdx.x] =
            (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// =======================================================================================
// K7b.  The BGR interpolation rule of include/bbme.h: k_interpolate's selection on the LUMA planes (ip_load_run, ip_select: the same
// loads, multiply-shifts and v_sad_u8), then the blend of the two B,G,R frames at the selected p1 and p2, written as the
// unpadded frame.  Same split as k_interpolate -- a lane takes a run of 4 cells, blockIdx.z = phase, so every phase but the
// first finds planes, grids and colour in L2 -- and the same kind of kernel, a memory-bound gather with three times the pixel
// bytes: per cell and frame two rows of two pixels, 6 contiguous bytes each, as one unaligned dword and one u16 load where both
// pixels lie inside the frame, by bytes (0 outside) where they straddle its edge.  A run's output row is 8 pixels = 24 bytes,
// collected by bgr_row_put and stored by bgr_store_rows.  Runs wholly outside the frame load nothing.
// =======================================================================================
struct IpBgrArgs : IpCommon {           // out: the fw x fh B,G,R frames
    const uint8_t *bgr1, *bgr2;           // the fw x fh colour frames, rows bgr_pitch bytes apart
    int fw, fh, pad_x, pad_y, bgr_pitch;
};

// pixels (x, y) and (x + 1, y) of a colour frame as six bytes B,G,R,B,G,R from bit 0 up; a pixel outside the frame is 0
__device__ __forceinline__ uint64_t bgr_two(const uint8_t *img, int pitch, int fw, int fh, int x, int y)
{
    if (y < 0 || y >= fh || x < -1 || x >= fw) return 0;
    const uint8_t *row = img + (size_t)y * pitch;
    if (x >= 0 && x + 1 < fw)
        return (uint64_t)reinterpret_cast<const ua_u32 *>(row + 3 * x)->v | (uint64_t)reinterpret_cast<const ua_u16 *>(row + 3 * x + 4)->v << 32;
    const int px = x < 0 ? 0 : x;                             // the one pixel inside: the second of the two (x = -1) or the first
    const uint64_t v = (uint64_t)row[3 * px] | (uint64_t)row[3 * px + 1] << 8 | (uint64_t)row[3 * px + 2] << 16;
    return x < 0 ? v << 24 : v;
}

__global__ __launch_bounds__(256) void k_interpolate_bgr(IpBgrArgs a)
{
    const mv_t *F = a.fwd, *B = a.bwd;
    const int W = a.width, H = a.height, CW = a.cw, den = a.den, num = a.num0 + (int)blockIdx.z, half = den >> 1;
    const uint32_t magic = a.magic, w1 = (uint32_t)(den - num), w2 = (uint32_t)num;
    const int bias = 32768 * den;
#pragma unroll
    for (int r = 0; r < kIpRunsPerLane; ++r) {
        const long long i = ((long long)blockIdx.x * kIpRunsPerLane + r) * 256 + threadIdx.x;
        if (i >= a.runs) break;
        const int cy = (int)(i / a.runs_per_row), x0 = (int)(i % a.runs_per_row) * 4;
        const int n = min(4, CW - x0);                        // cells of the run inside the row
        const int oy = 2 * cy;
        const int fy = oy - a.pad_y, fx = 2 * x0 - a.pad_x;    // the run's first pixel in frame coordinates
        if (fy + 1 < 0 || fy >= a.fh || fx + 2 * n <= 0 || fx >= a.fw) continue;      // no pixel of the run is in the frame
        const IpRun run = ip_load_run(a.img1, a.img2, F, B, W, CW, cy, x0, n);
        uint64_t rows[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's two output rows, 24 bytes each
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const IpPick s = ip_select(a.img1, a.img2, W, H, 2 * (x0 + j), oy, run.f[j], run.b[j], B != nullptr, run.z1[j], run.z2[j],
                                       num, half, bias, magic);
            const int q1x = s.p1x - a.pad_x, q1y = s.p1y - a.pad_y, q2x = q1x + s.vx, q2y = q1y + s.vy;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const uint64_t c1 = bgr_two(a.bgr1, a.bgr_pitch, a.fw, a.fh, q1x, q1y + y);
                const uint64_t c2 = bgr_two(a.bgr2, a.bgr_pitch, a.fw, a.fh, q2x, q2y + y);
                uint64_t px = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const uint32_t v = __umulhi(w1 * ((uint32_t)(c1 >> (8 * q)) & 0xffu) + w2 * ((uint32_t)(c2 >> (8 * q)) & 0xffu) +
                                                (uint32_t)half, magic);
                    px |= (uint64_t)v << (8 * q);
                }
                bgr_row_put(rows[y], j, px);
            }
        }
        bgr_store_rows(a.out + blockIdx.z * a.out_stride, a.out_pitch, a.fw, a.fh, fx, fy, n, bgr_run_whole(n, fx, a.fw), rows);
    }
}

// =======================================================================================
// K9.  Motion-compensated temporal filter of a frame C with its previous frame P and / or its next frame N (the TEMPORAL FILTER
// RULE of include/bbme.h): output cell (cx, cy) with origin o reads, for each present neighbour X with grid G on C, the 2x2 cell
// of X at p = o + G[cy][cx]; inside the plane and with cost = SAD(C cell, X cell) < thr it gets the weight w = 8 (thr - cost) /
// thr (0..8), otherwise 0, and out = (8 C + wP P + wN N + S / 2) / S with S = 8 + wP + wN.
// K9 and K13 are one body, tf_body<SUBPEL, RPL>: K13 differs in how a neighbour's cell is taken (tf_weight<SUBPEL>) and in the
// row pitch of its grids.  The shared split of runs of 4 cells (gather_index / gather_split): GP and GN arrive by load_mv4 and C by
// load_cells4; each moved cell is one dword (ip_cell: two unaligned u16 loads; si_cell: rounded samples), so that v_sad_u8 gives
// the cost -- and, on the finished cell, |out - C| -- in one instruction.  A lane writes its two output rows by store_rows2 and its
// four weight bytes wP | wN << 4 by store_bytes4.
// Both divisions are multiply-shifts by k_interpolate's argument: with magic = floor(2^32 / d) + 1 = (2^32 + e) / d, 0 < e <= d,
// umulhi(n, magic) = floor(n / d) for every n with n e < 2^32.  By thr (tf_cost_weight): n = 8 (thr - cost) <= 8 * 1021 and
// e <= 1021, n e < 2^23 (thr = 1 has no 32-bit magic, 2^32 + 1: there only cost 0 passes, and cost 0 is answered without the
// division).  By S: n <= 255 * 24 + 12 and e <= 24, n e < 2^18; S is the lane's own, so the 17 magics of S = 8..24 come with the
// arguments and are read from LDS.  The bounds hold for every sampling: a cell is four bytes, rounded samples included, so the
// cost is at most 1020 and the blend's numerator at most 255 * 24 + 12.
// blockIdx.y = batch pair, blockIdx.z = the frame of a run (tf_frame); frames lie out_stride bytes apart along z and need
// gridDim.y = 1; the map only with one frame per launch.  Statistics over the window [wx0, wx1) x [wy0, wy1) in cells: cells with
// wP > 0, cells with wN > 0, the sum of wP + wN and the sum of |out - C| over the cells' pixels; a lane holds at most 4 RPL cells
// of at most 1020 each (store_partial4, frame = y gridDim.z + z, then k_mc_reduce: no atomics).
// __shared__ arrays are the kernels' and come in as arguments: inside the body they would be module-level LDS variables.
// =======================================================================================
struct TfArgs {
    const uint8_t *cur, *prev, *next;     // level-0 padded planes, pitch = width; prev / next null = no such neighbour at all
    const mv_t *gp, *gn;                  // cw entries per row, ch rows: on C, into P and into N
    uint8_t *out;                         // frames (rows out_pitch, frames out_stride bytes apart), or null
    uint8_t *wmap;                        // one byte wP | wN << 4 per cell (rows wmap_pitch bytes apart; one-frame launches only), or null
    unsigned long long *partial;          // per frame and workgroup {cells wP > 0, cells wN > 0, weights, |out - C|}; or null
    long long cur_y, cur_z, prev_y, prev_z, next_y, next_z;      // bytes from pair to pair and from frame to frame
    long long gp_y, gp_z, gn_y, gn_z;                            // words
    size_t out_stride;
    int width, height, cw, ch, thr, out_pitch, wmap_pitch;
    int first_prev, last_next;
    uint32_t magic_thr;                   // floor(2^32 / thr) + 1; not used at thr = 1
    uint32_t magic_s[17];                 // floor(2^32 / S) + 1 for S = 8..24
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

constexpr int kTfRunsPerLane = 2;

// One neighbour of the cell c with origin (ox, oy): its weight, and its cell in *q when the weight is not 0.  g is in pixels and
// the cell ip_cell's; with SUBPEL g is in quarter pels, the cell lies at o + (g >> 2) with the fractions g & 3, is valid when
// every tap of non-zero weight lies in the plane, and holds the SUBPEL RULE's four rounded bilinear samples (si_cell, which never
// addresses a tap of weight 0).
template <bool SUBPEL>
__device__ __forceinline__ uint32_t tf_weight(const uint8_t *X, int W, int H, int ox, int oy, mv_t g, uint32_t c, uint32_t thr,
                                              uint32_t magic_thr, uint32_t *q)
{
    const int gx = mv_x(g), gy = mv_y(g);
    const int fx = SUBPEL ? gx & 3 : 0, fy = SUBPEL ? gy & 3 : 0;
    const int sx = ox + (SUBPEL ? gx >> 2 : gx), sy = oy + (SUBPEL ? gy >> 2 : gy);
    *q = 0;
    if (sx < 0 || sy < 0 || sx + 2 + (fx != 0) > W || sy + 2 + (fy != 0) > H) return 0u;
    uint32_t x;
    if constexpr (SUBPEL) x = si_cell(X, W, sx, sy, fx, fy);
    else x = ip_cell(X, W, sx, sy);
    const uint32_t cost = __builtin_amdgcn_sad_u8(c, x, 0u);
    if (cost < thr) *q = x;
    return tf_cost_weight(cost, thr, magic_thr);
}

// K9's and K13's body: g_pitch = cells from row to row of both grids
template <bool SUBPEL, int RPL>
__device__ __forceinline__ void tf_body(const TfArgs &a, int g_pitch, const uint32_t (&magic_s)[17], uint32_t (&part)[4][4])
{
    const TfFrame f = tf_frame(a);
    const int W = a.width, H = a.height, CW = a.cw;
    const uint32_t thr = (uint32_t)a.thr, magic_thr = a.magic_thr;
    uint32_t np = 0, nn = 0, wsum = 0, dsum = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        const size_t g0 = (size_t)cy * g_pitch + x0;
        uint32_t gp[4] = {0, 0, 0, 0}, gn[4] = {0, 0, 0, 0}, c[4];
        if (f.has_p) load_mv4(f.GP + g0, n, gp);
        if (f.has_n) load_mv4(f.GN + g0, n, gn);
        load_cells4(f.C, W, oy, x0, n, c);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint32_t rows[2][2] = {{0, 0}, {0, 0}}, ws = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ox = 2 * (x0 + j);
            uint32_t qp = 0, qn = 0;
            const uint32_t wp = f.has_p ? tf_weight<SUBPEL>(f.P, W, H, ox, oy, gp[j], c[j], thr, magic_thr, &qp) : 0u;
            const uint32_t wn = f.has_n ? tf_weight<SUBPEL>(f.N, W, H, ox, oy, gn[j], c[j], thr, magic_thr, &qn) : 0u;
            const uint32_t S = 8u + wp + wn, m = magic_s[wp + wn], half = S >> 1;
            uint32_t px = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t v = __umulhi(8u * ((c[j] >> (8 * q)) & 0xffu) + wp * ((qp >> (8 * q)) & 0xffu) +
                                            wn * ((qn >> (8 * q)) & 0xffu) + half, m);
                px |= v << (8 * q);
            }
            rows_put(rows, j, px);
            ws |= (wp | wn << 4) << (8 * j);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                np += wp != 0u; nn += wn != 0u;
                wsum += wp + wn;
                dsum += __builtin_amdgcn_sad_u8(px, c[j], 0u);
            }
        }
        if (a.out) store_rows2(a.out + blockIdx.z * a.out_stride + (size_t)oy * a.out_pitch + 2 * x0, a.out_pitch, n, rows);
        if (a.wmap) store_bytes4(a.wmap + (size_t)cy * a.wmap_pitch + x0, n, ws);
    }
    if (!a.partial) return;
    store_partial4(a.partial, (size_t)blockIdx.y * gridDim.z + blockIdx.z, part, np, nn, wsum, dsum);
}

__global__ __launch_bounds__(256) void k_temporal_filter(TfArgs a)
{
    __shared__ uint32_t magic_s[17], part[4][4];
    if (threadIdx.x < 17) magic_s[threadIdx.x] = a.magic_s[threadIdx.x];
    __syncthreads();
    tf_body<false, kTfRunsPerLane>(a, a.cw, magic_s, part);
}

// =======================================================================================
// K9b.  The BGR TEMPORAL FILTER RULE of include/bbme.h: K9 on three B,G,R frames, the cost of a neighbour's cell being the LARGEST
// of its three per-channel 2x2 SADs, and the UNPADDED frame written.  It reads no luma plane: the cells are those of the padded
// view (a pixel outside the fw x fh frame is 0 in every channel), cell (cx, cy) with origin o = (2 cx, 2 cy) holding the frame's
// pixels o - (pad_x, pad_y) + (j, i).  Same split, grid loads, map store and statistics tail as k_temporal_filter, same
// arguments (TfBgrArgs is TfArgs and the frame's place in the padded view: blockIdx.y = batch pair, blockIdx.z = the frame of a
// run, every input base + y s_y + z s_z in 64 bits, first_prev / last_next) and the colour accesses of k_interpolate_bgr: a neighbour's cell
// row is 6 contiguous bytes (bgr_two: one unaligned dword and one u16 load, bytes at the frame's edge, 0 outside); the run's own
// row is 24 bytes, three unaligned 8-byte loads where the run is whole and inside the frame and bgr_two cell by cell otherwise;
// the output row is collected in three 64-bit words and leaves as six dword stores when the run is whole, inside the frame and its
// row address dword-aligned, by bytes otherwise (with an odd padding cells straddle the frame's edge and only their pixels inside
// are written).  A run with no pixel in the frame is skipped before any load unless the map or the statistics are asked for: its
// cells are all-zero on C but belong to both.
// A cell row of a frame is the dword B0 G0 R0 B1 and the u16 G1 R1: the two u16 of a cell share a dword, and the per-channel SADs
// are v_sad_u8 on channel-masked dwords (B: 2, G and R: 3 each).  The divisions are K9's multiply-shifts with K9's bounds.
// Statistics as K9 (|out - C| over the cells' four pixels and three channels, at most 3060 a cell), same partial layout.
// K9b and K13b are made of the shared pieces (tf_frame, tf_cost_weight, the colour row helpers) but keep a kernel loop each: as
// one body, made as tf_body is, K9b measured up to 3.8 % and K13b up to 1.2 % above the parent (profiles/r28_gather_pieces.txt).
// =======================================================================================
// TfArgs, with cur / prev / next and out the fw x fh B,G,R frames (rows bgr_pitch and out_pitch bytes apart) and width x height the
// padded view, and the frame's place inside that view
struct TfBgrArgs : TfArgs {
    int fw, fh, pad_x, pad_y, bgr_pitch;
};

// the largest per-channel SAD of two cells; lo0, lo1: B0 G0 R0 B1 of the cell's rows, hi: G1 R1 of row 0 | G1 R1 of row 1 << 16
__device__ __forceinline__ uint32_t bgr_cell_cost(uint32_t c0, uint32_t c1, uint32_t ch, uint32_t x0, uint32_t x1, uint32_t xh)
{
    const uint32_t mB = 0xff0000ffu, mG = 0x0000ff00u, mR = 0x00ff0000u, hG = 0x00ff00ffu, hR = 0xff00ff00u;
    const uint32_t b = __builtin_amdgcn_sad_u8(c0 & mB, x0 & mB, __builtin_amdgcn_sad_u8(c1 & mB, x1 & mB, 0u));
    const uint32_t g = __builtin_amdgcn_sad_u8(c0 & mG, x0 & mG, __builtin_amdgcn_sad_u8(c1 & mG, x1 & mG,
                                               __builtin_amdgcn_sad_u8(ch & hG, xh & hG, 0u)));
    const uint32_t r = __builtin_amdgcn_sad_u8(c0 & mR, x0 & mR, __builtin_amdgcn_sad_u8(c1 & mR, x1 & mR,
                                               __builtin_amdgcn_sad_u8(ch & hR, xh & hR, 0u)));
    return max(b, max(g, r));
}

// One neighbour of the cell (c0, c1: its two rows of 6 bytes) with origin (ox, oy) on the padded view: its weight, and its two
// rows in q[] when the weight is not 0
__device__ __forceinline__ uint32_t tf_bgr_weight(const uint8_t *X, const TfBgrArgs &a, int ox, int oy, mv_t g, uint64_t c0, uint64_t c1,
                                                  uint32_t thr, uint32_t magic_thr, uint64_t *q)
{
    const int px = ox + mv_x(g), py = oy + mv_y(g);
    q[0] = q[1] = 0;
    if (px < 0 || py < 0 || px > a.width - 2 || py > a.height - 2) return 0u;
    const uint64_t x0 = bgr_two(X, a.bgr_pitch, a.fw, a.fh, px - a.pad_x, py - a.pad_y);
    const uint64_t x1 = bgr_two(X, a.bgr_pitch, a.fw, a.fh, px - a.pad_x, py - a.pad_y + 1);
    const uint32_t cost = bgr_cell_cost((uint32_t)c0, (uint32_t)c1, (uint32_t)(c0 >> 32) | (uint32_t)(c1 >> 32) << 16,
                                        (uint32_t)x0, (uint32_t)x1, (uint32_t)(x0 >> 32) | (uint32_t)(x1 >> 32) << 16);
    if (cost < thr) { q[0] = x0; q[1] = x1; }
    return tf_cost_weight(cost, thr, magic_thr);
}

__global__ __launch_bounds__(256) void k_temporal_filter_bgr(TfBgrArgs a)
{
    __shared__ uint32_t magic_s[17];
    if (threadIdx.x < 17) magic_s[threadIdx.x] = a.magic_s[threadIdx.x];
    __syncthreads();
    const TfFrame f = tf_frame(a);
    const uint8_t *C = f.C, *P = f.P, *N = f.N;
    const bool has_p = f.has_p, has_n = f.has_n;
    const mv_t *GP = f.GP, *GN = f.GN;
    const int CW = a.cw;
    const uint32_t thr = (uint32_t)a.thr, magic_thr = a.magic_thr;
    uint32_t np = 0, nn = 0, wsum = 0, dsum = 0;
#pragma unroll
    for (int r = 0; r < kTfRunsPerLane; ++r) {
        const long long i = gather_index<kTfRunsPerLane>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        const int fy = oy - a.pad_y, fx = 2 * x0 - a.pad_x;    // the run's first pixel in frame coordinates
        if (fy + 1 < 0 || fy >= a.fh || fx + 2 * n <= 0 || fx >= a.fw) {      // no pixel of the run is in the frame
            if (!a.partial && !a.wmap) continue;
        }
        const size_t g0 = (size_t)cy * CW + x0;
        uint32_t gp[4] = {0, 0, 0, 0}, gn[4] = {0, 0, 0, 0};
        if (has_p) load_mv4(GP + g0, n, gp);
        if (has_n) load_mv4(GN + g0, n, gn);
        const bool whole = bgr_run_whole(n, fx, a.fw);        // the run's 8 pixels lie inside a frame row
        uint64_t crow[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's own two rows, 24 bytes each
        if (whole) bgr_load_rows(C, a.bgr_pitch, a.fh, fx, fy, crow);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint64_t rows[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's two output rows
        uint32_t ws = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ox = 2 * (x0 + j);
            uint64_t c[2];
#pragma unroll
            for (int yy = 0; yy < 2; ++yy)
                c[yy] = whole ? bgr_row_get(crow[yy], j) : bgr_two(C, a.bgr_pitch, a.fw, a.fh, fx + 2 * j, fy + yy);
            uint64_t qp[2] = {0, 0}, qn[2] = {0, 0};
            const uint32_t wp = has_p ? tf_bgr_weight(P, a, ox, oy, gp[j], c[0], c[1], thr, magic_thr, qp) : 0u;
            const uint32_t wn = has_n ? tf_bgr_weight(N, a, ox, oy, gn[j], c[0], c[1], thr, magic_thr, qn) : 0u;
            const uint32_t S = 8u + wp + wn, m = magic_s[wp + wn], half = S >> 1;
            uint32_t diff = 0;
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                uint64_t px = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const uint32_t v = __umulhi(8u * ((uint32_t)(c[yy] >> (8 * q)) & 0xffu) + wp * ((uint32_t)(qp[yy] >> (8 * q)) & 0xffu) +
                                                wn * ((uint32_t)(qn[yy] >> (8 * q)) & 0xffu) + half, m);
                    px |= (uint64_t)v << (8 * q);
                }
                bgr_row_put(rows[yy], j, px);
                diff = __builtin_amdgcn_sad_u8((uint32_t)px, (uint32_t)c[yy], diff);
                diff = __builtin_amdgcn_sad_u8((uint32_t)(px >> 32), (uint32_t)(c[yy] >> 32), diff);
            }
            ws |= (wp | wn << 4) << (8 * j);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                np += wp != 0u; nn += wn != 0u;
                wsum += wp + wn;
                dsum += diff;
            }
        }
        if (a.out) bgr_store_rows(a.out + blockIdx.z * a.out_stride, a.out_pitch, a.fw, a.fh, fx, fy, n, whole, rows);
        if (a.wmap) store_bytes4(a.wmap + (size_t)cy * a.wmap_pitch + x0, n, ws);
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, (size_t)blockIdx.y * gridDim.z + blockIdx.z, part, np, nn, wsum, dsum);
}


// =======================================================================================
// K10.  Quarter-pel refinement of a 2x2-cell grid at the planes' own resolution (the SUBPEL RULE of include/bbme.h): a valid cell
// compares I1's 8 x 8 window around it with bilinear quarter-pel samples of I2 at 17 offsets q -- (0, 0), the eight half-pel
// neighbours, the eight quarter-pel neighbours of the best of those -- and leaves sat16(4 v + q).
// One cell per lane, a workgroup a tile of 32 x 8 cells (blockIdx.x = tile, row-major; a wave two tile rows), so that neighbouring
// lanes' windows overlap in L1 / TA: the window is 8 unaligned 8-byte loads, I2's 10 x 10 patch b + (-1 .. 8, -1 .. 8) ten unaligned
// 8 + 4-byte loads (12 bytes: the two past the patch are b.x + 9 and b.x + 10 <= W0 of a row that is not the plane's last), and
// with cells that share v the lanes' addresses run along the rows as the window's do.  Both stay in registers as bytes, 16 + 30
// dwords, for all 17 candidates; the loads are 18 of the 6 800 instructions a valid cell takes, so neither goes through LDS.
// A candidate (sp_cost) is the rule's separable form on 16-bit pairs.  Its integer part picks, per lane, the nine patch rows
// (v_cndmask) and, along x, the byte pairs (v_perm_b32 with a selector that holds the shift); then per row four v_pk_mul_lo_u16 /
// v_pk_mad_u16 give the horizontal sums (4 - fx) P0 + fx P1 of eight pixels, per output row a v_pk_mul_lo_u16, a v_pk_mad_u16,
// a v_pk_add_u16 (the rounding 8) and a v_pk_lshrrev_b16 per pixel pair the samples, two v_perm_b32 repack them to bytes and two
// v_sad_u8 add |I1 - sample|: about 400 VALU a candidate (88 v_perm_b32, 168 packed 16-bit, 16 v_sad_u8, 27 v_cndmask, moves).  The 17 candidates are one loop (not unrolled: the order of the rule's visits is its index), a lane keeping best
// and q; ties keep the earlier candidate because the comparison is strict.
// Statistics over the window [wx0, wx1) x [wy0, wy1) in cells: valid cells, cells with q != 0, the sums of cost(0, 0) and of
// best; a lane holds one cell of at most 16320 (store_partial4, frame = pair).  blockIdx.y = pair: planes s_plane bytes, grids
// s_grid and outputs s_out words apart.
// =======================================================================================
struct SpArgs {
    const uint8_t *img1, *img2;           // packed width x height planes
    const mv_t *grid;                     // cw entries per row, ch rows: integer vectors on img1 into img2
    mv_t *out;                            // quarter-pel vectors, rows out_pitch cells apart; or null
    unsigned long long *partial;          // per pair and workgroup {valid, moved, cost(0, 0), best}; or null
    size_t s_plane, s_grid, s_out;
    int width, height, cw, ch, out_pitch, tiles_x;
    int wx0, wy0, wx1, wy1;
};

constexpr int kSpTileW = 32, kSpTileH = 8;

typedef unsigned short sp_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ sp_u16x2 sp_pair(uint32_t v) { return __builtin_bit_cast(sp_u16x2, v); }
__device__ __forceinline__ sp_u16x2 sp_splat(int v) { return sp_u16x2{(unsigned short)v, (unsigned short)v}; }

// cost(q) of the rule: ref = I1's window, two dwords per row; pat = I2 at b + (-1 .. 10, -1 .. 8), three dwords per row
__device__ __forceinline__ uint32_t sp_cost(const uint32_t (&ref)[8][2], const uint32_t (&pat)[10][3], int qx, int qy)
{
    const bool up = qy < 0;                                   // iy = -1: the rows start one higher
    const uint32_t sx = (uint32_t)(1 + (qx >> 2));            // first byte of a row's nine: 0 or 1
    // byte pair (k, k + 1) of two dwords as two 16-bit values: the selector of v_perm_b32 (0x0c = a zero byte)
    const uint32_t s0 = 0x0c010c00u + sx * 0x00010001u, s1 = s0 + 0x00010001u, s2 = s1 + 0x00010001u, s3 = s2 + 0x00010001u;
    const sp_u16x2 wx1 = sp_splat(qx & 3), wx0 = sp_splat(4 - (qx & 3)), wy1 = sp_splat(qy & 3), wy0 = sp_splat(4 - (qy & 3));
    const sp_u16x2 half = sp_splat(8), four = sp_splat(4);
    sp_u16x2 above[4] = {};
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const uint32_t d0 = up ? pat[i][0] : pat[i + 1][0], d1 = up ? pat[i][1] : pat[i + 1][1], d2 = up ? pat[i][2] : pat[i + 1][2];
        sp_u16x2 h[4];
        h[0] = sp_pair(__builtin_amdgcn_perm(d1, d0, s0)) * wx0 + sp_pair(__builtin_amdgcn_perm(d1, d0, s1)) * wx1;
        h[1] = sp_pair(__builtin_amdgcn_perm(d1, d0, s2)) * wx0 + sp_pair(__builtin_amdgcn_perm(d1, d0, s3)) * wx1;
        h[2] = sp_pair(__builtin_amdgcn_perm(d2, d1, s0)) * wx0 + sp_pair(__builtin_amdgcn_perm(d2, d1, s1)) * wx1;
        h[3] = sp_pair(__builtin_amdgcn_perm(d2, d1, s2)) * wx0 + sp_pair(__builtin_amdgcn_perm(d2, d1, s3)) * wx1;
        if (i > 0) {
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = __builtin_bit_cast(uint32_t, (above[k] * wy0 + h[k] * wy1 + half) >> four);
            sum = __builtin_amdgcn_sad_u8(ref[i - 1][0], __builtin_amdgcn_perm(v[1], v[0], 0x06040200u), sum);
            sum = __builtin_amdgcn_sad_u8(ref[i - 1][1], __builtin_amdgcn_perm(v[3], v[2], 0x06040200u), sum);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) above[k] = h[k];
    }
    return sum;
}

__global__ __launch_bounds__(256) void k_subpel_refine(SpArgs a)
{
    const size_t pair = blockIdx.y;
    const uint8_t *I1 = a.img1 + pair * a.s_plane, *I2 = a.img2 + pair * a.s_plane;
    const int W = a.width, H = a.height;
    const int cx = (int)(blockIdx.x % (unsigned)a.tiles_x) * kSpTileW + (int)(threadIdx.x & (kSpTileW - 1));
    const int cy = (int)(blockIdx.x / (unsigned)a.tiles_x) * kSpTileH + (int)(threadIdx.x / kSpTileW);
    uint32_t nvalid = 0, nmoved = 0, sum0 = 0, sumb = 0;
    if (cx < a.cw && cy < a.ch) {
        const mv_t g = a.grid[pair * a.s_grid + (size_t)cy * a.cw + cx];
        const int vx = mv_x(g), vy = mv_y(g);
        const int ax = 2 * cx - 3, ay = 2 * cy - 3, bx = ax + vx, by = ay + vy;
        int qx = 0, qy = 0;
        if (ax >= 0 && ax + 8 <= W && ay >= 0 && ay + 8 <= H && bx >= 2 && bx + 10 <= W && by >= 2 && by + 10 <= H) {
            uint32_t ref[8][2], pat[10][3];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const ua_u32x2 t = *reinterpret_cast<const ua_u32x2 *>(I1 + (size_t)(ay + i) * W + ax);
                ref[i][0] = t.v[0]; ref[i][1] = t.v[1];
            }
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const uint8_t *row = I2 + (size_t)(by - 1 + i) * W + (bx - 1);
                const ua_u32x2 t = *reinterpret_cast<const ua_u32x2 *>(row);
                pat[i][0] = t.v[0]; pat[i][1] = t.v[1];
                pat[i][2] = reinterpret_cast<const ua_u32 *>(row + 8)->v;
            }
            int best = 0x7fffffff, cost0 = 0, ox = 0, oy = 0;     // (ox, oy): the q a stage starts from
#pragma unroll 1
            for (int k = 0; k < 17; ++k) {
                int dx = 0, dy = 0;
                if (k) {                                          // the rule's order: the 3 x 3 raster without its centre
                    const int t = (k - 1) & 7, idx = t + (t >= 4);
                    dx = idx % 3 - 1; dy = idx / 3 - 1;
                    if (k < 9) { dx *= 2; dy *= 2; }
                }
                if (k == 9) { ox = qx; oy = qy; }
                const int tx = ox + dx, ty = oy + dy;
                const int cost = (int)sp_cost(ref, pat, tx, ty);
                if (k == 0) cost0 = cost;
                if (cost < best) { best = cost; qx = tx; qy = ty; }
            }
            if (a.partial && cx >= a.wx0 && cx < a.wx1 && cy >= a.wy0 && cy < a.wy1) {
                nvalid = 1; nmoved = (qx | qy) != 0; sum0 = (uint32_t)cost0; sumb = (uint32_t)best;
            }
        }
        if (a.out) {
            const int ux = min(max(4 * vx + qx, -32768), 32767), uy = min(max(4 * vy + qy, -32768), 32767);
            a.out[pair * a.s_out + (size_t)cy * a.out_pitch + cx] = ((uint32_t)ux & 0xffffu) | ((uint32_t)uy << 16);
        }
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, pair, part, nvalid, nmoved, sum0, sumb);
}

// The quarter-pel grid as the driver's field (main_class.cpp:58-70, k_subsample's indexing): out(y, x) = cell((pad_y + s y) >> 1,
// (pad_x + s x) >> 1) / (4 s) for the ceil(W / s) x ceil(H / s) field of the unpadded frame; packed rows.  One pixel per thread.
__global__ __launch_bounds__(256) void k_subsample_q4(const mv_t *cells, int cell_cols, int pad_x, int pad_y, int scale, float *out,
                                                      int out_width, int out_height)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)out_width * out_height) return;
    const int x = (int)(t % out_width), y = (int)(t / out_width);
    const mv_t m = cells[(size_t)((pad_y + scale * y) >> 1) * cell_cols + ((pad_x + scale * x) >> 1)];
    const float s = (float)(4 * scale);
    *reinterpret_cast<float2 *>(out + 2 * (size_t)t) = make_float2((float)mv_x(m) / s, (float)mv_y(m) / s);
}

// =======================================================================================
// K11.  Motion compensation along a quarter-pel grid, fused with the residual statistics against I1 (the SUBPEL COMPENSATION RULE
// of include/bbme.h): cell (cx, cy) with origin o and (qx, qy) = Q[cy][cx] takes its 2 x 2 pixels as the SUBPEL RULE's bilinear
// samples of I2 at s = o + (qx >> 2, qy >> 2) with the fractions f = (qx & 3, qy & 3); a cell one of whose taps of non-zero weight
// would leave the plane is skipped and gets `fill`.  It is k_motion_compensate's sibling in the gather family: the shared split of
// runs of 4 cells of one cell row (gather_index / gather_split), Q by load_mv4, blockIdx.y = pair.
// Loads.  A cell needs 2 + (fx != 0) bytes of 2 + (fy != 0) rows of I2 at an arbitrary byte address.  The third row and the third
// column are addressed at offset 1 + (f != 0): where the fraction is 0 they fold onto the second (their weight is 0 then), so no
// address leaves the plane that the rule does not name.  A row's bytes are one unaligned dword when the four bytes from s.x on lie
// in the row (s.x + 4 <= W0: all but cells at the right edge), else an unaligned u16 and a byte: three loads a cell, where widening
// every load to a dword could touch the byte behind a caller's plane.  The sample is the separable form: the horizontal sums of the
// three rows, then the vertical sums with the single rounding.
// Stores.  A run is 8 bytes in each of two pixel rows: one 8-byte store when the run is whole and the address 8-byte aligned
// (a caller's rows need not be), bytes otherwise.  I1 is read -- 8 bytes a row, or a cell at a time on a cut run -- only for cell
// rows that meet the window.
// Statistics over the window [wx0, wx1) x [wy0, wy1) in PIXELS: sse, sad and pixels over the compensated cells' window pixels,
// skipped over the others'.  A lane sums at most kScRunsPerLane runs of 16 pixels in 32 bits, and a wave's sum stays below 2^32:
// 64 * kScRunsPerLane * 16 * 255^2 = 133 171 200 (store_partial4, frame = pair).
// =======================================================================================
struct ScArgs {
    const uint8_t *img1, *img2;           // packed width x height planes; img1 may be null without statistics
    const mv_t *q4;                       // quarter-pel vectors: cw entries per row, rows q4_pitch cells apart
    uint8_t *out;                         // compensated plane (rows out_pitch bytes apart), or null
    unsigned long long *partial;          // per pair and workgroup {sse, sad, pixels, skipped}; or null (no statistics)
    size_t s_plane, s_q4;                 // from pair to pair: bytes, words
    int width, height, cw, q4_pitch, fill, out_pitch;
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

constexpr int kScRunsPerLane = 2;

__global__ __launch_bounds__(256) void k_subpel_compensate(ScArgs a)
{
    const size_t pair = blockIdx.y;
    const uint8_t *I2 = a.img2 + pair * a.s_plane;
    const mv_t *Q = a.q4 + pair * a.s_q4;
    const int W = a.width, H = a.height, CW = a.cw;
    uint32_t sse = 0, sad = 0, npix = 0, nskip = 0;
#pragma unroll
    for (int r = 0; r < kScRunsPerLane; ++r) {
        const long long i = gather_index<kScRunsPerLane>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        uint32_t q[4];
        load_mv4(Q + (size_t)cy * a.q4_pitch + x0, n, q);
        uint32_t row0[2] = {0, 0}, row1[2] = {0, 0}, ok = 0;  // the two pixel rows of the run; bit j: cell x0 + j was compensated
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int qx = mv_x(q[j]), qy = mv_y(q[j]);
            const int fx = qx & 3, fy = qy & 3, x1 = fx != 0, y1 = fy != 0;
            const int sx = 2 * (x0 + j) + (qx >> 2), sy = oy + (qy >> 2);
            uint32_t px = (uint32_t)a.fill * 0x01010101u;     // the cell: its upper pixels in bits 0-15, its lower ones in 16-31
            if (sx >= 0 && sx + 2 + x1 <= W && sy >= 0 && sy + 2 + y1 <= H) {
                const uint8_t *p = I2 + (size_t)sy * W + sx;
                const bool wide = sx + 4 <= W;
                const uint32_t t0 = sc_row(p, wide, x1), t1 = sc_row(p + W, wide, x1), t2 = sc_row(p + (size_t)(1 + y1) * W, wide, x1);
                const uint32_t wx = (uint32_t)fx, wy = (uint32_t)fy;
                uint32_t h[3][2];                             // (4 - fx) P0 + fx P1 of the three rows' two pixels, <= 1020
                h[0][0] = (4u - wx) * (t0 & 0xffu) + wx * ((t0 >> 8) & 0xffu); h[0][1] = (4u - wx) * ((t0 >> 8) & 0xffu) + wx * (t0 >> 16);
                h[1][0] = (4u - wx) * (t1 & 0xffu) + wx * ((t1 >> 8) & 0xffu); h[1][1] = (4u - wx) * ((t1 >> 8) & 0xffu) + wx * (t1 >> 16);
                h[2][0] = (4u - wx) * (t2 & 0xffu) + wx * ((t2 >> 8) & 0xffu); h[2][1] = (4u - wx) * ((t2 >> 8) & 0xffu) + wx * (t2 >> 16);
                px = 0;
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int m = 0; m < 2; ++m) px |= (((4u - wy) * h[k][m] + wy * h[k + 1][m] + 8u) >> 4) << (16 * k + 8 * m);
                ok |= 1u << j;
            }
            row0[j >> 1] |= (px & 0xffffu) << (16 * (j & 1));
            row1[j >> 1] |= (px >> 16) << (16 * (j & 1));
        }
        if (a.out) {
            uint8_t *o = a.out + (size_t)oy * a.out_pitch + 2 * x0;
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                const uint32_t *row = yy ? row1 : row0;
                uint8_t *d = o + (size_t)yy * a.out_pitch;
                if (n == 4 && ((uintptr_t)d & 7u) == 0) *reinterpret_cast<uint2 *>(d) = make_uint2(row[0], row[1]);
                else for (int x = 0; x < 2 * n; ++x) d[x] = (uint8_t)(row[x >> 2] >> (8 * (x & 3)));
            }
        }
        if (a.partial && oy + 1 >= a.wy0 && oy < a.wy1) {
            const uint8_t *r1 = a.img1 + pair * a.s_plane + (size_t)oy * W + 2 * x0;
            uint32_t ref0[2] = {0, 0}, ref1[2] = {0, 0};
            if (n == 4) {
                const ua_u32x2 t = *reinterpret_cast<const ua_u32x2 *>(r1), u = *reinterpret_cast<const ua_u32x2 *>(r1 + W);
                ref0[0] = t.v[0]; ref0[1] = t.v[1]; ref1[0] = u.v[0]; ref1[1] = u.v[1];
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (j >= n) break;
                    ref0[j >> 1] |= (uint32_t)reinterpret_cast<const ua_u16 *>(r1 + 2 * j)->v << (16 * (j & 1));
                    ref1[j >> 1] |= (uint32_t)reinterpret_cast<const ua_u16 *>(r1 + W + 2 * j)->v << (16 * (j & 1));
                }
            }
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                if (oy + yy < a.wy0 || oy + yy >= a.wy1) continue;
                const uint32_t *row = yy ? row1 : row0, *ref = yy ? ref1 : ref0;
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int X = 2 * x0 + x;
                    if (x >= 2 * n || X < a.wx0 || X >= a.wx1) continue;
                    if ((ok >> (x >> 1)) & 1u) {
                        const int d = (int)((row[x >> 2] >> (8 * (x & 3))) & 0xffu) - (int)((ref[x >> 2] >> (8 * (x & 3))) & 0xffu);
                        sse += (uint32_t)(d * d);
                        sad += (uint32_t)abs(d);
                        ++npix;
                    } else {
                        ++nskip;
                    }
                }
            }
        }
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, pair, part, sse, sad, npix, nskip);
}

// =======================================================================================
// K12.  Motion-compensated interpolation at phase num / den at QUARTER-PEL positions (the SUBPEL INTERPOLATION RULE of
// include/bbme.h): output cell (cx, cy) with origin o tries v = QF[cy][cx], v = -QB[cy][cx] (when QB is given) and v = 0, all in
// quarter pels; a hypothesis samples the 2x2 cell of I1 at P1 = 4 o - round(num v / den) and the one of I2 at P2 = P1 + v as the
// SUBPEL RULE's bilinear samples, is valid when every tap of non-zero weight of both lies in the plane, and costs the SAD of the
// ROUNDED samples; the cheapest valid one (the earliest of equals) is blended, ((den - num) S1 + num S2 + den / 2) / den.  It is
// k_interpolate's and k_subpel_compensate's sibling in the gather family: the shared split of runs of 4 cells of one cell row
// (gather_index / gather_split), QF and QB by load_mv4 (rows q4_pitch cells apart), blockIdx.y = pair (planes s_plane bytes, grids
// s_q4 words apart), blockIdx.z = phase num0 + z (frames out_stride, maps sel_stride bytes apart), so that every phase but the
// first finds planes and grids in L2.  `out` and `sel` only with one pair per launch.
// Loads.  A moved cell needs 2 + (fx != 0) bytes of 2 + (fy != 0) rows of its plane at an arbitrary byte address: K11's
// addressing (si_cell through sc_row: the third row and the third column at offset 1 + (f != 0), folding onto the second where the
// weight is 0; one unaligned dword a row where its four bytes lie in the row, a u16 and a byte at the right edge), three loads a
// cell and plane, six a hypothesis, and none of them leaves the plane.  The zero hypothesis keeps k_interpolate's loads
// (load_cells4).
// Arithmetic.  The horizontal sums of the three rows, then the vertical sums with the single rounding; the four samples packed
// into one dword per cell as ip_cell packs pixels, so that v_sad_u8 gives the cost in one instruction.  The cost is taken on the
// rounded samples because those are what the blend mixes: it is the SAD of the two cells the output is made of, 0..1020, as in
// k_interpolate, and with all fractions 0 it is k_interpolate's cost.
// Divisions by den are k_interpolate's multiply-shifts by magic = floor(2^32 / den) + 1, exact below 2^24 (e <= 256): the blend's
// numerators stay below 255 * 256 + 128, and |num v| <= (den - 1) 32768 for every int16 v, -(-32768) = 32768 included, so the
// shifts' num v + den / 2 + 32768 den lies in [32768, 511 * 32768 + 128], below 2^24.  Positions are 32-bit: |P| < 2^17.
// Stores as k_interpolate: the rows by store_rows2, the map by store_bytes4.  The selection is si_select, which
// k_subpel_interpolate_bgr shares.  Statistics over the window [wx0, wx1) x [wy0, wy1) in cells: cells that selected k = 0, 1, 2 and the sum of the
// selected costs; a lane holds at most 4 kSiRunsPerLane cells of cost <= 1020 (store_partial4, frame = (phase, pair)).
// =======================================================================================
struct SiArgs {
    const uint8_t *img1, *img2;           // level-0 padded (luma) planes, pitch = width
    const mv_t *qf, *qb;                  // quarter-pel grids: cw entries per row, rows q4_pitch cells apart; qb may be null
    uint8_t *out;                         // frames (rows out_pitch, phases out_stride bytes apart), or null
    uint8_t *sel;                         // one byte k per cell (rows sel_pitch, phases sel_stride bytes apart), or null
    unsigned long long *partial;          // per (phase, pair) and workgroup {k = 0, k = 1, k = 2, cost}; or null
    size_t out_stride, sel_stride;
    size_t s_plane, s_q4;                 // from pair to pair: bytes, words
    int width, height, cw, q4_pitch, num0, den, out_pitch, sel_pitch;
    uint32_t magic;                       // floor(2^32 / den) + 1
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * height / 2
};

constexpr int kSiRunsPerLane = 2;

// every tap of non-zero weight of the cell at quarter-pel position p (one axis) lies in a plane of `size`
__device__ __forceinline__ bool si_inside(int p, int size)
{
    const int i = p >> 2;
    return i >= 0 && i + 2 + ((p & 3) != 0) <= size;
}

// What the cell with the quarter-pel origin (ox4, oy4) = 4 o selects: hypothesis k and its cost, its two cells of rounded samples
// c1 (of I1 at P1) and c2 (of I2 at P2 = P1 + v), P1 and v; z1 and z2 are the cells of the zero hypothesis.  Shared by
// k_subpel_interpolate, which blends the cells, and k_subpel_interpolate_bgr, which samples colour at P1 and P2.
struct SiPick { uint32_t c1, c2, k, cost; int p1x, p1y, vx, vy; };

__device__ __forceinline__ SiPick si_select(const uint8_t *img1, const uint8_t *img2, int W, int H, int ox4, int oy4, uint32_t qf,
                                            uint32_t qb, bool has_b, uint32_t z1, uint32_t z2, int num, int half, int bias,
                                            uint32_t magic)
{
    SiPick s{0u, 0u, 2u, ~0u, ox4, oy4, 0, 0};                // nothing selected yet
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1 && !has_b) break;
        const int vx = h ? -mv_x(qb) : mv_x(qf), vy = h ? -mv_y(qb) : mv_y(qf);
        const int sx = (int)__umulhi((uint32_t)(num * vx + half + bias), magic) - 32768;
        const int sy = (int)__umulhi((uint32_t)(num * vy + half + bias), magic) - 32768;
        const int p1x = ox4 - sx, p1y = oy4 - sy, p2x = p1x + vx, p2y = p1y + vy;
        if (!si_inside(p1x, W) || !si_inside(p2x, W) || !si_inside(p1y, H) || !si_inside(p2y, H)) continue;
        const uint32_t q1 = si_cell(img1, W, p1x >> 2, p1y >> 2, p1x & 3, p1y & 3);
        const uint32_t q2 = si_cell(img2, W, p2x >> 2, p2y >> 2, p2x & 3, p2y & 3);
        const uint32_t c = __builtin_amdgcn_sad_u8(q1, q2, 0u);
        if (c < s.cost) s = SiPick{q1, q2, (uint32_t)h, c, p1x, p1y, vx, vy};      // strictly cheaper: the earliest of equals stays
    }
    const uint32_t cz = __builtin_amdgcn_sad_u8(z1, z2, 0u);
    if (cz < s.cost) s = SiPick{z1, z2, 2u, cz, ox4, oy4, 0, 0};
    return s;
}

__global__ __launch_bounds__(256) void k_subpel_interpolate(SiArgs a)
{
    const size_t pair = blockIdx.y;
    const uint8_t *img1 = a.img1 + pair * a.s_plane, *img2 = a.img2 + pair * a.s_plane;
    const mv_t *QF = a.qf + pair * a.s_q4, *QB = a.qb ? a.qb + pair * a.s_q4 : nullptr;
    const int W = a.width, H = a.height, CW = a.cw, den = a.den, num = a.num0 + (int)blockIdx.z, half = den >> 1;
    const uint32_t magic = a.magic, w1 = (uint32_t)(den - num), w2 = (uint32_t)num;
    const int bias = 32768 * den;
    uint32_t n0 = 0, n1 = 0, n2 = 0, csum = 0;
#pragma unroll
    for (int r = 0; r < kSiRunsPerLane; ++r) {
        const long long i = gather_index<kSiRunsPerLane>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        uint32_t qf[4], qb[4] = {0, 0, 0, 0}, z1[4], z2[4];
        load_mv4(QF + (size_t)cy * a.q4_pitch + x0, n, qf);
        if (QB) load_mv4(QB + (size_t)cy * a.q4_pitch + x0, n, qb);
        load_cells4(img1, W, oy, x0, n, z1);                  // the zero hypothesis' cells
        load_cells4(img2, W, oy, x0, n, z2);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint32_t rows[2][2] = {{0, 0}, {0, 0}}, ks = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const SiPick s = si_select(img1, img2, W, H, 8 * (x0 + j), 8 * cy, qf[j], qb[j], QB != nullptr, z1[j], z2[j], num, half,
                                       bias, magic);
            const uint32_t c1 = s.c1, c2 = s.c2, k = s.k, cost = s.cost;
            uint32_t px = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t v = __umulhi(w1 * ((c1 >> (8 * q)) & 0xffu) + w2 * ((c2 >> (8 * q)) & 0xffu) + (uint32_t)half, magic);
                px |= v << (8 * q);
            }
            rows_put(rows, j, px);
            ks |= k << (8 * j);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                n0 += k == 0u; n1 += k == 1u; n2 += k == 2u;
                csum += cost;
            }
        }
        if (a.out) store_rows2(a.out + blockIdx.z * a.out_stride + (size_t)oy * a.out_pitch + 2 * x0, a.out_pitch, n, rows);
        if (a.sel) store_bytes4(a.sel + blockIdx.z * a.sel_stride + (size_t)cy * a.sel_pitch + x0, n, ks);
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, (size_t)blockIdx.z * gridDim.y + pair, part, n0, n1, n2, csum);
}

// =======================================================================================
// K12b.  The BGR SUBPEL INTERPOLATION RULE of include/bbme.h: k_subpel_interpolate's selection on the LUMA planes (si_select: the
// same loads through si_cell, the same multiply-shifts by `magic`, validity by si_inside and v_sad_u8 on the packed rounded samples),
// then both B,G,R frames sampled bilinearly at the selected P1 and P2 and blended, written as the unpadded frame.  The sibling of
// k_subpel_interpolate and of k_interpolate_bgr in the gather family: the shared split of runs of 4 cells of one cell row
// (gather_index / gather_split), QF and QB by load_mv4, blockIdx.z = phase num0 + z, so that every phase but the first finds planes,
// grids and colour in L2 as far as they fit; one pair per launch.
// Colour loads.  A cell's 2x2 output pixels need, per frame, 2 + (fx != 0) pixels of 2 + (fy != 0) rows from t = (P >> 2) -
// (pad_x, pad_y) on: up to 3 rows of 9 contiguous bytes (bgr_three).  Where those pixels lie inside the frame's row they arrive as
// unaligned dwords (a dword and a u16 for two pixels; two dwords and a byte for three); at the frame's edges pixel by pixel in
// single bytes, a pixel outside reading 0 without a load.  A row or a column of weight 0 is not loaded, and no byte outside the
// colour frames is read.
// Arithmetic.  Separable as the rule allows: the horizontal sums (4 - fx) T0 + fx T1 <= 1020 of the rows, then the vertical sum
// with the single rounding.  B and R share a word in 16-bit lanes (T & 0xff00ff; the sums stay below 4088 < 2^16), G has its own.
// The blend divides by den with k_interpolate's multiply-shift: numerators below 255 * 256 + 128.
// Stores are k_interpolate_bgr's (bgr_row_put, bgr_store_rows).  Runs wholly outside the frame load nothing.
// A template over the runs per lane (instantiated with kSiRunsPerLane): template kernels are emitted behind the plain ones in the
// order of their first use, so this one lies behind every kernel of the estimate in the code object.  As a plain kernel it lay
// behind k_subpel_interpolate, and every k_search_* and k_reg_* kernel lay 77 056 bytes further on than before.
// =======================================================================================
struct SiBgrArgs {
    const uint8_t *img1, *img2;           // level-0 padded luma planes, pitch = width
    const mv_t *qf, *qb;                  // quarter-pel grids: cw entries per row, rows q4_pitch cells apart; qb may be null
    const uint8_t *bgr1, *bgr2;           // the fw x fh colour frames, rows bgr_pitch bytes apart
    uint8_t *out;                         // the fw x fh B,G,R frames (rows out_pitch, phases out_stride bytes apart)
    size_t out_stride;
    int width, height, cw, q4_pitch, num0, den, out_pitch;
    int fw, fh, pad_x, pad_y, bgr_pitch;
    uint32_t magic;                       // floor(2^32 / den) + 1
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * height / 2
};

// Pixels x, x + 1 and, with x1, x + 2 of row y of a colour frame, each as B | G << 8 | R << 16; a pixel outside the frame is 0,
// and without x1 the third is 0 and not read
__device__ __forceinline__ void bgr_three(const uint8_t *img, int pitch, int fw, int fh, int x, int y, int x1, uint32_t (&p)[3])
{
    p[0] = p[1] = p[2] = 0;
    if (y < 0 || y >= fh || x + 1 + x1 < 0 || x >= fw) return;
    const uint8_t *row = img + (size_t)y * pitch;
    if (x >= 0 && x + 2 + x1 <= fw) {                         // bytes 3 x .. 3 x + 5 + 3 x1 lie in the row
        const uint8_t *q = row + 3 * x;
        const uint32_t d0 = reinterpret_cast<const ua_u32 *>(q)->v;
        p[0] = d0 & 0xffffffu;
        if (x1) {
            const uint32_t d1 = reinterpret_cast<const ua_u32 *>(q + 4)->v;
            p[1] = (d0 >> 24) | (d1 & 0xffffu) << 8;
            p[2] = (d1 >> 16) | (uint32_t)q[8] << 16;
        } else {
            p[1] = (d0 >> 24) | (uint32_t)reinterpret_cast<const ua_u16 *>(q + 4)->v << 8;
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int px = x + m;
        if (m >= 2 + x1 || px < 0 || px >= fw) continue;
        const uint8_t *q = row + 3 * px;
        p[m] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    }
}

// The 2x2 pixels of a colour frame sampled at the integer position (tx, ty) (frame coordinates) with the fractions (fx, fy):
// e[r][m] holds B in bits 0-7 and R in bits 16-23, g[r][m] holds G
__device__ __forceinline__ void si_bgr_cell(const uint8_t *img, int pitch, int fw, int fh, int tx, int ty, int fx, int fy,
                                            uint32_t (&e)[2][2], uint32_t (&g)[2][2])
{
    const int x1 = fx != 0, y1 = fy != 0;
    const uint32_t wx = (uint32_t)fx, wy = (uint32_t)fy;
    uint32_t he[3][2], hg[3][2];                              // the horizontal sums of the three rows' two pixels, <= 1020 a lane
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t p[3] = {0, 0, 0};
        if (k < 2 + y1) bgr_three(img, pitch, fw, fh, tx, ty + k, x1, p);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            he[k][m] = (4u - wx) * (p[m] & 0xff00ffu) + wx * (p[m + 1] & 0xff00ffu);
            hg[k][m] = (4u - wx) * ((p[m] >> 8) & 0xffu) + wx * ((p[m + 1] >> 8) & 0xffu);
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            e[r][m] = (((4u - wy) * he[r][m] + wy * he[r + 1][m] + 0x00080008u) >> 4) & 0x00ff00ffu;
            g[r][m] = ((4u - wy) * hg[r][m] + wy * hg[r + 1][m] + 8u) >> 4;
        }
}

template <int RPL>
__global__ __launch_bounds__(256) void k_subpel_interpolate_bgr(SiBgrArgs a)
{
    const mv_t *QF = a.qf, *QB = a.qb;
    const int W = a.width, H = a.height, CW = a.cw, den = a.den, num = a.num0 + (int)blockIdx.z, half = den >> 1;
    const uint32_t magic = a.magic, w1 = (uint32_t)(den - num), w2 = (uint32_t)num;
    const int bias = 32768 * den;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        const int ry = oy - a.pad_y, rx = 2 * x0 - a.pad_x;   // the run's first pixel in frame coordinates
        if (ry + 1 < 0 || ry >= a.fh || rx + 2 * n <= 0 || rx >= a.fw) continue;      // no pixel of the run is in the frame
        uint32_t qf[4], qb[4] = {0, 0, 0, 0}, z1[4], z2[4];
        load_mv4(QF + (size_t)cy * a.q4_pitch + x0, n, qf);
        if (QB) load_mv4(QB + (size_t)cy * a.q4_pitch + x0, n, qb);
        load_cells4(a.img1, W, oy, x0, n, z1);                // the zero hypothesis' cells
        load_cells4(a.img2, W, oy, x0, n, z2);
        uint64_t rows[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's two output rows, 24 bytes each
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const SiPick s = si_select(a.img1, a.img2, W, H, 8 * (x0 + j), 8 * cy, qf[j], qb[j], QB != nullptr, z1[j], z2[j], num, half,
                                       bias, magic);
            const int p2x = s.p1x + s.vx, p2y = s.p1y + s.vy;
            uint32_t e1[2][2], g1[2][2], e2[2][2], g2[2][2];
            si_bgr_cell(a.bgr1, a.bgr_pitch, a.fw, a.fh, (s.p1x >> 2) - a.pad_x, (s.p1y >> 2) - a.pad_y, s.p1x & 3, s.p1y & 3, e1, g1);
            si_bgr_cell(a.bgr2, a.bgr_pitch, a.fw, a.fh, (p2x >> 2) - a.pad_x, (p2y >> 2) - a.pad_y, p2x & 3, p2y & 3, e2, g2);
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                uint64_t px = 0;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const uint32_t vb = __umulhi(w1 * (e1[y][m] & 0xffu) + w2 * (e2[y][m] & 0xffu) + (uint32_t)half, magic);
                    const uint32_t vg = __umulhi(w1 * g1[y][m] + w2 * g2[y][m] + (uint32_t)half, magic);
                    const uint32_t vr = __umulhi(w1 * (e1[y][m] >> 16) + w2 * (e2[y][m] >> 16) + (uint32_t)half, magic);
                    px |= (uint64_t)(vb | vg << 8 | vr << 16) << (24 * m);
                }
                bgr_row_put(rows[y], j, px);
            }
        }
        bgr_store_rows(a.out + blockIdx.z * a.out_stride, a.out_pitch, a.fw, a.fh, rx, ry, n, bgr_run_whole(n, rx, a.fw), rows);
    }
}

// =======================================================================================
// K13.  Motion-compensated temporal filter along QUARTER-PEL grids (the SUBPEL TEMPORAL FILTER RULE of include/bbme.h): K9 with
// each neighbour's cell taken as K11 and K12 take theirs.  For each present neighbour X with grid Q on C, (qx, qy) = Q[cy][cx],
// s = o + (qx >> 2, qy >> 2), f = (qx & 3, qy & 3); the neighbour is valid when every tap of non-zero weight lies in the plane, and
// its cell is the SUBPEL RULE's four rounded bilinear samples (tf_weight<true>).  Everything else -- layout, weight, blend, map,
// statistics and the divisions' bounds -- is tf_body's, with K9; the grids' rows lie q4_pitch cells apart.
// A template, as K12b: a template's code lies behind the estimate's template kernels in the code object, a plain kernel's before.
// =======================================================================================
struct TfSpArgs : TfArgs {                // gp / gn: quarter-pel vectors
    int q4_pitch;                         // cells from row to row of both grids
};

template <int RPL>
__global__ __launch_bounds__(256) void k_subpel_temporal_filter(TfSpArgs a)
{
    __shared__ uint32_t magic_s[17], part[4][4];
    if (threadIdx.x < 17) magic_s[threadIdx.x] = a.magic_s[threadIdx.x];
    __syncthreads();
    tf_body<true, RPL>(a, a.q4_pitch, magic_s, part);
}

// =======================================================================================
// K13b.  The BGR SUBPEL TEMPORAL FILTER RULE of include/bbme.h: K9b with each neighbour's cell taken at a QUARTER-PEL position of
// the zero-padded view of the colour frames, as K13 takes it on a plane.  Output cell (cx, cy) with origin o reads, for each present
// neighbour X with grid Q on C, (qx, qy) = Q[cy][cx], s = o + (qx >> 2, qy >> 2), f = (qx & 3, qy & 3); the neighbour is valid when
// every tap of non-zero weight lies in the padded view (K13's test); its cell is the four rounded bilinear samples of each channel
// (si_bgr_cell, K12b's: up to three frame rows of nine bytes at an arbitrary byte address, a pixel outside the frame 0, the third
// row and the third column folded away where the fraction is 0 so that a tap of weight 0 is never addressed), repacked into K9b's
// layout of a cell row -- the dword B0 G0 R0 B1 and the u16 G1 R1 -- so that bgr_cell_cost gives the largest per-channel SAD on
// the ROUNDED samples, and the weight, the blend, the output rows, the map and the statistics are K9b's from there on.
// Layout is K9b's: the shared split of runs of 4 cells, the run's own rows as three unaligned 8-byte loads where the run is whole
// and inside the frame (bgr_two otherwise), the straddling-edge stores; QP and QN by load_mv4, rows q4_pitch cells apart, as K13
// reads them; blockIdx.y = batch pair, blockIdx.z = the frame of a run.
// Both divisions are K9's multiply-shifts with K9's bounds: the samples are bytes, so the cost is still <= 1020 and the blend's
// numerator still <= 255 * 24 + 12.  Statistics as K9b (at most 3060 a cell), same partial layout: no atomics.
// A template, as K12b and K13: a template's code lies behind the estimate's template kernels in the code object.
// =======================================================================================
struct TfSpBgrArgs : TfBgrArgs {          // gp / gn: quarter-pel vectors
    int q4_pitch;                         // cells from row to row of both grids
};

// One neighbour of the cell (c0, c1: its two rows of 6 bytes) with origin (ox, oy) on the padded view: its weight, and its two
// rows of rounded samples in q[] when the weight is not 0
__device__ __forceinline__ uint32_t stf_bgr_weight(const uint8_t *X, const TfSpBgrArgs &a, int ox, int oy, mv_t g, uint64_t c0, uint64_t c1,
                                                   uint32_t thr, uint32_t magic_thr, uint64_t *q)
{
    const int qx = mv_x(g), qy = mv_y(g);
    const int fx = qx & 3, fy = qy & 3;
    const int sx = ox + (qx >> 2), sy = oy + (qy >> 2);
    q[0] = q[1] = 0;
    if (sx < 0 || sy < 0 || sx + 2 + (fx != 0) > a.width || sy + 2 + (fy != 0) > a.height) return 0u;
    uint32_t e[2][2], gr[2][2];
    si_bgr_cell(X, a.bgr_pitch, a.fw, a.fh, sx - a.pad_x, sy - a.pad_y, fx, fy, e, gr);
    uint32_t lo[2], hi[2];                                    // B0 G0 R0 B1; G1 R1
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        lo[r] = (e[r][0] & 0xffu) | gr[r][0] << 8 | (e[r][0] & 0xff0000u) | e[r][1] << 24;
        hi[r] = gr[r][1] | (e[r][1] >> 16) << 8;
    }
    const uint32_t cost = bgr_cell_cost((uint32_t)c0, (uint32_t)c1, (uint32_t)(c0 >> 32) | (uint32_t)(c1 >> 32) << 16,
                                        lo[0], lo[1], hi[0] | hi[1] << 16);
    if (cost < thr) { q[0] = (uint64_t)lo[0] | (uint64_t)hi[0] << 32; q[1] = (uint64_t)lo[1] | (uint64_t)hi[1] << 32; }
    return tf_cost_weight(cost, thr, magic_thr);
}

template <int RPL>
__global__ __launch_bounds__(256) void k_subpel_temporal_filter_bgr(TfSpBgrArgs a)
{
    __shared__ uint32_t magic_s[17];
    if (threadIdx.x < 17) magic_s[threadIdx.x] = a.magic_s[threadIdx.x];
    __syncthreads();
    const TfFrame f = tf_frame(a);
    const uint8_t *C = f.C, *P = f.P, *N = f.N;
    const bool has_p = f.has_p, has_n = f.has_n;
    const mv_t *QP = f.GP, *QN = f.GN;
    const int CW = a.cw;
    const uint32_t thr = (uint32_t)a.thr, magic_thr = a.magic_thr;
    uint32_t np = 0, nn = 0, wsum = 0, dsum = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        const int fy = oy - a.pad_y, fx = 2 * x0 - a.pad_x;    // the run's first pixel in frame coordinates
        if (fy + 1 < 0 || fy >= a.fh || fx + 2 * n <= 0 || fx >= a.fw) {      // no pixel of the run is in the frame
            if (!a.partial && !a.wmap) continue;
        }
        const size_t g0 = (size_t)cy * a.q4_pitch + x0;
        uint32_t gp[4] = {0, 0, 0, 0}, gn[4] = {0, 0, 0, 0};
        if (has_p) load_mv4(QP + g0, n, gp);
        if (has_n) load_mv4(QN + g0, n, gn);
        const bool whole = bgr_run_whole(n, fx, a.fw);        // the run's 8 pixels lie inside a frame row
        uint64_t crow[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's own two rows, 24 bytes each
        if (whole) bgr_load_rows(C, a.bgr_pitch, a.fh, fx, fy, crow);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint64_t rows[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's two output rows
        uint32_t ws = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ox = 2 * (x0 + j);
            uint64_t c[2];
#pragma unroll
            for (int yy = 0; yy < 2; ++yy)
                c[yy] = whole ? bgr_row_get(crow[yy], j) : bgr_two(C, a.bgr_pitch, a.fw, a.fh, fx + 2 * j, fy + yy);
            uint64_t qp[2] = {0, 0}, qn[2] = {0, 0};
            const uint32_t wp = has_p ? stf_bgr_weight(P, a, ox, oy, gp[j], c[0], c[1], thr, magic_thr, qp) : 0u;
            const uint32_t wn = has_n ? stf_bgr_weight(N, a, ox, oy, gn[j], c[0], c[1], thr, magic_thr, qn) : 0u;
            const uint32_t S = 8u + wp + wn, m = magic_s[wp + wn], half = S >> 1;
            uint32_t diff = 0;
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                uint64_t px = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const uint32_t v = __umulhi(8u * ((uint32_t)(c[yy] >> (8 * q)) & 0xffu) + wp * ((uint32_t)(qp[yy] >> (8 * q)) & 0xffu) +
                                                wn * ((uint32_t)(qn[yy] >> (8 * q)) & 0xffu) + half, m);
                    px |= (uint64_t)v << (8 * q);
                }
                bgr_row_put(rows[yy], j, px);
                diff = __builtin_amdgcn_sad_u8((uint32_t)px, (uint32_t)c[yy], diff);
                diff = __builtin_amdgcn_sad_u8((uint32_t)(px >> 32), (uint32_t)(c[yy] >> 32), diff);
            }
            ws |= (wp | wn << 4) << (8 * j);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                np += wp != 0u; nn += wn != 0u;
                wsum += wp + wn;
                dsum += diff;
            }
        }
        if (a.out) bgr_store_rows(a.out + blockIdx.z * a.out_stride, a.out_pitch, a.fw, a.fh, fx, fy, n, whole, rows);
        if (a.wmap) store_bytes4(a.wmap + (size_t)cy * a.wmap_pitch + x0, n, ws);
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, (size_t)blockIdx.y * gridDim.z + blockIdx.z, part, np, nn, wsum, dsum);
}

// =======================================================================================
// K14.  Composition of two cell grids (the CELL COMPOSITION RULE of include/bbme.h): cell (cx, cy) of A with vector a lands at
// t = ((2 cx, 2 cy) << u) + a, looks up B at the cell c' whose origin is nearest (ties upward, clamped into the grid) and gets
// sat16(a + B[c']).  Layout is K6's and K9's: the shared split of runs of 4 cells (gather_index / gather_split), A by load_mv4
// (rows a_pitch cells apart), B as one dword gather per cell (rows b_pitch apart), the four results as one 16-byte store where the
// run is whole and its address 16-byte aligned (a caller's rows need not be), word by word otherwise.  blockIdx.z = the frame of a
// run: A, B and the output each base + z stride (words), so that one launch composes every slot of a chain; blockIdx.y is 1 (the
// composition exists on chains only, which have one row of pairs).
// No index leaves the grid for any int16: |t| <= 2^16 + 2^15 in 32 bits, c' is clamped before it is used.
// Statistics over the window in cells: cells whose c' was clamped, cells that saturated; a lane holds at most 4 RPL of each
// (store_partial4 with two idle words, frame = z, then k_mc_reduce: no atomics).
// A template, as K12b: a template's code lies behind the estimate's template kernels in the code object, a plain kernel's before.
// =======================================================================================
struct CmpArgs {
    const mv_t *a, *b;                    // cw entries per row, rows a_pitch / b_pitch cells apart
    mv_t *out;                            // rows out_pitch cells apart, or null
    unsigned long long *partial;          // per frame and workgroup {clamped, saturated, 0, 0}; or null
    long long a_z, b_z;                   // words from frame to frame
    size_t out_stride;                    // words from frame to frame
    int cw, ch, a_pitch, b_pitch, out_pitch, ushift;
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

constexpr int kCmpRunsPerLane = 2;

template <int RPL>
__global__ __launch_bounds__(256) void k_compose_cells(CmpArgs a)
{
    const long long z = blockIdx.z;
    const mv_t *A = a.a + z * a.a_z, *B = a.b + z * a.b_z;
    const int CW = a.cw, CH = a.ch, u = a.ushift, half = 1 << u;
    uint32_t nclamp = 0, nsat = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        uint32_t m[4], o[4] = {0, 0, 0, 0};
        load_mv4(A + (size_t)cy * a.a_pitch + x0, n, m);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ax = mv_x(m[j]), ay = mv_y(m[j]);
            const int px = (((2 * (x0 + j)) << u) + ax + half) >> (u + 1), py = (((2 * cy) << u) + ay + half) >> (u + 1);
            const int qx = min(max(px, 0), CW - 1), qy = min(max(py, 0), CH - 1);
            const mv_t e = B[(size_t)qy * a.b_pitch + qx];
            const int sx = ax + mv_x(e), sy = ay + mv_y(e);
            const int rx = min(max(sx, -32768), 32767), ry = min(max(sy, -32768), 32767);
            o[j] = mv_pack(rx, ry);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                nclamp += (qx != px) | (qy != py);
                nsat += (rx != sx) | (ry != sy);
            }
        }
        if (a.out) {
            mv_t *dst = a.out + blockIdx.z * a.out_stride + (size_t)cy * a.out_pitch + x0;
            if (n == 4 && ((uintptr_t)dst & 15u) == 0) *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
            else for (int j = 0; j < n; ++j) dst[j] = o[j];
        }
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, blockIdx.z, part, nclamp, nsat, 0u, 0u);
}

// =======================================================================================
// K15.  Motion-compensated temporal filter over TWO frames on each side (the WIDE TEMPORAL FILTER RULE of include/bbme.h): K13
// with up to four neighbours, k = 0 .. 3 = P1, N1, P2, N2, each a plane x[k] with a quarter-pel grid g[k] on C.  Each neighbour's
// validity, samples, cost and weight are K13's (tf_weight<true>), independent of the others; S = 8 + sum w_k (8..40) and
// out = (8 C + sum w_k X'_k + S / 2) / S.
// Layout is K13's and made of the same pieces (gather_index / gather_split, load_mv4 with rows q4_pitch cells apart, load_cells4,
// rows_put / store_rows2), but the kernel keeps a loop of its own over its neighbours and is not tf_body: head, map, magics and
// statistics all differ with the neighbour count.  The weight map is one uint16 per cell, w_k << 4 k: one aligned 8-byte store
// where the run is whole and its address 8-byte aligned, uint16 by uint16 otherwise; it is stored before the rows (in the other
// order the compiler spills 34 SGPRs to lanes instead of 8).
// blockIdx.z = the frame of a run; every plane is addressed base + z plane_z (bytes) and every grid base + z g_z (words).  Frame z
// of a run of gridDim.z has min(2, z + first_prev) previous and min(2, gridDim.z - 1 - z + last_next) next neighbours: P1 / N1
// are read when that is >= 1, P2 / N2 when it is 2, and only where x[k] is not null.  One launch so serves the slots of a chain
// (first_prev, last_next = how many slots the chain has before the first and after the last frame of the run, at most 2) as well
// as a caller's single frame (both 2: the null pointers alone decide).
// The division by thr is K9's; the one by S is K9's multiply-shift with magic = floor(2^32 / S) + 1 = (2^32 + e) / S, 0 < e <= S:
// umulhi(n, magic) = floor(n / S) for n e < 2^32, and here n <= 255 * 40 + 20 = 10220, e <= 40.  The 33 magics of S = 8..40 come
// with the arguments and are read from LDS.
// Statistics: six counters in 32 bits per lane (at most 4 RPL cells: a count each, a weight sum <= 32, a change <= 1020), through
// shuffles to two partial quadruples per workgroup (store_partial4, frames 2 z and 2 z + 1: {w_0 > 0, .. w_3 > 0} and {weights,
// |out - C|, 0, 0}), then k_mc_reduce over 2 gridDim.z quadruples: no atomics.
// A template, as K12b and K13.
// =======================================================================================
struct WtfArgs {
    const uint8_t *cur;                   // level-0 padded plane, pitch = width
    const uint8_t *x[4];                  // P1, N1, P2, N2; null = no such neighbour at all
    const mv_t *g[4];                     // their quarter-pel grids on C: cw entries per row, rows q4_pitch cells apart
    uint8_t *out;                         // frames (rows out_pitch, frames out_stride bytes apart), or null
    uint16_t *wmap;                       // one uint16 per cell (rows wmap_pitch uint16 apart; one-frame launches only), or null
    unsigned long long *partial;          // per frame and workgroup, two quadruples; or null
    long long plane_z, g_z;               // from frame to frame: bytes, words
    size_t out_stride;
    int width, height, cw, ch, thr, out_pitch, wmap_pitch, q4_pitch;
    int first_prev, last_next;            // 0..2
    uint32_t magic_thr;                   // floor(2^32 / thr) + 1; not used at thr = 1
    uint32_t magic_s[33];                 // floor(2^32 / S) + 1 for S = 8..40
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

template <int RPL>
__global__ __launch_bounds__(256) void k_wide_temporal_filter(WtfArgs a)
{
    __shared__ uint32_t magic_s[33];
    if (threadIdx.x < 33) magic_s[threadIdx.x] = a.magic_s[threadIdx.x];
    __syncthreads();
    const long long z = blockIdx.z;
    const int prevs = min(2, (int)blockIdx.z + a.first_prev), nexts = min(2, (int)(gridDim.z - 1 - blockIdx.z) + a.last_next);
    const uint8_t *C = a.cur + z * a.plane_z;
    const uint8_t *X[4];
    const mv_t *Q[4];
    bool has[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        has[k] = a.x[k] && ((k & 1) ? nexts : prevs) > (k >> 1);
        X[k] = has[k] ? a.x[k] + z * a.plane_z : nullptr;
        Q[k] = has[k] ? a.g[k] + z * a.g_z : nullptr;
    }
    const int W = a.width, H = a.height, CW = a.cw;
    const uint32_t thr = (uint32_t)a.thr, magic_thr = a.magic_thr;
    uint32_t cnt[4] = {0, 0, 0, 0}, wsum = 0, dsum = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        const size_t g0 = (size_t)cy * a.q4_pitch + x0;
        uint32_t g[4][4] = {}, c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (has[k]) load_mv4(Q[k] + g0, n, g[k]);
        load_cells4(C, W, oy, x0, n, c);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint32_t rows[2][2] = {{0, 0}, {0, 0}}, ws[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ox = 2 * (x0 + j);
            uint32_t w[4], q[4], wt = 0, wm = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q[k] = 0;
                w[k] = has[k] ? tf_weight<true>(X[k], W, H, ox, oy, g[k][j], c[j], thr, magic_thr, &q[k]) : 0u;
                wt += w[k];
                wm |= w[k] << (4 * k);
            }
            const uint32_t S = 8u + wt, m = magic_s[wt], half = S >> 1;
            uint32_t px = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                uint32_t num = 8u * ((c[j] >> (8 * p)) & 0xffu) + half;
#pragma unroll
                for (int k = 0; k < 4; ++k) num += w[k] * ((q[k] >> (8 * p)) & 0xffu);
                px |= __umulhi(num, m) << (8 * p);
            }
            rows_put(rows, j, px);
            ws[j >> 1] |= wm << (16 * (j & 1));
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) cnt[k] += w[k] != 0u;
                wsum += wt;
                dsum += __builtin_amdgcn_sad_u8(px, c[j], 0u);
            }
        }
        if (a.wmap) {
            uint16_t *d = a.wmap + (size_t)cy * a.wmap_pitch + x0;
            if (n == 4 && ((uintptr_t)d & 7u) == 0) *reinterpret_cast<uint2 *>(d) = make_uint2(ws[0], ws[1]);
            else for (int j = 0; j < n; ++j) d[j] = (uint16_t)(ws[j >> 1] >> (16 * (j & 1)));
        }
        if (a.out) store_rows2(a.out + blockIdx.z * a.out_stride + (size_t)oy * a.out_pitch + 2 * x0, a.out_pitch, n, rows);
    }
    if (!a.partial) return;
    __shared__ uint32_t part[2][4][4];
    store_partial4(a.partial, 2 * (size_t)blockIdx.z, part[0], cnt[0], cnt[1], cnt[2], cnt[3]);
    store_partial4(a.partial, 2 * (size_t)blockIdx.z + 1, part[1], wsum, dsum, 0u, 0u);
}

// =======================================================================================
// K15b.  The BGR WIDE TEMPORAL FILTER RULE of include/bbme.h: K15 on B,G,R frames, each neighbour's cell taken as K13b takes it.
// Neighbours k = 0 .. 3 = P1, N1, P2, N2, each a colour frame x[k] with a quarter-pel grid g[k] on C; for each present one
// (qx, qy) = Q[cy][cx], s = o + (qx >> 2, qy >> 2), f = (qx & 3, qy & 3), valid when every tap of non-zero weight lies in the padded
// view; its cell is the four rounded bilinear samples of each channel (si_bgr_cell: a pixel outside the frame 0, a tap of weight 0
// never addressed), its cost the largest per-channel SAD on the rounded samples (bgr_cell_cost on K9b's cell-row layout) and its
// weight tf_cost_weight's, as stf_bgr_weight does all three.
// The samples are not held until S is known: the numerators 8 C + sum w_k X'_k do not depend on S, so each neighbour's w_k X'_k is
// added into the cell's numerators as the neighbour is done.  They stay in si_bgr_cell's layout, B in bits 0-15 and R in bits
// 16-31 of one dword (each at most 255 * 40 = 10200: no carry from B into R) and G in a dword of its own, so a neighbour costs 8
// multiply-adds a cell and the cell holds 8 dwords whatever the neighbour count; S / 2 is added when S is known.
// Layout is K13b's and K15's, made of the same pieces: the shared split of runs of 4 cells (gather_index / gather_split), the grids
// by load_mv4 with rows q4_pitch cells apart, the run's own rows by bgr_load_rows where the run is whole and inside the frame
// (bgr_two cell by cell otherwise), the output rows by bgr_row_put and bgr_store_rows, K15's uint16 map store (before the rows).  A
// run with no pixel in the frame is skipped before any load unless the map or the statistics are asked for.
// blockIdx.z = the frame of a run; every colour frame is addressed base + z plane_z (bytes: the colour store's slot stride) and
// every grid base + z g_z (words); first_prev / last_next decide which neighbours a slot has, as in K15.
// The divisions are K15's with K15's bounds: by thr as K9; by S, n <= 255 * 40 + 20 = 10220 and e <= 40, the 33 magics of
// S = 8..40 come with the arguments and are read from LDS.
// Statistics as K15: six counters in 32 bits per lane (at most 4 RPL cells: a count each, a weight sum <= 32, a change <= 3060),
// two partial quadruples per workgroup (store_partial4, frames 2 z and 2 z + 1), then k_mc_reduce: no atomics.
// A template, as K12b, K13b and K15: a template's code lies behind the estimate's template kernels in the code object.
// =======================================================================================
// WtfArgs with cur / x[] and out the fw x fh B,G,R frames (rows bgr_pitch and out_pitch bytes apart), width x height the padded
// view, and the frame's place inside that view
struct WtfBgrArgs : WtfArgs {
    int fw, fh, pad_x, pad_y, bgr_pitch;
};

// One neighbour of the cell (c0, c1: its two rows of 6 bytes) with origin (ox, oy) on the padded view: its weight w, and w times
// its rounded samples added into the cell's numerators (ne: B and R, ng: G; [row][pixel])
__device__ __forceinline__ uint32_t wtf_bgr_add(const uint8_t *X, const WtfBgrArgs &a, int ox, int oy, mv_t g, uint64_t c0, uint64_t c1,
                                                uint32_t thr, uint32_t magic_thr, uint32_t (&ne)[2][2], uint32_t (&ng)[2][2])
{
    const int qx = mv_x(g), qy = mv_y(g);
    const int fx = qx & 3, fy = qy & 3;
    const int sx = ox + (qx >> 2), sy = oy + (qy >> 2);
    if (sx < 0 || sy < 0 || sx + 2 + (fx != 0) > a.width || sy + 2 + (fy != 0) > a.height) return 0u;
    uint32_t e[2][2], gr[2][2];
    si_bgr_cell(X, a.bgr_pitch, a.fw, a.fh, sx - a.pad_x, sy - a.pad_y, fx, fy, e, gr);
    uint32_t lo[2], hi[2];                                    // B0 G0 R0 B1; G1 R1
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        lo[r] = (e[r][0] & 0xffu) | gr[r][0] << 8 | (e[r][0] & 0xff0000u) | e[r][1] << 24;
        hi[r] = gr[r][1] | (e[r][1] >> 16) << 8;
    }
    const uint32_t cost = bgr_cell_cost((uint32_t)c0, (uint32_t)c1, (uint32_t)(c0 >> 32) | (uint32_t)(c1 >> 32) << 16,
                                        lo[0], lo[1], hi[0] | hi[1] << 16);
    const uint32_t w = tf_cost_weight(cost, thr, magic_thr);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            ne[r][m] += w * e[r][m];
            ng[r][m] += w * gr[r][m];
        }
    return w;
}

template <int RPL>
__global__ __launch_bounds__(256) void k_wide_temporal_filter_bgr(WtfBgrArgs a)
{
    __shared__ uint32_t magic_s[33];
    if (threadIdx.x < 33) magic_s[threadIdx.x] = a.magic_s[threadIdx.x];
    __syncthreads();
    const long long z = blockIdx.z;
    const int prevs = min(2, (int)blockIdx.z + a.first_prev), nexts = min(2, (int)(gridDim.z - 1 - blockIdx.z) + a.last_next);
    const uint8_t *C = a.cur + z * a.plane_z;
    const uint8_t *X[4];
    const mv_t *Q[4];
    bool has[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        has[k] = a.x[k] && ((k & 1) ? nexts : prevs) > (k >> 1);
        X[k] = has[k] ? a.x[k] + z * a.plane_z : nullptr;
        Q[k] = has[k] ? a.g[k] + z * a.g_z : nullptr;
    }
    const int CW = a.cw;
    const uint32_t thr = (uint32_t)a.thr, magic_thr = a.magic_thr;
    uint32_t cnt[4] = {0, 0, 0, 0}, wsum = 0, dsum = 0;
    // the loop over the lane's runs stays a loop: one run is four cells of four neighbours, 16 inlined si_bgr_cell, and the
    // compiler declines to unroll it further
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        const int oy = 2 * cy;
        const int fy = oy - a.pad_y, fx = 2 * x0 - a.pad_x;    // the run's first pixel in frame coordinates
        if (fy + 1 < 0 || fy >= a.fh || fx + 2 * n <= 0 || fx >= a.fw) {      // no pixel of the run is in the frame
            if (!a.partial && !a.wmap) continue;
        }
        const size_t g0 = (size_t)cy * a.q4_pitch + x0;
        uint32_t g[4][4] = {};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (has[k]) load_mv4(Q[k] + g0, n, g[k]);
        const bool whole = bgr_run_whole(n, fx, a.fw);        // the run's 8 pixels lie inside a frame row
        uint64_t crow[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's own two rows, 24 bytes each
        if (whole) bgr_load_rows(C, a.bgr_pitch, a.fh, fx, fy, crow);
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint64_t rows[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's two output rows
        uint32_t ws[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ox = 2 * (x0 + j);
            uint64_t c[2];
            uint32_t ne[2][2], ng[2][2];                      // the numerators 8 C + sum w_k X'_k
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                c[yy] = whole ? bgr_row_get(crow[yy], j) : bgr_two(C, a.bgr_pitch, a.fw, a.fh, fx + 2 * j, fy + yy);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const uint32_t p = (uint32_t)(c[yy] >> (24 * m));
                    ne[yy][m] = 8u * (p & 0xff00ffu);
                    ng[yy][m] = 8u * ((p >> 8) & 0xffu);
                }
            }
            uint32_t w[4], wt = 0, wm = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[k] = has[k] ? wtf_bgr_add(X[k], a, ox, oy, g[k][j], c[0], c[1], thr, magic_thr, ne, ng) : 0u;
                wt += w[k];
                wm |= w[k] << (4 * k);
            }
            const uint32_t S = 8u + wt, mg = magic_s[wt], half = S >> 1;
            uint32_t diff = 0;
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                uint64_t px = 0;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const uint32_t vb = __umulhi((ne[yy][m] & 0xffffu) + half, mg);
                    const uint32_t vg = __umulhi(ng[yy][m] + half, mg);
                    const uint32_t vr = __umulhi((ne[yy][m] >> 16) + half, mg);
                    px |= (uint64_t)(vb | vg << 8 | vr << 16) << (24 * m);
                }
                bgr_row_put(rows[yy], j, px);
                diff = __builtin_amdgcn_sad_u8((uint32_t)px, (uint32_t)c[yy], diff);
                diff = __builtin_amdgcn_sad_u8((uint32_t)(px >> 32), (uint32_t)(c[yy] >> 32), diff);
            }
            ws[j >> 1] |= wm << (16 * (j & 1));
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) cnt[k] += w[k] != 0u;
                wsum += wt;
                dsum += diff;
            }
        }
        if (a.wmap) {
            uint16_t *d = a.wmap + (size_t)cy * a.wmap_pitch + x0;
            if (n == 4 && ((uintptr_t)d & 7u) == 0) *reinterpret_cast<uint2 *>(d) = make_uint2(ws[0], ws[1]);
            else for (int j = 0; j < n; ++j) d[j] = (uint16_t)(ws[j >> 1] >> (16 * (j & 1)));
        }
        if (a.out) bgr_store_rows(a.out + blockIdx.z * a.out_stride, a.out_pitch, a.fw, a.fh, fx, fy, n, whole, rows);
    }
    if (!a.partial) return;
    __shared__ uint32_t part[2][4][4];
    store_partial4(a.partial, 2 * (size_t)blockIdx.z, part[0], cnt[0], cnt[1], cnt[2], cnt[3]);
    store_partial4(a.partial, 2 * (size_t)blockIdx.z + 1, part[1], wsum, dsum, 0u, 0u);
}

// =======================================================================================
// K16 .. K18b.  The GLOBAL MOTION RULE, the GLOBAL COMPENSATION RULE and its BGR form of include/bbme.h.  They are templates so that they lie
// behind the estimate's template kernels in the code object, as K12b does.
// =======================================================================================

// One exclusion byte per unit of a run, bit j of the result set when unit x0 + j is excluded: one dword when the run is whole and
// its address dword-aligned (a caller's rows need not be), bytes otherwise.
__device__ __forceinline__ uint32_t gm_excluded4(const uint8_t *e, int n)
{
    uint32_t bits = 0;
    if (n == 4 && ((uintptr_t)e & 3u) == 0) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(e);
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= ((v >> (8 * j)) & 0xffu) ? 1u << j : 0u;
    } else {
        for (int j = 0; j < n; ++j) bits |= e[j] ? 1u << j : 0u;
    }
    return bits;
}

// The sixteen-word sibling of store_partial4, for sums that need 64 bits in the lane already: the lane's sixteen 64-bit sums over
// its wave, the four waves' over the workgroup through `part`, stored as the partial of (frame, workgroup) at word
// 16 (frame gridDim.x + blockIdx.x), for k_reduce_words to add up.  All adds are modulo 2^64.
__device__ __forceinline__ void store_partial16(unsigned long long *partial, size_t frame, unsigned long long (&part)[4][16],
                                                unsigned long long (&s)[16])
{
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        unsigned long long v = s[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16)
        partial[16 * (frame * gridDim.x + blockIdx.x) + threadIdx.x] =
            part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// k_mc_reduce's sibling for partials of WORDS (a power of two <= 256) words: one workgroup per pair (blockIdx.x), lane t adds
// word t % WORDS of every (256 / WORDS)-th workgroup's partial, then the slices are added through LDS.
template <int WORDS>
__global__ __launch_bounds__(256) void k_reduce_words(const unsigned long long *partial, int groups, unsigned long long *out)
{
    constexpr int kSlices = 256 / WORDS;
    const unsigned long long *p = partial + (size_t)WORDS * groups * blockIdx.x;
    const int k = threadIdx.x % WORDS, slice = threadIdx.x / WORDS;
    unsigned long long s = 0;
    for (int g = slice; g < groups; g += kSlices) s += p[(size_t)WORDS * g + k];
    __shared__ unsigned long long red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    if ((int)threadIdx.x < WORDS) {
        unsigned long long t = 0;
        for (int q = 0; q < kSlices; ++q) t += red[q * WORDS + threadIdx.x];
        out[(size_t)WORDS * blockIdx.x + threadIdx.x] = t;
    }
}

// K16.  The histogram part: over the window's cells that the exclusion mask does not exclude, the counts of clamp(dx) and of
// clamp(dy) in BINS bins each.  A bounded number of workgroups (gridDim.x <= kVhMaxGroups) stride over the runs of 4 cells, so the
// flush traffic does not grow with the frame; each fills one histogram pair in LDS (2 BINS words = 16 KB) with LDS atomics and
// then adds its non-zero bins to the pair's table in memory (blockIdx.y = pair), which the host zeroes in front of the launch.
// Integer adds commute: the counts are exact whatever the order.
// Contention.  A regularised field is mostly uniform, and 64 lanes adding to one LDS word serialise.  vh_add therefore
// aggregates inside the wave first: the lowest lane still to do broadcasts its bin, the lanes with the same bin are counted by a
// ballot and leave, and that lane adds the count once.  A uniform run costs one LDS add per wave and component; 64 distinct
// bins cost 64 turns of the loop.  The loop runs in wave-uniform control flow (every lane of the wave takes part, `on` says
// whether it has a value), so ballot and shuffle see whole waves.
struct VhArgs {
    const mv_t *cells;                    // cw entries per row, rows `pitch` cells apart
    const uint8_t *excl;                  // one byte per cell, rows excl_pitch bytes apart, non-zero = excluded; or null
    uint32_t *hist;                       // per pair 2 BINS words, zero before the launch
    size_t s_cells, s_excl;               // from pair to pair: words, bytes
    int cw, pitch, excl_pitch;
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

constexpr int kVhMaxGroups = 256;                      // one per compute unit of an MI355X

__device__ __forceinline__ void vh_add(uint32_t *h, bool on, uint32_t bin)
{
    unsigned long long todo = __ballot(on);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t b = (uint32_t)__shfl((int)bin, leader);
        const unsigned long long same = __ballot(on && bin == b);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[b], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

template <int BINS>
__global__ __launch_bounds__(256) void k_vector_histogram(VhArgs a)
{
    __shared__ uint32_t h[2 * BINS];
    for (int b = threadIdx.x; b < 2 * BINS; b += 256) h[b] = 0;
    __syncthreads();
    const size_t pair = blockIdx.y;
    const mv_t *Q = a.cells + pair * a.s_cells;
    const uint8_t *E = a.excl ? a.excl + pair * a.s_excl : nullptr;
    for (long long base = (long long)blockIdx.x * 256; base < a.runs; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        int cy = 0, x0 = 0, n = 0;
        uint32_t m[4] = {0, 0, 0, 0}, e = 0;
        if (i < a.runs) {
            gather_split(i, a.runs_per_row, a.cw, cy, x0, n);
            if (cy < a.wy0 || cy >= a.wy1 || x0 + n <= a.wx0 || x0 >= a.wx1) {
                n = 0;                                        // no cell of the run lies in the window: nothing is loaded
            } else {
                load_mv4(Q + (size_t)cy * a.pitch + x0, n, m);
                if (E) e = gm_excluded4(E + (size_t)cy * a.excl_pitch + x0, n);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = j < n && x0 + j >= a.wx0 && x0 + j < a.wx1 && !((e >> j) & 1u);
            vh_add(h, on, (uint32_t)(min(max(mv_x(m[j]), -BINS / 2), BINS / 2 - 1) + BINS / 2));
            vh_add(h + BINS, on, (uint32_t)(min(max(mv_y(m[j]), -BINS / 2), BINS / 2 - 1) + BINS / 2));
        }
    }
    __syncthreads();
    uint32_t *out = a.hist + pair * (size_t)(2 * BINS);
    for (int b = threadIdx.x; b < 2 * BINS; b += 256) {
        const uint32_t v = h[b];
        if (v) atomicAdd(&out[b], v);
    }
}

// K17.  The moments part: every cell's class under a model and a tolerance, the class map and the sixteen words over the window.
// It has k_fb_consistency's shape: a lane takes runs of 4 consecutive cells of one row (2 at a row's end when CW = 2 mod 4), the
// grid arrives as one 16-byte load (load_mv4), the exclusion bytes as one dword where aligned, the map leaves as one dword
// (store_bytes4); blockIdx.y = pair, with the pair's model from a device table (`models`, six words per pair) or, without one,
// from the arguments.  pu and pv advance along the run by 4 m1 and 4 m4 in 64 bits.
// Sums.  One product is up to 2^28 and r up to 2^47, so a lane's sums are 64-bit from the first add, and so are the wave's and
// the workgroup's (store_partial16); k_reduce_words<16> adds the workgroups' partials.  All sums are modulo 2^64, as the rule's.
struct GmArgs {
    const mv_t *cells;                    // cw entries per row, rows `pitch` cells apart
    const uint8_t *excl;                  // one byte per cell, rows excl_pitch bytes apart, non-zero = excluded; or null
    uint8_t *map;                         // one class byte per cell, rows map_pitch bytes apart; or null
    unsigned long long *partial;          // per pair and workgroup the sixteen words; or null (no statistics)
    const int32_t *models;                // six words per pair; or null: `model` for every pair
    int32_t model[6];
    long long tol;
    size_t s_cells, s_excl, s_map;        // from pair to pair: words, bytes, bytes
    int cw, ch, pitch, excl_pitch, map_pitch;
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

constexpr int kGmRunsPerLane = 4;

template <int RPL>
__global__ __launch_bounds__(256) void k_global_moments(GmArgs a)
{
    const size_t pair = blockIdx.y;
    const mv_t *Q = a.cells + pair * a.s_cells;
    const uint8_t *E = a.excl ? a.excl + pair * a.s_excl : nullptr;
    long long m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = a.models ? a.models[6 * pair + k] : a.model[k];
    const int CW = a.cw;
    unsigned long long s[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row (4, or 2 at the row's end)
        gather_split(i, a.runs_per_row, CW, cy, x0, n);
        uint32_t q[4];
        load_mv4(Q + (size_t)cy * a.pitch + x0, n, q);
        const uint32_t e = E ? gm_excluded4(E + (size_t)cy * a.excl_pitch + x0, n) : 0u;
        const long long Y = 4LL * cy + 2 - 2LL * a.ch;
        long long X = 4LL * x0 + 2 - 2LL * CW, pu = m[0] + m[1] * X + m[2] * Y, pv = m[3] + m[4] * X + m[5] * Y;
        const bool in_rows = a.partial && cy >= a.wy0 && cy < a.wy1;
        uint32_t cls = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const long long dx = mv_x(q[j]), dy = mv_y(q[j]);
            uint32_t c = 2u;
            long long res = 0;
            if (!((e >> j) & 1u)) {
                const long long ru = dx * 65536 - pu, rv = dy * 65536 - pv;
                res = (ru < 0 ? -ru : ru) + (rv < 0 ? -rv : rv);
                c = res > a.tol ? 1u : 0u;
            }
            cls |= c << (8 * j);
            if (in_rows && x0 + j >= a.wx0 && x0 + j < a.wx1) {
                s[0] += c == 0u; s[1] += c == 1u; s[2] += c == 2u;
                if (c == 0u) {
                    s[3] += (unsigned long long)res;
                    s[4] += (unsigned long long)X; s[5] += (unsigned long long)Y;
                    s[6] += (unsigned long long)(X * X); s[7] += (unsigned long long)(X * Y); s[8] += (unsigned long long)(Y * Y);
                    s[9] += (unsigned long long)dx; s[10] += (unsigned long long)dy;
                    s[11] += (unsigned long long)(X * dx); s[12] += (unsigned long long)(Y * dx);
                    s[13] += (unsigned long long)(X * dy); s[14] += (unsigned long long)(Y * dy);
                    s[15] += (unsigned long long)(dx * dx + dy * dy);
                }
            }
            X += 4; pu += 4 * m[1]; pv += 4 * m[4];
        }
        if (a.map) store_bytes4(a.map + pair * a.s_map + (size_t)cy * a.map_pitch + x0, n, cls);
    }
    if (!a.partial) return;
    __shared__ unsigned long long part[4][16];
    store_partial16(a.partial, pair, part, s);
}

// K18.  The GLOBAL COMPENSATION RULE: pixel (x, y) takes the SUBPEL RULE's sample of I2 at s = (x, y) + (q >> 2) with the
// fractions q & 3, q = (d (4 / unit) + 32768) >> 16 the model's displacement there in quarter pels; a pixel one of whose taps of
// non-zero weight would leave the plane gets `fill`.  It is k_motion_compensate's sibling: a lane takes runs of 4 pixels of one
// row, the model advances along the run by 2 m1 and 2 m4 per pixel in 64 bits, the run leaves as one dword (store_bytes4) and I1
// is read, as a dword, only for rows that meet the window; blockIdx.y = pair, the model as in K17.
// Loads.  Neighbouring pixels of a zooming or rotating model need not be neighbours in I2, and a single pixel's second column
// and row exist only where the fraction is not 0: sc_row and si_cell read byte s.x + 1 and row s.y + 1 whatever the fraction --
// right for a 2x2 cell, whose second pixel lies there, but one byte or one row past the plane for a lone pixel on its last column
// or row.  So the four taps are byte loads at offsets x1 = (fx != 0) and y1 W: where a fraction is 0 its tap folds onto the
// first (weight 0), and no address leaves the plane that the rule does not name.  The sample is the separable form.
// Statistics over the window [wx0, wx1) x [wy0, wy1) in PIXELS: sse, sad, pixels over the compensated pixels, skipped over the
// others.  A lane sums at most 4 RPL pixels in 32 bits and a wave's sum stays below 2^32: 64 * 4 RPL * 255^2 (store_partial4,
// frame = pair; k_mc_reduce).
struct GcArgs {
    const uint8_t *img1, *img2;           // packed width x height planes; img1 may be null without statistics
    uint8_t *out;                         // compensated plane (rows out_pitch bytes apart), or null
    unsigned long long *partial;          // per pair and workgroup {sse, sad, pixels, skipped}; or null (no statistics)
    const int32_t *models;                // six words per pair; or null: `model` for every pair
    int32_t model[6];
    size_t s_plane;                       // bytes from pair to pair
    int width, height, mul, fill, out_pitch;      // mul = 4 / unit
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(width / 4)
    long long runs;                       // runs_per_row * height
};

constexpr int kGcRunsPerLane = 4;

template <int RPL>
__global__ __launch_bounds__(256) void k_global_compensate(GcArgs a)
{
    const size_t pair = blockIdx.y;
    const uint8_t *I2 = a.img2 + pair * a.s_plane;
    long long m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = a.models ? a.models[6 * pair + k] : a.model[k];
    const int W = a.width, H = a.height;
    const long long mul = a.mul;
    uint32_t sse = 0, sad = 0, npix = 0, nskip = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int y, x0, n;                                         // n pixels of the run lie inside the row
        gather_split(i, a.runs_per_row, W, y, x0, n);
        const long long X = 2LL * x0 + 1 - W, Y = 2LL * y + 1 - H;
        long long pu = m[0] + m[1] * X + m[2] * Y, pv = m[3] + m[4] * X + m[5] * Y;
        uint32_t mc = 0, ok = 0;                              // sampled bytes; bit j: pixel x0 + j was compensated
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const long long qx = (pu * mul + 32768) >> 16, qy = (pv * mul + 32768) >> 16;
            const uint32_t fx = (uint32_t)(qx & 3), fy = (uint32_t)(qy & 3);
            const int x1 = fx != 0, y1 = fy != 0;
            const long long sx = x0 + j + (qx >> 2), sy = y + (qy >> 2);
            if (sx >= 0 && sx + 1 + x1 <= W && sy >= 0 && sy + 1 + y1 <= H) {
                const uint8_t *p = I2 + (size_t)sy * W + (size_t)sx, *p1 = p + (size_t)y1 * W;
                const uint32_t h0 = (4u - fx) * p[0] + fx * p[x1], h1 = (4u - fx) * p1[0] + fx * p1[x1];
                mc |= (((4u - fy) * h0 + fy * h1 + 8u) >> 4) << (8 * j);
                ok |= 1u << j;
            }
            pu += 2 * m[1]; pv += 2 * m[4];
        }
        if (a.out) {
            uint32_t keep = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) keep |= ((ok >> j) & 1u) ? 0xffu << (8 * j) : 0u;
            store_bytes4(a.out + (size_t)y * a.out_pitch + x0, n, (mc & keep) | ((uint32_t)a.fill * 0x01010101u & ~keep));
        }
        if (a.partial && y >= a.wy0 && y < a.wy1) {
            const uint8_t *r1 = a.img1 + pair * a.s_plane + (size_t)y * W + x0;
            uint32_t ref = 0;
            if (n == 4) ref = reinterpret_cast<const ua_u32 *>(r1)->v;
            else for (int j = 0; j < n; ++j) ref |= (uint32_t)r1[j] << (8 * j);
            for (int j = 0; j < n; ++j) {
                if (x0 + j < a.wx0 || x0 + j >= a.wx1) continue;
                if ((ok >> j) & 1u) {
                    const int d = (int)((mc >> (8 * j)) & 0xffu) - (int)((ref >> (8 * j)) & 0xffu);
                    sse += (uint32_t)(d * d);
                    sad += (uint32_t)abs(d);
                    ++npix;
                } else {
                    ++nskip;
                }
            }
        }
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, pair, part, sse, sad, npix, nskip);
}

// K18b.  The BGR GLOBAL COMPENSATION RULE: K18 on the zero-padded view of a colour frame, written as the unpadded frame.  Output
// pixel (x, y) of the fw x fh frame has the X, Y of the frame's own centre (the padded plane's are the same numbers), q, i and f
// are K18's, and s = (x, y) + i in FRAME coordinates: the pixel is compensated when s lies in [-pad_x, fw + pad_x - 1 - (fx != 0)]
// x [-pad_y, fh + pad_y - 1 - (fy != 0)], the padded plane, and a tap outside [0, fw) x [0, fh) is the padding's 0.  Same split as
// K18 -- a lane takes runs of 4 pixels of one frame row, the model advances by 2 m1 and 2 m4 per pixel in 64 bits --;
// blockIdx.y = FRAME of a run of frames frame_stride bytes apart in both inputs and out_stride in the output, the frame's model
// from a device table (`models`, six words per frame) or, without one, `model` for all of them.
// Loads.  The two taps of a row are six adjacent bytes, one unaligned dword and one u16 where both lie in the frame (gcb_row);
// where they straddle the frame's edge the one inside is a u16 and a byte, and a tap outside is 0 without a load.  The second
// column is loaded only where fx != 0 and the second row only where fy != 0, so no tap of weight 0 is read and no address
// leaves the frame's fw x fh pixels: a lone pixel is 3 bytes, never a dword that would reach into the next pixel or past the row.
// Stores: the run's 12 bytes by bgr_run_put / bgr_store_run.  Frame 1's run arrives as three unaligned dwords, for rows that meet
// the window only.
// Statistics over the window [wx0, wx1) x [wy0, wy1) in FRAME pixels: sse and sad over the three channels of the compensated
// pixels, pixels and skipped in pixels.  Bound: a lane sums at most 4 RPL pixels of three channels, 4 * 4 * 3 * 255^2 = 3 121 200 at
// RPL = 4, and a wave 64 times that, 64 * 4 RPL * 3 * 255^2 = 199 756 800 < 2^32 (up to RPL = 86); the workgroup's sums are 64-bit
// (store_partial4, frame = blockIdx.y; k_mc_reduce).
struct GcBgrArgs {
    const uint8_t *bgr1, *bgr2;           // fw x fh colour frames, rows bgr_pitch bytes apart; bgr1 may be null without statistics
    uint8_t *out;                         // compensated frames (rows out_pitch, frames out_stride bytes apart), or null
    unsigned long long *partial;          // per frame and workgroup {sse, sad, pixels, skipped}; or null (no statistics)
    const int32_t *models;                // six words per frame; or null: `model` for every frame
    int32_t model[6];
    size_t frame_stride, out_stride;      // bytes from frame to frame: inputs, output
    int fw, fh, pad_x, pad_y, bgr_pitch, out_pitch, mul, fill;      // mul = 4 / unit
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(fw / 4)
    long long runs;                       // runs_per_row * fh
};

constexpr int kGcBgrRunsPerLane = 4;

// pixel (x, y) of a colour frame as three bytes B,G,R from bit 0 up
__device__ __forceinline__ uint32_t gcb_pixel(const uint8_t *p)
{
    return (uint32_t)reinterpret_cast<const ua_u16 *>(p)->v | (uint32_t)p[2] << 16;
}

// Pixel (x, y) of a colour frame in bits 0-23 and, with x1, pixel (x + 1, y) in bits 24-47; a pixel outside the frame is 0 and is
// not loaded, and without x1 the second one is not looked at.
__device__ __forceinline__ uint64_t gcb_row(const uint8_t *img, int pitch, int fw, int fh, int x, int y, int x1)
{
    if (y < 0 || y >= fh) return 0;
    const uint8_t *row = img + (size_t)y * pitch;
    const bool in0 = x >= 0 && x < fw, in1 = x1 && x + 1 >= 0 && x + 1 < fw;
    if (in0 && in1)
        return (uint64_t)reinterpret_cast<const ua_u32 *>(row + 3 * x)->v | (uint64_t)reinterpret_cast<const ua_u16 *>(row + 3 * x + 4)->v << 32;
    if (in0) return gcb_pixel(row + 3 * x);
    if (in1) return (uint64_t)gcb_pixel(row + 3 * (x + 1)) << 24;
    return 0;
}

template <int RPL>
__global__ __launch_bounds__(256) void k_global_compensate_bgr(GcBgrArgs a)
{
    const size_t frame = blockIdx.y;
    const uint8_t *C2 = a.bgr2 + frame * a.frame_stride;
    long long m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = a.models ? a.models[6 * frame + k] : a.model[k];
    const int FW = a.fw, FH = a.fh;
    const long long mul = a.mul;
    uint32_t sse = 0, sad = 0, npix = 0, nskip = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int y, x0, n;                                         // n pixels of the run lie inside the frame row
        gather_split(i, a.runs_per_row, FW, y, x0, n);
        const long long X = 2LL * x0 + 1 - FW, Y = 2LL * y + 1 - FH;
        long long pu = m[0] + m[1] * X + m[2] * Y, pv = m[3] + m[4] * X + m[5] * Y;
        uint32_t run[3] = {0, 0, 0}, ok = 0;                  // the sampled pixels; bit j: pixel x0 + j was compensated
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const long long qx = (pu * mul + 32768) >> 16, qy = (pv * mul + 32768) >> 16;
            const uint32_t fx = (uint32_t)(qx & 3), fy = (uint32_t)(qy & 3);
            const int x1 = fx != 0, y1 = fy != 0;
            const long long sx = x0 + j + (qx >> 2), sy = y + (qy >> 2);
            if (sx >= -a.pad_x && sx + 1 + x1 <= (long long)FW + a.pad_x && sy >= -a.pad_y && sy + 1 + y1 <= (long long)FH + a.pad_y) {
                const uint64_t t0 = gcb_row(C2, a.bgr_pitch, FW, FH, (int)sx, (int)sy, x1);
                const uint64_t t1 = y1 ? gcb_row(C2, a.bgr_pitch, FW, FH, (int)sx, (int)sy + 1, x1) : 0;
                uint32_t px = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t h0 = (4u - fx) * ((uint32_t)(t0 >> (8 * c)) & 0xffu) + fx * ((uint32_t)(t0 >> (24 + 8 * c)) & 0xffu);
                    const uint32_t h1 = (4u - fx) * ((uint32_t)(t1 >> (8 * c)) & 0xffu) + fx * ((uint32_t)(t1 >> (24 + 8 * c)) & 0xffu);
                    px |= (((4u - fy) * h0 + fy * h1 + 8u) >> 4) << (8 * c);
                }
                bgr_run_put(run, j, px);
                ok |= 1u << j;
            }
            pu += 2 * m[1]; pv += 2 * m[4];
        }
        if (a.partial && y >= a.wy0 && y < a.wy1) {
            const uint8_t *r1 = a.bgr1 + frame * a.frame_stride + (size_t)y * a.bgr_pitch + (size_t)3 * x0;
            uint32_t ref[3] = {0, 0, 0};
            if (n == 4) {
#pragma unroll
                for (int d = 0; d < 3; ++d) ref[d] = reinterpret_cast<const ua_u32 *>(r1)[d].v;
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    if (k < 3 * n) ref[k >> 2] |= (uint32_t)r1[k] << (8 * (k & 3));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= n || x0 + j < a.wx0 || x0 + j >= a.wx1) continue;
                if ((ok >> j) & 1u) {
#pragma unroll
                    for (int k = 3 * j; k < 3 * j + 3; ++k) {
                        const int d = (int)((run[k >> 2] >> (8 * (k & 3))) & 0xffu) - (int)((ref[k >> 2] >> (8 * (k & 3))) & 0xffu);
                        sse += (uint32_t)(d * d);
                        sad += (uint32_t)abs(d);
                    }
                    ++npix;
                } else {
                    ++nskip;
                }
            }
        }
        if (a.out) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n && !((ok >> j) & 1u)) bgr_run_put(run, j, (uint32_t)a.fill * 0x010101u);
            bgr_store_run(a.out + frame * a.out_stride + (size_t)y * a.out_pitch + (size_t)3 * x0, n, run);
        }
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, frame, part, sse, sad, npix, nskip);
}

// =======================================================================================
// K11b.  The BGR COMPENSATION RULE of include/bbme.h: K11 on the zero-padded view of a colour frame, written as the unpadded frame.
// Cell (cx, cy) of the padded W0 x H0 plane with origin o = (2 cx, 2 cy) and (qx, qy) = mul * G[cy][cx] in 32 bits (mul = 4 / unit:
// 4 for a grid of integer cells, whose 4 G need not fit int16, 1 for a quarter-pel grid) has s = o + (qx >> 2, qy >> 2) and
// f = (qx & 3, qy & 3); it is compensated under K11's condition on the padded plane and its pixels that lie inside the fw x fh
// frame, at o + (j, k) - (pad_x, pad_y), take in every channel the SUBPEL RULE's sample, a tap outside the frame being the padding's
// 0; a skipped cell's get `fill`.  K11's layout from the shared pieces: runs of 4 cells of one cell row (gather_index /
// gather_split), G by load_mv4 with rows grid_pitch cells apart, blockIdx.y = pair (colour frames frame_stride bytes, grids s_grid
// words apart).  A run with no pixel in the frame loads nothing.
// Loads.  The cell is K12b's si_bgr_cell at s - pad: up to three frame rows of nine bytes at an arbitrary byte address, unaligned
// dwords where the pixels lie inside the row, single bytes at the frame's edges, a pixel outside 0 without a load and a row or
// column of weight 0 not loaded: no byte outside the frame's fw x fh pixels is read.  Stores are K7b's (bgr_row_put /
// bgr_store_rows: six dwords a row where the run is whole and the row's address dword-aligned, bytes otherwise, nothing outside the
// frame).  Frame 1's rows arrive by bgr_load_rows where the run is whole and by bgr_two cell by cell otherwise, only for cell rows
// that meet the window.
// Statistics over the window [wx0, wx1) x [wy0, wy1) in FRAME pixels: sse and sad over the three channels of the compensated
// cells' window pixels, pixels and skipped in pixels.  Bound: a lane sums at most RPL runs of 16 pixels of three channels in 32
// bits, RPL * 16 * 3 * 255^2 = RPL * 3 121 200, and a wave 64 times that, RPL * 199 756 800, which stays below 2^32 up to RPL = 21;
// RPL = kCbRunsPerLane = 2 (K11's): 399 513 600.  The workgroup's sums are 64-bit (store_partial4, frame = pair; k_mc_reduce): no
// atomics.  A template, as K12b: its code lies behind the estimate's template kernels in the code object.
// =======================================================================================
struct CbArgs {
    const uint8_t *bgr1, *bgr2;           // fw x fh colour frames, rows bgr_pitch bytes apart; bgr1 may be null without statistics
    const mv_t *grid;                     // cw entries per row, rows grid_pitch cells apart
    uint8_t *out;                         // the compensated fw x fh frame (rows out_pitch bytes apart; one pair only), or null
    unsigned long long *partial;          // per pair and workgroup {sse, sad, pixels, skipped}; or null (no statistics)
    size_t frame_stride, s_grid;          // from pair to pair: bytes, words
    int fw, fh, pad_x, pad_y, cw, grid_pitch, bgr_pitch, out_pitch, mul, fill;      // mul = 4 / unit
    int wx0, wy0, wx1, wy1;
    int runs_per_row;                     // ceil(cw / 4)
    long long runs;                       // runs_per_row * ch
};

constexpr int kCbRunsPerLane = 2;

template <int RPL>
__global__ __launch_bounds__(256) void k_compensate_bgr(CbArgs a)
{
    const size_t pair = blockIdx.y;
    const uint8_t *C2 = a.bgr2 + pair * a.frame_stride;
    const mv_t *G = a.grid + pair * a.s_grid;
    const int FW = a.fw, FH = a.fh, W0 = FW + 2 * a.pad_x, H0 = FH + 2 * a.pad_y;
    const uint64_t fill6 = (uint64_t)a.fill * 0x010101010101ull;
    uint32_t sse = 0, sad = 0, npix = 0, nskip = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const long long i = gather_index<RPL>(r);
        if (i >= a.runs) break;
        int cy, x0, n;                                        // n cells of the run lie inside the row
        gather_split(i, a.runs_per_row, a.cw, cy, x0, n);
        const int oy = 2 * cy;
        const int ry = oy - a.pad_y, rx = 2 * x0 - a.pad_x;   // the run's first pixel in frame coordinates
        if (ry + 1 < 0 || ry >= FH || rx + 2 * n <= 0 || rx >= FW) continue;          // no pixel of the run is in the frame
        uint32_t g[4];
        load_mv4(G + (size_t)cy * a.grid_pitch + x0, n, g);
        const bool whole = bgr_run_whole(n, rx, FW);
        const bool stat = a.partial && ry + 1 >= a.wy0 && ry < a.wy1;
        uint64_t ref[2][3] = {{0, 0, 0}, {0, 0, 0}};          // frame 1's two rows of a whole run
        if (stat && whole) bgr_load_rows(a.bgr1 + pair * a.frame_stride, a.bgr_pitch, FH, rx, ry, ref);
        uint64_t rows[2][3] = {{0, 0, 0}, {0, 0, 0}};         // the run's two output rows, 24 bytes each
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int qx = a.mul * mv_x(g[j]), qy = a.mul * mv_y(g[j]);
            const int fx = qx & 3, fy = qy & 3;
            const int sx = 2 * (x0 + j) + (qx >> 2), sy = oy + (qy >> 2);
            const bool ok = sx >= 0 && sx + 2 + (fx != 0) <= W0 && sy >= 0 && sy + 2 + (fy != 0) <= H0;
            uint64_t px[2] = {fill6, fill6};                  // the cell's two rows, six bytes each
            if (ok) {
                uint32_t e[2][2], gr[2][2];
                si_bgr_cell(C2, a.bgr_pitch, FW, FH, sx - a.pad_x, sy - a.pad_y, fx, fy, e, gr);
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    px[y] = 0;
#pragma unroll
                    for (int m = 0; m < 2; ++m) px[y] |= (uint64_t)(e[y][m] | gr[y][m] << 8) << (24 * m);
                }
            }
#pragma unroll
            for (int y = 0; y < 2; ++y) bgr_row_put(rows[y], j, px[y]);
            if (!stat) continue;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                if (ry + y < a.wy0 || ry + y >= a.wy1) continue;
                const uint64_t c1 = whole ? bgr_row_get(ref[y], j)
                                          : bgr_two(a.bgr1 + pair * a.frame_stride, a.bgr_pitch, FW, FH, rx + 2 * j, ry + y);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int X = rx + 2 * j + m;
                    if (X < a.wx0 || X >= a.wx1) continue;
                    if (ok) {
#pragma unroll
                        for (int k = 3 * m; k < 3 * m + 3; ++k) {
                            const int d = (int)((px[y] >> (8 * k)) & 0xffu) - (int)((c1 >> (8 * k)) & 0xffu);
                            sse += (uint32_t)(d * d);
                            sad += (uint32_t)abs(d);
                        }
                        ++npix;
                    } else {
                        ++nskip;
                    }
                }
            }
        }
        if (a.out) bgr_store_rows(a.out, a.out_pitch, FW, FH, rx, ry, n, whole, rows);
    }
    if (!a.partial) return;
    __shared__ uint32_t part[4][4];
    store_partial4(a.partial, pair, part, sse, sad, npix, nskip);
}

}  // namespace bbme
