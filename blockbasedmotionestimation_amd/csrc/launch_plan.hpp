// launch_plan.hpp -- what an estimate launches: every choice of kernel, form, grid, LDS size, stream and fork point, as data.
// Plain C++ (no HIP): bbme_device.hip fills kernel arguments from the context and launches what an entry says;
// tests/cpp/launch_plan_test.cpp checks the plan's invariants, and prints the plan of a geometry and a set of knobs, without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace bbme {

// Everything the environment tunes, with its default.  Read once per context, at creation (read_tuning): never through
// statics, so two contexts of a process may differ and a test may set a knob between them.
struct Tuning {
    int relax_steps = -1;                         // k_reg_iter launches per sweep; -1 = by grid size (BBME_RELAX_STEPS overrides)
    bool split_forced = false;                    // threshold given in the environment: split whatever the plans' lengths (tests)
    long long scan_fine_max = 140000;             // grids of at most this many blocks: scan segments of 4 flags (BBME_SCAN_FINE_MAX)
    long long pass1_lanes_max = 140000;           // grids of at most this many blocks: pass 1 in the chain form (BBME_PASS1_LANES_MAX)
    bool list_split = true;                       // two waves per listed block in the fix-up search of small levels; BBME_LIST_SPLIT
    bool pass1_lazy = true;                       // pass 1 leaves its evaluations to a relaxation launch that follows it; BBME_PASS1_LAZY
    int pass1_strip = -1;                         // the strip form of pass 1 at b <= 4 (k_reg_pass1_strip): -1 = batched contexts only; BBME_PASS1_STRIP
    int split_blocks = 10000;                     // levels of at most this many macroblocks: two waves per block (BBME_SEARCH_SPLIT_BLOCKS)
    int round_cap = 0;                            // > 0: test knob, the regulariser's waves give up after this many rounds
    bool use_memo = true;                         // BBME_MEMO
    int memo_min_block = 16;                      // sweeps at smaller blocks run without it (8: measured slower); BBME_MEMO_MIN_B
    bool memo_forward = false;                    // BBME_MEMO_FORWARD (measured slower: off)
    int local_rounds = 8;                         // k_reg_iter: heavy rounds of a tile per launch; BBME_LOCAL_ROUNDS
    int wide_threshold = 16;                      // solver: queue length above which a round takes the throughput form; BBME_WIDE_THRESHOLD
    int solve_waves = 4;                          // waves per solver workgroup (1, 2 or 4); BBME_SOLVE_WAVES
    bool solve_share = true;                      // k_reg_solve: idle waves of a workgroup take a sibling's surplus; BBME_SOLVE_SHARE=0
    // k_reg_solve<.., true> (the chain rounds speculate along floods) on sweeps at b >= flood_min_b whose grid has at least
    // flood_min_blocks blocks; a flood claims flood_depth blocks ahead of itself (0: never).  BBME_FLOOD_RULE="min_b,min_blocks,depth".
    // The wave-level model (tests/cpp/flood_model.cpp) on cfg3, rounds of the busiest wave at depth 2: 37 + 64 -> 17 + 27 at level 0,
    // b = 8 (130 560 blocks; measured 38 + 64 -> 18 + 23), 23 + 18 -> 14 + 11 at level 1 (32 640; measured 23 + 18 -> 15 + 13); depth 1
    // leaves 57 / 29, depth 3 46 / 33; grids of 8 160 blocks and fewer stay within a round, b <= 4 needs more rounds with it.  A
    // speculating round costs 2.5 us against 1.8, so only the deepest chains pay: level 0, b = 8 -67 us per pyramid, level 1, b = 8
    // (-3 / +6 us) and level 0, b = 16 (+6 / +2 us) do not -- hence 100 000 blocks (profiles/r22_flood_speculation.txt)
    int flood_min_b = 8, flood_depth = 2;
    long long flood_min_blocks = 100000;
    int solve_wgs = 256;                          // most workgroups of k_reg_solve (4 independent waves each); r04: 256 measured 1.5 % ahead of 128 (one wave per SIMD)
    int xcd_remap = 1;                            // XCD-aware block order in k_search_fast; BBME_XCD_REMAP
    bool loose_plan = false;                      // the round-2 search plan without rim rounds; BBME_LOOSE_PLAN (set at all = on)
    long long relax_min_blocks = 300000;          // BBME_RELAX_RULE="min_blocks,max_b,steps_first,steps_second" (relax_steps_for)
    int relax_max_b = 2, relax_s1 = 1, relax_s2 = 0;
    bool force_generic_search = false;            // BBME_GENERIC_SEARCH=1: use k_search_generic everywhere
    bool use_graph = true;                        // BBME_NO_GRAPH=1: eager launches
    bool speculate = true;                        // overlap every level's search with the coarser level's late sweeps; BBME_SPECULATE
    bool fork_both = false;                       // BBME_SPECULATE_BOTH_GRAPHS=1: both directions' graphs forked (bbme_ctx::graph_forked)
    // a speculative search may keep at most this many of its (one-wave) workgroups on a CU: the rest of the CU's wave
    // slots, registers and LDS (40 KB) stay free for the regulariser kernels it runs beside
    // (r04, on the faster solver.  Behind a level of 16 x 16 blocks -- three late block sizes to hide the search behind -- 6-7 is
    // best: cfg3 1.614 / 1.585 / 1.591 / 1.626 ms at 8 / 6 / 7 / 5.  Behind a level of 8 x 8 blocks the sweeps are over long
    // before the search is, and any cap only delays it: cfg4 1.80 / 1.72 / 1.67 / 1.62 ms at 6 / 8 / 10 / 24 = uncapped.)
    int spec_per_cu = 0;                          // BBME_SPEC_WGS_PER_CU; 0 = by the coarser level's block size (spec_lds_for)
    int spec_per_cu_l0 = 0;                       // second value of BBME_SPEC_WGS_PER_CU="other,level0": the level-0 launch's own cap
    // LDS per workgroup of a speculative search launch beside the late sweeps of `coarser_block`-sized level: the occupancy cap
    size_t spec_lds_for(int coarser_block, int level = 1) const
    {
        // (r04: 7, not 6, since the level-0 search -- not the level-1 sweeps beside it, shorter now -- is what the level waits for:
        //  cfg3 1.494 -> 1.470 ms; 8 and more cost the sweeps more than the search gains)
        int per_cu = spec_per_cu > 0 ? spec_per_cu : (coarser_block >= 16 ? 7 : 24);
        if (level == 0 && spec_per_cu_l0 > 0) per_cu = spec_per_cu_l0;
        return ((size_t)(160 - 40) * 1024 / per_cu) / 256 * 256;
    }
    double spec_min_absdiffs = 8e9;               // levels with less search work are not speculated; BBME_SPEC_MIN_GABS
    // where a speculative search's block takes its prediction from (newest_coarse_grid): 1 = the newest grid of the coarser level
    // that is complete when the block starts; 0 = the grid at the fork, every block (A/B runs); 2 = test setting: the LAST grid
    // of the table whatever is complete, so that blocks read grids that are unwritten, mid-write or of another geometry
    int spec_late = 1;                            // BBME_SPEC_LATE
    // the sweep at B the speculative search is forked behind: the first (with late predictions the blocks no longer depend on the
    // grid at the fork; cfg4 1.547 -> 1.514 ms, cfg3 1.460 / 1.463: profiles/r18_late_prediction.txt) or, =0, the second.  Without
    // late predictions (BBME_SPEC_LATE=0) always the second: behind the first, cfg3 loses 2 %
    bool spec_fork_first = true;                  // BBME_SPEC_FORK_FIRST
};

struct Knob {
    const char *name;
    void (*parse)(const char *value, Tuning &t);  // the field(s) the variable sets, with its clamp
};
inline const Knob kKnobs[] = {
    {"BBME_SOLVE_SHARE", [](const char *e, Tuning &t) { t.solve_share = atoi(e) != 0; }},
    {"BBME_SOLVE_WGS", [](const char *e, Tuning &t) { t.solve_wgs = std::max(1, std::min(8192, atoi(e))); }},
    {"BBME_RELAX_STEPS", [](const char *e, Tuning &t) { t.relax_steps = std::max(0, std::min(64, atoi(e))); }},
    {"BBME_SOLVE_WAVES", [](const char *e, Tuning &t) { const int v = atoi(e); t.solve_waves = v <= 1 ? 1 : (v == 2 ? 2 : 4); }},
    {"BBME_TEST_ROUND_CAP", [](const char *e, Tuning &t) { t.round_cap = std::max(0, atoi(e)); }},
    {"BBME_PASS1_LANES_MAX", [](const char *e, Tuning &t) { t.pass1_lanes_max = atoll(e); }},
    {"BBME_SCAN_FINE_MAX", [](const char *e, Tuning &t) { t.scan_fine_max = atoll(e); }},
    {"BBME_PASS1_STRIP", [](const char *e, Tuning &t) { t.pass1_strip = atoi(e) != 0 ? 1 : 0; }},
    {"BBME_LIST_SPLIT", [](const char *e, Tuning &t) { t.list_split = atoi(e) != 0; }},
    {"BBME_PASS1_LAZY", [](const char *e, Tuning &t) { t.pass1_lazy = atoi(e) != 0; }},
    {"BBME_SEARCH_SPLIT_BLOCKS", [](const char *e, Tuning &t) { t.split_blocks = std::max(0, atoi(e)); t.split_forced = true; }},
    {"BBME_NO_GRAPH", [](const char *e, Tuning &t) { t.use_graph = atoi(e) == 0; }},
    {"BBME_SPECULATE", [](const char *e, Tuning &t) { t.speculate = atoi(e) != 0; }},
    {"BBME_SPECULATE_BOTH_GRAPHS", [](const char *e, Tuning &t) { t.fork_both = atoi(e) != 0; }},
    {"BBME_SPEC_WGS_PER_CU", [](const char *e, Tuning &t) {                                   // "n" or "n,n0"
         t.spec_per_cu = std::max(1, std::min(32, atoi(e)));
         if (const char *comma = strchr(e, ',')) t.spec_per_cu_l0 = std::max(1, std::min(32, atoi(comma + 1)));
     }},
    {"BBME_SPEC_MIN_GABS", [](const char *e, Tuning &t) { t.spec_min_absdiffs = atof(e) * 1e9; }},
    {"BBME_SPEC_LATE", [](const char *e, Tuning &t) { t.spec_late = std::max(0, std::min(2, atoi(e))); }},
    {"BBME_SPEC_FORK_FIRST", [](const char *e, Tuning &t) { t.spec_fork_first = atoi(e) != 0; }},
    {"BBME_GENERIC_SEARCH", [](const char *e, Tuning &t) { t.force_generic_search = atoi(e) != 0; }},
    {"BBME_LOCAL_ROUNDS", [](const char *e, Tuning &t) { t.local_rounds = std::max(1, atoi(e)); }},
    {"BBME_WIDE_THRESHOLD", [](const char *e, Tuning &t) { t.wide_threshold = std::max(4, atoi(e)); }},
    {"BBME_MEMO", [](const char *e, Tuning &t) { t.use_memo = atoi(e) != 0; }},
    {"BBME_MEMO_FORWARD", [](const char *e, Tuning &t) { t.memo_forward = atoi(e) != 0; }},
    {"BBME_MEMO_MIN_B", [](const char *e, Tuning &t) { t.memo_min_block = std::max(8, atoi(e)); }},
    {"BBME_XCD_REMAP", [](const char *e, Tuning &t) { t.xcd_remap = atoi(e) != 0; }},
    {"BBME_LOOSE_PLAN", [](const char *, Tuning &t) { t.loose_plan = true; }},                // presence, whatever the value
    {"BBME_RELAX_RULE", [](const char *e, Tuning &t) {                                        // leading fields; the rest keep their defaults
         sscanf(e, "%lld,%d,%d,%d", &t.relax_min_blocks, &t.relax_max_b, &t.relax_s1, &t.relax_s2);
     }},
    {"BBME_FLOOD_RULE", [](const char *e, Tuning &t) {                                        // leading fields, as above
         sscanf(e, "%d,%lld,%d", &t.flood_min_b, &t.flood_min_blocks, &t.flood_depth);
         t.flood_depth = std::max(0, std::min(3, t.flood_depth));
     }},
};

inline Tuning read_tuning(int pairs)
{
    Tuning t;
    // a batched context is throughput-bound (every launch carries several pairs): the chain form of pass 1, which trades
    // instructions for latency, only pays on its small grids (24 pairs as 4 x 6: 53.7 -> 55.0 Mblocks/s)
    if (pairs > 1) t.pass1_lanes_max = 40000;
    for (const auto &k : kKnobs)
        if (const char *e = getenv(k.name)) k.parse(e, t);
    return t;
}

// ---- the plan's inputs ---------------------------------------------------------------------------------------------------------

// A pyramid level as the launches see it (bbme_device.hip's Level holds the same numbers next to its buffers)
struct PlanLevel {
    int width = 0, height = 0, block = 0, range = 0;
    bool fast = false;                            // the strip kernel serves it (fast_kernel_serves)
    bool split_pays = false;                      // the two-wave plan is at least 20 % shorter per wave
    size_t lds_bytes = 0, fast_lds_bytes = 0;     // the search window in LDS: k_search_generic's, k_search_fast's
    int fast_pitch_dw = 0;
    int blocks_at(int b) const { return (width / b) * (height / b); }
};

struct PlanInputs {
    std::vector<PlanLevel> lv;                    // level 0 first
    int pairs = 1;                                // blockIdx.y of every launch
    bool jacobi = false, raster_search = false, relax = true;
    Tuning tune;
    size_t memo_blocks = 0;                       // the SAD memo's room, blocks per pair (memo_room at creation; 0 = no memo)
};

// the strip kernel: blocks of 8, 16 and 32 pixels, ranges its packed keys hold
inline bool fast_kernel_serves(int block, int range) { return (block == 8 || block == 16 || block == 32) && range <= 63; }
inline int generic_pitch_dw(int block, int range) { return (block + 2 * range) / 4 + 2; }
inline size_t generic_lds_bytes(int block, int range)
{
    return ((size_t)(block + 2 * range) * generic_pitch_dw(block, range) + (size_t)block * block / 4) * 4;
}
// the window (+ for B <= 16 a copy of the block, 16-byte aligned, for the rim rounds of the tight plan)
inline size_t fast_lds_bytes(int block, int range, int pitch_dw)
{
    return (((size_t)(block + 2 * range) * pitch_dw + 3) & ~(size_t)3) * 4 + (size_t)block * block;
}
// a round of strips of S rows walks S + B - 1 window rows: the split only pays where it shortens a wave's walk
// (+-32 at B <= 16: 0.6x; +-16: the square is too small to fill 128 lanes with tall strips, 0.94-1.0x -- measured slower).
// `rounds`, `rounds2`: SearchPlan::rounds of the one-wave and of the two-wave plan
inline bool split_shortens_walk(const std::vector<uint32_t> &rounds, const std::vector<uint32_t> &rounds2, int block)
{
    auto walk = [&](const std::vector<uint32_t> &r) {
        int w = 0;
        for (uint32_t code : r) w += (code >> 8) ? block / 4 : (int)(code & 0xffu) + block - 1;   // rim rounds are short
        return w;
    };
    return 5 * walk(rounds2) <= 4 * walk(rounds);
}

// ---- a search launch -----------------------------------------------------------------------------------------------------------

enum PredictionMode { kPredictPlain = 0, kPredictSpeculative = 1, kPredictFixup = 2 };     // kSearchPlain .. of bbme_kernels.hpp
enum class SearchKernel { Generic, Fast, List };  // List: k_fixup_list (list_grid x 256 lanes, no LDS), then k_search_list

struct SearchLaunch {
    SearchKernel kernel = SearchKernel::Generic;
    int level = 0;
    int mode = kPredictPlain;
    int waves = 1;                                // per block: 64 * waves lanes per workgroup
    int grid = 0, list_grid = 0;                  // grid x (y: the pairs)
    size_t lds = 0;                               // dynamic LDS, the speculative launch's floor included
    bool late = false, late_force = false;        // FastSearchArgs::late is attached; every block reads the table's last grid
    bool side_stream = false;
};

// Dynamic LDS of a search launch of level `level` on k_search_fast (`fast_kernel`) or k_search_generic.  `coarser_block` > 0: the
// launch is speculative, beside the sweeps of a level of that block size, and pads its workgroups so that only
// Tuning::spec_lds_for's count of them fits a CU and the regulariser's kernels still find wave slots, registers and LDS.
// Creation raises each kernel's limit to what this gives for a speculative launch (only the one-wave k_search_fast and
// k_search_generic are ever launched with a floor; the others stay at fast_lds_bytes, < 26 KB).
inline size_t search_lds_bytes(const Tuning &t, const PlanLevel &L, bool fast_kernel, int level, int coarser_block)
{
    const size_t floor = coarser_block > 0 ? t.spec_lds_for(coarser_block, level) : 0;
    return std::max(fast_kernel ? L.fast_lds_bytes : L.lds_bytes, floor);
}

inline SearchLaunch plan_search_launch(const PlanInputs &in, int level, int mode)
{
    const Tuning &t = in.tune;
    const PlanLevel &L = in.lv[level];
    const bool has_coarse = level + 1 < (int)in.lv.size();
    const bool speculative = mode == kPredictSpeculative;
    const int nblocks = L.blocks_at(L.block);
    SearchLaunch s;
    s.level = level;
    s.mode = mode;
    s.side_stream = speculative;
    const bool fast = L.fast && !t.force_generic_search && !in.raster_search;
    s.lds = search_lds_bytes(t, L, fast, level, speculative && has_coarse ? in.lv[level + 1].block : 0);
    s.grid = nblocks;
    if (!fast) return s;
    s.kernel = SearchKernel::Fast;
    if (t.xcd_remap) s.grid = (nblocks + 7) / 8 * 8;
    s.late = speculative && has_coarse && t.spec_late != 0;
    s.late_force = s.late && t.spec_late == 2;
    // a level with fewer macroblocks than the chip has SIMDs: one wave per block leaves most SIMDs idle and every busy one
    // with a single wave, so the launch lasts as long as one block does -- two waves share each block then
    const bool split = nblocks <= t.split_blocks && (L.split_pays || t.split_forced);
    bool two_waves = mode == kPredictPlain && split;
    if (mode == kPredictFixup && has_coarse) {
        // list the blocks whose prediction changed, then search those (k_fixup_list, k_search_list)
        s.kernel = SearchKernel::List;
        s.list_grid = (nblocks + 255) / 256;
        s.grid = std::max(64, nblocks / 4);
        // two waves per listed block on the levels that are searched with two waves per block anyway (r04): the list is ONE
        // generation of waves, and on a level of 8 160 blocks (~1 200 listed) halves fill the chip where wholes leave three SIMDs
        // in four idle -- 30.4 -> 24.8 us.  Level 0 (~5 000 listed) stays with one wave per block: at two, the 123 registers of
        // the 128-lane form allow four waves per SIMD, 10 000 halves are two and a half generations, 58.8 -> 65.8 us.
        two_waves = t.list_split && split;
    }
    s.waves = two_waves ? 2 : 1;
    return s;
}

// ---- a sweep launch ------------------------------------------------------------------------------------------------------------

enum GridId { kSmall0 = 0, kSmall1, kBig0, kBig1 };     // Level::small[], Level::big[]
enum class Pass1 { Plain, Strip, Chain, ChainMemo };    // k_reg_pass1, k_reg_pass1_strip, k_reg_pass1_lanes, k_reg_pass1_lanes<.., true>

struct SweepLaunch {
    int level = 0, block = 0, mult = 0;
    GridId from = kSmall0, to = kSmall1;          // the grid it reads (cells of block << old_shift pixels) and the one it leaves
    int old_shift = 0;
    float lambda_mult = 0;
    uint32_t round_cap = 0;
    Pass1 pass1 = Pass1::Plain;
    int pass1_grid = 0;                           // workgroups of 256 lanes
    bool lazy = false;                            // RegArgs::lazy: pass 1 flags its evaluations for the relaxation launch behind it
    int relax_steps = 0, relax_tiles = 0;         // k_reg_iter launches and their workgroups
    bool solve = true;                            // (Jacobi sweeps end with pass 1)
    int solve_segment = 4;                        // k_reg_solve<b, 4 or 16, memo>
    int solve_grid = 0, solve_waves = 0;
    int flood = 0;                                // > 0: k_reg_solve<.., true> (same launch geometry), RegArgs::flood
    bool memo = false;
    int publish = -1;                             // the value the solver stores in the level's word when the sweep is complete, or none
};

// The SAD memo serves the sweeps at b >= memo_min_block whose grid the chain-form pass 1 takes (it is what fills the slots).
// One predicate for the room creation allocates and for the sweeps that are handed the memo.
inline bool memo_eligible(const Tuning &t, const PlanLevel &L, int b)
{
    return t.use_memo && b >= 8 && b >= t.memo_min_block && (long long)L.blocks_at(b) <= t.pass1_lanes_max &&
           L.width <= 8192 && L.height <= 8192;   // (group_sads packs a vector into 2 x 14 bits)
}
// blocks per pair of the largest grid a sweep takes the memo to
inline size_t memo_room(const Tuning &t, const std::vector<PlanLevel> &lv)
{
    size_t room = 0;
    for (const PlanLevel &L : lv)
        for (int b = L.block; b >= 2; b >>= 1)
            if (memo_eligible(t, L, b)) room = std::max(room, (size_t)L.blocks_at(b));
    return room;
}

// relaxation launches (k_reg_iter, 8 local rounds per tile): one more launch (>= 5 us), which only the sweeps with
// heavy first generations repay -- measured on cfg3 / cfg4 / cfg2: large grids of small blocks, one launch per sweep
inline int relax_steps_for(const PlanInputs &in, long long blocks, int b, int mult)
{
    const Tuning &t = in.tune;
    if (t.relax_steps >= 0) return t.relax_steps;
    // BBME_RELAX_RULE="min_blocks,max_b,steps_first,steps_second" (Tuning)
    // (r03: no relaxation launch in front of the second sweep at a block size -- it changes little, and the launch cost more
    // than it took off the solver: 1.760 -> 1.735 ms per cfg3 pair; r04: nor at 4 x 4 -- with the memo-less solver of this
    // round the chain form takes those sweeps' first generations faster than a 40 us launch does: cfg3 1.566 -> 1.547 ms,
    // cfg4 1.605 -> 1.585 ms, interleaved medians of 5 / 4 runs; and, once the solver's waves shared their queues, only on
    // grids of >= 300 000 blocks: cfg3 1.523 -> 1.496, cfg2 0.699 -> 0.680, cfg4 1.611 -> 1.603, reference literals 1.336 -> 1.331)
    return (in.relax && blocks >= t.relax_min_blocks && b <= t.relax_max_b) ? (mult == 1 ? t.relax_s1 : t.relax_s2) : 0;
}

// The sweep of `level` at block size b (a power of two, 2 .. the level's) with lambda multiplier `mult`, on the grid `from` whose
// cells are `from_block` (b or 2 b) pixels.
inline SweepLaunch plan_sweep(const PlanInputs &in, int level, int b, int mult, GridId from, int from_block)
{
    const Tuning &t = in.tune;
    const PlanLevel &L = in.lv[level];
    const int rows = L.height / b, cols = L.width / b;
    const long long blocks = (long long)rows * cols;
    const int P = in.pairs;
    SweepLaunch s;
    s.level = level; s.block = b; s.mult = mult;
    s.from = from;
    s.old_shift = from_block == 2 * b ? 1 : 0;
    // sweeps at the level's own block size ping-pong in small[], the others in big[] (see Level)
    const GridId pool = b == L.block ? kSmall0 : kBig0;
    s.to = from == pool ? GridId(pool + 1) : pool;
    // lambda = (float)(B/2), doubled at every halving (motion_framework.cpp:73,95,151); times
    // (float)lambda_multiplier as at :607
    float lambda = (float)(L.block / 2);
    for (int k = L.block; k > b; k >>= 1) lambda = lambda * 2;
    s.lambda_mult = lambda * (float)mult;
    // every round of a wave either empties part of its queue or follows a real change, and a change can only travel
    // along the raster dependency chain (< 2 * rows + cols blocks): the cap is an exit every wave reaches even if
    // that reasoning were wrong; hitting it raises counters[5] and the result is refused (BBME_ERR_STATE)
    s.round_cap = t.round_cap > 0 ? (uint32_t)t.round_cap : 64u * (uint32_t)(2 * rows + cols + 16);
    // the first sweep at a (level, block size) finds nothing in the memo and rewrites every slot (RegArgs::memo_init, launch_sweep)
    s.memo = !in.jacobi && memo_eligible(t, L, b) && (size_t)blocks <= in.memo_blocks;
    s.relax_steps = in.jacobi ? 0 : relax_steps_for(in, blocks, b, mult);
    const int T = b <= 4 ? 32 : (b == 8 ? 16 : 8);                 // RegIter<b>::T, the tile edge in blocks
    s.relax_tiles = ((cols + T - 1) / T) * ((rows + T - 1) / T);
    // pass 1.  Grids up to ~130 000 blocks: the chain form (a third of the instructions per wave; 16 lanes per block fill the
    // chip from ~32 000 blocks on, and it still wins up to four times that: 1.815 -> 1.78 ms per cfg3 pair; slower from 500 000)
    const int chain_grid = (int)((blocks * 16 + 255) / 256);
    if (s.memo) {
        s.pass1 = Pass1::ChainMemo; s.pass1_grid = chain_grid;
    } else if (b <= 16 && blocks <= t.pass1_lanes_max) {           // (b >= 32: a lane would walk 32+ rows -- 13 against 6 us at b = 32)
        s.pass1 = Pass1::Chain; s.pass1_grid = chain_grid;
    } else {
        const int lpb = b >= 4 ? std::min(b, 64) : 1;              // RegCfg<b>::LPB, lanes per block
        s.pass1 = Pass1::Plain; s.pass1_grid = (int)((blocks * lpb + 255) / 256);
        if (b <= 4) {
            // the large grids of small blocks in a BATCHED context: strips of four blocks per lane, the blocks that need their
            // images listed per wave and worked off densely.  A third fewer vector instructions per pair -- which a batch,
            // throughput-bound, turns into time (24 pairs as 4 x 6: 60.0 -> 62.3 Mblocks/s) -- in a quarter of the waves, each of
            // which now walks its list pass after pass -- which a single pair, latency-bound, pays for (level 0, b = 4: 15.8 ->
            // 53 us; 1.563 -> 1.657 ms per step).  BBME_PASS1_STRIP=0 / 1 forces it off / on.
            // ... and, for any context, the sweeps with a relaxation launch behind pass 1: the strip test alone (level 0: 5.1 us at
            // b = 4, 6.5 at b = 2, against 15.5 / 18.4 for the whole of k_reg_pass1), the blocks that need their images flagged for
            // the relaxation's first round (RegArgs::lazy)
            const bool lazy = t.pass1_lazy && s.relax_steps > 0;
            const bool strip_form = lazy || (t.pass1_strip < 0 ? P > 1 : t.pass1_strip != 0);
            if (strip_form && cols % 4 == 0 && cols >= 12) {
                s.pass1 = Pass1::Strip; s.pass1_grid = (int)((blocks / 4 + 255) / 256);
                s.lazy = lazy;
            }
        }
    }
    // opt-in, NOT the reference's field: a Jacobi sweep takes every block against the field as the previous sweep left it, and no more
    s.solve = !in.jacobi;
    // small grids: scan segments of 4 flags, so that the stale blocks of a row are dealt to four times as many waves
    s.solve_segment = blocks <= t.scan_fine_max ? 4 : 16;
    // a multiple of 8 workgroups: one share per XCD (k_reg_solve's bands)
    s.solve_grid = (int)((std::min<long long>(t.solve_wgs, (blocks + 63) / 64) + 7) / 8 * 8);
    s.solve_waves = t.solve_waves;
    s.flood = (b >= t.flood_min_b && blocks >= t.flood_min_blocks) ? t.flood_depth : 0;   // BBME_FLOOD_RULE (Tuning)
    return s;
}

// ---- the pyramid ---------------------------------------------------------------------------------------------------------------

// A speculative search pays its fork, its fix-up launches and the stretch it puts on the sweeps beside it only when the
// search it hides is long: levels below ~8 G abs-diffs (~90 us) are searched in line (measured: cfg2, cfg1 and the reference's
// literals lose 3-12 % when every level is speculated; cfg3 / cfg4 gain 8-10 % from their two largest levels).
inline bool worth_speculating(const PlanInputs &in, int level)
{
    if (in.jacobi) return false;                     // Jacobi sweeps are too short to hide a search behind
    const PlanLevel &L = in.lv[level];
    const double side = 2.0 * L.range + 1.0;
    const double absdiffs = (double)(L.width / L.block) * (L.height / L.block) * side * side * L.block * L.block;
    return absdiffs >= in.tune.spec_min_absdiffs;
}

// the sweep at B the search of the next finer level is forked behind (Tuning::spec_fork_first): its lambda multiplier
inline int fork_mult(const Tuning &t) { return t.spec_fork_first && t.spec_late ? 1 : 2; }

struct Step {
    // Search: on the main stream.  ForkSearch: record the fork on the main stream, the side stream waits for it, runs `search`
    // (speculative) and records the join.  JoinFixup: the main stream waits for the join, then runs `search` (fix-up).
    enum Kind { Search, Sweep, ForkSearch, JoinFixup, Expand } kind = Search;
    int level = 0;
    SearchLaunch search;
    SweepLaunch sweep;
    int expand_grid = 0;                          // k_expand: workgroups of 256 lanes
};

struct PyramidPlan {
    std::vector<Step> steps;
    uint32_t spec_levels = 0;                     // bit l: level l's search is speculative (bbme_fixup_counts)
};

// The level loop of MF::calcMotionBlockMatching (:115-206).  With `speculate`, the search of level l-1 is started on a
// second stream as soon as level l has finished the first sweep at its own block size (Tuning::spec_fork_first), and runs
// beside the level's remaining sweeps (which are latency-bound and leave most of the chip idle); when the level is final, a fix-up launch
// searches again the blocks whose prediction those sweeps changed (search_prediction, bbme_kernels.hpp).
// The sweep in front of the fork publishes 0 in the level's word and every later sweep of the level its number, 1, 2, ...
// (RegArgs::publish): the speculative search's blocks choose their prediction source by it (newest_coarse_grid).  The 0 is
// stored before the fork in every replay, so no search sees the count of the step before.
inline PyramidPlan plan_pyramid(const PlanInputs &in, bool speculate)
{
    PyramidPlan plan;
    const int nl = (int)in.lv.size();
    bool speculated = false;
    for (int l = nl - 1; l >= 0; --l) {
        Step s;
        s.level = l;
        s.kind = speculated ? Step::JoinFixup : Step::Search;
        s.search = plan_search_launch(in, l, speculated ? kPredictFixup : kPredictPlain);
        plan.steps.push_back(s);
        speculated = false;
        const PlanLevel &L = in.lv[l];
        const bool fork_here = speculate && l > 0 && L.block > 2 && worth_speculating(in, l - 1);
        const bool publish = fork_here && in.tune.spec_late != 0;
        int behind_fork = 0;                                       // sweeps of the level enqueued behind the fork
        GridId grid = kSmall0;                                     // the search's output
        int grid_block = L.block;
        for (int b = L.block; b > 1; b >>= 1) {                    // while (block_size > 1) :141
            for (int mult = 1; mult <= 2; ++mult) {                // lambda_multiplier = l + 1 :145
                const bool at_fork = fork_here && b == L.block && mult == fork_mult(in.tune);
                Step w;
                w.kind = Step::Sweep; w.level = l;
                w.sweep = plan_sweep(in, l, b, mult, grid, grid_block);
                if (publish && (speculated || at_fork)) w.sweep.publish = behind_fork;
                plan.steps.push_back(w);
                grid = w.sweep.to; grid_block = b;
                if (speculated) ++behind_fork;
                if (at_fork) {
                    Step f;
                    f.kind = Step::ForkSearch; f.level = l - 1;
                    f.search = plan_search_launch(in, l - 1, kPredictSpeculative);
                    plan.steps.push_back(f);
                    speculated = true;
                    behind_fork = 1;
                    plan.spec_levels |= 1u << (l - 1);
                }
            }
        }
    }
    Step e;
    e.kind = Step::Expand;
    e.expand_grid = (int)(((long long)(in.lv[0].width / 2) * (in.lv[0].height / 2) * 2 + 255) / 256);
    plan.steps.push_back(e);
    return plan;
}

}  // namespace bbme
