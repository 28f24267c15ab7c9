// The launch plan of an estimate (csrc/launch_plan.hpp), without a GPU.  Links bbme_host.cpp for plan_padding, build_spiral and
// plan_search, so the levels it plans on have the sizes, windows and two-wave verdicts a context would have.
//
//   launch_plan_test                                         the invariants below, over block sizes, depths, modes and knobs
//   launch_plan_test dump W H SEARCH,.. BLOCK,.. [pairs=N] [chain=1] [jacobi=1] [raster=1] [relax=0] [speculate=0]
//                                                            one line per kernel launch of that context's estimate; knobs from
//                                                            the environment, as a context reads them
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "bbme_internal.hpp"
#include "launch_plan.hpp"
#include "spec_grids.hpp"

using namespace bbme;

static int failures = 0;
static std::string context;                                      // what is being checked, for the messages
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 40) { printf("FAIL %s:%d [%s]: ", __FILE__, __LINE__, context.c_str()); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// The levels of a context, as create_context describes them.  False: the context would be refused.
static bool describe_levels(int width, int height, const std::vector<int> &search, const std::vector<int> &block, bool loose,
                            std::vector<PlanLevel> &lv)
{
    bbme_params p{};
    p.num_levels = (int)block.size();
    for (int l = 0; l < p.num_levels; ++l) { p.block_size[l] = block[l]; p.search_size[l] = search[l]; }
    Geometry g;
    if (validate_params(p) || plan_padding(width, height, p, g)) return false;
    lv.assign(block.size(), PlanLevel{});
    static std::map<std::tuple<int, int, bool>, PlanLevel> cache;         // (search, block, loose) -> what the search plans give
    for (int l = 0; l < p.num_levels; ++l) {
        PlanLevel &L = lv[l];
        auto hit = cache.find({search[l], block[l], loose});
        if (hit == cache.end()) {
            PlanLevel c;
            c.block = block[l];
            c.range = build_spiral(search[l], block[l]).range;
            c.lds_bytes = generic_lds_bytes(c.block, c.range);
            c.fast = fast_kernel_serves(c.block, c.range);
            if (c.fast) {
                const SearchPlan one = plan_search(c.range, c.block, c.block == 32 ? 8 : 16, 64, loose);
                const SearchPlan two = plan_search(c.range, c.block, 8, 128, loose);
                c.fast_pitch_dw = one.pitch_dw;
                c.fast_lds_bytes = fast_lds_bytes(c.block, c.range, one.pitch_dw);
                c.split_pays = split_shortens_walk(one.rounds, two.rounds, c.block);
            }
            hit = cache.emplace(std::make_tuple(search[l], block[l], loose), c).first;
        }
        L = hit->second;
        L.width = g.padded_width >> l; L.height = g.padded_height >> l;
        if (L.width / L.block < 2 || L.height / L.block < 2 || L.width % 4 != 0) return false;
        if (!L.fast && L.lds_bytes > 160 * 1024) return false;
    }
    return true;
}

static PlanInputs make_inputs(const std::vector<PlanLevel> &lv, int pairs, bool jacobi, bool raster, bool relax, const Tuning &t)
{
    PlanInputs in;
    in.lv = lv; in.pairs = pairs; in.jacobi = jacobi; in.raster_search = raster; in.relax = relax; in.tune = t;
    in.memo_blocks = memo_room(t, lv);                              // as creation allocates it
    return in;
}

// ---- the plan in words: one line per kernel launch, as a kernel trace names it ---------------------------------------------------
static void print_launch(const char *kernel, int gx, int gy, int wg, size_t lds, bool side)
{
    printf("%s grid=%dx%d wg=%d lds=%zu stream=%s\n", kernel, gx, gy, wg, lds, side ? "side" : "main");
}

static void print_search(const PlanInputs &in, const SearchLaunch &s)
{
    const int B = in.lv[s.level].block, P = in.pairs;
    char name[96];
    if (s.kernel == SearchKernel::Generic) {
        snprintf(name, sizeof name, "k_search_generic<%d>", B);
    } else if (s.kernel == SearchKernel::Fast) {
        snprintf(name, sizeof name, "k_search_fast<%d, %d>", B, s.waves);
    } else {
        print_launch("k_fixup_list", s.list_grid, P, 256, 0, s.side_stream);
        snprintf(name, sizeof name, "k_search_list<%d, %d>", B, s.waves);
    }
    print_launch(name, s.grid, P, 64 * s.waves, s.lds, s.side_stream);
}

static void print_sweep(const PlanInputs &in, const SweepLaunch &s)
{
    const int P = in.pairs;
    char name[96];
    switch (s.pass1) {
    case Pass1::Plain: snprintf(name, sizeof name, "k_reg_pass1<%d>", s.block); break;
    case Pass1::Strip: snprintf(name, sizeof name, "k_reg_pass1_strip<%d>", s.block); break;
    case Pass1::Chain: snprintf(name, sizeof name, "k_reg_pass1_lanes<%d, false>", s.block); break;
    case Pass1::ChainMemo: snprintf(name, sizeof name, "k_reg_pass1_lanes<%d, true>", s.block); break;
    }
    print_launch(name, s.pass1_grid, P, 256, 0, false);
    snprintf(name, sizeof name, "k_reg_iter<%d>", s.block);
    for (int i = 0; i < s.relax_steps; ++i) print_launch(name, s.relax_tiles, P, 256, 0, false);
    if (!s.solve) return;
    snprintf(name, sizeof name, "k_reg_solve<%d, %d, %s>", s.block, s.solve_segment, s.memo ? "true" : "false");
    print_launch(name, s.solve_grid, P, 64 * s.solve_waves, 0, false);
}

// Every launch in enqueue order; the lines that start with '#' say what a trace cannot show
static void print_plan(const PlanInputs &in, const PyramidPlan &plan)
{
    for (const Step &s : plan.steps) {
        if (s.kind == Step::Expand) {
            print_launch("k_expand", s.expand_grid, in.pairs, 256, 0, false);
        } else if (s.kind == Step::Sweep) {
            const SweepLaunch &w = s.sweep;
            printf("# level %d sweep b=%d mult=%d lambda=%g old_shift=%d round_cap=%u lazy=%d publish=%d\n", w.level, w.block, w.mult,
                   (double)w.lambda_mult, w.old_shift, w.round_cap, w.lazy ? 1 : 0, w.publish);
            print_sweep(in, w);
        } else {
            printf("# level %d %s late=%d late_force=%d\n", s.level,
                   s.kind == Step::Search ? "search" : (s.kind == Step::ForkSearch ? "fork, speculative search" : "join, fix-up search"),
                   s.search.late ? 1 : 0, s.search.late_force ? 1 : 0);
            print_search(in, s.search);
        }
    }
    printf("# speculated levels mask %u\n", plan.spec_levels);
}

static std::vector<int> csv(const char *s)
{
    std::vector<int> v;
    for (const char *p = s; *p;) { v.push_back(atoi(p)); p = strchr(p, ','); if (!p) break; ++p; }
    return v;
}

static int dump(int argc, char **argv)
{
    if (argc < 6) { fprintf(stderr, "dump W H SEARCH,.. BLOCK,.. [pairs=N] [chain=1] [jacobi=1] [raster=1] [relax=0] [speculate=0]\n"); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    const std::vector<int> search = csv(argv[4]), block = csv(argv[5]);
    std::map<std::string, int> opt = {{"pairs", 1}, {"chain", 0}, {"jacobi", 0}, {"raster", 0}, {"relax", 1}, {"speculate", 1}};
    for (int i = 6; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq || !opt.count(std::string(argv[i], (size_t)(eq - argv[i])))) { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        opt[std::string(argv[i], (size_t)(eq - argv[i]))] = atoi(eq + 1);
    }
    if (search.size() != block.size() || block.empty()) { fprintf(stderr, "one search size per block size\n"); return 2; }
    const Tuning t = read_tuning(opt["pairs"]);
    std::vector<PlanLevel> lv;
    if (!describe_levels(w, h, search, block, t.loose_plan, lv)) { fprintf(stderr, "a context of this geometry is refused\n"); return 2; }
    const PlanInputs in = make_inputs(lv, opt["pairs"], opt["jacobi"] != 0, opt["raster"] != 0, opt["relax"] != 0, t);
    printf("# %dx%d search %s block %s pairs %d%s%s%s%s\n", w, h, argv[4], argv[5], in.pairs, opt["chain"] ? " chain" : "",
           in.jacobi ? " jacobi" : "", in.raster_search ? " raster" : "", in.relax ? "" : " no-relax");
    print_plan(in, plan_pyramid(in, t.speculate && opt["speculate"] != 0));       // (a chain context launches what a batch of its pairs does)
    return 0;
}

// ---- the invariants -----------------------------------------------------------------------------------------------------------
static void check_search(const PlanInputs &in, const SearchLaunch &s, Step::Kind kind)
{
    const Tuning &t = in.tune;
    const PlanLevel &L = in.lv[s.level];
    const int nl = (int)in.lv.size();
    const int coarser = s.level + 1 < nl ? in.lv[s.level + 1].block : 0;
    CHECK(s.mode == (kind == Step::Search ? kPredictPlain : kind == Step::ForkSearch ? kPredictSpeculative : kPredictFixup), "mode %d", s.mode);
    CHECK(s.side_stream == (kind == Step::ForkSearch), "stream");
    const bool fast = L.fast && !t.force_generic_search && !in.raster_search;
    CHECK((s.kernel != SearchKernel::Generic) == fast, "level %d: kernel", s.level);
    CHECK((s.kernel == SearchKernel::List) == (fast && kind == Step::JoinFixup), "level %d: the list form serves the strip kernel's fix-ups", s.level);
    CHECK(s.waves == 1 || (s.waves == 2 && s.kernel != SearchKernel::Generic && kind != Step::ForkSearch), "level %d: %d waves", s.level, s.waves);
    if (s.waves == 2) CHECK(L.blocks_at(L.block) <= t.split_blocks && (L.split_pays || t.split_forced), "level %d: two waves", s.level);
    CHECK(s.grid > 0 && (s.kernel != SearchKernel::List || s.list_grid > 0), "level %d: empty grid", s.level);
    if (s.kernel == SearchKernel::Fast) CHECK(s.grid >= L.blocks_at(L.block) && s.grid < L.blocks_at(L.block) + 8, "level %d: grid %d", s.level, s.grid);
    if (s.kernel == SearchKernel::Generic) CHECK(s.grid == L.blocks_at(L.block), "level %d: grid %d", s.level, s.grid);
    // the limit creation raises: for k_search_generic and the one-wave k_search_fast what a speculative launch of the level asks
    // for; every other kernel keeps the 48 KB a kernel may use without the attribute
    size_t limit = 48 * 1024;
    if (s.kernel == SearchKernel::Generic || (s.kernel == SearchKernel::Fast && s.waves == 1))
        limit = std::max(limit, search_lds_bytes(t, L, s.kernel == SearchKernel::Fast, s.level, coarser));
    CHECK(s.lds <= limit && s.lds <= 160 * 1024, "level %d: %zu bytes of LDS, limit %zu", s.level, s.lds, limit);
    CHECK(s.lds >= (s.kernel == SearchKernel::Generic ? L.lds_bytes : L.fast_lds_bytes), "level %d: LDS below the window", s.level);
    if (kind == Step::ForkSearch) CHECK(s.lds >= t.spec_lds_for(coarser, s.level), "level %d: LDS below the speculative floor", s.level);
    CHECK(s.late == (kind == Step::ForkSearch && s.kernel == SearchKernel::Fast && t.spec_late != 0), "level %d: late table", s.level);
    CHECK(s.late_force == (s.late && t.spec_late == 2), "level %d: late_force", s.level);
}

static void check_sweep(const PlanInputs &in, const SweepLaunch &s, size_t room)
{
    const Tuning &t = in.tune;
    const PlanLevel &L = in.lv[s.level];
    const int cols = L.width / s.block;
    const long long blocks = L.blocks_at(s.block);
    CHECK(s.pass1_grid > 0 && s.solve_grid > 0 && s.relax_tiles > 0, "sweep %d/%d: empty grid", s.level, s.block);
    CHECK(s.solve_grid % 8 == 0 && s.solve_grid <= 8192 + 7, "sweep %d/%d: solver grid %d", s.level, s.block, s.solve_grid);
    CHECK(s.solve_waves == 1 || s.solve_waves == 2 || s.solve_waves == 4, "solver waves");
    CHECK(s.solve_segment == (blocks <= t.scan_fine_max ? 4 : 16), "sweep %d/%d: segment", s.level, s.block);
    CHECK((s.pass1 == Pass1::ChainMemo) == s.memo, "sweep %d/%d: a memo without the chain form that fills it", s.level, s.block);
    if (s.memo) {
        CHECK((size_t)blocks <= room, "sweep %d/%d: %lld blocks, memo room %zu", s.level, s.block, blocks, room);
        CHECK(!in.jacobi && t.use_memo && s.block >= 8 && s.block >= t.memo_min_block && L.width <= 8192 && L.height <= 8192 &&
              blocks <= t.pass1_lanes_max, "sweep %d/%d: memo", s.level, s.block);
    }
    if (s.pass1 == Pass1::Chain) CHECK(s.block <= 16 && blocks <= t.pass1_lanes_max, "sweep %d/%d: chain form", s.level, s.block);
    if (s.pass1 == Pass1::Strip) CHECK(cols % 4 == 0 && cols >= 12 && s.block <= 4, "sweep %d/%d: strip form on %d columns", s.level, s.block, cols);
    if (s.lazy) CHECK(s.relax_steps > 0 && s.pass1 == Pass1::Strip && s.solve, "sweep %d/%d: lazy without a relaxation launch", s.level, s.block);
    CHECK(s.solve == !in.jacobi && (s.solve || s.relax_steps == 0), "sweep %d/%d: Jacobi", s.level, s.block);
    CHECK(s.lambda_mult == (float)(L.block / 2) * (float)(L.block / s.block) * (float)s.mult, "sweep %d/%d: lambda", s.level, s.block);
    CHECK(s.round_cap > 0, "round cap");
}

static void check_plan(const PlanInputs &in, bool speculate)
{
    const Tuning &t = in.tune;
    const PyramidPlan plan = plan_pyramid(in, speculate);
    const int nl = (int)in.lv.size();
    const size_t room = memo_room(t, in.lv);
    size_t i = 0;
    uint32_t mask = 0;
    bool forked = false;                                           // the level's search has been started behind the coarser level's fork
    const uint32_t dummy[4] = {0, 0, 0, 0};                        // stand-ins for small[0], small[1], big[0], big[1]
    for (int l = nl - 1; l >= 0; --l) {
        const PlanLevel &L = in.lv[l];
        CHECK(i < plan.steps.size() && plan.steps[i].kind == (forked ? Step::JoinFixup : Step::Search) && plan.steps[i].level == l,
              "level %d: search step", l);
        if (i >= plan.steps.size()) return;
        check_search(in, plan.steps[i].search, plan.steps[i].kind);
        ++i;
        // does the next finer level's search fork here, by the rule's own words
        bool expect_fork = false;
        if (speculate && !in.jacobi && l > 0 && L.block > 2) {
            const PlanLevel &F = in.lv[l - 1];
            const double side = 2.0 * F.range + 1.0;
            expect_fork = (double)(F.width / F.block) * (F.height / F.block) * side * side * F.block * F.block >= t.spec_min_absdiffs;
        }
        const int fm = t.spec_fork_first && t.spec_late ? 1 : 2;
        CoarseGrid table[kMaxCoarseGrids];
        const int table_n = fill_coarse_grids(table, L.width, L.block, fm == 1, &dummy[kSmall0], &dummy[kSmall1], 0, &dummy[kBig0], &dummy[kBig1], 0);
        forked = false;
        GridId grid = kSmall0;
        int grid_block = L.block, published = 0;
        for (int b = L.block; b >= 2; b >>= 1)
            for (int mult = 1; mult <= 2; ++mult) {
                CHECK(i < plan.steps.size() && plan.steps[i].kind == Step::Sweep, "level %d b %d mult %d: sweep step", l, b, mult);
                if (i >= plan.steps.size() || plan.steps[i].kind != Step::Sweep) return;
                const SweepLaunch &s = plan.steps[i].sweep;
                ++i;
                CHECK(s.level == l && s.block == b && s.mult == mult, "level %d: sweep %d x %d where %d x %d is due", l, s.block, s.mult, b, mult);
                CHECK(s.from == grid && s.to != grid && s.old_shift == (grid_block == 2 * b ? 1 : 0) && grid_block == b << s.old_shift,
                      "level %d b %d mult %d: grids", l, b, mult);
                CHECK((s.to == kSmall0 || s.to == kSmall1) == (b == L.block), "level %d b %d: pool", l, b);
                grid = s.to; grid_block = b;
                check_sweep(in, s, room);
                const bool at_fork = expect_fork && b == L.block && mult == fm;
                const bool publishes = (forked || at_fork) && t.spec_late != 0;
                CHECK((s.publish >= 0) == publishes, "level %d b %d mult %d: publish %d", l, b, mult, s.publish);
                if (s.publish >= 0) {
                    // what enqueue_pyramid checks while it captures: the sweep that publishes n leaves entry n of the table
                    CHECK(s.publish == published && s.publish < table_n, "level %d b %d mult %d: publishes %d, entry %d of %d is due", l, b, mult, s.publish, published, table_n);
                    if (s.publish < table_n)
                        CHECK(table[s.publish].grid == &dummy[s.to] && 1 << table[s.publish].cell_shift == b && table[s.publish].cols == L.width / b,
                              "level %d b %d mult %d: not entry %d of the coarse grid table", l, b, mult, s.publish);
                    ++published;
                }
                const bool fork_step = i < plan.steps.size() && plan.steps[i].kind == Step::ForkSearch;
                CHECK(fork_step == at_fork, "level %d b %d mult %d: fork", l, b, mult);
                if (fork_step) {
                    CHECK(plan.steps[i].level == l - 1, "fork of level %d behind level %d", plan.steps[i].level, l);
                    check_search(in, plan.steps[i].search, Step::ForkSearch);
                    mask |= 1u << (l - 1);
                    forked = true;
                    ++i;
                }
            }
        CHECK(forked == expect_fork, "level %d: fork expected %d", l, (int)expect_fork);
        if (forked && t.spec_late != 0) CHECK(published == table_n, "level %d: %d sweeps published, the table has %d entries", l, published, table_n);
    }
    CHECK(i + 1 == plan.steps.size() && plan.steps[i].kind == Step::Expand && plan.steps[i].expand_grid > 0, "the expansion ends the plan");
    CHECK(plan.spec_levels == mask && !(mask >> (nl - 1)), "speculated levels %u, forks seen %u", plan.spec_levels, mask);
}

// every knob at its default and at the values the GPU tests give it (tests/helpers.py, tests/test_gpu_*.py)
static const std::vector<std::vector<std::pair<const char *, const char *>>> kKnobSets = {
    {},
    {{"BBME_SPEC_MIN_GABS", "0"}},
    {{"BBME_LIST_SPLIT", "0"}, {"BBME_SPEC_MIN_GABS", "0"}},
    {{"BBME_PASS1_LAZY", "0"}, {"BBME_RELAX_STEPS", "1"}},
    {{"BBME_RELAX_STEPS", "1"}}, {{"BBME_RELAX_STEPS", "0"}},
    {{"BBME_XCD_REMAP", "0"}},
    {{"BBME_LOOSE_PLAN", "1"}},
    {{"BBME_RELAX_RULE", "0,64,2,2"}}, {{"BBME_RELAX_RULE", "1,64,2,1"}},
    {{"BBME_LOCAL_ROUNDS", "1"}, {"BBME_RELAX_STEPS", "1"}}, {{"BBME_LOCAL_ROUNDS", "32"}, {"BBME_RELAX_STEPS", "1"}},
    {{"BBME_NO_GRAPH", "1"}},
    {{"BBME_SEARCH_SPLIT_BLOCKS", "0"}}, {{"BBME_SEARCH_SPLIT_BLOCKS", "100000000"}}, {{"BBME_SEARCH_SPLIT_BLOCKS", "100000000"}, {"BBME_SPEC_MIN_GABS", "0"}},
    {{"BBME_GENERIC_SEARCH", "1"}}, {{"BBME_GENERIC_SEARCH", "1"}, {"BBME_SPEC_MIN_GABS", "0"}},
    {{"BBME_PASS1_STRIP", "1"}, {"BBME_PASS1_LANES_MAX", "0"}}, {{"BBME_PASS1_STRIP", "0"}, {"BBME_PASS1_LANES_MAX", "0"}},
    {{"BBME_PASS1_LANES_MAX", "0"}}, {{"BBME_PASS1_LANES_MAX", "100000000"}},
    {{"BBME_SCAN_FINE_MAX", "0"}}, {{"BBME_SCAN_FINE_MAX", "100000000"}},
    {{"BBME_SOLVE_WAVES", "1"}}, {{"BBME_SOLVE_WAVES", "2"}}, {{"BBME_SOLVE_WGS", "1"}, {"BBME_SOLVE_WAVES", "1"}}, {{"BBME_SOLVE_WGS", "8192"}},
    {{"BBME_SOLVE_SHARE", "0"}}, {{"BBME_WIDE_THRESHOLD", "4"}}, {{"BBME_TEST_ROUND_CAP", "3"}},
    {{"BBME_MEMO", "0"}}, {{"BBME_MEMO", "1"}, {"BBME_MEMO_MIN_B", "8"}, {"BBME_MEMO_FORWARD", "0"}},
    {{"BBME_MEMO", "1"}, {"BBME_MEMO_MIN_B", "8"}, {"BBME_MEMO_FORWARD", "1"}}, {{"BBME_MEMO_MIN_B", "32"}},
    {{"BBME_SPECULATE", "0"}}, {{"BBME_SPECULATE_BOTH_GRAPHS", "1"}},
    {{"BBME_SPEC_MIN_GABS", "0"}, {"BBME_SPEC_LATE", "0"}}, {{"BBME_SPEC_MIN_GABS", "0"}, {"BBME_SPEC_LATE", "2"}},
    {{"BBME_SPEC_MIN_GABS", "0"}, {"BBME_SPEC_LATE", "0"}, {"BBME_SPEC_FORK_FIRST", "1"}},
    {{"BBME_SPEC_MIN_GABS", "0"}, {"BBME_SPEC_LATE", "1"}, {"BBME_SPEC_FORK_FIRST", "0"}},
    {{"BBME_SPEC_MIN_GABS", "0"}, {"BBME_SPEC_LATE", "2"}, {"BBME_SPEC_FORK_FIRST", "0"}},
    {{"BBME_SPEC_WGS_PER_CU", "2"}, {"BBME_SPEC_MIN_GABS", "0"}}, {{"BBME_SPEC_WGS_PER_CU", "1"}, {"BBME_SPEC_MIN_GABS", "0"}},
    {{"BBME_SPEC_WGS_PER_CU", "24,1"}, {"BBME_SPEC_MIN_GABS", "0"}},
};

static int invariants()
{
    for (const auto &k : kKnobs) unsetenv(k.name);
    struct Shape { int w, h; };
    const Shape shapes[] = {{200, 136}, {584, 388}, {1920, 1080}, {3840, 2160}, {16384, 256}};       // the last: beyond the memo's 8192
    std::vector<std::vector<int>> blocks;
    for (int B = 2; B <= 64; B <<= 1)
        for (int nl = 1; nl <= 4; ++nl) blocks.push_back(std::vector<int>(nl, B));
    for (std::vector<int> mixed : {std::vector<int>{16, 16, 32}, {4, 8, 16}, {16, 16, 8}, {32, 8}, {8, 2, 16, 4}}) blocks.push_back(mixed);
    long long plans = 0, contexts = 0;
    for (const auto &set : kKnobSets) {
        std::string knobs;
        for (const auto &kv : set) { setenv(kv.first, kv.second, 1); knobs += std::string(" ") + kv.first + "=" + kv.second; }
        for (const Shape &sh : shapes)
            for (const std::vector<int> &block : blocks)
                for (int range : {7, 32, 64}) {
                    if (range == 64 && (sh.w > 600 || block[0] == 2)) continue;      // (the generic kernel's ranges: the small shapes do)
                    std::vector<int> search;
                    for (int b : block) search.push_back(b + 2 * range);
                    for (int pairs : {1, 6, 4}) {                                     // a single pair, a batch, a chain of 4 pairs
                        const Tuning t = read_tuning(pairs);
                        std::vector<PlanLevel> lv;
                        if (!describe_levels(sh.w, sh.h, search, block, t.loose_plan, lv)) continue;
                        ++contexts;
                        for (int mode = 0; mode < 8; ++mode) {
                            const bool jacobi = mode & 1, raster = mode & 2, relax = !(mode & 4);
                            const PlanInputs in = make_inputs(lv, pairs, jacobi, raster, relax, t);
                            for (int speculate = 0; speculate < 2; ++speculate) {
                                char what[256];
                                snprintf(what, sizeof what, "%dx%d B %d.. x%zu R %d pairs %d%s%s%s%s%s", sh.w, sh.h, block[0], block.size(), range,
                                         pairs, jacobi ? " jacobi" : "", raster ? " raster" : "", relax ? "" : " no-relax",
                                         speculate ? " speculating" : "", knobs.c_str());
                                context = what;
                                check_plan(in, speculate != 0 && t.speculate);
                                ++plans;
                            }
                        }
                    }
                }
        for (const auto &kv : set) unsetenv(kv.first);
    }
    CHECK(contexts > 1000, "only %lld contexts were planned", contexts);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("launch plan ok: %lld plans of %lld contexts\n", plans, contexts);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "dump")) return dump(argc, argv);
    return invariants();
}
