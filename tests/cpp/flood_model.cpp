// flood_model.cpp -- a CPU model of k_reg_solve's schedule at the level of waves, to price flood speculation and queue sharing.
//
//   flood_model W H LEVELS BLOCK SEARCH frame1.raw frame2.raw [DEPTH]      (8-bit planes, W x H, as the oracle takes them)
//
// The pyramid runs on the oracle (search, raster sweeps, block halving: oracle/bbme_oracle.h).  In front of every raster sweep
// the model solves the same sweep from the same field four times -- plain, flood speculation, shared queues, both -- and prints
// the rounds of the busiest wave in each; then the oracle's raster sweep runs and every modelled field is compared with its field.
//
// The model (DESIGN.md K2 "r02: what the chains are", second model; the rules are the kernel's, bbme_kernels.hpp):
//   * pass 1 evaluates every block with new := old and flags the dependants R, DR, D, DL of the blocks that change;
//   * the flagged blocks are dealt to the waves as the scan deals them (XCD bands, segments of 4 or 16 flags round-robin over a
//     band's waves, four waves per workgroup) and claimed: one ownership counter per block, as "work-list state" has it;
//   * rounds are synchronous: every wave with a queue pops 4 entries, all evaluations of a round read the estimates as the round
//     found them, then all stores, then every wave's releases and claims.  The claimer keeps its dependants;
//   * sharing: a wave with more than a round's worth hands its newest surplus to the idle waves of its workgroup, split evenly;
//   * flood speculation of depth D: a block that took the value of its updated input L, UL, U or UR while its wave's queue is
//     short claims D more blocks along that direction and queues them, marked, at the front behind the dependant that leads them;
//     a marked entry popped into the slot behind its predecessor is evaluated with the predecessor's estimate replaced by the
//     value the run's first block read from the flood's direction, and counts if the predecessor's evaluation counted and gave
//     that value; the predecessor then does not claim it.  Entries that do not count return to the front of the queue.
// The oracle's evaluator has no entry point of its own (one block, a given set of candidates), so score() restates it
// (find_min_candidate: SAD + lambda * multiplier * smoothness, FLT_MAX outside the image, first strict minimum); the comparison
// of every modelled field with the raster sweep's is what pins it.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "bbme_oracle.h"

namespace {

struct Mv {
    float u, v;
    bool operator==(const Mv &o) const { return u == o.u && v == o.v; }
    bool operator!=(const Mv &o) const { return !(*this == o); }
};

// candidate order of motion_framework.cpp:441-449 (C, L, R, DR, UL, UR, U, D, DL) and the inputs a raster sweep has updated
const int kOff[9][2] = {{0, 0}, {0, -1}, {0, 1}, {1, 1}, {-1, -1}, {-1, 1}, {-1, 0}, {1, 0}, {1, -1}};
const bool kNew[9] = {false, true, false, false, true, true, true, false, false};
const int kDep[4][2] = {{0, 1}, {1, 1}, {1, 0}, {1, -1}};      // dependants R, DR, D, DL ...
const int kDepCand[4] = {1, 4, 6, 5};                          // ... read the block as their candidate L, UL, U, UR

struct Sweep {
    const orc_mf *mf;
    const orc_level *lv;
    int bs, rows, cols;
    std::vector<Mv> old;

    Mv score(int r, int c, const Mv (&cand)[9], const bool (&present)[9]) const
    {
        const int px = c * bs, py = r * bs, W = lv->width, H = lv->height;
        float best = 0;
        int best_k = -1;
        for (int k = 0; k < 9; ++k) {
            if (!present[k]) continue;
            const float p2x = (float)px + cand[k].u, p2y = (float)py + cand[k].v;
            float e = FLT_MAX;
            if (!((int)p2x < 0 || (int)p2x > W - bs || (int)p2y < 0 || (int)p2y > H - bs)) {
                int sad = 0;
                for (int y = 0; y < bs; ++y) {
                    const uint8_t *a = lv->image1 + (size_t)(py + y) * W + px, *b = lv->image2 + (size_t)((int)p2y + y) * W + (int)p2x;
                    for (int x = 0; x < bs; ++x) sad += abs((int)a[x] - (int)b[x]);
                }
                float smooth = 0;
                for (int m = 0; m < 9; ++m)
                    if (present[m]) smooth += fabsf(cand[m].u - cand[k].u) + fabsf(cand[m].v - cand[k].v);
                float t = lv->lambda * (float)mf->lambda_multiplier;
                t = t * smooth;
                e = (float)sad + t;
            }
            if (best_k < 0 || e < best) { best = e; best_k = k; }
        }
        return cand[best_k];
    }
    // block x against `est`; subst >= 0: candidate `subst` is given the value `with` instead
    Mv eval(const std::vector<Mv> &est, int x, int subst = -1, Mv with = Mv{0, 0}, Mv *seen = nullptr) const
    {
        const int r = x / cols, c = x % cols;
        Mv cand[9];
        bool present[9];
        for (int k = 0; k < 9; ++k) {
            const int rr = r + kOff[k][0], cc = c + kOff[k][1];
            present[k] = rr >= 0 && rr < rows && cc >= 0 && cc < cols;
            cand[k] = present[k] ? (kNew[k] ? est : old)[(size_t)rr * cols + cc] : Mv{0, 0};
            if (k == subst) cand[k] = with;
            if (seen) seen[k] = cand[k];
        }
        if (seen) for (int k = 0; k < 9; ++k) if (!present[k]) seen[k] = Mv{NAN, NAN};     // never equal to a result
        return score(r, c, cand, present);
    }
};

struct Result { int rounds = 0, evaluated = 0, speculated = 0, kept = 0; std::vector<Mv> field; };

const uint32_t kMark = 0x80000000u;

Result solve(const Sweep &s, bool share, int depth)
{
    const int n = s.rows * s.cols, cols = s.cols;
    Result out;
    std::vector<Mv> est(n);
    std::vector<uint8_t> flag(n, 0);
    for (int x = 0; x < n; ++x) est[x] = s.eval(s.old, x);      // pass 1: new := old, every candidate comes from `old`
    for (int x = 0; x < n; ++x)
        if (est[x] != s.old[x])
            for (int d = 0; d < 4; ++d) {
                const int rr = x / cols + kDep[d][0], cc = x % cols + kDep[d][1];
                if (rr < s.rows && cc >= 0 && cc < cols) flag[(size_t)rr * cols + cc] = 1;
            }
    // the launch: plan_sweep's grid, four waves per workgroup, the scan's deal
    const int wpw = 4, seg = n <= 140000 ? 4 : 16;
    const int nwg = (std::min(256, (n + 63) / 64) + 7) / 8 * 8, W = nwg * wpw, Wx = (nwg / 8) * wpw;
    const int nseg = (n + seg - 1) / seg, band = (nseg + 7) / 8;
    std::vector<std::deque<uint32_t>> q(W);
    std::vector<uint32_t> own(n, 0);
    std::vector<int> rounds(W, 0);
    for (int sg = 0; sg < nseg; ++sg) {
        const int xcd = sg / band, wx = (sg - xcd * band) % Wx;
        const int wg = (wx / wpw) * 8 + xcd, wave = wg * wpw + wx % wpw;
        for (int x = sg * seg; x < std::min(n, (sg + 1) * seg); ++x)
            if (flag[x] && own[x]++ == 0) q[wave].push_back((uint32_t)x);
    }
    struct Slot { uint32_t e; int x, kd; Mv hyp, res, seen[9]; bool valid, changed; };
    for (;;) {
        bool any = false;
        for (int w = 0; w < W; ++w) any |= !q[w].empty();
        if (!any) break;
        if (share)
            for (int w = 0; w < W; ++w) {
                if (q[w].size() <= 4) continue;
                std::vector<int> idle;
                for (int j = w / wpw * wpw; j < w / wpw * wpw + wpw; ++j) if (q[j].empty()) idle.push_back(j);
                size_t surplus = q[w].size() - 4;
                for (size_t i = 0; i < idle.size() && surplus; ++i) {
                    const size_t left = idle.size() - 1 - i;
                    const size_t part = std::min<size_t>(64, (surplus + left + 1) / (left + 2));
                    q[idle[i]].insert(q[idle[i]].end(), q[w].end() - part, q[w].end());      // the newest go, in order
                    q[w].erase(q[w].end() - part, q[w].end());
                    surplus -= part;
                }
            }
        // every wave's evaluations, against the estimates as the round found them
        std::vector<std::vector<Slot>> slots(W);
        for (int w = 0; w < W; ++w) {
            if (q[w].empty()) continue;
            ++rounds[w];
            std::vector<Slot> &sl = slots[w];
            for (int g = 0; g < 4 && !q[w].empty(); ++g) {
                Slot t{};
                t.e = q[w].front(); q[w].pop_front();
                t.x = (int)(t.e & ~kMark);
                t.kd = 0;
                if (g >= 1 && (t.e & kMark) && depth > 0 && cols >= 4) {
                    const int dist = t.x - sl[g - 1].x, c = t.x % cols;
                    t.kd = (dist == 1 && c >= 1) ? 1 : (dist == cols + 1 && c >= 1) ? 4 : dist == cols ? 6 : (dist == cols - 1 && c + 1 < cols) ? 5 : 0;
                }
                sl.push_back(t);
            }
            for (size_t g = 0; g < sl.size(); ++g) {
                Slot &t = sl[g];
                if (t.kd) {
                    // the run's expectation: what its first, unlinked block read from the direction of ITS successor
                    t.hyp = sl[g - 1].kd ? sl[g - 1].hyp : sl[g - 1].seen[t.kd];
                    t.res = s.eval(est, t.x, t.kd, t.hyp, t.seen);
                    t.valid = sl[g - 1].valid && sl[g - 1].res == t.hyp;
                    ++out.speculated;
                    out.kept += t.valid;
                } else {
                    t.res = s.eval(est, t.x, -1, Mv{0, 0}, t.seen);
                    t.valid = true;
                }
                ++out.evaluated;
            }
        }
        for (int w = 0; w < W; ++w)
            for (Slot &t : slots[w]) {
                t.changed = t.valid && t.res != est[t.x];
                if (t.changed) est[t.x] = t.res;
            }
        // releases and claims
        for (int w = 0; w < W; ++w) {
            std::vector<Slot> &sl = slots[w];
            std::vector<uint32_t> front, back;
            const size_t left = q[w].size();
            for (size_t g = 0; g < sl.size(); ++g) {
                Slot &t = sl[g];
                if (!t.valid) { front.push_back(t.e); continue; }
                const uint32_t wasx = own[t.x];
                own[t.x] = 0;
                if (t.changed) {
                    const int nk = g + 1 < sl.size() ? sl[g + 1].kd : 0;
                    int fd = -1;
                    for (int d = 0; d < 4 && fd < 0; ++d) if (t.seen[kDepCand[d]] == t.res) fd = d;
                    const bool grow = depth > 0 && cols >= 4 && nk == 0 && fd >= 0 && left < 4;
                    const int r = t.x / cols, c = t.x % cols;
                    for (int d = 0; d < 4; ++d) {
                        if (nk != 0 && kDepCand[d] == nk) continue;          // evaluated behind this block in this round
                        const int rr = r + kDep[d][0], cc = c + kDep[d][1];
                        if (rr >= s.rows || cc < 0 || cc >= cols) continue;
                        const int tx = rr * cols + cc;
                        if (own[tx]++ == 0) (grow && d == fd ? front : back).push_back((uint32_t)tx);
                    }
                    if (grow) {
                        // (the kernel's lanes queue in lane order: the leading dependant, lane fd, then the blocks ahead)
                        for (int j = 2; j < 2 + depth; ++j) {
                            const int rr = r + j * kDep[fd][0], cc = c + j * kDep[fd][1];
                            if (rr >= s.rows || cc < 0 || cc >= cols) continue;
                            const int tx = rr * cols + cc;
                            if (own[tx]++ == 0) front.push_back((uint32_t)tx | kMark);
                        }
                    }
                }
                if (wasx >= 2 && own[t.x]++ == 0) back.push_back((uint32_t)t.x);
            }
            q[w].insert(q[w].begin(), front.begin(), front.end());
            q[w].insert(q[w].end(), back.begin(), back.end());
        }
    }
    for (int w = 0; w < W; ++w) out.rounds = std::max(out.rounds, rounds[w]);
    out.field = est;
    return out;
}

std::vector<uint8_t> read_plane(const char *path, size_t bytes)
{
    std::vector<uint8_t> v(bytes);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %zu bytes of %s\n", bytes, path); exit(2); }
    fclose(f);
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 8) { fprintf(stderr, "usage: flood_model W H LEVELS BLOCK SEARCH frame1.raw frame2.raw [DEPTH]\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), levels = atoi(argv[3]), block = atoi(argv[4]), search = atoi(argv[5]);
    const int depth = argc > 8 ? atoi(argv[8]) : 2;
    const std::vector<uint8_t> f1 = read_plane(argv[6], (size_t)w * h), f2 = read_plane(argv[7], (size_t)w * h);
    std::vector<int> searches(levels, search), blocks(levels, block);
    orc_mf *mf = nullptr;
    if (orc_mf_create(f1.data(), f2.data(), w, h, w, searches.data(), blocks.data(), levels, 0, &mf) != 0) { fprintf(stderr, "orc_mf_create failed\n"); return 2; }
    int bad = 0;
    // orc_level_schedule, with the model in front of every sweep
    for (int level = levels - 1; level >= 0; --level) {
        orc_level *lv = &mf->lv[level];
        if (level != levels - 1) orc_copy_mvs(mf, level);
        orc_calc_level_bm(mf, level);
        const int init_block = lv->block_size;
        while (lv->block_size > 1) {
            for (int l = 0; l < 2; ++l) {
                mf->lambda_multiplier = l + 1;
                Sweep s;
                s.mf = mf; s.lv = lv; s.bs = lv->block_size; s.rows = lv->height / s.bs; s.cols = lv->width / s.bs;
                s.old.resize((size_t)s.rows * s.cols);
                auto cell = [&](int r, int c) { return lv->flow + 2 * ((size_t)r * s.bs * lv->width + (size_t)c * s.bs); };
                for (int r = 0; r < s.rows; ++r)
                    for (int c = 0; c < s.cols; ++c) s.old[(size_t)r * s.cols + c] = Mv{cell(r, c)[0], cell(r, c)[1]};
                const Result plain = solve(s, false, 0), flood = solve(s, false, depth), shared = solve(s, true, 0), both = solve(s, true, depth);
                orc_regularize_mvs(mf, level);
                bool same = true;
                for (const Result *res : {&plain, &flood, &shared, &both})
                    for (int r = 0; r < s.rows; ++r)
                        for (int c = 0; c < s.cols; ++c)
                            same &= res->field[(size_t)r * s.cols + c] == Mv{cell(r, c)[0], cell(r, c)[1]};
                bad += !same;
                printf("sweep level=%d b=%d mult=%d blocks=%d rounds plain=%d flood=%d share=%d both=%d evaluated plain=%d both=%d speculated=%d kept=%d field=%s\n",
                       level, s.bs, l + 1, s.rows * s.cols, plain.rounds, flood.rounds, shared.rounds, both.rounds, plain.evaluated, both.evaluated,
                       both.speculated, both.kept, same ? "same" : "DIFFERENT");
                fflush(stdout);
            }
            orc_divide_blocks(mf, level);
            lv->block_size >>= 1;
            lv->lambda = lv->lambda * 2;
        }
        lv->block_size = init_block;
    }
    orc_mf_destroy(mf);
    printf(bad ? "flood model: %d sweeps DIFFERENT\n" : "flood model ok\n", bad);
    return bad ? 1 : 0;
}
