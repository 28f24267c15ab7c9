// guard_layout_test.cpp -- csrc/guard_layout.hpp without a GPU: the layout of a guarded allocation, the scan of a guard band's
// host copy and the parsing of the two knobs.  A program of its own, built under AddressSanitizer and UBSan by
// tests/test_guard_layout_cpu.py: the scan must not read one byte outside the band it is given.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "guard_layout.hpp"

using namespace bbme;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// A host image of one guarded allocation, every byte of it in a vector of exactly total() bytes (so that the sanitizer sees a
// scan that leaves it): guards as the library fills them, payload of another value.
static std::vector<uint8_t> image(const GuardLayout &g)
{
    std::vector<uint8_t> m(g.total(), 0x11);
    memset(m.data(), kGuardByte, g.front);
    memset(m.data() + g.back_offset(), kGuardByte, g.back);
    return m;
}

static void check_layout(size_t n)
{
    const GuardLayout g = guard_layout(n, true);
    CHECK(g.front == kGuardBytes && g.back == kGuardBytes && g.payload == n);
    CHECK(g.payload_offset() == 4096);
    CHECK(g.payload_offset() % 4096 == 0);                  // the payload keeps the base's alignment up to 4 KiB
    CHECK(g.back_offset() == 4096 + n);
    CHECK(g.total() == n + 8192);
    CHECK(g.payload_offset() + g.payload == g.back_offset() && g.back_offset() + g.back == g.total());   // no gap, no overlap
    const GuardLayout u = guard_layout(n, false);
    CHECK(u.front == 0 && u.back == 0 && u.payload_offset() == 0 && u.total() == n);                   // knob unset: the caller's bytes

    std::vector<uint8_t> m = image(g);
    const uint8_t *front = m.data(), *back = m.data() + g.back_offset();
    CHECK(scan_guard(front, g.front, false).count == 0);
    CHECK(scan_guard(back, g.back, true).count == 0);

    // the byte that touches the payload, on either side
    m[g.payload_offset() - 1] = 0x00;
    m[g.back_offset()] = 0x01;
    GuardDamage f = scan_guard(front, g.front, false), b = scan_guard(back, g.back, true);
    CHECK(f.count == 1 && f.first == 0 && f.last == 0 && f.first_byte == 0x00);
    CHECK(b.count == 1 && b.first == 0 && b.last == 0 && b.first_byte == 0x01);
    // ... and the byte farthest from it: the first and the last byte of the allocation
    m[0] = 0x02;
    m[g.total() - 1] = 0x03;
    f = scan_guard(front, g.front, false);
    b = scan_guard(back, g.back, true);
    CHECK(f.count == 2 && f.first == 0 && f.last == kGuardBytes - 1 && f.first_byte == 0x00);
    CHECK(b.count == 2 && b.first == 0 && b.last == kGuardBytes - 1 && b.first_byte == 0x01);
    // the near bytes restored: the far ones alone
    m[g.payload_offset() - 1] = kGuardByte;
    m[g.back_offset()] = kGuardByte;
    f = scan_guard(front, g.front, false);
    b = scan_guard(back, g.back, true);
    CHECK(f.count == 1 && f.first == kGuardBytes - 1 && f.first_byte == 0x02);
    CHECK(b.count == 1 && b.first == kGuardBytes - 1 && b.first_byte == 0x03);
    m[0] = m[g.total() - 1] = kGuardByte;

    // offset 5 from the payload's edge (what the GPU test damages), one side at a time: the other side scans clean
    for (int side = 0; side < 2; ++side) {
        uint8_t *band = m.data() + (side ? g.back_offset() : 0);
        const size_t i = guard_index(kGuardBytes, side != 0, 5);
        CHECK(i == (side ? 5u : kGuardBytes - 6));
        band[i] = kPoisonByte;                              // poison in a guard is damage too: the patterns differ
        const GuardDamage hit = scan_guard(band, kGuardBytes, side != 0);
        const GuardDamage other = scan_guard(m.data() + (side ? 0 : g.back_offset()), kGuardBytes, side == 0);
        CHECK(hit.count == 1 && hit.first == 5 && hit.last == 5 && hit.first_byte == kPoisonByte);
        CHECK(other.count == 0);
        band[i] = kGuardByte;
    }
    // a run that a dword store one element past the end leaves, and a second one deeper in
    for (size_t k = 0; k < 4; ++k) m[g.back_offset() + k] = 0;
    m[g.back_offset() + 100] = 7;
    b = scan_guard(back, g.back, true);
    CHECK(b.count == 5 && b.first == 0 && b.last == 100 && b.first_byte == 0);
    // the payload itself is never looked at: every byte of it changed, both scans as before
    memset(m.data() + g.payload_offset(), kGuardByte ^ 0xff, g.payload);
    CHECK(scan_guard(front, g.front, false).count == 0);
    CHECK(scan_guard(back, g.back, true).count == 5);
}

int main()
{
    static_assert(kGuardBytes == 4096, "the guard is one 4 KiB page");
    static_assert(kGuardByte != kPoisonByte && kPoisonByte != 0 && kGuardByte != 0, "three distinguishable fills");
    // 8 294 400 = 3840 x 2160 = 2025 x 4096: a 4K plane, the size that lands exactly on the allocator's rounding
    for (size_t n : {(size_t)0, (size_t)1, (size_t)4095, (size_t)4096, (size_t)4097, (size_t)8294400}) check_layout(n);
    CHECK((size_t)8294400 == (size_t)2025 * 4096);

    // a band shorter than a page, and an empty one
    const uint8_t two[2] = {kGuardByte, 0x00};
    CHECK(scan_guard(two, 2, true).first == 1 && scan_guard(two, 2, false).first == 0);
    CHECK(scan_guard(two, 0, true).count == 0 && scan_guard(nullptr, 0, false).count == 0);

    // the knobs
    CHECK(!test_knob_on(nullptr));
    for (const char *off : {"", "0", "00", " 0", "0 ", "\t"}) CHECK(!test_knob_on(off));
    for (const char *on : {"1", "2", "-1", "01", "10", "on", "yes", " 1"}) CHECK(test_knob_on(on));
    CHECK(setenv("BBME_TEST_GUARD", "1", 1) == 0 && test_knob_on(getenv("BBME_TEST_GUARD")));
    CHECK(setenv("BBME_TEST_GUARD", "0", 1) == 0 && !test_knob_on(getenv("BBME_TEST_GUARD")));
    CHECK(unsetenv("BBME_TEST_GUARD") == 0 && !test_knob_on(getenv("BBME_TEST_GUARD")));

    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("guard layout ok\n");
    return 0;
}
