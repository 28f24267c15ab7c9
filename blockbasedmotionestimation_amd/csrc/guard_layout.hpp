// guard_layout.hpp -- the test layout of a device allocation (DevBuf, bbme_device.hip): guard bands around the payload, the byte
// patterns of guards and poison, the two knobs that switch them on, and the scan of a host copy of a guard band.
// Plain C++17 without HIP: tests/cpp/guard_layout_test.cpp checks the arithmetic without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace bbme {

// BBME_TEST_GUARD=1: an allocation of n bytes becomes [kGuardBytes][n payload bytes][kGuardBytes], both bands filled with
// kGuardByte.  A multiple of 4 KiB keeps every alignment the code relies on (hipMalloc's own, and the 4 KiB of Level::img2).
// BBME_TEST_POISON=1: the payload of a data buffer starts as kPoisonByte in every byte.  As a motion vector 0xC7C7 is
// (-14393, -14393), far outside any plane; as a float or double the word is a large finite negative number; as a 64-bit sum it
// is beyond anything a statistic reaches: a result computed from a poisoned word differs from its reference.
constexpr size_t kGuardBytes = 4096;
constexpr uint8_t kGuardByte = 0xA5;
constexpr uint8_t kPoisonByte = 0xC7;

// A knob is on when it is set to anything but blanks and zeros ("", "0", "00", " 0" are off; "1", "on", "-1" are on).
inline bool test_knob_on(const char *value)
{
    if (!value) return false;
    for (const char *p = value; *p; ++p)
        if (*p != ' ' && *p != '\t' && *p != '0') return true;
    return false;
}

struct GuardLayout {
    size_t front = 0;          // bytes of guard in front of the payload (0: unguarded)
    size_t payload = 0;        // the caller's bytes
    size_t back = 0;           // bytes of guard behind it
    size_t total() const { return front + payload + back; }             // what to allocate
    size_t payload_offset() const { return front; }                     // from the base
    size_t back_offset() const { return front + payload; }              // from the base
};

inline GuardLayout guard_layout(size_t payload, bool guarded)
{
    GuardLayout g;
    g.payload = payload;
    g.front = g.back = guarded ? kGuardBytes : 0;
    return g;
}

// The damage of one guard band, as offsets FROM THE PAYLOAD'S EDGE: 0 is the byte that touches the payload (the last byte of
// the front band, the first byte of the back band), kGuardBytes - 1 the byte farthest from it.
struct GuardDamage {
    size_t count = 0;          // damaged bytes
    size_t first = 0, last = 0;    // nearest and farthest damaged offset (count > 0)
    uint8_t first_byte = 0;    // what the nearest one holds
};

// Scans a host copy of a band of `n` bytes; `back` says on which side of the payload it lies.
inline GuardDamage scan_guard(const uint8_t *band, size_t n, bool back)
{
    GuardDamage d;
    for (size_t off = 0; off < n; ++off) {
        const uint8_t v = back ? band[off] : band[n - 1 - off];
        if (v == kGuardByte) continue;
        if (!d.count) { d.first = off; d.first_byte = v; }
        d.last = off;
        ++d.count;
    }
    return d;
}

// The index into a band of `n` bytes of the byte at offset `off` from the payload's edge (scan_guard's inverse).
inline size_t guard_index(size_t n, bool back, size_t off) { return back ? off : n - 1 - off; }

}  // namespace bbme
