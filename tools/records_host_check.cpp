// records_host_check.cpp -- the record toolkit the tensor stages share (audio-formats_amd/csrc/afg_records.h, header only)
// under AddressSanitizer and UndefinedBehaviorSanitizer: the containment test afg::rows_inside at its extremes -- planes,
// offsets and strides near 2^64, each case just inside and just outside by one float, and a grid against 128-bit
// arithmetic -- the overlap sweep afg::first_overlap over the cases the filter and loudness checks meet, and the caps of a
// launch.  `make -C audio-formats_amd records_host_check` compiles this file with -fsanitize=address,undefined (the header's
// code with it; afg_last_error comes from the library) and runs it.  It needs no device and makes no device call.
#include "../audio-formats_amd/csrc/afg_records.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                                                    \
    do {                                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

typedef unsigned __int128 u128;
static const uint64_t kMax = ~(uint64_t)0;

// off + (rows - 1) * stride + len <= floats, in arithmetic that cannot wrap (below 2^64 * 65535 + 2^65)
static bool wide_inside(uint64_t off, uint64_t rows, uint64_t stride, uint64_t len, uint64_t floats)
{
    return (u128)off + (u128)(rows - 1) * stride + len <= (u128)floats;
}

static void containment()
{
    const uint64_t rows_of[] = { 1, 2, 65535 }, lens[] = { 0, 1, 0xffffffffull };
    const uint64_t planes[] = { kMax, kMax - 1, ((uint64_t)1 << 63) + 3, (uint64_t)1 << 63, ((uint64_t)1 << 32) + 7, 0xffffffffull };
    unsigned edges = 0;
    for (uint64_t floats : planes)
        for (uint64_t rows : rows_of)
            for (uint64_t len : lens) {
                if (len > floats) continue;
                // strides from none to the largest the plane takes with offset 0, and the one past it
                const uint64_t most = rows == 1 ? kMax : (floats - len) / (rows - 1);
                const uint64_t strides[] = { 0, 1, len, most / 2, most > 0 ? most - 1 : 0, most };
                for (uint64_t stride : strides) {
                    const u128 body = (u128)(rows - 1) * stride + len;
                    if (rows > 1 && body > floats) continue;
                    const uint64_t reach = rows == 1 ? len : (uint64_t)body, off = floats - reach;       // the last offset inside
                    EXPECT(afg::rows_inside(off, rows, stride, len, floats));
                    EXPECT(afg::rows_inside(0, rows, stride, len, floats));
                    if (off < kMax) EXPECT(!afg::rows_inside(off + 1, rows, stride, len, floats));       // one float further
                    if (floats > 0 && reach + off == floats) EXPECT(!afg::rows_inside(off, rows, stride, len, floats - 1));   // one float less
                    EXPECT(!afg::rows_inside(kMax, rows, stride, len, floats) || (off == kMax));
                    edges++;
                }
                if (rows > 1 && most < kMax) {
                    EXPECT(afg::rows_inside(0, rows, most, len, floats));
                    EXPECT(!afg::rows_inside(0, rows, most + 1, len, floats));                           // one float further a row
                    for (uint64_t stride : { kMax - 1, kMax })
                        EXPECT(afg::rows_inside(0, rows, stride, len, floats) == wide_inside(0, rows, stride, len, floats));
                }
            }
    EXPECT(edges > 100);
    EXPECT(!afg::rows_inside(0, 1, 0, 1, 0) && afg::rows_inside(0, 1, 0, 0, 0) && !afg::rows_inside(1, 1, 0, 0, 0));
    EXPECT(!afg::rows_inside(0, 65535, 1, 0xffffffffull, 0xffffffffull + 65533) && afg::rows_inside(0, 65535, 1, 0xffffffffull, 0xffffffffull + 65534));
    // a grid around every boundary against the wide form
    const uint64_t marks[] = { 0, 1, 2, 0xfffffffeull, 0xffffffffull, (uint64_t)1 << 32, ((uint64_t)1 << 63) - 1, (uint64_t)1 << 63, kMax - 2, kMax - 1, kMax };
    unsigned long long grid = 0, inside = 0;
    for (uint64_t floats : marks)
        for (uint64_t off : marks)
            for (uint64_t stride : marks)
                for (uint64_t rows : rows_of)
                    for (uint64_t len : lens) {
                        const bool got = afg::rows_inside(off, rows, stride, len, floats);
                        EXPECT(got == wide_inside(off, rows, stride, len, floats));
                        grid++;
                        inside += got ? 1 : 0;
                    }
    EXPECT(grid == 11ull * 11 * 11 * 9 && inside > 100 && inside < grid);
}

// the ranges in a heap buffer of exactly their size, as the checks push them
static bool overlap(std::vector<afg::Range> r, uint64_t *owner, uint64_t *other)
{
    r.shrink_to_fit();
    *owner = *other = 99;
    return afg::first_overlap(r, owner, other);
}

static void sweep()
{
    uint64_t a = 0, b = 0;
    const uint64_t top = kMax - 64;
    EXPECT(!overlap({}, &a, &b));
    // disjoint, in any order, up to the end of the address range
    EXPECT(!overlap({ { 100, 200, 0, true }, { 0, 50, 1, true }, { top, kMax, 2, true }, { 300, 400, 3, false } }, &a, &b));
    // ranges that touch: outputs, and an output against an input on either side
    EXPECT(!overlap({ { 0, 100, 0, true }, { 100, 200, 1, true }, { 200, 300, 2, false }, { 300, 400, 3, true } }, &a, &b));
    // in place: the caller gives an output at its input's offset one range, whatever the other records' inputs do
    EXPECT(!overlap({ { 0, 100, 0, true }, { 100, 200, 1, true }, { 500, 600, 2, false }, { 550, 650, 3, false } }, &a, &b));
    // an input overlapping an input, also at the same offset, is allowed
    EXPECT(!overlap({ { 0, 100, 0, false }, { 50, 150, 1, false }, { 50, 120, 2, false }, { 200, 300, 0, true }, { 300, 301, 1, true } }, &a, &b));
    // two outputs that overlap: by one float, one inside the other, the same range twice
    EXPECT(overlap({ { 0, 100, 0, true }, { 99, 199, 1, true } }, &a, &b) && a == 1 && b == 0);
    EXPECT(overlap({ { 50, 60, 4, true }, { 0, 100, 7, true } }, &a, &b) && a == 4 && b == 7);
    EXPECT(overlap({ { 10, 20, 2, true }, { 10, 20, 3, true } }, &a, &b) && ((a == 2 && b == 3) || (a == 3 && b == 2)));
    EXPECT(overlap({ { top, kMax, 0, true }, { kMax - 1, kMax, 1, true } }, &a, &b) && a == 1 && b == 0);
    // an output overlapping a foreign input, from either side and at the same offset
    EXPECT(overlap({ { 0, 100, 0, false }, { 99, 199, 1, true } }, &a, &b) && a == 1 && b == 0);
    EXPECT(overlap({ { 0, 100, 0, true }, { 99, 199, 1, false } }, &a, &b) && a == 1 && b == 0);
    EXPECT(overlap({ { 40, 140, 5, false }, { 40, 50, 6, true } }, &a, &b) && a == 5 && b == 6);
    // ... behind a longer range that ended earlier in the order: the furthest end counts, not the last one
    EXPECT(overlap({ { 0, 1000, 0, true }, { 10, 20, 1, false }, { 500, 600, 2, false } }, &a, &b) && a == 1 && b == 0);
    EXPECT(overlap({ { 0, 1000, 0, false }, { 10, 20, 1, false }, { 500, 600, 2, true } }, &a, &b) && a == 2 && b == 0);
    // the first offender in offset order is the one reported
    EXPECT(overlap({ { 700, 800, 3, true }, { 750, 760, 4, true }, { 0, 100, 0, true }, { 50, 60, 1, true } }, &a, &b) && a == 1 && b == 0);
}

static void caps()
{
    EXPECT(afg::launch_caps("afg_x_hip", "rows", 0xffffffffull, 0x7fffffffull) == AFG_OK);
    EXPECT(afg::launch_caps("afg_x_hip", "rows", 0x100000000ull, 0) == AFG_ERR_INVALID);
    EXPECT(std::strcmp(afg_last_error(), "afg_x_hip: at most 2^32 - 1 rows and 2^31 - 1 tiles per launch") == 0);
    EXPECT(afg::launch_caps("afg_y_hip", "spans", 1, 0x80000000ull) == AFG_ERR_INVALID);
    EXPECT(std::strcmp(afg_last_error(), "afg_y_hip: at most 2^32 - 1 spans and 2^31 - 1 tiles per launch") == 0);
    EXPECT(afg::launch_caps("afg_y_hip", "spans", kMax, kMax) == AFG_ERR_INVALID);
    EXPECT(afg::gcd32(48000, 44100) == 300 && afg::gcd32(0, 7) == 7 && afg::gcd32(7, 0) == 7 && afg::gcd32(0xffffffffu, 0xffffffffu) == 0xffffffffu);
}

int main()
{
    containment();
    sweep();
    caps();
    if (failures) { std::fprintf(stderr, "records_host_check: %d failures\n", failures); return 1; }
    std::printf("records_host_check: ok\n");
    return 0;
}
