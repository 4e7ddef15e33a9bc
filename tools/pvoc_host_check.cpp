// pvoc_host_check.cpp -- the host-only half of the phase-vocoder stage under AddressSanitizer and UndefinedBehaviorSanitizer:
// afg_pvoc_out_frames, afg_pvoc_bound and the record and parameter checks of afg_pvoc_hip (afg_pvoc_check_rows), each at its
// extremes -- n_fft 2 and 65536, rate 1/64 and 64, n_frames 2^24, offsets at the ends of the planes, pitches of 2^32 - 1 --
// with the records in heap buffers of exactly their size.  `make -C audio-formats_amd pvoc_host_check` compiles the host side
// of csrc/pvoc.hip with -fsanitize=address,undefined into this program (everything else comes from the library as it is) and
// runs it.  It needs no device and makes no device call.
#include "../include/afg.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                                                    \
    do {                                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, afg_last_error()); failures++; } \
    } while (0)

static afg_pvoc_params params_of(uint32_t n_fft, uint32_t hop)
{
    afg_pvoc_params p;
    std::memset(&p, 0, sizeof(p));
    p.n_fft = n_fft; p.hop = hop;
    return p;
}

// the count by its definition, walked from a safe start
static uint32_t count_of(uint32_t n_frames, double rate)
{
    uint64_t t = (uint64_t)((double)n_frames / rate);
    t = t > 4 ? t - 4 : 0;
    for (;; t++) {
        volatile double s = (double)t * rate;
        if (!(s < (double)n_frames)) return (uint32_t)t;
    }
}

static void frame_counts()
{
    const double rates[] = { 1.0, 0.5, 2.0, 1.25, 0.8, 1.0 / 3.0, 1.1, 0.9, 64.0, 1.0 / 64.0, 0.999999999, 1.000000001, 63.999, 0.0157 };
    const uint32_t frames[] = { 1, 2, 3, 63, 64, 65, 1000, 65537, (1u << 24) - 1, 1u << 24 };
    for (double r : rates)
        for (uint32_t f : frames) EXPECT(afg_pvoc_out_frames(f, r) == count_of(f, r));
    EXPECT(afg_pvoc_out_frames(1u << 24, 1.0 / 64.0) == (1u << 30));
    EXPECT(afg_pvoc_out_frames(0, 1.0) == 0 && afg_pvoc_out_frames((1u << 24) + 1, 1.0) == 0 && afg_pvoc_out_frames(0xffffffffu, 1.0) == 0);
    const double bad[] = { 0.0, -1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                           -std::numeric_limits<double>::infinity(), 1.0 / 64.001, 64.001, 5e-324 };
    for (double r : bad) EXPECT(afg_pvoc_out_frames(5, r) == 0);
}

static void records_and_refusals()
{
    const afg_pvoc_params shapes[] = { params_of(400, 160), params_of(2, 1), params_of(2, 2), params_of(16, 4), params_of(65536, 65536), params_of(65535, 1) };
    for (const afg_pvoc_params &p : shapes) {
        const uint64_t n_bins = p.n_fft / 2 + 1;
        const struct { uint32_t f; double rate; uint32_t in_pitch, out_pitch; } want[] = {
            { 1, 1.0, 0, 0 }, { 7, 0.8, 0xffffffffu, 0 }, { 0, 1.0, 0, 0 }, { 40, 64.0, 0, 0xffffffffu }, { 1u << 24, 1.0 / 64.0, 0, 0 }, { 1000, 1.25, 0, 0 } };
        std::vector<afg_pvoc_row> made;
        uint64_t a = 3, b = 5;
        for (const auto &w : want) {
            afg_pvoc_row r;
            std::memset(&r, 0, sizeof(r));
            r.in_off = a; r.out_off = b; r.rate = w.rate; r.n_frames = w.f;
            r.out_frames = w.f ? afg_pvoc_out_frames(w.f, w.rate) : 0;
            r.in_pitch = w.in_pitch ? w.in_pitch : w.f;
            r.out_pitch = w.out_pitch ? w.out_pitch : r.out_frames;
            made.push_back(r);
            if (r.out_frames) {
                a += 2 * ((n_bins - 1) * r.in_pitch + r.n_frames);
                b += 2 * ((n_bins - 1) * r.out_pitch + r.out_frames);
            }
        }
        const uint64_t n = made.size();
        afg_pvoc_row *heap = (afg_pvoc_row *)std::malloc(n * sizeof(afg_pvoc_row));                  // exactly the records
        std::memcpy(heap, made.data(), n * sizeof(afg_pvoc_row));
        EXPECT(afg_pvoc_check_rows(heap, n, &p, a, b) == AFG_OK);
        EXPECT(afg_pvoc_check_rows(nullptr, 0, &p, 0, 0) == AFG_OK);
        EXPECT(afg_pvoc_check_rows(nullptr, n, &p, a, b) == AFG_ERR_INVALID);
        EXPECT(afg_pvoc_check_rows(heap, n, &p, a - 1, b) == AFG_ERR_INVALID);                       // the last slab ends on the plane's end
        EXPECT(afg_pvoc_check_rows(heap, n, &p, a, b - 1) == AFG_ERR_INVALID);
        EXPECT(afg_pvoc_check_rows(heap, n, &p, 0, b) == AFG_ERR_INVALID);
        const uint64_t top = ~(uint64_t)0;
        for (int k = 0; k < 12; k++) {
            const afg_pvoc_row keep = heap[3];
            switch (k) {
            case 0: heap[3].in_off = top - 3; break;
            case 1: heap[3].out_off = top - 3; break;
            case 2: heap[3].out_frames += 1; break;
            case 3: heap[3].out_frames = 0xffffffffu; break;
            case 4: heap[3].n_frames = 0; break;
            case 5: heap[3].in_pitch = 39; break;
            case 6: heap[3].out_pitch = heap[3].out_frames - 1; break;
            case 7: heap[3].rate = std::numeric_limits<double>::quiet_NaN(); break;
            case 8: heap[3].rate = 64.5; break;
            case 9: heap[3].reserved[1] = 1; break;
            case 10: heap[3].n_frames = 0xffffffffu; heap[3].in_pitch = 0xffffffffu; break;
            default: heap[3].in_off = top / 2 + 1; heap[3].out_off = top / 2 + 1; break;
            }
            EXPECT(afg_pvoc_check_rows(heap, n, &p, a, b) == AFG_ERR_INVALID);
            heap[3] = keep;
        }
        EXPECT(afg_pvoc_check_rows(heap, n, &p, a, b) == AFG_OK);
        const double b0 = afg_pvoc_bound(&p, 0), b1 = afg_pvoc_bound(&p, ~(uint64_t)0);
        EXPECT(b0 > AFG_PVOC_KA * 0x1p-24 && b0 < (AFG_PVOC_KA + 1) * 0x1p-24 && b1 > b0 && std::isfinite(b1));
        // a kernel entry with made-up device addresses stops at the parameters or the arguments
        afg_pvoc_params bad = p;
        bad.reserved[5] = 1;
        EXPECT(afg_pvoc_hip(n, (const afg_pvoc_row *)0x1000, &bad, (const float *)0x2000, 8, (float *)0x4000, 8, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_pvoc_hip(n, nullptr, &p, (const float *)0x2000, 8, (float *)0x4000, 8, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_pvoc_hip(n, (const afg_pvoc_row *)0x1000, &p, (const float *)0x2001, 8, (float *)0x4000, 8, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_pvoc_hip(n, (const afg_pvoc_row *)0x1000, &p, (const float *)0x2000, 8, (float *)0x2010, 8, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_pvoc_hip(0x7fffffffull, (const afg_pvoc_row *)0x1000, &p, (const float *)0x2000, 8, (float *)0x4000, 8, nullptr) == AFG_ERR_INVALID || n_bins <= 4);
        EXPECT(afg_pvoc_hip(0, nullptr, &p, nullptr, 0, nullptr, 0, nullptr) == AFG_OK);
        std::free(heap);
    }
}

static void parameters()
{
    EXPECT(afg_pvoc_bound(nullptr, 0) < 0.0 && afg_pvoc_check_rows(nullptr, 0, nullptr, 0, 0) == AFG_ERR_INVALID);
    for (int k = 0; k < 7; k++) {
        afg_pvoc_params p = params_of(400, 160);
        switch (k) {
        case 0: p.n_fft = 1; p.hop = 1; break;
        case 1: p.n_fft = 65537; break;
        case 2: p.n_fft = 0xffffffffu; break;
        case 3: p.hop = 0; break;
        case 4: p.hop = 401; break;
        case 5: p.reserved[0] = 1; break;
        default: p.reserved[5] = 0x80000000u; break;
        }
        EXPECT(afg_pvoc_bound(&p, 0) < 0.0 && afg_pvoc_check_rows(nullptr, 0, &p, 0, 0) == AFG_ERR_INVALID);
    }
}

int main()
{
    frame_counts();
    records_and_refusals();
    parameters();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("pvoc_host_check: ok\n");
    return 0;
}
