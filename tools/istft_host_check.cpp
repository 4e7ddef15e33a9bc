// istft_host_check.cpp -- the host-only half of the inverse STFT stage under AddressSanitizer and UndefinedBehaviorSanitizer:
// afg_istft_tile_samples, afg_istft_layout, afg_istft_envelope_min and the record and parameter checks of afg_istft_hip
// (afg_istft_check_rows), each at its extremes -- n_fft 16 and 2048, hop 1 and n_fft, offsets at the ends of the planes,
// in_pitch 2^32 - 1 -- with the records in heap buffers of exactly their size.  `make -C audio-formats_amd istft_host_check`
// compiles the host side of csrc/istft.hip with -fsanitize=address,undefined into this program (everything else comes from
// the library as it is) and runs it.  It needs no device and makes no device call.
#include "../include/afg.h"

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                                                    \
    do {                                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, afg_last_error()); failures++; } \
    } while (0)

static afg_istft_params params_of(uint32_t n_fft, uint32_t win, uint32_t hop, uint32_t center)
{
    afg_istft_params p;
    std::memset(&p, 0, sizeof(p));
    p.n_fft = n_fft; p.win_length = win; p.hop = hop; p.center = center;
    return p;
}

static uint64_t line_of(const afg_istft_params &p, uint32_t n_frames) { return (uint64_t)p.n_fft + (uint64_t)p.hop * (n_frames - 1); }

static void records_and_refusals()
{
    const afg_istft_params shapes[] = { params_of(400, 400, 160, 1), params_of(16, 16, 1, 1), params_of(16, 16, 4, 0), params_of(75, 60, 20, 1),
                                        params_of(1024, 1000, 256, 1), params_of(2048, 2048, 1, 1), params_of(2048, 2048, 1024, 0),
                                        params_of(1875, 1875, 625, 1), params_of(2025, 2000, 405, 0) };
    const uint32_t frames[] = { 1, 2, 3, 40, 1000, 0xffffffffu };
    for (const afg_istft_params &p : shapes) {
        const uint32_t tile = afg_istft_tile_samples(&p), n_bins = p.n_fft / 2 + 1, pad = p.center ? p.n_fft / 2 : 0, n_lo = (p.n_fft - p.win_length) / 2;
        EXPECT(tile >= 256 && tile % 256 == 0 && tile <= 16384);
        const uint64_t table = (uint64_t)p.win_length + 2 * (uint64_t)p.n_fft;
        std::vector<afg_istft_row> made;
        uint64_t a = 3, b = 5, want = 0;
        for (uint32_t f : frames) {
            afg_istft_row r;
            std::memset(&r, 0, sizeof(r));
            r.in_off = a; r.out_off = b; r.n_frames = f; r.in_pitch = f == 40 ? 0xffffffffu : f;
            r.out_first = p.center ? 0 : n_lo + 2;                  // (w[1]^2 is below 1e-11 for the longest windows)
            const uint64_t room = line_of(p, f) - pad - r.out_first;
            const uint64_t most = f == 1 ? (uint64_t)p.win_length / 4 : room - p.n_fft / 2;      // (short of the line's end, where the last window tails off)
            r.out_frames = (uint32_t)(most > 0xffffffffull ? 0xffffffffull : most);
            if (f == 3) r.out_frames = 0;
            made.push_back(r);
            a += 2 * ((uint64_t)(n_bins - 1) * r.in_pitch + f);
            b += r.out_frames;
            want += ((uint64_t)r.out_frames + tile - 1) / tile;
        }
        const uint64_t n = made.size();
        afg_istft_row *heap = (afg_istft_row *)std::malloc(n * sizeof(afg_istft_row));                // exactly the records
        std::memcpy(heap, made.data(), n * sizeof(afg_istft_row));
        const uint64_t tiles = afg_istft_layout(heap, n, &p);
        EXPECT(tiles == want && heap[0].first_tile == 0 && heap[n - 1].first_tile + ((uint64_t)heap[n - 1].out_frames + tile - 1) / tile == tiles);
        EXPECT(afg_istft_check_rows(heap, n, tiles, &p, a, table, b) == AFG_OK);
        EXPECT(afg_istft_check_rows(nullptr, 0, 0, &p, 0, 0, 0) == AFG_OK);
        EXPECT(afg_istft_check_rows(nullptr, n, tiles, &p, a, table, b) == AFG_ERR_INVALID);
        EXPECT(afg_istft_check_rows(heap, n, tiles, &p, a - 1, table, b) == AFG_ERR_INVALID);        // the last slab ends on the plane's end
        EXPECT(afg_istft_check_rows(heap, n, tiles, &p, a, table, b - 1) == AFG_ERR_INVALID);
        EXPECT(afg_istft_check_rows(heap, n, tiles, &p, a, table - 1, b) == AFG_ERR_INVALID);
        EXPECT(afg_istft_check_rows(heap, n, tiles + 1, &p, a, table, b) == AFG_ERR_INVALID);
        const uint64_t top = ~(uint64_t)0;
        for (int k = 0; k < 8; k++) {
            const afg_istft_row keep = heap[3];
            switch (k) {
            case 0: heap[3].in_off = top - 3; break;
            case 1: heap[3].out_off = top - 3; break;
            case 2: heap[3].first_tile += 1; break;
            case 3: heap[3].out_frames = 0xffffffffu; break;                                         // past the line
            case 4: heap[3].n_frames = 0; break;
            case 5: heap[3].in_pitch = 39; break;
            case 6: heap[3].out_first = 0xffffffffu; break;
            default: heap[3].out_first = p.center ? 0 : n_lo; heap[3].out_frames = p.center ? (uint32_t)(line_of(p, 40) - pad) : 1; break;      // the envelope's zero, or its tail
            }
            const int rc = afg_istft_check_rows(heap, n, tiles, &p, a, table, b);
            if (k < 7) EXPECT(rc == AFG_ERR_INVALID);
            else EXPECT(rc == AFG_ERR_INVALID || p.center);                                          // (a centred line may end above 1e-11)
            heap[3] = keep;
        }
        EXPECT(afg_istft_check_rows(heap, n, tiles, &p, a, table, b) == AFG_OK);
        // the envelope of the longest row, from either end, costs no pass over it
        const double d = afg_istft_envelope_min(&p, 0xffffffffu, heap[n - 1].out_first, heap[n - 1].out_frames);
        EXPECT(d >= 1e-11);
        EXPECT(afg_istft_envelope_min(&p, 1, p.center ? 0 : n_lo + 2, 1) > 0.0);
        EXPECT(afg_istft_envelope_min(&p, 1, 0, (uint32_t)(line_of(p, 1) - pad) + 1) < 0.0);
        EXPECT(afg_istft_envelope_min(&p, 0xffffffffu, 0xffffffffu, 0xffffffffu) < 0.0 || line_of(p, 0xffffffffu) >= 2 * (uint64_t)0xffffffffu + pad);
        // a kernel entry with made-up device addresses stops at the parameters or the arguments
        afg_istft_params bad = p;
        bad.reserved[3] = 1;
        EXPECT(afg_istft_hip(n, (const afg_istft_row *)0x1000, tiles, &bad, (const float *)0x2000, a, (const float *)0x3000, table, (float *)0x4000, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_istft_hip(n, nullptr, tiles, &p, (const float *)0x2000, a, (const float *)0x3000, table, (float *)0x4000, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_istft_hip(n, (const afg_istft_row *)0x1000, tiles, &p, (const float *)0x2001, a, (const float *)0x3000, table, (float *)0x4000, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_istft_hip(0, nullptr, 0, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == AFG_OK);
        std::free(heap);
    }
}

static void parameters()
{
    const afg_istft_params good = params_of(400, 400, 160, 1);
    EXPECT(afg_istft_tile_samples(&good) == 10240 && afg_istft_layout(nullptr, 0, &good) == 0);
    EXPECT(afg_istft_tile_samples(nullptr) == 0 && afg_istft_layout(nullptr, 0, nullptr) == 0 && afg_istft_envelope_min(nullptr, 1, 0, 1) < 0.0);
    for (uint32_t n_fft : { 0u, 15u, 17u, 2049u, 14u * 3u * 5u, 0xffffffffu }) {
        afg_istft_params p = good;
        p.n_fft = n_fft;
        EXPECT(afg_istft_tile_samples(&p) == 0 && afg_istft_layout(nullptr, 0, &p) == 0 && afg_istft_envelope_min(&p, 1, 0, 1) < 0.0);
        EXPECT(afg_istft_check_rows(nullptr, 0, 0, &p, 0, 0, 0) == AFG_ERR_UNSUPPORTED);
    }
    for (int k = 0; k < 8; k++) {
        afg_istft_params p = good;
        switch (k) {
        case 0: p.win_length = 0; break;
        case 1: p.win_length = 401; break;
        case 2: p.hop = 0; break;
        case 3: p.hop = 401; break;
        case 4: p.center = 2; break;
        case 5: p.reserved[0] = 1; break;
        case 6: p.reserved[3] = 0x80000000u; break;
        default: p.hop = 0xffffffffu; break;
        }
        EXPECT(afg_istft_tile_samples(&p) == 0 && afg_istft_envelope_min(&p, 1, 0, 1) < 0.0);
        EXPECT(afg_istft_check_rows(nullptr, 0, 0, &p, 0, 0, 0) == AFG_ERR_INVALID);
    }
    // every n_fft the path takes has a geometry, at the shortest and the longest hop
    for (uint32_t n_fft = 16; n_fft <= 2048; n_fft++) {
        uint32_t m = n_fft;
        for (uint32_t q : { 2u, 3u, 5u })
            while (m % q == 0) m /= q;
        for (uint32_t hop : { 1u, n_fft }) {
            const afg_istft_params p = params_of(n_fft, n_fft, hop, 1);
            EXPECT((afg_istft_tile_samples(&p) != 0) == (m == 1));
        }
    }
}

int main()
{
    records_and_refusals();
    parameters();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("istft_host_check: ok\n");
    return 0;
}
