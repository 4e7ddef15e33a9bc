// convolve_host_check.cpp -- the host-only half of the convolution stage under AddressSanitizer and UndefinedBehaviorSanitizer:
// afg_convolve_bank_layout, afg_convolve_bank_check, afg_convolve_layout, afg_convolve_bound and the record checks of
// afg_convolve_hip (afg_convolve_check_rows), each at its extremes -- taps 1 and 65536, rows of 1 and of 2^31 - 65536 frames,
// ranges at both ends of the line, offsets at the ends of the planes and ones that would wrap, planes that touch and that
// overlap -- with the records in heap buffers of exactly their size.  `make -C audio-formats_amd convolve_host_check` compiles
// the host side of csrc/convolve.hip with -fsanitize=address,undefined into this program (everything else comes from the
// library as it is) and runs it.  It needs no device and makes no device call.
#include "../include/afg.h"

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

static afg_convolve_params params_of(uint32_t direct_max)
{
    afg_convolve_params p;
    std::memset(&p, 0, sizeof(p));
    p.direct_max = direct_max;
    return p;
}

template <typename T> static T *heap_of(const std::vector<T> &v)
{
    T *h = (T *)std::malloc(v.size() * sizeof(T));               // exactly the records
    std::memcpy(h, v.data(), v.size() * sizeof(T));
    return h;
}

static void banks_and_rows()
{
    const uint32_t taps[] = { 1, 128, 129, 1024, 1025, 65535, 65536 };
    std::vector<afg_convolve_kernel> made;
    uint64_t bank = 2, parts = 0;
    for (uint32_t t : taps) {
        afg_convolve_kernel k;
        std::memset(&k, 0, sizeof(k));
        k.bank_off = bank; k.taps = t;
        made.push_back(k);
        bank += t;
        parts += (t + AFG_CONV_BLOCK - 1) / AFG_CONV_BLOCK;
    }
    const uint64_t nk = made.size();
    afg_convolve_kernel *ks = heap_of(made);
    const uint64_t spec = afg_convolve_bank_layout(ks, nk);
    EXPECT(spec == AFG_CONV_TABLE_FLOATS + parts * AFG_CONV_SPEC_FLOATS);
    EXPECT(ks[0].spec_off == AFG_CONV_TABLE_FLOATS && ks[nk - 1].spec_off == spec - 64 * (uint64_t)AFG_CONV_SPEC_FLOATS);
    EXPECT(afg_convolve_bank_check(ks, nk, bank, spec) == AFG_OK);
    EXPECT(afg_convolve_bank_check(ks, nk, bank - 1, spec) == AFG_ERR_INVALID && afg_convolve_bank_check(ks, nk, bank, spec - 1) == AFG_ERR_INVALID);
    EXPECT(afg_convolve_bank_check(nullptr, nk, bank, spec) == AFG_ERR_INVALID && afg_convolve_bank_check(nullptr, 0, 0, AFG_CONV_TABLE_FLOATS) == AFG_OK);
    EXPECT(afg_convolve_bank_layout(nullptr, 0) == AFG_CONV_TABLE_FLOATS && afg_convolve_bank_layout(nullptr, 3) == 0);
    for (int c = 0; c < 6; c++) {
        const afg_convolve_kernel keep = ks[4];
        int want = AFG_ERR_INVALID;
        switch (c) {
        case 0: ks[4].taps = 0; break;
        case 1: ks[4].taps = 65537; want = AFG_ERR_UNSUPPORTED; break;
        case 2: ks[4].taps = 0xffffffffu; want = AFG_ERR_UNSUPPORTED; break;
        case 3: ks[4].bank_off = ~(uint64_t)0 - 3; break;
        case 4: ks[4].spec_off += 2; break;
        default: ks[4].reserved = 1; break;
        }
        EXPECT(afg_convolve_bank_check(ks, nk, bank, spec) == want);
        if (c < 3) EXPECT(afg_convolve_bank_layout(ks, nk) == 0);
        ks[4] = keep;
        EXPECT(afg_convolve_bank_layout(ks, nk) == spec);
    }

    const uint32_t big = 0x7fff0000u;
    for (uint32_t direct_max : { 128u, 0u, 64u }) {
        const afg_convolve_params p = params_of(direct_max);
        // frames, kernel, out_first, out_frames
        const struct { uint32_t frames, kernel, first, count; } want[] = {
            { 1, 0, 0, 1 }, { 1, 6, 0, 65536 }, { 1, 6, 65535, 1 }, { 5000, 1, 127, 5000 }, { 0, 3, 0, 0 }, { 3000, 4, 1024, 3000 }, { 77, 5, 65000, 611 },
            { big, 0, 0, big }, { big, 6, big, 65535 }, { 4097, 2, 0, 4097 + 128 }, { 10, 3, 5, 0 } };
        std::vector<afg_convolve_row> rows;
        uint64_t a = 3, b = 5;
        for (const auto &w : want) {
            afg_convolve_row r;
            std::memset(&r, 0, sizeof(r));
            r.in_off = a; r.out_off = b; r.frames = w.frames; r.kernel = w.kernel; r.out_first = w.first; r.out_frames = w.count;
            rows.push_back(r);
            a += w.frames; b += w.count;
        }
        const uint64_t n = rows.size();
        afg_convolve_row *heap = heap_of(rows);
        uint64_t work = 1;
        const uint64_t tiles = afg_convolve_layout(heap, n, ks, nk, &p, &work);
        EXPECT(tiles > 0 && work % AFG_CONV_SPEC_FLOATS == 0 && (direct_max == 0 || work < 3 * (a + 1024 * n)));
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work, b, nullptr) == AFG_OK);
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a - 1, bank, spec, work, b, nullptr) == AFG_OK);      // (the last row delivers nothing)
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a - 11, bank, spec, work, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work, b - 1, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank - 1, spec, work, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec - 1, work, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(work == 0 || afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work - 1, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_check_rows(heap, n, tiles + 1, ks, nk, &p, a, bank, spec, work, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_check_rows(nullptr, n, tiles, ks, nk, &p, a, bank, spec, work, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_check_rows(nullptr, 0, 0, ks, nk, &p, 0, bank, spec, 0, 0, nullptr) == AFG_OK);
        // planes in one address space: in, bank, spectra, work, out -- touching passes, one float of overlap does not
        const uint64_t at[5] = { 0, a, a + bank, a + bank + spec, a + bank + spec + work };
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work, b, at) == AFG_OK);
        for (int q = 0; q < 4; q++) {
            uint64_t moved[5] = { at[0], at[1], at[2], at[3], at[4] };
            moved[4] = (q == 3 ? at[4] : at[q + 1]) - 6;          // the first output row starts at float 5 of its plane
            if (q == 3 && work == 0) continue;
            EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work, b, moved) == AFG_ERR_INVALID);
        }
        if (work) {
            uint64_t moved[5] = { at[0], at[1], at[2], at[3] - 1, at[4] };
            EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work, b, moved) == AFG_ERR_INVALID);
        }
        const uint64_t top = ~(uint64_t)0;
        for (int c = 0; c < 10; c++) {
            const afg_convolve_row keep = heap[5];
            switch (c) {
            case 0: heap[5].in_off = top - 3; break;
            case 1: heap[5].out_off = top - 3; break;
            case 2: heap[5].out_frames += 1026; break;           // past the line (and other tiles)
            case 3: heap[5].out_first = 0xffffffffu; break;
            case 4: heap[5].frames = 0; break;
            case 5: heap[5].frames = big + 1; break;
            case 6: heap[5].kernel = (uint32_t)nk; break;
            case 7: heap[5].kernel = 0xffffffffu; break;
            case 8: heap[5].first_tile += 1; break;
            default: heap[5].work_off += AFG_CONV_SPEC_FLOATS; break;
            }
            EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work, b, nullptr) == AFG_ERR_INVALID);
            uint64_t w2 = 0;
            if (c == 6 || c == 7) EXPECT(afg_convolve_layout(heap, n, ks, nk, &p, &w2) == 0);
            heap[5] = keep;
        }
        EXPECT(afg_convolve_layout(heap, n, ks, nk, &p, nullptr) == tiles);
        EXPECT(afg_convolve_check_rows(heap, n, tiles, ks, nk, &p, a, bank, spec, work, b, nullptr) == AFG_OK);
        // a kernel entry with made-up device addresses stops at the parameters or the arguments
        afg_convolve_params bad = p;
        bad.reserved[6] = 1;
        const float *in = (const float *)0x10000, *bk = (const float *)0x20000, *sp = (const float *)0x30000;
        float *wk = (float *)0x40000, *out = (float *)0x50000;
        const afg_convolve_row *dr = (const afg_convolve_row *)0x1000;
        const afg_convolve_kernel *dk = (const afg_convolve_kernel *)0x2000;
        EXPECT(afg_convolve_hip(n, dr, tiles, dk, nk, &bad, in, a, bk, bank, sp, spec, wk, work, out, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_hip(n, nullptr, tiles, dk, nk, &p, in, a, bk, bank, sp, spec, wk, work, out, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_hip(n, dr, tiles, dk, nk, &p, in, a, bk, bank, (const float *)0x30004, spec, wk, work, out, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_hip(n, dr, tiles, dk, nk, &p, in, a, bk, bank, sp, spec, wk, work, (float *)0x50002, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_hip(n, dr, 0x80000000ull, dk, nk, &p, in, a, bk, bank, sp, spec, wk, work, out, b, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_hip(0, nullptr, 0, nullptr, 0, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == AFG_OK);
        EXPECT(afg_convolve_bank_hip(nk, nullptr, bk, bank, wk, spec, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_bank_hip(nk, dk, bk, bank, (float *)0x40004, spec, nullptr) == AFG_ERR_INVALID);
        EXPECT(afg_convolve_bank_hip(0, nullptr, nullptr, 0, nullptr, 0, nullptr) == AFG_OK);
        std::free(heap);
    }
    std::free(ks);
}

static void parameters_and_the_bound()
{
    const afg_convolve_params p = params_of(128);
    EXPECT(afg_convolve_bound(&p, 1) == 589.0 && afg_convolve_bound(&p, 1024) == 589.0 && afg_convolve_bound(&p, 1025) == 591.0);
    EXPECT(afg_convolve_bound(&p, 65536) == 715.0 && afg_convolve_bound(&p, 0) < 0.0 && afg_convolve_bound(&p, 65537) < 0.0);
    EXPECT(afg_convolve_bound(nullptr, 5) < 0.0 && afg_convolve_check_rows(nullptr, 0, 0, nullptr, 0, nullptr, 0, 0, 0, 0, 0, nullptr) == AFG_ERR_INVALID);
    for (int c = 0; c < 4; c++) {
        afg_convolve_params q = params_of(128);
        switch (c) {
        case 0: q.direct_max = 129; break;
        case 1: q.direct_max = 0xffffffffu; break;
        case 2: q.reserved[0] = 1; break;
        default: q.reserved[6] = 0x80000000u; break;
        }
        uint64_t work = 7;
        EXPECT(afg_convolve_bound(&q, 5) < 0.0 && afg_convolve_layout(nullptr, 0, nullptr, 0, &q, &work) == 0 && work == 0);
        EXPECT(afg_convolve_check_rows(nullptr, 0, 0, nullptr, 0, &q, 0, 0, AFG_CONV_TABLE_FLOATS, 0, 0, nullptr) == AFG_ERR_INVALID);
    }
}

int main()
{
    banks_and_rows();
    parameters_and_the_bound();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("convolve_host_check: ok\n");
    return 0;
}
