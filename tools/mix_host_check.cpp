// mix_host_check.cpp -- the host-only half of the mixing stage under AddressSanitizer and UndefinedBehaviorSanitizer:
// afg_mix_layout, afg_mix_ratio, every refusal of afg_mix_check_groups and the extremes of its offset arithmetic, and the
// refusals afg_batch_decode_mixed makes before any device call, with the records in heap buffers of exactly their size.
// `make -C audio-formats_amd mix_host_check` compiles host/afg_mix.cpp with -fsanitize=address,undefined into this program
// (everything else comes from the library as it is) and runs it.  It needs no device and makes no device call.
#include "../audio-formats_amd/host/afg_stage.h"

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

static afg_mix_group group_of(uint64_t off, uint64_t stride, uint32_t rows, uint32_t valid, uint64_t noise_off, uint32_t N, uint64_t noise_stride)
{
    afg_mix_group g;
    std::memset(&g, 0, sizeof(g));
    g.in_off = g.out_off = off; g.stride = stride; g.rows = rows; g.valid = valid;
    g.noise_off = noise_off; g.noise_len = N; g.noise_start = N - 1; g.noise_stride = noise_stride;
    g.flags = AFG_MIX_SNR; g.ratio = 1.0;
    return g;
}

static void groups_and_refusals()
{
    const uint32_t lengths[] = { 0, 1, 3, 255, 1024, 4095, 4096, 4097, 2 * 4096 + 5, 0xffffffffu };
    const uint32_t clips[] = { 1, 2, 3, 5, 63, 64, 4095, 4096, 4097, 0xffffffffu };
    std::vector<afg_mix_group> made;
    uint64_t at = 0, nat = 0, want_tiles = 0;
    for (uint32_t k = 0; k < sizeof lengths / sizeof lengths[0]; k++) {
        const uint32_t rows = k == 9 ? 65535 : 1 + k % 3;
        const bool per_row = k % 2 == 1;
        made.push_back(group_of(at, (uint64_t)lengths[k] + 5, rows, lengths[k], nat, clips[k], per_row ? (uint64_t)clips[k] + 1 : 0));
        at += (uint64_t)rows * ((uint64_t)lengths[k] + 5);
        nat += (per_row ? rows : 1) * ((uint64_t)clips[k] + 1);
        want_tiles += (((uint64_t)lengths[k] + 4095) / 4096) * rows;
    }
    const uint64_t n = made.size(), floats = at - 5, nfloats = nat - 1;      // the last gaps are not part of the planes
    afg_mix_group *heap = (afg_mix_group *)std::malloc(n * sizeof(afg_mix_group));               // exactly the records
    std::memcpy(heap, made.data(), n * sizeof(afg_mix_group));
    const uint64_t tiles = afg_mix_layout(heap, n);
    EXPECT(tiles == want_tiles && heap[0].first_tile == 0 && heap[1].first_tile == 0 && heap[2].first_tile == 2);
    EXPECT(afg_mix_layout(nullptr, n) == 0);
    // (more than 2^31 - 1 tiles: the launch's cap refuses what is otherwise in order)
    EXPECT(afg_mix_check_groups(heap, n, tiles, floats, nfloats, floats, nullptr) == AFG_ERR_INVALID);
    const uint64_t m = n - 1, t9 = heap[9].first_tile, f9 = heap[9].in_off - 5, nf9 = heap[9].noise_off - 1;     // without the giant
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, nullptr) == AFG_OK);
    EXPECT(afg_mix_check_groups(nullptr, 0, 0, 0, 0, 0, nullptr) == AFG_OK);
    EXPECT(afg_mix_check_groups(nullptr, 1, 0, 0, 0, 0, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9 - 1, nf9, f9, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9 - 1, f9, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9 - 1, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_mix_check_groups(heap, m, t9 + 1, f9, nf9, f9, nullptr) == AFG_ERR_INVALID);
    const uint64_t top = ~(uint64_t)0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 22; k++) {
        const afg_mix_group keep = heap[8], keep7 = heap[7];
        switch (k) {
        case 0: heap[8].in_off = top - 3; break;
        case 1: heap[8].out_off = top - 3; break;
        case 2: heap[8].noise_off = top - 3; break;
        case 3: heap[8].stride = top; break;
        case 4: heap[8].stride = top / 2 + 1; break;            // (rows - 1) * stride wraps to 0
        case 5: heap[8].stride = heap[8].valid - 1; break;
        case 6: heap[8].rows = 0; break;
        case 7: heap[8].rows = 65536; break;
        case 8: heap[8].first_tile += 1; break;
        case 9: heap[8].valid += 4096; break;                   // one more tile a row than the layout counted
        case 10: heap[8].flags = 2; break;
        case 11: heap[8].ratio = nan; break;
        case 12: heap[8].ratio = inf; break;
        case 13: heap[8].ratio = -1e-300; break;
        case 14: heap[8].flags = AFG_MIX_GAIN; heap[8].gain = -1.0f; break;
        case 15: heap[8].flags = AFG_MIX_GAIN; heap[8].gain = (float)inf; break;
        case 16: heap[8].noise_len = 0; break;
        case 17: heap[8].noise_start = heap[8].noise_len; break;
        case 18: heap[7].noise_stride = heap[7].noise_len - 1; break;     // (group 7 has a noise row per row)
        case 19: heap[7].noise_stride = top; break;
        case 20: heap[7].noise_stride = top / 2 + 1; break;
        default: heap[8].out_off = heap[7].out_off + 1; break;  // an output over another output
        }
        EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, nullptr) == AFG_ERR_INVALID);
        heap[8] = keep; heap[7] = keep7;
    }
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, nullptr) == AFG_OK);
    // planes in one address space: in place, apart, the output over the noise, an output over another group's input
    const uint64_t far = (uint64_t)1 << 60;
    const uint64_t in_place[3] = { far, 0, far }, apart[3] = { 0, far, 2 * far }, on_noise[3] = { 0, far, far + nf9 - 1 }, behind_noise[3] = { 0, far, far + nf9 };
    const uint64_t shifted[3] = { 0, far, 1 }, in_on_noise[3] = { far, far, 0 }, high[3] = { top / 4, 0, top / 4 };
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, in_place) == AFG_OK);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, apart) == AFG_OK);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, on_noise) == AFG_ERR_INVALID);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, behind_noise) == AFG_OK);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, shifted) == AFG_ERR_INVALID);
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, in_on_noise) == AFG_OK);               // inputs may meet the noise
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, high) == AFG_OK);                      // byte addresses near 2^64
    heap[0].in_off = heap[0].out_off = heap[0].noise_off = top;  // nothing of a group without floats is looked at but its mode, level and rows
    heap[0].noise_len = 0;
    heap[3].stride = 0;                                          // one row: the stride is not used
    heap[4].gain = (float)nan;                                   // the other mode's field is ignored
    heap[5].ratio = 0.0;
    EXPECT(afg_mix_check_groups(heap, m, t9, f9, nf9, f9, nullptr) == AFG_OK);
    // the giant alone: 65535 rows of 2^32 - 1 floats against a clip of 2^32 - 1 -- in order but for the tile cap
    afg_mix_group big = group_of(0, 0xffffffffull, 65535, 0xffffffffu, 0, 0xffffffffu, 0);
    const uint64_t big_tiles = afg_mix_layout(&big, 1), big_floats = 65535ull * 0xffffffffull;
    EXPECT(big_tiles == 65535ull << 20);
    EXPECT(afg_mix_check_groups(&big, 1, big_tiles, big_floats, 0xffffffffull, big_floats, nullptr) == AFG_ERR_INVALID);
    EXPECT(std::strstr(afg_last_error(), "2^31 - 1 tiles") != nullptr);
    big.rows = 1;                                                // 2^20 tiles: fine, at the last float of planes of 2^64 - 1
    big.in_off = big.out_off = top - 0xffffffffull; big.noise_off = top - 0xffffffffull;
    EXPECT(afg_mix_layout(&big, 1) == 1u << 20);
    EXPECT(afg_mix_check_groups(&big, 1, 1u << 20, top, top, top, nullptr) == AFG_OK);
    EXPECT(afg_mix_check_groups(&big, 1, 1u << 20, top - 1, top, top, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_mix_check_groups(&big, 1, 1u << 20, top, top - 1, top, nullptr) == AFG_ERR_INVALID);
    std::free(heap);
    EXPECT(afg_mix_ratio(0.0) == 1.0 && afg_mix_ratio(10.0) == 0.1 && afg_mix_ratio(-20.0) == 100.0 && afg_mix_ratio(inf) == 0.0);
    EXPECT(std::isinf(afg_mix_ratio(-1e6)) && std::isnan(afg_mix_ratio(nan)));
}

static void batch_refusals()
{
    const uint8_t byte = 0;
    const uint8_t *data[1] = { &byte };
    const size_t length[1] = { 1 };
    afg_resample_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o); o.channels = 2; o.frames = 1000; o.samplerate = 16000;
    uint32_t *lengths = (uint32_t *)std::malloc(2 * sizeof(uint32_t)), *index = (uint32_t *)std::malloc(sizeof(uint32_t));
    uint64_t *start = (uint64_t *)std::malloc(sizeof(uint64_t));
    double *snr = (double *)std::malloc(sizeof(double));
    lengths[0] = 100; lengths[1] = 1; index[0] = 1; start[0] = ~(uint64_t)0; snr[0] = 10.0;
    float *const d_out = (float *)(uintptr_t)0x10000, *const d_noise = (float *)(uintptr_t)0x100000;
    afg_batch_result res;
    const afg_mix_noise good = { d_noise, 2, 100, 2, lengths, index, start, snr };
    for (int k = 0; k < 14; k++) {
        afg_mix_noise b = good;
        const afg_mix_noise *pb = &b;
        float *out_plane = d_out;
        lengths[0] = 100; index[0] = 1; snr[0] = 10.0;
        switch (k) {
        case 0: pb = nullptr; break;
        case 1: b.d_noise = nullptr; break;
        case 2: b.snr_db = nullptr; break;
        case 3: b.d_noise = (const float *)(uintptr_t)0x100001; break;
        case 4: b.n_clips = 0; break;
        case 5: b.clip_pitch = 0; break;
        case 6: b.clip_rows = 3; break;                          // neither 1 nor the tensor's two channels
        case 7: b.n_clips = ~(uint64_t)0; b.lengths = nullptr; break;
        case 8: lengths[0] = 0; break;
        case 9: lengths[0] = 101; break;
        case 10: index[0] = 2; break;
        case 11: snr[0] = std::numeric_limits<double>::quiet_NaN(); break;
        case 12: snr[0] = -1e5; break;
        default: out_plane = (float *)((uintptr_t)d_noise + 4 * 399 - 4 * 1999); break;      // the tensor's last float on the bank's last
        }
        EXPECT(afg_batch_decode_mixed(data, length, 1, &o, pb, out_plane, nullptr, &res) == AFG_ERR_INVALID);
        EXPECT(res.n_files == 0 && res.items == nullptr);
    }
    lengths[0] = 100; index[0] = 1; snr[0] = 10.0;
    EXPECT(afg_batch_decode_mixed(data, length, 0, &o, &good, d_out, nullptr, &res) == AFG_OK);      // no file: nothing is touched
    std::free(lengths); std::free(index); std::free(start); std::free(snr);
}

int main()
{
    groups_and_refusals();
    batch_refusals();
    std::printf(failures ? "mix_host_check: %d FAILED\n" : "mix_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
