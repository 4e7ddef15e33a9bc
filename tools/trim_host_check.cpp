// trim_host_check.cpp -- the host-only half of the silence trim under AddressSanitizer and UndefinedBehaviorSanitizer:
// afg_trim_layout, the group and parameter checks of afg_trim_hip (afg_trim_check_groups) and the refusals of
// afg_batch_decode_trimmed, each at its extremes (valid = 0xffffffff, hop = 1, offsets near 2^64), with the records in heap
// buffers of exactly their size.  `make -C audio-formats_amd trim_host_check` compiles host/afg_trim.cpp with
// -fsanitize=address,undefined into this program (everything else comes from the library as it is) and runs it.  It needs
// no device and makes no device call.
#include "../include/afg.h"

#include <cmath>
#include <cstddef>
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

static afg_trim_params params_of(uint32_t frame_length, uint32_t hop, uint32_t reference = AFG_TRIM_REF_MAX)
{
    afg_trim_params p;
    std::memset(&p, 0, sizeof(p));
    p.frame_length = frame_length; p.hop = hop; p.reference = reference; p.ratio = 1e-6; p.abs_power = 1.0;
    return p;
}

static afg_trim_group group_of(uint64_t in_off, uint64_t out_off, uint32_t rows, uint32_t valid, uint32_t out_rows, uint32_t out_frames)
{
    afg_trim_group g;
    std::memset(&g, 0, sizeof(g));
    g.in_off = in_off; g.out_off = out_off; g.in_stride = (uint64_t)valid + 5; g.out_stride = (uint64_t)out_frames + 3;
    g.rows = rows; g.valid = valid; g.out_rows = out_rows; g.out_frames = out_frames;
    return g;
}

static void groups_and_refusals()
{
    const uint32_t lengths[] = { 0, 1, 511, 512, 513, 2047, 2049, 2 * 4096 + 5, 0xffffffffu };
    const uint32_t n_lengths = sizeof lengths / sizeof lengths[0];
    const afg_trim_params shapes[] = { params_of(2048, 512), params_of(1, 1), params_of(64, 1), params_of(65536, 1024, AFG_TRIM_REF_ABS),
                                       params_of(65536, 65536) };
    for (const afg_trim_params &p : shapes) {
        std::vector<afg_trim_group> made;
        uint64_t a = 0, b = 0, want_blocks = 0, want_tiles = 0, in_floats = 0, out_floats = 0;      // the planes end with their last float
        for (uint32_t k = 0; k < n_lengths; k++) {
            const uint32_t rows = k == n_lengths - 1 ? 65535 : 1 + k % 3, out_rows = rows + k % 2, out_frames = lengths[n_lengths - 1 - k];
            made.push_back(group_of(a, b, rows, lengths[k], out_rows, out_frames));
            if (lengths[k]) in_floats = a + (uint64_t)(rows - 1) * ((uint64_t)lengths[k] + 5) + lengths[k];
            if (out_frames) out_floats = b + (uint64_t)(out_rows - 1) * ((uint64_t)out_frames + 3) + out_frames;
            a += (uint64_t)rows * ((uint64_t)lengths[k] + 5);
            b += (uint64_t)out_rows * ((uint64_t)out_frames + 3);
            want_blocks += ((uint64_t)lengths[k] + p.hop - 1) / p.hop;
            want_tiles += (((uint64_t)out_frames + 4095) / 4096) * out_rows;
        }
        const uint64_t n = made.size();
        afg_trim_group *heap = (afg_trim_group *)std::malloc(n * sizeof(afg_trim_group));            // exactly the records
        std::memcpy(heap, made.data(), n * sizeof(afg_trim_group));
        uint64_t blocks = 7, tiles = 7;
        EXPECT(afg_trim_layout(heap, n, &p, &blocks, &tiles) == 1 && blocks == want_blocks && tiles == want_tiles);
        EXPECT(heap[0].first_block == 0 && heap[1].first_block == 0 && heap[2].first_block == 1 && heap[1].first_tile == heap[0].out_rows * ((uint64_t)1 << 20));
        EXPECT(afg_trim_check_groups(heap, n, blocks, tiles, &p, in_floats, out_floats) == AFG_OK);
        EXPECT(afg_trim_check_groups(nullptr, 0, 0, 0, &p, 0, 0) == AFG_OK);
        EXPECT(afg_trim_check_groups(heap, n, blocks, tiles, &p, in_floats - 1, out_floats) == AFG_ERR_INVALID);
        EXPECT(afg_trim_check_groups(heap, n, blocks, tiles, &p, in_floats, out_floats - 1) == AFG_ERR_INVALID);
        EXPECT(afg_trim_check_groups(heap, n, blocks + 1, tiles, &p, in_floats, out_floats) == AFG_ERR_INVALID);
        EXPECT(afg_trim_check_groups(heap, n, blocks, tiles - 1, &p, in_floats, out_floats) == AFG_ERR_INVALID);
        EXPECT(afg_trim_check_groups(nullptr, n, blocks, tiles, &p, in_floats, out_floats) == AFG_ERR_INVALID);
        const uint64_t top = ~(uint64_t)0;
        for (int k = 0; k < 12; k++) {
            const afg_trim_group keep = heap[7];
            switch (k) {
            case 0: heap[7].in_off = top - 3; break;
            case 1: heap[7].out_off = top - 3; break;
            case 2: heap[7].in_stride = top; break;
            case 3: heap[7].out_stride = top; break;
            case 4: heap[7].in_off = top; heap[7].in_stride = top; break;
            case 5: heap[7].in_stride = heap[7].valid - 1; break;
            case 6: heap[7].out_stride = heap[7].out_frames - 1; break;
            case 7: heap[7].rows = 0; break;
            case 8: heap[7].rows = 65536; heap[7].out_rows = 65536; break;
            case 9: heap[7].out_rows = heap[7].rows - 1; break;
            case 10: heap[7].first_block = top; break;
            case 11: heap[7].first_tile = top; break;
            }
            EXPECT(afg_trim_check_groups(heap, n, blocks, tiles, &p, in_floats, out_floats) == AFG_ERR_INVALID);
            EXPECT(std::strncmp(afg_last_error(), "afg_trim_group 7", 16) == 0);
            heap[7] = keep;
        }
        EXPECT(afg_trim_check_groups(heap, n, blocks, tiles, &p, in_floats, out_floats) == AFG_OK);
        // planes of 2^64 - 1 floats hold everything; a group at the very end of one
        EXPECT(afg_trim_check_groups(heap, n, blocks, tiles, &p, top, top) == AFG_OK);
        afg_trim_group last = group_of(top - 0xffffffffull, top - 7, 1, 0xffffffffu, 1, 7);
        uint64_t lb = 0, lt = 0;
        EXPECT(afg_trim_layout(&last, 1, &p, &lb, &lt) == 1 && lt == 1);
        EXPECT(afg_trim_check_groups(&last, 1, lb, lt, &p, top, top) == AFG_OK);
        last.in_off++;
        EXPECT(afg_trim_check_groups(&last, 1, lb, lt, &p, top, top) == AFG_ERR_INVALID);
        last.in_off--;
        last.out_off++;
        EXPECT(afg_trim_check_groups(&last, 1, lb, lt, &p, top, top) == AFG_ERR_INVALID);
        std::free(heap);
    }
    uint64_t nb = 0, nt = 0;
    const afg_trim_params good = params_of(2048, 512);
    EXPECT(afg_trim_layout(nullptr, 0, &good, &nb, &nt) == 1 && nb == 0 && nt == 0);
    EXPECT(afg_trim_layout(nullptr, 3, &good, &nb, &nt) == 0);
    EXPECT(afg_trim_layout(nullptr, 0, nullptr, &nb, &nt) == 0);
    EXPECT(afg_trim_layout(nullptr, 0, &good, nullptr, &nt) == 0 && afg_trim_layout(nullptr, 0, &good, &nb, nullptr) == 0);
}

static void parameters()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (uint32_t k : { 1u, 2u, 4u, 62u, 64u }) {
        const afg_trim_params p = params_of(k * 1024 > 65536 ? k * 4 : k * 1024, k * 1024 > 65536 ? 4 : 1024);
        EXPECT(afg_trim_check_groups(nullptr, 0, 0, 0, &p, 0, 0) == AFG_OK);
    }
    std::vector<afg_trim_params> bad;
    bad.push_back(params_of(2048, 0));
    bad.push_back(params_of(0, 512));
    bad.push_back(params_of(65537, 1));
    bad.push_back(params_of(0xffffffffu, 0xffffffffu));
    bad.push_back(params_of(2048, 500));
    bad.push_back(params_of(3 * 512, 512));
    bad.push_back(params_of(66, 1));
    bad.push_back(params_of(2048, 512, 2));
    for (double r : { 0.0, -1.0, inf, nan, 1.0000001 }) { bad.push_back(params_of(2048, 512)); bad.back().ratio = r; }
    for (double a : { 0.0, -1.0, inf, nan }) { bad.push_back(params_of(2048, 512, AFG_TRIM_REF_ABS)); bad.back().abs_power = a; }
    for (int k = 0; k < 3; k++) { bad.push_back(params_of(2048, 512)); bad.back().reserved[k] = 1; }
    for (const afg_trim_params &p : bad) {
        uint64_t nb = 0, nt = 0;
        EXPECT(afg_trim_check_groups(nullptr, 0, 0, 0, &p, 0, 0) == AFG_ERR_INVALID);
        EXPECT(std::strncmp(afg_last_error(), "afg_trim_params.", 16) == 0);
        EXPECT(afg_trim_layout(nullptr, 0, &p, &nb, &nt) == 0);
        EXPECT(afg_trim_hip(0, nullptr, 0, 0, &p, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) == AFG_ERR_INVALID);
    }
    afg_trim_params p = params_of(2048, 512, AFG_TRIM_REF_ABS);
    p.ratio = 7.0;                                               // above 1 over an absolute reference is allowed
    EXPECT(afg_trim_check_groups(nullptr, 0, 0, 0, &p, 0, 0) == AFG_OK);
    p = params_of(2048, 512);
    p.abs_power = nan;                                           // ignored with AFG_TRIM_REF_MAX
    p.lead = p.trail = 0xffffffffu;
    EXPECT(afg_trim_check_groups(nullptr, 0, 0, 0, &p, 0, 0) == AFG_OK);
    EXPECT(afg_trim_check_groups(nullptr, 0, 0, 0, nullptr, 0, 0) == AFG_ERR_INVALID);
}

static void batch_entry()
{
    const uint8_t byte = 0;
    const uint8_t *data[1] = { &byte };
    const size_t length[1] = { 1 };
    afg_resample_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o); o.channels = 1; o.frames = 16000; o.samplerate = 16000;
    const afg_trim_params p = params_of(2048, 512);
    afg_trim_region region;
    afg_batch_result res;
    float *const d_out = (float *)(uintptr_t)0x1000;             // never touched: every call below is refused, or has no file
    EXPECT(afg_batch_decode_trimmed(data, length, 1, nullptr, &p, 0, d_out, &region, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &o, nullptr, 0, d_out, &region, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &o, &p, 0, nullptr, &region, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &o, &p, 0, d_out, &region, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &o, &p, 15999, d_out, &region, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &o, &p, 1, d_out, nullptr, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_trimmed(data, length, -1, &o, &p, 0, d_out, &region, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_trimmed(nullptr, nullptr, 1, &o, &p, 0, d_out, &region, &res) == AFG_ERR_INVALID);
    afg_resample_opts up = o;                                    // the scratch row of the longest scan from the highest rate
    up.samplerate = 8000;
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &up, &p, 0xffffffffu, d_out, &region, &res) == AFG_ERR_INVALID);
    afg_resample_opts small = o;
    small.struct_size = (uint32_t)offsetof(afg_resample_opts, lowpass_width);
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &small, &p, 0, d_out, &region, &res) == AFG_ERR_INVALID);
    const int64_t neg = -1;
    afg_resample_opts early = o;
    early.first_frame = &neg;
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &early, &p, 0, d_out, &region, &res) == AFG_ERR_INVALID);
    const afg_trim_params odd = params_of(2048, 500);
    EXPECT(afg_batch_decode_trimmed(data, length, 1, &o, &odd, 0, d_out, &region, &res) == AFG_ERR_INVALID);
    EXPECT(res.n_files == 0 && res.items == nullptr && res.owner == nullptr);
    // no file: nothing is touched, whatever the scan
    for (uint32_t scan : { 0u, 16000u, 64000u }) {
        EXPECT(afg_batch_decode_trimmed(nullptr, nullptr, 0, &o, &p, scan, d_out, nullptr, &res) == AFG_OK);
        EXPECT(res.n_files == 0 && res.items == nullptr);
    }
}

int main()
{
    groups_and_refusals();
    parameters();
    batch_entry();
    if (failures) { std::fprintf(stderr, "trim_host_check: %d failure(s)\n", failures); return 1; }
    std::printf("trim_host_check: ok\n");
    return 0;
}
