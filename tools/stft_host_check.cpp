// stft_host_check.cpp -- the host-only half of the linear spectrogram stage under AddressSanitizer and
// UndefinedBehaviorSanitizer: afg_stft_tile_frames, afg_stft_layout, the record and parameter checks of afg_stft_hip
// (afg_stft_check_rows) and the refusals of afg_batch_decode_stft, each at its extremes (rows of 2^32 - 1 samples, offsets
// near 2^64), with the records in heap buffers of exactly their size.  `make -C audio-formats_amd stft_host_check` compiles
// the host side of csrc/stft.hip and host/afg_stft.cpp with -fsanitize=address,undefined into this program (everything else
// comes from the library as it is) and runs it.  It needs no device and makes no device call.
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

static afg_stft_params params_of(uint32_t n_fft, uint32_t win, uint32_t hop, uint32_t center, uint32_t kind, uint32_t pad_mode = AFG_MEL_PAD_REFLECT)
{
    afg_stft_params p;
    std::memset(&p, 0, sizeof(p));
    p.n_fft = n_fft; p.win_length = win; p.hop = hop; p.center = center; p.pad_mode = pad_mode; p.out_kind = kind;
    return p;
}

static uint32_t frames_of(const afg_stft_params &p, uint32_t in_frames)
{
    const int64_t num = (int64_t)in_frames + 2 * (int64_t)(p.center ? p.n_fft / 2 : 0) - (int64_t)p.n_fft;
    return num < 0 ? 0 : (uint32_t)(1 + num / (int64_t)p.hop);
}

static void records_and_refusals()
{
    const uint32_t lengths[] = { 0, 1025, 2048, 2049, 4000, 48000, 480000, 0xffffffffu };
    const uint32_t n_lengths = sizeof lengths / sizeof lengths[0];
    for (uint32_t kind = AFG_STFT_COMPLEX; kind <= AFG_STFT_LOG10; kind++) {
        const afg_stft_params shapes[] = { params_of(400, 400, 160, 1, kind), params_of(16, 1, 1, 1, kind, AFG_MEL_PAD_ZERO), params_of(75, 75, 25, 0, kind),
                                           params_of(1024, 1000, 256, 1, kind), params_of(2048, 2048, 2048, 0, kind), params_of(2048, 2048, 1, 1, kind),
                                           params_of(1875, 1875, 625, 1, kind), params_of(2025, 2000, 2025, 0, kind) };   // (two transforming wavefronts)
        for (const afg_stft_params &p : shapes) {
            const uint32_t tile = afg_stft_tile_frames(&p), comps = kind == AFG_STFT_COMPLEX ? 2 : 1, n_bins = p.n_fft / 2 + 1;
            EXPECT(tile == 64 / comps || tile == 32 / comps || tile == 16 / comps);
            const uint64_t table = (uint64_t)p.win_length + 2 * (uint64_t)p.n_fft;
            std::vector<afg_mel_row> made;
            uint64_t a = 3, b = 5, want = 0;
            for (uint32_t k = 0; k < n_lengths; k++) {
                afg_mel_row r;
                std::memset(&r, 0, sizeof(r));
                r.in_off = a; r.out_off = b; r.in_frames = lengths[k];
                r.out_frames = frames_of(p, lengths[k]) - (k % 2 && frames_of(p, lengths[k]) ? 1 : 0);
                if (p.pad_mode == AFG_MEL_PAD_REFLECT && p.center && lengths[k] <= p.n_fft / 2) r.out_frames = 0;
                made.push_back(r);
                a += lengths[k];
                b += (uint64_t)comps * n_bins * r.out_frames;
                want += ((uint64_t)r.out_frames + tile - 1) / tile;
            }
            const uint64_t n = made.size();
            afg_mel_row *heap = (afg_mel_row *)std::malloc(n * sizeof(afg_mel_row));                // exactly the records
            std::memcpy(heap, made.data(), n * sizeof(afg_mel_row));
            const uint64_t tiles = afg_stft_layout(heap, n, &p);
            EXPECT(tiles == want && heap[0].first_tile == 0 && heap[n - 1].first_tile + ((uint64_t)heap[n - 1].out_frames + tile - 1) / tile == tiles);
            EXPECT(afg_stft_check_rows(heap, n, tiles, &p, a, table, b) == AFG_OK);
            EXPECT(afg_stft_check_rows(nullptr, 0, 0, &p, 0, 0, 0) == AFG_OK);
            EXPECT(afg_stft_check_rows(nullptr, n, tiles, &p, a, table, b) == AFG_ERR_INVALID);
            EXPECT(afg_stft_check_rows(heap, n, tiles, &p, a - 1, table, b) == AFG_ERR_INVALID);
            EXPECT(afg_stft_check_rows(heap, n, tiles, &p, a, table, b - 1) == AFG_ERR_INVALID);
            EXPECT(afg_stft_check_rows(heap, n, tiles, &p, a, table - 1, b) == AFG_ERR_INVALID);
            EXPECT(afg_stft_check_rows(heap, n, tiles + 1, &p, a, table, b) == AFG_ERR_INVALID);
            const uint64_t top = ~(uint64_t)0;
            for (int k = 0; k < 6; k++) {
                const afg_mel_row keep = heap[4];
                switch (k) {
                case 0: heap[4].in_off = top - 3; break;
                case 1: heap[4].out_off = top - 3; break;
                case 2: heap[4].first_tile += 1; break;
                case 3: heap[4].out_frames = frames_of(p, heap[4].in_frames) + 1; break;
                case 4: heap[4].out_frames = 0xffffffffu; break;
                default: heap[4].in_frames = 1; break;                 // too few samples for its frames
                }
                EXPECT(afg_stft_check_rows(heap, n, tiles, &p, a, table, b) == AFG_ERR_INVALID);
                heap[4] = keep;
            }
            EXPECT(afg_stft_check_rows(heap, n, tiles, &p, a, table, b) == AFG_OK);
            // a kernel entry with made-up device addresses stops at the parameters or the arguments
            afg_stft_params bad = p;
            bad.reserved = 1;
            EXPECT(afg_stft_hip(n, (const afg_mel_row *)0x1000, tiles, &bad, (const float *)0x2000, a, (const float *)0x3000, table, (float *)0x4000, b, nullptr) == AFG_ERR_INVALID);
            EXPECT(afg_stft_hip(n, nullptr, tiles, &p, (const float *)0x2000, a, (const float *)0x3000, table, (float *)0x4000, b, nullptr) == AFG_ERR_INVALID);
            EXPECT(afg_stft_hip(0, nullptr, 0, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == AFG_OK);
            std::free(heap);
        }
    }
}

static void parameters()
{
    const afg_stft_params good = params_of(400, 400, 160, 1, AFG_STFT_POWER);
    EXPECT(afg_stft_tile_frames(&good) == 64 && afg_stft_layout(nullptr, 0, &good) == 0);
    EXPECT(afg_stft_tile_frames(nullptr) == 0 && afg_stft_layout(nullptr, 0, nullptr) == 0);
    for (uint32_t n_fft : { 0u, 15u, 17u, 2049u, 14u * 3u * 5u, 0xffffffffu }) {
        afg_stft_params p = good;
        p.n_fft = n_fft;
        EXPECT(afg_stft_tile_frames(&p) == 0 && afg_stft_layout(nullptr, 0, &p) == 0);
        EXPECT(afg_stft_check_rows(nullptr, 0, 0, &p, 0, 0, 0) == AFG_ERR_UNSUPPORTED);
    }
    for (int k = 0; k < 12; k++) {
        afg_stft_params p = good;
        switch (k) {
        case 0: p.win_length = 0; break;
        case 1: p.win_length = 401; break;
        case 2: p.hop = 0; break;
        case 3: p.hop = 401; break;
        case 4: p.center = 2; break;
        case 5: p.pad_mode = 2; break;
        case 6: p.out_kind = 4; break;
        case 7: p.log_floor = -1.0f; break;
        case 8: p.log_floor = std::numeric_limits<float>::quiet_NaN(); break;
        case 9: p.log_floor = std::numeric_limits<float>::infinity(); break;
        case 10: p.reserved = 1; break;
        default: p.out_kind = 0xffffffffu; break;
        }
        EXPECT(afg_stft_tile_frames(&p) == 0);
        EXPECT(afg_stft_check_rows(nullptr, 0, 0, &p, 0, 0, 0) == AFG_ERR_INVALID);
    }
}

static void batch_refusals()
{
    const uint8_t byte = 'x';
    const uint8_t *data[1] = { &byte };
    const size_t length[1] = { 1 };
    afg_stft_opts good;
    std::memset(&good, 0, sizeof(good));
    good.struct_size = (uint32_t)sizeof(good); good.n_threads = 1; good.channels = 1; good.frames = 16000; good.samplerate = 16000; good.mono = 1;
    good.stft = params_of(400, 400, 160, 1, AFG_STFT_POWER);
    afg_batch_result res;
    float *const fake = (float *)0x1000;
    EXPECT(afg_batch_decode_stft(data, length, 0, &good, fake, &res) == AFG_OK && res.n_files == 0 && res.items == nullptr);
    for (int k = 0; k < 9; k++) {
        afg_stft_opts o = good;
        int want = AFG_ERR_INVALID;
        switch (k) {
        case 0: o.struct_size -= 4; break;
        case 1: o.reserved = 1; break;
        case 2: o.n_out = 102; break;                            // 16000 samples have 101 frames
        case 3: o.frames = 200; break;                           // reflect with T <= pad
        case 4: o.stft.n_fft = 14 * 3 * 5; o.stft.win_length = 16; o.stft.hop = 16; want = AFG_ERR_UNSUPPORTED; break;
        case 5: o.stft.center = 0; o.frames = 399; break;        // no frame
        case 6: o.stft.reserved = 7; break;
        case 7: o.channels = 0; break;
        default: o.stft.out_kind = 4; break;
        }
        EXPECT(afg_batch_decode_stft(data, length, 1, &o, fake, &res) == want && res.n_files == 0 && res.items == nullptr);
    }
    EXPECT(afg_batch_decode_stft(data, length, 1, nullptr, fake, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_stft(data, length, 1, &good, nullptr, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_stft(data, length, 1, &good, fake, nullptr) == AFG_ERR_INVALID);
}

int main()
{
    records_and_refusals();
    parameters();
    batch_refusals();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("stft_host_check: ok\n");
    return 0;
}
