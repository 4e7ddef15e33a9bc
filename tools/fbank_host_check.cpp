// fbank_host_check.cpp -- the host-only half of the Kaldi-compatible filter-bank stage under AddressSanitizer and
// UndefinedBehaviorSanitizer: afg_fbank_n_fft, afg_fbank_frames, the tables and the bank into heap buffers of exactly their
// size, afg_fbank_layout, the record and parameter checks of afg_fbank_hip (afg_fbank_check_rows) on hostile records (rows of
// 2^32 - 1 samples, offsets near 2^64) and the refusals of afg_batch_decode_fbank.  `make -C audio-formats_amd
// fbank_host_check` compiles the host side of csrc/fbank.hip and host/afg_fbank.cpp with -fsanitize=address,undefined into
// this program (everything else comes from the library as it is) and runs it.  It needs no device and makes no device call.
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

static afg_fbank_params params_of(uint32_t win, uint32_t hop, uint32_t n_fft, uint32_t n_mels, uint32_t snip, uint32_t energy, uint32_t layout)
{
    afg_fbank_params p;
    std::memset(&p, 0, sizeof(p));
    p.win_length = win; p.hop = hop; p.n_fft = n_fft; p.n_mels = n_mels; p.snip_edges = snip; p.remove_dc = 1; p.use_power = 1; p.use_log = 1;
    p.use_energy = energy; p.raw_energy = 1; p.layout = layout; p.preemph = 0.97f;
    return p;
}

static uint32_t frames_of(const afg_fbank_params &p, uint32_t n)
{
    if (p.snip_edges) return n < p.win_length ? 0 : 1 + (n - p.win_length) / p.hop;
    return (uint32_t)(((uint64_t)n + p.hop / 2) / p.hop);
}

static void helpers()
{
    EXPECT(afg_fbank_n_fft(400, 1) == 512 && afg_fbank_n_fft(400, 0) == 400 && afg_fbank_n_fft(2, 1) == 2 && afg_fbank_n_fft(2048, 1) == 2048);
    EXPECT(afg_fbank_n_fft(1025, 1) == 2048 && afg_fbank_n_fft(1, 1) == 0 && afg_fbank_n_fft(2049, 0) == 0 && afg_fbank_n_fft(0xffffffffu, 1) == 0);
    for (uint32_t wt = AFG_FBANK_WINDOW_POVEY; wt <= AFG_FBANK_WINDOW_RECTANGULAR; wt++)
        for (uint32_t win : { 2u, 25u, 400u, 2048u }) {
            const uint32_t n_fft = afg_fbank_n_fft(win, 1) < 16 ? 16 : afg_fbank_n_fft(win, 1);
            const uint64_t need = afg_fbank_tables(wt, win, n_fft, 0.42, nullptr, 0);
            EXPECT(need == (uint64_t)win + 2 * (uint64_t)n_fft);
            float *t = (float *)std::malloc(need * sizeof(float));                           // exactly the table
            EXPECT(afg_fbank_tables(wt, win, n_fft, 0.42, t, need) == need);
            EXPECT(afg_fbank_tables(wt, win, n_fft, 0.42, t, need - 1) == need);             // too small: left alone
            for (uint32_t j = 0; j < win; j++) EXPECT(t[j] >= -1e-6f && t[j] <= 1.0f && std::fabs(t[j] - t[win - 1 - j]) <= 1e-6f);
            EXPECT(t[win] == 1.0f && t[win + 1] == 0.0f);
            std::free(t);
        }
    EXPECT(afg_fbank_tables(5, 400, 512, 0.42, nullptr, 0) == 0 && afg_fbank_tables(0, 1, 16, 0.42, nullptr, 0) == 0);
    EXPECT(afg_fbank_tables(0, 400, 399, 0.42, nullptr, 0) == 0 && afg_fbank_tables(0, 1102, 1102, 0.42, nullptr, 0) == 0);
    EXPECT(afg_fbank_tables(3, 400, 512, std::numeric_limits<double>::quiet_NaN(), nullptr, 0) == 0);
    for (uint32_t n_fft : { 16u, 400u, 405u, 512u, 2048u })
        for (uint32_t n_mels : { 1u, 23u, 256u }) {
            const uint64_t need = afg_fbank_filters(16000, n_fft, n_mels, 20.0, -400.0, nullptr, 0), n_bins = n_fft / 2 + 1;
            EXPECT(need == n_mels * n_bins);
            float *w = (float *)std::malloc(need * sizeof(float));                           // exactly the bank
            EXPECT(afg_fbank_filters(16000, n_fft, n_mels, 20.0, -400.0, w, need) == need);
            for (uint64_t i = 0; i < need; i++) EXPECT(w[i] >= 0.0f && w[i] <= 1.0f);
            if (n_fft % 2 == 0)
                for (uint32_t m = 0; m < n_mels; m++) EXPECT(w[m * n_bins + n_fft / 2] == 0.0f && !std::signbit(w[m * n_bins + n_fft / 2]));
            std::free(w);
        }
    EXPECT(afg_fbank_filters(0, 512, 23, 20.0, 0.0, nullptr, 0) == 0 && afg_fbank_filters(16000, 512, 0, 20.0, 0.0, nullptr, 0) == 0);
    EXPECT(afg_fbank_filters(16000, 512, 23, 20.0, 8001.0, nullptr, 0) == 0 && afg_fbank_filters(16000, 512, 23, 9000.0, 0.0, nullptr, 0) == 0);
    EXPECT(afg_fbank_filters(16000, 512, 23, std::numeric_limits<double>::quiet_NaN(), 0.0, nullptr, 0) == 0);
    EXPECT(afg_fbank_filters(16000, 512, 23, 20.0, -std::numeric_limits<double>::infinity(), nullptr, 0) == 0);
}

static void records_and_refusals()
{
    const uint32_t lengths[] = { 0, 1, 399, 400, 2049, 4000, 480000, 0xffffffffu };
    const uint32_t n_lengths = sizeof lengths / sizeof lengths[0];
    for (uint32_t layout = AFG_FBANK_FRAMES_MAJOR; layout <= AFG_FBANK_MEL_MAJOR; layout++) {
        const afg_fbank_params shapes[] = { params_of(400, 160, 512, 80, 1, 0, layout), params_of(400, 160, 512, 23, 0, 1, layout),
                                            params_of(64, 100, 64, 17, 0, 1, layout), params_of(2, 1, 16, 1, 1, 0, layout),
                                            params_of(2048, 65535, 2048, 256, 0, 1, layout), params_of(2025, 1, 2025, 256, 1, 1, layout) };
        for (const afg_fbank_params &p : shapes) {
            const uint64_t table = (uint64_t)p.win_length + 2 * (uint64_t)p.n_fft, bank = (uint64_t)p.n_mels * (p.n_fft / 2 + 1), cols = p.n_mels + p.use_energy;
            std::vector<afg_mel_row> made;
            uint64_t a = 3, b = 5, want = 0;
            for (uint32_t k = 0; k < n_lengths; k++) {
                afg_mel_row r;
                std::memset(&r, 0, sizeof(r));
                r.in_off = a; r.out_off = b; r.in_frames = lengths[k];
                EXPECT(afg_fbank_frames(&p, lengths[k]) == frames_of(p, lengths[k]));
                r.out_frames = frames_of(p, lengths[k]) - (k % 2 && frames_of(p, lengths[k]) ? 1 : 0);
                made.push_back(r);
                a += lengths[k];
                b += cols * r.out_frames;
                want += ((uint64_t)r.out_frames + 15) / 16;
            }
            const uint64_t n = made.size();
            afg_mel_row *heap = (afg_mel_row *)std::malloc(n * sizeof(afg_mel_row));                // exactly the records
            std::memcpy(heap, made.data(), n * sizeof(afg_mel_row));
            const uint64_t tiles = afg_fbank_layout(heap, n, &p);
            EXPECT(tiles == want && heap[0].first_tile == 0 && heap[n - 1].first_tile + ((uint64_t)heap[n - 1].out_frames + 15) / 16 == tiles);
            EXPECT(afg_fbank_check_rows(heap, n, tiles, &p, a, table, bank, b) == AFG_OK);
            EXPECT(afg_fbank_check_rows(nullptr, 0, 0, &p, 0, 0, 0, 0) == AFG_OK);
            EXPECT(afg_fbank_check_rows(nullptr, n, tiles, &p, a, table, bank, b) == AFG_ERR_INVALID);
            EXPECT(afg_fbank_check_rows(heap, n, tiles, &p, a - 1, table, bank, b) == AFG_ERR_INVALID);
            EXPECT(afg_fbank_check_rows(heap, n, tiles, &p, a, table, bank, b - 1) == AFG_ERR_INVALID);
            EXPECT(afg_fbank_check_rows(heap, n, tiles, &p, a, table - 1, bank, b) == AFG_ERR_INVALID);
            EXPECT(afg_fbank_check_rows(heap, n, tiles, &p, a, table, bank - 1, b) == AFG_ERR_INVALID);
            EXPECT(afg_fbank_check_rows(heap, n, tiles + 1, &p, a, table, bank, b) == AFG_ERR_INVALID);
            const uint64_t top = ~(uint64_t)0;
            for (int k = 0; k < 6; k++) {
                const afg_mel_row keep = heap[6];
                switch (k) {
                case 0: heap[6].in_off = top - 3; break;
                case 1: heap[6].out_off = top - 3; break;
                case 2: heap[6].first_tile += 1; break;
                case 3: heap[6].out_frames = frames_of(p, heap[6].in_frames) + 1; break;
                case 4: heap[6].out_frames = 0xffffffffu; break;
                default: heap[6].in_frames = 0; break;                 // no samples, no frames
                }
                EXPECT(afg_fbank_check_rows(heap, n, tiles, &p, a, table, bank, b) == AFG_ERR_INVALID);
                heap[6] = keep;
            }
            EXPECT(afg_fbank_check_rows(heap, n, tiles, &p, a, table, bank, b) == AFG_OK);
            // a kernel entry with made-up device addresses stops at the parameters or the arguments
            afg_fbank_params bad = p;
            bad.reserved = 1;
            EXPECT(afg_fbank_hip(n, (const afg_mel_row *)0x1000, tiles, &bad, (const float *)0x2000, a, (const float *)0x3000, table, (const float *)0x4000, bank,
                                 (float *)0x5000, b, nullptr) == AFG_ERR_INVALID);
            EXPECT(afg_fbank_hip(n, nullptr, tiles, &p, (const float *)0x2000, a, (const float *)0x3000, table, (const float *)0x4000, bank, (float *)0x5000, b,
                                 nullptr) == AFG_ERR_INVALID);
            EXPECT(afg_fbank_hip(0, nullptr, 0, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == AFG_OK);
            std::free(heap);
        }
    }
}

static void parameters()
{
    const afg_fbank_params good = params_of(400, 160, 512, 23, 1, 1, AFG_FBANK_FRAMES_MAJOR);
    EXPECT(afg_fbank_frames(&good, 16000) == 98 && afg_fbank_layout(nullptr, 0, &good) == 0);
    EXPECT(afg_fbank_frames(nullptr, 16000) == 0 && afg_fbank_layout(nullptr, 0, nullptr) == 0);
    EXPECT(afg_fbank_check_rows(nullptr, 0, 0, nullptr, 0, 0, 0, 0) == AFG_ERR_INVALID);
    for (uint32_t n_fft : { 14u * 3u * 5u * 2u, 1102u, 401u }) {
        afg_fbank_params p = good;
        p.n_fft = n_fft;
        EXPECT(afg_fbank_frames(&p, 16000) == 0 && afg_fbank_check_rows(nullptr, 0, 0, &p, 0, 0, 0, 0) == AFG_ERR_UNSUPPORTED);
    }
    for (int k = 0; k < 24; k++) {
        afg_fbank_params p = good;
        switch (k) {
        case 0: p.win_length = 1; break;
        case 1: p.win_length = 2049; break;
        case 2: p.hop = 0; break;
        case 3: p.hop = 65536; break;
        case 4: p.n_fft = 399; break;
        case 5: p.n_fft = 2049; break;
        case 6: p.n_mels = 0; break;
        case 7: p.n_mels = 257; break;
        case 8: p.snip_edges = 2; break;
        case 9: p.remove_dc = 2; break;
        case 10: p.use_power = 2; break;
        case 11: p.use_log = 0xffffffffu; break;
        case 12: p.use_energy = 2; break;
        case 13: p.raw_energy = 2; break;
        case 14: p.htk_compat = 2; break;
        case 15: p.layout = 2; break;
        case 16: p.preemph = -0.5f; break;
        case 17: p.preemph = 1.0001f; break;
        case 18: p.preemph = std::numeric_limits<float>::quiet_NaN(); break;
        case 19: p.energy_floor = -1.0f; break;
        case 20: p.energy_floor = std::numeric_limits<float>::infinity(); break;
        case 21: p.scale = -32768.0f; break;
        case 22: p.scale = std::numeric_limits<float>::quiet_NaN(); break;
        default: p.reserved = 1; break;
        }
        EXPECT(afg_fbank_frames(&p, 16000) == 0 && afg_fbank_layout(nullptr, 0, &p) == 0);
        EXPECT(afg_fbank_check_rows(nullptr, 0, 0, &p, 0, 0, 0, 0) == AFG_ERR_INVALID);
    }
}

static void batch_refusals()
{
    const uint8_t byte = 'x';
    const uint8_t *data[1] = { &byte };
    const size_t length[1] = { 1 };
    afg_fbank_opts good;
    std::memset(&good, 0, sizeof(good));
    good.struct_size = (uint32_t)sizeof(good); good.n_threads = 1; good.channels = 1; good.frames = 16000; good.samplerate = 16000; good.mono = 1;
    good.fbank = params_of(400, 160, 512, 23, 1, 1, AFG_FBANK_FRAMES_MAJOR);
    good.low_freq = 20.0; good.blackman_coeff = 0.42;
    afg_batch_result res;
    uint32_t counts[1] = { 77 };
    float *const fake = (float *)0x1000;
    EXPECT(afg_batch_decode_fbank(data, length, 0, &good, fake, counts, &res) == AFG_OK && res.n_files == 0 && res.items == nullptr);
    EXPECT(afg_batch_decode_fbank(data, length, 0, &good, fake, nullptr, &res) == AFG_OK);
    for (int k = 0; k < 11; k++) {
        afg_fbank_opts o = good;
        int want = AFG_ERR_INVALID;
        switch (k) {
        case 0: o.struct_size -= 4; break;
        case 1: o.reserved = 1; break;
        case 2: o.n_out = 99; break;                             // 16000 samples have 98 frames
        case 3: o.frames = 399; break;                           // no frame
        case 4: o.fbank.win_length = 1102; o.fbank.hop = 441; o.fbank.n_fft = 1102; want = AFG_ERR_UNSUPPORTED; break;
        case 5: o.fbank.reserved = 7; break;
        case 6: o.channels = 0; break;
        case 7: o.window_type = 5; break;
        case 8: o.low_freq = 8000.0; break;
        case 9: o.high_freq = 8000.5; break;
        default: o.blackman_coeff = std::numeric_limits<double>::infinity(); break;
        }
        EXPECT(afg_batch_decode_fbank(data, length, 1, &o, fake, counts, &res) == want && res.n_files == 0 && res.items == nullptr);
    }
    EXPECT(afg_batch_decode_fbank(data, length, 1, nullptr, fake, counts, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_fbank(data, length, 1, &good, nullptr, counts, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_fbank(data, length, 1, &good, fake, counts, nullptr) == AFG_ERR_INVALID);
    EXPECT(counts[0] == 77);
}

int main()
{
    helpers();
    records_and_refusals();
    parameters();
    batch_refusals();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("fbank_host_check: ok\n");
    return 0;
}
