// melspec_host_check.cpp -- the host-only half of the mel spectrogram stage under AddressSanitizer and
// UndefinedBehaviorSanitizer: afg_mel_basis, afg_mel_filters, afg_mel_frames, afg_mel_layout and the record checks of
// afg_melspec_hip (afg_mel_check_rows), over the shapes the GPU tests use and over every refusal, with every table in a
// heap buffer of exactly the size the entry asks for; and the same of the FFT path: afg_mel_fft_tables, afg_mel_fft_layout,
// afg_mel_fft_check_rows.  `make -C audio-formats_amd melspec_host_check` compiles the host side of csrc/melspec.hip and
// csrc/melspec_fft.hip and host/afg_melspec.cpp with -fsanitize=address,undefined into this program (everything else
// comes from the library as it is) and runs it.  It needs no device and makes no device call.
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

struct Shape { uint32_t n_fft, win, hop, n_mels, center; };

static afg_mel_params params_of(const Shape &s, uint32_t pad_mode)
{
    afg_mel_params p;
    std::memset(&p, 0, sizeof(p));
    p.n_fft = s.n_fft; p.win_length = s.win; p.hop = s.hop; p.n_mels = s.n_mels; p.center = s.center;
    p.pad_mode = pad_mode; p.out_kind = AFG_MEL_LOG10;
    return p;
}

static void shape(const Shape &s)
{
    // the tables, each in a buffer of exactly its size (and one float short: untouched)
    const uint64_t nb = afg_mel_basis(s.n_fft, s.win, nullptr, 0);
    EXPECT(nb == (uint64_t)s.win * 2 * ((s.n_fft / 2 + 1 + 15) / 16 * 16));
    float *basis = (float *)std::malloc((size_t)nb * sizeof(float));
    EXPECT(afg_mel_basis(s.n_fft, s.win, basis, nb) == nb);
    float *shorter = (float *)std::malloc((size_t)(nb - 1) * sizeof(float));
    EXPECT(afg_mel_basis(s.n_fft, s.win, shorter, nb - 1) == nb);
    std::free(shorter);
    std::free(basis);
    for (uint32_t scale = 0; scale < 2; scale++)
        for (uint32_t norm = 0; norm < 2; norm++) {
            const uint64_t nf = afg_mel_filters(16000, s.n_fft, s.n_mels, 0.0, 0.0, scale, norm, nullptr, 0);
            EXPECT(nf == (uint64_t)s.n_mels * (s.n_fft / 2 + 1));
            float *bank = (float *)std::malloc((size_t)nf * sizeof(float));
            EXPECT(afg_mel_filters(16000, s.n_fft, s.n_mels, 20.0, 7000.0, scale, norm, bank, nf) == nf);
            std::free(bank);
        }
    const uint64_t bank_floats = (uint64_t)s.n_mels * (s.n_fft / 2 + 1);
    for (uint32_t pad_mode = 0; pad_mode < 2; pad_mode++) {
        const afg_mel_params p = params_of(s, pad_mode);
        const uint32_t pad = s.center ? s.n_fft / 2 : 0;
        // the rows of tests/test_melspec_gpu.py, and the 2^32 - 1 samples a record can name
        const uint32_t lengths[] = { 3 * s.n_fft + 5, pad + 1 > (s.center ? 0 : s.n_fft) ? pad + 1 : s.n_fft, 64 * s.hop + s.n_fft - 2 * pad, 0,
                                     5 * s.hop + s.n_fft, 0xffffffffu };
        std::vector<afg_mel_row> rows;
        uint64_t in_at = 0, out_at = 0;
        for (uint32_t n : lengths) {
            afg_mel_row r;
            std::memset(&r, 0, sizeof(r));
            r.in_off = in_at; r.out_off = out_at; r.in_frames = n;
            r.out_frames = afg_mel_frames(&p, n);
            if (pad_mode == AFG_MEL_PAD_REFLECT && n <= pad) r.out_frames = 0;
            in_at += n; out_at += (uint64_t)s.n_mels * r.out_frames;
            rows.push_back(r);
        }
        afg_mel_row *heap = (afg_mel_row *)std::malloc(rows.size() * sizeof(afg_mel_row));       // exactly the records
        std::memcpy(heap, rows.data(), rows.size() * sizeof(afg_mel_row));
        const uint64_t tiles = afg_mel_layout(heap, rows.size(), &p);
        EXPECT(tiles > 0);
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at) == AFG_OK);
        // the refusals
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles + 1, &p, in_at, nb, bank_floats, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at - 1, nb, bank_floats, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb - 1, bank_floats, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats - 1, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at - 1) == AFG_ERR_INVALID);
        afg_mel_row keep = heap[0];
        heap[0].out_frames += 1;
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[0] = keep; heap[0].in_off = ~(uint64_t)0 - 3;
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[0] = keep; heap[0].out_off = ~(uint64_t)0 - 3;
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[0] = keep; heap[1].first_tile += 1;
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[1].first_tile -= 1;
        if (pad_mode == AFG_MEL_PAD_REFLECT && pad) {
            heap[0].in_frames = pad; heap[0].out_frames = 1;
            EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at) == AFG_ERR_INVALID);
            heap[0] = keep;
        }
        EXPECT(afg_mel_check_rows(heap, rows.size(), tiles, &p, in_at, nb, bank_floats, out_at) == AFG_OK);
        std::free(heap);
    }
}

static bool fft_takes(uint32_t n)
{
    if (n < 16 || n > 2048) return false;
    for (uint32_t q : { 2u, 3u, 5u })
        while (n % q == 0) n /= q;
    return n == 1;
}

// the FFT path over the same rows: its table in a heap buffer of exactly its size, its layout (tiles of 16 frames), every refusal
static void fft_shape(const Shape &s)
{
    const uint64_t nt = afg_mel_fft_tables(s.n_fft, s.win, nullptr, 0);
    if (!fft_takes(s.n_fft)) {
        afg_mel_params p = params_of(s, 0);
        afg_mel_row row;
        std::memset(&row, 0, sizeof(row));
        EXPECT(nt == 0);
        EXPECT(afg_mel_fft_layout(&row, 1, &p) == 0);
        EXPECT(afg_mel_fft_check_rows(&row, 1, 0, &p, 0, 0, 0, 0) == AFG_ERR_UNSUPPORTED);
        return;
    }
    EXPECT(nt == (uint64_t)s.win + 2 * (uint64_t)s.n_fft);
    float *table = (float *)std::malloc((size_t)nt * sizeof(float));
    EXPECT(afg_mel_fft_tables(s.n_fft, s.win, table, nt) == nt);
    EXPECT(table[s.win] == 1.0f && table[s.win + 1] == 0.0f && table[0] == 0.0f);
    float *shorter = (float *)std::malloc((size_t)(nt - 1) * sizeof(float));
    EXPECT(afg_mel_fft_tables(s.n_fft, s.win, shorter, nt - 1) == nt);
    std::free(shorter);
    std::free(table);
    const uint64_t bank_floats = (uint64_t)s.n_mels * (s.n_fft / 2 + 1);
    for (uint32_t pad_mode = 0; pad_mode < 2; pad_mode++) {
        const afg_mel_params p = params_of(s, pad_mode);
        const uint32_t pad = s.center ? s.n_fft / 2 : 0;
        const uint32_t lengths[] = { 3 * s.n_fft + 5, pad + 1 > (s.center ? 0 : s.n_fft) ? pad + 1 : s.n_fft, 16 * s.hop + s.n_fft - 2 * pad, 0,
                                     5 * s.hop + s.n_fft, 0xffffffffu };
        std::vector<afg_mel_row> rows;
        uint64_t in_at = 0, out_at = 0, want_tiles = 0;
        for (uint32_t n : lengths) {
            afg_mel_row r;
            std::memset(&r, 0, sizeof(r));
            r.in_off = in_at; r.out_off = out_at; r.in_frames = n;
            r.out_frames = afg_mel_frames(&p, n);
            if (pad_mode == AFG_MEL_PAD_REFLECT && n <= pad) r.out_frames = 0;
            in_at += n; out_at += (uint64_t)s.n_mels * r.out_frames;
            want_tiles += ((uint64_t)r.out_frames + 15) / 16;
            rows.push_back(r);
        }
        afg_mel_row *heap = (afg_mel_row *)std::malloc(rows.size() * sizeof(afg_mel_row));       // exactly the records
        std::memcpy(heap, rows.data(), rows.size() * sizeof(afg_mel_row));
        const uint64_t tiles = afg_mel_fft_layout(heap, rows.size(), &p);
        EXPECT(tiles == want_tiles);
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at) == AFG_OK);
        // the refusals
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles + 1, &p, in_at, nt, bank_floats, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at - 1, nt, bank_floats, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt - 1, bank_floats, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats - 1, out_at) == AFG_ERR_INVALID);
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at - 1) == AFG_ERR_INVALID);
        afg_mel_row keep = heap[0];
        heap[0].out_frames += 1;
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[0] = keep; heap[0].in_off = ~(uint64_t)0 - 3;
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[0] = keep; heap[0].out_off = ~(uint64_t)0 - 3;
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[0] = keep; heap[1].first_tile += 1;
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at) == AFG_ERR_INVALID);
        heap[1].first_tile -= 1;
        if (pad_mode == AFG_MEL_PAD_REFLECT && pad) {
            heap[0].in_frames = pad; heap[0].out_frames = 1;
            EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at) == AFG_ERR_INVALID);
            heap[0] = keep;
        }
        EXPECT(afg_mel_fft_check_rows(heap, rows.size(), tiles, &p, in_at, nt, bank_floats, out_at) == AFG_OK);
        std::free(heap);
    }
}

int main()
{
    const Shape shapes[] = { { 400, 400, 160, 80, 1 }, { 512, 400, 128, 23, 1 }, { 16, 16, 1, 1, 1 }, { 2048, 2048, 2048, 256, 0 },
                             { 2048, 1, 1, 256, 1 }, { 401, 7, 401, 3, 1 } };
    for (const Shape &s : shapes) shape(s);
    const Shape fft_shapes[] = { { 400, 400, 160, 80, 1 }, { 512, 400, 128, 23, 1 }, { 16, 16, 1, 1, 1 }, { 60, 45, 7, 5, 1 }, { 250, 250, 100, 17, 1 },
                                 { 2048, 2048, 2048, 256, 0 }, { 2048, 1, 1, 256, 1 }, { 75, 75, 30, 9, 1 }, { 2025, 7, 2025, 3, 1 },
                                 { 401, 7, 401, 3, 1 }, { 17, 16, 4, 3, 1 }, { 77, 16, 4, 3, 1 }, { 2047, 16, 4, 3, 1 } };
    for (const Shape &s : fft_shapes) fft_shape(s);
    // parameters out of range: every entry refuses them
    const Shape good = shapes[0];
    afg_mel_row row;
    std::memset(&row, 0, sizeof(row));
    for (int k = 0; k < 12; k++) {
        afg_mel_params p = params_of(good, 0);
        switch (k) {
        case 0: p.n_fft = 15; break;
        case 1: p.n_fft = 2049; break;
        case 2: p.win_length = 0; break;
        case 3: p.win_length = 401; break;
        case 4: p.hop = 0; break;
        case 5: p.hop = 401; break;
        case 6: p.n_mels = 0; break;
        case 7: p.n_mels = 257; break;
        case 8: p.center = 2; break;
        case 9: p.pad_mode = 2; break;
        case 10: p.out_kind = 2; break;
        default: p.log_floor = -1.0f; break;
        }
        EXPECT(afg_mel_frames(&p, 1000) == 0);
        EXPECT(afg_mel_layout(&row, 1, &p) == 0);
        EXPECT(afg_mel_check_rows(&row, 1, 0, &p, 0, 0, 0, 0) == AFG_ERR_INVALID);
        EXPECT(afg_mel_fft_layout(&row, 1, &p) == 0);
        EXPECT(afg_mel_fft_check_rows(&row, 1, 0, &p, 0, 0, 0, 0) == AFG_ERR_INVALID);
    }
    EXPECT(afg_mel_fft_tables(15, 15, nullptr, 0) == 0 && afg_mel_fft_tables(2049, 1, nullptr, 0) == 0 && afg_mel_fft_tables(400, 401, nullptr, 0) == 0);
    EXPECT(afg_mel_fft_tables(400, 0, nullptr, 0) == 0);
    EXPECT(afg_mel_frames(nullptr, 1000) == 0);
    EXPECT(afg_mel_basis(15, 15, nullptr, 0) == 0 && afg_mel_basis(2049, 1, nullptr, 0) == 0 && afg_mel_basis(400, 401, nullptr, 0) == 0);
    EXPECT(afg_mel_filters(0, 400, 80, 0, 0, 0, 0, nullptr, 0) == 0 && afg_mel_filters(16000, 400, 257, 0, 0, 0, 0, nullptr, 0) == 0);
    EXPECT(afg_mel_filters(16000, 400, 80, 8000.0, 0, 0, 0, nullptr, 0) == 0 && afg_mel_filters(16000, 400, 80, 0, 8001.0, 0, 0, nullptr, 0) == 0);
    EXPECT(afg_mel_filters(16000, 400, 80, 0, 0, 2, 0, nullptr, 0) == 0 && afg_mel_filters(16000, 400, 80, 0, 0, 0, 2, nullptr, 0) == 0);
    std::printf(failures ? "melspec_host_check: %d FAILED\n" : "melspec_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
