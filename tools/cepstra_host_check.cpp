// cepstra_host_check.cpp -- the host-only half of the cepstral stage under AddressSanitizer and UndefinedBehaviorSanitizer:
// afg_cep_dct, afg_cep_layout, the record and parameter checks of afg_cepstra_hip (afg_cep_check_rows) and the refusals
// afg_batch_decode_mfcc makes before any device call, each at its extremes, with tables and records in heap buffers of
// exactly their size.  `make -C audio-formats_amd cepstra_host_check` compiles host/afg_cepstra.cpp with
// -fsanitize=address,undefined into this program (everything else comes from the library as it is) and runs it.  It needs no
// device and makes no device call.
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

static afg_cep_params params_of(uint32_t n_mels, uint32_t n_ceps, uint32_t order, uint32_t win)
{
    afg_cep_params p;
    std::memset(&p, 0, sizeof(p));
    p.n_mels = n_mels; p.n_ceps = n_ceps; p.delta_order = order; p.delta_win = win;
    return p;
}

static void tables()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (uint32_t n_mels : { 1u, 3u, 80u, 256u })
        for (uint32_t n_ceps : { 1u, n_mels })
            for (uint32_t norm : { (uint32_t)AFG_CEP_DCT_NONE, (uint32_t)AFG_CEP_DCT_ORTHO })
                for (double lifter : { 0.0, 22.0, 1e-300, 1e300 }) {
                    const uint64_t need = afg_cep_dct(n_ceps, n_mels, norm, lifter, std::log(10.0), nullptr, 0);
                    EXPECT(need == (uint64_t)n_ceps * n_mels);
                    float *heap = (float *)std::malloc(need * sizeof(float));                  // exactly the table
                    EXPECT(afg_cep_dct(n_ceps, n_mels, norm, lifter, std::log(10.0), heap, need) == need);
                    const double s0 = norm == AFG_CEP_DCT_ORTHO ? std::sqrt(1.0 / n_mels) : 2.0;
                    EXPECT(heap[0] == (float)(std::log(10.0) * s0));                           // q = 0: the lifter is 1, the cosine is 1
                    for (uint64_t k = 0; k < need; k++) EXPECT(std::isfinite(heap[k]));
                    heap[need - 1] = -77.0f;
                    EXPECT(afg_cep_dct(n_ceps, n_mels, norm, lifter, std::log(10.0), heap, need - 1) == need && heap[need - 1] == -77.0f);   // too small: untouched
                    std::free(heap);
                }
    EXPECT(afg_cep_dct(1, 0, AFG_CEP_DCT_ORTHO, 0.0, 1.0, nullptr, 0) == 0 && afg_cep_dct(1, 257, AFG_CEP_DCT_ORTHO, 0.0, 1.0, nullptr, 0) == 0);
    EXPECT(afg_cep_dct(0, 80, AFG_CEP_DCT_ORTHO, 0.0, 1.0, nullptr, 0) == 0 && afg_cep_dct(81, 80, AFG_CEP_DCT_ORTHO, 0.0, 1.0, nullptr, 0) == 0);
    EXPECT(afg_cep_dct(13, 80, 2, 0.0, 1.0, nullptr, 0) == 0 && afg_cep_dct(13, 80, 0xffffffffu, 0.0, 1.0, nullptr, 0) == 0);
    for (double bad : { -1.0, inf, -inf, nan }) EXPECT(afg_cep_dct(13, 80, AFG_CEP_DCT_ORTHO, bad, 1.0, nullptr, 0) == 0);
    for (double bad : { 0.0, inf, -inf, nan }) EXPECT(afg_cep_dct(13, 80, AFG_CEP_DCT_ORTHO, 0.0, bad, nullptr, 0) == 0);
    EXPECT(afg_cep_dct(13, 80, AFG_CEP_DCT_ORTHO, 0.0, -1.0, nullptr, 0) == 13 * 80);
}

static void records_and_refusals()
{
    const uint32_t frames[] = { 0, 1, 63, 64, 65, 129, 0, 0xffffffffu };
    const afg_cep_params p = params_of(256, 256, 2, 8);
    const uint64_t n = sizeof frames / sizeof frames[0], in_rows = 256, out_rows = 3 * 256;
    afg_cep_row *heap = (afg_cep_row *)std::malloc(n * sizeof(afg_cep_row));                   // exactly the records
    std::memset(heap, 0, n * sizeof(afg_cep_row));
    uint64_t in_at = 3, out_at = 5, want_tiles = 0;
    for (uint64_t k = 0; k < n; k++) {
        heap[k].in_off = in_at; heap[k].out_off = out_at; heap[k].frames = frames[k];
        in_at += in_rows * frames[k];
        out_at += out_rows * frames[k];
        want_tiles += ((uint64_t)frames[k] + 63) / 64;
    }
    const uint64_t tiles = afg_cep_layout(heap, n, &p);
    EXPECT(tiles == want_tiles && heap[0].first_tile == 0 && heap[2].first_tile == 1 && heap[5].first_tile == 5 && heap[7].first_tile == 8);
    EXPECT(afg_cep_layout(nullptr, n, &p) == 0 && afg_cep_layout(heap, n, nullptr) == 0);
    const uint64_t dct = 256 * 256;
    EXPECT(afg_cep_check_rows(heap, n, tiles, &p, in_at, dct, out_at) == AFG_OK);
    EXPECT(afg_cep_check_rows(nullptr, 0, 0, &p, 0, 0, 0) == AFG_OK);
    EXPECT(afg_cep_check_rows(heap, n, tiles, &p, in_at - 1, dct, out_at) == AFG_ERR_INVALID);
    EXPECT(afg_cep_check_rows(heap, n, tiles, &p, in_at, dct - 1, out_at) == AFG_ERR_INVALID);
    EXPECT(afg_cep_check_rows(heap, n, tiles, &p, in_at, dct, out_at - 1) == AFG_ERR_INVALID);
    EXPECT(afg_cep_check_rows(heap, n, tiles + 1, &p, in_at, dct, out_at) == AFG_ERR_INVALID);
    EXPECT(afg_cep_check_rows(nullptr, 1, 0, &p, 0, dct, 0) == AFG_ERR_INVALID);
    EXPECT(afg_cep_check_rows(heap, n, tiles, nullptr, in_at, dct, out_at) == AFG_ERR_INVALID);
    const uint64_t top = ~(uint64_t)0;
    for (int k = 0; k < 5; k++) {
        const afg_cep_row keep = heap[5];
        switch (k) {
        case 0: heap[5].in_off = top - 3; break;                // offsets that would wrap
        case 1: heap[5].out_off = top - 3; break;
        case 2: heap[5].first_tile += 1; break;
        case 3: heap[5].reserved = 1; break;
        default: heap[5].frames += 64; break;                   // one more tile than the layout counted
        }
        EXPECT(afg_cep_check_rows(heap, n, tiles, &p, in_at, dct, out_at) == AFG_ERR_INVALID);
        heap[5] = keep;
    }
    heap[0].in_off = heap[0].out_off = top;                      // nothing of a record without frames is looked at
    EXPECT(afg_cep_check_rows(heap, n, tiles, &p, in_at, dct, out_at) == AFG_OK);
    std::free(heap);
    // parameters
    struct { uint32_t n_mels, n_ceps, order, win; bool ok; } cases[] = {
        { 1, 1, 0, 0, true }, { 256, 256, 2, 8, true }, { 80, 13, 0, 99, true }, { 80, 13, 1, 1, true },
        { 0, 1, 0, 0, false }, { 257, 1, 0, 0, false }, { 80, 0, 0, 0, false }, { 80, 81, 0, 0, false }, { 80, 13, 3, 2, false },
        { 80, 13, 0xffffffffu, 2, false }, { 80, 13, 1, 0, false }, { 80, 13, 2, 9, false },
    };
    for (const auto &c : cases) {
        const afg_cep_params q = params_of(c.n_mels, c.n_ceps, c.order, c.win);
        EXPECT((afg_cep_check_rows(nullptr, 0, 0, &q, 0, 0, 0) == AFG_OK) == c.ok);
        EXPECT((afg_cep_layout(nullptr, 0, &q) == 0));
    }
    for (int k = 0; k < 4; k++) {
        afg_cep_params q = params_of(80, 13, 2, 2);
        q.reserved[k] = 1u << k;
        EXPECT(afg_cep_check_rows(nullptr, 0, 0, &q, 0, 0, 0) == AFG_ERR_INVALID);
    }
}

static afg_mfcc_opts mfcc_opts()
{
    afg_mfcc_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o);
    o.dct_norm = AFG_CEP_DCT_ORTHO;
    o.mel.struct_size = (uint32_t)sizeof(o.mel);
    o.mel.n_threads = 1; o.mel.channels = 1; o.mel.frames = 16000; o.mel.samplerate = 16000; o.mel.mono = 1;
    o.mel.mel.n_fft = 400; o.mel.mel.win_length = 400; o.mel.mel.hop = 160; o.mel.mel.n_mels = 80; o.mel.mel.center = 1;
    o.mel.mel.out_kind = AFG_MEL_LOG10;
    o.mel.norm = AFG_MEL_NORM_SLANEY;
    o.cep = params_of(80, 13, 2, 2);
    return o;
}

static int call(int n_files, const afg_mfcc_opts *o, const afg_norm_params *wave, const afg_norm_params *cmvn, bool d_out = true, bool out = true)
{
    static const uint8_t byte = 'x';
    const uint8_t *data[1] = { &byte };
    const size_t length[1] = { 1 };
    afg_batch_result res;
    res.n_files = -1; res.items = nullptr; res.owner = nullptr;
    const int rc = afg_batch_decode_mfcc(data, length, n_files, o, wave, cmvn, d_out ? (float *)0x1000 : nullptr, out ? &res : nullptr);
    if (o && d_out && out) EXPECT(res.n_files == 0 && !res.items && !res.owner);
    return rc;
}

static void batch_refusals()
{
    afg_norm_params std_ = { AFG_NORM_STANDARD, 1.0f, 0.0f, 8.0f, 4.0f, 0.25f };
    afg_mfcc_opts o = mfcc_opts();
    EXPECT(call(0, &o, nullptr, nullptr) == AFG_OK && call(0, &o, &std_, &std_) == AFG_OK);      // no file: ok, nothing touched
    EXPECT(call(1, nullptr, nullptr, nullptr) == AFG_ERR_INVALID);
    EXPECT(call(1, &o, nullptr, nullptr, false) == AFG_ERR_INVALID && call(1, &o, nullptr, nullptr, true, false) == AFG_ERR_INVALID);
    EXPECT(call(-1, &o, nullptr, nullptr) == AFG_ERR_INVALID);
#define REFUSED(change)                                             \
    do {                                                            \
        afg_mfcc_opts b = mfcc_opts();                              \
        change;                                                     \
        EXPECT(call(1, &b, nullptr, nullptr) == AFG_ERR_INVALID);   \
        EXPECT(call(0, &b, nullptr, nullptr) == AFG_ERR_INVALID);   \
    } while (0)
    REFUSED(b.struct_size -= 8);
    REFUSED(b.mel.struct_size -= 8);
    REFUSED(b.mel.channels = 0);
    REFUSED(b.mel.reserved = 1);
    REFUSED(b.mel.algorithm = 2);
    REFUSED(b.mel.mel.n_fft = 15);
    REFUSED(b.mel.mel.out_kind = AFG_MEL_POWER);
    REFUSED(b.mel.mel.n_mels = 40);
    REFUSED(b.cep.n_mels = 40);
    REFUSED(b.cep.n_ceps = 81);
    REFUSED(b.cep.delta_order = 3);
    REFUSED(b.cep.delta_win = 9);
    REFUSED(b.cep.reserved[3] = 1);
    REFUSED(b.dct_norm = 2);
    REFUSED(b.lifter = -1.0);
    REFUSED(b.lifter = std::numeric_limits<double>::quiet_NaN());
    REFUSED(b.log_scale = std::numeric_limits<double>::infinity());
#undef REFUSED
    afg_norm_params bad = std_;
    bad.mode = 5;
    EXPECT(call(1, &o, nullptr, &bad) == AFG_ERR_INVALID && call(1, &o, &bad, nullptr) == AFG_ERR_INVALID);
    bad = std_;
    bad.eps = -1.0f;
    EXPECT(call(1, &o, nullptr, &bad) == AFG_ERR_INVALID);
}

int main()
{
    tables();
    records_and_refusals();
    batch_refusals();
    std::printf(failures ? "cepstra_host_check: %d FAILED\n" : "cepstra_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
