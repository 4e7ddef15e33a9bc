// filter_host_check.cpp -- the host-only half of the filter stage under AddressSanitizer and UndefinedBehaviorSanitizer:
// afg_biquad_design, afg_filter_bound, the row and parameter checks of afg_filter_hip (afg_filter_check_rows) and the refusals
// of afg_batch_decode_filtered, each at its extremes (frames = 0xffffffff, offsets near 2^64, eight sections, poles next to
// the unit circle), with the records in heap buffers of exactly their size.  `make -C audio-formats_amd filter_host_check`
// compiles host/afg_filter.cpp with -fsanitize=address,undefined into this program (everything else comes from the library
// as it is) and runs it.  It needs no device and makes no device call.
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

static afg_filter_params *cascade(std::vector<afg_biquad> sec)
{
    // exactly the sections the cascade has: reading sec[n_sections ..] is reading past the buffer
    const size_t bytes = offsetof(afg_filter_params, sec) + sec.size() * sizeof(afg_biquad);
    afg_filter_params *p = (afg_filter_params *)std::malloc(bytes);
    p->n_sections = (uint32_t)sec.size();
    std::memcpy((char *)p + offsetof(afg_filter_params, sec), sec.data(), sec.size() * sizeof(afg_biquad));
    return p;
}

static afg_biquad design(uint32_t kind, double fs, double f0, double q = std::sqrt(0.5), double db = 0.0)
{
    afg_biquad b;
    EXPECT(afg_biquad_design(kind, fs, f0, q, db, &b) == AFG_OK);
    return b;
}

static void helper_and_bound()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (uint32_t kind = AFG_BIQUAD_LOWPASS; kind <= AFG_BIQUAD_HIGHSHELF; kind++)
        for (double f0 : { 1e-3, 20.0, 1000.0, 23999.999 })
            for (double q : { 1e-3, 0.5, 8.0, 1e3 }) {
                afg_biquad b;
                const int rc = afg_biquad_design(kind, 48000.0, f0, q, 6.0, &b);
                if (rc != AFG_OK) continue;                      // (a section that is not stable in double is refused, not delivered)
                EXPECT(std::fabs(b.a2) < 1.0 && std::fabs(b.a1) < 1.0 + b.a2);
            }
    afg_biquad keep = { 7, 7, 7, 7, 7 };
    EXPECT(afg_biquad_design(10, 48000.0, 100.0, 1.0, 0.0, &keep) == AFG_ERR_INVALID && keep.b0 == 7);
    EXPECT(afg_biquad_design(0, 48000.0, 24000.0, 1.0, 0.0, &keep) == AFG_ERR_INVALID);
    EXPECT(afg_biquad_design(0, 48000.0, nan, 1.0, 0.0, &keep) == AFG_ERR_INVALID);
    EXPECT(afg_biquad_design(0, inf, 100.0, 1.0, 0.0, &keep) == AFG_ERR_INVALID);
    EXPECT(afg_biquad_design(0, 48000.0, 100.0, 0.0, 0.0, &keep) == AFG_ERR_INVALID);
    EXPECT(afg_biquad_design(5, 48000.0, 100.0, 1.0, nan, &keep) == AFG_ERR_INVALID);
    EXPECT(afg_biquad_design(8, 0.0, 1.5, 0.0, 0.0, &keep) == AFG_ERR_INVALID && keep.a2 == 7);
    EXPECT(afg_biquad_design(0, 48000.0, 100.0, 1.0, 0.0, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_biquad_design(AFG_BIQUAD_PREEMPHASIS, nan, 0.97, nan, nan, &keep) == AFG_OK && keep.b1 == -0.97 && keep.a1 == 0.0);

    const afg_biquad hp = design(AFG_BIQUAD_HIGHPASS, 48000.0, 20.0), lp = design(AFG_BIQUAD_LOWPASS, 48000.0, 50.0, 5.0);
    afg_filter_params *one = cascade({ hp }), *eight = cascade({ hp, lp, hp, lp, hp, lp, hp, lp });
    EXPECT(afg_filter_bound(one) > 0.0 && afg_filter_bound(one) < 1e-9);
    EXPECT(afg_filter_bound(eight) > afg_filter_bound(one));
    // a pole within 1e-6 of the circle: a long sum that ends
    afg_filter_params *slow = cascade({ design(AFG_BIQUAD_DC_BLOCK, 48000.0, 0.01) });
    EXPECT(afg_filter_bound(slow) > 0.0);
    afg_filter_params *fir = cascade({ afg_biquad{ 1.0, -0.97, 0.0, 0.0, 0.0 } });
    EXPECT(afg_filter_bound(fir) == std::ldexp(1.97, -53));
    afg_filter_params *loud = cascade(std::vector<afg_biquad>(8, afg_biquad{ 2048.0, 0.0, 0.0, 0.0, 0.0 }));
    EXPECT(afg_filter_bound(loud) == 0.0 && std::strstr(afg_last_error(), "2^30"));
    for (afg_biquad bad : { afg_biquad{ 1, 0, 0, -2.0, 1.0 }, afg_biquad{ 1, 0, 0, 0, 1.0 }, afg_biquad{ 1, 0, 0, 0, -1.0 }, afg_biquad{ 1, 0, 0, 1.6, 0.5 },
                            afg_biquad{ nan, 0, 0, 0, 0 }, afg_biquad{ 1, 0, inf, 0, 0 }, afg_biquad{ 1, 0, 0, nan, 0 }, afg_biquad{ 1, 0, 0, 0, nan } }) {
        afg_filter_params *p = cascade({ hp, bad });
        EXPECT(afg_filter_bound(p) == 0.0 && std::strstr(afg_last_error(), "sec[1]"));
        EXPECT(afg_filter_check_rows(nullptr, 0, p, 0, 0, 0) == AFG_ERR_INVALID);
        EXPECT(afg_filter_hip(0, nullptr, p, nullptr, 0, nullptr, 0, nullptr, nullptr) == AFG_ERR_INVALID);
        std::free(p);
    }
    afg_filter_params none, nine;
    std::memset(&none, 0, sizeof none);
    std::memset(&nine, 0, sizeof nine);
    nine.n_sections = 9;
    EXPECT(afg_filter_bound(&none) == 0.0 && afg_filter_bound(&nine) == 0.0 && afg_filter_bound(nullptr) == 0.0);
    EXPECT(afg_filter_tile_frames() == AFG_FILTER_TILE);
    std::free(one); std::free(eight); std::free(slow); std::free(fir); std::free(loud);
}

static afg_filter_row *rows_of(const std::vector<afg_filter_row> &r)
{
    afg_filter_row *heap = (afg_filter_row *)std::malloc(r.size() * sizeof(afg_filter_row) + 1);     // exactly the records
    std::memcpy(heap, r.data(), r.size() * sizeof(afg_filter_row));
    return heap;
}

static int check(const std::vector<afg_filter_row> &r, const afg_filter_params *p, uint64_t in_floats, uint64_t out_floats, int same)
{
    afg_filter_row *heap = rows_of(r);
    const int rc = afg_filter_check_rows(heap, r.size(), p, in_floats, out_floats, same);
    std::free(heap);
    return rc;
}

static void rows_and_refusals()
{
    afg_filter_params *p = cascade({ design(AFG_BIQUAD_HIGHPASS, 48000.0, 20.0) });
    const uint64_t top = ~(uint64_t)0;
    const uint32_t longest = 0xffffffffu;
    EXPECT(check({ { 0, 0, 100, 0 }, { 100, 100, 0, 0 }, { 150, 150, 50, 0 }, { 200, 300, 50, 0 }, { 200, 400, 50, 0 }, { top, top, 0, 0 } }, p, 500, 500, 1) == AFG_OK);
    EXPECT(check({ { 0, 0, longest, 0 } }, p, longest, longest, 1) == AFG_OK);
    EXPECT(check({ { 0, 0, longest, 0 } }, p, longest - 1, longest, 1) == AFG_ERR_INVALID);
    EXPECT(check({ { 0, 0, longest, 0 } }, p, longest, longest - 1, 0) == AFG_ERR_INVALID);
    EXPECT(check({ { top - 4, 0, 10, 0 } }, p, top, top, 0) == AFG_ERR_INVALID);                     // an offset that would wrap
    EXPECT(check({ { 0, top - 4, 10, 0 } }, p, top, top, 0) == AFG_ERR_INVALID);
    EXPECT(check({ { top - 10, top - 10, 10, 0 } }, p, top, top, 1) == AFG_OK);                      // the last floats of the largest plane
    EXPECT(check({ { 0, 0, 100, 0 }, { 200, 50, 100, 0 } }, p, 500, 500, 0) == AFG_ERR_INVALID);     // two outputs
    EXPECT(check({ { 0, 0, 100, 0 }, { 0, 0, 100, 0 } }, p, 500, 500, 1) == AFG_ERR_INVALID);
    EXPECT(check({ { 0, 1, 100, 0 } }, p, 500, 500, 1) == AFG_ERR_INVALID);                          // a row shifted onto itself
    EXPECT(check({ { 0, 1, 100, 0 } }, p, 500, 500, 0) == AFG_OK);                                   // ... in two planes it is not
    EXPECT(check({ { 0, 100, 100, 0 }, { 150, 300, 100, 0 } }, p, 500, 500, 1) == AFG_ERR_INVALID);  // an output over an input
    EXPECT(check({ { 100, 0, 100, 0 }, { 150, 150, 100, 0 } }, p, 500, 500, 1) == AFG_ERR_INVALID);
    EXPECT(check({ { 0, 0, 10, 1 } }, p, 500, 500, 1) == AFG_ERR_INVALID && std::strstr(afg_last_error(), "reserved"));
    EXPECT(afg_filter_check_rows(nullptr, 3, p, 500, 500, 1) == AFG_ERR_INVALID);
    EXPECT(afg_filter_check_rows(nullptr, 0, p, 0, 0, 1) == AFG_OK);
    // many rows, in place, packed: the overlap sweep over a sorted copy
    std::vector<afg_filter_row> many;
    for (uint32_t k = 0; k < 5000; k++) many.push_back(afg_filter_row{ (uint64_t)(4999 - k) * 7, (uint64_t)(4999 - k) * 7, 7, 0 });
    EXPECT(check(many, p, 35000, 35000, 1) == AFG_OK);
    many[77].frames = 8;
    EXPECT(check(many, p, 35000, 35000, 1) == AFG_ERR_INVALID);

    // the kernel entry's own checks come before any device call
    const float *in = (const float *)0x20000;
    float *out = (float *)0x30000;
    const afg_filter_row *d_rows = (const afg_filter_row *)0x1000;
    EXPECT(afg_filter_hip(0, nullptr, p, nullptr, 0, nullptr, 0, nullptr, nullptr) == AFG_OK);
    EXPECT(afg_filter_hip(1, nullptr, p, in, 1000, out, 1000, nullptr, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_filter_hip(1, d_rows, p, (const float *)0x20002, 1000, out, 1000, nullptr, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_filter_hip(1, d_rows, p, in, 1000, out, 1000, (double *)0x4004, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_filter_hip((uint64_t)1 << 31, d_rows, p, in, 1000, out, 1000, nullptr, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_filter_hip(1, d_rows, p, in, (uint64_t)1 << 61, out, 1000, nullptr, nullptr) == AFG_ERR_INVALID);
    EXPECT(afg_filter_hip(1, d_rows, p, in, 1000, (float *)(0x20000 + 3996), 1000, nullptr, nullptr) == AFG_ERR_INVALID);

    // the batch entry's refusals
    afg_resample_opts o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = (uint32_t)sizeof o; o.n_threads = 1; o.channels = 1; o.frames = 16000; o.samplerate = 16000; o.mono = 1;
    const uint8_t byte = 'x';
    const uint8_t *data[1] = { &byte };
    const size_t length[1] = { 1 };
    afg_batch_result res;
    float *d_out = (float *)0x1000;
    EXPECT(afg_batch_decode_filtered(data, length, 1, nullptr, p, d_out, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_filtered(data, length, 1, &o, nullptr, d_out, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_filtered(data, length, 1, &o, p, nullptr, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_filtered(data, length, 1, &o, p, d_out, nullptr) == AFG_ERR_INVALID);
    afg_resample_opts bad = o;
    bad.channels = 0;
    EXPECT(afg_batch_decode_filtered(data, length, 1, &bad, p, d_out, &res) == AFG_ERR_INVALID && res.n_files == 0 && !res.items);
    bad = o; bad.struct_size -= 8;
    EXPECT(afg_batch_decode_filtered(data, length, 1, &bad, p, d_out, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_filtered(data, length, -1, &o, p, d_out, &res) == AFG_ERR_INVALID);
    afg_filter_params *unstable = cascade({ afg_biquad{ 1, 0, 0, -2.0, 1.0 } });
    EXPECT(afg_batch_decode_filtered(data, length, 1, &o, unstable, d_out, &res) == AFG_ERR_INVALID && std::strstr(afg_last_error(), "unit circle"));
    EXPECT(afg_batch_decode_filtered(data, length, 0, &o, p, d_out, &res) == AFG_OK && res.n_files == 0);
    std::free(unstable);
    std::free(p);
}

int main()
{
    helper_and_bound();
    rows_and_refusals();
    if (failures) { std::fprintf(stderr, "filter_host_check: %d failures\n", failures); return 1; }
    std::printf("filter_host_check: ok\n");
    return 0;
}
