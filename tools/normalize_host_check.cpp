// normalize_host_check.cpp -- the host-only half of the normalisation stage under AddressSanitizer and
// UndefinedBehaviorSanitizer: afg_norm_layout, the group and parameter checks of afg_normalize_hip (afg_norm_check_groups),
// the valid length of a file's rows in the tensor at one rate and the groups made of a batch's items, each at its extremes,
// with the records in heap buffers of exactly their size.  `make -C audio-formats_amd normalize_host_check` compiles
// host/afg_normalize.cpp with -fsanitize=address,undefined into this program (everything else comes from the library as it is)
// and runs it.  It needs no device and makes no device call.
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

static afg_norm_params params_of(uint32_t mode)
{
    afg_norm_params p;
    p.mode = mode; p.target = 1.0f; p.eps = 0.0f; p.range = 8.0f; p.shift = 4.0f; p.gain = 0.25f;
    return p;
}

static afg_norm_group group_of(uint64_t off, uint64_t stride, uint32_t rows, uint32_t valid)
{
    afg_norm_group g;
    std::memset(&g, 0, sizeof(g));
    g.in_off = g.out_off = off; g.stride = stride; g.rows = rows; g.valid = valid;
    return g;
}

static void groups_and_refusals()
{
    const uint32_t lengths[] = { 0, 1, 3, 255, 1024, 4095, 4096, 4097, 2 * 4096 + 5, 0xffffffffu };
    std::vector<afg_norm_group> made;
    uint64_t at = 0, want_tiles = 0;
    for (uint32_t k = 0; k < sizeof lengths / sizeof lengths[0]; k++) {
        const uint32_t rows = k == 9 ? 65535 : 1 + k % 3;
        made.push_back(group_of(at, (uint64_t)lengths[k] + 5, rows, lengths[k]));
        at += (uint64_t)rows * ((uint64_t)lengths[k] + 5);
        want_tiles += (((uint64_t)lengths[k] + 4095) / 4096) * rows;
    }
    const uint64_t n = made.size(), floats = at - 5;             // the last row's gap is not part of the plane
    afg_norm_group *heap = (afg_norm_group *)std::malloc(n * sizeof(afg_norm_group));            // exactly the records
    std::memcpy(heap, made.data(), n * sizeof(afg_norm_group));
    const uint64_t tiles = afg_norm_layout(heap, n);
    EXPECT(tiles == want_tiles && heap[0].first_tile == 0 && heap[1].first_tile == 0 && heap[2].first_tile == 2);
    EXPECT(afg_norm_layout(nullptr, n) == 0);
    for (uint32_t mode = AFG_NORM_NONE; mode <= AFG_NORM_DYNAMIC_RANGE; mode++) {
        const afg_norm_params p = params_of(mode);
        EXPECT(afg_norm_check_groups(heap, n, tiles, &p, floats, floats) == AFG_OK);
        EXPECT(afg_norm_check_groups(nullptr, 0, 0, &p, 0, 0) == AFG_OK);
        EXPECT(afg_norm_check_groups(heap, n, tiles, &p, floats - 1, floats) == AFG_ERR_INVALID);
        EXPECT(afg_norm_check_groups(heap, n, tiles, &p, floats, floats - 1) == (mode == AFG_NORM_NONE ? AFG_OK : AFG_ERR_INVALID));
        EXPECT(afg_norm_check_groups(heap, n, tiles + 1, &p, floats, floats) == AFG_ERR_INVALID);
    }
    const afg_norm_params p = params_of(AFG_NORM_STANDARD);
    const uint64_t top = ~(uint64_t)0;
    for (int k = 0; k < 9; k++) {
        const afg_norm_group keep = heap[8];
        switch (k) {
        case 0: heap[8].in_off = top - 3; break;
        case 1: heap[8].out_off = top - 3; break;
        case 2: heap[8].stride = top; break;
        case 3: heap[8].stride = top / 2 + 1; break;            // (rows - 1) * stride wraps to 0
        case 4: heap[8].stride = heap[8].valid - 1; break;
        case 5: heap[8].rows = 0; break;
        case 6: heap[8].rows = 65536; break;
        case 7: heap[8].first_tile += 1; break;
        default: heap[8].valid += 4096; break;                  // one more tile a row than the layout counted
        }
        EXPECT(afg_norm_check_groups(heap, n, tiles, &p, floats, floats) == AFG_ERR_INVALID);
        heap[8] = keep;
    }
    heap[0].in_off = heap[0].out_off = top;                      // nothing of a group without floats is looked at but its rows
    heap[3].stride = 0;                                          // one row: the stride is not used
    EXPECT(afg_norm_check_groups(heap, n, tiles, &p, floats, floats) == AFG_OK);
    EXPECT(afg_norm_check_groups(heap, n, tiles, nullptr, floats, floats) == AFG_ERR_INVALID);
    EXPECT(afg_norm_check_groups(nullptr, 1, 0, &p, 0, 0) == AFG_ERR_INVALID);
    std::free(heap);
    // parameters
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float bad : { 0.0f, -1.0f, inf, -inf, nan }) {
        afg_norm_params q = params_of(AFG_NORM_PEAK);
        q.target = bad;
        EXPECT(afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID);
        q.mode = AFG_NORM_RMS;
        EXPECT(afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID);
        q = params_of(AFG_NORM_DYNAMIC_RANGE);
        q.range = bad;
        EXPECT(afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID);
        q = params_of(AFG_NORM_DYNAMIC_RANGE);
        q.gain = bad;
        EXPECT(afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID);
        q = params_of(AFG_NORM_DYNAMIC_RANGE);
        q.shift = bad;
        EXPECT((afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID) == !std::isfinite(bad));
        q = params_of(AFG_NORM_STANDARD);
        q.eps = bad;
        EXPECT((afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID) == (bad != 0.0f));
        q = params_of(AFG_NORM_NONE);                            // a mode looks at its own fields only
        q.target = q.eps = q.range = q.shift = q.gain = bad;
        EXPECT(afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_OK);
    }
    afg_norm_params q = params_of(5);
    EXPECT(afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID);
    q.mode = 0xffffffffu;
    EXPECT(afg_norm_check_groups(nullptr, 0, 0, &q, 0, 0) == AFG_ERR_INVALID);
}

static void valid_lengths()
{
    using afg_front::norm_valid;
    const int64_t most = std::numeric_limits<int64_t>::max();
    const uint32_t top = 0xffffffffu;
    EXPECT(norm_valid(3001, 0, 8000, 16000, 4000) == 4000 && norm_valid(1000, 0, 8000, 16000, 4000) == 2000);
    EXPECT(norm_valid(9000, 0, 44100, 16000, 4000) == 3266 && norm_valid(9000, 8999, 44100, 16000, 4000) == 1);
    EXPECT(norm_valid(1, 0, 1u << 20, 1, 10) == 1 && norm_valid(1, 0, 1, 1u << 20, top) == 1u << 20);
    EXPECT(norm_valid(0, 0, 8000, 16000, 10) == 0 && norm_valid(5, 5, 8000, 16000, 10) == 0 && norm_valid(5, 6, 8000, 16000, 10) == 0);
    EXPECT(norm_valid(-1, 0, 8000, 16000, 10) == 0 && norm_valid(5, -1, 8000, 16000, 10) == 0);
    EXPECT(norm_valid(5, 0, 0, 16000, 10) == 0 && norm_valid(5, 0, 8000, 0, 10) == 0);
    // the extremes: the product passes 2^64, the difference is the whole range
    EXPECT(norm_valid(most, 0, 1, top, top) == top && norm_valid(most, 0, top, 1, top) == 2147483649u);
    EXPECT(norm_valid(most, 0, top, top - 1, top) == top && norm_valid(most, most - 1, top, 1, top) == 1);
    EXPECT(norm_valid(most, most - 3, 3, 1u << 20, top) == 1u << 20);
    EXPECT(norm_valid((int64_t)top * 7, 0, 7, 1, top) == top && norm_valid((int64_t)top * 7 - 7, 0, 7, 1, top) == top - 1);

    // the groups of a batch's items
    afg_front::ResampleJob job;
    job.C = 2; job.T = 4000; job.samplerate = 16000;
    afg_batch_item items[5];
    std::memset(items, 0, sizeof(items));
    items[0].channels = 1; items[0].samplerate = 8000.0f; items[0].frames = 1000;
    items[1].channels = 6; items[1].samplerate = 44100.0f; items[1].frames = most;
    items[2].status = AFG_ERR_INVALID; items[2].channels = 2; items[2].samplerate = 16000.0f; items[2].frames = 100;
    items[3].channels = 2; items[3].samplerate = std::numeric_limits<float>::quiet_NaN(); items[3].frames = 100;
    items[4].channels = 0; items[4].samplerate = 5e9f; items[4].frames = -1;
    const int64_t first[5] = { 10, 0, 0, 0, 0 };
    std::vector<afg_norm_group> groups;
    afg_front::norm_file_groups(job, items, 5, first, groups);
    EXPECT(groups.size() == 5);
    EXPECT(groups[0].rows == 1 && groups[0].valid == 1980 && groups[0].stride == 4000 && groups[0].in_off == 0);
    EXPECT(groups[1].rows == 2 && groups[1].valid == 4000 && groups[1].in_off == 8000 && groups[1].out_off == 8000);
    EXPECT(groups[2].rows == 1 && groups[2].valid == 0 && groups[3].valid == 0 && groups[4].valid == 0 && groups[4].rows == 1);
    const uint64_t tiles = afg_norm_layout(groups.data(), groups.size());
    const afg_norm_params p = params_of(AFG_NORM_PEAK);
    EXPECT(tiles == 3 && afg_norm_check_groups(groups.data(), groups.size(), tiles, &p, 5 * 8000, 5 * 8000) == AFG_OK);
    job.mono = true; job.C = 1;
    groups.clear();
    afg_front::norm_file_groups(job, items, 5, nullptr, groups);
    EXPECT(groups[1].rows == 1 && groups[1].in_off == 4000 && groups[0].valid == 2000);
}

int main()
{
    groups_and_refusals();
    valid_lengths();
    std::printf(failures ? "normalize_host_check: %d FAILED\n" : "normalize_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
