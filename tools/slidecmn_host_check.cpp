// slidecmn_host_check.cpp -- the host-only half of the sliding-window normalisation under AddressSanitizer and
// UndefinedBehaviorSanitizer: afg_cmn_layout, afg_cmn_work_bytes, the slab and parameter checks of afg_slide_cmn_hip
// (afg_cmn_check_slabs) and the refusals afg_batch_decode_fbank_cmn makes before any device call, each at its extremes, with
// the records in heap buffers of exactly their size.  `make -C audio-formats_amd slidecmn_host_check` compiles
// host/afg_slidecmn.cpp with -fsanitize=address,undefined into this program (everything else comes from the library as it is)
// and runs it.  It needs no device and makes no device call.
#include "../audio-formats_amd/host/afg_stage.h"

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

static afg_cmn_params params_of(uint32_t cols, uint32_t layout)
{
    afg_cmn_params p;
    std::memset(&p, 0, sizeof(p));
    p.cmn_window = 600; p.min_cmn_window = 100; p.center = 0; p.norm_vars = 1; p.cols = cols; p.layout = layout;
    return p;
}

static afg_cmn_slab slab_of(uint64_t off, uint64_t pitch, uint32_t n)
{
    afg_cmn_slab s;
    std::memset(&s, 0, sizeof(s));
    s.in_off = s.out_off = off; s.pitch = pitch; s.n_frames = n;
    return s;
}

static void slabs_and_refusals(uint32_t layout)
{
    const uint32_t cols = 81, frames[] = { 0, 1, 31, 32, 33, 3000, 0x7fffffffu };
    const bool cm = layout == AFG_CMN_COL_MAJOR;
    std::vector<afg_cmn_slab> made;
    uint64_t at = 0, want = 0;
    for (uint32_t n : frames) {
        const uint64_t pitch = (cm ? n : cols) + 3, rows = cm ? cols : n;
        made.push_back(slab_of(at, pitch, n));
        at += rows * pitch;
        want += ((uint64_t)n + 31) / 32;
    }
    const uint64_t k = made.size(), floats = at - 3;             // the last row's gap is not part of the plane
    afg_cmn_slab *heap = (afg_cmn_slab *)std::malloc(k * sizeof(afg_cmn_slab));                  // exactly the records
    std::memcpy(heap, made.data(), k * sizeof(afg_cmn_slab));
    const uint64_t tiles = afg_cmn_layout(heap, k);
    EXPECT(tiles == want && heap[0].first_tile == 0 && heap[1].first_tile == 0 && heap[2].first_tile == 1 && heap[5].first_tile == 5);
    EXPECT(afg_cmn_layout(nullptr, k) == 0);
    EXPECT(afg_cmn_work_bytes(tiles, cols) == tiles * cols * 144 && afg_cmn_work_bytes(0, cols) == 0);
    const afg_cmn_params p = params_of(cols, layout);
    for (int same = 0; same < 2; same++) {
        EXPECT(afg_cmn_check_slabs(heap, k, tiles, &p, floats, floats, same) == AFG_OK);
        EXPECT(afg_cmn_check_slabs(heap, k, tiles, &p, floats - 1, floats, same) == AFG_ERR_INVALID);
        EXPECT(afg_cmn_check_slabs(heap, k, tiles, &p, floats, floats - 1, same) == AFG_ERR_INVALID);
        EXPECT(afg_cmn_check_slabs(heap, k, tiles + 1, &p, floats, floats, same) == AFG_ERR_INVALID);
    }
    const uint64_t top = ~(uint64_t)0;
    for (int c = 0; c < 10; c++) {
        const afg_cmn_slab keep = heap[5], keep4 = heap[4];
        int same = 0;
        switch (c) {
        case 0: heap[5].in_off = top - 3; break;
        case 1: heap[5].out_off = top - 3; break;
        case 2: heap[5].pitch = top; break;
        case 3: heap[5].pitch = top / 2 + 1; break;             // (rows - 1) * pitch wraps
        case 4: heap[5].pitch = (cm ? 3000 : cols) - 1; break;
        case 5: heap[5].first_tile += 1; break;
        case 6: heap[5].n_frames += 32; break;                  // one more tile than the layout counted
        case 7: heap[5].reserved[2] = 1; break;
        case 8: heap[5].out_off = heap[4].out_off + 1; break;   // two outputs meet
        default: heap[4].out_off = heap[5].in_off; heap[5].out_off = heap[4].in_off; same = 1; break;   // swapped in one plane
        }
        EXPECT(afg_cmn_check_slabs(heap, k, tiles, &p, floats, floats, same) == AFG_ERR_INVALID);
        heap[5] = keep; heap[4] = keep4;
    }
    heap[0].in_off = heap[0].out_off = top;                      // nothing of a slab without frames is looked at
    heap[0].pitch = 0;
    EXPECT(afg_cmn_check_slabs(heap, k, tiles, &p, floats, floats, 1) == AFG_OK);
    heap[6].n_frames = 0x80000000u;
    EXPECT(afg_cmn_check_slabs(heap, k, tiles, &p, top, top, 0) == AFG_ERR_INVALID);
    EXPECT(afg_cmn_check_slabs(heap, k, tiles, nullptr, floats, floats, 0) == AFG_ERR_INVALID);
    EXPECT(afg_cmn_check_slabs(nullptr, 1, 0, &p, 0, 0, 0) == AFG_ERR_INVALID);
    std::free(heap);
}

static void parameters()
{
    const afg_cmn_params good = params_of(80, AFG_CMN_FRAMES_MAJOR);
    EXPECT(afg_cmn_check_slabs(nullptr, 0, 0, &good, 0, 0, 0) == AFG_OK);
    for (int c = 0; c < 10; c++) {
        afg_cmn_params q = good;
        switch (c) {
        case 0: q.cmn_window = 0; break;
        case 1: q.cmn_window = AFG_CMN_MAX_WINDOW + 1; break;
        case 2: q.min_cmn_window = 0; break;
        case 3: q.min_cmn_window = 0xffffffffu; break;
        case 4: q.center = 2; break;
        case 5: q.norm_vars = 2; break;
        case 6: q.cols = 0; break;
        case 7: q.cols = AFG_CMN_MAX_COLS + 1; break;
        case 8: q.layout = 2; break;
        default: q.reserved[1] = 1; break;
        }
        EXPECT(afg_cmn_check_slabs(nullptr, 0, 0, &q, 0, 0, 0) == AFG_ERR_INVALID);
    }
    afg_cmn_params q = good;
    q.cmn_window = AFG_CMN_MAX_WINDOW; q.min_cmn_window = 1; q.center = 1; q.cols = AFG_CMN_MAX_COLS; q.layout = AFG_CMN_COL_MAJOR;
    EXPECT(afg_cmn_check_slabs(nullptr, 0, 0, &q, 0, 0, 0) == AFG_OK);
}

// what the one-call entry refuses before any device call
static void batch_refusals()
{
    afg_fbank_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o);
    o.channels = 1; o.frames = 4000; o.samplerate = 16000; o.mono = 1;
    o.fbank.win_length = 400; o.fbank.hop = 160; o.fbank.n_fft = 512; o.fbank.n_mels = 23;
    o.fbank.snip_edges = 1; o.fbank.remove_dc = 1; o.fbank.use_power = 1; o.fbank.use_log = 1; o.fbank.preemph = 0.97f;
    o.low_freq = 20.0;
    afg_cmn_params cmn = params_of(0, 7);                        // cols and layout are filled in from the fbank options
    afg_batch_result res;
    float dummy = 0.0f;
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, &o, &cmn, &dummy, nullptr, &res) == AFG_OK && res.n_files == 0);
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, &o, nullptr, &dummy, nullptr, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, nullptr, &cmn, &dummy, nullptr, &res) == AFG_ERR_INVALID);
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, &o, &cmn, nullptr, nullptr, &res) == AFG_ERR_INVALID);
    cmn.cmn_window = 0;
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, &o, &cmn, &dummy, nullptr, &res) == AFG_ERR_INVALID);
    cmn.cmn_window = 300; cmn.norm_vars = 3;
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, &o, &cmn, &dummy, nullptr, &res) == AFG_ERR_INVALID);
    cmn.norm_vars = 1;
    o.fbank.n_mels = 0;                                          // the fbank parameters are refused in front of the window's
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, &o, &cmn, &dummy, nullptr, &res) != AFG_OK);
    o.fbank.n_mels = 23; o.struct_size -= 1;
    EXPECT(afg_batch_decode_fbank_cmn(nullptr, nullptr, 0, &o, &cmn, &dummy, nullptr, &res) == AFG_ERR_INVALID);
}

int main()
{
    slabs_and_refusals(AFG_CMN_FRAMES_MAJOR);
    slabs_and_refusals(AFG_CMN_COL_MAJOR);
    parameters();
    batch_refusals();
    std::printf(failures ? "slidecmn_host_check: %d FAILED\n" : "slidecmn_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
