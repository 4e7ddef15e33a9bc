// afg_records.h -- what the tensor stages share around their records (header only, host and device; DESIGN.md "A tensor
// stage's three layers"): the search by which a kernel finds the record of its tile, the containment test and the overlap
// sweep of the record checks, the caps of a launch, the download of the records in front of an afg_*_hip entry's checks, and
// the constants the host and device halves must agree on (the afg_mel_row check of the framing stages: mel_rows.h).  Every
// message keeps the wording of the stage that reports it: the caller passes its prefix and nouns.
#pragma once
#include "afg_common.h"

#include <algorithm>
#include <vector>

namespace afg {

constexpr double kPi = 3.14159265358979323846;
constexpr uint32_t kPlaneTile = 4096;                           // floats of one row per tile: normalize.hip and trim.hip, both halves

inline uint32_t gcd32(uint32_t a, uint32_t b)
{
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

// The last record whose `first` (first_tile, first_block) is <= key, of n >= 1 records sorted by it: the record of tile or
// block `key`, records without tiles having none.  What follows the search -- the guards, the tile's place in its record --
// is the kernel's own.
template <typename Rec, typename Key>
__device__ __forceinline__ uint32_t last_at_or_before(const Rec *__restrict__ recs, uint32_t n, uint64_t key, Key Rec::*first)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (recs[mid].*first <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// off + (rows - 1) * stride + len <= floats, without a sum that wraps (rows >= 1; a span or a single row: rows 1)
inline bool rows_inside(uint64_t off, uint64_t rows, uint64_t stride, uint64_t len, uint64_t floats)
{
    if (len > floats || off > floats - len) return false;
    return rows == 1 || stride <= (floats - len - off) / (rows - 1);
}

// One row [lo, hi) of a record `owner`: an output, or an input that shares the plane with the outputs at another offset.
struct Range { uint64_t lo, hi, owner; bool out; };

// An output row may meet nothing but its own input at the same offset (which the caller gives no range of its own); inputs
// may overlap inputs.  Sorts r.  True: *owner's row overlaps one of *other.
inline bool first_overlap(std::vector<Range> &r, uint64_t *owner, uint64_t *other)
{
    std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return a.lo != b.lo ? a.lo < b.lo : a.out > b.out; });
    uint64_t out_hi = 0, any_hi = 0, out_owner = 0, any_owner = 0;   // the furthest end so far of the outputs, of all ranges
    for (const Range &x : r) {
        if (x.lo < (x.out ? any_hi : out_hi)) {
            *owner = x.owner;
            *other = x.out ? any_owner : out_owner;
            return true;
        }
        if (x.out && x.hi > out_hi) { out_hi = x.hi; out_owner = x.owner; }
        if (x.hi > any_hi) { any_hi = x.hi; any_owner = x.owner; }
    }
    return false;
}

// The caps of a launch that finds records by tile: 2^32 - 1 records (`noun`: rows, spans, groups ...) and 2^31 - 1 tiles.
inline int launch_caps(const char *who, const char *noun, uint64_t n_recs, uint64_t n_tiles)
{
    if (n_recs <= 0xffffffffull && n_tiles <= 0x7fffffffull) return AFG_OK;
    set_error("%s: at most 2^32 - 1 %s and 2^31 - 1 tiles per launch", who, noun);
    return AFG_ERR_INVALID;
}

// fn(h) over the n records at d_recs as the kernel will see them (whatever wrote them was queued on `stream`): an
// afg_*_hip entry's way to its *_launch, which checks records in host memory.
template <typename Rec, typename Fn> int with_host_records(const Rec *d_recs, uint64_t n, hipStream_t stream, Fn fn)
{
    try {
        std::vector<Rec> h((size_t)n);
        AFG_HIP_CHECK(hipMemcpyAsync(h.data(), d_recs, (size_t)n * sizeof(Rec), hipMemcpyDeviceToHost, stream));
        AFG_HIP_CHECK(hipStreamSynchronize(stream));
        return fn((const Rec *)h.data());
    } catch (...) {
        set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

}  // namespace afg
