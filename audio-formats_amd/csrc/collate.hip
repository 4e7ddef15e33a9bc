// collate.hip -- runs of interleaved float samples inside a batch decode stage's plane to planar, padded rows of a
// [files, channels, frames] float32 tensor in device memory (afg_batch_decode_to_device), for gfx950.
//
// Work: a scatter of 4-byte words, memory-bound, no arithmetic on the samples.  One workgroup of 256 lanes per tile of
// 4096 input samples of one span (afg_collate_span), found by a search over the spans' first tiles (uniform per
// workgroup: scalar loads), as pcm_pack.hip does.  Sample s = sample0 + i of a run is frame s / channels, channel
// s % channels; the division is done once per tile on uniform values (for 1 and 2 channels it is a shift), and a lane
// only ever adds to its result.  Paths:
//   zero run      the tile's floats, cut at the 16-byte boundaries of the output address: head (up to 3 floats, one per
//                 lane), interior (units of 16 floats = 4 aligned dwordx4 per lane), tail (one float per lane)
//   1 channel     a shifted copy with the same cut: dwordx4 loads at dword alignment, aligned dwordx4 stores
//   2 channels    the frames both of whose samples are in the tile, cut at row 0's address: a unit is 8 frames = four
//                 dwordx4 loads at dword alignment and 8 floats to each of the two rows (row 0 aligned, row 1 at whatever
//                 phase `frames` leaves it: dword-aligned dwordx4).  Head and tail frames go one float per lane, and so
//                 do the half frames a run or a tile may begin and end with.
//   3 or more     up to 64 channels: a uniform loop over the rows, lanes over the row's frames of the tile (strided reads,
//                 contiguous stores); more than 64: a tile holds a frame or two, so a loop over frames, lanes over rows
// Interior stores are non-temporal (the tensor is read by another kernel much later).  No word is read back, and nothing
// but the elements a span names is written: spans may write neighbouring floats of one row, and a slab's neighbours may
// be foreign data.  No LDS.
//
// Bounds: every span is checked on the host before the launch (check_spans below); the kernel relies on it -- a copy
// span reads floats [in_off, in_off + count) only and writes rows k < out_channels at t in [0, frames) only.
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_WAV_TILE_SAMPLES;
constexpr uint32_t kUnit = 16;                                  // floats per lane (1 channel, zero run); 8 frames of 2 channels
static_assert(kTile == kThreads * kUnit, "a tile is one unit per lane");
constexpr uint64_t kMaxIndex = (uint64_t)1 << 62;               // sample0 and count stay below it ...
constexpr int64_t kMaxFrame = (int64_t)1 << 61;                 // ... and |first_frame| below this: no sum or doubling in the kernel wraps

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a dwordx4 at dword alignment

__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// floats from p to the next 16-byte boundary, n at the most
__device__ __forceinline__ uint32_t head_of(const uint32_t *p, uint32_t n)
{
    return min((0u - (uint32_t)((uintptr_t)p >> 2)) & 3u, n);
}

// n <= 4096 zero floats from dst on
__device__ __forceinline__ void zero_tile(uint32_t *dst, uint32_t n)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t h = head_of(dst, n), units = (n - h) / kUnit, tail0 = h + units * kUnit, edge = h + (n - tail0);
    if (lane < units) {
        u32x4 *o = (u32x4 *)(dst + h + lane * kUnit);
        const u32x4 z = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (int k = 0; k < 4; k++) __builtin_nontemporal_store(z, o + k);
    }
    if (lane < edge) dst[lane < h ? lane : tail0 + (lane - h)] = 0u;
}

// n <= 4096 words from src to dst
__device__ __forceinline__ void copy1_tile(const uint32_t *src, uint32_t *dst, uint32_t n)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t h = head_of(dst, n), units = (n - h) / kUnit, tail0 = h + units * kUnit, edge = h + (n - tail0);
    if (lane < units) {
        const u32x4u *s = (const u32x4u *)(src + h + lane * kUnit);
        u32x4 *o = (u32x4 *)(dst + h + lane * kUnit);
        u32x4 w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = s[k];
#pragma unroll
        for (int k = 0; k < 4; k++) __builtin_nontemporal_store(w[k], o + k);
    }
    if (lane < edge) {
        const uint32_t j = lane < h ? lane : tail0 + (lane - h);
        dst[j] = src[j];
    }
}

// nf <= 2048 whole stereo frames from src (channel 0 of the first one) to row0 and -- unless NULL -- row1
__device__ __forceinline__ void copy2_tile(const uint32_t *src, uint32_t *row0, uint32_t *row1, uint32_t nf)
{
    constexpr uint32_t kFrames = kUnit / 2;
    const uint32_t lane = threadIdx.x;
    const uint32_t h = head_of(row0, nf), units = (nf - h) / kFrames, tail0 = h + units * kFrames, edge = h + (nf - tail0);
    if (lane < units) {
        const uint32_t f = h + lane * kFrames;
        const u32x4u *s = (const u32x4u *)(src + 2 * f);
        u32x4 w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = s[k];
        const u32x4 a0 = { w[0].x, w[0].z, w[1].x, w[1].z }, a1 = { w[2].x, w[2].z, w[3].x, w[3].z };
        u32x4 *o0 = (u32x4 *)(row0 + f);
        __builtin_nontemporal_store(a0, o0);
        __builtin_nontemporal_store(a1, o0 + 1);
        if (row1) {
            const u32x4u b0 = { w[0].y, w[0].w, w[1].y, w[1].w }, b1 = { w[2].y, w[2].w, w[3].y, w[3].w };
            u32x4u *o1 = (u32x4u *)(row1 + f);
            __builtin_nontemporal_store(b0, o1);
            __builtin_nontemporal_store(b1, o1 + 1);
        }
    }
    if (lane < 2 * edge) {                                       // head and tail frames: one float per lane
        const uint32_t j = lane >> 1, c = lane & 1u;
        const uint32_t f = j < h ? j : tail0 + (j - h);
        if (c == 0) row0[f] = src[2 * f];
        else if (row1) row1[f] = src[2 * f + 1];
    }
}

__global__ __launch_bounds__(kThreads) void collate_kernel(uint32_t n_spans, const afg_collate_span *__restrict__ spans,
                                                           const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    const uint64_t t = blockIdx.x;
    // the span of tile t: the last one whose first tile is <= t (spans without samples have no tiles)
    const uint32_t lo = afg::last_at_or_before(spans, n_spans, t, &afg_collate_span::first_tile);
    const afg_collate_span sp = spans[lo];
    if (sp.first_tile > t) return;
    const uint64_t s0 = (t - sp.first_tile) * kTile;             // first sample of the tile within the span
    if (s0 >= sp.count) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, sp.count - s0);
    if (sp.channels == 0) {
        zero_tile(out + sp.out_off + sp.sample0 + s0, n);
        return;
    }
    const uint32_t lane = threadIdx.x;
    const uint32_t ch = sp.channels, rows = min(ch, (uint32_t)sp.out_channels), T = sp.frames;
    const int64_t S0 = (int64_t)(sp.sample0 + s0), S1 = S0 + n;  // the tile's samples, counted in the file
    const int64_t ff = sp.first_frame, fe = ff + (int64_t)T;     // the file frames of the row
    const uint32_t *src = in + sp.in_off + s0;                   // sample S0
    uint32_t *slab = out + sp.out_off;
    if (ch == 1) {
        const int64_t a = max64(S0, ff), b = min64(S1, fe);
        if (a < b) copy1_tile(src + (a - S0), slab + (a - ff), (uint32_t)(b - a));
        return;
    }
    if (ch == 2) {
        const int64_t a = max64(S0, 2 * ff), b = min64(S1, 2 * fe);  // the samples whose frame is in the row
        if (a >= b) return;
        const int64_t f0 = (a + 1) >> 1, f1 = b >> 1;            // the frames that are whole in [a, b)
        if (lane == 0 && (a & 1) && rows > 1) slab[(uint64_t)T + (uint64_t)((a >> 1) - ff)] = src[a - S0];     // a leading channel 1
        if (lane == 1 && (b & 1)) slab[(b >> 1) - ff] = src[b - 1 - S0];                                       // a trailing channel 0
        if (f1 > f0) copy2_tile(src + (2 * f0 - S0), slab + (f0 - ff), rows > 1 ? slab + T + (f0 - ff) : nullptr, (uint32_t)(f1 - f0));
        return;
    }
    // the one division: S0 = q0 * ch + r0; the tile's end follows from a 32-bit one
    const int64_t q0 = (int64_t)((uint64_t)S0 / ch);
    const uint32_t r0 = (uint32_t)((uint64_t)S0 - (uint64_t)q0 * ch);
    const uint32_t x = r0 + n, qx = x / ch, r1 = x - qx * ch;
    const int64_t q1 = q0 + qx;                                  // S1 = q1 * ch + r1
    if (ch <= 64) {
        for (uint32_t k = 0; k < rows; k++) {                    // row k has frames [q0 + (k < r0), q1 + (k < r1)) of the tile
            const int64_t a = max64(q0 + (k < r0 ? 1 : 0), ff), b = min64(q1 + (k < r1 ? 1 : 0), fe);
            uint32_t *row = slab + (uint64_t)k * T;
            for (int64_t f = a + lane; f < b; f += kThreads)
                __builtin_nontemporal_store(src[f * (int64_t)ch + k - S0], row + (f - ff));
        }
        return;
    }
    const int64_t a = max64(q0, ff), b = min64(q1 + (r1 ? 1 : 0), fe);
    for (int64_t f = a; f < b; f++)
        for (uint32_t k = lane; k < rows; k += kThreads) {
            const int64_t s = f * (int64_t)ch + k;
            if (s >= S0 && s < S1) slab[(uint64_t)k * T + (uint64_t)(f - ff)] = src[s - S0];
        }
}

// every span against the planes and the tile table, before anything runs
int check_spans(const afg_collate_span *sp, uint64_t n_spans, uint64_t n_tiles, bool have_in, uint64_t in_floats, uint64_t out_floats)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; k < n_spans; k++) {
        const afg_collate_span &s = sp[k];
        if (s.first_tile != tiles) {
            afg::set_error("afg_collate_hip: span %llu: first_tile %llu, afg_collate_layout gives %llu", (unsigned long long)k,
                           (unsigned long long)s.first_tile, (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        if (s.count >= kMaxIndex || s.sample0 >= kMaxIndex) {
            afg::set_error("afg_collate_hip: span %llu: count and sample0 must be below 2^62", (unsigned long long)k);
            return AFG_ERR_INVALID;
        }
        tiles += (s.count + kTile - 1) / kTile;
        if (s.channels == 0) {
            if (s.count && (s.out_off > out_floats || s.sample0 > out_floats - s.out_off || s.count > out_floats - s.out_off - s.sample0)) {
                afg::set_error("afg_collate_hip: span %llu: the zero run leaves the output (%llu floats)", (unsigned long long)k, (unsigned long long)out_floats);
                return AFG_ERR_INVALID;
            }
            continue;
        }
        if (s.frames == 0 || s.out_channels == 0) {
            afg::set_error("afg_collate_hip: span %llu: frames and out_channels must be at least 1", (unsigned long long)k);
            return AFG_ERR_INVALID;
        }
        if (s.first_frame <= -kMaxFrame || s.first_frame >= kMaxFrame) {
            afg::set_error("afg_collate_hip: span %llu: |first_frame| must be below 2^61", (unsigned long long)k);
            return AFG_ERR_INVALID;
        }
        if (s.count && (!have_in || !afg::rows_inside(s.in_off, 1, 0, s.count, in_floats))) {
            afg::set_error("afg_collate_hip: span %llu: the run leaves the input (%llu floats)", (unsigned long long)k, (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        const uint64_t slab = (uint64_t)s.out_channels * s.frames;        // < 2^48
        if (!afg::rows_inside(s.out_off, 1, 0, slab, out_floats)) {
            afg::set_error("afg_collate_hip: span %llu: the slab leaves the output (%llu floats)", (unsigned long long)k, (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
    }
    if (tiles != n_tiles) {
        afg::set_error("afg_collate_hip: n_tiles %llu, afg_collate_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// what can be said without the spans
int check_args(uint64_t n_spans, const afg_collate_span *d_spans, uint64_t n_tiles, const float *d_in, uint64_t in_floats, float *d_out)
{
    if (!d_spans || !d_out || (!d_in && in_floats)) {
        afg::set_error("afg_collate_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_collate_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_collate_hip", "spans", n_spans, n_tiles);
}

}  // namespace

int afg::collate_launch(const afg_collate_span *h_spans, uint64_t n_spans, const afg_collate_span *d_spans, uint64_t n_tiles,
                        const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, hipStream_t stream)
{
    if (n_spans == 0) return AFG_OK;
    if (int rc = check_args(n_spans, d_spans, n_tiles, d_in, in_floats, d_out)) return rc;
    if (int rc = check_spans(h_spans, n_spans, n_tiles, d_in != nullptr, in_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (int rc = afg::require_device()) return rc;
    hipLaunchKernelGGL(collate_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, stream, (uint32_t)n_spans, d_spans,
                       (const uint32_t *)d_in, (uint32_t *)d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" uint64_t afg_collate_layout(afg_collate_span *spans, uint64_t n_spans)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; spans && k < n_spans; k++) {
        spans[k].first_tile = tiles;
        tiles += (spans[k].count + kTile - 1) / kTile;
    }
    return tiles;
}

extern "C" int afg_collate_hip(uint64_t n_spans, const afg_collate_span *d_spans, uint64_t n_tiles, const float *d_in,
                               uint64_t in_floats, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (n_spans == 0) return AFG_OK;
    if (int rc = check_args(n_spans, d_spans, n_tiles, d_in, in_floats, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_spans, n_spans, (hipStream_t)hip_stream, [&](const afg_collate_span *h) {
        return afg::collate_launch(h, n_spans, d_spans, n_tiles, d_in, in_floats, d_out, out_floats, (hipStream_t)hip_stream);
    });
}
