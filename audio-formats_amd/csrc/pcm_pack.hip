// pcm_pack.hip -- float32 planes of a batch decode stage to packed integer PCM (the bytes of WAVEncoder.writeSamples,
// wav.d:482-527, with TPDFDither.process, wav.d:679-700, in front when asked for) for gfx950.
//
// wav_encode.hip's arithmetic without its alignment rules: a span (afg_pcm_pack_span) starts at any float of the input
// and at any byte of the output, because a file's samples start wherever the decode stage left them in its plane.  The
// conversion expressions and the generator below are those of wav_encode.hip, kept word for word (that file is the
// write stream's and the batch encoder's and stays as it is).
//
// Work: element-wise and memory-bound (4 bytes in, 1-3 bytes out per sample).  One workgroup of 256 lanes per tile of
// 4096 samples of one span, found by a search over the spans' first tiles (uniform per workgroup: scalar loads).  The
// tile's output bytes [b0, b1) are cut at the 16-byte boundaries of the output *address*:
//   head      [b0, a)            a = b0 rounded up to 16 bytes: up to 15 bytes
//   interior  [a, a + U * 16 B)  U units of 16 samples = B aligned 16-byte words each (B bytes per sample), one unit per lane
//   tail      the rest           fewer than 16 B bytes
// A tile is 4096 B bytes, a multiple of 16, so every tile of a span has the same head length h.  A unit starts r = h % B
// bytes into a sample: its lane converts the 16 samples it covers, and a 17th when r != 0 (the lane after it converts
// that sample again: a sample's bytes depend on nothing but its value and its index in the file), packs them tight into
// dwords and moves the byte window by r with v_alignbyte_b32.  Loads are dwordx4 at 4-byte alignment, stores are aligned
// dwordx4.  Head and tail go one *byte* per lane: the lane converts the sample its byte belongs to and stores that byte,
// so no word is ever read back and two spans -- or a span and foreign bytes -- may share a dword.  No LDS.
//
// Input: NaN becomes 0, everything else is clamped to [-1, 1] first (decoded audio overshoots; the reference asserts).
// Dither: sample n of a file uses draws draw0 + 2n and draw0 + 2n + 1 of the 31-bit LCG.  n steps of it are one affine
// map; a workgroup computes the map to its first unit's first draw from uniform values, a lane composes it with entry
// `lane` of a constant table (32 draws per unit) and steps from there.  A byte lane jumps straight to its sample.
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_WAV_TILE_SAMPLES;
constexpr uint32_t kUnit = 16;                                  // samples per lane
static_assert(kTile == kThreads * kUnit, "a tile is one unit per lane");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a dwordx4 at dword alignment

constexpr uint32_t kMul = 1103515245u, kAdd = 12345u, kMask = 0x7fffffffu;
constexpr double kRandMax = 2147483647.0;

struct Jump { uint32_t a, c; };                                 // x -> (a * x + c) mod 2^31
__host__ __device__ constexpr Jump then(Jump f, Jump g)         // f first, g after it
{
    return Jump{ (g.a * f.a) & kMask, (g.a * f.c + g.c) & kMask };
}
__host__ __device__ constexpr Jump jump_of(uint64_t draws)
{
    Jump r{ 1u, 0u }, p{ kMul, kAdd };
    draws &= kMask;                                              // the generator has period 2^31
    for (; draws; draws >>= 1) {
        if (draws & 1) r = then(r, p);
        p = then(p, p);
    }
    return r;
}
__host__ __device__ constexpr uint32_t apply(Jump j, uint32_t state) { return (j.a * state + j.c) & kMask; }

struct LaneJumps { Jump at[kThreads]; };
constexpr LaneJumps make_lane_jumps()
{
    LaneJumps t{};
    for (int l = 0; l < kThreads; l++) t.at[l] = jump_of(2u * kUnit * (uint32_t)l);
    return t;
}
__constant__ LaneJumps kUnitJumps = make_lane_jumps();          // 2 KB

__device__ __forceinline__ uint32_t next_draw(uint32_t &state)
{
    state = (state * kMul + kAdd) & kMask;
    return state;
}

// TPDFDither.process for one sample; two draws, in this order
__device__ __forceinline__ double dither_one(double x, double scale, uint32_t &state)
{
    x *= scale;
    x += 0.3125;                                                 // 0.5 - 0.5 * (TUNE0 + TUNE1)
    x += 0.25 * ((double)(int32_t)next_draw(state) / kRandMax);
    x += 0.125 * ((double)(int32_t)next_draw(state) / kRandMax);
    x = __builtin_floor(x);
    x /= scale;
    if (x < -1.0) x = -1.0;
    if (x > 1.0) x = 1.0;
    return x;
}

// what this kernel adds in front: NaN -> 0, then [-1, 1]
__device__ __forceinline__ double in_range(uint32_t bits)
{
    float x = __uint_as_float(bits);
    if (x != x) x = 0.0f;
    if (x < -1.0f) x = -1.0f;
    if (x > 1.0f) x = 1.0f;
    return (double)x;
}

template <int F> struct Fmt;
template <> struct Fmt<AFG_WAV_S8> {
    static constexpr uint32_t bytes = 1;
    static constexpr double scale = 127.0;
    static __device__ __forceinline__ uint32_t one(double x) { return (uint32_t)(int)(128.5 + x * 127.0) & 0xffu; }          // wav.d:486-487
    // samples q[4k .. 4k + 3] as dword k
    static __device__ __forceinline__ void pack(const uint32_t (&q)[kUnit + 1], uint32_t (&p)[4 * bytes + 1])
    {
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = q[4 * k] | (q[4 * k + 1] << 8) | (q[4 * k + 2] << 16) | (q[4 * k + 3] << 24);
        p[4] = q[16];
    }
};
template <> struct Fmt<AFG_WAV_S16LE> {
    static constexpr uint32_t bytes = 2;
    static constexpr double scale = 32767.0;
    static __device__ __forceinline__ uint32_t one(double x) { return (uint32_t)((int)(32768.5 + x * 32767.0) - 32768) & 0xffffu; }   // :501-502
    static __device__ __forceinline__ void pack(const uint32_t (&q)[kUnit + 1], uint32_t (&p)[4 * bytes + 1])
    {
#pragma unroll
        for (int k = 0; k < 8; k++) p[k] = q[2 * k] | (q[2 * k + 1] << 16);
        p[8] = q[16];
    }
};
template <> struct Fmt<AFG_WAV_S24LE> {
    static constexpr uint32_t bytes = 3;
    static constexpr double scale = 8388607.0;
    static __device__ __forceinline__ uint32_t one(double x) { return (uint32_t)((int)(8388608.5 + x * 8388607.0) - 8388608) & 0xffffffu; }   // :517-518
    static __device__ __forceinline__ void pack(const uint32_t (&q)[kUnit + 1], uint32_t (&p)[4 * bytes + 1])
    {
#pragma unroll
        for (int k = 0; k < 4; k++) {                            // 4 samples = 12 bytes = 3 dwords
            p[3 * k] = q[4 * k] | (q[4 * k + 1] << 24);
            p[3 * k + 1] = (q[4 * k + 1] >> 8) | (q[4 * k + 2] << 16);
            p[3 * k + 2] = (q[4 * k + 2] >> 16) | (q[4 * k + 3] << 8);
        }
        p[12] = q[16];
    }
};

// One tile of an integer format.  src: its first float; dst: its first byte; n: its samples; seed / draw: the generator's
// start state and the index of the draw that the tile's first sample begins with.
template <int F, bool D> __device__ __forceinline__ void pack_tile(const uint32_t *src, uint8_t *dst, uint32_t n, uint32_t seed, uint64_t draw)
{
    typedef Fmt<F> T;
    constexpr uint32_t B = T::bytes, kUnitBytes = kUnit * B;
    const uint32_t lane = threadIdx.x;
    const uint32_t nb = n * B;                                                   // bytes of the tile
    const uint32_t h = min((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u, nb);  // head
    const uint32_t hq = h / B, r = h % B;                                        // whole samples of the head, bytes of the one it splits
    const uint32_t units = (nb - h) / kUnitBytes;
    const uint32_t tail0 = h + units * kUnitBytes, edge = h + (nb - tail0);      // the tail's first byte; head + tail bytes
    if (lane < units) {
        const uint32_t i0 = hq + lane * kUnit;
        const uint32_t *s = src + i0;
        u32x4 w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = *((const u32x4u *)s + k);
        uint32_t last = 0;
        if (r) last = s[kUnit];                                  // (a sample of the tile: some of its bytes are in this unit)
        uint32_t state = 0;
        if (D) state = apply(kUnitJumps.at[lane], apply(jump_of(draw + 2 * (uint64_t)hq), seed));   // (the inner map is uniform)
        uint32_t q[kUnit + 1];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t x[4] = { w[k].x, w[k].y, w[k].z, w[k].w };
#pragma unroll
            for (int j = 0; j < 4; j++) q[4 * k + j] = T::one(D ? dither_one(in_range(x[j]), T::scale, state) : in_range(x[j]));
        }
        q[kUnit] = 0;
        if (r) q[kUnit] = T::one(D ? dither_one(in_range(last), T::scale, state) : in_range(last));
        uint32_t p[4 * B + 1];
        T::pack(q, p);
        u32x4 *o = (u32x4 *)(dst + h + (size_t)lane * kUnitBytes);
#pragma unroll
        for (uint32_t k = 0; k < B; k++) {
            u32x4 v;
            v.x = __builtin_amdgcn_alignbyte(p[4 * k + 1], p[4 * k], r);
            v.y = __builtin_amdgcn_alignbyte(p[4 * k + 2], p[4 * k + 1], r);
            v.z = __builtin_amdgcn_alignbyte(p[4 * k + 3], p[4 * k + 2], r);
            v.w = __builtin_amdgcn_alignbyte(p[4 * k + 4], p[4 * k + 3], r);
            __builtin_nontemporal_store(v, o + k);
        }
    }
    // head and tail: one byte per lane, nothing read back
    if (lane < edge) {
        const uint32_t b = lane < h ? lane : tail0 + (lane - h);
        const uint32_t i = b / B;
        uint32_t state = 0;
        if (D) state = apply(jump_of(draw + 2 * (uint64_t)i), seed);
        const double x = in_range(src[i]);
        const uint32_t v = T::one(D ? dither_one(x, T::scale, state) : x);
        dst[b] = (uint8_t)(v >> (8 * (b - i * B)));
    }
}

__global__ __launch_bounds__(kThreads) void pcm_pack_kernel(uint32_t n_spans, const afg_pcm_pack_span *__restrict__ spans,
                                                            const uint32_t *__restrict__ in, uint64_t in_floats,
                                                            uint8_t *__restrict__ out, uint64_t out_bytes)
{
    const uint64_t t = blockIdx.x;
    // the span of tile t: the last one whose first tile is <= t (spans without samples have no tiles)
    const uint32_t lo = afg::last_at_or_before(spans, n_spans, t, &afg_pcm_pack_span::first_tile);
    const afg_pcm_pack_span sp = spans[lo];
    if (sp.first_tile > t || sp.format > AFG_WAV_S24LE) return;
    const uint64_t s0 = (t - sp.first_tile) * kTile;             // first sample of the tile within the span
    if (s0 >= sp.count) return;
    const uint32_t bytes = sp.format == AFG_WAV_S8 ? 1u : sp.format == AFG_WAV_S16LE ? 2u : 3u;
    // a span that leaves the planes is not touched (counts are bounded first, so that the products cannot wrap)
    if (sp.count > in_floats || sp.in_off > in_floats - sp.count) return;
    if (sp.count > out_bytes / bytes || sp.out_off > out_bytes - sp.count * bytes) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, sp.count - s0);
    const uint32_t *src = in + sp.in_off + s0;
    uint8_t *dst = out + sp.out_off + s0 * bytes;
    const uint32_t seed = sp.seed & kMask;
    const uint64_t draw = sp.draw0 + 2 * s0;
    if (!sp.dither) {
        switch (sp.format) {
        case AFG_WAV_S8: pack_tile<AFG_WAV_S8, false>(src, dst, n, 0, 0); break;
        case AFG_WAV_S16LE: pack_tile<AFG_WAV_S16LE, false>(src, dst, n, 0, 0); break;
        default: pack_tile<AFG_WAV_S24LE, false>(src, dst, n, 0, 0); break;
        }
        return;
    }
    switch (sp.format) {
    case AFG_WAV_S8: pack_tile<AFG_WAV_S8, true>(src, dst, n, seed, draw); break;
    case AFG_WAV_S16LE: pack_tile<AFG_WAV_S16LE, true>(src, dst, n, seed, draw); break;
    default: pack_tile<AFG_WAV_S24LE, true>(src, dst, n, seed, draw); break;
    }
}

}  // namespace

extern "C" uint64_t afg_pcm_pack_layout(afg_pcm_pack_span *spans, uint64_t n_spans)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; spans && k < n_spans; k++) {
        spans[k].first_tile = tiles;
        tiles += (spans[k].count + kTile - 1) / kTile;
    }
    return tiles;
}

extern "C" int afg_pcm_pack_hip(uint64_t n_spans, const afg_pcm_pack_span *d_spans, uint64_t n_tiles, const float *d_in,
                                uint64_t in_floats, uint8_t *d_out, uint64_t out_bytes, void *hip_stream)
{
    if (n_spans == 0 || n_tiles == 0) return AFG_OK;
    if (!d_spans || !d_in || !d_out) {
        afg::set_error("afg_pcm_pack_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0) {
        afg::set_error("afg_pcm_pack_hip: the input plane must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    if (int rc = afg::launch_caps("afg_pcm_pack_hip", "spans", n_spans, n_tiles)) return rc;
    if (int rc = afg::require_device()) return rc;
    hipLaunchKernelGGL(pcm_pack_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, (hipStream_t)hip_stream, (uint32_t)n_spans,
                       d_spans, (const uint32_t *)d_in, in_floats, d_out, out_bytes);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
