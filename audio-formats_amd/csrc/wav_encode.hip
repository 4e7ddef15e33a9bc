// wav_encode.hip -- float32 to WAV sample bytes (WAVEncoder.writeSamples, wav.d:482-547, with TPDFDither.process,
// wav.d:679-700) for gfx950: the mirror image of wav_pcm.hip.
//
// Work: element-wise and memory-bound (4 bytes in, 1-8 bytes out per sample).  A launch packs any mix of spans
// (afg_wav_pack_span: a run of samples of one output file); its grid is one workgroup per tile of 4096 samples.  A
// workgroup finds its span by a search over the spans' first tiles (uniform: scalar loads), then every lane takes 4
// consecutive floats per step as one 16-byte word and stores their 4 (s8), 8 (s16), 12 (s24), 16 (fp32) or 2 x 16 (fp64)
// bytes as one access, consecutive lanes next to each other.  The last count % 4 samples of a span go one per lane.
//
// Arithmetic: the reference's, in double: x * scale and the add are separate operations (the build has no contraction),
// the cast truncates.  fp32 moves the 32 bits through integer registers; fp64 widens (v_cvt_f64_f32).
//
// Dither: scale, + 0.3125, + 0.25 * (r0 / rmax), + 0.125 * (r1 / rmax), floor, / scale, clamp -- the order of
// host/afg_wav.cpp, every division the IEEE fp64 division.  The draws come from the 31-bit LCG
// state = (state * 1103515245 + 12345) & 0x7fffffff; sample n of a file uses draws 2n and 2n + 1.  The LCG is an affine map
// modulo 2^31, and n steps of it are again one: x -> a_n * x + c_n.  A workgroup computes the map to its tile's first
// draw once, from uniform values (31 square-and-multiply steps on the scalar unit); a lane composes that state with
// entry `lane` of a constant table (the maps of 8 * lane draws: its four samples of step 0) and reaches the steps after
// it through three compile-time maps (2048 draws each).  Inside its four samples a lane steps the LCG eight times.
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_WAV_TILE_SAMPLES;               // samples per workgroup: 4 steps of 4 samples per lane
constexpr uint32_t kSteps = kTile / (kThreads * 4);
static_assert(kTile % (kThreads * 4) == 0, "a tile is whole steps");
static_assert((kTile * 3) % 16 == 0, "s24 tiles start on 16-byte boundaries");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
struct alignas(4) u32x3 { uint32_t a, b, c; };

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
    for (int l = 0; l < kThreads; l++) t.at[l] = jump_of(8u * (uint32_t)l);
    return t;
}
__constant__ LaneJumps kLaneJumps = make_lane_jumps();          // 2 KB
constexpr uint32_t kStepDraws = 8u * kThreads;                   // draws between a lane's samples of consecutive steps

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

template <int F> struct Fmt;
template <> struct Fmt<AFG_WAV_S8> {
    static constexpr uint32_t bytes = 1;
    static constexpr double scale = 127.0;
    static __device__ __forceinline__ uint32_t one(double x) { return (uint32_t)(int)(128.5 + x * 127.0) & 0xffu; }          // wav.d:486-487
    static __device__ __forceinline__ void four(uint8_t *p, const uint32_t (&q)[4])
    {
        __builtin_nontemporal_store(q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24), (uint32_t *)p);
    }
};
template <> struct Fmt<AFG_WAV_S16LE> {
    static constexpr uint32_t bytes = 2;
    static constexpr double scale = 32767.0;
    static __device__ __forceinline__ uint32_t one(double x) { return (uint32_t)((int)(32768.5 + x * 32767.0) - 32768) & 0xffffu; }   // :501-502
    static __device__ __forceinline__ void four(uint8_t *p, const uint32_t (&q)[4])
    {
        __builtin_nontemporal_store(u32x2{ q[0] | (q[1] << 16), q[2] | (q[3] << 16) }, (u32x2 *)p);
    }
};
template <> struct Fmt<AFG_WAV_S24LE> {
    static constexpr uint32_t bytes = 3;
    static constexpr double scale = 8388607.0;
    static __device__ __forceinline__ uint32_t one(double x) { return (uint32_t)((int)(8388608.5 + x * 8388607.0) - 8388608) & 0xffffffu; }   // :517-518
    static __device__ __forceinline__ void four(uint8_t *p, const uint32_t (&q)[4])
    {
        *(u32x3 *)p = u32x3{ q[0] | (q[1] << 24), (q[1] >> 8) | (q[2] << 16), (q[2] >> 16) | (q[3] << 8) };   // 12 bytes = 4 samples
    }
};

// samples [0, n) of a tile of an integer format: src / dst point at its first sample, `base` is the generator's state
// before the tile's first draw
template <int F, bool D> __device__ __forceinline__ void pack_tile(const float *src, uint8_t *dst, uint32_t n, uint32_t base)
{
    typedef Fmt<F> T;
    const uint32_t lane = threadIdx.x, groups = n >> 2;
    uint32_t lane_state = 0;
    if (D) lane_state = apply(kLaneJumps.at[lane], base);
    constexpr Jump step_jump[4] = { jump_of(0), jump_of(kStepDraws), jump_of(2 * kStepDraws), jump_of(3 * kStepDraws) };
    static_assert(kSteps == 4, "one compile-time map per step");
#pragma unroll
    for (uint32_t step = 0; step < kSteps; step++) {
        const uint32_t g = step * kThreads + lane;
        if (g < groups) {
            const u32x4 w = __builtin_nontemporal_load((const u32x4 *)src + g);
            const float x[4] = { __uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w) };
            uint32_t state = apply(step_jump[step], lane_state), q[4];
#pragma unroll
            for (int j = 0; j < 4; j++) q[j] = T::one(D ? dither_one((double)x[j], T::scale, state) : (double)x[j]);
            T::four(dst + (size_t)g * 4 * T::bytes, q);
        }
    }
    // the tail: the last n % 4 samples, one per lane
    if (lane < (n & 3u)) {
        const uint32_t i = groups * 4 + lane;
        uint32_t state = 0;
        if (D) {
            state = apply(step_jump[(groups >> 8) & 3u], apply(kLaneJumps.at[groups & (kThreads - 1)], base));
            for (uint32_t k = 0; k < 2 * lane; k++) (void)next_draw(state);
        }
        const double x = (double)src[i];
        const uint32_t q = T::one(D ? dither_one(x, T::scale, state) : x);
        uint8_t *p = dst + (size_t)i * T::bytes;
        p[0] = (uint8_t)q;
        if (T::bytes > 1) p[1] = (uint8_t)(q >> 8);
        if (T::bytes > 2) p[2] = (uint8_t)(q >> 16);
    }
}

// fp32: the bits as they are; fp64: widened
template <bool Wide> __device__ __forceinline__ void move_tile(const float *src, uint8_t *dst, uint32_t n)
{
    const uint32_t lane = threadIdx.x, groups = n >> 2;
#pragma unroll
    for (uint32_t step = 0; step < kSteps; step++) {
        const uint32_t g = step * kThreads + lane;
        if (g < groups) {
            const u32x4 w = __builtin_nontemporal_load((const u32x4 *)src + g);
            if (!Wide) {
                __builtin_nontemporal_store(w, (u32x4 *)dst + g);
            } else {
                __builtin_nontemporal_store(f64x2{ (double)__uint_as_float(w.x), (double)__uint_as_float(w.y) }, (f64x2 *)dst + 2 * (size_t)g);
                __builtin_nontemporal_store(f64x2{ (double)__uint_as_float(w.z), (double)__uint_as_float(w.w) }, (f64x2 *)dst + 2 * (size_t)g + 1);
            }
        }
    }
    if (lane < (n & 3u)) {
        const uint32_t i = groups * 4 + lane;
        if (!Wide) ((uint32_t *)dst)[i] = ((const uint32_t *)src)[i];
        else ((double *)dst)[i] = (double)src[i];
    }
}

__device__ __forceinline__ uint32_t bytes_of(uint32_t format)
{
    return format == AFG_WAV_S8 ? 1u : format == AFG_WAV_S16LE ? 2u : format == AFG_WAV_S24LE ? 3u : format == AFG_WAV_FP32LE ? 4u : 8u;
}

__global__ __launch_bounds__(kThreads) void wav_pack_kernel(uint32_t n_spans, const afg_wav_pack_span *__restrict__ spans,
                                                            const float *__restrict__ in, uint64_t in_floats,
                                                            uint8_t *__restrict__ out, uint64_t out_bytes)
{
    const uint64_t t = blockIdx.x;
    // the span of tile t: the last one whose first tile is <= t (spans without samples have no tiles)
    const uint32_t lo = afg::last_at_or_before(spans, n_spans, t, &afg_wav_pack_span::first_tile);
    const afg_wav_pack_span sp = spans[lo];
    if (sp.first_tile > t || sp.format > AFG_WAV_FP64LE) return;
    const uint64_t s0 = (t - sp.first_tile) * kTile;             // first sample of the tile within the span
    if (s0 >= sp.count) return;
    const uint32_t bytes = bytes_of(sp.format);
    // a span that leaves the planes, or is not aligned for the 16-byte accesses, is not touched (counts are bounded
    // first, so that the products cannot wrap)
    if (((sp.in_off & 3u) | (sp.out_off & 15u)) != 0) return;
    if (sp.count > in_floats || sp.in_off > in_floats - sp.count) return;
    if (sp.count > out_bytes / bytes || sp.out_off > out_bytes - sp.count * bytes) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, sp.count - s0);
    const float *src = in + sp.in_off + s0;
    uint8_t *dst = out + sp.out_off + s0 * bytes;
    if (sp.format == AFG_WAV_FP32LE) { move_tile<false>(src, dst, n); return; }
    if (sp.format == AFG_WAV_FP64LE) { move_tile<true>(src, dst, n); return; }
    if (!sp.dither) {
        switch (sp.format) {
        case AFG_WAV_S8: pack_tile<AFG_WAV_S8, false>(src, dst, n, 0); break;
        case AFG_WAV_S16LE: pack_tile<AFG_WAV_S16LE, false>(src, dst, n, 0); break;
        default: pack_tile<AFG_WAV_S24LE, false>(src, dst, n, 0); break;
        }
        return;
    }
    // the generator's state before the tile's first draw: uniform over the workgroup
    const uint32_t base = apply(jump_of(sp.draw0 + 2 * s0), sp.seed & kMask);
    switch (sp.format) {
    case AFG_WAV_S8: pack_tile<AFG_WAV_S8, true>(src, dst, n, base); break;
    case AFG_WAV_S16LE: pack_tile<AFG_WAV_S16LE, true>(src, dst, n, base); break;
    default: pack_tile<AFG_WAV_S24LE, true>(src, dst, n, base); break;
    }
}

}  // namespace

extern "C" uint32_t afg_lcg31_jump(uint32_t seed, uint64_t n_draws) { return apply(jump_of(n_draws), seed & kMask); }

extern "C" uint64_t afg_wav_pack_layout(afg_wav_pack_span *spans, uint64_t n_spans)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; spans && k < n_spans; k++) {
        spans[k].first_tile = tiles;
        tiles += (spans[k].count + kTile - 1) / kTile;
    }
    return tiles;
}

extern "C" int afg_wav_pack_hip(uint64_t n_spans, const afg_wav_pack_span *d_spans, uint64_t n_tiles, const float *d_in,
                                uint64_t in_floats, uint8_t *d_out, uint64_t out_bytes, void *hip_stream)
{
    if (n_spans == 0 || n_tiles == 0) return AFG_OK;
    if (!d_spans || !d_in || !d_out) {
        afg::set_error("afg_wav_pack_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if ((((uintptr_t)d_in | (uintptr_t)d_out) & 15u) != 0) {
        afg::set_error("afg_wav_pack_hip: the planes must be 16-byte aligned");
        return AFG_ERR_INVALID;
    }
    if (int rc = afg::launch_caps("afg_wav_pack_hip", "spans", n_spans, n_tiles)) return rc;
    if (int rc = afg::require_device()) return rc;
    hipLaunchKernelGGL(wav_pack_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, (hipStream_t)hip_stream, (uint32_t)n_spans,
                       d_spans, d_in, in_floats, d_out, out_bytes);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
