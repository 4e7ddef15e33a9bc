// wav_pcm.hip -- WAV sample conversion (WAVDecoder.readSamples!float, wav.d:242-344) for gfx950.
//
// Work: element-wise and memory-bound (1-8 bytes in, 4 bytes out per sample).  A launch converts any mix of spans
// (afg_wav_span: a run of samples of one kind); its grid is one workgroup per tile of 4096 output samples, so a long file
// and a short one load the device in proportion to their length.  A workgroup finds its span by a search over the
// spans' first tiles (uniform per workgroup: scalar loads), then every lane converts 4 consecutive samples per step and
// stores them as one 16-byte word, consecutive lanes next to each other; the loads that feed a store are 4 (u8), 8 (s16),
// 12 (s24), 16 (s32, f32) or 2 x 16 (f64) bytes per lane, consecutive as well.  The last count % 4 samples of a span, and
// all of a span whose base is not aligned for those loads and stores, go one sample per lane from single bytes.
//
// Arithmetic: the reference divides in double and narrows to float.  For u8 / s16 / s24 a correctly rounded float32
// division gives the same bits for every input (checked exhaustively: tests/test_wav_gpu.py); multiplying by a float32
// reciprocal does not.  The build has neither fast-math nor a relaxed division, so `/` is the IEEE division
// (v_div_scale / v_div_fmas / v_div_fixup).  s32: int-to-float conversion rounds once and the scale by 2^-31 is exact.
// f32: the 32 bits are moved as an integer, so NaN payloads survive.  f64: v_cvt_f32_f64 (round to nearest even,
// denormal results kept).
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_WAV_TILE_SAMPLES;               // samples per workgroup: 4 steps of 4 samples per lane
static_assert(kTile % (kThreads * 4) == 0, "a tile is whole steps");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
struct alignas(4) u32x3 { uint32_t a, b, c; };

__device__ __forceinline__ float from_u8(uint32_t b) { return (float)((int32_t)b - 128) / 127.0f; }
__device__ __forceinline__ float from_s16(uint32_t v) { return (float)(int32_t)(int16_t)v / 32767.0f; }
__device__ __forceinline__ float from_s24(uint32_t v) { return (float)((int32_t)(v << 8) >> 8) / 8388607.0f; }
__device__ __forceinline__ float from_s32(uint32_t v) { return (float)(int32_t)v * 0x1p-31f; }

template <int K> struct Kind;
template <> struct Kind<AFG_WAV_KIND_U8> {
    static constexpr uint32_t bytes = 1, align = 4;
    static __device__ __forceinline__ f32x4 four(const uint8_t *p)
    {
        const uint32_t w = __builtin_nontemporal_load((const uint32_t *)p);
        return f32x4{ from_u8(w & 255u), from_u8((w >> 8) & 255u), from_u8((w >> 16) & 255u), from_u8(w >> 24) };
    }
    static __device__ __forceinline__ uint32_t one(const uint8_t *p) { return __float_as_uint(from_u8(p[0])); }
};
template <> struct Kind<AFG_WAV_KIND_S16> {
    static constexpr uint32_t bytes = 2, align = 8;
    static __device__ __forceinline__ f32x4 four(const uint8_t *p)
    {
        const u32x2 w = __builtin_nontemporal_load((const u32x2 *)p);
        return f32x4{ from_s16(w.x & 0xffffu), from_s16(w.x >> 16), from_s16(w.y & 0xffffu), from_s16(w.y >> 16) };
    }
    static __device__ __forceinline__ uint32_t one(const uint8_t *p) { return __float_as_uint(from_s16((uint32_t)p[0] | ((uint32_t)p[1] << 8))); }
};
template <> struct Kind<AFG_WAV_KIND_S24> {
    static constexpr uint32_t bytes = 3, align = 4;
    static __device__ __forceinline__ f32x4 four(const uint8_t *p)
    {
        const u32x3 w = *(const u32x3 *)p;                      // 12 bytes = 4 samples
        return f32x4{ from_s24(w.a), from_s24((w.a >> 24) | (w.b << 8)), from_s24((w.b >> 16) | (w.c << 16)), from_s24(w.c >> 8) };
    }
    static __device__ __forceinline__ uint32_t one(const uint8_t *p)
    {
        return __float_as_uint(from_s24((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)));
    }
};
__device__ __forceinline__ uint32_t le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
template <> struct Kind<AFG_WAV_KIND_S32> {
    static constexpr uint32_t bytes = 4, align = 16;
    static __device__ __forceinline__ f32x4 four(const uint8_t *p)
    {
        const u32x4 w = __builtin_nontemporal_load((const u32x4 *)p);
        return f32x4{ from_s32(w.x), from_s32(w.y), from_s32(w.z), from_s32(w.w) };
    }
    static __device__ __forceinline__ uint32_t one(const uint8_t *p) { return __float_as_uint(from_s32(le32(p))); }
};
template <> struct Kind<AFG_WAV_KIND_F32> {
    static constexpr uint32_t bytes = 4, align = 16;
    static __device__ __forceinline__ f32x4 four(const uint8_t *p)
    {
        const u32x4 w = __builtin_nontemporal_load((const u32x4 *)p);
        return f32x4{ __uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w) };   // moves, no arithmetic
    }
    static __device__ __forceinline__ uint32_t one(const uint8_t *p) { return le32(p); }
};
template <> struct Kind<AFG_WAV_KIND_F64> {
    static constexpr uint32_t bytes = 8, align = 16;
    static __device__ __forceinline__ f32x4 four(const uint8_t *p)
    {
        const f64x2 a = __builtin_nontemporal_load((const f64x2 *)p), b = __builtin_nontemporal_load((const f64x2 *)p + 1);
        return f32x4{ (float)a.x, (float)a.y, (float)b.x, (float)b.y };
    }
    static __device__ __forceinline__ uint32_t one(const uint8_t *p)
    {
        const uint64_t bits = (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32);
        return __float_as_uint((float)__longlong_as_double((long long)bits));
    }
};

// samples [0, n) of a tile: src / dst point at its first sample
template <int K> __device__ __forceinline__ void convert_tile(const uint8_t *src, float *dst, uint32_t n)
{
    typedef Kind<K> T;
    const uint32_t lane = threadIdx.x;
    const bool fast = (((uintptr_t)src & (T::align - 1)) | ((uintptr_t)dst & 15)) == 0;
    const uint32_t groups = fast ? n >> 2 : 0;                   // whole 16-byte words of output
#pragma unroll
    for (uint32_t step = 0; step < kTile / (kThreads * 4); step++) {
        const uint32_t g = step * kThreads + lane;
        if (g < groups) __builtin_nontemporal_store(T::four(src + (size_t)g * 4 * T::bytes), (f32x4 *)dst + g);
    }
    // the tail, or everything when the tile cannot take the fast path (bits stored as integers: an f32 NaN keeps its payload)
    for (uint32_t i = groups * 4 + lane; i < n; i += kThreads) ((uint32_t *)dst)[i] = T::one(src + (size_t)i * T::bytes);
}

__global__ __launch_bounds__(kThreads) void wav_convert_kernel(uint32_t n_spans, const afg_wav_span *__restrict__ spans,
                                                               const uint8_t *__restrict__ in, uint64_t in_bytes,
                                                               float *__restrict__ out, uint64_t out_floats)
{
    const uint64_t t = blockIdx.x;
    // the span of tile t: the last one whose first tile is <= t (spans without samples have no tiles)
    const uint32_t lo = afg::last_at_or_before(spans, n_spans, t, &afg_wav_span::tile_first);
    const afg_wav_span sp = spans[lo];
    if (sp.tile_first > t || sp.kind > AFG_WAV_KIND_F64) return;
    const uint64_t s0 = (t - sp.tile_first) * kTile;             // first sample of the tile within the span
    if (s0 >= sp.count) return;
    const uint32_t bytes = sp.kind == AFG_WAV_KIND_U8 ? 1u : sp.kind == AFG_WAV_KIND_S16 ? 2u : sp.kind == AFG_WAV_KIND_S24 ? 3u
                           : sp.kind == AFG_WAV_KIND_F64 ? 8u : 4u;
    // a span that leaves the planes is not touched (counts are bounded first, so that the products cannot wrap)
    if (sp.count > out_floats || sp.out_off > out_floats - sp.count) return;
    if (sp.count > in_bytes / bytes || sp.in_off > in_bytes - sp.count * bytes) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, sp.count - s0);
    const uint8_t *src = in + sp.in_off + s0 * bytes;
    float *dst = out + sp.out_off + s0;
    switch (sp.kind) {
    case AFG_WAV_KIND_U8: convert_tile<AFG_WAV_KIND_U8>(src, dst, n); break;
    case AFG_WAV_KIND_S16: convert_tile<AFG_WAV_KIND_S16>(src, dst, n); break;
    case AFG_WAV_KIND_S24: convert_tile<AFG_WAV_KIND_S24>(src, dst, n); break;
    case AFG_WAV_KIND_S32: convert_tile<AFG_WAV_KIND_S32>(src, dst, n); break;
    case AFG_WAV_KIND_F32: convert_tile<AFG_WAV_KIND_F32>(src, dst, n); break;
    default: convert_tile<AFG_WAV_KIND_F64>(src, dst, n); break;
    }
}

}  // namespace

extern "C" uint64_t afg_wav_layout(afg_wav_span *spans, uint64_t n_spans)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; spans && k < n_spans; k++) {
        spans[k].tile_first = tiles;
        tiles += (spans[k].count + kTile - 1) / kTile;
    }
    return tiles;
}

extern "C" int afg_wav_convert_hip(uint64_t n_spans, const afg_wav_span *d_spans, uint64_t n_tiles, const uint8_t *d_in,
                                   uint64_t in_bytes, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (n_spans == 0 || n_tiles == 0) return AFG_OK;
    if (!d_spans || !d_in || !d_out) {
        afg::set_error("afg_wav_convert_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (int rc = afg::launch_caps("afg_wav_convert_hip", "spans", n_spans, n_tiles)) return rc;
    if (int rc = afg::require_device()) return rc;
    hipLaunchKernelGGL(wav_convert_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, (hipStream_t)hip_stream, (uint32_t)n_spans,
                       d_spans, d_in, in_bytes, d_out, out_floats);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
