// pcm_f64.hip -- sample conversion to float64 (AudioStream.readSamplesDouble, stream.d:656-747; WAVDecoder.readSamples!double,
// wav.d:242-344) for gfx950.
//
// wav_pcm.hip with an 8-byte output element: the same spans (afg_wav_span, out_off and count in doubles), the same grid
// -- one workgroup of 256 lanes per tile of 4096 samples, found by a search over the spans' first tiles (uniform per
// workgroup: scalar loads) -- and the same access pattern: a lane converts 4 consecutive samples per step from 4 (u8),
// 8 (s16), 12 (s24), 16 (s32, f32, FLAC int32) or 2 x 16 (f64) bytes and stores them as two adjacent 16-byte non-temporal
// words next to its neighbours': 2 KB contiguous per wavefront and step.  The last count % 4 samples of a span, and all
// of a span whose input is not 16-byte aligned or whose output is not, go one sample per lane from single bytes.  No LDS.
//
// Arithmetic, bit-identical to IEEE float64:
//   u8 / s16 / s24  the exact integer divided by 127 / 32767 / 8388607 in double: the build has neither fast-math nor a
//                   relaxed division, so `/` is the correctly rounded division (v_div_scale / v_div_fmas / v_div_fixup on
//                   f64), as in wav_encode.hip.  Multiplying by the rounded reciprocal is not the same number.
//   s32             (double)s * 2^-31: exact.
//   FLAC int32      (double)s * (1.0 / 2147483647.0), one rounding (stream.d:713-716): what flac_restore.hip narrows to float.
//   f32             v_cvt_f64_f32: exact, denormals kept, a quiet NaN keeps sign and payload (top mantissa bits), a
//                   signalling NaN comes out quiet with its sign.
//   f64             the 64 bits moved through integer registers.
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_WAV_TILE_SAMPLES;               // samples per workgroup: 4 steps of 4 samples per lane
static_assert(kTile % (kThreads * 4) == 0, "a tile is whole steps");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
struct alignas(4) u32x3 { uint32_t a, b, c; };
struct Four { u64x2 lo, hi; };                                 // 4 doubles as bits

__device__ __forceinline__ uint64_t bits(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ uint64_t from_u8(uint32_t b) { return bits((double)((int32_t)b - 128) / 127.0); }
__device__ __forceinline__ uint64_t from_s16(uint32_t v) { return bits((double)(int32_t)(int16_t)v / 32767.0); }
__device__ __forceinline__ uint64_t from_s24(uint32_t v) { return bits((double)((int32_t)(v << 8) >> 8) / 8388607.0); }
__device__ __forceinline__ uint64_t from_s32(uint32_t v) { return bits((double)(int32_t)v * 0x1p-31); }
__device__ __forceinline__ uint64_t from_flac(uint32_t v) { return bits((double)(int32_t)v * (1.0 / 2147483647.0)); }
__device__ __forceinline__ uint64_t from_f32(uint32_t v) { return bits((double)__uint_as_float(v)); }

__device__ __forceinline__ uint32_t le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

template <int K> struct Kind;
template <> struct Kind<AFG_WAV_KIND_U8> {
    static constexpr uint32_t bytes = 1;
    static __device__ __forceinline__ Four four(const uint8_t *p)
    {
        const uint32_t w = __builtin_nontemporal_load((const uint32_t *)p);
        return Four{ u64x2{ from_u8(w & 255u), from_u8((w >> 8) & 255u) }, u64x2{ from_u8((w >> 16) & 255u), from_u8(w >> 24) } };
    }
    static __device__ __forceinline__ uint64_t one(const uint8_t *p) { return from_u8(p[0]); }
};
template <> struct Kind<AFG_WAV_KIND_S16> {
    static constexpr uint32_t bytes = 2;
    static __device__ __forceinline__ Four four(const uint8_t *p)
    {
        const u32x2 w = __builtin_nontemporal_load((const u32x2 *)p);
        return Four{ u64x2{ from_s16(w.x & 0xffffu), from_s16(w.x >> 16) }, u64x2{ from_s16(w.y & 0xffffu), from_s16(w.y >> 16) } };
    }
    static __device__ __forceinline__ uint64_t one(const uint8_t *p) { return from_s16((uint32_t)p[0] | ((uint32_t)p[1] << 8)); }
};
template <> struct Kind<AFG_WAV_KIND_S24> {
    static constexpr uint32_t bytes = 3;
    static __device__ __forceinline__ Four four(const uint8_t *p)
    {
        const u32x3 w = *(const u32x3 *)p;                      // 12 bytes = 4 samples
        return Four{ u64x2{ from_s24(w.a), from_s24((w.a >> 24) | (w.b << 8)) }, u64x2{ from_s24((w.b >> 16) | (w.c << 16)), from_s24(w.c >> 8) } };
    }
    static __device__ __forceinline__ uint64_t one(const uint8_t *p)
    {
        return from_s24((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
    }
};
// the three kinds of 4 bytes differ in the arithmetic only
template <uint64_t (*F)(uint32_t)> struct Word {
    static constexpr uint32_t bytes = 4;
    static __device__ __forceinline__ Four four(const uint8_t *p)
    {
        const u32x4 w = __builtin_nontemporal_load((const u32x4 *)p);
        return Four{ u64x2{ F(w.x), F(w.y) }, u64x2{ F(w.z), F(w.w) } };
    }
    static __device__ __forceinline__ uint64_t one(const uint8_t *p) { return F(le32(p)); }
};
template <> struct Kind<AFG_WAV_KIND_S32> : Word<from_s32> {};
template <> struct Kind<AFG_WAV_KIND_F32> : Word<from_f32> {};
template <> struct Kind<AFG_F64_KIND_FLAC_S32> : Word<from_flac> {};
template <> struct Kind<AFG_WAV_KIND_F64> {
    static constexpr uint32_t bytes = 8;
    static __device__ __forceinline__ Four four(const uint8_t *p)
    {
        return Four{ __builtin_nontemporal_load((const u64x2 *)p), __builtin_nontemporal_load((const u64x2 *)p + 1) };   // moves, no arithmetic
    }
    static __device__ __forceinline__ uint64_t one(const uint8_t *p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
};

// samples [0, n) of a tile: src / dst point at its first sample
template <int K> __device__ __forceinline__ void convert_tile(const uint8_t *src, uint64_t *dst, uint32_t n)
{
    typedef Kind<K> T;
    const uint32_t lane = threadIdx.x;
    const bool fast = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const uint32_t groups = fast ? n >> 2 : 0;                   // whole 32-byte pieces of output
#pragma unroll
    for (uint32_t step = 0; step < kTile / (kThreads * 4); step++) {
        const uint32_t g = step * kThreads + lane;
        if (g < groups) {
            const Four v = T::four(src + (size_t)g * 4 * T::bytes);
            __builtin_nontemporal_store(v.lo, (u64x2 *)dst + 2 * g);
            __builtin_nontemporal_store(v.hi, (u64x2 *)dst + 2 * g + 1);
        }
    }
    // the tail, or everything when the tile cannot take the fast path
    for (uint32_t i = groups * 4 + lane; i < n; i += kThreads) dst[i] = T::one(src + (size_t)i * T::bytes);
}

__global__ __launch_bounds__(kThreads) void pcm_to_f64_kernel(uint32_t n_spans, const afg_wav_span *__restrict__ spans,
                                                              const uint8_t *__restrict__ in, uint64_t in_bytes,
                                                              uint64_t *__restrict__ out, uint64_t out_doubles)
{
    const uint64_t t = blockIdx.x;
    // the span of tile t: the last one whose first tile is <= t (spans without samples have no tiles)
    const uint32_t lo = afg::last_at_or_before(spans, n_spans, t, &afg_wav_span::tile_first);
    const afg_wav_span sp = spans[lo];
    if (sp.tile_first > t || sp.kind > AFG_F64_KIND_FLAC_S32) return;
    const uint64_t s0 = (t - sp.tile_first) * kTile;             // first sample of the tile within the span
    if (s0 >= sp.count) return;
    const uint32_t bytes = sp.kind == AFG_WAV_KIND_U8 ? 1u : sp.kind == AFG_WAV_KIND_S16 ? 2u : sp.kind == AFG_WAV_KIND_S24 ? 3u
                           : sp.kind == AFG_WAV_KIND_F64 ? 8u : 4u;
    // a span that leaves the planes is not touched (counts are bounded first, so that the products cannot wrap)
    if (sp.count > out_doubles || sp.out_off > out_doubles - sp.count) return;
    if (sp.count > in_bytes / bytes || sp.in_off > in_bytes - sp.count * bytes) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, sp.count - s0);
    const uint8_t *src = in + sp.in_off + s0 * bytes;
    uint64_t *dst = out + sp.out_off + s0;
    switch (sp.kind) {
    case AFG_WAV_KIND_U8: convert_tile<AFG_WAV_KIND_U8>(src, dst, n); break;
    case AFG_WAV_KIND_S16: convert_tile<AFG_WAV_KIND_S16>(src, dst, n); break;
    case AFG_WAV_KIND_S24: convert_tile<AFG_WAV_KIND_S24>(src, dst, n); break;
    case AFG_WAV_KIND_S32: convert_tile<AFG_WAV_KIND_S32>(src, dst, n); break;
    case AFG_WAV_KIND_F32: convert_tile<AFG_WAV_KIND_F32>(src, dst, n); break;
    case AFG_WAV_KIND_F64: convert_tile<AFG_WAV_KIND_F64>(src, dst, n); break;
    default: convert_tile<AFG_F64_KIND_FLAC_S32>(src, dst, n); break;
    }
}

}  // namespace

extern "C" int afg_pcm_to_f64_hip(uint64_t n_spans, const afg_wav_span *d_spans, uint64_t n_tiles, const uint8_t *d_in,
                                  uint64_t in_bytes, double *d_out, uint64_t out_doubles, void *hip_stream)
{
    if (n_spans == 0 || n_tiles == 0) return AFG_OK;
    if (!d_spans || !d_in || !d_out) {
        afg::set_error("afg_pcm_to_f64_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (int rc = afg::launch_caps("afg_pcm_to_f64_hip", "spans", n_spans, n_tiles)) return rc;
    if (int rc = afg::require_device()) return rc;
    hipLaunchKernelGGL(pcm_to_f64_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, (hipStream_t)hip_stream, (uint32_t)n_spans,
                       d_spans, d_in, in_bytes, (uint64_t *)d_out, out_doubles);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
