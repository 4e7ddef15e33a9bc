// normalize.hip -- statistics per group of float rows (sum, sum of squares, min, max), and the gain / offset pass they
// decide (afg_normalize_hip, afg_batch_decode_resampled_norm, afg_batch_decode_mel_norm), for gfx950.  The definition -- a
// fixed summation order in float64, a float32 apply without fused multiply-add -- is in include/afg.h; the Makefile builds
// this file with -ffp-contract=off like every other exact-mode kernel.  The host half (layout, record checks, the batch
// entry) is host/afg_normalize.cpp.
//
// Three launches on the caller's stream, no atomics:
//   stats    one workgroup of 256 lanes per tile of 4096 floats of one row, found by a search over the groups' first tiles
//            (uniform per workgroup), as collate.hip and resample.hip do.  Lane l takes the floats (e / 4) % 256 == l: four
//            dwordx4 loads, all issued before the first add, when the tile is whole and its address 16-byte aligned
//            (in_off is only 4-byte aligned), otherwise dword loads of the same elements.  16 elements per lane: a
//            conversion, an exact product and two float64 adds each -- about 256 cycles of a SIMD per tile against the
//            1600 or so its 16 KiB take to arrive, so the pass stays bound by memory.  The lanes' tree runs steps 1 .. 16 with
//            ds_swizzle (xor mode: lane l reads lane l ^ d, which is l + d for the lanes whose sums go on), and the eight
//            32-lane results meet in LDS, where lane 0 does steps 32 .. 128 and stores the tile's 32-byte partial.
//            Min and max travel as order-preserving integer keys: -0 below +0, NaN left out.
//   finish   one lane per group adds its partials in tile order and writes the group's afg_norm_stats record
//   apply    the same tiles; one read and one write per valid float, dwordx4 where both addresses allow
//
// Bounds: every group is checked on the host before the launch (afg_norm_check_groups); the kernels rely on it.  They
// read in[in_off + r * stride + e] and write out[out_off + r * stride + e] for r < rows and e < valid only, partials
// [0, n_tiles) and stats [0, n_groups).
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = afg::kPlaneTile;                      // floats; 16 per lane
constexpr uint32_t kKeyPosInf = 0xff800000u, kKeyNegInf = 0x007fffffu;

struct Partial { double sum, sumsq; float mn, mx; uint32_t pad[2]; };
static_assert(sizeof(Partial) == 32, "a tile's partial is 32 bytes");
static_assert(sizeof(afg_norm_group) == 48 && sizeof(afg_norm_stats) == 40 && sizeof(afg_norm_params) == 24, "include/afg.h");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// floats in the order of their values as unsigned integers (-0 below +0)
__device__ __forceinline__ uint32_t key_of(float x)
{
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// a NaN result is the positive quiet NaN, whichever NaN the hardware made of its operands (include/afg.h)
__device__ __forceinline__ float one_nan(float v) { return v == v ? v : __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ double one_nan(double v) { return v == v ? v : __longlong_as_double(0x7ff8000000000000ll); }

struct Acc {
    double s, q;
    uint32_t mn, mx;
    __device__ __forceinline__ void take(float x)
    {
        const double d = (double)x;
        s = s + d;
        q = q + d * d;
        if (x == x) {
            const uint32_t k = key_of(x);
            mn = min(mn, k);
            mx = max(mx, k);
        }
    }
    __device__ __forceinline__ void join(const Acc &o)
    {
        s = s + o.s;
        q = q + o.q;
        mn = min(mn, o.mn);
        mx = max(mx, o.mx);
    }
};

// lane l ^ D's value, D = 1 .. 16 (ds_swizzle in bit-mask mode: and 0x1f, or 0, xor D)
template <int D> __device__ __forceinline__ uint32_t from_xor(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1f | (D << 10));
}
template <int D> __device__ __forceinline__ double from_xor(double v)
{
    const uint32_t lo = from_xor<D>((uint32_t)__double2loint(v)), hi = from_xor<D>((uint32_t)__double2hiint(v));
    return __hiloint2double((int)hi, (int)lo);
}
template <int D> __device__ __forceinline__ void tree_step(Acc &a)
{
    Acc o;
    o.s = from_xor<D>(a.s);
    o.q = from_xor<D>(a.q);
    o.mn = from_xor<D>(a.mn);
    o.mx = from_xor<D>(a.mx);
    a.join(o);                                                   // own + other: v[l] + v[l + D] in the lanes with l % (2 D) == 0
}

// The tile `tile` of the launch: its group (index *gi), the float index of its first element from the group's row 0,
// element 0, and its length.  False: no group has it (never, behind the checks).
__device__ __forceinline__ bool find_tile(uint32_t n_groups, const afg_norm_group *__restrict__ groups, uint64_t tile, afg_norm_group *g,
                                          uint32_t *gi, uint64_t *at, uint32_t *n)
{
    const uint32_t lo = afg::last_at_or_before(groups, n_groups, tile, &afg_norm_group::first_tile);   // (groups without floats have no tiles)
    *g = groups[lo];
    *gi = lo;
    if (g->first_tile > tile || g->valid == 0) return false;
    const uint64_t per_row = ((uint64_t)g->valid + kTile - 1) / kTile, local = tile - g->first_tile;
    const uint64_t r = local / per_row, t = local - r * per_row;
    if (r >= g->rows) return false;
    *at = r * g->stride + t * kTile;
    *n = (uint32_t)min((uint64_t)kTile, (uint64_t)g->valid - t * kTile);
    return true;
}

__global__ __launch_bounds__(kThreads) void norm_stats_kernel(uint32_t n_groups, const afg_norm_group *__restrict__ groups,
                                                              const float *__restrict__ in, Partial *__restrict__ partials)
{
    __shared__ double sh_s[8], sh_q[8];
    __shared__ uint32_t sh_mn[8], sh_mx[8];
    const uint64_t tile = blockIdx.x;
    afg_norm_group g;
    uint32_t gi, n;
    uint64_t at;
    if (!find_tile(n_groups, groups, tile, &g, &gi, &at, &n)) return;
    const float *p = in + g.in_off + at;
    const uint32_t lane = threadIdx.x;
    Acc a = { 0.0, 0.0, kKeyPosInf, kKeyNegInf };
    if (n == kTile && ((uintptr_t)p & 15u) == 0) {
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = *(const f32x4 *)(p + k * 1024 + 4 * lane);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a.take(v[k].x); a.take(v[k].y); a.take(v[k].z); a.take(v[k].w);
        }
    } else {
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t e = k * 1024 + 4 * lane;
            for (uint32_t j = 0; j < 4 && e + j < n; j++) a.take(p[e + j]);
        }
    }
    tree_step<1>(a);
    tree_step<2>(a);
    tree_step<4>(a);
    tree_step<8>(a);
    tree_step<16>(a);
    if ((lane & 31u) == 0) {
        const uint32_t w = lane >> 5;
        sh_s[w] = a.s; sh_q[w] = a.q; sh_mn[w] = a.mn; sh_mx[w] = a.mx;
    }
    __syncthreads();
    if (lane != 0) return;
    Acc v[8];
    for (int i = 0; i < 8; i++) v[i] = { sh_s[i], sh_q[i], sh_mn[i], sh_mx[i] };
    for (int d = 1; d < 8; d <<= 1)                              // steps 32, 64 and 128 of the lanes' tree
        for (int i = 0; i < 8; i += 2 * d) v[i].join(v[i + d]);
    Partial out;
    out.sum = v[0].s; out.sumsq = v[0].q;
    out.mn = float_of(v[0].mn); out.mx = float_of(v[0].mx);
    out.pad[0] = out.pad[1] = 0;
    partials[tile] = out;
}

__global__ __launch_bounds__(kThreads) void norm_finish_kernel(uint32_t n_groups, const afg_norm_group *__restrict__ groups,
                                                               const Partial *__restrict__ partials, afg_norm_params prm,
                                                               afg_norm_stats *__restrict__ stats)
{
    const uint64_t gi = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gi >= n_groups) return;
    const afg_norm_group g = groups[gi];
    afg_norm_stats st;
    st.sum = 0.0; st.sumsq = 0.0; st.count = 0;
    st.min = 0.0f; st.max = 0.0f; st.offset = 0.0f; st.scale = 0.0f;
    if (g.valid != 0) {
        const uint64_t nt = (((uint64_t)g.valid + kTile - 1) / kTile) * g.rows;
        const Partial *p = partials + g.first_tile;
        double s = 0.0, q = 0.0;
        uint32_t mn = kKeyPosInf, mx = kKeyNegInf;
        for (uint64_t t = 0; t < nt; t++) {
            s = s + p[t].sum;
            q = q + p[t].sumsq;
            mn = min(mn, key_of(p[t].mn));
            mx = max(mx, key_of(p[t].mx));
        }
        st.sum = one_nan(s); st.sumsq = one_nan(q);
        st.count = (uint64_t)g.rows * g.valid;
        st.min = float_of(mn); st.max = float_of(mx);
        const double count = (double)st.count;
        float offset = 0.0f, scale = 1.0f;
        if (prm.mode == AFG_NORM_PEAK) {
            const float pk = fmaxf(-st.min, st.max);
            if (pk != 0.0f && isfinite(pk)) scale = prm.target / pk;
        } else if (prm.mode == AFG_NORM_RMS) {
            const float r = (float)sqrt(q / count);
            if (r != 0.0f && isfinite(r)) scale = prm.target / r;
        } else if (prm.mode == AFG_NORM_STANDARD) {
            const double mean = s / count, m2 = q / count, mm = mean * mean;
            const double var = fmax(m2 - mm, 0.0);
            const float eps = prm.eps == 0.0f ? 1e-7f : prm.eps;
            offset = (float)mean;
            scale = (float)(1.0 / sqrt(var + (double)eps));
        } else if (prm.mode == AFG_NORM_DYNAMIC_RANGE) {
            offset = st.max - prm.range;
            scale = prm.gain;
        }
        st.offset = one_nan(offset); st.scale = one_nan(scale);
    }
    stats[gi] = st;
}

template <bool kFloor> __device__ __forceinline__ float apply_one(float x, float offset, float scale, float shift)
{
    if (kFloor) {
        const float m = x > offset ? x : offset;                 // (a NaN sample takes the floor)
        const float a = m + shift;
        return one_nan(a * scale);
    }
    const float d = x - offset;
    return one_nan(d * scale);
}

template <bool kFloor> __device__ __forceinline__ void apply_tile(const float *__restrict__ p, float *__restrict__ y, uint32_t n, float offset,
                                                                  float scale, float shift)
{
    const uint32_t lane = threadIdx.x;
    if (n == kTile && (((uintptr_t)p | (uintptr_t)y) & 15u) == 0) {
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = *(const f32x4 *)(p + k * 1024 + 4 * lane);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            f32x4 o;
            o.x = apply_one<kFloor>(v[k].x, offset, scale, shift);
            o.y = apply_one<kFloor>(v[k].y, offset, scale, shift);
            o.z = apply_one<kFloor>(v[k].z, offset, scale, shift);
            o.w = apply_one<kFloor>(v[k].w, offset, scale, shift);
            *(f32x4 *)(y + k * 1024 + 4 * lane) = o;
        }
        return;
    }
    for (uint32_t e = lane; e < n; e += kThreads) y[e] = apply_one<kFloor>(p[e], offset, scale, shift);
}

// (in and out may be the same plane: no __restrict__; every element is read and then written by one lane)
__global__ __launch_bounds__(kThreads) void norm_apply_kernel(uint32_t n_groups, const afg_norm_group *__restrict__ groups,
                                                              const afg_norm_stats *__restrict__ stats, afg_norm_params prm, const float *in,
                                                              float *out)
{
    const uint64_t tile = blockIdx.x;
    afg_norm_group g;
    uint32_t gi, n;
    uint64_t at;
    if (!find_tile(n_groups, groups, tile, &g, &gi, &at, &n)) return;
    const float offset = stats[gi].offset, scale = stats[gi].scale;
    const float *p = in + g.in_off + at;
    float *y = out + g.out_off + at;
    if (prm.mode == AFG_NORM_DYNAMIC_RANGE) apply_tile<true>(p, y, n, offset, scale, prm.shift);
    else apply_tile<false>(p, y, n, offset, scale, 0.0f);
}

int check_args(uint64_t n_groups, const afg_norm_group *d_groups, uint64_t n_tiles, const afg_norm_params *params, const float *d_in,
               float *d_out, void *d_partials, afg_norm_stats *d_stats)
{
    if (!params) {
        afg::set_error("afg_normalize_hip: NULL params");
        return AFG_ERR_INVALID;
    }
    if (!d_groups || !d_stats || (n_tiles && (!d_in || !d_partials)) || (n_tiles && params->mode != AFG_NORM_NONE && !d_out)) {
        afg::set_error("afg_normalize_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || ((uintptr_t)d_partials & 7u) != 0 || ((uintptr_t)d_stats & 7u) != 0 ||
        ((uintptr_t)d_groups & 7u) != 0) {
        afg::set_error("afg_normalize_hip: the planes must be 4-byte aligned, the records, partials and statistics 8-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_normalize_hip", "groups", n_groups, n_tiles);
}

}  // namespace

int afg::normalize_launch(const afg_norm_group *h_groups, uint64_t n_groups, const afg_norm_group *d_groups, uint64_t n_tiles,
                          const afg_norm_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats,
                          void *d_partials, afg_norm_stats *d_stats, hipStream_t stream)
{
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, n_tiles, params, d_in, d_out, d_partials, d_stats)) return rc;
    if (int rc = afg_norm_check_groups(h_groups, n_groups, n_tiles, params, in_floats, out_floats)) return rc;
    if (int rc = afg::require_device()) return rc;
    const uint32_t ng = (uint32_t)n_groups;
    if (n_tiles)
        hipLaunchKernelGGL(norm_stats_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, stream, ng, d_groups, d_in, (Partial *)d_partials);
    hipLaunchKernelGGL(norm_finish_kernel, dim3((uint32_t)((n_groups + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, ng, d_groups,
                       (const Partial *)d_partials, *params, d_stats);
    if (n_tiles && params->mode != AFG_NORM_NONE)
        hipLaunchKernelGGL(norm_apply_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, stream, ng, d_groups, (const afg_norm_stats *)d_stats,
                           *params, d_in, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_normalize_hip(uint64_t n_groups, const afg_norm_group *d_groups, uint64_t n_tiles, const afg_norm_params *params,
                                 const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, void *d_partials,
                                 afg_norm_stats *d_stats, void *hip_stream)
{
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, n_tiles, params, d_in, d_out, d_partials, d_stats)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_groups, n_groups, (hipStream_t)hip_stream, [&](const afg_norm_group *h) {
        return afg::normalize_launch(h, n_groups, d_groups, n_tiles, params, d_in, in_floats, d_out, out_floats, d_partials, d_stats,
                                     (hipStream_t)hip_stream);
    });
}
