// mix.hip -- noise from a bank of clips added to groups of float rows at a signal-to-noise ratio (afg_mix_hip,
// afg_batch_decode_mixed), for gfx950.  The definition -- both energies in float64 in the normalisation's summation order, the
// gain from one division, one product and one square root, a float32 apply without fused multiply-add -- is in
// include/afg.h; the Makefile builds this file with -ffp-contract=off like every other exact-mode kernel.  The host half
// (layout, record checks, the batch entry) is host/afg_mix.cpp.
//
// Three launches on the caller's stream, no atomics:
//   stats    one workgroup of 256 lanes per tile of 4096 floats of one row, found by a search over the groups' first tiles
//            (uniform per workgroup), as normalize.hip does.  Lane l takes the floats (e / 4) % 256 == l of the signal tile
//            and the noise under them: sixteen floats of each, all loaded before the first add.  The signal comes in four
//            dwordx4 loads when the tile is whole and its address 16-byte aligned, otherwise in dword loads of the same
//            elements; the noise likewise when its 4096 samples do not pass the clip's end and start 16-byte aligned.  The
//            tile's first noise position, (noise_start + tile_in_row * 4096) mod N, is formed once per workgroup in 64-bit
//            arithmetic; from there a lane's index takes one compare and one subtraction when N >= 4096 (a tile wraps at most
//            once) and a 32-bit remainder when N < 4096.  The lanes' tree is normalize.hip's, restated here so that file's
//            code does not move: steps 1 .. 16 with ds_swizzle, the eight 32-lane results through LDS, lane 0 doing steps
//            32 .. 128 and storing the tile's 16-byte partial.
//   finish   one lane per group adds its partials in tile order, forms the gain and writes the group's afg_mix_stats record
//   apply    the same tiles and the same two load shapes; one write per valid float, dwordx4 where the address allows.  A
//            group whose gain is 0 copies its input's bits, or -- in place -- does nothing, and never touches the noise.
//
// Bounds: every group is checked on the host before the launch (afg_mix_check_groups); the kernels rely on it.  They read
// in[in_off + r * stride + e], noise[noise_off + r * noise_stride + i] with i < noise_len and write
// out[out_off + r * stride + e] for r < rows and e < valid only, partials [0, n_tiles) and stats [0, n_groups).
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = afg::kPlaneTile;                      // floats; 16 per lane

struct Partial { double es, en; };
static_assert(sizeof(Partial) == 16, "a tile's partial is 16 bytes");
static_assert(sizeof(afg_mix_group) == 80 && sizeof(afg_mix_stats) == 24, "include/afg.h");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// a NaN result is the positive quiet NaN, whichever NaN the hardware made of its operands (include/afg.h)
__device__ __forceinline__ float one_nan(float v) { return v == v ? v : __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ double one_nan(double v) { return v == v ? v : __longlong_as_double(0x7ff8000000000000ll); }

// lane l ^ D's value, D = 1 .. 16 (ds_swizzle in bit-mask mode: and 0x1f, or 0, xor D)
template <int D> __device__ __forceinline__ double from_xor(double v)
{
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x1f | (D << 10));
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x1f | (D << 10));
    return __hiloint2double(hi, lo);
}
template <int D> __device__ __forceinline__ void tree_step(double &a, double &b)
{
    const double oa = from_xor<D>(a), ob = from_xor<D>(b);
    a = a + oa;                                                  // own + other: v[l] + v[l + D] in the lanes with l % (2 D) == 0
    b = b + ob;
}

// One tile of the launch: its group, the row it lies in, its first element in that row and its length.
struct Tile {
    afg_mix_group g;
    uint32_t gi, row, n;
    uint64_t e0;
};

// False: no group has the tile (never, behind the checks).
__device__ __forceinline__ bool find_tile(uint32_t n_groups, const afg_mix_group *__restrict__ groups, uint64_t tile, Tile *t)
{
    const uint32_t lo = afg::last_at_or_before(groups, n_groups, tile, &afg_mix_group::first_tile);   // (groups without floats have no tiles)
    t->g = groups[lo];
    t->gi = lo;
    if (t->g.first_tile > tile || t->g.valid == 0) return false;
    const uint64_t per_row = ((uint64_t)t->g.valid + kTile - 1) / kTile, local = tile - t->g.first_tile;
    const uint64_t r = local / per_row, k = local - r * per_row;
    if (r >= t->g.rows) return false;
    t->row = (uint32_t)r;
    t->e0 = k * kTile;
    t->n = (uint32_t)min((uint64_t)kTile, (uint64_t)t->g.valid - t->e0);
    return true;
}

// The lane's sixteen floats of a tile of n at p, element e = 1024 k + 4 lane + j in v[4 k + j]; +0.0f behind n.
__device__ __forceinline__ void load_signal(const float *p, uint32_t n, uint32_t lane, float (&v)[16])
{
    if (n == kTile && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const f32x4 q = *(const f32x4 *)(p + k * 1024 + 4 * lane);
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t e = k * 1024 + 4 * lane + j;
            v[4 * k + j] = e < n ? p[e] : 0.0f;
        }
}

// Likewise the noise under the tile: sample (p0 + e) mod N of the row at `row`, p0 < N the position under the tile's element 0.
__device__ __forceinline__ void load_noise(const float *__restrict__ row, uint32_t N, uint32_t p0, uint32_t n, uint32_t lane, float (&v)[16])
{
    const uint32_t room = N - p0;                                // samples from p0 to the clip's end, >= 1
    if (n == kTile && room >= kTile && ((uintptr_t)(row + p0) & 15u) == 0) {
        const float *p = row + p0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const f32x4 q = *(const f32x4 *)(p + k * 1024 + 4 * lane);
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
        return;
    }
    if (N >= kTile) {                                            // the tile passes the clip's end at most once
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t e = k * 1024 + 4 * lane + j;
                const uint32_t i = e < room ? p0 + e : e - room;   // (p0 + e < N: no wrap of the 32-bit sum; e - room < 4096 <= N)
                v[4 * k + j] = e < n ? row[i] : 0.0f;
            }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t e = k * 1024 + 4 * lane + j;
            const uint32_t i = (p0 + e) % N;                     // p0 + e < 8192
            v[4 * k + j] = e < n ? row[i] : 0.0f;
        }
}

// the noise row of the tile's row and the position under the tile's first element
__device__ __forceinline__ const float *noise_row(const Tile &t, const float *__restrict__ noise, uint32_t *p0)
{
    *p0 = (uint32_t)(((uint64_t)t.g.noise_start + t.e0) % t.g.noise_len);
    return noise + t.g.noise_off + (uint64_t)t.row * t.g.noise_stride;
}

__global__ __launch_bounds__(kThreads) void mix_stats_kernel(uint32_t n_groups, const afg_mix_group *__restrict__ groups,
                                                             const float *__restrict__ in, const float *__restrict__ noise,
                                                             Partial *__restrict__ partials)
{
    __shared__ double sh_s[8], sh_n[8];
    const uint64_t tile = blockIdx.x;
    Tile t;
    if (!find_tile(n_groups, groups, tile, &t)) return;
    const uint32_t lane = threadIdx.x;
    uint32_t p0;
    const float *nrow = noise_row(t, noise, &p0);
    float x[16], z[16];
    load_signal(in + t.g.in_off + (uint64_t)t.row * t.g.stride + t.e0, t.n, lane, x);
    load_noise(nrow, t.g.noise_len, p0, t.n, lane, z);
    double es = 0.0, en = 0.0;                                   // (an element behind n adds +0.0: the sums keep their bits)
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const double d = (double)x[i], m = (double)z[i];
        es = es + d * d;
        en = en + m * m;
    }
    tree_step<1>(es, en);
    tree_step<2>(es, en);
    tree_step<4>(es, en);
    tree_step<8>(es, en);
    tree_step<16>(es, en);
    if ((lane & 31u) == 0) { sh_s[lane >> 5] = es; sh_n[lane >> 5] = en; }
    __syncthreads();
    if (lane != 0) return;
    double s[8], m[8];
    for (int i = 0; i < 8; i++) { s[i] = sh_s[i]; m[i] = sh_n[i]; }
    for (int d = 1; d < 8; d <<= 1)                              // steps 32, 64 and 128 of the lanes' tree
        for (int i = 0; i < 8; i += 2 * d) { s[i] = s[i] + s[i + d]; m[i] = m[i] + m[i + d]; }
    f64x2 out;
    out.x = s[0]; out.y = m[0];
    *(f64x2 *)(partials + tile) = out;                           // one 16-byte vector store
}

__global__ __launch_bounds__(kThreads) void mix_finish_kernel(uint32_t n_groups, const afg_mix_group *__restrict__ groups,
                                                              const Partial *__restrict__ partials, afg_mix_stats *__restrict__ stats)
{
    const uint64_t gi = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gi >= n_groups) return;
    const afg_mix_group g = groups[gi];
    afg_mix_stats st;
    st.signal_energy = 0.0; st.noise_energy = 0.0; st.gain = 0.0f; st.flags = 0;
    if (g.valid != 0) {
        const uint64_t nt = (((uint64_t)g.valid + kTile - 1) / kTile) * g.rows;
        const Partial *p = partials + g.first_tile;
        double es = 0.0, en = 0.0;
        for (uint64_t t = 0; t < nt; t++) {
            es = es + p[t].es;
            en = en + p[t].en;
        }
        st.signal_energy = one_nan(es); st.noise_energy = one_nan(en);
        if (g.flags == AFG_MIX_GAIN) {
            st.gain = g.gain;
        } else {
            uint32_t why = 0;
            if (es == 0.0) why |= AFG_MIX_SILENT_SIGNAL;
            if (en == 0.0) why |= AFG_MIX_SILENT_NOISE;
            if (!isfinite(es) || !isfinite(en)) why |= AFG_MIX_ENERGY_NOT_FINITE;
            float gain = 0.0f;
            if (why == 0) {
                const double q = es / en;
                const double v = q * g.ratio;
                gain = (float)sqrt(v);
                if (!isfinite(gain)) { why = AFG_MIX_GAIN_NOT_FINITE; gain = 0.0f; }
            }
            st.gain = gain; st.flags = why;
        }
    }
    stats[gi] = st;
}

// (in and out may be the same plane: no __restrict__; every element is read and then written by one lane)
__global__ __launch_bounds__(kThreads) void mix_apply_kernel(uint32_t n_groups, const afg_mix_group *__restrict__ groups,
                                                             const afg_mix_stats *__restrict__ stats, const float *in,
                                                             const float *__restrict__ noise, float *out)
{
    const uint64_t tile = blockIdx.x;
    Tile t;
    if (!find_tile(n_groups, groups, tile, &t)) return;
    const uint32_t lane = threadIdx.x;
    const float gain = stats[t.gi].gain;
    const uint64_t at = (uint64_t)t.row * t.g.stride + t.e0;
    const float *p = in + t.g.in_off + at;
    float *y = out + t.g.out_off + at;
    float x[16];
    if (gain == 0.0f) {                                          // the input's bits; the noise is not read
        if (p == y) return;
        load_signal(p, t.n, lane, x);
    } else {
        uint32_t p0;
        const float *nrow = noise_row(t, noise, &p0);
        float z[16];
        load_signal(p, t.n, lane, x);
        load_noise(nrow, t.g.noise_len, p0, t.n, lane, z);
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = one_nan(__fadd_rn(x[i], __fmul_rn(gain, z[i])));
    }
    if (t.n == kTile && ((uintptr_t)y & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            f32x4 o;
            o.x = x[4 * k]; o.y = x[4 * k + 1]; o.z = x[4 * k + 2]; o.w = x[4 * k + 3];
            *(f32x4 *)(y + k * 1024 + 4 * lane) = o;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t e = k * 1024 + 4 * lane + j;
            if (e < t.n) y[e] = x[4 * k + j];
        }
}

int check_args(uint64_t n_groups, const afg_mix_group *d_groups, uint64_t n_tiles, const float *d_in, const float *d_noise, float *d_out,
               void *d_partials, afg_mix_stats *d_stats)
{
    if (!d_groups || !d_stats || (n_tiles && (!d_in || !d_noise || !d_out || !d_partials))) {
        afg::set_error("afg_mix_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_noise & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || ((uintptr_t)d_partials & 15u) != 0 ||
        ((uintptr_t)d_stats & 7u) != 0 || ((uintptr_t)d_groups & 7u) != 0) {
        afg::set_error("afg_mix_hip: the planes must be 4-byte aligned, the records and statistics 8-byte aligned, the partials 16-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_mix_hip", "groups", n_groups, n_tiles);
}

}  // namespace

int afg::mix_launch(const afg_mix_group *h_groups, uint64_t n_groups, const afg_mix_group *d_groups, uint64_t n_tiles, const float *d_in,
                    uint64_t in_floats, const float *d_noise, uint64_t noise_floats, float *d_out, uint64_t out_floats, void *d_partials,
                    afg_mix_stats *d_stats, hipStream_t stream)
{
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, n_tiles, d_in, d_noise, d_out, d_partials, d_stats)) return rc;
    const uint64_t plane_at[3] = { (uint64_t)(uintptr_t)d_in / 4, (uint64_t)(uintptr_t)d_noise / 4, (uint64_t)(uintptr_t)d_out / 4 };
    if (int rc = afg_mix_check_groups(h_groups, n_groups, n_tiles, in_floats, noise_floats, out_floats, plane_at)) return rc;
    if (int rc = afg::require_device()) return rc;
    const uint32_t ng = (uint32_t)n_groups;
    if (n_tiles)
        hipLaunchKernelGGL(mix_stats_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, stream, ng, d_groups, d_in, d_noise, (Partial *)d_partials);
    hipLaunchKernelGGL(mix_finish_kernel, dim3((uint32_t)((n_groups + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, ng, d_groups,
                       (const Partial *)d_partials, d_stats);
    if (n_tiles)
        hipLaunchKernelGGL(mix_apply_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, stream, ng, d_groups, (const afg_mix_stats *)d_stats, d_in,
                           d_noise, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_mix_hip(uint64_t n_groups, const afg_mix_group *d_groups, uint64_t n_tiles, const float *d_in, uint64_t in_floats,
                           const float *d_noise, uint64_t noise_floats, float *d_out, uint64_t out_floats, void *d_partials,
                           afg_mix_stats *d_stats, void *hip_stream)
{
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, n_tiles, d_in, d_noise, d_out, d_partials, d_stats)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_groups, n_groups, (hipStream_t)hip_stream, [&](const afg_mix_group *h) {
        return afg::mix_launch(h, n_groups, d_groups, n_tiles, d_in, in_floats, d_noise, noise_floats, d_out, out_floats, d_partials, d_stats,
                               (hipStream_t)hip_stream);
    });
}
