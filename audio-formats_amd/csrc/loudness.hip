// loudness.hip -- integrated loudness after ITU-R BS.1770-4 per group of float rows and the gain to a target (afg_loudness_hip,
// afg_batch_decode_loudnorm), for gfx950.  The definition, the interval the block energies are held to and the constant K_L in
// it are in include/afg.h; the host half (K-weighting design, layout, checks, the batch entry) is host/afg_loudness.cpp.
//
// Three launches on the caller's stream, no atomics, nothing that waits for another workgroup, no host round trip:
//   measure  one workgroup of 256 lanes per row, the walk of csrc/filter.hip with its two sections fixed: tiles of 4096 frames
//            come in as dwordx4 at dword alignment one tile ahead, go through LDS into chunks of 16 frames per lane, and each
//            section runs over the chunk from a zero state in float64, the chunks' end states meeting in the scan of
//            s -> A^16 s + e inside the wavefront and through LDS across the four -- the filter kernel's evaluation, operation
//            for operation, which is why K_L is AFG_FILTER_K.  The K-weighted chunk is never rounded or stored: the lane adds its
//            squares to the 100 ms sub-block they fall into -- a chunk meets at most one sub-block edge (a sub-block has 800
//            samples or more), which may lie anywhere inside it: 44.1 kHz has 4410 samples to the sub-block --, the wavefront
//            folds the lanes' sums per sub-block it touches (four at the most) in a xor tree, and lanes 0 .. 7 of the workgroup
//            keep the running sums of the eight sub-blocks a tile can reach, by sub-block index modulo 8, writing a sum to
//            d_sub once no later tile adds to it.  Every order is fixed by the row's own indices: the same row gives the same
//            bits wherever it stands.  The row's largest |x| goes behind its sub-block sums.
//   gate     one wavefront per group: z_j from four sub-block sums per row and the weights into d_blocks, the absolute gate's
//            count and compensated sum, the relative threshold, the second gate's count and sum, and lane 0 writes the record
//            with the gain.
//   apply    y = x * gain over the valid elements: a row's interior, from the output's first 16-byte boundary, as dwordx4
//            stores (the input side read as dwordx4 at whatever dword alignment that leaves it), head and tail one float a
//            lane; a workgroup takes 4096 floats a step.
//
// Bounds: every group is checked on the host before the launch (afg_loudness_check_groups); the kernels rely on it.  They
// read in[in_off + r * stride + e] and write out[out_off + r * stride + e] for r < rows and e < valid only, the group's
// doubles of d_sub ([first_sub, first_sub + rows * (n_sub + 1)) with n_sub its sub-blocks per row) and of d_blocks
// ([first_block, first_block + n_blocks)), its record, and the K-weighting's table of 2 * 300 doubles.
#include "afg_records.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_FILTER_TILE, kChunk = AFG_FILTER_CHUNK, kPad = 20;      // kPad: dwords from one lane's chunk to the next in LDS
constexpr uint32_t kNsec = 2;                                   // the shelf and the high-pass
constexpr uint32_t kH1 = afg::kFilterH1, kH2 = afg::kFilterH2, kPow = afg::kFilterPow, kSec = afg::kFilterSecDoubles;
constexpr uint32_t kSlots = 4;                                  // sub-blocks one wavefront's 1024 frames can add to
constexpr uint32_t kApplyZ = 1024;                              // workgroups along one row of the apply pass, at the most

static_assert(kTile == kThreads * kChunk && kChunk == 16, "include/afg.h");
static_assert(AFG_LOUDNESS_K == AFG_FILTER_K, "the evaluation below is csrc/filter.hip's");
static_assert(sizeof(afg_loudness_group) == 64 && sizeof(afg_loudness_params) == 96 && sizeof(afg_loudness_stats) == 40 &&
              sizeof(afg_loudness_counts) == 16, "include/afg.h");
// a wavefront's frames and a tile's, with the sub-block behind the last one's, stay inside kSlots and 8 sub-blocks
static_assert((800 - 1 + 64 * 16 - 16) / 800 + 2 <= kSlots && (800 - 1 + 4096 - 16) / 800 + 2 <= 8, "sub-blocks of 800 samples at the least");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a dwordx4 at dword alignment

struct GateArgs {
    uint32_t step;
    float max_peak, max_gain;
    double weights[8], gamma_abs, target_energy;                 // the weights resolved; 10^((-70 + 0.691) / 10); T
};

__device__ __forceinline__ double dfma(double a, double b, double c) { return __builtin_fma(a, b, c); }

__device__ __forceinline__ uint32_t blocks_of(uint32_t valid, uint32_t step) { return valid >= 4u * step ? (valid - 4u * step) / step + 1u : 0u; }

// the tile's 16-byte word k * 256 + lane: frames e .. e + 3 of the nt the tile has, +0.0f behind them
__device__ __forceinline__ void fetch_tile(f32x4 (&v)[4], const float *p, uint32_t nt, uint32_t lane)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t e = 4u * (k * kThreads + lane);
        if (e + 4 <= nt) {
            v[k] = *(const f32x4u *)(p + e);
        } else {
            v[k] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
            if (e < nt) v[k].x = p[e];
            if (e + 1 < nt) v[k].y = p[e + 1];
            if (e + 2 < nt) v[k].z = p[e + 2];
        }
    }
}

__global__ __launch_bounds__(kThreads) void loudness_measure_kernel(const afg_loudness_group *__restrict__ groups, uint32_t step,
                                                                    const double *__restrict__ tab, const float *__restrict__ in,
                                                                    double *__restrict__ sub)
{
    __shared__ __attribute__((aligned(16))) float sh_tile[kThreads * kPad];
    __shared__ __attribute__((aligned(16))) double sh_pow[kNsec * 64 * 4];       // A^(16 i), i < 64, per section
    __shared__ double sh_wave[2][4][2];                          // by section parity: the wavefronts' totals
    __shared__ double sh_carry[2][kNsec][4];                     // by tile parity: u[n-1], u[n-2], v[n-1], v[n-2] in front of the tile
    __shared__ double sh_part[4][kSlots];                        // a tile's sums by wavefront and sub-block, counted from ...
    __shared__ uint32_t sh_first[4];                             // ... the wavefront's first
    __shared__ float sh_peak[4];
    const afg_loudness_group g = groups[blockIdx.x];
    const uint32_t r = blockIdx.y;
    if (r >= g.rows || g.valid == 0) return;
    const uint32_t nb = blocks_of(g.valid, step), nsub = nb ? nb + 3u : 0u;
    const uint64_t lim = (uint64_t)nsub * step;                  // the frames that lie in a block; lim <= valid
    double *const my_sub = sub + g.first_sub + (uint64_t)r * (nsub + 1u);
    const uint32_t lane = threadIdx.x, i = lane & 63u, w = lane >> 6;
    for (uint32_t k = lane; k < kNsec * 256u; k += kThreads) sh_pow[k] = tab[(k >> 8) * kSec + kPow + (k & 255u)];
    if (lane < kNsec * 4u) sh_carry[0][lane >> 2][lane & 3u] = 0.0;
    const float *const x = in + g.in_off + (uint64_t)r * g.stride;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)g.valid + kTile - 1) / kTile);
    uint32_t s_t = 0, o_t = 0;                                   // the tile's first frame lies o_t frames into sub-block s_t
    uint32_t s_prev = 0, base = 0;                               // lanes 0 .. 7: the lowest sub-block not yet written
    double run = 0.0;                                            // lanes 0 .. 7: the running sum of the sub-block = lane mod 8 at or above base
    float pk = 0.0f;
    // lanes 0 .. 7 take the sums of the tile whose first sub-block is st: what no tile from that one on adds to is written
    auto take = [&](uint32_t st) {
        const uint32_t mine = base + ((lane - base) & 7u);
        if (mine < st) {
            if (mine < nsub) my_sub[mine] = run;
            run = 0.0;
        }
        base = st;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint32_t f = sh_first[v];
#pragma unroll
            for (int k = 0; k < (int)kSlots; k++) {
                const double p = sh_part[v][k];
                if (((f + k) & 7u) == lane) run = run + p;
            }
        }
    };
    f32x4 pre[4];
    fetch_tile(pre, x, min(g.valid, kTile), lane);
    for (uint32_t t = 0; t < n_tiles; t++) {
        const uint64_t t0 = (uint64_t)t * kTile;
        const uint32_t par = t & 1u;
        const bool last = t + 1 == n_tiles;
        if (t) __syncthreads();                                  // the tile before has left LDS, its sums are in sh_part
        if (t && lane < 8) take(s_prev);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t e = 4u * (k * kThreads + lane);
            *(f32x4 *)&sh_tile[(e >> 4) * kPad + (e & 15u)] = pre[k];
            pk = fmaxf(pk, fmaxf(fmaxf(fabsf(pre[k].x), fabsf(pre[k].y)), fmaxf(fabsf(pre[k].z), fabsf(pre[k].w))));
        }
        __syncthreads();
        if (!last) fetch_tile(pre, x + t0 + kTile, (uint32_t)min((uint64_t)kTile, (uint64_t)g.valid - t0 - kTile), lane);
        double xs[kChunk];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f32x4 v = *(const f32x4 *)&sh_tile[lane * kPad + 4 * q];
            xs[4 * q] = (double)v.x; xs[4 * q + 1] = (double)v.y; xs[4 * q + 2] = (double)v.z; xs[4 * q + 3] = (double)v.w;
        }
        double Pa = 0.0, Pb = 0.0;                               // the state this wavefront started the section before from
        for (uint32_t s = 0; s < kNsec; s++) {
            const double *T = tab + s * kSec;
            const double b0 = T[0], b1 = T[1], b2 = T[2], na1 = -T[3], na2 = -T[4];
            // the input's history in front of the chunk
            double p1 = __shfl_up(xs[15], 1), p2 = __shfl_up(xs[14], 1);
            if (i == 0) {
                if (w == 0) { p1 = sh_carry[par][s][0]; p2 = sh_carry[par][s][1]; }
                else if (s == 0) { p1 = (double)sh_tile[(lane - 1) * kPad + 15]; p2 = (double)sh_tile[(lane - 1) * kPad + 14]; }
                else { p1 = Pa; p2 = Pb; }
            }
            const double x15 = xs[15], x14 = xs[14];
            // the chunk from a zero output state
            double u1 = p1, u2 = p2, z1 = 0.0, z2 = 0.0;
#pragma unroll
            for (int n = 0; n < (int)kChunk; n++) {
                const double xn = xs[n];
                const double fir = dfma(b0, xn, dfma(b1, u1, b2 * u2));
                const double zn = dfma(na1, z1, dfma(na2, z2, fir));
                u2 = u1; u1 = xn; z2 = z1; z1 = zn;
                xs[n] = zn;
            }
            // inclusive scan of s -> A^16 s + e over the wavefront
            double ea = z1, eb = z2;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const uint32_t d = 1u << k;
                const double *M = T + kPow + 4 * d;
                const double ta = __shfl_up(ea, d), tb = __shfl_up(eb, d);
                if (i >= d) {
                    ea = dfma(M[0], ta, dfma(M[1], tb, ea));
                    eb = dfma(M[2], ta, dfma(M[3], tb, eb));
                }
            }
            double ca = __shfl_up(ea, 1), cb = __shfl_up(eb, 1);  // what the lanes below in the wavefront add up to
            if (i == 0) { ca = 0.0; cb = 0.0; }
            if (i == 63) { sh_wave[s & 1u][w][0] = ea; sh_wave[s & 1u][w][1] = eb; }
            __syncthreads();
            // the state the wavefront starts from: the tile's carry and the wavefronts below
            Pa = sh_carry[par][s][2]; Pb = sh_carry[par][s][3];
            const double *M64 = T + kPow + 4 * 64;
            for (uint32_t v = 0; v < w; v++) {
                const double na = dfma(M64[0], Pa, dfma(M64[1], Pb, sh_wave[s & 1u][v][0]));
                const double nb2 = dfma(M64[2], Pa, dfma(M64[3], Pb, sh_wave[s & 1u][v][1]));
                Pa = na; Pb = nb2;
            }
            // ... the lane's: A^(16 i) of that (the identity for lane 0) and the lanes below
            const double *Mi = &sh_pow[(s * 64u + i) * 4u];
            const double Sa = dfma(Mi[0], Pa, dfma(Mi[1], Pb, ca)), Sb = dfma(Mi[2], Pa, dfma(Mi[3], Pb, cb));
#pragma unroll
            for (int n = 0; n < (int)kChunk; n++) xs[n] = dfma(T[kH1 + n], Sa, dfma(T[kH2 + n], Sb, xs[n]));
            if (lane == kThreads - 1) {
                double *c = sh_carry[par ^ 1u][s];
                c[0] = x15; c[1] = x14; c[2] = xs[15]; c[3] = xs[14];
            }
        }
        // the chunk's squares, to the sub-block the chunk starts in (the first `e` frames) and the one behind it
        const uint32_t at = o_t + lane * kChunk, q0 = at / step;
        const uint32_t s0 = s_t + q0, e = step - (at - q0 * step);
        const uint64_t n0 = t0 + (uint64_t)lane * kChunk;
        const uint32_t cnt = lim > n0 ? (uint32_t)min((uint64_t)kChunk, lim - n0) : 0u;   // the chunk's frames that lie in a block
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (int n = 0; n < (int)kChunk; n++) {
            const bool here = (uint32_t)n < cnt, first = (uint32_t)n < e;
            const double v0 = here && first ? xs[n] : 0.0, v1 = here && !first ? xs[n] : 0.0;
            acc0 = dfma(v0, v0, acc0);
            acc1 = dfma(v1, v1, acc1);
        }
        const uint32_t f = __shfl(s0, 0), l = __shfl(s0, 63);     // the wavefront's first and last chunk's sub-blocks
#pragma unroll
        for (int k = 0; k < (int)kSlots; k++) {
            double c = 0.0;
            if (f + k <= l + 1u) {                               // (the same for the whole wavefront)
                c = (s0 == f + k ? acc0 : 0.0) + (s0 + 1u == f + k ? acc1 : 0.0);
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) c = c + __shfl_xor(c, d);
            }
            if (i == 0) sh_part[w][k] = c;
        }
        if (i == 0) sh_first[w] = f;
        s_prev = s_t;
        o_t += kTile;
        while (o_t >= step) { o_t -= step; s_t++; }
    }
    for (int d = 1; d < 64; d <<= 1) pk = fmaxf(pk, __shfl_xor(pk, d));
    if (i == 0) sh_peak[w] = pk;
    __syncthreads();
    if (lane < 8) {
        take(s_prev);
        const uint32_t mine = base + ((lane - base) & 7u);
        if (mine < nsub) my_sub[mine] = run;
    }
    if (lane == 0) my_sub[nsub] = (double)fmaxf(fmaxf(sh_peak[0], sh_peak[1]), fmaxf(sh_peak[2], sh_peak[3]));
}

// the 64 lanes' sum and count in every lane
__device__ __forceinline__ double wave_sum(double v)
{
    for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ uint32_t wave_count(uint32_t v)
{
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

// s + v with the rounding error carried along (Kahan): the sum of any number of blocks is off by a few units in the last place
__device__ __forceinline__ void add_to(double &s, double &comp, double v)
{
    const double y = v - comp, t = s + y;
    comp = (t - s) - y;
    s = t;
}

__global__ __launch_bounds__(64) void loudness_gate_kernel(const afg_loudness_group *__restrict__ groups, GateArgs a,
                                                           const double *__restrict__ sub, double *blocks,
                                                           afg_loudness_stats *__restrict__ stats)
{
    const afg_loudness_group g = groups[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint32_t nb = g.valid ? blocks_of(g.valid, a.step) : 0u, nsub = nb ? nb + 3u : 0u;
    const double *const S = sub + g.first_sub;
    double *const Z = blocks + g.first_block;
    const double N = (double)(4u * a.step);
    // z_j, the absolute gate
    uint32_t n_abs = 0;
    double sum = 0.0, comp = 0.0;
    for (uint32_t j = lane; j < nb; j += 64) {
        double acc = 0.0;
        for (uint32_t r = 0; r < g.rows; r++) {
            const double *p = S + (uint64_t)r * (nsub + 1u) + j;
            acc = dfma(a.weights[r], (p[0] + p[1]) + (p[2] + p[3]), acc);
        }
        const double z = acc / N;
        Z[j] = z;
        if (z > a.gamma_abs) { n_abs++; add_to(sum, comp, z); }
    }
    n_abs = wave_count(n_abs);
    sum = wave_sum(sum);
    const double rel = n_abs ? 0.1 * (sum / (double)n_abs) : 0.0;
    // the relative gate (a lane reads the z_j it wrote)
    uint32_t n_gated = 0;
    sum = 0.0; comp = 0.0;
    for (uint32_t j = lane; j < nb; j += 64) {
        const double z = Z[j];
        if (z > a.gamma_abs && z > rel) { n_gated++; add_to(sum, comp, z); }
    }
    n_gated = wave_count(n_gated);
    sum = wave_sum(sum);
    if (lane != 0) return;
    afg_loudness_stats rec;
    rec.energy = n_gated ? sum / (double)n_gated : 0.0;
    rec.rel_threshold = rel;
    rec.n_blocks = nb; rec.n_abs = n_abs; rec.n_gated = n_gated;
    rec.flags = 0;
    rec.peak = 0.0f;
    for (uint32_t r = 0; r < g.rows && g.valid != 0; r++) rec.peak = fmaxf(rec.peak, (float)S[(uint64_t)r * (nsub + 1u) + nsub]);
    rec.gain = 1.0f;
    if (n_gated == 0) {
        rec.flags = AFG_LOUDNESS_UNGATED;
    } else {
        float gain = (float)sqrt(a.target_energy / rec.energy);
        if (a.max_gain > 0.0f && gain > a.max_gain) { gain = a.max_gain; rec.flags |= AFG_LOUDNESS_GAIN_CLAMPED; }
        if (a.max_peak > 0.0f && rec.peak > 0.0f) {
            const float top = a.max_peak / rec.peak;
            if (gain > top) { gain = top; rec.flags |= AFG_LOUDNESS_PEAK_CLAMPED; }
        }
        rec.gain = gain;
    }
    stats[blockIdx.x] = rec;
}

__global__ __launch_bounds__(kThreads) void loudness_apply_kernel(const afg_loudness_group *__restrict__ groups,
                                                                  const afg_loudness_stats *__restrict__ stats, const float *in, float *out)
{
    const afg_loudness_group g = groups[blockIdx.x];
    const uint32_t r = blockIdx.y, n = g.valid, lane = threadIdx.x;
    if (r >= g.rows || n == 0) return;
    const float gain = stats[blockIdx.x].gain;
    const float *const x = in + g.in_off + (uint64_t)r * g.stride;
    float *const y = out + g.out_off + (uint64_t)r * g.stride;
    const uint32_t head = min(n, (uint32_t)((16u - ((uintptr_t)y & 15u)) & 15u) / 4u);
    const uint32_t words = (n - head) / 4, tail0 = head + 4 * words;
    if (blockIdx.z == 0) {
        if (lane < head) y[lane] = x[lane] * gain;
        if (tail0 + lane < n) y[tail0 + lane] = x[tail0 + lane] * gain;
    }
    for (uint32_t first = blockIdx.z * 1024u; first < words; first += gridDim.z * 1024u) {
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t wd = first + k * kThreads + lane;
            if (wd < words) v[k] = *(const f32x4u *)(x + head + 4 * (uint64_t)wd);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t wd = first + k * kThreads + lane;
            if (wd < words) *(f32x4 *)(y + head + 4 * (uint64_t)wd) = f32x4{ v[k].x * gain, v[k].y * gain, v[k].z * gain, v[k].w * gain };
        }
    }
}

int check_args(uint64_t n_groups, const afg_loudness_group *d_groups, const afg_loudness_counts *counts, const afg_loudness_params *params,
               const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_sub, double *d_blocks,
               afg_loudness_stats *d_stats)
{
    if (!counts) {
        afg::set_error("afg_loudness_hip: NULL counts");
        return AFG_ERR_INVALID;
    }
    if (!d_groups || !d_stats || (counts->n_sub && (!d_in || !d_sub)) || (counts->n_blocks && !d_blocks) || (params->apply && counts->n_sub && !d_out)) {
        afg::set_error("afg_loudness_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || (((uintptr_t)d_groups | (uintptr_t)d_sub | (uintptr_t)d_blocks | (uintptr_t)d_stats) & 7u) != 0) {
        afg::set_error("afg_loudness_hip: the planes must be 4-byte aligned, the groups, sub-block sums, block energies and records 8-byte aligned");
        return AFG_ERR_INVALID;
    }
    if (n_groups > 0x7fffffffull) {
        afg::set_error("afg_loudness_hip: at most 2^31 - 1 groups per launch");
        return AFG_ERR_INVALID;
    }
    if (in_floats > (~(uint64_t)0 >> 3) || out_floats > (~(uint64_t)0 >> 3)) {
        afg::set_error("afg_loudness_hip: a plane of 2^61 floats or more");
        return AFG_ERR_INVALID;
    }
    // the planes as byte ranges: the same plane, or apart
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + in_floats * 4, b0 = (uintptr_t)d_out, b1 = b0 + out_floats * 4;
    if (params->apply && d_out && a0 != b0 && in_floats && out_floats && a0 < b1 && b0 < a1) {
        afg::set_error("afg_loudness_hip: the output plane overlaps the input plane without being the same");
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// the device copy of a rate's K-weighting tables, made once per device and rate and kept
int tables_for(uint32_t samplerate, const double **d_tab)
{
    static std::mutex mu;
    static std::map<uint32_t, double *> cache[AFG_MAX_DEVICES];
    int dev = 0;
    if (int rc = afg::device_slot(&dev, "afg_loudness_hip")) return rc;
    std::lock_guard<std::mutex> lk(mu);
    auto &mine = cache[dev];
    auto it = mine.find(samplerate);
    if (it != mine.end()) { *d_tab = it->second; return AFG_OK; }
    afg_filter_params kw;
    if (int rc = afg::loudness_kweight(samplerate, &kw)) return rc;
    std::vector<double> tab;
    afg::filter_tables(&kw, tab);
    double *d = nullptr;
    AFG_HIP_CHECK(hipMalloc((void **)&d, tab.size() * sizeof(double)));
    if (hipMemcpy(d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        afg::set_error("afg_loudness_hip: the table upload failed");
        return AFG_ERR_HIP;
    }
    mine.emplace(samplerate, d);
    *d_tab = d;
    return AFG_OK;
}

}  // namespace

int afg::loudness_launch(const afg_loudness_group *h_groups, uint64_t n_groups, const afg_loudness_group *d_groups, const afg_loudness_counts *counts,
                         const afg_loudness_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats,
                         double *d_sub, double *d_blocks, afg_loudness_stats *d_stats, hipStream_t stream)
{
    if (int rc = afg::loudness_check_params(params)) return rc;  // the parameters count without groups too
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, counts, params, d_in, in_floats, d_out, out_floats, d_sub, d_blocks, d_stats)) return rc;
    if (int rc = afg_loudness_check_groups(h_groups, n_groups, counts, params, in_floats, out_floats, d_in == d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    GateArgs a;
    a.step = afg::loudness_step(params->samplerate);
    a.max_peak = params->max_peak; a.max_gain = params->max_gain;
    bool any = false;
    for (int k = 0; k < 8; k++) any = any || params->weights[k] != 0.0;
    for (int k = 0; k < 8; k++) a.weights[k] = any ? params->weights[k] : 1.0;
    a.gamma_abs = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    a.target_energy = std::pow(10.0, (params->target_lufs + 0.691) / 10.0);
    uint32_t max_rows = 0, max_valid = 0;
    for (uint64_t k = 0; k < n_groups; k++)
        if (h_groups[k].valid) { max_rows = std::max(max_rows, h_groups[k].rows); max_valid = std::max(max_valid, h_groups[k].valid); }
    const uint32_t ng = (uint32_t)n_groups;
    if (max_rows) {
        const double *d_tab = nullptr;
        if (int rc = tables_for(params->samplerate, &d_tab)) return rc;
        hipLaunchKernelGGL(loudness_measure_kernel, dim3(ng, max_rows), dim3(kThreads), 0, stream, d_groups, a.step, d_tab, d_in, d_sub);
    }
    hipLaunchKernelGGL(loudness_gate_kernel, dim3(ng), dim3(64), 0, stream, d_groups, a, (const double *)d_sub, d_blocks, d_stats);
    if (params->apply && max_rows) {
        const uint32_t z = std::min<uint32_t>(kApplyZ, (uint32_t)(((uint64_t)max_valid + kTile - 1) / kTile));
        hipLaunchKernelGGL(loudness_apply_kernel, dim3(ng, max_rows, z), dim3(kThreads), 0, stream, d_groups, (const afg_loudness_stats *)d_stats,
                           d_in, d_out);
    }
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_loudness_hip(uint64_t n_groups, const afg_loudness_group *d_groups, const afg_loudness_counts *counts,
                                const afg_loudness_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats,
                                double *d_sub, double *d_blocks, afg_loudness_stats *d_stats, void *hip_stream)
{
    if (int rc = afg::loudness_check_params(params)) return rc;
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, counts, params, d_in, in_floats, d_out, out_floats, d_sub, d_blocks, d_stats)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_groups, n_groups, (hipStream_t)hip_stream, [&](const afg_loudness_group *h) {
        return afg::loudness_launch(h, n_groups, d_groups, counts, params, d_in, in_floats, d_out, out_floats, d_sub, d_blocks, d_stats,
                                    (hipStream_t)hip_stream);
    });
}
