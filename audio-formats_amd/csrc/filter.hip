// filter.hip -- cascades of second-order recursive sections over float rows (afg_filter_hip, afg_batch_decode_filtered), for
// gfx950.  The definition, the interval the result is held to and the constant K in it are in include/afg.h; the host half
// (coefficient helper, bound, checks, the tables, the batch entry) is host/afg_filter.cpp.
//
// One launch, one workgroup of 256 lanes per row, no atomics and nothing that waits for another workgroup.  The workgroup
// walks its row in tiles of 4096 frames:
//   fetch    the tile comes in as dwordx4 at dword alignment (lane l takes 16-byte words l, 256 + l ..: coalesced), one tile
//            ahead of the arithmetic, and goes to LDS with every 16 floats followed by 4 of padding, so that
//   chunk    lane l reads its 16 consecutive frames as four ds_read_b128 at a lane stride of 20 dwords (16 lanes of a read
//            group on 16 different bank quads; a stride of 16 would put them on four) and widens them to float64.
//   section  per section, with A = [-a1 -a2; 1 0] the step of the state (v[n-1], v[n-2]):
//            the lane runs v[n] = b0 u[n] + b1 u[n-1] + b2 u[n-2] - a1 v[n-1] - a2 v[n-2] over its chunk from a zero v state
//            with the true u history -- the lane below holds it (one shuffle), the wavefront below left it in the state it
//            started from, the tile before in the carry --; the chunks' end states e meet in a log-step scan of
//            s -> A^16 s + e inside the wavefront (six steps, powers A^(16 d) from the host's table, a lane below the step
//            keeps its value: nothing flows downwards, so a NaN reaches only what lies behind it); the four wavefront
//            totals meet through LDS behind the section's one barrier, each wavefront folding the ones below it onto the
//            tile's carry; a lane's incoming state is A^(16 i) times its wavefront's plus the scan's value of the lane
//            below, and goes onto the chunk through the two homogeneous responses of length 16 (host table, scalar
//            loads).  The corrected chunk is the next section's input; lane 255 leaves (u, v) history for the next tile.
//   store    the last section is rounded once to float32 and goes back through the same LDS layout as dwordx4; a short last
//            tile was filled with zeros behind its frames, stores only the frames it has and takes the outgoing state from
//            the lane and frame where they end.
// Every fused multiply-add is written as one (the Makefile's -ffp-contract=off does not touch them).
//
// Bounds: every row is checked on the host before the launch (afg_filter_check_rows); the kernel relies on it.  It reads
// in[in_off + e] and writes out[out_off + e] for e < frames only, d_state[(row * n_sections + s) * 4 ..+ 4) for rows with
// frames, the cascade's table inside n_sections * 300 doubles.
#include "afg_records.h"

#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_FILTER_TILE, kChunk = AFG_FILTER_CHUNK, kPad = 20;      // kPad: dwords from one lane's chunk to the next in LDS
constexpr uint32_t kMaxSec = AFG_FILTER_MAX_SECTIONS;
constexpr uint32_t kH1 = afg::kFilterH1, kH2 = afg::kFilterH2, kPow = afg::kFilterPow, kSec = afg::kFilterSecDoubles;

static_assert(kTile == kThreads * kChunk && kChunk == 16, "include/afg.h");
static_assert(sizeof(afg_filter_row) == 24 && sizeof(afg_biquad) == 40 && sizeof(afg_filter_params) == 328, "include/afg.h");
static_assert(kPow + 4 * 65 == kSec, "afg_common.h");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a dwordx4 at dword alignment

__device__ __forceinline__ double dfma(double a, double b, double c) { return __builtin_fma(a, b, c); }

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

__global__ __launch_bounds__(kThreads) void filter_kernel(const afg_filter_row *__restrict__ rows, uint32_t nsec, const double *__restrict__ tab,
                                                          const float *in, float *out, double *state)
{
    __shared__ __attribute__((aligned(16))) float sh_tile[kThreads * kPad];
    __shared__ __attribute__((aligned(16))) double sh_pow[kMaxSec * 64 * 4];     // A^(16 i), i < 64, per section
    __shared__ double sh_wave[2][4][2];                          // by section parity: the wavefronts' totals
    __shared__ double sh_carry[2][kMaxSec][4];                   // by tile parity: u[n-1], u[n-2], v[n-1], v[n-2] in front of the tile
    const afg_filter_row row = rows[blockIdx.x];
    if (row.frames == 0) return;
    const uint32_t lane = threadIdx.x, i = lane & 63u, w = lane >> 6;
    for (uint32_t k = lane; k < nsec * 256u; k += kThreads) sh_pow[k] = tab[(k >> 8) * kSec + kPow + (k & 255u)];
    double *const my_state = state ? state + (uint64_t)blockIdx.x * nsec * 4u : nullptr;
    if (lane < nsec * 4u) sh_carry[0][lane >> 2][lane & 3u] = my_state ? my_state[lane] : 0.0;
    const float *const x = in + row.in_off;
    float *const y = out + row.out_off;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)row.frames + kTile - 1) / kTile);
    f32x4 pre[4];
    fetch_tile(pre, x, min(row.frames, kTile), lane);
    for (uint32_t t = 0; t < n_tiles; t++) {
        const uint64_t t0 = (uint64_t)t * kTile;
        const uint32_t nt = (uint32_t)min((uint64_t)kTile, (uint64_t)row.frames - t0), par = t & 1u;
        const bool last = t + 1 == n_tiles;
        if (t) __syncthreads();                                  // the tile before has left LDS
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t e = 4u * (k * kThreads + lane);
            *(f32x4 *)&sh_tile[(e >> 4) * kPad + (e & 15u)] = pre[k];
        }
        __syncthreads();
        if (!last) fetch_tile(pre, x + t0 + kTile, (uint32_t)min((uint64_t)kTile, (uint64_t)row.frames - t0 - kTile), lane);
        double xs[kChunk];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f32x4 v = *(const f32x4 *)&sh_tile[lane * kPad + 4 * q];
            xs[4 * q] = (double)v.x; xs[4 * q + 1] = (double)v.y; xs[4 * q + 2] = (double)v.z; xs[4 * q + 3] = (double)v.w;
        }
        const uint32_t l_end = (nt - 1) >> 4, j_end = (nt - 1) & 15u;   // where the tile's frames end
        double Pa = 0.0, Pb = 0.0;                               // the state this wavefront started the section before from
        for (uint32_t s = 0; s < nsec; s++) {
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
            double su1 = 0.0, su2 = 0.0;                         // the input's history behind the tile's last frame
            if (last && my_state) {
#pragma unroll
                for (int n = 0; n < (int)kChunk; n++)
                    if ((uint32_t)n == j_end) { su1 = xs[n]; su2 = n ? xs[n > 0 ? n - 1 : 0] : p1; }
            }
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
                const double nb = dfma(M64[2], Pa, dfma(M64[3], Pb, sh_wave[s & 1u][v][1]));
                Pa = na; Pb = nb;
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
            if (last && my_state && lane == l_end) {
                double sv1 = 0.0, sv2 = 0.0;
#pragma unroll
                for (int n = 0; n < (int)kChunk; n++)
                    if ((uint32_t)n == j_end) { sv1 = xs[n]; sv2 = n ? xs[n > 0 ? n - 1 : 0] : Sa; }
                my_state[4 * s] = su1; my_state[4 * s + 1] = su2; my_state[4 * s + 2] = sv1; my_state[4 * s + 3] = sv2;
            }
        }
        // the chunk goes back, rounded once
#pragma unroll
        for (int q = 0; q < 4; q++)
            *(f32x4 *)&sh_tile[lane * kPad + 4 * q] = f32x4{ (float)xs[4 * q], (float)xs[4 * q + 1], (float)xs[4 * q + 2], (float)xs[4 * q + 3] };
        __syncthreads();
        float *const yt = y + t0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t e = 4u * (k * kThreads + lane);
            const f32x4 v = *(const f32x4 *)&sh_tile[(e >> 4) * kPad + (e & 15u)];
            if (e + 4 <= nt) {
                *(f32x4u *)(yt + e) = v;
            } else {
                if (e < nt) yt[e] = v.x;
                if (e + 1 < nt) yt[e + 1] = v.y;
                if (e + 2 < nt) yt[e + 2] = v.z;
            }
        }
    }
}

int check_args(uint64_t n_rows, const afg_filter_row *d_rows, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats,
               const double *d_state)
{
    if (!d_rows || !d_in || !d_out) {
        afg::set_error("afg_filter_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || ((uintptr_t)d_rows & 7u) != 0 || ((uintptr_t)d_state & 7u) != 0) {
        afg::set_error("afg_filter_hip: the planes must be 4-byte aligned, the rows and the state 8-byte aligned");
        return AFG_ERR_INVALID;
    }
    if (n_rows > 0x7fffffffull) {
        afg::set_error("afg_filter_hip: at most 2^31 - 1 rows per launch");
        return AFG_ERR_INVALID;
    }
    if (in_floats > (~(uint64_t)0 >> 3) || out_floats > (~(uint64_t)0 >> 3)) {
        afg::set_error("afg_filter_hip: a plane of 2^61 floats or more");
        return AFG_ERR_INVALID;
    }
    // the planes as byte ranges: the same plane, or apart
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + in_floats * 4, b0 = (uintptr_t)d_out, b1 = b0 + out_floats * 4;
    if (a0 != b0 && in_floats && out_floats && a0 < b1 && b0 < a1) {
        afg::set_error("afg_filter_hip: the output plane overlaps the input plane without being the same");
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// the device copy of a cascade's tables, made once per device and distinct cascade and kept (64 at the most, then all are
// let go: hipFree waits for the kernels that read them)
int tables_for(const afg_filter_params *params, const double **d_tab)
{
    static std::mutex mu;
    static std::map<std::string, double *> cache[AFG_MAX_DEVICES];
    int dev = 0;
    if (int rc = afg::device_slot(&dev, "afg_filter_hip")) return rc;
    const std::string key((const char *)params->sec, (size_t)params->n_sections * sizeof(afg_biquad));
    std::lock_guard<std::mutex> lk(mu);
    auto &mine = cache[dev];
    auto it = mine.find(key);
    if (it != mine.end()) { *d_tab = it->second; return AFG_OK; }
    if (mine.size() >= 64) {
        for (auto &e : mine) (void)hipFree(e.second);
        mine.clear();
    }
    std::vector<double> tab;
    afg::filter_tables(params, tab);
    double *d = nullptr;
    AFG_HIP_CHECK(hipMalloc((void **)&d, tab.size() * sizeof(double)));
    if (hipMemcpy(d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        afg::set_error("afg_filter_hip: the table upload failed");
        return AFG_ERR_HIP;
    }
    mine.emplace(key, d);
    *d_tab = d;
    return AFG_OK;
}

}  // namespace

int afg::filter_launch(const afg_filter_row *h_rows, uint64_t n_rows, const afg_filter_row *d_rows, const afg_filter_params *params,
                       const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_state, hipStream_t stream)
{
    if (int rc = afg::filter_check_params(params)) return rc;  // the parameters count without rows too
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, d_in, in_floats, d_out, out_floats, d_state)) return rc;
    if (int rc = afg_filter_check_rows(h_rows, n_rows, params, in_floats, out_floats, d_in == d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    const double *d_tab = nullptr;
    if (int rc = tables_for(params, &d_tab)) return rc;
    hipLaunchKernelGGL(filter_kernel, dim3((uint32_t)n_rows), dim3(kThreads), 0, stream, d_rows, params->n_sections, d_tab, d_in, d_out, d_state);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_filter_hip(uint64_t n_rows, const afg_filter_row *d_rows, const afg_filter_params *params, const float *d_in,
                              uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_state, void *hip_stream)
{
    if (int rc = afg::filter_check_params(params)) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, d_in, in_floats, d_out, out_floats, d_state)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_filter_row *h) {
        return afg::filter_launch(h, n_rows, d_rows, params, d_in, in_floats, d_out, out_floats, d_state, (hipStream_t)hip_stream);
    });
}
