// yin.hip -- the YIN fundamental frequency per frame (afg_yin_hip), for gfx950: the value include/afg.h defines, bit for bit
// -- the difference function as float32 fmaf chains in ascending sample order, the cumulative mean in float64 in chunks of
// AFG_YIN_CHUNK lags, the first trough under the threshold or else the first global minimum, the parabolic refinement in
// float64.  Nothing is free: tests/yin_model.py restates every step and the result is compared as bit patterns.
//
// One workgroup of 256 lanes (four wavefronts) per tile of kTile = AFG_YIN_TILE = 4 frames of one row (afg_mel_row), found
// by the search over the rows' first tiles that the other stages use.
//   stage      samples 0 .. W - 1 + tau_max of every frame of the tile into X[f][.] in LDS, the padding resolved on the way
//              in (reflect without the edge, or +0.0f), +0.0f behind them up to the pitch.  A frame has its own segment
//              (pitch a multiple of 4 floats), so that every read below is an aligned ds_read_b128 whatever the hop.
//   difference a lane owns 4 consecutive lags 4 g .. 4 g + 3 of one frame (lag 0 and the lags above tau_max ride along and
//              are never looked at): 4 independent fmaf chains.  Per 4 samples it reads x_j .. x_(j+3) (one address per
//              frame: a broadcast) and x_(j + 4 g + 4) .. x_(j + 4 g + 7) (consecutive lanes, consecutive 16 bytes: no bank
//              conflict), keeps the previous 4 in registers, and makes 16 subtract-and-fmaf pairs: 2 LDS reads per 32
//              vector operations.  The units (frame, g) are dealt to the 256 lanes in turn; a wavefront without units in a
//              round skips it.
//   mean       a wavefront per frame.  A lane sums its chunks' 16 lags in float64 in lag order; lane 0 turns the chunk totals
//              into their exclusive prefix B_c, at most 256 dependent adds; the lanes walk their chunks again (the same adds,
//              the same bits) and put d' over d in LDS.  A NaN d' raises the frame's flag.
//   choice     lanes along tau: the first lag per lane with trough and d' < threshold, the first strict minimum per lane,
//              reduced over the wavefront with ties to the smaller tau; lane 0 refines and stores the frame's two floats.
// No atomics, no scratch.
//
// Bounds: every row is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + g] for 0 <= g < in_frames only and writes out[out_off .. out_off + 2 * out_frames) only.
#include "mel_rows.h"

#include <cmath>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_YIN_TILE;                         // frames per tile: one per wavefront in the mean and the choice
constexpr uint32_t kLags = 4;                                    // lags per lane
constexpr uint32_t kNaN = 0x7fc00000u;

static_assert(sizeof(afg_yin_params) == 48 && sizeof(afg_mel_row) == 32, "include/afg.h");
static_assert(kTile == kThreads / 64, "a wavefront per frame");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// LDS: X[kTile][xp] floats, D[kTile][dp] floats, S[kTile][chunks] doubles
struct YinGeo {
    uint32_t G;                                                 // lag groups of kLags: lags 0 .. kLags * G - 1 >= tau_max
    uint32_t xp, dp, chunks;
    uint32_t d_at, s_at, lds_floats;                            // float offsets (s_at a multiple of 4)
};

// (params already checked: afg::yin_check_params)
YinGeo geo_of(const afg_yin_params &p)
{
    YinGeo g;
    g.G = p.tau_max / kLags + 1;
    g.dp = kLags * g.G;
    g.xp = ((p.win_length + 3) & ~3u) + g.dp;                   // the last read: sample roundup4(W) - 1 + kLags * G
    g.chunks = (p.tau_max + AFG_YIN_CHUNK - 1) / AFG_YIN_CHUNK;
    g.d_at = kTile * g.xp;
    g.s_at = g.d_at + kTile * g.dp;
    g.lds_floats = g.s_at + 2 * kTile * g.chunks;
    return g;
}

__global__ __launch_bounds__(kThreads) void yin_kernel(uint32_t n_rows, const afg_mel_row *__restrict__ rows, afg_yin_params prm, YinGeo geo,
                                                       const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint64_t tile = blockIdx.x;
    // the row of this tile: the last one whose first tile is <= tile (rows without output have no tiles)
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_mel_row::first_tile);
    const afg_mel_row r = rows[lo];
    if (r.first_tile > tile) return;
    const uint64_t t0 = (tile - r.first_tile) * kTile;          // first frame of the tile
    if (t0 >= r.out_frames) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, r.out_frames - t0);
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t W = prm.win_length, tau_min = prm.tau_min, tau_max = prm.tau_max;
    float *const X = lds, *const D = lds + geo.d_at;
    double *const S = (double *)(lds + geo.s_at);

    // ---- X: sample j of frame f at X[f * xp + j]; +0.0f from W + tau_max on
    {
        const int64_t nin = r.in_frames;
        const int64_t pad = prm.center ? prm.frame_length / 2 : 0;
        const uint32_t span = W + tau_max;
        const float *x = in + r.in_off;
        for (uint32_t f = wave; f < n; f += kThreads / 64) {
            const int64_t s0 = (int64_t)(t0 + f) * prm.hop - pad;
            float *row = X + f * geo.xp;
            for (uint32_t j = lane; j < geo.xp; j += 64) {
                float v = 0.0f;
                if (j < span) {
                    int64_t s = s0 + j;
                    if (prm.pad_mode == AFG_MEL_PAD_REFLECT) {  // in_frames > pad (check_rows): one fold lands inside
                        if (s < 0) s = -s;
                        else if (s >= nin) s = 2 * (nin - 1) - s;
                    }
                    if (s >= 0 && s < nin) v = x[s];
                }
                row[j] = v;
            }
        }
    }
    __syncthreads();

    // ---- d: unit u = f * G + g is lags 4 g .. 4 g + 3 of frame f
    for (uint32_t u = threadIdx.x; u < n * geo.G; u += kThreads) {
        const uint32_t f = u / geo.G, g = u - f * geo.G;
        const f32x4 *xb = (const f32x4 *)(X + f * geo.xp);      // x_j
        const f32x4 *xl = xb + g;                               // x_(j + 4 g)
        float a[kLags] = { 0.0f, 0.0f, 0.0f, 0.0f };
        f32x4 cur = xl[0];
        const uint32_t whole = W >> 2, rest = W & 3;
        for (uint32_t q = 0; q < whole; q++) {
            const f32x4 nxt = xl[q + 1], b = xb[q];
            const float w[8] = { cur[0], cur[1], cur[2], cur[3], nxt[0], nxt[1], nxt[2], nxt[3] };
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float e = b[i] - w[i + k];
                    a[k] = fmaf(e, e, a[k]);
                }
            cur = nxt;
        }
        if (rest) {                                              // (uniform)
            const f32x4 nxt = xl[whole + 1], b = xb[whole];
            const float w[8] = { cur[0], cur[1], cur[2], cur[3], nxt[0], nxt[1], nxt[2], nxt[3] };
#pragma unroll
            for (int i = 0; i < 3; i++)
                if ((uint32_t)i < rest)
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float e = b[i] - w[i + k];
                        a[k] = fmaf(e, e, a[k]);
                    }
        }
        *(f32x4 *)(D + f * geo.dp + kLags * g) = f32x4{ a[0], a[1], a[2], a[3] };
    }
    __syncthreads();

    // ---- d': wavefront f has frame f; every barrier below is met by all four
    const bool has = wave < n;
    float *const d = D + wave * geo.dp;
    double *const sc = S + wave * geo.chunks;
    if (has)
        for (uint32_t c = lane; c < geo.chunks; c += 64) {
            double p = 0.0;
            const uint32_t first = c * AFG_YIN_CHUNK + 1, last = min(first + AFG_YIN_CHUNK - 1, tau_max);
            for (uint32_t tau = first; tau <= last; tau++) p = p + (double)d[tau];
            sc[c] = p;
        }
    __syncthreads();
    if (has && lane == 0) {
        double run = 0.0;
        for (uint32_t c = 0; c < geo.chunks; c++) {
            const double t = sc[c];
            sc[c] = run;
            run = run + t;
        }
    }
    __syncthreads();
    bool bad = false;
    if (has)
        for (uint32_t c = lane; c < geo.chunks; c += 64) {
            double p = 0.0;
            const double base = sc[c];
            const uint32_t first = c * AFG_YIN_CHUNK + 1, last = min(first + AFG_YIN_CHUNK - 1, tau_max);
            for (uint32_t tau = first; tau <= last; tau++) {
                const float dv = d[tau];
                p = p + (double)dv;
                const double s = base + p;
                const float v = s == 0.0 ? 1.0f : (float)((double)dv * (double)tau / s);
                d[tau] = v;
                bad = bad || v != v;
            }
        }
    __syncthreads();
    if (!has) return;
    const bool any_nan = __ballot(bad) != 0;

    // ---- tau*
    uint32_t first = 0xffffffffu, bt = 0xffffffffu;
    float bv = INFINITY;
    for (uint32_t tau = tau_min + lane; tau <= tau_max; tau += 64) {
        const float v = d[tau];
        bool trough = false;
        if (tau_min != tau_max) {
            if (tau == tau_min) trough = v < d[tau + 1];
            else if (tau < tau_max) trough = v < d[tau - 1] && v <= d[tau + 1];
        }
        if (trough && v < prm.threshold && first == 0xffffffffu) first = tau;
        if (v < bv) { bv = v; bt = tau; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        first = min(first, (uint32_t)__shfl_xor((int)first, s, 64));
        const float ov = __shfl_xor(bv, s, 64);
        const uint32_t ot = (uint32_t)__shfl_xor((int)bt, s, 64);
        if (ov < bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; }
    }
    if (lane != 0) return;
    const uint32_t ts = first != 0xffffffffu ? first : (bt != 0xffffffffu ? bt : tau_min);
    const float b = d[ts];
    double shift = 0.0;
    if (ts > tau_min && ts < tau_max) {
        const double a = (double)d[ts - 1], c = (double)d[ts + 1];
        const double A = (c + a) - 2.0 * (double)b, B = (c - a) * 0.5;
        if (fabs(B) < fabs(A)) shift = -B / A;
    }
    float f0 = (float)(prm.samplerate / ((double)ts + shift)), dm = b;
    if (any_nan) f0 = dm = __uint_as_float(kNaN);
    float *y = out + r.out_off + t0 + wave;
    y[0] = f0;
    y[r.out_frames] = dm;
}

// every row against the planes and the tile table, before anything runs
int check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_yin_params &p, uint64_t in_floats, uint64_t out_floats)
{
    const uint32_t pad = p.center ? p.frame_length / 2 : 0;
    return afg::check_mel_rows("afg_yin_hip", "afg_yin_layout", rows, n_rows, n_tiles, kTile, p.pad_mode == AFG_MEL_PAD_REFLECT ? pad : 0, 2, in_floats,
                               out_floats, [&](uint32_t in_frames) { return afg::yin_frames_of(p, in_frames); });
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const float *d_in, float *d_out)
{
    if (!d_rows || !d_out) {
        afg::set_error("afg_yin_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_yin_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_yin_hip", "rows", n_rows, n_tiles);
}

}  // namespace

int afg::yin_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_yin_params *params,
                    const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, hipStream_t stream)
{
    if (int rc = afg::yin_check_params(params, "afg_yin_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_out)) return rc;
    if (int rc = check_rows(h_rows, n_rows, n_tiles, *params, in_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (!d_in) { afg::set_error("afg_yin_hip: NULL d_in with rows that have frames"); return AFG_ERR_INVALID; }
    if (int rc = afg::require_device()) return rc;
    const YinGeo g = geo_of(*params);
    const size_t bytes = (size_t)g.lds_floats * sizeof(float);
    if (bytes > 160 * 1024) {                                    // (frame_length <= 4096 stays below: 4 * (4106 + 4098 + 512) floats)
        afg::set_error("afg_yin_hip: frame_length %u needs %u floats of LDS", params->frame_length, g.lds_floats);
        return AFG_ERR_INVALID;
    }
    AFG_HIP_CHECK(hipFuncSetAttribute((const void *)yin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(yin_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), bytes, stream, (uint32_t)n_rows, d_rows, *params, g, d_in, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_yin_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_yin_params *params, const float *d_in,
                           uint64_t in_floats, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = afg::yin_check_params(params, "afg_yin_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_mel_row *h) {
        return afg::yin_launch(h, n_rows, d_rows, n_tiles, params, d_in, in_floats, d_out, out_floats, (hipStream_t)hip_stream);
    });
}
