// resample.hip -- planar float rows at a file's sample rate to rows at the caller's rate, with an optional mono mix of the
// file's rows on the way in (afg_resample_hip, afg_batch_decode_resampled), for gfx950.  The definition -- a polyphase
// Hann-windowed sinc, every product and every add rounded to float32, no fused multiply-add -- is in include/afg.h;
// the Makefile builds this file with -ffp-contract=off like every other exact-mode kernel.
//
// Work: K = 2 W taps (14 .. 38 for audio rates, 146 for 96 kHz -> 8 kHz) per output float, two LDS reads, one multiply and
// one add each.  One workgroup of 256 lanes per tile of one output row (afg_resample_row), found by a search over the rows'
// first tiles (uniform per workgroup), as collate.hip does.  A tile is 1024 output frames, halved down to 64 while its input
// window -- floor(tile * M / L) + 2 W + 1 frames -- exceeds 4096 floats, so that window (16 KiB) and table (24 KiB) leave room
// for four workgroups per compute unit.
//   window   staged in LDS with coalesced loads, the file's rows mixed on the way in; frames outside [0, in_frames) are
//            staged as +0.0f and never read from memory (acc + h * 0 has the bits of acc: acc is never -0)
//   table    copied to LDS when L * K <= 6144 floats (every rate pair of 8 / 16 / 22.05 / 44.1 / 48 kHz); larger tables
//            (44101 -> 16000: 544 000 floats) are read through L2.  With L == 1 all lanes read the same tap: a broadcast
//   lanes    take consecutive t, so a wavefront stores whole lines; the one division per output is 32-bit
//   W == 0   equal rates: a copy of words (or the mix), no LDS
// A ratio so steep that 64 frames' window does not fit (M / L above about 54) is computed from global memory, lane by
// lane: correct, slow, and outside what audio rates ask for.
//
// Bounds: every row is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + r * in_stride + g] for r < in_rows and 0 <= g < in_frames only, taps[taps_off .. taps_off + L * K) only, and
// writes out[out_off .. out_off + out_frames) only.
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTileMax = 1024, kTileMin = 64;             // output frames per tile
constexpr uint32_t kWindow = 4096;                              // floats of LDS for a tile's input window
constexpr uint32_t kTapsLds = 6144;                             // a table up to this many floats is copied to LDS
constexpr uint32_t kMaxRatio = 1u << 20;                        // M and L: r0 + 1023 * M stays below 2^32
constexpr uint32_t kMaxW = 1u << 21;
constexpr uint64_t kMaxTable = (uint64_t)1 << 22;               // what afg_resample_taps makes at the most
constexpr int64_t kMaxFrame = (int64_t)1 << 61;                 // |in_frame0| below this: no sum in the kernel wraps

// the input frames the outputs of a tile of n frames may touch, whatever phase the tile starts with
__host__ __device__ inline uint64_t window_of(uint32_t n, uint32_t M, uint32_t L, uint32_t W)
{
    return (uint64_t)n * M / L + 2ull * W + 1;
}

__host__ __device__ inline uint32_t tile_frames(uint32_t M, uint32_t L, uint32_t W)
{
    uint32_t n = kTileMax;
    while (W && n > kTileMin && window_of(n, M, L, W) > kWindow) n >>= 1;
    return n;
}

// frame g (inside the rows) of the mix of the record's rows
__device__ __forceinline__ float mix_at(const float *__restrict__ in, const afg_resample_row &r, int64_t g)
{
    const float *p = in + r.in_off + (uint64_t)g;
    float s = p[0];
    if (r.in_rows == 1) return s;
    for (uint32_t k = 1; k < r.in_rows; k++) s = s + p[(uint64_t)k * r.in_stride];
    return s / (float)r.in_rows;
}

// outputs [0, n) of a tile whose first output has phase r0 and whose window begins at input frame wbeg (win[0])
template <bool kTabLds, bool kStaged>
__device__ __forceinline__ void fir_tile(const afg_resample_row &r, const float *__restrict__ in, const float *__restrict__ h,
                                         const float *tab, const float *win, int64_t wbeg, uint32_t r0, uint32_t n, float *__restrict__ y)
{
    const uint32_t K = 2 * r.W;
    const int64_t nin = r.in_frames;
    for (uint32_t j = threadIdx.x; j < n; j += kThreads) {
        const uint32_t x = r0 + j * r.M, dq = x / r.L, p = x - dq * r.L;
        float acc = 0.0f;
        if (kStaged) {
            const float *w = win + dq;
            if (kTabLds) {
                const float *hp = tab + p * K;
                for (uint32_t k = 0; k < K; k++) acc = acc + hp[k] * w[k];
            } else {
                const float *hp = h + (uint64_t)p * K;
                for (uint32_t k = 0; k < K; k++) acc = acc + hp[k] * w[k];
            }
        } else {
            const float *hp = h + (uint64_t)p * K;
            const int64_t g0 = wbeg + dq;
            for (uint32_t k = 0; k < K; k++) {
                const int64_t g = g0 + k;
                const float v = (g >= 0 && g < nin) ? mix_at(in, r, g) : 0.0f;
                acc = acc + hp[k] * v;
            }
        }
        y[j] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void resample_kernel(uint32_t n_rows, const afg_resample_row *__restrict__ rows,
                                                            const float *__restrict__ in, const float *__restrict__ taps,
                                                            float *__restrict__ out)
{
    __shared__ float win[kWindow];
    __shared__ float tab[kTapsLds];
    const uint64_t tile = blockIdx.x;
    // the row of this tile: the last one whose first tile is <= tile (rows without output have no tiles)
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_resample_row::first_tile);
    const afg_resample_row r = rows[lo];
    if (r.first_tile > tile) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t nt = tile_frames(r.M, r.L, r.W);
    const uint64_t t0 = (tile - r.first_tile) * nt;              // first output frame of the tile
    if (t0 >= r.out_frames) return;
    const uint32_t n = (uint32_t)min((uint64_t)nt, r.out_frames - t0);
    float *y = out + r.out_off + t0;
    const int64_t nin = r.in_frames;
    if (r.W == 0) {                                              // equal rates: the words as they are, or the mix
        const int64_t q0 = r.in_frame0 + (int64_t)t0;
        for (uint32_t j = lane; j < n; j += kThreads) {
            const int64_t q = q0 + j;
            if (q < 0 || q >= nin) y[j] = 0.0f;
            else if (r.in_rows == 1) ((uint32_t *)y)[j] = ((const uint32_t *)in)[r.in_off + (uint64_t)q];
            else y[j] = mix_at(in, r, q);
        }
        return;
    }
    const uint32_t K = 2 * r.W;
    const uint64_t pos0 = t0 * r.M;                              // below 2^52
    const uint64_t q0 = pos0 / r.L;
    const uint32_t r0 = (uint32_t)(pos0 - q0 * r.L);
    const int64_t wbeg = r.in_frame0 + (int64_t)q0 - (int64_t)(r.W - 1);
    const uint32_t wlen = (r0 + (n - 1) * r.M) / r.L + K;       // <= window_of(nt, ...)
    if (nin == 0 || wbeg >= nin || wbeg + (int64_t)wlen <= 0) {  // nothing of the row under the window
        for (uint32_t j = lane; j < n; j += kThreads) y[j] = 0.0f;
        return;
    }
    const float *h = taps + r.taps_off;
    const uint32_t tab_floats = r.L * K;                         // <= 2^22 (check_rows)
    const bool tab_lds = tab_floats <= kTapsLds;
    const bool staged = window_of(nt, r.M, r.L, r.W) <= kWindow;
    if (tab_lds)
        for (uint32_t i = lane; i < tab_floats; i += kThreads) tab[i] = h[i];
    if (staged)
        for (uint32_t i = lane; i < wlen; i += kThreads) {
            const int64_t g = wbeg + i;
            win[i] = (g >= 0 && g < nin) ? mix_at(in, r, g) : 0.0f;
        }
    __syncthreads();
    if (!staged) fir_tile<false, false>(r, in, h, tab, win, wbeg, r0, n, y);
    else if (tab_lds) fir_tile<true, true>(r, in, h, tab, win, wbeg, r0, n, y);
    else fir_tile<false, true>(r, in, h, tab, win, wbeg, r0, n, y);
}

uint64_t tiles_of(const afg_resample_row &r)
{
    if (r.out_frames == 0 || r.M == 0 || r.L == 0) return 0;
    const uint32_t nt = tile_frames(r.M, r.L, r.W);
    return ((uint64_t)r.out_frames + nt - 1) / nt;
}

// every row against the planes and the tile table, before anything runs
int check_rows(const afg_resample_row *rows, uint64_t n_rows, uint64_t n_tiles, bool have_in, uint64_t in_floats, bool have_taps,
               uint64_t taps_floats, uint64_t out_floats)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; k < n_rows; k++) {
        const afg_resample_row &r = rows[k];
        const unsigned long long kk = (unsigned long long)k;
        if (r.first_tile != tiles) {
            afg::set_error("afg_resample_hip: row %llu: first_tile %llu, afg_resample_layout gives %llu", kk, (unsigned long long)r.first_tile,
                           (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        if (r.M == 0 || r.L == 0 || r.M > kMaxRatio || r.L > kMaxRatio || r.W > kMaxW || (r.W == 0 && (r.M != 1 || r.L != 1))) {
            afg::set_error("afg_resample_hip: row %llu: M %u, L %u, W %u: M and L are 1 .. 2^20, W at most 2^21, and W == 0 goes with M == L == 1", kk, r.M, r.L, r.W);
            return AFG_ERR_INVALID;
        }
        if (r.in_frame0 <= -kMaxFrame || r.in_frame0 >= kMaxFrame) {
            afg::set_error("afg_resample_hip: row %llu: |in_frame0| must be below 2^61", kk);
            return AFG_ERR_INVALID;
        }
        tiles += tiles_of(r);
        if (r.out_frames && !afg::rows_inside(r.out_off, 1, 0, r.out_frames, out_floats)) {
            afg::set_error("afg_resample_hip: row %llu: the row leaves the output (%llu floats)", kk, (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
        if (r.in_frames == 0) continue;
        if (r.in_rows == 0 || r.in_rows > 0xffff) {
            afg::set_error("afg_resample_hip: row %llu: in_rows %u: 1 .. 65535", kk, r.in_rows);
            return AFG_ERR_INVALID;
        }
        if (!have_in || !afg::rows_inside(r.in_off, r.in_rows, r.in_stride, r.in_frames, in_floats)) {
            afg::set_error("afg_resample_hip: row %llu: the input rows leave the input (%llu floats)", kk, (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        if (r.W == 0) continue;
        const uint64_t table = (uint64_t)r.L * 2 * r.W;
        if (!have_taps || table > kMaxTable || !afg::rows_inside(r.taps_off, 1, 0, table, taps_floats)) {
            afg::set_error("afg_resample_hip: row %llu: the table of %llu floats leaves d_taps (%llu floats; a table holds 2^22 at the most)", kk,
                           (unsigned long long)table, (unsigned long long)taps_floats);
            return AFG_ERR_INVALID;
        }
    }
    if (tiles != n_tiles) {
        afg::set_error("afg_resample_hip: n_tiles %llu, afg_resample_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_resample_row *d_rows, uint64_t n_tiles, const float *d_in, const float *d_taps, float *d_out)
{
    if (!d_rows || !d_out) {
        afg::set_error("afg_resample_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_taps & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_resample_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_resample_hip", "rows", n_rows, n_tiles);
}

}  // namespace

int afg::resample_launch(const afg_resample_row *h_rows, uint64_t n_rows, const afg_resample_row *d_rows, uint64_t n_tiles,
                         const float *d_in, uint64_t in_floats, const float *d_taps, uint64_t taps_floats, float *d_out,
                         uint64_t out_floats, hipStream_t stream)
{
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_taps, d_out)) return rc;
    if (int rc = check_rows(h_rows, n_rows, n_tiles, d_in != nullptr, in_floats, d_taps != nullptr, taps_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (int rc = afg::require_device()) return rc;
    hipLaunchKernelGGL(resample_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, stream, (uint32_t)n_rows, d_rows, d_in, d_taps, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" uint64_t afg_resample_layout(afg_resample_row *rows, uint64_t n_rows)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += tiles_of(rows[k]);
    }
    return tiles;
}

extern "C" int afg_resample_hip(uint64_t n_rows, const afg_resample_row *d_rows, uint64_t n_tiles, const float *d_in, uint64_t in_floats,
                                const float *d_taps, uint64_t taps_floats, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_taps, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_resample_row *h) {
        return afg::resample_launch(h, n_rows, d_rows, n_tiles, d_in, in_floats, d_taps, taps_floats, d_out, out_floats, (hipStream_t)hip_stream);
    });
}
