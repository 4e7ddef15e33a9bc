// stft.hip -- the linear-frequency spectrogram (afg_stft_hip), for gfx950: the short-time Fourier transform that
// melspec_fft.hip computes per frame and multiplies into a mel bank, delivered instead -- complex, magnitude, power or log10
// power, [n_bins, out_frames] per row with frames contiguous.  The transform is that kernel's (fft_frame.h: the same passes in
// the same order, so the same bits of re and im); the tiling and the epilogue are this file's, and they are shaped by the
// store: the output is n_bins / n_mels times the mel kernel's, and nothing follows the transform but writing it out.
//
// One workgroup of 256 lanes (four wavefronts, `waves` of which transform) per tile of `tile` frames of one row (afg_mel_row), found by the search over
// the rows' first tiles that the other stages use.
//   transform  every transforming wavefront owns whole frames (w, w + waves, ...) of the tile, as in melspec_fft.hip: the frame's samples are
//              fetched with lanes along samples (reflection and zeros resolved on the way in), multiplied by the window and
//              written into the wavefront's own LDS buffers; an even n_fft runs the complex transform of half the length and
//              a split pass, an odd n_fft the full length with a zero imaginary part.  No workgroup barrier stands inside.
//   stage      the frame's n_bins results go into S[bin][column] in LDS, lanes along bins: column f of a one-component kind
//              (the value already final: p, sqrtf(p) or log10f(fmaxf(p, floor))), columns 2 f and 2 f + 1 (re, im) of
//              AFG_STFT_COMPLEX.  A row of S is `width` = comps * tile floats at pitch width + 1: the writes of a wavefront
//              are pitch floats apart, on 64 different banks.  Frames the tile does not have are not computed.
//   store      after one barrier all four wavefronts write S out.  `width` is 64, 32 or 16 floats, so a wavefront's store
//              instruction covers 64 / width bin rows, and within a bin row its lanes write consecutive floats: one run of
//              width * 4 bytes (256, 128 or 64) per bin row and instruction, cut only where the row's last tile ends.  The
//              reads of S are consecutive floats per row (one bank each; two rows of pitch 33 share a single bank).
//              A bin row starts at float out_off + comps * (k * out_frames + t0), at whatever dword alignment out_off and
//              out_frames leave it, and is 256 bytes at most: the stores are one dword per lane, which fills those runs
//              whole, and not trim.hip's dwordx4, which needs a 16-byte aligned interior per row.
//
// Tile and LDS.  A transforming wavefront's buffers are 4 nc floats (nc = n_fft / 2, or n_fft when odd) and S is
// n_bins * (width + 1); stft_geo takes the widest of 64, 32, 16 for which S and four wavefronts' buffers fit 152 KB:
//   n_fft  400  (nc 200):  3200 +  201 * 65 = 16265 floats,  64 KB: width 64 -- 64 frames, 32 complex
//   n_fft  512  (nc 256):  4096 +  257 * 65 = 20801 floats,  82 KB: width 64
//   n_fft 1024  (nc 512):  8192 +  513 * 65 = 41537 floats, 163 KB does not fit; 8192 + 513 * 33 = 25121, 99 KB: width 32
//   n_fft 2048 (nc 1024): 16384 + 1025 * 33 = 50209 floats, 197 KB does not fit; 16384 + 1025 * 17 = 33809, 133 KB: width 16
// An odd n_fft transforms at full length, and for the two largest the path takes even width 16 does not fit beside four
// wavefronts' buffers; there `waves` drops to two, as melspec_fft.hip's does, and the other two wavefronts only store:
//   n_fft 1875 (nc 1875): 30000 +  938 * 17 = 45946 floats, 184 KB does not fit; 15000 + 15946 = 30946, 124 KB: width 16, 2 waves
//   n_fft 2025 (nc 2025): 32400 + 1013 * 17 = 49621 floats, 198 KB does not fit; 16200 + 17221 = 33421, 134 KB: width 16, 2 waves
// Every other n_fft (the next odd one is 1215) keeps four.  afg_stft_check_rows refuses a geometry that does not fit, as the
// launch does; none exists for 16 .. 2048.
//
// Bounds: every row is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + g] for 0 <= g < in_frames only and table[0 .. win_length + 2 * n_fft) only, and writes
// out[out_off .. out_off + comps * n_bins * out_frames) only.
#include "mel_rows.h"
#include "fft_frame.h"

#include <cmath>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = 4;
constexpr uint32_t kLdsBudget = 152 * 1024;

static_assert(sizeof(afg_stft_params) == 32 && sizeof(afg_mel_row) == 32, "include/afg.h");

struct StftGeo {
    FftGeo fft;
    uint32_t comps;                                             // floats per bin and frame: 2 for AFG_STFT_COMPLEX
    uint32_t tile;                                              // frames per tile
    uint32_t width;                                             // floats of a row of S: comps * tile, 64, 32 or 16
};

// (params already checked: check_params)
StftGeo stft_geo(const afg_stft_params &p)
{
    StftGeo g;
    g.fft = fft_geo_of(p.n_fft);
    g.comps = p.out_kind == AFG_STFT_COMPLEX ? 2 : 1;
    const uint32_t n_bins = p.n_fft / 2 + 1;
    auto fits = [&](uint32_t waves, uint32_t width) {
        g.fft.waves = waves; g.width = width;
        g.fft.lds_floats = waves * g.fft.wbuf + n_bins * (width + 1);
        return g.fft.lds_floats * 4 <= kLdsBudget;
    };
    // the widest row of S beside all four wavefronts' buffers; where not even 16 fits, fewer transforming wavefronts
    if (!fits(kWaves, 64) && !fits(kWaves, 32) && !fits(kWaves, 16) && !fits(2, 16)) fits(1, 16);
    g.tile = g.width / g.comps;
    return g;
}

__global__ __launch_bounds__(kThreads) void stft_kernel(uint32_t n_rows, const afg_mel_row *__restrict__ rows, afg_stft_params prm, FftGeo geo,
                                                        uint32_t tile_frames, const float *__restrict__ in, const float *__restrict__ table,
                                                        float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint64_t tile = blockIdx.x;
    // the row of this tile: the last one whose first tile is <= tile (rows without output have no tiles)
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_mel_row::first_tile);
    const afg_mel_row r = rows[lo];
    if (r.first_tile > tile) return;
    const uint64_t t0 = (tile - r.first_tile) * tile_frames;    // first frame of the tile
    if (t0 >= r.out_frames) return;
    const uint32_t n = (uint32_t)min((uint64_t)tile_frames, r.out_frames - t0);
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t n_fft = prm.n_fft, n_bins = n_fft / 2 + 1, win = prm.win_length, n_lo = (n_fft - win) / 2, nc = geo.nc;
    const uint32_t kind = prm.out_kind, comps = kind == AFG_STFT_COMPLEX ? 2 : 1, width = tile_frames * comps, pitch = width + 1;
    const float floor_ = prm.log_floor == 0.0f ? 1e-10f : prm.log_floor;
    float *const S = lds + geo.waves * geo.wbuf;
    const float *const tw = table + win;

    // what a one-component kind delivers of re and im
    auto value = [&](cf X) -> float {
        const float p = X.re * X.re + X.im * X.im;
        if (kind == AFG_STFT_MAGNITUDE) return sqrtf(p);
        if (kind == AFG_STFT_LOG10) return log10f(fmaxf(p, floor_));
        return p;
    };

    if (wave < geo.waves) {
        float *const buf = lds + wave * geo.wbuf;
        const int64_t nin = r.in_frames;
        const float *x = in + r.in_off;
        for (uint32_t f = wave; f < n; f += geo.waves) {        // (uniform per wavefront)
            const int64_t s0 = (int64_t)(t0 + f) * prm.hop - (int64_t)(prm.center ? n_fft / 2 : 0);
            // sample i of the frame times its window value; +0.0f outside the window
            auto fetch = [&](uint32_t i) -> float {
                if (i < n_lo || i >= n_lo + win) return 0.0f;
                int64_t s = s0 + i;
                if (prm.pad_mode == AFG_MEL_PAD_REFLECT) {      // in_frames > pad (check_rows): one fold lands inside
                    if (s < 0) s = -s;
                    else if (s >= nin) s = 2 * (nin - 1) - s;
                }
                const float v = (s >= 0 && s < nin) ? x[s] : 0.0f;
                return v * table[i - n_lo];
            };
            const float *sr, *si;
            fft_frame(geo, n_fft, buf, tw, lane, fetch, &sr, &si);
            // ---- bins 0 .. n_fft / 2 into the frame's column(s) of S
            for (uint32_t k = lane; k < n_bins; k += 64) {
                const cf X = geo.half ? fft_split_bin(sr, si, nc, k, tw) : cf{ sr[k], si[k] };
                float *s = S + k * pitch + f * comps;
                if (comps == 2) { s[0] = X.re; s[1] = X.im; }
                else s[0] = value(X);
            }
        }
    }
    __syncthreads();

    // ---- store: 64 / width bin rows per wavefront and instruction, `width` consecutive floats of each
    const uint32_t per = 64 / width, col = lane & (width - 1), sub = lane / width, cols = n * comps;
    float *y = out + r.out_off + t0 * comps;
    const uint64_t row_floats = (uint64_t)r.out_frames * comps;
    if (col < cols)
        for (uint32_t k = wave * per + sub; k < n_bins; k += kWaves * per) y[k * row_floats + col] = S[k * pitch + col];
}

int check_params(const afg_stft_params *p, const char *who)
{
    if (!p) { afg::set_error("%s: NULL params", who); return AFG_ERR_INVALID; }
    if (!n_fft_ok(p->n_fft)) {
        afg::set_error("afg_stft_params.n_fft %u: 16 .. 2048 with prime factors 2, 3 and 5 only", p->n_fft);
        return AFG_ERR_UNSUPPORTED;
    }
    if (p->win_length < 1 || p->win_length > p->n_fft) { afg::set_error("afg_stft_params.win_length %u: 1 .. n_fft (%u)", p->win_length, p->n_fft); return AFG_ERR_INVALID; }
    if (p->hop < 1 || p->hop > p->n_fft) { afg::set_error("afg_stft_params.hop %u: 1 .. n_fft (%u)", p->hop, p->n_fft); return AFG_ERR_INVALID; }
    if (p->center > 1) { afg::set_error("afg_stft_params.center %u: 0 or 1", p->center); return AFG_ERR_INVALID; }
    if (p->pad_mode != AFG_MEL_PAD_REFLECT && p->pad_mode != AFG_MEL_PAD_ZERO) { afg::set_error("afg_stft_params.pad_mode %u: AFG_MEL_PAD_REFLECT or AFG_MEL_PAD_ZERO", p->pad_mode); return AFG_ERR_INVALID; }
    if (p->out_kind > AFG_STFT_LOG10) { afg::set_error("afg_stft_params.out_kind %u: AFG_STFT_COMPLEX .. AFG_STFT_LOG10", p->out_kind); return AFG_ERR_INVALID; }
    if (!(p->log_floor >= 0.0f) || !std::isfinite(p->log_floor)) { afg::set_error("afg_stft_params.log_floor %g: a finite float >= 0", (double)p->log_floor); return AFG_ERR_INVALID; }
    if (p->reserved != 0) { afg::set_error("afg_stft_params.reserved %u: must be 0", p->reserved); return AFG_ERR_INVALID; }
    const StftGeo g = stft_geo(*p);
    if ((size_t)g.fft.lds_floats * sizeof(float) > kLdsBudget) {     // (none for 16 .. 2048: the file's head)
        afg::set_error("afg_stft_params.n_fft %u needs %u floats of LDS", p->n_fft, g.fft.lds_floats);
        return AFG_ERR_UNSUPPORTED;
    }
    return AFG_OK;
}

}  // namespace

uint32_t afg::stft_frames(const afg_stft_params &p, uint32_t in_frames)
{
    const int64_t num = (int64_t)in_frames + 2 * (int64_t)(p.center ? p.n_fft / 2 : 0) - (int64_t)p.n_fft;
    return num < 0 ? 0 : (uint32_t)(1 + num / (int64_t)p.hop);
}

namespace {

uint64_t tiles_of(const afg_mel_row &r, uint32_t tile) { return ((uint64_t)r.out_frames + tile - 1) / tile; }

// every row against the planes, the table and the tile table, before anything runs
int check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_stft_params &p, uint64_t in_floats, uint64_t table_floats,
               uint64_t out_floats)
{
    const StftGeo g = stft_geo(p);
    const uint32_t pad = p.center ? p.n_fft / 2 : 0;
    if (table_floats < (uint64_t)p.win_length + 2 * (uint64_t)p.n_fft) {
        afg::set_error("afg_stft_hip: table_floats %llu: afg_mel_fft_tables gives %llu", (unsigned long long)table_floats,
                       (unsigned long long)p.win_length + 2 * (unsigned long long)p.n_fft);
        return AFG_ERR_INVALID;
    }
    return afg::check_mel_rows("afg_stft_hip", "afg_stft_layout", rows, n_rows, n_tiles, g.tile, p.pad_mode == AFG_MEL_PAD_REFLECT ? pad : 0,
                               (uint64_t)g.comps * (p.n_fft / 2 + 1), in_floats, out_floats,
                               [&](uint32_t in_frames) { return afg::stft_frames(p, in_frames); });
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const float *d_in, const float *d_table, float *d_out)
{
    if (!d_rows || !d_table || !d_out) {
        afg::set_error("afg_stft_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_table & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_stft_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_stft_hip", "rows", n_rows, n_tiles);
}

}  // namespace

int afg::stft_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_stft_params *params,
                     const float *d_in, uint64_t in_floats, const float *d_table, uint64_t table_floats, float *d_out, uint64_t out_floats,
                     hipStream_t stream)
{
    if (int rc = check_params(params, "afg_stft_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_table, d_out)) return rc;
    if (int rc = check_rows(h_rows, n_rows, n_tiles, *params, in_floats, table_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (int rc = afg::require_device()) return rc;
    const StftGeo g = stft_geo(*params);
    static_assert((size_t)kLdsBudget <= 160 * 1024, "LDS budget");
    const size_t bytes = (size_t)g.fft.lds_floats * sizeof(float);      // <= kLdsBudget: check_params
    AFG_HIP_CHECK(hipFuncSetAttribute((const void *)stft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(stft_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), bytes, stream, (uint32_t)n_rows, d_rows, *params, g.fft, g.tile, d_in,
                       d_table, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" uint32_t afg_stft_tile_frames(const afg_stft_params *params)
{
    if (check_params(params, "afg_stft_tile_frames")) return 0;
    return stft_geo(*params).tile;
}

extern "C" uint64_t afg_stft_layout(afg_mel_row *rows, uint64_t n_rows, const afg_stft_params *params)
{
    if (check_params(params, "afg_stft_layout")) return 0;
    const uint32_t tile = stft_geo(*params).tile;
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += tiles_of(rows[k], tile);
    }
    return tiles;
}

extern "C" int afg_stft_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_stft_params *params, uint64_t in_floats,
                                   uint64_t table_floats, uint64_t out_floats)
{
    if (int rc = check_params(params, "afg_stft_check_rows")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!rows) { afg::set_error("afg_stft_check_rows: NULL rows"); return AFG_ERR_INVALID; }
    return check_rows(rows, n_rows, n_tiles, *params, in_floats, table_floats, out_floats);
}

extern "C" int afg_stft_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_stft_params *params, const float *d_in,
                            uint64_t in_floats, const float *d_table, uint64_t table_floats, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = check_params(params, "afg_stft_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_table, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_mel_row *h) {
        return afg::stft_launch(h, n_rows, d_rows, n_tiles, params, d_in, in_floats, d_table, table_floats, d_out, out_floats,
                                (hipStream_t)hip_stream);
    });
}
