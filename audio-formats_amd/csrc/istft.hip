// istft.hip -- the inverse short-time Fourier transform (afg_istft_hip), for gfx950: the way back from stft.hip's
// AFG_STFT_COMPLEX slab ([n_bins, frames] pairs, frames contiguous) to a waveform -- per frame the inverse real transform,
// then the windowed overlap-add divided by the window envelope (include/afg.h has the definition and the bound).  The
// transform is fft_frame.h's, run backwards: the split pass undone (fft_unsplit_bin), the half-length complex transform
// through the same forward passes with the planes swapped (the inverse of a transform is the swap of the transform of the
// swap, up to 1 / nc), and z[j] = x[2j] + i x[2j+1] read apart again; an odd n_fft runs the Hermitian extension at full length.
//
// Output-stationary: one workgroup of 256 lanes (four wavefronts, `waves` of which transform) per tile of `tile` consecutive
// delivered samples of one row (afg_istft_row), found by the search over the rows' first tiles that the other stages use.
// The workgroup transforms every frame whose window span meets its tile, in ascending order; the at most m - 1 frames it
// shares with the tile before it, m = ceil(win_length / hop), are computed by both.  With f_lo .. f_hi those frames:
//   stage      `gs` frames at a time, all four wavefronts copy the spectrum into Sp[bin][2 gs] in LDS (pitch 2 gs + 1).  A
//              wavefront's load instruction covers 64 / (2 gs) bin rows, and within a bin row its lanes read consecutive
//              floats -- runs of 8 gs bytes along frames, the mirror of stft.hip's store.
//   transform  `waves` frames at a time, wavefront w takes frame w of the group: lanes along bins build Z from column 2 g of
//              Sp (addresses 2 gs + 1 floats apart: different banks), scaled by 1 / n_fft, into its own buffers, and run the
//              passes.  The imaginary parts of bin 0 and of bin n_fft / 2 are not read from Sp.  A NaN among what was read
//              turns the whole frame into NaN (a wavefront vote): containment is stated per frame, and the passes alone
//              spread a NaN over both planes only by the grace of the factorisation.
//   add        after a barrier all 256 lanes run along the samples the group's frames cover inside the tile: sample t takes
//              its running sum from the ring (or +0.0f when no earlier frame covered it), adds w[j] * x_f[j] for the
//              group's frames in ascending order, and either puts it back or -- when no later frame covers t -- divides by
//              D[t] and stores it, lanes along consecutive samples.  D[t] is summed there from the window in LDS, w * w in
//              ascending frame order from +0.0f.  So every sample's sum runs over its frames in ascending order from +0.0f
//              whatever tile it falls in and however the frames fall into groups, and the same row gives the same bits.
//              The ring holds a power of two >= (waves - 1) hop + n_fft floats: the samples a group can leave unfinished.
//
// Tile and LDS.  The tile is 64 hops or two frames, whichever is longer, rounded up to 256 and at most 16384 samples: 10240
// at 400 / 160 (64 + 2 frames, 3 % computed twice), 16384 at 1024 / 256 (64 + 3, 5 %).  LDS holds the wavefronts' buffers
// (4 nc floats each, nc = n_fft / 2 or n_fft when odd), Sp, the ring and the window; istft_geo takes four wavefronts and the
// widest gs of 32 .. 4 that fits 152 KB, then two wavefronts (1875 and 2025 at full length), then one:
//   n_fft  400 hop 160:  3200 +  201 * 65 + 1024 +  400 = 17689 floats,  69 KB: gs 32, 4 waves
//   n_fft 1024 hop 256:  8192 +  513 * 33 + 2048 + 1024 = 28193 floats, 110 KB: gs 16
//   n_fft 2048 hop 512: 16384 + 1025 *  9 + 4096 + 2048 = 31753 floats, 124 KB: gs 4
//   n_fft 2025 hop 405: 16200 + 1013 *  9 + 4096 + 2025 = 31438 floats, 123 KB: gs 4, 2 waves
// Nothing in 16 .. 2048 is left without a geometry (the last resort, one wavefront and gs 1, needs 59 KB at 2025).
//
// Bounds: every row is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + 2 (k in_pitch + f)] and the float behind it for k < n_bins, f < n_frames only, table[0 .. win_length + 2 n_fft)
// only, and writes out[out_off .. out_off + out_frames) only.  No atomics, no inline assembly.
#include "afg_records.h"
#include "fft_frame.h"

#include <cmath>
#include <limits>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = 4;
constexpr uint32_t kLdsBudget = 152 * 1024;
constexpr uint32_t kMaxTile = 16384;
constexpr double kEnvelopeFloor = 1e-11;

static_assert(sizeof(afg_istft_params) == 32 && sizeof(afg_istft_row) == 40, "include/afg.h");

struct IstftGeo {
    FftGeo fft;
    uint32_t gs;                                                // frames staged at a time: a multiple of fft.waves
    uint32_t ring;                                              // floats of the ring, a power of two
    uint32_t tile;                                              // delivered samples per tile
};

uint32_t pow2_ceil(uint32_t v)
{
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// (params already checked: check_params)
IstftGeo istft_geo(const afg_istft_params &p)
{
    IstftGeo g;
    g.fft = fft_geo_of(p.n_fft);
    const uint32_t n_bins = p.n_fft / 2 + 1;
    const uint32_t longer = 64 * p.hop > 2 * p.n_fft ? 64 * p.hop : 2 * p.n_fft;
    g.tile = (longer + 255) / 256 * 256;
    if (g.tile > kMaxTile) g.tile = kMaxTile;
    auto fits = [&](uint32_t waves, uint32_t gs) {
        g.fft.waves = waves; g.gs = gs;
        g.ring = pow2_ceil((waves - 1) * p.hop + p.n_fft);
        g.fft.lds_floats = waves * g.fft.wbuf + n_bins * (2 * gs + 1) + g.ring + p.win_length;
        return g.fft.lds_floats * 4 <= kLdsBudget;
    };
    for (uint32_t waves : { kWaves, 2u, 1u })
        for (uint32_t gs = 32; gs >= waves; gs >>= 1)
            if (fits(waves, gs)) return g;
    return g;                                                   // (does not fit: check_params says so)
}

__global__ __launch_bounds__(kThreads) void istft_kernel(uint32_t n_rows, const afg_istft_row *__restrict__ rows, afg_istft_params prm, FftGeo geo,
                                                         uint32_t gs, uint32_t ring_floats, uint32_t tile_samples, const float *__restrict__ in,
                                                         const float *__restrict__ table, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint64_t tile = blockIdx.x;
    // the row of this tile: the last one whose first tile is <= tile (rows without output have no tiles)
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_istft_row::first_tile);
    const afg_istft_row r = rows[lo];
    if (r.first_tile > tile) return;
    const uint64_t i0 = (tile - r.first_tile) * tile_samples;   // first delivered sample of the tile
    if (i0 >= r.out_frames) return;
    const uint32_t n = (uint32_t)min((uint64_t)tile_samples, r.out_frames - i0);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t n_fft = prm.n_fft, n_bins = n_fft / 2 + 1, win = prm.win_length, hop = prm.hop, n_lo = (n_fft - win) / 2, nc = geo.nc;
    const uint32_t pitch = 2 * gs + 1, mask = ring_floats - 1;
    float *const Sp = lds + geo.waves * geo.wbuf, *const ring = Sp + n_bins * pitch, *const Wl = ring + ring_floats;
    const float *const tw = table + win;

    // ---- the frames whose window span [f hop + n_lo, f hop + n_lo + win) meets the tile [T0, T0 + n) of the line
    const uint64_t T0 = (uint64_t)(prm.center ? n_fft / 2 : 0) + r.out_first + i0, span = (uint64_t)n_lo + win;
    if (T0 + n - 1 < n_lo) return;                              // (no frame reaches it: the envelope check refuses such a row)
    const uint64_t f_lo = T0 >= span ? (T0 - span) / hop + 1 : 0;
    const uint64_t f_hi = min((uint64_t)r.n_frames - 1, (T0 + n - 1 - n_lo) / hop);
    if (f_hi < f_lo) return;                                    // (likewise)
    const uint32_t nf = (uint32_t)(f_hi - f_lo + 1);
    // from here on positions count from the first sample of frame f_lo, and frames from f_lo
    const int32_t t0 = (int32_t)((int64_t)T0 - (int64_t)(f_lo * hop)), t1 = t0 + (int32_t)n;
    const float *const x = in + r.in_off + 2 * f_lo;
    float *const y = out + r.out_off + i0;
    const float s = 1.0f / (float)n_fft;
    const uint32_t res = (geo.n_pass & 1) ? 2 * nc : 0;         // where fft_passes leaves the result inside a wavefront's buffers

    for (uint32_t i = tid; i < win; i += kThreads) Wl[i] = table[i];

    const uint32_t width = 2 * gs, shift = (uint32_t)__builtin_ctz(width), per = 64 >> shift, col = lane & (width - 1), sub = lane >> shift;
    for (uint32_t fs = 0; fs < nf; fs += gs) {
        const uint32_t ns = min(gs, nf - fs);
        // ---- stage: frames fs .. fs + ns of every bin row, 64 / width bin rows per wavefront and instruction
        if (col < 2 * ns)
            for (uint32_t k = wave * per + sub; k < n_bins; k += kWaves * per) Sp[k * pitch + col] = x[2 * ((uint64_t)k * r.in_pitch + fs) + col];
        __syncthreads();
        for (uint32_t c0 = 0; c0 < ns; c0 += geo.waves) {
            const uint32_t gc = min(geo.waves, ns - c0), fc = fs + c0;
            // ---- transform: frame fc + wave, from column c0 + wave of Sp
            if (wave < gc) {
                const float *const X = Sp + 2 * (c0 + wave);
                bool bad = false;
                const float *zr, *zi;
                if (geo.half) {
                    auto fetch = [&](uint32_t j) -> cf {
                        cf Z;
                        if (j == 0) {
                            const float a = X[0], c = X[nc * pitch];
                            Z = { s * (a + c), s * (a - c) };
                        } else {
                            const float *p = X + j * pitch, *q = X + (nc - j) * pitch;
                            Z = fft_unsplit_bin(cf{ p[0], p[1] }, cf{ q[0], q[1] }, s, j, tw);
                        }
                        bad |= (Z.re != Z.re) || (Z.im != Z.im);
                        return { Z.im, Z.re };
                    };
                    fft_frame_complex(geo, n_fft, lds + wave * geo.wbuf, tw, lane, fetch, &zr, &zi);
                } else {
                    auto fetch = [&](uint32_t j) -> cf {
                        const uint32_t k = j <= n_fft / 2 ? j : n_fft - j;
                        const float *p = X + k * pitch;
                        const float a = s * p[0], b = k == 0 ? 0.0f : s * p[1];
                        bad |= (a != a) || (b != b);
                        return { j <= n_fft / 2 ? b : -b, a };
                    };
                    fft_frame_complex(geo, n_fft, lds + wave * geo.wbuf, tw, lane, fetch, &zr, &zi);
                }
                if (__any(bad)) {                                // (uniform per wavefront)
                    float *const w0 = lds + wave * geo.wbuf + res;
                    for (uint32_t j = lane; j < 2 * nc; j += 64) w0[j] = std::numeric_limits<float>::quiet_NaN();
                }
            }
            __syncthreads();
            // ---- add: the samples of the tile under the group's frames, lanes along samples
            {
                const int32_t cs = (int32_t)(fc * hop + n_lo), ce = (int32_t)((fc + gc - 1) * hop + n_lo + win);
                const int32_t tA = max(t0, cs), tB = min(t1, ce);
                const int32_t fin = fc + gc == nf ? tB : min(tB, (int32_t)((fc + gc) * hop + n_lo));      // below it no later frame adds
                const int32_t seen = fc ? (int32_t)((fc - 1) * hop + n_lo + win) : tA;                    // below it the ring holds a sum
                for (int32_t t = tA + (int32_t)tid; t < tB; t += kThreads) {
                    float a = t < seen ? ring[(uint32_t)t & mask] : 0.0f;
                    for (uint32_t g = 0; g < gc; g++) {
                        const int32_t j = t - (int32_t)((fc + g) * hop);
                        if (j < (int32_t)n_lo || j >= (int32_t)(n_lo + win)) continue;
                        const float *const rr = lds + g * geo.wbuf + res, *const ri = rr + nc;
                        const float v = geo.half ? ((j & 1) ? rr[j >> 1] : ri[j >> 1]) : ri[j];
                        a += Wl[j - (int32_t)n_lo] * v;
                    }
                    if (t < fin) {
                        const uint32_t u = (uint32_t)t - n_lo;
                        const uint32_t fb = min(nf - 1, u / hop), fa = u >= win ? (u - win) / hop + 1 : 0;
                        float D = 0.0f;
                        for (uint32_t f = fa; f <= fb; f++) {
                            const float w = Wl[u - f * hop];
                            D += w * w;
                        }
                        y[t - t0] = a / D;
                    } else {
                        ring[(uint32_t)t & mask] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

int check_params(const afg_istft_params *p, const char *who)
{
    if (!p) { afg::set_error("%s: NULL params", who); return AFG_ERR_INVALID; }
    if (!n_fft_ok(p->n_fft)) {
        afg::set_error("afg_istft_params.n_fft %u: 16 .. 2048 with prime factors 2, 3 and 5 only", p->n_fft);
        return AFG_ERR_UNSUPPORTED;
    }
    if (p->win_length < 1 || p->win_length > p->n_fft) { afg::set_error("afg_istft_params.win_length %u: 1 .. n_fft (%u)", p->win_length, p->n_fft); return AFG_ERR_INVALID; }
    if (p->hop < 1 || p->hop > p->n_fft) { afg::set_error("afg_istft_params.hop %u: 1 .. n_fft (%u)", p->hop, p->n_fft); return AFG_ERR_INVALID; }
    if (p->center > 1) { afg::set_error("afg_istft_params.center %u: 0 or 1", p->center); return AFG_ERR_INVALID; }
    for (uint32_t v : p->reserved)
        if (v != 0) { afg::set_error("afg_istft_params.reserved: must be 0"); return AFG_ERR_INVALID; }
    const IstftGeo g = istft_geo(*p);
    if ((size_t)g.fft.lds_floats * sizeof(float) > kLdsBudget) {     // (none for 16 .. 2048: the file's head)
        afg::set_error("afg_istft_params.n_fft %u needs %u floats of LDS", p->n_fft, g.fft.lds_floats);
        return AFG_ERR_UNSUPPORTED;
    }
    return AFG_OK;
}

uint64_t tiles_of(const afg_istft_row &r, uint32_t tile) { return ((uint64_t)r.out_frames + tile - 1) / tile; }

uint64_t line_of(const afg_istft_params &p, uint32_t n_frames) { return (uint64_t)p.n_fft + (uint64_t)p.hop * (n_frames - 1); }      // n_frames >= 1

// the table's window, the float32 values the device squares
std::vector<float> window_of(const afg_istft_params &p)
{
    std::vector<float> t((size_t)p.win_length + 2 * (size_t)p.n_fft);
    afg_mel_fft_tables(p.n_fft, p.win_length, t.data(), t.size());
    t.resize(p.win_length);
    return t;
}

// The smallest D[t] over the delivered samples [first, first + count) (the range inside the line, count >= 1).  D[t + hop] is
// D[t] term for term wherever no frame is missing at either end -- for n_lo + win_length - 1 <= t < (n_frames - 1) hop + n_lo
// -- so the range is walked whole only up to one hop into that stretch and from where it ends.
double envelope_min(const std::vector<float> &w, const afg_istft_params &p, uint32_t n_frames, uint32_t first, uint32_t count)
{
    const uint64_t win = p.win_length, hop = p.hop, n_lo = (p.n_fft - p.win_length) / 2;
    const uint64_t a = (uint64_t)(p.center ? p.n_fft / 2 : 0) + first, b = a + count;
    const uint64_t steady = n_lo + win - 1, tail = (uint64_t)(n_frames - 1) * hop + n_lo;
    double least = std::numeric_limits<double>::infinity();
    auto D = [&](uint64_t t) {
        if (t < n_lo) return 0.0;
        const uint64_t u = t - n_lo, fb = std::min<uint64_t>(n_frames - 1, u / hop), fa = u >= win ? (u - win) / hop + 1 : 0;
        double d = 0.0;
        for (uint64_t f = fa; f <= fb; f++) {
            const double v = (double)w[(size_t)(u - f * hop)];
            d += v * v;
        }
        return d;
    };
    uint64_t t = a;
    for (; t < b && t < std::max(a, steady) + hop; t++) least = std::min(least, D(t));      // the head, and one period of the steady stretch
    if (t < b && t < tail) t = std::max(t, std::min(b, tail));
    for (; t < b; t++) least = std::min(least, D(t));
    return least;
}

// every row against the planes, the table and the tile table, before anything runs
int check_rows(const afg_istft_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_istft_params &p, uint64_t in_floats, uint64_t table_floats,
               uint64_t out_floats)
{
    const IstftGeo g = istft_geo(p);
    const uint64_t pad = p.center ? p.n_fft / 2 : 0, n_bins = p.n_fft / 2 + 1;
    if (table_floats < (uint64_t)p.win_length + 2 * (uint64_t)p.n_fft) {
        afg::set_error("afg_istft_hip: table_floats %llu: afg_mel_fft_tables gives %llu", (unsigned long long)table_floats,
                       (unsigned long long)p.win_length + 2 * (unsigned long long)p.n_fft);
        return AFG_ERR_INVALID;
    }
    const std::vector<float> w = window_of(p);
    uint32_t last[3] = { 0, 0, 0 };                              // the row before with output: rows of a batch mostly share their envelope
    uint64_t tiles = 0;
    for (uint64_t k = 0; k < n_rows; k++) {
        const afg_istft_row &r = rows[k];
        const unsigned long long kk = (unsigned long long)k;
        if (r.first_tile != tiles) {
            afg::set_error("afg_istft_hip: row %llu: first_tile %llu, afg_istft_layout gives %llu", kk, (unsigned long long)r.first_tile, (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        tiles += tiles_of(r, g.tile);
        if (r.out_frames == 0) continue;                         // nothing read, nothing written
        if (r.n_frames < 1) { afg::set_error("afg_istft_hip: row %llu: %u samples of no frame", kk, r.out_frames); return AFG_ERR_INVALID; }
        if (r.n_frames > r.in_pitch) { afg::set_error("afg_istft_hip: row %llu: n_frames %u above in_pitch %u", kk, r.n_frames, r.in_pitch); return AFG_ERR_INVALID; }
        const uint64_t need = 2 * ((n_bins - 1) * r.in_pitch + r.n_frames);                                // < 2^44
        if (!afg::rows_inside(r.in_off, 1, 0, need, in_floats)) {
            afg::set_error("afg_istft_hip: row %llu: the slab's %llu floats leave the input (%llu floats)", kk, (unsigned long long)need, (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        if (!afg::rows_inside(r.out_off, 1, 0, r.out_frames, out_floats)) {
            afg::set_error("afg_istft_hip: row %llu: the row's %u samples leave the output (%llu floats)", kk, r.out_frames, (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
        if (pad + r.out_first + r.out_frames > line_of(p, r.n_frames)) {
            afg::set_error("afg_istft_hip: row %llu: samples %llu .. %llu, but %u frames make a line of %llu", kk, (unsigned long long)(pad + r.out_first),
                           (unsigned long long)(pad + r.out_first + r.out_frames), r.n_frames, (unsigned long long)line_of(p, r.n_frames));
            return AFG_ERR_INVALID;
        }
        if (r.n_frames == last[0] && r.out_first == last[1] && r.out_frames == last[2]) continue;
        const double least = envelope_min(w, p, r.n_frames, r.out_first, r.out_frames);
        if (least < kEnvelopeFloor) {
            afg::set_error("afg_istft_hip: row %llu: the window envelope falls to %g inside the delivered range (at least 1e-11)", kk, least);
            return AFG_ERR_INVALID;
        }
        last[0] = r.n_frames; last[1] = r.out_first; last[2] = r.out_frames;
    }
    if (tiles != n_tiles) {
        afg::set_error("afg_istft_hip: n_tiles %llu, afg_istft_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_istft_row *d_rows, uint64_t n_tiles, const float *d_in, const float *d_table, float *d_out)
{
    if (!d_rows || !d_in || !d_table || !d_out) {
        afg::set_error("afg_istft_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_table & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_istft_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_istft_hip", "rows", n_rows, n_tiles);
}

}  // namespace

extern "C" uint32_t afg_istft_tile_samples(const afg_istft_params *params)
{
    if (check_params(params, "afg_istft_tile_samples")) return 0;
    return istft_geo(*params).tile;
}

extern "C" uint64_t afg_istft_layout(afg_istft_row *rows, uint64_t n_rows, const afg_istft_params *params)
{
    if (check_params(params, "afg_istft_layout")) return 0;
    const uint32_t tile = istft_geo(*params).tile;
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += tiles_of(rows[k], tile);
    }
    return tiles;
}

extern "C" double afg_istft_envelope_min(const afg_istft_params *params, uint32_t n_frames, uint32_t out_first, uint32_t out_frames)
{
    if (check_params(params, "afg_istft_envelope_min")) return -1.0;
    if (n_frames < 1 || out_frames < 1) { afg::set_error("afg_istft_envelope_min: n_frames and out_frames must be at least 1"); return -1.0; }
    const uint64_t pad = params->center ? params->n_fft / 2 : 0;
    if (pad + out_first + out_frames > line_of(*params, n_frames)) {
        afg::set_error("afg_istft_envelope_min: samples %llu .. %llu, but %u frames make a line of %llu", (unsigned long long)(pad + out_first),
                       (unsigned long long)(pad + out_first + out_frames), n_frames, (unsigned long long)line_of(*params, n_frames));
        return -1.0;
    }
    try {
        return envelope_min(window_of(*params), *params, n_frames, out_first, out_frames);
    } catch (...) {
        afg::set_error("out of host memory");
        return -1.0;
    }
}

extern "C" int afg_istft_check_rows(const afg_istft_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_istft_params *params, uint64_t in_floats,
                                    uint64_t table_floats, uint64_t out_floats)
{
    if (int rc = check_params(params, "afg_istft_check_rows")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!rows) { afg::set_error("afg_istft_check_rows: NULL rows"); return AFG_ERR_INVALID; }
    try {
        return check_rows(rows, n_rows, n_tiles, *params, in_floats, table_floats, out_floats);
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

extern "C" int afg_istft_hip(uint64_t n_rows, const afg_istft_row *d_rows, uint64_t n_tiles, const afg_istft_params *params, const float *d_in,
                             uint64_t in_floats, const float *d_table, uint64_t table_floats, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = check_params(params, "afg_istft_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_table, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int rc = afg::with_host_records(d_rows, n_rows, stream, [&](const afg_istft_row *h) {
            return check_rows(h, n_rows, n_tiles, *params, in_floats, table_floats, out_floats);
        }))
        return rc;
    if (n_tiles == 0) return AFG_OK;
    const IstftGeo g = istft_geo(*params);
    static_assert((size_t)kLdsBudget <= 160 * 1024, "LDS budget");
    const size_t bytes = (size_t)g.fft.lds_floats * sizeof(float);      // <= kLdsBudget: check_params
    AFG_HIP_CHECK(hipFuncSetAttribute((const void *)istft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(istft_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), bytes, stream, (uint32_t)n_rows, d_rows, *params, g.fft, g.gs, g.ring,
                       g.tile, d_in, d_table, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
