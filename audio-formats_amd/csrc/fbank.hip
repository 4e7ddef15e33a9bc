// fbank.hip -- Kaldi-compatible filter-bank features (afg_fbank_hip), for gfx950: the value include/afg.h defines -- frames
// with snip_edges or mirrored with the edge repeated, the DC offset removed per frame, pre-emphasis per frame, a window of
// win_length values, zero padding to n_fft, the spectrum of melspec_fft.hip's transform (fft_frame.h, unchanged: the same
// passes in the same order), a dense bank, a natural log over a float32-epsilon floor and an optional log-energy column.
// Only the orders of summation are free; the result is held to the bound stated in include/afg.h.
//
// One workgroup of 256 lanes (four wavefronts) per tile of kTile = 16 frames of one row (afg_mel_row), found by the search
// over the rows' first tiles that the other stages use.
//   sum        every transforming wavefront owns whole frames (w, w + waves, ...), so no workgroup barrier stands inside the
//              transform.  With remove_dc the frame's win_length samples are read with lanes along samples (coalesced; the
//              mirror resolved on the way in), scaled, and added in float64: a few adds per lane and a wavefront reduction.
//   fetch      fft_frame's callable: sample j is read (again, through L1: the mean has to be known before the first d can
//              be formed, and a frame of 2048 samples does not fit a lane's registers under a loop of run-time length),
//              scaled, d = float32(double(s) - mu), e = d - c * d_prev, z = e * w.  d_prev of an odd j is the value the lane
//              formed for j - 1 (fft_frame asks for 2 j and 2 j + 1 in turn); of an even j it is a second read of sample
//              j - 1.  The energy sum (d * d or z * z) is added per lane on the way and reduced behind the transform.
//   p          re * re + im * im, or its square root, into P[bin][frame] in LDS, pitch 17, as melspec_fft.hip does.
//   product    on v_mfma_f32_16x16x4_f32; a wavefront owns column tiles w, w + 4, w + 8, w + 12 of 16 mels.
//              AFG_FBANK_MEL_MAJOR   D[mel][frame] (A: the bank, B: P), stored as melspec_fft.hip stores: sixteen lanes write
//                                    sixteen consecutive frames of one column.
//              AFG_FBANK_FRAMES_MAJOR  the operand roles swapped, D[frame][mel] (A: P, B: the bank): a lane holds four frames
//                                    of one mel, sixteen lanes sixteen consecutive mels of a frame.  They go into O[frame][col]
//                                    in LDS (pitch cols: the tile's image in the output), and behind one barrier all 256
//                                    lanes write the tile's n * cols floats -- one contiguous piece of the output -- in
//                                    consecutive floats, 1 KB per wavefront and instruction.
//   energy     one float per frame in LDS behind the frame's transform; it joins O (frames-major) or is stored by wavefront
//              0 (mel-major) in its column: 0, or cols - 1 with htk_compat.
// No atomics, no scratch.
//
// Bounds: every row is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + g] for 0 <= g < in_frames only, table[0 .. win_length + 2 * n_fft) and filters[0 .. n_mels * n_bins) only, and
// writes out[out_off .. out_off + cols * out_frames) only.
#include "mel_rows.h"
#include "fft_frame.h"

#include <cmath>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = 16;                                  // frames per tile: one MFMA column block
constexpr uint32_t kPPitch = 17;
constexpr uint32_t kMelTiles = 4;                               // mel tiles of 16 per wavefront: 256 mels
constexpr uint32_t kLdsBudget = 152 * 1024;                     // the FFT mel path's
constexpr float kEps = 1.1920928955078125e-07f;                 // 2^-23

static_assert(sizeof(afg_fbank_params) == 64 && sizeof(afg_mel_row) == 32, "include/afg.h");

typedef float f32x4 __attribute__((ext_vector_type(4)));

uint32_t cols_of(const afg_fbank_params &p) { return p.n_mels + (p.use_energy ? 1 : 0); }

// LDS: the transforming wavefronts' buffers, P, the tile's energies, and with frames-major the tile's image O
struct FbankGeo {
    FftGeo fft;
    uint32_t en_at, o_at;                                       // float offsets of En[kTile] and O[kTile][cols]
};

// (params already checked: check_params)
FbankGeo geo_of(const afg_fbank_params &p)
{
    FbankGeo g;
    g.fft = fft_geo_of(p.n_fft);
    const uint32_t p_floats = (p.n_fft / 2 + 1) * kPPitch;
    const uint32_t o_floats = p.layout == AFG_FBANK_FRAMES_MAJOR ? kTile * cols_of(p) : 0;
    for (g.fft.waves = 4;; g.fft.waves >>= 1) {
        g.en_at = g.fft.waves * g.fft.wbuf + p_floats;
        g.o_at = g.en_at + kTile;
        g.fft.lds_floats = g.o_at + o_floats;
        if (g.fft.waves == 1 || g.fft.lds_floats * 4 <= kLdsBudget) break;
    }
    return g;
}

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void fbank_kernel(uint32_t n_rows, const afg_mel_row *__restrict__ rows, afg_fbank_params prm, FbankGeo fg,
                                                         const float *__restrict__ in, const float *__restrict__ table,
                                                         const float *__restrict__ filters, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FftGeo &geo = fg.fft;
    const uint64_t tile = blockIdx.x;
    // the row of this tile: the last one whose first tile is <= tile (rows without output have no tiles)
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_mel_row::first_tile);
    const afg_mel_row r = rows[lo];
    if (r.first_tile > tile) return;
    const uint64_t t0 = (tile - r.first_tile) * kTile;          // first frame of the tile
    if (t0 >= r.out_frames) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, r.out_frames - t0);
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t li = lane & 15, lk = lane >> 4;
    const uint32_t n_fft = prm.n_fft, n_bins = n_fft / 2 + 1, win = prm.win_length, nc = geo.nc;
    const uint32_t cols = prm.n_mels + (prm.use_energy ? 1 : 0), col0 = (prm.use_energy && !prm.htk_compat) ? 1 : 0;
    const uint32_t ecol = prm.htk_compat ? prm.n_mels : 0;
    float *const P = lds + geo.waves * geo.wbuf;
    float *const En = lds + fg.en_at;
    float *const O = lds + fg.o_at;
    const float *const tw = table + win;
    const float scale_ = prm.scale == 0.0f ? 1.0f : prm.scale, c = prm.preemph;

    if (wave < geo.waves) {
        float *const buf = lds + wave * geo.wbuf;
        const int64_t nin = r.in_frames;                         // >= 1: the row has frames
        const float *x = in + r.in_off;
        const int64_t pad = prm.snip_edges ? 0 : (int64_t)(win / 2) - (int64_t)(prm.hop / 2);
        for (uint32_t f = wave; f < kTile; f += geo.waves) {
            if (f >= n) {                                        // (uniform per wavefront)
                for (uint32_t k = lane; k < n_bins; k += 64) P[k * kPPitch + f] = 0.0f;
                continue;
            }
            const int64_t s0 = (int64_t)(t0 + f) * prm.hop - pad;
            // sample j of the frame, scaled: the mirror with the edge repeated has period 2 N
            auto sample = [&](uint32_t j) -> float {
                int64_t s = s0 + j;
                if ((uint64_t)s >= (uint64_t)nin) {              // (never with snip_edges: check_rows)
                    s %= 2 * nin;
                    if (s < 0) s += 2 * nin;
                    if (s >= nin) s = 2 * nin - 1 - s;
                }
                return x[s] * scale_;
            };
            double mu = 0.0;
            if (prm.remove_dc) {
                double acc = 0.0;
                for (uint32_t j = lane; j < win; j += 64) acc += (double)sample(j);
                mu = wave_sum(acc) / (double)win;
            }
            auto centred = [&](uint32_t j) -> float { return prm.remove_dc ? (float)((double)sample(j) - mu) : sample(j); };
            float en = 0.0f, d_last = 0.0f;
            uint32_t j_last = 0xffffffffu;
            // z of sample i of the frame; +0.0f behind the window
            auto fetch = [&](uint32_t i) -> float {
                if (i >= win) return 0.0f;
                const float d = centred(i);
                float e = d;
                if (c != 0.0f) {
                    const float dp = i == 0 ? d : (i - 1 == j_last ? d_last : centred(i - 1));
                    e = d - c * dp;
                }
                j_last = i; d_last = d;
                const float z = e * table[i];
                if (prm.use_energy) en += prm.raw_energy ? d * d : z * z;
                return z;
            };
            const float *sr, *si;
            fft_frame(geo, n_fft, buf, tw, lane, fetch, &sr, &si);
            // ---- p of bins 0 .. n_fft / 2
            for (uint32_t k = lane; k < n_bins; k += 64) {
                const cf X = geo.half ? fft_split_bin(sr, si, nc, k, tw) : cf{ sr[k], si[k] };
                const float p = X.re * X.re + X.im * X.im;
                P[k * kPPitch + f] = prm.use_power ? p : sqrtf(p);
            }
            if (prm.use_energy) {
                float v = logf(fmaxf(wave_sum(en), kEps));
                if (prm.energy_floor > 0.0f) v = fmaxf(v, logf(prm.energy_floor));
                if (lane == 0) En[f] = v;
            }
        }
    }
    __syncthreads();

    // ---- the bank times P
    const bool fm = prm.layout == AFG_FBANK_FRAMES_MAJOR;
    const uint32_t mel_tiles = (prm.n_mels + 15) >> 4;
#pragma unroll 1
    for (uint32_t t = 0; t < kMelTiles; t++) {
        const uint32_t mt = wave + 4 * t;
        if (mt >= mel_tiles) break;                              // (uniform per wavefront)
        const uint32_t m = mt * 16 + li;
        const float *wr = filters + (uint64_t)(m < prm.n_mels ? m : 0) * n_bins;
        f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (uint32_t k0 = 0; k0 < n_bins; k0 += 4) {
            const uint32_t k = k0 + lk;
            const bool in_k = k < n_bins;
            const float a = (m < prm.n_mels && in_k) ? wr[k] : 0.0f;
            const float b = in_k ? P[k * kPPitch + li] : 0.0f;
            acc = fm ? __builtin_amdgcn_mfma_f32_16x16x4f32(b, a, acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        if (fm) {                                                // D: frame 4 (l >> 4) + e, mel l & 15
            if (m < prm.n_mels) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float v = acc[e];
                    if (prm.use_log) v = logf(fmaxf(v, kEps));
                    O[(lk * 4 + e) * cols + col0 + m] = v;
                }
            }
        } else {                                                 // D: mel 4 (l >> 4) + e, frame l & 15
            float *y = out + r.out_off + t0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t mm = mt * 16 + lk * 4 + e;
                if (mm >= prm.n_mels || li >= n) continue;
                float v = acc[e];
                if (prm.use_log) v = logf(fmaxf(v, kEps));
                y[(uint64_t)(col0 + mm) * r.out_frames + li] = v;
            }
        }
    }
    if (!fm) {
        if (prm.use_energy && threadIdx.x < n) out[r.out_off + (uint64_t)ecol * r.out_frames + t0 + threadIdx.x] = En[threadIdx.x];
        return;
    }
    if (prm.use_energy && threadIdx.x < n) O[threadIdx.x * cols + ecol] = En[threadIdx.x];
    __syncthreads();
    // ---- the tile's n * cols floats: one contiguous piece of the output
    float *y = out + r.out_off + t0 * cols;
    for (uint32_t i = threadIdx.x; i < n * cols; i += kThreads) y[i] = O[i];
}

bool unit(uint32_t v) { return v <= 1; }

int check_params(const afg_fbank_params *p, const char *who)
{
    if (!p) { afg::set_error("%s: NULL params", who); return AFG_ERR_INVALID; }
    if (p->win_length < 2 || p->win_length > 2048) { afg::set_error("%s: win_length %u: 2 .. 2048", who, p->win_length); return AFG_ERR_INVALID; }
    if (p->hop < 1 || p->hop > 65535) { afg::set_error("%s: hop %u: 1 .. 65535", who, p->hop); return AFG_ERR_INVALID; }
    if (p->n_fft < p->win_length || p->n_fft > 2048) {
        afg::set_error("%s: n_fft %u: win_length (%u) .. 2048", who, p->n_fft, p->win_length);
        return AFG_ERR_INVALID;
    }
    if (p->n_mels < 1 || p->n_mels > 256) { afg::set_error("%s: n_mels %u: 1 .. 256", who, p->n_mels); return AFG_ERR_INVALID; }
    const struct { const char *name; uint32_t v; } flags[] = { { "snip_edges", p->snip_edges }, { "remove_dc", p->remove_dc }, { "use_power", p->use_power },
        { "use_log", p->use_log }, { "use_energy", p->use_energy }, { "raw_energy", p->raw_energy }, { "htk_compat", p->htk_compat } };
    for (const auto &f : flags)
        if (!unit(f.v)) { afg::set_error("%s: %s %u: 0 or 1", who, f.name, f.v); return AFG_ERR_INVALID; }
    if (p->layout != AFG_FBANK_FRAMES_MAJOR && p->layout != AFG_FBANK_MEL_MAJOR) {
        afg::set_error("%s: layout %u: AFG_FBANK_FRAMES_MAJOR or AFG_FBANK_MEL_MAJOR", who, p->layout);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->preemph) || p->preemph < 0.0f || p->preemph > 1.0f) {
        afg::set_error("%s: preemph %g: a finite value in [0, 1]", who, (double)p->preemph);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->energy_floor) || p->energy_floor < 0.0f) {
        afg::set_error("%s: energy_floor %g: a finite value >= 0", who, (double)p->energy_floor);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->scale) || p->scale < 0.0f) {
        afg::set_error("%s: scale %g: a finite value > 0 (0 means 1)", who, (double)p->scale);
        return AFG_ERR_INVALID;
    }
    if (p->reserved != 0) { afg::set_error("%s: reserved %u: must be 0", who, p->reserved); return AFG_ERR_INVALID; }
    if (!n_fft_ok(p->n_fft)) {
        afg::set_error("%s: n_fft %u: the transform takes 16 .. 2048 with prime factors 2, 3 and 5 only", who, p->n_fft);
        return AFG_ERR_UNSUPPORTED;
    }
    return AFG_OK;
}

uint32_t frames_of(const afg_fbank_params &p, uint32_t in_frames)
{
    if (p.snip_edges) return in_frames < p.win_length ? 0 : 1 + (in_frames - p.win_length) / p.hop;
    return (uint32_t)(((uint64_t)in_frames + p.hop / 2) / p.hop);
}

uint64_t tiles_of(const afg_mel_row &r) { return ((uint64_t)r.out_frames + kTile - 1) / kTile; }

// every row against the planes, the tables and the tile table, before anything runs
int check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_fbank_params &p, uint64_t in_floats, uint64_t table_floats,
               uint64_t filters_floats, uint64_t out_floats)
{
    if (table_floats < (uint64_t)p.win_length + 2 * (uint64_t)p.n_fft) {
        afg::set_error("afg_fbank_hip: table_floats %llu: afg_fbank_tables gives %llu", (unsigned long long)table_floats,
                       (unsigned long long)p.win_length + 2 * (unsigned long long)p.n_fft);
        return AFG_ERR_INVALID;
    }
    if (filters_floats < (uint64_t)p.n_mels * (p.n_fft / 2 + 1)) {
        afg::set_error("afg_fbank_hip: filters_floats %llu: the bank is n_mels x n_bins = %llu floats", (unsigned long long)filters_floats,
                       (unsigned long long)p.n_mels * (p.n_fft / 2 + 1));
        return AFG_ERR_INVALID;
    }
    // (the mirror folds a row of any length >= 1, and a row of 0 samples has no frames: no padding rule)
    return afg::check_mel_rows("afg_fbank_hip", "afg_fbank_layout", rows, n_rows, n_tiles, kTile, 0, cols_of(p), in_floats, out_floats,
                               [&](uint32_t in_frames) { return frames_of(p, in_frames); });
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const float *d_in, const float *d_table, const float *d_filters,
               float *d_out)
{
    if (!d_rows || !d_table || !d_filters || !d_out) {
        afg::set_error("afg_fbank_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_table & 3u) != 0 || ((uintptr_t)d_filters & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_fbank_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_fbank_hip", "rows", n_rows, n_tiles);
}

}  // namespace

int afg::fbank_check_params(const afg_fbank_params *params, const char *who) { return check_params(params, who); }

int afg::fbank_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_fbank_params *params,
                      const float *d_in, uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters,
                      uint64_t filters_floats, float *d_out, uint64_t out_floats, hipStream_t stream)
{
    if (int rc = check_params(params, "afg_fbank_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_table, d_filters, d_out)) return rc;
    if (int rc = check_rows(h_rows, n_rows, n_tiles, *params, in_floats, table_floats, filters_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (!d_in) { afg::set_error("afg_fbank_hip: NULL d_in with rows that have frames"); return AFG_ERR_INVALID; }
    if (int rc = afg::require_device()) return rc;
    const FbankGeo g = geo_of(*params);
    static_assert((size_t)kLdsBudget <= 160 * 1024, "LDS budget");
    const size_t bytes = (size_t)g.fft.lds_floats * sizeof(float);
    if (bytes > 160 * 1024) {                                    // (n_fft <= 2048 stays below: geo_of)
        afg::set_error("afg_fbank_hip: n_fft %u needs %u floats of LDS", params->n_fft, g.fft.lds_floats);
        return AFG_ERR_INVALID;
    }
    AFG_HIP_CHECK(hipFuncSetAttribute((const void *)fbank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(fbank_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), bytes, stream, (uint32_t)n_rows, d_rows, *params, g, d_in, d_table,
                       d_filters, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" uint32_t afg_fbank_frames(const afg_fbank_params *params, uint32_t in_frames)
{
    if (check_params(params, "afg_fbank_frames")) return 0;
    return frames_of(*params, in_frames);
}

extern "C" uint64_t afg_fbank_layout(afg_mel_row *rows, uint64_t n_rows, const afg_fbank_params *params)
{
    if (check_params(params, "afg_fbank_layout")) return 0;
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += tiles_of(rows[k]);
    }
    return tiles;
}

extern "C" int afg_fbank_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_fbank_params *params, uint64_t in_floats,
                                    uint64_t table_floats, uint64_t filters_floats, uint64_t out_floats)
{
    if (int rc = check_params(params, "afg_fbank_check_rows")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!rows) { afg::set_error("afg_fbank_check_rows: NULL rows"); return AFG_ERR_INVALID; }
    return check_rows(rows, n_rows, n_tiles, *params, in_floats, table_floats, filters_floats, out_floats);
}

extern "C" int afg_fbank_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_fbank_params *params, const float *d_in,
                             uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters, uint64_t filters_floats,
                             float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = check_params(params, "afg_fbank_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_table, d_filters, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_mel_row *h) {
        return afg::fbank_launch(h, n_rows, d_rows, n_tiles, params, d_in, in_floats, d_table, table_floats, d_filters, filters_floats, d_out,
                                 out_floats, (hipStream_t)hip_stream);
    });
}
