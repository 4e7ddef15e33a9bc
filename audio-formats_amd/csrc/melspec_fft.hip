// melspec_fft.hip -- the opt-in fast path of the mel spectrogram features (afg_melspec_fft_hip, AFG_MEL_ALGO_FFT), for gfx950:
// the value include/afg.h defines for afg_melspec_hip, with the short-time Fourier transform computed by a mixed-radix FFT
// per frame instead of a matrix product.  Only the float32 summation order differs from the direct kernel (melspec.hip); the
// result is held to the error bound stated in include/afg.h, not to bit patterns.
//
// One workgroup of 256 lanes (four wavefronts) per tile of kTile = 16 frames of one row (afg_mel_row), found by the search
// over the rows' first tiles that the other stages use.
//   transform  every wavefront owns whole frames (w, w + waves, ...), so no workgroup barrier stands inside the transform.
//              The frame's samples are fetched with lanes along samples (coalesced; reflection and zeros resolved on the
//              way in), multiplied by the window and written into the wavefront's own LDS buffer.  An even n_fft runs the
//              complex transform of half the length over z[j] = x[2j] + i x[2j+1] and a split pass; an odd n_fft runs the
//              full length with a zero imaginary part.  Both are transforms of ONE frame: a non-finite sample cannot leave
//              its frame.  The passes are Stockham autosort passes of radix 4, 2, 3 and 5 between two buffers (real and
//              imaginary parts in planes of their own, so a pass's reads are consecutive floats), with the twiddles read
//              from afg_mel_fft_tables' table through L1 / L2.
//   p          re * re + im * im into P[bin][frame] in LDS, pitch 17: a wavefront writes one frame's bins, 17 floats apart,
//              on 32 different banks per half.  Frames the tile does not have are written as +0.0f.
//   mel        D[mel][frame] = sum over bins of Wm[mel][bin] * P[bin][frame] on v_mfma_f32_16x16x4_f32 as in melspec.hip
//              (A: mel l & 15, bin l >> 4; B: frame l & 15, bin l >> 4); a wavefront owns mel tiles w, w + 4, w + 8, w + 12.
//              A column of the product depends on that column of P alone: frames do not mix.
//   store      D holds mel 4 (l >> 4) + e of frame l & 15: sixteen lanes write sixteen consecutive frames of one mel row.
// Samples are read through the caches, not staged per tile: a frame is read once by its own wavefront, and the overlap of
// neighbouring frames (win_length / hop reads per sample) is served by L1 / L2.
//
// Bounds: every row is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + g] for 0 <= g < in_frames only, table[0 .. win_length + 2 * n_fft) and filters[0 .. n_mels * n_bins) only, and
// writes out[out_off .. out_off + n_mels * out_frames) only.
#include "mel_rows.h"
#include "fft_frame.h"

#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = 16;                                  // frames per tile: one MFMA column block
constexpr uint32_t kPPitch = 17;
constexpr uint32_t kMelTiles = 4;                               // mel tiles of 16 per wavefront: 256 mels
constexpr uint32_t kLdsBudget = 152 * 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// (params already checked: check_params)
FftGeo geo_of(const afg_mel_params &p)
{
    FftGeo g = fft_geo_of(p.n_fft);
    const uint32_t p_floats = (p.n_fft / 2 + 1) * kPPitch;
    for (g.waves = 4;; g.waves >>= 1) {
        g.lds_floats = g.waves * g.wbuf + p_floats;
        if (g.waves == 1 || g.lds_floats * 4 <= kLdsBudget) break;
    }
    return g;
}

__global__ __launch_bounds__(kThreads) void melspec_fft_kernel(uint32_t n_rows, const afg_mel_row *__restrict__ rows, afg_mel_params prm, FftGeo geo,
                                                               const float *__restrict__ in, const float *__restrict__ table,
                                                               const float *__restrict__ filters, float *__restrict__ out)
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
    const uint32_t li = lane & 15, lk = lane >> 4;
    const uint32_t n_fft = prm.n_fft, n_bins = n_fft / 2 + 1, win = prm.win_length, n_lo = (n_fft - win) / 2, nc = geo.nc;
    float *const P = lds + geo.waves * geo.wbuf;
    const float *const tw = table + win;

    if (wave < geo.waves) {
        float *const buf = lds + wave * geo.wbuf;
        const int64_t nin = r.in_frames;
        const float *x = in + r.in_off;
        for (uint32_t f = wave; f < kTile; f += geo.waves) {
            if (f >= n) {                                        // (uniform per wavefront)
                for (uint32_t k = lane; k < n_bins; k += 64) P[k * kPPitch + f] = 0.0f;
                continue;
            }
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
            // ---- p of bins 0 .. n_fft / 2
            for (uint32_t k = lane; k < n_bins; k += 64) {
                const cf X = geo.half ? fft_split_bin(sr, si, nc, k, tw) : cf{ sr[k], si[k] };
                P[k * kPPitch + f] = X.re * X.re + X.im * X.im;
            }
        }
    }
    __syncthreads();

    // ---- mel: the bank times P, and the store
    const uint32_t mel_tiles = (prm.n_mels + 15) >> 4;
    const float floor_ = prm.log_floor == 0.0f ? 1e-10f : prm.log_floor;
    float *y = out + r.out_off + t0;
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
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t mm = mt * 16 + lk * 4 + e;
            if (mm >= prm.n_mels || li >= n) continue;
            float v = acc[e];
            if (prm.out_kind == AFG_MEL_LOG10) v = log10f(fmaxf(v, floor_));
            y[(uint64_t)mm * r.out_frames + li] = v;
        }
    }
}

int check_params(const afg_mel_params *p, const char *who)
{
    if (int rc = afg_mel_check_rows(nullptr, 0, 0, p, 0, 0, 0, 0)) return rc;        // the ranges of the direct path
    if (!n_fft_ok(p->n_fft)) {
        afg::set_error("%s: n_fft %u: the FFT path takes 16 .. 2048 with prime factors 2, 3 and 5 only (AFG_MEL_ALGO_DIRECT takes the rest)", who, p->n_fft);
        return AFG_ERR_UNSUPPORTED;
    }
    return AFG_OK;
}

uint32_t max_frames_of(const afg_mel_params &p, uint32_t in_frames)
{
    const int64_t num = (int64_t)in_frames + 2 * (int64_t)(p.center ? p.n_fft / 2 : 0) - (int64_t)p.n_fft;
    return num < 0 ? 0 : (uint32_t)(1 + num / (int64_t)p.hop);
}

uint64_t tiles_of(const afg_mel_row &r) { return ((uint64_t)r.out_frames + kTile - 1) / kTile; }

// every row against the planes, the tables and the tile table, before anything runs
int check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_mel_params &p, uint64_t in_floats, uint64_t table_floats,
               uint64_t filters_floats, uint64_t out_floats)
{
    const uint32_t pad = p.center ? p.n_fft / 2 : 0;
    if (table_floats < (uint64_t)p.win_length + 2 * (uint64_t)p.n_fft) {
        afg::set_error("afg_melspec_fft_hip: table_floats %llu: afg_mel_fft_tables gives %llu", (unsigned long long)table_floats,
                       (unsigned long long)p.win_length + 2 * (unsigned long long)p.n_fft);
        return AFG_ERR_INVALID;
    }
    if (filters_floats < (uint64_t)p.n_mels * (p.n_fft / 2 + 1)) {
        afg::set_error("afg_melspec_fft_hip: filters_floats %llu: the bank is n_mels x n_bins = %llu floats", (unsigned long long)filters_floats,
                       (unsigned long long)p.n_mels * (p.n_fft / 2 + 1));
        return AFG_ERR_INVALID;
    }
    return afg::check_mel_rows("afg_melspec_fft_hip", "afg_mel_fft_layout", rows, n_rows, n_tiles, kTile, p.pad_mode == AFG_MEL_PAD_REFLECT ? pad : 0,
                               p.n_mels, in_floats, out_floats, [&](uint32_t in_frames) { return max_frames_of(p, in_frames); });
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const float *d_in, const float *d_table, const float *d_filters,
               float *d_out)
{
    if (!d_rows || !d_table || !d_filters || !d_out) {
        afg::set_error("afg_melspec_fft_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_table & 3u) != 0 || ((uintptr_t)d_filters & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_melspec_fft_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_melspec_fft_hip", "rows", n_rows, n_tiles);
}

}  // namespace

bool afg::mel_fft_n_ok(uint32_t n_fft) { return n_fft_ok(n_fft); }

int afg::melspec_fft_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params,
                            const float *d_in, uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters,
                            uint64_t filters_floats, float *d_out, uint64_t out_floats, hipStream_t stream)
{
    if (int rc = check_params(params, "afg_melspec_fft_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_table, d_filters, d_out)) return rc;
    if (int rc = check_rows(h_rows, n_rows, n_tiles, *params, in_floats, table_floats, filters_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (int rc = afg::require_device()) return rc;
    const FftGeo g = geo_of(*params);
    static_assert((size_t)kLdsBudget <= 160 * 1024, "LDS budget");
    const size_t bytes = (size_t)g.lds_floats * sizeof(float);
    if (bytes > 160 * 1024) {                                    // (n_fft <= 2048 stays below: geo_of)
        afg::set_error("afg_melspec_fft_hip: n_fft %u needs %u floats of LDS", params->n_fft, g.lds_floats);
        return AFG_ERR_INVALID;
    }
    AFG_HIP_CHECK(hipFuncSetAttribute((const void *)melspec_fft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(melspec_fft_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), bytes, stream, (uint32_t)n_rows, d_rows, *params, g, d_in,
                       d_table, d_filters, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" uint64_t afg_mel_fft_layout(afg_mel_row *rows, uint64_t n_rows, const afg_mel_params *params)
{
    if (check_params(params, "afg_mel_fft_layout")) return 0;
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += tiles_of(rows[k]);
    }
    return tiles;
}

extern "C" int afg_mel_fft_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_mel_params *params, uint64_t in_floats,
                                      uint64_t table_floats, uint64_t filters_floats, uint64_t out_floats)
{
    if (int rc = check_params(params, "afg_mel_fft_check_rows")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!rows) { afg::set_error("afg_mel_fft_check_rows: NULL rows"); return AFG_ERR_INVALID; }
    return check_rows(rows, n_rows, n_tiles, *params, in_floats, table_floats, filters_floats, out_floats);
}

extern "C" int afg_melspec_fft_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params, const float *d_in,
                                   uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters,
                                   uint64_t filters_floats, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = check_params(params, "afg_melspec_fft_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_table, d_filters, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_mel_row *h) {
        return afg::melspec_fft_launch(h, n_rows, d_rows, n_tiles, params, d_in, in_floats, d_table, table_floats, d_filters,
                                       filters_floats, d_out, out_floats, (hipStream_t)hip_stream);
    });
}
