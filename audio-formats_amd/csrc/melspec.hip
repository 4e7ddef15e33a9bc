// melspec.hip -- planar float rows to (log-)mel spectrogram rows (afg_melspec_hip, afg_batch_decode_mel), for gfx950: a
// short-time Fourier transform by direct matrix product, the power spectrum, a dense mel filter bank and an optional log10,
// in one pass.  The definition -- every sum a chain of float32 fmaf in ascending index order from +0.0f -- is in
// include/afg.h; both products run on the exact float32 matrix instruction (v_mfma_f32_16x16x4_f32), whose result is such a
// chain in k order.  The Makefile builds this file with -ffp-contract=off like every other exact-mode kernel.
//
// One workgroup of 256 lanes (four wavefronts) per tile of F frames of one row (afg_mel_row), found by a search over the
// rows' first tiles as collate.hip and resample.hip do.  F is 64, halved down to 16 while the tile's LDS exceeds kLdsBudget.
//   X        the tile's frames, one padded row of K4 = win_length rounded up to 4 samples per frame, staged once with
//            coalesced loads; reflection and zeros are resolved on the way in.  The MFMA's B operand takes frame l & 15 and
//            sample l >> 4 per lane: a Toeplitz view (frame f's sample n at f * hop + n) would put sixteen frames of hop 160
//            on two LDS banks, so every frame has a row of its own with a pitch that is 4 mod 8 -- sixteen rows then start on
//            sixteen different multiples of four banks, and the 64 lanes of a fetch hit 64 banks.  Only the samples under the
//            window are staged (n_lo .. n_lo + win_length of a frame).
//   product 1 D[bin][frame] = sum over n of basis[n][bin] * X[frame][n]: the basis fragment (A operand: bin l & 15, sample
//            l >> 4; four 64-byte pieces of the table per load, read through L2) is used for all F / 16 frame groups and for
//            the cosine and the sine half: 2 F / 16 independent accumulators per wavefront.  A wavefront owns one column tile
//            of 16 bins per round; a round is 64 bins.
//   p        fmaf(im, im, re * re) in registers; bins >= n_bins are written as +0.0f; into the round's P chunk in LDS
//   product 2 D[mel][frame] += sum over the round's bins of Wm[mel][bin] * P[bin][frame]: rounds ascend, so every mel chain
//            sees its bins in ascending order; a wavefront owns mel tiles w, w + 4, w + 8, w + 12
//   store    the mel tile goes through LDS (over X, which is done with) and leaves with lanes along frames: a wavefront
//            writes 64 consecutive frames of one mel row
// Padding: K is padded to a multiple of 4 and the bins to a multiple of 16 with basis and weight entries of +0.0f (loads
// outside the tables are replaced by +0.0f; the tables' own padding columns hold +0.0f) and samples of +0.0f.  A padding
// term is fmaf(+0, +0, acc), which has the bits of acc unless acc is -0.  No chain here holds -0 where it matters: a chain
// starts from +0.0f and x + (-x) is +0 in round-to-nearest, so -0 can only come from a product that underflows to nothing
// from below; re and im enter p squared, p is never negative, and with weights >= 0 (every afg_mel_filters bank) no mel
// term is.  (A caller's own bank with negative weights whose products underflow completely may see +0 for -0.)  A padded
// bin's re and im are NOT relied on -- an infinite sample times a zero basis entry is NaN -- which is why p is forced.
//
// Bounds: every row is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + g] for 0 <= g < in_frames only, basis[0 .. win_length * ld) and filters[0 .. n_mels * n_bins) only, and writes
// out[out_off .. out_off + n_mels * out_frames) only.
#include "mel_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTileMax = 64, kTileMin = 16;               // frames per tile
constexpr uint32_t kRoundBins = 64;                             // bins per round: one column tile of 16 per wavefront
constexpr uint32_t kMelTiles = 4;                               // mel tiles of 16 per wavefront: 256 mels
constexpr uint32_t kLdsBudget = 152 * 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MelGeo {
    uint32_t K4, pitch, nb16, ld, F, ppitch, mpitch, x_floats, lds_floats;
};

__host__ __device__ inline uint32_t max_frames_of(const afg_mel_params &p, uint32_t in_frames)
{
    const int64_t num = (int64_t)in_frames + 2 * (int64_t)(p.center ? p.n_fft / 2 : 0) - (int64_t)p.n_fft;
    return num < 0 ? 0 : (uint32_t)(1 + num / (int64_t)p.hop);
}

// (params already checked: check_params)
__host__ __device__ inline MelGeo geo_of(const afg_mel_params &p)
{
    MelGeo g;
    g.K4 = (p.win_length + 3) & ~3u;
    g.pitch = (g.K4 & 7) == 4 ? g.K4 : g.K4 + 4;
    g.nb16 = (p.n_fft / 2 + 1 + 15) & ~15u;
    g.ld = 2 * g.nb16;
    const uint32_t mel16 = (p.n_mels + 15) & ~15u;
    for (g.F = kTileMax;; g.F >>= 1) {
        g.ppitch = g.F == 16 ? 16 : g.F + 16;                  // 16 mod 64: four bins' rows of 16 frames on 64 banks
        g.mpitch = g.F + 4;
        g.x_floats = g.F * g.pitch > mel16 * g.mpitch ? g.F * g.pitch : mel16 * g.mpitch;
        g.lds_floats = g.x_floats + kRoundBins * g.ppitch;
        if (g.F == kTileMin || g.lds_floats * 4 <= kLdsBudget) break;
    }
    return g;
}

template <int G>
__global__ __launch_bounds__(kThreads) void melspec_kernel(uint32_t n_rows, const afg_mel_row *__restrict__ rows, afg_mel_params prm, MelGeo geo,
                                                           const float *__restrict__ in, const float *__restrict__ basis,
                                                           const float *__restrict__ filters, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr uint32_t F = 16 * G;
    float *const X = lds, *const P = lds + geo.x_floats;
    const uint64_t tile = blockIdx.x;
    // the row of this tile: the last one whose first tile is <= tile (rows without output have no tiles)
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_mel_row::first_tile);
    const afg_mel_row r = rows[lo];
    if (r.first_tile > tile) return;
    const uint64_t t0 = (tile - r.first_tile) * F;              // first frame of the tile
    if (t0 >= r.out_frames) return;
    const uint32_t n = (uint32_t)min((uint64_t)F, r.out_frames - t0);
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t li = lane & 15, lk = lane >> 4;
    const uint32_t n_bins = prm.n_fft / 2 + 1, win = prm.win_length;

    // ---- X: frame f's windowed samples at X[f * pitch + j]; j >= win_length, and frames the tile does not have, are +0.0f
    {
        const int64_t nin = r.in_frames;
        const int64_t base = (int64_t)(prm.n_fft - win) / 2 - (int64_t)(prm.center ? prm.n_fft / 2 : 0);
        const float *x = in + r.in_off;
        for (uint32_t f = wave; f < F; f += kThreads / 64) {
            const int64_t s0 = (int64_t)(t0 + f) * prm.hop + base;
            float *row = X + f * geo.pitch;
            for (uint32_t j = lane; j < geo.K4; j += 64) {
                float v = 0.0f;
                if (f < n && j < win) {
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

    f32x4 mel[kMelTiles][G];
#pragma unroll
    for (uint32_t t = 0; t < kMelTiles; t++)
#pragma unroll
        for (int g = 0; g < G; g++) mel[t][g] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const uint32_t mel_tiles = (prm.n_mels + 15) >> 4;

    for (uint32_t b0 = 0; b0 < n_bins; b0 += kRoundBins) {
        // ---- product 1: this wavefront's 16 bins x F frames, cosine and sine
        const uint32_t cb = b0 + wave * 16;
        f32x4 re[G], im[G];
#pragma unroll
        for (int g = 0; g < G; g++) re[g] = im[g] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
        if (cb < n_bins) {                                       // (uniform per wavefront)
            const float *bc = basis + cb + li;                   // cb + li < nb16: inside the table's row
            const float *xb = X + li * geo.pitch + lk;
            for (uint32_t j0 = 0; j0 < geo.K4; j0 += 4) {
                const uint32_t j = j0 + lk;
                float ac = 0.0f, as = 0.0f;
                if (j < win) { ac = bc[(uint64_t)j * geo.ld]; as = bc[(uint64_t)j * geo.ld + geo.nb16]; }
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const float xv = xb[g * 16 * geo.pitch + j0];
                    re[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac, xv, re[g], 0, 0, 0);
                    im[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, xv, im[g], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                         // the round before has read its P
        // ---- p: D holds bin cb + 4 lk + e (register e) of frame 16 g + li
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float a = re[g][e], b = im[g][e];
                const float pw = __builtin_fmaf(b, b, a * a);
                P[(wave * 16 + lk * 4 + e) * geo.ppitch + g * 16 + li] = cb + lk * 4 + e < n_bins ? pw : 0.0f;
            }
        __syncthreads();
        // ---- product 2: the round's bins into the mel chains
        const uint32_t kn = min(kRoundBins, (n_bins - b0 + 3) & ~3u);
#pragma unroll
        for (uint32_t t = 0; t < kMelTiles; t++) {
            const uint32_t mt = wave + 4 * t;
            if (mt >= mel_tiles) continue;                       // (uniform per wavefront)
            const uint32_t m = mt * 16 + li;
            const float *wr = filters + (uint64_t)(m < prm.n_mels ? m : 0) * n_bins;
            for (uint32_t k0 = 0; k0 < kn; k0 += 4) {
                const uint32_t k = b0 + k0 + lk;
                const float a = (m < prm.n_mels && k < n_bins) ? wr[k] : 0.0f;
#pragma unroll
                for (int g = 0; g < G; g++)
                    mel[t][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, P[(k0 + lk) * geo.ppitch + g * 16 + li], mel[t][g], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                             // X is done with: the mel tile goes over it
    float *const M = lds;
#pragma unroll
    for (uint32_t t = 0; t < kMelTiles; t++) {
        const uint32_t mt = wave + 4 * t;
        if (mt >= mel_tiles) continue;
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
            for (int e = 0; e < 4; e++) M[(mt * 16 + lk * 4 + e) * geo.mpitch + g * 16 + li] = mel[t][g][e];
    }
    __syncthreads();
    const float floor_ = prm.log_floor == 0.0f ? 1e-10f : prm.log_floor;
    float *y = out + r.out_off + t0;
    for (uint32_t i = threadIdx.x; i < prm.n_mels * F; i += kThreads) {
        const uint32_t m = i / F, f = i % F;
        if (f >= n) continue;
        float v = M[m * geo.mpitch + f];
        if (prm.out_kind == AFG_MEL_LOG10) v = log10f(fmaxf(v, floor_));
        y[(uint64_t)m * r.out_frames + f] = v;
    }
}

int check_params(const afg_mel_params *p)
{
    if (!p) { afg::set_error("afg_melspec_hip: NULL params"); return AFG_ERR_INVALID; }
    if (p->n_fft < 16 || p->n_fft > 2048) { afg::set_error("afg_mel_params.n_fft %u: 16 .. 2048", p->n_fft); return AFG_ERR_INVALID; }
    if (p->win_length < 1 || p->win_length > p->n_fft) { afg::set_error("afg_mel_params.win_length %u: 1 .. n_fft (%u)", p->win_length, p->n_fft); return AFG_ERR_INVALID; }
    if (p->hop < 1 || p->hop > p->n_fft) { afg::set_error("afg_mel_params.hop %u: 1 .. n_fft (%u)", p->hop, p->n_fft); return AFG_ERR_INVALID; }
    if (p->n_mels < 1 || p->n_mels > 256) { afg::set_error("afg_mel_params.n_mels %u: 1 .. 256", p->n_mels); return AFG_ERR_INVALID; }
    if (p->center > 1) { afg::set_error("afg_mel_params.center %u: 0 or 1", p->center); return AFG_ERR_INVALID; }
    if (p->pad_mode != AFG_MEL_PAD_REFLECT && p->pad_mode != AFG_MEL_PAD_ZERO) { afg::set_error("afg_mel_params.pad_mode %u: AFG_MEL_PAD_REFLECT or AFG_MEL_PAD_ZERO", p->pad_mode); return AFG_ERR_INVALID; }
    if (p->out_kind != AFG_MEL_POWER && p->out_kind != AFG_MEL_LOG10) { afg::set_error("afg_mel_params.out_kind %u: AFG_MEL_POWER or AFG_MEL_LOG10", p->out_kind); return AFG_ERR_INVALID; }
    if (!(p->log_floor >= 0.0f) || p->log_floor > 3.0e38f) { afg::set_error("afg_mel_params.log_floor %g: a finite float >= 0 (0 means 1e-10)", (double)p->log_floor); return AFG_ERR_INVALID; }
    return AFG_OK;
}

uint64_t tiles_of(const afg_mel_row &r, uint32_t F) { return ((uint64_t)r.out_frames + F - 1) / F; }

// every row against the planes, the tables and the tile table, before anything runs
int check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_mel_params &p, uint64_t in_floats, uint64_t basis_floats,
               uint64_t filters_floats, uint64_t out_floats)
{
    const MelGeo g = geo_of(p);
    const uint32_t pad = p.center ? p.n_fft / 2 : 0;
    if (basis_floats < (uint64_t)p.win_length * g.ld) {
        afg::set_error("afg_melspec_hip: basis_floats %llu: afg_mel_basis gives %llu", (unsigned long long)basis_floats, (unsigned long long)p.win_length * g.ld);
        return AFG_ERR_INVALID;
    }
    if (filters_floats < (uint64_t)p.n_mels * (p.n_fft / 2 + 1)) {
        afg::set_error("afg_melspec_hip: filters_floats %llu: the bank is n_mels x n_bins = %llu floats", (unsigned long long)filters_floats,
                       (unsigned long long)p.n_mels * (p.n_fft / 2 + 1));
        return AFG_ERR_INVALID;
    }
    return afg::check_mel_rows("afg_melspec_hip", "afg_mel_layout", rows, n_rows, n_tiles, g.F, p.pad_mode == AFG_MEL_PAD_REFLECT ? pad : 0, p.n_mels,
                               in_floats, out_floats, [&](uint32_t in_frames) { return max_frames_of(p, in_frames); });
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const float *d_in, const float *d_basis, const float *d_filters,
               float *d_out)
{
    if (!d_rows || !d_basis || !d_filters || !d_out) {
        afg::set_error("afg_melspec_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_basis & 3u) != 0 || ((uintptr_t)d_filters & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) {
        afg::set_error("afg_melspec_hip: the planes must be 4-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_melspec_hip", "rows", n_rows, n_tiles);
}

template <int G>
int launch_g(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params &p, const MelGeo &g, const float *d_in,
             const float *d_basis, const float *d_filters, float *d_out, hipStream_t stream)
{
    const size_t bytes = (size_t)g.lds_floats * sizeof(float);
    AFG_HIP_CHECK(hipFuncSetAttribute((const void *)melspec_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(melspec_kernel<G>, dim3((uint32_t)n_tiles), dim3(kThreads), bytes, stream, (uint32_t)n_rows, d_rows, p, g, d_in, d_basis,
                       d_filters, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

}  // namespace

int afg::melspec_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params,
                        const float *d_in, uint64_t in_floats, const float *d_basis, uint64_t basis_floats, const float *d_filters,
                        uint64_t filters_floats, float *d_out, uint64_t out_floats, hipStream_t stream)
{
    if (int rc = check_params(params)) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_basis, d_filters, d_out)) return rc;
    if (int rc = check_rows(h_rows, n_rows, n_tiles, *params, in_floats, basis_floats, filters_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (int rc = afg::require_device()) return rc;
    const MelGeo g = geo_of(*params);
    static_assert((size_t)kLdsBudget <= 160 * 1024, "LDS budget");
    if ((size_t)g.lds_floats * sizeof(float) > 160 * 1024) {     // (n_fft <= 2048 and n_mels <= 256 stay below: geo_of)
        afg::set_error("afg_melspec_hip: a tile of %u frames needs %u floats of LDS", g.F, g.lds_floats);
        return AFG_ERR_INVALID;
    }
    switch (g.F) {
    case 64: return launch_g<4>(n_rows, d_rows, n_tiles, *params, g, d_in, d_basis, d_filters, d_out, stream);
    case 32: return launch_g<2>(n_rows, d_rows, n_tiles, *params, g, d_in, d_basis, d_filters, d_out, stream);
    default: return launch_g<1>(n_rows, d_rows, n_tiles, *params, g, d_in, d_basis, d_filters, d_out, stream);
    }
}

extern "C" uint64_t afg_mel_layout(afg_mel_row *rows, uint64_t n_rows, const afg_mel_params *params)
{
    if (check_params(params)) return 0;
    const uint32_t F = geo_of(*params).F;
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += tiles_of(rows[k], F);
    }
    return tiles;
}

extern "C" uint32_t afg_mel_frames(const afg_mel_params *params, uint32_t in_frames)
{
    if (check_params(params)) return 0;
    return max_frames_of(*params, in_frames);
}

extern "C" int afg_mel_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_mel_params *params, uint64_t in_floats,
                                  uint64_t basis_floats, uint64_t filters_floats, uint64_t out_floats)
{
    if (int rc = check_params(params)) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!rows) { afg::set_error("afg_mel_check_rows: NULL rows"); return AFG_ERR_INVALID; }
    return check_rows(rows, n_rows, n_tiles, *params, in_floats, basis_floats, filters_floats, out_floats);
}

extern "C" int afg_melspec_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params, const float *d_in,
                               uint64_t in_floats, const float *d_basis, uint64_t basis_floats, const float *d_filters, uint64_t filters_floats,
                               float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = check_params(params)) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_basis, d_filters, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_mel_row *h) {
        return afg::melspec_launch(h, n_rows, d_rows, n_tiles, params, d_in, in_floats, d_basis, basis_floats, d_filters, filters_floats,
                                   d_out, out_floats, (hipStream_t)hip_stream);
    });
}
