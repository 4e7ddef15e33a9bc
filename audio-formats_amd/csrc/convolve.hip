// convolve.hip -- convolution of waveform rows with the kernels of a bank (afg_convolve_hip, afg_convolve_bank_hip), for
// gfx950: y = h * x, delivered as a range of the line per record (include/afg.h has the definition, the two contracts and
// the bound).  A kernel of at most direct_max taps takes the direct path, every other the FFT path.
//
// Direct (conv_direct_kernel).  A workgroup of 256 lanes per tile of kDirectTile = 4096 delivered samples of one record,
// found by the search over first_tile that the other stages use.  It stages the taps (hs) and the tile's span of the row
// with a halo of taps - 1 samples in front (xs, zero where the line leaves the row) in LDS.  The tile is cut at the 16-byte
// boundaries of the output address: the interior is quads of four consecutive samples, quad w of the tile by lane w & 255
// in round w >> 8 -- the lane-interleaved dwordx4 store shape, one store instruction of the workgroup writing 4 KiB whole --
// head and tail one float per lane.  xs is shifted so that a quad's first sample sits at a multiple of four floats: a quad
// walks the taps four at a time with one ds_read_b128 of the row (the four samples before the window it holds) and one
// broadcast ds_read_b128 of the taps per 16 fmaf.  Every sample's sum is acc = +0.0f, acc = fmaf(h[k], x[n - k], acc) in
// ascending k over the terms inside the row: a quad whose terms all lie inside takes the blocked walk, any other the plain
// loop with its own k range, and both give the same bits.
//
// FFT: uniformly partitioned overlap-save on fft_frame.h, B = 1024, n_fft = 2048, a wavefront per transform (a workgroup
// is one wavefront with 16 KB of LDS: its two buffers).
//   conv_bank_kernel     partition p of a kernel, h[p B .. p B + B) and B zeros behind, to its spectrum in d_spec
//   conv_spectra_kernel  (a) block pair j of a row, x[(j - 1) B .. (j + 1) B) with zeros outside the row, to d_work
//   conv_blocks_kernel   (b) output block b of a record: lane l holds Y of the bins l + 64 i, i < 8, and of their partners
//                        1024 - (l + 64 i) -- the two bins a value of the half-length inverse needs -- and bin 512; it adds
//                        H_p X_{b-p} in ascending p from +0.0f, 8-byte loads that run along the bins, up in one half and
//                        down in the other.  fft_unsplit_bin with s = 1 / 2048 makes Z, swapped into the wavefront's buffers,
//                        the forward passes run, and the planes come out swapped again: sample 2 m in zi[m], 2 m + 1 in
//                        zr[m].  The last B samples go out as v + 0.0f, lanes along consecutive samples.
// A spectrum is 1025 pairs (re, im).  The table (2048 pairs) is the head of d_spec.  NaN: a pair or partition that holds one
// is stored as NaN in every bin, and a block whose Y holds one is delivered as NaN whole (wavefront votes).
//
// Bounds: every record is checked on the host before a launch (check_rows, check_bank); the kernels rely on it.  They read
// in[in_off .. in_off + frames), bank[bank_off .. bank_off + taps), the spectra and the table, read and write the record's
// own spectra in d_work, and write out[out_off .. out_off + out_frames) only.  No atomics, no inline assembly.
#include "afg_records.h"
#include "fft_frame.h"

#include <cmath>
#include <limits>
#include <vector>

namespace {

constexpr int kDirectThreads = 256;
constexpr uint32_t kB = AFG_CONV_BLOCK, kNfft = 2 * kB, kSpec = AFG_CONV_SPEC_FLOATS, kTable = AFG_CONV_TABLE_FLOATS;
constexpr uint32_t kDirectTile = AFG_CONV_DIRECT_TILE, kDirectMax = AFG_CONV_DIRECT_MAX;
constexpr uint32_t kXs = 4 + 3 + (kDirectMax - 1) + kDirectTile + 2;       // slack, shift, halo, tile; a multiple of 4
constexpr uint32_t kMaxFrames = 0x7fff0000u;                               // 2^31 - 65536: line positions fit 32 bits, signed

static_assert(sizeof(afg_convolve_params) == 32 && sizeof(afg_convolve_kernel) == 24 && sizeof(afg_convolve_row) == 48, "include/afg.h");
static_assert(kTable == 2 * kNfft && kSpec == 2 * (kB + 1) && kXs % 4 == 0, "include/afg.h");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- what the host and the kernels agree on
__host__ __device__ inline uint32_t parts_of(uint32_t taps) { return (taps + kB - 1) / kB; }
__host__ __device__ inline bool is_direct(uint32_t taps, uint32_t direct_max) { return taps <= direct_max; }
// the last block pair that meets a row of frames >= 1 samples
__host__ __device__ inline uint32_t last_pair(uint32_t frames) { return (frames - 1) / kB + 1; }
// the block pairs an FFT record keeps in the work plane: *j_lo and the count (out_frames >= 1, frames >= 1)
__host__ __device__ inline uint32_t pairs_of(const afg_convolve_row &r, uint32_t taps, uint32_t *j_lo)
{
    const uint32_t b_lo = r.out_first / kB, b_hi = (uint32_t)(((uint64_t)r.out_first + r.out_frames - 1) / kB), P = parts_of(taps);
    const uint32_t lo = b_lo + 1 > P ? b_lo + 1 - P : 0, last = last_pair(r.frames), hi = b_hi < last ? b_hi : last;
    *j_lo = lo;
    return hi >= lo ? hi - lo + 1 : 0;
}

__global__ __launch_bounds__(kDirectThreads) void conv_direct_kernel(uint32_t n_rows, const afg_convolve_row *__restrict__ rows,
                                                                     const afg_convolve_kernel *__restrict__ kernels, uint32_t direct_max,
                                                                     const float *__restrict__ in, const float *__restrict__ bank, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float hs[kDirectMax];
    __shared__ __attribute__((aligned(16))) float xs[kXs];
    const uint64_t tile = blockIdx.x;
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_convolve_row::first_tile);
    const afg_convolve_row r = rows[lo];
    if (r.first_tile > tile || r.out_frames == 0) return;
    const afg_convolve_kernel kr = kernels[r.kernel];
    const uint32_t taps = kr.taps;
    if (!is_direct(taps, direct_max)) return;
    const uint64_t i0 = (tile - r.first_tile) * kDirectTile;    // first delivered sample of the tile
    if (i0 >= r.out_frames) return;
    const int32_t n = (int32_t)min((uint64_t)kDirectTile, r.out_frames - i0);
    const int32_t tid = (int32_t)threadIdx.x, frames = (int32_t)r.frames, T = (int32_t)taps;
    const int32_t N0 = (int32_t)(r.out_first + i0);             // its place in the line
    float *const y = out + r.out_off + i0;
    const float *const x = in + r.in_off;
    const float *const h = bank + kr.bank_off;
    const int32_t head = min(n, (int32_t)((4 - (((uintptr_t)y >> 2) & 3)) & 3)), quads = (n - head) >> 2, tail0 = head + 4 * quads;
    // xs[m - M0] is x[m]: the first quad's first sample at a multiple of 4, four floats of slack in front
    const int32_t shift = (4 - ((T - 1 + head) & 3)) & 3, M0 = N0 - (T - 1) - shift - 4;

    for (int32_t i = tid; i < (int32_t)kDirectMax; i += kDirectThreads) hs[i] = i < T ? h[i] : 0.0f;
    const int32_t span = 4 + shift + T - 1 + n;
    for (int32_t i = tid; i < span; i += kDirectThreads) {
        const int32_t m = M0 + i;
        xs[i] = (i >= 4 + shift && m >= 0 && m < frames) ? x[m] : 0.0f;
    }
    __syncthreads();

    auto plain = [&](int32_t nn) -> float {                     // line sample nn, the terms inside the row
        const int32_t k_lo = nn >= frames ? nn - frames + 1 : 0, k_hi = min(T - 1, nn);
        float acc = 0.0f;
        for (int32_t k = k_lo; k <= k_hi; k++) acc = fmaf(hs[k], xs[nn - k - M0], acc);
        return acc;
    };
    if (tid < head) y[tid] = plain(N0 + tid);
    if (tid < n - tail0) y[tail0 + tid] = plain(N0 + tail0 + tid);
    for (int32_t w = tid; w < quads; w += kDirectThreads) {
        const int32_t n0 = N0 + head + 4 * w, base = n0 - M0;     // base % 4 == 0
        f32x4 v;
        if (n0 >= T - 1 && n0 + 3 < frames) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            f32x4 hi4 = *(const f32x4 *)(xs + base);
            for (int32_t k0 = 0; k0 < T; k0 += 4) {
                const f32x4 lo4 = *(const f32x4 *)(xs + base - k0 - 4), h4 = *(const f32x4 *)(hs + k0);
                const int32_t rem = T - k0;                      // (uniform)
                // x[n0 - k0 - 4 + i] is lo4[i], i < 4, and hi4[i - 4]
                a0 = fmaf(h4.x, hi4.x, a0); a1 = fmaf(h4.x, hi4.y, a1); a2 = fmaf(h4.x, hi4.z, a2); a3 = fmaf(h4.x, hi4.w, a3);
                if (rem > 1) { a0 = fmaf(h4.y, lo4.w, a0); a1 = fmaf(h4.y, hi4.x, a1); a2 = fmaf(h4.y, hi4.y, a2); a3 = fmaf(h4.y, hi4.z, a3); }
                if (rem > 2) { a0 = fmaf(h4.z, lo4.z, a0); a1 = fmaf(h4.z, lo4.w, a1); a2 = fmaf(h4.z, hi4.x, a2); a3 = fmaf(h4.z, hi4.y, a3); }
                if (rem > 3) { a0 = fmaf(h4.w, lo4.y, a0); a1 = fmaf(h4.w, lo4.z, a1); a2 = fmaf(h4.w, lo4.w, a2); a3 = fmaf(h4.w, hi4.x, a3); }
                hi4 = lo4;
            }
            v = { a0, a1, a2, a3 };
        } else {
            v = { plain(n0), plain(n0 + 1), plain(n0 + 2), plain(n0 + 3) };
        }
        __builtin_nontemporal_store(v, (f32x4 *)(y + head + 4 * w));
    }
}

// the spectrum of 2048 samples fetch(i) by one wavefront: 1025 pairs to dst (8-byte aligned); a NaN among the samples makes
// NaN of every bin
template <typename Fetch>
__device__ inline void spectrum_to(const FftGeo &geo, float *lds, const float *__restrict__ tw, uint32_t lane, Fetch fetch, float *__restrict__ dst)
{
    bool bad = false;
    auto checked = [&](uint32_t i) -> float {
        const float v = fetch(i);
        bad |= v != v;
        return v;
    };
    const float *zr, *zi;
    fft_frame(geo, kNfft, lds, tw, lane, checked, &zr, &zi);
    const bool any_bad = __any(bad);
    for (uint32_t k = lane; k <= kB; k += 64) {
        cf X = fft_split_bin(zr, zi, kB, k, tw);
        if (any_bad) X = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::quiet_NaN() };
        *(f32x2 *)(dst + 2 * k) = f32x2{ X.re, X.im };
    }
}

__global__ __launch_bounds__(64) void conv_bank_kernel(uint32_t n_kernels, const afg_convolve_kernel *__restrict__ kernels, FftGeo geo,
                                                       const float *__restrict__ bank, float *__restrict__ spec)
{
    __shared__ __attribute__((aligned(16))) float lds[4 * kB];
    const uint64_t key = (uint64_t)kTable + (uint64_t)blockIdx.x * kSpec;
    const uint32_t lo = afg::last_at_or_before(kernels, n_kernels, key, &afg_convolve_kernel::spec_off);
    const afg_convolve_kernel kr = kernels[lo];
    if (kr.spec_off > key) return;
    const uint32_t p = (uint32_t)((key - kr.spec_off) / kSpec);
    if (p >= parts_of(kr.taps)) return;
    const float *const h = bank + kr.bank_off;
    const uint32_t k0 = p * kB, count = min(kB, kr.taps - k0);
    spectrum_to(geo, lds, spec, threadIdx.x, [&](uint32_t i) { return i < count ? h[k0 + i] : 0.0f; }, spec + key);
}

__global__ __launch_bounds__(64) void conv_spectra_kernel(uint32_t n_rows, const afg_convolve_row *__restrict__ rows,
                                                          const afg_convolve_kernel *__restrict__ kernels, uint32_t direct_max, FftGeo geo,
                                                          const float *__restrict__ in, const float *__restrict__ spec, float *__restrict__ work)
{
    __shared__ __attribute__((aligned(16))) float lds[4 * kB];
    const uint64_t key = (uint64_t)blockIdx.x * kSpec;
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, key, &afg_convolve_row::work_off);
    const afg_convolve_row r = rows[lo];
    if (r.work_off > key || r.out_frames == 0) return;
    const uint32_t taps = kernels[r.kernel].taps;
    if (is_direct(taps, direct_max)) return;
    uint32_t j_lo;
    const uint32_t count = pairs_of(r, taps, &j_lo), local = (uint32_t)((key - r.work_off) / kSpec);
    if (local >= count) return;
    const int32_t m0 = ((int32_t)(j_lo + local) - 1) * (int32_t)kB, frames = (int32_t)r.frames;
    const float *const x = in + r.in_off;
    spectrum_to(geo, lds, spec, threadIdx.x, [&](uint32_t i) {
        const int32_t m = m0 + (int32_t)i;
        return m >= 0 && m < frames ? x[m] : 0.0f;
    }, work + key);
}

__global__ __launch_bounds__(64) void conv_blocks_kernel(uint32_t n_rows, const afg_convolve_row *__restrict__ rows,
                                                         const afg_convolve_kernel *__restrict__ kernels, uint32_t direct_max, FftGeo geo,
                                                         const float *__restrict__ spec, const float *__restrict__ work, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float lds[4 * kB];
    const uint64_t tile = blockIdx.x;
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_convolve_row::first_tile);
    const afg_convolve_row r = rows[lo];
    if (r.first_tile > tile || r.out_frames == 0) return;
    const afg_convolve_kernel kr = kernels[r.kernel];
    if (is_direct(kr.taps, direct_max)) return;
    const uint32_t P = parts_of(kr.taps), b = r.out_first / kB + (uint32_t)(tile - r.first_tile), lane = threadIdx.x;
    const uint64_t end = (uint64_t)r.out_first + r.out_frames;
    if ((uint64_t)b * kB >= end) return;
    uint32_t j_lo;
    const uint32_t count = pairs_of(r, kr.taps, &j_lo);
    const float *const tw = spec;

    // ---- Y of the bins lane + 64 i (ya), of their partners 1024 - (lane + 64 i) (yb) and of bin 512 (yc)
    cf ya[8], yb[8], yc = { 0.0f, 0.0f };
#pragma unroll
    for (int i = 0; i < 8; i++) ya[i] = yb[i] = { 0.0f, 0.0f };
    for (uint32_t p = 0; p < P && p <= b; p++) {
        const uint32_t j = b - p;
        if (j < j_lo || j - j_lo >= count) continue;            // the pair lies wholly outside the row
        const float *const H = spec + kr.spec_off + (uint64_t)p * kSpec, *const X = work + r.work_off + (uint64_t)(j - j_lo) * kSpec;
        auto term = [&](uint32_t k) -> cf {
            const f32x2 hv = *(const f32x2 *)(H + 2 * k), xv = *(const f32x2 *)(X + 2 * k);
            return cmul(cf{ hv.x, hv.y }, cf{ xv.x, xv.y });
        };
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t k = lane + 64 * i;
            ya[i] = ya[i] + term(k);
            yb[i] = yb[i] + term(kB - k);
        }
        yc = yc + term(kB / 2);
    }
    bool bad = (yc.re != yc.re) || (yc.im != yc.im);
#pragma unroll
    for (int i = 0; i < 8; i++) bad |= (ya[i].re != ya[i].re) || (ya[i].im != ya[i].im) || (yb[i].re != yb[i].re) || (yb[i].im != yb[i].im);
    const bool any_bad = __any(bad);

    // ---- the split pass backwards into the buffers, planes swapped; the passes; the planes come out swapped again
    const float s = 1.0f / (float)kNfft;
    float *const sr = lds, *const si = lds + kB;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t k = lane + 64 * i;
        if (k == 0) {
            const float a = ya[i].re, c = yb[i].re;             // the two real-only bins
            sr[0] = s * (a - c); si[0] = s * (a + c);
        } else {
            const cf Z1 = fft_unsplit_bin(ya[i], yb[i], s, k, tw), Z2 = fft_unsplit_bin(yb[i], ya[i], s, kB - k, tw);
            sr[k] = Z1.im; si[k] = Z1.re;
            sr[kB - k] = Z2.im; si[kB - k] = Z2.re;
        }
    }
    if (lane == 0) {
        const cf Z = fft_unsplit_bin(yc, yc, s, kB / 2, tw);
        sr[kB / 2] = Z.im; si[kB / 2] = Z.re;
    }
    wave_sync();
    const float *zr, *zi;
    fft_passes(geo, kNfft, lds, tw, lane, &zr, &zi);

    // ---- the last B of the 2 B samples, cropped to the record's range
    const uint64_t n_lo = max((uint64_t)b * kB, (uint64_t)r.out_first), n_hi = min((uint64_t)(b + 1) * kB, end);
    float *const y = out + r.out_off;
    for (uint64_t nn = n_lo + lane; nn < n_hi; nn += 64) {
        const uint32_t t = kB + (uint32_t)(nn - (uint64_t)b * kB);
        const float v = (t & 1) ? zr[t >> 1] : zi[t >> 1];
        y[nn - r.out_first] = any_bad ? std::numeric_limits<float>::quiet_NaN() : v + 0.0f;
    }
}

// ---- the host half
int check_params(const afg_convolve_params *p, const char *who)
{
    if (!p) { afg::set_error("%s: NULL params", who); return AFG_ERR_INVALID; }
    if (p->direct_max > kDirectMax) { afg::set_error("afg_convolve_params.direct_max %u: 0 .. %u", p->direct_max, kDirectMax); return AFG_ERR_INVALID; }
    for (uint32_t v : p->reserved)
        if (v != 0) { afg::set_error("afg_convolve_params.reserved: must be 0"); return AFG_ERR_INVALID; }
    return AFG_OK;
}

int check_taps(uint32_t taps, unsigned long long k)
{
    if (taps == 0) { afg::set_error("afg_convolve_kernel %llu: taps 0: 1 .. %u", k, (unsigned)AFG_CONV_MAX_TAPS); return AFG_ERR_INVALID; }
    if (taps > AFG_CONV_MAX_TAPS) {
        afg::set_error("afg_convolve_kernel %llu: taps %u: at most %u (%u partitions of %u)", k, taps, (unsigned)AFG_CONV_MAX_TAPS,
                       (unsigned)(AFG_CONV_MAX_TAPS / kB), kB);
        return AFG_ERR_UNSUPPORTED;
    }
    return AFG_OK;
}

// every kernel against the bank and the spectrum plane; *need: the plane's floats
int check_bank(const afg_convolve_kernel *kernels, uint64_t n_kernels, uint64_t bank_floats, uint64_t spec_floats, const char *who)
{
    uint64_t at = kTable;
    for (uint64_t k = 0; k < n_kernels; k++) {
        const afg_convolve_kernel &kr = kernels[k];
        const unsigned long long kk = (unsigned long long)k;
        if (int rc = check_taps(kr.taps, kk)) return rc;
        if (kr.reserved != 0) { afg::set_error("afg_convolve_kernel %llu: reserved must be 0", kk); return AFG_ERR_INVALID; }
        if (!afg::rows_inside(kr.bank_off, 1, 0, kr.taps, bank_floats)) {
            afg::set_error("afg_convolve_kernel %llu: its %u taps leave the bank (%llu floats)", kk, kr.taps, (unsigned long long)bank_floats);
            return AFG_ERR_INVALID;
        }
        if (kr.spec_off != at) {
            afg::set_error("afg_convolve_kernel %llu: spec_off %llu, afg_convolve_bank_layout gives %llu", kk, (unsigned long long)kr.spec_off,
                           (unsigned long long)at);
            return AFG_ERR_INVALID;
        }
        at += (uint64_t)parts_of(kr.taps) * kSpec;
    }
    if (spec_floats < at) {
        afg::set_error("%s: spec_floats %llu: afg_convolve_bank_layout gives %llu", who, (unsigned long long)spec_floats, (unsigned long long)at);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

uint64_t tiles_of(const afg_convolve_row &r, uint32_t taps, uint32_t direct_max)
{
    if (r.out_frames == 0) return 0;
    if (is_direct(taps, direct_max)) return ((uint64_t)r.out_frames + kDirectTile - 1) / kDirectTile;
    return ((uint64_t)r.out_first + r.out_frames - 1) / kB - r.out_first / kB + 1;
}

uint64_t work_of(const afg_convolve_row &r, uint32_t taps, uint32_t direct_max)
{
    if (r.out_frames == 0 || r.frames == 0 || is_direct(taps, direct_max)) return 0;
    uint32_t j_lo;
    return (uint64_t)pairs_of(r, taps, &j_lo) * kSpec;
}

bool meet(uint64_t a, uint64_t a_len, uint64_t b, uint64_t b_len) { return a_len && b_len && a < b + b_len && b < a + a_len; }

// every row against the planes, the bank and the two layouts, before anything runs (params and bank checked)
int check_rows(const afg_convolve_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_convolve_kernel *kernels, uint64_t n_kernels,
               const afg_convolve_params &p, uint64_t in_floats, uint64_t bank_floats, uint64_t spec_floats, uint64_t work_floats, uint64_t out_floats,
               const uint64_t *plane_at)
{
    static const char *const planes[4] = { "the input plane", "the bank", "the spectra", "the work plane" };
    const uint64_t lens[4] = { in_floats, bank_floats, spec_floats, work_floats };
    uint64_t tiles = 0, work = 0;
    std::vector<afg::Range> ranges;
    for (uint64_t k = 0; k < n_rows; k++) {
        const afg_convolve_row &r = rows[k];
        const unsigned long long kk = (unsigned long long)k;
        if (r.kernel >= n_kernels) {
            afg::set_error("afg_convolve_row %llu: kernel %u outside the bank of %llu", kk, r.kernel, (unsigned long long)n_kernels);
            return AFG_ERR_INVALID;
        }
        const uint32_t taps = kernels[r.kernel].taps;
        if (r.first_tile != tiles) {
            afg::set_error("afg_convolve_row %llu: first_tile %llu, afg_convolve_layout gives %llu", kk, (unsigned long long)r.first_tile,
                           (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        if (r.work_off != work) {
            afg::set_error("afg_convolve_row %llu: work_off %llu, afg_convolve_layout gives %llu", kk, (unsigned long long)r.work_off,
                           (unsigned long long)work);
            return AFG_ERR_INVALID;
        }
        tiles += tiles_of(r, taps, p.direct_max);
        work += work_of(r, taps, p.direct_max);
        if (r.out_frames == 0) continue;                         // nothing read, nothing written
        if (r.frames == 0) { afg::set_error("afg_convolve_row %llu: %u samples of a row without frames", kk, r.out_frames); return AFG_ERR_INVALID; }
        if (r.frames > kMaxFrames) { afg::set_error("afg_convolve_row %llu: frames %u: at most 2^31 - 65536", kk, r.frames); return AFG_ERR_INVALID; }
        if (!afg::rows_inside(r.in_off, 1, 0, r.frames, in_floats)) {
            afg::set_error("afg_convolve_row %llu: the row's %u samples leave the input (%llu floats)", kk, r.frames, (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        if (!afg::rows_inside(r.out_off, 1, 0, r.out_frames, out_floats)) {
            afg::set_error("afg_convolve_row %llu: the %u delivered samples leave the output (%llu floats)", kk, r.out_frames,
                           (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
        const uint64_t line = (uint64_t)r.frames + taps - 1;
        if ((uint64_t)r.out_first + r.out_frames > line) {
            afg::set_error("afg_convolve_row %llu: samples %u .. %llu, but %u frames and %u taps make a line of %llu", kk, r.out_first,
                           (unsigned long long)r.out_first + r.out_frames, r.frames, taps, (unsigned long long)line);
            return AFG_ERR_INVALID;
        }
        if (plane_at) {
            ranges.push_back(afg::Range{ plane_at[4] + r.out_off, plane_at[4] + r.out_off + r.out_frames, k, true });
            ranges.push_back(afg::Range{ plane_at[0] + r.in_off, plane_at[0] + r.in_off + r.frames, k, false });
        }
    }
    if (tiles != n_tiles) {
        afg::set_error("afg_convolve_hip: n_tiles %llu, afg_convolve_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    if (work_floats < work) {
        afg::set_error("afg_convolve_hip: work_floats %llu: afg_convolve_layout gives %llu", (unsigned long long)work_floats, (unsigned long long)work);
        return AFG_ERR_INVALID;
    }
    if (tiles > 0x7fffffffull || work / kSpec > 0x7fffffffull) {
        afg::set_error("afg_convolve_hip: at most 2^32 - 1 rows, 2^31 - 1 tiles and 2^31 - 1 block pairs per launch");
        return AFG_ERR_INVALID;
    }
    if (plane_at) {
        // the planes an output may not meet, whole, as inputs of owners behind the rows; the work plane only where it is used
        for (uint64_t q = 1; q < 4; q++) {
            const uint64_t len = q == 3 ? work : lens[q];
            if (len) ranges.push_back(afg::Range{ plane_at[q], plane_at[q] + len, n_rows + q, false });
        }
        uint64_t owner = 0, other = 0;
        if (afg::first_overlap(ranges, &owner, &other)) {
            const uint64_t row = owner < n_rows ? owner : other, what = owner < n_rows ? other : owner;
            if (what >= n_rows) afg::set_error("afg_convolve_row %llu: its output overlaps %s", (unsigned long long)row, planes[what - n_rows]);
            else afg::set_error("afg_convolve_row %llu: its output overlaps a row of record %llu", (unsigned long long)owner, (unsigned long long)other);
            return AFG_ERR_INVALID;
        }
        for (uint64_t q = 0; q < 3; q++)
            if (meet(plane_at[3], work, plane_at[q], lens[q])) {
                afg::set_error("afg_convolve_hip: the work plane overlaps %s", planes[q]);
                return AFG_ERR_INVALID;
            }
    }
    return AFG_OK;
}

// the table at the head of the spectrum plane: afg_mel_fft_tables' pairs, made once and kept for the process
const std::vector<float> &table_of()
{
    static const std::vector<float> t = [] {
        std::vector<float> v(1 + (size_t)kTable);
        afg_mel_fft_tables(kNfft, 1, v.data(), v.size());
        v.erase(v.begin());                                      // (the window of one value)
        return v;
    }();
    return t;
}

}  // namespace

extern "C" uint64_t afg_convolve_bank_layout(afg_convolve_kernel *kernels, uint64_t n_kernels)
{
    if (n_kernels && !kernels) { afg::set_error("afg_convolve_bank_layout: NULL kernels"); return 0; }
    uint64_t at = kTable;
    for (uint64_t k = 0; k < n_kernels; k++) {
        if (check_taps(kernels[k].taps, (unsigned long long)k)) return 0;
        kernels[k].spec_off = at;
        at += (uint64_t)parts_of(kernels[k].taps) * kSpec;
    }
    return at;
}

extern "C" int afg_convolve_bank_check(const afg_convolve_kernel *kernels, uint64_t n_kernels, uint64_t bank_floats, uint64_t spec_floats)
{
    if (n_kernels && !kernels) { afg::set_error("afg_convolve_bank_check: NULL kernels"); return AFG_ERR_INVALID; }
    return check_bank(kernels, n_kernels, bank_floats, spec_floats, "afg_convolve_bank_check");
}

extern "C" int afg_convolve_bank_hip(uint64_t n_kernels, const afg_convolve_kernel *d_kernels, const float *d_bank, uint64_t bank_floats, float *d_spec,
                                     uint64_t spec_floats, void *hip_stream)
{
    if (n_kernels == 0) return AFG_OK;
    if (!d_kernels || !d_bank || !d_spec) { afg::set_error("afg_convolve_bank_hip: NULL device pointer"); return AFG_ERR_INVALID; }
    if (((uintptr_t)d_bank & 3u) != 0 || ((uintptr_t)d_spec & 7u) != 0 || ((uintptr_t)d_kernels & 7u) != 0) {
        afg::set_error("afg_convolve_bank_hip: the bank must be 4-byte aligned, the spectra and the records 8-byte");
        return AFG_ERR_INVALID;
    }
    if (n_kernels > 0xffffffffull) { afg::set_error("afg_convolve_bank_hip: at most 2^32 - 1 kernels"); return AFG_ERR_INVALID; }
    if (int rc = afg::require_device()) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint64_t parts = 0;
    if (int rc = afg::with_host_records(d_kernels, n_kernels, stream, [&](const afg_convolve_kernel *h) {
            if (int rc2 = check_bank(h, n_kernels, bank_floats, spec_floats, "afg_convolve_bank_hip")) return rc2;
            parts = (h[n_kernels - 1].spec_off - kTable) / kSpec + parts_of(h[n_kernels - 1].taps);
            if (meet((uintptr_t)d_spec >> 2, (uint64_t)kTable + parts * kSpec, (uintptr_t)d_bank >> 2, bank_floats)) {
                afg::set_error("afg_convolve_bank_hip: the spectra overlap the bank");
                return (int)AFG_ERR_INVALID;
            }
            return (int)AFG_OK;
        }))
        return rc;
    if (parts > 0x7fffffffull) { afg::set_error("afg_convolve_bank_hip: at most 2^31 - 1 partitions"); return AFG_ERR_INVALID; }
    try {
        AFG_HIP_CHECK(hipMemcpyAsync(d_spec, table_of().data(), (size_t)kTable * sizeof(float), hipMemcpyHostToDevice, stream));
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
    hipLaunchKernelGGL(conv_bank_kernel, dim3((uint32_t)parts), dim3(64), 0, stream, (uint32_t)n_kernels, d_kernels, fft_geo_of(kNfft), d_bank, d_spec);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" uint64_t afg_convolve_layout(afg_convolve_row *rows, uint64_t n_rows, const afg_convolve_kernel *kernels, uint64_t n_kernels,
                                        const afg_convolve_params *params, uint64_t *work_floats)
{
    if (work_floats) *work_floats = 0;
    if (check_params(params, "afg_convolve_layout")) return 0;
    if (n_rows == 0) return 0;
    if (!rows || !kernels) { afg::set_error("afg_convolve_layout: NULL records"); return 0; }
    for (uint64_t k = 0; k < n_rows; k++)
        if (rows[k].kernel >= n_kernels) {
            afg::set_error("afg_convolve_row %llu: kernel %u outside the bank of %llu", (unsigned long long)k, rows[k].kernel, (unsigned long long)n_kernels);
            return 0;
        }
    uint64_t tiles = 0, work = 0;
    for (uint64_t k = 0; k < n_rows; k++) {
        const uint32_t taps = kernels[rows[k].kernel].taps;
        rows[k].first_tile = tiles;
        rows[k].work_off = work;
        tiles += tiles_of(rows[k], taps, params->direct_max);
        work += work_of(rows[k], taps, params->direct_max);
    }
    if (work_floats) *work_floats = work;
    return tiles;
}

extern "C" double afg_convolve_bound(const afg_convolve_params *params, uint32_t taps)
{
    if (check_params(params, "afg_convolve_bound")) return -1.0;
    if (check_taps(taps, 0)) return -1.0;
    const double B_f = 8.0 * 11.0 + 8.0;                        // ceil(log2 2048) = 11
    return 6.0 * B_f + 2.0 * (double)parts_of(taps) + 11.0;
}

extern "C" int afg_convolve_check_rows(const afg_convolve_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_convolve_kernel *kernels,
                                       uint64_t n_kernels, const afg_convolve_params *params, uint64_t in_floats, uint64_t bank_floats,
                                       uint64_t spec_floats, uint64_t work_floats, uint64_t out_floats, const uint64_t *plane_at)
{
    if (int rc = check_params(params, "afg_convolve_check_rows")) return rc;
    if ((n_rows && !rows) || (n_kernels && !kernels)) { afg::set_error("afg_convolve_check_rows: NULL records"); return AFG_ERR_INVALID; }
    if (int rc = check_bank(kernels, n_kernels, bank_floats, spec_floats, "afg_convolve_check_rows")) return rc;
    if (n_rows == 0) return AFG_OK;
    try {
        return check_rows(rows, n_rows, n_tiles, kernels, n_kernels, *params, in_floats, bank_floats, spec_floats, work_floats, out_floats, plane_at);
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

extern "C" int afg_convolve_hip(uint64_t n_rows, const afg_convolve_row *d_rows, uint64_t n_tiles, const afg_convolve_kernel *d_kernels,
                                uint64_t n_kernels, const afg_convolve_params *params, const float *d_in, uint64_t in_floats, const float *d_bank,
                                uint64_t bank_floats, const float *d_spec, uint64_t spec_floats, float *d_work, uint64_t work_floats, float *d_out,
                                uint64_t out_floats, void *hip_stream)
{
    if (int rc = check_params(params, "afg_convolve_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!d_rows || !d_kernels || !d_in || !d_bank || !d_spec || !d_out || (work_floats && !d_work)) {
        afg::set_error("afg_convolve_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if ((((uintptr_t)d_in | (uintptr_t)d_bank | (uintptr_t)d_out) & 3u) != 0 || (((uintptr_t)d_spec | (uintptr_t)d_work | (uintptr_t)d_rows | (uintptr_t)d_kernels) & 7u) != 0) {
        afg::set_error("afg_convolve_hip: the input, bank and output planes must be 4-byte aligned, the spectra, the work plane and the records 8-byte");
        return AFG_ERR_INVALID;
    }
    if (n_kernels > 0xffffffffull) { afg::set_error("afg_convolve_hip: at most 2^32 - 1 kernels"); return AFG_ERR_INVALID; }
    if (int rc = afg::launch_caps("afg_convolve_hip", "rows", n_rows, n_tiles)) return rc;
    if (int rc = afg::require_device()) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const uint64_t plane_at[5] = { (uintptr_t)d_in >> 2, (uintptr_t)d_bank >> 2, (uintptr_t)d_spec >> 2, (uintptr_t)d_work >> 2, (uintptr_t)d_out >> 2 };
    uint64_t pairs = 0;
    bool direct = false, fft = false;
    if (int rc = afg::with_host_records(d_kernels, n_kernels, stream, [&](const afg_convolve_kernel *hk) {
            if (int rc2 = check_bank(hk, n_kernels, bank_floats, spec_floats, "afg_convolve_hip")) return rc2;
            return afg::with_host_records(d_rows, n_rows, stream, [&](const afg_convolve_row *h) {
                if (int rc3 = check_rows(h, n_rows, n_tiles, hk, n_kernels, *params, in_floats, bank_floats, spec_floats, work_floats, out_floats, plane_at))
                    return rc3;
                for (uint64_t k = 0; k < n_rows; k++) {
                    if (h[k].out_frames == 0) continue;
                    const uint32_t taps = hk[h[k].kernel].taps;
                    (is_direct(taps, params->direct_max) ? direct : fft) = true;
                    pairs += work_of(h[k], taps, params->direct_max) / kSpec;
                }
                return (int)AFG_OK;
            });
        }))
        return rc;
    if (n_tiles == 0) return AFG_OK;
    const FftGeo geo = fft_geo_of(kNfft);
    if (direct)
        hipLaunchKernelGGL(conv_direct_kernel, dim3((uint32_t)n_tiles), dim3(kDirectThreads), 0, stream, (uint32_t)n_rows, d_rows, d_kernels,
                           params->direct_max, d_in, d_bank, d_out);
    if (fft) {
        if (pairs)
            hipLaunchKernelGGL(conv_spectra_kernel, dim3((uint32_t)pairs), dim3(64), 0, stream, (uint32_t)n_rows, d_rows, d_kernels, params->direct_max, geo,
                               d_in, d_spec, d_work);
        hipLaunchKernelGGL(conv_blocks_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, stream, (uint32_t)n_rows, d_rows, d_kernels, params->direct_max, geo,
                           d_spec, d_work, d_out);
    }
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
