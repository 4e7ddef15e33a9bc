// fft_frame.h -- the device-side pieces of the per-frame mixed-radix FFT that melspec_fft.hip (afg_melspec_fft_hip),
// stft.hip (afg_stft_hip) and istft.hip (afg_istft_hip) share: the n_fft the transform takes, its pass list, the butterflies
// of radix 2, 3, 4 and 5, one Stockham autosort pass over a wavefront's LDS buffers, the wavefront-level ordering of that
// LDS traffic, one frame's run through the passes (fft_frame; fft_frame_complex for complex input) and a bin of the split
// pass, forwards and backwards (fft_split_bin, fft_unsplit_bin).  The kernels keep their own tiling, fetch and epilogue;
// what is here decides the bits of (re, im), and the two forward kernels get the same.
#pragma once
#include "afg_common.h"

namespace {

constexpr uint32_t kMaxPasses = 12;

struct FftGeo {
    uint32_t nc;                                                // length of the complex transform: n_fft / 2 (even) or n_fft
    uint32_t half;                                              // 1: n_fft even, the split pass follows
    uint32_t n_pass;
    uint32_t waves;                                             // wavefronts that transform (4, or fewer while LDS is short)
    uint32_t wbuf;                                              // floats of one wavefront's two buffers: 4 * nc
    uint32_t lds_floats;
    uint8_t radix[kMaxPasses];
};

bool n_fft_ok(uint32_t n)
{
    if (n < 16 || n > 2048) return false;
    for (uint32_t q : { 2u, 3u, 5u })
        while (n % q == 0) n /= q;
    return n == 1;
}

// the transform of an n_fft the path takes: its length, its passes and a wavefront's buffers (waves and lds_floats are the
// kernel's own choice)
FftGeo fft_geo_of(uint32_t n_fft)
{
    FftGeo g;
    std::memset(&g, 0, sizeof(g));
    g.half = (n_fft & 1) ? 0 : 1;
    g.nc = g.half ? n_fft / 2 : n_fft;
    uint32_t m = g.nc;
    for (uint32_t q : { 4u, 2u, 3u, 5u })
        while (m % q == 0 && g.n_pass < kMaxPasses) { g.radix[g.n_pass++] = (uint8_t)q; m /= q; }
    g.wbuf = 4 * g.nc;
    return g;
}

struct cf { float re, im; };
__device__ inline cf operator+(cf a, cf b) { return { a.re + b.re, a.im + b.im }; }
__device__ inline cf operator-(cf a, cf b) { return { a.re - b.re, a.im - b.im }; }
__device__ inline cf cmul(cf a, cf b) { return { a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re }; }
__device__ inline cf scale(cf a, float s) { return { a.re * s, a.im * s }; }
__device__ inline cf mul_mi(cf a) { return { a.im, -a.re }; }   // a * -i

// the DFT of R values, forward (e^{-2 pi i / R})
template <int R> __device__ inline void butterfly(cf *v);
template <> __device__ inline void butterfly<2>(cf *v)
{
    const cf a = v[0] + v[1], b = v[0] - v[1];
    v[0] = a; v[1] = b;
}
template <> __device__ inline void butterfly<4>(cf *v)
{
    const cf t0 = v[0] + v[2], t1 = v[0] - v[2], t2 = v[1] + v[3], t3 = mul_mi(v[1] - v[3]);
    v[0] = t0 + t2; v[1] = t1 + t3; v[2] = t0 - t2; v[3] = t1 - t3;
}
template <> __device__ inline void butterfly<3>(cf *v)
{
    const cf t = v[1] + v[2], m = v[0] - scale(t, 0.5f), s = mul_mi(scale(v[1] - v[2], 0.86602540378443864676f));
    v[0] = v[0] + t; v[1] = m + s; v[2] = m - s;
}
template <> __device__ inline void butterfly<5>(cf *v)
{
    constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f, s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
    const cf t1 = v[1] + v[4], t2 = v[2] + v[3], t3 = v[1] - v[4], t4 = v[2] - v[3];
    const cf a1 = v[0] + (scale(t1, c1) + scale(t2, c2)), a2 = v[0] + (scale(t1, c2) + scale(t2, c1));
    const cf b1 = mul_mi(scale(t3, s1) + scale(t4, s2)), b2 = mul_mi(scale(t3, s2) - scale(t4, s1));
    v[0] = v[0] + (t1 + t2); v[1] = a1 + b1; v[2] = a2 + b2; v[3] = a2 - b2; v[4] = a1 - b1;
}

// One Stockham pass of radix R over nc values: butterfly j takes src[j + r * nc / R], turned by e^{-2 pi i r k / (ns R)} with
// k = j mod ns, and leaves dst[(j - k) R + k + r ns].  tw is the table of n_fft pairs; ns R divides nc, which divides n_fft.
template <int R>
__device__ inline void fft_pass(const float *__restrict__ sr, const float *__restrict__ si, float *__restrict__ dr, float *__restrict__ di,
                                uint32_t nc, uint32_t ns, uint32_t n_fft, const float *__restrict__ tw, uint32_t lane)
{
    const uint32_t m = nc / R, tstep = n_fft / (ns * R);
    const bool pow2 = (ns & (ns - 1)) == 0;
    for (uint32_t j = lane; j < m; j += 64) {
        const uint32_t k = pow2 ? (j & (ns - 1)) : j % ns;
        cf v[R];
#pragma unroll
        for (int r = 0; r < R; r++) v[r] = { sr[j + r * m], si[j + r * m] };
        if (ns > 1) {
#pragma unroll
            for (int r = 1; r < R; r++) {
                const uint32_t t = 2 * (r * k * tstep);         // r k < R ns: inside the table
                v[r] = cmul(v[r], cf{ tw[t], tw[t + 1] });
            }
        }
        butterfly<R>(v);
        const uint32_t j0 = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; r++) { dr[j0 + r * ns] = v[r].re; di[j0 + r * ns] = v[r].im; }
    }
}

// a wavefront's LDS traffic in program order: what one pass wrote, the next reads in other lanes
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The passes over a wavefront's filled buffers `buf` (4 nc floats; planes 0 and 1 hold the input, the wavefront has synchronised
// behind the fill): leaves the planes of the result in *zr, *zi (inside buf: the first pair after an even number of passes).
__device__ inline void fft_passes(const FftGeo &geo, uint32_t n_fft, float *buf, const float *__restrict__ tw, uint32_t lane, const float **zr,
                                  const float **zi)
{
    const uint32_t nc = geo.nc;
    float *sr = buf, *si = buf + nc, *dr = buf + 2 * nc, *di = buf + 3 * nc;
    uint32_t ns = 1;
    for (uint32_t p = 0; p < geo.n_pass; p++) {
        const uint32_t R = geo.radix[p];
        switch (R) {
        case 4: fft_pass<4>(sr, si, dr, di, nc, ns, n_fft, tw, lane); break;
        case 2: fft_pass<2>(sr, si, dr, di, nc, ns, n_fft, tw, lane); break;
        case 3: fft_pass<3>(sr, si, dr, di, nc, ns, n_fft, tw, lane); break;
        default: fft_pass<5>(sr, si, dr, di, nc, ns, n_fft, tw, lane); break;
        }
        ns *= R;
        float *t = sr; sr = dr; dr = t;
        t = si; si = di; di = t;
        wave_sync();
    }
    *zr = sr; *zi = si;
}

// One frame through the transform, by one wavefront in its own buffers `buf` (4 nc floats): fetch(i) is sample i of the frame
// times its window value; an even n_fft packs z[j] = x[2j] + i x[2j+1] into half the length (the caller's split pass follows),
// an odd n_fft runs the full length with a zero imaginary part.  Leaves the planes of the result in *zr, *zi (inside buf).
template <typename Fetch>
__device__ inline void fft_frame(const FftGeo &geo, uint32_t n_fft, float *buf, const float *__restrict__ tw, uint32_t lane, Fetch fetch,
                                 const float **zr, const float **zi)
{
    const uint32_t nc = geo.nc;
    float *sr = buf, *si = buf + nc;
    wave_sync();                                                 // the frame before has read its result
    if (geo.half)
        for (uint32_t j = lane; j < nc; j += 64) { sr[j] = fetch(2 * j); si[j] = fetch(2 * j + 1); }
    else
        for (uint32_t j = lane; j < nc; j += 64) { sr[j] = fetch(j); si[j] = 0.0f; }
    wave_sync();
    fft_passes(geo, n_fft, buf, tw, lane, zr, zi);
}

// The complex transform of length nc alone, for a caller with complex input (istft.hip): fetch(j) is value j, j < nc.
template <typename Fetch>
__device__ inline void fft_frame_complex(const FftGeo &geo, uint32_t n_fft, float *buf, const float *__restrict__ tw, uint32_t lane, Fetch fetch,
                                         const float **zr, const float **zi)
{
    const uint32_t nc = geo.nc;
    float *sr = buf, *si = buf + nc;
    wave_sync();
    for (uint32_t j = lane; j < nc; j += 64) { const cf v = fetch(j); sr[j] = v.re; si[j] = v.im; }
    wave_sync();
    fft_passes(geo, n_fft, buf, tw, lane, zr, zi);
}

// bin k of an even n_fft from the half-length result Z (the split pass): X[k] = E + W^k O with E = (Z[k] + conj Z[nc - k]) / 2,
// O = -i (Z[k] - conj Z[nc - k]) / 2, W = e^{-2 pi i / n_fft}; k = 0 .. nc
__device__ inline cf fft_split_bin(const float *zr, const float *zi, uint32_t nc, uint32_t k, const float *__restrict__ tw)
{
    const uint32_t k1 = k == nc ? 0 : k, k2 = k == 0 ? 0 : nc - k;
    const float a = zr[k1], b = zi[k1], c = zr[k2], d = zi[k2];
    const cf E = { 0.5f * (a + c), 0.5f * (b - d) }, O = { 0.5f * (b + d), -0.5f * (a - c) };
    return E + cmul(cf{ tw[2 * k], tw[2 * k + 1] }, O);
}

// the split pass backwards: Z[k], k = 1 .. nc - 1, of the half-length transform from X[k] = (a, b) and X[nc - k] = (c, d) of an
// even n_fft, times s: E = s (X[k] + conj X[nc - k]), O = conj(W^k) s (X[k] - conj X[nc - k]), Z = E + i O.  (Z[0] comes from
// the two real-only bins and is the caller's: s (re_0 + re_nc) + i s (re_0 - re_nc).)
__device__ inline cf fft_unsplit_bin(cf Xk, cf Xm, float s, uint32_t k, const float *__restrict__ tw)
{
    const cf E = { s * (Xk.re + Xm.re), s * (Xk.im - Xm.im) };
    const cf O = cmul(cf{ tw[2 * k], -tw[2 * k + 1] }, cf{ s * (Xk.re - Xm.re), s * (Xk.im + Xm.im) });
    return { E.re - O.im, E.im + O.re };
}

}  // namespace
