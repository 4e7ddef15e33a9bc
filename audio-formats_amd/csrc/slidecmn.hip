// slidecmn.hip -- sliding-window cepstral mean (and variance) normalisation of feature slabs, Kaldi's window
// (afg_slide_cmn_hip, afg_batch_decode_fbank_cmn), for gfx950.  The definition -- the window of a frame, the order of the
// float64 sums over chunks of 32 frames, the output -- is in include/afg.h and again in tests/slidecmn_model.py.  The Makefile
// builds this file with -ffp-contract=off like every other exact-mode kernel: var = S2 / n - mean * mean and (x - mean) *
// (1 / sqrt(var)) are a product and a sum each, never a fused multiply-add.  The host half (layout, record checks, the batch
// entry) is host/afg_slidecmn.cpp.
//
// A tile is one chunk: AFG_CMN_CHUNK = 32 frames of one slab, all of its columns.  Two launches on the caller's stream, no
// atomics:
//   scan     one workgroup of 256 lanes per tile.  It reads the tile once, coalesced in the slab's own layout (lanes along
//            columns frames-major, along frames col-major), writes it compact into the workspace in the same orientation, and
//            through LDS (row c at c * 33: no bank is met twice by the lanes of a column group) gives every column to one lane,
//            which forms the chunk's totals of x and x * x ascending and stores them as one 16-byte pair.
//   apply    the same tiles.  A lane per element (t, c): the window of t; the descending sum from the end of ws's chunk down to
//            ws, the totals of the chunks between, the ascending sum up to we - 1 -- all read from the workspace copy, where
//            lanes that are neighbours in the slab are neighbours again -- and one store of the result.
// Why the copy: the window of a frame reaches into other tiles, so in place a tile would read frames another tile has already
// overwritten.  With the copy nothing but the scan reads d_in, every scan has ended when the first apply starts (stream
// order), and in place and out of place run the same code and give the same bits.  The price is one more write and the
// workspace: 144 bytes per column and tile (afg_cmn_work_bytes).
//
// Bounds: every slab is checked on the host before the launch (afg_cmn_check_slabs); the kernels rely on it.  They read
// in[in_off + ...] and write out[out_off + ...] for t < n_frames and c < cols only; of the workspace the totals
// [0, n_tiles * cols) and the copy [0, n_tiles * cols * 32) behind them, a short last chunk leaving the rest of its 32 * cols
// floats unwritten and unread (0 <= ws < we <= n_frames for every frame).
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kChunk = AFG_CMN_CHUNK;
constexpr uint32_t kColGroup = 256;                              // columns per pass of the scan
constexpr uint32_t kRowPad = kChunk + 1;

static_assert(sizeof(afg_cmn_slab) == 48 && sizeof(afg_cmn_params) == 32, "include/afg.h");
static_assert(kChunk == 32, "the chunk index of a frame is f >> 5");

struct Tot { double s, q; };                                     // a chunk's totals of one column
static_assert(sizeof(Tot) == 16, "a pair of totals is 16 bytes");

// a NaN result is the positive quiet NaN, whichever NaN the hardware made of its operands (include/afg.h)
__device__ __forceinline__ float one_nan(float v) { return v == v ? v : __uint_as_float(0x7fc00000u); }

// The tile `tile` of the launch: its slab and its first frame.  False: no slab has it (never, behind the checks).
__device__ __forceinline__ bool find_tile(uint32_t n_slabs, const afg_cmn_slab *__restrict__ slabs, uint64_t tile, afg_cmn_slab *s, uint32_t *t0,
                                          uint32_t *nf)
{
    const uint32_t lo = afg::last_at_or_before(slabs, n_slabs, tile, &afg_cmn_slab::first_tile);   // (slabs without frames have no tiles)
    *s = slabs[lo];
    if (s->first_tile > tile || s->n_frames == 0) return false;
    const uint64_t local = tile - s->first_tile;
    if (local >= ((uint64_t)s->n_frames + kChunk - 1) / kChunk) return false;
    *t0 = (uint32_t)local * kChunk;
    *nf = min(kChunk, s->n_frames - *t0);
    return true;
}

// Element e of a tile piece of w columns and nf frames, in the order that is contiguous in memory: (j, c) = (e / w, e % w)
// frames-major, (e % nf, e / nf) col-major.  One division per lane, then steps of kThreads.
struct Walk {
    uint32_t q, r, dq, dr, m;
    __device__ __forceinline__ Walk(uint32_t e, uint32_t modulus) : q(e / modulus), r(e % modulus), dq(kThreads / modulus), dr(kThreads % modulus), m(modulus) {}
    __device__ __forceinline__ void step()
    {
        q += dq; r += dr;
        if (r >= m) { r -= m; q++; }
    }
};

template <bool kColMajor>
__global__ __launch_bounds__(kThreads) void cmn_scan_kernel(uint32_t n_slabs, const afg_cmn_slab *__restrict__ slabs, uint32_t cols,
                                                            const float *__restrict__ in, Tot *__restrict__ tot, float *__restrict__ copy)
{
    __shared__ float sh[kColGroup * kRowPad];
    const uint64_t tile = blockIdx.x;
    afg_cmn_slab s;
    uint32_t t0, nf;
    if (!find_tile(n_slabs, slabs, tile, &s, &t0, &nf)) return;
    const float *p = in + s.in_off;
    float *cp = copy + tile * ((uint64_t)kChunk * cols);
    const uint32_t lane = threadIdx.x;
    for (uint32_t c0 = 0; c0 < cols; c0 += kColGroup) {
        const uint32_t w = min(kColGroup, cols - c0), n = w * nf;
        Walk k(lane, kColMajor ? nf : w);
        for (uint32_t e = lane; e < n; e += kThreads, k.step()) {
            const uint32_t j = kColMajor ? k.r : k.q, c = kColMajor ? k.q : k.r;
            const float x = kColMajor ? p[(uint64_t)(c0 + c) * s.pitch + t0 + j] : p[(uint64_t)(t0 + j) * s.pitch + c0 + c];
            cp[kColMajor ? (c0 + c) * kChunk + j : j * cols + c0 + c] = x;
            sh[c * kRowPad + j] = x;
        }
        __syncthreads();
        if (lane < w) {
            double a = 0.0, b = 0.0;
            for (uint32_t j = 0; j < nf; j++) {
                const double d = (double)sh[lane * kRowPad + j];
                a = a + d;
                b = b + d * d;
            }
            tot[tile * cols + c0 + lane] = Tot{ a, b };
        }
        __syncthreads();
    }
}

// frame f, column c of the slab whose first tile is `first`, in the workspace copy
template <bool kColMajor> __device__ __forceinline__ float copy_at(const float *__restrict__ copy, uint64_t first, uint32_t cols, uint32_t f, uint32_t c)
{
    if (kColMajor) return copy[(first + (f >> 5)) * ((uint64_t)kChunk * cols) + c * kChunk + (f & 31u)];
    return copy[first * ((uint64_t)kChunk * cols) + (uint64_t)f * cols + c];
}

template <bool kColMajor>
__global__ __launch_bounds__(kThreads) void cmn_apply_kernel(uint32_t n_slabs, const afg_cmn_slab *__restrict__ slabs, afg_cmn_params prm,
                                                             const Tot *__restrict__ tot, const float *__restrict__ copy, float *__restrict__ out)
{
    const uint64_t tile = blockIdx.x;
    afg_cmn_slab s;
    uint32_t t0, nf;
    if (!find_tile(n_slabs, slabs, tile, &s, &t0, &nf)) return;
    const uint32_t cols = prm.cols, n = nf * cols;
    const int64_t N = (int64_t)s.n_frames, W = (int64_t)prm.cmn_window;
    float *y = out + s.out_off;
    Walk k(threadIdx.x, kColMajor ? nf : cols);
    for (uint32_t e = threadIdx.x; e < n; e += kThreads, k.step()) {
        const uint32_t j = kColMajor ? k.r : k.q, c = kColMajor ? k.q : k.r;
        const int64_t t = (int64_t)t0 + j;
        // the window of frame t (include/afg.h): Kaldi's SlidingWindowCmnInternal
        int64_t ws = prm.center ? t - W / 2 : t - W, we = prm.center ? ws + W : t + 1;
        if (ws < 0) { we -= ws; ws = 0; }
        if (!prm.center && we > t) we = t + 1 > (int64_t)prm.min_cmn_window ? t + 1 : (int64_t)prm.min_cmn_window;
        if (we > N) { ws -= we - N; we = N; ws = ws > 0 ? ws : 0; }
        const uint32_t a = (uint32_t)ws, b = (uint32_t)we - 1u;      // first and last frame, 0 <= a <= b < N
        double s1 = 0.0, s2 = 0.0;
        if ((a >> 5) == (b >> 5)) {
            for (uint32_t f = a; f <= b; f++) {
                const double d = (double)copy_at<kColMajor>(copy, s.first_tile, cols, f, c);
                s1 = s1 + d;
                s2 = s2 + d * d;
            }
        } else {
            const uint32_t last = min((a | 31u), (uint32_t)(N - 1));   // (the chunk of a is whole: b lies behind it)
            for (uint32_t f = last + 1; f-- > a;) {
                const double d = (double)copy_at<kColMajor>(copy, s.first_tile, cols, f, c);
                s1 = s1 + d;
                s2 = s2 + d * d;
            }
            for (uint32_t ch = (a >> 5) + 1; ch < (b >> 5); ch++) {
                const Tot v = tot[(s.first_tile + ch) * cols + c];
                s1 = s1 + v.s;
                s2 = s2 + v.q;
            }
            double p1 = 0.0, p2 = 0.0;
            for (uint32_t f = b & ~31u; f <= b; f++) {
                const double d = (double)copy_at<kColMajor>(copy, s.first_tile, cols, f, c);
                p1 = p1 + d;
                p2 = p2 + d * d;
            }
            s1 = s1 + p1;
            s2 = s2 + p2;
        }
        const double x = (double)copy_at<kColMajor>(copy, s.first_tile, cols, (uint32_t)t, c);
        const double cnt = (double)(we - ws), mean = s1 / cnt;
        float r;
        if (!prm.norm_vars) {
            r = (float)(x - mean);
        } else if (we - ws == 1) {
            r = 0.0f;
        } else {
            const double m2 = s2 / cnt, mm = mean * mean;
            double var = m2 - mm;
            var = var < 1e-10 ? 1e-10 : var;                     // Kaldi's floor; a NaN stays
            const double d = x - mean, rs = 1.0 / sqrt(var);
            r = (float)(d * rs);
        }
        y[kColMajor ? (uint64_t)c * s.pitch + (uint64_t)t : (uint64_t)t * s.pitch + c] = one_nan(r);
    }
}

int check_args(uint64_t n_slabs, const afg_cmn_slab *d_slabs, uint64_t n_tiles, const afg_cmn_params *params, const float *d_in, float *d_out,
               void *d_work, uint64_t work_bytes)
{
    if (!params) {
        afg::set_error("afg_slide_cmn_hip: NULL params");
        return AFG_ERR_INVALID;
    }
    if (!d_slabs || (n_tiles && (!d_in || !d_out || !d_work))) {
        afg::set_error("afg_slide_cmn_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || ((uintptr_t)d_work & 15u) != 0 || ((uintptr_t)d_slabs & 7u) != 0) {
        afg::set_error("afg_slide_cmn_hip: the planes must be 4-byte aligned, the records 8-byte and the workspace 16-byte aligned");
        return AFG_ERR_INVALID;
    }
    if (int rc = afg::launch_caps("afg_slide_cmn_hip", "slabs", n_slabs, n_tiles)) return rc;
    if (int rc = afg_cmn_check_slabs(nullptr, 0, 0, params, 0, 0, 0)) return rc;                  // the parameters: cols enters the size
    const uint64_t need = afg_cmn_work_bytes(n_tiles, params->cols);
    if (work_bytes < need) {
        afg::set_error("afg_slide_cmn_hip: a workspace of %llu bytes, afg_cmn_work_bytes gives %llu", (unsigned long long)work_bytes,
                       (unsigned long long)need);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

}  // namespace

int afg::slide_cmn_launch(const afg_cmn_slab *h_slabs, uint64_t n_slabs, const afg_cmn_slab *d_slabs, uint64_t n_tiles, const afg_cmn_params *params,
                          const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, void *d_work, uint64_t work_bytes,
                          hipStream_t stream)
{
    if (n_slabs == 0) return AFG_OK;
    if (int rc = check_args(n_slabs, d_slabs, n_tiles, params, d_in, d_out, d_work, work_bytes)) return rc;
    if (int rc = afg_cmn_check_slabs(h_slabs, n_slabs, n_tiles, params, in_floats, out_floats, d_in == d_out ? 1 : 0)) return rc;
    if (int rc = afg::require_device()) return rc;
    if (n_tiles == 0) return AFG_OK;
    const uint32_t ns = (uint32_t)n_slabs, cols = params->cols;
    Tot *tot = (Tot *)d_work;
    float *copy = (float *)(tot + n_tiles * cols);
    const dim3 grid((uint32_t)n_tiles), block(kThreads);
    if (params->layout == AFG_CMN_COL_MAJOR) {
        hipLaunchKernelGGL(cmn_scan_kernel<true>, grid, block, 0, stream, ns, d_slabs, cols, d_in, tot, copy);
        hipLaunchKernelGGL(cmn_apply_kernel<true>, grid, block, 0, stream, ns, d_slabs, *params, (const Tot *)tot, (const float *)copy, d_out);
    } else {
        hipLaunchKernelGGL(cmn_scan_kernel<false>, grid, block, 0, stream, ns, d_slabs, cols, d_in, tot, copy);
        hipLaunchKernelGGL(cmn_apply_kernel<false>, grid, block, 0, stream, ns, d_slabs, *params, (const Tot *)tot, (const float *)copy, d_out);
    }
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_slide_cmn_hip(uint64_t n_slabs, const afg_cmn_slab *d_slabs, uint64_t n_tiles, const afg_cmn_params *params, const float *d_in,
                                 uint64_t in_floats, float *d_out, uint64_t out_floats, void *d_work, uint64_t work_bytes, void *hip_stream)
{
    if (n_slabs == 0) return AFG_OK;
    if (int rc = check_args(n_slabs, d_slabs, n_tiles, params, d_in, d_out, d_work, work_bytes)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_slabs, n_slabs, (hipStream_t)hip_stream, [&](const afg_cmn_slab *h) {
        return afg::slide_cmn_launch(h, n_slabs, d_slabs, n_tiles, params, d_in, in_floats, d_out, out_floats, d_work, work_bytes,
                                     (hipStream_t)hip_stream);
    });
}
