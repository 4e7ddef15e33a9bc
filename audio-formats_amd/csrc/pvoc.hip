// pvoc.hip -- the phase-vocoder time stretch (afg_pvoc_hip), for gfx950: from one AFG_STFT_COMPLEX slab ([n_bins, frames]
// pairs, frames contiguous) to another with out_frames = the steps t with fl(t * rate) < n_frames, torchaudio's
// phase_vocoder as include/afg.h writes it out, with the interval the result is held to and the constants K_A and K_P.
//
// One launch, no atomics, nothing that waits for another workgroup or wavefront.  A (slab, bin) pair is one row, and one
// wavefront walks its row from the first step to the last in tiles of kTile = 256 steps; a workgroup is four wavefronts on
// four neighbouring bins of one slab, which share nothing and meet at no barrier.  All phases are kept in turns (radians
// over 2 pi): x - rint(x) is then the wrap and it is exact, and sincospi takes the reduced phase.  Per tile:
//   stage    the frames the tile's steps read go through atan2 and sqrt once, in float64, into the wavefront's own LDS as
//            (angle in turns, magnitude): for rate <= 1 the contiguous run i_first .. i_last + 1 (at most kTile + 2 frames,
//            lanes along frames, 512 bytes a load), each frame serving its 1 / rate steps; for rate > 1 the pair i_t, i_t + 1
//            of every step (slot 2 (t - t0) and the one behind it), so that in both cases step t finds its pair in slots
//            a and a + 1.  Frame n_frames is (+0, +0) and is not read.
//   chunk    lane l takes the kChunk = 4 consecutive steps t0 + 4 l ..: d = th[a + 1] - th[a] - w, p = d - rint(d), with
//            w = centred((hop k) mod n_fft) / n_fft -- the bin's advance modulo one turn -- and sums them from 0.
//   scan     the chunk totals meet in a log-step inclusive scan over the wavefront (six shuffles; a lane below the step
//            keeps its value, so nothing flows downwards and a NaN reaches only what lies behind it); the carry, reduced
//            by rint at every tile, passes from tile to tile in a register.  It starts as frame 0's angle.
//   phase    ph_t = carry + lanes below + steps below in the chunk + centred((hop k t) mod n_fft) / n_fft: the advance's
//            share t w_k is kept in 32-bit integers modulo n_fft and is exact but for its one division by n_fft.
//   store    (float)(m cos), (float)(m sin) with m = a |X_{i+1}| + (1 - a) |X_i| in float64: the one float32 rounding.  A
//            lane's four pairs are 32 contiguous bytes and go out as two dwordx4 at dword alignment (dwordx2 at a row's end).
// s_t = t * rate is one IEEE double product (__dmul_rn: never fused, whatever -ffp-contract says), as the definition has it.
//
// Bounds: every record is checked on the host before the launch (check_rows below); the kernel relies on it.  It reads
// in[in_off + 2 (k in_pitch + f)] and the float behind it for k < n_bins, f < n_frames only and writes
// out[out_off + 2 (k out_pitch + t)] and the float behind it for t < out_frames only.  LDS slots are clamped to the array.
#include "afg_records.h"

#include <cmath>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = 4, kChunk = AFG_PVOC_CHUNK, kTile = AFG_PVOC_TILE, kSlots = 2 * kTile + 2;
constexpr double kInv2Pi = 0.15915494309189533576888376337251436;

static_assert(kTile == 64 * kChunk && kChunk == 4, "include/afg.h");
static_assert(sizeof(afg_pvoc_params) == 32 && sizeof(afg_pvoc_row) == 48, "include/afg.h");

typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));     // a dwordx2 at dword alignment
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a dwordx4 at dword alignment

struct Slot { double th, mag; };                                 // a frame's angle in turns and its magnitude

__device__ __forceinline__ uint32_t step_frame(uint32_t t, double rate) { return (uint32_t)floor(__dmul_rn((double)t, rate)); }

__global__ __launch_bounds__(kThreads) void pvoc_kernel(const afg_pvoc_row *__restrict__ rows, uint32_t n_fft, uint32_t hop, uint32_t groups,
                                                        const float *__restrict__ in, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) Slot sh[kWaves][kSlots];
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t slab = blockIdx.x / groups, k = (blockIdx.x % groups) * kWaves + wave, n_bins = n_fft / 2 + 1;
    if (k >= n_bins) return;
    const afg_pvoc_row r = rows[slab];
    if (r.out_frames == 0) return;
    Slot *const S = sh[wave];
    const float *const x = in + r.in_off + 2 * (uint64_t)k * r.in_pitch;
    float *const y = out + r.out_off + 2 * (uint64_t)k * r.out_pitch;
    const double rate = r.rate, inv_n = 1.0 / (double)n_fft;
    const bool run = rate <= 1.0;                                // the tile's frames are one contiguous run
    // the bin's advance per step, modulo one turn: hop * k < 2^31, everything below stays under 2^32
    const uint32_t adv = (hop * k) % n_fft;
    const double w = (double)(2 * adv > n_fft ? (int32_t)adv - (int32_t)n_fft : (int32_t)adv) / (double)n_fft;
    const uint32_t q_lane = (adv * (lane * kChunk)) % n_fft, q_step = (adv * kTile) % n_fft;
    uint32_t q_tile = 0;                                         // (hop k t0) mod n_fft
    double carry = atan2((double)x[1], (double)x[0]) * kInv2Pi;  // th_0 (n_frames >= 1)

    for (uint32_t t0 = 0; t0 < r.out_frames; t0 += kTile) {
        const uint32_t nt = min(kTile, r.out_frames - t0);
        // ---- stage
        const uint32_t f_lo = run ? step_frame(t0, rate) : 0;
        const uint32_t ns = run ? min(step_frame(t0 + nt - 1, rate) + 2 - f_lo, kSlots) : 2 * nt;
        for (uint32_t s = lane; s < ns; s += 64) {
            const uint32_t f = run ? f_lo + s : step_frame(t0 + (s >> 1), rate) + (s & 1u);
            float re = 0.0f, im = 0.0f;
            if (f < r.n_frames) {
                const f32x2u v = *(const f32x2u *)(x + 2 * (uint64_t)f);
                re = v.x; im = v.y;
            }
            const double dr = (double)re, di = (double)im;
            S[s].th = atan2(di, dr) * kInv2Pi;
            S[s].mag = sqrt(dr * dr + di * di);
        }
        // the wavefront's LDS operations complete in order; this keeps the compiler from moving the reads up
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- chunk
        double p[kChunk], m[kChunk];
#pragma unroll
        for (uint32_t j = 0; j < kChunk; j++) {
            const uint32_t e = lane * kChunk + j;
            p[j] = 0.0; m[j] = 0.0;
            if (e < nt) {
                const double st = __dmul_rn((double)(t0 + e), rate), fl = floor(st), a = st - fl;      // a: exact
                const uint32_t slot = min(run ? (uint32_t)fl - f_lo : 2 * e, kSlots - 2);
                const Slot A = S[slot], B = S[slot + 1];
                const double d = (B.th - A.th) - w;
                p[j] = d - rint(d);
                m[j] = a * B.mag + (1.0 - a) * A.mag;
            }
        }
        // ---- scan: the steps below in the chunk, the lanes below in the wavefront
        const double pre1 = p[0], pre2 = pre1 + p[1], pre3 = pre2 + p[2];
        double inc = pre3 + p[3];
#pragma unroll
        for (int b = 0; b < 6; b++) {
            const uint32_t d = 1u << b;
            const double below = __shfl_up(inc, d);
            if (lane >= d) inc += below;
        }
        double excl = __shfl_up(inc, 1);
        if (lane == 0) excl = 0.0;
        const double total = __shfl(inc, 63);
        const double base = carry + excl;
        // ---- phase and store
        uint32_t q = q_tile + q_lane;
        if (q >= n_fft) q -= n_fft;
        float o[2 * kChunk];
#pragma unroll
        for (uint32_t j = 0; j < kChunk; j++) {
            const double pre = j == 0 ? 0.0 : j == 1 ? pre1 : j == 2 ? pre2 : pre3;
            const double wq = (double)(2 * q > n_fft ? (int32_t)q - (int32_t)n_fft : (int32_t)q) * inv_n;
            double ph = (base + pre) + wq;
            ph -= rint(ph);
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            o[2 * j] = (float)(m[j] * cs);
            o[2 * j + 1] = (float)(m[j] * sn);
            q += adv;
            if (q >= n_fft) q -= n_fft;
        }
        const uint32_t e0 = lane * kChunk;
        float *const yt = y + 2 * (uint64_t)(t0 + e0);
        if (e0 + kChunk <= nt) {
            *(f32x4u *)yt = f32x4u{ o[0], o[1], o[2], o[3] };
            *(f32x4u *)(yt + 4) = f32x4u{ o[4], o[5], o[6], o[7] };
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kChunk; j++)
                if (e0 + j < nt) *(f32x2u *)(yt + 2 * j) = f32x2u{ o[2 * j], o[2 * j + 1] };
        }
        // ---- to the next tile (the reads above are done before the next stage writes: in order, and fenced)
        carry += total;
        carry -= rint(carry);
        q_tile += q_step;
        if (q_tile >= n_fft) q_tile -= n_fft;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

int check_params(const afg_pvoc_params *p, const char *who)
{
    if (!p) { afg::set_error("%s: NULL params", who); return AFG_ERR_INVALID; }
    if (p->n_fft < 2 || p->n_fft > 65536) { afg::set_error("afg_pvoc_params.n_fft %u: 2 .. 65536", p->n_fft); return AFG_ERR_INVALID; }
    if (p->hop < 1 || p->hop > p->n_fft) { afg::set_error("afg_pvoc_params.hop %u: 1 .. n_fft (%u)", p->hop, p->n_fft); return AFG_ERR_INVALID; }
    for (uint32_t v : p->reserved)
        if (v != 0) { afg::set_error("afg_pvoc_params.reserved: must be 0"); return AFG_ERR_INVALID; }
    return AFG_OK;
}

bool rate_ok(double rate) { return rate >= 1.0 / 64 && rate <= 64.0; }      // (false for a NaN)

// the number of t >= 0 with fl(t * rate) < n_frames (n_frames 1 .. 2^24, rate in range): at most 2^30.  The product is one
// rounded double multiplication here as on the device (the host objects are built with -ffp-contract=off, and a lone
// product has nothing to fuse with).
uint32_t out_frames_of(uint32_t n_frames, double rate)
{
    const double n = (double)n_frames;
    uint64_t c = (uint64_t)std::ceil(n / rate);
    auto pos = [&](uint64_t t) { volatile double s = (double)t * rate; return (double)s; };
    while (c > 0 && pos(c - 1) >= n) c--;
    while (pos(c) < n) c++;
    return (uint32_t)c;
}

// every record against the planes, before anything runs
int check_rows(const afg_pvoc_row *rows, uint64_t n_rows, const afg_pvoc_params &p, uint64_t in_floats, uint64_t out_floats)
{
    const uint64_t n_bins = p.n_fft / 2 + 1;
    for (uint64_t k = 0; k < n_rows; k++) {
        const afg_pvoc_row &r = rows[k];
        const unsigned long long kk = (unsigned long long)k;
        if (r.reserved[0] != 0 || r.reserved[1] != 0) { afg::set_error("afg_pvoc_hip: row %llu: reserved words must be 0", kk); return AFG_ERR_INVALID; }
        if (!rate_ok(r.rate)) { afg::set_error("afg_pvoc_hip: row %llu: rate %g: finite, 1/64 .. 64", kk, r.rate); return AFG_ERR_INVALID; }
        if (r.out_frames == 0) continue;                         // nothing read, nothing written
        if (r.n_frames < 1 || r.n_frames > (1u << 24)) { afg::set_error("afg_pvoc_hip: row %llu: n_frames %u: 1 .. 2^24", kk, r.n_frames); return AFG_ERR_INVALID; }
        if (r.n_frames > r.in_pitch) { afg::set_error("afg_pvoc_hip: row %llu: n_frames %u above in_pitch %u", kk, r.n_frames, r.in_pitch); return AFG_ERR_INVALID; }
        const uint32_t want = out_frames_of(r.n_frames, r.rate);
        if (r.out_frames != want) {
            afg::set_error("afg_pvoc_hip: row %llu: out_frames %u, afg_pvoc_out_frames gives %u (or 0 for none)", kk, r.out_frames, want);
            return AFG_ERR_INVALID;
        }
        if (r.out_frames > r.out_pitch) { afg::set_error("afg_pvoc_hip: row %llu: out_frames %u above out_pitch %u", kk, r.out_frames, r.out_pitch); return AFG_ERR_INVALID; }
        const uint64_t need = 2 * ((n_bins - 1) * r.in_pitch + r.n_frames), make = 2 * ((n_bins - 1) * r.out_pitch + r.out_frames);      // < 2^49
        if (!afg::rows_inside(r.in_off, 1, 0, need, in_floats)) {
            afg::set_error("afg_pvoc_hip: row %llu: the slab's %llu floats leave the input (%llu floats)", kk, (unsigned long long)need, (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        if (!afg::rows_inside(r.out_off, 1, 0, make, out_floats)) {
            afg::set_error("afg_pvoc_hip: row %llu: the slab's %llu floats leave the output (%llu floats)", kk, (unsigned long long)make, (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
    }
    return AFG_OK;
}

// what can be said without the rows
int check_args(uint64_t n_rows, const afg_pvoc_row *d_rows, const afg_pvoc_params &p, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats)
{
    if (!d_rows || !d_in || !d_out) { afg::set_error("afg_pvoc_hip: NULL device pointer"); return AFG_ERR_INVALID; }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || ((uintptr_t)d_rows & 7u) != 0) {
        afg::set_error("afg_pvoc_hip: the planes must be 4-byte aligned, the rows 8-byte aligned");
        return AFG_ERR_INVALID;
    }
    const uint64_t groups = ((uint64_t)p.n_fft / 2 + 1 + kWaves - 1) / kWaves;
    if (n_rows > 0x7fffffffull / groups) {
        afg::set_error("afg_pvoc_hip: at most %llu rows of %u bins per launch", (unsigned long long)(0x7fffffffull / groups), p.n_fft / 2 + 1);
        return AFG_ERR_INVALID;
    }
    if (in_floats > (~(uint64_t)0 >> 3) || out_floats > (~(uint64_t)0 >> 3)) { afg::set_error("afg_pvoc_hip: a plane of 2^61 floats or more"); return AFG_ERR_INVALID; }
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + in_floats * 4, b0 = (uintptr_t)d_out, b1 = b0 + out_floats * 4;
    if (in_floats && out_floats && a0 < b1 && b0 < a1) { afg::set_error("afg_pvoc_hip: the output plane overlaps the input plane"); return AFG_ERR_INVALID; }
    return AFG_OK;
}

}  // namespace

extern "C" uint32_t afg_pvoc_out_frames(uint32_t n_frames, double rate)
{
    if (n_frames < 1 || n_frames > (1u << 24)) { afg::set_error("afg_pvoc_out_frames: n_frames %u: 1 .. 2^24", n_frames); return 0; }
    if (!rate_ok(rate)) { afg::set_error("afg_pvoc_out_frames: rate %g: finite, 1/64 .. 64", rate); return 0; }
    return out_frames_of(n_frames, rate);
}

extern "C" double afg_pvoc_bound(const afg_pvoc_params *params, uint64_t t)
{
    if (check_params(params, "afg_pvoc_bound")) return -1.0;
    return AFG_PVOC_KA * 0x1p-24 + AFG_PVOC_KP * 0x1p-53 * afg::kPi * ((double)t + 1.0);
}

extern "C" int afg_pvoc_check_rows(const afg_pvoc_row *rows, uint64_t n_rows, const afg_pvoc_params *params, uint64_t in_floats, uint64_t out_floats)
{
    if (int rc = check_params(params, "afg_pvoc_check_rows")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!rows) { afg::set_error("afg_pvoc_check_rows: NULL rows"); return AFG_ERR_INVALID; }
    return check_rows(rows, n_rows, *params, in_floats, out_floats);
}

extern "C" int afg_pvoc_hip(uint64_t n_rows, const afg_pvoc_row *d_rows, const afg_pvoc_params *params, const float *d_in, uint64_t in_floats,
                            float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = check_params(params, "afg_pvoc_hip")) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, *params, d_in, in_floats, d_out, out_floats)) return rc;
    if (int rc = afg::require_device()) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int rc = afg::with_host_records(d_rows, n_rows, stream, [&](const afg_pvoc_row *h) {
            return check_rows(h, n_rows, *params, in_floats, out_floats);
        }))
        return rc;
    const uint32_t groups = (params->n_fft / 2 + 1 + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(pvoc_kernel, dim3((uint32_t)(n_rows * groups)), dim3(kThreads), 0, stream, d_rows, params->n_fft, params->hop, groups, d_in, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
