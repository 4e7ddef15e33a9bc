// xm_mix.hip -- the FastTracker II XM mixer (xm_next_of_sample and xm_sample, libxm.d:2313-2475) for gfx950.
//
// Work: one wavefront mixes one tick of one song at a time (ticks are taken round-robin by a fixed grid).  Lane l owns one
// group of 16 consecutive frames, aligned to 16 song-relative frames, so its output is one 128-byte line that it stores
// itself with eight 16-byte stores: no LDS.  For every segment of the tick (channels in index order, as the reference adds
// them) a lane whose frames the segment covers takes its first position -- in closed form (mod_chain.h) where the chain runs
// forward, from the side table where the host stepped it -- then steps and gathers sequentially with the reference's own
// adds.  Inside a segment 0 <= position < length holds by construction (the host ends a segment at every wrap, turn and
// sample end), so a frame is a truncating conversion, a min against the last index, a gather and two multiply-adds kept
// separate (-ffp-contract=off).  Segments whose volumes rest and that are past the trigger cross-fade take the short loop;
// ramp, cross-fade and partly covered groups take the general one.  The tick's scale is applied to the finished sum.
#include "afg_common.h"
#include "mod_chain.h"

#include <algorithm>
#include <atomic>

namespace {

constexpr int kThreads = 64;
constexpr int kPer = 16;                             // frames per lane: one 128-byte line of output
constexpr int kTile = kThreads * kPer;
constexpr uint32_t kGridRounds = 8;                  // as mod_mix.hip: ticks differ in cost, the dispatcher backfills

template <bool k16>
__device__ __forceinline__ float sample_at(const uint8_t *data, uint32_t last, float p)
{
    // the reference's cast for a position in range; a NaN or negative position reads index 0 and one past the end the last
    // sample, as the host's index_of() spells out (a float-to-unsigned conversion out of range is undefined in C++)
    const uint32_t a = min(p >= 0.0f ? (uint32_t)fminf(p, 4294967040.0f) : 0u, last);
    if (k16) return (float)((const int16_t *)data)[a] * (1.0f / 32768.0f);
    return (float)((const int8_t *)data)[a] * (1.0f / 128.0f);
}

template <bool k16>
__device__ __forceinline__ void steady16(const uint8_t *data, const afg_xm_segment &g, float p, float sstep, float *acc_l, float *acc_r)
{
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        const float v = sample_at<k16>(data, g.last, p);
        acc_l[j] = acc_l[j] + v * g.vol_l;
        acc_r[j] = acc_r[j] + v * g.vol_r;
        p = p + sstep;
    }
}

__global__ __launch_bounds__(kThreads) void xm_mix_kernel(uint32_t n_songs, const afg_xm_song *__restrict__ songs,
                                                          const afg_xm_segment *__restrict__ segs,
                                                          const afg_xm_tick *__restrict__ ticks,
                                                          const uint8_t *__restrict__ bytes, const float *__restrict__ aux_all,
                                                          float *__restrict__ out)
{
    const uint64_t n_ticks = songs[n_songs - 1].tick_base + songs[n_songs - 1].n_ticks;
    uint64_t t = blockIdx.x;
    if (t >= n_ticks) return;
    uint32_t s = 0;
    {
        uint32_t lo = 0, hi = n_songs - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (songs[mid].tick_base <= t) lo = mid; else hi = mid - 1;
        }
        s = lo;
    }
    const uint32_t lane = threadIdx.x;
    for (; t < n_ticks; t += gridDim.x) {
        while (s + 1 < n_songs && songs[s + 1].tick_base <= t) s++;
        const afg_xm_song song = songs[s];
        const afg_xm_tick tk = ticks[t];
        const afg_xm_segment *sg = segs + song.seg_base + tk.seg;
        const uint8_t *plane = bytes + song.sample_base;
        const float *aux = aux_all + song.aux_base;
        const uint32_t t_end = tk.frame + tk.frames;
        for (uint32_t g0 = tk.frame & ~15u; g0 < t_end; g0 += kTile) {
            const uint32_t f0 = g0 + lane * kPer;            // song-relative first frame of this lane's group
            float acc_l[kPer], acc_r[kPer];
#pragma unroll
            for (int j = 0; j < kPer; j++) { acc_l[j] = 0.0f; acc_r[j] = 0.0f; }
            afg_xm_segment next;
            if (tk.n_seg) next = sg[0];
            for (uint32_t k = 0; k < tk.n_seg; k++) {
                const afg_xm_segment g = next;
                if (k + 1 < tk.n_seg) next = sg[k + 1];      // the next record is on its way while this one is mixed
                const uint32_t lo = max(f0, g.frame);
                const uint32_t hi = min(f0 + kPer, g.frame + g.frames);
                if (lo >= hi) continue;
                float p = (g.flags & AFG_XM_SEG_TABLE) ? aux[g.aux_pos + (lo >> 4) - (g.frame >> 4)]
                                                       : afg_mod::chain_jump(g.position, g.step, lo - g.frame);
                const float sstep = (g.flags & AFG_XM_SEG_BACK) ? -g.step : g.step;      // p - step == p + (-step)
                const uint8_t *data = plane + g.sample_off;
                const bool is16 = (g.flags & AFG_XM_SEG_16BIT) != 0;
                if (hi - lo == kPer && !(g.flags & (AFG_XM_SEG_RAMP | AFG_XM_SEG_FADE))) {
                    if (is16) steady16<true>(data, g, p, sstep, acc_l, acc_r);
                    else steady16<false>(data, g, p, sstep, acc_l, acc_r);
                    continue;
                }
                const bool ramp = (g.flags & AFG_XM_SEG_RAMP) != 0, fade = (g.flags & AFG_XM_SEG_FADE) != 0;
#pragma unroll
                for (int j = 0; j < kPer; j++) {
                    const uint32_t f = f0 + (uint32_t)j;
                    if (f >= lo && f < hi) {
                        const uint32_t rel = f - g.frame;
                        float v = is16 ? sample_at<true>(data, g.last, p) : sample_at<false>(data, g.last, p);
                        if (fade) {
                            const float u = aux[g.aux_fade + rel];
                            v = u + ((float)(g.fade_count + rel) / 32.0f) * (v - u);
                        }
                        float vl = g.vol_l, vr = g.vol_r;
                        if (ramp) { vl = aux[g.aux_vol + 2 * rel]; vr = aux[g.aux_vol + 2 * rel + 1]; }
                        acc_l[j] = acc_l[j] + v * vl;
                        acc_r[j] = acc_r[j] + v * vr;
                        p = p + sstep;
                    }
                }
            }
            if (f0 >= t_end) continue;
            const uint64_t at = song.out_frame + f0;         // this lane's line of the output
            if (f0 >= tk.frame && f0 + kPer <= t_end && !(at & 1)) {
                float4 *o4 = (float4 *)(out + 2 * at);
#pragma unroll
                for (int j = 0; j < kPer; j += 2)
                    o4[j >> 1] = make_float4(acc_l[j] * tk.scale, acc_r[j] * tk.scale, acc_l[j + 1] * tk.scale, acc_r[j + 1] * tk.scale);
            } else {
#pragma unroll
                for (int j = 0; j < kPer; j++) {
                    const uint32_t f = f0 + (uint32_t)j;
                    if (f >= tk.frame && f < t_end) *(float2 *)(out + 2 * (at + j)) = make_float2(acc_l[j] * tk.scale, acc_r[j] * tk.scale);
                }
            }
        }
    }
}

}  // namespace

extern "C" int afg_xm_render_hip(uint32_t n_songs, const afg_xm_song *d_songs, const afg_xm_segment *d_segments,
                                 const afg_xm_tick *d_ticks, const uint8_t *d_sample_bytes, const float *d_aux, float *d_out,
                                 void *hip_stream)
{
    if (n_songs == 0) return AFG_OK;
    if (!d_songs || !d_segments || !d_ticks || !d_sample_bytes || !d_aux || !d_out) {
        afg::set_error("afg_xm_render_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (int rc = afg::require_device()) return rc;
    int dev = 0;
    AFG_HIP_CHECK(hipGetDevice(&dev));
    static std::atomic<uint32_t> s_groups[AFG_MAX_DEVICES];
    uint32_t groups = (dev >= 0 && dev < AFG_MAX_DEVICES) ? s_groups[dev].load(std::memory_order_relaxed) : 0u;
    if (!groups) {
        int cus = 0, per_cu = 0;
        AFG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        AFG_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xm_mix_kernel, kThreads, 0));
        groups = (uint32_t)std::max(1, cus) * (uint32_t)std::max(1, per_cu) * kGridRounds;
        if (dev >= 0 && dev < AFG_MAX_DEVICES) s_groups[dev].store(groups, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(xm_mix_kernel, dim3(groups), dim3(kThreads), 0, (hipStream_t)hip_stream, n_songs, d_songs, d_segments,
                       d_ticks, d_sample_bytes, d_aux, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
