// mod_mix.hip -- the ProTracker MOD mixer (pocketmod.d:664-721, :908-952) for gfx950.
//
// Work: one workgroup of one wavefront mixes one tick of one song at a time (ticks are taken round-robin by a fixed grid),
// in tiles of 1024 frames: lane l owns 16 consecutive frames of the tile.  For every segment of the tick (channels in index
// order, as the reference adds them) a lane whose frames it covers jumps to its first frame in closed form
// (mod_chain.h), then steps and gathers sequentially -- the adds are the reference's own, so the positions are exact.
// Each frame starts at +0.0f and takes level * s in segment order, a separate multiply and add (-ffp-contract=off).
// The mixed tile is transposed through LDS so that the stores are 16-byte, whole-line and in address order: the output
// (8 bytes per frame) is the only stream of bytes that grows with the work.
#include "afg_common.h"
#include "mod_chain.h"

#include <algorithm>
#include <atomic>

namespace {

constexpr int kThreads = 64;
constexpr int kPer = 16;                             // frames per lane: a lane jumps once per segment and steps 16 frames
constexpr int kTile = kThreads * kPer;               // frames per tile
// Grid: this many times what is resident at once.  Ticks go out round-robin in equal shares but differ in cost (segments
// per tick); with a grid of one residency the slowest shares set the time, with more the dispatcher backfills CUs as
// workgroups finish and the last partial round is a small part of the work.  1024 four-channel songs (tools/bench_mod.py):
// 1 x residency 33.8 ms, 2 x 27.1, 4 x 24.7, 8 x 24.1, 16 x 24.3; a fixed 32 workgroups per CU (1.6 x) 27.8.
constexpr uint32_t kGridRounds = 8;

// (float)(int8)plane[sample_off + (int)p], 0 outside the plane.  (An unconditional load behind a clamped address and a
// select measured no faster and took 136 VGPRs instead of 75.)
__device__ __forceinline__ float gather(const uint8_t *plane, uint32_t bytes, uint32_t sample_off, float p)
{
    const int32_t x = afg_mod::cvt_i32(p);
    const uint32_t at = sample_off + (uint32_t)x;
    return (x >= 0 && at < bytes) ? (float)(int8_t)plane[at] : 0.0f;
}

__global__ __launch_bounds__(kThreads) void mod_mix_kernel(uint32_t n_songs, const afg_mod_song *__restrict__ songs,
                                                           const afg_mod_segment *__restrict__ segs,
                                                           const afg_mod_tick *__restrict__ ticks,
                                                           const uint8_t *__restrict__ bytes, float *__restrict__ out)
{
    __shared__ float2 tile[kTile];
    const uint64_t n_ticks = songs[n_songs - 1].tick_base + songs[n_songs - 1].n_ticks;
    uint64_t t = blockIdx.x;
    if (t >= n_ticks) return;
    // the song of tick t: a binary search once, then forward steps as t grows by the grid size
    uint32_t s = 0;
    {
        uint32_t lo = 0, hi = n_songs - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (songs[mid].tick_base <= t) lo = mid; else hi = mid - 1;
        }
        s = lo;
    }
    const int lane = (int)threadIdx.x;
    for (; t < n_ticks; t += gridDim.x) {
        while (s + 1 < n_songs && songs[s + 1].tick_base <= t) s++;
        const afg_mod_song song = songs[s];
        const afg_mod_tick tk = ticks[t];
        const afg_mod_segment *sg = segs + song.seg_base + tk.seg;
        const uint8_t *plane = bytes + song.sample_base;
        for (uint32_t t0 = 0; t0 < tk.frames; t0 += kTile) {
            const uint32_t nf = min((uint32_t)kTile, tk.frames - t0);
            const uint32_t f0 = tk.frame + t0 + (uint32_t)lane * kPer;          // song-relative first frame of this lane
            float acc_l[kPer], acc_r[kPer];
#pragma unroll
            for (int j = 0; j < kPer; j++) { acc_l[j] = 0.0f; acc_r[j] = 0.0f; }
            for (uint32_t k = 0; k < tk.n_seg; k++) {
                const afg_mod_segment g = sg[k];
                const uint32_t lo = max(f0, g.frame);
                const uint32_t hi = min(f0 + kPer, g.frame + g.frames);
                if (lo >= hi) continue;
                float p = afg_mod::chain_jump(g.position, g.increment, lo - g.frame);
                if (lo == f0 && hi == f0 + kPer) {           // the segment covers all of the lane's frames (the usual case)
#pragma unroll
                    for (int j = 0; j < kPer; j++) {
                        const float v = gather(plane, song.sample_bytes, g.sample_off, p);
                        acc_l[j] = acc_l[j] + g.level_l * v;
                        acc_r[j] = acc_r[j] + g.level_r * v;
                        p = p + g.increment;
                    }
                    continue;
                }
#pragma unroll
                for (int j = 0; j < kPer; j++) {
                    const uint32_t f = f0 + (uint32_t)j;
                    if (f >= lo && f < hi) {
                        const float v = gather(plane, song.sample_bytes, g.sample_off, p);
                        acc_l[j] = acc_l[j] + g.level_l * v;
                        acc_r[j] = acc_r[j] + g.level_r * v;
                        p = p + g.increment;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kPer; j++) tile[lane * kPer + j] = make_float2(acc_l[j], acc_r[j]);
            __syncthreads();
            // floats [b, b + 2 nf) of the output: a float2 head up to 16-byte alignment, then float4 stores
            const uint64_t b = 2 * (song.out_frame + tk.frame + t0);
            const uint32_t head = (uint32_t)((b >> 1) & 1);                        // frames before the first aligned float4
            if (head && lane == 0) *(float2 *)(out + b) = tile[0];
            const uint32_t body = (nf - min(head, nf)) >> 1;                        // float4 (two-frame) stores
            float4 *o4 = (float4 *)(out + b + 2 * head);
            for (uint32_t i = (uint32_t)lane; i < body; i += kThreads) {
                const float2 a = tile[head + 2 * i], c = tile[head + 2 * i + 1];
                o4[i] = make_float4(a.x, a.y, c.x, c.y);
            }
            const uint32_t done = head + 2 * body;
            if (done < nf && lane == 1) *(float2 *)(out + b + 2 * done) = tile[done];
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" int afg_mod_render_hip(uint32_t n_songs, const afg_mod_song *d_songs, const afg_mod_segment *d_segments,
                                  const afg_mod_tick *d_ticks, const uint8_t *d_sample_bytes, float *d_out, void *hip_stream)
{
    if (n_songs == 0) return AFG_OK;
    if (!d_songs || !d_segments || !d_ticks || !d_sample_bytes || !d_out) {
        afg::set_error("afg_mod_render_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (int rc = afg::require_device()) return rc;
    // A fixed grid that takes the ticks round-robin (the tick count lives on the device), sized from what is resident at once
    // (kGridRounds above).  LDS bounds residency (an 8 KiB tile per one-wavefront workgroup: 20 per CU, 5 per SIMD; the
    // 75 VGPRs would allow 6).
    int dev = 0;
    AFG_HIP_CHECK(hipGetDevice(&dev));
    static std::atomic<uint32_t> s_groups[AFG_MAX_DEVICES];
    uint32_t groups = (dev >= 0 && dev < AFG_MAX_DEVICES) ? s_groups[dev].load(std::memory_order_relaxed) : 0u;
    if (!groups) {
        int cus = 0, per_cu = 0;
        AFG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        AFG_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mod_mix_kernel, kThreads, 0));
        groups = (uint32_t)std::max(1, cus) * (uint32_t)std::max(1, per_cu) * kGridRounds;
        if (dev >= 0 && dev < AFG_MAX_DEVICES) s_groups[dev].store(groups, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(mod_mix_kernel, dim3(groups), dim3(kThreads), 0, (hipStream_t)hip_stream, n_songs, d_songs, d_segments,
                       d_ticks, d_sample_bytes, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}
