// trim.hip -- the non-silent region of a group of float rows and the rows shifted to start there (afg_trim_hip,
// afg_batch_decode_trimmed), for gfx950.  The definition -- block powers in float64 in a fixed order, frames of k blocks, a
// threshold, the region's index arithmetic -- is in include/afg.h; the Makefile builds this file with -ffp-contract=off like
// every other exact-mode kernel.  The host half (layout, group checks, the batch entry) is host/afg_trim.cpp.
//
// Three launches on the caller's stream, no atomics, no host round trip between them:
//   powers   one workgroup of 256 lanes per run of 16 consecutive blocks of the launch; each of its four wavefronts takes the
//            blocks b % 4 == its index, finds the block's group by a search over the groups' first blocks (the first one) or by
//            walking on from the block before, and loops over the rows: lane l adds the squares of the samples i % 64 == l
//            of the block in ascending i (coalesced dword loads, eight in flight), the 64 lanes combine in the definition's
//            tree -- steps 1 .. 16 with ds_swizzle in xor mode, step 32 across the halves -- and the row's result goes onto
//            the block's sum, a plain add in ascending row order.  Lane 0 stores S_j to d_blocks.  No LDS.
//   region   one workgroup per group: lane t forms P_f of the frames f % 256 == t from up to k consecutive S_j, the maximum
//            and -- in a second pass over the same sums -- the first and last frame above the threshold meet in LDS, and
//            lane 0 writes the group's afg_trim_region.  A maximum and the two index reductions need no order.
//   apply    one workgroup per tile of 4096 floats of one output row.  The tile reads its group's region from device memory
//            and is a shifted copy followed by zeros, cut at the 16-byte boundaries of the output address: the interior is
//            stored as dwordx4 with unit k of lane l at 16-byte word k * 256 + l, so that one store instruction of the
//            workgroup writes 4 KiB whole; head and tail go one float per lane.  The input side is read as dwordx4 at
//            whatever dword alignment begin leaves it; a word that straddles the end of the copy is filled element by
//            element.  Rows the group has no input for, and what lies behind the region, are the same stores of +0.0f.
//
// Bounds: every group is checked on the host before the launch (afg_trim_check_groups); the kernels rely on it.  They read
// in[in_off + r * in_stride + e] for r < rows and e < valid only -- the apply pass reads e in [begin, end), and the region
// kernel makes end <= valid -- write out[out_off + r * out_stride + t] for r < out_rows and t < out_frames, blocks
// [0, n_blocks) and regions [0, n_groups).
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = afg::kPlaneTile;                      // floats of one output row per tile
constexpr uint32_t kRun = 16;                                   // blocks per workgroup of the powers kernel

static_assert(sizeof(afg_trim_group) == 64 && sizeof(afg_trim_region) == 16 && sizeof(afg_trim_params) == 48, "include/afg.h");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a dwordx4 at dword alignment

// lane l ^ D's value, D = 1 .. 16 (ds_swizzle in bit-mask mode: and 0x1f, or 0, xor D)
template <int D> __device__ __forceinline__ double from_xor(double v)
{
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x1f | (D << 10));
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x1f | (D << 10));
    return __hiloint2double(hi, lo);
}

// the 64 lanes' tree: in lane 0, v[l] + v[l + d] for d = 1, 2 .. 32
__device__ __forceinline__ double lane_tree(double q)
{
    q = q + from_xor<1>(q);
    q = q + from_xor<2>(q);
    q = q + from_xor<4>(q);
    q = q + from_xor<8>(q);
    q = q + from_xor<16>(q);
    return q + __shfl_xor(q, 32, 64);
}

__global__ __launch_bounds__(kThreads) void trim_powers_kernel(uint32_t n_groups, const afg_trim_group *__restrict__ groups, uint64_t n_blocks,
                                                               uint32_t hop, const float *__restrict__ in, double *__restrict__ blocks)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t b0 = (uint64_t)blockIdx.x * kRun;
    uint32_t gi = 0;
    bool found = false;
    for (uint32_t s = wave; s < kRun; s += 4) {
        const uint64_t b = b0 + s;
        if (b >= n_blocks) break;
        if (!found) {
            // the last group whose first block is <= b (groups without samples have no blocks)
            gi = afg::last_at_or_before(groups, n_groups, b, &afg_trim_group::first_block);
            found = true;
        } else {
            while (gi + 1 < n_groups && groups[gi + 1].first_block <= b) gi++;
        }
        const afg_trim_group g = groups[gi];
        const uint64_t j = b - g.first_block, at = j * hop;
        if (g.first_block > b || at >= g.valid) continue;       // (never, behind the checks)
        const uint32_t n = (uint32_t)min((uint64_t)hop, (uint64_t)g.valid - at);
        double S = 0.0;
        for (uint32_t r = 0; r < g.rows; r++) {
            const float *p = in + g.in_off + (uint64_t)r * g.in_stride + at;
            double q = 0.0;
            uint32_t i = lane;
            for (; i + 7 * 64 < n; i += 8 * 64) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = p[i + u * 64];
#pragma unroll
                for (int u = 0; u < 8; u++) q = q + (double)v[u] * (double)v[u];
            }
            for (; i < n; i += 64) {
                const double d = (double)p[i];
                q = q + d * d;
            }
            S = S + lane_tree(q);
        }
        if (lane == 0) blocks[b] = S;
    }
}

// P_f: the frame's S_j in ascending j from +0.0; blocks [f - k / 2, f + k / 2) cut to [0, nb), block f alone for k == 1
__device__ __forceinline__ double frame_power(const double *__restrict__ S, uint64_t f, uint64_t nb, uint32_t k)
{
    const uint64_t h = k / 2, j0 = f > h ? f - h : 0, j1 = k == 1 ? f + 1 : min(nb, f + h);
    double P = 0.0;
    for (uint64_t j = j0; j < j1; j++) P = P + S[j];
    return P;
}

__global__ __launch_bounds__(kThreads) void trim_region_kernel(const afg_trim_group *__restrict__ groups, afg_trim_params prm,
                                                               const double *__restrict__ blocks, afg_trim_region *__restrict__ regions)
{
    __shared__ double sh_m[kThreads];
    __shared__ uint64_t sh_first[kThreads], sh_last[kThreads];
    const afg_trim_group g = groups[blockIdx.x];
    const uint32_t t = threadIdx.x, k = prm.frame_length / prm.hop;
    const uint64_t nb = ((uint64_t)g.valid + prm.hop - 1) / prm.hop;
    const double *S = blocks + g.first_block;
    double m = 0.0;
    for (uint64_t f = t; f < nb; f += kThreads) {
        const double P = frame_power(S, f, nb, k);
        m = P > m ? P : m;
    }
    sh_m[t] = m;
    __syncthreads();
    for (uint32_t d = kThreads / 2; d > 0; d >>= 1) {
        if (t < d) { const double o = sh_m[t + d]; if (o > sh_m[t]) sh_m[t] = o; }
        __syncthreads();
    }
    const double ref = sh_m[0];
    double thr;
    if (prm.reference == AFG_TRIM_REF_ABS) {
        thr = prm.ratio * prm.abs_power;
        thr = thr * (double)((uint64_t)g.rows * prm.frame_length);
    } else {
        thr = prm.ratio * ref;
    }
    uint64_t first = ~(uint64_t)0, last = 0;                     // last counts from 1: 0 means none
    for (uint64_t f = t; f < nb; f += kThreads)
        if (frame_power(S, f, nb, k) > thr) {
            first = min(first, f);
            last = f + 1;
        }
    sh_first[t] = first;
    sh_last[t] = last;
    __syncthreads();
    for (uint32_t d = kThreads / 2; d > 0; d >>= 1) {
        if (t < d) {
            sh_first[t] = min(sh_first[t], sh_first[t + d]);
            sh_last[t] = max(sh_last[t], sh_last[t + d]);
        }
        __syncthreads();
    }
    if (t != 0) return;
    afg_trim_region rec;
    rec.begin = 0; rec.end = 0;
    rec.ref_power = ref;
    if (sh_last[0] != 0) {
        const uint64_t b = sh_first[0] * prm.hop, e = min((uint64_t)g.valid, sh_last[0] * prm.hop);
        rec.begin = (uint32_t)(b > prm.lead ? b - prm.lead : 0);
        rec.end = (uint32_t)min((uint64_t)g.valid, e + prm.trail);
    }
    regions[blockIdx.x] = rec;
}

// element e of the tile: the input's bits in front of c, +0.0f from there on
__device__ __forceinline__ float copy_one(const float *__restrict__ p, uint32_t e, uint32_t c) { return e < c ? p[e] : 0.0f; }

__global__ __launch_bounds__(kThreads) void trim_apply_kernel(uint32_t n_groups, const afg_trim_group *__restrict__ groups,
                                                              const afg_trim_region *__restrict__ regions, const float *__restrict__ in,
                                                              float *__restrict__ out)
{
    const uint64_t tile = blockIdx.x;
    // the last group whose first tile is <= tile (groups without output have no tiles)
    const uint32_t lo = afg::last_at_or_before(groups, n_groups, tile, &afg_trim_group::first_tile);
    const afg_trim_group g = groups[lo];
    if (g.first_tile > tile || g.out_frames == 0) return;       // (never, behind the checks)
    const uint64_t per_row = ((uint64_t)g.out_frames + kTile - 1) / kTile, local = tile - g.first_tile;
    const uint64_t r = local / per_row, t0 = (local - r * per_row) * kTile;
    if (r >= g.out_rows) return;
    const uint32_t n = (uint32_t)min((uint64_t)kTile, (uint64_t)g.out_frames - t0);
    const afg_trim_region reg = regions[lo];
    // the tile's first c floats are in[r][begin + t0 ...], the rest zero
    uint32_t c = 0;
    const uint64_t len = reg.end > reg.begin ? reg.end - reg.begin : 0;
    if (r < g.rows && len > t0) c = (uint32_t)min((uint64_t)n, len - t0);
    const float *p = in + g.in_off + r * g.in_stride + reg.begin + t0;      // (read below c only)
    float *y = out + g.out_off + r * g.out_stride + t0;
    const uint32_t lane = threadIdx.x;
    const uint32_t head = min(n, (uint32_t)((16u - ((uintptr_t)y & 15u)) & 15u) / 4u);
    const uint32_t words = (n - head) / 4, tail0 = head + 4 * words;
    if (lane < head) y[lane] = copy_one(p, lane, c);
    if (tail0 + lane < n) y[tail0 + lane] = copy_one(p, tail0 + lane, c);
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t w = k * kThreads + lane, e = head + 4 * w;
        v[k] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
        if (w >= words || e >= c) continue;
        if (e + 4 <= c) {
            v[k] = *(const f32x4u *)(p + e);
        } else {
            v[k].x = p[e];
            v[k].y = copy_one(p, e + 1, c);
            v[k].z = copy_one(p, e + 2, c);
            v[k].w = copy_one(p, e + 3, c);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t w = k * kThreads + lane;
        if (w < words) __builtin_nontemporal_store(v[k], (f32x4 *)(y + head + 4 * w));
    }
}

int check_args(uint64_t n_groups, const afg_trim_group *d_groups, uint64_t n_blocks, uint64_t n_tiles, const afg_trim_params *params,
               const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_blocks, afg_trim_region *d_regions)
{
    if (!params) {
        afg::set_error("afg_trim_hip: NULL params");
        return AFG_ERR_INVALID;
    }
    if (!d_groups || !d_regions || (n_blocks && (!d_in || !d_blocks)) || (n_tiles && !d_out)) {
        afg::set_error("afg_trim_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || ((uintptr_t)d_blocks & 7u) != 0 || ((uintptr_t)d_regions & 7u) != 0 ||
        ((uintptr_t)d_groups & 7u) != 0) {
        afg::set_error("afg_trim_hip: the planes must be 4-byte aligned, the groups, block powers and regions 8-byte aligned");
        return AFG_ERR_INVALID;
    }
    if (n_groups > 0x7fffffffull || n_tiles > 0x7fffffffull || n_blocks > 0x7fffffffull * kRun) {
        afg::set_error("afg_trim_hip: at most 2^31 - 1 groups, 2^31 - 1 tiles and 16 * (2^31 - 1) blocks per launch");
        return AFG_ERR_INVALID;
    }
    if (in_floats > (~(uint64_t)0 >> 3) || out_floats > (~(uint64_t)0 >> 3)) {
        afg::set_error("afg_trim_hip: a plane of 2^61 floats or more");
        return AFG_ERR_INVALID;
    }
    // the planes as byte ranges: the output may not overlap the input
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + in_floats * 4, b0 = (uintptr_t)d_out, b1 = b0 + out_floats * 4;
    if (d_in && d_out && in_floats && out_floats && a0 < b1 && b0 < a1) {
        afg::set_error("afg_trim_hip: the output plane overlaps the input plane");
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

}  // namespace

int afg::trim_launch(const afg_trim_group *h_groups, uint64_t n_groups, const afg_trim_group *d_groups, uint64_t n_blocks, uint64_t n_tiles,
                     const afg_trim_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_blocks,
                     afg_trim_region *d_regions, hipStream_t stream)
{
    if (int rc = afg_trim_check_groups(nullptr, 0, 0, 0, params, 0, 0)) return rc;          // the parameters count without groups too
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, n_blocks, n_tiles, params, d_in, in_floats, d_out, out_floats, d_blocks, d_regions)) return rc;
    if (int rc = afg_trim_check_groups(h_groups, n_groups, n_blocks, n_tiles, params, in_floats, out_floats)) return rc;
    if (int rc = afg::require_device()) return rc;
    const uint32_t ng = (uint32_t)n_groups;
    if (n_blocks)
        hipLaunchKernelGGL(trim_powers_kernel, dim3((uint32_t)((n_blocks + kRun - 1) / kRun)), dim3(kThreads), 0, stream, ng, d_groups, n_blocks,
                           params->hop, d_in, d_blocks);
    hipLaunchKernelGGL(trim_region_kernel, dim3(ng), dim3(kThreads), 0, stream, d_groups, *params, (const double *)d_blocks, d_regions);
    if (n_tiles)
        hipLaunchKernelGGL(trim_apply_kernel, dim3((uint32_t)n_tiles), dim3(kThreads), 0, stream, ng, d_groups, (const afg_trim_region *)d_regions,
                           d_in, d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_trim_hip(uint64_t n_groups, const afg_trim_group *d_groups, uint64_t n_blocks, uint64_t n_tiles, const afg_trim_params *params,
                            const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_blocks,
                            afg_trim_region *d_regions, void *hip_stream)
{
    if (int rc = afg_trim_check_groups(nullptr, 0, 0, 0, params, 0, 0)) return rc;
    if (n_groups == 0) return AFG_OK;
    if (int rc = check_args(n_groups, d_groups, n_blocks, n_tiles, params, d_in, in_floats, d_out, out_floats, d_blocks, d_regions)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_groups, n_groups, (hipStream_t)hip_stream, [&](const afg_trim_group *h) {
        return afg::trim_launch(h, n_groups, d_groups, n_blocks, n_tiles, params, d_in, in_floats, d_out, out_floats, d_blocks, d_regions,
                                (hipStream_t)hip_stream);
    });
}
