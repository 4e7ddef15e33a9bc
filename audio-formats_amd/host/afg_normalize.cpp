// afg_normalize.cpp -- the host half of the normalisation stage (include/afg.h; kernels in csrc/normalize.hip): the tile
// layout and the checks of groups and parameters, which need no device; the valid lengths and groups of a tensor at one
// sample rate (afg_stage.h: norm_valid, norm_file_groups, NormPlane); and afg_batch_decode_resampled_norm.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

constexpr uint32_t kTile = afg::kPlaneTile;

uint64_t tiles_of(const afg_norm_group &g)
{
    return (((uint64_t)g.valid + kTile - 1) / kTile) * g.rows;
}

bool positive(float v) { return std::isfinite(v) && v > 0.0f; }

int check_params(const afg_norm_params *p)
{
    if (!p) { afg::set_error("afg_norm_params: NULL"); return AFG_ERR_INVALID; }
    switch (p->mode) {
    case AFG_NORM_NONE:
        return AFG_OK;
    case AFG_NORM_PEAK:
    case AFG_NORM_RMS:
        if (positive(p->target)) return AFG_OK;
        afg::set_error("afg_norm_params.target %g: finite and above 0", (double)p->target);
        return AFG_ERR_INVALID;
    case AFG_NORM_STANDARD:
        if (std::isfinite(p->eps) && p->eps >= 0.0f) return AFG_OK;
        afg::set_error("afg_norm_params.eps %g: finite and at least 0 (0 means 1e-7)", (double)p->eps);
        return AFG_ERR_INVALID;
    case AFG_NORM_DYNAMIC_RANGE:
        if (positive(p->range) && positive(p->gain) && std::isfinite(p->shift)) return AFG_OK;
        afg::set_error("afg_norm_params: range %g and gain %g must be finite and above 0, shift %g finite", (double)p->range, (double)p->gain,
                       (double)p->shift);
        return AFG_ERR_INVALID;
    default:
        afg::set_error("afg_norm_params.mode %u: AFG_NORM_NONE .. AFG_NORM_DYNAMIC_RANGE", p->mode);
        return AFG_ERR_INVALID;
    }
}

}  // namespace

extern "C" uint64_t afg_norm_layout(afg_norm_group *groups, uint64_t n_groups)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; groups && k < n_groups; k++) {
        groups[k].first_tile = tiles;
        tiles += tiles_of(groups[k]);
    }
    return tiles;
}

extern "C" int afg_norm_check_groups(const afg_norm_group *groups, uint64_t n_groups, uint64_t n_tiles, const afg_norm_params *params,
                                     uint64_t in_floats, uint64_t out_floats)
{
    if (int rc = check_params(params)) return rc;
    if (n_groups == 0) return AFG_OK;
    if (!groups) { afg::set_error("afg_norm_check_groups: NULL groups"); return AFG_ERR_INVALID; }
    uint64_t tiles = 0;
    for (uint64_t k = 0; k < n_groups; k++) {
        const afg_norm_group &g = groups[k];
        const unsigned long long kk = (unsigned long long)k;
        if (g.rows == 0 || g.rows > 0xffff) {
            afg::set_error("afg_normalize_hip: group %llu: rows %u: 1 .. 65535", kk, g.rows);
            return AFG_ERR_INVALID;
        }
        if (g.first_tile != tiles) {
            afg::set_error("afg_normalize_hip: group %llu: first_tile %llu, afg_norm_layout gives %llu", kk, (unsigned long long)g.first_tile,
                           (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        tiles += tiles_of(g);                                    // below 2^36 a group: no wrap before the launch's cap refuses
        if (tiles > ((uint64_t)1 << 62)) { afg::set_error("afg_normalize_hip: group %llu: too many tiles", kk); return AFG_ERR_INVALID; }
        if (g.valid == 0) continue;
        if (g.rows > 1 && g.stride < g.valid) {
            afg::set_error("afg_normalize_hip: group %llu: stride %llu below valid %u with %u rows", kk, (unsigned long long)g.stride, g.valid, g.rows);
            return AFG_ERR_INVALID;
        }
        if (!afg::rows_inside(g.in_off, g.rows, g.stride, g.valid, in_floats)) {
            afg::set_error("afg_normalize_hip: group %llu: its rows leave the input (%llu floats)", kk, (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        if (params->mode != AFG_NORM_NONE && !afg::rows_inside(g.out_off, g.rows, g.stride, g.valid, out_floats)) {
            afg::set_error("afg_normalize_hip: group %llu: its rows leave the output (%llu floats)", kk, (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
    }
    if (tiles != n_tiles) {
        afg::set_error("afg_normalize_hip: n_tiles %llu, afg_norm_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

namespace afg_front {

uint32_t norm_valid(int64_t frames, int64_t first_frame, uint32_t in_rate, uint32_t out_rate, uint32_t T)
{
    if (in_rate == 0 || out_rate == 0 || first_frame < 0 || frames <= first_frame) return 0;
    const uint32_t g = afg::gcd32(in_rate, out_rate);
    const uint64_t M = in_rate / g, L = out_rate / g;
    const unsigned __int128 d = (unsigned __int128)(uint64_t)(frames - first_frame) * L;      // below 2^95
    const unsigned __int128 v = (d + (M - 1)) / M;
    return v >= T ? T : (uint32_t)v;
}

void norm_file_groups(const ResampleJob &job, const afg_batch_item *items, size_t n, const int64_t *first_frame, std::vector<afg_norm_group> &groups)
{
    const uint64_t slab = (uint64_t)job.C * job.T;
    for (size_t i = 0; i < n; i++) {
        const afg_batch_item &it = items[i];
        afg_norm_group g;
        std::memset(&g, 0, sizeof(g));
        g.in_off = g.out_off = i * slab;
        g.stride = job.T;
        g.rows = 1;
        if (it.status == AFG_OK && it.channels > 0) {
            const double rate = (double)it.samplerate;
            const uint32_t in_rate = rate >= 1.0 && rate < 4294967296.0 ? (uint32_t)std::llround(rate) : 0;
            g.rows = job.mono ? 1 : (uint32_t)std::min<int64_t>(it.channels, job.C);
            g.valid = norm_valid(it.frames, first_frame ? first_frame[i] : 0, in_rate, job.samplerate, job.T);
        }
        groups.push_back(g);
    }
}

int NormPlane::launch(const afg_norm_params &prm, std::vector<afg_norm_group> &groups, float *d_plane, uint64_t plane_floats,
                      afg_norm_stats *d_stats, hipStream_t st)
{
    recs.swap(groups);                                           // the upload's source lives as long as the object
    if (recs.empty()) return AFG_OK;
    const uint64_t tiles = afg_norm_layout(recs.data(), recs.size());
    if (int rc = d_partials.alloc((size_t)std::max<uint64_t>(tiles, 1) * 32)) return rc;
    if (!d_stats) {
        if (int rc = d_own_stats.alloc(recs.size() * sizeof(afg_norm_stats))) return rc;
        d_stats = (afg_norm_stats *)d_own_stats.p;
    }
    if (int rc = upload_records(d_recs, recs, st)) return rc;
    return afg::normalize_launch(recs.data(), recs.size(), (const afg_norm_group *)d_recs.p, tiles, &prm, d_plane, plane_floats, d_plane,
                                 plane_floats, d_partials.p, d_stats, st);
}

}  // namespace afg_front

extern "C" int afg_batch_decode_resampled_norm(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                                               const afg_norm_params *norm, float *d_out, afg_norm_stats *d_stats, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        afg_front::ResampleJob job;
        if (int rc = afg_front::entry_args("afg_batch_decode_resampled_norm", { { "opts", opts }, { "norm", norm }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (int rc = afg_front::resampled_opts_check(opts, data, length, n_files, job)) return rc;
        if (int rc = afg_norm_check_groups(nullptr, 0, 0, norm, 0, 0)) return rc;
        if (((uintptr_t)d_stats & 7u) != 0) { afg::set_error("afg_batch_decode_resampled_norm: d_stats must be 8-byte aligned"); return AFG_ERR_INVALID; }
        if (n_files == 0) return AFG_OK;
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg_front::resampled_run(job, opts, data, length, n_files, d_out, items, messages)) return rc;
        // the tensor is whole (resampled_run returns drained): one group per file, in place
        afg_front::NormPlane plane;                              // (declared in front of the drain: it holds what the upload reads)
        afg_front::NullStreamDrain drain;
        std::vector<afg_norm_group> groups;
        afg_front::norm_file_groups(job, items, (size_t)n_files, opts->first_frame, groups);
        if (int rc = plane.launch(*norm, groups, d_out, (uint64_t)n_files * job.C * job.T, d_stats, nullptr)) return rc;
        AFG_HIP_CHECK(hipStreamSynchronize(nullptr));
        return res.finish(out);
    });
}
