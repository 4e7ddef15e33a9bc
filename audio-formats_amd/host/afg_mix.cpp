// afg_mix.cpp -- the host half of the mixing stage (include/afg.h; kernels in csrc/mix.hip): the tile layout, the SNR ratio
// and the checks of groups and planes -- none of which needs a device -- and afg_batch_decode_mixed: afg_front::resampled_run
// into the caller's tensor, then one afg_mix_hip launch in place.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

constexpr uint32_t kTile = afg::kPlaneTile;

uint64_t tiles_of(const afg_mix_group &g)
{
    return (((uint64_t)g.valid + kTile - 1) / kTile) * g.rows;
}

// [a, a + n) and [b, b + m) share a float (n, m > 0; the sums do not wrap: both are spans of real memory)
bool planes_meet(uint64_t a, uint64_t n, uint64_t b, uint64_t m)
{
    return n != 0 && m != 0 && a < b + m && b < a + n;
}

}  // namespace

extern "C" double afg_mix_ratio(double snr_db) { return std::pow(10.0, -snr_db / 10.0); }

extern "C" uint64_t afg_mix_layout(afg_mix_group *groups, uint64_t n_groups)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; groups && k < n_groups; k++) {
        groups[k].first_tile = tiles;
        tiles += tiles_of(groups[k]);
    }
    return tiles;
}

extern "C" int afg_mix_check_groups(const afg_mix_group *groups, uint64_t n_groups, uint64_t n_tiles, uint64_t in_floats, uint64_t noise_floats,
                                    uint64_t out_floats, const uint64_t *plane_at)
{
    try {
        if (n_groups == 0) return AFG_OK;
        if (!groups) { afg::set_error("afg_mix_check_groups: NULL groups"); return AFG_ERR_INVALID; }
        const uint64_t at_in = plane_at ? plane_at[0] : 0, at_noise = plane_at ? plane_at[1] : 0, at_out = plane_at ? plane_at[2] : 0;
        if (plane_at && planes_meet(at_out, out_floats, at_noise, noise_floats)) {
            afg::set_error("afg_mix_hip: the output plane overlaps the noise plane");
            return AFG_ERR_INVALID;
        }
        const bool shared = plane_at && planes_meet(at_in, in_floats, at_out, out_floats);   // input rows can meet output rows at all
        uint64_t tiles = 0;
        std::vector<afg::Range> r;
        for (uint64_t k = 0; k < n_groups; k++) {
            const afg_mix_group &g = groups[k];
            const unsigned long long kk = (unsigned long long)k;
            if (g.flags != AFG_MIX_SNR && g.flags != AFG_MIX_GAIN) {
                afg::set_error("afg_mix_hip: group %llu: flags %u: AFG_MIX_SNR or AFG_MIX_GAIN", kk, g.flags);
                return AFG_ERR_INVALID;
            }
            if (g.flags == AFG_MIX_SNR && !(std::isfinite(g.ratio) && g.ratio >= 0.0)) {
                afg::set_error("afg_mix_hip: group %llu: ratio %g: finite and at least 0", kk, g.ratio);
                return AFG_ERR_INVALID;
            }
            if (g.flags == AFG_MIX_GAIN && !(std::isfinite(g.gain) && g.gain >= 0.0f)) {
                afg::set_error("afg_mix_hip: group %llu: gain %g: finite and at least 0", kk, (double)g.gain);
                return AFG_ERR_INVALID;
            }
            if (g.rows == 0 || g.rows > 0xffff) {
                afg::set_error("afg_mix_hip: group %llu: rows %u: 1 .. 65535", kk, g.rows);
                return AFG_ERR_INVALID;
            }
            if (g.first_tile != tiles) {
                afg::set_error("afg_mix_hip: group %llu: first_tile %llu, afg_mix_layout gives %llu", kk, (unsigned long long)g.first_tile,
                               (unsigned long long)tiles);
                return AFG_ERR_INVALID;
            }
            tiles += tiles_of(g);                                    // below 2^36 a group: no wrap before the launch's cap refuses
            if (tiles > ((uint64_t)1 << 62)) { afg::set_error("afg_mix_hip: group %llu: too many tiles", kk); return AFG_ERR_INVALID; }
            if (g.valid == 0) continue;
            if (g.rows > 1 && g.stride < g.valid) {
                afg::set_error("afg_mix_hip: group %llu: stride %llu below valid %u with %u rows", kk, (unsigned long long)g.stride, g.valid, g.rows);
                return AFG_ERR_INVALID;
            }
            if (g.noise_len == 0) { afg::set_error("afg_mix_hip: group %llu: noise_len 0: at least 1", kk); return AFG_ERR_INVALID; }
            if (g.noise_start >= g.noise_len) {
                afg::set_error("afg_mix_hip: group %llu: noise_start %u: below noise_len %u", kk, g.noise_start, g.noise_len);
                return AFG_ERR_INVALID;
            }
            if (g.noise_stride != 0 && g.noise_stride < g.noise_len) {
                afg::set_error("afg_mix_hip: group %llu: noise_stride %llu: 0 or at least noise_len %u", kk, (unsigned long long)g.noise_stride,
                               g.noise_len);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(g.in_off, g.rows, g.stride, g.valid, in_floats)) {
                afg::set_error("afg_mix_hip: group %llu: its rows leave the input (%llu floats)", kk, (unsigned long long)in_floats);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(g.out_off, g.rows, g.stride, g.valid, out_floats)) {
                afg::set_error("afg_mix_hip: group %llu: its rows leave the output (%llu floats)", kk, (unsigned long long)out_floats);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(g.noise_off, g.noise_stride ? g.rows : 1, g.noise_stride, g.noise_len, noise_floats)) {
                afg::set_error("afg_mix_hip: group %llu: its noise rows leave the noise plane (%llu floats)", kk, (unsigned long long)noise_floats);
                return AFG_ERR_INVALID;
            }
            for (uint32_t q = 0; q < g.rows; q++) {                  // (inside their planes: none of these sums wraps)
                const uint64_t o = at_out + g.out_off + q * g.stride, i = at_in + g.in_off + q * g.stride;
                r.push_back(afg::Range{ o, o + g.valid, k, true });
                if (shared && i != o) r.push_back(afg::Range{ i, i + g.valid, k, false });
            }
        }
        if (tiles != n_tiles) {
            afg::set_error("afg_mix_hip: n_tiles %llu, afg_mix_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        if (int rc = afg::launch_caps("afg_mix_hip", "groups", n_groups, n_tiles)) return rc;
        uint64_t group = 0, other = 0;
        if (afg::first_overlap(r, &group, &other)) {
            afg::set_error("afg_mix_hip: group %llu: a row of it overlaps one of group %llu without being in place", (unsigned long long)group,
                           (unsigned long long)other);
            return AFG_ERR_INVALID;
        }
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

extern "C" int afg_batch_decode_mixed(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                                      const afg_mix_noise *noise, float *d_out, afg_mix_stats *stats, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        const char *const who = "afg_batch_decode_mixed";
        afg_front::ResampleJob job;
        if (int rc = afg_front::entry_args(who, { { "opts", opts }, { "noise", noise }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (int rc = afg_front::resampled_opts_check(opts, data, length, n_files, job)) return rc;
        if (!noise->d_noise || !noise->snr_db) { afg::set_error("%s: NULL afg_mix_noise.%s", who, !noise->d_noise ? "d_noise" : "snr_db"); return AFG_ERR_INVALID; }
        if (((uintptr_t)noise->d_noise & 3u) != 0) { afg::set_error("%s: afg_mix_noise.d_noise must be 4-byte aligned", who); return AFG_ERR_INVALID; }
        if (noise->n_clips == 0 || noise->clip_pitch == 0) {
            afg::set_error("%s: afg_mix_noise: n_clips %llu and clip_pitch %u must be at least 1", who, (unsigned long long)noise->n_clips, noise->clip_pitch);
            return AFG_ERR_INVALID;
        }
        if (noise->clip_rows != 1 && noise->clip_rows != job.C) {
            afg::set_error("%s: afg_mix_noise.clip_rows %u: 1 or the tensor's %u channels", who, noise->clip_rows, job.C);
            return AFG_ERR_INVALID;
        }
        const uint64_t clip_floats = (uint64_t)noise->clip_rows * noise->clip_pitch;             // below 2^48
        if (noise->n_clips > (((uint64_t)1 << 62) / clip_floats)) { afg::set_error("%s: afg_mix_noise.n_clips %llu: too many", who, (unsigned long long)noise->n_clips); return AFG_ERR_INVALID; }
        const uint64_t noise_floats = noise->n_clips * clip_floats, plane = (uint64_t)(n_files > 0 ? n_files : 0) * job.C * job.T;
        for (uint64_t k = 0; noise->lengths && k < noise->n_clips; k++)
            if (noise->lengths[k] == 0 || noise->lengths[k] > noise->clip_pitch) {
                afg::set_error("%s: afg_mix_noise.lengths[%llu] %u: 1 .. clip_pitch %u", who, (unsigned long long)k, noise->lengths[k], noise->clip_pitch);
                return AFG_ERR_INVALID;
            }
        for (int i = 0; i < n_files; i++) {
            if (noise->index && noise->index[i] >= noise->n_clips) {
                afg::set_error("%s: afg_mix_noise.index[%d] %u: the bank has %llu clips", who, i, noise->index[i], (unsigned long long)noise->n_clips);
                return AFG_ERR_INVALID;
            }
            if (!std::isfinite(noise->snr_db[i])) { afg::set_error("%s: afg_mix_noise.snr_db[%d] %g: finite", who, i, noise->snr_db[i]); return AFG_ERR_INVALID; }
            const double ratio = afg_mix_ratio(noise->snr_db[i]);
            if (!std::isfinite(ratio)) { afg::set_error("%s: afg_mix_noise.snr_db[%d] %g: its ratio is not finite", who, i, noise->snr_db[i]); return AFG_ERR_INVALID; }
        }
        if (planes_meet((uint64_t)(uintptr_t)d_out / 4, plane, (uint64_t)(uintptr_t)noise->d_noise / 4, noise_floats)) {
            afg::set_error("%s: the noise bank overlaps the tensor", who);
            return AFG_ERR_INVALID;
        }
        if (n_files == 0) return AFG_OK;
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg_front::resampled_run(job, opts, data, length, n_files, d_out, items, messages)) return rc;
        // the tensor is whole (resampled_run returns drained): one group per file, in place
        std::vector<afg_mix_group> groups;                       // (declared in front of the drain: the upload reads them)
        afg_front::DevBuf d_groups, d_partials, d_stats;
        afg_front::NullStreamDrain drain;
        std::vector<afg_norm_group> file_groups;
        afg_front::norm_file_groups(job, items, (size_t)n_files, opts->first_frame, file_groups);
        for (size_t i = 0; i < file_groups.size(); i++) {
            const afg_norm_group &f = file_groups[i];
            const uint64_t clip = noise->index ? noise->index[i] : 0;
            afg_mix_group g;
            std::memset(&g, 0, sizeof(g));
            g.in_off = f.in_off; g.out_off = f.out_off; g.stride = f.stride; g.rows = f.rows; g.valid = f.valid;
            g.noise_off = clip * clip_floats;
            g.noise_stride = noise->clip_rows == 1 ? 0 : noise->clip_pitch;
            g.noise_len = noise->lengths ? noise->lengths[clip] : noise->clip_pitch;
            g.noise_start = (uint32_t)((noise->start ? noise->start[i] : 0) % g.noise_len);
            g.flags = AFG_MIX_SNR;
            g.ratio = afg_mix_ratio(noise->snr_db[i]);
            groups.push_back(g);
        }
        const uint64_t tiles = afg_mix_layout(groups.data(), groups.size());
        if (int rc = d_partials.alloc((size_t)std::max<uint64_t>(tiles, 1) * 16)) return rc;
        if (int rc = d_stats.alloc(groups.size() * sizeof(afg_mix_stats))) return rc;
        if (int rc = afg_front::upload_records(d_groups, groups, nullptr)) return rc;
        if (int rc = afg::mix_launch(groups.data(), groups.size(), (const afg_mix_group *)d_groups.p, tiles, d_out, plane, noise->d_noise, noise_floats,
                                     d_out, plane, d_partials.p, (afg_mix_stats *)d_stats.p, nullptr))
            return rc;
        AFG_HIP_CHECK(hipStreamSynchronize(nullptr));
        if (stats) AFG_HIP_CHECK(hipMemcpy(stats, d_stats.p, groups.size() * sizeof(afg_mix_stats), hipMemcpyDeviceToHost));
        return res.finish(out);
    });
}
