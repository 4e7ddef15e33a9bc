// afg_trim.cpp -- the host half of the silence trim (include/afg.h; kernels in csrc/trim.hip): the block and tile layout and
// the checks of groups and parameters, which need no device; and afg_batch_decode_trimmed -- afg_front::resampled_run of a
// sublist at scan_frames into a pooled scratch, then one afg_trim_hip launch into the caller's tensor.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

constexpr uint32_t kTile = afg::kPlaneTile;

uint64_t blocks_of(const afg_trim_group &g, uint32_t hop) { return ((uint64_t)g.valid + hop - 1) / hop; }
uint64_t tiles_of(const afg_trim_group &g) { return (((uint64_t)g.out_frames + kTile - 1) / kTile) * g.out_rows; }

int check_params(const afg_trim_params *p)
{
    if (!p) { afg::set_error("afg_trim_params: NULL"); return AFG_ERR_INVALID; }
    if (p->hop < 1) { afg::set_error("afg_trim_params.hop %u: at least 1", p->hop); return AFG_ERR_INVALID; }
    if (p->frame_length < 1 || p->frame_length > 65536) {
        afg::set_error("afg_trim_params.frame_length %u: 1 .. 65536", p->frame_length);
        return AFG_ERR_INVALID;
    }
    if (p->frame_length % p->hop != 0) {
        afg::set_error("afg_trim_params.frame_length %u: a multiple of hop (%u)", p->frame_length, p->hop);
        return AFG_ERR_INVALID;
    }
    const uint32_t k = p->frame_length / p->hop;
    if (k != 1 && (k % 2 != 0 || k > 64)) {
        afg::set_error("afg_trim_params.frame_length / hop is %u: 1 or an even number up to 64", k);
        return AFG_ERR_INVALID;
    }
    if (p->reference != AFG_TRIM_REF_MAX && p->reference != AFG_TRIM_REF_ABS) {
        afg::set_error("afg_trim_params.reference %u: AFG_TRIM_REF_MAX or AFG_TRIM_REF_ABS", p->reference);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->ratio) || !(p->ratio > 0.0)) { afg::set_error("afg_trim_params.ratio %g: finite and above 0", p->ratio); return AFG_ERR_INVALID; }
    if (p->reference == AFG_TRIM_REF_MAX && p->ratio > 1.0) {
        afg::set_error("afg_trim_params.ratio %g: at most 1 over the loudest frame (AFG_TRIM_REF_MAX)", p->ratio);
        return AFG_ERR_INVALID;
    }
    if (p->reference == AFG_TRIM_REF_ABS && (!std::isfinite(p->abs_power) || !(p->abs_power > 0.0))) {
        afg::set_error("afg_trim_params.abs_power %g: finite and above 0 (AFG_TRIM_REF_ABS)", p->abs_power);
        return AFG_ERR_INVALID;
    }
    for (int k3 = 0; k3 < 3; k3++)
        if (p->reserved[k3] != 0) { afg::set_error("afg_trim_params.reserved[%d] %u: must be 0", k3, p->reserved[k3]); return AFG_ERR_INVALID; }
    return AFG_OK;
}

}  // namespace

extern "C" int afg_trim_layout(afg_trim_group *groups, uint64_t n_groups, const afg_trim_params *params, uint64_t *n_blocks, uint64_t *n_tiles)
{
    if (n_blocks) *n_blocks = 0;
    if (n_tiles) *n_tiles = 0;
    if (check_params(params)) return 0;
    if (!n_blocks || !n_tiles || (n_groups && !groups)) {
        afg::set_error("afg_trim_layout: NULL %s", !n_blocks ? "n_blocks" : !n_tiles ? "n_tiles" : "groups");
        return 0;
    }
    uint64_t blocks = 0, tiles = 0;
    for (uint64_t k = 0; k < n_groups; k++) {
        groups[k].first_block = blocks;
        groups[k].first_tile = tiles;
        blocks += blocks_of(groups[k], params->hop);
        tiles += tiles_of(groups[k]);
    }
    *n_blocks = blocks;
    *n_tiles = tiles;
    return 1;
}

extern "C" int afg_trim_check_groups(const afg_trim_group *groups, uint64_t n_groups, uint64_t n_blocks, uint64_t n_tiles,
                                     const afg_trim_params *params, uint64_t in_floats, uint64_t out_floats)
{
    if (int rc = check_params(params)) return rc;
    if (n_groups == 0) return AFG_OK;
    if (!groups) { afg::set_error("afg_trim_group: NULL groups"); return AFG_ERR_INVALID; }
    uint64_t blocks = 0, tiles = 0;
    for (uint64_t k = 0; k < n_groups; k++) {
        const afg_trim_group &g = groups[k];
        const unsigned long long kk = (unsigned long long)k;
        if (g.rows == 0 || g.rows > 0xffff) { afg::set_error("afg_trim_group %llu: rows %u: 1 .. 65535", kk, g.rows); return AFG_ERR_INVALID; }
        if (g.out_rows < g.rows) { afg::set_error("afg_trim_group %llu: out_rows %u below rows %u", kk, g.out_rows, g.rows); return AFG_ERR_INVALID; }
        if (g.first_block != blocks) {
            afg::set_error("afg_trim_group %llu: first_block %llu, afg_trim_layout gives %llu", kk, (unsigned long long)g.first_block,
                           (unsigned long long)blocks);
            return AFG_ERR_INVALID;
        }
        if (g.first_tile != tiles) {
            afg::set_error("afg_trim_group %llu: first_tile %llu, afg_trim_layout gives %llu", kk, (unsigned long long)g.first_tile,
                           (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        blocks += blocks_of(g, params->hop);                     // below 2^32 and 2^52 a group: no wrap before the caps refuse
        tiles += tiles_of(g);
        if (blocks > ((uint64_t)1 << 62) || tiles > ((uint64_t)1 << 62)) {
            afg::set_error("afg_trim_group %llu: too many blocks or tiles", kk);
            return AFG_ERR_INVALID;
        }
        if (g.valid != 0) {
            if (g.rows > 1 && g.in_stride < g.valid) {
                afg::set_error("afg_trim_group %llu: in_stride %llu below valid %u with %u rows", kk, (unsigned long long)g.in_stride, g.valid, g.rows);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(g.in_off, g.rows, g.in_stride, g.valid, in_floats)) {
                afg::set_error("afg_trim_group %llu: its rows leave the input (%llu floats)", kk, (unsigned long long)in_floats);
                return AFG_ERR_INVALID;
            }
        }
        if (g.out_frames != 0) {
            if (g.out_rows > 1 && g.out_stride < g.out_frames) {
                afg::set_error("afg_trim_group %llu: out_stride %llu below out_frames %u with %u rows", kk, (unsigned long long)g.out_stride,
                               g.out_frames, g.out_rows);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(g.out_off, g.out_rows, g.out_stride, g.out_frames, out_floats)) {
                afg::set_error("afg_trim_group %llu: its rows leave the output (%llu floats)", kk, (unsigned long long)out_floats);
                return AFG_ERR_INVALID;
            }
        }
    }
    if (blocks != n_blocks) {
        afg::set_error("afg_trim_group: n_blocks %llu, afg_trim_layout gives %llu", (unsigned long long)n_blocks, (unsigned long long)blocks);
        return AFG_ERR_INVALID;
    }
    if (tiles != n_tiles) {
        afg::set_error("afg_trim_group: n_tiles %llu, afg_trim_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

extern "C" int afg_batch_decode_trimmed(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                                        const afg_trim_params *trim, uint32_t scan_frames, float *d_out, afg_trim_region *regions,
                                        afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        afg_front::ResampleJob clip, job;                        // the caller's tensor; the scratch that is examined
        if (int rc = afg_front::entry_args("afg_batch_decode_trimmed", { { "opts", opts }, { "trim", trim }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (int rc = afg_front::resampled_opts_check(opts, data, length, n_files, clip)) return rc;
        if (int rc = afg_trim_check_groups(nullptr, 0, 0, 0, trim, 0, 0)) return rc;
        const uint32_t scan = scan_frames ? scan_frames : opts->frames;
        if (scan < opts->frames) {
            afg::set_error("afg_batch_decode_trimmed: scan_frames %u below frames %u", scan_frames, opts->frames);
            return AFG_ERR_INVALID;
        }
        afg_resample_opts ro = afg_front::resample_opts_of(*opts);
        ro.frames = scan;
        if (int rc = afg_front::resampled_check(&ro, data, length, n_files, job)) return rc;
        if (n_files == 0) return AFG_OK;
        const uint64_t slab_in = (uint64_t)job.C * scan, slab_out = (uint64_t)job.C * opts->frames;
        if (slab_in > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_trimmed: a scratch of %d x %u x %u floats", n_files, job.C, scan);
            return AFG_ERR_INVALID;
        }
        const size_t per_list = afg_front::sublist_size(n_files, slab_in * sizeof(float), afg::kDevTrimScratchBytes);
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg::require_device()) return rc;
        std::vector<afg_trim_group> groups;                      // (declared in front of the drain: the uploads read them)
        std::vector<afg_norm_group> file_groups;
        afg_front::DevBuf scratch, d_groups, d_blocks, d_regions;
        afg_front::NullStreamDrain drain;
        if (int rc = scratch.alloc((size_t)(per_list * slab_in * sizeof(float)))) return rc;
        if (int rc = d_regions.alloc((size_t)n_files * sizeof(afg_trim_region))) return rc;
        for (size_t f0 = 0; f0 < (size_t)n_files; f0 += per_list) {
            const size_t n = std::min(per_list, (size_t)n_files - f0);
            afg_resample_opts sub = ro;
            if (sub.first_frame) sub.first_frame += f0;
            // the tensor at one rate of the sublist, scan_frames long, every element written (a failed file's slab is zero) ...
            if (int rc = afg_front::resampled_run(job, &sub, data + f0, length + f0, (int)n, (float *)scratch.p, items + f0, messages)) return rc;
            // ... and every file's rows as one group, over its own samples, into its slab of the caller's tensor
            file_groups.clear();
            afg_front::norm_file_groups(job, items + f0, n, sub.first_frame, file_groups);
            groups.clear();
            for (size_t i = 0; i < n; i++) {
                afg_trim_group g;
                std::memset(&g, 0, sizeof(g));
                g.in_off = file_groups[i].in_off;
                g.in_stride = scan;
                g.out_off = i * slab_out;
                g.out_stride = opts->frames;
                g.rows = file_groups[i].rows;
                g.valid = file_groups[i].valid;
                g.out_rows = job.C;
                g.out_frames = opts->frames;
                groups.push_back(g);
            }
            uint64_t n_blocks = 0, n_tiles = 0;
            if (!afg_trim_layout(groups.data(), groups.size(), trim, &n_blocks, &n_tiles)) return AFG_ERR_INVALID;
            if (int rc = d_blocks.alloc((size_t)std::max<uint64_t>(n_blocks, 1) * sizeof(double))) return rc;
            if (int rc = afg_front::upload_records(d_groups, groups, nullptr)) return rc;
            float *y = d_out + f0 * slab_out;
            if (int rc = afg::trim_launch(groups.data(), groups.size(), (const afg_trim_group *)d_groups.p, n_blocks, n_tiles, trim,
                                          (const float *)scratch.p, n * slab_in, y, n * slab_out, (double *)d_blocks.p,
                                          (afg_trim_region *)d_regions.p + f0, nullptr))
                return rc;
            for (size_t i = 0; i < n; i++)
                if (items[f0 + i].pcm) items[f0 + i].pcm = y + i * slab_out;
            AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
        }
        if (regions) AFG_HIP_CHECK(hipMemcpy(regions, d_regions.p, (size_t)n_files * sizeof(afg_trim_region), hipMemcpyDeviceToHost));
        return res.finish(out);
    });
}
