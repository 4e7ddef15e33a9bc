// afg_loudness.cpp -- the host half of the loudness stage (include/afg.h; kernels in csrc/loudness.hip): the K-weighting of a
// sample rate, the layout of sub-block sums and block energies and the checks of parameters and groups -- none of which needs a
// device -- and afg_batch_decode_loudnorm: afg_front::resampled_run into the caller's tensor, then one afg_loudness_hip launch
// in place.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace {

constexpr uint32_t kMinRate = 8000, kMaxRate = 192000, kMaxRows = 8;

// the sub-blocks a row of the group has sums for, and the doubles the group takes in d_sub (a peak behind every row's sums)
uint32_t subs_of(const afg_loudness_group &g, uint32_t step)
{
    const uint32_t nb = afg::loudness_blocks(g.valid, step);
    return nb ? nb + 3u : 0u;
}
uint64_t sub_doubles(const afg_loudness_group &g, uint32_t step) { return g.valid ? (uint64_t)g.rows * ((uint64_t)subs_of(g, step) + 1u) : 0; }

}  // namespace

int afg::loudness_check_params(const afg_loudness_params *p)
{
    if (!p) { afg::set_error("afg_loudness_params: NULL"); return AFG_ERR_INVALID; }
    if (p->samplerate < kMinRate || p->samplerate > kMaxRate) {
        afg::set_error("afg_loudness_params.samplerate %u: %u .. %u", p->samplerate, kMinRate, kMaxRate);
        return AFG_ERR_INVALID;
    }
    if (p->apply > 1) { afg::set_error("afg_loudness_params.apply %u: 0 or 1", p->apply); return AFG_ERR_INVALID; }
    if (!std::isfinite(p->target_lufs) || std::fabs(p->target_lufs) > 200.0) {
        afg::set_error("afg_loudness_params.target_lufs %g: finite, -200 .. 200", p->target_lufs);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->max_peak) || p->max_peak < 0.0f) {
        afg::set_error("afg_loudness_params.max_peak %g: finite and at least 0 (0: no ceiling)", (double)p->max_peak);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->max_gain) || p->max_gain < 0.0f) {
        afg::set_error("afg_loudness_params.max_gain %g: finite and at least 0 (0: none)", (double)p->max_gain);
        return AFG_ERR_INVALID;
    }
    for (int k = 0; k < 8; k++)
        if (!std::isfinite(p->weights[k]) || p->weights[k] < 0.0) {
            afg::set_error("afg_loudness_params.weights[%d] %g: finite and at least 0", k, p->weights[k]);
            return AFG_ERR_INVALID;
        }
    for (int k = 0; k < 2; k++)
        if (p->reserved[k] != 0) { afg::set_error("afg_loudness_params.reserved[%d] %u: must be 0", k, p->reserved[k]); return AFG_ERR_INVALID; }
    return AFG_OK;
}

int afg::loudness_kweight(uint32_t samplerate, afg_filter_params *out)
{
    if (!out) { afg::set_error("afg_kweight_design: NULL out"); return AFG_ERR_INVALID; }
    if (samplerate < kMinRate || samplerate > kMaxRate) {
        afg::set_error("afg_kweight_design: samplerate %u: %u .. %u", samplerate, kMinRate, kMaxRate);
        return AFG_ERR_INVALID;
    }
    afg_filter_params kw;
    std::memset(&kw, 0, sizeof(kw));
    kw.n_sections = 2;
    {   // the shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(afg::kPi * f0 / (double)samplerate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        afg_biquad &s = kw.sec[0];
        s.b0 = (Vh + Vb * K / Q + K * K) / a0;
        s.b1 = 2.0 * (K * K - Vh) / a0;
        s.b2 = (Vh - Vb * K / Q + K * K) / a0;
        s.a1 = 2.0 * (K * K - 1.0) / a0;
        s.a2 = (1.0 - K / Q + K * K) / a0;
    }
    {   // the high-pass; its numerator is the standard's table's (1, -2, 1)
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(afg::kPi * f0 / (double)samplerate);
        const double a0 = 1.0 + K / Q + K * K;
        afg_biquad &s = kw.sec[1];
        s.b0 = 1.0; s.b1 = -2.0; s.b2 = 1.0;
        s.a1 = 2.0 * (K * K - 1.0) / a0;
        s.a2 = (1.0 - K / Q + K * K) / a0;
    }
    if (int rc = afg::filter_check_params(&kw)) return rc;       // (every rate in range passes the filter stage's pole test and bound)
    *out = kw;
    return AFG_OK;
}

extern "C" int afg_kweight_design(uint32_t samplerate, afg_filter_params *out) { return afg::loudness_kweight(samplerate, out); }

extern "C" double afg_loudness_lufs(double energy)
{
    if (energy == 0.0) return -std::numeric_limits<double>::infinity();
    return -0.691 + 10.0 * std::log10(energy);
}

extern "C" int afg_loudness_layout(afg_loudness_group *groups, uint64_t n_groups, const afg_loudness_params *params, afg_loudness_counts *counts)
{
    if (counts) { counts->n_sub = 0; counts->n_blocks = 0; }
    if (afg::loudness_check_params(params)) return 0;
    if (!counts || (n_groups && !groups)) {
        afg::set_error("afg_loudness_layout: NULL %s", !counts ? "counts" : "groups");
        return 0;
    }
    const uint32_t step = afg::loudness_step(params->samplerate);
    uint64_t subs = 0, blocks = 0;
    for (uint64_t k = 0; k < n_groups; k++) {
        groups[k].first_sub = subs;
        groups[k].first_block = blocks;
        subs += sub_doubles(groups[k], step);
        blocks += afg::loudness_blocks(groups[k].valid, step);
    }
    counts->n_sub = subs;
    counts->n_blocks = blocks;
    return 1;
}

extern "C" int afg_loudness_check_groups(const afg_loudness_group *groups, uint64_t n_groups, const afg_loudness_counts *counts,
                                         const afg_loudness_params *params, uint64_t in_floats, uint64_t out_floats, int same_plane)
{
    try {
        if (int rc = afg::loudness_check_params(params)) return rc;
        if (n_groups == 0) return AFG_OK;
        if (!groups || !counts) { afg::set_error("afg_loudness_check_groups: NULL %s", !groups ? "groups" : "counts"); return AFG_ERR_INVALID; }
        const uint32_t step = afg::loudness_step(params->samplerate);
        uint64_t subs = 0, blocks = 0;
        std::vector<afg::Range> r;
        for (uint64_t k = 0; k < n_groups; k++) {
            const afg_loudness_group &g = groups[k];
            const unsigned long long kk = (unsigned long long)k;
            if (g.rows == 0 || g.rows > kMaxRows) { afg::set_error("afg_loudness_group %llu: rows %u: 1 .. %u", kk, g.rows, kMaxRows); return AFG_ERR_INVALID; }
            for (int q = 0; q < 4; q++)
                if (g.reserved[q] != 0) { afg::set_error("afg_loudness_group %llu: reserved[%d] %u: must be 0", kk, q, g.reserved[q]); return AFG_ERR_INVALID; }
            if (g.first_sub != subs) {
                afg::set_error("afg_loudness_group %llu: first_sub %llu, afg_loudness_layout gives %llu", kk, (unsigned long long)g.first_sub,
                               (unsigned long long)subs);
                return AFG_ERR_INVALID;
            }
            if (g.first_block != blocks) {
                afg::set_error("afg_loudness_group %llu: first_block %llu, afg_loudness_layout gives %llu", kk, (unsigned long long)g.first_block,
                               (unsigned long long)blocks);
                return AFG_ERR_INVALID;
            }
            subs += sub_doubles(g, step);                        // below 2^27 a group: no wrap before the cap refuses
            blocks += afg::loudness_blocks(g.valid, step);
            if (subs > ((uint64_t)1 << 58)) { afg::set_error("afg_loudness_group %llu: too many sub-blocks", kk); return AFG_ERR_INVALID; }
            if (g.valid == 0) continue;
            if (g.rows > 1 && g.stride < g.valid) {
                afg::set_error("afg_loudness_group %llu: stride %llu below valid %u with %u rows", kk, (unsigned long long)g.stride, g.valid, g.rows);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(g.in_off, g.rows, g.stride, g.valid, in_floats)) {
                afg::set_error("afg_loudness_group %llu: its rows leave the input (%llu floats)", kk, (unsigned long long)in_floats);
                return AFG_ERR_INVALID;
            }
            if (!params->apply) continue;
            if (!afg::rows_inside(g.out_off, g.rows, g.stride, g.valid, out_floats)) {
                afg::set_error("afg_loudness_group %llu: its rows leave the output (%llu floats)", kk, (unsigned long long)out_floats);
                return AFG_ERR_INVALID;
            }
            for (uint32_t q = 0; q < g.rows; q++) {
                const uint64_t o = g.out_off + q * g.stride, i = g.in_off + q * g.stride;
                r.push_back(afg::Range{ o, o + g.valid, k, true });
                if (same_plane && g.in_off != g.out_off) r.push_back(afg::Range{ i, i + g.valid, k, false });
            }
        }
        if (subs != counts->n_sub) {
            afg::set_error("afg_loudness_group: n_sub %llu, afg_loudness_layout gives %llu", (unsigned long long)counts->n_sub, (unsigned long long)subs);
            return AFG_ERR_INVALID;
        }
        if (blocks != counts->n_blocks) {
            afg::set_error("afg_loudness_group: n_blocks %llu, afg_loudness_layout gives %llu", (unsigned long long)counts->n_blocks,
                           (unsigned long long)blocks);
            return AFG_ERR_INVALID;
        }
        uint64_t group = 0, other = 0;
        if (afg::first_overlap(r, &group, &other)) {
            afg::set_error("afg_loudness_group %llu: a row of it overlaps one of group %llu without being in place", (unsigned long long)group,
                           (unsigned long long)other);
            return AFG_ERR_INVALID;
        }
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

extern "C" int afg_batch_decode_loudnorm(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                                         const afg_loudness_params *loudness, float *d_out, afg_loudness_stats *stats, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        afg_front::ResampleJob job;
        if (int rc = afg_front::entry_args("afg_batch_decode_loudnorm", { { "opts", opts }, { "loudness", loudness }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (int rc = afg_front::resampled_opts_check(opts, data, length, n_files, job)) return rc;
        if (int rc = afg::loudness_check_params(loudness)) return rc;
        if (loudness->samplerate != job.samplerate) {
            afg::set_error("afg_batch_decode_loudnorm: afg_loudness_params.samplerate %u is not the tensor's %u", loudness->samplerate, job.samplerate);
            return AFG_ERR_INVALID;
        }
        if (job.C > kMaxRows) { afg::set_error("afg_batch_decode_loudnorm: channels %u: a group has at most %u rows", job.C, kMaxRows); return AFG_ERR_INVALID; }
        if (n_files == 0) return AFG_OK;
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg_front::resampled_run(job, opts, data, length, n_files, d_out, items, messages)) return rc;
        // the tensor is whole (resampled_run returns drained): one group per file, in place
        std::vector<afg_loudness_group> groups;                  // (declared in front of the drain: the upload reads them)
        afg_front::DevBuf d_groups, d_sub, d_blocks, d_stats;
        afg_front::NullStreamDrain drain;
        std::vector<afg_norm_group> file_groups;
        afg_front::norm_file_groups(job, items, (size_t)n_files, opts->first_frame, file_groups);
        for (const afg_norm_group &f : file_groups) {
            afg_loudness_group g;
            std::memset(&g, 0, sizeof(g));
            g.in_off = f.in_off; g.out_off = f.out_off; g.stride = f.stride; g.rows = f.rows; g.valid = f.valid;
            groups.push_back(g);
        }
        afg_loudness_counts counts;
        if (!afg_loudness_layout(groups.data(), groups.size(), loudness, &counts)) return AFG_ERR_INVALID;
        const uint64_t plane = (uint64_t)n_files * job.C * job.T;
        if (int rc = d_sub.alloc((size_t)std::max<uint64_t>(counts.n_sub, 1) * sizeof(double))) return rc;
        if (int rc = d_blocks.alloc((size_t)std::max<uint64_t>(counts.n_blocks, 1) * sizeof(double))) return rc;
        if (int rc = d_stats.alloc(groups.size() * sizeof(afg_loudness_stats))) return rc;
        if (int rc = afg_front::upload_records(d_groups, groups, nullptr)) return rc;
        if (int rc = afg::loudness_launch(groups.data(), groups.size(), (const afg_loudness_group *)d_groups.p, &counts, loudness, d_out, plane, d_out,
                                          plane, (double *)d_sub.p, (double *)d_blocks.p, (afg_loudness_stats *)d_stats.p, nullptr))
            return rc;
        AFG_HIP_CHECK(hipStreamSynchronize(nullptr));
        if (stats) AFG_HIP_CHECK(hipMemcpy(stats, d_stats.p, groups.size() * sizeof(afg_loudness_stats), hipMemcpyDeviceToHost));
        return res.finish(out);
    });
}
