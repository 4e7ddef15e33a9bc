// afg_yin.cpp -- the host half of the YIN pitch stage (csrc/yin.hip): the check of afg_yin_params, afg_yin_lags (librosa's
// choice of the lag range), afg_yin_frames, afg_yin_layout, and afg_batch_decode_pitch -- the resampled tensor of a sublist
// into a scratch pooled under afg_dev_option "resample_scratch_bytes", one afg_yin_hip launch over its rows, one per file and
// channel, and zeros over the frames past each file's own.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

int afg::yin_check_params(const afg_yin_params *p, const char *who)
{
    if (!p) { afg::set_error("%s: NULL params", who); return AFG_ERR_INVALID; }
    if (p->frame_length < 4 || p->frame_length > 4096) {
        afg::set_error("%s: frame_length %u: 4 .. 4096", who, p->frame_length);
        return AFG_ERR_INVALID;
    }
    if (p->win_length < 1 || p->win_length > p->frame_length - 2) {
        afg::set_error("%s: win_length %u: 1 .. frame_length - 2 (%u)", who, p->win_length, p->frame_length - 2);
        return AFG_ERR_INVALID;
    }
    if (p->hop < 1) { afg::set_error("%s: hop %u: at least 1", who, p->hop); return AFG_ERR_INVALID; }
    const uint32_t most = p->frame_length - p->win_length - 1;
    if (p->tau_min < 1 || p->tau_min > p->tau_max) {
        afg::set_error("%s: tau_min %u: 1 .. tau_max (%u)", who, p->tau_min, p->tau_max);
        return AFG_ERR_INVALID;
    }
    if (p->tau_max > most) {
        afg::set_error("%s: tau_max %u: tau_min (%u) .. frame_length - win_length - 1 (%u)", who, p->tau_max, p->tau_min, most);
        return AFG_ERR_INVALID;
    }
    if (p->center > 1) { afg::set_error("%s: center %u: 0 or 1", who, p->center); return AFG_ERR_INVALID; }
    if (p->pad_mode != AFG_MEL_PAD_REFLECT && p->pad_mode != AFG_MEL_PAD_ZERO) {
        afg::set_error("%s: pad_mode %u: AFG_MEL_PAD_REFLECT or AFG_MEL_PAD_ZERO", who, p->pad_mode);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->threshold) || p->threshold < 0.0f) {
        afg::set_error("%s: threshold %g: a finite value >= 0", who, (double)p->threshold);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(p->samplerate) || !(p->samplerate > 0.0)) {
        afg::set_error("%s: samplerate %g: a finite value > 0", who, p->samplerate);
        return AFG_ERR_INVALID;
    }
    if (p->reserved[0] != 0 || p->reserved[1] != 0) {
        afg::set_error("%s: reserved %u, %u: must be 0", who, p->reserved[0], p->reserved[1]);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// afg_mel_frames' formula with n_fft = frame_length (params already checked)
uint32_t afg::yin_frames_of(const afg_yin_params &p, uint32_t in_frames)
{
    const uint64_t have = (uint64_t)in_frames + 2 * (uint64_t)(p.center ? p.frame_length / 2 : 0);
    if (have < p.frame_length) return 0;
    return (uint32_t)std::min<uint64_t>(1 + (have - p.frame_length) / p.hop, 0xffffffffull);
}

extern "C" int afg_yin_lags(double samplerate, double fmin, double fmax, uint32_t frame_length, uint32_t win_length, uint32_t *tau_min,
                            uint32_t *tau_max)
{
    if (!tau_min || !tau_max) { afg::set_error("afg_yin_lags: NULL tau_min or tau_max"); return AFG_ERR_INVALID; }
    if (frame_length < 4 || frame_length > 4096) { afg::set_error("afg_yin_lags: frame_length %u: 4 .. 4096", frame_length); return AFG_ERR_INVALID; }
    if (win_length < 1 || win_length > frame_length - 2) {
        afg::set_error("afg_yin_lags: win_length %u: 1 .. frame_length - 2 (%u)", win_length, frame_length - 2);
        return AFG_ERR_INVALID;
    }
    if (!std::isfinite(samplerate) || !(samplerate > 0.0)) { afg::set_error("afg_yin_lags: samplerate %g: a finite value > 0", samplerate); return AFG_ERR_INVALID; }
    if (!std::isfinite(fmin) || !std::isfinite(fmax) || !(fmin > 0.0) || !(fmin < fmax)) {
        afg::set_error("afg_yin_lags: fmin %g, fmax %g: finite, 0 < fmin < fmax", fmin, fmax);
        return AFG_ERR_INVALID;
    }
    const double most = (double)(frame_length - win_length - 1);
    const double lo = std::floor(samplerate / fmax), hi = std::min(std::ceil(samplerate / fmin), most);
    if (lo < 1.0 || lo > hi) {
        afg::set_error("afg_yin_lags: no lag in the range: floor(samplerate / fmax) = %g, min(ceil(samplerate / fmin), frame_length - win_length - 1) = %g", lo,
                       hi);
        return AFG_ERR_INVALID;
    }
    *tau_min = (uint32_t)lo;
    *tau_max = (uint32_t)hi;
    return AFG_OK;
}

extern "C" uint32_t afg_yin_frames(const afg_yin_params *params, uint32_t in_frames)
{
    if (afg::yin_check_params(params, "afg_yin_frames")) return 0;
    return afg::yin_frames_of(*params, in_frames);
}

extern "C" uint64_t afg_yin_layout(afg_mel_row *rows, uint64_t n_rows, const afg_yin_params *params)
{
    if (afg::yin_check_params(params, "afg_yin_layout")) return 0;
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += ((uint64_t)rows[k].out_frames + AFG_YIN_TILE - 1) / AFG_YIN_TILE;
    }
    return tiles;
}

namespace {

// One launch of afg_yin_hip over rows [0, n_rows) of T samples each, contiguous in d_in, to slabs [2, n_out], contiguous in
// d_out.  The object holds the records its upload reads: it lives until `st` has drained.
struct YinPlane {
    std::vector<afg_mel_row> recs;
    afg_front::DevBuf d_recs;
    int launch(const afg_pitch_opts &o, uint32_t n_out, const float *d_in, uint64_t n_rows, float *d_out, hipStream_t st)
    {
        recs.clear();
        for (uint64_t i = 0; i < n_rows; i++) {
            afg_mel_row r;
            std::memset(&r, 0, sizeof(r));
            r.in_off = i * o.frames;
            r.in_frames = o.frames;
            r.out_off = i * 2 * n_out;
            r.out_frames = n_out;
            recs.push_back(r);
        }
        if (recs.empty()) return AFG_OK;
        const uint64_t tiles = afg_yin_layout(recs.data(), recs.size(), &o.yin);
        if (int rc = afg_front::upload_records(d_recs, recs, st)) return rc;
        return afg::yin_launch(recs.data(), recs.size(), (const afg_mel_row *)d_recs.p, tiles, &o.yin, d_in, n_rows * o.frames, d_out,
                               n_rows * 2 * n_out, st);
    }
};

}  // namespace

extern "C" int afg_batch_decode_pitch(const uint8_t *const *data, const size_t *length, int n_files, const afg_pitch_opts *opts, float *d_out,
                                      uint32_t *n_frames, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (int rc = afg_front::entry_args("afg_batch_decode_pitch", { { "opts", opts }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (opts->struct_size < sizeof(afg_pitch_opts)) {
            afg::set_error("afg_pitch_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        const afg_pitch_opts &o = *opts;
        if (o.reserved != 0) { afg::set_error("afg_pitch_opts.reserved %u: must be 0", o.reserved); return AFG_ERR_INVALID; }
        const afg_resample_opts ro = afg_front::resample_opts_of(o);
        afg_front::ResampleJob job;
        if (int rc = afg_front::resampled_check(&ro, data, length, n_files, job)) return rc;
        if (int rc = afg::yin_check_params(&o.yin, "afg_batch_decode_pitch")) return rc;
        if (o.yin.samplerate != (double)o.samplerate) {
            afg::set_error("afg_batch_decode_pitch: yin.samplerate %g, but the tensor's samplerate is %u", o.yin.samplerate, o.samplerate);
            return AFG_ERR_INVALID;
        }
        const uint32_t most = afg::yin_frames_of(o.yin, o.frames), pad = o.yin.center ? o.yin.frame_length / 2 : 0;
        if (most == 0) {
            afg::set_error("afg_batch_decode_pitch: %u samples hold no frame of frame_length %u", o.frames, o.yin.frame_length);
            return AFG_ERR_INVALID;
        }
        if (o.yin.pad_mode == AFG_MEL_PAD_REFLECT && pad && o.frames <= pad) {
            afg::set_error("afg_batch_decode_pitch: reflect padding of %u samples needs more than %u samples (frames %u)", pad, pad, o.frames);
            return AFG_ERR_INVALID;
        }
        if (o.n_out > most) {
            afg::set_error("afg_batch_decode_pitch: n_out %u, but %u samples have %u frames", o.n_out, o.frames, most);
            return AFG_ERR_INVALID;
        }
        if (n_files == 0) return AFG_OK;
        const uint32_t n_out = o.n_out ? o.n_out : most;
        const uint64_t row_out = 2 * (uint64_t)n_out;                                          // one row's slab
        const uint64_t slab_out = (uint64_t)o.channels * row_out, slab_in = (uint64_t)o.channels * o.frames;
        if (slab_out > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_pitch: a tensor of %d x %u x 2 x %u floats", n_files, o.channels, n_out);
            return AFG_ERR_INVALID;
        }
        const size_t per_list = afg_front::sublist_size(n_files, slab_in * sizeof(float), afg::kDevResampleScratchBytes);
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg::require_device()) return rc;
        YinPlane plane;                                          // (declared in front of the drain: it holds what the upload reads)
        std::vector<afg_norm_group> groups;
        afg_front::DevBuf scratch;
        afg_front::NullStreamDrain drain;
        if (int rc = scratch.alloc((size_t)(per_list * slab_in * sizeof(float)))) return rc;
        for (size_t f0 = 0; f0 < (size_t)n_files; f0 += per_list) {
            const size_t n = std::min(per_list, (size_t)n_files - f0);
            afg_resample_opts sub = ro;
            if (sub.first_frame) sub.first_frame += f0;
            // the tensor at one rate of the sublist, every element written (a failed file's slab is zero) ...
            if (int rc = afg_front::resampled_run(job, &sub, data + f0, length + f0, (int)n, (float *)scratch.p, items + f0, messages)) return rc;
            // ... its two planes: one row per file and channel ...
            float *y = d_out + f0 * slab_out;
            if (int rc = plane.launch(o, n_out, (const float *)scratch.p, n * o.channels, y, nullptr)) return rc;
            // ... and +0.0f over the frames past each file's own (the valid lengths of the normalisation's groups)
            groups.clear();
            afg_front::norm_file_groups(job, items + f0, n, o.first_frame ? o.first_frame + f0 : nullptr, groups);
            for (size_t i = 0; i < n; i++) {
                const uint32_t own = groups[i].valid ? std::min(n_out, afg::yin_frames_of(o.yin, groups[i].valid)) : 0;
                if (n_frames) n_frames[f0 + i] = own;
                if (own < n_out)
                    AFG_HIP_CHECK(hipMemset2DAsync(y + i * slab_out + own, (size_t)n_out * sizeof(float), 0, (size_t)(n_out - own) * sizeof(float),
                                                   2 * (size_t)o.channels, nullptr));
                if (items[f0 + i].pcm) items[f0 + i].pcm = y + i * slab_out;
            }
            AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
        }
        return res.finish(out);
    });
}
