// afg_melspec.cpp -- the host half of the mel spectrogram features (afg_stage.h: MelTables, MelPlane): the basis and the
// filter bank of include/afg.h's definition, computed in double and kept per parameter set, and afg_batch_decode_mel -- the
// resampled tensor into a pooled scratch, then one afg_melspec_hip (or, by afg_mel_opts.algorithm, afg_melspec_fft_hip,
// whose window and twiddle table is made and kept here too) launch per sublist, with the optional normalisations of
// afg_batch_decode_mel_norm around it.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

namespace {

bool basis_shape_ok(uint32_t n_fft, uint32_t win_length)
{
    if (n_fft < 16 || n_fft > 2048) { afg::set_error("afg_mel_basis: n_fft %u: 16 .. 2048", n_fft); return false; }
    if (win_length < 1 || win_length > n_fft) { afg::set_error("afg_mel_basis: win_length %u: 1 .. n_fft (%u)", win_length, n_fft); return false; }
    return true;
}

uint32_t nb16_of(uint32_t n_fft) { return (n_fft / 2 + 1 + 15) & ~15u; }

void fill_basis(float *out, uint32_t n_fft, uint32_t win)
{
    const uint32_t n_bins = n_fft / 2 + 1, nb16 = nb16_of(n_fft), ld = 2 * nb16, n_lo = (n_fft - win) / 2;
    std::memset(out, 0, (size_t)win * ld * sizeof(float));      // the padding columns: +0.0f
    for (uint32_t j = 0; j < win; j++) {
        const double w = 0.5 - 0.5 * std::cos(2.0 * afg::kPi * (double)j / (double)win);
        float *row = out + (size_t)j * ld;
        for (uint32_t k = 0; k < n_bins; k++) {
            const double a = 2.0 * afg::kPi * (double)(((uint64_t)(n_lo + j) * k) % n_fft) / (double)n_fft;
            row[k] = (float)(w * std::cos(a));
            row[nb16 + k] = (float)(-w * std::sin(a));
        }
    }
}

bool fft_shape_ok(uint32_t n_fft, uint32_t win_length)
{
    if (n_fft < 16 || n_fft > 2048) { afg::set_error("afg_mel_fft_tables: n_fft %u: 16 .. 2048", n_fft); return false; }
    if (win_length < 1 || win_length > n_fft) { afg::set_error("afg_mel_fft_tables: win_length %u: 1 .. n_fft (%u)", win_length, n_fft); return false; }
    if (!afg::mel_fft_n_ok(n_fft)) {
        afg::set_error("afg_mel_fft_tables: n_fft %u: the FFT path takes 16 .. 2048 with prime factors 2, 3 and 5 only", n_fft);
        return false;
    }
    return true;
}

// the window, then n_fft pairs (cos, -sin) of 2 pi j / n_fft
void fill_fft_tables(float *out, uint32_t n_fft, uint32_t win)
{
    for (uint32_t j = 0; j < win; j++) out[j] = (float)(0.5 - 0.5 * std::cos(2.0 * afg::kPi * (double)j / (double)win));
    for (uint32_t j = 0; j < n_fft; j++) {
        const double a = 2.0 * afg::kPi * (double)j / (double)n_fft;
        out[win + 2 * j] = (float)std::cos(a);
        out[win + 2 * j + 1] = (float)(-std::sin(a));
    }
}

double hz_to_mel(double f, uint32_t scale)
{
    if (scale == AFG_MEL_SCALE_HTK) return 2595.0 * std::log10(1.0 + f / 700.0);
    return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + 27.0 * std::log(f / 1000.0) / std::log(6.4);
}

double mel_to_hz(double m, uint32_t scale)
{
    if (scale == AFG_MEL_SCALE_HTK) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * std::exp(std::log(6.4) * (m - 15.0) / 27.0);
}

bool filters_shape_ok(uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double f_min, double *f_max, uint32_t scale, uint32_t norm)
{
    if (samplerate == 0) { afg::set_error("afg_mel_filters: a sample rate of 0"); return false; }
    if (n_fft < 16 || n_fft > 2048) { afg::set_error("afg_mel_filters: n_fft %u: 16 .. 2048", n_fft); return false; }
    if (n_mels < 1 || n_mels > 256) { afg::set_error("afg_mel_filters: n_mels %u: 1 .. 256", n_mels); return false; }
    if (scale != AFG_MEL_SCALE_SLANEY && scale != AFG_MEL_SCALE_HTK) { afg::set_error("afg_mel_filters: scale %u: AFG_MEL_SCALE_SLANEY or AFG_MEL_SCALE_HTK", scale); return false; }
    if (norm != AFG_MEL_NORM_NONE && norm != AFG_MEL_NORM_SLANEY) { afg::set_error("afg_mel_filters: norm %u: AFG_MEL_NORM_NONE or AFG_MEL_NORM_SLANEY", norm); return false; }
    if (*f_max == 0.0) *f_max = (double)samplerate / 2.0;
    if (!(f_min >= 0.0) || !(f_min < *f_max) || !(*f_max <= (double)samplerate / 2.0)) {
        afg::set_error("afg_mel_filters: f_min %g, f_max %g: 0 <= f_min < f_max <= samplerate / 2 (%g)", f_min, *f_max, (double)samplerate / 2.0);
        return false;
    }
    return true;
}

void fill_filters(float *out, uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double f_min, double f_max, uint32_t scale, uint32_t norm)
{
    const uint32_t n_bins = n_fft / 2 + 1;
    const double lo = hz_to_mel(f_min, scale), hi = hz_to_mel(f_max, scale);
    std::vector<double> f((size_t)n_mels + 2);
    for (uint32_t i = 0; i < n_mels + 2; i++) f[i] = mel_to_hz(lo + (hi - lo) * (double)i / (double)(n_mels + 1), scale);
    for (uint32_t m = 0; m < n_mels; m++) {
        const double gain = norm == AFG_MEL_NORM_SLANEY ? 2.0 / (f[m + 2] - f[m]) : 1.0;
        for (uint32_t k = 0; k < n_bins; k++) {
            const double fk = (double)k * (double)samplerate / (double)n_fft;
            const double up = (fk - f[m]) / (f[m + 1] - f[m]), down = (f[m + 2] - fk) / (f[m + 2] - f[m + 1]);
            out[(size_t)m * n_bins + k] = (float)(std::max(0.0, std::min(up, down)) * gain);
        }
    }
}

}  // namespace

extern "C" uint64_t afg_mel_basis(uint32_t n_fft, uint32_t win_length, float *out, uint64_t cap)
{
    if (!basis_shape_ok(n_fft, win_length)) return 0;
    const uint64_t need = (uint64_t)win_length * 2 * nb16_of(n_fft);
    if (out && cap >= need) fill_basis(out, n_fft, win_length);
    return need;
}

extern "C" uint64_t afg_mel_filters(uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double f_min, double f_max, uint32_t scale,
                                    uint32_t norm, float *out, uint64_t cap)
{
    if (!filters_shape_ok(samplerate, n_fft, n_mels, f_min, &f_max, scale, norm)) return 0;
    const uint64_t need = (uint64_t)n_mels * (n_fft / 2 + 1);
    if (out && cap >= need) fill_filters(out, samplerate, n_fft, n_mels, f_min, f_max, scale, norm);
    return need;
}

extern "C" uint64_t afg_mel_fft_tables(uint32_t n_fft, uint32_t win_length, float *out, uint64_t cap)
{
    if (!fft_shape_ok(n_fft, win_length)) return 0;
    const uint64_t need = (uint64_t)win_length + 2 * (uint64_t)n_fft;
    if (out && cap >= need) fill_fft_tables(out, n_fft, win_length);
    return need;
}

namespace afg_front {

int mel_tables(const afg_mel_opts &o, MelTables &t)
{
    static std::mutex mu;
    static std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::shared_ptr<const std::vector<float>>> bases;   // (algorithm, n_fft, win_length)
    static std::map<std::tuple<uint32_t, uint32_t, uint32_t, double, double, uint32_t, uint32_t>, std::shared_ptr<const std::vector<float>>> banks;
    double f_max = o.f_max;
    const bool fft = o.algorithm == AFG_MEL_ALGO_FFT;
    if (!basis_shape_ok(o.mel.n_fft, o.mel.win_length)) return AFG_ERR_INVALID;
    if (fft && !fft_shape_ok(o.mel.n_fft, o.mel.win_length)) return AFG_ERR_UNSUPPORTED;
    if (!filters_shape_ok(o.samplerate, o.mel.n_fft, o.mel.n_mels, o.f_min, &f_max, o.scale, o.norm)) return AFG_ERR_INVALID;
    std::lock_guard<std::mutex> lk(mu);
    const auto bkey = std::make_tuple(o.algorithm, o.mel.n_fft, o.mel.win_length);
    auto b = bases.find(bkey);
    if (b == bases.end()) {
        auto v = std::make_shared<std::vector<float>>(fft ? (size_t)o.mel.win_length + 2 * (size_t)o.mel.n_fft
                                                          : (size_t)o.mel.win_length * 2 * nb16_of(o.mel.n_fft));
        if (fft) fill_fft_tables(v->data(), o.mel.n_fft, o.mel.win_length);
        else fill_basis(v->data(), o.mel.n_fft, o.mel.win_length);
        b = bases.emplace(bkey, std::move(v)).first;
    }
    const auto fkey = std::make_tuple(o.samplerate, o.mel.n_fft, o.mel.n_mels, o.f_min, f_max, o.scale, o.norm);
    auto f = banks.find(fkey);
    if (f == banks.end()) {
        auto v = std::make_shared<std::vector<float>>((size_t)o.mel.n_mels * (o.mel.n_fft / 2 + 1));
        fill_filters(v->data(), o.samplerate, o.mel.n_fft, o.mel.n_mels, o.f_min, f_max, o.scale, o.norm);
        f = banks.emplace(fkey, std::move(v)).first;
    }
    t.basis = b->second;
    t.filters = f->second;
    return AFG_OK;
}

int MelPlane::launch(const afg_mel_opts &o, const MelTables &t, const float *d_in, uint64_t n_rows, float *d_out, hipStream_t st)
{
    const uint32_t n_out = o.n_out ? o.n_out : afg_mel_frames(&o.mel, o.frames);
    const uint64_t slab = (uint64_t)o.mel.n_mels * n_out;
    recs.clear();                                                // the upload's source lives as long as the object
    for (uint64_t i = 0; i < n_rows; i++) {
        afg_mel_row r;
        std::memset(&r, 0, sizeof(r));
        r.in_off = i * o.frames;
        r.in_frames = o.frames;
        r.out_off = i * slab;
        r.out_frames = n_out;
        recs.push_back(r);
    }
    if (recs.empty()) return AFG_OK;
    const bool fft = o.algorithm == AFG_MEL_ALGO_FFT;
    const uint64_t tiles = fft ? afg_mel_fft_layout(recs.data(), recs.size(), &o.mel) : afg_mel_layout(recs.data(), recs.size(), &o.mel);
    if (!tables_up) {                                            // (the tables live as long as the process: mel_tables)
        if (int rc = d_basis.alloc(t.basis->size() * sizeof(float))) return rc;
        if (int rc = d_filters.alloc(t.filters->size() * sizeof(float))) return rc;
        AFG_HIP_CHECK(hipMemcpyAsync(d_basis.p, t.basis->data(), t.basis->size() * sizeof(float), hipMemcpyHostToDevice, st));
        AFG_HIP_CHECK(hipMemcpyAsync(d_filters.p, t.filters->data(), t.filters->size() * sizeof(float), hipMemcpyHostToDevice, st));
        tables_up = true;
    }
    if (int rc = upload_records(d_recs, recs, st)) return rc;
    if (fft)
        return afg::melspec_fft_launch(recs.data(), recs.size(), (const afg_mel_row *)d_recs.p, tiles, &o.mel, d_in, n_rows * o.frames,
                                       (const float *)d_basis.p, t.basis->size(), (const float *)d_filters.p, t.filters->size(), d_out,
                                       n_rows * slab, st);
    return afg::melspec_launch(recs.data(), recs.size(), (const afg_mel_row *)d_recs.p, tiles, &o.mel, d_in, n_rows * o.frames,
                               (const float *)d_basis.p, t.basis->size(), (const float *)d_filters.p, t.filters->size(), d_out,
                               n_rows * slab, st);
}

}  // namespace afg_front

// afg_batch_decode_mel, and with wave_norm / feat_norm afg_batch_decode_mel_norm: the tensor at one rate of a sublist,
// normalised in place per file; its features; those normalised in place per slab
int afg_front::mel_batch(const uint8_t *const *data, const size_t *length, int n_files, const afg_mel_opts *opts, const afg_norm_params *wave_norm,
                         const afg_norm_params *feat_norm, float *d_out, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (int rc = entry_args("afg_batch_decode_mel", { { "opts", opts }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (opts->struct_size < sizeof(afg_mel_opts)) {
            afg::set_error("afg_mel_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        const afg_mel_opts &o = *opts;
        if (o.algorithm != AFG_MEL_ALGO_DIRECT && o.algorithm != AFG_MEL_ALGO_FFT) {
            afg::set_error("afg_mel_opts.algorithm %u: AFG_MEL_ALGO_DIRECT or AFG_MEL_ALGO_FFT", o.algorithm);
            return AFG_ERR_INVALID;
        }
        if (o.reserved != 0) { afg::set_error("afg_mel_opts.reserved %u: must be 0", o.reserved); return AFG_ERR_INVALID; }
        const afg_resample_opts ro = resample_opts_of(o);
        afg_front::ResampleJob job;
        if (int rc = afg_front::resampled_check(&ro, data, length, n_files, job)) return rc;
        if (int rc = afg_mel_check_rows(nullptr, 0, 0, &o.mel, 0, 0, 0, 0)) return rc;       // the mel parameters alone
        if (o.algorithm == AFG_MEL_ALGO_FFT)
            if (int rc = afg_mel_fft_check_rows(nullptr, 0, 0, &o.mel, 0, 0, 0, 0)) return rc;   // and the n_fft that path takes
        afg_front::MelTables tables;
        if (int rc = afg_front::mel_tables(o, tables)) return rc;
        const uint32_t most = afg_mel_frames(&o.mel, o.frames), pad = o.mel.center ? o.mel.n_fft / 2 : 0;
        if (most == 0) {
            afg::set_error("afg_batch_decode_mel: %u samples hold no frame of n_fft %u", o.frames, o.mel.n_fft);
            return AFG_ERR_INVALID;
        }
        if (o.n_out > most) {
            afg::set_error("afg_batch_decode_mel: n_out %u, but %u samples have %u frames", o.n_out, o.frames, most);
            return AFG_ERR_INVALID;
        }
        if (o.mel.pad_mode == AFG_MEL_PAD_REFLECT && pad && o.frames <= pad) {
            afg::set_error("afg_batch_decode_mel: reflect padding of %u samples needs more than %u samples (frames is %u)", pad, pad, o.frames);
            return AFG_ERR_INVALID;
        }
        if (wave_norm)
            if (int rc = afg_norm_check_groups(nullptr, 0, 0, wave_norm, 0, 0)) return rc;
        if (feat_norm)
            if (int rc = afg_norm_check_groups(nullptr, 0, 0, feat_norm, 0, 0)) return rc;
        if (feat_norm && (uint64_t)o.mel.n_mels * (o.n_out ? o.n_out : most) > 0xffffffffull) {
            afg::set_error("afg_batch_decode_mel_norm: a slab of %u x %u floats is more than a group's row holds", o.mel.n_mels, o.n_out ? o.n_out : most);
            return AFG_ERR_INVALID;
        }
        if (n_files == 0) return AFG_OK;
        const uint32_t n_out = o.n_out ? o.n_out : most;
        const uint64_t slab_out = (uint64_t)o.channels * o.mel.n_mels * n_out, slab_in = (uint64_t)o.channels * o.frames;
        if (slab_out > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_mel: a tensor of %d x %u x %u x %u floats", n_files, o.channels, o.mel.n_mels, n_out);
            return AFG_ERR_INVALID;
        }
        const size_t per_list = afg_front::sublist_size(n_files, slab_in * sizeof(float), afg::kDevMelScratchBytes);
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg::require_device()) return rc;
        afg_front::MelPlane plane;                               // (declared in front of the drain: it holds what the uploads read)
        afg_front::NormPlane wave, feat;
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
            if (wave_norm) {                                     // ... every file's rows as one group, over its own samples ...
                groups.clear();
                afg_front::norm_file_groups(job, items + f0, n, o.first_frame ? o.first_frame + f0 : nullptr, groups);
                if (int rc = wave.launch(*wave_norm, groups, (float *)scratch.p, n * slab_in, nullptr, nullptr)) return rc;
            }
            // ... and its features: one row per file and channel
            float *y = d_out + f0 * slab_out;
            if (int rc = plane.launch(o, tables, (const float *)scratch.p, n * o.channels, y, nullptr)) return rc;
            if (feat_norm) {                                     // every slab one group of a single row
                groups.clear();
                afg_norm_group g;
                std::memset(&g, 0, sizeof(g));
                g.rows = 1;
                g.valid = (uint32_t)((uint64_t)o.mel.n_mels * n_out);
                g.stride = g.valid;
                for (uint64_t k = 0; k < n * o.channels; k++) {
                    g.in_off = g.out_off = k * g.valid;
                    groups.push_back(g);
                }
                if (int rc = feat.launch(*feat_norm, groups, y, n * slab_out, nullptr, nullptr)) return rc;
            }
            for (size_t i = 0; i < n; i++)
                if (items[f0 + i].pcm) items[f0 + i].pcm = y + i * slab_out;
            AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
        }
        return res.finish(out);
    });
}

extern "C" int afg_batch_decode_mel(const uint8_t *const *data, const size_t *length, int n_files, const afg_mel_opts *opts, float *d_out,
                                    afg_batch_result *out)
{
    return afg_front::mel_batch(data, length, n_files, opts, nullptr, nullptr, d_out, out);
}

extern "C" int afg_batch_decode_mel_norm(const uint8_t *const *data, const size_t *length, int n_files, const afg_mel_opts *opts,
                                         const afg_norm_params *wave_norm, const afg_norm_params *feat_norm, float *d_out, afg_batch_result *out)
{
    return afg_front::mel_batch(data, length, n_files, opts, wave_norm, feat_norm, d_out, out);
}
