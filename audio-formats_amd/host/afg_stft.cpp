// afg_stft.cpp -- afg_batch_decode_stft: the resampled tensor of a sublist into the pooled scratch the mel entry uses
// (afg_dev_option "mel_scratch_bytes"), then one afg_stft_hip launch (csrc/stft.hip) over its rows, one per file and channel.
// The window and twiddle table is afg_mel_fft_tables', made once per (n_fft, win_length) and kept for the process.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

namespace {

typedef std::shared_ptr<const std::vector<float>> Table;

// (n_fft and win_length already checked: afg_stft_check_rows)
int table_of(const afg_stft_params &p, Table &t)
{
    static std::mutex mu;
    static std::map<std::pair<uint32_t, uint32_t>, Table> tables;                   // (n_fft, win_length)
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(p.n_fft, p.win_length);
    auto it = tables.find(key);
    if (it == tables.end()) {
        auto v = std::make_shared<std::vector<float>>((size_t)p.win_length + 2 * (size_t)p.n_fft);
        if (afg_mel_fft_tables(p.n_fft, p.win_length, v->data(), v->size()) != v->size()) return AFG_ERR_INVALID;
        it = tables.emplace(key, std::move(v)).first;
    }
    t = it->second;
    return AFG_OK;
}

// One launch of afg_stft_hip over rows [0, n_rows) of T samples each, contiguous in d_in, to slabs of `slab` floats,
// contiguous in d_out.  The object holds the records its upload reads and the table on the device (uploaded on the first
// launch): it lives until `st` has drained.
struct StftPlane {
    std::vector<afg_mel_row> recs;
    afg_front::DevBuf d_recs, d_table;
    bool table_up = false;
    int launch(const afg_stft_opts &o, const Table &t, uint32_t n_out, uint64_t slab, const float *d_in, uint64_t n_rows, float *d_out, hipStream_t st)
    {
        recs.clear();
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
        const uint64_t tiles = afg_stft_layout(recs.data(), recs.size(), &o.stft);
        if (!table_up) {                                         // (the table lives as long as the process: table_of)
            if (int rc = d_table.alloc(t->size() * sizeof(float))) return rc;
            AFG_HIP_CHECK(hipMemcpyAsync(d_table.p, t->data(), t->size() * sizeof(float), hipMemcpyHostToDevice, st));
            table_up = true;
        }
        if (int rc = afg_front::upload_records(d_recs, recs, st)) return rc;
        return afg::stft_launch(recs.data(), recs.size(), (const afg_mel_row *)d_recs.p, tiles, &o.stft, d_in, n_rows * o.frames,
                                (const float *)d_table.p, t->size(), d_out, n_rows * slab, st);
    }
};

}  // namespace

extern "C" int afg_batch_decode_stft(const uint8_t *const *data, const size_t *length, int n_files, const afg_stft_opts *opts, float *d_out,
                                     afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (int rc = afg_front::entry_args("afg_batch_decode_stft", { { "opts", opts }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (opts->struct_size < sizeof(afg_stft_opts)) {
            afg::set_error("afg_stft_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        const afg_stft_opts &o = *opts;
        if (o.reserved != 0) { afg::set_error("afg_stft_opts.reserved %u: must be 0", o.reserved); return AFG_ERR_INVALID; }
        const afg_resample_opts ro = afg_front::resample_opts_of(o);
        afg_front::ResampleJob job;
        if (int rc = afg_front::resampled_check(&ro, data, length, n_files, job)) return rc;
        if (int rc = afg_stft_check_rows(nullptr, 0, 0, &o.stft, 0, 0, 0)) return rc;        // the parameters alone
        Table table;
        if (int rc = table_of(o.stft, table)) return rc;
        const uint32_t most = afg::stft_frames(o.stft, o.frames), pad = o.stft.center ? o.stft.n_fft / 2 : 0;
        if (most == 0) {
            afg::set_error("afg_batch_decode_stft: %u samples hold no frame of n_fft %u", o.frames, o.stft.n_fft);
            return AFG_ERR_INVALID;
        }
        if (o.n_out > most) {
            afg::set_error("afg_batch_decode_stft: n_out %u, but %u samples have %u frames", o.n_out, o.frames, most);
            return AFG_ERR_INVALID;
        }
        if (o.stft.pad_mode == AFG_MEL_PAD_REFLECT && pad && o.frames <= pad) {
            afg::set_error("afg_batch_decode_stft: reflect padding of %u samples needs more than %u samples (frames is %u)", pad, pad, o.frames);
            return AFG_ERR_INVALID;
        }
        if (n_files == 0) return AFG_OK;
        const uint32_t n_out = o.n_out ? o.n_out : most, comps = o.stft.out_kind == AFG_STFT_COMPLEX ? 2 : 1;
        const uint64_t row_out = (uint64_t)comps * (o.stft.n_fft / 2 + 1) * n_out;           // one row's slab
        const uint64_t slab_out = (uint64_t)o.channels * row_out, slab_in = (uint64_t)o.channels * o.frames;
        if (row_out > (((uint64_t)1 << 62) / o.channels) || slab_out > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_stft: a tensor of %d x %u x %u x %u floats", n_files, o.channels, comps * (o.stft.n_fft / 2 + 1), n_out);
            return AFG_ERR_INVALID;
        }
        const size_t per_list = afg_front::sublist_size(n_files, slab_in * sizeof(float), afg::kDevMelScratchBytes);
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg::require_device()) return rc;
        StftPlane plane;                                         // (declared in front of the drain: it holds what the uploads read)
        afg_front::DevBuf scratch;
        afg_front::NullStreamDrain drain;
        if (int rc = scratch.alloc((size_t)(per_list * slab_in * sizeof(float)))) return rc;
        for (size_t f0 = 0; f0 < (size_t)n_files; f0 += per_list) {
            const size_t n = std::min(per_list, (size_t)n_files - f0);
            afg_resample_opts sub = ro;
            if (sub.first_frame) sub.first_frame += f0;
            // the tensor at one rate of the sublist, every element written (a failed file's slab is zero) ...
            if (int rc = afg_front::resampled_run(job, &sub, data + f0, length + f0, (int)n, (float *)scratch.p, items + f0, messages)) return rc;
            // ... and its spectra: one row per file and channel
            float *y = d_out + f0 * slab_out;
            if (int rc = plane.launch(o, table, n_out, row_out, (const float *)scratch.p, n * o.channels, y, nullptr)) return rc;
            for (size_t i = 0; i < n; i++)
                if (items[f0 + i].pcm) items[f0 + i].pcm = y + i * slab_out;
            AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
        }
        return res.finish(out);
    });
}
