// afg_fbank.cpp -- the host half of the Kaldi-compatible filter-bank features (csrc/fbank.hip): afg_fbank_n_fft, the window
// and twiddle table and the mel-axis bank of include/afg.h's definition, computed in double and kept per parameter set, and
// afg_batch_decode_fbank -- the resampled tensor of a sublist into the pooled scratch the mel entry uses (afg_dev_option
// "mel_scratch_bytes"), then one afg_fbank_hip launch over its rows, one per file and channel, and the frames each file's own
// samples give.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

namespace {

typedef std::shared_ptr<const std::vector<float>> Table;

bool tables_shape_ok(uint32_t window_type, uint32_t win, uint32_t n_fft, double blackman_coeff)
{
    if (window_type > AFG_FBANK_WINDOW_RECTANGULAR) {
        afg::set_error("afg_fbank_tables: window_type %u: AFG_FBANK_WINDOW_POVEY .. AFG_FBANK_WINDOW_RECTANGULAR", window_type);
        return false;
    }
    if (win < 2 || win > 2048) { afg::set_error("afg_fbank_tables: win_length %u: 2 .. 2048", win); return false; }
    if (n_fft < win || n_fft > 2048) { afg::set_error("afg_fbank_tables: n_fft %u: win_length (%u) .. 2048", n_fft, win); return false; }
    if (!std::isfinite(blackman_coeff)) { afg::set_error("afg_fbank_tables: blackman_coeff is not finite"); return false; }
    if (!afg::mel_fft_n_ok(n_fft)) {
        afg::set_error("afg_fbank_tables: n_fft %u: the transform takes 16 .. 2048 with prime factors 2, 3 and 5 only", n_fft);
        return false;
    }
    return true;
}

// the window, then n_fft pairs (cos, -sin) of 2 pi j / n_fft (afg_mel_fft_tables' expressions)
void fill_tables(float *out, uint32_t window_type, uint32_t win, uint32_t n_fft, double b)
{
    for (uint32_t j = 0; j < win; j++) {
        const double a = 2.0 * afg::kPi * (double)j / (double)(win - 1);
        double w = 1.0;
        switch (window_type) {
        case AFG_FBANK_WINDOW_POVEY: w = std::pow(0.5 - 0.5 * std::cos(a), 0.85); break;
        case AFG_FBANK_WINDOW_HAMMING: w = 0.54 - 0.46 * std::cos(a); break;
        case AFG_FBANK_WINDOW_HANNING: w = 0.5 - 0.5 * std::cos(a); break;
        case AFG_FBANK_WINDOW_BLACKMAN: w = b - 0.5 * std::cos(a) + (0.5 - b) * std::cos(2.0 * a); break;
        default: break;
        }
        out[j] = (float)w;
    }
    for (uint32_t j = 0; j < n_fft; j++) {
        const double a = 2.0 * afg::kPi * (double)j / (double)n_fft;
        out[win + 2 * j] = (float)std::cos(a);
        out[win + 2 * j + 1] = (float)(-std::sin(a));
    }
}

double mel_of(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

// (high_freq <= 0 becomes the offset from Nyquist it stands for)
bool filters_shape_ok(uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double low, double *high)
{
    if (samplerate == 0) { afg::set_error("afg_fbank_filters: a sample rate of 0"); return false; }
    if (n_fft < 2 || n_fft > 2048) { afg::set_error("afg_fbank_filters: n_fft %u: 2 .. 2048", n_fft); return false; }
    if (n_mels < 1 || n_mels > 256) { afg::set_error("afg_fbank_filters: n_mels %u: 1 .. 256", n_mels); return false; }
    const double nyquist = (double)samplerate / 2.0;
    if (*high <= 0.0) *high += nyquist;
    if (!(low >= 0.0) || !(low < *high) || !(*high <= nyquist)) {
        afg::set_error("afg_fbank_filters: low_freq %g, high_freq %g: 0 <= low_freq < high_freq <= samplerate / 2 (%g)", low, *high, nyquist);
        return false;
    }
    return true;
}

void fill_filters(float *out, uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double low, double high)
{
    const uint32_t n_bins = n_fft / 2 + 1;
    const double m_lo = mel_of(low), delta = (mel_of(high) - m_lo) / (double)(n_mels + 1);
    for (uint32_t m = 0; m < n_mels; m++) {
        const double left = m_lo + (double)m * delta, centre = m_lo + (double)(m + 1) * delta, right = m_lo + (double)(m + 2) * delta;
        for (uint32_t k = 0; k < n_bins; k++) {
            const double mk = mel_of((double)k * (double)samplerate / (double)n_fft);
            const double up = (mk - left) / (centre - left), down = (right - mk) / (right - centre);
            out[(size_t)m * n_bins + k] = (float)std::max(0.0, std::min(up, down));
        }
        if ((n_fft & 1) == 0) out[(size_t)m * n_bins + n_fft / 2] = 0.0f;   // the Nyquist bin
    }
}

struct FbankTables { Table table, bank; };

// (the shapes already checked)
void tables_of(const afg_fbank_opts &o, double high, FbankTables &t)
{
    static std::mutex mu;
    static std::map<std::tuple<uint32_t, uint32_t, uint32_t, double>, Table> tables;   // (window, win_length, n_fft, blackman_coeff)
    static std::map<std::tuple<uint32_t, uint32_t, uint32_t, double, double>, Table> banks;
    std::lock_guard<std::mutex> lk(mu);
    const afg_fbank_params &p = o.fbank;
    const double b = o.window_type == AFG_FBANK_WINDOW_BLACKMAN ? o.blackman_coeff : 0.0;
    const auto tkey = std::make_tuple(o.window_type, p.win_length, p.n_fft, b);
    auto it = tables.find(tkey);
    if (it == tables.end()) {
        auto v = std::make_shared<std::vector<float>>((size_t)p.win_length + 2 * (size_t)p.n_fft);
        fill_tables(v->data(), o.window_type, p.win_length, p.n_fft, b);
        it = tables.emplace(tkey, std::move(v)).first;
    }
    const auto fkey = std::make_tuple(o.samplerate, p.n_fft, p.n_mels, o.low_freq, high);
    auto f = banks.find(fkey);
    if (f == banks.end()) {
        auto v = std::make_shared<std::vector<float>>((size_t)p.n_mels * (p.n_fft / 2 + 1));
        fill_filters(v->data(), o.samplerate, p.n_fft, p.n_mels, o.low_freq, high);
        f = banks.emplace(fkey, std::move(v)).first;
    }
    t.table = it->second;
    t.bank = f->second;
}

// One launch of afg_fbank_hip over rows [0, n_rows) of T samples each, contiguous in d_in, to slabs of `slab` floats,
// contiguous in d_out.  The object holds the records its upload reads and the tables on the device (uploaded on the first
// launch): it lives until `st` has drained.
struct FbankPlane {
    std::vector<afg_mel_row> recs;
    afg_front::DevBuf d_recs, d_table, d_bank;
    bool tables_up = false;
    int launch(const afg_fbank_opts &o, const FbankTables &t, uint32_t n_out, uint64_t slab, const float *d_in, uint64_t n_rows, float *d_out,
               hipStream_t st)
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
        const uint64_t tiles = afg_fbank_layout(recs.data(), recs.size(), &o.fbank);
        if (!tables_up) {                                        // (the tables live as long as the process: tables_of)
            if (int rc = d_table.alloc(t.table->size() * sizeof(float))) return rc;
            if (int rc = d_bank.alloc(t.bank->size() * sizeof(float))) return rc;
            AFG_HIP_CHECK(hipMemcpyAsync(d_table.p, t.table->data(), t.table->size() * sizeof(float), hipMemcpyHostToDevice, st));
            AFG_HIP_CHECK(hipMemcpyAsync(d_bank.p, t.bank->data(), t.bank->size() * sizeof(float), hipMemcpyHostToDevice, st));
            tables_up = true;
        }
        if (int rc = afg_front::upload_records(d_recs, recs, st)) return rc;
        return afg::fbank_launch(recs.data(), recs.size(), (const afg_mel_row *)d_recs.p, tiles, &o.fbank, d_in, n_rows * o.frames,
                                 (const float *)d_table.p, t.table->size(), (const float *)d_bank.p, t.bank->size(), d_out, n_rows * slab, st);
    }
};

}  // namespace

extern "C" uint32_t afg_fbank_n_fft(uint32_t win_length, uint32_t round_pow2)
{
    if (win_length < 2 || win_length > 2048) { afg::set_error("afg_fbank_n_fft: win_length %u: 2 .. 2048", win_length); return 0; }
    if (!round_pow2) return win_length;
    uint32_t n = 2;
    while (n < win_length) n <<= 1;
    return n;
}

extern "C" uint64_t afg_fbank_tables(uint32_t window_type, uint32_t win_length, uint32_t n_fft, double blackman_coeff, float *out, uint64_t cap)
{
    if (!tables_shape_ok(window_type, win_length, n_fft, blackman_coeff)) return 0;
    const uint64_t need = (uint64_t)win_length + 2 * (uint64_t)n_fft;
    if (out && cap >= need) fill_tables(out, window_type, win_length, n_fft, blackman_coeff);
    return need;
}

extern "C" uint64_t afg_fbank_filters(uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double low_freq, double high_freq, float *out,
                                      uint64_t cap)
{
    if (!filters_shape_ok(samplerate, n_fft, n_mels, low_freq, &high_freq)) return 0;
    const uint64_t need = (uint64_t)n_mels * (n_fft / 2 + 1);
    if (out && cap >= need) fill_filters(out, samplerate, n_fft, n_mels, low_freq, high_freq);
    return need;
}

extern "C" int afg_batch_decode_fbank(const uint8_t *const *data, const size_t *length, int n_files, const afg_fbank_opts *opts, float *d_out,
                                      uint32_t *n_frames, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (int rc = afg_front::entry_args("afg_batch_decode_fbank", { { "opts", opts }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (opts->struct_size < sizeof(afg_fbank_opts)) {
            afg::set_error("afg_fbank_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        const afg_fbank_opts &o = *opts;
        if (o.reserved != 0) { afg::set_error("afg_fbank_opts.reserved %u: must be 0", o.reserved); return AFG_ERR_INVALID; }
        const afg_resample_opts ro = afg_front::resample_opts_of(o);
        afg_front::ResampleJob job;
        if (int rc = afg_front::resampled_check(&ro, data, length, n_files, job)) return rc;
        if (int rc = afg::fbank_check_params(&o.fbank, "afg_batch_decode_fbank")) return rc;   // the parameters alone
        if (!tables_shape_ok(o.window_type, o.fbank.win_length, o.fbank.n_fft, o.blackman_coeff)) return AFG_ERR_INVALID;
        double high = o.high_freq;
        if (!filters_shape_ok(o.samplerate, o.fbank.n_fft, o.fbank.n_mels, o.low_freq, &high)) return AFG_ERR_INVALID;
        FbankTables tables;
        tables_of(o, high, tables);
        const uint32_t most = afg_fbank_frames(&o.fbank, o.frames);
        if (most == 0) {
            afg::set_error("afg_batch_decode_fbank: %u samples hold no frame of win_length %u", o.frames, o.fbank.win_length);
            return AFG_ERR_INVALID;
        }
        if (o.n_out > most) {
            afg::set_error("afg_batch_decode_fbank: n_out %u, but %u samples have %u frames", o.n_out, o.frames, most);
            return AFG_ERR_INVALID;
        }
        if (n_files == 0) return AFG_OK;
        const uint32_t n_out = o.n_out ? o.n_out : most, cols = o.fbank.n_mels + (o.fbank.use_energy ? 1 : 0);
        const uint64_t row_out = (uint64_t)cols * n_out;                                       // one row's slab
        const uint64_t slab_out = (uint64_t)o.channels * row_out, slab_in = (uint64_t)o.channels * o.frames;
        if (row_out > (((uint64_t)1 << 62) / o.channels) || slab_out > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_fbank: a tensor of %d x %u x %u x %u floats", n_files, o.channels, n_out, cols);
            return AFG_ERR_INVALID;
        }
        const size_t per_list = afg_front::sublist_size(n_files, slab_in * sizeof(float), afg::kDevMelScratchBytes);
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg::require_device()) return rc;
        FbankPlane plane;                                        // (declared in front of the drain: it holds what the uploads read)
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
            // ... its features: one row per file and channel ...
            float *y = d_out + f0 * slab_out;
            if (int rc = plane.launch(o, tables, n_out, row_out, (const float *)scratch.p, n * o.channels, y, nullptr)) return rc;
            // ... and the frames each file's own samples give (the valid lengths of the normalisation's groups)
            if (n_frames) {
                groups.clear();
                afg_front::norm_file_groups(job, items + f0, n, o.first_frame ? o.first_frame + f0 : nullptr, groups);
                for (size_t i = 0; i < n; i++) n_frames[f0 + i] = std::min(n_out, afg_fbank_frames(&o.fbank, groups[i].valid));
            }
            for (size_t i = 0; i < n; i++)
                if (items[f0 + i].pcm) items[f0 + i].pcm = y + i * slab_out;
            AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
        }
        return res.finish(out);
    });
}
