// afg_resample.cpp -- the host half of the tensor at one sample rate (afg_stage.h: ResampleJob, ResampleTable,
// ResamplePlane): the filter tables of include/afg.h's definition, computed in double and kept per rate pair, and the
// records of the one afg_resample_hip launch that follows a collate pass.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>

namespace {

constexpr double kRolloff = 0.99;
constexpr uint64_t kMaxTable = (uint64_t)1 << 22;

// W of a rate pair that does filter: ceil(Z / fc) with fc = 0.99 * min(1, L / M)
uint32_t width_of(double fc, uint32_t Z, bool *fits)
{
    const double w = std::ceil((double)Z / fc);
    *fits = w < 4294967296.0;
    return *fits ? (uint32_t)w : 0;
}

// M, L, W of (in, out, Z); false with afg_last_error set when the pair is refused
bool shape_of(uint32_t in_rate, uint32_t out_rate, uint32_t lowpass_width, uint32_t *Z, uint32_t *M, uint32_t *L, uint32_t *W, double *fc)
{
    if (in_rate == 0 || out_rate == 0) { afg::set_error("afg_resample_taps: a sample rate of 0 (%u -> %u)", in_rate, out_rate); return false; }
    if (lowpass_width > 64) { afg::set_error("afg_resample_taps: lowpass_width %u: at most 64 (0 means 6)", lowpass_width); return false; }
    *Z = lowpass_width ? lowpass_width : 6;
    const uint32_t g = afg::gcd32(in_rate, out_rate);
    *M = in_rate / g;
    *L = out_rate / g;
    *fc = kRolloff * std::min(1.0, (double)*L / (double)*M);
    if (in_rate == out_rate) { *W = 0; return true; }
    bool fits = false;
    *W = width_of(*fc, *Z, &fits);
    if (!fits || (uint64_t)*L * 2 * *W > kMaxTable) {
        afg::set_error("afg_resample_taps: %u -> %u Hz needs a table of %u phases of %.0f taps: more than 2^22 floats", in_rate, out_rate, *L,
                       2 * std::ceil((double)*Z / *fc));
        return false;
    }
    return true;
}

void fill_taps(float *taps, uint32_t Z, uint32_t L, uint32_t W, double fc)
{
    const uint32_t K = 2 * W;
    for (uint32_t p = 0; p < L; p++)
        for (uint32_t k = 0; k < K; k++) {
            const double d = ((double)k - (double)(W - 1)) - (double)p / (double)L;
            const double x = std::max(-(double)Z, std::min((double)Z, d * fc));
            const double s = x == 0.0 ? 1.0 : std::sin(afg::kPi * x) / (afg::kPi * x);
            const double c = std::cos(afg::kPi * x / (2.0 * (double)Z));
            taps[(size_t)p * K + k] = (float)(fc * s * (c * c));
        }
}

}  // namespace

extern "C" uint64_t afg_resample_taps(uint32_t in_rate, uint32_t out_rate, uint32_t lowpass_width, float *taps, uint64_t cap,
                                      uint32_t *M, uint32_t *L, uint32_t *W)
{
    uint32_t z = 0, m = 0, l = 0, w = 0;
    double fc = 0;
    const bool ok = shape_of(in_rate, out_rate, lowpass_width, &z, &m, &l, &w, &fc);
    if (!ok) m = l = w = 0;
    if (M) *M = m;
    if (L) *L = l;
    if (W) *W = w;
    if (!ok) return 0;
    const uint64_t need = (uint64_t)l * 2 * w;
    if (taps && need && cap >= need) fill_taps(taps, z, l, w, fc);
    return need;
}

namespace afg_front {

void ResampleJob::plan()
{
    R_s = mono ? in_channels : C;
    // H: the W of the steepest pair a file may bring (W grows with the file's rate, and is ceil(Z / 0.99) going up)
    const uint32_t top = std::max(max_in_rate, samplerate);
    bool fits = false;
    H = width_of(kRolloff * ((double)samplerate / (double)top), Z, &fits);
    T_s = ((uint64_t)T * max_in_rate + samplerate - 1) / samplerate + 2ull * H + 1;
    if (!fits) T_s = ~(uint64_t)0;
}

int resample_table(uint32_t in_rate, uint32_t out_rate, uint32_t Z, ResampleTable &t)
{
    static std::mutex mu;
    static std::map<std::tuple<uint32_t, uint32_t, uint32_t>, ResampleTable> cache;
    const auto key = std::make_tuple(in_rate, out_rate, Z);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) { t = it->second; return AFG_OK; }
    uint32_t z = 0;
    double fc = 0;
    ResampleTable made;
    if (!shape_of(in_rate, out_rate, Z, &z, &made.M, &made.L, &made.W, &fc)) return AFG_ERR_INVALID;
    auto taps = std::make_shared<std::vector<float>>((size_t)made.L * 2 * made.W);
    if (!taps->empty()) fill_taps(taps->data(), z, made.L, made.W, fc);
    made.taps = std::move(taps);
    cache.emplace(key, made);
    t = made;
    return AFG_OK;
}

int ResamplePlane::launch(const ResampleJob &job, const float *d_scratch, afg_batch_item *items, size_t n, const int64_t *first_frame,
                          const int64_t *scratch_frame0, float *d_out, std::deque<std::string> &messages, hipStream_t st)
{
    recs.clear();                                            // the uploads' sources live as long as the object
    taps.clear();
    std::map<uint32_t, std::pair<ResampleTable, uint64_t>> used;   // per file rate: the table and its place in `taps`
    const uint64_t slab_in = (uint64_t)job.R_s * job.T_s, slab_out = (uint64_t)job.C * job.T;
    auto refuse = [&](afg_batch_item &it, const std::string &why) {
        messages.push_back(why);
        it.status = AFG_ERR_UNSUPPORTED;
        it.message = messages.back().c_str();
        it.pcm = nullptr;
    };
    char text[256];
    for (size_t i = 0; i < n; i++) {
        afg_batch_item &it = items[i];
        const ResampleTable *tab = nullptr;
        uint64_t taps_off = 0;
        if (it.status == AFG_OK) {
            const double rate = (double)it.samplerate;
            const uint32_t in_rate = rate >= 1.0 && rate < 4294967296.0 ? (uint32_t)std::llround(rate) : 0;
            if (in_rate == 0 || in_rate > job.max_in_rate) {
                std::snprintf(text, sizeof text, "Cannot resample stream: its sample rate of %.9g Hz is 0 or above max_in_rate %u.", rate, job.max_in_rate);
                refuse(it, text);
            } else if (job.mono && (it.channels < 1 || (uint32_t)it.channels > job.in_channels)) {
                std::snprintf(text, sizeof text, "Cannot mix stream to mono: it has %d channels, in_channels is %u.", it.channels, job.in_channels);
                refuse(it, text);
            } else {
                auto u = used.find(in_rate);
                if (u == used.end()) {
                    ResampleTable t;
                    if (resample_table(in_rate, job.samplerate, job.Z, t) != AFG_OK) {
                        refuse(it, std::string("Cannot resample stream: ") + afg_last_error());
                    } else {
                        u = used.emplace(in_rate, std::make_pair(t, (uint64_t)taps.size())).first;
                        taps.insert(taps.end(), t.taps->begin(), t.taps->end());
                    }
                }
                if (u != used.end()) { tab = &u->second.first; taps_off = u->second.second; }
            }
        }
        const bool ok = tab != nullptr;
        if (ok) it.pcm = d_out + i * slab_out;
        // what the collate pass wrote of the file: frames [scratch_frame0, frames) of rows k < min(channels, R_s), T_s at the most
        const int64_t have = ok ? std::min<int64_t>(std::max<int64_t>(it.frames - scratch_frame0[i], 0), (int64_t)job.T_s) : 0;
        const uint32_t rows = ok ? (uint32_t)std::min<int64_t>(std::max(it.channels, 0), (int64_t)job.R_s) : 0;
        for (uint32_t k = 0; k < job.C; k++) {
            afg_resample_row r;
            std::memset(&r, 0, sizeof(r));
            r.out_off = i * slab_out + (uint64_t)k * job.T;
            r.out_frames = job.T;
            r.M = r.L = 1;
            if (ok && have > 0 && (job.mono || k < rows)) {
                r.in_off = i * slab_in + (job.mono ? 0 : (uint64_t)k * job.T_s);
                r.in_stride = job.T_s;
                r.in_rows = job.mono ? rows : 1;
                r.in_frames = (uint32_t)have;
                r.in_frame0 = (first_frame ? first_frame[i] : 0) - scratch_frame0[i];
                r.M = tab->M; r.L = tab->L; r.W = tab->W;
                r.taps_off = taps_off;
            }
            recs.push_back(r);
        }
    }
    if (recs.empty()) return AFG_OK;
    const uint64_t tiles = afg_resample_layout(recs.data(), recs.size());
    if (int rc = upload_records(d_recs, recs, st)) return rc;
    if (!taps.empty()) {
        if (int rc = d_taps.alloc(taps.size() * sizeof(float))) return rc;
        AFG_HIP_CHECK(hipMemcpyAsync(d_taps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, st));
    }
    return afg::resample_launch(recs.data(), recs.size(), (const afg_resample_row *)d_recs.p, tiles, d_scratch, n * slab_in,
                                taps.empty() ? nullptr : (const float *)d_taps.p, taps.size(), d_out, n * slab_out, st);
}

}  // namespace afg_front
