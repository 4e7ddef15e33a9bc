// afg_filter.cpp -- the host half of the filter stage (include/afg.h; kernel in csrc/filter.hip): the coefficient helper, the
// error bound, the checks of parameters and rows, the tables the kernel reads -- none of which needs a device -- and
// afg_batch_decode_filtered: afg_front::resampled_run into the caller's tensor, then one afg_filter_hip launch in place.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>

namespace {

constexpr double kBoundCap = 1073741824.0;                      // 2^30
constexpr uint64_t kMaxResponse = (uint64_t)1 << 28;            // samples of an impulse response that are summed at the most

int check_section(const afg_biquad &q, uint32_t s)
{
    if (!std::isfinite(q.b0) || !std::isfinite(q.b1) || !std::isfinite(q.b2) || !std::isfinite(q.a1) || !std::isfinite(q.a2)) {
        afg::set_error("afg_filter_params.sec[%u]: a coefficient that is not finite", s);
        return AFG_ERR_INVALID;
    }
    if (!(std::fabs(q.a2) < 1.0) || !(std::fabs(q.a1) < 1.0 + q.a2)) {
        afg::set_error("afg_filter_params.sec[%u]: a1 %.17g, a2 %.17g: the poles must lie inside the unit circle (|a2| < 1, |a1| < 1 + a2)", s,
                       q.a1, q.a2);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

int check_sections(const afg_filter_params *p)
{
    if (!p) { afg::set_error("afg_filter_params: NULL"); return AFG_ERR_INVALID; }
    if (p->n_sections < 1 || p->n_sections > AFG_FILTER_MAX_SECTIONS) {
        afg::set_error("afg_filter_params.n_sections %u: 1 .. %d", p->n_sections, AFG_FILTER_MAX_SECTIONS);
        return AFG_ERR_INVALID;
    }
    for (uint32_t s = 0; s < p->n_sections; s++)
        if (int rc = check_section(p->sec[s], s)) return rc;
    return AFG_OK;
}

// |g|_1 and |h|_1 of a section: g the impulse response of 1 / A, h = b * g; summed until what is left of both -- behind
// sample n no more than (beta or 1) * sum over m > n of (m + 1) r^m, r the pole radius -- is below 2^-60 of the sum
bool response_norms(const afg_biquad &q, uint32_t s, double *G, double *H)
{
    const double beta = std::fabs(q.b0) + std::fabs(q.b1) + std::fabs(q.b2);
    if (q.a1 == 0.0 && q.a2 == 0.0) { *G = 1.0; *H = beta; return true; }
    const double disc = q.a1 * q.a1 - 4.0 * q.a2;
    const double r = disc < 0.0 ? std::sqrt(q.a2) : 0.5 * (std::fabs(q.a1) + std::sqrt(disc));
    const double d = 1.0 - r;
    if (!(d > 0.0)) { afg::set_error("afg_filter_bound: sec[%u]: a pole radius of 1 in double", s); return false; }
    const double eps = std::ldexp(1.0, -60);
    double g1 = 0.0, g2 = 0.0, sg = 0.0, sh = 0.0, rn = 1.0;    // g[n-1], g[n-2]; r^n
    for (uint64_t n = 0; n < kMaxResponse; n++) {
        const double g = (n == 0 ? 1.0 : 0.0) - q.a1 * g1 - q.a2 * g2;
        const double h = q.b0 * g + q.b1 * g1 + q.b2 * g2;
        sg += std::fabs(g);
        sh += std::fabs(h);
        g2 = g1; g1 = g;
        rn *= r;                                                 // r^(n + 1)
        if ((n & 15) != 15) continue;
        // sum over m >= n + 1 of (m + 1) r^m = r^(n+1) ((n + 1) (1 - r) + 1) / (1 - r)^2
        const double tail = rn * ((double)(n + 1) * d + 1.0) / (d * d);
        if (tail <= eps * sg && beta * tail <= eps * sh) { *G = sg; *H = sh; return true; }
        if (!(sg < 1e300) || !(sh < 1e300)) break;
    }
    afg::set_error("afg_filter_bound: sec[%u]: the impulse response has not decayed after 2^28 samples", s);
    return false;
}

// E / max|x| of include/afg.h; 0 with afg_last_error set
double bound_of(const afg_filter_params *p)
{
    if (check_sections(p)) return 0.0;
    double G[AFG_FILTER_MAX_SECTIONS], H[AFG_FILTER_MAX_SECTIONS];
    for (uint32_t s = 0; s < p->n_sections; s++)
        if (!response_norms(p->sec[s], s, &G[s], &H[s])) return 0.0;
    double after[AFG_FILTER_MAX_SECTIONS + 1];
    after[p->n_sections] = 1.0;
    for (uint32_t s = p->n_sections; s-- > 0;) after[s] = after[s + 1] * H[s];      // product over t >= s
    double P = 1.0, sum = 0.0;
    for (uint32_t s = 0; s < p->n_sections; s++) {
        const afg_biquad &q = p->sec[s];
        const double beta = std::fabs(q.b0) + std::fabs(q.b1) + std::fabs(q.b2), alpha = std::fabs(q.a1) + std::fabs(q.a2);
        const double Pn = P * H[s];
        sum += G[s] * (beta * P + alpha * Pn) * after[s + 1];
        P = Pn;
    }
    const double E = std::ldexp(sum, -53);
    if (!(E <= kBoundCap)) {
        afg::set_error("afg_filter_bound: the cascade's error bound %g exceeds 2^30", E);
        return 0.0;
    }
    return E;
}

}  // namespace

// (the cascades that passed are remembered: a launch does not sum impulse responses again)
int afg::filter_check_params(const afg_filter_params *params)
{
    static std::mutex mu;
    static std::set<std::string> passed;
    if (int rc = check_sections(params)) return rc;
    const std::string key((const char *)params->sec, (size_t)params->n_sections * sizeof(afg_biquad));
    {
        std::lock_guard<std::mutex> lk(mu);
        if (passed.count(key)) return AFG_OK;
    }
    if (!(bound_of(params) > 0.0)) return AFG_ERR_INVALID;
    std::lock_guard<std::mutex> lk(mu);
    if (passed.size() >= 256) passed.clear();
    passed.insert(key);
    return AFG_OK;
}

// per section kFilterSecDoubles doubles: b0 b1 b2 a1 a2 and three of padding; the two homogeneous responses of a chunk --
// h1[n], h2[n]: what v[-1] = 1 and what v[-2] = 1 leave at frame n with no input, the first row of A^(n + 1) -- and
// A^(16 i) for i = 0 .. 64, row-major, with A = [-a1 -a2; 1 0] the step of (v[n-1], v[n-2]).  Long double, rounded once.
void afg::filter_tables(const afg_filter_params *params, std::vector<double> &tab)
{
    tab.assign((size_t)params->n_sections * kFilterSecDoubles, 0.0);
    for (uint32_t s = 0; s < params->n_sections; s++) {
        const afg_biquad &q = params->sec[s];
        double *t = tab.data() + (size_t)s * kFilterSecDoubles;
        t[0] = q.b0; t[1] = q.b1; t[2] = q.b2; t[3] = q.a1; t[4] = q.a2;
        const long double a1 = q.a1, a2 = q.a2;
        long double m[4] = { 1.0L, 0.0L, 0.0L, 1.0L };         // A^n
        for (int n = 0; n < AFG_FILTER_CHUNK; n++) {
            const long double r[4] = { -a1 * m[0] - a2 * m[2], -a1 * m[1] - a2 * m[3], m[0], m[1] };    // A * A^n
            std::memcpy(m, r, sizeof m);
            t[kFilterH1 + n] = (double)m[0];
            t[kFilterH2 + n] = (double)m[1];
        }
        const long double c[4] = { m[0], m[1], m[2], m[3] };   // A^16
        long double p[4] = { 1.0L, 0.0L, 0.0L, 1.0L };
        for (int i = 0; i <= 64; i++) {
            for (int k = 0; k < 4; k++) t[kFilterPow + 4 * i + k] = (double)p[k];
            const long double r[4] = { c[0] * p[0] + c[1] * p[2], c[0] * p[1] + c[1] * p[3], c[2] * p[0] + c[3] * p[2], c[2] * p[1] + c[3] * p[3] };
            std::memcpy(p, r, sizeof p);
        }
    }
}

extern "C" int afg_biquad_design(uint32_t kind, double samplerate, double f0, double q, double gain_db, afg_biquad *out)
{
    if (!out) { afg::set_error("afg_biquad_design: NULL out"); return AFG_ERR_INVALID; }
    if (kind > AFG_BIQUAD_DC_BLOCK) { afg::set_error("afg_biquad_design: kind %u: AFG_BIQUAD_LOWPASS .. AFG_BIQUAD_DC_BLOCK", kind); return AFG_ERR_INVALID; }
    afg_biquad r;
    if (kind == AFG_BIQUAD_PREEMPHASIS) {
        if (!std::isfinite(f0) || std::fabs(f0) > 1.0) {
            afg::set_error("afg_biquad_design: pre-emphasis coefficient %g (in the f0 argument): finite and at most 1 in size", f0);
            return AFG_ERR_INVALID;
        }
        r.b0 = 1.0; r.b1 = -f0; r.b2 = 0.0; r.a1 = 0.0; r.a2 = 0.0;
        *out = r;
        return AFG_OK;
    }
    if (!std::isfinite(samplerate) || !(samplerate > 0.0)) { afg::set_error("afg_biquad_design: samplerate %g: finite and above 0", samplerate); return AFG_ERR_INVALID; }
    if (!std::isfinite(f0) || !(f0 > 0.0) || !(f0 < samplerate / 2.0)) {
        afg::set_error("afg_biquad_design: f0 %g: inside (0, samplerate / 2) = (0, %g)", f0, samplerate / 2.0);
        return AFG_ERR_INVALID;
    }
    const double w = 2.0 * afg::kPi * f0 / samplerate;
    if (kind == AFG_BIQUAD_DC_BLOCK) {
        r.b0 = 1.0; r.b1 = -1.0; r.b2 = 0.0; r.a1 = -std::exp(-w); r.a2 = 0.0;
        *out = r;
        return AFG_OK;
    }
    if (!std::isfinite(q) || !(q > 0.0)) { afg::set_error("afg_biquad_design: q %g: finite and above 0", q); return AFG_ERR_INVALID; }
    const bool gained = kind == AFG_BIQUAD_PEAKING || kind == AFG_BIQUAD_LOWSHELF || kind == AFG_BIQUAD_HIGHSHELF;
    if (gained && !std::isfinite(gain_db)) { afg::set_error("afg_biquad_design: gain_db %g: finite", gain_db); return AFG_ERR_INVALID; }
    const double c = std::cos(w), alpha = std::sin(w) / (2.0 * q), A = gained ? std::pow(10.0, gain_db / 40.0) : 1.0;
    double b0, b1, b2, a0 = 1.0 + alpha, a1 = -2.0 * c, a2 = 1.0 - alpha;
    switch (kind) {
    case AFG_BIQUAD_LOWPASS:  b0 = (1.0 - c) / 2.0; b1 = 1.0 - c; b2 = (1.0 - c) / 2.0; break;
    case AFG_BIQUAD_HIGHPASS: b0 = (1.0 + c) / 2.0; b1 = -(1.0 + c); b2 = (1.0 + c) / 2.0; break;
    case AFG_BIQUAD_BANDPASS: b0 = alpha; b1 = 0.0; b2 = -alpha; break;
    case AFG_BIQUAD_NOTCH:    b0 = 1.0; b1 = -2.0 * c; b2 = 1.0; break;
    case AFG_BIQUAD_ALLPASS:  b0 = 1.0 - alpha; b1 = -2.0 * c; b2 = 1.0 + alpha; break;
    case AFG_BIQUAD_PEAKING:
        b0 = 1.0 + alpha * A; b1 = -2.0 * c; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a2 = 1.0 - alpha / A;
        break;
    case AFG_BIQUAD_LOWSHELF: {
        const double S = 2.0 * std::sqrt(A) * alpha;
        b0 = A * ((A + 1.0) - (A - 1.0) * c + S); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * c); b2 = A * ((A + 1.0) - (A - 1.0) * c - S);
        a0 = (A + 1.0) + (A - 1.0) * c + S; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * c); a2 = (A + 1.0) + (A - 1.0) * c - S;
        break;
    }
    default: {                                                   // AFG_BIQUAD_HIGHSHELF
        const double S = 2.0 * std::sqrt(A) * alpha;
        b0 = A * ((A + 1.0) + (A - 1.0) * c + S); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * c); b2 = A * ((A + 1.0) + (A - 1.0) * c - S);
        a0 = (A + 1.0) - (A - 1.0) * c + S; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * c); a2 = (A + 1.0) - (A - 1.0) * c - S;
        break;
    }
    }
    r.b0 = b0 / a0; r.b1 = b1 / a0; r.b2 = b2 / a0; r.a1 = a1 / a0; r.a2 = a2 / a0;
    if (check_section(r, 0)) {
        afg::set_error("afg_biquad_design: kind %u, f0 %g, q %g, gain_db %g at %g Hz does not give a stable section in double", kind, f0, q, gain_db, samplerate);
        return AFG_ERR_INVALID;
    }
    *out = r;
    return AFG_OK;
}

extern "C" double afg_filter_bound(const afg_filter_params *params) { return bound_of(params); }

extern "C" uint32_t afg_filter_tile_frames(void) { return AFG_FILTER_TILE; }

extern "C" int afg_filter_check_rows(const afg_filter_row *rows, uint64_t n_rows, const afg_filter_params *params, uint64_t in_floats,
                                     uint64_t out_floats, int same_plane)
{
    try {
        if (int rc = afg::filter_check_params(params)) return rc;
        if (n_rows == 0) return AFG_OK;
        if (!rows) { afg::set_error("afg_filter_row: NULL rows"); return AFG_ERR_INVALID; }
        std::vector<afg::Range> r;
        for (uint64_t k = 0; k < n_rows; k++) {
            const afg_filter_row &w = rows[k];
            const unsigned long long kk = (unsigned long long)k;
            if (w.reserved != 0) { afg::set_error("afg_filter_row %llu: reserved %u: must be 0", kk, w.reserved); return AFG_ERR_INVALID; }
            if (w.frames == 0) continue;
            if (!afg::rows_inside(w.in_off, 1, 0, w.frames, in_floats)) {
                afg::set_error("afg_filter_row %llu: it leaves the input (%llu floats)", kk, (unsigned long long)in_floats);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(w.out_off, 1, 0, w.frames, out_floats)) {
                afg::set_error("afg_filter_row %llu: it leaves the output (%llu floats)", kk, (unsigned long long)out_floats);
                return AFG_ERR_INVALID;
            }
            r.push_back(afg::Range{ w.out_off, w.out_off + w.frames, k, true });
            if (same_plane && w.in_off != w.out_off) r.push_back(afg::Range{ w.in_off, w.in_off + w.frames, k, false });
        }
        uint64_t row = 0, other = 0;
        if (afg::first_overlap(r, &row, &other)) {
            afg::set_error("afg_filter_row %llu: it overlaps row %llu without being in place", (unsigned long long)row, (unsigned long long)other);
            return AFG_ERR_INVALID;
        }
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

extern "C" int afg_batch_decode_filtered(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                                         const afg_filter_params *filter, float *d_out, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        afg_front::ResampleJob job;
        if (int rc = afg_front::entry_args("afg_batch_decode_filtered", { { "opts", opts }, { "filter", filter }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (int rc = afg_front::resampled_opts_check(opts, data, length, n_files, job)) return rc;
        if (int rc = afg::filter_check_params(filter)) return rc;
        if (n_files == 0) return AFG_OK;
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        afg_batch_item *const items = res.items;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg_front::resampled_run(job, opts, data, length, n_files, d_out, items, messages)) return rc;
        // the tensor is whole (resampled_run returns drained): every file's rows over their valid frames, in place
        std::vector<afg_filter_row> rows;                        // (declared in front of the drain: the upload reads them)
        afg_front::DevBuf d_rows;
        afg_front::NullStreamDrain drain;
        std::vector<afg_norm_group> groups;
        afg_front::norm_file_groups(job, items, (size_t)n_files, opts->first_frame, groups);
        for (const afg_norm_group &g : groups)
            for (uint32_t k = 0; k < g.rows && g.valid != 0; k++) {
                afg_filter_row w;
                std::memset(&w, 0, sizeof(w));
                w.in_off = w.out_off = g.in_off + (uint64_t)k * g.stride;
                w.frames = g.valid;
                rows.push_back(w);
                // (the resampler's own tail, a few frames behind the file's last, goes: nothing lies behind valid)
                if (g.valid < job.T) AFG_HIP_CHECK(hipMemsetAsync(d_out + w.out_off + g.valid, 0, (size_t)(job.T - g.valid) * sizeof(float), nullptr));
            }
        if (!rows.empty()) {
            const uint64_t plane = (uint64_t)n_files * job.C * job.T;
            if (int rc = afg_front::upload_records(d_rows, rows, nullptr)) return rc;
            if (int rc = afg::filter_launch(rows.data(), rows.size(), (const afg_filter_row *)d_rows.p, filter, d_out, plane, d_out, plane, nullptr, nullptr))
                return rc;
            AFG_HIP_CHECK(hipStreamSynchronize(nullptr));
        }
        return res.finish(out);
    });
}
