// afg_cepstra.cpp -- the host half of the cepstral features (include/afg.h; kernel in csrc/cepstra.hip): the DCT table of
// the definition, computed in double and kept per parameter set; the tile layout and the checks of records and parameters,
// which need no device; and afg_batch_decode_mfcc -- afg_front::mel_batch of a sublist into a pooled log-mel scratch, then
// one afg_cepstra_hip launch, then the optional per-row normalisation (CMVN) in place.
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

constexpr uint32_t kTile = AFG_CEP_TILE;

uint64_t tiles_of(const afg_cep_row &r) { return ((uint64_t)r.frames + kTile - 1) / kTile; }

int check_params(const afg_cep_params *p)
{
    if (!p) { afg::set_error("afg_cep_params: NULL"); return AFG_ERR_INVALID; }
    if (p->n_mels < 1 || p->n_mels > 256) { afg::set_error("afg_cep_params.n_mels %u: 1 .. 256", p->n_mels); return AFG_ERR_INVALID; }
    if (p->n_ceps < 1 || p->n_ceps > p->n_mels) { afg::set_error("afg_cep_params.n_ceps %u: 1 .. n_mels (%u)", p->n_ceps, p->n_mels); return AFG_ERR_INVALID; }
    if (p->delta_order > 2) { afg::set_error("afg_cep_params.delta_order %u: 0, 1 or 2", p->delta_order); return AFG_ERR_INVALID; }
    if (p->delta_order && (p->delta_win < 1 || p->delta_win > 8)) { afg::set_error("afg_cep_params.delta_win %u: 1 .. 8", p->delta_win); return AFG_ERR_INVALID; }
    for (int k = 0; k < 4; k++)
        if (p->reserved[k] != 0) { afg::set_error("afg_cep_params.reserved[%d] %u: must be 0", k, p->reserved[k]); return AFG_ERR_INVALID; }
    return AFG_OK;
}

bool dct_args_ok(uint32_t n_ceps, uint32_t n_mels, uint32_t norm, double lifter, double log_scale)
{
    if (n_mels < 1 || n_mels > 256) { afg::set_error("afg_cep_dct: n_mels %u: 1 .. 256", n_mels); return false; }
    if (n_ceps < 1 || n_ceps > n_mels) { afg::set_error("afg_cep_dct: n_ceps %u: 1 .. n_mels (%u)", n_ceps, n_mels); return false; }
    if (norm != AFG_CEP_DCT_NONE && norm != AFG_CEP_DCT_ORTHO) { afg::set_error("afg_cep_dct: norm %u: AFG_CEP_DCT_NONE or AFG_CEP_DCT_ORTHO", norm); return false; }
    if (!std::isfinite(lifter) || lifter < 0.0) { afg::set_error("afg_cep_dct: lifter %g: finite and at least 0 (0 means none)", lifter); return false; }
    if (!std::isfinite(log_scale) || log_scale == 0.0) { afg::set_error("afg_cep_dct: log_scale %g: finite and not 0", log_scale); return false; }
    return true;
}

void fill_dct(float *out, uint32_t n_ceps, uint32_t n_mels, uint32_t norm, double lifter, double log_scale)
{
    for (uint32_t q = 0; q < n_ceps; q++) {
        const double L = lifter > 0.0 ? 1.0 + (lifter / 2.0) * std::sin(afg::kPi * (double)q / lifter) : 1.0;
        const double s = norm == AFG_CEP_DCT_ORTHO ? std::sqrt((q == 0 ? 1.0 : 2.0) / (double)n_mels) : 2.0;
        for (uint32_t m = 0; m < n_mels; m++) {
            const uint64_t r = ((uint64_t)q * (2 * (uint64_t)m + 1)) % (4 * (uint64_t)n_mels);
            out[(size_t)q * n_mels + m] = (float)(log_scale * L * s * std::cos(afg::kPi * (double)r / (2.0 * (double)n_mels)));
        }
    }
}

// the table of one parameter set, made once and kept for the process
std::shared_ptr<const std::vector<float>> dct_table(uint32_t n_ceps, uint32_t n_mels, uint32_t norm, double lifter, double log_scale)
{
    static std::mutex mu;
    static std::map<std::tuple<uint32_t, uint32_t, uint32_t, double, double>, std::shared_ptr<const std::vector<float>>> tables;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(n_ceps, n_mels, norm, lifter, log_scale);
    auto t = tables.find(key);
    if (t == tables.end()) {
        auto v = std::make_shared<std::vector<float>>((size_t)n_ceps * n_mels);
        fill_dct(v->data(), n_ceps, n_mels, norm, lifter, log_scale);
        t = tables.emplace(key, std::move(v)).first;
    }
    return t->second;
}

}  // namespace

extern "C" uint64_t afg_cep_dct(uint32_t n_ceps, uint32_t n_mels, uint32_t norm, double lifter, double log_scale, float *out, uint64_t cap)
{
    if (!dct_args_ok(n_ceps, n_mels, norm, lifter, log_scale)) return 0;
    const uint64_t need = (uint64_t)n_ceps * n_mels;
    if (out && cap >= need) fill_dct(out, n_ceps, n_mels, norm, lifter, log_scale);
    return need;
}

extern "C" uint64_t afg_cep_layout(afg_cep_row *rows, uint64_t n_rows, const afg_cep_params *params)
{
    if (check_params(params)) return 0;
    uint64_t tiles = 0;
    for (uint64_t k = 0; rows && k < n_rows; k++) {
        rows[k].first_tile = tiles;
        tiles += tiles_of(rows[k]);
    }
    return tiles;
}

extern "C" int afg_cep_check_rows(const afg_cep_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_cep_params *params, uint64_t in_floats,
                                  uint64_t dct_floats, uint64_t out_floats)
{
    if (int rc = check_params(params)) return rc;
    if (n_rows == 0) return AFG_OK;
    if (!rows) { afg::set_error("afg_cep_check_rows: NULL rows"); return AFG_ERR_INVALID; }
    const afg_cep_params &p = *params;
    if (dct_floats < (uint64_t)p.n_ceps * p.n_mels) {
        afg::set_error("afg_cepstra_hip: dct_floats %llu: the table is n_ceps x n_mels = %llu floats", (unsigned long long)dct_floats,
                       (unsigned long long)p.n_ceps * p.n_mels);
        return AFG_ERR_INVALID;
    }
    const uint64_t out_rows = (uint64_t)(1 + p.delta_order) * p.n_ceps;
    uint64_t tiles = 0;
    for (uint64_t k = 0; k < n_rows; k++) {
        const afg_cep_row &r = rows[k];
        const unsigned long long kk = (unsigned long long)k;
        if (r.reserved != 0) { afg::set_error("afg_cepstra_hip: record %llu: reserved %u: must be 0", kk, r.reserved); return AFG_ERR_INVALID; }
        if (r.first_tile != tiles) {
            afg::set_error("afg_cepstra_hip: record %llu: first_tile %llu, afg_cep_layout gives %llu", kk, (unsigned long long)r.first_tile,
                           (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        tiles += tiles_of(r);                                    // below 2^26 a record: no wrap before the launch's cap refuses
        if (tiles > ((uint64_t)1 << 62)) { afg::set_error("afg_cepstra_hip: record %llu: too many tiles", kk); return AFG_ERR_INVALID; }
        if (r.frames == 0) continue;
        if (!afg::rows_inside(r.in_off, 1, 0, (uint64_t)p.n_mels * r.frames, in_floats)) {
            afg::set_error("afg_cepstra_hip: record %llu: its slab of %u x %u floats leaves the input (%llu floats)", kk, p.n_mels, r.frames,
                           (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        if (!afg::rows_inside(r.out_off, 1, 0, out_rows * r.frames, out_floats)) {
            afg::set_error("afg_cepstra_hip: record %llu: its %llu x %u floats leave the output (%llu floats)", kk, (unsigned long long)out_rows,
                           r.frames, (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
    }
    if (tiles != n_tiles) {
        afg::set_error("afg_cepstra_hip: n_tiles %llu, afg_cep_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

extern "C" int afg_batch_decode_mfcc(const uint8_t *const *data, const size_t *length, int n_files, const afg_mfcc_opts *opts,
                                     const afg_norm_params *wave_norm, const afg_norm_params *cmvn, float *d_out, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (int rc = afg_front::entry_args("afg_batch_decode_mfcc", { { "opts", opts }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (opts->struct_size < sizeof(afg_mfcc_opts)) {
            afg::set_error("afg_mfcc_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        const afg_mfcc_opts &o = *opts;
        {
            // what afg_batch_decode_mel_norm checks of its options (an empty list: it touches nothing), then of the list
            afg_batch_result none;
            if (int rc = afg_front::mel_batch(data, length, 0, &o.mel, wave_norm, nullptr, d_out, &none)) return rc;
            const afg_resample_opts ro = afg_front::resample_opts_of(o.mel);
            afg_front::ResampleJob job;
            if (int rc = afg_front::resampled_check(&ro, data, length, n_files, job)) return rc;
        }
        if (o.mel.mel.out_kind != AFG_MEL_LOG10) {
            afg::set_error("afg_mfcc_opts.mel.mel.out_kind %u: the cepstra are taken of AFG_MEL_LOG10 features", o.mel.mel.out_kind);
            return AFG_ERR_INVALID;
        }
        if (o.cep.n_mels != o.mel.mel.n_mels) {
            afg::set_error("afg_mfcc_opts.cep.n_mels %u, but mel.mel.n_mels is %u", o.cep.n_mels, o.mel.mel.n_mels);
            return AFG_ERR_INVALID;
        }
        if (int rc = afg_cep_check_rows(nullptr, 0, 0, &o.cep, 0, 0, 0)) return rc;
        const double log_scale = o.log_scale == 0.0 ? 1.0 : o.log_scale;
        if (!dct_args_ok(o.cep.n_ceps, o.cep.n_mels, o.dct_norm, o.lifter, log_scale)) return AFG_ERR_INVALID;
        if (cmvn)
            if (int rc = afg_norm_check_groups(nullptr, 0, 0, cmvn, 0, 0)) return rc;
        if (n_files == 0) return AFG_OK;
        const uint32_t n_out = o.mel.n_out ? o.mel.n_out : afg_mel_frames(&o.mel.mel, o.mel.frames);
        const uint64_t out_rows = (uint64_t)(1 + o.cep.delta_order) * o.cep.n_ceps;
        const uint64_t slab_in = (uint64_t)o.mel.channels * o.cep.n_mels * n_out, slab_out = (uint64_t)o.mel.channels * out_rows * n_out;
        if (std::max(slab_in, slab_out) > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_mfcc: a tensor of %d x %u x %llu x %u floats", n_files, o.mel.channels, (unsigned long long)out_rows, n_out);
            return AFG_ERR_INVALID;
        }
        const auto table = dct_table(o.cep.n_ceps, o.cep.n_mels, o.dct_norm, o.lifter, log_scale);
        const size_t per_list = afg_front::sublist_size(n_files, slab_in * sizeof(float), afg::kDevMelScratchBytes);
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        std::deque<std::string> &messages = res.messages();
        if (int rc = afg::require_device()) return rc;
        std::vector<afg_cep_row> recs;                           // (declared in front of the drain: the uploads read them)
        std::vector<afg_norm_group> groups;
        afg_front::NormPlane norm;
        afg_front::DevBuf scratch, d_recs, d_dct;
        afg_front::NullStreamDrain drain;
        if (int rc = scratch.alloc((size_t)(per_list * slab_in * sizeof(float)))) return rc;
        if (int rc = d_dct.alloc(table->size() * sizeof(float))) return rc;
        AFG_HIP_CHECK(hipMemcpyAsync(d_dct.p, table->data(), table->size() * sizeof(float), hipMemcpyHostToDevice, nullptr));
        for (size_t f0 = 0; f0 < (size_t)n_files; f0 += per_list) {
            const size_t n = std::min(per_list, (size_t)n_files - f0);
            // the log-mel tensor of the sublist, every element written (a failed file's slab is the floor) ...
            afg_mel_opts sub = o.mel;
            if (sub.first_frame) sub.first_frame += f0;
            afg_batch_result part;
            if (int rc = afg_front::mel_batch(data + f0, length + f0, (int)n, &sub, wave_norm, nullptr, (float *)scratch.p, &part)) return rc;
            struct FreePart { afg_batch_result *r; ~FreePart() { afg_batch_free(r); } } free_part{ &part };
            float *y = d_out + f0 * slab_out;
            for (size_t i = 0; i < n; i++) {
                afg_batch_item it = part.items[i];
                if (it.message) {                                // (the sublist's strings go with its result)
                    messages.emplace_back(it.message);
                    it.message = messages.back().c_str();
                }
                if (it.pcm) it.pcm = y + i * slab_out;
                res.items[f0 + i] = it;
            }
            // ... its cepstra: one record per file and channel ...
            recs.clear();
            for (uint64_t k = 0; k < n * o.mel.channels; k++) {
                afg_cep_row r;
                std::memset(&r, 0, sizeof(r));
                r.in_off = k * o.cep.n_mels * n_out;
                r.out_off = k * out_rows * n_out;
                r.frames = n_out;
                recs.push_back(r);
            }
            const uint64_t tiles = afg_cep_layout(recs.data(), recs.size(), &o.cep);
            if (int rc = afg_front::upload_records(d_recs, recs, nullptr)) return rc;
            if (int rc = afg::cepstra_launch(recs.data(), recs.size(), (const afg_cep_row *)d_recs.p, tiles, &o.cep, (const float *)scratch.p,
                                             n * slab_in, (const float *)d_dct.p, table->size(), y, n * slab_out, nullptr))
                return rc;
            if (cmvn) {                                          // ... and every output row one group, over its n_out frames
                groups.clear();
                afg_norm_group g;
                std::memset(&g, 0, sizeof(g));
                g.rows = 1;
                g.valid = n_out;
                g.stride = n_out;
                for (uint64_t k = 0; k < n * o.mel.channels * out_rows; k++) {
                    g.in_off = g.out_off = k * n_out;
                    groups.push_back(g);
                }
                if (int rc = norm.launch(*cmvn, groups, y, n * slab_out, nullptr, nullptr)) return rc;
            }
            AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
        }
        return res.finish(out);
    });
}
