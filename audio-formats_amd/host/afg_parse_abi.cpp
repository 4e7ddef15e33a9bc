// afg_parse_abi.cpp -- the host front-ends as the C ABI shows them (afg_flac_parse ... afg_qoa_parse): one file parsed into
// the transform-stage records of its codec, owned by the result until its *_free.  Tests and callers that drive the device
// stages themselves use them; the batch path and the streams call the front-ends directly.
#include "afg_batch.h"

#include <new>

using namespace afg_front;

extern "C" {

namespace {
struct FlacParsedOwner {
    FlacRecords rec;
};
}  // namespace

int afg_flac_parse(const uint8_t *data, size_t length, afg_flac_parsed *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<FlacParsedOwner> own_guard(new (std::nothrow) FlacParsedOwner);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        FlacInfo fi;
        if (!flac_parse(data, length, fi, own->rec)) {
            own_guard.reset();
            afg::set_error("afg_flac_parse: not a native FLAC stream");
            return AFG_ERR_UNSUPPORTED;
        }
        out->sample_rate = fi.sample_rate;
        out->channels = fi.channels;
        out->bps = fi.bps;
        out->max_block = fi.max_block;
        out->total_samples = fi.total_samples;
        out->n_frames = own->rec.frames.size();
        out->n_subframes = own->rec.subframes.size();
        out->n_res = own->rec.res.size();
        out->out_samples = own->rec.out_samples;
        out->frames = own->rec.frames.data();
        out->subframes = own->rec.subframes.data();
        out->res = own->rec.res.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_flac_parsed_free(afg_flac_parsed *p)
{
    if (!p) return;
    delete (FlacParsedOwner *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_mp3_parse(const uint8_t *data, size_t length, afg_mp3_parsed *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_mp3::File> own_guard(new (std::nothrow) afg_mp3::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        if (!afg_mp3::parse_file(data, length, *own)) {
            own_guard.reset();
            afg::set_error("afg_mp3_parse: no MPEG Layer III stream found");
            return AFG_ERR_UNSUPPORTED;
        }
        static_assert(sizeof(afg_mp3::Copy) == sizeof(afg_mp3_copy), "copy plan layout");
        out->channels = own->channels;
        out->hz = own->hz;
        out->tagged = own->tagged ? 1 : 0;
        out->start_delay = own->start_delay;
        out->detected_samples = own->detected_samples;
        out->declared_samples = own->declared_samples;
        out->pcm_samples = own->pcm_samples;
        out->n_runs = own->run_granules.size();
        out->n_blocks = own->blocks();
        out->n_copies = own->copies.size();
        out->run_granules = own->run_granules.data();
        out->coef = own->coef.data();
        out->flags = own->flags.data();
        out->copies = (afg_mp3_copy *)own->copies.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_mp3_parsed_free(afg_mp3_parsed *p)
{
    if (!p) return;
    delete (afg_mp3::File *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_mp3_parse_q(const uint8_t *data, size_t length, afg_mp3_parsed_q *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_mp3::File> own_guard(new (std::nothrow) afg_mp3::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        own->quantised = true;
        if (!afg_mp3::parse_file(data, length, *own)) {
            own_guard.reset();
            afg::set_error("afg_mp3_parse_q: no MPEG Layer III stream found");
            return AFG_ERR_UNSUPPORTED;
        }
        if (own->q_unsupported) {
            own_guard.reset();
            afg::set_error("afg_mp3_parse_q: the stream holds granules the device requantiser does not cover (MPEG-2.5 8 kHz mixed blocks, or a mono frame with the intensity bit set)");
            return AFG_ERR_UNSUPPORTED;
        }
        afg_mp3_parsed &b = out->base;
        b.channels = own->channels;
        b.hz = own->hz;
        b.tagged = own->tagged ? 1 : 0;
        b.start_delay = own->start_delay;
        b.detected_samples = own->detected_samples;
        b.declared_samples = own->declared_samples;
        b.pcm_samples = own->pcm_samples;
        b.n_runs = own->run_granules.size();
        b.n_blocks = own->blocks();
        b.n_copies = own->copies.size();
        b.run_granules = own->run_granules.data();
        b.coef = nullptr;
        b.flags = own->flags.data();
        b.copies = (afg_mp3_copy *)own->copies.data();
        b.owner = own;                                  // (released from the guard at the end)
        out->n_granules = own->qgr.size();
        out->n_sdesc = own->sdesc.size();
        out->q = own->q.data();
        out->granules = own->qgr.data();
        out->sdesc = own->sdesc.data();
        own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_mp3_qtables(uint8_t band_of_line[24][576], uint16_t dst_of_src[24][576], float pow43[145])
{
    const afg_mp3::QTables &t = afg_mp3::qtables();
    if (band_of_line) std::memcpy(band_of_line, t.band_of_line, sizeof(t.band_of_line));
    if (dst_of_src) std::memcpy(dst_of_src, t.dst_of_src, sizeof(t.dst_of_src));
    if (pow43) std::memcpy(pow43, t.pow43, sizeof(t.pow43));
}

void afg_mp3_parsed_q_free(afg_mp3_parsed_q *p)
{
    if (!p) return;
    delete (afg_mp3::File *)p->base.owner;
    std::memset(p, 0, sizeof(*p));
}

static int vorbis_parse_any(const uint8_t *data, size_t length, afg_vorbis_parsed *out, bool device_floor)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_vorbis::File> own_guard(new (std::nothrow) afg_vorbis::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        if (!afg_vorbis::parse_file(data, length, *own, device_floor)) {
            own_guard.reset();
            afg::set_error("afg_vorbis_parse: not an Ogg Vorbis I stream");
            return AFG_ERR_UNSUPPORTED;
        }
        out->channels = own->channels;
        out->blocksize0 = own->blocksize0;
        out->blocksize1 = own->blocksize1;
        out->sample_rate = own->sample_rate;
        out->total_samples = own->total_samples;
        out->n_packets = own->pflags.size();
        out->spec_floats = own->spec.size();
        out->pcm_frames = own->pcm_frames;
        out->pflags = own->pflags.data();
        out->spec = own->spec.data();
        out->take_from = own->take_from.data();
        out->take_count = own->take_count.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

int afg_vorbis_parse(const uint8_t *data, size_t length, afg_vorbis_parsed *out) { return vorbis_parse_any(data, length, out, false); }

void afg_vorbis_parsed_free(afg_vorbis_parsed *p)
{
    if (!p) return;
    delete (afg_vorbis::File *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_vorbis_parse_r(const uint8_t *data, size_t length, afg_vorbis_parsed_r *out)
{
    if (!out) return AFG_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    if (int rc = vorbis_parse_any(data, length, &out->base, true)) return rc;
    afg_vorbis::File *own = (afg_vorbis::File *)out->base.owner;
    out->n_curves = own->fl_curves.size();
    out->n_points = own->fl_points.size() / 2;
    out->n_steps = own->fl_steps.size() / 2;
    out->packets = own->fl_packets.data();
    out->curves = own->fl_curves.data();
    out->points = own->fl_points.data();
    out->steps = own->fl_steps.data();
    return AFG_OK;
}

void afg_vorbis_parsed_r_free(afg_vorbis_parsed_r *p)
{
    if (!p) return;
    afg_vorbis_parsed_free(&p->base);
    std::memset(p, 0, sizeof(*p));
}

int afg_opus_parse(const uint8_t *data, size_t length, afg_opus_parsed *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_opus::File> own_guard(new (std::nothrow) afg_opus::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        const afg_opus::Status st = afg_opus::parse_file(data, length, *own);
        if (st != afg_opus::kOpened) {
            if (st == afg_opus::kUnsupported) {
                out->channels = own->channels;
                out->preskip = own->preskip;
                afg::set_error("afg_opus_parse: the stream holds SILK or hybrid packets (only CELT-only Opus is decoded)");
            } else {
                afg::set_error("afg_opus_parse: not an Ogg Opus stream");
            }
            own_guard.reset();
            return AFG_ERR_UNSUPPORTED;
        }
        out->channels = own->channels;
        out->preskip = own->preskip;
        out->gain_i = own->gain_i;
        out->error = own->error ? 1 : 0;
        out->gain = own->gain;
        out->declared_frames = own->declared_frames;
        out->pcm_frames = own->pcm_frames;
        out->n_frames = own->frames.size();
        out->n_coeffs = own->coeffs.size();
        out->frames = own->frames.data();
        out->coeffs = own->coeffs.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_opus_parsed_free(afg_opus_parsed *p)
{
    if (!p) return;
    delete (afg_opus::File *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_qoa_parse(const uint8_t *data, size_t length, uint32_t *channels, uint32_t *samplerate, uint32_t *samples,
                  afg_qoa_frame *frames, size_t frame_cap, size_t *n_frames)
{
    if (!data) return AFG_ERR_INVALID;
    QoaInfo qi;
    std::vector<afg_qoa_frame> fr;
    if (!qoa_parse(data, length, qi, fr)) {
        afg::set_error("afg_qoa_parse: not a QOA file");
        return AFG_ERR_UNSUPPORTED;
    }
    if (channels) *channels = qi.channels;
    if (samplerate) *samplerate = qi.samplerate;
    if (samples) *samples = qi.samples;
    if (n_frames) *n_frames = fr.size();
    if (frames) std::memcpy(frames, fr.data(), std::min(frame_cap, fr.size()) * sizeof(afg_qoa_frame));
    return AFG_OK;
}

}  // extern "C"
