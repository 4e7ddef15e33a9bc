// afg_xm_stage.cpp -- the device side of XM decoding: a stream's reads, the batch path's XM stage and afg_xm_parse.
//
// Like the MOD stage it runs on what afg_stage.h gives every stage: pooled device buffers, page-locked staging, and chunks
// of about 128 MB of PCM with chunk c + 1 mixed while chunk c comes back.  Its record set is its own: the side table of
// floats and XM's song, tick and segment records.
#include "afg_xm_front.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>

namespace afg_xm {

using afg_front::align16;
using afg_front::DevBuf;

namespace {

// The inputs of one launch in one buffer: ticks, segments, side table, sample data (each 16-byte aligned)
struct InLayout {
    size_t ticks = 0, segs = 0, aux = 0, data = 0, bytes = 0;
    InLayout(size_t n_ticks, size_t n_segs, size_t n_aux, size_t data_bytes)
    {
        segs = align16(n_ticks * sizeof(afg_xm_tick));
        aux = segs + align16(std::max<size_t>(n_segs, 1) * sizeof(afg_xm_segment));
        data = aux + align16(std::max<size_t>(n_aux, 1) * sizeof(float));
        bytes = data + align16(std::max<size_t>(data_bytes, 16));
    }
};

}  // namespace

int StreamMix::read(void *out, int frames, bool f64)
{
    if (frames <= 0 || song.loop_count() >= 1) return 0;            // stream.d:600: the song is finished
    rec_.clear();
    const int n = (int)song.render((uint64_t)frames, false, rec_);  // exactly `frames`: zeros once the loop count is raised
    if (rec_.overflow) { afg::set_error(kMessageTooManyRecords); return -1; }
    hipStream_t st = nullptr;
    bool moved = false;
    const int rc = stream_.current(&st, &moved);
    if (moved) uploaded_ = false;     // the caller changed devices between reads: the sample data is uploaded again
    if (rc) return rc;
    const std::vector<uint8_t> &data = song.sample_data();
    if (!uploaded_ || data_.dev != stream_.dev) {
        if (data_.alloc(data.size())) return -1;
        AFG_HIP_CHECK(hipMemcpyAsync(data_.p, data.data(), data.size(), hipMemcpyHostToDevice, st));
        uploaded_ = true;
    }
    const InLayout L(rec_.ticks.size(), rec_.segs.size(), rec_.aux.size(), 0);
    const size_t song_at = L.data;                                   // the song record rides in the (unused) data slot
    staging_.assign(L.bytes + sizeof(afg_xm_song), 0);
    afg_xm_song sg;
    std::memset(&sg, 0, sizeof(sg));
    sg.n_ticks = (uint32_t)rec_.ticks.size();
    sg.sample_bytes = (uint32_t)data.size();
    std::memcpy(staging_.data() + song_at, &sg, sizeof(sg));
    std::memcpy(staging_.data() + L.ticks, rec_.ticks.data(), rec_.ticks.size() * sizeof(afg_xm_tick));
    if (!rec_.segs.empty()) std::memcpy(staging_.data() + L.segs, rec_.segs.data(), rec_.segs.size() * sizeof(afg_xm_segment));
    if (!rec_.aux.empty()) std::memcpy(staging_.data() + L.aux, rec_.aux.data(), rec_.aux.size() * sizeof(float));
    const size_t out_bytes = (size_t)n * 2 * sizeof(float);
    if (recs_.alloc(staging_.size()) || out_.alloc(out_bytes)) return -1;
    AFG_HIP_CHECK(hipMemcpyAsync(recs_.p, staging_.data(), staging_.size(), hipMemcpyHostToDevice, st));
    const uint8_t *r = (const uint8_t *)recs_.p;
    if (afg_xm_render_hip(1, (const afg_xm_song *)(r + song_at), (const afg_xm_segment *)(r + L.segs), (const afg_xm_tick *)(r + L.ticks),
                          (const uint8_t *)data_.p, (const float *)(r + L.aux), (float *)out_.p, st))
        return -1;
    if (fetch_.run(out_.p, AFG_WAV_KIND_F32, (uint64_t)n * 2, out, f64, st)) return -1;
    return n;
}

int batch_stage(const uint8_t *const *data, const size_t *length, const std::vector<int> &which,
                int n_threads, afg_batch_item *items, std::shared_ptr<void> &keep, afg_front::SampleOut so)
{
    const size_t es = so.es();                                    // bytes per sample of the PCM plane the items point into
    if (which.empty()) return AFG_OK;
    struct Sim {
        bool ok = false, capped = false, refused = false;
        uint64_t frames = 0;
        Song song;
        Records rec;
    };
    std::vector<Sim> sims(which.size());
    std::atomic<bool> oom{ false };
    afg_front::parallel_run(which.size(), n_threads, [&](size_t k) {
        const int i = which[k];
        try {
            Sim &s = sims[k];
            if (!data[i] || !probe(data[i], length[i], &s.song)) return;
            s.frames = render_song(s.song, s.rec, &s.capped);
            if (s.rec.overflow) { s.refused = true; s.rec = Records(); return; }
            s.ok = true;
        } catch (...) {
            oom = true;
        }
    });
    if (oom) { afg::set_error("XM stage: out of host memory"); return AFG_ERR_OOM; }
    std::vector<size_t> mods;
    for (size_t k = 0; k < sims.size(); k++) {
        if (sims[k].ok) mods.push_back(k);
        if (sims[k].refused) {                                       // an XM, but not one this library will mix
            afg_batch_item &it = items[which[k]];
            it.status = AFG_ERR_UNSUPPORTED;
            it.message = kMessageTooManyRecords;
            it.format = AFG_FORMAT_XM;
        }
    }
    if (mods.empty()) return AFG_OK;

    // ---- layout: songs start on 16-frame boundaries of the PCM plane, so that every lane stores whole lines ----
    const size_t M = mods.size();
    std::vector<afg_xm_song> songs(M);
    std::vector<uint64_t> start(M), end(M);
    uint64_t frames = 0, n_ticks = 0, n_segs = 0, n_aux = 0, data_bytes = 0;
    for (size_t j = 0; j < M; j++) {
        const Sim &s = sims[mods[j]];
        afg_xm_song &g = songs[j];
        std::memset(&g, 0, sizeof(g));
        g.out_frame = frames; g.tick_base = n_ticks; g.seg_base = n_segs; g.aux_base = n_aux; g.sample_base = data_bytes;
        g.n_ticks = (uint32_t)s.rec.ticks.size();
        g.sample_bytes = (uint32_t)s.song.sample_data().size();
        start[j] = frames;
        frames += (s.frames + 15) & ~(uint64_t)15;
        end[j] = frames;
        n_ticks += s.rec.ticks.size(); n_segs += s.rec.segs.size(); n_aux += s.rec.aux.size();
        data_bytes += align16(s.song.sample_data().size());
    }
    void *pcm = nullptr, *in = nullptr;
    const size_t pcm_bytes = std::max<uint64_t>(frames, 1) * 2 * es;
    const InLayout L(n_ticks, n_segs, n_aux, data_bytes);
    std::shared_ptr<void> pcm_owner;                       // (collate: the floats go on to the tensor, nothing comes back)
    if (so.fetch() && !(pcm_owner = afg_front::staging_lease(pcm_bytes, &pcm))) return AFG_ERR_OOM;
    std::shared_ptr<void> in_owner = afg_front::staging_lease(L.bytes, &in);
    if (!in_owner) return AFG_ERR_OOM;
    uint8_t *hin = (uint8_t *)in;
    afg_front::parallel_run(M, n_threads, [&](size_t j) {
        const Sim &s = sims[mods[j]];
        const afg_xm_song &g = songs[j];
        if (!s.rec.ticks.empty()) std::memcpy(hin + L.ticks + g.tick_base * sizeof(afg_xm_tick), s.rec.ticks.data(), s.rec.ticks.size() * sizeof(afg_xm_tick));
        if (!s.rec.segs.empty()) std::memcpy(hin + L.segs + g.seg_base * sizeof(afg_xm_segment), s.rec.segs.data(), s.rec.segs.size() * sizeof(afg_xm_segment));
        if (!s.rec.aux.empty()) std::memcpy(hin + L.aux + g.aux_base * sizeof(float), s.rec.aux.data(), s.rec.aux.size() * sizeof(float));
        std::memcpy(hin + L.data + g.sample_base, s.song.sample_data().data(), s.song.sample_data().size());
    });

    // ---- chunks of songs, about 128 MB of output each: chunk c + 1 is mixed while chunk c comes back ----
    const afg_front::SongChunks chunks(start, end);
    const std::vector<size_t> &first = chunks.first;
    const std::vector<afg_xm_song> rel = chunks.relative(songs);
    DevBuf d_in, d_songs, d_out[2];
    if (int rc = d_in.alloc(L.bytes)) return rc;
    if (int rc = d_songs.alloc(M * sizeof(afg_xm_song))) return rc;
    for (DevBuf &b : d_out) if (int rc = b.alloc(chunks.max_frames * 2 * sizeof(float))) return rc;
    afg_front::WideSlots wide;                             // f64, AFG_SAMPLE_PCM_*, collate: the mixed floats stay on the device and are converted there
    std::vector<afg_front::PackRun> runs;                  // a song is one run of its own samples
    if (so.wide() && so.fetch()) if (int rc = wide.alloc(chunks.max_frames * 2, es)) return rc;
    for (size_t j = 0; j < M && so.runs(); j++) runs.push_back(afg_front::PackRun{ 2 * start[j], 2 * sims[mods[j]].frames, 0, (uint32_t)which[mods[j]], 2 });
    const uint8_t *din = (const uint8_t *)d_in.p;
    const int rc = afg_front::run_chunks(
        chunks.count(),
        [&](hipStream_t up) -> int {                       // everything the mixer reads goes up once
            AFG_HIP_CHECK(hipMemcpyAsync(d_in.p, in, L.bytes, hipMemcpyHostToDevice, up));
            AFG_HIP_CHECK(hipMemcpyAsync(d_songs.p, rel.data(), M * sizeof(afg_xm_song), hipMemcpyHostToDevice, up));
            return AFG_OK;
        },
        /* upload */ nullptr,                              // no per-chunk upload: nothing waits on the host
        [&](size_t c, int slot, hipStream_t up) -> int {
            // the padding frames between songs are never mixed; the items do not reach them
            if (int rc = afg_xm_render_hip((uint32_t)(first[c + 1] - first[c]), (const afg_xm_song *)d_songs.p + first[c],
                                           (const afg_xm_segment *)(din + L.segs), (const afg_xm_tick *)(din + L.ticks) + songs[first[c]].tick_base,
                                           din + L.data, (const float *)(din + L.aux), (float *)d_out[slot].p, up))
                return rc;
            return wide.launch(slot, so, AFG_WAV_KIND_F32, d_out[slot].p, 2 * start[first[c]], chunks.frames[c] * 2, runs, up);
        },
        [&](size_t c, int slot, hipStream_t down) -> int {
            if (chunks.frames[c] && so.fetch())
                AFG_HIP_CHECK(hipMemcpyAsync((uint8_t *)pcm + 2 * start[first[c]] * es, so.wide() ? wide.buf[slot].p : d_out[slot].p, chunks.frames[c] * 2 * es,
                                             hipMemcpyDeviceToHost, down));
            return AFG_OK;
        });
    if (rc) return rc;
    for (size_t j = 0; j < M; j++) {
        const Sim &s = sims[mods[j]];
        afg_batch_item &it = items[which[mods[j]]];
        it.status = AFG_OK;
        it.message = s.capped ? afg_mod::kMessageCapped : nullptr;
        it.format = AFG_FORMAT_XM;
        it.channels = 2;
        it.samplerate = (float)kRate;
        it.frames = (int64_t)s.frames;
        it.pcm = s.frames && pcm ? (float *)((uint8_t *)pcm + 2 * songs[j].out_frame * es) : nullptr;
    }
    keep = pcm_owner;
    return AFG_OK;
}

}  // namespace afg_xm

namespace {
struct XmParsedOwner {
    afg_xm::Song song;
    afg_xm::Records rec;
};
}  // namespace

extern "C" int afg_xm_parse(const uint8_t *data, size_t length, afg_xm_parsed *out)
{
    if (!out) { afg::set_error("afg_xm_parse: NULL argument"); return AFG_ERR_INVALID; }
    std::memset(out, 0, sizeof(*out));
    if (!data) { afg::set_error("afg_xm_parse: NULL argument"); return AFG_ERR_INVALID; }
    try {
        std::unique_ptr<XmParsedOwner> o(new XmParsedOwner);
        if (!afg_xm::probe(data, length, &o->song)) { afg::set_error("afg_xm_parse: not an XM module"); return AFG_ERR_UNSUPPORTED; }
        out->channels = (uint32_t)o->song.num_channels();
        out->length = (uint32_t)o->song.length();
        out->patterns = (uint32_t)o->song.num_patterns();
        out->instruments = (uint32_t)o->song.num_instruments();
        out->restart = (uint32_t)o->song.restart();
        bool capped = false;
        out->n_frames = afg_xm::render_song(o->song, o->rec, &capped);
        if (o->rec.overflow) { std::memset(out, 0, sizeof(*out)); afg::set_error(afg_xm::kMessageTooManyRecords); return AFG_ERR_UNSUPPORTED; }
        out->capped = capped;
        if (o->rec.segs.empty()) o->rec.segs.resize(1), std::memset(o->rec.segs.data(), 0, sizeof(afg_xm_segment)), out->n_segments = 0;
        else out->n_segments = o->rec.segs.size();
        out->n_aux = o->rec.aux.size();
        if (o->rec.aux.empty()) o->rec.aux.push_back(0.0f);
        out->n_ticks = o->rec.ticks.size();
        out->n_sample_bytes = o->song.sample_data().size();
        out->ticks = o->rec.ticks.data();
        out->segments = o->rec.segs.data();
        out->sample_bytes = const_cast<uint8_t *>(o->song.sample_data().data());
        out->aux = o->rec.aux.data();
        out->owner = o.release();
        return AFG_OK;
    } catch (...) {
        std::memset(out, 0, sizeof(*out));
        afg::set_error("afg_xm_parse: out of host memory");
        return AFG_ERR_OOM;
    }
}

extern "C" void afg_xm_parsed_free(afg_xm_parsed *p)
{
    if (!p) return;
    delete (XmParsedOwner *)p->owner;
    std::memset(p, 0, sizeof(*p));
}
