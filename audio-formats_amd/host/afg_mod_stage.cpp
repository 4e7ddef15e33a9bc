// afg_mod_stage.cpp -- the device side of MOD decoding: a stream's reads and the batch path's MOD stage.
//
// Both hand the mixer (csrc/mod_mix.hip) what the control layer (afg_mod_front.cpp) wrote down: the file's sample area,
// per song one afg_mod_song, and its ticks and segments.  Records are small next to the output (a 4-channel tick of
// 882 frames is 24 + 4 x 48 bytes against 7 KB of PCM), so the transfers that matter are the PCM coming back.
#include "afg_mod_front.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>

namespace afg_mod {

using afg_front::align16;
using afg_front::DevBuf;

const char *const kMessageCapped = "MOD: the song does not end; cut at AFG_MOD_MAX_FRAMES (30 minutes)";

namespace {

// Records of one launch in one buffer: songs, then ticks, then segments (each 16-byte aligned)
struct RecLayout {
    size_t songs = 0, ticks = 0, segs = 0, bytes = 0;
    RecLayout(size_t n_songs, size_t n_ticks, size_t n_segs)
    {
        songs = 0;
        ticks = align16(n_songs * sizeof(afg_mod_song));
        segs = ticks + align16(n_ticks * sizeof(afg_mod_tick));
        bytes = segs + align16(std::max<size_t>(n_segs, 1) * sizeof(afg_mod_segment));
    }
};

}  // namespace

int StreamMix::read(void *out, int frames, bool f64)
{
    if (frames <= 0 || song.loop_count() >= 1) return 0;           // stream.d:614: the song has ended
    ticks_.clear();
    segs_.clear();
    const int n = song.render(frames, 0, 0, ticks_, segs_);
    if (n <= 0) return 0;
    hipStream_t st = nullptr;
    bool moved = false;
    const int rc = stream_.current(&st, &moved);
    if (moved) uploaded_ = false;     // the caller changed devices between reads: the buffers follow, the plane is uploaded again
    if (rc) return rc;
    const std::vector<uint8_t> &plane = song.plane();
    if (!uploaded_ || plane_.dev != stream_.dev) {
        if (plane_.alloc(plane.size())) return -1;
        AFG_HIP_CHECK(hipMemcpyAsync(plane_.p, plane.data(), plane.size(), hipMemcpyHostToDevice, st));
        uploaded_ = true;
    }
    const RecLayout L(1, ticks_.size(), segs_.size());
    staging_.assign(L.bytes, 0);
    afg_mod_song sg;
    std::memset(&sg, 0, sizeof(sg));
    sg.n_ticks = (uint32_t)ticks_.size();
    sg.sample_bytes = (uint32_t)plane.size();
    std::memcpy(staging_.data() + L.songs, &sg, sizeof(sg));
    std::memcpy(staging_.data() + L.ticks, ticks_.data(), ticks_.size() * sizeof(afg_mod_tick));
    if (!segs_.empty()) std::memcpy(staging_.data() + L.segs, segs_.data(), segs_.size() * sizeof(afg_mod_segment));
    const size_t out_bytes = (size_t)n * 2 * sizeof(float);
    if (recs_.alloc(L.bytes) || out_.alloc(out_bytes)) return -1;
    AFG_HIP_CHECK(hipMemcpyAsync(recs_.p, staging_.data(), L.bytes, hipMemcpyHostToDevice, st));
    uint8_t *r = (uint8_t *)recs_.p;
    if (afg_mod_render_hip(1, (const afg_mod_song *)(r + L.songs), (const afg_mod_segment *)(r + L.segs),
                           (const afg_mod_tick *)(r + L.ticks), (const uint8_t *)plane_.p, (float *)out_.p, st))
        return -1;
    if (fetch_.run(out_.p, AFG_WAV_KIND_F32, (uint64_t)n * 2, out, f64, st)) return -1;
    return n;
}

int batch_stage(const uint8_t *const *data, const size_t *length, const std::vector<int> &which,
                int n_threads, afg_batch_item *items, std::shared_ptr<void> &keep, afg_front::SampleOut so)
{
    const size_t es = so.es();                                    // bytes per sample of the PCM plane the items point into
    if (which.empty()) return AFG_OK;
    // ---- the control layer, one file per helper-thread job ----
    // (the records go to per-file vectors first: their sizes are known only once a song has played, and they are small next
    // to the PCM -- a 4-channel tick is 24 + 4 x 48 bytes against 7 KB of output; the helper threads then gather them)
    struct Sim {
        bool ok = false, capped = false;
        uint64_t frames = 0;
        Song song;                                      // holds the sample plane
        std::vector<afg_mod_tick> ticks;
        std::vector<afg_mod_segment> segs;
    };
    std::vector<Sim> sims(which.size());
    std::atomic<bool> oom{ false };
    afg_front::parallel_run(which.size(), n_threads, [&](size_t k) {
        const int i = which[k];
        try {
            Sim &s = sims[k];
            if (!data[i] || !probe(data[i], length[i], &s.song)) return;
            s.frames = render_song(s.song, s.ticks, s.segs, &s.capped);
            s.ok = true;
        } catch (...) {
            oom = true;
        }
    });
    if (oom) { afg::set_error("MOD stage: out of host memory"); return AFG_ERR_OOM; }
    std::vector<size_t> mods;
    for (size_t k = 0; k < sims.size(); k++) if (sims[k].ok) mods.push_back(k);
    if (mods.empty()) return AFG_OK;

    // ---- layout: per song its output frame, ticks, segments and plane bytes in the batch ----
    const size_t M = mods.size();
    std::vector<afg_mod_song> songs(M);
    std::vector<uint64_t> start(M), end(M);
    uint64_t frames = 0, n_ticks = 0, n_segs = 0, plane_bytes = 0;
    for (size_t j = 0; j < M; j++) {
        const Sim &s = sims[mods[j]];
        afg_mod_song &g = songs[j];
        std::memset(&g, 0, sizeof(g));
        g.out_frame = frames; g.tick_base = n_ticks; g.seg_base = n_segs; g.sample_base = plane_bytes;
        g.n_ticks = (uint32_t)s.ticks.size();
        g.sample_bytes = (uint32_t)s.song.plane().size();
        start[j] = frames; end[j] = frames + s.frames;
        frames += s.frames; n_ticks += s.ticks.size(); n_segs += s.segs.size(); plane_bytes += align16(s.song.plane().size());
    }
    // page-locked: the PCM plane the items point into (owned by `keep`), and the inputs staged for one upload
    void *pcm = nullptr, *in = nullptr;
    const size_t pcm_bytes = std::max<uint64_t>(frames, 1) * 2 * es;
    const size_t tick_bytes = align16(n_ticks * sizeof(afg_mod_tick)), seg_bytes = align16(std::max<uint64_t>(n_segs, 1) * sizeof(afg_mod_segment));
    const size_t in_bytes = tick_bytes + seg_bytes + align16(plane_bytes);
    std::shared_ptr<void> pcm_owner;                       // (collate: the floats go on to the tensor, nothing comes back)
    if (so.fetch() && !(pcm_owner = afg_front::staging_lease(pcm_bytes, &pcm))) return AFG_ERR_OOM;
    std::shared_ptr<void> in_owner = afg_front::staging_lease(in_bytes, &in);
    if (!in_owner) return AFG_ERR_OOM;
    uint8_t *hin = (uint8_t *)in;
    afg_front::parallel_run(M, n_threads, [&](size_t j) {
        const Sim &s = sims[mods[j]];
        const afg_mod_song &g = songs[j];
        if (!s.ticks.empty()) std::memcpy(hin + g.tick_base * sizeof(afg_mod_tick), s.ticks.data(), s.ticks.size() * sizeof(afg_mod_tick));
        if (!s.segs.empty()) std::memcpy(hin + tick_bytes + g.seg_base * sizeof(afg_mod_segment), s.segs.data(), s.segs.size() * sizeof(afg_mod_segment));
        std::memcpy(hin + tick_bytes + seg_bytes + g.sample_base, s.song.plane().data(), s.song.plane().size());
    });

    // ---- chunks of songs, about 128 MB of output each: chunk c + 1 is mixed while chunk c comes back ----
    const afg_front::SongChunks chunks(start, end);
    const std::vector<size_t> &first = chunks.first;
    const std::vector<afg_mod_song> rel = chunks.relative(songs);
    DevBuf d_in, d_songs, d_out[2];
    if (int rc = d_in.alloc(in_bytes)) return rc;
    if (int rc = d_songs.alloc(M * sizeof(afg_mod_song))) return rc;
    for (DevBuf &b : d_out) if (int rc = b.alloc(chunks.max_frames * 2 * sizeof(float))) return rc;
    afg_front::WideSlots wide;                             // f64, AFG_SAMPLE_PCM_*, collate: the mixed floats stay on the device and are converted there
    std::vector<afg_front::PackRun> runs;                  // a song is one run of its own samples
    if (so.wide() && so.fetch()) if (int rc = wide.alloc(chunks.max_frames * 2, es)) return rc;
    for (size_t j = 0; j < M && so.runs(); j++) runs.push_back(afg_front::PackRun{ 2 * start[j], 2 * sims[mods[j]].frames, 0, (uint32_t)which[mods[j]], 2 });
    const uint8_t *din = (const uint8_t *)d_in.p;
    const int rc = afg_front::run_chunks(
        chunks.count(),
        [&](hipStream_t up) -> int {                       // everything the mixer reads goes up once
            AFG_HIP_CHECK(hipMemcpyAsync(d_in.p, in, in_bytes, hipMemcpyHostToDevice, up));
            AFG_HIP_CHECK(hipMemcpyAsync(d_songs.p, rel.data(), M * sizeof(afg_mod_song), hipMemcpyHostToDevice, up));
            return AFG_OK;
        },
        /* upload */ nullptr,                              // no per-chunk upload: nothing waits on the host
        [&](size_t c, int slot, hipStream_t up) -> int {
            if (int rc = afg_mod_render_hip((uint32_t)(first[c + 1] - first[c]), (const afg_mod_song *)d_songs.p + first[c],
                                            (const afg_mod_segment *)(din + tick_bytes), (const afg_mod_tick *)din + songs[first[c]].tick_base,
                                            din + tick_bytes + seg_bytes, (float *)d_out[slot].p, up))
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
        it.message = s.capped ? kMessageCapped : nullptr;
        it.format = AFG_FORMAT_MOD;
        it.channels = 2;
        it.samplerate = (float)kRate;
        it.frames = (int64_t)s.frames;
        it.pcm = s.frames && pcm ? (float *)((uint8_t *)pcm + 2 * songs[j].out_frame * es) : nullptr;
    }
    keep = pcm_owner;
    return AFG_OK;
}

}  // namespace afg_mod
