// afg_batch.cpp -- the batch path: decode_parsed, which runs the device stages of a set of parsed files (a batch's, or a
// stream's chunk: afg_stream.cpp); batch_decode_device, the passes over a batch on one device, each codec's staging pass in
// its stage file (afg_batch.h); and the batch entries of the C ABI with their grouping and multi-device sharding.
#include "afg_batch.h"
#include "afg_mod_front.h"
#include "afg_wav_front.h"
#include "afg_xm_front.h"

#include <cstdlib>
#include <mutex>
#include <new>
#include <thread>

using namespace afg_front;

namespace afg_front {

StageCtx stage_ctx(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, const uint8_t *own, unsigned threads,
                   SampleOut so, BatchOut &out)
{
    return StageCtx{ parsed, data, len, own, threads, so, stage_chunks(), out, StageTimer() };
}

// what the caller is told of every file (the PCM offsets are the layouts')
static void fill_metadata(StageCtx &ctx)
{
    for (size_t i = 0; i < ctx.nf(); i++) {
        Parsed &p = ctx.parsed[i];
        Decoded &dcd = ctx.out.files[i];
        const int fmt = dcd.format = ctx.fmt_of(i);
        if (fmt == AFG_FORMAT_FLAC) {
            dcd.channels = (int)p.fi.channels;
            dcd.samplerate = (float)p.fi.sample_rate;
            dcd.frames = (int64_t)(p.flac.out_samples / p.fi.channels);
            dcd.declared_frames = (int64_t)p.fi.total_samples;      // totalSampleCount / channels, stream.d:1631
        } else if (fmt == AFG_FORMAT_MP3) {
            dcd.channels = p.mp3.channels;
            dcd.samplerate = (float)p.mp3.hz;
            dcd.frames = (int64_t)(p.mp3.pcm_samples / (uint64_t)p.mp3.channels);
            dcd.declared_frames = (int64_t)(p.mp3.declared_samples / (uint64_t)p.mp3.channels);   // stream.d:1737
        } else if (fmt == AFG_FORMAT_OGG) {
            dcd.channels = p.ogg.channels;
            dcd.samplerate = (float)p.ogg.sample_rate;
            dcd.frames = (int64_t)p.ogg.pcm_frames;
            dcd.declared_frames = (int64_t)p.ogg.total_samples;    // stb_vorbis_stream_length_in_samples, stream.d:1696
        } else if (fmt == AFG_FORMAT_OPUS) {
            dcd.channels = p.opus.channels;
            dcd.samplerate = 48000.0f;                              // OpusFileCtx.rate (dopus.d:7973)
            dcd.declared_frames = p.opus.declared_frames;           // smpduration(), stream.d:1609
            // the reference never reads past the declared length (stream.d:439-442); the pre-skip samples are not dropped
            dcd.frames = std::min<int64_t>((int64_t)p.opus.pcm_frames, std::max<int64_t>(p.opus.declared_frames, 0));
            if (p.opus.error) {                                     // a packet failed: the read that reaches it reports an error
                dcd.status = AFG_ERR_INVALID;
                dcd.message = kErrorDecoderInitializationFailed;    // (the string stream.d:454 sets)
            }
        } else if (fmt == AFG_FORMAT_QOA) {
            dcd.channels = (int)p.qi.channels;
            dcd.samplerate = (float)p.qi.samplerate;
            dcd.frames = (int64_t)(p.qoa.back().out_off / p.qi.channels) + p.qoa.back().samples;
            dcd.declared_frames = (int64_t)p.qi.samples;
        } else {
            dcd.status = AFG_ERR_UNSUPPORTED;
            dcd.message = p.opus_mode ? kErrorOpusMode : kErrorUnknownFormat;
        }
    }
}

// The device stages for a set of parsed files (afg_batch.h), each handed in with its optional inputs set: every FLAC record
// of the batch in one stage, every QOA frame in another, and so on; the results come back as one plane, laid out FLAC,
// QOA, MP3, Vorbis, Opus.
// so.f64() (afg_read_samples_double, afg_batch_opts.sample_type): the result plane holds doubles.  Every stage's device plane
// -- int32 for FLAC, float for the others -- is widened by afg_pcm_to_f64_hip behind the stage's kernels, on their
// stream, and the doubles are what comes back.  The batch path's MP3 and Opus planes were widened by their own pipelines.
// AFG_SAMPLE_PCM_* (afg_batch_opts.sample_type): the result plane holds samples of 1, 2 or 3 bytes, packed from every
// stage's float plane by afg_pcm_pack_hip at the same place; FLAC restores to float as for a float read.
// Collate mode (afg_batch_decode_to_device): there is no result plane.  afg_collate_hip scatters every stage's float plane
// into the caller's tensor where the other types convert, and the downloads are left out; parsed[i] is batch file i.
int decode_parsed(StageCtx &ctx, FlacDecode &flac, Mp3Decode &mp3, VorbisDecode &ogg, OpusDecode &opus)
{
    const SampleOut &so = ctx.so;
    if (mp3.staged && mp3.staged->blocks && mp3.staged->so != so) { afg::set_error("decode_parsed: the MP3 stage's sample type differs"); return AFG_ERR_INVALID; }
    BatchOut &out = ctx.out;
    out.f64 = so.f64();
    out.files.assign(ctx.nf(), Decoded());
    QoaDecode qoa;
    size_t at = flac.layout(ctx, 0);
    at += qoa.layout(ctx, at);
    const size_t main_floats = at;                           // FLAC and QOA: converted in place of the plane
    at += mp3.layout(ctx, at);
    size_t ogg_floats = 0;
    if (int rc = ogg.layout(ctx, at, &ogg_floats)) return rc;
    at += ogg_floats;
    mp3.deliver_in_place(ctx);
    at += opus.layout(ctx, at);
    out.plane_floats = at;
    if (out.plane_floats) {
        if (so.fetch()) if (int rc = staging_take(out.plane_floats * so.es(), out.plane)) return rc;
        ctx.tm.lap("layout + plane alloc");
        // (the converted planes and the conversion records live out here and in the stages the caller holds: on an early way
        //  out of a stage they are let go only after the device has drained, below them)
        StageDev dev;
        if (int rc = dev.d_out.alloc(out.plane_floats * sizeof(float))) return rc;
        if (so.wide() && so.fetch()) if (int rc = dev.d_out64.alloc(std::max<size_t>(main_floats * so.es(), 16))) return rc;
        struct Drain { bool on; ~Drain() { if (on) (void)hipDeviceSynchronize(); } } drain{ so.wide() };
        if (int rc = flac.run(ctx, dev)) return rc;
        if (int rc = qoa.run(ctx, dev)) return rc;
        if (int rc = mp3.run(ctx, dev)) return rc;
        if (int rc = ogg.run(ctx, dev)) return rc;
        if (int rc = opus.run(ctx, dev)) return rc;
        drain.on = false;                                    // every stage has drained its own streams
    }
    fill_metadata(ctx);
    return AFG_OK;
}

// What a batch result owns: one BatchOut per device the batch ran on.
struct BatchOwner {
    std::vector<std::unique_ptr<BatchOut>> parts;
    std::deque<std::string> messages;                            // the item messages that are not static strings (afg_batch_decode_resampled)
};

BatchResult::~BatchResult() { std::free(items); delete owner; }
int BatchResult::alloc(int n)
{
    owner = new BatchOwner;
    items = (afg_batch_item *)std::calloc((size_t)n, sizeof(afg_batch_item));
    if (!items) return AFG_ERR_OOM;
    n_files = n;
    return AFG_OK;
}
std::deque<std::string> &BatchResult::messages() { return owner->messages; }
int BatchResult::finish(afg_batch_result *out)
{
    out->n_files = n_files;
    out->items = items;
    out->owner = owner;
    items = nullptr; owner = nullptr;
    return AFG_OK;
}

}  // namespace afg_front

namespace {

// The FLAC and QOA files of a batch are complete after pass 1b: their device stage (mostly PCIe time) runs on a second host
// thread while the first parses the MP3 and Ogg files.  Each call of decode_parsed only touches the files it owns.
struct EarlyJob {
    std::thread th;
    int rc = AFG_OK;
    std::string error;
    ~EarlyJob() { if (th.joinable()) th.join(); }
};
void early_decode(EarlyJob &job, int dev, std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *length, const uint8_t *own,
                  SampleOut so, BatchOut &out, const FlacStaging *staged)
{
    try {
        // HIP's current device is per host thread and starts at 0: this thread works for the caller's device
        if (hipSetDevice(dev) != hipSuccess) { afg::set_error("hipSetDevice(%d) failed", dev); job.rc = AFG_ERR_HIP; return; }
        StageCtx early = stage_ctx(parsed, data, length, own, 1 /* no helpers: they are parsing */, so, out);
        FlacDecode early_flac;
        early_flac.staged = staged;
        Mp3Decode no_mp3;
        VorbisDecode no_ogg;
        OpusDecode no_opus;
        job.rc = decode_parsed(early, early_flac, no_mp3, no_ogg, no_opus);
    } catch (...) {
        afg::set_error("out of host memory");
        job.rc = AFG_ERR_OOM;
    }
    if (job.rc) job.error = afg_last_error();
}

// What the caller is told of every file: own_early (optional) marks the files owner.early decoded; the MP3 and Opus planes
// are the owner's either way.
void fill_items(afg_batch_item *items, int n_files, const BatchOut &owner, const uint8_t *own_early, const SampleOut &so)
{
    for (int i = 0; i < n_files; i++) {
        const BatchOut *src = (own_early && own_early[i]) ? owner.early.get() : &owner;
        const Decoded &d = src->files[(size_t)i];
        items[i].status = d.status;
        items[i].message = d.message;
        items[i].format = d.format;
        items[i].channels = d.channels;
        items[i].samplerate = d.samplerate;
        items[i].frames = d.frames;
        const uint8_t *plane = d.in_mp3_plane ? (const uint8_t *)owner.mp3_plane.p
                               : d.in_opus_plane ? (const uint8_t *)owner.opus_plane.p : (const uint8_t *)src->plane.p;
        items[i].pcm = (d.status == AFG_OK && d.frames > 0 && so.fetch()) ? (float *)(plane + d.pcm_off * so.es()) : nullptr;
    }
}

// the files of `unknown` a stage has taken (decoded, or refused with a message of its own) leave the list
void drop_taken(std::vector<int> &unknown, const afg_batch_item *items)
{
    unknown.erase(std::remove_if(unknown.begin(), unknown.end(), [&](int i) { return items[i].status == AFG_OK || items[i].message != kErrorUnknownFormat; }), unknown.end());
}

// Collate mode, every stage drained: the items point at the slabs, and what the files did not fill is padding -- tails, the
// rows a file has no channel for, and the whole slab of a file that failed or starts past its end: whatever a stage may have
// written there (an Opus file whose last packet failed) is overwritten.
int collate_items(const SampleOut &so, afg_batch_item *items, int n_files, StageTimer &tm)
{
    std::vector<int64_t> frames((size_t)n_files, 0);
    std::vector<int> channels((size_t)n_files, 0);
    for (int i = 0; i < n_files; i++) {
        const bool ok = items[i].status == AFG_OK;
        if (ok) { frames[(size_t)i] = items[i].frames; channels[(size_t)i] = items[i].channels; }
        items[i].pcm = ok ? so.d_out + (size_t)i * so.C * so.T : nullptr;
    }
    if (!so.no_pad) {
        CollatePlane padding;
        if (int rc = padding.pad(so, frames, channels, nullptr)) return rc;
        AFG_HIP_CHECK(hipStreamSynchronize(nullptr));
        tm.lap("collate padding");
    }
    return AFG_OK;
}

// The whole batch path for the files handed in, on the calling thread's current device; fills items[0..n_files).
// `parse_done` (optional) is called once, when the host passes that keep every helper thread busy are over and what remains is
// the device stages of decode_parsed: a grouped batch lets its next group start parsing then.
int batch_decode_device(const uint8_t *const *data, const size_t *length, int n_files, int n_threads, afg_batch_item *items,
                        std::unique_ptr<BatchOut> &keep, const std::function<void()> *parse_done = nullptr, SampleOut so = SampleOut())
{
    // so (afg_batch_opts.sample_type, dither, dither_seed): every plane the items point into holds doubles or packed integer
    // samples, made on the device
    // Collate mode: nothing comes back.  Every stage scatters its chunks into so.d_out; what the files did not fill is written
    // as zero runs at the end, when every file's delivered length is known, and the items point at the slabs.  With
    // so.no_pad (afg_batch_decode_resampled: the tensor is a scratch whose reader knows every file's length) they are left out.
    if (int rc = afg::require_device()) return rc;
    int cur_dev = 0;
    AFG_HIP_CHECK(hipGetDevice(&cur_dev));
    StageTimer tm;
    struct ExitLap { StageTimer *t; const char *what; ~ExitLap() { t->lap(what); } } exit_lap{ &tm, "records released (call ends)" };
    const size_t nf = (size_t)n_files;
    std::vector<Parsed> parsed(nf);
    tm.lap("call set-up");
    // default: one thread per physical core of an SMT-2 host (half the logical CPUs).  With one thread per logical
    // CPU the parse stages ran up to 10x longer on a shared 256-CPU box: the stragglers wait for a CPU.
    const unsigned nt = n_threads > 0 ? (unsigned)n_threads : default_threads();
    const unsigned nt_long = n_threads > 0 ? (unsigned)n_threads : sustained_threads();
    std::unique_ptr<BatchOut> owner(new (std::nothrow) BatchOut);         // (in front of the stagings: their pipelines drain first)
    if (!owner) return AFG_ERR_OOM;
    // pass 1: containers with a signature are parsed at once; files of a staged codec (FLAC of declared length, Ogg Vorbis,
    // MP3 candidates) only get an upper bound of their records, so that its pass can parse them straight into one
    // page-locked staging buffer
    FlacStaging flac(nf);
    Mp3Staging mp3(nf);
    OggStaging ogg(nf);
    std::vector<uint8_t> opus_open(nf, 0);
    parallel_for(nf, nt, [&](size_t i) {
        if (!data[i] || !length[i]) return;
        Parsed &p = parsed[i];
        try {
            if (length[i] >= 4 && std::memcmp(data[i], "OggS", 4) == 0) {                             // Opus is tried first (stream.d:1596)
                afg_opus::Reader rd;                                                                  // headers + sizes; decoded in pass 1c
                const afg_opus::Status st = rd.open(data[i], length[i], p.opus);
                if (st == afg_opus::kOpened) { opus_open[i] = 1; return; }
                p.opus = afg_opus::File();
                if (st == afg_opus::kUnsupported) { p.opus_mode = true; return; }
            }
            if (flac.bound(i, data[i], length[i]) != 0) return;                                       // parsed in pass 1b
            p.flac.pack16 = flac_rows_int16();
            if (flac_parse(data[i], length[i], p.fi, p.flac)) { p.format = AFG_FORMAT_FLAC; return; }
            p.flac = FlacRecords();
            if (qoa_parse(data[i], length[i], p.qi, p.qoa)) { p.format = AFG_FORMAT_QOA; return; }
            if (ogg.bound(i, data[i], length[i]) != 0) return;                                        // parsed in pass 1b
            mp3.bound(i, data[i], length[i]);
        } catch (...) { p = Parsed(); }
    });
    tm.lap("pass 1: flac / qoa parse, ogg + mp3 bounds");
    flac.prefix(4);                                              // 16-byte aligned planes
    mp3.prefix(1);
    ogg.prefix(1);
    if (int rc = flac.parse(parsed, data, length, nt, tm)) return rc;
    // ---- pass 1c: Ogg Opus, decoded by all helper threads and queued chunk by chunk (afg_opus_stage.cpp)
    std::vector<size_t> opus_pcm_at;
    bool opus_staged = false;
    if (int rc = opus_pipeline(parsed, data, length, opus_open, nt_long, so, owner->opus_plane, opus_pcm_at, &opus_staged, tm)) return rc;
    // the FLAC and QOA files are complete now: they go to the second host thread (EarlyJob)
    std::vector<uint8_t> own_early(nf, 0), own_late(nf, 1);
    size_t n_early = 0;
    for (size_t i = 0; i < nf; i++)
        if (parsed[i].format == AFG_FORMAT_FLAC || parsed[i].format == AFG_FORMAT_QOA) { own_early[i] = 1; own_late[i] = 0; n_early++; }
    EarlyJob early_job;
    const bool split = n_early && (mp3.total || ogg.total);
    if (split) {
        owner->early.reset(new BatchOut);
        early_job.th = std::thread(early_decode, std::ref(early_job), cur_dev, std::ref(parsed), data, length, own_early.data(), so,
                                   std::ref(*owner->early), &flac);
    }
    // MP3: parsed chunk by chunk into its staging, every chunk's device work queued behind it -- and the Ogg Vorbis files
    // parsed into theirs while the MP3 chunks are still moving
    if (int rc = mp3.open(owner->mp3_plane, so, tm)) return rc;
    mp3.parse_and_submit(parsed, data, length, nt, tm);
    if (int rc = ogg.parse(parsed, data, length, nt, tm)) return rc;
    if (int rc = mp3.close(tm)) return rc;
    if (parse_done) (*parse_done)();
    StageCtx late = stage_ctx(parsed, data, length, split ? own_late.data() : nullptr, nt, so, *owner);
    FlacDecode late_flac;
    if (!split) late_flac.staged = &flac;                        // (every stage asks its staging whether the files are in it)
    Mp3Decode late_mp3;
    late_mp3.staged = &mp3;
    VorbisDecode late_ogg;
    late_ogg.staged = &ogg;
    OpusDecode late_opus;
    if (opus_staged) late_opus.done_at = opus_pcm_at.data();
    int rc = decode_parsed(late, late_flac, late_mp3, late_ogg, late_opus);
    tm.lap("decode_parsed total");
    if (split) {
        early_job.th.join();
        tm.lap("flac / qoa thread joined");
        if (!rc && early_job.rc) { afg::set_error("%s", early_job.error.c_str()); rc = early_job.rc; }
    }
    if (rc) return rc;
    fill_items(items, n_files, *owner, split ? own_early.data() : nullptr, so);
    // MOD is probed last (stream.d:1796): files no other front-end took go to its stage
    std::vector<int> unknown;
    for (int i = 0; i < n_files; i++)
        if (items[i].status == AFG_ERR_UNSUPPORTED && items[i].message == kErrorUnknownFormat) unknown.push_back(i);
    // WAV comes well before either (stream.d:1638); no probe between it and them takes a file its scan accepts (QOA and
    // Ogg have their own magic, looks_like_mp3 declines RIFF), so its stage can run here, on the files nothing took
    if (int wrc = afg_wav::batch_stage(data, length, unknown, (int)nt, items, owner->wav_plane, so)) return wrc;
    tm.lap("wav stage");
    drop_taken(unknown, items);
    // ... and XM directly before it (stream.d:1751)
    if (int xrc = afg_xm::batch_stage(data, length, unknown, (int)nt, items, owner->xm_plane, so)) return xrc;
    tm.lap("xm stage");
    drop_taken(unknown, items);
    if (int mrc = afg_mod::batch_stage(data, length, unknown, (int)nt, items, owner->mod_plane, so)) return mrc;
    tm.lap("mod stage");
    if (so.collate()) if (int crc = collate_items(so, items, n_files, tm)) return crc;
    keep = std::move(owner);
    tm.lap("items filled");
    return AFG_OK;
}

// ---- which devices: none named -- the caller's current one (an empty list) ----
int which_devices(const afg_batch_opts *opts, std::vector<int> &devs)
{
    const int want = opts ? opts->n_devices : 0;
    if (want == 0) return AFG_OK;
    const int visible = afg_device_count();
    if (visible <= 0) { afg::set_error("no HIP device available; this library has no CPU fallback"); return AFG_ERR_NO_DEVICE; }
    if (want < 0) for (int d = 0; d < visible; d++) devs.push_back(d);
    else for (int k = 0; k < want; k++) {
        const int d = opts->devices ? opts->devices[k] : k;
        if (d < 0 || d >= visible) { afg::set_error("afg_batch_decode_ex: device %d of %d visible", d, visible); return AFG_ERR_INVALID; }
        devs.push_back(d);
    }
    if (devs.size() > 16) { afg::set_error("afg_batch_decode_ex: at most 16 devices"); return AFG_ERR_INVALID; }
    return AFG_OK;
}

// One device, the calling thread's current one.
// A large batch runs as a pipeline of GROUPS of files (round 6): while one group's device stages run -- the host mostly
// waiting -- the next group is parsed.  Two host threads take the groups in turn; a token serialises their parse passes
// (one set of helper threads at a time), handed on when a group reaches its device stages.  Results do not depend on
// the grouping (files are independent).  afg_dev_option("batch_groups", n) forces n (1: off).
int run_grouped(const uint8_t *const *data, const size_t *length, int n_files, int n_threads, afg_batch_item *items,
                std::vector<std::unique_ptr<BatchOut>> &parts, const SampleOut &so)
{
    size_t total_bytes = 0;
    for (int i = 0; i < n_files; i++) total_bytes += length[i];
    // By default only batches of (almost only) native FLAC and Ogg Vorbis files, from 512 files and 16 MB up, in 4 groups:
    // their calls are a parse pass followed by device stages; the MP3 and Opus paths overlap their parsing with their own
    // transfers already and lose 5-10 % to the split (2048-file batches, 24 helper threads, samples/s ungrouped -> 4 groups:
    // Vorbis 5.3e9 -> 6.2e9, FLAC 5.0e9 -> 5.7e9, MP3 6.5e9 -> 6.0e9, Opus 2.5e9 -> 2.3e9, mixed 4.9e9 -> 4.5e9).
    long groups = afg::dev_option(afg::kDevBatchGroups);
    if (groups <= 0) {
        groups = 1;
        if (n_files >= 512 && total_bytes >= ((size_t)16 << 20)) {
            int staged = 0;
            for (int i = 0; i < n_files; i++) {
                const uint8_t *b = data[i];
                const size_t n = length[i];
                if (n >= 4 && !std::memcmp(b, "fLaC", 4)) staged++;
                else if (n >= 28 && !std::memcmp(b, "OggS", 4) && n >= (size_t)27 + b[26] + 7 &&
                         !std::memcmp(b + 27 + b[26], "\x01vorbis", 7)) staged++;      // (the first page's payload: the identification header)
            }
            if ((size_t)staged * 10 >= (size_t)n_files * 9) groups = 4;
        }
    }
    if (groups > n_files) groups = n_files;
    if (groups <= 1) {
        parts.emplace_back();
        return batch_decode_device(data, length, n_files, n_threads, items, parts.back(), nullptr, so);
    }
    const size_t G = (size_t)groups;
    parts.resize(G);
    std::vector<int> first(G + 1, n_files);          // contiguous ranges of about equal compressed size
    {
        size_t acc = 0, g = 0;
        first[0] = 0;
        for (int i = 0; i < n_files && g + 1 < G; i++) {
            acc += length[i];
            if (acc * G >= total_bytes * (g + 1)) first[++g] = i + 1;
        }
    }
    int dev = 0;
    AFG_HIP_CHECK(hipGetDevice(&dev));
    std::mutex token;
    std::atomic<bool> failed{ false };
    struct Job { int rc = AFG_OK; std::string error; } jobs[2];
    auto work = [&](int w) {
        try {
            if (w && hipSetDevice(dev) != hipSuccess) { jobs[w].rc = AFG_ERR_HIP; jobs[w].error = "hipSetDevice failed"; failed = true; return; }
            HelperScope scope(w ? HelperScope::kGroup : HelperScope::kGroupLead, dev);
            for (size_t g = (size_t)w; g < G && !failed; g += 2) {
                const int f0 = first[g], f1 = first[g + 1];
                if (f1 <= f0) continue;
                std::unique_lock<std::mutex> lk(token);
                bool released = false;
                const std::function<void()> done = [&] { if (!released) { released = true; lk.unlock(); } };
                const int r = batch_decode_device(data + f0, length + f0, f1 - f0, n_threads, items + f0, parts[g], &done, so);
                done();
                if (r) { jobs[w].rc = r; jobs[w].error = afg_last_error(); failed = true; }
            }
        } catch (...) {
            jobs[w].rc = AFG_ERR_OOM; jobs[w].error = "out of host memory"; failed = true;
        }
    };
    {
        struct Joiner { std::thread th; ~Joiner() { if (th.joinable()) th.join(); } } j;
        j.th = std::thread(work, 1);
        work(0);
    }
    for (const Job &jb : jobs)
        if (jb.rc) { afg::set_error("%s", jb.error.c_str()); return jb.rc; }
    return AFG_OK;
}

// Files are independent (stream.d:1363-1434 is all per-instance): the batch shards by file, longest file first
// onto the least loaded device (compressed bytes stand for decode work), no exchange between devices.
int run_sharded(const std::vector<int> &devs, const uint8_t *const *data, const size_t *length, int n_files, int n_threads,
                afg_batch_item *items, std::vector<std::unique_ptr<BatchOut>> &owned, const SampleOut &so)
{
    const size_t nd = devs.size();
    std::vector<size_t> order((size_t)n_files);
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return length[a] > length[b]; });
    std::vector<std::vector<size_t>> mine(nd);
    std::vector<uint64_t> load(nd, 0);
    for (size_t f : order) {
        size_t best = 0;
        for (size_t k = 1; k < nd; k++) if (load[k] < load[best]) best = k;
        mine[best].push_back(f);
        load[best] += length[f] + 1;
    }
    for (auto &v : mine) std::sort(v.begin(), v.end());
    const unsigned total_threads = n_threads > 0 ? (unsigned)n_threads : default_threads();
    const int per_dev_threads = (int)std::max<unsigned>(1u, total_threads / (unsigned)nd);
    owned.resize(nd);
    struct Part {
        std::vector<const uint8_t *> data;
        std::vector<size_t> len;
        std::vector<afg_batch_item> items;
        int rc = AFG_OK;
        std::string error;
    };
    std::vector<Part> parts(nd);
    int caller_dev = 0;
    AFG_HIP_CHECK(hipGetDevice(&caller_dev));
    auto run_part = [&](size_t k) {
        Part &p = parts[k];
        try {
            for (size_t f : mine[k]) { p.data.push_back(data[f]); p.len.push_back(length[f]); }
            p.items.assign(mine[k].size(), afg_batch_item{});
            if (mine[k].empty()) return;
            if (hipSetDevice(devs[k]) != hipSuccess) { p.rc = AFG_ERR_HIP; p.error = "hipSetDevice failed"; return; }
            HelperScope scope(HelperScope::kDevice, (int)k);
            p.rc = batch_decode_device(p.data.data(), p.len.data(), (int)mine[k].size(), per_dev_threads, p.items.data(), owned[k], nullptr, so);
            if (p.rc) p.error = afg_last_error();
        } catch (...) {
            p.rc = AFG_ERR_OOM; p.error = "out of host memory";
        }
    };
    {
        // joins on every way out: a thread that cannot be created after others have started must not take the
        // process down (std::terminate on a joinable std::thread) instead of returning AFG_ERR_OOM
        struct Joiner {
            std::vector<std::thread> th;
            ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); }
        } j;
        j.th.reserve(nd);
        for (size_t k = 1; k < nd; k++) j.th.emplace_back(run_part, k);
        run_part(0);
    }
    (void)hipSetDevice(caller_dev);
    for (size_t k = 0; k < nd; k++)
        if (parts[k].rc) { afg::set_error("device %d: %s", devs[k], parts[k].error.c_str()); return parts[k].rc; }
    for (size_t k = 0; k < nd; k++)
        for (size_t j = 0; j < mine[k].size(); j++) items[mine[k][j]] = parts[k].items[j];
    return AFG_OK;
}

}  // namespace

extern "C" {

int afg_set_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        afg::set_error("no HIP device available (%s); this library has no CPU fallback", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return AFG_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        afg::set_error("afg_set_device(%d): %d device(s) visible", device, n);
        return AFG_ERR_INVALID;
    }
    AFG_HIP_CHECK(hipSetDevice(device));
    return afg::require_device();
}

int afg_get_device(void)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        afg::set_error("hipGetDevice failed: %s", hipGetErrorString(e));
        return e == hipErrorNoDevice ? AFG_ERR_NO_DEVICE : AFG_ERR_HIP;
    }
    return dev;
}

int afg_batch_decode_ex(const uint8_t *const *data, const size_t *length, int n_files, const afg_batch_opts *opts, afg_batch_result *out)
{
    try {
        if (!out || n_files < 0 || (n_files && (!data || !length))) return AFG_ERR_INVALID;
        out->n_files = 0; out->items = nullptr; out->owner = nullptr;
        // (a caller built before sample_type was appended hands in the struct up to `devices`: it gets float, as it always did)
        if (opts && opts->struct_size < offsetof(afg_batch_opts, sample_type)) { afg::set_error("afg_batch_opts.struct_size too small"); return AFG_ERR_INVALID; }
        uint32_t sample_type = AFG_SAMPLE_F32;
        if (opts && opts->struct_size >= offsetof(afg_batch_opts, sample_type) + sizeof(uint32_t)) sample_type = opts->sample_type;
        if (sample_type > AFG_SAMPLE_PCM_S24) {
            afg::set_error("afg_batch_opts.sample_type %u: AFG_SAMPLE_F32 (0), AFG_SAMPLE_F64 (1) or AFG_SAMPLE_PCM_S8 / _S16 / _S24 (2 - 4)", sample_type);
            return AFG_ERR_INVALID;
        }
        // (dither and dither_seed were appended together: a struct that ends before dither_seed means no dither)
        int dither = AFG_DITHER_OFF;
        uint32_t dither_seed = 0;
        if (opts && opts->struct_size >= offsetof(afg_batch_opts, dither_seed) + sizeof(uint32_t)) { dither = opts->dither; dither_seed = opts->dither_seed; }
        if (dither == AFG_DITHER_LIBC) {
            afg::set_error("afg_batch_opts.dither: libc rand() dither has no defined draw order across files; use AFG_DITHER_LCG31 or AFG_DITHER_OFF");
            return AFG_ERR_INVALID;
        }
        if (dither != AFG_DITHER_OFF && dither != AFG_DITHER_LCG31) {
            afg::set_error("afg_batch_opts.dither %d: AFG_DITHER_OFF (0) or AFG_DITHER_LCG31 (2)", dither);
            return AFG_ERR_INVALID;
        }
        SampleOut so;
        so.type = sample_type;
        so.dither = so.pcm() && dither == AFG_DITHER_LCG31;       // (the float types never dither)
        so.seed = so.dither ? dither_seed : 0;
        if (n_files == 0) return AFG_OK;
        std::vector<int> devs;
        if (int rc = which_devices(opts, devs)) return rc;
        const int n_threads = opts ? opts->n_threads : 0;
        BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        if (devs.size() <= 1) {
            // one device: the caller's current one, or the one named
            int restore = -1;
            if (devs.size() == 1) {
                int cur = 0;
                AFG_HIP_CHECK(hipGetDevice(&cur));
                if (cur != devs[0]) { restore = cur; AFG_HIP_CHECK(hipSetDevice(devs[0])); }
            }
            const int rc = run_grouped(data, length, n_files, n_threads, res.items, res.owner->parts, so);
            if (restore >= 0) (void)hipSetDevice(restore);
            if (rc) return rc;
        } else {
            if (int rc = run_sharded(devs, data, length, n_files, n_threads, res.items, res.owner->parts, so)) return rc;
        }
        return res.finish(out);
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

int afg_batch_decode(const uint8_t *const *data, const size_t *length, int n_files, int n_threads, afg_batch_result *out)
{
    afg_batch_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o);
    o.n_threads = n_threads;
    return afg_batch_decode_ex(data, length, n_files, &o, out);
}

int afg_batch_decode_to_device(const uint8_t *const *data, const size_t *length, int n_files, const afg_collate_opts *opts,
                               float *d_out, afg_batch_result *out)
{
    try {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (!opts || !d_out || !out) { afg::set_error("afg_batch_decode_to_device: NULL %s", !opts ? "opts" : !d_out ? "d_out" : "out"); return AFG_ERR_INVALID; }
        out->n_files = 0; out->items = nullptr; out->owner = nullptr;
        if (opts->struct_size < offsetof(afg_collate_opts, first_frame) + sizeof(const int64_t *)) {
            afg::set_error("afg_collate_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        if (opts->channels == 0 || opts->frames == 0) {
            afg::set_error("afg_collate_opts: channels and frames must be at least 1 (%u, %u)", opts->channels, opts->frames);
            return AFG_ERR_INVALID;
        }
        if (n_files < 0 || (n_files && (!data || !length))) { afg::set_error("afg_batch_decode_to_device: n_files %d, or no file list", n_files); return AFG_ERR_INVALID; }
        for (int i = 0; i < n_files && opts->first_frame; i++)
            if (opts->first_frame[i] < 0) { afg::set_error("afg_collate_opts.first_frame[%d] is negative", i); return AFG_ERR_INVALID; }
        if (n_files == 0) return AFG_OK;
        if ((uint64_t)opts->channels * opts->frames > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_to_device: a tensor of %d x %u x %u floats", n_files, opts->channels, opts->frames);
            return AFG_ERR_INVALID;
        }
        SampleOut so;
        so.type = afg_front::kSampleCollate;
        so.d_out = d_out;
        so.C = opts->channels;
        so.T = opts->frames;
        so.n_files = (uint64_t)n_files;
        so.first_frame = opts->first_frame;
        BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        // one pass over the whole list on the current device: a slab's place follows from the file's index in it
        res.owner->parts.emplace_back();
        if (int rc = batch_decode_device(data, length, n_files, opts->n_threads, res.items, res.owner->parts.back(), nullptr, so)) return rc;
        return res.finish(out);
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

}  // extern "C"

namespace afg_front {

// What afg_batch_decode_resampled checks of its options behind struct_size, before any device call; fills in the job.
int resampled_check(const afg_resample_opts *opts, const uint8_t *const *data, const size_t *length, int n_files, ResampleJob &job)
{
    if (opts->channels == 0 || opts->frames == 0) {
        afg::set_error("afg_resample_opts: channels and frames must be at least 1 (%u, %u)", opts->channels, opts->frames);
        return AFG_ERR_INVALID;
    }
    constexpr uint32_t kMaxRate = 1u << 20;
    if (opts->samplerate == 0 || opts->samplerate > kMaxRate) {
        afg::set_error("afg_resample_opts.samplerate %u: 1 .. %u Hz", opts->samplerate, kMaxRate);
        return AFG_ERR_INVALID;
    }
    if (opts->mono > 1 || (opts->mono && opts->channels != 1)) {
        afg::set_error("afg_resample_opts.mono %u with %u channels: mono is 0 or 1, and a mono tensor has one channel", opts->mono, opts->channels);
        return AFG_ERR_INVALID;
    }
    if (opts->in_channels > 0xffff) { afg::set_error("afg_resample_opts.in_channels %u: at most 65535 (0 means 2)", opts->in_channels); return AFG_ERR_INVALID; }
    if (opts->max_in_rate > kMaxRate) { afg::set_error("afg_resample_opts.max_in_rate %u: at most %u Hz (0 means 48000)", opts->max_in_rate, kMaxRate); return AFG_ERR_INVALID; }
    if (opts->lowpass_width > 64) { afg::set_error("afg_resample_opts.lowpass_width %u: at most 64 (0 means 6)", opts->lowpass_width); return AFG_ERR_INVALID; }
    if (n_files < 0 || (n_files && (!data || !length))) { afg::set_error("afg_batch_decode_resampled: n_files %d, or no file list", n_files); return AFG_ERR_INVALID; }
    for (int i = 0; i < n_files && opts->first_frame; i++)
        if (opts->first_frame[i] < 0) { afg::set_error("afg_resample_opts.first_frame[%d] is negative", i); return AFG_ERR_INVALID; }
    job.C = opts->channels;
    job.T = opts->frames;
    job.samplerate = opts->samplerate;
    job.mono = opts->mono != 0;
    job.Z = opts->lowpass_width ? opts->lowpass_width : 6;
    job.in_channels = opts->in_channels ? opts->in_channels : 2;
    job.max_in_rate = opts->max_in_rate ? opts->max_in_rate : 48000;
    job.plan();
    if (job.T_s > 0xffffffffull) {
        afg::set_error("afg_batch_decode_resampled: %u frames at %u Hz from files of up to %u Hz: a scratch row of 2^32 floats or more", job.T,
                       job.samplerate, job.max_in_rate);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// The resampled tensor of a checked call into d_out; items (n_files of them, zeroed) and messages as the entry returns them.
int resampled_run(const ResampleJob &job, const afg_resample_opts *opts, const uint8_t *const *data, const size_t *length, int n_files,
              float *d_out, afg_batch_item *items, std::deque<std::string> &messages)
{
    if ((uint64_t)opts->channels * opts->frames > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
        afg::set_error("afg_batch_decode_resampled: a tensor of %d x %u x %u floats", n_files, opts->channels, opts->frames);
        return AFG_ERR_INVALID;
    }
    const uint64_t slab_bytes = (uint64_t)job.R_s * job.T_s * sizeof(float);
    const size_t per_list = sublist_size(n_files, slab_bytes, afg::kDevResampleScratchBytes);
    // scratch frame 0 of a file: H frames ahead of its first frame, as far as the file reaches
    std::vector<int64_t> frame0((size_t)n_files, 0);
    for (int i = 0; i < n_files && opts->first_frame; i++) frame0[(size_t)i] = std::max<int64_t>(opts->first_frame[i] - (int64_t)job.H, 0);
    if (int rc = afg::require_device()) return rc;
    afg_front::ResamplePlane plane;                           // (declared in front of the drain: it holds what the uploads read)
    afg_front::DevBuf scratch;
    NullStreamDrain drain;
    if (int rc = scratch.alloc((size_t)(per_list * slab_bytes))) return rc;
    SampleOut so;
    so.type = afg_front::kSampleCollate;
    so.d_out = (float *)scratch.p;
    so.C = job.R_s;
    so.T = (uint32_t)job.T_s;
    so.no_pad = true;
    for (size_t f0 = 0; f0 < (size_t)n_files; f0 += per_list) {
        const size_t n = std::min(per_list, (size_t)n_files - f0);
        so.n_files = n;
        so.first_frame = frame0.data() + f0;
        // the collate pass at the files' own rates: a slab's place follows from the file's index in the sublist.  It returns
        // with its streams drained; the items point at nothing it owns (messages are static), so its part is let go.
        std::unique_ptr<BatchOut> part;
        if (int rc = batch_decode_device(data + f0, length + f0, (int)n, opts->n_threads, items + f0, part, nullptr, so)) return rc;
        if (int rc = plane.launch(job, (const float *)scratch.p, items + f0, n, opts->first_frame ? opts->first_frame + f0 : nullptr,
                                  frame0.data() + f0, d_out + f0 * (size_t)job.C * job.T, messages, nullptr)) return rc;
        AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
    }
    return AFG_OK;
}

}  // namespace afg_front

extern "C" {

int afg_batch_decode_resampled(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                               float *d_out, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        afg_front::ResampleJob job;
        if (int rc = afg_front::entry_args("afg_batch_decode_resampled", { { "opts", opts }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (int rc = afg_front::resampled_opts_check(opts, data, length, n_files, job)) return rc;
        if (n_files == 0) return AFG_OK;
        afg_front::BatchResult res;
        if (int rc = res.alloc(n_files)) return rc;
        if (int rc = afg_front::resampled_run(job, opts, data, length, n_files, d_out, res.items, res.messages())) return rc;
        return res.finish(out);
    });
}

void afg_batch_free(afg_batch_result *r)
{
    if (!r) return;
    StageTimer tm;
    std::free(r->items);
    delete (BatchOwner *)r->owner;
    r->items = nullptr; r->owner = nullptr; r->n_files = 0;
    tm.lap("afg_batch_free");
}

}  // extern "C"
