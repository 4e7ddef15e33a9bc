// afg_stage.cpp -- the shared half of the host stages (afg_stage.h).
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cstring>

namespace afg_front {

int DevBuf::alloc(size_t bytes)
{
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) cur = 0;
    if (p && cap >= bytes && dev == cur) return AFG_OK;
    release();
    if (int rc = devpool_take(bytes, &p, &cap)) { p = nullptr; cap = 0; return rc; }
    dev = cur;
    if (bytes && poison_alloc()) {
        (void)hipMemset(p, 0xff, bytes);
        (void)hipStreamSynchronize(nullptr);
    }
    return AFG_OK;
}

bool DevBuf::here() const
{
    int cur = 0;
    return p && hipGetDevice(&cur) == hipSuccess && dev == cur;
}

void DevBuf::release()
{
    if (p) devpool_give(p, cap, dev);
    p = nullptr; cap = 0; dev = -1;
}

namespace {
void destroy_on(int dev, hipStream_t st)
{
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    (void)hipStreamDestroy(st);
    if (cur != dev && cur >= 0) (void)hipSetDevice(cur);
}
}  // namespace

HandleStream::~HandleStream() { if (stream) destroy_on(dev, stream); }

int HandleStream::current(hipStream_t *st, bool *moved)
{
    int cur = 0;
    AFG_HIP_CHECK(hipGetDevice(&cur));
    if (stream && dev != cur) {
        destroy_on(dev, stream);
        stream = nullptr;
        if (moved) *moved = true;
    }
    if (!stream) {
        AFG_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        dev = cur;
    }
    *st = stream;
    return AFG_OK;
}

int F64Plane::launch(uint32_t kind, const void *d_in, uint64_t count, double *d_out, hipStream_t st)
{
    if (count == 0) return AFG_OK;
    afg_wav_span &sp = rec;                                  // the upload's source lives as long as the object
    std::memset(&sp, 0, sizeof(sp));
    sp.count = count;
    sp.kind = kind;
    const uint64_t tiles = afg_wav_layout(&sp, 1);
    if (int rc = span.alloc(sizeof(sp))) return rc;
    AFG_HIP_CHECK(hipMemcpyAsync(span.p, &sp, sizeof(sp), hipMemcpyHostToDevice, st));
    return afg_pcm_to_f64_hip(1, (const afg_wav_span *)span.p, tiles, (const uint8_t *)d_in, count * f64_kind_bytes(kind), d_out, count, st);
}

uint64_t stage_chunk_samples(uint64_t dflt)
{
    const long v = afg::dev_option(afg::kDevStageChunkSamples);
    return v > 0 ? (uint64_t)v : dflt;
}

void sort_runs(std::vector<PackRun> &runs)
{
    std::sort(runs.begin(), runs.end(), [](const PackRun &x, const PackRun &y) { return x.at < y.at; });
}

int PackPlane::launch(const SampleOut &out, const float *d_in, uint8_t *d_out, uint64_t origin, uint64_t c0, uint64_t n,
                      const std::vector<PackRun> &runs, hipStream_t st)
{
    if (n == 0) return AFG_OK;
    const uint64_t B = out.es(), c1 = c0 + n;
    recs.clear();                                            // the upload's source lives as long as the object
    auto add = [&](uint64_t at, uint64_t count, uint64_t sample0) {
        afg_pcm_pack_span sp;
        std::memset(&sp, 0, sizeof(sp));
        sp.in_off = at - origin;
        sp.out_off = (at - origin) * B;
        sp.count = count;
        sp.draw0 = 2 * sample0;
        sp.seed = out.seed;
        sp.format = out.wav_format();
        sp.dither = out.dither ? 1 : 0;
        recs.push_back(sp);
    };
    if (!out.dither) {
        add(c0, n, 0);
    } else {
        // the first run that ends behind c0, then every run that starts before c1
        auto it = std::upper_bound(runs.begin(), runs.end(), c0, [](uint64_t v, const PackRun &r) { return v < r.at + r.count; });
        for (; it != runs.end() && it->at < c1; ++it) {
            const uint64_t a = std::max(it->at, c0), b = std::min(it->at + it->count, c1);
            if (a < b) add(a, b - a, it->sample0 + (a - it->at));
        }
        if (recs.empty()) return AFG_OK;
    }
    const uint64_t tiles = afg_pcm_pack_layout(recs.data(), recs.size());
    if (int rc = upload_records(spans, recs, st)) return rc;
    return afg_pcm_pack_hip(recs.size(), (const afg_pcm_pack_span *)spans.p, tiles, d_in, c1 - origin, d_out, (c1 - origin) * B, st);
}

int CollatePlane::submit(const SampleOut &out, const float *d_in, uint64_t in_floats, hipStream_t st)
{
    if (recs.empty()) return AFG_OK;
    const uint64_t tiles = afg_collate_layout(recs.data(), recs.size());
    if (int rc = upload_records(spans, recs, st)) return rc;
    return afg::collate_launch(recs.data(), recs.size(), (const afg_collate_span *)spans.p, tiles, d_in, in_floats, out.d_out,
                               out.n_files * out.C * out.T, st);
}

int CollatePlane::launch(const SampleOut &out, const float *d_in, uint64_t origin, uint64_t c0, uint64_t n, const std::vector<PackRun> &runs, hipStream_t st)
{
    if (n == 0) return AFG_OK;
    const uint64_t c1 = c0 + n;
    recs.clear();                                            // the upload's source lives as long as the object
    // the first run that ends behind c0, then every run that starts before c1
    auto it = std::upper_bound(runs.begin(), runs.end(), c0, [](uint64_t v, const PackRun &r) { return v < r.at + r.count; });
    for (; it != runs.end() && it->at < c1; ++it) {
        uint64_t a = std::max(it->at, c0), b = std::min(it->at + it->count, c1);
        if (a >= b || it->channels == 0 || it->channels > 0xffff || it->file >= out.n_files) continue;
        // only the samples of frames [first_frame, first_frame + T) get a tile: a crop of a long file launches the crop
        const uint64_t ff = out.first_frame ? (uint64_t)out.first_frame[it->file] : 0;
        const unsigned __int128 w0 = (unsigned __int128)ff * it->channels, w1 = w0 + (unsigned __int128)out.T * it->channels;
        const uint64_t s_a = it->sample0 + (a - it->at), s_b = it->sample0 + (b - it->at);    // the piece, in file samples
        if (w0 >= s_b || w1 <= s_a) continue;
        if (w0 > s_a) a += (uint64_t)w0 - s_a;
        if (w1 < s_b) b -= s_b - (uint64_t)w1;
        afg_collate_span sp;
        std::memset(&sp, 0, sizeof(sp));
        sp.in_off = a - origin;
        sp.count = b - a;
        sp.sample0 = it->sample0 + (a - it->at);
        sp.out_off = (uint64_t)it->file * out.C * out.T;
        sp.first_frame = (int64_t)ff;
        sp.frames = out.T;
        sp.channels = (uint16_t)it->channels;
        sp.out_channels = (uint16_t)std::min<uint32_t>(out.C, 0xffff);   // (a file has 65535 channels at the most: the rows behind are padding)
        recs.push_back(sp);
    }
    return submit(out, d_in, c1 - origin, st);
}

int CollatePlane::pad(const SampleOut &out, const std::vector<int64_t> &frames, const std::vector<int> &channels, hipStream_t st)
{
    recs.clear();
    const uint64_t C = out.C, T = out.T;
    auto zero = [&](uint64_t at, uint64_t count) {
        if (!count) return;
        afg_collate_span sp;
        std::memset(&sp, 0, sizeof(sp));
        sp.out_off = at;
        sp.count = count;
        recs.push_back(sp);
    };
    for (uint64_t i = 0; i < out.n_files; i++) {
        const uint64_t slab = i * C * T;
        const int64_t ff = out.first_frame ? out.first_frame[i] : 0;
        const uint64_t rows = std::min<uint64_t>((uint64_t)std::max(channels[i], 0), C);
        const uint64_t filled = rows && frames[i] > ff ? std::min<uint64_t>((uint64_t)(frames[i] - ff), T) : 0;   // per row
        if (filled == 0) { zero(slab, C * T); continue; }
        for (uint64_t k = 0; k < rows && filled < T; k++) zero(slab + k * T + filled, T - filled);
        zero(slab + rows * T, (C - rows) * T);
    }
    return submit(out, nullptr, 0, st);
}

int SampleConv::launch(const SampleOut &out, uint32_t kind, const void *d_in, uint64_t origin, uint64_t c0, uint64_t n, void *d_out,
                       const std::vector<PackRun> &runs, hipStream_t st)
{
    if (out.collate()) {
        collated.emplace_back(new CollatePlane);
        return collated.back()->launch(out, (const float *)d_in, origin, c0, n, runs, st);
    }
    if (out.pcm()) {
        packs.emplace_back(new PackPlane);
        return packs.back()->launch(out, (const float *)d_in, (uint8_t *)d_out, origin, c0, n, runs, st);
    }
    if (!out.f64()) return AFG_OK;
    widen.emplace_back(new F64Plane);
    return widen.back()->launch(kind, (const uint8_t *)d_in + (c0 - origin) * 4, n, (double *)d_out + (c0 - origin), st);
}

int WideSlots::alloc(size_t samples, size_t es)
{
    for (DevBuf &b : buf) if (int rc = b.alloc(std::max<size_t>(samples * es, 16))) return rc;
    return AFG_OK;
}

void StageStreams::take(bool three)
{
    const hipError_t got = streams_take(&up, &down, three ? &mid : nullptr);
    if (e == hipSuccess) e = got;
}

void StageStreams::chain(hipStream_t from, hipStream_t to)
{
    if (e != hipSuccess) return;
    drained = false;
    hipEvent_t ev = nullptr;
    e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return;
    events.push_back(ev);
    e = hipEventRecord(ev, from);
    if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
}

void StageStreams::sync(hipStream_t st)
{
    if (!st) return;
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
}

void StageStreams::drain(const std::function<void()> &uploads_done)
{
    sync(up);
    sync(mid);
    if (uploads_done) uploads_done();
    sync(down);
    drained = true;
}

void StageStreams::release()
{
    if (!up && !down && !mid) return;
    if (!drained) {
        const hipError_t first = e;
        drain();
        e = first;                                           // (what the stage saw, not what this last wait says)
    }
    for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
    events.clear();
    streams_give(up, down, mid);
    up = down = mid = nullptr;
    drained = false;
}

int PlaneFetch::run(const void *d_plane, uint32_t kind, uint64_t count, void *out, bool f64, hipStream_t st)
{
    const size_t bytes = (size_t)count * (f64 ? sizeof(double) : (size_t)f64_kind_bytes(kind));
    const void *src = d_plane;
    if (f64) {
        if (int rc = wide.alloc(std::max<size_t>(bytes, 16))) return rc;
        if (int rc = conv.launch(kind, d_plane, count, (double *)wide.p, st)) return rc;
        src = wide.p;
    }
    if (!out) { bounce.resize(bytes); out = bounce.data(); }
    AFG_HIP_CHECK(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, st));
    AFG_HIP_CHECK(hipStreamSynchronize(st));
    return AFG_OK;
}

namespace {
struct Events {
    hipEvent_t e[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    ~Events() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); }
};
}  // namespace

int run_chunks(size_t n_chunks, const std::function<int(hipStream_t up)> &before, const ChunkStep &upload, const ChunkStep &launch,
               const ChunkStep &download)
{
    StageStreams pair;                                       // given back drained on every way out
    pair.take();
    AFG_HIP_CHECK(pair.e);
    const hipStream_t up = pair.up, down = pair.down;
    // Rings of two events, one per slot.  A wait takes the event's state when it is queued, so at chunk c `uploaded[slot]`
    // and `fetched[slot]` still stand for chunk c - 2: the last chunk that used the slot.
    Events ev;
    for (hipEvent_t &e : ev.e) AFG_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipEvent_t *uploaded = ev.e, *done = ev.e + 2, *fetched = ev.e + 4;
    if (before) if (int rc = before(up)) return rc;
    for (size_t c = 0; c < n_chunks; c++) {
        const int slot = (int)(c & 1);
        if (upload) {
            if (c >= 2) AFG_HIP_CHECK(hipEventSynchronize(uploaded[slot]));    // the staging is free: chunk c - 2 has gone up
            if (int rc = upload(c, slot, up)) return rc;
            AFG_HIP_CHECK(hipEventRecord(uploaded[slot], up));
        }
        if (c >= 2) AFG_HIP_CHECK(hipStreamWaitEvent(up, fetched[slot], 0));  // the output buffer is free: chunk c - 2 has come back
        if (int rc = launch(c, slot, up)) return rc;
        AFG_HIP_CHECK(hipEventRecord(done[slot], up));
        AFG_HIP_CHECK(hipStreamWaitEvent(down, done[slot], 0));
        if (int rc = download(c, slot, down)) return rc;
        AFG_HIP_CHECK(hipEventRecord(fetched[slot], down));
    }
    AFG_HIP_CHECK(hipStreamSynchronize(down));
    AFG_HIP_CHECK(hipStreamSynchronize(up));
    return AFG_OK;
}

SongChunks::SongChunks(const std::vector<uint64_t> &start, const std::vector<uint64_t> &end) : first{ 0 }
{
    const size_t M = start.size();
    for (size_t j = 0; j + 1 < M; j++)
        if (end[j] - start[first.back()] >= (stage_chunk_samples(2 * kSongChunkFrames) + 1) / 2) first.push_back(j + 1);
    first.push_back(M);
    for (size_t c = 0; c < count(); c++) {
        frames.push_back(end[first[c + 1] - 1] - start[first[c]]);
        max_frames = std::max(max_frames, frames.back());
    }
}

}  // namespace afg_front
