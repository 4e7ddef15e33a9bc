// afg_opus_stage.cpp -- the Opus (CELT) device stages (afg_batch.h): the gathered stage of decode_parsed (a stream's chunk
// with its carry, files parsed into their own buffers) and the pipelined stage of the batch path's pass 1c.  Both: records +
// coefficients -> transform -> gain / int16 round trip -> conversion -> host plane.
#include "afg_batch.h"

namespace afg_front {

namespace {

// The channel sequences of a launch: one per output channel of every file, each the index of its first record; the table
// ends with the record count.  The transform stage walks sequences 2p and 2p + 1 of a launch together when they are the
// two channels of a stream (one wavefront, half each: afg.h), so a stereo file starts on an even index of its launch: an
// empty sequence goes in front of it after an odd number of mono files, and in front of a chunk (a launch of its own)
// that would start on an odd one.  Without it such a file is walked one channel at a time -- slower, and in
// AFG_NUMERIC_TOLERANCE to samples that depend on what else is in the batch (tools/soak_damaged.py found one).
struct OpusSeqs {
    std::vector<uint64_t> table;
    // a file of `channels` sequences of `frames` records from rec0 on; returns the index of its first sequence
    size_t add(uint64_t rec0, size_t frames, int channels, bool starts_launch = false)
    {
        if ((table.size() & 1) && (channels == 2 || starts_launch)) table.push_back(rec0);   // the empty sequence
        const size_t at = table.size();
        for (int c = 0; c < channels; c++) table.push_back(rec0 + (uint64_t)c * frames);
        return at;
    }
    size_t count() const { return table.size(); }
    size_t bytes() const { return ((count() + 1) * sizeof(uint64_t) + 15) & ~(size_t)15; }
    void write(uint64_t *to, uint64_t recs) const
    {
        std::copy(table.begin(), table.end(), to);
        to[count()] = recs;
    }
};

// A file's records, one set per channel, from those of channel 0 with file-relative offsets (src; it may be dst itself:
// the channels are written last to first): channel c reads its coefficients behind channel c - 1's within every frame and
// writes every C-th sample of the file's interleaved PCM.
void derive_records(const afg_celt_frame *src, afg_celt_frame *dst, size_t n, int channels, uint64_t coef_base, uint64_t pcm_base)
{
    for (int c = channels - 1; c >= 0; c--)
        for (size_t q = 0; q < n; q++) {
            afg_celt_frame r = src[q];
            r.coef_off += coef_base + (uint64_t)c * r.frame_size;
            r.out_off += pcm_base + (uint64_t)c;
            dst[(size_t)c * n + q] = r;
        }
}

// output gain (when a file asks for one) and the reference's int16 round trip, in place: floats [c0, c0 + n) of the plane
// in one launch, or -- a file has a gain -- file by file
struct OpusFileOut { uint64_t at, n; int gain_i; float gain; };
int opus_output(float *d_pcm, uint64_t c0, uint64_t n, const std::vector<OpusFileOut> &files, hipStream_t st)
{
    bool any_gain = false;
    for (const OpusFileOut &f : files) any_gain = any_gain || f.gain_i != 0;
    if (!any_gain) return afg_opus_output_hip(n, d_pcm + c0, nullptr, d_pcm + c0, st);
    for (const OpusFileOut &f : files) {
        float *at = d_pcm + f.at;
        const int rc = f.gain_i ? afg_opus_output_gain_hip(f.n, at, f.gain, nullptr, at, st) : afg_opus_output_hip(f.n, at, nullptr, at, st);
        if (rc) return rc;
    }
    return AFG_OK;
}

// what a file delivers: the reference never reads past the declared length (stream.d:439-442)
uint64_t delivered_frames(const afg_opus::File &f) { return (uint64_t)std::min<int64_t>((int64_t)f.pcm_frames, std::max<int64_t>(f.declared_frames, 0)); }

}  // namespace

// the PCM plane holds the files back to back, interleaved
size_t OpusDecode::layout(StageCtx &ctx, size_t off)
{
    const size_t nf = ctx.nf();
    const SampleOut &so = ctx.so;
    plane_off = off;
    rec_base.assign(nf, 0); coef_base.assign(nf, 0); pcm_base.assign(nf, 0);
    OpusSeqs sq;
    for (size_t i = 0; i < nf; i++) {
        const Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_OPUS) continue;
        if (done_at) {
            ctx.out.files[i].pcm_off = done_at[i];
            ctx.out.files[i].in_opus_plane = true;
            continue;
        }
        rec_base[i] = recs; coef_base[i] = coefs; pcm_base[i] = out_floats;
        if (so.dither) runs.push_back(PackRun{ out_floats, (uint64_t)p.opus.pcm_frames * (uint64_t)p.opus.channels, 0 });
        else if (so.collate())                                   // (what is delivered: the declared length cuts it)
            runs.push_back(PackRun{ out_floats, delivered_frames(p.opus) * (uint64_t)p.opus.channels, 0, (uint32_t)i, (uint32_t)p.opus.channels });
        ctx.out.files[i].pcm_off = plane_off + out_floats;
        sq.add(recs, p.opus.frames.size(), p.opus.channels);
        recs += p.opus.frames.size() * (size_t)p.opus.channels;
        coefs += p.opus.coeffs.size();
        out_floats += (size_t)p.opus.pcm_frames * (size_t)p.opus.channels;
    }
    seqs = sq.count();
    seq_table.swap(sq.table);
    sort_runs(runs);
    return out_floats;
}

int OpusDecode::run(StageCtx &ctx, StageDev &dev)
{
    if (!out_floats) return AFG_OK;
    std::vector<Parsed> &parsed = ctx.parsed;
    const SampleOut &so = ctx.so;
    const bool wide = so.wide(), fetch = so.fetch();
    const size_t nf = ctx.nf(), es = so.es();
    const hipStream_t stream = nullptr;
    if (seqs > 0xffffffffull) { afg::set_error("Opus stage: too many channel sequences"); return AFG_ERR_INVALID; }
    OpusSeqs sq;
    sq.table.swap(seq_table);
    const size_t base_bytes = sq.bytes();
    const size_t rec_bytes = (recs * sizeof(afg_celt_frame) + 15) & ~(size_t)15;
    StagingLease h_in;
    DevBuf d_in, d_pcm;
    if (wide && fetch) if (int rc = d_pcm64.alloc(std::max<size_t>(out_floats * es, 16))) return rc;
    if (int rc = staging_take(base_bytes + rec_bytes + coefs * sizeof(float), h_in)) return rc;
    if (int rc = d_in.alloc(base_bytes + rec_bytes + coefs * sizeof(float))) return rc;
    if (int rc = d_pcm.alloc(out_floats * sizeof(float))) return rc;
    afg_celt_frame *hr = (afg_celt_frame *)((uint8_t *)h_in.p + base_bytes);
    float *hc = (float *)((uint8_t *)h_in.p + base_bytes + rec_bytes);
    sq.write((uint64_t *)h_in.p, recs);
    std::vector<OpusFileOut> files;
    for (size_t i = 0; i < nf; i++)
        if (ctx.fmt_of(i) == AFG_FORMAT_OPUS)
            files.push_back(OpusFileOut{ pcm_base[i], parsed[i].opus.pcm_frames * (uint64_t)parsed[i].opus.channels, parsed[i].opus.gain_i, parsed[i].opus.gain });
    parallel_for(nf, ctx.threads, [&](size_t i) {
        Parsed &p = parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_OPUS) return;
        derive_records(p.opus.frames.data(), hr + rec_base[i], p.opus.frames.size(), p.opus.channels, coef_base[i], pcm_base[i]);
        if (!p.opus.coeffs.empty()) std::memcpy(hc + coef_base[i], p.opus.coeffs.data(), p.opus.coeffs.size() * sizeof(float));
        std::vector<float>().swap(p.opus.coeffs);
    });
    AFG_HIP_CHECK(hipMemcpyAsync(d_in.p, h_in.p, base_bytes + rec_bytes + coefs * sizeof(float), hipMemcpyHostToDevice, stream));
    // chunked stream (one file): the channel states live on the device between chunks, zero for a fresh decoder -- and
    // for one whose states were left on another device (the stream has moved: they are stale)
    float *states = nullptr;
    if (carry) {
        const size_t sb = seqs * AFG_CELT_STATE_FLOATS * sizeof(float);
        if (!carry->states.here()) {
            carry->valid = false;
            if (int rc = carry->states.alloc(sb)) return rc;
        }
        if (!carry->valid) AFG_HIP_CHECK(hipMemsetAsync(carry->states.p, 0, sb, stream));
        carry->valid = true;
        states = (float *)carry->states.p;
    }
    if (int rc = afg_celt_transform_hip((uint32_t)seqs, (const uint64_t *)d_in.p, (const afg_celt_frame *)((const uint8_t *)d_in.p + base_bytes),
                                        (const float *)((const uint8_t *)d_in.p + base_bytes + rec_bytes), (float *)d_pcm.p, states, stream))
        return rc;
    if (int rc = opus_output((float *)d_pcm.p, 0, out_floats, files, stream)) return rc;
    if (wide) if (int rc = dev.conv.launch(so, AFG_WAV_KIND_F32, d_pcm.p, 0, 0, out_floats, d_pcm64.p, runs, stream)) return rc;
    if (fetch)
        AFG_HIP_CHECK(hipMemcpyAsync(ctx.plane_at(plane_off), wide ? d_pcm64.p : d_pcm.p, out_floats * es, hipMemcpyDeviceToHost, stream));
    AFG_HIP_CHECK(hipStreamSynchronize(stream));
    ctx.tm.lap("opus gather | h2d | kernel | d2h");
    return AFG_OK;
}

int opus_pipeline(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *length, const std::vector<uint8_t> &opened,
                  unsigned threads, const SampleOut &so, StagingLease &plane, std::vector<size_t> &pcm_at, bool *staged, StageTimer &tm)
{
    const bool wide = so.wide(), fetch = so.fetch();
    const size_t nf = parsed.size(), es = so.es();
    *staged = false;
    pcm_at.assign(nf, 0);
    size_t n_opus = 0, recs_total = 0, coefs_total = 0;
    std::vector<size_t> rec_at(nf, 0), coef_at(nf, 0), seq_at(nf, 0);
    for (size_t i = 0; i < nf; i++) {
        if (!opened[i]) continue;
        const afg_opus::File &m = parsed[i].opus;
        rec_at[i] = recs_total; coef_at[i] = coefs_total;
        pcm_at[i] = coefs_total;                          // one PCM float per coefficient
        recs_total += m.bound_frames * (size_t)m.channels;
        coefs_total += m.bound_coeffs;
        n_opus++;
    }
    if (!n_opus) return AFG_OK;
    const size_t target = std::max<size_t>((coefs_total + 7) / 8, (size_t)stage_chunk_samples((size_t)4 << 20));      // coefficients per chunk
    auto cut = [&](size_t f0) { return cut_chunk(f0, nf, target, [&](size_t i, size_t &w) { w = parsed[i].opus.bound_coeffs; return opened[i] != 0; }); };
    OpusSeqs sq;
    for (size_t f0 = 0; f0 < nf;) {
        const FileChunk ch = cut(f0);
        for (size_t i = f0; i < ch.f1; i++)
            if (opened[i]) seq_at[i] = sq.add(rec_at[i], parsed[i].opus.bound_frames, parsed[i].opus.channels, i == ch.first);
        f0 = ch.f1;
    }
    if (sq.count() > 0xffffffffull) { afg::set_error("Opus stage: too many channel sequences"); return AFG_ERR_INVALID; }
    const size_t base_bytes = sq.bytes();
    const size_t rec_bytes = (recs_total * sizeof(afg_celt_frame) + 15) & ~(size_t)15;
    StagingLease h_in;
    DevBuf d_in, d_pcm, d_pcm64;
    SampleConv conv;
    std::vector<PackRun> runs;                        // (ascending: the files lie in the plane in order)
    for (size_t i = 0; i < nf && so.dither; i++)
        if (opened[i]) runs.push_back(PackRun{ pcm_at[i], parsed[i].opus.bound_coeffs, 0 });
    if (int rc = staging_take(base_bytes + rec_bytes + coefs_total * sizeof(float), h_in)) return rc;
    if (fetch) if (int rc = staging_take(std::max<size_t>(coefs_total, 1) * es, plane)) return rc;
    if (wide && fetch) if (int rc = d_pcm64.alloc(std::max<size_t>(coefs_total * es, 16))) return rc;
    if (int rc = d_in.alloc(base_bytes + rec_bytes + coefs_total * sizeof(float))) return rc;
    if (int rc = d_pcm.alloc(std::max<size_t>(coefs_total, 1) * sizeof(float))) return rc;
    uint64_t *hb = (uint64_t *)h_in.p;
    afg_celt_frame *hr = (afg_celt_frame *)((uint8_t *)h_in.p + base_bytes);
    float *hc = (float *)((uint8_t *)h_in.p + base_bytes + rec_bytes);
    const uint64_t *db = (const uint64_t *)d_in.p;
    const afg_celt_frame *dr = (const afg_celt_frame *)((const uint8_t *)d_in.p + base_bytes);
    const float *dc = (const float *)((const uint8_t *)d_in.p + base_bytes + rec_bytes);
    sq.write(hb, recs_total);
    StageStreams s;
    hipError_t &e = s.e;
    s.take();
    const hipStream_t up = s.up, down = s.down;
    if (e == hipSuccess) e = hipMemcpyAsync(d_in.p, hb, base_bytes, hipMemcpyHostToDevice, up);
    int rc = AFG_OK;
    for (size_t f0 = 0; f0 < nf && !rc && e == hipSuccess;) {
        const FileChunk ch = cut(f0);
        const size_t f1 = ch.f1, first = ch.first, last = ch.last;
        if (first == nf) { f0 = f1; continue; }
        parallel_for(f1 - f0, threads, [&](size_t k) {
            const size_t i = f0 + k;
            if (!opened[i]) return;
            Parsed &p = parsed[i];
            const size_t nfr = p.opus.bound_frames, nco = p.opus.bound_coeffs;
            const int C = p.opus.channels;
            afg_celt_frame *recs = hr + rec_at[i];
            bool ok = false;
            try {
                afg_opus::File f;
                ok = afg_opus::parse_file_into(data[i], length[i], f, recs, nfr, hc + coef_at[i], nco) == afg_opus::kOpened &&
                     !f.overflow && f.n_frames == nfr && f.n_coeffs == nco;
                f.ext_frames = nullptr;                // (the staging outlives this record)
                f.ext_coeffs = nullptr;
                if (ok) p.opus = f;
            } catch (...) { ok = false; }
            if (!ok) {                                 // cannot happen (the sizes are exact): an empty, failed file
                p.opus.error = true;
                p.opus.pcm_frames = 0;
                std::memset((void *)recs, 0, nfr * (size_t)C * sizeof(afg_celt_frame));
                std::memset(hc + coef_at[i], 0, nco * sizeof(float));
                for (size_t q = 0; q < nfr * (size_t)C; q++) { recs[q].frame_size = 120; recs[q].blocks = 1; recs[q].out_stride = 1; recs[q].imdct_scale = 1.0f; recs[q].out_off = pcm_at[i]; recs[q].coef_off = coef_at[i]; }
                p.format = AFG_FORMAT_OPUS;
                return;
            }
            derive_records(recs, recs, nfr, C, coef_at[i], pcm_at[i]);     // channel 0's records are in place
            p.format = AFG_FORMAT_OPUS;
        });
        const size_t r0 = rec_at[first], r1 = rec_at[last] + parsed[last].opus.bound_frames * (size_t)parsed[last].opus.channels;
        const size_t c0 = coef_at[first], c1 = coef_at[last] + parsed[last].opus.bound_coeffs;
        const size_t s0 = seq_at[first], s1 = seq_at[last] + (size_t)parsed[last].opus.channels;
        e = hipMemcpyAsync((void *)(dr + r0), hr + r0, (r1 - r0) * sizeof(afg_celt_frame), hipMemcpyHostToDevice, up);
        if (e == hipSuccess && c1 > c0) e = hipMemcpyAsync((void *)(dc + c0), hc + c0, (c1 - c0) * sizeof(float), hipMemcpyHostToDevice, up);
        if (e != hipSuccess) break;
        if (c1 > c0) {
            rc = afg_celt_transform_hip((uint32_t)(s1 - s0), db + s0, dr, dc, (float *)d_pcm.p, nullptr, up);
            if (rc) break;
            std::vector<OpusFileOut> files;
            // collate: the chunk's files have just been decoded: a file's run is what it delivers, not its bound (the
            // declared length cuts the delivery); a failed file has none
            std::vector<PackRun> delivered;
            for (size_t i = first; i <= last; i++) {
                if (!opened[i]) continue;
                const afg_opus::File &m = parsed[i].opus;
                files.push_back(OpusFileOut{ pcm_at[i], m.bound_coeffs, m.gain_i, m.gain });
                if (so.collate() && !m.error)
                    delivered.push_back(PackRun{ pcm_at[i], std::min<uint64_t>(delivered_frames(m) * (uint64_t)m.channels, m.bound_coeffs), 0, (uint32_t)i, (uint32_t)m.channels });
            }
            rc = opus_output((float *)d_pcm.p, c0, c1 - c0, files, up);
            if (rc) break;
            if (wide && (rc = conv.launch(so, AFG_WAV_KIND_F32, d_pcm.p, 0, c0, c1 - c0, d_pcm64.p, so.collate() ? delivered : runs, up)) != AFG_OK) break;
            s.chain(up, down);
            if (e == hipSuccess && fetch)
                e = hipMemcpyAsync((uint8_t *)plane.p + c0 * es, (const uint8_t *)(wide ? d_pcm64.p : d_pcm.p) + c0 * es, (c1 - c0) * es, hipMemcpyDeviceToHost, down);
        }
        f0 = f1;
    }
    s.drain();
    s.release();
    if (rc) return rc;
    if (e != hipSuccess) { afg::set_error("Opus stage failed: %s", hipGetErrorString(e)); return AFG_ERR_HIP; }
    *staged = true;
    tm.lap("pass 1c: opus decode into staging | h2d | kernels | d2h (chunks overlapped)");
    return AFG_OK;
}

}  // namespace afg_front
