// afg_flac_stage.cpp -- the batch path's FLAC staging pass, and the FLAC and QOA device stages of decode_parsed
// (afg_batch.h): every FLAC record of the batch restored chunk by chunk on three streams, every QOA frame in one launch;
// both write their range of the shared device plane, in the result plane's layout.
#include "afg_batch.h"

namespace afg_front {

bool flac_rows_int16() { return afg::dev_option(afg::kDevFlacHostRes32) <= 0; }

// pass 1b: FLAC files of known length straight into one page-locked residual buffer
int FlacStaging::parse(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, unsigned nt, StageTimer &tm)
{
    if (!total) return AFG_OK;
    if (int rc = staging_take(total * sizeof(int32_t), lease)) return rc;
    int32_t *res0 = (int32_t *)lease.p;
    std::atomic<bool> lost{ false };
    parallel_for(parsed.size(), nt, [&](size_t i) {
        if (!bounds[i]) return;
        Parsed &p = parsed[i];
        bool ok = false;
        try {
            p.flac.pack16 = flac_rows_int16();
            ok = flac_parse_into(data[i], len[i], p.fi, p.flac, res0 + base[i], bounds[i]);
            if (ok && p.flac.overflow) {                 // more audio than STREAMINFO declares: the file's own buffer
                p.flac = FlacRecords();
                p.flac.pack16 = flac_rows_int16();
                ok = flac_parse(data[i], len[i], p.fi, p.flac);
                lost = true;
            }
        } catch (...) { ok = false; }
        if (ok) p.format = AFG_FORMAT_FLAC;
        else p.flac = FlacRecords();
    });
    // the staged layout is used only when every FLAC file of the batch is in it (a file of undeclared length
    // was parsed into its own buffer in pass 1): otherwise everything is gathered, wherever it sits
    bool all_staged = !lost;
    for (size_t i = 0; i < parsed.size() && all_staged; i++)
        if (parsed[i].format == AFG_FORMAT_FLAC && !parsed[i].flac.ext_res && parsed[i].flac.res_size()) all_staged = false;
    if (all_staged) { res = res0; words = total; }
    tm.lap("pass 1b: flac parse into staging");
    return AFG_OK;
}

size_t FlacDecode::layout(StageCtx &ctx, size_t plane_off)
{
    const size_t nf = ctx.nf();
    res_base.assign(nf, 0); fr_base.assign(nf, 0); sf_base.assign(nf, 0);
    for (size_t i = 0; i < nf; i++) {
        Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_FLAC) continue;
        if (!is_staged()) res_total = (res_total + 3) & ~(size_t)3;     // 16-byte aligned planes (int16 rows: afg_flac_frame.res16)
        res_base[i] = is_staged() ? staged->base[i] : res_total; fr_base[i] = fr_total; sf_base[i] = sf_total;
        ctx.out.files[i].pcm_off = plane_off + out_floats;
        if (ctx.so.runs()) runs.push_back(PackRun{ plane_off + out_floats, p.flac.out_samples, 0, (uint32_t)i, (uint32_t)p.fi.channels });
        res_total += p.flac.res_size(); fr_total += p.flac.frames.size(); sf_total += p.flac.subframes.size();
        out_floats += p.flac.out_samples;
    }
    if (is_staged()) res_total = staged->words;              // the device plane mirrors the staging layout (gaps and all)
    sort_runs(runs);
    return out_floats;
}

// Chunks of files: gather (host threads) -> upload on `up` -> kernel on `mid` behind the upload's event -> download on
// `down` behind the kernel's, so the gather of chunk k+1, the upload of chunk k and the download of chunk k-1 overlap and
// the next chunk's upload never waits behind this chunk's kernel.
int FlacDecode::run(StageCtx &ctx, StageDev &dev)
{
    if (!out_floats) return AFG_OK;
    std::vector<Parsed> &parsed = ctx.parsed;
    const SampleOut &so = ctx.so;
    const bool f64 = so.f64(), wide = so.wide(), fetch = so.fetch(), flac_staged = is_staged();
    const size_t nf = ctx.nf(), es = so.es();
    const size_t rec_bytes = fr_total * sizeof(afg_flac_frame) + sf_total * sizeof(afg_flac_subframe);
    const size_t rec_pad = (rec_bytes + 15) & ~(size_t)15;
    StagingLease h_in;
    DevBuf d_in;
    if (int rc = staging_take(rec_pad + (flac_staged ? 0 : res_total * 4), h_in)) return rc;
    if (int rc = d_in.alloc(rec_pad + res_total * 4)) return rc;
    afg_flac_frame *hf = (afg_flac_frame *)h_in.p;
    afg_flac_subframe *hs = (afg_flac_subframe *)(hf + fr_total);
    int32_t *hr = (int32_t *)((uint8_t *)h_in.p + rec_pad);           // (not staged: the residuals are gathered here)
    const int32_t *hres = flac_staged ? staged->res : hr;
    const afg_flac_frame *df = (const afg_flac_frame *)d_in.p;
    const afg_flac_subframe *ds = (const afg_flac_subframe *)(df + fr_total);
    const int32_t *dr = (const int32_t *)((const uint8_t *)d_in.p + rec_pad);
    StageStreams s;
    hipError_t &e = s.e;
    s.take(true);
    const hipStream_t up = s.up, down = s.down, mid = s.mid;
    int rc = AFG_OK;
    const size_t target = std::max<size_t>((res_total + ctx.chunks - 1) / ctx.chunks, (size_t)stage_chunk_samples((size_t)4 << 20));
    // AFG_TRACE: host wall-clock of every chunk's gather and submission, device time of its upload, kernel and download
    struct ChunkTrace { double t_begin, t_gathered, t_queued; hipEvent_t e_up0, e_up1, e_k1, e_d0, e_d1; };
    std::vector<ChunkTrace> ctrace;
    const auto t_stage = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_stage).count(); };
    hipEvent_t e_stage = nullptr;
    if (g_trace && e == hipSuccess) { (void)hipEventCreate(&e_stage); (void)hipEventRecord(e_stage, up); }
    auto mark = [&](hipStream_t st) { hipEvent_t ev = nullptr; (void)hipEventCreate(&ev); (void)hipEventRecord(ev, st); return ev; };
    for (size_t f0 = 0; f0 < nf && !rc && e == hipSuccess;) {
        const FileChunk ch = cut_chunk(f0, nf, target, [&](size_t i, size_t &w) { return ctx.fmt_of(i) == AFG_FORMAT_FLAC && ((w = parsed[i].flac.res_size()), true); });
        const size_t f1 = ch.f1, first = ch.first, last = ch.last;
        if (first == nf) { f0 = f1; continue; }
        ChunkTrace ct{};
        ct.t_begin = since();
        parallel_for(f1 - f0, ctx.threads, [&](size_t k) {
            const size_t i = f0 + k;
            Parsed &p = parsed[i];
            if (ctx.fmt_of(i) != AFG_FORMAT_FLAC) return;
            for (size_t q = 0; q < p.flac.frames.size(); q++) {
                afg_flac_frame f = p.flac.frames[q];
                f.in_off += (f.res16 ? 2 : 1) * (uint64_t)res_base[i]; f.out_off += ctx.out.files[i].pcm_off; f.sf_index += (uint32_t)sf_base[i];
                hf[fr_base[i] + q] = f;
            }
            std::memcpy(hs + sf_base[i], p.flac.subframes.data(), p.flac.subframes.size() * sizeof(afg_flac_subframe));
            if (!flac_staged) {
                std::memcpy(hr + res_base[i], p.flac.res_data(), p.flac.res_size() * 4);
                std::vector<int32_t>().swap(p.flac.res);       // the residual plane is the big one: drop it early
            }
        });
        const size_t fr0 = fr_base[first], fr1 = fr_base[last] + parsed[last].flac.frames.size();
        const size_t sf0 = sf_base[first], sf1 = sf_base[last] + parsed[last].flac.subframes.size();
        const size_t r0 = res_base[first];
        size_t r1 = r0;
        for (size_t q = fr0; q < fr1; q++)                           // (a packed frame keeps the words it was parsed into)
            r1 = std::max<size_t>(r1, (size_t)(hf[q].res16 ? hf[q].in_off / 2 : hf[q].in_off) + (size_t)hf[q].channels * hf[q].block_size);
        const size_t o0 = ctx.out.files[first].pcm_off, o1 = ctx.out.files[last].pcm_off + parsed[last].flac.out_samples;
        ct.t_gathered = since();
        if (g_trace) ct.e_up0 = mark(up);
        e = hipMemcpyAsync((void *)(df + fr0), hf + fr0, (fr1 - fr0) * sizeof(afg_flac_frame), hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipMemcpyAsync((void *)(ds + sf0), hs + sf0, (sf1 - sf0) * sizeof(afg_flac_subframe), hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipMemcpyAsync((void *)(dr + r0), hres + r0, (r1 - r0) * 4, hipMemcpyHostToDevice, up);
        if (e != hipSuccess) break;
        if (g_trace) ct.e_up1 = mark(up);
        s.chain(up, mid);
        if (e != hipSuccess) break;
        // (the records are still here in host memory: only the populated instantiations are launched)
        rc = afg_flac_transform_variants_hip(fr1 - fr0, df + fr0, ds, dr, f64 ? (int32_t *)dev.d_out.p : nullptr, f64 ? nullptr : (float *)dev.d_out.p,
                                             afg_flac_variants(fr1 - fr0, hf + fr0, hs), mid);
        if (rc) break;
        // (f64: the restored int32 samples are widened; the other types convert the floats)
        if (wide && (rc = dev.conv.launch(so, f64 ? AFG_F64_KIND_FLAC_S32 : AFG_WAV_KIND_F32, dev.d_out.p, 0, o0, o1 - o0, dev.d_out64.p, runs, mid)) != AFG_OK) break;
        if (g_trace) ct.e_k1 = mark(mid);
        s.chain(mid, down);
        if (g_trace) ct.e_d0 = mark(down);
        if (e == hipSuccess && fetch)
            e = hipMemcpyAsync(ctx.plane_at(o0), (const uint8_t *)(wide ? dev.d_out64.p : dev.d_out.p) + o0 * es, (o1 - o0) * es, hipMemcpyDeviceToHost, down);
        if (g_trace) { ct.e_d1 = mark(down); ct.t_queued = since(); ctrace.push_back(ct); }
        f0 = f1;
    }
    const double t_loop = since();
    double t_up = 0;
    s.drain([&] { t_up = since(); });
    if (g_trace) {
        std::fprintf(stderr, "[afg] flac stage: loop done %.2f ms, up drained %.2f, down drained %.2f\n", t_loop, t_up, since());
        for (size_t k = 0; k < ctrace.size(); k++) {
            const ChunkTrace &c = ctrace[k];
            float u0 = 0, u1 = 0, k1 = 0, d0 = 0, d1 = 0;
            (void)hipEventElapsedTime(&u0, e_stage, c.e_up0); (void)hipEventElapsedTime(&u1, e_stage, c.e_up1);
            (void)hipEventElapsedTime(&k1, e_stage, c.e_k1); (void)hipEventElapsedTime(&d0, e_stage, c.e_d0);
            (void)hipEventElapsedTime(&d1, e_stage, c.e_d1);
            std::fprintf(stderr, "[afg]   chunk %zu: host begin %.2f gathered %.2f queued %.2f | device up %.2f-%.2f kernel -%.2f down %.2f-%.2f\n",
                         k, c.t_begin, c.t_gathered, c.t_queued, u0, u1, k1, d0, d1);
            for (hipEvent_t ev : { c.e_up0, c.e_up1, c.e_k1, c.e_d0, c.e_d1 }) (void)hipEventDestroy(ev);
        }
        if (e_stage) (void)hipEventDestroy(e_stage);
    }
    s.release();
    if (rc) return rc;
    if (e != hipSuccess) { afg::set_error("FLAC stage failed: %s", hipGetErrorString(e)); return AFG_ERR_HIP; }
    ctx.tm.lap("flac gather | h2d | kernel | d2h (chunks overlapped)");
    return AFG_OK;
}

size_t QoaDecode::layout(StageCtx &ctx, size_t off)
{
    const size_t nf = ctx.nf();
    plane_off = off;
    byte_base.assign(nf, 0); fr_base.assign(nf, 0);
    for (size_t i = 0; i < nf; i++) {
        Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_QOA) continue;
        byte_base[i] = bytes; fr_base[i] = frames;
        ctx.out.files[i].pcm_off = plane_off + out_floats;
        bytes += (ctx.len[i] + 15) & ~(size_t)15;
        frames += p.qoa.size();
        const size_t q_samples = p.qoa.back().out_off + (size_t)p.qoa.back().samples * p.qoa.back().channels;
        if (ctx.so.runs()) runs.push_back(PackRun{ plane_off + out_floats, q_samples, 0, (uint32_t)i, (uint32_t)p.qi.channels });
        out_floats += q_samples;
    }
    sort_runs(runs);
    return out_floats;
}

// one gather, one upload, one launch, one download, on the null stream
int QoaDecode::run(StageCtx &ctx, StageDev &dev)
{
    const SampleOut &so = ctx.so;
    const bool wide = so.wide();
    const hipStream_t stream = nullptr;
    if (out_floats) {
        const size_t rec_pad = (frames * sizeof(afg_qoa_frame) + 15) & ~(size_t)15;
        StagingLease h_in;
        DevBuf d_in;
        if (int rc = staging_take(rec_pad + bytes, h_in)) return rc;
        if (int rc = d_in.alloc(rec_pad + bytes)) return rc;
        afg_qoa_frame *hq = (afg_qoa_frame *)h_in.p;
        uint8_t *hb = (uint8_t *)h_in.p + rec_pad;
        parallel_for(ctx.nf(), ctx.threads, [&](size_t i) {
            Parsed &p = ctx.parsed[i];
            if (ctx.fmt_of(i) != AFG_FORMAT_QOA) return;
            for (size_t k = 0; k < p.qoa.size(); k++) {
                afg_qoa_frame f = p.qoa[k];
                f.byte_off += byte_base[i]; f.out_off += ctx.out.files[i].pcm_off;
                hq[fr_base[i] + k] = f;
            }
            std::memcpy(hb + byte_base[i], ctx.data[i], ctx.len[i]);
        });
        AFG_HIP_CHECK(hipMemcpyAsync(d_in.p, h_in.p, rec_pad + bytes, hipMemcpyHostToDevice, stream));
        if (int rc = afg_qoa_transform_hip(frames, (const afg_qoa_frame *)d_in.p, (const uint8_t *)d_in.p + rec_pad, nullptr,
                                           (float *)dev.d_out.p, stream))
            return rc;
        if (wide) if (int rc = dev.conv.launch(so, AFG_WAV_KIND_F32, dev.d_out.p, 0, plane_off, out_floats, dev.d_out64.p, runs, stream)) return rc;
        AFG_HIP_CHECK(hipStreamSynchronize(stream));         // (d_in is let go here)
    }
    if (out_floats && so.fetch()) {                          // (the FLAC part came back chunk by chunk)
        AFG_HIP_CHECK(hipMemcpyAsync(ctx.plane_at(plane_off), (const uint8_t *)(wide ? dev.d_out64.p : dev.d_out.p) + plane_off * so.es(), out_floats * so.es(),
                                     hipMemcpyDeviceToHost, stream));
        AFG_HIP_CHECK(hipStreamSynchronize(stream));
    }
    ctx.tm.lap("qoa stage");
    return AFG_OK;
}

}  // namespace afg_front
