/*
 * afg.h -- C ABI of the MI355X-native batched audio-decode transform path.
 *
 * Drop-in boundary for the transform stage of AuburnSounds/audio-formats'
 * decoders (reference paths are relative to /root/reference).  The reference
 * is pure D and has no FFI layer; the seams below are the D function calls a
 * maintainer would redirect to this library (binding stub: INTEGRATION.md,
 * bindings/d/afgpu.d).  Bitstream / entropy decoding stays on the host; only
 * the per-frame transform stage runs on the device.
 *
 * Conventions (reference: stream.d:31-33, :105, internals.d:16-23):
 *   - no exceptions, nothing aborts; every entry returns an afg_status (0 = ok)
 *   - a handle is not thread-safe; distinct handles share no mutable state
 *   - d_* pointers are device (HIP) pointers, everything else is host memory
 *   - hip_stream is a hipStream_t passed as void* (NULL = default stream);
 *     *_hip entries only enqueue work, they never synchronise
 *   - the persistent kernels (Vorbis, CELT) draw their work from per-launch counters kept in rings: 32 launches of
 *     one Vorbis plan, 64 CELT launches per device may be in flight at once on different streams (launches on ONE
 *     stream run in order and cannot collide)
 *   - the library fails loudly (AFG_ERR_NO_DEVICE) when no gfx950 device or
 *     no device code is available: there is no CPU fallback in the product.
 */
#ifndef AFG_H
#define AFG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): afg_dev_option replaced the per-call AFG_* environment knobs of version 1 (round 5 added the call without
 * counting); afg_host_pool_trim also releases pooled device planes. */
#define AFG_ABI_VERSION 2

typedef enum afg_status {
    AFG_OK              =  0,
    AFG_ERR_INVALID     = -1,   /* bad argument / inconsistent batch description */
    AFG_ERR_NO_DEVICE   = -2,   /* no HIP device, or device code not loadable    */
    AFG_ERR_HIP         = -3,   /* a HIP runtime call failed (see afg_last_error) */
    AFG_ERR_OOM         = -4,
    AFG_ERR_UNSUPPORTED = -5
} afg_status;

int         afg_abi_version(void);
const char *afg_status_string(int status);
const char *afg_last_error(void);          /* thread-local detail of the last failure, never NULL */
int         afg_device_count(void);        /* number of HIP devices visible, <0 on error */

/* Numeric mode of the float transform stages, process-wide.
 *   AFG_NUMERIC_EXACT      every float32 result is produced by the reference's own expression tree (no fused
 *                          multiply-adds, recurrences in the reference's order): bit-identical to the D decoders' arithmetic.
 *   AFG_NUMERIC_TOLERANCE  (default) results within the 1e-5 RMS of the decoders' float output that drop-in use asks
 *                          for; lets the Opus/CELT stage re-associate the de-emphasis recurrence (dopus.d:3695-3701) into a
 *                          prefix sum inside the frame walk, fuse multiply-adds there, and cut a stream into independently
 *                          walked segments wherever the post-filter is provably idle (dopus.d:3294-3296, :3333); lets the
 *                          Vorbis stage compute inverse_mdct (stb_vorbis2.d:1941-2242) of 1024-, 2048- and 4096-sample long
 *                          blocks as ONE complex FFT of n/4 points with fused multiply-adds instead of scheduling the reference's
 *                          8-step algorithm, and write window + overlap (:2606-2657) on the transform's DCT-IV (csrc/vorbis_walk.hip);
 *                          lets the MP3 stage fuse multiply-adds and sum the polyphase window's sixteen products per output
 *                          (minimp3.d:1371-1405) in one chain (csrc/mp3_tolerance.hip).
 * FLAC and QOA (integer work) compute the same bits in both modes.  The environment variable AFG_NUMERIC=exact|tolerance
 * decides until afg_set_numeric_mode is called, and again after afg_set_numeric_mode(AFG_NUMERIC_FROM_ENV).  Returns the
 * mode that was in effect before, AFG_ERR_INVALID for an unknown one. */
#define AFG_NUMERIC_FROM_ENV  (-1)
#define AFG_NUMERIC_EXACT     0
#define AFG_NUMERIC_TOLERANCE 1
int         afg_set_numeric_mode(int mode);

/* Test hooks, not part of the reference's surface: alternative code paths that deliver the same samples as the default
 * ones, which the test-suite runs against each other.  The library reads no environment variable for them (rounds 1-4
 * did, on every call); value < 0 returns an option to "not set".  Names: "celt_path" (1 stream walk, 2 split kernels --
 * the two bit-exact paths --, 3 the tolerance-mode walk), "celt_de_seq" (2 .. 32 sequences per de-emphasis wavefront),
 * "celt_de_duo" (0 / 1), "celt_seg_recs", "celt_whole_frames", "vorbis_single" (1: one channel per wavefront),
 * "mp3_chunks", "mp3_float_upload" (1: float spectra instead of quantised values cross the bus), "vorbis_host_floor"
 * (1: floor curves on the host), "flac_host_res32" (1: int32 residual rows only), "vorbis_seg_packets" (packets per walk
 * item of plans created with seg_packets = 0, instead of the library's choice), "batch_groups" (groups of files a batch call
 * pipelines: 1 = none; default 4 for batches of FLAC / Ogg Vorbis files from 512 files up, else 1), "stage_chunk_samples" (samples per chunk of
 * the FLAC, Vorbis, Opus, WAV, MOD and XM batch stages in place of their own millions, so that small files span several
 * chunks).  AFG_ERR_INVALID: no such name. */
int         afg_dev_option(const char *name, int value);
int         afg_get_numeric_mode(void);
int         afg_device_name(int device, char *buf, size_t buflen);

/* ========================================================================== *
 *  MP3 Layer III transform stage
 *  replaces, for every granule of every stream of a batch:
 *    minimp3.d:1226-1228  L3_antialias -> L3_imdct_gr -> L3_change_sign
 *    minimp3.d:1553       mp3d_synth_granule (mp3d_DCT_II + 9 x mp3d_synth)
 *  Input is the dequantised, stereo-processed, reordered spectrum that
 *  L3_decode holds in scratch.grbuf right before minimp3.d:1226.
 * ========================================================================== */

/* per gr-ch flag word */
#define AFG_MP3_FLAGS(block_type, n_long_bands, aa_bands) \
    ((uint32_t)(block_type) | ((uint32_t)(n_long_bands) << 8) | ((uint32_t)((aa_bands) + 1) << 16))
/*   block_type    gr_info.block_type (0 normal, 1 start, 2 short, 3 stop)
 *   n_long_bands  minimp3.d:1218 (0, 2 or 4)
 *   aa_bands      minimp3.d:1217/1222 (31, or n_long_bands-1 for short blocks; -1 = none) */

/* Optional, OR-ed into the flag word: the first `bands` subbands (0..32) are the only ones that may hold nonzero
 * lines; the lines of the others must be +0.0 (what L3_huffman's zero fill leaves above the last coded line,
 * minimp3.d:868-883) and are not read by the device.  Absent (field 0): all 576 lines are read. */
#define AFG_MP3_NZ_BANDS(bands) ((uint32_t)((bands) + 1) << 24)

/* Optional, OR-ed into the flag word: the block holds subband samples, not a spectrum -- what the Layer I / II decoder
 * hands to mp3d_synth_granule (minimp3.d:1563-1566): index band * 18 + time slot.  Alias reduction, IMDCT and frequency
 * inversion are skipped, the 18 slots go to the synthesis (mp3d_DCT_II + mp3d_synth) as they are.  The reference runs
 * that synthesis 12 slots at a time; it is a filterbank over slot pairs with a 15-slot history and no notion of a
 * granule, so a front-end packs the slots of a run of frames into 18-slot blocks (three 12-slot granules = two blocks). */
#define AFG_MP3_SUBBAND 0x80000000u

#define AFG_MP3_STATE_FLOATS 1536   /* opaque per-stream carry state (same size as mdct_overlap+qmf_state, minimp3.d:40-41) */

typedef struct afg_mp3_plan afg_mp3_plan;

/* Describe a batch: stream s has granules[s] granules of channels[s] (1|2)
 * channels.  Blocks of 576 floats are laid out stream after stream, inside a
 * stream as [granule][channel]; PCM uses the same float offsets, 576*nch
 * interleaved floats per granule (minimp3.d:1549 `pcm += 576*channels`).
 * seg_granules = granules a wavefront walks sequentially (0 = default). */
int      afg_mp3_plan_create(afg_mp3_plan **plan, uint32_t n_streams, const uint32_t *granules,
                             const uint8_t *channels, uint32_t seg_granules);
void     afg_mp3_plan_destroy(afg_mp3_plan *plan);
uint64_t afg_mp3_plan_blocks(const afg_mp3_plan *plan);     /* total gr-ch blocks = floats/576 */
uint32_t afg_mp3_plan_segments(const afg_mp3_plan *plan);   /* workgroups one launch uses */

/* d_coef   : blocks*576 floats      d_flags : blocks words (AFG_MP3_FLAGS)
 * d_pcm    : blocks*576 floats, scaled by 1/32768, not clipped (minimp3.d:1300)
 * d_state  : NULL (every stream starts from zero state, minimp3.d:1509) or
 *            n_streams*AFG_MP3_STATE_FLOATS floats read at the first granule of
 *            each stream and rewritten after its last (chunked decoding). */
int afg_mp3_transform_hip(const afg_mp3_plan *plan, const float *d_coef, const uint32_t *d_flags,
                          float *d_pcm, float *d_state, void *hip_stream);

/* -------------------------------------------------------------------------- *
 *  MP3 requantisation on the device (ship the Huffman values, not floats)
 *  replaces, between the entropy decoder and the transform stage above:
 *    minimp3.d:722-746   L3_pow_43 and the `* sf` of L3_huffman (:835-858, :868-879)
 *    minimp3.d:885-982   L3_midside_stereo / L3_intensity_stereo / L3_stereo_process
 *    minimp3.d:984-1000  L3_reorder
 *  The host keeps Huffman decoding and the scalefactor arithmetic (L3_decode_scalefactors, :616-719: 39 floats per
 *  granule-channel) and decides the stereo plan (which band is mid/side or intensity coded, with which factors); the
 *  device turns int16 values into exactly the floats L3_decode holds in grbuf at :1226 -- 2 bytes per line cross the
 *  bus instead of 4.  Two cases are not covered: MPEG-2.5 8 kHz mixed blocks (their reorder walks outside the channel,
 *  :1218-1223) and a MONO frame whose header carries the intensity-stereo bit (the reference runs L3_intensity_stereo over
 *  the one channel and the scratch row behind it, :100, :1207-1210: damaged files).  afg_mp3_parse_q reports
 *  AFG_ERR_UNSUPPORTED for such a file and the float path takes it.
 * -------------------------------------------------------------------------- */
#define AFG_MP3_NO_SDESC 0xffffffffu

typedef struct afg_mp3_qgranule {
    uint64_t q_off;          /* int16 index of channel 0's 576 values; channel c at q_off + 576*c */
    uint64_t coef_off;       /* float index of channel 0's block in the coefficient plane; channel c at + 576*c */
    uint32_t sdesc;          /* stereo == 2: index of the granule's afg_mp3_sdesc, else AFG_MP3_NO_SDESC */
    uint8_t  nch;            /* 1 | 2; 0: unused record slot, skipped */
    uint8_t  stereo;         /* 0 none, 1 mid/side on every line (:1203), 2 per band (intensity frames, :1201) */
    uint8_t  table[2];       /* per channel: scalefactor-band table (kind*8 + rate row; kind 0 long, 1 short, 2 mixed),
                                bit 7: the short part is reordered (block_type 2) */
    float    scale[2][40];   /* band scales of each channel (scf[] of L3_decode_scalefactors) */
} afg_mp3_qgranule;          /* 344 bytes */

typedef struct afg_mp3_sdesc {
    uint8_t type[40];        /* per band of channel 0's table: 0 leave, 1 mid/side, 2 intensity */
    float   fl[40], fr[40];  /* intensity: right = left * fr, then left = left * fl (:929-936) */
} afg_mp3_sdesc;             /* 360 bytes */

/* d_q: quantised lines (sign included, |v| <= 8206); d_coef receives 576 floats per granule-channel. */
int afg_mp3_requant_hip(uint64_t n_granules, const afg_mp3_qgranule *d_granules, const int16_t *d_q,
                        const afg_mp3_sdesc *d_sdesc, float *d_coef, void *hip_stream);

/* ========================================================================== *
 *  Vorbis transform stage
 *  replaces stb_vorbis2.d:2526-2527 (inverse_mdct per channel) and
 *  stb_vorbis2.d:2606-2657 (vorbis_finish_frame: window + overlap-add),
 *  plus the interleave of stb_vorbis2.d:3927-3952.  Tables are those of
 *  stb_vorbis2.d:851-898, built on the host at plan creation.
 * ========================================================================== */

#define AFG_VORBIS_LONG 1u   /* mode blockflag          (stb_vorbis2.d:2324) */
#define AFG_VORBIS_PREV 2u   /* previous-window flag    (stb_vorbis2.d:2326) */
#define AFG_VORBIS_NEXT 4u   /* next-window flag        (stb_vorbis2.d:2327) */
/* Optional, bits 4..7 of a LONG packet's flag byte: only the first e eighths of every channel's n/2 spectral values may be
 * different from +0.0 (e = 0 .. 8) -- what the host decoder knows from the residue's `end` (stb_vorbis2.d:1586-1600: bins past
 * it are never written, inverse coupling and the floor multiply keep +0.0).  The device then need not fetch the rest (the
 * tolerance-mode walk does not; the bit-exact kernels ignore the declaration).  0 in these bits: nothing declared. */
#define AFG_VORBIS_NZ_EIGHTHS(e) ((((unsigned)(e)) + 1u) << 4)

typedef struct afg_vorbis_plan afg_vorbis_plan;

/* Stream s: packets[s] audio packets, channels[s] channels, block sizes
 * blocksize0/1[s] (powers of two, 256..8192; 64/128 are rejected).
 * pflags: one byte per packet, streams concatenated.
 * Packet p reads channels*(n/2) floats ([ch][n/2]) at spec offset p and writes
 * (right_start-left_start)*channels interleaved floats at out offset p; the
 * first packet of a stream produces no output (stb_vorbis2.d:2645-2649). */
int      afg_vorbis_plan_create(afg_vorbis_plan **plan, uint32_t n_streams, const uint32_t *packets,
                                const uint8_t *channels, const uint16_t *blocksize0,
                                const uint16_t *blocksize1, const uint8_t *pflags, uint32_t seg_packets);
void     afg_vorbis_plan_destroy(afg_vorbis_plan *plan);
uint64_t afg_vorbis_plan_packets(const afg_vorbis_plan *plan);
uint64_t afg_vorbis_plan_spec_floats(const afg_vorbis_plan *plan);
uint64_t afg_vorbis_plan_out_floats(const afg_vorbis_plan *plan);
/* copies the per-packet float offsets (total packets entries each; either may be NULL) */
int      afg_vorbis_plan_offsets(const afg_vorbis_plan *plan, uint64_t *spec_off, uint64_t *out_off);

int afg_vorbis_transform_hip(const afg_vorbis_plan *plan, const float *d_spec, float *d_out, void *hip_stream);

/* Vorbis inverse coupling and floor curve on the device: replaces stb_vorbis2.d:2493-2514 (inverse coupling),
 * :2516-2523 / :2255-2284 (do_floor, silent channels) and :1534-1563 (draw_line) between the host's residue decode and the
 * transform above.  d_spec holds the decoded *residue* vectors in the transform's layout ([channel][n2] per packet) and is
 * rewritten in place with the spectra.
 * A curve is the list of floor-1 points that survive step 2 (finalY >= 0), in sorted_order, as int32 pairs
 * (x = Xlist[j], y = finalY[j] * floor1_multiplier), the first one at x = 0.  n_points == 0: really_zero_channel.
 * Coupling steps are byte pairs (magnitude channel, angle channel) in the order they are applied (coupling_steps-1 .. 0). */
typedef struct afg_vorbis_floor_packet {
    uint64_t spec_off;     /* float index of channel 0's n2 values; channel c at spec_off + c*n2 */
    uint32_t n2;           /* blocksize / 2, a multiple of 4 */
    uint32_t channels;
    uint32_t curve_index;  /* channel 0's afg_vorbis_floor_curve; channel c at curve_index + c */
    uint32_t step_off;     /* first coupling step: bytes d_steps[2*step_off], d_steps[2*step_off + 1] */
    uint32_t n_steps;
    uint32_t pad;
} afg_vorbis_floor_packet; /* 32 bytes */

typedef struct afg_vorbis_floor_curve {
    uint32_t point_off;    /* first point: d_points[2*point_off] = x, d_points[2*point_off + 1] = y */
    uint32_t n_points;
} afg_vorbis_floor_curve;  /* 8 bytes */

int afg_vorbis_floor_hip(uint64_t n_packets, const afg_vorbis_floor_packet *d_packets, const afg_vorbis_floor_curve *d_curves,
                         const int32_t *d_points, const uint8_t *d_steps, float *d_spec, void *hip_stream);

/* ========================================================================== *
 *  FLAC sample restore
 *  replaces drflac.d:1235 (residual + drflac__calculate_prediction_32/_64,
 *  drflac.d:1060-1140) for whole subframes, and the decorrelate / shift /
 *  interleave of drflac_read_s32 (drflac.d:2885-2941); optionally also the
 *  int32 -> float conversion of stream.d:505-511.  Bit-exact int32.
 * ========================================================================== */

#define AFG_FLAC_INDEPENDENT 0
#define AFG_FLAC_LEFT_SIDE   8    /* DRFLAC_CHANNEL_ASSIGNMENT_LEFT_SIDE  */
#define AFG_FLAC_RIGHT_SIDE  9    /* DRFLAC_CHANNEL_ASSIGNMENT_RIGHT_SIDE */
#define AFG_FLAC_MID_SIDE   10    /* DRFLAC_CHANNEL_ASSIGNMENT_MID_SIDE   */

typedef struct afg_flac_subframe {
    int16_t coef[32];   /* LPC coefficients (fixed predictors: drflac.d:1397-1403 table, shift 0) */
    uint8_t order;      /* 0..32; warm-up samples occupy res[0..order) (constant/verbatim: order 0) */
    uint8_t shift;      /* lpcShift 0..31 */
    uint8_t wasted;     /* wastedBitsPerSample */
    uint8_t use64;      /* subframe bitsPerSample > 16 -> 64-bit accumulator (drflac.d:1308) */
} afg_flac_subframe;     /* 68 bytes */

/* Residual rows of a frame whose residuals and warm-up samples all fit 16 bits may be stored as int16 (half
 * the bytes on the bus and in HBM): rows padded to 16 bytes. */
#define AFG_FLAC_ROW16(block_size) (((uint64_t)(block_size) + 7u) & ~(uint64_t)7u)

typedef struct afg_flac_frame {
    uint64_t in_off;      /* res16 == 0: int32 index of channel 0's residual row; channel c at in_off + c*block_size.
                             res16 == 1: int16 index (d_res viewed as int16_t), a multiple of 8; channel c at
                             in_off + c*AFG_FLAC_ROW16(block_size); the row padding is read, never used */
    uint64_t out_off;     /* int32 index of the interleaved output (block_size*channels samples) */
    uint32_t block_size;
    uint32_t sf_index;    /* index of channel 0's afg_flac_subframe; channel c at sf_index + c */
    uint8_t  channels;    /* 1..8 */
    uint8_t  assignment;  /* AFG_FLAC_* */
    uint8_t  bps;         /* STREAMINFO bitsPerSample */
    uint8_t  res16;       /* 0: int32 residual rows, 1: int16 rows */
    uint8_t  pad[4];
} afg_flac_frame;         /* 32 bytes */

/* d_out_i32 and/or d_out_f32 may be NULL (at least one must be given). */
int afg_flac_transform_hip(uint64_t n_frames, const afg_flac_frame *d_frames,
                           const afg_flac_subframe *d_subframes, const int32_t *d_res,
                           int32_t *d_out_i32, float *d_out_f32, void *hip_stream);

/* The restore kernel exists in 8 instantiations (LPC-order bucket <= 4 / 8 / 12 / 32 x 64-bit accumulator, so that each gets
 * the registers it needs and no more) plus 4 of a kernel for groups of frames with one channel count above two (round 6:
 * order <= 12 / 32 x accumulator); a wavefront of 32 consecutive frames -- a lane per subframe -- runs in the one its
 * largest order and widest subframe select.  afg_flac_transform_hip is stream-ordered -- the records are read by the
 * device when hip_stream gets there, never by the host at the call -- so it launches all 12; the ones nobody selects exit
 * at once.  A caller that still holds the FINAL records in host memory can say which are populated:
 * afg_flac_variants (host pointers, pure host code) returns the set as a bit mask, and afg_flac_transform_variants_hip
 * launches only those -- two or more of them side by side on the caller's stream and an internal one, joined before
 * the call returns to the stream's order.  Frames of an instantiation missing from `variants` are NOT decoded.  The mask
 * is only meaningful within the process that computed it. */
uint32_t afg_flac_variants(uint64_t n_frames, const afg_flac_frame *frames, const afg_flac_subframe *subframes);
int afg_flac_transform_variants_hip(uint64_t n_frames, const afg_flac_frame *d_frames,
                                    const afg_flac_subframe *d_subframes, const int32_t *d_res,
                                    int32_t *d_out_i32, float *d_out_f32, uint32_t variants, void *hip_stream);

/* ========================================================================== *
 *  QOA frame decode (LMS predict / dequantise / clamp / update)
 *  replaces the slice loop of qoa_decode_frame (qoa.d:489-530, qoa_lms_predict /
 *  qoa_lms_update :231-254) and the float conversion of QOADecoder.readSamples
 *  (qoa.d:831-838).  Input is the raw file bytes: the host only locates frames
 *  (qoa.d:465-486) -- the LMS state and the 64-bit slices are read on the device.
 * ========================================================================== */

typedef struct afg_qoa_frame {
    uint64_t byte_off;    /* offset of the 8-byte frame header in the byte plane (multiple of 8) */
    uint64_t out_off;     /* index of the frame's first output value (interleaved) */
    uint16_t samples;     /* samples per channel in this frame, <= 5120 (header field, qoa.d:476) */
    uint8_t  channels;    /* 1..8 (header field) */
    uint8_t  pad[5];
} afg_qoa_frame;           /* 24 bytes */
/* A record with samples == 0 is skipped -- it writes nothing -- but the kernel still loads through it: its channels
 * must be 1..8 and its byte_off must point at a whole frame header with its LMS state (8 + 16 * channels bytes) inside
 * the byte plane. */

/* d_out_i16 (qoa_decode_frame's sample_data) and/or d_out_f32 (value * (1.0f/32767)) may be NULL. */
int afg_qoa_transform_hip(uint64_t n_frames, const afg_qoa_frame *d_frames, const uint8_t *d_bytes,
                          int16_t *d_out_i16, float *d_out_f32, void *hip_stream);

/* ========================================================================== *
 *  Opus / CELT transform stage
 *  replaces the per-channel tail of ff_celt_decode_frame (dopus.d:3680-3702):
 *  imdct15_half (dopus.d:1611-1637) + vector_fmul_window (dopus.d:230-243) per
 *  block, celt_postfilter (dopus.d:3281-3378) and de-emphasis / output scaling
 *  (dopus.d:3695-3701).  Input is coeffs[ch] after celt_denormalize / downmix
 *  (dopus.d:3653-3668); output is ff_celt_decode_frame's float output[ch][].
 *  The post-filter and de-emphasis are recursive over the whole stream, so the
 *  unit of parallelism is a channel sequence: all frames of one output channel
 *  of one stream, processed in order.
 * ========================================================================== */

typedef struct afg_celt_frame {
    uint64_t coef_off;       /* float index of coeffs[ch][0]: frame_size floats, short blocks interleaved */
    uint64_t out_off;        /* float index of output sample 0 */
    uint32_t out_stride;     /* distance between consecutive output samples (1 = planar) */
    uint16_t frame_size;     /* 120, 240, 480 or 960 */
    uint8_t  blocks;         /* 1, or 1 << duration when transient (dopus.d:3630) */
    uint8_t  pad;
    int32_t  pf_period_new;  /* dopus.d:3407 (>= 15) */
    float    pf_gains_new[3];
    float    imdct_scale;    /* 1.0, or 0.5 for the stereo -> mono downmix (dopus.d:3665) */
    uint32_t pad2;
} afg_celt_frame;            /* 48 bytes */

#define AFG_CELT_STATE_FLOATS 2064   /* afg_celt_state: buf[2048] + post-filter + de-emphasis memory */

/* Channel sequence k owns records [rec_base[k], rec_base[k+1]) (n_chan + 1 entries).
 * d_states: NULL (zero state: a fresh decoder) or n_chan * AFG_CELT_STATE_FLOATS words read
 * before the first and rewritten after the last frame of each sequence (chunked decoding).
 * Sequences 2p and 2p + 1 are walked by one wavefront, half each, when they are the two channels of a stereo stream
 * (equally long, records of equal geometry, out_stride 2, out_off even and out_off + 1): put a stereo stream's channels on
 * an even and the following odd index -- an empty sequence (rec_base[k] == rec_base[k+1]) after an odd number of mono
 * streams does it, as afg_batch_decode does.  Any layout is decoded correctly; in AFG_NUMERIC_TOLERANCE the two forms
 * of the walk round differently (both within the tolerance), in AFG_NUMERIC_EXACT they are the same bits. */
int afg_celt_transform_hip(uint32_t n_chan, const uint64_t *d_rec_base, const afg_celt_frame *d_recs,
                           const float *d_coeffs, float *d_out, float *d_states, void *hip_stream);

/* The same with the sequential part on a second stream.  The post-filter and the de-emphasis are serial chains per
 * channel sequence: with few, long sequences (a file-sharded mixed corpus holds ~1600 of up to 1.4 M samples per wave)
 * they occupy a fraction of the device for the length of the longest sequence.  Here the record-parallel transform is
 * queued on hip_stream and the per-sequence passes on hip_tail_stream behind an event, so that they run beside whatever
 * the caller queues on hip_stream next; the caller joins the two streams (an event on hip_tail_stream) before it reads
 * d_out -- and before it frees or overwrites d_coeffs, d_recs or d_rec_base: in AFG_NUMERIC_TOLERANCE the whole walk,
 * input reads included, runs on hip_tail_stream.  hip_tail_stream NULL or equal to hip_stream: afg_celt_transform_hip. */
int afg_celt_transform_streams_hip(uint32_t n_chan, const uint64_t *d_rec_base, const afg_celt_frame *d_recs,
                                   const float *d_coeffs, float *d_out, float *d_states, void *hip_stream,
                                   void *hip_tail_stream);

/* What OpusFile.readFrame and AudioStream.readSamplesFloat do to the decoder's floats (dopus.d:7923-7926,
 * :8098-8105; stream.d:480): Float2IntScaled (x * 32768 rounded to nearest even by a magic-number add, saturated
 * to int16), then int16 / 32767.0f.  Element-wise; d_out_f32 may alias d_in; either output may be NULL. */
int afg_opus_output_hip(uint64_t n_samples, const float *d_in, int16_t *d_out_i16, float *d_out_f32, void *hip_stream);
/* The same behind opus_decode_packet's output gain (dopus.d:6688-6691: every float times OpusContext.gain, applied when the
 * header gain + R128_TRACK_GAIN is not zero): x * gain rounded to float, then the conversion above. */
int afg_opus_output_gain_hip(uint64_t n_samples, const float *d_in, float gain, int16_t *d_out_i16, float *d_out_f32,
                             void *hip_stream);

/* ========================================================================== *
 *  Outer surface: the AudioStream subset (stream.d:102-637) over the host front-ends
 *  -- FLAC (native container, drflac.d:680-1695, :1887-2153), QOA (qoa.d:413-486, :703-851), MP3 Layer I / II / III
 *  (minimp3.d, minimp3_ex.d), Ogg Vorbis (stb_vorbis2.d) and Ogg Opus with CELT-only packets (dopus.d; a file that holds
 *  SILK / hybrid packets is refused at open with this library's own message), ProTracker MOD (pocketmod.d: below) ,
 *  FastTracker II XM (libxm.d: below) and WAV (wav.d: below; probed after FLAC and before QOA, stream.d:1638-1655).  Like the reference the stream decodes as the caller pulls:
 *  afg_open_from_memory parses the container only, a read that finds the FIFO empty decodes the next chunk (64 MP3 frames /
 *  Vorbis or Opus packets, 16 FLAC or QOA frames) on the device; afg_batch_decode parses whole files into transform-stage
 *  records and decodes them in one pass.  A MOD stream has no FIFO: each read runs the module's control layer on the host
 *  up to the read's end and mixes exactly those frames on the device (pocketmod_render(..., frames * 8), stream.d:611-620),
 *  so a read stops early at every pattern boundary, as the reference's does, and the first read after the song has come
 *  back to an order index it already played returns 0.  A WAV stream converts its sample bytes on the device, a chunk of
 *  about 2^18 samples at a time; a read that needs a sample the file does not hold returns 0 and sets the error state.
 * ========================================================================== */

typedef enum afg_format {          /* AudioFileFormat, stream.d:36-47 */
    AFG_FORMAT_WAV = 0, AFG_FORMAT_MP3 = 1, AFG_FORMAT_FLAC = 2, AFG_FORMAT_OGG = 3, AFG_FORMAT_OPUS = 4,
    AFG_FORMAT_QOA = 5, AFG_FORMAT_MOD = 6, AFG_FORMAT_XM = 7, AFG_FORMAT_UNKNOWN = 8
} afg_format;

#define AFG_UNKNOWN_LENGTH (-1)    /* audiostreamUnknownLength, stream.d:90 */

typedef struct afg_stream afg_stream;

/* openFromMemory (stream.d:150-170): copies the bytes, as the reference does (stream.d:2031-2041) -- `data` may be freed
 * when the call returns; never throws; returns NULL only when out of memory.  On failure the stream is in error state with the
 * reference's message (internals.d:16-23). */
afg_stream *afg_open_from_memory(const uint8_t *data, size_t length);
int         afg_is_error(const afg_stream *s);                 /* stream.d:295-301 */
const char *afg_error_message(const afg_stream *s);            /* NULL when valid, stream.d:310-316 */
int         afg_get_format(const afg_stream *s);               /* afg_format */
int         afg_get_num_channels(const afg_stream *s);
int64_t     afg_get_length_in_frames(const afg_stream *s);     /* AFG_UNKNOWN_LENGTH if unknown */
float       afg_get_samplerate(const afg_stream *s);
/* readSamplesFloat (stream.d:429-637): interleaved, returns frames read (< frames: end or error). */
int         afg_read_samples_float(afg_stream *s, float *out, int frames);
/* readSamplesDouble (stream.d:656-747): the same contract with float64 samples -- 0 on NULL, an errored or writing handle
 * or frames <= 0; the FLAC entry check, the WAV and Opus failure rules, out == NULL skipping frames, and one position
 * shared with the float read, seek and tell.  The doubles are the reference's: WAV samples converted directly
 * (wav.d:242-344: the double quotient, all 32 bits of s32, f64 as stored), FLAC the int32 sample times 1.0 / int.max
 * without narrowing (stream.d:707-717), every other format the float read widened (stream.d:732-739; QOA: qoa.d:831-838).
 * They are made on the device (afg_pcm_to_f64_hip) from the file's sample bytes (WAV), the int32 plane (FLAC) or the
 * float plane of the chunk; neither floats nor ints come to the host.  Float and double reads may be mixed on one
 * handle: each returns what a handle that only ever used its type returns at that position (a change of type is a seek
 * to the current position: what was decoded ahead in the other type is dropped and decoded again). */
int         afg_read_samples_double(afg_stream *s, double *out, int frames);
/* canSeek / seekPosition / tellPosition (stream.d:352-369, :1095-1189, :1208-1261): positions are frames; a seek outside
 * [0, length] fails and leaves the position alone (the invariants of examples/transcode's additionalTests). */
int         afg_can_seek(const afg_stream *s);
int         afg_seek_position(afg_stream *s, int frame);     /* 1 = done, 0 = refused */
int         afg_tell_position(const afg_stream *s);          /* -1 on an invalid stream (a WAV stream whose read failed
                                                                 * still tells: see the WAV section) */
void        afg_close(afg_stream *s);

/* Host front-ends on their own (no device needed): what the stream and batch entry points run
 * before the device stage.  afg_flac_parse walks the native FLAC container (drflac.d:1901-2118),
 * every frame and subframe header (drflac.d:1444-1569) and the Rice residuals (drflac.d:1279-1328)
 * and returns transform-stage records; it stops at the first frame that does not parse, like the
 * reference's read loop (drflac.d:2860).  afg_qoa_parse validates the headers (qoa.d:413-486). */
typedef struct afg_flac_parsed {
    uint32_t sample_rate, channels, bps, max_block;
    uint64_t total_samples;        /* per channel, from STREAMINFO; 0 = unknown */
    uint64_t n_frames, n_subframes, n_res, out_samples;
    afg_flac_frame    *frames;
    afg_flac_subframe *subframes;
    int32_t           *res;
    void              *owner;      /* internal */
} afg_flac_parsed;

int  afg_flac_parse(const uint8_t *data, size_t length, afg_flac_parsed *out);  /* AFG_ERR_UNSUPPORTED: not FLAC */
void afg_flac_parsed_free(afg_flac_parsed *parsed);
/* frames may be NULL (count only); at most frame_cap records are written, *n_frames gets the total. */
int  afg_qoa_parse(const uint8_t *data, size_t length, uint32_t *channels, uint32_t *samplerate,
                   uint32_t *samples, afg_qoa_frame *frames, size_t frame_cap, size_t *n_frames);

/* MP3 (MPEG-1/2/2.5 Layer III) front-end on its own: frame sync, side info, scalefactors, Huffman +
 * requantisation, stereo processing, reorder and bit reservoir (minimp3.d:487-1000, :1170-1230, :1436-1581)
 * driven the way minimp3_ex does it (ID3/APE skipping, Xing/Info tag, delay/padding: minimp3_ex.d:93-190,
 * :566-639, :787-888).  Result: the records afg_mp3_transform_hip consumes -- one plan stream per run of
 * continuous decoder state -- and the copy plan that turns its PCM plane into what mp3dec_ex_read delivers. */
typedef struct afg_mp3_copy { uint64_t src_float, count; } afg_mp3_copy;
typedef struct afg_mp3_parsed {
    int32_t  channels, hz, tagged, start_delay;
    uint64_t detected_samples;     /* 0: delivery runs to the end of the data */
    uint64_t declared_samples;     /* mp3dec_ex_t.samples; AudioStream length = this / channels (stream.d:1737) */
    uint64_t pcm_samples;          /* floats the copy plan delivers */
    uint64_t n_runs, n_blocks, n_copies;
    uint32_t *run_granules;        /* [n_runs] granules per plan stream, all with `channels` channels */
    float    *coef;                /* n_blocks * 576 */
    uint32_t *flags;               /* n_blocks, AFG_MP3_FLAGS */
    afg_mp3_copy *copies;
    void     *owner;               /* internal */
} afg_mp3_parsed;

int  afg_mp3_parse(const uint8_t *data, size_t length, afg_mp3_parsed *out);   /* AFG_ERR_UNSUPPORTED: no Layer III stream */
void afg_mp3_parsed_free(afg_mp3_parsed *parsed);

/* The same front-end in quantised mode: `coef` stays NULL, the records of afg_mp3_requant_hip come back instead
 * (coef_off = q_off = 576 * first block of the granule). */
typedef struct afg_mp3_parsed_q {
    afg_mp3_parsed    base;          /* coef == NULL */
    uint64_t          n_granules, n_sdesc;
    int16_t          *q;             /* n_blocks * 576 */
    afg_mp3_qgranule *granules;
    afg_mp3_sdesc    *sdesc;
} afg_mp3_parsed_q;

int  afg_mp3_parse_q(const uint8_t *data, size_t length, afg_mp3_parsed_q *out);
void afg_mp3_parsed_q_free(afg_mp3_parsed_q *parsed);
/* The requantiser's tables, as the device holds them (24 scalefactor-band tables = 3 kinds x 8 rate rows): band of every
 * line, destination of every line under L3_reorder, and g_pow43 (minimp3.d:722-735).  Any pointer may be NULL. */
void afg_mp3_qtables(uint8_t band_of_line[24][576], uint16_t dst_of_src[24][576], float pow43[145]);

/* Ogg Vorbis I front-end on its own: Ogg pages and lacing, the three header packets (code books, floor 1,
 * residues 0/1/2, mappings, modes: stb_vorbis2.d:2669-3266) and every audio packet up to the transform seam
 * (floor decode, residue decode, inverse coupling, floor curve: :2354-2523), plus what the pull API delivers of
 * each packet's output (first frame primed only, last-page truncation: :2531-2596, :2606-2657) and the stream
 * length (:3797-3868).  Result: the inputs of afg_vorbis_plan_create / afg_vorbis_transform_hip for one stream. */
typedef struct afg_vorbis_parsed {
    int32_t  channels, blocksize0, blocksize1;
    uint32_t sample_rate;
    uint32_t total_samples;        /* 0 = unknown */
    uint64_t n_packets, spec_floats, pcm_frames;
    uint8_t *pflags;               /* [n_packets] */
    float   *spec;                 /* per packet [channel][n/2] */
    int32_t *take_from, *take_count;   /* frames [take_from, take_from + take_count) of packet p's output are delivered */
    void    *owner;                /* internal */
} afg_vorbis_parsed;

int  afg_vorbis_parse(const uint8_t *data, size_t length, afg_vorbis_parsed *out);   /* AFG_ERR_UNSUPPORTED: not Ogg Vorbis */
void afg_vorbis_parsed_free(afg_vorbis_parsed *parsed);
/* The same with the tail of the packet decode left to the device: base.spec holds the residue vectors and the records
 * below are the inputs of afg_vorbis_floor_hip (spec_off counted from base.spec; steps per mapping, shared by its packets). */
typedef struct afg_vorbis_parsed_r {
    afg_vorbis_parsed base;
    uint64_t n_curves, n_points, n_steps;
    afg_vorbis_floor_packet *packets;  /* [base.n_packets] */
    afg_vorbis_floor_curve  *curves;   /* [n_curves] = one per packet-channel */
    int32_t *points;                   /* [2 * n_points] */
    uint8_t *steps;                    /* [2 * n_steps] */
} afg_vorbis_parsed_r;

int  afg_vorbis_parse_r(const uint8_t *data, size_t length, afg_vorbis_parsed_r *out);
void afg_vorbis_parsed_r_free(afg_vorbis_parsed_r *parsed);

/* Ogg Opus front-end on its own, CELT-only packets: Ogg pages, OpusHead / OpusTags (dopus.d:7791-7829, :8120-8193; output
 * gain :1311-1316 with R128_TRACK_GAIN :8011-8059), packet framing (ff_opus_parse_packet, :1081-1258), the range decoder
 * (:809-1034) and the CELT frame decoder up to the transform seam (:2128-3678).  Result: the inputs of
 * afg_celt_transform_hip for one stream.  frames[i] is channel 0's record of frame i, addressed for interleaved output
 * (out_off = first sample * channels, out_stride = channels); channel c of the same frame reads coef_off + c * frame_size
 * and writes out_off + c.  AFG_ERR_UNSUPPORTED: not an Ogg Opus stream the reference opens (no fields set), or one that
 * holds SILK / hybrid packets, which this front-end does not decode (channels != 0 then; afg_last_error says which). */
typedef struct afg_opus_parsed {
    int32_t  channels, preskip;
    int32_t  gain_i;               /* header gain + R128_TRACK_GAIN, Q7.8 dB; 0: the decoder does not scale */
    int32_t  error;                /* 1: a packet failed to frame; the records end there and the reference's read reports an error */
    float    gain;                 /* 10^(gain_i / 5120) as a float: afg_opus_output_gain_hip's factor */
    int32_t  pad;
    int64_t  declared_frames;      /* last page's granule position - preskip (dopus.d:8159): AudioStream's length */
    uint64_t pcm_frames;           /* frames the records decode to (the reference delivers min(pcm_frames, declared_frames)) */
    uint64_t n_frames, n_coeffs;
    afg_celt_frame *frames;
    float   *coeffs;
    void    *owner;                /* internal */
} afg_opus_parsed;

int  afg_opus_parse(const uint8_t *data, size_t length, afg_opus_parsed *out);
void afg_opus_parsed_free(afg_opus_parsed *parsed);

/* Batch decode (no reference counterpart: the throughput path).  Files are parsed by n_threads
 * pooled host threads (0 = one per physical core: half the logical CPUs of an SMT host) straight
 * into page-locked staging, restored on the current device chunk by chunk with upload, kernel and
 * download overlapped, and returned as interleaved float PCM owned by the result. */
typedef struct afg_batch_item {
    int         status;        /* afg_status of this file: a bad file never poisons the batch */
    const char *message;       /* static string, NULL when ok */
    int         format;        /* afg_format */
    int         channels;
    float       samplerate;
    int64_t     frames;
    float      *pcm;           /* frames * channels floats, NULL on error; with afg_batch_opts.sample_type ==
                                  AFG_SAMPLE_F64 it points at frames * channels doubles, with AFG_SAMPLE_PCM_* at as many
                                  samples of 1, 2 or 3 bytes (cast it) */
} afg_batch_item;

typedef struct afg_batch_result {
    int             n_files;
    afg_batch_item *items;
    void           *owner;     /* internal */
} afg_batch_result;

int  afg_batch_decode(const uint8_t *const *data, const size_t *length, int n_files, int n_threads,
                      afg_batch_result *out);
void afg_batch_free(afg_batch_result *result);

/* Device selection (files are independent -- stream.d:1363-1434 is all per-instance -- so a batch shards
 * by file across the GPUs of a node, with no exchange between devices).
 *   afg_set_device   makes `device` current for the calling host thread (HIP's current device is per thread) and
 *                    checks that it is a gfx950; plans, *_hip entries, afg_open_from_memory and afg_batch_decode
 *                    all work on the calling thread's current device.
 *   afg_batch_decode_ex  the batch entry with options: n_devices = 0 runs on the current device (what
 *                    afg_batch_decode does), n_devices = -1 on every visible device, n_devices = k > 0 on
 *                    devices[0..k) (NULL: 0..k-1; a device may be named more than once).  Files are assigned
 *                    longest-first to the least loaded device; every device gets its own host thread, helper
 *                    threads (n_threads in total, 0 = one per physical core) and stream set.  Per-file results do
 *                    not depend on the number of devices. */
/*   sample_type      AFG_SAMPLE_F32: the items' pcm are floats, as afg_batch_decode delivers them.  AFG_SAMPLE_F64: they
 *                    are the doubles of afg_read_samples_double (stream.d:656-747), made on the device in every stage
 *                    between the codec's kernels and the download -- WAV from the file's bytes, FLAC from the int32
 *                    plane, every other format from its float plane.  Any other value: AFG_ERR_INVALID, before any work. */
/*                    AFG_SAMPLE_PCM_S8 / _S16 / _S24: the items' pcm are the sample bytes WAVEncoder.writeSamples
 *                    (wav.d:482-527) makes of those floats in AFG_WAV_S8 / _S16LE / _S24LE -- the body of the WAV file
 *                    that `transcode` (readSamplesFloat, then writeSamplesFloat) writes -- made on the device
 *                    (afg_pcm_pack_hip) between the codec's kernels and the download, so that 1, 2 or 3 bytes per sample
 *                    cross the bus.  The float is the one AFG_SAMPLE_F32 delivers for that sample, for FLAC too; WAV input
 *                    is converted to float first.  Floats outside [-1, 1] are clamped and NaN becomes 0 (afg_pcm_pack_hip).
 *   dither           AFG_SAMPLE_PCM_* only.  AFG_DITHER_OFF, or AFG_DITHER_LCG31: TPDFDither.process (wav.d:679-700) with
 *                    the 31-bit generator, every file starting at draw 0 of dither_seed, so that a file's bytes depend on
 *                    nothing but the file: not on its neighbours, the stages' chunks or the devices.  AFG_DITHER_LIBC:
 *                    AFG_ERR_INVALID for the whole call, before any work -- rand() has no draw order across files. */
#define AFG_SAMPLE_F32 0
#define AFG_SAMPLE_F64 1
#define AFG_SAMPLE_PCM_S8  2
#define AFG_SAMPLE_PCM_S16 3
#define AFG_SAMPLE_PCM_S24 4
typedef struct afg_batch_opts {
    uint32_t   struct_size;    /* sizeof(afg_batch_opts) */
    int        n_threads;
    int        n_devices;
    const int *devices;
    uint32_t   sample_type;    /* AFG_SAMPLE_*; a struct_size that does not reach this field means AFG_SAMPLE_F32 */
    int        dither;         /* AFG_DITHER_OFF / AFG_DITHER_LCG31; a struct_size that does not reach these two fields */
    uint32_t   dither_seed;    /* means AFG_DITHER_OFF */
} afg_batch_opts;

int  afg_set_device(int device);
int  afg_get_device(void);                 /* current device of the calling thread, < 0: afg_status */
int  afg_batch_decode_ex(const uint8_t *const *data, const size_t *length, int n_files, const afg_batch_opts *opts,
                         afg_batch_result *out);
/* Page-locked staging buffers and the device planes of the batch path are pooled between batch calls (pinning costs about
 * as much as the transfer; freed device memory is wiped by the copy engines the next call's transfers need): this
 * releases every pooled buffer -- host and device -- that is not in use and returns the bytes freed. */
uint64_t afg_host_pool_trim(void);

/* ========================================================================== *
 *  Utilities used by the host mirror, the tests and bench.py
 * ========================================================================== */
int afg_device_malloc(void **d_ptr, size_t bytes);
int afg_device_free(void *d_ptr);
int afg_memcpy_h2d(void *d_dst, const void *src, size_t bytes, void *hip_stream);
int afg_memcpy_d2h(void *dst, const void *d_src, size_t bytes, void *hip_stream);
int afg_stream_synchronize(void *hip_stream);
/* ========================================================================== *
 *  Output side: what `transcode` needs after the decode.
 *
 *  QOA encoder: replaces qoa_encode_frame (qoa.d:295-399) and the framing of QOAEncoder (qoa.d:538-700).
 *  The LMS state of the encoder runs through a whole stream, so a stream's channels are serial; the brute-force
 *  search over the 16 scalefactors of every slice runs on 16 lanes.  Output bytes are the reference's.
 * ========================================================================== */

typedef struct afg_qoa_enc_stream {
    uint64_t pcm_off;      /* index of the stream's first sample in the interleaved input plane (int16 or float) */
    uint64_t out_off;      /* byte offset of the stream's file in the output plane (multiple of 8) */
    uint32_t samples;      /* frames (samples per channel) */
    uint32_t samplerate;   /* 1 .. 0xffffff (QOAEncoder.initialize rejects others, qoa.d:592) */
    uint8_t  channels;     /* 1 .. 8 */
    uint8_t  pad[7];
} afg_qoa_enc_stream;      /* 32 bytes */

/* Size in bytes of the QOA file for `samples` frames of `channels` channels (file header + frames). */
uint64_t afg_qoa_encoded_size(uint32_t samples, uint32_t channels);

/* Exactly one of d_pcm_i16 / d_pcm_f32 is given.  Descriptors must respect the ranges above.
 *
 * A float (or, through the write stream, double) sample x of any value, beyond full scale, infinite or NaN included,
 * becomes the int16 sample s that a release build of QOAEncoder.writeSamples (qoa.d:632-636) makes of it on x86-64:
 *     v = 32768.5 + (double)x * 32767.0
 *     t = trunc(v) if -2147483649 < v < 2147483648, else INT32_MIN (NaN falls here)
 *     s = (int16)(uint16)((uint32)t - 32768u), the low 16 bits in two's complement
 * so 1.0 is 32767, -1.0 is -32767, and 1.0001f wraps to -32766; nothing clamps.  The kernel, afg_write_samples_float,
 * afg_write_samples_double and afg_batch_encode all convert by this one definition (csrc/qoa_sample.h). */
int afg_qoa_encode_hip(uint32_t n_streams, const afg_qoa_enc_stream *d_streams, const int16_t *d_pcm_i16,
                       const float *d_pcm_f32, uint8_t *d_out, void *hip_stream);

/* WAV writer (wav.d:365-701, host only): 44-byte RIFF/WAVE header ('fmt ' of 16 bytes, tag 1 for PCM, 3 for IEEE
 * float) followed by the samples; PCM conversions are the reference's (wav.d:482-527).  afg_wav_encode is
 * EncodingOptions.enableDither = false; afg_wav_encode_dithered applies TPDFDither.process (wav.d:674-701) to the
 * integer formats first, as WAVEncoder.writeSamples does by default (stream.d:66): per sample, in order, two draws
 * rng(user) / rng_max.  rng = NULL is the reference's generator, libc rand() / RAND_MAX (rng_max ignored). */
#define AFG_WAV_S8     0
#define AFG_WAV_S16LE  1
#define AFG_WAV_S24LE  2
#define AFG_WAV_FP32LE 3
#define AFG_WAV_FP64LE 4
uint64_t afg_wav_encoded_size(uint64_t frames, uint32_t channels, int format);          /* 0: bad arguments */
/* Writes the whole file into `out` (capacity `cap`); returns the bytes written, 0 on bad arguments / short buffer. */
uint64_t afg_wav_encode(const float *samples, uint64_t frames, uint32_t channels, uint32_t samplerate, int format,
                        uint8_t *out, uint64_t cap);
typedef int (*afg_rand_fn)(void *user);        /* a draw in [0, rng_max] */
uint64_t afg_wav_encode_dithered(const float *samples, uint64_t frames, uint32_t channels, uint32_t samplerate, int format,
                                 afg_rand_fn rng, void *rng_user, uint32_t rng_max, uint8_t *out, uint64_t cap);

/* WAV sample packing on the device: float32 to the sample bytes WAVEncoder.writeSamples produces (wav.d:482-547), with
 * TPDFDither.process (wav.d:679-700) in front of the integer formats when asked for.  The mirror image of
 * afg_wav_convert_hip: spans, tiles of AFG_WAV_TILE_SAMPLES samples, one workgroup per tile.  The reference draws its
 * dither from libc rand(), one process-wide serial sequence that cannot be spread over lanes; the device draws from the
 * 31-bit generator  state = (state * 1103515245 + 12345) & 0x7fffffff  (the draw is the new state, rng_max = 0x7fffffff),
 * and sample n of a file -- counted over its interleaved samples -- uses draws 2n and 2n + 1 of the file's seed: the bytes
 * are those of afg_wav_encode_dithered with that generator as its callback. */
#define AFG_DITHER_OFF    0
#define AFG_DITHER_LIBC   1      /* EncodingOptions.enableDither = true with the reference's rand(): host only */
#define AFG_DITHER_LCG31  2

typedef struct afg_wav_pack_span { /* one run of samples of one output file (48 bytes) */
    uint64_t in_off;               /* first float in d_in, a multiple of 4 */
    uint64_t out_off;              /* first byte in d_out, a multiple of 16 */
    uint64_t count;                /* samples */
    uint64_t first_tile;           /* first tile of the span in the launch: afg_wav_pack_layout fills it in */
    uint64_t draw0;                /* index of the span's first dither draw = 2 x (samples of the file before it) */
    uint32_t seed;                 /* the file's generator starts from this state */
    uint8_t  format;               /* AFG_WAV_S8 .. AFG_WAV_FP64LE */
    uint8_t  dither;               /* 0 off, 1 the 31-bit generator (integer formats only; the float formats never dither) */
    uint8_t  pad[2];
} afg_wav_pack_span;

/* Host: the generator's state after n_draws steps from `seed` (taken modulo 2^31) -- the n-th draw itself for
 * n_draws >= 1.  The generator is an affine map modulo 2^31, so this takes 31 steps for any n_draws. */
uint32_t afg_lcg31_jump(uint32_t seed, uint64_t n_draws);
/* Host: gives every span its tiles (first_tile) and returns the launch's tile count. */
uint64_t afg_wav_pack_layout(afg_wav_pack_span *spans, uint64_t n_spans);
/* Packs every span in one launch.  d_spans is the device copy of spans laid out by afg_wav_pack_layout, n_tiles what
 * it returned; d_in and d_out are 16-byte aligned and do not overlap.  A span that does not lie inside [0, in_floats) /
 * [0, out_bytes), or whose offsets are not aligned as stated, is not touched at all.  The integer formats are defined
 * for inputs in [-1, 1] (the reference asserts). */
int afg_wav_pack_hip(uint64_t n_spans, const afg_wav_pack_span *d_spans, uint64_t n_tiles, const float *d_in,
                     uint64_t in_floats, uint8_t *d_out, uint64_t out_bytes, void *hip_stream);

/* The packer of the batch decode stages (afg_batch_opts.sample_type AFG_SAMPLE_PCM_*, afg_batch_transcode): the integer
 * formats of afg_wav_pack_hip -- the bytes of WAVEncoder.writeSamples (wav.d:482-527) and TPDFDither.process
 * (wav.d:679-700), the same generator, the same draw numbering -- for spans that start at any float of d_in and any byte
 * of d_out: a file's samples start wherever its decode stage left them in the plane.  Tiles are AFG_WAV_TILE_SAMPLES
 * samples, one workgroup per tile.  The interior of a tile is written as 16-byte words aligned in d_out's address space,
 * what lies before and behind them one byte at a time; no byte outside a span is written or read back, so spans may abut
 * inside one dword.  One difference from the host writer, which asserts |x| <= 1 (wav.d:485): decoded audio does leave
 * the range (MP3 overshoot, float WAV), so every input is clamped to [-1, 1] first and NaN becomes 0; for inputs in range
 * the bytes are afg_wav_encode's / afg_wav_encode_dithered's. */
typedef struct afg_pcm_pack_span {   /* one run of samples of one file inside a decode plane (48 bytes) */
    uint64_t in_off;     /* first float in d_in: any index */
    uint64_t out_off;    /* first byte in d_out: any offset */
    uint64_t count;      /* samples */
    uint64_t first_tile; /* filled in by afg_pcm_pack_layout */
    uint64_t draw0;      /* 2 x (samples of the file before this run) */
    uint32_t seed;       /* the file's generator starts from this state */
    uint8_t  format;     /* AFG_WAV_S8, AFG_WAV_S16LE, AFG_WAV_S24LE only */
    uint8_t  dither;     /* 0 off, 1 the 31-bit generator */
    uint8_t  pad[2];
} afg_pcm_pack_span;
/* Host: gives every span its tiles (first_tile) and returns the launch's tile count. */
uint64_t afg_pcm_pack_layout(afg_pcm_pack_span *spans, uint64_t n_spans);
/* Packs every span in one launch.  d_in is 4-byte aligned, d_out any address; the planes do not overlap.  A span that
 * does not lie inside [0, in_floats) / [0, out_bytes), or whose format is not one of the three, is not touched at all. */
int afg_pcm_pack_hip(uint64_t n_spans, const afg_pcm_pack_span *d_spans, uint64_t n_tiles, const float *d_in,
                     uint64_t in_floats, uint8_t *d_out, uint64_t out_bytes, void *hip_stream);

/* Collate on the device: runs of interleaved float samples inside a decode plane to planar, padded rows -- the
 * [files, channels, frames] float32 tensor a training or feature-extraction job on the same GPU wants, with no download.
 * A copy span: sample s = sample0 + i of its run (i < count) is frame f = s / channels, channel k = s % channels of its
 * file, and is stored at d_out[out_off + k * frames + (f - first_frame)] when k < out_channels and
 * 0 <= f - first_frame < frames; otherwise it is dropped.  The stored word is the input word (NaN payloads included).
 * A zero run (channels == 0): `count` zero floats from d_out[out_off + sample0] on -- how padding is written; the tensor is
 * never cleared as a whole.  Tiles are AFG_WAV_TILE_SAMPLES input samples (or zero floats), one workgroup per tile.  No
 * word of d_out is read back and nothing outside the stated elements is written, so spans may write neighbouring floats
 * of one row and a slab's neighbours may be foreign data.  The fields need 48 bytes; the tile table of the sibling spans
 * (first_tile) makes it 56. */
typedef struct afg_collate_span {   /* one run of one file's interleaved samples (56 bytes) */
    uint64_t in_off;      /* float index in d_in of the run's first sample: any value */
    uint64_t count;       /* samples in the run (not frames: a run may begin and end mid-frame) */
    uint64_t sample0;     /* index of that first sample in its file */
    uint64_t out_off;     /* float index in d_out of element [file, 0, 0] */
    int64_t  first_frame; /* file frame that lands at t = 0 */
    uint64_t first_tile;  /* filled in by afg_collate_layout */
    uint32_t frames;      /* T: row length, >= 1 */
    uint16_t channels;    /* of the file, 1 .. 65535; 0 = a zero run */
    uint16_t out_channels;/* C: rows of the slab, >= 1 */
} afg_collate_span;
/* Host: gives every span its tiles (first_tile) and returns the launch's tile count. */
uint64_t afg_collate_layout(afg_collate_span *spans, uint64_t n_spans);
/* Runs every span in one launch.  d_spans is the device copy of spans laid out by afg_collate_layout, n_tiles what it
 * returned; d_in (4-byte aligned; may be NULL when in_floats is 0: zero runs only) and d_out do not overlap.  Every span
 * is checked before the launch (the entry fetches d_spans on hip_stream and waits for it): a copy span must lie inside
 * [0, in_floats) and its whole slab -- out_channels * frames floats from out_off -- inside [0, out_floats), a zero run
 * inside [0, out_floats); sample0 and count are below 2^62, |first_frame| below 2^61.  Otherwise AFG_ERR_INVALID and nothing is
 * written. */
int afg_collate_hip(uint64_t n_spans, const afg_collate_span *d_spans, uint64_t n_tiles, const float *d_in, uint64_t in_floats,
                    float *d_out, uint64_t out_floats, void *hip_stream);

/* Batch decode into a padded planar device tensor: afg_batch_decode_ex without the download.  d_out is n_files * channels *
 * frames floats on the current device, and element [i, k, t] is the float AudioStream.readSamplesFloat (stream.d:429-637)
 * -- afg_batch_decode_ex with AFG_SAMPLE_F32 in the same numeric mode -- delivers as sample (first_frame[i] + t) *
 * channels_i + k of file i, for every format (FLAC and WAV go to float first, as for packed PCM); 0 where k >= channels_i,
 * where the frame is past the file's delivered end, and for a file that failed.  Every stage keeps its float plane on the
 * device and afg_collate_hip scatters each chunk into the tensor behind the stage's kernels; padding is written as zero
 * runs, once.  No decoded sample is downloaded and no host staging is taken for output.  Synchronous: when the call returns
 * every element of d_out has been written.  The current device only (one tensor lives on one device), and the whole list as
 * one pass: a slab's place follows from the file's index in the list, so the pipeline of groups of files in which
 * afg_batch_decode_ex runs large FLAC / Ogg Vorbis batches (one group parsed while the previous one's device stages run) is
 * not used here.  d_out must not be in use by work queued on another stream: the library's streams are ordered with nobody's.
 * items[i].pcm is the device address of file i's slab (NULL when the file failed; afg_batch_free does not free it);
 * frames and channels are the file's own, uncropped; status and message as afg_batch_decode_ex: a bad file never poisons
 * the batch.  Checked before any device call, AFG_ERR_INVALID with afg_last_error set: NULL opts, d_out or out; a
 * struct_size that does not reach first_frame; channels == 0 or frames == 0; a negative first_frame entry; n_files < 0.
 * n_files == 0 is AFG_OK and touches nothing. */
typedef struct afg_collate_opts {
    uint32_t       struct_size;   /* sizeof(afg_collate_opts) */
    int            n_threads;     /* as afg_batch_opts */
    uint32_t       channels;      /* C >= 1 */
    uint32_t       frames;        /* T >= 1 */
    const int64_t *first_frame;   /* per file, >= 0; NULL: 0 for every file */
} afg_collate_opts;
int afg_batch_decode_to_device(const uint8_t *const *data, const size_t *length, int n_files, const afg_collate_opts *opts,
                               float *d_out, afg_batch_result *out);

/* The writing half of AudioStream (stream.d:216-286 openToBuffer / openToMemory, :762-902 writeSamplesFloat /
 * writeSamplesDouble, :1282-1349 finalizeEncoding / finalizeAndGetEncodedResult) for WAV and QOA, on the same handle
 * type: afg_is_error, afg_error_message, afg_get_format, afg_get_num_channels, afg_get_samplerate and afg_close work
 * on it; reads and seeks return 0.  Any other format puts the stream in error state with the reference's
 * unsupported-encoding-format message (internals.d:17), every failure with its encoder-error message (:22).
 *   WAV  the 44-byte header is written at open; writes queue floats, and whenever about 2^18 samples are queued, and at
 *        finalize, one upload, one afg_wav_pack_hip launch and one download append their bytes; the dither's draw index
 *        runs on across writes.  AFG_DITHER_LIBC with an integer format is the one case that stays on the host writer's
 *        loop (afg_wav_encode_dithered): its draws are a serial, process-global sequence.  afg_write_samples_double to
 *        an fp64 stream stores the doubles as they are (wav.d:538-546), to any other it narrows to float first
 *        (stream.d:886-894).  Finalize patches the two length fields (wav.d:572-603) and reports 1: the reference
 *        reports every WAV finalize as failed (wav.d:604); this library does not.
 *   QOA  writes queue frames; finalize encodes the whole stream with one afg_qoa_encode_hip call -- the bytes of the
 *        reference's frame-by-frame writes, since the LMS state runs through the stream either way.  Doubles are
 *        converted in double (qoa.d:632-634); floats and doubles alike by the definition at afg_qoa_encode_hip, so a
 *        value beyond full scale wraps the same way whichever call wrote it.
 * afg_open_to_memory: the first write whose bytes would pass max_length writes nothing, returns 0 and sets the error
 * state; for QOA the bound is checked at finalize.  A write after finalize returns 0 and sets the error state (the
 * reference asserts). */
typedef struct afg_encoding_options {          /* EncodingOptions, stream.d:59-67 */
    uint32_t struct_size;     /* sizeof(afg_encoding_options) */
    int      sample_format;   /* AFG_WAV_*; NULL options = the reference's defaults: AFG_WAV_FP32LE, AFG_DITHER_LIBC */
    int      dither;          /* AFG_DITHER_* */
    uint32_t dither_seed;     /* AFG_DITHER_LCG31 only */
} afg_encoding_options;
/* The integer sample rate is (int)(samplerate + 0.5f) (stream.d:1852).  Return NULL only when out of memory. */
afg_stream *afg_open_to_buffer(int format, float samplerate, int channels, const afg_encoding_options *opts);
afg_stream *afg_open_to_memory(uint8_t *data, size_t max_length, int format, float samplerate, int channels,
                               const afg_encoding_options *opts);
int  afg_is_open_for_reading(const afg_stream *s);           /* stream.d:377-391 */
int  afg_is_open_for_writing(const afg_stream *s);
int  afg_write_samples_float(afg_stream *s, const float *in, int frames);     /* frames written */
int  afg_write_samples_double(afg_stream *s, const double *in, int frames);
int  afg_finalize_encoding(afg_stream *s);                   /* 1 = done */
/* Buffer streams only: finalizes if that has not happened and hands out the file, owned by the stream and valid until
 * afg_close; may be called again.  1 = done. */
int  afg_finalize_and_get_encoded(afg_stream *s, const uint8_t **bytes, size_t *length);

/* Batch encode (no reference counterpart: the throughput path outward, the mirror of afg_batch_decode).  Interleaved
 * float PCM in host memory becomes file bytes in host memory, on the current device: pooled threads copy the PCM into
 * page-locked staging, chunks go through two staging and two pairs of device buffers with upload, kernel and download
 * overlapped, and the files land in a page-locked plane owned by the result.  format is AFG_FORMAT_WAV (opts as above;
 * every file's dither starts at draw 0 of dither_seed, so a file's bytes depend on nothing but the file) or
 * AFG_FORMAT_QOA.  A bad item -- no or too many channels (WAV 1..1024, QOA 1..8), a sample rate out of range, NULL pcm
 * with frames > 0, a QOA of 2^32 frames or more -- carries its own status and never poisons the batch.
 * AFG_DITHER_LIBC with an integer WAV format is refused for the whole call (AFG_ERR_UNSUPPORTED): there is no defined
 * draw order across files. */
typedef struct afg_encode_input { const float *pcm; uint64_t frames; uint32_t channels; float samplerate; } afg_encode_input;
typedef struct afg_encoded_item { int status; const char *message; uint8_t *bytes; uint64_t size; } afg_encoded_item;
typedef struct afg_encode_result { int n_files; afg_encoded_item *items; void *owner; } afg_encode_result;
int  afg_batch_encode(const afg_encode_input *in, int n_files, int format, const afg_encoding_options *opts,
                      int n_threads, afg_encode_result *out);
void afg_encode_free(afg_encode_result *r);

/* Batch transcode: the reference's example program `transcode` (open, readSamplesFloat, writeSamplesFloat to a WAV,
 * finalize: stream.d:480-570, :762-832, wav.d:365-603) for a batch of files in one call.  Every file goes through
 * afg_batch_decode_ex with the sample type that enc->sample_format asks for -- AFG_SAMPLE_PCM_* for the integer formats,
 * AFG_SAMPLE_F32 / AFG_SAMPLE_F64 for the float ones -- so the body of each WAV file is made on the device and crosses
 * the bus once, at its own width; the pooled host threads then put the 44-byte header in front (one host copy per file).
 * Item i is a complete WAV file: the bytes of afg_wav_encode[_dithered] over the floats afg_batch_decode_ex returns for
 * file i, with its channel count and (int)(samplerate + 0.5f) (stream.d:1852); floats outside [-1, 1] are clamped and NaN
 * becomes 0 for the integer formats (afg_pcm_pack_hip).  enc NULL: AFG_WAV_FP32LE.  enc->dither follows afg_batch_opts.dither
 * (AFG_DITHER_LIBC with an integer format: AFG_ERR_INVALID); the float formats never dither.  opts (may be NULL) supplies
 * threads and devices; its sample_type and dither are ignored.  A file that does not decode is an item with the decoder's
 * status and message and no bytes.  out_format: AFG_FORMAT_WAV.  AFG_FORMAT_QOA is refused (AFG_ERR_UNSUPPORTED): the QOA
 * encoder's LMS state runs through a whole file and the decode stages cut files at chunk borders.  Free the result with
 * afg_encode_free. */
int  afg_batch_transcode(const uint8_t *const *data, const size_t *length, int n_files, int out_format,
                         const afg_encoding_options *enc, const afg_batch_opts *opts, afg_encode_result *out);

/* ========================================================================== *
 *  ProTracker MOD (pocketmod.d; stream.d:1796-1830): 2 channels at 44100 Hz, length AFG_UNKNOWN_LENGTH, one numeric mode
 *  (both AFG_NUMERIC settings give the same bits).  The control layer -- pattern lines, effects, LFOs, tempo, once per tick
 *  (pocketmod.d:354-662) -- runs on the host and describes the mix as segment records: a run of output frames over which
 *  one channel steps through one sample with a fixed increment (one pass of the loop at pocketmod.d:684-720).  The device
 *  mixer (afg_mod_render_hip) resamples, scales and adds them in channel order, bit-identical to pocketmod_render.
 *  Probe: MOD is tried last, after every other format; files that begin like a RIFF/WAVE file or pass the XM header check
 *  (libxm.d:360-380) are left to those formats and stay refused.
 *  The batch path's output (afg_batch_decode, afg_mod_parse) is the reference's read loop with requests as long as the
 *  frames left below AFG_MOD_MAX_FRAMES: every read runs to its pattern boundary, so reads cut the mix at tick boundaries
 *  only; the loop ends at the first read after the song returns to a visited order index (stream.d:614).  A song that never
 *  does is cut at AFG_MOD_MAX_FRAMES (30 minutes): the item is AFG_OK, with frames == AFG_MOD_MAX_FRAMES and a message.
 * ========================================================================== */
#define AFG_MOD_MAX_FRAMES (30 * 60 * 44100)

typedef struct afg_mod_song {      /* one song of a launch (48 bytes) */
    uint64_t out_frame;            /* first stereo frame of the song in d_out */
    uint64_t tick_base;            /* first afg_mod_tick of the song */
    uint64_t seg_base;             /* first afg_mod_segment of the song */
    uint64_t sample_base;          /* first byte of the song's sample plane in d_sample_bytes */
    uint32_t n_ticks;
    uint32_t sample_bytes;         /* bytes of the plane (sample area of the file, then zero padding) */
    uint64_t reserved;             /* 0 */
} afg_mod_song;

typedef struct afg_mod_tick {      /* a run of output frames mixed with one set of channel states (24 bytes) */
    uint32_t frame, frames;        /* first output frame (relative to the song) and count */
    uint32_t seg, n_seg;           /* its segments: song seg_base + seg ..., channels in index order */
    int16_t pattern, line;         /* song position when the run was mixed */
    uint32_t pad;
} afg_mod_tick;

typedef struct afg_mod_segment {   /* one channel stepping through one sample (48 bytes) */
    uint32_t frame, frames;        /* output frames (relative to the song) */
    float position, increment;     /* position at `frame`; position += increment per frame */
    float level_l, level_r;        /* output += level * data[(int)position] */
    uint32_t sample_off;           /* byte offset of the sample in the song's plane */
    int32_t loop_start, loop_length, loop_end, length;
    uint32_t channel;
} afg_mod_segment;

/* Mixes every tick of n_songs songs into d_out (interleaved float pairs): each frame of a tick starts at +0.0f and takes
 * level_l * s, level_r * s of every segment that covers it, segments in record order.  s = (float)(int8)byte at
 * sample_off + (int)position of the song's plane; an index outside [0, sample_bytes) reads 0.  Positions are
 * position + increment added sequentially (exactly: mod_chain.h), as pocketmod.d:691-705 does.  Songs, ticks and segments
 * are device arrays; the songs' ticks follow one another in song order (tick_base ascending), and the ticks of a song cover
 * its frames once.  d_out is 16-byte aligned. */
int afg_mod_render_hip(uint32_t n_songs, const afg_mod_song *d_songs, const afg_mod_segment *d_segments,
                       const afg_mod_tick *d_ticks, const uint8_t *d_sample_bytes, float *d_out, void *hip_stream);

/* Host front-end on its own (no device needed): the batch path's control layer for one file (definition above). */
typedef struct afg_mod_parsed {
    uint32_t channels;             /* the module's channels (1..32) */
    uint32_t capped;               /* 1: cut at AFG_MOD_MAX_FRAMES */
    uint64_t n_frames, n_ticks, n_segments, n_sample_bytes;
    afg_mod_tick *ticks;           /* song-relative: seg indexes into segments */
    afg_mod_segment *segments;
    uint8_t *sample_bytes;         /* the plane the segments' sample_off point into */
    void *owner;                   /* internal */
} afg_mod_parsed;
int  afg_mod_parse(const uint8_t *data, size_t length, afg_mod_parsed *out);    /* AFG_ERR_UNSUPPORTED: not a MOD */
void afg_mod_parsed_free(afg_mod_parsed *p);

/* ========================================================================== *
 *  FastTracker II XM (libxm.d; stream.d:595-605, :1751-1793): 2 channels at 44100 Hz, xm_set_max_loop_count(ctx, 1),
 *  length AFG_UNKNOWN_LENGTH, one numeric mode.  The loader and the control layer (xm_row, xm_tick, envelopes, effects:
 *  libxm.d:1154-2311) run on the host once per tick and describe the mix as records; the device mixer (afg_xm_render_hip)
 *  does the per-frame layer (xm_next_of_sample, xm_sample: libxm.d:2313-2475), bit-identical float32.
 *  A segment is one channel stepping through one sample in one direction: no loop wrap, ping-pong turn or sample end
 *  falls inside it (the host does those itself, with the reference's float operations), and it is of one kind: its
 *  volumes are steady or ramping (XM_SLIDE_TOWARDS per frame), and it is inside the 32-frame cross-fade after a trigger
 *  or not.  What cannot be computed in closed form travels in a side table of floats (`aux`): the ramp's volumes per
 *  frame, the cross-fade's stored values per frame, and for a segment that runs backwards (or whose step is not a finite
 *  number >= 0) the position at the first frame of each group of 16 song-relative frames.
 *  Probe: XM is tried directly before MOD (stream.d:1751).  A file with the XM header that the loader refuses stays
 *  refused.  A read returns 0 once the loop count is >= 1, else exactly the frames asked for; ticks that start with a loop
 *  count >= 1 are zeros (libxm.d:2438).  The batch path's output is the frames before the tick that raises the loop count
 *  to 1, cut at AFG_MOD_MAX_FRAMES like a MOD.
 * ========================================================================== */
#define AFG_XM_SEG_16BIT    1u     /* int16 samples (scaled by 1/32768), else int8 (1/128) */
#define AFG_XM_SEG_BACK     2u     /* position -= step per frame */
#define AFG_XM_SEG_TABLE    4u     /* lane start positions from aux_pos (else the closed form of mod_chain.h) */
#define AFG_XM_SEG_RAMP     8u     /* volumes per frame from aux_vol (left, right pairs), else vol_l / vol_r */
#define AFG_XM_SEG_FADE     16u    /* XM_LERP(aux_fade[k], s, (fade_count + k) / 32) */

typedef struct afg_xm_song {       /* one song of a launch (64 bytes) */
    uint64_t out_frame;            /* first stereo frame of the song in d_out */
    uint64_t tick_base;            /* first afg_xm_tick of the song */
    uint64_t seg_base;             /* first afg_xm_segment of the song */
    uint64_t sample_base;          /* first byte of the song's sample data in d_sample_bytes (a multiple of 2) */
    uint64_t aux_base;             /* first float of the song's side table in d_aux */
    uint32_t n_ticks;
    uint32_t sample_bytes;
    uint64_t reserved[2];          /* 0 */
} afg_xm_song;

/* A tick, or a piece of one: a read's end cuts a tick, and a tick longer than 4096 frames is written as several records. */
typedef struct afg_xm_tick {       /* a run of output frames mixed with one set of channel states (32 bytes) */
    uint32_t frame, frames;        /* first output frame (relative to the song) and count */
    uint32_t seg, n_seg;           /* its segments: song seg_base + seg ..., channels in index order */
    float scale;                   /* global_volume * amplification, applied to the channel sum */
    int16_t table_index, row;      /* song position when the run was mixed */
    uint32_t loop_count;           /* >= 1: the frames are zeros and no channel steps */
    uint32_t pad;
} afg_xm_tick;

typedef struct afg_xm_segment {    /* 64 bytes */
    uint32_t frame, frames;        /* output frames (relative to the song) */
    uint32_t sample_off;           /* byte offset of the sample in the song's sample data */
    uint32_t last;                 /* sample length - 1, in samples: an index above it reads this one */
    uint32_t flags;                /* AFG_XM_SEG_* */
    uint32_t channel;
    float position, step;          /* position at `frame` */
    float vol_l, vol_r;            /* steady volumes */
    uint32_t aux_vol, aux_fade, aux_pos;   /* song-relative float indexes into the side table */
    uint32_t fade_count;           /* frame_count at `frame` */
    uint32_t pad[2];
} afg_xm_segment;

/* Mixes every tick of n_songs songs into d_out (interleaved float pairs), as afg_mod_render_hip does for MOD records:
 * each frame starts at +0.0f, takes s * vol of every segment that covers it in record order (separate multiply and add),
 * and is then multiplied by the tick's scale.  All arrays are device arrays; d_out is 16-byte aligned. */
int afg_xm_render_hip(uint32_t n_songs, const afg_xm_song *d_songs, const afg_xm_segment *d_segments,
                      const afg_xm_tick *d_ticks, const uint8_t *d_sample_bytes, const float *d_aux, float *d_out,
                      void *hip_stream);

/* Host front-end on its own (no device needed): the batch path's loader and control layer for one file. */
typedef struct afg_xm_parsed {
    uint32_t channels;
    uint32_t capped;               /* 1: cut at AFG_MOD_MAX_FRAMES */
    uint32_t length, patterns, instruments, restart;
    uint64_t n_frames, n_ticks, n_segments, n_sample_bytes, n_aux;
    afg_xm_tick *ticks;
    afg_xm_segment *segments;
    uint8_t *sample_bytes;         /* delta-decoded sample data (int8, or int16 in host order at even offsets) */
    float *aux;
    void *owner;                   /* internal */
} afg_xm_parsed;
int  afg_xm_parse(const uint8_t *data, size_t length, afg_xm_parsed *out);      /* AFG_ERR_UNSUPPORTED: not an XM */
void afg_xm_parsed_free(afg_xm_parsed *p);

/* The module half of AudioStream (stream.d:330-345, :906-1080) for a MOD or XM stream; 0 / -1 on any other stream.
 * For an XM: pattern count and length are xm_get_number_of_patterns / xm_get_module_length, rows are per pattern (-1 out
 * of range, stream.d:979-983), tell is current_table_index / current_row, and afg_module_seek is xm_seek (libxm.d:951-959:
 * index, row, tick 0, remaining_samples_in_tick = 0, channels untouched) for an index inside the order and a row below 256.
 * afg_can_seek is 1 for a MOD (stream.d:366); afg_seek_position(frame) refuses it (the reference asserts, stream.d:1097).
 * afg_module_seek is pocketmod_seek (pocketmod.d:954-962) as written: it sets the order index and line, tick 0, and
 * checks nothing. */
int afg_is_module(const afg_stream *s);
int afg_module_pattern_count(const afg_stream *s);           /* countModulePatterns: num_patterns */
int afg_module_length(const afg_stream *s);                  /* getModuleLength: patterns in the order */
int afg_module_rows_in_pattern(const afg_stream *s, int pattern);   /* 64 */
int afg_module_tell_pattern(const afg_stream *s);
int afg_module_tell_row(const afg_stream *s);
int afg_module_seek(afg_stream *s, int pattern, int row);    /* 1 = done */

/* ========================================================================== *
 *  WAV (wav.d:21-358; stream.d:557-570, :1197-1199, :1249-1251, :1638-1655): RIFF/WAVE with PCM of 8 / 16 / 24 / 32 bits
 *  or IEEE float of 32 / 64 bits, any channel count up to 65535, length = the frames the 'data' chunk declares.
 *  The host walks the chunks the way WAVDecoder.scan does (afg_wav_parse; its habits and the two refusals that are this
 *  library's own are listed in INTEGRATION.md); the device converts the sample bytes, as they are in the file, to
 *  float32 with readSamples!float's arithmetic (afg_wav_convert_hip), bit-identical; f64 NaNs stay NaNs.
 *  Stream: afg_seek_position(frame) succeeds for 0 <= frame <= length; a read returns min(frames, length - position)
 *  frames; when the file does not hold all the samples of that read (a 'data' chunk cut short), or the format is one the
 *  scan lets through and readSamples refuses (PCM of 64 bits, float of 8 / 16 / 24), the read returns 0 and the stream
 *  is in error state with the reference's decoding-error message.  As in the reference (wav.d:253) the position has
 *  advanced by the clamped request all the same, and afg_tell_position still reports it.
 *  Batch: one read of the whole declared length; a file for which that read fails is an error item (AFG_ERR_INVALID,
 *  the decoding-error message, format AFG_FORMAT_WAV).
 * ========================================================================== */
#define AFG_WAV_KIND_U8   0      /* (b - 128) / 127.0           wav.d:297 */
#define AFG_WAV_KIND_S16  1      /* s / 32767.0                 wav.d:307 */
#define AFG_WAV_KIND_S24  2      /* sign-extended / 8388607.0   wav.d:318-319 */
#define AFG_WAV_KIND_S32  3      /* s / 2147483648.0            wav.d:329 */
#define AFG_WAV_KIND_F32  4      /* the bits as they are        wav.d:266-269 */
#define AFG_WAV_KIND_F64  5      /* narrowed to float           wav.d:276-279 */
#define AFG_WAV_TILE_SAMPLES 4096u

typedef struct afg_wav_span {      /* a run of samples of one kind (40 bytes) */
    uint64_t in_off;               /* first byte in d_in; 16-byte aligned for the fast path (any offset is converted) */
    uint64_t out_off;              /* first float in d_out; a multiple of 4 for the fast path */
    uint64_t count;                /* samples (little-endian, interleaved as in the file) */
    uint64_t tile_first;           /* first tile of the span in the launch: afg_wav_layout fills it in */
    uint32_t kind;                 /* AFG_WAV_KIND_* */
    uint32_t pad;
} afg_wav_span;

/* Host: gives every span its tiles of AFG_WAV_TILE_SAMPLES samples (tile_first) and returns the launch's tile count. */
uint64_t afg_wav_layout(afg_wav_span *spans, uint64_t n_spans);
/* Converts every span in one launch, one workgroup per tile.  d_spans is the device copy of spans laid out by
 * afg_wav_layout, n_tiles what it returned.  A span that does not lie inside [0, in_bytes) / [0, out_floats) is not
 * converted at all.  Input and output must not overlap. */
int afg_wav_convert_hip(uint64_t n_spans, const afg_wav_span *d_spans, uint64_t n_tiles, const uint8_t *d_in, uint64_t in_bytes,
                        float *d_out, uint64_t out_floats, void *hip_stream);

/* The same spans to float64: readSamples!double (wav.d:242-344) for the six WAV kinds, and what AudioStream.
 * readSamplesDouble does to the other decoders' output (stream.d:656-747).  out_off and count are in doubles; the fast
 * path needs in_off 16-byte aligned and out_off even.  Bit-identical to IEEE float64 arithmetic:
 *   U8 / S16 / S24  the correctly rounded quotient of the integer by 127.0 / 32767.0 / 8388607.0   wav.d:297-319
 *   S32             s / 2147483648.0, exact                                                         wav.d:329
 *   F32             widened: denormals kept, a quiet NaN keeps sign and payload, a signalling NaN comes out a NaN with
 *                   its sign (stream.d:732-739 for the float decoders' planes)                      wav.d:266-269
 *   F64             the 64 bits as they are                                                         wav.d:276-279
 *   FLAC_S32        (double)s * (1.0 / 2147483647.0), one rounding: drflac_read_s32's int32          stream.d:713-716
 * A span that does not lie inside [0, in_bytes) / [0, out_doubles) is not converted at all. */
#define AFG_F64_KIND_FLAC_S32 6
int afg_pcm_to_f64_hip(uint64_t n_spans, const afg_wav_span *d_spans, uint64_t n_tiles, const uint8_t *d_in, uint64_t in_bytes,
                       double *d_out, uint64_t out_doubles, void *hip_stream);

/* Host front-end on its own (no device needed): WAVDecoder.scan.  AFG_ERR_UNSUPPORTED: the scan refuses the file
 * (afg_last_error carries the reference's reason). */
typedef struct afg_wav_parsed {
    uint32_t tag;                  /* 1 PCM, 3 IEEE float (an extensible header with the float GUID has become 3) */
    uint32_t channels, bits, sample_rate;
    uint32_t frames;               /* declared by the 'data' chunk */
    int32_t  kind;                 /* AFG_WAV_KIND_*, or -1: opens, and the first read fails */
    uint64_t samples_offset;       /* byte offset of the first sample */
    uint64_t present_samples;      /* whole samples the file holds from there, at most frames * channels */
} afg_wav_parsed;
int afg_wav_parse(const uint8_t *data, size_t length, afg_wav_parsed *out);

/* Streaming device-to-device copy (16-byte aligned) used by bench.py to measure the copy rate this device
 * actually sustains, the practical ceiling the HBM-bound kernels are compared with next to the 8 TB/s spec. */
int afg_copy_probe_hip(void *d_dst, const void *d_src, size_t bytes, void *hip_stream);

/* Test aid: fills the LDS of every compute unit with `word` (workgroups of 160 KiB, many times the CU count).  LDS is not
 * cleared between kernels, so a kernel that reads a location it never wrote normally finds zeros or old finite data and
 * passes; with 0x7fc00000 (NaN) behind it such a read shows.  The GPU tests run every case behind this. */
int afg_lds_fill_probe_hip(uint32_t word, void *hip_stream);

/* Sample-rate conversion and mono downmix behind the collate: afg_batch_decode_to_device's tensor at ONE sample rate.  The
 * reference has no resampler (AudioStream delivers every file at its own rate), so nothing of it is restated here: the
 * definition below is this library's own, and tests/resample_model.py states it again in numpy.
 *
 * The filter is a Hann-windowed sinc with Z zero crossings (lowpass_width; 0 means 6) and roll-off 0.99.  For a file rate
 * `in` and a target rate `out`: g = gcd(in, out), M = in / g, L = out / g, fc = 0.99 * min(1, L / M), W = ceil(Z / fc),
 * K = 2 W.  The tap of phase p in [0, L) and index k in [0, K): d = (k - (W - 1)) - p / L, x = clamp(d * fc, -Z, Z),
 * h[p][k] = fc * sinc(x) * cos(pi x / (2 Z))^2 with sinc(x) = sin(pi x) / (pi x), computed in double and rounded once to
 * float32.  Output frame t of a row: q = in_frame0 + floor(t * M / L), p = (t * M) mod L, and y[t] is the sum over
 * k = 0 .. K - 1, in that order and starting from +0.0f, of h[p][k] * x[q - (W - 1) + k]: every product rounded to float32,
 * then every add, no fused multiply-add.  Input indexes outside [0, in_frames) contribute nothing.  Equal rates have no
 * filter (M = L = 1, W = 0): y[t] is the input word at q, NaN payloads included, +0.0f when q lies outside the row.
 * The mono mix comes before the filter: for in_rows = R rows s = x[0], then s = s + x[r] in row order, m = s / (float)R
 * (the IEEE division); for R == 1 the row itself.
 *
 * afg_resample_taps: host only, no device needed.  Returns L * K, the floats the table of (in_rate, out_rate,
 * lowpass_width) needs, sets *M, *L, *W (each may be NULL) and fills taps[p * K + k] when cap >= L * K (taps may be NULL
 * with cap 0).  Equal rates: returns 0 with *M = *L = 1, *W = 0, and no error.  Returns 0 with *M = *L = *W = 0 and
 * afg_last_error set for a rate of 0, a lowpass_width above 64, or a table of more than 2^22 floats. */
uint64_t afg_resample_taps(uint32_t in_rate, uint32_t out_rate, uint32_t lowpass_width, float *taps, uint64_t cap,
                           uint32_t *M, uint32_t *L, uint32_t *W);
typedef struct afg_resample_row {   /* one output row (72 bytes) */
    uint64_t in_off;      /* float index in d_in of frame 0 of the file's first row */
    uint64_t in_stride;   /* floats from one input row of the file to the next */
    int64_t  in_frame0;   /* input frame of output frame 0: any value below 2^61 in size, before and past the row included */
    uint64_t out_off;     /* float index in d_out of y[0] */
    uint64_t first_tile;  /* filled in by afg_resample_layout */
    uint64_t taps_off;    /* float index in d_taps of h[0][0] (unused when W == 0) */
    uint32_t in_rows;     /* R: rows mixed into this one, 1 .. 65535 (1: no mix); unused when in_frames == 0 */
    uint32_t in_frames;   /* frames of every input row; 0: the row is +0.0f throughout and d_in is not read */
    uint32_t out_frames;  /* floats written */
    uint32_t M, L, W;     /* as afg_resample_taps gives them: 1 <= M, L <= 2^20; W == 0 only with M == L == 1 */
} afg_resample_row;
/* Host: gives every row its tiles (first_tile) and returns the launch's tile count.  A tile is 1024 output frames of one
 * row, fewer (512 ... 64) while the input frames a tile needs -- floor(tile * M / L) + 2 W + 1 -- exceed 4096. */
uint64_t afg_resample_layout(afg_resample_row *rows, uint64_t n_rows);
/* Runs every row in one launch, one workgroup per tile.  d_rows is the device copy of rows laid out by afg_resample_layout,
 * n_tiles what it returned; d_in, d_taps (4-byte aligned; NULL allowed when no row reads them) and d_out do not overlap.
 * Every record is checked before the launch (the entry fetches d_rows on hip_stream and waits for it): its input rows --
 * in_frames floats from in_off + r * in_stride, r < in_rows -- must lie inside [0, in_floats), its table of L * 2 W floats
 * inside [0, taps_floats), its out_frames floats inside [0, out_floats), and M, L, W and in_frame0 inside the ranges
 * above.  Otherwise AFG_ERR_INVALID and nothing is written.  The kernel writes exactly out_frames floats per record and
 * reads no input float outside [0, in_frames) of the record's rows. */
int afg_resample_hip(uint64_t n_rows, const afg_resample_row *d_rows, uint64_t n_tiles, const float *d_in, uint64_t in_floats,
                     const float *d_taps, uint64_t taps_floats, float *d_out, uint64_t out_floats, void *hip_stream);

/* afg_batch_decode_to_device at one sample rate: d_out is n_files * channels * frames floats on the current device, and
 * element [i, k, t] is the definition above applied to what afg_batch_decode_ex with AFG_SAMPLE_F32 delivers for file i in
 * the same numeric mode -- row k of the file, or with `mono` (channels must be 1) the mix of all its rows -- from the
 * file's rate to `samplerate`, with in_frame0 = first_frame[i] (in the file's own frames, as in afg_collate_opts).
 * Without mono a row k >= channels_i is zero; the slab of a file that failed is zero.  Two kinds of file are refused with
 * status AFG_ERR_UNSUPPORTED, a message of this library's own that names both numbers, and a zero slab, their neighbours
 * undisturbed: a file whose rate is 0 or above max_in_rate, and -- with mono -- a file with more channels than
 * in_channels.  (So is a file whose rate makes a table afg_resample_taps refuses.)
 * The collate pass of afg_batch_decode_to_device runs at the files' own rates into a pooled scratch of
 * [files, R, ceil(frames * max_in_rate / samplerate) + 2 H + 1] floats, R = channels or in_channels and H the W of
 * max_in_rate; then one afg_resample_hip launch writes every element of d_out.  A list whose scratch would exceed
 * afg_dev_option("resample_scratch_bytes") (default 2 GiB) is processed in sublists of at least one file.  Synchronous,
 * the current device only, and d_out as for afg_batch_decode_to_device.  items[i] keeps the file's own frames, channels
 * and samplerate; pcm is the device address of its slab (NULL when the file failed or was refused).
 * Checked before any device call, AFG_ERR_INVALID with afg_last_error set: NULL opts, d_out or out; a struct_size that does
 * not reach lowpass_width; channels == 0 or frames == 0; samplerate == 0 or above 2^20; mono with channels != 1; in_channels
 * above 65535; max_in_rate above 2^20; lowpass_width above 64; a negative first_frame entry; n_files < 0; a scratch row of
 * 2^32 floats or more.  n_files == 0 is AFG_OK and touches nothing. */
typedef struct afg_resample_opts {
    uint32_t       struct_size;   /* sizeof(afg_resample_opts) */
    int            n_threads;     /* as afg_batch_opts */
    uint32_t       channels;      /* C >= 1 */
    uint32_t       frames;        /* T >= 1, at `samplerate` */
    const int64_t *first_frame;   /* per file, >= 0, in the file's own frames; NULL: 0 for every file */
    uint32_t       samplerate;    /* of the tensor, Hz */
    uint32_t       mono;          /* 0, or 1: channels == 1 and the row is the mean of the file's rows */
    uint32_t       in_channels;   /* mono: rows of a file kept for the mix, 0 means 2 */
    uint32_t       max_in_rate;   /* 0 means 48000 */
    uint32_t       lowpass_width; /* Z, 0 means 6 */
} afg_resample_opts;
int afg_batch_decode_resampled(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                               float *d_out, afg_batch_result *out);

/* Log-mel spectrogram features behind the tensor at one sample rate: a short-time Fourier transform by direct matrix
 * product, the power spectrum, a dense mel filter bank and an optional log10, in one kernel on the float32 matrix
 * instruction.  The reference has no such stage (and no resampler either), so nothing of it is restated here: the
 * definition below is this library's own, and tests/melspec_model.py states it again in numpy.
 *
 * Parameters of a call (afg_mel_params), uniform over its rows: n_fft 16 .. 2048, win_length 1 .. n_fft, hop 1 .. n_fft,
 * n_mels 1 .. 256, center 0 or 1, pad_mode AFG_MEL_PAD_REFLECT or AFG_MEL_PAD_ZERO, out_kind AFG_MEL_POWER or
 * AFG_MEL_LOG10, log_floor a finite float >= 0 (0 means 1e-10f).  n_bins = n_fft / 2 + 1.
 *
 * Basis, computed on the host in double and rounded once to float32.  The window is a periodic Hann of win_length,
 * w[j] = 0.5 - 0.5 cos(2 pi j / win_length), centred in the frame: n_lo = (n_fft - win_length) / 2 and sample n of a frame
 * uses w[n - n_lo].  For n in [n_lo, n_lo + win_length) and k in [0, n_bins):
 *   C[n][k] = float32( w * cos(2 pi ((n * k) mod n_fft) / n_fft)),  S[n][k] = float32(-w * sin(2 pi ((n * k) mod n_fft) / n_fft)),
 * the product n * k reduced in integers before the trigonometry.
 *
 * Frame f of a row of in_frames samples: sample n is x[idx(f * hop + n - pad)] with pad = center ? n_fft / 2 : 0.  An index
 * outside [0, in_frames) is reflected without repeating the edge (-i -> i, in_frames - 1 + i -> in_frames - 1 - i) or
 * contributes +0.0f, according to pad_mode.  Reflect needs in_frames > pad: a record with output that breaks this is refused
 * before the launch.  The row has max_frames = 1 + (in_frames + 2 pad - n_fft) / hop frames, 0 when the numerator is negative
 * (afg_mel_frames); a record asks for out_frames <= max_frames.
 *
 * Arithmetic: every sum starts from +0.0f and runs in ascending index order, one fmaf per term and nothing wider:
 *   re[k] = chain over n = n_lo .. n_lo + win_length - 1 of fmaf(x_n, C[n][k], acc), im[k] likewise with S,
 *   p[k] = fmaf(im, im, re * re) with the product rounded to float32,
 *   mel[m] = chain over k = 0 .. n_bins - 1 of fmaf(Wm[m][k], p[k], acc): all bins, a dense weight matrix.
 * AFG_MEL_POWER delivers mel, AFG_MEL_LOG10 log10f(fmaxf(mel, log_floor)) (fmaxf: a NaN mel gives the floor).
 * Output: [rows, n_mels, out_frames] float32, frames contiguous: record r's mel m, frame f at out_off + m * out_frames + f.
 *
 * afg_mel_basis: host only.  Returns win_length * ld floats, ld = 2 * nb16 and nb16 = n_bins rounded up to 16, and with
 * cap >= that fills out[j * ld + k] = C[n_lo + j][k] and out[j * ld + nb16 + k] = S[n_lo + j][k], +0.0f in the columns
 * k >= n_bins (out may be NULL with cap 0).  Returns 0 with afg_last_error set for n_fft or win_length out of range.
 *
 * afg_mel_filters: host only.  Returns n_mels * n_bins and with cap >= that fills out[m * n_bins + k] = Wm[m][k]: n_mels + 2
 * points equally spaced on the mel scale from f_min to f_max (0 means samplerate / 2), converted back to Hz as
 * f[0 .. n_mels + 1]; bin k lies at fk = k * samplerate / n_fft;
 *   Wm[m][k] = max(0, min((fk - f[m]) / (f[m+1] - f[m]), (f[m+2] - fk) / (f[m+2] - f[m+1]))),
 * with AFG_MEL_NORM_SLANEY times 2 / (f[m+2] - f[m]); computed in double, rounded once to float32.  Scales:
 * AFG_MEL_SCALE_SLANEY mel = 3 f / 200 below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 above; AFG_MEL_SCALE_HTK
 * 2595 log10(1 + f / 700).  Returns 0 with afg_last_error set for samplerate 0, n_fft or n_mels out of range, an unknown
 * scale or norm, or not 0 <= f_min < f_max <= samplerate / 2.  The kernel entry takes any dense float32 [n_mels, n_bins]
 * matrix of the caller's own instead. */
#define AFG_MEL_PAD_REFLECT 0
#define AFG_MEL_PAD_ZERO    1
#define AFG_MEL_POWER       0
#define AFG_MEL_LOG10       1
#define AFG_MEL_SCALE_SLANEY 0
#define AFG_MEL_SCALE_HTK    1
#define AFG_MEL_NORM_NONE    0
#define AFG_MEL_NORM_SLANEY  1
typedef struct afg_mel_params {     /* 32 bytes */
    uint32_t n_fft, win_length, hop, n_mels;
    uint32_t center, pad_mode, out_kind;
    float    log_floor;
} afg_mel_params;
typedef struct afg_mel_row {        /* one input row and its [n_mels, out_frames] output (32 bytes) */
    uint64_t in_off;      /* float index in d_in of sample 0 */
    uint64_t out_off;     /* float index in d_out of mel 0, frame 0 */
    uint64_t first_tile;  /* filled in by afg_mel_layout */
    uint32_t in_frames;   /* samples of the row; 0: d_in is not read */
    uint32_t out_frames;  /* frames written per mel, <= afg_mel_frames(params, in_frames) */
} afg_mel_row;
uint64_t afg_mel_basis(uint32_t n_fft, uint32_t win_length, float *out, uint64_t cap);
uint64_t afg_mel_filters(uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double f_min, double f_max, uint32_t scale, uint32_t norm,
                         float *out, uint64_t cap);
/* max_frames of a row of in_frames samples; 0 for params out of range (afg_last_error set). */
uint32_t afg_mel_frames(const afg_mel_params *params, uint32_t in_frames);
/* Host: gives every row its tiles (first_tile) and returns the launch's tile count.  A tile is 64 frames of one row, fewer
 * (32, 16) while the tile's frames -- one LDS row of win_length samples each -- exceed the tile's LDS.  Returns 0 with
 * afg_last_error set for params out of range. */
uint64_t afg_mel_layout(afg_mel_row *rows, uint64_t n_rows, const afg_mel_params *params);
/* Host: the checks afg_melspec_hip makes on every record before it launches, on a host copy of the records: params in
 * range; basis_floats and filters_floats at least what afg_mel_basis and the bank need; first_tile and n_tiles as
 * afg_mel_layout gives them; every row's in_frames floats inside [0, in_floats); out_frames <= max_frames; reflect with
 * output only with in_frames > pad; its n_mels * out_frames floats inside [0, out_floats).  AFG_ERR_INVALID with
 * afg_last_error set otherwise. */
int afg_mel_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_mel_params *params, uint64_t in_floats,
                       uint64_t basis_floats, uint64_t filters_floats, uint64_t out_floats);
/* Runs every row in one launch, one workgroup per tile.  d_rows is the device copy of rows laid out by afg_mel_layout,
 * n_tiles what it returned; d_basis is afg_mel_basis's table and d_filters a dense [n_mels, n_bins] bank, both on the
 * device; the planes are 4-byte aligned and do not overlap (d_in may be NULL when no row reads it).  Params are checked
 * first, then every record (the entry fetches d_rows on hip_stream and waits for it) as afg_mel_check_rows does; anything
 * else than a pass is AFG_ERR_INVALID and nothing is written.  The kernel writes exactly n_mels * out_frames floats per
 * record and reads no input float outside the record's row. */
int afg_melspec_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params, const float *d_in,
                    uint64_t in_floats, const float *d_basis, uint64_t basis_floats, const float *d_filters, uint64_t filters_floats,
                    float *d_out, uint64_t out_floats, void *hip_stream);

/* The same features through an FFT per frame: an opt-in algorithm (AFG_MEL_ALGO_FFT) beside the direct product above.  It
 * computes the value defined above -- the same window, centring, padding, frame count, bank, fmaxf floor and output layout,
 * whose float64 statement is basis64, power64 and filters64 of tests/melspec_model.py -- but only the float32 summation
 * order is free, so it is held to an error bound and not to bit patterns.  It does not listen to AFG_NUMERIC or
 * afg_set_numeric_mode.  n_fft: 16 .. 2048 whose prime factors are 2, 3 and 5 only (400, 480, 512, 800, 960, 1024, 2048
 * among them); any other n_fft is AFG_ERR_UNSUPPORTED and the direct path remains for it.
 *
 * Bound.  u = 2^-24; A_f = sum over n of |x_n| w[n] of frame f in float64; B = 8 ceil(log2(n_fft)) + 8.  Then
 * |re - re64| and |im - im64| are at most E_f = B u A_f: a binary level of a Cooley-Tukey factorisation costs a value at
 * most a rounded twiddle, a complex multiply (3 roundings), a butterfly add and the rotation constants of radix 3 and 5 --
 * 8 per level -- and 8 more cover the window multiply, the real / complex split pass and second-order terms.  p and mel are
 * summed in any order, fused or not, over the bank's weights as given (dense, every bin).  For a bank without negative
 * weights, with p_hi = (|re64| + E)^2 + (|im64| + E)^2 and p_lo = max(|re64| - E, 0)^2 + max(|im64| - E, 0)^2, the
 * AFG_MEL_POWER output lies in [(1 - (n_bins + 4) u) sum_k W p_lo, (1 + (n_bins + 4) u) sum_k W p_hi], W the float32 bank
 * taken to float64, and AFG_MEL_LOG10 within 3 ulp of log10 of that interval after the floor.
 * Locality.  A frame's outputs depend on that row's samples under that frame and on the parameters, and on nothing else:
 * the same row gives the same bits wherever it stands, and a NaN sample makes NaN (AFG_MEL_POWER; log10f(floor) with
 * AFG_MEL_LOG10) of every mel of exactly the frames whose window span covers it.  A row without samples under zero padding
 * and padding outside the row give +0.0f power, or log10f(log_floor), as above.
 *
 * afg_mel_fft_tables: host only.  Returns win_length + 2 * n_fft floats and with cap >= that fills the window w[j],
 * j < win_length, then n_fft pairs (cos, -sin) of 2 pi j / n_fft; each computed in double and rounded once to float32.
 * Returns 0 with afg_last_error set for sizes out of range or an n_fft this path does not take.
 * afg_mel_fft_layout, afg_mel_fft_check_rows, afg_melspec_fft_hip: as afg_mel_layout, afg_mel_check_rows and
 * afg_melspec_hip, with the same afg_mel_params and afg_mel_row records and afg_mel_fft_tables' table in place of the
 * basis.  A tile is 16 frames of one row, so a layout made by afg_mel_layout does not serve here.  The same checks are
 * made before the launch; afg_mel_fft_check_rows needs no device.  The kernel writes exactly n_mels * out_frames floats
 * per record and reads no input float outside the record's row. */
#define AFG_MEL_ALGO_DIRECT 0
#define AFG_MEL_ALGO_FFT    1
uint64_t afg_mel_fft_tables(uint32_t n_fft, uint32_t win_length, float *out, uint64_t cap);
uint64_t afg_mel_fft_layout(afg_mel_row *rows, uint64_t n_rows, const afg_mel_params *params);
int afg_mel_fft_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_mel_params *params, uint64_t in_floats,
                           uint64_t table_floats, uint64_t filters_floats, uint64_t out_floats);
int afg_melspec_fft_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params, const float *d_in,
                        uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters, uint64_t filters_floats,
                        float *d_out, uint64_t out_floats, void *hip_stream);

/* The linear-frequency spectrum itself: the short-time Fourier transform afg_melspec_fft_hip computes per frame, delivered
 * instead of multiplied into a bank -- complex for separation and enhancement, magnitude for vocoders, power for a bank of
 * the caller's own.  A stage of its own beside the mel stage, with its own parameters (afg_stft_params); the rows are
 * afg_mel_row records.  The value is the one defined above up to re / im: the periodic Hann window of win_length centred in
 * the frame, center / pad_mode (reflect without edge repeat, or +0.0f), max_frames (afg_mel_frames' formula), and the FFT
 * path's n_fft: 16 .. 2048 with prime factors 2, 3 and 5 only, anything else AFG_ERR_UNSUPPORTED.  Its float64 statement is
 * basis64 / power64 of tests/melspec_model.py; tests/stft_model.py holds the intervals below.  n_bins = n_fft / 2 + 1.
 *
 * Parameters: n_fft as above, win_length 1 .. n_fft, hop 1 .. n_fft, center 0 or 1, pad_mode AFG_MEL_PAD_REFLECT or
 * AFG_MEL_PAD_ZERO, out_kind AFG_STFT_*, log_floor a finite float >= 0 (0 means 1e-10f; read by AFG_STFT_LOG10 only, checked
 * always), reserved 0.  With p = re * re + im * im: AFG_STFT_COMPLEX delivers (re, im), AFG_STFT_MAGNITUDE sqrtf(p),
 * AFG_STFT_POWER p, AFG_STFT_LOG10 log10f(fmaxf(p, log_floor)).
 *
 * Output: record r writes comps * n_bins * out_frames floats at out_off, comps = 2 for AFG_STFT_COMPLEX and 1 otherwise, as
 * [n_bins, out_frames] with frames contiguous (torch.stft's layout): bin k, frame f at out_off + k * out_frames + f, and for
 * AFG_STFT_COMPLEX the pair at out_off + 2 * (k * out_frames + f), re first -- torch.view_as_real of a [n_bins, out_frames]
 * complex64.
 *
 * Bound.  With u, A_f, B and E_f = B u A_f exactly as in the FFT mel path above, and p_hi = (|re64| + E)^2 + (|im64| + E)^2,
 * p_lo = max(|re64| - E, 0)^2 + max(|im64| - E, 0)^2:
 *   AFG_STFT_COMPLEX    |re - re64| <= E_f and |im - im64| <= E_f;
 *   AFG_STFT_POWER      inside [(1 - 4u) p_lo, (1 + 4u) p_hi] (two products and a sum, fused or not);
 *   AFG_STFT_MAGNITUDE  within 2 float32 ulp of the square root of that interval (the hardware square root is specified to
 *                       1 ulp; the second is margin);
 *   AFG_STFT_LOG10      within 3 float32 ulp of log10 of that interval after the floor, the mel path's figure.
 * Locality as above: the same row gives the same bits wherever it stands; a NaN sample makes NaN of every bin of exactly the
 * frames whose window span covers it (AFG_STFT_LOG10: log10f(floor), since fmaxf drops the NaN); padding outside the row and
 * rows without samples give +0.0f under zero padding (AFG_STFT_LOG10: log10f(floor)).  The kernel does not listen to
 * AFG_NUMERIC or afg_set_numeric_mode.
 *
 * The table is afg_mel_fft_tables' (the same window and twiddles).  afg_stft_tile_frames: host only; the frames of one row a
 * workgroup takes for these parameters -- it depends on n_fft and out_kind, because the tile's LDS does -- or 0 with
 * afg_last_error set for parameters out of range.  afg_stft_layout: host only; gives every row its tiles (first_tile) and
 * returns their count, the sum of ceil(out_frames / tile); 0 with afg_last_error set for parameters out of range.  A layout
 * made by afg_mel_layout or afg_mel_fft_layout does not serve.  afg_stft_check_rows: host only, needs no device; the checks
 * afg_stft_hip makes before it launches, on a host copy of the records: parameters in range; table_floats at least
 * win_length + 2 * n_fft; first_tile and n_tiles as afg_stft_layout gives them; every row's in_frames floats inside
 * [0, in_floats); out_frames <= max_frames; reflect with output only with in_frames > pad; the record's comps * n_bins *
 * out_frames floats inside [0, out_floats).  AFG_ERR_UNSUPPORTED for the n_fft, AFG_ERR_INVALID otherwise, afg_last_error set.
 * afg_stft_hip runs every row in one launch, one workgroup per tile; arguments as afg_melspec_fft_hip's without the bank.
 * The same checks come first (the entry fetches d_rows on hip_stream and waits for it); on anything but a pass nothing is
 * written.  The kernel writes exactly the record's floats and reads no input float outside the record's row. */
#define AFG_STFT_COMPLEX   0   /* (re, im) pairs */
#define AFG_STFT_MAGNITUDE 1   /* sqrtf(p) */
#define AFG_STFT_POWER     2   /* p = re*re + im*im */
#define AFG_STFT_LOG10     3   /* log10f(fmaxf(p, log_floor)), log_floor 0 means 1e-10f */
typedef struct afg_stft_params {   /* 32 bytes */
    uint32_t n_fft, win_length, hop, center, pad_mode, out_kind;
    float    log_floor;
    uint32_t reserved;             /* 0 */
} afg_stft_params;
uint32_t afg_stft_tile_frames(const afg_stft_params *params);
uint64_t afg_stft_layout(afg_mel_row *rows, uint64_t n_rows, const afg_stft_params *params);
int afg_stft_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_stft_params *params, uint64_t in_floats,
                        uint64_t table_floats, uint64_t out_floats);
int afg_stft_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_stft_params *params, const float *d_in,
                 uint64_t in_floats, const float *d_table, uint64_t table_floats, float *d_out, uint64_t out_floats, void *hip_stream);

/* afg_batch_decode_resampled followed by afg_stft_hip: d_out is n_files * channels * n_bins * n_out floats on the current
 * device (twice that for AFG_STFT_COMPLEX), and slab [i, k] is the definition above applied to row [i, k] of the tensor
 * afg_batch_decode_resampled makes of the same list with the leading fields of the options.  In every other respect it is
 * afg_batch_decode_mel (below): n_out == 0 means max_frames of T, the scratch is pooled under
 * afg_dev_option("mel_scratch_bytes") with sublists of at least one file, the table is made once per (n_fft, win_length) and
 * kept, a file that failed or was refused keeps its status and message and gets the all-zero row's slab, items[i].pcm points
 * at the file's slab (NULL when it failed or was refused), n_files == 0 is AFG_OK and touches nothing.  Checked before any
 * device call, afg_last_error set: everything afg_batch_decode_resampled checks, a struct_size below sizeof(afg_stft_opts),
 * a non-zero `reserved`, the parameters (AFG_ERR_UNSUPPORTED for the n_fft), T without a frame, n_out above max_frames,
 * reflect with T <= pad. */
typedef struct afg_stft_opts {
    uint32_t        struct_size;   /* sizeof(afg_stft_opts) */
    int             n_threads;     /* from here to lowpass_width: as afg_resample_opts */
    uint32_t        channels;
    uint32_t        frames;        /* T, samples at `samplerate` */
    const int64_t  *first_frame;
    uint32_t        samplerate;
    uint32_t        mono;
    uint32_t        in_channels;
    uint32_t        max_in_rate;
    uint32_t        lowpass_width;
    uint32_t        n_out;         /* frames per bin row; 0 means max_frames of T */
    afg_stft_params stft;
    uint32_t        reserved;      /* 0 */
} afg_stft_opts;
int afg_batch_decode_stft(const uint8_t *const *data, const size_t *length, int n_files, const afg_stft_opts *opts, float *d_out,
                          afg_batch_result *out);

/* afg_batch_decode_resampled followed by afg_melspec_hip: d_out is n_files * channels * n_mels * n_out floats on the
 * current device, and slab [i, k] is the definition above applied to row [i, k] of the tensor afg_batch_decode_resampled
 * makes of the same list with the leading fields of the options (frames is T, in samples at `samplerate`).  n_out == 0
 * means max_frames of T; otherwise n_out <= max_frames (Whisper takes 3000 of 3001), and reflect needs T > pad.  The tensor
 * is a pooled scratch [files, channels, T]; a list whose scratch would exceed afg_dev_option("mel_scratch_bytes") (default
 * 2 GiB) runs in sublists of at least one file.  The basis and the bank (afg_mel_filters of samplerate, n_fft, n_mels,
 * f_min, f_max, scale, norm) are made once per parameter set and kept.  A file that failed or was refused upstream keeps
 * its status and message, and its slab is what an all-zero row gives: +0.0f, or log10f(log_floor).  items[i] is as in
 * afg_batch_decode_resampled; pcm points at the file's mel slab (NULL when the file failed or was refused).
 * Checked before any device call, AFG_ERR_INVALID with afg_last_error set: everything afg_batch_decode_resampled checks, a
 * struct_size below sizeof(afg_mel_opts), the mel parameters and the bank's arguments out of range, T without a frame,
 * n_out above max_frames, reflect with T <= pad, an unknown algorithm, a non-zero `reserved`; AFG_ERR_UNSUPPORTED for
 * AFG_MEL_ALGO_FFT with an n_fft that path does not take.  n_files == 0 is AFG_OK and touches nothing.
 * algorithm: AFG_MEL_ALGO_DIRECT (0) is afg_melspec_hip; AFG_MEL_ALGO_FFT runs afg_melspec_fft_hip in its place, its table
 * kept per parameter set like the basis; everything around the kernel is the same. */
typedef struct afg_mel_opts {
    uint32_t       struct_size;   /* sizeof(afg_mel_opts) */
    int            n_threads;     /* from here to lowpass_width: as afg_resample_opts */
    uint32_t       channels;
    uint32_t       frames;        /* T, samples at `samplerate` */
    const int64_t *first_frame;
    uint32_t       samplerate;
    uint32_t       mono;
    uint32_t       in_channels;
    uint32_t       max_in_rate;
    uint32_t       lowpass_width;
    uint32_t       n_out;         /* frames per mel row; 0 means max_frames of T */
    afg_mel_params mel;
    uint32_t       scale;         /* AFG_MEL_SCALE_* */
    uint32_t       norm;          /* AFG_MEL_NORM_* */
    double         f_min;         /* Hz */
    double         f_max;         /* Hz; 0 means samplerate / 2 */
    uint32_t       algorithm;     /* AFG_MEL_ALGO_* */
    uint32_t       reserved;      /* 0 */
} afg_mel_opts;
int afg_batch_decode_mel(const uint8_t *const *data, const size_t *length, int n_files, const afg_mel_opts *opts, float *d_out,
                         afg_batch_result *out);

/* ---- normalisation: statistics per group of rows, and the gain / offset they decide ------------------------------------
 * The last step in front of a model: peak or RMS gain of a waveform, zero mean and unit variance per utterance over its
 * own samples (wav2vec2, HuBERT, WavLM), Whisper's dynamic range of a log-mel slab.  The reference has no such stage; the
 * definition is this library's own, restated in numpy in tests/normalize_model.py, and the device follows it bit for bit.
 *
 * Groups.  A group (afg_norm_group) is what one set of statistics covers: rows 1 .. 65535; row r starts at float
 * in_off + r * stride of d_in and out_off + r * stride of d_out; only the first `valid` floats of a row count and are
 * touched.  One file's channel rows are one group; one mel slab is one group of a single row.  valid == 0: nothing is read,
 * nothing written, and the statistics record is all zero.
 *
 * Tiles.  A tile is 4096 consecutive floats of one row, counted from the row's element 0; a row's last tile may be short.
 * Tiles are numbered rows ascending, then tiles ascending inside a row; a group's tiles follow those of the group before.
 *
 * Statistics, in a fixed order, without atomics, sums in float64.  Element e of a tile belongs to lane (e / 4) % 256 of
 * 256 lanes.  A lane starts from s = q = +0.0 and over its elements in ascending e does s = s + (double)x and
 * q = q + (double)x * (double)x (the product is exact, only the adds round).  Lanes combine in a binary tree: step
 * d = 1, 2, 4 .. 128, lane l with l % (2 d) == 0 takes v[l] = v[l] + v[l + d].  A group's tile results combine one after
 * the other in tile order, starting from +0.0.  min and max are those of the samples that are no NaN, with -0 below +0
 * (+inf and -inf when there is none); a NaN sample propagates through the sums.  count = rows * valid.
 *
 * Modes.  The mode gives offset and scale (float32), which go into the record; every valid element then becomes
 * y = (x - offset) * scale: the float32 subtraction rounded, then the float32 product, no fused multiply-add.
 *   AFG_NORM_NONE           statistics only (offset 0, scale 1); d_out is not used and may be NULL
 *   AFG_NORM_PEAK           p = fmaxf(-min, max); offset 0, scale = target / p (float32 division), 1 when p is 0 or not finite
 *   AFG_NORM_RMS            r = (float)sqrt(sumsq / count); offset 0, scale = target / r, 1 when r is 0 or not finite
 *   AFG_NORM_STANDARD       in double: mean = sum / count, var = fmax(sumsq / count - mean * mean, 0) (a NaN gives 0);
 *                           offset = (float)mean, scale = (float)(1.0 / sqrt(var + (double)eps)); eps 0 means 1e-7f
 *   AFG_NORM_DYNAMIC_RANGE  y = ((x > offset ? x : offset) + shift) * gain with offset = max - range (a NaN sample takes
 *                           the floor); scale = gain.  Whisper: range 8, shift 4, gain 0.25
 * A NaN in sum, sumsq, offset, scale or the output is always the positive quiet NaN (0x7fc00000, 0x7ff8000000000000):
 * which NaN an operation returns is the hardware's affair, and the definition leaves none of that in its results.
 * The fields a mode uses must be finite; target, range and gain positive, eps at least 0.  The others are ignored.
 * In place (d_out == d_in, out_off == in_off) is allowed; other overlaps of what a launch reads and writes are not.  No
 * float outside the valid elements of a group is read or written. */
#define AFG_NORM_NONE          0
#define AFG_NORM_PEAK          1
#define AFG_NORM_RMS           2
#define AFG_NORM_STANDARD      3
#define AFG_NORM_DYNAMIC_RANGE 4
typedef struct afg_norm_group {   /* 48 bytes */
    uint64_t in_off, out_off;     /* float index of row 0, element 0 in d_in / d_out */
    uint64_t stride;              /* floats from one row to the next, in both planes; >= valid when rows > 1 */
    uint64_t first_tile;          /* filled in by afg_norm_layout */
    uint32_t rows, valid;
    uint32_t reserved[2];
} afg_norm_group;
typedef struct afg_norm_stats {   /* 40 bytes, one per group */
    double sum, sumsq; uint64_t count; float min, max, offset, scale;
} afg_norm_stats;
typedef struct afg_norm_params { uint32_t mode; float target, eps, range, shift, gain; } afg_norm_params;
/* Host: fills first_tile of every group, returns the launch's tile count. */
uint64_t afg_norm_layout(afg_norm_group *groups, uint64_t n_groups);
/* Host only, no device: the checks afg_normalize_hip makes before it launches, on a host copy of the groups: the mode known
 * and its parameters in range; rows 1 .. 65535; first_tile and n_tiles as afg_norm_layout gives them; and for a group with
 * valid > 0: stride >= valid when rows > 1, its rows inside [0, in_floats) and -- unless the mode is AFG_NORM_NONE -- inside
 * [0, out_floats).  AFG_ERR_INVALID with afg_last_error set otherwise.  n_groups == 0 checks the parameters alone. */
int afg_norm_check_groups(const afg_norm_group *groups, uint64_t n_groups, uint64_t n_tiles, const afg_norm_params *params,
                          uint64_t in_floats, uint64_t out_floats);
/* Three launches on hip_stream: the tiles' partial sums into d_partials (n_tiles * 32 bytes, 8-byte aligned), the groups'
 * records into d_stats (n_groups of them), and the apply pass.  d_groups is the device copy of groups laid out by
 * afg_norm_layout; the entry fetches it on hip_stream, waits for it and checks every group as afg_norm_check_groups does:
 * anything else than a pass is AFG_ERR_INVALID and nothing is written. */
int afg_normalize_hip(uint64_t n_groups, const afg_norm_group *d_groups, uint64_t n_tiles, const afg_norm_params *params,
                      const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, void *d_partials,
                      afg_norm_stats *d_stats, void *hip_stream);

/* afg_batch_decode_resampled, then one group per file, in place: rows = min(channels, the file's channels), or 1 with
 * mono; with g = gcd(file rate, samplerate), M = file rate / g and L = samplerate / g,
 * valid = min(T, ceil((frames - first_frame) * L / M)), 0 when that is not positive: the samples whose place lies inside
 * the file.  What lies behind them, and the rows a file has no channel for, stay as afg_batch_decode_resampled leaves them.  A
 * failed or refused file is a group with valid == 0: a zero slab, a zero record.  d_stats (device, n_files records) may be
 * NULL.  Checked before any device call: everything afg_batch_decode_resampled checks, and NULL or out-of-range norm.
 * Statuses, messages and items[i] are afg_batch_decode_resampled's. */
int afg_batch_decode_resampled_norm(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                                    const afg_norm_params *norm, float *d_out, afg_norm_stats *d_stats, afg_batch_result *out);
/* afg_batch_decode_mel with wave_norm (NULL: none) applied to the pooled [files, channels, T] tensor in front of the mel
 * launch, in the groups of afg_batch_decode_resampled_norm, and feat_norm (NULL: none) applied to every [i, k] slab as one
 * group of n_mels * n_out floats, all of them valid.  A failed file's slab is what the definition gives for the all-floor
 * slab.  Checked before any device call: everything afg_batch_decode_mel checks, and norm parameters out of range. */
int afg_batch_decode_mel_norm(const uint8_t *const *data, const size_t *length, int n_files, const afg_mel_opts *opts,
                              const afg_norm_params *wave_norm, const afg_norm_params *feat_norm, float *d_out, afg_batch_result *out);

/* ---- cepstral features behind the log-mel stage: a DCT-II over the mel axis, a lifter, and regression deltas -------------
 * What speaker and keyword models and Kaldi-style recipes take: MFCC statics with their first and second time derivatives
 * stacked behind them (torchaudio.transforms.MFCC and ComputeDeltas), in one kernel.  The reference has no such stage; the
 * definition is this library's own, restated in numpy in tests/cepstra_model.py, and the device follows it bit for bit.
 *
 * Parameters of a call (afg_cep_params), uniform over its records: n_mels 1 .. 256 (rows of an input slab), n_ceps
 * 1 .. n_mels, delta_order 0, 1 or 2 (planes behind the statics), delta_win N 1 .. 8 (ignored when delta_order is 0;
 * torchaudio's win_length 5 is N = 2), reserved words 0.  Anything else is AFG_ERR_INVALID.
 *
 * A record (afg_cep_row) is one slab [n_mels, F] of d_in, frames contiguous, mel 0 frame 0 at float in_off, and its output
 * [(1 + delta_order) * n_ceps, F] float32: plane p, coefficient q, frame t lies at out_off + (p * n_ceps + q) * F + t.  The
 * planes are p = 0 statics, 1 delta, 2 delta-delta.  frames == 0: nothing is read, nothing written.
 *
 * Arithmetic.  Every operation is float32 and nothing wider; every sum starts from +0.0f and runs in ascending index
 * order, one fmaf per term.  D is the caller's dense [n_ceps, n_mels] matrix (afg_cep_dct makes the usual ones).
 *   c[q][t]  = chain over m = 0 .. n_mels - 1 of fmaf(D[q][m], x[m][t], acc)
 *   d1[q][t] = (chain over n = 1 .. N of fmaf((float)n, c[q][min(t + n, F - 1)] - c[q][max(t - n, 0)], acc)) * g
 * with the difference rounded to float32, the final product rounded to float32, and g = float32(1 / (2 * sum n^2)) computed
 * in double.  d2 is the same expression over d1 taken at the clamped frame indices: the delta of the edge-replicated delta
 * sequence, which is what ComputeDeltas(mode="replicate") applied twice computes.  (librosa.feature.delta fits a
 * Savitzky-Golay polynomial and treats the edges differently: a different definition, not provided here.)
 *
 * Locality.  A record's outputs depend on that record's slab and the parameters only; the same slab gives the same bits
 * wherever it stands.  A NaN at input frame t makes NaN of every static of frame t; of the deltas of exactly the frames t'
 * whose clamped span reads it -- some min(t' + n, F - 1) or max(t' - n, 0), n = 1 .. N, is t: the frames within N of t, and t
 * itself only where the clamp lands on it (t = 0, t = F - 1); of the delta-deltas of exactly the frames whose span reads one
 * of those; and of nothing else.  No float outside a record's n_mels * F inputs is read, and exactly
 * (1 + delta_order) * n_ceps * F floats are written.
 *
 * afg_cep_dct: host only.  Returns n_ceps * n_mels and with cap >= that fills out[q * n_mels + m] = D[q][m] (out may be NULL
 * with cap 0):  D[q][m] = float32(log_scale * L[q] * s[q] * cos(pi * r / (2 * n_mels))),  r = (q * (2 m + 1)) mod (4 * n_mels)
 * reduced in integers before the cosine, all of it in double and rounded once.  AFG_CEP_DCT_ORTHO: s[0] = sqrt(1 / n_mels),
 * s[q] = sqrt(2 / n_mels) otherwise; AFG_CEP_DCT_NONE: s = 2 (scipy's and torchaudio's unnormalised type II).  lifter 0:
 * L = 1; lifter > 0: L[q] = 1 + (lifter / 2) * sin(pi * q / lifter) with q counted from 0, the HTK / Kaldi convention
 * (librosa counts q from 1).  log_scale is finite and not 0: 1 keeps the log10 units of the mel stage, 10 gives dB of power,
 * ln 10 natural-log cepstra.  Returns 0 with afg_last_error set for n_mels, n_ceps or norm out of range, a lifter that is
 * negative or not finite, or such a log_scale.
 *
 * afg_cep_layout, afg_cep_check_rows, afg_cepstra_hip: as afg_mel_layout, afg_mel_check_rows and afg_melspec_hip.  A tile is
 * 64 consecutive frames of one record (AFG_CEP_TILE); a record's last tile may be short.  The layout fills first_tile and
 * returns the launch's tile count (0 with afg_last_error set for params out of range).  The check function needs no device:
 * params in range; dct_floats at least n_ceps * n_mels; first_tile and n_tiles as the layout gives them; reserved words 0;
 * and for a record with frames > 0 its n_mels * F floats inside [0, in_floats) and its (1 + delta_order) * n_ceps * F floats
 * inside [0, out_floats); n_rows == 0 checks the parameters alone.  The entry runs every record in one launch, one
 * workgroup per tile: d_rows is the device copy of the laid-out records, which the entry fetches on hip_stream, waits for
 * and checks in the same way; anything else than a pass is AFG_ERR_INVALID and nothing is written.  The planes are 4-byte
 * aligned, offsets may be odd, and d_in and d_out do not overlap. */
#define AFG_CEP_DCT_NONE  0
#define AFG_CEP_DCT_ORTHO 1
#define AFG_CEP_TILE      64
typedef struct afg_cep_params {   /* 32 bytes */
    uint32_t n_mels;       /* 1 .. 256: rows of an input slab */
    uint32_t n_ceps;       /* 1 .. n_mels */
    uint32_t delta_order;  /* 0, 1 or 2: planes behind the statics */
    uint32_t delta_win;    /* N, 1 .. 8 (ignored when delta_order is 0); torchaudio's win_length 5 is N = 2 */
    uint32_t reserved[4];  /* 0 */
} afg_cep_params;
typedef struct afg_cep_row {      /* 32 bytes */
    uint64_t in_off;       /* float index in d_in of mel 0, frame 0; the slab is [n_mels, frames], frames contiguous */
    uint64_t out_off;      /* float index in d_out of plane 0, coefficient 0, frame 0 */
    uint64_t first_tile;   /* filled in by afg_cep_layout */
    uint32_t frames;       /* F; 0: nothing read, nothing written */
    uint32_t reserved;     /* 0 */
} afg_cep_row;
uint64_t afg_cep_dct(uint32_t n_ceps, uint32_t n_mels, uint32_t norm, double lifter, double log_scale, float *out, uint64_t cap);
uint64_t afg_cep_layout(afg_cep_row *rows, uint64_t n_rows, const afg_cep_params *params);
int afg_cep_check_rows(const afg_cep_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_cep_params *params, uint64_t in_floats,
                       uint64_t dct_floats, uint64_t out_floats);
int afg_cepstra_hip(uint64_t n_rows, const afg_cep_row *d_rows, uint64_t n_tiles, const afg_cep_params *params, const float *d_in,
                    uint64_t in_floats, const float *d_dct, uint64_t dct_floats, float *d_out, uint64_t out_floats, void *hip_stream);

/* afg_batch_decode_mel_norm(..., wave_norm, NULL, ...) followed by afg_cepstra_hip: d_out is n_files * channels *
 * (1 + delta_order) * n_ceps * n_out floats on the current device, and slab [i, k] is the definition above applied to slab
 * [i, k] of the log-mel tensor that call makes of the same list (either algorithm), with D = afg_cep_dct(cep.n_ceps,
 * cep.n_mels, dct_norm, lifter, log_scale); log_scale 0 means 1.  The log-mel tensor is a pooled scratch; a list whose scratch
 * would exceed afg_dev_option("mel_scratch_bytes") runs in sublists of at least one file, one afg_cepstra_hip launch each.
 * The table is made once per parameter set and kept, like the bank.  cmvn (NULL: none): every one of the
 * (1 + delta_order) * n_ceps rows of every slab is one afg_norm_group of a single row with valid = n_out, normalised in
 * place -- with AFG_NORM_STANDARD, per-coefficient mean and variance normalisation over time; the other modes work too.
 * A failed or refused file keeps its status and message, and its slab is what the definition gives for the all-floor mel
 * slab.  items[i] is as in afg_batch_decode_mel, with pcm at the file's slab.
 * Checked before any device call, AFG_ERR_INVALID with afg_last_error set: everything afg_batch_decode_mel_norm checks, a
 * struct_size below sizeof(afg_mfcc_opts), mel.mel.out_kind other than AFG_MEL_LOG10, cep.n_mels other than mel.mel.n_mels,
 * the cepstral parameters, dct_norm, lifter and log_scale out of range, cmvn parameters out of range.  n_files == 0 is AFG_OK
 * and touches nothing. */
typedef struct afg_mfcc_opts {
    uint32_t       struct_size;   /* sizeof(afg_mfcc_opts) */
    uint32_t       dct_norm;      /* AFG_CEP_DCT_* */
    afg_mel_opts   mel;           /* as for afg_batch_decode_mel; mel.mel.out_kind must be AFG_MEL_LOG10 */
    afg_cep_params cep;           /* cep.n_mels must equal mel.mel.n_mels */
    double         lifter, log_scale;   /* log_scale 0 means 1 */
} afg_mfcc_opts;
int afg_batch_decode_mfcc(const uint8_t *const *data, const size_t *length, int n_files, const afg_mfcc_opts *opts,
                          const afg_norm_params *wave_norm, const afg_norm_params *cmvn, float *d_out, afg_batch_result *out);

/* ---- trimming silence: the non-silent region of a group of rows, and the rows shifted to start there ----------------------
 * What librosa.effects.trim and the non-silent region operators of loaders do, behind the collate on planar rows, so that a
 * clip of a fixed length starts where the sound starts.  The reference has no such stage; the definition is this library's
 * own, restated in numpy in tests/trim_model.py, and the device follows it bit for bit.
 *
 * Parameters (afg_trim_params), uniform over a call: hop >= 1, frame_length a multiple of hop and at most 65536,
 * k = frame_length / hop 1 or an even number up to 64; reference AFG_TRIM_REF_MAX or AFG_TRIM_REF_ABS; ratio finite and above
 * 0, at most 1 with AFG_TRIM_REF_MAX (a power ratio: 10 ^ (-top_db / 10) -- the library never sees decibels); abs_power finite
 * and above 0 with AFG_TRIM_REF_ABS, ignored otherwise; lead and trail: samples kept in front of and behind the region;
 * reserved words 0.  Anything else is AFG_ERR_INVALID.
 *
 * Groups.  A group (afg_trim_group) is `rows` input rows (1 .. 65535) of `valid` floats, row r at float in_off + r * in_stride
 * of d_in -- one file's channel rows -- and out_rows >= rows output rows of out_frames floats, row r at out_off + r * out_stride
 * of d_out.
 *
 * Blocks.  Block j of a group is samples [j * hop, min((j + 1) * hop, valid)) of every row; n_blocks = ceil(valid / hop).  Its
 * power S_j is a float64 in a fixed order: in row r, sample i of the block (counted from the block's start) belongs to lane
 * i % 64 of 64 lanes; a lane starts from +0.0 and over its samples in ascending i does q = q + (double)x * (double)x (the
 * product is exact); the lanes combine in the tree of the normalisation stage -- step d = 1, 2 .. 32, lane l with
 * l % (2 d) == 0 takes v[l] + v[l + d]; the rows' results are added in ascending r, starting from +0.0.
 *
 * Frames.  There are n_blocks analysis frames; frame f covers blocks [f - k / 2, f + k / 2) cut to [0, n_blocks) -- the frame of
 * frame_length samples centred on sample f * hop -- and for k == 1 block f alone.  P_f is the sum of the frame's S_j in
 * ascending j from +0.0.  P_ref = max over f of P_f, taken as P > m ? P : m from +0.0: a NaN never wins.  The threshold is
 * ratio * P_ref with AFG_TRIM_REF_MAX and ratio * abs_power * (double)(rows * frame_length) -- two products in that order --
 * with AFG_TRIM_REF_ABS (abs_power is a mean square per sample).  A frame is non-silent when P_f > threshold; a NaN is silent.
 *
 * Region (afg_trim_region).  No non-silent frame: begin = end = 0.  Otherwise, with f_first and f_last the first and last
 * non-silent frame, b = f_first * hop, e = min(valid, (f_last + 1) * hop) -- librosa.effects.trim's index arithmetic -- and
 * begin = b > lead ? b - lead : 0, end = min(valid, e + trail).  ref_power is P_ref in both modes.
 *
 * Output.  For r < rows and t < min(out_frames, end - begin), out[r][t] has the bits of in[r][begin + t]; every other element
 * of the out_rows x out_frames slab is +0.0f.  Every element of the slab is written; no float outside [0, valid) of the input
 * rows is read; the output may not overlap the input.  valid == 0: a zero slab and a zero record.
 *
 * afg_trim_layout fills first_block (blocks are numbered through the groups in order) and first_tile (a tile is 4096
 * consecutive floats of one output row, rows ascending, then tiles ascending inside a row) and stores the two counts; it
 * returns 1, or 0 with afg_last_error set for parameters out of range or a NULL pointer.  afg_trim_check_groups needs no
 * device: the parameters in range; rows 1 .. 65535 and out_rows >= rows; with more than one row a stride at least the row
 * (in_stride >= valid, out_stride >= out_frames); the rows inside [0, in_floats) and [0, out_floats), offsets that would wrap
 * included; first_block, first_tile and the counts as the layout gives them.  n_groups == 0 checks the parameters alone.
 * afg_trim_hip runs three launches on hip_stream -- the blocks' powers into d_blocks (n_blocks doubles), the regions into
 * d_regions (n_groups records), the shifted copy -- without atomics and without a host round trip between them.  d_groups is
 * the device copy of the laid-out groups; the entry fetches it on hip_stream, waits for it and checks it in the same way,
 * and refuses planes that overlap (from the pointers and the float counts): anything else than a pass is AFG_ERR_INVALID
 * and nothing is written.  The planes are 4-byte aligned, d_blocks, d_regions and d_groups 8-byte aligned. */
#define AFG_TRIM_REF_MAX 0
#define AFG_TRIM_REF_ABS 1
typedef struct afg_trim_params {  /* 48 bytes */
    uint32_t frame_length, hop;   /* samples; frame_length = k * hop */
    uint32_t reference;           /* AFG_TRIM_REF_* */
    uint32_t lead, trail;         /* samples kept in front of / behind the non-silent region */
    uint32_t reserved[3];         /* 0 */
    double   ratio;               /* threshold over the reference, as a power ratio */
    double   abs_power;           /* AFG_TRIM_REF_ABS: the reference, a mean square per sample */
} afg_trim_params;
typedef struct afg_trim_group {   /* 64 bytes */
    uint64_t in_off, out_off;     /* float index of row 0, element 0 in d_in / d_out */
    uint64_t in_stride, out_stride;   /* floats from one row to the next */
    uint64_t first_block, first_tile; /* filled in by afg_trim_layout */
    uint32_t rows, valid;         /* input rows and their length */
    uint32_t out_rows, out_frames;    /* the output slab; out_rows >= rows */
} afg_trim_group;
typedef struct afg_trim_region {  /* 16 bytes, one per group */
    uint32_t begin, end;          /* out[r][t] = in[r][begin + t] for t < min(out_frames, end - begin) */
    double   ref_power;           /* P_ref */
} afg_trim_region;
int afg_trim_layout(afg_trim_group *groups, uint64_t n_groups, const afg_trim_params *params, uint64_t *n_blocks, uint64_t *n_tiles);
int afg_trim_check_groups(const afg_trim_group *groups, uint64_t n_groups, uint64_t n_blocks, uint64_t n_tiles,
                          const afg_trim_params *params, uint64_t in_floats, uint64_t out_floats);
int afg_trim_hip(uint64_t n_groups, const afg_trim_group *d_groups, uint64_t n_blocks, uint64_t n_tiles, const afg_trim_params *params,
                 const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_blocks, afg_trim_region *d_regions,
                 void *hip_stream);

/* afg_batch_decode_resampled with frames = scan_frames into a pooled scratch [files, channels, scan_frames], then one group
 * per file as afg_batch_decode_resampled_norm makes them -- rows = min(channels, the file's channels), or 1 with mono; valid
 * as defined there with T = scan_frames, 0 for a failed or refused file; out_rows = channels -- trimmed into d_out, which is
 * n_files * channels * opts->frames floats on the current device.  scan_frames >= opts->frames says how many frames at the
 * target rate are decoded and examined, counted from first_frame; 0 means opts->frames.  A list whose scratch would exceed
 * afg_dev_option("trim_scratch_bytes") (default 2 GiB) runs in sublists of at least one file, one afg_trim_hip launch each.
 * regions (host, n_files records) may be NULL; it is filled when the call's last launch has drained.  Checked before any
 * device call, AFG_ERR_INVALID with afg_last_error set: everything afg_batch_decode_resampled checks, NULL opts, trim, d_out or
 * out, scan_frames below opts->frames, the trim parameters.  Statuses, messages and items[i] are afg_batch_decode_resampled's. */
int afg_batch_decode_trimmed(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                             const afg_trim_params *trim, uint32_t scan_frames, float *d_out, afg_trim_region *regions,
                             afg_batch_result *out);

/* ---- filtering: cascades of second-order recursive sections over float rows ------------------------------------------------
 * A rumble or DC high-pass in front of trim and normalisation, pre-emphasis in front of the spectral features, band limiting
 * and equalisers, behind the collate on planar rows.  The reference has no such stage; the definition is this library's
 * own, restated in numpy in tests/filter_model.py.
 *
 * Parameters (afg_filter_params), uniform over a call's rows: n_sections 1 .. 8 sections (afg_biquad) b0, b1, b2, a1, a2
 * with a0 normalised to 1.  Section s maps its input u to
 *     v[n] = b0 u[n] + b1 u[n-1] + b2 u[n-2] - a1 v[n-1] - a2 v[n-2]
 * over the real numbers -- scipy.signal.sosfilt's definition.  Everything in front of a row's first sample is zero unless
 * a state is passed in (below).  The sections run in order: the first reads the row's float32 samples, the last is rounded
 * once to float32.  A section is refused (AFG_ERR_INVALID) unless its five numbers are finite and its poles lie strictly
 * inside the unit circle: |a2| < 1 and |a1| < 1 + a2.  a1 == a2 == 0 is a plain FIR section.
 *
 * The device computes in float64, in chunks (below); the chunking is not part of the definition.  The contract is an
 * interval round the exact result y^ of the definition:
 *     |y - y^| <= ulp32(|y^| + K E) / 2 + K E,        ulp32 never below 2^-149,
 *     E = 2^-53 * max|x| * sum over s of |g_s|_1 * (beta_s * P_(s-1) + alpha_s * P_s) * product over t > s of |h_t|_1
 * with g_s the impulse response of 1 / A_s, h_s that of the whole section, |.|_1 the sum of magnitudes,
 * beta = |b0| + |b1| + |b2|, alpha = |a1| + |a2|, P_s = product over t <= s of |h_t|_1 and P_0 = 1: one rounding unit on
 * every term of every section's recurrence, carried by the rest of the cascade.  afg_filter_bound returns E / max|x|: host
 * only, it sums the impulse responses in double until what is left of them -- bounded through the pole radius r by
 * (n + 1) r^n -- is below 2^-60 of the sum.  It returns 0 with afg_last_error set for a refused cascade, for one whose
 * responses have not decayed after 2^28 samples, and for one whose bound exceeds 2^30; such a cascade is refused by every
 * entry below as well.
 *
 * K = AFG_FILTER_K = 64, from the operations an output passes through in the evaluation of csrc/filter.hip, every fused
 * multiply-add counted as one rounding on each of its terms: the zero-state run of a chunk, 5 (three for the b terms, two
 * for the a terms, as a sequential evaluation has them); the carry correction, 3 (two products, the sum onto the run); the
 * state a lane's carry is made of, 3 for each of the 6 steps of the scan inside a wavefront, of the 3 steps across the four
 * wavefronts and of the product with the lane's power of the chunk matrix, 30 in all, and 1 for the tables (rounded once
 * from long double); the previous section's state standing in for its output at a wavefront's first lane, 1; and the
 * model's own long-double recurrence, below 1.  That is 41, taken to the next power of two.  (A count to first order, as
 * E is: inside a chunk of 16 the zero-state run may exceed the true signal, by at most the 16-sample partial sum of |g_s|.)
 *
 * From a row's first non-finite input sample onward that row's outputs and outgoing state are unspecified; everything in
 * front of it, every other row and every float outside the rows keep the contract.
 *
 * afg_biquad_design: host only, in double.  With w = 2 pi f0 / samplerate, c = cos w, alpha = sin w / (2 q) and
 * A = 10^(gain_db / 40), the Audio EQ Cookbook's (R. Bristow-Johnson) sections, every coefficient divided by a0:
 *   LOWPASS    b = ((1-c)/2, 1-c, (1-c)/2)              a = (1+alpha, -2c, 1-alpha)
 *   HIGHPASS   b = ((1+c)/2, -(1+c), (1+c)/2)           a likewise
 *   BANDPASS   b = (alpha, 0, -alpha)                   a likewise        (constant 0 dB peak gain)
 *   NOTCH      b = (1, -2c, 1)                          a likewise
 *   ALLPASS    b = (1-alpha, -2c, 1+alpha)              a likewise
 *   PEAKING    b = (1+alpha A, -2c, 1-alpha A)          a = (1+alpha/A, -2c, 1-alpha/A)
 *   LOWSHELF   with S = 2 sqrt(A) alpha:
 *              b = (A((A+1)-(A-1)c+S), 2A((A-1)-(A+1)c), A((A+1)-(A-1)c-S))    a = ((A+1)+(A-1)c+S, -2((A-1)+(A+1)c), (A+1)+(A-1)c-S)
 *   HIGHSHELF  b = (A((A+1)+(A-1)c+S), -2A((A-1)+(A+1)c), A((A+1)+(A-1)c-S))   a = ((A+1)-(A-1)c+S, 2((A-1)-(A+1)c), (A+1)-(A-1)c-S)
 *   PREEMPHASIS  b = (1, -f0, 0), a1 = a2 = 0: the coefficient (0.97, say) stands in the f0 argument; |f0| <= 1
 *   DC_BLOCK     b = (1, -1, 0), a1 = -r, a2 = 0 with r = exp(-2 pi f0 / samplerate): a zero at z = 1 and a pole at r
 * samplerate, q and gain_db are not looked at by PREEMPHASIS; q and gain_db not by DC_BLOCK; gain_db by the shelves and
 * PEAKING only.  AFG_ERR_INVALID with a message and *out untouched: an unknown kind, NULL out, an argument that is looked at
 * and not finite, samplerate <= 0, f0 outside (0, samplerate / 2), q <= 0, a pre-emphasis coefficient above 1 in size.
 *
 * Rows.  A row (afg_filter_row) is `frames` floats at in_off of d_in, filtered into `frames` floats at out_off of d_out;
 * frames == 0 reads and writes nothing.  d_in == d_out with in_off == out_off is in place; any other overlap -- of one
 * row's output with another's, of a row's output with any row's input, or of the two planes when they are not the same
 * pointer -- is refused.  afg_filter_check_rows needs no device (same_plane says whether d_in == d_out): the parameters as
 * above, the bound included; every row inside [0, in_floats) and [0, out_floats), offsets that would wrap included;
 * reserved 0; the overlaps.  n_rows == 0 checks the parameters alone.
 *
 * State.  d_state is NULL or n_rows * n_sections * 4 doubles, 8-byte aligned: for row i and section s the four at
 * (i * n_sections + s) * 4 are u[n-1], u[n-2], v[n-1], v[n-2] of the section, unrounded -- read as the row's history in
 * front of frame 0, overwritten with the history behind the last frame, untouched for frames == 0.  A row filtered in
 * pieces through its state meets the interval of the whole row.
 *
 * afg_filter_hip is one launch on hip_stream, one workgroup of 256 lanes per row, without atomics or waiting between
 * workgroups: the row is walked in tiles of AFG_FILTER_TILE = 4096 frames (afg_filter_tile_frames returns it), every lane
 * takes a chunk of AFG_FILTER_CHUNK = 16 consecutive frames, runs each section over it from zero state in float64, and
 * the chunks' end states meet in a scan of the map s -> A^16 s + e over the workgroup, the tile's outgoing state carried
 * to the next.  d_rows is the device copy of the rows; the entry fetches it on hip_stream, waits for it and checks it as
 * afg_filter_check_rows does: anything but a pass is AFG_ERR_INVALID and nothing is written.  Exactly `frames` floats are
 * written per row.  The planes are 4-byte aligned, d_rows and d_state 8-byte aligned; at most 2^31 - 1 rows a launch.  The
 * tables of a cascade (16 KiB at the most) are kept on the device per distinct parameters. */
#define AFG_FILTER_MAX_SECTIONS 8
#define AFG_FILTER_TILE   4096
#define AFG_FILTER_CHUNK  16
#define AFG_FILTER_K      64
#define AFG_BIQUAD_LOWPASS     0
#define AFG_BIQUAD_HIGHPASS    1
#define AFG_BIQUAD_BANDPASS    2
#define AFG_BIQUAD_NOTCH       3
#define AFG_BIQUAD_ALLPASS     4
#define AFG_BIQUAD_PEAKING     5
#define AFG_BIQUAD_LOWSHELF    6
#define AFG_BIQUAD_HIGHSHELF   7
#define AFG_BIQUAD_PREEMPHASIS 8
#define AFG_BIQUAD_DC_BLOCK    9
typedef struct afg_biquad {       /* 40 bytes */
    double b0, b1, b2, a1, a2;    /* a0 == 1 */
} afg_biquad;
typedef struct afg_filter_params {    /* 328 bytes */
    uint32_t   n_sections;        /* 1 .. 8 */
    afg_biquad sec[8];            /* sec[n_sections ..] are not looked at */
} afg_filter_params;
typedef struct afg_filter_row {   /* 24 bytes */
    uint64_t in_off, out_off;     /* float index of frame 0 in d_in / d_out */
    uint32_t frames, reserved;    /* reserved 0 */
} afg_filter_row;
int afg_biquad_design(uint32_t kind, double samplerate, double f0, double q, double gain_db, afg_biquad *out);
double afg_filter_bound(const afg_filter_params *params);
uint32_t afg_filter_tile_frames(void);
int afg_filter_check_rows(const afg_filter_row *rows, uint64_t n_rows, const afg_filter_params *params, uint64_t in_floats,
                          uint64_t out_floats, int same_plane);
int afg_filter_hip(uint64_t n_rows, const afg_filter_row *d_rows, const afg_filter_params *params, const float *d_in,
                   uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_state, void *hip_stream);

/* afg_batch_decode_resampled, then one afg_filter_hip launch in place over the rows and lengths that
 * afg_batch_decode_resampled_norm defines: rows = min(channels, the file's channels), or 1 with mono, each over its valid
 * frames, from zero state.  What lies behind `valid` is +0.0f -- the filter's ringing into the padding is not produced, and
 * the few frames of the resampler's own tail that afg_batch_decode_resampled leaves there are cleared --, and so are the rows
 * a file has no channel for and the slab of a file that failed or was refused.  Sublists as in
 * afg_batch_decode_resampled.  Checked before any device call, AFG_ERR_INVALID with afg_last_error set: everything
 * afg_batch_decode_resampled checks, NULL filter, a cascade afg_filter_bound refuses.  Statuses, messages and items[i] are
 * afg_batch_decode_resampled's. */
int afg_batch_decode_filtered(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                              const afg_filter_params *filter, float *d_out, afg_batch_result *out);

/* ---- loudness: integrated loudness after ITU-R BS.1770-4 / EBU R 128 per group of rows, and the gain to a target ---------
 * What speech and music corpora are levelled with ("every file at -23 LUFS"), as pyloudnorm and ffmpeg's loudnorm measure
 * it: K-weighting, blocks of 400 ms with 75 % overlap, an absolute gate at -70 LKFS and a relative gate 10 LU below the
 * mean of what passes it.  The reference has no such stage; the definition is restated in numpy in tests/loudness_model.py.
 *
 * Parameters (afg_loudness_params), uniform over a call: samplerate 8000 .. 192000 Hz; target_lufs finite, -200 .. 200;
 * max_peak finite and >= 0 (0: no ceiling); max_gain finite and >= 0, linear (0: none); apply 0 (measure only; d_out is not
 * used and may be NULL) or 1; weights[8] the channel weights G_i of rows 0 .. 7, finite and >= 0 -- all zero means every row
 * has weight 1; BS.1770's surround weight is 1.41, its LFE weight 0 --; reserved words 0.  Anything else is AFG_ERR_INVALID.
 *
 * K-weighting.  afg_kweight_design(samplerate, out): host only, in double; out becomes a cascade of two sections, the
 * shelf and then the high-pass, from the analogue prototypes of the standard's 48 kHz table (which these formulas reproduce
 * to 1e-15):
 *   shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs),
 *              Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;
 *              b = (Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2) / a0, a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 *   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; K, a0, a1, a2 of the same form; b = (1, -2, 1), not divided
 *              by a0 -- the standard's table
 * AFG_ERR_INVALID with *out untouched for a samplerate out of range or NULL out.
 *
 * Groups.  A group (afg_loudness_group) is what one measurement covers -- one file's channel rows: rows 1 .. 8; row i
 * starts at float in_off + i * stride of d_in and out_off + i * stride of d_out; only the first `valid` floats of a row count
 * and are touched.
 *
 * Blocks, with libebur128's rounding: step = (samplerate + 5) / 10 in integers, a gating block is N = 4 step samples, block j
 * covers samples [j step, j step + N) of every row, and only whole blocks count:
 * n_blocks = valid >= N ? (valid - N) / step + 1 : 0.  With v_i the K-weighted row i from zero state, over the real numbers,
 *     z_j = (1 / N) * sum over i of G_i * sum over the block's n of v_i[n]^2.
 * Gating is linear throughout -- the device takes no logarithm.  Gamma_abs = 10^((-70 + 0.691) / 10), rounded once in
 * double on the host.  Block j passes the absolute gate when z_j > Gamma_abs; n_abs counts those; Gamma_rel
 * (rel_threshold) = 0.1 * their mean; block j is gated in when z_j > Gamma_abs and z_j > Gamma_rel; n_gated counts those and
 * energy is their mean.  The integrated loudness is -0.691 + 10 log10(energy): afg_loudness_lufs(energy), host only, -inf
 * for 0.
 *
 * Gain.  T = 10^((target_lufs + 0.691) / 10), in double on the host; g = (float)sqrt(T / energy), double division and square
 * root, both correctly rounded; peak is the largest |x| of the group's valid samples, a float32 and exact; with
 * max_gain > 0, g = min(g, max_gain) (AFG_LOUDNESS_GAIN_CLAMPED when that lowers it); with max_peak > 0 and peak > 0,
 * g = min(g, max_peak / peak), a float32 division (AFG_LOUDNESS_PEAK_CLAMPED likewise).  No block gated in -- a group
 * shorter than 400 ms among them --: energy = 0, rel_threshold as computed (0 without a block above the absolute gate),
 * g = 1 and AFG_LOUDNESS_UNGATED.  With apply, every valid element becomes y = x * g, one float32 product; in place
 * (d_out == d_in, out_off == in_off) is allowed, other overlaps of what a launch reads and writes are not.  Nothing outside
 * the valid elements is read or written.  valid == 0: nothing read, nothing written but the record: zero, gain 1,
 * AFG_LOUDNESS_UNGATED.
 *
 * Contract.  An interval, like the filter's, not bits: the device evaluates the K-weighting in float64 exactly as
 * afg_filter_hip evaluates a cascade (chunks of 16 from zero state, the scan), squares and adds in float64 in an order of
 * its own -- the same for the same group wherever it stands.  With
 *     e    = K_L * afg_filter_bound(the K-weighting) * max|x| of the group, K_L = AFG_LOUDNESS_K = 64 = AFG_FILTER_K: the
 *            evaluation is the filter kernel's, operation for operation, and nothing is rounded to float32;
 *     S_ij = the exact sum of squares of the K-weighted row i over block j;
 *     c    = N + rows + 8, which bounds the additions on any path of any summation order,
 * the delivered z^_j (d_blocks) lies within
 *     |z_j - z^_j| <= B_j = (1 / N) * sum over i of G_i * (2 e sqrt(N S_ij) + N e^2) + c * 2^-53 * z^_j
 * of the exact z_j.  A block's gate decision may differ from the exact one only where z^_j lies within its bound of the
 * threshold -- B_j for Gamma_abs, B_j + 0.1 * mean B for Gamma_rel --; given equal gate sets,
 * |energy - e^| <= mean of the gated-in B_j * (1 + 2^-50) (the means are summed with compensation), and the gain follows
 * from the delivered energy by the definition's own operations.  A group holding a sample that is not finite has unspecified
 * results of its own; every other group keeps the contract, and nothing outside the group's valid outputs is written.
 *
 * afg_loudness_layout fills first_sub and first_block of every group and the counts: a group with n_blocks > 0 has
 * n_blocks + 3 sub-blocks of `step` samples per row, and every row of a group with valid > 0 takes its sub-block sums and
 * one more double, its peak, in d_sub; blocks are numbered through the groups in order.  It returns 1, or 0 with
 * afg_last_error set for parameters out of range or a NULL pointer.  afg_loudness_check_groups needs no device
 * (same_plane: whether d_in == d_out): the parameters in range; rows 1 .. 8; reserved words 0; first_sub, first_block and
 * the counts as the layout gives them; for a group with valid > 0, stride >= valid when rows > 1 and its rows inside
 * [0, in_floats) and -- with apply -- [0, out_floats), offsets that would wrap included; and with apply no output row
 * meeting another output row or any input row but its own at the same offset.  n_groups == 0 checks the parameters alone.
 *
 * afg_loudness_hip runs three launches on hip_stream, without atomics, without a workgroup waiting for another and
 * without a host round trip: measure (one workgroup per row: the K-weighted signal is never written, only its sub-block sums
 * and the row's peak, into d_sub, counts->n_sub doubles), gate (one wavefront per group: z^_j into d_blocks,
 * counts->n_blocks doubles, and the record into d_stats, n_groups of them) and, with apply, the product.  d_groups is the
 * device copy of the laid-out groups; the entry fetches it on hip_stream, waits for it and checks it as
 * afg_loudness_check_groups does: anything but a pass is AFG_ERR_INVALID and nothing is written.  The planes are 4-byte
 * aligned, d_groups, d_sub, d_blocks and d_stats 8-byte aligned; at most 2^31 - 1 groups a launch. */
#define AFG_LOUDNESS_K            64
#define AFG_LOUDNESS_UNGATED      1u   /* flags: no block gated in; energy 0, gain 1 */
#define AFG_LOUDNESS_GAIN_CLAMPED 2u   /* flags: max_gain lowered the gain */
#define AFG_LOUDNESS_PEAK_CLAMPED 4u   /* flags: max_peak lowered the gain */
typedef struct afg_loudness_params {  /* 96 bytes */
    uint32_t samplerate;          /* Hz, 8000 .. 192000 */
    uint32_t apply;               /* 0: measure only; 1: also y = x * gain */
    double   target_lufs;
    float    max_peak;            /* 0: no ceiling */
    float    max_gain;            /* linear; 0: none */
    double   weights[8];          /* G_i; all zero: every row 1 */
    uint32_t reserved[2];         /* 0 */
} afg_loudness_params;
typedef struct afg_loudness_group {   /* 64 bytes */
    uint64_t in_off, out_off;     /* float index of row 0, element 0 in d_in / d_out */
    uint64_t stride;              /* floats from one row to the next, in both planes; >= valid when rows > 1 */
    uint64_t first_sub, first_block;  /* filled in by afg_loudness_layout */
    uint32_t rows, valid;
    uint32_t reserved[4];         /* 0 */
} afg_loudness_group;
typedef struct afg_loudness_counts { uint64_t n_sub, n_blocks; } afg_loudness_counts;
typedef struct afg_loudness_stats {   /* 40 bytes, one per group */
    double   energy, rel_threshold;
    uint32_t n_blocks, n_abs, n_gated, flags;
    float    peak, gain;
} afg_loudness_stats;
int afg_kweight_design(uint32_t samplerate, afg_filter_params *out);
double afg_loudness_lufs(double energy);
int afg_loudness_layout(afg_loudness_group *groups, uint64_t n_groups, const afg_loudness_params *params, afg_loudness_counts *counts);
int afg_loudness_check_groups(const afg_loudness_group *groups, uint64_t n_groups, const afg_loudness_counts *counts,
                              const afg_loudness_params *params, uint64_t in_floats, uint64_t out_floats, int same_plane);
int afg_loudness_hip(uint64_t n_groups, const afg_loudness_group *d_groups, const afg_loudness_counts *counts,
                     const afg_loudness_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats,
                     double *d_sub, double *d_blocks, afg_loudness_stats *d_stats, void *hip_stream);

/* afg_batch_decode_resampled, then one afg_loudness_hip launch in place, one group per file exactly as
 * afg_batch_decode_resampled_norm makes them: rows = min(channels, the file's channels), or 1 with mono, and `valid` as
 * defined there; what lies behind `valid` stays as afg_batch_decode_resampled leaves it.  loudness->samplerate must equal
 * opts->samplerate, and at most 8 channels.  A failed or refused file is a group with valid == 0: a zero slab, a zero record
 * with gain 1.  stats (host, n_files records) may be NULL; it is filled when the launch has drained.  Sublists as in
 * afg_batch_decode_resampled; the scratch for sub-block sums, block energies and records is pooled.  Checked before any
 * device call, AFG_ERR_INVALID with afg_last_error set: everything afg_batch_decode_resampled checks, NULL loudness, its
 * parameters, the two rates differing, more than 8 channels.  Statuses, messages and items[i] are
 * afg_batch_decode_resampled's. */
int afg_batch_decode_loudnorm(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                              const afg_loudness_params *loudness, float *d_out, afg_loudness_stats *stats, afg_batch_result *out);

/* The inverse of the linear spectrogram: from a complex spectrum in AFG_STFT_COMPLEX's layout -- masked or edited on the
 * device, or any other -- back to a waveform, by the inverse real transform of every frame and the windowed overlap-add
 * divided by the window envelope: torch.istft's value.  The reference has no such stage.  tests/istft_model.py holds the
 * float64 definition and the interval below.
 *
 * Parameters (afg_istft_params, 32 bytes): n_fft 16 .. 2048 with prime factors 2, 3 and 5 only (anything else is
 * AFG_ERR_UNSUPPORTED), win_length 1 .. n_fft, hop 1 .. n_fft, center 0 or 1, reserved zeros.  The window is the forward
 * stage's: periodic Hann of win_length, w[j] = 0.5 - 0.5 cos(2 pi j / win_length), at n_lo = (n_fft - win_length) / 2 inside
 * the frame.  The table is afg_mel_fft_tables' table unchanged: one device table serves afg_stft_hip and its inverse.
 *
 * Records (afg_istft_row, 40 bytes).  The input is AFG_STFT_COMPLEX's layout: the pair (re, im) of bin k, frame f lies at
 * float in_off + 2 * (k * in_pitch + f), k < n_bins = n_fft / 2 + 1, f < n_frames <= in_pitch (in_pitch lets a padded batch
 * tensor carry a frame count per row).  out_frames samples are written at out_off.
 *
 * Frame f, in float64:
 *   x_f[j] = (1 / n_fft) (re_0 + [n_fft even] (-1)^j re_{n_fft/2}
 *                         + 2 sum over 0 < k < n_fft / 2 of (re_k cos(2 pi k j / n_fft) - im_k sin(2 pi k j / n_fft)))
 * (for odd n_fft the sum runs over 0 < k <= (n_fft - 1) / 2).  im of bin 0, and of bin n_fft / 2 for even n_fft, takes no
 * part, as in torch.istft and every complex-to-real transform: a NaN or an infinity there changes nothing.
 * Line.  n_frames frames make a line of L = n_fft + hop * (n_frames - 1) samples,
 *   N[t] = sum over f of w[t - f hop - n_lo] x_f[t - f hop],    D[t] = sum over f of w[t - f hop - n_lo]^2,
 * both over the frames whose window span (win_length samples from f hop + n_lo) holds t.  Delivered sample i of the record
 * is N[t] / D[t] at t = pad + out_first + i, pad = center ? n_fft / 2 : 0, and pad + out_first + out_frames <= L must hold.
 * torch.istft(..., center=True, length=n) is out_first = 0, out_frames = n.  Without centring the caller sets out_first past
 * the window's zero: the Hann window starts at 0, so center = 0, out_first = 0 is refused, as torch refuses it.
 * Envelope.  afg_istft_envelope_min: host only; the smallest D[t] over the delivered range of a record with these
 * n_frames, out_first and out_frames (each at least 1, the range inside the line), summed in double from the float32 window
 * of the table -- what the device divides by -- or a negative value with afg_last_error set for parameters out of range.
 * A record whose minimum is below 1e-11 (torch.istft's figure) is refused with AFG_ERR_INVALID before the launch; the
 * kernel divides unconditionally.  hop > win_length leaves samples under no window and is refused this way.
 *
 * Bound.  u = 2^-24, B = 8 ceil(log2 n_fft) + 8 (the forward path's), m = ceil(win_length / hop),
 * A'_f = (1 / n_fft) sum over k of c_k (|re_k| + |im_k|) with c_k = 1 and im not counted for the real-only bins and c_k = 2
 * otherwise, S[t] = sum over f of w A'_f over the frames that cover t.  Every delivered sample lies within
 *   E[t] = (B + 2 m + 8) u S[t] / D[t]
 * of the float64 value: to first order a frame sample carries B u A'_f from the transform as in the forward direction; the
 * window product and the sum of at most m terms, in any fixed order, add m u S; D's squares and its sum add m u relative;
 * the division one more u; the remaining 8 cover the float32 window in N and D, the 1 / n_fft scale and second-order terms.
 * Locality and order.  The sum over frames for one sample runs in ascending frame order from +0.0f whatever the tile,
 * wavefront or position of the row, without floating-point atomics: the same row gives the same bits wherever it stands in
 * the batch and whichever tile a sample falls in.  A NaN in a part that is read, in frame f, makes NaN of exactly the
 * delivered samples inside frame f's window span -- the one where w is 0 included, since 0 * NaN is NaN -- and of nothing
 * else.  An all-zero spectrum gives +0.0f.  A record with out_frames = 0 writes nothing and reads nothing.  The kernel
 * writes exactly out_frames floats per record and reads no input float outside the record's n_bins x n_frames pairs.  It
 * does not listen to AFG_NUMERIC or afg_set_numeric_mode.
 *
 * afg_istft_tile_samples: host only; the consecutive delivered samples of one row a workgroup owns for these parameters (it
 * depends on n_fft and hop), or 0 with afg_last_error set for parameters out of range.  afg_istft_layout: host only; gives
 * every row its tiles (first_tile) and returns their count, the sum of ceil(out_frames / tile); 0 with afg_last_error set for
 * parameters out of range.  afg_istft_check_rows: host only, needs no device; the checks afg_istft_hip makes before it
 * launches, on a host copy of the records: parameters in range (AFG_ERR_UNSUPPORTED for the n_fft, AFG_ERR_INVALID
 * otherwise); table_floats at least win_length + 2 * n_fft; first_tile and n_tiles as afg_istft_layout gives them; and for
 * every record with output: n_frames >= 1; n_frames <= in_pitch; the slab's 2 * ((n_bins - 1) * in_pitch + n_frames) floats
 * inside [0, in_floats); its out_frames floats inside [0, out_floats); pad + out_first + out_frames <= L; the envelope's
 * minimum at least 1e-11.  afg_last_error says which.  afg_istft_hip runs every row in one launch, one workgroup per tile;
 * the same checks come first (the entry fetches d_rows on hip_stream and waits for it), and on anything but a pass nothing
 * is written. */
typedef struct afg_istft_params {  /* 32 bytes */
    uint32_t n_fft, win_length, hop, center;
    uint32_t reserved[4];          /* 0 */
} afg_istft_params;
typedef struct afg_istft_row {     /* one [n_bins, n_frames] slab of pairs and its out_frames samples (40 bytes) */
    uint64_t in_off;               /* float index of (re, im) of bin 0, frame 0 */
    uint64_t out_off;              /* float index of the first output sample */
    uint64_t first_tile;           /* filled in by afg_istft_layout */
    uint32_t n_frames;             /* spectrum frames used */
    uint32_t in_pitch;             /* frames per bin row of the slab, >= n_frames */
    uint32_t out_first;            /* first delivered sample of the line, behind pad */
    uint32_t out_frames;           /* samples written */
} afg_istft_row;
uint32_t afg_istft_tile_samples(const afg_istft_params *params);
uint64_t afg_istft_layout(afg_istft_row *rows, uint64_t n_rows, const afg_istft_params *params);
double afg_istft_envelope_min(const afg_istft_params *params, uint32_t n_frames, uint32_t out_first, uint32_t out_frames);
int afg_istft_check_rows(const afg_istft_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_istft_params *params, uint64_t in_floats,
                         uint64_t table_floats, uint64_t out_floats);
int afg_istft_hip(uint64_t n_rows, const afg_istft_row *d_rows, uint64_t n_tiles, const afg_istft_params *params, const float *d_in,
                  uint64_t in_floats, const float *d_table, uint64_t table_floats, float *d_out, uint64_t out_floats, void *hip_stream);

/* The phase-vocoder time stretch: between afg_stft_hip and afg_istft_hip, a complex spectrum is stretched along time by a
 * rate per slab -- torchaudio's phase_vocoder (TimeStretch; librosa.effects.time_stretch's core), as one pass with the phase
 * summed in float64.  The reference has no such stage.  tests/pvoc_model.py holds the definition in long double and the
 * interval below.
 *
 * Input: a slab in AFG_STFT_COMPLEX's layout, the pair (re, im) of bin k, frame f at float in_off + 2 * (k * in_pitch + f),
 * k < n_bins = n_fft / 2 + 1, f < n_frames <= in_pitch.  Output: the same layout with out_pitch and out_frames.
 * Parameters (afg_pvoc_params, 32 bytes): n_fft 2 .. 65536 (no factor rule: nothing is transformed), hop 1 .. n_fft,
 * reserved zeros.  Records (afg_pvoc_row, 48 bytes): in_off, out_off, rate (a double, finite, 1/64 <= rate <= 64), n_frames
 * 1 .. 2^24, in_pitch, out_frames, out_pitch, reserved zeros.
 *
 * Steps.  s_t = fl(t * rate), the one IEEE double product of the integer t and the record's rate (the library is built with
 * -ffp-contract=off, and the kernel writes the product as __dmul_rn, which is never fused); i_t = floor(s_t);
 * a_t = s_t - i_t, which is exact.  afg_pvoc_out_frames(n_frames, rate): host only; the number of t >= 0 with s_t < n_frames
 * -- ceil(n_frames / rate), corrected by at most one where the rounded product disagrees -- or 0 with afg_last_error set for
 * arguments out of range.  A record's out_frames is 0 or exactly that number; with 0 it reads nothing and writes nothing
 * (and only its rate and reserved words are looked at).  The steps go through the rounded product on purpose: floor is
 * discontinuous, and over the real product two evaluations could pick different frame pairs for some rates.
 *
 * Per bin k, over the real numbers from the float32 inputs:
 *   th_f = atan2(im_f, re_f), f < n_frames (IEEE atan2, signed zeros included, as torch.angle has it);
 *   |X_f| = sqrt(re_f^2 + im_f^2); frame n_frames is one frame of (+0, +0), only ever read as i_t + 1;
 *   w_k  = 2 pi hop k / n_fft -- for even n_fft torchaudio's linspace(0, pi hop, n_bins)[k]; for odd n_fft it is the bin's
 *          true advance per hop, which torchaudio's figure (pi hop k / (n_bins - 1)) is not;
 *   d_t  = th_{i_t + 1} - th_{i_t} - w_k,   p_t = d_t - 2 pi round(d_t / 2 pi) + w_k,   ph_t = th_0 + sum over s < t of p_s,
 *   m_t  = a_t |X_{i_t + 1}| + (1 - a_t) |X_{i_t}|,   Y_t = (m_t cos ph_t, m_t sin ph_t), delivered as float32.
 * Only ph_t modulo 2 pi reaches the result: round's tie rule is free, and so is where multiples of 2 pi are dropped.
 *
 * Contract: an interval, not bits.  With u = 2^-24 and v = 2^-53 every delivered component lies within
 *     E_t = m_t * (K_A * u + K_P * v * pi * (t + 1)),   K_A = AFG_PVOC_KA = 2,  K_P = AFG_PVOC_KP = 52
 * of the model's value; afg_pvoc_bound(params, t) returns the bracket (host only; negative with afg_last_error set for
 * parameters out of range).  The accounting, counted from csrc/pvoc.hip's operations before its first run:
 *   K_A  the delivered product is rounded once to float32 (u, relative to |Y| <= m_t); the second u covers the float64
 *        roundings of the magnitude (below) many times over.  (Below float32's normal range a rounding is 2^-150 absolute;
 *        the interval is stated for m_t >= 2^-100.)
 *   K_P  in units of v * pi of phase.  The device keeps every phase in turns (radians / 2 pi), where a value of at most half a
 *        turn rounds by at most v / 2 turn = v * pi radians: one unit; x - rint(x) is then the wrap, and it is exact, as are
 *        the reduction of the carry at every tile and the one in front of sincospi.  Accuracy of the device library: no page
 *        of it is installed with the toolkit, so the assumption is the OpenCL full-profile limits its functions are written
 *        to: double atan2 6 ulp, sinpi / cospi 4 ulp, sqrt correctly rounded; an ulp of x is at most 2 v |x|.
 *        Per summed step s < t (34):  the two atan2, 6 ulp of at most half a turn each: 2 * 12;  their products with
 *        1 / (2 pi), the constant's rounding and the product's: 2 * 2;  th_{i+1} - th_i, at most one turn: 2;  minus the
 *        advance, at most 1.5 turns: 3;  the advance itself, w = centred((hop k) mod n_fft) / n_fft, one division: 1.
 *        Additions, each v times its result, a result of n terms being at most n half-turns (18 (t + 1)):  the chunk sums
 *        (3 deep) and the wavefront scan (6 deep), every level over disjoint terms, all tiles: 9;  the carry's addition per
 *        tile, (T + 1) half-turns each: 2;  carry + lanes below: 1;  the steps below in the chunk: 3;  adding them: 1;
 *        adding the advance's share, up to t + 2 half-turns: 2.
 *        Once (22, under the 34 the step t itself does not spend):  th_0 as above: 14;  the advance's share
 *        centred((hop k t) mod n_fft) * (1 / n_fft), exact integers and two roundings: 2;  sincospi, 4 ulp of at most 1,
 *        8 v <= 3 v pi: 3;  the magnitude -- the sum of two exact squares, the square root, 1 - a, two products, their sum,
 *        the product with cos or sin: at most 8 v relative <= 3 v pi: 3.
 *        34 t + 18 (t + 1) + 22 <= 52 (t + 1).
 * The phase does not grow: its floating sum holds wrapped differences only and is reduced at every tile, so (t + 1) pi, not
 * (t + 1) pi (hop + 1), is the size behind the bound.  m_t = 0 delivers a zero of either sign, with no error allowed.  A NaN or
 * an infinity in bin k, frame f may change the outputs of bin k at the steps with i_t + 1 >= f, and nothing else; every other
 * bin and record keeps the contract.  The same slab gives the same bits wherever it stands in a batch: a row's order of
 * summation is fixed by t alone (chunks of AFG_PVOC_CHUNK steps per lane, tiles of AFG_PVOC_TILE steps, one wavefront per
 * row).  The kernel writes exactly 2 * n_bins * out_frames floats per record, at the pitch, and reads nothing outside the
 * record's n_bins x n_frames pairs.  In place is not allowed: the planes must not overlap.  It does not listen to
 * AFG_NUMERIC or afg_set_numeric_mode.  The launch needs no tiles, so there is no layout helper: a workgroup is four rows.
 *
 * afg_pvoc_check_rows: host only, needs no device; the checks afg_pvoc_hip makes before it launches, on a host copy of the
 * records: n_fft and hop in range and the parameters' reserved words 0; per record the reserved words 0; rate finite and
 * in 1/64 .. 64 (a NaN is refused); and for a record with out_frames > 0: n_frames 1 .. 2^24; n_frames <= in_pitch;
 * out_frames as afg_pvoc_out_frames gives it; out_frames <= out_pitch; the slab's 2 * ((n_bins - 1) * in_pitch + n_frames)
 * floats inside [0, in_floats) and its 2 * ((n_bins - 1) * out_pitch + out_frames) floats inside [0, out_floats), offsets
 * that would wrap included.  Everything is AFG_ERR_INVALID, and afg_last_error says which.  n_rows == 0 checks the
 * parameters alone.  afg_pvoc_hip runs every record in one launch; it fetches d_rows (8-byte aligned; the planes 4-byte)
 * on hip_stream, waits, makes the same checks, and on anything but a pass writes nothing. */
#define AFG_PVOC_KA    2
#define AFG_PVOC_KP    52
#define AFG_PVOC_CHUNK 4      /* consecutive steps a lane sums */
#define AFG_PVOC_TILE  256    /* steps between two reductions of the carry */
typedef struct afg_pvoc_params {   /* 32 bytes */
    uint32_t n_fft, hop;
    uint32_t reserved[6];          /* 0 */
} afg_pvoc_params;
typedef struct afg_pvoc_row {      /* one [n_bins, n_frames] slab of pairs and the [n_bins, out_frames] slab it makes (48 bytes) */
    uint64_t in_off;               /* float index of (re, im) of bin 0, frame 0 in d_in */
    uint64_t out_off;              /* likewise in d_out */
    double   rate;                 /* input frames per output step, 1/64 .. 64 */
    uint32_t n_frames;             /* spectrum frames used, 1 .. 2^24 */
    uint32_t in_pitch;             /* frames per bin row of the input slab, >= n_frames */
    uint32_t out_frames;           /* 0, or afg_pvoc_out_frames(n_frames, rate) */
    uint32_t out_pitch;            /* frames per bin row of the output slab, >= out_frames */
    uint32_t reserved[2];          /* 0 */
} afg_pvoc_row;
uint32_t afg_pvoc_out_frames(uint32_t n_frames, double rate);
double afg_pvoc_bound(const afg_pvoc_params *params, uint64_t t);
int afg_pvoc_check_rows(const afg_pvoc_row *rows, uint64_t n_rows, const afg_pvoc_params *params, uint64_t in_floats, uint64_t out_floats);
int afg_pvoc_hip(uint64_t n_rows, const afg_pvoc_row *d_rows, const afg_pvoc_params *params, const float *d_in, uint64_t in_floats,
                 float *d_out, uint64_t out_floats, void *hip_stream);

/* Convolution of waveform rows with finite kernels: y = h * x for FIR filters, room impulse responses and short smoothing
 * kernels.  The reference has no such stage.  tests/convolve_model.py holds the float64 definition, the float32 restatement
 * of the direct path, S[b] and the interval below.
 *
 * Definition.  A row is `frames` float32 samples x at in_off of the input plane, x[m] = 0 for m outside [0, frames).  A
 * kernel is `taps` >= 1 float32 values h at bank_off of the bank plane (afg_convolve_kernel, 24 bytes).  A record
 * (afg_convolve_row, 48 bytes) names one row and one kernel of the bank by index: rows may share a kernel or each have
 * their own.  Line sample n = 0 .. frames + taps - 2 is, over the real numbers,
 *   y[n] = sum over k = 0 .. taps - 1 with 0 <= n - k < frames of h[k] x[n - k],
 * and the record delivers out_frames samples from out_first at out_off; out_first + out_frames <= frames + taps - 1 must
 * hold.  "full" is out_first = 0, out_frames = frames + taps - 1; "same" is out_first = (taps - 1) / 2, out_frames =
 * frames; a reverb that keeps the file's length and its direct-path alignment is out_first = the index of the response's
 * peak, out_frames = frames.  There is no in-place form: an output shares no float with any input row, the bank, the
 * spectra, the work plane or another output.
 *
 * Two paths, chosen per kernel by its length: a kernel of at most afg_convolve_params.direct_max taps (0 ..
 * AFG_CONV_DIRECT_MAX = 128) takes the direct path, every other kernel the FFT path; direct_max = 0 sends everything
 * through the FFT path.
 *
 * Direct path: bits.  One launch for all direct rows, a workgroup per tile of AFG_CONV_DIRECT_TILE delivered samples.
 * Every sample is
 *   acc = +0.0f;  for k ascending over the terms inside the row:  acc = fmaf(h[k], x[n - k], acc)
 * -- terms outside the row are skipped, not multiplied by zero -- and the result is that float32 bit pattern whatever the
 * tile, the lane, out_first or the place of the row.  A NaN at input sample m reaches exactly the line samples [m, m + taps).
 *
 * FFT path: an interval.  Uniformly partitioned overlap-save on the transform of the STFT stages (csrc/fft_frame.h) with one
 * block length B = AFG_CONV_BLOCK = 1024 and n_fft = 2 B.  A kernel of `taps` has P = ceil(taps / B) partitions; taps goes
 * up to AFG_CONV_MAX_TAPS = 65536 (P <= 64), more is AFG_ERR_UNSUPPORTED.  The block grid is anchored to the line: block b
 * holds line samples [b B, (b + 1) B), whatever out_first is.
 *   The spectrum plane d_spec (afg_convolve_bank_layout gives its size and every kernel's spec_off; 8-byte aligned) starts
 * with the transform's table -- AFG_CONV_TABLE_FLOATS floats, the 2048 pairs (cos, -sin) of afg_mel_fft_tables -- and holds
 * per kernel P spectra of AFG_CONV_SPEC_FLOATS floats: the 1025 pairs (re, im) of the forward real transform of partition p,
 * h[p B .. p B + B) in the first B places of 2 B and zeros behind.  afg_convolve_bank_hip makes the plane: the table is
 * copied in and one launch transforms every partition.  A fixed bank of responses is transformed once and reused over every
 * batch; afg_convolve_hip never writes d_spec.
 *   afg_convolve_hip queues two launches for its FFT rows.  (a) The forward spectrum of every input block pair
 * x[(j - 1) B .. (j + 1) B), zero outside the row, that an output block of the record needs, into the caller's work plane
 * d_work (8-byte aligned; afg_convolve_layout gives its size and every row's work_off): pairs j_lo .. j_hi with
 * j_lo = max(0, b_lo - P + 1), j_hi = min(b_hi, (frames - 1) / B + 1), b_lo and b_hi the first and last block of the
 * delivered range -- about twice the input plus one block per row.  (b) One wavefront per output block forms
 *   Y[k] = sum over p = 0 .. P - 1 of H_p[k] X_{b-p}[k]      in ascending p from +0.0f,
 * each term the four products and two sums of the complex product, unfused; pairs wholly outside the row (b - p < 0 or
 * b - p > (frames - 1) / B + 1) are skipped.  Then the split pass backwards (fft_unsplit_bin) with the scale 1 / n_fft, the
 * inverse complex transform, and the last B samples of the 2 B are delivered as v + (+0.0f), cropped to the record's range.
 * No floating-point atomics: the same (row, kernel) gives the same bits wherever it stands in the batch, in whichever
 * launch, and for any out_first / out_frames that deliver the same line sample.
 *
 * Bound of the FFT path.  u = 2^-24, B_f = 8 ceil(log2 2048) + 8 = 96 per transform (the forward path's: each component of
 * a bin within B_f u A of its float64 value, A the sum of |input|).  A_x(j) = the sum of |x| over block pair j, A_h(p) = the
 * sum of |h| over partition p, S[b] = sum over p of A_h(p) A_x(b - p).  Every delivered sample of block b lies within
 *   E[b] = C u S[b],   C = 6 B_f + 2 P + 11   (afg_convolve_bound; 589 at P = 1, 715 at P = 64)
 * of the float64 value.  Counted per component, to first order, before the first run:
 *   the two forward transforms entering a product: with |X| <= A_x, |H| <= A_h and component errors B_f u A_x, B_f u A_h
 *       a component of H X moves by at most 2 sqrt(2) B_f u A_h A_x:                                       3 B_f
 *   the complex product: two rounded products and their rounded sum, 2 u (|ac| + |bd|) <= 2 u A_h A_x:    2
 *   the sum of at most P terms in fixed order from +0.0f, P - 1 roundings of partial sums within S:        P
 *   so a component of Y is within (3 B_f + 2 + P) u S; the exact inverse, a sum of re cos - im sin over the bins with
 *       weights c_k / n_fft that add up to 1, takes that to at most sqrt(2) (3 B_f + 2 + P) u S:            4.5 B_f + 3 + 1.5 P
 *   the inverse's own arithmetic, B_f u A' with A' = (1 / n_fft) sum of c_k (|re_k| + |im_k|) <= sqrt(2) S: 1.5 B_f
 *   the scale 1 / n_fft is a power of two and v + 0.0f is exact; second-order terms and the roundings up:   8 + 0.5 P
 * The largest share of E[b] used over the GPU suite is measured, not fixed: DESIGN.md has it.
 *
 * NaN.  An FFT row's spectrum of a pair that holds a NaN is NaN in every bin, and a block whose Y holds a NaN is delivered
 * as NaN whole (wavefront votes: containment is stated per block).  So a NaN at input sample m of an FFT row may reach
 * only delivered samples of blocks floor(m / B) .. floor(m / B) + P + 1 of that row, and reaches all of [m, m + taps) inside
 * the delivered range; on the direct path it reaches exactly [m, m + taps).  Other rows are untouched bit for bit.  An
 * all-zero row gives +0.0f on both paths.  A record with out_frames = 0 reads and writes nothing.  Exactly out_frames
 * floats are written per record; no input float outside [in_off, in_off + frames) is read, and no bank float outside a
 * kernel's taps.  The stage does not listen to AFG_NUMERIC or afg_set_numeric_mode.
 *
 * Host entries.  afg_convolve_bank_layout: host only; fills spec_off of every kernel (AFG_CONV_TABLE_FLOATS +
 * AFG_CONV_SPEC_FLOATS * the partitions before it) and returns the spectrum plane's floats; 0 with afg_last_error set for
 * taps 0 (AFG_ERR_INVALID's case) or above 65536.  afg_convolve_bank_check: host only; taps 1 .. 65536 (0: AFG_ERR_INVALID,
 * more: AFG_ERR_UNSUPPORTED), reserved 0, the taps inside [0, bank_floats), spec_off as the layout gives it, spec_floats at
 * least the layout's.  afg_convolve_bank_hip: fetches d_kernels on hip_stream, waits, makes those checks and refuses a
 * spectrum plane that overlaps the bank; then the copy and the launch.  afg_convolve_layout: host only; fills first_tile
 * and work_off of every row and returns the tile count -- a direct row has ceil(out_frames / AFG_CONV_DIRECT_TILE) tiles,
 * an FFT row one per block its range meets -- and *work_floats (AFG_CONV_SPEC_FLOATS per pair; 0 with nothing on the FFT
 * path); 0 with afg_last_error set for parameters out of range or a kernel index outside the bank.  afg_convolve_bound:
 * host only; C for a kernel of `taps` (negative with afg_last_error set when taps or the parameters are out of range).
 * afg_convolve_check_rows: host only, needs no device; the checks afg_convolve_hip makes before it launches, on host
 * copies of the records: direct_max <= 128 and reserved words 0; the bank's checks; first_tile, work_off, n_tiles as the
 * layout gives them and work_floats at least its figure; per record a kernel index inside the bank, and with output asked
 * for: frames 1 .. 2^31 - 65536; the row inside [0, in_floats); the output inside [0, out_floats); out_first + out_frames
 * <= frames + taps - 1.  plane_at: NULL, or the float index of the first float of the input, bank, spectrum, work and
 * output plane (in that order) in one address space, for planes that share an allocation: then an output that meets an
 * input row, the bank, the spectra, the work plane or another output is refused, and so is a work plane that meets the
 * input plane, the bank or the spectra.  Everything is AFG_ERR_INVALID unless said otherwise, and afg_last_error says
 * which.  afg_convolve_hip fetches d_rows and d_kernels on hip_stream, waits, makes the same checks with plane_at taken
 * from the pointers, and queues at most three launches; on anything but a pass nothing is written. */
#define AFG_CONV_BLOCK        1024
#define AFG_CONV_MAX_TAPS     65536
#define AFG_CONV_DIRECT_MAX   128
#define AFG_CONV_DIRECT_TILE  4096
#define AFG_CONV_TABLE_FLOATS 4096
#define AFG_CONV_SPEC_FLOATS  2050
typedef struct afg_convolve_params {  /* 32 bytes */
    uint32_t direct_max;           /* kernels of at most this many taps take the direct path: 0 .. 128 */
    uint32_t reserved[7];          /* 0 */
} afg_convolve_params;
typedef struct afg_convolve_kernel {  /* one kernel of the bank (24 bytes) */
    uint64_t bank_off;             /* float index of h[0] in the bank plane */
    uint64_t spec_off;             /* float index of its first spectrum in d_spec: filled in by afg_convolve_bank_layout */
    uint32_t taps;                 /* 1 .. 65536 */
    uint32_t reserved;             /* 0 */
} afg_convolve_kernel;
typedef struct afg_convolve_row {     /* one row, one kernel, out_frames samples of their line (48 bytes) */
    uint64_t in_off;               /* float index of x[0] */
    uint64_t out_off;              /* float index of the first delivered sample */
    uint64_t first_tile;           /* filled in by afg_convolve_layout */
    uint64_t work_off;             /* likewise: float index of the row's first input spectrum in d_work */
    uint32_t frames;               /* samples of the row */
    uint32_t kernel;               /* index into the bank's records */
    uint32_t out_first;            /* first delivered sample of the line */
    uint32_t out_frames;           /* samples written */
} afg_convolve_row;
uint64_t afg_convolve_bank_layout(afg_convolve_kernel *kernels, uint64_t n_kernels);
int afg_convolve_bank_check(const afg_convolve_kernel *kernels, uint64_t n_kernels, uint64_t bank_floats, uint64_t spec_floats);
int afg_convolve_bank_hip(uint64_t n_kernels, const afg_convolve_kernel *d_kernels, const float *d_bank, uint64_t bank_floats, float *d_spec,
                          uint64_t spec_floats, void *hip_stream);
uint64_t afg_convolve_layout(afg_convolve_row *rows, uint64_t n_rows, const afg_convolve_kernel *kernels, uint64_t n_kernels,
                             const afg_convolve_params *params, uint64_t *work_floats);
double afg_convolve_bound(const afg_convolve_params *params, uint32_t taps);
int afg_convolve_check_rows(const afg_convolve_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_convolve_kernel *kernels, uint64_t n_kernels,
                            const afg_convolve_params *params, uint64_t in_floats, uint64_t bank_floats, uint64_t spec_floats, uint64_t work_floats,
                            uint64_t out_floats, const uint64_t *plane_at);
int afg_convolve_hip(uint64_t n_rows, const afg_convolve_row *d_rows, uint64_t n_tiles, const afg_convolve_kernel *d_kernels, uint64_t n_kernels,
                     const afg_convolve_params *params, const float *d_in, uint64_t in_floats, const float *d_bank, uint64_t bank_floats,
                     const float *d_spec, uint64_t spec_floats, float *d_work, uint64_t work_floats, float *d_out, uint64_t out_floats,
                     void *hip_stream);

/* ---- mixing: noise added to waveform rows at a signal-to-noise ratio, per group of rows -------------------------------------
 * The third waveform augmentation of speech-training recipes beside speed perturbation (the resampler) and reverberation
 * (afg_convolve_hip): additive noise from a bank of clips at a chosen SNR (MUSAN-style; torchaudio.functional.add_noise).
 * The reference has no such stage; the definition is this library's own, restated in numpy in tests/mix_model.py, and the
 * device follows it bit for bit.
 *
 * Groups.  A group (afg_mix_group) is what one gain covers -- one file's channel rows: rows 1 .. 65535; row r starts at
 * float in_off + r * stride of d_in and out_off + r * stride of d_out (4-byte aligned only); only the first `valid` floats
 * of a row count and are touched.  Tiles are afg_norm_group's: 4096 consecutive floats of one row from its element 0, rows
 * ascending, then tiles ascending; afg_mix_layout fills first_tile and returns the tile count.  valid == 0: nothing is
 * read, nothing written, and the record is all zero.
 *
 * Noise source.  The group names its noise in the noise plane d_noise: noise_off (floats, any residue mod 4), noise_len
 * = N >= 1, noise_start < N, noise_stride.  noise_stride 0: one noise row, at noise_off, is shared by all the group's rows;
 * otherwise row r reads the row at noise_off + r * noise_stride, and noise_stride >= N.  The noise sample under element e
 * of row r is n[(noise_start + e) mod N]: a clip shorter than the row loops.
 *
 * Modes (afg_mix_group.flags).  AFG_MIX_SNR: the group carries `ratio`, a float64 the host computes as 10^(-snr_db / 10)
 * (afg_mix_ratio(snr_db): host only; there is no pow on the device, so its results can be compared as bits); finite and
 * >= 0.  AFG_MIX_GAIN: the group carries the float32 `gain` itself, finite and >= 0; the energies are still measured and
 * reported, the record's flags are 0.  The field of the other mode is ignored.
 *
 * Energies, in float64, in the normalisation's order, without atomics.  Es is the sum of x^2 over the valid elements of
 * all rows; En the sum of the squared noise samples as used under the same elements, wrapped -- a shared noise row is
 * counted once per row.  Element e of a tile belongs to lane (e / 4) % 256 of 256 lanes; a lane starts from +0.0 and over
 * its elements in ascending e does q = q + (double)v * (double)v (the product is exact, only the adds round); lanes combine
 * in a binary tree, step d = 1, 2, 4 .. 128, lane l with l % (2 d) == 0 taking v[l] = v[l] + v[l + d]; a group's tile
 * results combine one after the other in tile order from +0.0.
 *
 * Gain.  AFG_MIX_SNR: g = (float)sqrt((Es / En) * ratio): IEEE double division, product and square root, each rounded,
 * nothing contracted, then one rounding to float32.  The gain is 0, and the record's flags say why, when Es is 0
 * (AFG_MIX_SILENT_SIGNAL), En is 0 (AFG_MIX_SILENT_NOISE), Es or En is not finite (AFG_MIX_ENERGY_NOT_FINITE; a NaN
 * sample propagates through its sum), or -- with none of these -- the float32 gain is not finite
 * (AFG_MIX_GAIN_NOT_FINITE).  Several of the first three may be set together.
 *
 * Output.  y = x + g * n: the float32 product rounded first, the float32 sum after it, no fused multiply-add -- with the
 * same gain, torchaudio's expression bit for bit.  With g == 0 the output is the input's bits and the noise is not read
 * (in place: nothing is written).  A NaN in Es, En or the output is always the positive quiet NaN (0x7ff8000000000000,
 * 0x7fc00000), the normalisation's rule: which NaN an operation returns is the hardware's affair, and the definition leaves
 * none of that in its results.  No float behind `valid` is read or written, in any plane.  In place (d_out == d_in,
 * out_off == in_off) is allowed: every element is read and then written by one lane.  Any other meeting of an output row
 * with an input row or another output row is refused, and so is an output plane that overlaps the noise plane.
 *
 * afg_mix_check_groups: host only, needs no device; the checks afg_mix_hip makes before it launches, on a host copy of the
 * groups: flags AFG_MIX_SNR or AFG_MIX_GAIN; the mode's ratio or gain finite and >= 0; rows 1 .. 65535; first_tile and
 * n_tiles as afg_mix_layout gives them; at most 2^32 - 1 groups and 2^31 - 1 tiles; and for a group with valid > 0:
 * stride >= valid when rows > 1; noise_len >= 1, noise_start < noise_len, noise_stride 0 or >= noise_len; its rows inside
 * [0, in_floats) and [0, out_floats) and its noise rows inside [0, noise_floats), offsets and strides that would wrap
 * included; no output row meeting another output row.  plane_at: NULL (three separate planes), or the float index of the
 * first float of the input, noise and output plane (in that order) in one address space: then an output row may meet no
 * input row but its own at the same address, and the output plane must not overlap the noise plane.  AFG_ERR_INVALID with
 * afg_last_error set otherwise.
 *
 * afg_mix_hip: three launches on hip_stream -- the tiles' partial sums into d_partials (n_tiles * 16 bytes, 16-byte
 * aligned), the groups' records into d_stats (n_groups of them, 8-byte aligned), and the apply pass.  d_groups (8-byte
 * aligned) is the device copy of the laid-out groups; the entry fetches it on hip_stream, waits for it and checks every
 * group as afg_mix_check_groups does with plane_at taken from the pointers: anything but a pass is AFG_ERR_INVALID and
 * nothing is written.  The planes are 4-byte aligned. */
#define AFG_MIX_SNR                0u   /* afg_mix_group.flags: the gain follows from the energies and `ratio` */
#define AFG_MIX_GAIN               1u   /* afg_mix_group.flags: the gain is `gain` */
#define AFG_MIX_SILENT_SIGNAL      1u   /* afg_mix_stats.flags: Es is 0; gain 0 */
#define AFG_MIX_SILENT_NOISE       2u   /* afg_mix_stats.flags: En is 0; gain 0 */
#define AFG_MIX_ENERGY_NOT_FINITE  4u   /* afg_mix_stats.flags: Es or En is an infinity or a NaN; gain 0 */
#define AFG_MIX_GAIN_NOT_FINITE    8u   /* afg_mix_stats.flags: the float32 gain came out an infinity or a NaN; gain 0 */
typedef struct afg_mix_group {    /* 80 bytes */
    uint64_t in_off, out_off;     /* float index of row 0, element 0 in d_in / d_out */
    uint64_t stride;              /* floats from one row to the next, in both planes; >= valid when rows > 1 */
    uint64_t first_tile;          /* filled in by afg_mix_layout */
    uint64_t noise_off;           /* float index of the (first) noise row's sample 0 in d_noise */
    uint64_t noise_stride;        /* 0: one noise row for all rows; else floats from one noise row to the next, >= noise_len */
    double   ratio;               /* AFG_MIX_SNR: 10^(-snr_db / 10), afg_mix_ratio */
    uint32_t rows, valid;
    uint32_t noise_len;           /* N: samples of a noise row, >= 1 */
    uint32_t noise_start;         /* the noise sample under element 0, < noise_len */
    uint32_t flags;               /* AFG_MIX_SNR or AFG_MIX_GAIN */
    float    gain;                /* AFG_MIX_GAIN */
} afg_mix_group;
typedef struct afg_mix_stats {    /* 24 bytes, one per group */
    double   signal_energy, noise_energy;
    float    gain;                /* what the apply pass used */
    uint32_t flags;               /* AFG_MIX_SILENT_SIGNAL .. AFG_MIX_GAIN_NOT_FINITE */
} afg_mix_stats;
/* Host only: pow(10, -snr_db / 10) in double. */
double afg_mix_ratio(double snr_db);
/* Host: fills first_tile of every group, returns the launch's tile count. */
uint64_t afg_mix_layout(afg_mix_group *groups, uint64_t n_groups);
int afg_mix_check_groups(const afg_mix_group *groups, uint64_t n_groups, uint64_t n_tiles, uint64_t in_floats, uint64_t noise_floats,
                         uint64_t out_floats, const uint64_t *plane_at);
int afg_mix_hip(uint64_t n_groups, const afg_mix_group *d_groups, uint64_t n_tiles, const float *d_in, uint64_t in_floats,
                const float *d_noise, uint64_t noise_floats, float *d_out, uint64_t out_floats, void *d_partials, afg_mix_stats *d_stats,
                void *hip_stream);

/* afg_batch_decode_resampled, then one afg_mix_hip launch in place over the whole tensor, one group per file exactly as
 * afg_batch_decode_resampled_norm makes them (rows, `valid`); what lies behind `valid`, and the rows a file has no channel
 * for, stay as afg_batch_decode_resampled leaves them.  The noise bank (afg_mix_noise) is the caller's device memory, at the
 * tensor's rate already: n_clips clips of clip_rows rows of clip_pitch floats.  clip_rows 1: a clip's one row is shared by
 * a file's channels; otherwise clip_rows == opts->channels and channel r takes row r.  lengths (host, one per clip, 1 ..
 * clip_pitch; NULL: clip_pitch), index (host, one per file, below n_clips; NULL: clip 0), start (host, one per file, reduced
 * modulo the clip's length; NULL: 0), snr_db (host, one per file, finite).  File i's group is in AFG_MIX_SNR mode with ratio
 * afg_mix_ratio(snr_db[i]).  A failed or refused file is a group with valid == 0: a zero slab, a zero record, gain 0.  stats
 * (host, n_files records) may be NULL; it is filled when the launch has drained.  Checked before any device call,
 * AFG_ERR_INVALID with afg_last_error set: everything afg_batch_decode_resampled checks; NULL noise, d_noise or snr_db;
 * d_noise not 4-byte aligned; n_clips, clip_pitch or clip_rows 0; clip_rows neither 1 nor the tensor's channels; a length,
 * an index or an snr_db out of range; a bank that overlaps the tensor.  Statuses, messages and items[i] are
 * afg_batch_decode_resampled's. */
typedef struct afg_mix_noise {    /* 56 bytes */
    const float    *d_noise;      /* device: [n_clips, clip_rows, clip_pitch] floats */
    uint64_t        n_clips;
    uint32_t        clip_pitch;   /* floats of a clip row */
    uint32_t        clip_rows;    /* 1, or the tensor's channels */
    const uint32_t *lengths;      /* host, n_clips, or NULL */
    const uint32_t *index;        /* host, n_files, or NULL */
    const uint64_t *start;        /* host, n_files, or NULL */
    const double   *snr_db;       /* host, n_files */
} afg_mix_noise;
int afg_batch_decode_mixed(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                           const afg_mix_noise *noise, float *d_out, afg_mix_stats *stats, afg_batch_result *out);

/* ---- Kaldi-compatible filter-bank features (compute-fbank-feats, torchaudio.compliance.kaldi.fbank) -------------------------
 * The other family of speech front-ends beside the centred, reflect-padded, Hann-windowed log10 mel stage above: frames with
 * snip_edges or mirrored with the edge repeated, the DC offset removed per frame, pre-emphasis per frame, Povey's window, zero
 * padding to a power of two, triangles drawn on the mel axis, a natural log over a float32-epsilon floor, an optional
 * log-energy column, frames-major output.  The reference has no such stage: the definition below is this library's own, and
 * tests/fbank_model.py states it again in float64.  There is no dither and no VTLN warp, and subtract_mean (a mean over the
 * frames of an utterance) is the caller's: one tensor op over the valid frames of the result.
 *
 * Parameters (afg_fbank_params), uniform over a launch: win_length ws 2 .. 2048; hop 1 .. 65535 (it may exceed ws); n_fft with
 * ws <= n_fft <= 2048, and one the FFT mel path takes (16 .. 2048, prime factors 2, 3 and 5 only), any other being
 * AFG_ERR_UNSUPPORTED -- afg_fbank_n_fft(ws, round_pow2) gives Kaldi's choice, the next power of two >= ws, or ws itself;
 * n_mels 1 .. 256; snip_edges, remove_dc, use_power, use_log, use_energy, raw_energy, htk_compat each 0 or 1; preemph a finite
 * float in [0, 1]; energy_floor a finite float >= 0; scale a finite float > 0, 0 meaning 1 (Kaldi reads 16-bit samples as
 * integers: 32768 turns a [-1, 1] waveform into what Kaldi sees); layout AFG_FBANK_FRAMES_MAJOR (Kaldi's [frames, cols]) or
 * AFG_FBANK_MEL_MAJOR ([cols, frames], which afg_cepstra_hip consumes); reserved 0.  cols = n_mels + use_energy,
 * n_bins = n_fft / 2 + 1.
 *
 * Frames of a row of N samples (afg_fbank_frames): with snip_edges 0 when N < ws, else 1 + (N - ws) / hop; without,
 * (N + hop / 2) / hop, which is 0 when N is 0.  A record asks for out_frames <= that.
 * Sample j of frame f is x[idx(f * hop + j - pad)], pad = 0 with snip_edges and ws / 2 - hop / 2 (integer divisions; it may
 * be negative) without.  An index outside [0, N) is mirrored with the edge repeated until it lies inside: i < 0 -> -1 - i,
 * i >= N -> 2 N - 1 - i (Kaldi's loop; the extension has period 2 N).  It equals torchaudio's flipped-copy padding wherever
 * that is defined.
 *
 * Per frame.  s_j = float32(x_i * scale) is the one float32 rounding the definition starts from; from there, in float64:
 *   mu = mean of the ws values s_j and d_j = s_j - mu (without remove_dc: d_j = s_j);
 *   e_0 = d_0 - c d_0, e_j = d_j - c d_(j-1), c = preemph;   z_j = e_j w_j for j < ws, 0 up to n_fft;
 *   X_k = DFT of z, k = 0 .. n_fft / 2;   p_k = |X_k|^2, or |X_k| without use_power;   mel_m = sum_k W[m][k] p_k;
 *   the output is mel_m, or with use_log logf(fmaxf(mel_m, 2^-23)).  fmaxf: a NaN takes the floor, this library's convention
 *   (torch.max would hand the NaN on).
 * Energy column (use_energy): En = sum_j d_j^2 with raw_energy, else sum_j z_j^2; its value is logf(fmaxf(En, 2^-23)), raised
 * to logf(energy_floor) when energy_floor > 0.  It is column 0, the mels behind it, or the last column with htk_compat.
 * Output: record r's frame f, column c at out_off + f * cols + c (frames-major) or out_off + c * out_frames + f (mel-major).
 *
 * Tables, host only, computed in double and rounded once to float32.  afg_fbank_tables(window_type, ws, n_fft,
 * blackman_coeff, out, cap) returns ws + 2 * n_fft and with cap >= that fills ws window values, then the n_fft twiddle pairs
 * exactly as afg_mel_fft_tables gives them.  Windows, all symmetric, a = 2 pi j / (ws - 1): AFG_FBANK_WINDOW_POVEY
 * (0.5 - 0.5 cos a)^0.85, _HAMMING 0.54 - 0.46 cos a, _HANNING 0.5 - 0.5 cos a, _BLACKMAN b - 0.5 cos a + (0.5 - b) cos 2a
 * with b = blackman_coeff, _RECTANGULAR 1.  Returns 0 with afg_last_error set for sizes out of range, an unknown window, a
 * blackman_coeff that is not finite, or an n_fft the transform does not take.
 * afg_fbank_filters(samplerate, n_fft, n_mels, low_freq, high_freq, out, cap) returns n_mels * n_bins and with cap >= that
 * fills a dense bank out[m * n_bins + k]: mel(f) = 1127 ln(1 + f / 700); high_freq <= 0 is an offset from Nyquist; n_mels + 2
 * points equally spaced in mel from mel(low_freq) to mel(high_freq), left, centre, right of filter m being points m, m + 1,
 * m + 2; bin k lies at mel_k = mel(k * samplerate / n_fft);
 *   W[m][k] = max(0, min((mel_k - left) / (centre - left), (right - mel_k) / (right - centre))),
 * and the column of the Nyquist bin (k = n_fft / 2 of an even n_fft) is +0.0f.  Returns 0 with afg_last_error set for
 * samplerate 0, sizes out of range, or anything but 0 <= low_freq < high_freq <= samplerate / 2.  The kernel entry takes any
 * dense float32 [n_mels, n_bins] bank of the caller's own instead.
 *
 * What the device may do, and the bound.  Only the orders of summation are free.  The frame's sum, the mean and s_j - mu are
 * formed in float64 and d_j is rounded once to float32 -- required: a waveform at Kaldi's scale with a DC offset loses the
 * signal in a float32 mean.  Everything after that is float32.  u = 2^-24; A_f = sum_j w_j (|d_j| + c |d_(j-1)|) in float64,
 * d_(-1) = d_0; B_k = 8 ceil(log2 n_fft) + 12; then |re - re64| and |im - im64| are at most E_f = B_k u A_f.  Derivation: the
 * value that enters the transform is z_j = fl(fl(d_j - fl(c d_(j-1))) w_j) with d_j itself a rounded value; each of the four
 * roundings (d, the product, the difference, the window product) moves z_j by at most u w_j (|d_j| + c |d_(j-1)|) to first
 * order, and the transform hands an input error on with gain at most 1 per bin, so they cost 4 u A_f together.  The FFT mel
 * path's B = 8 ceil(log2 n_fft) + 8 holds for the transform of these z_j (8 per binary level; its + 8 covers the window
 * product -- counted again here, as margin -- the split pass and second-order terms), with its A_f = sum |z_j| <= this A_f.
 * With p_hi = (|re64| + E)^2 + (|im64| + E)^2 and p_lo = max(|re64| - E, 0)^2 + max(|im64| - E, 0)^2 as in the STFT stage, and
 * a bank without negative weights:
 *   mel lies in [(1 - (n_bins + 4) u) sum_k W p_lo, (1 + (n_bins + 4) u) sum_k W p_hi];
 *   without use_power, p lies within 2 float32 ulp of the square roots of [(1 - 4u) p_lo, (1 + 4u) p_hi], and mel in
 *   [(1 - (n_bins + 4) u) sum_k W m_lo, (1 + (n_bins + 4) u) sum_k W m_hi] of those;
 *   with use_log the output lies within 3 float32 ulp of the natural log of the interval after the floor.
 * Energy: raw, En lies within a relative (ws + 12) u of the float64 value (ws products and adds, and the rounding of d, which
 * moves d^2 by 2 u d^2; the rest is margin); windowed, En lies in (1 -+ (ws + 4) u) sum_j (|z_j| -+ eps_j)^2 with
 * eps_j = 4 u w_j (|d_j| + c |d_(j-1)|), the lower end clamped at 0 per term.  Its log is within 3 ulp as above.
 * Locality.  The same row gives the same bits wherever it stands in a launch.  A NaN sample reaches exactly the frames whose
 * ws samples include it, through the mirror as well, and there every column: NaN, or the floor's log with use_log (the
 * energy column always).  A row with 0 frames has no tiles and nothing of it is read or written.
 *
 * afg_fbank_layout, afg_fbank_check_rows, afg_fbank_hip: as afg_mel_fft_layout, afg_mel_fft_check_rows and
 * afg_melspec_fft_hip, over the same afg_mel_row records; a tile is 16 frames of one row.  afg_fbank_check_rows is host
 * only and needs no device: parameters in range (AFG_ERR_UNSUPPORTED for the n_fft, AFG_ERR_INVALID otherwise); table_floats
 * and filters_floats at least what the tables and the bank need; first_tile and n_tiles as afg_fbank_layout gives them; every
 * row's in_frames floats inside [0, in_floats); out_frames <= afg_fbank_frames; the record's cols * out_frames floats inside
 * [0, out_floats).  afg_fbank_hip fetches d_rows on hip_stream, makes the same checks and on anything but a pass writes
 * nothing.  The kernel writes exactly cols * out_frames floats per record and reads no input float outside the record's row. */
#define AFG_FBANK_FRAMES_MAJOR 0
#define AFG_FBANK_MEL_MAJOR    1
#define AFG_FBANK_WINDOW_POVEY       0
#define AFG_FBANK_WINDOW_HAMMING     1
#define AFG_FBANK_WINDOW_HANNING     2
#define AFG_FBANK_WINDOW_BLACKMAN    3
#define AFG_FBANK_WINDOW_RECTANGULAR 4
typedef struct afg_fbank_params {  /* 64 bytes */
    uint32_t win_length, hop, n_fft, n_mels;
    uint32_t snip_edges, remove_dc, use_power, use_log;
    uint32_t use_energy, raw_energy, htk_compat, layout;
    float    preemph, energy_floor, scale;
    uint32_t reserved;             /* 0 */
} afg_fbank_params;
/* the next power of two >= win_length (round_pow2 != 0) or win_length itself; 0 with afg_last_error set for win_length
 * outside 2 .. 2048 */
uint32_t afg_fbank_n_fft(uint32_t win_length, uint32_t round_pow2);
/* the frames of a row of in_frames samples; 0 for params out of range (afg_last_error set) */
uint32_t afg_fbank_frames(const afg_fbank_params *params, uint32_t in_frames);
uint64_t afg_fbank_tables(uint32_t window_type, uint32_t win_length, uint32_t n_fft, double blackman_coeff, float *out, uint64_t cap);
uint64_t afg_fbank_filters(uint32_t samplerate, uint32_t n_fft, uint32_t n_mels, double low_freq, double high_freq, float *out, uint64_t cap);
uint64_t afg_fbank_layout(afg_mel_row *rows, uint64_t n_rows, const afg_fbank_params *params);
int afg_fbank_check_rows(const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, const afg_fbank_params *params, uint64_t in_floats,
                         uint64_t table_floats, uint64_t filters_floats, uint64_t out_floats);
int afg_fbank_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_fbank_params *params, const float *d_in,
                  uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters, uint64_t filters_floats,
                  float *d_out, uint64_t out_floats, void *hip_stream);

/* afg_batch_decode_resampled followed by afg_fbank_hip: d_out is n_files * channels * n_out * cols floats on the current
 * device -- [files, channels, n_out, cols], or [files, channels, cols, n_out] with AFG_FBANK_MEL_MAJOR -- and slab [i, k] is
 * the definition above applied to row [i, k] of the tensor afg_batch_decode_resampled makes of the same list with the leading
 * fields of the options.  n_out == 0 means afg_fbank_frames of T; otherwise n_out <= that.  n_frames (host, n_files entries,
 * may be NULL) receives per file the feature frames its own resampled samples give -- afg_fbank_frames of the valid length
 * afg_batch_decode_resampled_norm's groups use -- capped at n_out, 0 for a file that failed: what a collation masks by.  In
 * every other respect it is afg_batch_decode_mel: the scratch is pooled under afg_dev_option("mel_scratch_bytes") with
 * sublists of at least one file, the tables and the bank are made once per parameter set -- (window_type, win_length, n_fft,
 * blackman_coeff) and (samplerate, n_fft, n_mels, low_freq, high_freq) -- and kept for the life of the process, without a
 * bound: a caller that sweeps the frequencies builds its banks with afg_fbank_filters and calls afg_fbank_hip.  A file that failed or was
 * refused keeps its status and message and gets the all-zero row's slab, items[i].pcm points at the file's slab (NULL when
 * it failed or was refused), n_files == 0 is AFG_OK and touches nothing.  Checked before any device call, afg_last_error set:
 * everything afg_batch_decode_resampled checks, a struct_size below sizeof(afg_fbank_opts), a non-zero `reserved`, the
 * parameters (AFG_ERR_UNSUPPORTED for the n_fft), the window and the bank's arguments, T without a frame, n_out above the
 * frames of T. */
typedef struct afg_fbank_opts {
    uint32_t         struct_size;   /* sizeof(afg_fbank_opts) */
    int              n_threads;     /* from here to lowpass_width: as afg_resample_opts */
    uint32_t         channels;
    uint32_t         frames;        /* T, samples at `samplerate` */
    const int64_t   *first_frame;
    uint32_t         samplerate;
    uint32_t         mono;
    uint32_t         in_channels;
    uint32_t         max_in_rate;
    uint32_t         lowpass_width;
    uint32_t         n_out;         /* feature frames per slab; 0 means afg_fbank_frames of T */
    afg_fbank_params fbank;
    uint32_t         window_type;   /* AFG_FBANK_WINDOW_* */
    double           low_freq;      /* Hz */
    double           high_freq;     /* Hz; <= 0: an offset from samplerate / 2 */
    double           blackman_coeff;
    uint32_t         reserved;      /* 0 */
} afg_fbank_opts;
int afg_batch_decode_fbank(const uint8_t *const *data, const size_t *length, int n_files, const afg_fbank_opts *opts, float *d_out,
                           uint32_t *n_frames, afg_batch_result *out);

/* ---- Pitch tracking: the YIN fundamental frequency per frame (de Cheveigne & Kawahara 2002; the algorithm of librosa.yin) ----
 * The f0 contour that TTS, voice-conversion and "fbank + pitch" front ends want, behind the tensor at one sample rate.  The
 * reference has no such stage: the definition below is this library's own, every step in a fixed arithmetic order, so that
 * the device result is bit for bit what tests/yin_model.py restates in numpy, decisions included.
 *
 * Parameters of a call (afg_yin_params, 48 bytes), uniform over its rows: frame_length N 4 .. 4096; win_length W 1 .. N - 2;
 * hop >= 1 (it may exceed N); tau_min and tau_max with 1 <= tau_min <= tau_max <= N - W - 1; center 0 or 1; pad_mode
 * AFG_MEL_PAD_REFLECT or AFG_MEL_PAD_ZERO; threshold a finite float >= 0; samplerate a finite double > 0; reserved 0.
 * afg_yin_lags(samplerate, fmin, fmax, N, W, &tau_min, &tau_max) gives librosa's choice, tau_min = floor(samplerate / fmax)
 * and tau_max = min(ceil(samplerate / fmin), N - W - 1), and refuses (AFG_ERR_INVALID, afg_last_error set, nothing stored)
 * sizes out of range, anything but finite 0 < fmin < fmax and a finite samplerate > 0, and an empty range: tau_min < 1 or
 * tau_min > tau_max.
 *
 * Framing is the mel stage's: sample n of frame f is x[idx(f * hop + n - pad)], pad = center ? N / 2 : 0; an index outside
 * [0, in_frames) is reflected without repeating the edge or reads +0.0f, according to pad_mode; reflect needs in_frames > pad,
 * and a record with output that breaks this is refused before the launch.  The row has afg_mel_frames' count with n_fft = N:
 * 1 + (in_frames + 2 pad - N) / hop frames, 0 when the numerator is negative, 2^32 - 1 at the most (afg_yin_frames).  A frame reads only its
 * samples 0 .. W - 1 + tau_max.
 *
 * Per frame, with x_n its samples:
 *   1  difference.  For tau = 1 .. tau_max, d(tau) is the chain over j = 0 .. W - 1, in that order, from +0.0f, of
 *      fmaf(e, e, acc) with e = x_j - x_(j + tau) rounded to float32: one fmaf per term, nothing wider, no reassociation.
 *   2  cumulative mean, in float64, in chunks of AFG_YIN_CHUNK = 16 lags: c = (tau - 1) / 16; p(tau) is the sequential
 *      float64 sum of (double)d over the lags of chunk c up to and including tau; B_0 = +0.0, B_(c+1) = B_c + p(last lag of
 *      chunk c); s(tau) = B_c + p(tau).  d'(tau) = 1.0f when s(tau) == 0, otherwise float32((double)d(tau) * (double)tau /
 *      s(tau)): the product is exact, there is one IEEE division and one rounding to float32.
 *   3  choice.  Over tau in [tau_min, tau_max], trough(tau) is: for tau_min < tau < tau_max, d'(tau) < d'(tau - 1) and
 *      d'(tau) <= d'(tau + 1); for tau = tau_min, d'(tau_min) < d'(tau_min + 1), and false when tau_min == tau_max; for
 *      tau = tau_max > tau_min, false.  tau* is the smallest tau with trough(tau) and d'(tau) < threshold; if there is
 *      none, the smallest tau that attains the minimum of d' over the range.
 *   4  refinement, in float64 from the float32 values: with a = d'(tau* - 1), b = d'(tau*), c = d'(tau* + 1),
 *      A = ((double)c + (double)a) - 2.0 * (double)b, B = ((double)c - (double)a) * 0.5, shift = |B| < |A| ? -B / A : 0;
 *      shift = 0 when tau* is tau_min or tau_max.  f0 = float32(samplerate / ((double)tau* + shift)).
 *   5  non-finite input.  If any d'(tau), tau = 1 .. tau_max, is a NaN, both outputs of the frame are the word 0x7fc00000.
 * A silent or constant frame needs no case: every d' is 1.0f, so it delivers f0 = samplerate / tau_min and d' = 1.0f.  A
 * frame is voiced iff its plane 1 is below the threshold.
 * Output per record, two planes of out_frames floats, frames contiguous: f0 of frame f at out_off + f, d'(tau*) at
 * out_off + out_frames + f.
 *
 * Records are afg_mel_row; a record's slab is 2 * out_frames floats.  afg_yin_layout gives every row its tiles (first_tile)
 * and returns the launch's tile count, 0 with afg_last_error set for params out of range; a tile is AFG_YIN_TILE = 4
 * consecutive frames of one record.  afg_yin_hip fetches d_rows on hip_stream and checks the parameters and every record
 * before the launch: first_tile and n_tiles as afg_yin_layout gives them; every row's in_frames floats inside
 * [0, in_floats); out_frames <= afg_yin_frames; reflect with output only with in_frames > pad; the record's 2 * out_frames
 * floats inside [0, out_floats).  On a failed check it returns AFG_ERR_INVALID with afg_last_error set and writes nothing.
 * The kernel writes exactly 2 * out_frames floats per record and reads no input float outside the record's row.  n_rows == 0
 * is AFG_OK.  Locality: the same row gives the same bits wherever it stands, and a NaN sample reaches exactly the frames
 * whose samples 0 .. W - 1 + tau_max include it. */
#define AFG_YIN_CHUNK 16
#define AFG_YIN_TILE  4
typedef struct afg_yin_params {    /* 48 bytes */
    uint32_t frame_length, win_length, hop;
    uint32_t tau_min, tau_max;
    uint32_t center, pad_mode;     /* AFG_MEL_PAD_* */
    float    threshold;
    double   samplerate;           /* Hz, of the rows */
    uint32_t reserved[2];          /* 0 */
} afg_yin_params;
int afg_yin_lags(double samplerate, double fmin, double fmax, uint32_t frame_length, uint32_t win_length, uint32_t *tau_min, uint32_t *tau_max);
/* the frames of a row of in_frames samples; 0 for params out of range (afg_last_error set) */
uint32_t afg_yin_frames(const afg_yin_params *params, uint32_t in_frames);
uint64_t afg_yin_layout(afg_mel_row *rows, uint64_t n_rows, const afg_yin_params *params);
int afg_yin_hip(uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_yin_params *params, const float *d_in,
                uint64_t in_floats, float *d_out, uint64_t out_floats, void *hip_stream);

/* afg_batch_decode_resampled followed by afg_yin_hip: d_out is n_files * channels * 2 * n_out floats on the current device,
 * [files, channels, 2, n_out], and planes [i, k, 0] (f0) and [i, k, 1] (d') are the definition above applied to row [i, k] --
 * all T samples of it -- of the tensor afg_batch_decode_resampled makes of the same list with the leading fields of the
 * options.  n_out == 0 means afg_yin_frames of T; otherwise n_out <= that.  A file's own frames are the first
 * min(n_out, afg_yin_frames(valid)) of them, valid being the length afg_batch_decode_resampled_norm's groups use, and none
 * for a file that failed or has no sample; the frames past them are +0.0f in both planes.  n_frames (host, n_files entries,
 * may be NULL) receives that count per file.  yin.samplerate must equal `samplerate`.  The resampled tensor of a sublist
 * stands in a scratch pooled under afg_dev_option("resample_scratch_bytes"), sublists of at least one file.  A file that
 * failed or was refused keeps its status and message, items[i].pcm points at the file's slab (NULL when it failed or was
 * refused), n_files == 0 is AFG_OK and touches nothing.  Checked before any device call, afg_last_error set: everything
 * afg_batch_decode_resampled checks, a struct_size below sizeof(afg_pitch_opts), a non-zero `reserved`, the parameters, a
 * yin.samplerate that differs from samplerate, T without a frame, reflect padding with T <= pad, n_out above the frames
 * of T. */
typedef struct afg_pitch_opts {
    uint32_t         struct_size;   /* sizeof(afg_pitch_opts) */
    int              n_threads;     /* from here to lowpass_width: as afg_resample_opts */
    uint32_t         channels;
    uint32_t         frames;        /* T, samples at `samplerate` */
    const int64_t   *first_frame;
    uint32_t         samplerate;
    uint32_t         mono;
    uint32_t         in_channels;
    uint32_t         max_in_rate;
    uint32_t         lowpass_width;
    uint32_t         n_out;         /* frames per plane; 0 means afg_yin_frames of T */
    afg_yin_params   yin;
    uint32_t         reserved;      /* 0 */
} afg_pitch_opts;
int afg_batch_decode_pitch(const uint8_t *const *data, const size_t *length, int n_files, const afg_pitch_opts *opts, float *d_out,
                           uint32_t *n_frames, afg_batch_result *out);

/* ---- Sliding-window cepstral mean and variance normalisation (Kaldi's apply-cmvn-sliding, torchaudio's sliding_window_cmn) --
 * What the Kaldi recipes put behind fbank and MFCC features instead of one set of statistics per utterance: every frame is
 * normalised by the mean (and variance) of a window of frames around or in front of it -- 300 frames centred for x-vector and
 * ECAPA speaker models, 600 causal frames with min_cmn_window 100 for online ASR.  The reference has no such stage: the
 * definition below is this library's own, tests/slidecmn_model.py states it again in numpy, and the device follows it bit
 * for bit.
 *
 * Slab (afg_cmn_slab): n_frames = N valid frames by `cols` columns of float32; element [t][c] is at in_off + t * pitch + c of
 * d_in with AFG_CMN_FRAMES_MAJOR (what afg_fbank_hip writes by default; Kaldi's own layout) and at in_off + c * pitch + t
 * with AFG_CMN_COL_MAJOR (the mel, MFCC and AFG_FBANK_MEL_MAJOR slabs); out_off likewise in d_out, with the same pitch.
 * Frames at and beyond N are neither read nor written; N == 0 touches nothing.
 *
 * Parameters (afg_cmn_params), uniform over a launch: cmn_window 1 .. AFG_CMN_MAX_WINDOW (2^20: nothing a tile holds depends
 * on the window, but every output adds one pair of chunk totals per 32 frames of it, so the time grows with it);
 * min_cmn_window 1 .. AFG_CMN_MAX_WINDOW (used only without center); center and norm_vars each 0 or 1; cols
 * 1 .. AFG_CMN_MAX_COLS (1024); layout AFG_CMN_FRAMES_MAJOR or AFG_CMN_COL_MAJOR; reserved 0.  N is at most 2^31 - 1.
 *
 * Window of frame t, in integers -- Kaldi's SlidingWindowCmnInternal, quirks included:
 *   center:  ws = t - cmn_window / 2, we = ws + cmn_window;   otherwise:  ws = t - cmn_window, we = t + 1 (so the causal window
 *   holds cmn_window + 1 frames);
 *   if ws < 0: we -= ws, then ws = 0;
 *   if not center and we > t (always): we = max(t + 1, min_cmn_window);
 *   if we > N: ws -= we - N, then we = N, then ws = max(ws, 0);
 *   n = we - ws, at least 1; the window is frames ws .. we - 1.
 *
 * Sums S1 = sum of x and S2 = sum of x * x over the window, per column, in float64, in a fixed order, from the window's own
 * elements only (no difference of running prefixes: that would carry a NaN or an infinity of frame 0 into every later
 * window, and lose the low bits on long slabs).  (double)x * (double)x is exact; only the adds round.  Chunks are
 * AFG_CMN_CHUNK = 32 frames, aligned to frame 0 of the slab; the last may be short.  Inside a chunk pre[j] is the sum from
 * the chunk's first frame ascending to j inclusive and suf[j] the sum from the chunk's last valid frame descending to j
 * inclusive, each starting from +0.0; the chunk's total is pre of its last frame.  A window whose first and last frame lie in
 * different chunks sums as suf[ws], then the totals of the whole chunks strictly between added one after the other ascending,
 * then pre[we - 1] added last.  A window inside one chunk sums its elements ascending from +0.0.  S2 follows the same order.
 *
 * Output, in float64 until the last step, every operation rounded by itself (no fused multiply-add):
 *   mean = S1 / n;   without norm_vars  y = (float)((double)x - mean);
 *   with norm_vars and n == 1  y = +0.0f;
 *   with norm_vars and n > 1   var = S2 / n - mean * mean;  var = var < 1e-10 ? 1e-10 : var (Kaldi's floor; a NaN stays a NaN);
 *                              y = (float)(((double)x - mean) * (1.0 / sqrt(var))).
 * A NaN result is always 0x7fc00000, as in the normalise stage.  So a NaN frame makes NaN exactly of the outputs whose window
 * holds it; an infinite one likewise with norm_vars (var is inf - inf), while without it mean is infinite and finite elements
 * of such a window come out as the opposite infinity.  torchaudio.functional.sliding_window_cmn has no floor and, with
 * norm_vars, n == 1 gives 0 there too; away from the floor the two agree to rounding (tests/test_slidecmn_model.py).
 *
 * Records, tiles, checks.  A tile is one chunk of one slab, all columns; a slab has ceil(N / 32) of them, a slab's tiles follow
 * those of the slab before.  afg_cmn_layout fills first_tile and returns the launch's tile count.  The launch needs a
 * workspace of afg_cmn_work_bytes(n_tiles, cols) = n_tiles * cols * 144 bytes, 16-byte aligned, that overlaps neither plane:
 * the chunk totals, and a copy of every valid element -- the window of a frame reaches into other tiles, so in place nothing
 * may read the plane once the first result is written; both placements run through the copy and give the same bits.
 * afg_cmn_check_slabs is host only and runs every check the entry makes: parameters in range; first_tile and n_tiles as
 * afg_cmn_layout gives them; reserved 0; N <= 2^31 - 1; and for a slab with N > 0: pitch at least cols (frames-major, when
 * N > 1) or at least N (col-major, when cols > 1); the slab inside [0, in_floats) and [0, out_floats); no output slab -- its
 * whole span, the gaps a larger pitch leaves included -- overlapping another output slab, or with same_plane (the entry
 * passes d_in == d_out) any input slab but its own at the same offset.  AFG_ERR_INVALID with afg_last_error set otherwise;
 * n_slabs == 0 checks the parameters alone.  afg_slide_cmn_hip fetches d_slabs on hip_stream, waits, makes the same checks
 * and the workspace's, and on anything but a pass writes nothing; then two launches on hip_stream.  n_slabs == 0 is AFG_OK.
 * Locality: a slab's result is the same bits wherever it stands in the planes and whatever its neighbours are. */
#define AFG_CMN_FRAMES_MAJOR 0
#define AFG_CMN_COL_MAJOR    1
#define AFG_CMN_CHUNK        32
#define AFG_CMN_MAX_WINDOW   1048576
#define AFG_CMN_MAX_COLS     1024
typedef struct afg_cmn_params {    /* 32 bytes */
    uint32_t cmn_window, min_cmn_window, center, norm_vars;
    uint32_t cols, layout;         /* AFG_CMN_* */
    uint32_t reserved[2];          /* 0 */
} afg_cmn_params;
typedef struct afg_cmn_slab {      /* 48 bytes */
    uint64_t in_off, out_off;      /* float index of element [0][0] in d_in / d_out */
    uint64_t pitch;                /* floats from one frame (frames-major) or one column (col-major) to the next, in both planes */
    uint64_t first_tile;           /* filled in by afg_cmn_layout */
    uint32_t n_frames;             /* N */
    uint32_t reserved[3];          /* 0 */
} afg_cmn_slab;
/* Host: fills first_tile of every slab, returns the launch's tile count. */
uint64_t afg_cmn_layout(afg_cmn_slab *slabs, uint64_t n_slabs);
/* Host: the workspace of a launch, n_tiles * cols * 144 bytes. */
uint64_t afg_cmn_work_bytes(uint64_t n_tiles, uint32_t cols);
int afg_cmn_check_slabs(const afg_cmn_slab *slabs, uint64_t n_slabs, uint64_t n_tiles, const afg_cmn_params *params, uint64_t in_floats,
                        uint64_t out_floats, int same_plane);
int afg_slide_cmn_hip(uint64_t n_slabs, const afg_cmn_slab *d_slabs, uint64_t n_tiles, const afg_cmn_params *params, const float *d_in,
                      uint64_t in_floats, float *d_out, uint64_t out_floats, void *d_work, uint64_t work_bytes, void *hip_stream);

/* afg_batch_decode_fbank, then afg_slide_cmn_hip in place over the first n_frames[i] frames of every slab [i, k], in the
 * layout the fbank options name.  cols and layout of `cmn` are filled in from the fbank options (n_mels + use_energy and the
 * fbank layout), whatever the caller put there; its other fields are the caller's.  Frames behind n_frames[i] stay as
 * afg_batch_decode_fbank leaves them, and so do the slabs of failed and refused files, whose count is 0.  n_frames (host,
 * n_files entries) may be NULL.  Statuses, messages and items[i] are afg_batch_decode_fbank's, and so is every check it makes;
 * NULL or out-of-range cmn is refused before any device call as well.  The workspace is pooled. */
int afg_batch_decode_fbank_cmn(const uint8_t *const *data, const size_t *length, int n_files, const afg_fbank_opts *opts,
                               const afg_cmn_params *cmn, float *d_out, uint32_t *n_frames, afg_batch_result *out);

#ifdef __cplusplus
}
#endif
#endif /* AFG_H */
