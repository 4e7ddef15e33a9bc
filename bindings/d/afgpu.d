/// afgpu.d -- D binding of the MI355X transform-stage library (include/afg.h, ABI version 1).
///
/// Source only: no D compiler exists in the build image, so this file is exercised through the
/// same C symbols from C/Python harnesses instead.  Every prototype carries `nothrow @nogc`, which is
/// what makes it callable from audio-formats' `nothrow @nogc` decoder modules
/// (source/audioformats/minimp3.d:16-17, stb_vorbis2.d:110-111, drflac.d:21).
module audioformats.afgpu;

nothrow @nogc extern (C):

enum AFG_ABI_VERSION = 2;

enum afg_status : int
{
    AFG_OK = 0,
    AFG_ERR_INVALID = -1,
    AFG_ERR_NO_DEVICE = -2,
    AFG_ERR_HIP = -3,
    AFG_ERR_OOM = -4,
    AFG_ERR_UNSUPPORTED = -5,
}

int afg_abi_version();
const(char)* afg_status_string(int status);
const(char)* afg_last_error();
int afg_device_count();

/// Numeric mode of the float transform stages (afg.h): exact = the reference's expression trees bit for bit; tolerance
/// (default) = within 1e-5 RMS, which lets the Opus/CELT stage re-associate, the Vorbis stage use one radix-8 FFT per block
/// and the MP3 stage fuse its multiply-adds (round 4).  AFG_NUMERIC_FROM_ENV hands the choice back to
/// the environment variable AFG_NUMERIC.  Returns the mode in effect before.
enum AFG_NUMERIC_FROM_ENV = -1, AFG_NUMERIC_EXACT = 0, AFG_NUMERIC_TOLERANCE = 1;
int afg_set_numeric_mode(int mode);
int afg_dev_option(const(char)* name, int value);
int afg_get_numeric_mode();
int afg_device_name(int device, char* buf, size_t buflen);

// ---- MP3 (replaces minimp3.d:1226-1228 + :1553) ------------------------------------------
struct afg_mp3_plan;
enum AFG_MP3_STATE_FLOATS = 1536;

uint AFG_MP3_FLAGS(uint block_type, uint n_long_bands, int aa_bands) pure
{
    return block_type | (n_long_bands << 8) | (cast(uint)(aa_bands + 1) << 16);
}

// optional, OR-ed into the flag word: only the first `bands` subbands (0..32) may hold lines that are not +0.0
uint AFG_MP3_NZ_BANDS(uint bands) pure { return (bands + 1) << 24; }
enum uint AFG_MP3_SUBBAND = 0x80000000;   // the block holds Layer I / II subband samples (band * 18 + slot): synthesis only

int afg_mp3_plan_create(afg_mp3_plan** plan, uint n_streams, const(uint)* granules,
                        const(ubyte)* channels, uint seg_granules);
void afg_mp3_plan_destroy(afg_mp3_plan* plan);
ulong afg_mp3_plan_blocks(const(afg_mp3_plan)* plan);
uint afg_mp3_plan_segments(const(afg_mp3_plan)* plan);
int afg_mp3_transform_hip(const(afg_mp3_plan)* plan, const(float)* d_coef, const(uint)* d_flags,
                          float* d_pcm, float* d_state, void* hip_stream);

// ---- Vorbis (replaces stb_vorbis2.d:2526-2527 + :2606-2657 + :3927-3952) ---------------------
struct afg_vorbis_plan;
enum AFG_VORBIS_LONG = 1u, AFG_VORBIS_PREV = 2u, AFG_VORBIS_NEXT = 4u;
/// optional, long packets: only the first e eighths of the spectrum can be nonzero (residue end, stb_vorbis2.d:1586-1600)
uint AFG_VORBIS_NZ_EIGHTHS(uint e) { return (e + 1u) << 4; }

int afg_vorbis_plan_create(afg_vorbis_plan** plan, uint n_streams, const(uint)* packets,
                           const(ubyte)* channels, const(ushort)* blocksize0,
                           const(ushort)* blocksize1, const(ubyte)* pflags, uint seg_packets);
void afg_vorbis_plan_destroy(afg_vorbis_plan* plan);
ulong afg_vorbis_plan_packets(const(afg_vorbis_plan)* plan);
ulong afg_vorbis_plan_spec_floats(const(afg_vorbis_plan)* plan);
ulong afg_vorbis_plan_out_floats(const(afg_vorbis_plan)* plan);
int afg_vorbis_plan_offsets(const(afg_vorbis_plan)* plan, ulong* spec_off, ulong* out_off);
int afg_vorbis_transform_hip(const(afg_vorbis_plan)* plan, const(float)* d_spec, float* d_out,
                             void* hip_stream);

// inverse coupling + floor curves on the device (replaces stb_vorbis2.d:2493-2523 with do_floor :2255-2284 / draw_line :1534-1563)
struct afg_vorbis_floor_packet
{
    ulong spec_off;
    uint n2, channels, curve_index, step_off, n_steps, pad;
}
static assert(afg_vorbis_floor_packet.sizeof == 32);
struct afg_vorbis_floor_curve { uint point_off, n_points; }
int afg_vorbis_floor_hip(ulong n_packets, const(afg_vorbis_floor_packet)* d_packets, const(afg_vorbis_floor_curve)* d_curves,
                         const(int)* d_points, const(ubyte)* d_steps, float* d_spec, void* hip_stream);

// ---- FLAC (replaces drflac.d:1235 prediction half + :2885-2941, optionally stream.d:505-511) --
enum AFG_FLAC_INDEPENDENT = 0, AFG_FLAC_LEFT_SIDE = 8, AFG_FLAC_RIGHT_SIDE = 9, AFG_FLAC_MID_SIDE = 10;

struct afg_flac_subframe
{
    short[32] coef;
    ubyte order;
    ubyte shift;
    ubyte wasted;
    ubyte use64;
}
static assert(afg_flac_subframe.sizeof == 68);

struct afg_flac_frame
{
    ulong in_off;
    ulong out_off;
    uint block_size;
    uint sf_index;
    ubyte channels;
    ubyte assignment;
    ubyte bps;
    ubyte res16;          // 1: the frame's residual rows are int16 (in_off counts int16 elements, rows of AFG_FLAC_ROW16)
    ubyte[4] pad;
}
static assert(afg_flac_frame.sizeof == 32);
ulong AFG_FLAC_ROW16(ulong block_size) { return (block_size + 7) & ~7UL; }

int afg_flac_transform_hip(ulong n_frames, const(afg_flac_frame)* d_frames,
                           const(afg_flac_subframe)* d_subframes, const(int)* d_res,
                           int* d_out_i32, float* d_out_f32, void* hip_stream);
uint afg_flac_variants(ulong n_frames, const(afg_flac_frame)* frames, const(afg_flac_subframe)* subframes);   // host records
int afg_flac_transform_variants_hip(ulong n_frames, const(afg_flac_frame)* d_frames,
                                    const(afg_flac_subframe)* d_subframes, const(int)* d_res,
                                    int* d_out_i32, float* d_out_f32, uint variants, void* hip_stream);

// ---- QOA (replaces the slice loop of qoa_decode_frame, qoa.d:489-530, and qoa.d:831-838) --------
struct afg_qoa_frame
{
    ulong byte_off;
    ulong out_off;
    ushort samples;
    ubyte channels;
    ubyte[5] pad;
}
static assert(afg_qoa_frame.sizeof == 24);

int afg_qoa_transform_hip(ulong n_frames, const(afg_qoa_frame)* d_frames, const(ubyte)* d_bytes,
                          short* d_out_i16, float* d_out_f32, void* hip_stream);

// OpusFile.readFrame's Float2IntScaled + saturation (dopus.d:7923-7926, :8098-8105) and stream.d:480
int afg_opus_output_hip(ulong n_samples, const(float)* d_in, short* d_out_i16, float* d_out_f32, void* hip_stream);
int afg_opus_output_gain_hip(ulong n_samples, const(float)* d_in, float gain, short* d_out_i16, float* d_out_f32, void* hip_stream);

// ---- output side: QOA encoder (replaces qoa_encode_frame, qoa.d:295-399, and QOAEncoder's framing, :538-700) and
//      the WAV writer (WAVEncoder, wav.d:365-701; host only) ----
struct afg_qoa_enc_stream
{
    ulong pcm_off;
    ulong out_off;
    uint samples;
    uint samplerate;
    ubyte channels;
    ubyte[7] pad;
}
static assert(afg_qoa_enc_stream.sizeof == 32);

ulong afg_qoa_encoded_size(uint samples, uint channels);
int afg_qoa_encode_hip(uint n_streams, const(afg_qoa_enc_stream)* d_streams, const(short)* d_pcm_i16,
                       const(float)* d_pcm_f32, ubyte* d_out, void* hip_stream);

enum { AFG_WAV_S8 = 0, AFG_WAV_S16LE = 1, AFG_WAV_S24LE = 2, AFG_WAV_FP32LE = 3, AFG_WAV_FP64LE = 4 }
ulong afg_wav_encoded_size(ulong frames, uint channels, int format);
ulong afg_wav_encode(const(float)* samples, ulong frames, uint channels, uint samplerate, int format,
                     ubyte* out_, ulong cap);

// ---- Opus/CELT (replaces the per-channel tail of ff_celt_decode_frame, dopus.d:3680-3702) -------
struct afg_celt_frame
{
    ulong coef_off;
    ulong out_off;
    uint out_stride;
    ushort frame_size;
    ubyte blocks;
    ubyte pad;
    int pf_period_new;
    float[3] pf_gains_new;
    float imdct_scale;
    uint pad2;
}
static assert(afg_celt_frame.sizeof == 48);
enum AFG_CELT_STATE_FLOATS = 2064;

int afg_celt_transform_hip(uint n_chan, const(ulong)* d_rec_base, const(afg_celt_frame)* d_recs,
                           const(float)* d_coeffs, float* d_out, float* d_states, void* hip_stream);

// ---- utilities ----------------------------------------------------------------------------------
int afg_device_malloc(void** d_ptr, size_t bytes);
int afg_device_free(void* d_ptr);
int afg_memcpy_h2d(void* d_dst, const(void)* src, size_t bytes, void* hip_stream);
int afg_memcpy_d2h(void* dst, const(void)* d_src, size_t bytes, void* hip_stream);
int afg_stream_synchronize(void* hip_stream);
int afg_copy_probe_hip(void* d_dst, const(void)* d_src, size_t bytes, void* hip_stream);

// ---- outer surface: the reading half of AudioStream (stream.d:102-637) ----------------------------
enum afg_format : int   // AudioFileFormat, stream.d:36-47 (same order)
{
    wav = 0, mp3 = 1, flac = 2, ogg = 3, opus = 4, qoa = 5, mod = 6, xm = 7, unknown = 8,
}
enum long AFG_UNKNOWN_LENGTH = -1;   // audiostreamUnknownLength, stream.d:90

struct afg_stream;
afg_stream* afg_open_from_memory(const(ubyte)* data, size_t length);
int afg_is_error(const(afg_stream)* s);
const(char)* afg_error_message(const(afg_stream)* s);
int afg_get_format(const(afg_stream)* s);
int afg_get_num_channels(const(afg_stream)* s);
long afg_get_length_in_frames(const(afg_stream)* s);
float afg_get_samplerate(const(afg_stream)* s);
int afg_read_samples_float(afg_stream* s, float* outData, int frames);
int afg_read_samples_double(afg_stream* s, double* outData, int frames);   // readSamplesDouble, stream.d:656-747
int afg_can_seek(const(afg_stream)* s);
int afg_seek_position(afg_stream* s, int frame);
int afg_tell_position(const(afg_stream)* s);
void afg_close(afg_stream* s);

struct afg_flac_parsed
{
    uint sample_rate, channels, bps, max_block;
    ulong total_samples;
    ulong n_frames, n_subframes, n_res, out_samples;
    afg_flac_frame* frames;
    afg_flac_subframe* subframes;
    int* res;
    void* owner;
}
int afg_flac_parse(const(ubyte)* data, size_t length, afg_flac_parsed* parsed);
void afg_flac_parsed_free(afg_flac_parsed* parsed);
int afg_qoa_parse(const(ubyte)* data, size_t length, uint* channels, uint* samplerate, uint* samples,
                  afg_qoa_frame* frames, size_t frame_cap, size_t* n_frames);

struct afg_mp3_copy { ulong src_float, count; }
struct afg_mp3_parsed
{
    int channels, hz, tagged, start_delay;
    ulong detected_samples, declared_samples, pcm_samples;
    ulong n_runs, n_blocks, n_copies;
    uint* run_granules;
    float* coef;
    uint* flags;
    afg_mp3_copy* copies;
    void* owner;
}
int afg_mp3_parse(const(ubyte)* data, size_t length, afg_mp3_parsed* parsed);
void afg_mp3_parsed_free(afg_mp3_parsed* parsed);

struct afg_vorbis_parsed
{
    int channels, blocksize0, blocksize1;
    uint sample_rate, total_samples;
    ulong n_packets, spec_floats, pcm_frames;
    ubyte* pflags;
    float* spec;
    int* take_from;
    int* take_count;
    void* owner;
}
int afg_vorbis_parse(const(ubyte)* data, size_t length, afg_vorbis_parsed* parsed);
void afg_vorbis_parsed_free(afg_vorbis_parsed* parsed);
struct afg_vorbis_parsed_r
{
    afg_vorbis_parsed base;          // base.spec: residue vectors
    ulong n_curves, n_points, n_steps;
    afg_vorbis_floor_packet* packets;
    afg_vorbis_floor_curve* curves;
    int* points;
    ubyte* steps;
}
int afg_vorbis_parse_r(const(ubyte)* data, size_t length, afg_vorbis_parsed_r* parsed);
void afg_vorbis_parsed_r_free(afg_vorbis_parsed_r* parsed);

struct afg_opus_parsed
{
    int channels, preskip, gain_i, error;
    float gain;
    int pad;
    long declared_frames;
    ulong pcm_frames, n_frames, n_coeffs;
    afg_celt_frame* frames;
    float* coeffs;
    void* owner;
}
int afg_opus_parse(const(ubyte)* data, size_t length, afg_opus_parsed* parsed);
void afg_opus_parsed_free(afg_opus_parsed* parsed);

struct afg_batch_item
{
    int status;
    const(char)* message;
    int format;
    int channels;
    float samplerate;
    long frames;
    float* pcm;
}
struct afg_batch_result
{
    int n_files;
    afg_batch_item* items;
    void* owner;
}
int afg_batch_decode(const(ubyte*)* data, const(size_t)* length, int n_files, int n_threads, afg_batch_result* result);

// ---- round 2: device selection, multi-device batches, MP3 quantised upload, CELT on two streams, dithered WAV ----
enum uint AFG_SAMPLE_F32 = 0, AFG_SAMPLE_F64 = 1;   // AFG_SAMPLE_F64: an item's pcm points at frames * channels doubles (readSamplesDouble's)
// AFG_SAMPLE_PCM_*: an item's pcm points at frames * channels samples of 1, 2 or 3 bytes, the body of the WAV file that
// readSamplesFloat + writeSamplesFloat would write, packed on the device (afg_pcm_pack_hip); dither: AFG_DITHER_OFF or
// AFG_DITHER_LCG31 (every file from draw 0 of dither_seed), AFG_DITHER_LIBC is refused
enum uint AFG_SAMPLE_PCM_S8 = 2, AFG_SAMPLE_PCM_S16 = 3, AFG_SAMPLE_PCM_S24 = 4;
struct afg_batch_opts { uint struct_size; int n_threads; int n_devices; const(int)* devices; uint sample_type; int dither; uint dither_seed; }
int afg_set_device(int device);
int afg_get_device();
int afg_batch_decode_ex(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_batch_opts)* opts, afg_batch_result* result);
ulong afg_host_pool_trim();

enum uint AFG_MP3_NO_SDESC = 0xffffffffu;
struct afg_mp3_qgranule { ulong q_off; ulong coef_off; uint sdesc; ubyte nch; ubyte stereo; ubyte[2] table; float[40][2] scale; }
struct afg_mp3_sdesc { ubyte[40] type; float[40] fl; float[40] fr; }
static assert(afg_mp3_qgranule.sizeof == 344 && afg_mp3_sdesc.sizeof == 360);
int afg_mp3_requant_hip(ulong n_granules, const(afg_mp3_qgranule)* d_granules, const(short)* d_q,
                        const(afg_mp3_sdesc)* d_sdesc, float* d_coef, void* hip_stream);

struct afg_mp3_parsed_q
{
    afg_mp3_parsed base;             // base.coef is null
    ulong n_granules, n_sdesc;
    short* q;                        // n_blocks * 576 quantised lines
    afg_mp3_qgranule* granules;
    afg_mp3_sdesc* sdesc;
}
int afg_mp3_parse_q(const(ubyte)* data, size_t length, afg_mp3_parsed_q* parsed);
void afg_mp3_parsed_q_free(afg_mp3_parsed_q* parsed);
void afg_mp3_qtables(ubyte* band_of_line /* [24][576] */, ushort* dst_of_src /* [24][576] */, float* pow43 /* [145] */);
int afg_lds_fill_probe_hip(uint word, void* hip_stream);   // test aid: fills the LDS of every CU with `word`

// ProTracker MOD (afg.h): records of the device mixer, the host front-end, the module functions of AudioStream
enum AFG_MOD_MAX_FRAMES = 30 * 60 * 44100;
struct afg_mod_song { ulong out_frame, tick_base, seg_base, sample_base; uint n_ticks, sample_bytes; ulong reserved; }
struct afg_mod_tick { uint frame, frames, seg, n_seg; short pattern, line; uint pad; }
struct afg_mod_segment
{
    uint frame, frames;
    float position, increment, level_l, level_r;
    uint sample_off;
    int loop_start, loop_length, loop_end, length;
    uint channel;
}
struct afg_mod_parsed
{
    uint channels, capped;
    ulong n_frames, n_ticks, n_segments, n_sample_bytes;
    afg_mod_tick* ticks;
    afg_mod_segment* segments;
    ubyte* sample_bytes;
    void* owner;
}
int afg_mod_render_hip(uint n_songs, const(afg_mod_song)* d_songs, const(afg_mod_segment)* d_segments,
                       const(afg_mod_tick)* d_ticks, const(ubyte)* d_sample_bytes, float* d_out, void* hip_stream);
int afg_mod_parse(const(ubyte)* data, size_t length, afg_mod_parsed* parsed);
void afg_mod_parsed_free(afg_mod_parsed* parsed);
struct afg_xm_song { ulong out_frame, tick_base, seg_base, sample_base, aux_base; uint n_ticks, sample_bytes; ulong[2] reserved; }
struct afg_xm_tick { uint frame, frames, seg, n_seg; float scale; short table_index, row; uint loop_count, pad; }
struct afg_xm_segment
{
    uint frame, frames, sample_off, last, flags, channel;
    float position, step, vol_l, vol_r;
    uint aux_vol, aux_fade, aux_pos, fade_count;
    uint[2] pad;
}
struct afg_xm_parsed
{
    uint channels, capped, length, patterns, instruments, restart;
    ulong n_frames, n_ticks, n_segments, n_sample_bytes, n_aux;
    afg_xm_tick* ticks;
    afg_xm_segment* segments;
    ubyte* sample_bytes;
    float* aux;
    void* owner;
}
int afg_xm_render_hip(uint n_songs, const(afg_xm_song)* d_songs, const(afg_xm_segment)* d_segments,
                      const(afg_xm_tick)* d_ticks, const(ubyte)* d_sample_bytes, const(float)* d_aux, float* d_out,
                      void* hip_stream);
int afg_xm_parse(const(ubyte)* data, size_t length, afg_xm_parsed* parsed);
void afg_xm_parsed_free(afg_xm_parsed* parsed);
// WAV (afg.h): span records of the device conversion, the host front-end
enum { AFG_WAV_KIND_U8 = 0, AFG_WAV_KIND_S16 = 1, AFG_WAV_KIND_S24 = 2, AFG_WAV_KIND_S32 = 3, AFG_WAV_KIND_F32 = 4, AFG_WAV_KIND_F64 = 5 }
enum AFG_WAV_TILE_SAMPLES = 4096;
struct afg_wav_span { ulong in_off, out_off, count, tile_first; uint kind, pad; }
struct afg_wav_parsed
{
    uint tag, channels, bits, sample_rate, frames;
    int kind;
    ulong samples_offset, present_samples;
}
ulong afg_wav_layout(afg_wav_span* spans, ulong n_spans);
int afg_wav_convert_hip(ulong n_spans, const(afg_wav_span)* d_spans, ulong n_tiles, const(ubyte)* d_in, ulong in_bytes,
                        float* d_out, ulong out_floats, void* hip_stream);
enum uint AFG_F64_KIND_FLAC_S32 = 6;
int afg_pcm_to_f64_hip(ulong n_spans, const(afg_wav_span)* d_spans, ulong n_tiles, const(ubyte)* d_in, ulong in_bytes,
                       double* d_out, ulong out_doubles, void* hip_stream);
int afg_wav_parse(const(ubyte)* data, size_t length, afg_wav_parsed* parsed);
int afg_is_module(const(afg_stream)* s);
int afg_module_pattern_count(const(afg_stream)* s);
int afg_module_length(const(afg_stream)* s);
int afg_module_rows_in_pattern(const(afg_stream)* s, int pattern);
int afg_module_tell_pattern(const(afg_stream)* s);
int afg_module_tell_row(const(afg_stream)* s);
int afg_module_seek(afg_stream* s, int pattern, int row);
int afg_celt_transform_streams_hip(uint n_chan, const(ulong)* d_rec_base, const(afg_celt_frame)* d_recs, const(float)* d_coeffs,
                                   float* d_out, float* d_states, void* hip_stream, void* hip_tail_stream);
alias afg_rand_fn = extern(C) int function(void* user) nothrow @nogc;
ulong afg_wav_encode_dithered(const(float)* samples, ulong frames, uint channels, uint samplerate, int format,
                              afg_rand_fn rng, void* rng_user, uint rng_max, ubyte* outData, ulong cap);
void afg_batch_free(afg_batch_result* result);

/// Encode side: device WAV sample packing, the writing half of AudioStream, the batch encoder (afg.h has the contracts).
enum { AFG_DITHER_OFF = 0, AFG_DITHER_LIBC = 1, AFG_DITHER_LCG31 = 2 }
struct afg_wav_pack_span { ulong in_off, out_off, count, first_tile, draw0; uint seed; ubyte format, dither; ubyte[2] pad; }
uint afg_lcg31_jump(uint seed, ulong n_draws);
ulong afg_wav_pack_layout(afg_wav_pack_span* spans, ulong n_spans);
int afg_wav_pack_hip(ulong n_spans, const(afg_wav_pack_span)* d_spans, ulong n_tiles, const(float)* d_in, ulong in_floats,
                     ubyte* d_out, ulong out_bytes, void* hip_stream);
struct afg_encoding_options { uint struct_size; int sample_format; int dither; uint dither_seed; }
afg_stream* afg_open_to_buffer(int format, float samplerate, int channels, const(afg_encoding_options)* opts);
afg_stream* afg_open_to_memory(ubyte* data, size_t max_length, int format, float samplerate, int channels,
                               const(afg_encoding_options)* opts);
int afg_is_open_for_reading(const(afg_stream)* s);
int afg_is_open_for_writing(const(afg_stream)* s);
int afg_write_samples_float(afg_stream* s, const(float)* inData, int frames);
int afg_write_samples_double(afg_stream* s, const(double)* inData, int frames);
int afg_finalize_encoding(afg_stream* s);
int afg_finalize_and_get_encoded(afg_stream* s, const(ubyte)** bytes, size_t* length);
struct afg_encode_input { const(float)* pcm; ulong frames; uint channels; float samplerate; }
struct afg_encoded_item { int status; const(char)* message; ubyte* bytes; ulong size; }
struct afg_encode_result { int n_files; afg_encoded_item* items; void* owner; }
int afg_batch_encode(const(afg_encode_input)* inputs, int n_files, int format, const(afg_encoding_options)* opts, int n_threads,
                     afg_encode_result* result);
void afg_encode_free(afg_encode_result* result);
// the packer of the decode stages: afg_wav_pack_hip's integer formats for spans at any float / any byte; inputs are clamped to [-1, 1], NaN -> 0
struct afg_pcm_pack_span { ulong in_off, out_off, count, first_tile, draw0; uint seed; ubyte format, dither; ubyte[2] pad; }
ulong afg_pcm_pack_layout(afg_pcm_pack_span* spans, ulong n_spans);
int afg_pcm_pack_hip(ulong n_spans, const(afg_pcm_pack_span)* d_spans, ulong n_tiles, const(float)* d_in, ulong in_floats,
                     ubyte* d_out, ulong out_bytes, void* hip_stream);
// collate on the device: runs of interleaved floats to planar, padded rows (channels 0: `count` zeros from out_off + sample0 on)
struct afg_collate_span { ulong in_off, count, sample0, out_off; long first_frame; ulong first_tile; uint frames; ushort channels, out_channels; }
ulong afg_collate_layout(afg_collate_span* spans, ulong n_spans);
int afg_collate_hip(ulong n_spans, const(afg_collate_span)* d_spans, ulong n_tiles, const(float)* d_in, ulong in_floats,
                    float* d_out, ulong out_floats, void* hip_stream);
// batch decode into a [files, channels, frames] float tensor in device memory: the floats of readSamplesFloat, no download
struct afg_collate_opts { uint struct_size; int n_threads; uint channels; uint frames; const(long)* first_frame; }
int afg_batch_decode_to_device(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_collate_opts)* opts,
                               float* d_out, afg_batch_result* result);

// the tensor at one sample rate (afg.h has the filter's definition; the reference has no resampler)
ulong afg_resample_taps(uint in_rate, uint out_rate, uint lowpass_width, float* taps, ulong cap, uint* M, uint* L, uint* W);
struct afg_resample_row { ulong in_off, in_stride; long in_frame0; ulong out_off, first_tile, taps_off; uint in_rows, in_frames, out_frames, M, L, W; }
ulong afg_resample_layout(afg_resample_row* rows, ulong n_rows);
int afg_resample_hip(ulong n_rows, const(afg_resample_row)* d_rows, ulong n_tiles, const(float)* d_in, ulong in_floats,
                     const(float)* d_taps, ulong taps_floats, float* d_out, ulong out_floats, void* hip_stream);
struct afg_resample_opts { uint struct_size; int n_threads; uint channels; uint frames; const(long)* first_frame; uint samplerate, mono, in_channels, max_in_rate, lowpass_width; }
int afg_batch_decode_resampled(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_resample_opts)* opts,
                               float* d_out, afg_batch_result* result);

// mel spectrogram features behind it (afg.h has the definition; the reference has no such stage)
enum { AFG_MEL_PAD_REFLECT = 0, AFG_MEL_PAD_ZERO = 1 }
enum { AFG_MEL_POWER = 0, AFG_MEL_LOG10 = 1 }
enum { AFG_MEL_SCALE_SLANEY = 0, AFG_MEL_SCALE_HTK = 1 }
enum { AFG_MEL_NORM_NONE = 0, AFG_MEL_NORM_SLANEY = 1 }
struct afg_mel_params { uint n_fft, win_length, hop, n_mels, center, pad_mode, out_kind; float log_floor; }
struct afg_mel_row { ulong in_off, out_off, first_tile; uint in_frames, out_frames; }
ulong afg_mel_basis(uint n_fft, uint win_length, float* out_, ulong cap);
ulong afg_mel_filters(uint samplerate, uint n_fft, uint n_mels, double f_min, double f_max, uint scale, uint norm, float* out_, ulong cap);
uint afg_mel_frames(const(afg_mel_params)* params, uint in_frames);
ulong afg_mel_layout(afg_mel_row* rows, ulong n_rows, const(afg_mel_params)* params);
int afg_mel_check_rows(const(afg_mel_row)* rows, ulong n_rows, ulong n_tiles, const(afg_mel_params)* params, ulong in_floats,
                       ulong basis_floats, ulong filters_floats, ulong out_floats);
int afg_melspec_hip(ulong n_rows, const(afg_mel_row)* d_rows, ulong n_tiles, const(afg_mel_params)* params, const(float)* d_in,
                    ulong in_floats, const(float)* d_basis, ulong basis_floats, const(float)* d_filters, ulong filters_floats,
                    float* d_out, ulong out_floats, void* hip_stream);
// the same features through an FFT per frame (afg_mel_opts.algorithm, or the kernel-level entries below)
enum { AFG_MEL_ALGO_DIRECT = 0, AFG_MEL_ALGO_FFT = 1 }
ulong afg_mel_fft_tables(uint n_fft, uint win_length, float* out_, ulong cap);
ulong afg_mel_fft_layout(afg_mel_row* rows, ulong n_rows, const(afg_mel_params)* params);
int afg_mel_fft_check_rows(const(afg_mel_row)* rows, ulong n_rows, ulong n_tiles, const(afg_mel_params)* params, ulong in_floats,
                           ulong table_floats, ulong filters_floats, ulong out_floats);
int afg_melspec_fft_hip(ulong n_rows, const(afg_mel_row)* d_rows, ulong n_tiles, const(afg_mel_params)* params, const(float)* d_in,
                        ulong in_floats, const(float)* d_table, ulong table_floats, const(float)* d_filters, ulong filters_floats,
                        float* d_out, ulong out_floats, void* hip_stream);
struct afg_mel_opts { uint struct_size; int n_threads; uint channels; uint frames; const(long)* first_frame; uint samplerate, mono, in_channels, max_in_rate, lowpass_width, n_out; afg_mel_params mel; uint scale, norm; double f_min, f_max; uint algorithm, reserved; }
int afg_batch_decode_mel(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_mel_opts)* opts, float* d_out,
                         afg_batch_result* out_);
// normalisation: statistics per group of rows and the gain / offset they decide (include/afg.h has the definition)
enum : uint { AFG_NORM_NONE = 0, AFG_NORM_PEAK = 1, AFG_NORM_RMS = 2, AFG_NORM_STANDARD = 3, AFG_NORM_DYNAMIC_RANGE = 4 }
struct afg_norm_group { ulong in_off, out_off, stride, first_tile; uint rows, valid; uint[2] reserved; }
struct afg_norm_stats { double sum, sumsq; ulong count; float min, max, offset, scale; }
struct afg_norm_params { uint mode; float target, eps, range, shift, gain; }
ulong afg_norm_layout(afg_norm_group* groups, ulong n_groups);
int afg_norm_check_groups(const(afg_norm_group)* groups, ulong n_groups, ulong n_tiles, const(afg_norm_params)* params,
                          ulong in_floats, ulong out_floats);
int afg_normalize_hip(ulong n_groups, const(afg_norm_group)* d_groups, ulong n_tiles, const(afg_norm_params)* params,
                      const(float)* d_in, ulong in_floats, float* d_out, ulong out_floats, void* d_partials,
                      afg_norm_stats* d_stats, void* hip_stream);
int afg_batch_decode_resampled_norm(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_resample_opts)* opts,
                                    const(afg_norm_params)* norm, float* d_out, afg_norm_stats* d_stats, afg_batch_result* out_);
int afg_batch_decode_mel_norm(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_mel_opts)* opts,
                              const(afg_norm_params)* wave_norm, const(afg_norm_params)* feat_norm, float* d_out, afg_batch_result* out_);
// cepstral features behind the log-mel stage: a DCT-II over the mel axis with its lifter, and regression deltas (include/afg.h
// has the definition)
enum : uint { AFG_CEP_DCT_NONE = 0, AFG_CEP_DCT_ORTHO = 1 }
enum : uint { AFG_CEP_TILE = 64 }
struct afg_cep_params { uint n_mels, n_ceps, delta_order, delta_win; uint[4] reserved; }
struct afg_cep_row { ulong in_off, out_off, first_tile; uint frames, reserved; }
struct afg_mfcc_opts { uint struct_size, dct_norm; afg_mel_opts mel; afg_cep_params cep; double lifter, log_scale; }
ulong afg_cep_dct(uint n_ceps, uint n_mels, uint norm, double lifter, double log_scale, float* out_, ulong cap);
ulong afg_cep_layout(afg_cep_row* rows, ulong n_rows, const(afg_cep_params)* params);
int afg_cep_check_rows(const(afg_cep_row)* rows, ulong n_rows, ulong n_tiles, const(afg_cep_params)* params, ulong in_floats,
                       ulong dct_floats, ulong out_floats);
int afg_cepstra_hip(ulong n_rows, const(afg_cep_row)* d_rows, ulong n_tiles, const(afg_cep_params)* params, const(float)* d_in,
                    ulong in_floats, const(float)* d_dct, ulong dct_floats, float* d_out, ulong out_floats, void* hip_stream);
int afg_batch_decode_mfcc(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_mfcc_opts)* opts,
                          const(afg_norm_params)* wave_norm, const(afg_norm_params)* cmvn, float* d_out, afg_batch_result* out_);
// trimming silence: the non-silent region of a group of rows, and the rows shifted to start there (include/afg.h has the
// definition)
enum : uint { AFG_TRIM_REF_MAX = 0, AFG_TRIM_REF_ABS = 1 }
struct afg_trim_params { uint frame_length, hop, reference, lead, trail; uint[3] reserved; double ratio, abs_power; }
struct afg_trim_group { ulong in_off, out_off, in_stride, out_stride, first_block, first_tile; uint rows, valid, out_rows, out_frames; }
struct afg_trim_region { uint begin, end; double ref_power; }
int afg_trim_layout(afg_trim_group* groups, ulong n_groups, const(afg_trim_params)* params, ulong* n_blocks, ulong* n_tiles);
int afg_trim_check_groups(const(afg_trim_group)* groups, ulong n_groups, ulong n_blocks, ulong n_tiles,
                          const(afg_trim_params)* params, ulong in_floats, ulong out_floats);
int afg_trim_hip(ulong n_groups, const(afg_trim_group)* d_groups, ulong n_blocks, ulong n_tiles, const(afg_trim_params)* params,
                 const(float)* d_in, ulong in_floats, float* d_out, ulong out_floats, double* d_blocks, afg_trim_region* d_regions,
                 void* hip_stream);
int afg_batch_decode_trimmed(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_resample_opts)* opts,
                             const(afg_trim_params)* trim, uint scan_frames, float* d_out, afg_trim_region* regions,
                             afg_batch_result* out_);
// the linear-frequency spectrogram: the FFT mel path's transform delivered as complex, magnitude, power or log10 power
// (include/afg.h has the definition); rows are afg_mel_row, the table is afg_mel_fft_tables'
enum : uint { AFG_STFT_COMPLEX = 0, AFG_STFT_MAGNITUDE = 1, AFG_STFT_POWER = 2, AFG_STFT_LOG10 = 3 }
struct afg_stft_params { uint n_fft, win_length, hop, center, pad_mode, out_kind; float log_floor; uint reserved; }
struct afg_stft_opts { uint struct_size; int n_threads; uint channels; uint frames; const(long)* first_frame; uint samplerate, mono, in_channels, max_in_rate, lowpass_width, n_out; afg_stft_params stft; uint reserved; }
uint afg_stft_tile_frames(const(afg_stft_params)* params);
ulong afg_stft_layout(afg_mel_row* rows, ulong n_rows, const(afg_stft_params)* params);
int afg_stft_check_rows(const(afg_mel_row)* rows, ulong n_rows, ulong n_tiles, const(afg_stft_params)* params, ulong in_floats,
                        ulong table_floats, ulong out_floats);
int afg_stft_hip(ulong n_rows, const(afg_mel_row)* d_rows, ulong n_tiles, const(afg_stft_params)* params, const(float)* d_in,
                 ulong in_floats, const(float)* d_table, ulong table_floats, float* d_out, ulong out_floats, void* hip_stream);
int afg_batch_decode_stft(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_stft_opts)* opts, float* d_out,
                          afg_batch_result* out_);
// filtering: cascades of second-order recursive sections over float rows, computed in float64 (include/afg.h has the
// definition, the interval the result is held to and its constant AFG_FILTER_K)
enum : uint { AFG_FILTER_MAX_SECTIONS = 8, AFG_FILTER_TILE = 4096, AFG_FILTER_CHUNK = 16, AFG_FILTER_K = 64 }
enum : uint { AFG_BIQUAD_LOWPASS = 0, AFG_BIQUAD_HIGHPASS = 1, AFG_BIQUAD_BANDPASS = 2, AFG_BIQUAD_NOTCH = 3, AFG_BIQUAD_ALLPASS = 4,
              AFG_BIQUAD_PEAKING = 5, AFG_BIQUAD_LOWSHELF = 6, AFG_BIQUAD_HIGHSHELF = 7, AFG_BIQUAD_PREEMPHASIS = 8, AFG_BIQUAD_DC_BLOCK = 9 }
struct afg_biquad { double b0, b1, b2, a1, a2; }
struct afg_filter_params { uint n_sections; afg_biquad[8] sec; }
struct afg_filter_row { ulong in_off, out_off; uint frames, reserved; }
int afg_biquad_design(uint kind, double samplerate, double f0, double q, double gain_db, afg_biquad* out_);
double afg_filter_bound(const(afg_filter_params)* params);
uint afg_filter_tile_frames();
int afg_filter_check_rows(const(afg_filter_row)* rows, ulong n_rows, const(afg_filter_params)* params, ulong in_floats,
                          ulong out_floats, int same_plane);
int afg_filter_hip(ulong n_rows, const(afg_filter_row)* d_rows, const(afg_filter_params)* params, const(float)* d_in,
                   ulong in_floats, float* d_out, ulong out_floats, double* d_state, void* hip_stream);
int afg_batch_decode_filtered(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_resample_opts)* opts,
                              const(afg_filter_params)* filter, float* d_out, afg_batch_result* out_);
// loudness: integrated loudness after ITU-R BS.1770-4 per group of rows and the gain to a target (include/afg.h has the
// definition, the interval the block energies are held to and its constant AFG_LOUDNESS_K)
enum : uint { AFG_LOUDNESS_K = 64, AFG_LOUDNESS_UNGATED = 1, AFG_LOUDNESS_GAIN_CLAMPED = 2, AFG_LOUDNESS_PEAK_CLAMPED = 4 }
struct afg_loudness_params { uint samplerate, apply; double target_lufs; float max_peak, max_gain; double[8] weights; uint[2] reserved; }
struct afg_loudness_group { ulong in_off, out_off, stride, first_sub, first_block; uint rows, valid; uint[4] reserved; }
struct afg_loudness_counts { ulong n_sub, n_blocks; }
struct afg_loudness_stats { double energy, rel_threshold; uint n_blocks, n_abs, n_gated, flags; float peak, gain; }
int afg_kweight_design(uint samplerate, afg_filter_params* out_);
double afg_loudness_lufs(double energy);
int afg_loudness_layout(afg_loudness_group* groups, ulong n_groups, const(afg_loudness_params)* params, afg_loudness_counts* counts);
int afg_loudness_check_groups(const(afg_loudness_group)* groups, ulong n_groups, const(afg_loudness_counts)* counts,
                              const(afg_loudness_params)* params, ulong in_floats, ulong out_floats, int same_plane);
int afg_loudness_hip(ulong n_groups, const(afg_loudness_group)* d_groups, const(afg_loudness_counts)* counts,
                     const(afg_loudness_params)* params, const(float)* d_in, ulong in_floats, float* d_out, ulong out_floats,
                     double* d_sub, double* d_blocks, afg_loudness_stats* d_stats, void* hip_stream);
int afg_batch_decode_loudnorm(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_resample_opts)* opts,
                              const(afg_loudness_params)* loudness, float* d_out, afg_loudness_stats* stats, afg_batch_result* out_);
// the inverse of the linear spectrogram: AFG_STFT_COMPLEX's layout back to samples, overlap-add over the window envelope
// (include/afg.h has the definition and the bound); the table is afg_mel_fft_tables'
struct afg_istft_params { uint n_fft, win_length, hop, center; uint[4] reserved; }
struct afg_istft_row { ulong in_off, out_off, first_tile; uint n_frames, in_pitch, out_first, out_frames; }
uint afg_istft_tile_samples(const(afg_istft_params)* params);
ulong afg_istft_layout(afg_istft_row* rows, ulong n_rows, const(afg_istft_params)* params);
double afg_istft_envelope_min(const(afg_istft_params)* params, uint n_frames, uint out_first, uint out_frames);
int afg_istft_check_rows(const(afg_istft_row)* rows, ulong n_rows, ulong n_tiles, const(afg_istft_params)* params, ulong in_floats,
                         ulong table_floats, ulong out_floats);
int afg_istft_hip(ulong n_rows, const(afg_istft_row)* d_rows, ulong n_tiles, const(afg_istft_params)* params, const(float)* d_in,
                  ulong in_floats, const(float)* d_table, ulong table_floats, float* d_out, ulong out_floats, void* hip_stream);
// the phase-vocoder time stretch between afg_stft_hip and afg_istft_hip: AFG_STFT_COMPLEX's layout in and out, a rate per
// slab, the phase summed in double (include/afg.h has the definition, the interval and the constants)
enum AFG_PVOC_KA = 2, AFG_PVOC_KP = 52, AFG_PVOC_CHUNK = 4, AFG_PVOC_TILE = 256;
struct afg_pvoc_params { uint n_fft, hop; uint[6] reserved; }
struct afg_pvoc_row { ulong in_off, out_off; double rate; uint n_frames, in_pitch, out_frames, out_pitch; uint[2] reserved; }
uint afg_pvoc_out_frames(uint n_frames, double rate);
double afg_pvoc_bound(const(afg_pvoc_params)* params, ulong t);
int afg_pvoc_check_rows(const(afg_pvoc_row)* rows, ulong n_rows, const(afg_pvoc_params)* params, ulong in_floats, ulong out_floats);
int afg_pvoc_hip(ulong n_rows, const(afg_pvoc_row)* d_rows, const(afg_pvoc_params)* params, const(float)* d_in, ulong in_floats,
                 float* d_out, ulong out_floats, void* hip_stream);
// convolution of waveform rows with the kernels of a bank: a direct path for kernels of at most direct_max taps (bits), a
// partitioned overlap-save FFT path for the rest (an interval); include/afg.h has the definition, the bound and the checks
enum AFG_CONV_BLOCK = 1024, AFG_CONV_MAX_TAPS = 65536, AFG_CONV_DIRECT_MAX = 128, AFG_CONV_DIRECT_TILE = 4096,
     AFG_CONV_TABLE_FLOATS = 4096, AFG_CONV_SPEC_FLOATS = 2050;
struct afg_convolve_params { uint direct_max; uint[7] reserved; }
struct afg_convolve_kernel { ulong bank_off, spec_off; uint taps, reserved; }
struct afg_convolve_row { ulong in_off, out_off, first_tile, work_off; uint frames, kernel, out_first, out_frames; }
ulong afg_convolve_bank_layout(afg_convolve_kernel* kernels, ulong n_kernels);
int afg_convolve_bank_check(const(afg_convolve_kernel)* kernels, ulong n_kernels, ulong bank_floats, ulong spec_floats);
int afg_convolve_bank_hip(ulong n_kernels, const(afg_convolve_kernel)* d_kernels, const(float)* d_bank, ulong bank_floats, float* d_spec,
                          ulong spec_floats, void* hip_stream);
ulong afg_convolve_layout(afg_convolve_row* rows, ulong n_rows, const(afg_convolve_kernel)* kernels, ulong n_kernels,
                          const(afg_convolve_params)* params, ulong* work_floats);
double afg_convolve_bound(const(afg_convolve_params)* params, uint taps);
int afg_convolve_check_rows(const(afg_convolve_row)* rows, ulong n_rows, ulong n_tiles, const(afg_convolve_kernel)* kernels, ulong n_kernels,
                            const(afg_convolve_params)* params, ulong in_floats, ulong bank_floats, ulong spec_floats, ulong work_floats,
                            ulong out_floats, const(ulong)* plane_at);
int afg_convolve_hip(ulong n_rows, const(afg_convolve_row)* d_rows, ulong n_tiles, const(afg_convolve_kernel)* d_kernels, ulong n_kernels,
                     const(afg_convolve_params)* params, const(float)* d_in, ulong in_floats, const(float)* d_bank, ulong bank_floats,
                     const(float)* d_spec, ulong spec_floats, float* d_work, ulong work_floats, float* d_out, ulong out_floats,
                     void* hip_stream);
// mixing: noise from a bank of clips added to groups of rows at a signal-to-noise ratio (include/afg.h has the definition)
enum : uint { AFG_MIX_SNR = 0, AFG_MIX_GAIN = 1 }
enum : uint { AFG_MIX_SILENT_SIGNAL = 1, AFG_MIX_SILENT_NOISE = 2, AFG_MIX_ENERGY_NOT_FINITE = 4, AFG_MIX_GAIN_NOT_FINITE = 8 }
struct afg_mix_group { ulong in_off, out_off, stride, first_tile, noise_off, noise_stride; double ratio; uint rows, valid, noise_len, noise_start, flags; float gain; }
static assert(afg_mix_group.sizeof == 80);
struct afg_mix_stats { double signal_energy, noise_energy; float gain; uint flags; }
struct afg_mix_noise { const(float)* d_noise; ulong n_clips; uint clip_pitch, clip_rows; const(uint)* lengths; const(uint)* index; const(ulong)* start; const(double)* snr_db; }
double afg_mix_ratio(double snr_db);
ulong afg_mix_layout(afg_mix_group* groups, ulong n_groups);
int afg_mix_check_groups(const(afg_mix_group)* groups, ulong n_groups, ulong n_tiles, ulong in_floats, ulong noise_floats,
                         ulong out_floats, const(ulong)* plane_at);
int afg_mix_hip(ulong n_groups, const(afg_mix_group)* d_groups, ulong n_tiles, const(float)* d_in, ulong in_floats,
                const(float)* d_noise, ulong noise_floats, float* d_out, ulong out_floats, void* d_partials, afg_mix_stats* d_stats,
                void* hip_stream);
int afg_batch_decode_mixed(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_resample_opts)* opts,
                           const(afg_mix_noise)* noise, float* d_out, afg_mix_stats* stats, afg_batch_result* out_);
// Kaldi-compatible filter-bank features: snip_edges or mirrored frames, DC removal, pre-emphasis, Povey's window, a bank on the
// mel axis, natural log, an optional energy column (include/afg.h has the definition and the bound); rows are afg_mel_row
enum : uint { AFG_FBANK_FRAMES_MAJOR = 0, AFG_FBANK_MEL_MAJOR = 1 }
enum : uint { AFG_FBANK_WINDOW_POVEY = 0, AFG_FBANK_WINDOW_HAMMING = 1, AFG_FBANK_WINDOW_HANNING = 2, AFG_FBANK_WINDOW_BLACKMAN = 3, AFG_FBANK_WINDOW_RECTANGULAR = 4 }
struct afg_fbank_params { uint win_length, hop, n_fft, n_mels, snip_edges, remove_dc, use_power, use_log, use_energy, raw_energy, htk_compat, layout; float preemph, energy_floor, scale; uint reserved; }
struct afg_fbank_opts { uint struct_size; int n_threads; uint channels; uint frames; const(long)* first_frame; uint samplerate, mono, in_channels, max_in_rate, lowpass_width, n_out; afg_fbank_params fbank; uint window_type; double low_freq, high_freq, blackman_coeff; uint reserved; }
uint afg_fbank_n_fft(uint win_length, uint round_pow2);
uint afg_fbank_frames(const(afg_fbank_params)* params, uint in_frames);
ulong afg_fbank_tables(uint window_type, uint win_length, uint n_fft, double blackman_coeff, float* out_, ulong cap);
ulong afg_fbank_filters(uint samplerate, uint n_fft, uint n_mels, double low_freq, double high_freq, float* out_, ulong cap);
ulong afg_fbank_layout(afg_mel_row* rows, ulong n_rows, const(afg_fbank_params)* params);
int afg_fbank_check_rows(const(afg_mel_row)* rows, ulong n_rows, ulong n_tiles, const(afg_fbank_params)* params, ulong in_floats,
                         ulong table_floats, ulong filters_floats, ulong out_floats);
int afg_fbank_hip(ulong n_rows, const(afg_mel_row)* d_rows, ulong n_tiles, const(afg_fbank_params)* params, const(float)* d_in,
                  ulong in_floats, const(float)* d_table, ulong table_floats, const(float)* d_filters, ulong filters_floats,
                  float* d_out, ulong out_floats, void* hip_stream);
int afg_batch_decode_fbank(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_fbank_opts)* opts, float* d_out,
                           uint* n_frames, afg_batch_result* out_);
// YIN pitch per frame: f0 and d' at the chosen lag, two planes per row (include/afg.h has the definition); rows are afg_mel_row
enum : uint { AFG_YIN_CHUNK = 16, AFG_YIN_TILE = 4 }
struct afg_yin_params { uint frame_length, win_length, hop, tau_min, tau_max, center, pad_mode; float threshold; double samplerate; uint[2] reserved; }
struct afg_pitch_opts { uint struct_size; int n_threads; uint channels; uint frames; const(long)* first_frame; uint samplerate, mono, in_channels, max_in_rate, lowpass_width, n_out; afg_yin_params yin; uint reserved; }
int afg_yin_lags(double samplerate, double fmin, double fmax, uint frame_length, uint win_length, uint* tau_min, uint* tau_max);
uint afg_yin_frames(const(afg_yin_params)* params, uint in_frames);
ulong afg_yin_layout(afg_mel_row* rows, ulong n_rows, const(afg_yin_params)* params);
int afg_yin_hip(ulong n_rows, const(afg_mel_row)* d_rows, ulong n_tiles, const(afg_yin_params)* params, const(float)* d_in,
                ulong in_floats, float* d_out, ulong out_floats, void* hip_stream);
int afg_batch_decode_pitch(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_pitch_opts)* opts, float* d_out,
                           uint* n_frames, afg_batch_result* out_);
// sliding-window mean and variance normalisation of feature slabs, Kaldi's window (include/afg.h has the definition)
enum : uint { AFG_CMN_FRAMES_MAJOR = 0, AFG_CMN_COL_MAJOR = 1, AFG_CMN_CHUNK = 32, AFG_CMN_MAX_WINDOW = 1048576, AFG_CMN_MAX_COLS = 1024 }
struct afg_cmn_params { uint cmn_window, min_cmn_window, center, norm_vars, cols, layout; uint[2] reserved; }
struct afg_cmn_slab { ulong in_off, out_off, pitch, first_tile; uint n_frames; uint[3] reserved; }
ulong afg_cmn_layout(afg_cmn_slab* slabs, ulong n_slabs);
ulong afg_cmn_work_bytes(ulong n_tiles, uint cols);
int afg_cmn_check_slabs(const(afg_cmn_slab)* slabs, ulong n_slabs, ulong n_tiles, const(afg_cmn_params)* params, ulong in_floats,
                        ulong out_floats, int same_plane);
int afg_slide_cmn_hip(ulong n_slabs, const(afg_cmn_slab)* d_slabs, ulong n_tiles, const(afg_cmn_params)* params, const(float)* d_in,
                      ulong in_floats, float* d_out, ulong out_floats, void* d_work, ulong work_bytes, void* hip_stream);
int afg_batch_decode_fbank_cmn(const(ubyte*)* data, const(size_t)* length, int n_files, const(afg_fbank_opts)* opts,
                               const(afg_cmn_params)* cmn, float* d_out, uint* n_frames, afg_batch_result* out_);
// the `transcode` example for a batch: every item is a complete WAV file (out_format AFG_FORMAT_WAV; AFG_FORMAT_QOA is refused)
int afg_batch_transcode(const(ubyte*)* data, const(size_t)* length, int n_files, int out_format, const(afg_encoding_options)* enc,
                        const(afg_batch_opts)* opts, afg_encode_result* result);

/// Drop-in for the decoding use of `AudioStream` (stream.d:102): same member names and error-state contract
/// (never throws, `isError` + `errorMessage`), backed by the device library.  Not thread-safe per instance,
/// like the original (stream.d:31-33).
struct GpuAudioStream
{
nothrow @nogc:
    private afg_stream* _h;

    @disable this(this);
    ~this() { cleanUp(); }

    void openFromMemory(const(ubyte)[] inputData)
    {
        cleanUp();
        _h = afg_open_from_memory(inputData.ptr, inputData.length);
    }
    /// The writing half (stream.d:216-286, :762-902, :1282-1349): WAV and QOA.
    void openToBuffer(afg_format format, float sampleRate, int numChannels, const(afg_encoding_options)* options = null)
    {
        cleanUp();
        _h = afg_open_to_buffer(format, sampleRate, numChannels, options);
    }
    void openToMemory(ubyte* data, size_t maxLength, afg_format format, float sampleRate, int numChannels,
                      const(afg_encoding_options)* options = null)
    {
        cleanUp();
        _h = afg_open_to_memory(data, maxLength, format, sampleRate, numChannels, options);
    }
    bool isOpenForReading() { return afg_is_open_for_reading(_h) != 0; }
    bool isOpenForWriting() { return afg_is_open_for_writing(_h) != 0; }
    int writeSamplesFloat(const(float)* inData, int frames) { return afg_write_samples_float(_h, inData, frames); }
    int writeSamplesDouble(const(double)* inData, int frames) { return afg_write_samples_double(_h, inData, frames); }
    bool finalizeEncoding() { return afg_finalize_encoding(_h) != 0; }
    const(ubyte)[] finalizeAndGetEncodedResult()
    {
        const(ubyte)* p;
        size_t n;
        return afg_finalize_and_get_encoded(_h, &p, &n) ? p[0 .. n] : null;
    }
    void cleanUp() { if (_h !is null) { afg_close(_h); _h = null; } }

    bool isError() { return afg_is_error(_h) != 0; }
    bool isValid() { return !isError(); }
    const(char)[] errorMessage()
    {
        import core.stdc.string : strlen;
        const(char)* m = afg_error_message(_h);
        return m is null ? null : m[0 .. strlen(m)];
    }
    afg_format getFormat() { return cast(afg_format) afg_get_format(_h); }
    int getNumChannels() { return afg_get_num_channels(_h); }
    long getLengthInFrames() { return afg_get_length_in_frames(_h); }
    float getSamplerate() { return afg_get_samplerate(_h); }
    bool canSeek() { return afg_can_seek(_h) != 0; }
    bool seekPosition(int frame) { return afg_seek_position(_h, frame) != 0; }
    int tellPosition() { return afg_tell_position(_h); }
    bool isModule() { return afg_is_module(_h) != 0; }
    int countModulePatterns() { return afg_module_pattern_count(_h); }
    int getModuleLength() { return afg_module_length(_h); }
    int rowsInPattern(int pattern) { return afg_module_rows_in_pattern(_h, pattern); }
    int tellModulePattern() { return afg_module_tell_pattern(_h); }
    int tellModuleRow() { return afg_module_tell_row(_h); }
    bool seekPosition(int pattern, int row) { return afg_module_seek(_h, pattern, row) != 0; }
    int readSamplesFloat(float* outData, int frames) { return afg_read_samples_float(_h, outData, frames); }
    int readSamplesFloat(float[] outData)
    {
        const int ch = getNumChannels();
        return ch > 0 ? readSamplesFloat(outData.ptr, cast(int)(outData.length / ch)) : 0;
    }
    int readSamplesDouble(double* outData, int frames) { return afg_read_samples_double(_h, outData, frames); }
    int readSamplesDouble(double[] outData)
    {
        const int ch = getNumChannels();
        return ch > 0 ? readSamplesDouble(outData.ptr, cast(int)(outData.length / ch)) : 0;
    }
}
