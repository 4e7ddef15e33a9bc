"""afgpu -- Python host binding of the MI355X audio-decode transform path.

Thin ctypes view of ``audio-formats_amd/lib/libafg_hip.so`` (the C ABI declared in
``include/afg.h``).  PyTorch is used only as plumbing (device memory, streams,
``torch.distributed``); tensors cross the boundary as raw device pointers.

There is no CPU fallback: if the library or a gfx950 device is missing, every
entry point raises ``AfgError``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("AFG_LIB_PATH", os.path.join(PKG_ROOT, "lib", "libafg_hip.so"))   # override: A/B builds only

MP3_STATE_FLOATS = 1536
VORBIS_LONG, VORBIS_PREV, VORBIS_NEXT = 1, 2, 4


def VORBIS_NZ_EIGHTHS(e):
    """afg.h AFG_VORBIS_NZ_EIGHTHS: a long packet's declaration that only its first e eighths may be nonzero."""
    return (int(e) + 1) << 4

FLAC_INDEPENDENT, FLAC_LEFT_SIDE, FLAC_RIGHT_SIDE, FLAC_MID_SIDE = 0, 8, 9, 10

FLAC_SUBFRAME_DTYPE = np.dtype([("coef", np.int16, (32,)), ("order", np.uint8), ("shift", np.uint8),
                                ("wasted", np.uint8), ("use64", np.uint8)], align=True)
VORBIS_FLOOR_PACKET_DTYPE = np.dtype([("spec_off", np.uint64), ("n2", np.uint32), ("channels", np.uint32), ("curve_index", np.uint32),
                                      ("step_off", np.uint32), ("n_steps", np.uint32), ("pad", np.uint32)])
VORBIS_FLOOR_CURVE_DTYPE = np.dtype([("point_off", np.uint32), ("n_points", np.uint32)])
FLAC_FRAME_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("block_size", np.uint32),
                             ("sf_index", np.uint32), ("channels", np.uint8), ("assignment", np.uint8),
                             ("bps", np.uint8), ("res16", np.uint8), ("pad", np.uint8, (4,))], align=True)
assert FLAC_SUBFRAME_DTYPE.itemsize == 68 and FLAC_FRAME_DTYPE.itemsize == 32
CELT_FRAME_DTYPE = np.dtype([("coef_off", np.uint64), ("out_off", np.uint64), ("out_stride", np.uint32),
                             ("frame_size", np.uint16), ("blocks", np.uint8), ("pad", np.uint8),
                             ("pf_period_new", np.int32), ("pf_gains_new", np.float32, (3,)),
                             ("imdct_scale", np.float32), ("pad2", np.uint32)], align=True)
assert CELT_FRAME_DTYPE.itemsize == 48
CELT_STATE_FLOATS = 2064
QOA_FRAME_DTYPE = np.dtype([("byte_off", np.uint64), ("out_off", np.uint64), ("samples", np.uint16),
                            ("channels", np.uint8), ("pad", np.uint8, (5,))], align=True)
assert QOA_FRAME_DTYPE.itemsize == 24
QOA_ENC_STREAM_DTYPE = np.dtype([("pcm_off", np.uint64), ("out_off", np.uint64), ("samples", np.uint32),
                                 ("samplerate", np.uint32), ("channels", np.uint8), ("pad", np.uint8, 7)])
assert QOA_ENC_STREAM_DTYPE.itemsize == 32
WAV_S8, WAV_S16LE, WAV_S24LE, WAV_FP32LE, WAV_FP64LE = range(5)
WAV_FORMAT_BYTES = (1, 2, 3, 4, 8)
DITHER_OFF, DITHER_LIBC, DITHER_LCG31 = range(3)
WAV_PACK_SPAN_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("count", np.uint64), ("first_tile", np.uint64),
                                ("draw0", np.uint64), ("seed", np.uint32), ("format", np.uint8), ("dither", np.uint8),
                                ("pad", np.uint8, (2,))])
assert WAV_PACK_SPAN_DTYPE.itemsize == 48
PCM_PACK_SPAN_DTYPE = WAV_PACK_SPAN_DTYPE        # afg_pcm_pack_span: the same fields; in_off and out_off are free, format <= WAV_S24LE
# afg_collate_span: a run of interleaved samples to planar rows (channels 0: a run of zeros from out_off + sample0 on)
COLLATE_SPAN_DTYPE = np.dtype([("in_off", np.uint64), ("count", np.uint64), ("sample0", np.uint64), ("out_off", np.uint64),
                               ("first_frame", np.int64), ("first_tile", np.uint64), ("frames", np.uint32), ("channels", np.uint16),
                               ("out_channels", np.uint16)])
assert COLLATE_SPAN_DTYPE.itemsize == 56
# afg_resample_row: one output row of afg_resample_hip (in_frames 0: a row of zeros)
RESAMPLE_ROW_DTYPE = np.dtype([("in_off", np.uint64), ("in_stride", np.uint64), ("in_frame0", np.int64), ("out_off", np.uint64),
                               ("first_tile", np.uint64), ("taps_off", np.uint64), ("in_rows", np.uint32), ("in_frames", np.uint32),
                               ("out_frames", np.uint32), ("M", np.uint32), ("L", np.uint32), ("W", np.uint32)])
assert RESAMPLE_ROW_DTYPE.itemsize == 72
# afg_mel_row: one input row of afg_melspec_hip and its [n_mels, out_frames] output
MEL_ROW_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("first_tile", np.uint64), ("in_frames", np.uint32),
                          ("out_frames", np.uint32)])
assert MEL_ROW_DTYPE.itemsize == 32
MEL_PAD_REFLECT, MEL_PAD_ZERO = 0, 1             # afg_mel_params.pad_mode
MEL_POWER, MEL_LOG10 = 0, 1                      # afg_mel_params.out_kind
MEL_ALGO_DIRECT, MEL_ALGO_FFT = 0, 1             # afg_mel_opts.algorithm
MEL_SCALE_SLANEY, MEL_SCALE_HTK = 0, 1
MEL_NORM_NONE, MEL_NORM_SLANEY = 0, 1
NORM_NONE, NORM_PEAK, NORM_RMS, NORM_STANDARD, NORM_DYNAMIC_RANGE = range(5)     # afg_norm_params.mode
NORM_MODE_NAMES = {"none": NORM_NONE, "peak": NORM_PEAK, "rms": NORM_RMS, "standard": NORM_STANDARD, "dynamic_range": NORM_DYNAMIC_RANGE}
NORM_TILE = 4096                                 # floats of one row per tile of afg_normalize_hip
CEP_DCT_NONE, CEP_DCT_ORTHO = 0, 1               # afg_cep_dct's norm, afg_mfcc_opts.dct_norm
CEP_DCT_NAMES = {"none": CEP_DCT_NONE, "ortho": CEP_DCT_ORTHO}
CEP_TILE = 64                                    # frames of one record per tile of afg_cepstra_hip
TRIM_REF_MAX, TRIM_REF_ABS = 0, 1                # afg_trim_params.reference
TRIM_REF_NAMES = {"max": TRIM_REF_MAX, "abs": TRIM_REF_ABS}
TRIM_TILE = 4096                                 # floats of one output row per tile of afg_trim_hip
FILTER_TILE, FILTER_CHUNK, FILTER_K, FILTER_MAX_SECTIONS = 4096, 16, 64, 8     # afg_filter_hip: AFG_FILTER_*
BIQUAD_KINDS = {"lowpass": 0, "highpass": 1, "bandpass": 2, "notch": 3, "allpass": 4, "peaking": 5, "lowshelf": 6, "highshelf": 7,
                "preemphasis": 8, "dc_block": 9}                                  # AFG_BIQUAD_*
# afg_filter_row: one row of afg_filter_hip
FILTER_ROW_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("frames", np.uint32), ("reserved", np.uint32)])
assert FILTER_ROW_DTYPE.itemsize == 24
STFT_COMPLEX, STFT_MAGNITUDE, STFT_POWER, STFT_LOG10 = 0, 1, 2, 3       # afg_stft_params.out_kind
# afg_istft_row: one [n_bins, n_frames] slab of (re, im) pairs of afg_istft_hip and its out_frames samples
ISTFT_ROW_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("first_tile", np.uint64), ("n_frames", np.uint32),
                            ("in_pitch", np.uint32), ("out_first", np.uint32), ("out_frames", np.uint32)])
assert ISTFT_ROW_DTYPE.itemsize == 40
# afg_pvoc_row: one [n_bins, n_frames] slab of (re, im) pairs of afg_pvoc_hip and the [n_bins, out_frames] slab it makes
PVOC_ROW_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("rate", np.float64), ("n_frames", np.uint32),
                           ("in_pitch", np.uint32), ("out_frames", np.uint32), ("out_pitch", np.uint32), ("reserved", np.uint32, (2,))])
assert PVOC_ROW_DTYPE.itemsize == 48
PVOC_KA, PVOC_KP, PVOC_CHUNK, PVOC_TILE = 2, 52, 4, 256      # AFG_PVOC_*
# afg_convolve_kernel: one kernel of a bank; afg_convolve_row: one row, one kernel and the range of their line (afg_convolve_hip)
CONV_KERNEL_DTYPE = np.dtype([("bank_off", np.uint64), ("spec_off", np.uint64), ("taps", np.uint32), ("reserved", np.uint32)])
CONV_ROW_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("first_tile", np.uint64), ("work_off", np.uint64),
                           ("frames", np.uint32), ("kernel", np.uint32), ("out_first", np.uint32), ("out_frames", np.uint32)])
assert CONV_KERNEL_DTYPE.itemsize == 24 and CONV_ROW_DTYPE.itemsize == 48
CONV_BLOCK, CONV_MAX_TAPS, CONV_DIRECT_MAX, CONV_DIRECT_TILE, CONV_TABLE_FLOATS, CONV_SPEC_FLOATS = 1024, 65536, 128, 4096, 4096, 2050   # AFG_CONV_*
LOUDNESS_K = 64                                  # AFG_LOUDNESS_K
LOUDNESS_UNGATED, LOUDNESS_GAIN_CLAMPED, LOUDNESS_PEAK_CLAMPED = 1, 2, 4     # afg_loudness_stats.flags
MIX_SNR, MIX_GAIN = 0, 1                         # afg_mix_group.flags
MIX_SILENT_SIGNAL, MIX_SILENT_NOISE, MIX_ENERGY_NOT_FINITE, MIX_GAIN_NOT_FINITE = 1, 2, 4, 8   # afg_mix_stats.flags
MIX_TILE = 4096                                  # floats of one row per tile of afg_mix_hip
FBANK_FRAMES_MAJOR, FBANK_MEL_MAJOR = 0, 1       # afg_fbank_params.layout
FBANK_WINDOW_POVEY, FBANK_WINDOW_HAMMING, FBANK_WINDOW_HANNING, FBANK_WINDOW_BLACKMAN, FBANK_WINDOW_RECTANGULAR = range(5)
FBANK_WINDOW_NAMES = {"povey": FBANK_WINDOW_POVEY, "hamming": FBANK_WINDOW_HAMMING, "hanning": FBANK_WINDOW_HANNING,
                      "blackman": FBANK_WINDOW_BLACKMAN, "rectangular": FBANK_WINDOW_RECTANGULAR}
FBANK_TILE = 16                                  # frames of one row per tile of afg_fbank_hip
CMN_FRAMES_MAJOR, CMN_COL_MAJOR = 0, 1             # afg_cmn_params.layout
CMN_LAYOUT_NAMES = {"frames": CMN_FRAMES_MAJOR, "cols": CMN_COL_MAJOR}
CMN_CHUNK = 32                                   # frames of one slab per tile of afg_slide_cmn_hip
YIN_TILE, YIN_CHUNK = 4, 16                      # frames of one row per tile of afg_yin_hip; lags per chunk of its cumulative mean

# every symbol include/afg.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "afg_abi_version", "afg_status_string", "afg_last_error", "afg_device_count", "afg_device_name",
    "afg_set_numeric_mode", "afg_get_numeric_mode", "afg_dev_option",
    "afg_mp3_plan_create", "afg_mp3_plan_destroy", "afg_mp3_plan_blocks", "afg_mp3_plan_segments",
    "afg_mp3_transform_hip", "afg_mp3_requant_hip", "afg_mp3_parse_q", "afg_mp3_parsed_q_free", "afg_mp3_qtables",
    "afg_vorbis_plan_create", "afg_vorbis_plan_destroy", "afg_vorbis_plan_packets",
    "afg_vorbis_plan_spec_floats", "afg_vorbis_plan_out_floats", "afg_vorbis_plan_offsets",
    "afg_vorbis_transform_hip", "afg_vorbis_floor_hip", "afg_vorbis_parse_r", "afg_vorbis_parsed_r_free",
    "afg_flac_transform_hip", "afg_flac_variants", "afg_flac_transform_variants_hip",
    "afg_qoa_transform_hip",
    "afg_celt_transform_hip", "afg_celt_transform_streams_hip",
    "afg_open_from_memory", "afg_is_error", "afg_error_message", "afg_get_format", "afg_get_num_channels",
    "afg_get_length_in_frames", "afg_get_samplerate", "afg_read_samples_float", "afg_close",
    "afg_can_seek", "afg_seek_position", "afg_tell_position",
    "afg_flac_parse", "afg_flac_parsed_free", "afg_qoa_parse", "afg_mp3_parse", "afg_mp3_parsed_free", "afg_vorbis_parse", "afg_vorbis_parsed_free",
    "afg_opus_parse", "afg_opus_parsed_free", "afg_opus_output_gain_hip",
    "afg_batch_decode", "afg_batch_free", "afg_batch_decode_ex", "afg_set_device", "afg_get_device", "afg_host_pool_trim",
    "afg_device_malloc", "afg_device_free", "afg_memcpy_h2d", "afg_memcpy_d2h", "afg_stream_synchronize",
    "afg_copy_probe_hip", "afg_lds_fill_probe_hip",
    "afg_qoa_encoded_size", "afg_qoa_encode_hip", "afg_wav_encoded_size", "afg_wav_encode", "afg_wav_encode_dithered",
    "afg_opus_output_hip",
    "afg_mod_render_hip", "afg_mod_parse", "afg_mod_parsed_free", "afg_is_module", "afg_module_pattern_count",
    "afg_module_length", "afg_module_rows_in_pattern", "afg_module_tell_pattern", "afg_module_tell_row", "afg_module_seek",
    "afg_xm_render_hip", "afg_xm_parse", "afg_xm_parsed_free",
    "afg_wav_layout", "afg_wav_convert_hip", "afg_wav_parse",
    "afg_pcm_to_f64_hip", "afg_read_samples_double",
    "afg_lcg31_jump", "afg_wav_pack_layout", "afg_wav_pack_hip",
    "afg_open_to_buffer", "afg_open_to_memory", "afg_is_open_for_reading", "afg_is_open_for_writing",
    "afg_write_samples_float", "afg_write_samples_double", "afg_finalize_encoding", "afg_finalize_and_get_encoded",
    "afg_batch_encode", "afg_encode_free",
    "afg_pcm_pack_layout", "afg_pcm_pack_hip", "afg_batch_transcode",
    "afg_collate_layout", "afg_collate_hip", "afg_batch_decode_to_device",
    "afg_resample_taps", "afg_resample_layout", "afg_resample_hip", "afg_batch_decode_resampled",
    "afg_mel_basis", "afg_mel_filters", "afg_mel_frames", "afg_mel_layout", "afg_mel_check_rows", "afg_melspec_hip", "afg_batch_decode_mel",
    "afg_mel_fft_tables", "afg_mel_fft_layout", "afg_mel_fft_check_rows", "afg_melspec_fft_hip",
    "afg_norm_layout", "afg_norm_check_groups", "afg_normalize_hip", "afg_batch_decode_resampled_norm", "afg_batch_decode_mel_norm",
    "afg_cep_dct", "afg_cep_layout", "afg_cep_check_rows", "afg_cepstra_hip", "afg_batch_decode_mfcc",
    "afg_trim_layout", "afg_trim_check_groups", "afg_trim_hip", "afg_batch_decode_trimmed",
    "afg_stft_tile_frames", "afg_stft_layout", "afg_stft_check_rows", "afg_stft_hip", "afg_batch_decode_stft",
    "afg_biquad_design", "afg_filter_bound", "afg_filter_tile_frames", "afg_filter_check_rows", "afg_filter_hip", "afg_batch_decode_filtered",
    "afg_kweight_design", "afg_loudness_lufs", "afg_loudness_layout", "afg_loudness_check_groups", "afg_loudness_hip", "afg_batch_decode_loudnorm",
    "afg_istft_tile_samples", "afg_istft_layout", "afg_istft_envelope_min", "afg_istft_check_rows", "afg_istft_hip",
    "afg_pvoc_out_frames", "afg_pvoc_bound", "afg_pvoc_check_rows", "afg_pvoc_hip",
    "afg_convolve_bank_layout", "afg_convolve_bank_check", "afg_convolve_bank_hip", "afg_convolve_layout", "afg_convolve_bound",
    "afg_convolve_check_rows", "afg_convolve_hip",
    "afg_mix_ratio", "afg_mix_layout", "afg_mix_check_groups", "afg_mix_hip", "afg_batch_decode_mixed",
    "afg_fbank_n_fft", "afg_fbank_frames", "afg_fbank_tables", "afg_fbank_filters", "afg_fbank_layout", "afg_fbank_check_rows", "afg_fbank_hip",
    "afg_batch_decode_fbank",
    "afg_yin_lags", "afg_yin_frames", "afg_yin_layout", "afg_yin_hip", "afg_batch_decode_pitch",
    "afg_cmn_layout", "afg_cmn_work_bytes", "afg_cmn_check_slabs", "afg_slide_cmn_hip", "afg_batch_decode_fbank_cmn",
]


class AfgError(RuntimeError):
    pass


# AudioFileFormat (stream.d:36-47), in the reference's order
FORMAT_NAMES = ["wav", "mp3", "flac", "ogg", "opus", "qoa", "mod", "xm", "unknown"]
FORMAT_WAV, FORMAT_MP3, FORMAT_FLAC, FORMAT_OGG, FORMAT_OPUS, FORMAT_QOA, FORMAT_MOD, FORMAT_XM, FORMAT_UNKNOWN = range(9)
UNKNOWN_LENGTH = -1   # audiostreamUnknownLength, stream.d:90


class FlacParsed(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("channels", C.c_uint32), ("bps", C.c_uint32), ("max_block", C.c_uint32),
                ("total_samples", C.c_uint64), ("n_frames", C.c_uint64), ("n_subframes", C.c_uint64),
                ("n_res", C.c_uint64), ("out_samples", C.c_uint64), ("frames", C.c_void_p),
                ("subframes", C.c_void_p), ("res", C.c_void_p), ("owner", C.c_void_p)]


class Mp3Parsed(C.Structure):
    _fields_ = [("channels", C.c_int32), ("hz", C.c_int32), ("tagged", C.c_int32), ("start_delay", C.c_int32),
                ("detected_samples", C.c_uint64), ("declared_samples", C.c_uint64), ("pcm_samples", C.c_uint64),
                ("n_runs", C.c_uint64), ("n_blocks", C.c_uint64), ("n_copies", C.c_uint64),
                ("run_granules", C.c_void_p), ("coef", C.c_void_p), ("flags", C.c_void_p), ("copies", C.c_void_p),
                ("owner", C.c_void_p)]


class Mp3ParsedQ(C.Structure):
    _fields_ = [("base", Mp3Parsed), ("n_granules", C.c_uint64), ("n_sdesc", C.c_uint64), ("q", C.c_void_p),
                ("granules", C.c_void_p), ("sdesc", C.c_void_p)]


MP3_QGRANULE_DTYPE = np.dtype([("q_off", np.uint64), ("coef_off", np.uint64), ("sdesc", np.uint32), ("nch", np.uint8),
                               ("stereo", np.uint8), ("table", np.uint8, (2,)), ("scale", np.float32, (2, 40))], align=True)
MP3_SDESC_DTYPE = np.dtype([("type", np.uint8, (40,)), ("fl", np.float32, (40,)), ("fr", np.float32, (40,))], align=True)
assert MP3_QGRANULE_DTYPE.itemsize == 344 and MP3_SDESC_DTYPE.itemsize == 360


class VorbisParsed(C.Structure):
    _fields_ = [("channels", C.c_int32), ("blocksize0", C.c_int32), ("blocksize1", C.c_int32), ("sample_rate", C.c_uint32),
                ("total_samples", C.c_uint32), ("n_packets", C.c_uint64), ("spec_floats", C.c_uint64),
                ("pcm_frames", C.c_uint64), ("pflags", C.c_void_p), ("spec", C.c_void_p), ("take_from", C.c_void_p),
                ("take_count", C.c_void_p), ("owner", C.c_void_p)]


class VorbisParsedR(C.Structure):
    _fields_ = [("base", VorbisParsed), ("n_curves", C.c_uint64), ("n_points", C.c_uint64), ("n_steps", C.c_uint64),
                ("packets", C.c_void_p), ("curves", C.c_void_p), ("points", C.c_void_p), ("steps", C.c_void_p)]


class OpusParsed(C.Structure):
    _fields_ = [("channels", C.c_int32), ("preskip", C.c_int32), ("gain_i", C.c_int32), ("error", C.c_int32),
                ("gain", C.c_float), ("pad", C.c_int32), ("declared_frames", C.c_int64), ("pcm_frames", C.c_uint64),
                ("n_frames", C.c_uint64), ("n_coeffs", C.c_uint64), ("frames", C.c_void_p), ("coeffs", C.c_void_p),
                ("owner", C.c_void_p)]


# ProTracker MOD records (afg.h)
MOD_MAX_FRAMES = 30 * 60 * 44100
MOD_SONG_DTYPE = np.dtype([("out_frame", np.uint64), ("tick_base", np.uint64), ("seg_base", np.uint64), ("sample_base", np.uint64),
                           ("n_ticks", np.uint32), ("sample_bytes", np.uint32), ("reserved", np.uint64)])
assert MOD_SONG_DTYPE.itemsize == 48
MOD_TICK_DTYPE = np.dtype([("frame", np.uint32), ("frames", np.uint32), ("seg", np.uint32), ("n_seg", np.uint32),
                           ("pattern", np.int16), ("line", np.int16), ("pad", np.uint32)])
assert MOD_TICK_DTYPE.itemsize == 24
MOD_SEGMENT_DTYPE = np.dtype([("frame", np.uint32), ("frames", np.uint32), ("position", np.float32), ("increment", np.float32),
                              ("level_l", np.float32), ("level_r", np.float32), ("sample_off", np.uint32), ("loop_start", np.int32),
                              ("loop_length", np.int32), ("loop_end", np.int32), ("length", np.int32), ("channel", np.uint32)])
assert MOD_SEGMENT_DTYPE.itemsize == 48


XM_SONG_DTYPE = np.dtype([("out_frame", np.uint64), ("tick_base", np.uint64), ("seg_base", np.uint64), ("sample_base", np.uint64),
                          ("aux_base", np.uint64), ("n_ticks", np.uint32), ("sample_bytes", np.uint32), ("reserved", np.uint64, (2,))])
assert XM_SONG_DTYPE.itemsize == 64
XM_TICK_DTYPE = np.dtype([("frame", np.uint32), ("frames", np.uint32), ("seg", np.uint32), ("n_seg", np.uint32), ("scale", np.float32),
                          ("table_index", np.int16), ("row", np.int16), ("loop_count", np.uint32), ("pad", np.uint32)])
assert XM_TICK_DTYPE.itemsize == 32
XM_SEGMENT_DTYPE = np.dtype([("frame", np.uint32), ("frames", np.uint32), ("sample_off", np.uint32), ("last", np.uint32),
                             ("flags", np.uint32), ("channel", np.uint32), ("position", np.float32), ("step", np.float32),
                             ("vol_l", np.float32), ("vol_r", np.float32), ("aux_vol", np.uint32), ("aux_fade", np.uint32),
                             ("aux_pos", np.uint32), ("fade_count", np.uint32), ("pad", np.uint32, (2,))])
assert XM_SEGMENT_DTYPE.itemsize == 64
XM_SEG_16BIT, XM_SEG_BACK, XM_SEG_TABLE, XM_SEG_RAMP, XM_SEG_FADE = 1, 2, 4, 8, 16


class XmParsed(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("capped", C.c_uint32), ("length", C.c_uint32), ("patterns", C.c_uint32),
                ("instruments", C.c_uint32), ("restart", C.c_uint32), ("n_frames", C.c_uint64), ("n_ticks", C.c_uint64),
                ("n_segments", C.c_uint64), ("n_sample_bytes", C.c_uint64), ("n_aux", C.c_uint64), ("ticks", C.c_void_p),
                ("segments", C.c_void_p), ("sample_bytes", C.c_void_p), ("aux", C.c_void_p), ("owner", C.c_void_p)]


# WAV (afg.h): span records of afg_wav_convert_hip and what afg_wav_parse returns
WAV_KIND_U8, WAV_KIND_S16, WAV_KIND_S24, WAV_KIND_S32, WAV_KIND_F32, WAV_KIND_F64 = range(6)
WAV_KIND_BYTES = (1, 2, 3, 4, 4, 8)
F64_KIND_FLAC_S32 = 6                     # afg_pcm_to_f64_hip only: the int32 plane of the FLAC restore
F64_KIND_BYTES = WAV_KIND_BYTES + (4,)
WAV_TILE_SAMPLES = 4096
WAV_SPAN_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("count", np.uint64), ("tile_first", np.uint64),
                           ("kind", np.uint32), ("pad", np.uint32)])
assert WAV_SPAN_DTYPE.itemsize == 40


class WavParsed(C.Structure):
    _fields_ = [("tag", C.c_uint32), ("channels", C.c_uint32), ("bits", C.c_uint32), ("sample_rate", C.c_uint32),
                ("frames", C.c_uint32), ("kind", C.c_int32), ("samples_offset", C.c_uint64), ("present_samples", C.c_uint64)]


class ModParsed(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("capped", C.c_uint32), ("n_frames", C.c_uint64), ("n_ticks", C.c_uint64),
                ("n_segments", C.c_uint64), ("n_sample_bytes", C.c_uint64), ("ticks", C.c_void_p), ("segments", C.c_void_p),
                ("sample_bytes", C.c_void_p), ("owner", C.c_void_p)]


class BatchItem(C.Structure):
    _fields_ = [("status", C.c_int), ("message", C.c_char_p), ("format", C.c_int), ("channels", C.c_int),
                ("samplerate", C.c_float), ("frames", C.c_int64), ("pcm", C.POINTER(C.c_float))]


class BatchOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_threads", C.c_int), ("n_devices", C.c_int), ("devices", C.POINTER(C.c_int)),
                ("sample_type", C.c_uint32), ("dither", C.c_int), ("dither_seed", C.c_uint32)]


class CollateOpts(C.Structure):
    """afg_collate_opts (afg_batch_decode_to_device)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_threads", C.c_int), ("channels", C.c_uint32), ("frames", C.c_uint32),
                ("first_frame", C.POINTER(C.c_int64))]


class ResampleOpts(C.Structure):
    """afg_resample_opts (afg_batch_decode_resampled)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_threads", C.c_int), ("channels", C.c_uint32), ("frames", C.c_uint32),
                ("first_frame", C.POINTER(C.c_int64)), ("samplerate", C.c_uint32), ("mono", C.c_uint32), ("in_channels", C.c_uint32),
                ("max_in_rate", C.c_uint32), ("lowpass_width", C.c_uint32)]


class MelParams(C.Structure):
    """afg_mel_params (afg_melspec_hip)."""
    _fields_ = [("n_fft", C.c_uint32), ("win_length", C.c_uint32), ("hop", C.c_uint32), ("n_mels", C.c_uint32), ("center", C.c_uint32),
                ("pad_mode", C.c_uint32), ("out_kind", C.c_uint32), ("log_floor", C.c_float)]


class MelOpts(C.Structure):
    """afg_mel_opts (afg_batch_decode_mel): afg_resample_opts' fields, then the mel parameters and the bank's, then the
    algorithm (MEL_ALGO_*; 0: the direct path) and a reserved 0.  The structure has all of them (sizeof, offsets, attributes),
    but `_fields_` -- the list a positional construction walks -- stops at f_max as it did before the last two were appended:
    they are set by keyword or attribute, and a construction that leaves them out gets the direct path."""
    _fields_ = ResampleOpts._fields_ + [("n_out", C.c_uint32), ("mel", MelParams), ("scale", C.c_uint32), ("norm", C.c_uint32),
                                        ("f_min", C.c_double), ("f_max", C.c_double), ("algorithm", C.c_uint32), ("reserved", C.c_uint32)]


del MelOpts._fields_[-2:]                                    # (the layout is made; the list is what positional arguments map to)


class StftParams(C.Structure):
    """afg_stft_params (afg_stft_hip)."""
    _fields_ = [("n_fft", C.c_uint32), ("win_length", C.c_uint32), ("hop", C.c_uint32), ("center", C.c_uint32), ("pad_mode", C.c_uint32),
                ("out_kind", C.c_uint32), ("log_floor", C.c_float), ("reserved", C.c_uint32)]


class IstftParams(C.Structure):
    """afg_istft_params (afg_istft_hip)."""
    _fields_ = [("n_fft", C.c_uint32), ("win_length", C.c_uint32), ("hop", C.c_uint32), ("center", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class PvocParams(C.Structure):
    """afg_pvoc_params (afg_pvoc_hip)."""
    _fields_ = [("n_fft", C.c_uint32), ("hop", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class ConvolveParams(C.Structure):
    """afg_convolve_params (afg_convolve_hip)."""
    _fields_ = [("direct_max", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class StftOpts(C.Structure):
    """afg_stft_opts (afg_batch_decode_stft): afg_resample_opts' fields, n_out, the parameters and a reserved 0."""
    _fields_ = ResampleOpts._fields_ + [("n_out", C.c_uint32), ("stft", StftParams), ("reserved", C.c_uint32)]


class FbankParams(C.Structure):
    """afg_fbank_params (afg_fbank_hip)."""
    _fields_ = [("win_length", C.c_uint32), ("hop", C.c_uint32), ("n_fft", C.c_uint32), ("n_mels", C.c_uint32), ("snip_edges", C.c_uint32),
                ("remove_dc", C.c_uint32), ("use_power", C.c_uint32), ("use_log", C.c_uint32), ("use_energy", C.c_uint32),
                ("raw_energy", C.c_uint32), ("htk_compat", C.c_uint32), ("layout", C.c_uint32), ("preemph", C.c_float),
                ("energy_floor", C.c_float), ("scale", C.c_float), ("reserved", C.c_uint32)]


class FbankOpts(C.Structure):
    """afg_fbank_opts (afg_batch_decode_fbank): afg_resample_opts' fields, n_out, the parameters, the window type, the bank's
    arguments, the Blackman coefficient and a reserved 0."""
    _fields_ = ResampleOpts._fields_ + [("n_out", C.c_uint32), ("fbank", FbankParams), ("window_type", C.c_uint32), ("low_freq", C.c_double),
                                        ("high_freq", C.c_double), ("blackman_coeff", C.c_double), ("reserved", C.c_uint32)]


class YinParams(C.Structure):
    """afg_yin_params (afg_yin_hip)."""
    _fields_ = [("frame_length", C.c_uint32), ("win_length", C.c_uint32), ("hop", C.c_uint32), ("tau_min", C.c_uint32), ("tau_max", C.c_uint32),
                ("center", C.c_uint32), ("pad_mode", C.c_uint32), ("threshold", C.c_float), ("samplerate", C.c_double),
                ("reserved", C.c_uint32 * 2)]


class PitchOpts(C.Structure):
    """afg_pitch_opts (afg_batch_decode_pitch): afg_resample_opts' fields, n_out, the parameters and a reserved 0."""
    _fields_ = ResampleOpts._fields_ + [("n_out", C.c_uint32), ("yin", YinParams), ("reserved", C.c_uint32)]


class CmnParams(C.Structure):
    """afg_cmn_params (afg_slide_cmn_hip)."""
    _fields_ = [("cmn_window", C.c_uint32), ("min_cmn_window", C.c_uint32), ("center", C.c_uint32), ("norm_vars", C.c_uint32),
                ("cols", C.c_uint32), ("layout", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CmnSlab(C.Structure):
    """afg_cmn_slab: one slab of frames by columns (afg_slide_cmn_hip)."""
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("pitch", C.c_uint64), ("first_tile", C.c_uint64),
                ("n_frames", C.c_uint32), ("reserved", C.c_uint32 * 3)]


CMN_SLAB_DTYPE = np.dtype(CmnSlab)               # arrays of the records, as the other stages' *_DTYPE


class NormGroup(C.Structure):
    """afg_norm_group: the rows one set of statistics covers (afg_normalize_hip)."""
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("stride", C.c_uint64), ("first_tile", C.c_uint64),
                ("rows", C.c_uint32), ("valid", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class NormStats(C.Structure):
    """afg_norm_stats: one group's record."""
    _fields_ = [("sum", C.c_double), ("sumsq", C.c_double), ("count", C.c_uint64), ("min", C.c_float), ("max", C.c_float),
                ("offset", C.c_float), ("scale", C.c_float)]


class NormParams(C.Structure):
    """afg_norm_params."""
    _fields_ = [("mode", C.c_uint32), ("target", C.c_float), ("eps", C.c_float), ("range", C.c_float), ("shift", C.c_float),
                ("gain", C.c_float)]


NORM_GROUP_DTYPE = np.dtype(NormGroup)           # arrays of the records, as the other stages' *_DTYPE
NORM_STATS_DTYPE = np.dtype(NormStats)
assert NORM_GROUP_DTYPE.itemsize == 48 and NORM_STATS_DTYPE.itemsize == 40 and C.sizeof(NormParams) == 24


class CepParams(C.Structure):
    """afg_cep_params (afg_cepstra_hip)."""
    _fields_ = [("n_mels", C.c_uint32), ("n_ceps", C.c_uint32), ("delta_order", C.c_uint32), ("delta_win", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class CepRow(C.Structure):
    """afg_cep_row: one [n_mels, frames] slab and its [(1 + delta_order) * n_ceps, frames] output (afg_cepstra_hip)."""
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("first_tile", C.c_uint64), ("frames", C.c_uint32),
                ("reserved", C.c_uint32)]


class MfccOpts(C.Structure):
    """afg_mfcc_opts (afg_batch_decode_mfcc)."""
    _fields_ = [("struct_size", C.c_uint32), ("dct_norm", C.c_uint32), ("mel", MelOpts), ("cep", CepParams), ("lifter", C.c_double),
                ("log_scale", C.c_double)]


CEP_ROW_DTYPE = np.dtype(CepRow)                 # arrays of the records, as the other stages' *_DTYPE
assert CEP_ROW_DTYPE.itemsize == 32 and C.sizeof(CepParams) == 32


class TrimParams(C.Structure):
    """afg_trim_params (afg_trim_hip)."""
    _fields_ = [("frame_length", C.c_uint32), ("hop", C.c_uint32), ("reference", C.c_uint32), ("lead", C.c_uint32), ("trail", C.c_uint32),
                ("reserved", C.c_uint32 * 3), ("ratio", C.c_double), ("abs_power", C.c_double)]


class TrimGroup(C.Structure):
    """afg_trim_group: the input rows one region is found over, and the output slab they are shifted into (afg_trim_hip)."""
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("in_stride", C.c_uint64), ("out_stride", C.c_uint64),
                ("first_block", C.c_uint64), ("first_tile", C.c_uint64), ("rows", C.c_uint32), ("valid", C.c_uint32),
                ("out_rows", C.c_uint32), ("out_frames", C.c_uint32)]


class TrimRegion(C.Structure):
    """afg_trim_region: one group's record."""
    _fields_ = [("begin", C.c_uint32), ("end", C.c_uint32), ("ref_power", C.c_double)]


TRIM_GROUP_DTYPE = np.dtype(TrimGroup)           # arrays of the records, as the other stages' *_DTYPE
TRIM_REGION_DTYPE = np.dtype(TrimRegion)
assert TRIM_GROUP_DTYPE.itemsize == 64 and TRIM_REGION_DTYPE.itemsize == 16 and C.sizeof(TrimParams) == 48


SAMPLE_F32, SAMPLE_F64, SAMPLE_PCM_S8, SAMPLE_PCM_S16, SAMPLE_PCM_S24 = range(5)     # afg_batch_opts.sample_type
BATCH_OPTS_SIZE_V1 = BatchOpts.sample_type.offset        # the struct before sample_type was appended
BATCH_OPTS_SIZE_V2 = BatchOpts.dither.offset             # ... up to sample_type, before dither and dither_seed were
# what an item's pcm is viewed as, per sample type: (numpy dtype, trailing shape)
_SAMPLE_VIEW = {SAMPLE_F32: (np.float32, ()), SAMPLE_F64: (np.float64, ()), SAMPLE_PCM_S8: (np.uint8, ()),
                SAMPLE_PCM_S16: (np.int16, ()), SAMPLE_PCM_S24: (np.uint8, (3,))}


class Biquad(C.Structure):
    """afg_biquad: one second-order section, a0 == 1."""
    _fields_ = [("b0", C.c_double), ("b1", C.c_double), ("b2", C.c_double), ("a1", C.c_double), ("a2", C.c_double)]


class FilterParams(C.Structure):
    """afg_filter_params (afg_filter_hip)."""
    _fields_ = [("n_sections", C.c_uint32), ("sec", Biquad * 8)]


class LoudnessParams(C.Structure):
    """afg_loudness_params (afg_loudness_hip)."""
    _fields_ = [("samplerate", C.c_uint32), ("apply", C.c_uint32), ("target_lufs", C.c_double), ("max_peak", C.c_float), ("max_gain", C.c_float),
                ("weights", C.c_double * 8), ("reserved", C.c_uint32 * 2)]


class LoudnessGroup(C.Structure):
    """afg_loudness_group: the rows one measurement covers (afg_loudness_hip)."""
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("stride", C.c_uint64), ("first_sub", C.c_uint64), ("first_block", C.c_uint64),
                ("rows", C.c_uint32), ("valid", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class LoudnessCounts(C.Structure):
    """afg_loudness_counts: the doubles of d_sub and d_blocks a launch takes (afg_loudness_layout)."""
    _fields_ = [("n_sub", C.c_uint64), ("n_blocks", C.c_uint64)]


class LoudnessStats(C.Structure):
    """afg_loudness_stats: one group's record."""
    _fields_ = [("energy", C.c_double), ("rel_threshold", C.c_double), ("n_blocks", C.c_uint32), ("n_abs", C.c_uint32), ("n_gated", C.c_uint32),
                ("flags", C.c_uint32), ("peak", C.c_float), ("gain", C.c_float)]


LOUDNESS_GROUP_DTYPE = np.dtype(LoudnessGroup)   # arrays of the records, as the other stages' *_DTYPE
LOUDNESS_STATS_DTYPE = np.dtype(LoudnessStats)
assert LOUDNESS_GROUP_DTYPE.itemsize == 64 and LOUDNESS_STATS_DTYPE.itemsize == 40 and C.sizeof(LoudnessParams) == 96 and C.sizeof(LoudnessCounts) == 16


class MixGroup(C.Structure):
    """afg_mix_group: the rows one gain covers and the noise under them (afg_mix_hip)."""
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("stride", C.c_uint64), ("first_tile", C.c_uint64), ("noise_off", C.c_uint64),
                ("noise_stride", C.c_uint64), ("ratio", C.c_double), ("rows", C.c_uint32), ("valid", C.c_uint32), ("noise_len", C.c_uint32),
                ("noise_start", C.c_uint32), ("flags", C.c_uint32), ("gain", C.c_float)]


class MixStats(C.Structure):
    """afg_mix_stats: one group's record."""
    _fields_ = [("signal_energy", C.c_double), ("noise_energy", C.c_double), ("gain", C.c_float), ("flags", C.c_uint32)]


class MixNoise(C.Structure):
    """afg_mix_noise: the noise bank of afg_batch_decode_mixed and what every file takes of it."""
    _fields_ = [("d_noise", C.c_void_p), ("n_clips", C.c_uint64), ("clip_pitch", C.c_uint32), ("clip_rows", C.c_uint32),
                ("lengths", C.POINTER(C.c_uint32)), ("index", C.POINTER(C.c_uint32)), ("start", C.POINTER(C.c_uint64)),
                ("snr_db", C.POINTER(C.c_double))]


MIX_GROUP_DTYPE = np.dtype(MixGroup)             # arrays of the records, as the other stages' *_DTYPE
MIX_STATS_DTYPE = np.dtype(MixStats)
assert MIX_GROUP_DTYPE.itemsize == 80 and MIX_STATS_DTYPE.itemsize == 24 and C.sizeof(MixNoise) == 56


class EncodingOptions(C.Structure):
    """afg_encoding_options (EncodingOptions, stream.d:59-67)."""
    _fields_ = [("struct_size", C.c_uint32), ("sample_format", C.c_int), ("dither", C.c_int), ("dither_seed", C.c_uint32)]


class EncodeInput(C.Structure):
    _fields_ = [("pcm", C.c_void_p), ("frames", C.c_uint64), ("channels", C.c_uint32), ("samplerate", C.c_float)]


class EncodedItem(C.Structure):
    _fields_ = [("status", C.c_int), ("message", C.c_char_p), ("bytes", C.POINTER(C.c_uint8)), ("size", C.c_uint64)]


class EncodeResult(C.Structure):
    _fields_ = [("n_files", C.c_int), ("items", C.POINTER(EncodedItem)), ("owner", C.c_void_p)]


class BatchResult(C.Structure):
    _fields_ = [("n_files", C.c_int), ("items", C.POINTER(BatchItem)), ("owner", C.c_void_p)]


_lib = None
RAND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)      # afg_rand_fn


def mp3_flags(block_type=0, n_long_bands=0, aa_bands=31):
    """AFG_MP3_FLAGS of include/afg.h."""
    return np.uint32(block_type | (n_long_bands << 8) | ((aa_bands + 1) << 16))


# The library's test hooks (afg.h: afg_dev_option) under the environment-variable names the test-suite has always used:
# THIS module reads the variables -- the C library reads none -- and hands changed values over before the next call.
_DEV_ENV = {"AFG_CELT_PATH": ("celt_path", {"stream": 1, "split": 2, "walk": 3}), "AFG_CELT_DE_SEQ": ("celt_de_seq", None),
            "AFG_CELT_DE_DUO": ("celt_de_duo", None), "AFG_CELT_SEG_RECS": ("celt_seg_recs", None),
            "AFG_CELT_WHOLE_FRAMES": ("celt_whole_frames", None), "AFG_VORBIS_SINGLE": ("vorbis_single", None),
            "AFG_MP3_CHUNKS": ("mp3_chunks", None), "AFG_MP3_FLOAT_UPLOAD": ("mp3_float_upload", None),
            "AFG_VORBIS_HOST_FLOOR": ("vorbis_host_floor", None), "AFG_FLAC_HOST_RES32": ("flac_host_res32", None),
            "AFG_VORBIS_SEG_PACKETS": ("vorbis_seg_packets", None), "AFG_BATCH_GROUPS": ("batch_groups", None),
            "AFG_STAGE_CHUNK_SAMPLES": ("stage_chunk_samples", None), "AFG_RESAMPLE_SCRATCH_BYTES": ("resample_scratch_bytes", None),
            "AFG_MEL_SCRATCH_BYTES": ("mel_scratch_bytes", None), "AFG_TRIM_SCRATCH_BYTES": ("trim_scratch_bytes", None)}
_dev_seen = {}


def _sync_dev_options(L):
    for env, (name, words) in _DEV_ENV.items():
        raw = os.environ.get(env)
        if _dev_seen.get(env, None) == raw and env in _dev_seen:
            continue
        _dev_seen[env] = raw
        if raw is None:
            value = -1
        elif words is not None:
            value = words.get(raw, -1)
        else:
            try:
                value = int(raw)
            except ValueError:
                value = 1
        L.afg_dev_option(name.encode(), value)


def lib():
    """Load the C-ABI library (once).  torch is imported first so that both share one HIP runtime."""
    global _lib
    if _lib is not None:
        _sync_dev_options(_lib)
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AfgError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    try:
        import torch  # noqa: F401  (loads libamdhip64 so the C ABI binds to the same runtime)
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.afg_abi_version.restype = C.c_int
    L.afg_status_string.restype = C.c_char_p
    L.afg_status_string.argtypes = [C.c_int]
    L.afg_last_error.restype = C.c_char_p
    L.afg_device_count.restype = C.c_int
    L.afg_device_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.afg_opus_output_hip.argtypes = [u64, vp, vp, vp, vp]
    L.afg_opus_output_gain_hip.argtypes = [u64, vp, C.c_float, vp, vp, vp]
    L.afg_opus_parse.argtypes = [vp, C.c_size_t, C.POINTER(OpusParsed)]
    L.afg_opus_parsed_free.argtypes = [C.POINTER(OpusParsed)]
    L.afg_opus_parsed_free.restype = None
    L.afg_qoa_encoded_size.argtypes = [u32, u32]
    L.afg_qoa_encoded_size.restype = u64
    L.afg_qoa_encode_hip.argtypes = [u32, vp, vp, vp, vp, vp]
    L.afg_wav_encoded_size.argtypes = [u64, u32, C.c_int]
    L.afg_wav_encoded_size.restype = u64
    L.afg_wav_encode.argtypes = [vp, u64, u32, u32, C.c_int, vp, u64]
    L.afg_wav_encode.restype = u64
    L.afg_wav_encode_dithered.argtypes = [vp, u64, u32, u32, C.c_int, RAND_FN, vp, u32, vp, u64]
    L.afg_wav_encode_dithered.restype = u64
    L.afg_mp3_plan_create.argtypes = [C.POINTER(vp), u32, vp, vp, u32]
    L.afg_mp3_plan_destroy.argtypes = [vp]
    L.afg_mp3_plan_destroy.restype = None
    L.afg_mp3_plan_blocks.argtypes = [vp]
    L.afg_mp3_plan_blocks.restype = u64
    L.afg_mp3_plan_segments.argtypes = [vp]
    L.afg_mp3_plan_segments.restype = u32
    L.afg_mp3_transform_hip.argtypes = [vp, vp, vp, vp, vp, vp]
    L.afg_vorbis_plan_create.argtypes = [C.POINTER(vp), u32, vp, vp, vp, vp, vp, u32]
    L.afg_vorbis_plan_destroy.argtypes = [vp]
    L.afg_vorbis_plan_destroy.restype = None
    for fn in (L.afg_vorbis_plan_packets, L.afg_vorbis_plan_spec_floats, L.afg_vorbis_plan_out_floats):
        fn.argtypes = [vp]
        fn.restype = u64
    L.afg_vorbis_plan_offsets.argtypes = [vp, vp, vp]
    L.afg_vorbis_transform_hip.argtypes = [vp, vp, vp, vp]
    L.afg_vorbis_floor_hip.argtypes = [u64, vp, vp, vp, vp, vp, vp]
    L.afg_flac_transform_hip.argtypes = [u64, vp, vp, vp, vp, vp, vp]
    L.afg_flac_variants.argtypes = [u64, vp, vp]
    L.afg_flac_variants.restype = u32
    L.afg_flac_transform_variants_hip.argtypes = [u64, vp, vp, vp, vp, vp, u32, vp]
    L.afg_qoa_transform_hip.argtypes = [u64, vp, vp, vp, vp, vp]
    L.afg_celt_transform_hip.argtypes = [u32, vp, vp, vp, vp, vp, vp]
    L.afg_celt_transform_streams_hip.argtypes = [u32, vp, vp, vp, vp, vp, vp, vp]
    L.afg_open_from_memory.argtypes = [vp, C.c_size_t]
    L.afg_open_from_memory.restype = vp
    L.afg_is_error.argtypes = [vp]
    L.afg_error_message.argtypes = [vp]
    L.afg_error_message.restype = C.c_char_p
    L.afg_get_format.argtypes = [vp]
    L.afg_get_num_channels.argtypes = [vp]
    L.afg_get_length_in_frames.argtypes = [vp]
    L.afg_get_length_in_frames.restype = C.c_int64
    L.afg_get_samplerate.argtypes = [vp]
    L.afg_get_samplerate.restype = C.c_float
    L.afg_read_samples_float.argtypes = [vp, vp, C.c_int]
    L.afg_close.argtypes = [vp]
    L.afg_can_seek.argtypes = [vp]
    L.afg_seek_position.argtypes = [vp, C.c_int]
    L.afg_tell_position.argtypes = [vp]
    L.afg_close.restype = None
    L.afg_flac_parse.argtypes = [vp, C.c_size_t, C.POINTER(FlacParsed)]
    L.afg_flac_parsed_free.argtypes = [C.POINTER(FlacParsed)]
    L.afg_flac_parsed_free.restype = None
    L.afg_mp3_parse.argtypes = [vp, C.c_size_t, C.POINTER(Mp3Parsed)]
    L.afg_mp3_parsed_free.argtypes = [C.POINTER(Mp3Parsed)]
    L.afg_mp3_parsed_free.restype = None
    L.afg_mp3_parse_q.argtypes = [vp, C.c_size_t, C.POINTER(Mp3ParsedQ)]
    L.afg_mp3_parsed_q_free.argtypes = [C.POINTER(Mp3ParsedQ)]
    L.afg_mp3_parsed_q_free.restype = None
    L.afg_mp3_requant_hip.argtypes = [u64, vp, vp, vp, vp, vp]
    L.afg_vorbis_parse.argtypes = [vp, C.c_size_t, C.POINTER(VorbisParsed)]
    L.afg_vorbis_parsed_free.argtypes = [C.POINTER(VorbisParsed)]
    L.afg_vorbis_parsed_free.restype = None
    L.afg_vorbis_parse_r.argtypes = [vp, C.c_size_t, C.POINTER(VorbisParsedR)]
    L.afg_vorbis_parsed_r_free.argtypes = [C.POINTER(VorbisParsedR)]
    L.afg_vorbis_parsed_r_free.restype = None
    L.afg_qoa_parse.argtypes = [vp, C.c_size_t, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), vp, C.c_size_t,
                                C.POINTER(C.c_size_t)]
    L.afg_batch_decode.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(BatchResult)]
    L.afg_batch_free.argtypes = [C.POINTER(BatchResult)]
    L.afg_batch_decode_ex.argtypes = [vp, vp, C.c_int, C.POINTER(BatchOpts), C.POINTER(BatchResult)]
    L.afg_set_device.argtypes = [C.c_int]
    L.afg_get_device.restype = C.c_int
    L.afg_host_pool_trim.restype = u64
    L.afg_batch_free.restype = None
    L.afg_device_malloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.afg_device_free.argtypes = [vp]
    L.afg_memcpy_h2d.argtypes = [vp, vp, C.c_size_t, vp]
    L.afg_memcpy_d2h.argtypes = [vp, vp, C.c_size_t, vp]
    L.afg_stream_synchronize.argtypes = [vp]
    L.afg_copy_probe_hip.argtypes = [vp, vp, C.c_size_t, vp]
    L.afg_lds_fill_probe_hip.argtypes = [C.c_uint32, vp]
    L.afg_dev_option.argtypes = [C.c_char_p, C.c_int]
    L.afg_mod_render_hip.argtypes = [u32, vp, vp, vp, vp, vp, vp]
    L.afg_mod_parse.argtypes = [vp, C.c_size_t, C.POINTER(ModParsed)]
    L.afg_mod_parsed_free.argtypes = [C.POINTER(ModParsed)]
    L.afg_mod_parsed_free.restype = None
    L.afg_xm_render_hip.argtypes = [u32, vp, vp, vp, vp, vp, vp, vp]
    L.afg_xm_parse.argtypes = [vp, C.c_size_t, C.POINTER(XmParsed)]
    L.afg_wav_layout.argtypes = [vp, u64]
    L.afg_wav_layout.restype = u64
    L.afg_wav_convert_hip.argtypes = [u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_pcm_to_f64_hip.argtypes = [u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_read_samples_double.argtypes = [vp, vp, C.c_int]
    L.afg_wav_parse.argtypes = [vp, C.c_size_t, C.POINTER(WavParsed)]
    L.afg_xm_parsed_free.argtypes = [C.POINTER(XmParsed)]
    L.afg_xm_parsed_free.restype = None
    for fn in (L.afg_is_module, L.afg_module_pattern_count, L.afg_module_length, L.afg_module_tell_pattern, L.afg_module_tell_row):
        fn.argtypes = [vp]
    L.afg_module_rows_in_pattern.argtypes = [vp, C.c_int]
    L.afg_module_seek.argtypes = [vp, C.c_int, C.c_int]
    L.afg_lcg31_jump.argtypes = [u32, u64]
    L.afg_lcg31_jump.restype = u32
    L.afg_wav_pack_layout.argtypes = [vp, u64]
    L.afg_wav_pack_layout.restype = u64
    L.afg_wav_pack_hip.argtypes = [u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_open_to_buffer.argtypes = [C.c_int, C.c_float, C.c_int, C.POINTER(EncodingOptions)]
    L.afg_open_to_buffer.restype = vp
    L.afg_open_to_memory.argtypes = [vp, C.c_size_t, C.c_int, C.c_float, C.c_int, C.POINTER(EncodingOptions)]
    L.afg_open_to_memory.restype = vp
    L.afg_is_open_for_reading.argtypes = [vp]
    L.afg_is_open_for_writing.argtypes = [vp]
    L.afg_write_samples_float.argtypes = [vp, vp, C.c_int]
    L.afg_write_samples_double.argtypes = [vp, vp, C.c_int]
    L.afg_finalize_encoding.argtypes = [vp]
    L.afg_finalize_and_get_encoded.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.afg_batch_encode.argtypes = [C.POINTER(EncodeInput), C.c_int, C.c_int, C.POINTER(EncodingOptions), C.c_int,
                                   C.POINTER(EncodeResult)]
    L.afg_encode_free.argtypes = [C.POINTER(EncodeResult)]
    L.afg_encode_free.restype = None
    L.afg_pcm_pack_layout.argtypes = [vp, u64]
    L.afg_pcm_pack_layout.restype = u64
    L.afg_pcm_pack_hip.argtypes = [u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_transcode.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(EncodingOptions), C.POINTER(BatchOpts),
                                      C.POINTER(EncodeResult)]
    L.afg_collate_layout.argtypes = [vp, u64]
    L.afg_collate_layout.restype = u64
    L.afg_collate_hip.argtypes = [u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_decode_to_device.argtypes = [vp, vp, C.c_int, C.POINTER(CollateOpts), vp, C.POINTER(BatchResult)]
    L.afg_resample_taps.argtypes = [u32, u32, u32, vp, u64, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.afg_resample_taps.restype = u64
    L.afg_resample_layout.argtypes = [vp, u64]
    L.afg_resample_layout.restype = u64
    L.afg_resample_hip.argtypes = [u64, vp, u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_decode_resampled.argtypes = [vp, vp, C.c_int, C.POINTER(ResampleOpts), vp, C.POINTER(BatchResult)]
    L.afg_mel_basis.argtypes = [u32, u32, vp, u64]
    L.afg_mel_basis.restype = u64
    L.afg_mel_filters.argtypes = [u32, u32, u32, C.c_double, C.c_double, u32, u32, vp, u64]
    L.afg_mel_filters.restype = u64
    L.afg_mel_frames.argtypes = [C.POINTER(MelParams), u32]
    L.afg_mel_frames.restype = u32
    L.afg_mel_layout.argtypes = [vp, u64, C.POINTER(MelParams)]
    L.afg_mel_layout.restype = u64
    L.afg_mel_check_rows.argtypes = [vp, u64, u64, C.POINTER(MelParams), u64, u64, u64, u64]
    L.afg_melspec_hip.argtypes = [u64, vp, u64, C.POINTER(MelParams), vp, u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_decode_mel.argtypes = [vp, vp, C.c_int, C.POINTER(MelOpts), vp, C.POINTER(BatchResult)]
    L.afg_mel_fft_tables.argtypes = [u32, u32, vp, u64]
    L.afg_mel_fft_tables.restype = u64
    L.afg_mel_fft_layout.argtypes = [vp, u64, C.POINTER(MelParams)]
    L.afg_mel_fft_layout.restype = u64
    L.afg_mel_fft_check_rows.argtypes = [vp, u64, u64, C.POINTER(MelParams), u64, u64, u64, u64]
    L.afg_melspec_fft_hip.argtypes = [u64, vp, u64, C.POINTER(MelParams), vp, u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_norm_layout.argtypes = [vp, u64]
    L.afg_norm_layout.restype = u64
    L.afg_norm_check_groups.argtypes = [vp, u64, u64, C.POINTER(NormParams), u64, u64]
    L.afg_normalize_hip.argtypes = [u64, vp, u64, C.POINTER(NormParams), vp, u64, vp, u64, vp, vp, vp]
    L.afg_batch_decode_resampled_norm.argtypes = [vp, vp, C.c_int, C.POINTER(ResampleOpts), C.POINTER(NormParams), vp, vp, C.POINTER(BatchResult)]
    L.afg_cep_dct.argtypes = [u32, u32, u32, C.c_double, C.c_double, vp, u64]
    L.afg_cep_dct.restype = u64
    L.afg_cep_layout.argtypes = [vp, u64, C.POINTER(CepParams)]
    L.afg_cep_layout.restype = u64
    L.afg_cep_check_rows.argtypes = [vp, u64, u64, C.POINTER(CepParams), u64, u64, u64]
    L.afg_cepstra_hip.argtypes = [u64, vp, u64, C.POINTER(CepParams), vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_decode_mfcc.argtypes = [vp, vp, C.c_int, C.POINTER(MfccOpts), C.POINTER(NormParams), C.POINTER(NormParams), vp,
                                        C.POINTER(BatchResult)]
    L.afg_batch_decode_mel_norm.argtypes = [vp, vp, C.c_int, C.POINTER(MelOpts), C.POINTER(NormParams), C.POINTER(NormParams), vp,
                                            C.POINTER(BatchResult)]
    L.afg_trim_layout.argtypes = [vp, u64, C.POINTER(TrimParams), C.POINTER(u64), C.POINTER(u64)]
    L.afg_trim_check_groups.argtypes = [vp, u64, u64, u64, C.POINTER(TrimParams), u64, u64]
    L.afg_trim_hip.argtypes = [u64, vp, u64, u64, C.POINTER(TrimParams), vp, u64, vp, u64, vp, vp, vp]
    L.afg_biquad_design.argtypes = [u32, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(Biquad)]
    L.afg_filter_bound.argtypes = [C.POINTER(FilterParams)]
    L.afg_filter_bound.restype = C.c_double
    L.afg_filter_tile_frames.argtypes = []
    L.afg_filter_tile_frames.restype = u32
    L.afg_filter_check_rows.argtypes = [vp, u64, C.POINTER(FilterParams), u64, u64, C.c_int]
    L.afg_filter_hip.argtypes = [u64, vp, C.POINTER(FilterParams), vp, u64, vp, u64, vp, vp]
    L.afg_batch_decode_filtered.argtypes = [vp, vp, C.c_int, C.POINTER(ResampleOpts), C.POINTER(FilterParams), vp, C.POINTER(BatchResult)]
    L.afg_batch_decode_trimmed.argtypes = [vp, vp, C.c_int, C.POINTER(ResampleOpts), C.POINTER(TrimParams), u32, vp, vp, C.POINTER(BatchResult)]
    L.afg_kweight_design.argtypes = [u32, C.POINTER(FilterParams)]
    L.afg_loudness_lufs.argtypes = [C.c_double]
    L.afg_loudness_lufs.restype = C.c_double
    L.afg_loudness_layout.argtypes = [vp, u64, C.POINTER(LoudnessParams), C.POINTER(LoudnessCounts)]
    L.afg_loudness_check_groups.argtypes = [vp, u64, C.POINTER(LoudnessCounts), C.POINTER(LoudnessParams), u64, u64, C.c_int]
    L.afg_loudness_hip.argtypes = [u64, vp, C.POINTER(LoudnessCounts), C.POINTER(LoudnessParams), vp, u64, vp, u64, vp, vp, vp, vp]
    L.afg_batch_decode_loudnorm.argtypes = [vp, vp, C.c_int, C.POINTER(ResampleOpts), C.POINTER(LoudnessParams), vp, vp, C.POINTER(BatchResult)]
    L.afg_stft_tile_frames.argtypes = [C.POINTER(StftParams)]
    L.afg_stft_tile_frames.restype = u32
    L.afg_stft_layout.argtypes = [vp, u64, C.POINTER(StftParams)]
    L.afg_stft_layout.restype = u64
    L.afg_stft_check_rows.argtypes = [vp, u64, u64, C.POINTER(StftParams), u64, u64, u64]
    L.afg_stft_hip.argtypes = [u64, vp, u64, C.POINTER(StftParams), vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_decode_stft.argtypes = [vp, vp, C.c_int, C.POINTER(StftOpts), vp, C.POINTER(BatchResult)]
    L.afg_istft_tile_samples.argtypes = [C.POINTER(IstftParams)]
    L.afg_istft_tile_samples.restype = u32
    L.afg_istft_layout.argtypes = [vp, u64, C.POINTER(IstftParams)]
    L.afg_istft_layout.restype = u64
    L.afg_istft_envelope_min.argtypes = [C.POINTER(IstftParams), u32, u32, u32]
    L.afg_istft_envelope_min.restype = C.c_double
    L.afg_istft_check_rows.argtypes = [vp, u64, u64, C.POINTER(IstftParams), u64, u64, u64]
    L.afg_istft_hip.argtypes = [u64, vp, u64, C.POINTER(IstftParams), vp, u64, vp, u64, vp, u64, vp]
    L.afg_pvoc_out_frames.argtypes = [u32, C.c_double]
    L.afg_pvoc_out_frames.restype = u32
    L.afg_pvoc_bound.argtypes = [C.POINTER(PvocParams), u64]
    L.afg_pvoc_bound.restype = C.c_double
    L.afg_pvoc_check_rows.argtypes = [vp, u64, C.POINTER(PvocParams), u64, u64]
    L.afg_pvoc_hip.argtypes = [u64, vp, C.POINTER(PvocParams), vp, u64, vp, u64, vp]
    L.afg_convolve_bank_layout.argtypes = [vp, u64]
    L.afg_convolve_bank_layout.restype = u64
    L.afg_convolve_bank_check.argtypes = [vp, u64, u64, u64]
    L.afg_convolve_bank_hip.argtypes = [u64, vp, vp, u64, vp, u64, vp]
    L.afg_convolve_layout.argtypes = [vp, u64, vp, u64, C.POINTER(ConvolveParams), C.POINTER(u64)]
    L.afg_convolve_layout.restype = u64
    L.afg_convolve_bound.argtypes = [C.POINTER(ConvolveParams), u32]
    L.afg_convolve_bound.restype = C.c_double
    L.afg_convolve_check_rows.argtypes = [vp, u64, u64, vp, u64, C.POINTER(ConvolveParams), u64, u64, u64, u64, u64, C.POINTER(u64)]
    L.afg_convolve_hip.argtypes = [u64, vp, u64, vp, u64, C.POINTER(ConvolveParams), vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_mix_ratio.argtypes = [C.c_double]
    L.afg_mix_ratio.restype = C.c_double
    L.afg_mix_layout.argtypes = [vp, u64]
    L.afg_mix_layout.restype = u64
    L.afg_mix_check_groups.argtypes = [vp, u64, u64, u64, u64, u64, C.POINTER(u64)]
    L.afg_mix_hip.argtypes = [u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, vp, vp]
    L.afg_batch_decode_mixed.argtypes = [vp, vp, C.c_int, C.POINTER(ResampleOpts), C.POINTER(MixNoise), vp, vp, C.POINTER(BatchResult)]
    L.afg_fbank_n_fft.argtypes = [u32, u32]
    L.afg_fbank_n_fft.restype = u32
    L.afg_fbank_frames.argtypes = [C.POINTER(FbankParams), u32]
    L.afg_fbank_frames.restype = u32
    L.afg_fbank_tables.argtypes = [u32, u32, u32, C.c_double, vp, u64]
    L.afg_fbank_tables.restype = u64
    L.afg_fbank_filters.argtypes = [u32, u32, u32, C.c_double, C.c_double, vp, u64]
    L.afg_fbank_filters.restype = u64
    L.afg_fbank_layout.argtypes = [vp, u64, C.POINTER(FbankParams)]
    L.afg_fbank_layout.restype = u64
    L.afg_fbank_check_rows.argtypes = [vp, u64, u64, C.POINTER(FbankParams), u64, u64, u64, u64]
    L.afg_fbank_hip.argtypes = [u64, vp, u64, C.POINTER(FbankParams), vp, u64, vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_decode_fbank.argtypes = [vp, vp, C.c_int, C.POINTER(FbankOpts), vp, vp, C.POINTER(BatchResult)]
    L.afg_cmn_layout.argtypes = [vp, u64]
    L.afg_cmn_layout.restype = u64
    L.afg_cmn_work_bytes.argtypes = [u64, u32]
    L.afg_cmn_work_bytes.restype = u64
    L.afg_cmn_check_slabs.argtypes = [vp, u64, u64, C.POINTER(CmnParams), u64, u64, C.c_int]
    L.afg_slide_cmn_hip.argtypes = [u64, vp, u64, C.POINTER(CmnParams), vp, u64, vp, u64, vp, u64, vp]
    L.afg_batch_decode_fbank_cmn.argtypes = [vp, vp, C.c_int, C.POINTER(FbankOpts), C.POINTER(CmnParams), vp, vp, C.POINTER(BatchResult)]
    L.afg_yin_lags.argtypes = [C.c_double, C.c_double, C.c_double, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    L.afg_yin_frames.argtypes = [C.POINTER(YinParams), u32]
    L.afg_yin_frames.restype = u32
    L.afg_yin_layout.argtypes = [vp, u64, C.POINTER(YinParams)]
    L.afg_yin_layout.restype = u64
    L.afg_yin_hip.argtypes = [u64, vp, u64, C.POINTER(YinParams), vp, u64, vp, u64, vp]
    L.afg_batch_decode_pitch.argtypes = [vp, vp, C.c_int, C.POINTER(PitchOpts), vp, vp, C.POINTER(BatchResult)]
    _lib = L
    _sync_dev_options(L)
    return L


def check(rc):
    if rc != 0:
        L = lib()
        raise AfgError(f"afg: {L.afg_status_string(rc).decode()} ({rc}): {L.afg_last_error().decode()}")


def _ptr(t):
    """Device pointer of a torch tensor / int / None."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA(HIP) tensors"
    return t.data_ptr()


def _stream(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return getattr(stream, "cuda_stream", stream)


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


class Mp3Plan:
    """Batch description of the MP3 transform stage (afg_mp3_plan)."""

    def __init__(self, granules, channels, seg_granules=0):
        self.granules = _np(granules, np.uint32)
        self.channels = _np(channels, np.uint8)
        assert self.granules.shape == self.channels.shape
        self._h = C.c_void_p()
        check(lib().afg_mp3_plan_create(C.byref(self._h), len(self.granules), self.granules.ctypes.data,
                                        self.channels.ctypes.data, seg_granules))
        self.blocks = int(lib().afg_mp3_plan_blocks(self._h))
        self.segments = int(lib().afg_mp3_plan_segments(self._h))

    def transform(self, d_coef, d_flags, d_pcm, d_state=None, stream=None):
        """Enqueue the transform (no synchronisation).  Arguments are CUDA(HIP) tensors."""
        check(lib().afg_mp3_transform_hip(self._h, _ptr(d_coef), _ptr(d_flags), _ptr(d_pcm),
                                          _ptr(d_state), _stream(stream)))

    def close(self):
        if self._h:
            lib().afg_mp3_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VorbisPlan:
    """Batch description of the Vorbis transform stage (afg_vorbis_plan)."""

    def __init__(self, packets, channels, blocksize0, blocksize1, pflags, seg_packets=0):
        self.packets = _np(packets, np.uint32)
        self.channels = _np(channels, np.uint8)
        self.bs0 = _np(blocksize0, np.uint16)
        self.bs1 = _np(blocksize1, np.uint16)
        self.pflags = _np(pflags, np.uint8)
        assert int(self.packets.sum()) == self.pflags.size
        self._h = C.c_void_p()
        check(lib().afg_vorbis_plan_create(C.byref(self._h), len(self.packets), self.packets.ctypes.data,
                                           self.channels.ctypes.data, self.bs0.ctypes.data,
                                           self.bs1.ctypes.data, self.pflags.ctypes.data, seg_packets))
        self.total_packets = int(lib().afg_vorbis_plan_packets(self._h))
        self.spec_floats = int(lib().afg_vorbis_plan_spec_floats(self._h))
        self.out_floats = int(lib().afg_vorbis_plan_out_floats(self._h))

    def offsets(self):
        so = np.zeros(self.total_packets, np.uint64)
        oo = np.zeros(self.total_packets, np.uint64)
        check(lib().afg_vorbis_plan_offsets(self._h, so.ctypes.data, oo.ctypes.data))
        return so, oo

    def transform(self, d_spec, d_out, stream=None):
        check(lib().afg_vorbis_transform_hip(self._h, _ptr(d_spec), _ptr(d_out), _stream(stream)))

    def close(self):
        if self._h:
            lib().afg_vorbis_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def flac_transform(n_frames, d_frames, d_subframes, d_res, d_out_i32=None, d_out_f32=None, stream=None, variants=None):
    """Enqueue the FLAC restore (afg_flac_transform_hip).  Records are uint8 CUDA tensors holding
    FLAC_FRAME_DTYPE / FLAC_SUBFRAME_DTYPE arrays.  `variants`: the mask flac_variants() computed from the host records
    (afg_flac_transform_variants_hip: only the populated instantiations are launched, side by side)."""
    if variants is None:
        check(lib().afg_flac_transform_hip(int(n_frames), _ptr(d_frames), _ptr(d_subframes), _ptr(d_res),
                                           _ptr(d_out_i32), _ptr(d_out_f32), _stream(stream)))
    else:
        check(lib().afg_flac_transform_variants_hip(int(n_frames), _ptr(d_frames), _ptr(d_subframes), _ptr(d_res),
                                                    _ptr(d_out_i32), _ptr(d_out_f32), int(variants), _stream(stream)))


def flac_variants(frames, subframes):
    """afg_flac_variants on host record arrays (FLAC_FRAME_DTYPE / FLAC_SUBFRAME_DTYPE): bit mask of the kernel
    instantiations the batch populates."""
    frames = np.ascontiguousarray(frames)
    subframes = np.ascontiguousarray(subframes)
    assert frames.dtype.itemsize == 32 and subframes.dtype.itemsize == 68
    return int(lib().afg_flac_variants(len(frames), frames.ctypes.data, subframes.ctypes.data))


def qoa_frames(file_bytes, out_base=0, byte_base=0):
    """Locate the frames of one QOA file (host side of qoa.d:413-486: magic, frame headers).
    Returns (QOA_FRAME_DTYPE array, channels, samplerate, total samples per channel)."""
    b = np.frombuffer(file_bytes, np.uint8)
    if b.size < 16 or bytes(b[:4]) != b"qoaf":
        raise AfgError("not a QOA file")
    total = int.from_bytes(bytes(b[4:8]), "big")
    recs, pos, out = [], 8, out_base
    first = int.from_bytes(bytes(b[8:16]), "big")
    channels, rate = (first >> 56) & 0xff, (first >> 32) & 0xffffff
    if not total or not channels or not rate or channels > 8:
        raise AfgError("not a QOA file")
    # the reader of qoa.d:455-534: a frame is header + LMS state + ceil(samples / 20) slices per channel from the cursor;
    # the frame-size field is checked (:477, :481-486), never used to find the next frame
    while b.size - pos >= 8 + 16 * channels:
        hdr = int.from_bytes(bytes(b[pos:pos + 8]), "big")
        ch, sr, smp, fsz = (hdr >> 56) & 0xff, (hdr >> 32) & 0xffffff, (hdr >> 16) & 0xffff, hdr & 0xffff
        num_slices = int((fsz - 8 - 16 * ch) / 8)                    # truncating division, as D's
        if b.size - pos - 8 < fsz - 8:
            break
        if ch != channels or sr != rate or smp * ch > num_slices * 20 or smp == 0 or smp > 5120:
            break
        used = 8 + 16 * ch + 8 * ch * ((smp + 19) // 20)
        if used > b.size - pos:
            break
        recs.append((byte_base + pos, out, smp, ch, [0] * 5))
        out += smp * ch
        pos += used
    return np.array(recs, QOA_FRAME_DTYPE), channels, rate, total


def qoa_transform(n_frames, d_frames, d_bytes, d_out_i16=None, d_out_f32=None, stream=None):
    """Enqueue the QOA frame decode (afg_qoa_transform_hip)."""
    check(lib().afg_qoa_transform_hip(int(n_frames), _ptr(d_frames), _ptr(d_bytes), _ptr(d_out_i16),
                                      _ptr(d_out_f32), _stream(stream)))


def opus_output(n_samples, d_in, d_out_i16=None, d_out_f32=None, stream=None, gain=None):
    """Enqueue OpusFile.readFrame's float -> int16 (-> float / 32767) conversion (afg_opus_output_hip); gain: the decoder's
    output gain is applied first (afg_opus_output_gain_hip)."""
    if gain is None:
        check(lib().afg_opus_output_hip(int(n_samples), _ptr(d_in), _ptr(d_out_i16), _ptr(d_out_f32), _stream(stream)))
    else:
        check(lib().afg_opus_output_gain_hip(int(n_samples), _ptr(d_in), float(gain), _ptr(d_out_i16), _ptr(d_out_f32), _stream(stream)))


def qoa_encoded_size(samples, channels):
    return int(lib().afg_qoa_encoded_size(int(samples), int(channels)))


def qoa_encode(n_streams, d_streams, d_out, d_pcm_i16=None, d_pcm_f32=None, stream=None):
    """Enqueue the QOA encoder (afg_qoa_encode_hip): d_streams is a device array of QOA_ENC_STREAM_DTYPE."""
    check(lib().afg_qoa_encode_hip(int(n_streams), _ptr(d_streams), _ptr(d_pcm_i16), _ptr(d_pcm_f32), _ptr(d_out),
                                   _stream(stream)))


def qoa_encode_layout(shapes, samplerate=44100):
    """Stream table for interleaved PCM blocks laid back to back: shapes = [(frames, channels), ...].
    Returns (QOA_ENC_STREAM_DTYPE array, total input samples, total output bytes)."""
    recs = np.zeros(len(shapes), QOA_ENC_STREAM_DTYPE)
    pcm = out = 0
    for i, (n, ch) in enumerate(shapes):
        recs[i] = (pcm, out, n, samplerate, ch, 0)
        pcm += n * ch
        out += (qoa_encoded_size(n, ch) + 7) & ~7
    return recs, pcm, out


def wav_encode(samples, samplerate, fmt=WAV_FP32LE, dither=None, rng_max=0x7fffffff):
    """Host WAV writer: samples float32 [frames, channels] -> file bytes.  dither=None: afg_wav_encode (no dither);
    dither="libc": TPDF dither from libc rand() as the reference; dither=callable: draws in [0, rng_max] from it."""
    x = np.ascontiguousarray(samples, np.float32)
    if x.ndim == 1:
        x = x[:, None]
    frames, ch = x.shape
    size = int(lib().afg_wav_encoded_size(frames, ch, int(fmt)))
    if not size:
        raise AfgError("afg_wav_encode: bad arguments")
    out = np.zeros(size, np.uint8)
    if dither is None:
        n = int(lib().afg_wav_encode(x.ctypes.data, frames, ch, int(samplerate), int(fmt), out.ctypes.data, size))
    else:
        cb = RAND_FN() if dither == "libc" else RAND_FN(lambda _user: int(dither()))
        n = int(lib().afg_wav_encode_dithered(x.ctypes.data, frames, ch, int(samplerate), int(fmt), cb, None, int(rng_max),
                                              out.ctypes.data, size))
    if n != size:
        raise AfgError("afg_wav_encode failed")
    return out.tobytes()


def celt_transform(n_chan, d_rec_base, d_recs, d_coeffs, d_out, d_states=None, stream=None, tail_stream=None):
    """Enqueue the CELT transform stage (afg_celt_transform_hip; with tail_stream afg_celt_transform_streams_hip: the
    per-sequence passes go to that stream behind an event, the caller joins)."""
    if tail_stream is None:
        check(lib().afg_celt_transform_hip(int(n_chan), _ptr(d_rec_base), _ptr(d_recs), _ptr(d_coeffs), _ptr(d_out),
                                           _ptr(d_states), _stream(stream)))
    else:
        check(lib().afg_celt_transform_streams_hip(int(n_chan), _ptr(d_rec_base), _ptr(d_recs), _ptr(d_coeffs), _ptr(d_out),
                                                   _ptr(d_states), _stream(stream), _stream(tail_stream)))


def flac_parse(file_bytes):
    """Host front-end only (afg_flac_parse): returns (info dict, frames, subframes, residual planes) as numpy
    copies of the transform-stage records.  Needs no device."""
    buf = bytes(file_bytes)
    out = FlacParsed()
    check(lib().afg_flac_parse(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        info = {k: int(getattr(out, k)) for k in ("sample_rate", "channels", "bps", "max_block", "total_samples",
                                                  "out_samples")}
        return (info, view(out.frames, out.n_frames, FLAC_FRAME_DTYPE),
                view(out.subframes, out.n_subframes, FLAC_SUBFRAME_DTYPE), view(out.res, out.n_res, np.int32))
    finally:
        lib().afg_flac_parsed_free(C.byref(out))


def mp3_parse(file_bytes):
    """Host front-end only (afg_mp3_parse): (info dict, run_granules, coef [blocks, 576], flags, copies [n, 2])."""
    buf = bytes(file_bytes)
    out = Mp3Parsed()
    check(lib().afg_mp3_parse(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        info = {k: int(getattr(out, k)) for k in ("channels", "hz", "tagged", "start_delay", "detected_samples",
                                                  "declared_samples", "pcm_samples")}
        return (info, view(out.run_granules, out.n_runs, np.uint32),
                view(out.coef, out.n_blocks * 576, np.float32).reshape(-1, 576), view(out.flags, out.n_blocks, np.uint32),
                view(out.copies, out.n_copies * 2, np.uint64).reshape(-1, 2))
    finally:
        lib().afg_mp3_parsed_free(C.byref(out))


def mp3_parse_q(file_bytes):
    """Host front-end in quantised mode (afg_mp3_parse_q): (info, run_granules, q int16 [blocks, 576], flags, copies,
    granule records, stereo descriptors).  Raises AfgError (unsupported) for streams the device requantiser does not cover."""
    buf = bytes(file_bytes)
    out = Mp3ParsedQ()
    check(lib().afg_mp3_parse_q(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        b = out.base
        info = {k: int(getattr(b, k)) for k in ("channels", "hz", "tagged", "start_delay", "detected_samples",
                                                "declared_samples", "pcm_samples")}
        return (info, view(b.run_granules, b.n_runs, np.uint32), view(out.q, b.n_blocks * 576, np.int16).reshape(-1, 576),
                view(b.flags, b.n_blocks, np.uint32), view(b.copies, b.n_copies * 2, np.uint64).reshape(-1, 2),
                view(out.granules, out.n_granules, MP3_QGRANULE_DTYPE), view(out.sdesc, out.n_sdesc, MP3_SDESC_DTYPE))
    finally:
        lib().afg_mp3_parsed_q_free(C.byref(out))


def mp3_qtables():
    """afg_mp3_qtables: (band_of_line uint8 [24, 576], dst_of_src uint16 [24, 576], pow43 float32 [145])."""
    bol, dst, p43 = np.zeros((24, 576), np.uint8), np.zeros((24, 576), np.uint16), np.zeros(145, np.float32)
    fn = lib().afg_mp3_qtables
    fn.argtypes = [C.c_void_p] * 3
    fn.restype = None
    fn(bol.ctypes.data, dst.ctypes.data, p43.ctypes.data)
    return bol, dst, p43


def mp3_requant(n_granules, d_granules, d_q, d_sdesc, d_coef, stream=None):
    """Enqueue the MP3 requantisation (afg_mp3_requant_hip)."""
    check(lib().afg_mp3_requant_hip(int(n_granules), _ptr(d_granules), _ptr(d_q), _ptr(d_sdesc), _ptr(d_coef), _stream(stream)))


def vorbis_parse(file_bytes):
    """Host front-end only (afg_vorbis_parse): dict with channels, sample_rate, blocksize0/1, total_samples, pflags,
    spec, take_from, take_count, pcm_frames (numpy copies)."""
    buf = bytes(file_bytes)
    out = VorbisParsed()
    check(lib().afg_vorbis_parse(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        n = int(out.n_packets)
        return {"channels": out.channels, "sample_rate": out.sample_rate, "blocksize0": out.blocksize0,
                "blocksize1": out.blocksize1, "total_samples": int(out.total_samples), "pcm_frames": int(out.pcm_frames),
                "pflags": view(out.pflags, n, np.uint8), "spec": view(out.spec, int(out.spec_floats), np.float32),
                "take_from": view(out.take_from, n, np.int32), "take_count": view(out.take_count, n, np.int32)}
    finally:
        lib().afg_vorbis_parsed_free(C.byref(out))


def vorbis_parse_r(file_bytes):
    """afg_vorbis_parse_r: vorbis_parse's dict with `spec` holding residue vectors, plus the inputs of vorbis_floor:
    fl_packets (VORBIS_FLOOR_PACKET_DTYPE), fl_curves (VORBIS_FLOOR_CURVE_DTYPE), fl_points int32 [n, 2], fl_steps uint8 [n, 2]."""
    buf = bytes(file_bytes)
    out = VorbisParsedR()
    check(lib().afg_vorbis_parse_r(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        b = out.base
        n = int(b.n_packets)
        return {"channels": b.channels, "sample_rate": b.sample_rate, "blocksize0": b.blocksize0,
                "blocksize1": b.blocksize1, "total_samples": int(b.total_samples), "pcm_frames": int(b.pcm_frames),
                "pflags": view(b.pflags, n, np.uint8), "spec": view(b.spec, int(b.spec_floats), np.float32),
                "take_from": view(b.take_from, n, np.int32), "take_count": view(b.take_count, n, np.int32),
                "fl_packets": view(out.packets, n, VORBIS_FLOOR_PACKET_DTYPE),
                "fl_curves": view(out.curves, int(out.n_curves), VORBIS_FLOOR_CURVE_DTYPE),
                "fl_points": view(out.points, 2 * int(out.n_points), np.int32).reshape(-1, 2),
                "fl_steps": view(out.steps, 2 * int(out.n_steps), np.uint8).reshape(-1, 2)}
    finally:
        lib().afg_vorbis_parsed_r_free(C.byref(out))


def vorbis_floor(n_packets, d_packets, d_curves, d_points, d_steps, d_spec, stream=None):
    """afg_vorbis_floor_hip: inverse coupling + floor curves in place on the residue plane (device tensors; records as uint8
    views of the dtypes above)."""
    check(lib().afg_vorbis_floor_hip(int(n_packets), _ptr(d_packets), _ptr(d_curves), _ptr(d_points), _ptr(d_steps), _ptr(d_spec), _stream(stream)))


def opus_parse(file_bytes):
    """Host front-end only (afg_opus_parse): dict with channels, preskip, gain_i, gain, error, declared_frames, pcm_frames,
    frames (CELT_FRAME_DTYPE, channel 0's record per frame) and coeffs (numpy copies).  Raises AfgError for a stream that
    is not Ogg Opus or that holds SILK / hybrid packets."""
    buf = bytes(file_bytes)
    out = OpusParsed()
    check(lib().afg_opus_parse(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        return {"channels": out.channels, "preskip": out.preskip, "gain_i": out.gain_i, "gain": float(np.float32(out.gain)),
                "error": bool(out.error), "declared_frames": int(out.declared_frames), "pcm_frames": int(out.pcm_frames),
                "frames": view(out.frames, int(out.n_frames), CELT_FRAME_DTYPE),
                "coeffs": view(out.coeffs, int(out.n_coeffs), np.float32)}
    finally:
        lib().afg_opus_parsed_free(C.byref(out))


def qoa_parse(file_bytes):
    """afg_qoa_parse: (QOA_FRAME_DTYPE array, channels, samplerate, samples per channel)."""
    buf = bytes(file_bytes)
    ch, sr, smp, n = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib().afg_qoa_parse(buf, len(buf), C.byref(ch), C.byref(sr), C.byref(smp), None, 0, C.byref(n)))
    frames = np.zeros(n.value, QOA_FRAME_DTYPE)
    check(lib().afg_qoa_parse(buf, len(buf), None, None, None, frames.ctypes.data, n.value, None))
    return frames, ch.value, sr.value, smp.value


def mod_parse(file_bytes):
    """Host front-end only (afg_mod_parse): the batch path's control layer for one MOD file.  Returns a dict: channels,
    capped, frames, ticks (MOD_TICK_DTYPE), segments (MOD_SEGMENT_DTYPE), plane (uint8 sample area + padding).  Needs no
    device."""
    buf = bytes(file_bytes)
    out = ModParsed()
    check(lib().afg_mod_parse(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        return {"channels": int(out.channels), "capped": bool(out.capped), "frames": int(out.n_frames),
                "ticks": view(out.ticks, int(out.n_ticks), MOD_TICK_DTYPE),
                "segments": view(out.segments, int(out.n_segments), MOD_SEGMENT_DTYPE),
                "plane": view(out.sample_bytes, int(out.n_sample_bytes), np.uint8)}
    finally:
        lib().afg_mod_parsed_free(C.byref(out))


def mod_render(n_songs, d_songs, d_segments, d_ticks, d_sample_bytes, d_out, stream=None):
    """Enqueue the MOD mixer (afg_mod_render_hip) on device arrays."""
    check(lib().afg_mod_render_hip(int(n_songs), _ptr(d_songs), _ptr(d_segments), _ptr(d_ticks), _ptr(d_sample_bytes),
                                   _ptr(d_out), _stream(stream)))


def mod_layout(parsed_songs):
    """Concatenate afg_mod_parse results (dicts of mod_parse) into one launch: (songs, ticks, segments, plane, total
    frames) as numpy arrays, songs back to back in the output."""
    songs = np.zeros(len(parsed_songs), MOD_SONG_DTYPE)
    frames = ticks = segs = plane = 0
    for i, p in enumerate(parsed_songs):
        songs[i] = (frames, ticks, segs, plane, len(p["ticks"]), len(p["plane"]), 0)
        frames += p["frames"]
        ticks += len(p["ticks"])
        segs += len(p["segments"])
        plane += (len(p["plane"]) + 15) & ~15
    plane_arr = np.zeros(max(plane, 16), np.uint8)
    for i, p in enumerate(parsed_songs):
        plane_arr[int(songs[i]["sample_base"]):int(songs[i]["sample_base"]) + len(p["plane"])] = p["plane"]
    tick_arr = np.concatenate([p["ticks"] for p in parsed_songs]) if parsed_songs else np.zeros(0, MOD_TICK_DTYPE)
    seg_arr = np.concatenate([p["segments"] for p in parsed_songs] + [np.zeros(1, MOD_SEGMENT_DTYPE)])
    return songs, tick_arr, seg_arr, plane_arr, frames


def xm_parse(file_bytes):
    """Host front-end only (afg_xm_parse): the batch path's loader and control layer for one XM file.  Returns a dict:
    channels, length, patterns, instruments, restart, capped, frames, ticks (XM_TICK_DTYPE), segments (XM_SEGMENT_DTYPE),
    data (uint8: the delta-decoded samples), aux (float32 side table).  Needs no device."""
    buf = bytes(file_bytes)
    out = XmParsed()
    check(lib().afg_xm_parse(buf, len(buf), C.byref(out)))
    try:
        def view(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype)
            raw = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(raw, dtype=dtype, count=count).copy()
        return {"channels": int(out.channels), "length": int(out.length), "patterns": int(out.patterns),
                "instruments": int(out.instruments), "restart": int(out.restart), "capped": bool(out.capped),
                "frames": int(out.n_frames),
                "ticks": view(out.ticks, int(out.n_ticks), XM_TICK_DTYPE),
                "segments": view(out.segments, int(out.n_segments), XM_SEGMENT_DTYPE),
                "data": view(out.sample_bytes, int(out.n_sample_bytes), np.uint8),
                "aux": view(out.aux, int(out.n_aux), np.float32)}
    finally:
        lib().afg_xm_parsed_free(C.byref(out))


def xm_render(n_songs, d_songs, d_segments, d_ticks, d_sample_bytes, d_aux, d_out, stream=None):
    """Enqueue the XM mixer (afg_xm_render_hip) on device arrays."""
    check(lib().afg_xm_render_hip(int(n_songs), _ptr(d_songs), _ptr(d_segments), _ptr(d_ticks), _ptr(d_sample_bytes),
                                  _ptr(d_aux), _ptr(d_out), _stream(stream)))


def xm_layout(parsed_songs, align=16):
    """Concatenate afg_xm_parse results (dicts of xm_parse) into one launch: (songs, ticks, segments, data, aux, total
    frames) as numpy arrays; every song starts on a multiple of `align` output frames."""
    songs = np.zeros(len(parsed_songs), XM_SONG_DTYPE)
    frames = ticks = segs = data = aux = 0
    for i, p in enumerate(parsed_songs):
        songs[i] = (frames, ticks, segs, data, aux, len(p["ticks"]), len(p["data"]), (0, 0))
        frames += -(-p["frames"] // align) * align
        ticks += len(p["ticks"])
        segs += len(p["segments"])
        data += (len(p["data"]) + 15) & ~15
        aux += len(p["aux"])
    data_arr = np.zeros(max(data, 16), np.uint8)
    for i, p in enumerate(parsed_songs):
        data_arr[int(songs[i]["sample_base"]):int(songs[i]["sample_base"]) + len(p["data"])] = p["data"]
    tick_arr = np.concatenate([p["ticks"] for p in parsed_songs]) if parsed_songs else np.zeros(0, XM_TICK_DTYPE)
    seg_arr = np.concatenate([p["segments"] for p in parsed_songs] + [np.zeros(1, XM_SEGMENT_DTYPE)])
    aux_arr = np.concatenate([p["aux"] for p in parsed_songs] + [np.zeros(1, np.float32)])
    return songs, tick_arr, seg_arr, data_arr, aux_arr, frames


def wav_parse(file_bytes):
    """Host front-end only (afg_wav_parse): WAVDecoder.scan on one file.  Returns a dict: tag, channels, bits, sample_rate,
    frames (declared), kind (WAV_KIND_*, -1: the first read fails), samples_offset, present_samples.  Raises AfgError with
    the scan's reason when the file is refused.  Needs no device."""
    buf = bytes(file_bytes)
    out = WavParsed()
    check(lib().afg_wav_parse(buf, len(buf), C.byref(out)))
    return {name: int(getattr(out, name)) for name, _ in WavParsed._fields_}


def wav_layout(spans):
    """afg_wav_layout: fills tile_first of a WAV_SPAN_DTYPE array in place; returns the launch's tile count."""
    assert spans.dtype == WAV_SPAN_DTYPE and spans.flags.c_contiguous
    return int(lib().afg_wav_layout(spans.ctypes.data, len(spans)))


def wav_convert(n_spans, d_spans, n_tiles, d_in, in_bytes, d_out, out_floats, stream=None):
    """Enqueue the WAV sample conversion (afg_wav_convert_hip) on device arrays."""
    check(lib().afg_wav_convert_hip(int(n_spans), _ptr(d_spans), int(n_tiles), _ptr(d_in), int(in_bytes), _ptr(d_out),
                                    int(out_floats), _stream(stream)))


def pcm_to_f64(n_spans, d_spans, n_tiles, d_in, in_bytes, d_out, out_doubles, stream=None):
    """Enqueue the conversion to float64 (afg_pcm_to_f64_hip) on device arrays: WAV_SPAN_DTYPE records laid out by
    wav_layout, out_off / count in doubles, kinds WAV_KIND_* and F64_KIND_FLAC_S32."""
    check(lib().afg_pcm_to_f64_hip(int(n_spans), _ptr(d_spans), int(n_tiles), _ptr(d_in), int(in_bytes), _ptr(d_out),
                                   int(out_doubles), _stream(stream)))


def lcg31_jump(seed, n_draws):
    """afg_lcg31_jump: state of the dither generator after n_draws steps from seed.  Needs no device."""
    return int(lib().afg_lcg31_jump(int(seed) & 0xffffffff, int(n_draws)))


def wav_pack_layout(spans):
    """afg_wav_pack_layout: fills first_tile of a WAV_PACK_SPAN_DTYPE array in place; returns the launch's tile count."""
    assert spans.dtype == WAV_PACK_SPAN_DTYPE and spans.flags.c_contiguous
    return int(lib().afg_wav_pack_layout(spans.ctypes.data, len(spans)))


def wav_pack(n_spans, d_spans, n_tiles, d_in, in_floats, d_out, out_bytes, stream=None):
    """Enqueue the WAV sample packing (afg_wav_pack_hip) on device arrays."""
    check(lib().afg_wav_pack_hip(int(n_spans), _ptr(d_spans), int(n_tiles), _ptr(d_in), int(in_floats), _ptr(d_out),
                                 int(out_bytes), _stream(stream)))


def pcm_pack_layout(spans):
    """afg_pcm_pack_layout: fills first_tile of a PCM_PACK_SPAN_DTYPE array in place; returns the launch's tile count.
    Needs no device."""
    assert spans.dtype == PCM_PACK_SPAN_DTYPE and spans.flags.c_contiguous
    return int(lib().afg_pcm_pack_layout(spans.ctypes.data, len(spans)))


def pcm_pack(n_spans, d_spans, n_tiles, d_in, in_floats, d_out, out_bytes, stream=None):
    """Enqueue the decode stages' packer (afg_pcm_pack_hip) on device arrays: spans at any float / any byte."""
    check(lib().afg_pcm_pack_hip(int(n_spans), _ptr(d_spans), int(n_tiles), _ptr(d_in), int(in_floats), _ptr(d_out),
                                 int(out_bytes), _stream(stream)))


def encoding_options(sample_format=WAV_FP32LE, dither=DITHER_LIBC, dither_seed=0):
    return EncodingOptions(C.sizeof(EncodingOptions), int(sample_format), int(dither), int(dither_seed) & 0xffffffff)


def batch_encode(inputs, fmt=FORMAT_WAV, options=None, n_threads=0):
    """afg_batch_encode: inputs = [(float32 array [frames, channels] or [frames], samplerate), ...]; an input may also be a
    dict(pcm=, frames=, channels=, samplerate=) to describe an item as it is (pcm None = NULL).  Returns a list of dicts
    (status, message, bytes: the file as a bytes object, None on error)."""
    n = len(inputs)
    arr = (EncodeInput * max(n, 1))()
    keep = []
    for i, item in enumerate(inputs):
        if isinstance(item, dict):
            x = None if item.get("pcm") is None else np.ascontiguousarray(item["pcm"], np.float32)
            frames, ch, rate = item["frames"], item["channels"], item["samplerate"]
        else:
            x, rate = item
            x = np.ascontiguousarray(x, np.float32)
            if x.ndim == 1:
                x = x[:, None]
            frames, ch = x.shape
        keep.append(x)
        arr[i] = EncodeInput(None if x is None else x.ctypes.data, int(frames), int(ch), float(rate))
    res = EncodeResult()
    check(lib().afg_batch_encode(arr, n, int(fmt), None if options is None else C.byref(options), int(n_threads), C.byref(res)))
    try:
        out = []
        for i in range(res.n_files):
            it = res.items[i]
            out.append({"status": it.status, "message": None if it.message is None else it.message.decode(),
                        "bytes": C.string_at(it.bytes, it.size) if it.status == 0 else None})
        return out
    finally:
        lib().afg_encode_free(C.byref(res))


class AudioStream:
    """The reference's AudioStream (stream.d:102-902) over afg_open_from_memory and afg_open_to_buffer / _to_memory:
    same method names, same never-throw / error-state contract (stream.d:31-33)."""

    def __init__(self):
        self._h = None
        self._keep = None

    def openFromMemory(self, data):
        self.cleanUp()
        self._keep = bytes(data)
        self._h = lib().afg_open_from_memory(self._keep, len(self._keep))

    def openToBuffer(self, fmt, samplerate, channels, options=None):
        """options: encoding_options(...) or None for the reference's defaults."""
        self.cleanUp()
        self._h = lib().afg_open_to_buffer(int(fmt), float(samplerate), int(channels), None if options is None else C.byref(options))

    def openToMemory(self, out, fmt, samplerate, channels, options=None):
        """out: a writable uint8 numpy array the file is written into; it must outlive the stream."""
        self.cleanUp()
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable
        self._keep = out
        self._h = lib().afg_open_to_memory(out.ctypes.data, out.size, int(fmt), float(samplerate), int(channels),
                                           None if options is None else C.byref(options))

    def isOpenForReading(self):
        return bool(lib().afg_is_open_for_reading(self._h))

    def isOpenForWriting(self):
        return bool(lib().afg_is_open_for_writing(self._h))

    def _write(self, fn, data, dtype, frames):
        x = np.ascontiguousarray(data, dtype)
        if frames is None:
            frames = x.shape[0] if x.ndim == 2 else x.size // max(1, self.getNumChannels())
        return int(fn(self._h, x.ctypes.data, int(frames)))

    def writeSamplesFloat(self, data, frames=None):
        """data: float32 [frames, channels] or interleaved; returns the frames written."""
        return self._write(lib().afg_write_samples_float, data, np.float32, frames)

    def writeSamplesDouble(self, data, frames=None):
        return self._write(lib().afg_write_samples_double, data, np.float64, frames)

    def finalizeEncoding(self):
        return bool(lib().afg_finalize_encoding(self._h))

    def finalizeAndGetEncodedResult(self):
        """The encoded file of a buffer stream as bytes (may be called again); None when it failed."""
        p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        if not lib().afg_finalize_and_get_encoded(self._h, C.byref(p), C.byref(n)):
            return None
        return C.string_at(p, n.value)

    def cleanUp(self):
        if self._h:
            lib().afg_close(self._h)
        self._h = None

    __del__ = cleanUp

    def isError(self):
        return bool(lib().afg_is_error(self._h))

    def errorMessage(self):
        m = lib().afg_error_message(self._h)
        return None if m is None else m.decode()

    def getFormat(self):
        return int(lib().afg_get_format(self._h))

    def getNumChannels(self):
        return int(lib().afg_get_num_channels(self._h))

    def getLengthInFrames(self):
        return int(lib().afg_get_length_in_frames(self._h))

    def getSamplerate(self):
        return float(lib().afg_get_samplerate(self._h))

    def canSeek(self):
        return bool(lib().afg_can_seek(self._h))

    def seekPosition(self, frame, row=None):
        """seekPosition(frame), or on a module seekPosition(pattern, row) (stream.d:1059)."""
        if row is not None:
            return self.seekModulePosition(frame, row)
        return bool(lib().afg_seek_position(self._h, int(frame)))

    def tellPosition(self):
        return int(lib().afg_tell_position(self._h))

    # the module functions (stream.d:330-345, :906-1080); seekPosition(pattern, row) is the module form of seekPosition
    def isModule(self):
        return bool(lib().afg_is_module(self._h))

    def countModulePatterns(self):
        return int(lib().afg_module_pattern_count(self._h))

    def getModuleLength(self):
        return int(lib().afg_module_length(self._h))

    def rowsInPattern(self, pattern):
        return int(lib().afg_module_rows_in_pattern(self._h, int(pattern)))

    def tellModulePattern(self):
        return int(lib().afg_module_tell_pattern(self._h))

    def tellModuleRow(self):
        return int(lib().afg_module_tell_row(self._h))

    def seekModulePosition(self, pattern, row):
        return bool(lib().afg_module_seek(self._h, int(pattern), int(row)))

    def readSamplesFloat(self, out):
        """out: float32 numpy array whose size is a multiple of the channel count; returns frames read."""
        ch = max(1, self.getNumChannels())
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size % ch == 0
        return int(lib().afg_read_samples_float(self._h, out.ctypes.data, out.size // ch))

    def readSamplesDouble(self, out):
        """out: float64 numpy array whose size is a multiple of the channel count; returns frames read."""
        ch = max(1, self.getNumChannels())
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.size % ch == 0
        return int(lib().afg_read_samples_double(self._h, out.ctypes.data, out.size // ch))


class BatchDecoded:
    """Result of afg_batch_decode kept in the library's (page-locked) result plane: ``items[i]`` are dicts whose
    ``pcm`` arrays are views, valid until ``close()`` (or the end of a ``with`` block)."""

    def __init__(self, files, n_threads=0, devices=None, dtype=np.float32, sample_type=None, dither=DITHER_OFF, dither_seed=0):
        """devices: None = the current device; "all" = every visible device; or a list of device indices.
        dtype: np.float32, or np.float64 for the doubles of readSamplesDouble (afg_batch_opts.sample_type).
        sample_type (overrides dtype): SAMPLE_*; the SAMPLE_PCM_* types deliver uint8 (s8), int16 or uint8[..., 3] (s24)
        arrays, dithered as `dither` / `dither_seed` say (DITHER_OFF or DITHER_LCG31)."""
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("batch_decode delivers float32 or float64")
        self.sample_type = (SAMPLE_F64 if self.dtype == np.float64 else SAMPLE_F32) if sample_type is None else int(sample_type)
        self.dither, self.dither_seed = int(dither), int(dither_seed) & 0xffffffff
        self.devices = devices
        self._bufs = [bytes(f) for f in files]
        n = len(self._bufs)
        self._ptrs = (C.c_char_p * max(n, 1))(*self._bufs)
        self._lens = (C.c_size_t * max(n, 1))(*[len(b) for b in self._bufs])
        self._res = BatchResult()
        self._open = False
        self.n_threads = n_threads
        self._items = None

    def run(self):
        """The timed part: host parse + device restore + copy back -- the C call and nothing else (the per-file views of
        `items` are made when they are first asked for: two thousand numpy views cost more than some of these calls)."""
        self.close()
        opts = BatchOpts(C.sizeof(BatchOpts), self.n_threads, 0, None, self.sample_type, self.dither, self.dither_seed)
        if self.devices == "all":
            opts.n_devices = -1
        elif self.devices is not None:
            devs = (C.c_int * len(self.devices))(*[int(d) for d in self.devices])
            opts.n_devices, opts.devices = len(self.devices), devs
        check(lib().afg_batch_decode_ex(self._ptrs, self._lens, len(self._bufs), C.byref(opts), C.byref(self._res)))
        self._open = True
        self._items = None
        return self

    @property
    def items(self):
        if self._items is None:
            self._items = []
            if self._open:
                for i in range(self._res.n_files):
                    it = self._res.items[i]
                    cnt = it.frames * it.channels
                    dt, tail = _SAMPLE_VIEW[self.sample_type]
                    pcm = None
                    if cnt and it.pcm:
                        nbytes = cnt * np.dtype(dt).itemsize * (tail[0] if tail else 1)
                        raw = np.ctypeslib.as_array(C.cast(it.pcm, C.POINTER(C.c_uint8)), shape=(nbytes,))
                        pcm = raw.view(dt).reshape((-1, max(1, it.channels)) + tail)
                    self._items.append({"status": it.status, "message": None if it.message is None else it.message.decode(),
                                        "format": it.format, "channels": it.channels, "samplerate": it.samplerate,
                                        "frames": it.frames, "pcm": pcm})
        return self._items

    def close(self):
        if self._open:
            lib().afg_batch_free(C.byref(self._res))
            self._open = False
        self._items = None

    def __enter__(self):
        return self.run() if not self._open else self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


def set_device(device):
    """afg_set_device: make `device` current for the calling host thread (and keep torch's notion in step)."""
    check(lib().afg_set_device(int(device)))
    try:
        import torch
        torch.cuda.set_device(int(device))
    except Exception:  # pragma: no cover - torch is plumbing only
        pass


def get_device():
    d = int(lib().afg_get_device())
    if d < 0:
        check(d)
    return d


def batch_decode(files, n_threads=0, devices=None, dtype=np.float32, sample_type=None, dither=DITHER_OFF, dither_seed=0):
    """afg_batch_decode(_ex): list of dicts (status, message, format, channels, samplerate, frames, pcm ndarray copy of
    `dtype`: np.float32, or np.float64 for the doubles afg_read_samples_double returns).  sample_type = SAMPLE_PCM_S8 /
    _S16 / _S24: pcm is the WAV body made on the device, uint8 / int16 [frames, channels] or uint8 [frames, channels, 3]."""
    with BatchDecoded(files, n_threads, devices, dtype, sample_type, dither, dither_seed) as res:
        return [dict(it, pcm=None if it["pcm"] is None else it["pcm"].copy()) for it in res.items]


def collate_layout(spans):
    """afg_collate_layout: fills first_tile of a COLLATE_SPAN_DTYPE array in place; returns the launch's tile count."""
    assert spans.dtype == COLLATE_SPAN_DTYPE and spans.flags.c_contiguous
    return int(lib().afg_collate_layout(spans.ctypes.data, len(spans)))


def collate(n_spans, d_spans, n_tiles, d_in, in_floats, d_out, out_floats, stream=None):
    """Enqueue the collate kernel (afg_collate_hip) on device arrays: interleaved runs to planar, padded rows.  The spans
    are checked first (the call waits for `stream` to read them): AfgError, and nothing written, when one leaves a plane."""
    check(lib().afg_collate_hip(int(n_spans), _ptr(d_spans), int(n_tiles), _ptr(d_in), int(in_floats), _ptr(d_out),
                                int(out_floats), _stream(stream)))


def batch_decode_tensor(files, frames, channels, first_frame=None, out=None, n_threads=0):
    """afg_batch_decode_to_device: (tensor, meta).  tensor is a torch.float32 CUDA tensor [len(files), channels, frames] on
    the current device -- element [i, k, t] is sample (first_frame[i] + t) * channels_i + k of what batch_decode delivers for
    file i, 0 past the file's end, for a channel it does not have, and for a file that failed -- made on the device with no
    download; `out` (optional) is written in place of a new one.  meta: batch_decode's per-file dicts without pcm.
    The library works on HIP's current device of the calling thread, which must be torch's (afgpu.set_device keeps the two in
    step): ValueError otherwise.  torch's current stream is synchronised before the call, for a new tensor too -- torch's
    allocator hands a freed block out again at once and relies on stream order, which the library's own streams are not part of."""
    import torch
    bufs = [bytes(f) for f in files]
    n = len(bufs)
    frames, channels = int(frames), int(channels)
    if frames < 1 or channels < 1:
        raise ValueError("batch_decode_tensor: frames and channels must be at least 1")
    shape = (n, channels, frames)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    else:
        if tuple(out.shape) != shape or out.dtype != torch.float32:
            raise ValueError(f"batch_decode_tensor: out must be a float32 tensor of shape {shape}")
        if not out.is_cuda or out.device.index != torch.cuda.current_device():
            raise ValueError("batch_decode_tensor: out must live on the current device")
        if not out.is_contiguous():
            raise ValueError("batch_decode_tensor: out must be contiguous")
    if n == 0:
        return out, []
    if get_device() != torch.cuda.current_device():
        raise ValueError(f"batch_decode_tensor: HIP's current device is {get_device()}, torch's {torch.cuda.current_device()}")
    # Whatever is queued on `out` -- or, for a new tensor, on the block the allocator has just handed out again -- is over
    # before the library's streams, which torch's stream order does not cover, write it.
    torch.cuda.current_stream().synchronize()
    ff = None
    if first_frame is not None:
        if len(first_frame) != n:
            raise ValueError("batch_decode_tensor: one first_frame per file")
        ff = (C.c_int64 * n)(*[int(v) for v in first_frame])
    ptrs = (C.c_char_p * n)(*bufs)
    lens = (C.c_size_t * n)(*[len(b) for b in bufs])
    opts = CollateOpts(C.sizeof(CollateOpts), int(n_threads), channels, frames, ff)
    res = BatchResult()
    check(lib().afg_batch_decode_to_device(ptrs, lens, n, C.byref(opts), out.data_ptr(), C.byref(res)))
    try:
        meta = []
        for i in range(res.n_files):
            it = res.items[i]
            meta.append({"status": it.status, "message": None if it.message is None else it.message.decode(),
                         "format": it.format, "channels": it.channels, "samplerate": it.samplerate, "frames": it.frames})
        return out, meta
    finally:
        lib().afg_batch_free(C.byref(res))


def resample_taps(in_rate, out_rate, lowpass_width=0):
    """afg_resample_taps: (taps, M, L, W) -- the float32 table [L, 2 W] of the Hann-windowed sinc that takes in_rate to
    out_rate (include/afg.h has the definition); equal rates have no filter: an empty table, M = L = 1, W = 0.  Host only.
    AfgError for a rate of 0, a lowpass_width above 64, or a table of more than 2^22 floats."""
    L_ = lib()
    M, L, W = C.c_uint32(), C.c_uint32(), C.c_uint32()
    need = int(L_.afg_resample_taps(int(in_rate), int(out_rate), int(lowpass_width), None, 0, C.byref(M), C.byref(L), C.byref(W)))
    if M.value == 0:
        raise AfgError(f"afg: {L_.afg_last_error().decode()}")
    taps = np.zeros(need, np.float32)
    if need:
        L_.afg_resample_taps(int(in_rate), int(out_rate), int(lowpass_width), taps.ctypes.data, need, None, None, None)
    return taps.reshape(L.value, 2 * W.value), M.value, L.value, W.value


def resample_layout(rows):
    """afg_resample_layout: fills first_tile of a RESAMPLE_ROW_DTYPE array in place; returns the launch's tile count."""
    assert rows.dtype == RESAMPLE_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_resample_layout(rows.ctypes.data, len(rows)))


def resample(n_rows, d_rows, n_tiles, d_in, in_floats, d_taps, taps_floats, d_out, out_floats, stream=None):
    """Enqueue the resampling kernel (afg_resample_hip) on device arrays: planar rows at one rate, mixed to mono or not, to
    rows at another.  The rows are checked first (the call waits for `stream` to read them): AfgError, and nothing written,
    when one leaves a plane."""
    check(lib().afg_resample_hip(int(n_rows), _ptr(d_rows), int(n_tiles), _ptr(d_in), int(in_floats), _ptr(d_taps), int(taps_floats),
                                 _ptr(d_out), int(out_floats), _stream(stream)))


def batch_decode_tensor_resampled(files, frames, channels, samplerate, first_frame=None, mono=False, in_channels=0, max_in_rate=0,
                                  lowpass_width=0, out=None, n_threads=0):
    """afg_batch_decode_resampled: (tensor, meta) as batch_decode_tensor, with every file brought to `samplerate` (frames
    count at that rate; first_frame stays in each file's own frames) and, with mono (channels must be 1), mixed down to the
    mean of its channels first.  Files above max_in_rate (0: 48000 Hz), and with mono files of more than in_channels
    (0: 2) channels, are refused: status -5, a message, a zero slab.  lowpass_width: the filter's zero crossings (0: 6).
    The same device and stream rules as batch_decode_tensor."""
    import torch
    bufs = [bytes(f) for f in files]
    n = len(bufs)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_tensor_resampled: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_tensor_resampled: a mono tensor has one channel")
    shape = (n, channels, frames)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    else:
        if tuple(out.shape) != shape or out.dtype != torch.float32:
            raise ValueError(f"batch_decode_tensor_resampled: out must be a float32 tensor of shape {shape}")
        if not out.is_cuda or out.device.index != torch.cuda.current_device():
            raise ValueError("batch_decode_tensor_resampled: out must live on the current device")
        if not out.is_contiguous():
            raise ValueError("batch_decode_tensor_resampled: out must be contiguous")
    if n == 0:
        return out, []
    if get_device() != torch.cuda.current_device():
        raise ValueError(f"batch_decode_tensor_resampled: HIP's current device is {get_device()}, torch's {torch.cuda.current_device()}")
    torch.cuda.current_stream().synchronize()                # (as batch_decode_tensor: the library's streams are ordered with nobody's)
    ff = None
    if first_frame is not None:
        if len(first_frame) != n:
            raise ValueError("batch_decode_tensor_resampled: one first_frame per file")
        ff = (C.c_int64 * n)(*[int(v) for v in first_frame])
    ptrs = (C.c_char_p * n)(*bufs)
    lens = (C.c_size_t * n)(*[len(b) for b in bufs])
    opts = ResampleOpts(C.sizeof(ResampleOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                        int(max_in_rate), int(lowpass_width))
    res = BatchResult()
    check(lib().afg_batch_decode_resampled(ptrs, lens, n, C.byref(opts), out.data_ptr(), C.byref(res)))
    try:
        meta = []
        for i in range(res.n_files):
            it = res.items[i]
            meta.append({"status": it.status, "message": None if it.message is None else it.message.decode(),
                         "format": it.format, "channels": it.channels, "samplerate": it.samplerate, "frames": it.frames})
        return out, meta
    finally:
        lib().afg_batch_free(C.byref(res))


def mel_params(n_fft=400, hop=160, n_mels=80, win_length=None, center=True, pad_mode=MEL_PAD_REFLECT, out_kind=MEL_LOG10, log_floor=0.0):
    """afg_mel_params with Whisper's shape as the default (win_length None: n_fft)."""
    return MelParams(int(n_fft), int(n_fft if win_length is None else win_length), int(hop), int(n_mels), 1 if center else 0,
                     int(pad_mode), int(out_kind), float(log_floor))


def mel_basis(n_fft, win_length=None):
    """afg_mel_basis: the float32 table [win_length, 2 * nb16] -- the windowed cosines in columns [0, n_bins), the negated
    sines in [nb16, nb16 + n_bins), nb16 = n_bins rounded up to 16, zeros between (include/afg.h has the definition).
    Host only.  AfgError for n_fft outside 16 .. 2048 or win_length outside 1 .. n_fft."""
    L_ = lib()
    win = int(n_fft if win_length is None else win_length)
    need = int(L_.afg_mel_basis(int(n_fft), win, None, 0))
    if need == 0:
        raise AfgError(f"afg: {L_.afg_last_error().decode()}")
    out = np.zeros(need, np.float32)
    L_.afg_mel_basis(int(n_fft), win, out.ctypes.data, need)
    return out.reshape(win, need // win)


def mel_filters(samplerate, n_fft, n_mels, f_min=0.0, f_max=0.0, scale=MEL_SCALE_SLANEY, norm=MEL_NORM_SLANEY):
    """afg_mel_filters: the float32 bank [n_mels, n_fft // 2 + 1] (f_max 0: samplerate / 2).  Host only.  AfgError for
    arguments out of range."""
    L_ = lib()
    args = (int(samplerate), int(n_fft), int(n_mels), float(f_min), float(f_max), int(scale), int(norm))
    need = int(L_.afg_mel_filters(*args, None, 0))
    if need == 0:
        raise AfgError(f"afg: {L_.afg_last_error().decode()}")
    out = np.zeros(need, np.float32)
    L_.afg_mel_filters(*args, out.ctypes.data, need)
    return out.reshape(int(n_mels), need // int(n_mels))


def mel_frames(params, in_frames):
    """afg_mel_frames: the frames a row of in_frames samples has (max_frames of include/afg.h)."""
    return int(lib().afg_mel_frames(C.byref(params), int(in_frames)))


def mel_layout(rows, params):
    """afg_mel_layout: fills first_tile of a MEL_ROW_DTYPE array in place; returns the launch's tile count."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_mel_layout(rows.ctypes.data, len(rows), C.byref(params)))


def mel_check_rows(rows, n_tiles, params, in_floats, basis_floats, filters_floats, out_floats):
    """afg_mel_check_rows: what afg_melspec_hip checks before it launches, on host records.  AfgError when one fails."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    check(lib().afg_mel_check_rows(rows.ctypes.data, len(rows), int(n_tiles), C.byref(params), int(in_floats), int(basis_floats),
                                   int(filters_floats), int(out_floats)))


def melspec(n_rows, d_rows, n_tiles, params, d_in, in_floats, d_basis, basis_floats, d_filters, filters_floats, d_out, out_floats, stream=None):
    """Enqueue the mel spectrogram kernel (afg_melspec_hip) on device arrays: planar float rows to [rows, n_mels, out_frames].
    The parameters and the rows are checked first (the call waits for `stream` to read them): AfgError, and nothing written,
    when one fails."""
    check(lib().afg_melspec_hip(int(n_rows), _ptr(d_rows), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_basis),
                                int(basis_floats), _ptr(d_filters), int(filters_floats), _ptr(d_out), int(out_floats), _stream(stream)))


def _mel_algorithm(who, algorithm):
    if algorithm == "direct":
        return MEL_ALGO_DIRECT
    if algorithm == "fft":
        return MEL_ALGO_FFT
    raise ValueError(f"{who}: algorithm {algorithm!r}: 'direct' or 'fft'")


def mel_fft_tables(n_fft, win_length=None):
    """afg_mel_fft_tables: the float32 table of the FFT path, win_length window values then n_fft pairs (cos, -sin) of
    2 pi j / n_fft, as one array of win_length + 2 * n_fft floats.  Host only.  AfgError for sizes out of range or an n_fft
    with a prime factor other than 2, 3 and 5."""
    L_ = lib()
    win = int(n_fft if win_length is None else win_length)
    need = int(L_.afg_mel_fft_tables(int(n_fft), win, None, 0))
    if need == 0:
        raise AfgError(f"afg: {L_.afg_last_error().decode()}")
    out = np.zeros(need, np.float32)
    L_.afg_mel_fft_tables(int(n_fft), win, out.ctypes.data, need)
    return out


def mel_fft_layout(rows, params):
    """afg_mel_fft_layout: fills first_tile of a MEL_ROW_DTYPE array in place for the FFT path (tiles of 16 frames); returns
    the launch's tile count, 0 for parameters that path does not take."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_mel_fft_layout(rows.ctypes.data, len(rows), C.byref(params)))


def mel_fft_check_rows(rows, n_tiles, params, in_floats, table_floats, filters_floats, out_floats):
    """afg_mel_fft_check_rows: what afg_melspec_fft_hip checks before it launches, on host records.  AfgError when one fails."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    check(lib().afg_mel_fft_check_rows(rows.ctypes.data, len(rows), int(n_tiles), C.byref(params), int(in_floats), int(table_floats),
                                       int(filters_floats), int(out_floats)))


def melspec_fft(n_rows, d_rows, n_tiles, params, d_in, in_floats, d_table, table_floats, d_filters, filters_floats, d_out, out_floats, stream=None):
    """Enqueue the FFT mel spectrogram kernel (afg_melspec_fft_hip): melspec with mel_fft_tables' table in place of the basis
    and rows laid out by mel_fft_layout.  Checked like melspec: AfgError, and nothing written, when a check fails."""
    check(lib().afg_melspec_fft_hip(int(n_rows), _ptr(d_rows), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_table),
                                    int(table_floats), _ptr(d_filters), int(filters_floats), _ptr(d_out), int(out_floats), _stream(stream)))


def batch_decode_mel(files, frames, samplerate=16000, n_fft=400, hop=160, n_mels=80, win_length=None, center=True,
                     pad_mode=MEL_PAD_REFLECT, out_kind=MEL_LOG10, mono=True, out=None, channels=1, n_out=0, log_floor=0.0, f_min=0.0,
                     f_max=0.0, scale=MEL_SCALE_SLANEY, norm=MEL_NORM_SLANEY, first_frame=None, in_channels=0, max_in_rate=0,
                     lowpass_width=0, n_threads=0, algorithm="direct"):
    """afg_batch_decode_mel: (tensor, meta) as batch_decode_tensor_resampled, with the tensor [len(files), channels, n_mels,
    n_out] the (log-)mel spectrogram of every row of that call's tensor of `frames` samples at `samplerate` (include/afg.h
    has the definition).  n_out 0: every frame `frames` samples have.  algorithm "fft" computes the same features through an
    FFT per frame, held to include/afg.h's error bound instead of to bit patterns (n_fft with prime factors 2, 3 and 5 only).
    The same device and stream rules as batch_decode_tensor."""
    import torch
    algo = _mel_algorithm("batch_decode_mel", algorithm)
    bufs = [bytes(f) for f in files]
    n = len(bufs)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_mel: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_mel: a mono tensor has one channel")
    prm = mel_params(n_fft, hop, n_mels, win_length, center, pad_mode, out_kind, log_floor)
    most = mel_frames(prm, frames)
    if most == 0:
        raise ValueError(f"batch_decode_mel: {frames} samples hold no frame of these parameters ({lib().afg_last_error().decode()})")
    n_out = int(n_out)
    if n_out < 0 or n_out > most:
        raise ValueError(f"batch_decode_mel: n_out {n_out}, but {frames} samples have {most} frames")
    shape = (n, channels, int(n_mels), n_out if n_out else most)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    else:
        if tuple(out.shape) != shape or out.dtype != torch.float32:
            raise ValueError(f"batch_decode_mel: out must be a float32 tensor of shape {shape}")
        if not out.is_cuda or out.device.index != torch.cuda.current_device():
            raise ValueError("batch_decode_mel: out must live on the current device")
        if not out.is_contiguous():
            raise ValueError("batch_decode_mel: out must be contiguous")
    if n == 0:
        return out, []
    if get_device() != torch.cuda.current_device():
        raise ValueError(f"batch_decode_mel: HIP's current device is {get_device()}, torch's {torch.cuda.current_device()}")
    torch.cuda.current_stream().synchronize()                # (as batch_decode_tensor: the library's streams are ordered with nobody's)
    ff = None
    if first_frame is not None:
        if len(first_frame) != n:
            raise ValueError("batch_decode_mel: one first_frame per file")
        ff = (C.c_int64 * n)(*[int(v) for v in first_frame])
    ptrs = (C.c_char_p * n)(*bufs)
    lens = (C.c_size_t * n)(*[len(b) for b in bufs])
    opts = MelOpts(C.sizeof(MelOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                   int(max_in_rate), int(lowpass_width), n_out, prm, int(scale), int(norm), float(f_min), float(f_max), algorithm=algo, reserved=0)
    res = BatchResult()
    check(lib().afg_batch_decode_mel(ptrs, lens, n, C.byref(opts), out.data_ptr(), C.byref(res)))
    try:
        meta = []
        for i in range(res.n_files):
            it = res.items[i]
            meta.append({"status": it.status, "message": None if it.message is None else it.message.decode(),
                         "format": it.format, "channels": it.channels, "samplerate": it.samplerate, "frames": it.frames})
        return out, meta
    finally:
        lib().afg_batch_free(C.byref(res))


def norm_params(mode, target=1.0, eps=0.0, range=8.0, shift=4.0, gain=0.25):
    """afg_norm_params.  mode: NORM_* or its name ("none", "peak", "rms", "standard", "dynamic_range"); "whisper" is
    dynamic_range with range 8, shift 4, gain 0.25.  A NormParams passes through.  ValueError for an unknown name."""
    if isinstance(mode, NormParams):
        return mode
    if isinstance(mode, str):
        if mode == "whisper":
            return NormParams(NORM_DYNAMIC_RANGE, 1.0, 0.0, 8.0, 4.0, 0.25)
        if mode not in NORM_MODE_NAMES:
            raise ValueError(f"norm_params: unknown mode {mode!r}: one of {sorted(NORM_MODE_NAMES)} or 'whisper'")
        mode = NORM_MODE_NAMES[mode]
    return NormParams(int(mode), float(target), float(eps), float(range), float(shift), float(gain))


def norm_layout(groups):
    """afg_norm_layout: fills first_tile of a NORM_GROUP_DTYPE array in place; returns the launch's tile count."""
    assert groups.dtype == NORM_GROUP_DTYPE and groups.flags.c_contiguous
    return int(lib().afg_norm_layout(groups.ctypes.data, len(groups)))


def norm_check_groups(groups, n_tiles, params, in_floats, out_floats):
    """afg_norm_check_groups: what afg_normalize_hip checks before it launches, on host records.  AfgError when one fails."""
    assert groups.dtype == NORM_GROUP_DTYPE and groups.flags.c_contiguous
    check(lib().afg_norm_check_groups(groups.ctypes.data, len(groups), int(n_tiles), C.byref(params), int(in_floats), int(out_floats)))


def normalize(n_groups, d_groups, n_tiles, params, d_in, in_floats, d_out, out_floats, d_partials, d_stats, stream=None):
    """Enqueue the normalisation kernels (afg_normalize_hip) on device arrays: the statistics of every group into d_stats
    (NORM_STATS_DTYPE records), and -- unless the mode is NORM_NONE, where d_out may be None -- every valid element scaled into
    d_out (d_in itself for in place).  d_partials: n_tiles * 32 bytes.  The groups are checked first (the call waits for
    `stream` to read them): AfgError, and nothing written, when one fails."""
    check(lib().afg_normalize_hip(int(n_groups), _ptr(d_groups), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_out),
                                  int(out_floats), _ptr(d_partials), _ptr(d_stats), _stream(stream)))


def _batch_tensor_call(who, files, shape, out, first_frame, call):
    """What the normalised batch calls share: the output tensor checked or made, the file list as C arrays, call(ptrs, lens,
    n, first_frame array, out, result) run, and the items' metadata read.  Returns (out, meta)."""
    import torch
    bufs = [bytes(f) for f in files]
    n = len(bufs)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    else:
        if tuple(out.shape) != shape or out.dtype != torch.float32:
            raise ValueError(f"{who}: out must be a float32 tensor of shape {shape}")
        if not out.is_cuda or out.device.index != torch.cuda.current_device():
            raise ValueError(f"{who}: out must live on the current device")
        if not out.is_contiguous():
            raise ValueError(f"{who}: out must be contiguous")
    if n == 0:
        return out, []
    if get_device() != torch.cuda.current_device():
        raise ValueError(f"{who}: HIP's current device is {get_device()}, torch's {torch.cuda.current_device()}")
    torch.cuda.current_stream().synchronize()                # (as batch_decode_tensor: the library's streams are ordered with nobody's)
    ff = None
    if first_frame is not None:
        if len(first_frame) != n:
            raise ValueError(f"{who}: one first_frame per file")
        ff = (C.c_int64 * n)(*[int(v) for v in first_frame])
    ptrs = (C.c_char_p * n)(*bufs)
    lens = (C.c_size_t * n)(*[len(b) for b in bufs])
    res = BatchResult()
    check(call(ptrs, lens, n, ff, out, res))
    try:
        meta = []
        for i in range(res.n_files):
            it = res.items[i]
            meta.append({"status": it.status, "message": None if it.message is None else it.message.decode(),
                         "format": it.format, "channels": it.channels, "samplerate": it.samplerate, "frames": it.frames})
        return out, meta
    finally:
        lib().afg_batch_free(C.byref(res))


def batch_decode_tensor_normalized(files, frames, channels, samplerate, mode, target=1.0, eps=0.0, range=8.0, shift=4.0, gain=0.25,
                                   first_frame=None, mono=False, in_channels=0, max_in_rate=0, lowpass_width=0, out=None, n_threads=0,
                                   return_stats=False):
    """afg_batch_decode_resampled_norm: batch_decode_tensor_resampled, then every file normalised in place over its own
    samples -- its channel rows one group, the padding left out of the statistics and left as it is.  mode and its
    parameters: norm_params.  return_stats: (tensor, meta, stats), stats a NORM_STATS_DTYPE array with one record per file
    (all zero for a file that failed).  The same device and stream rules as batch_decode_tensor."""
    import torch
    prm = norm_params(mode, target, eps, range, shift, gain)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_tensor_normalized: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_tensor_normalized: a mono tensor has one channel")
    n = len(files)
    d_stats = torch.zeros(max(n, 1) * NORM_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda") if return_stats else None

    def call(ptrs, lens, n, ff, out, res):
        opts = ResampleOpts(C.sizeof(ResampleOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                            int(max_in_rate), int(lowpass_width))
        return lib().afg_batch_decode_resampled_norm(ptrs, lens, n, C.byref(opts), C.byref(prm), out.data_ptr(), _ptr(d_stats), C.byref(res))

    out, meta = _batch_tensor_call("batch_decode_tensor_normalized", files, (n, channels, frames), out, first_frame, call)
    if not return_stats:
        return out, meta
    return out, meta, d_stats.cpu().numpy().view(NORM_STATS_DTYPE)[:n].copy()


def batch_decode_mel_normalized(files, frames, samplerate=16000, n_fft=400, hop=160, n_mels=80, win_length=None, center=True,
                                pad_mode=MEL_PAD_REFLECT, out_kind=MEL_LOG10, mono=True, out=None, channels=1, n_out=0, log_floor=0.0,
                                f_min=0.0, f_max=0.0, scale=MEL_SCALE_SLANEY, norm=MEL_NORM_SLANEY, first_frame=None, in_channels=0,
                                max_in_rate=0, lowpass_width=0, n_threads=0, wave_norm=None, feat_norm=None, algorithm="direct"):
    """afg_batch_decode_mel_norm: batch_decode_mel with wave_norm applied to every file's samples in front of the features
    and feat_norm to every [n_mels, n_out] slab behind them.  Each is None, a NormParams (norm_params), or a mode name;
    feat_norm="whisper" is Whisper's max(x, x.max() - 8), then (x + 4) / 4.  algorithm as in batch_decode_mel."""
    algo = _mel_algorithm("batch_decode_mel_normalized", algorithm)
    wave = None if wave_norm is None else norm_params(wave_norm)
    feat = None if feat_norm is None else norm_params(feat_norm)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_mel_normalized: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_mel_normalized: a mono tensor has one channel")
    prm = mel_params(n_fft, hop, n_mels, win_length, center, pad_mode, out_kind, log_floor)
    most = mel_frames(prm, frames)
    if most == 0:
        raise ValueError(f"batch_decode_mel_normalized: {frames} samples hold no frame of these parameters ({lib().afg_last_error().decode()})")
    n_out = int(n_out)
    if n_out < 0 or n_out > most:
        raise ValueError(f"batch_decode_mel_normalized: n_out {n_out}, but {frames} samples have {most} frames")

    def call(ptrs, lens, n, ff, out, res):
        opts = MelOpts(C.sizeof(MelOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                       int(max_in_rate), int(lowpass_width), n_out, prm, int(scale), int(norm), float(f_min), float(f_max), algorithm=algo, reserved=0)
        return lib().afg_batch_decode_mel_norm(ptrs, lens, n, C.byref(opts), None if wave is None else C.byref(wave),
                                               None if feat is None else C.byref(feat), out.data_ptr(), C.byref(res))

    return _batch_tensor_call("batch_decode_mel_normalized", files, (len(files), channels, int(n_mels), n_out if n_out else most), out,
                              first_frame, call)


def cep_params(n_mels=80, n_ceps=13, delta_order=0, delta_win=2):
    """afg_cep_params: n_ceps coefficients of slabs of n_mels rows, delta_order planes of regression deltas over
    2 * delta_win + 1 frames behind them (torchaudio's win_length 5 is delta_win 2)."""
    return CepParams(int(n_mels), int(n_ceps), int(delta_order), int(delta_win))


def _cep_dct_norm(who, norm):
    if isinstance(norm, str):
        if norm not in CEP_DCT_NAMES:
            raise ValueError(f"{who}: dct norm {norm!r}: one of {sorted(CEP_DCT_NAMES)}")
        return CEP_DCT_NAMES[norm]
    return int(norm)


def cep_dct(n_ceps, n_mels, norm="ortho", lifter=0.0, log_scale=1.0):
    """afg_cep_dct: the float32 table [n_ceps, n_mels] of a DCT-II over the mel axis with its lifter (HTK / Kaldi: 1 +
    lifter / 2 * sin(pi q / lifter), q from 0; 0: none) and log_scale folded in (include/afg.h has the definition).  norm:
    "ortho", "none" or CEP_DCT_*.  Host only.  AfgError for arguments out of range."""
    L_ = lib()
    args = (int(n_ceps), int(n_mels), _cep_dct_norm("cep_dct", norm), float(lifter), float(log_scale))
    need = int(L_.afg_cep_dct(*args, None, 0))
    if need == 0:
        raise AfgError(f"afg: {L_.afg_last_error().decode()}")
    out = np.zeros(need, np.float32)
    L_.afg_cep_dct(*args, out.ctypes.data, need)
    return out.reshape(int(n_ceps), int(n_mels))


def cep_layout(rows, params):
    """afg_cep_layout: fills first_tile of a CEP_ROW_DTYPE array in place; returns the launch's tile count."""
    assert rows.dtype == CEP_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_cep_layout(rows.ctypes.data, len(rows), C.byref(params)))


def cep_check_rows(rows, n_tiles, params, in_floats, dct_floats, out_floats):
    """afg_cep_check_rows: what afg_cepstra_hip checks before it launches, on host records.  AfgError when one fails."""
    assert rows.dtype == CEP_ROW_DTYPE and rows.flags.c_contiguous
    check(lib().afg_cep_check_rows(rows.ctypes.data, len(rows), int(n_tiles), C.byref(params), int(in_floats), int(dct_floats),
                                   int(out_floats)))


def cepstra(n_rows, d_rows, n_tiles, params, d_in, in_floats, d_dct, dct_floats, d_out, out_floats, stream=None):
    """Enqueue the cepstral kernel (afg_cepstra_hip) on device arrays: [n_mels, frames] slabs to [(1 + delta_order) * n_ceps,
    frames] statics and deltas.  The parameters and the records are checked first (the call waits for `stream` to read
    them): AfgError, and nothing written, when one fails."""
    check(lib().afg_cepstra_hip(int(n_rows), _ptr(d_rows), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_dct),
                                int(dct_floats), _ptr(d_out), int(out_floats), _stream(stream)))


def batch_decode_mfcc(files, frames, n_mfcc=13, delta_order=0, delta_win=2, dct_norm="ortho", lifter=0, log_scale=1.0, cmvn=None,
                      wave_norm=None, algorithm="direct", samplerate=16000, n_fft=400, hop=160, n_mels=80, win_length=None, center=True,
                      pad_mode=MEL_PAD_REFLECT, mono=True, out=None, channels=1, n_out=0, log_floor=0.0, f_min=0.0, f_max=0.0,
                      scale=MEL_SCALE_SLANEY, norm=MEL_NORM_SLANEY, first_frame=None, in_channels=0, max_in_rate=0, lowpass_width=0,
                      n_threads=0):
    """afg_batch_decode_mfcc: (tensor, meta) as batch_decode_mel, with the tensor [len(files), channels, (1 + delta_order) *
    n_mfcc, n_out]: the cepstra (cep_dct of n_mfcc, n_mels, dct_norm, lifter, log_scale) of every log-mel slab
    batch_decode_mel_normalized(..., wave_norm=wave_norm) makes of the same list, their deltas and delta-deltas stacked
    behind them.  cmvn: None, a NormParams (norm_params) or a mode name, applied to every output row over its n_out frames;
    "standard" is per-coefficient mean and variance normalisation.  algorithm and the mel keywords as in batch_decode_mel."""
    algo = _mel_algorithm("batch_decode_mfcc", algorithm)
    dct = _cep_dct_norm("batch_decode_mfcc", dct_norm)
    wave = None if wave_norm is None else norm_params(wave_norm)
    rows = None if cmvn is None else norm_params(cmvn)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_mfcc: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_mfcc: a mono tensor has one channel")
    n_mfcc, delta_order = int(n_mfcc), int(delta_order)
    if n_mfcc < 1 or delta_order < 0:
        raise ValueError("batch_decode_mfcc: n_mfcc must be at least 1 and delta_order at least 0")
    prm = mel_params(n_fft, hop, n_mels, win_length, center, pad_mode, MEL_LOG10, log_floor)
    most = mel_frames(prm, frames)
    if most == 0:
        raise ValueError(f"batch_decode_mfcc: {frames} samples hold no frame of these parameters ({lib().afg_last_error().decode()})")
    n_out = int(n_out)
    if n_out < 0 or n_out > most:
        raise ValueError(f"batch_decode_mfcc: n_out {n_out}, but {frames} samples have {most} frames")

    def call(ptrs, lens, n, ff, out, res):
        mel = MelOpts(C.sizeof(MelOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                      int(max_in_rate), int(lowpass_width), n_out, prm, int(scale), int(norm), float(f_min), float(f_max), algorithm=algo, reserved=0)
        opts = MfccOpts(C.sizeof(MfccOpts), dct, mel, cep_params(n_mels, n_mfcc, delta_order, delta_win), float(lifter), float(log_scale))
        return lib().afg_batch_decode_mfcc(ptrs, lens, n, C.byref(opts), None if wave is None else C.byref(wave),
                                           None if rows is None else C.byref(rows), out.data_ptr(), C.byref(res))

    return _batch_tensor_call("batch_decode_mfcc", files, (len(files), channels, (1 + delta_order) * n_mfcc, n_out if n_out else most), out,
                              first_frame, call)


def trim_params(top_db=60.0, frame_length=2048, hop=512, reference="max", abs_power=1.0, lead=0, trail=0):
    """afg_trim_params with librosa.effects.trim's defaults: a frame is silent when its power lies top_db decibels or more
    below the reference -- ratio = 10 ** (-top_db / 10), computed here in double: the library never sees decibels.
    reference: TRIM_REF_* or its name, "max" (the loudest frame) or "abs" (abs_power, a mean square per sample).  lead, trail:
    samples kept in front of and behind the region.  ValueError for an unknown reference; the ranges are the library's to
    check."""
    if isinstance(reference, str):
        if reference not in TRIM_REF_NAMES:
            raise ValueError(f"trim_params: unknown reference {reference!r}: one of {sorted(TRIM_REF_NAMES)}")
        reference = TRIM_REF_NAMES[reference]
    return TrimParams(int(frame_length), int(hop), int(reference), int(lead), int(trail), (C.c_uint32 * 3)(0, 0, 0),
                      10.0 ** (-float(top_db) / 10.0), float(abs_power))


def trim_layout(groups, params):
    """afg_trim_layout: fills first_block and first_tile of a TRIM_GROUP_DTYPE array in place; returns (n_blocks, n_tiles).
    AfgError for parameters out of range."""
    assert groups.dtype == TRIM_GROUP_DTYPE and groups.flags.c_contiguous
    L = lib()
    n_blocks, n_tiles = C.c_uint64(), C.c_uint64()
    if not L.afg_trim_layout(groups.ctypes.data, len(groups), C.byref(params), C.byref(n_blocks), C.byref(n_tiles)):
        raise AfgError(f"afg: {L.afg_last_error().decode()}")
    return n_blocks.value, n_tiles.value


def trim_check_groups(groups, n_blocks, n_tiles, params, in_floats, out_floats):
    """afg_trim_check_groups: what afg_trim_hip checks before it launches, on host records.  AfgError when one fails."""
    assert groups.dtype == TRIM_GROUP_DTYPE and groups.flags.c_contiguous
    check(lib().afg_trim_check_groups(groups.ctypes.data, len(groups), int(n_blocks), int(n_tiles), C.byref(params), int(in_floats),
                                      int(out_floats)))


def trim(n_groups, d_groups, n_blocks, n_tiles, params, d_in, in_floats, d_out, out_floats, d_blocks, d_regions, stream=None):
    """Enqueue the trim kernels (afg_trim_hip) on device arrays: every group's block powers into d_blocks (n_blocks doubles),
    its region into d_regions (TRIM_REGION_DTYPE records), and its rows from `begin` on into its output slab, zeros behind
    them.  The groups are checked first (the call waits for `stream` to read them): AfgError, and nothing written, when one
    fails or the planes overlap."""
    check(lib().afg_trim_hip(int(n_groups), _ptr(d_groups), int(n_blocks), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats),
                             _ptr(d_out), int(out_floats), _ptr(d_blocks), _ptr(d_regions), _stream(stream)))


def batch_decode_tensor_trimmed(files, frames, channels, samplerate, scan_frames=None, top_db=60.0, frame_length=2048, hop=512,
                                reference="max", abs_power=1.0, lead=0, trail=0, trim=None, first_frame=None, mono=False, in_channels=0,
                                max_in_rate=0, lowpass_width=0, out=None, n_threads=0):
    """afg_batch_decode_trimmed: (tensor, meta) as batch_decode_tensor_resampled, with every file's slab starting at the
    begin of its non-silent region: scan_frames (None: frames) frames at `samplerate` from first_frame on are decoded and
    examined, and the first `frames` of [begin, end) are delivered, zeros behind them.  The trim parameters: trim_params'
    keywords, or a TrimParams as `trim`.  meta[i] has "begin" and "end" added, in frames at `samplerate` from first_frame.
    The same device and stream rules as batch_decode_tensor; ValueError for arguments out of range, before any call."""
    prm = trim if isinstance(trim, TrimParams) else trim_params(top_db, frame_length, hop, reference, abs_power, lead, trail)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_tensor_trimmed: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_tensor_trimmed: a mono tensor has one channel")
    scan = frames if scan_frames is None else int(scan_frames)
    if scan < frames or scan > 0xffffffff:
        raise ValueError(f"batch_decode_tensor_trimmed: scan_frames {scan} must be at least frames ({frames}) and below 2^32")
    L = lib()
    if L.afg_trim_check_groups(None, 0, 0, 0, C.byref(prm), 0, 0) != 0:
        raise ValueError(f"batch_decode_tensor_trimmed: {L.afg_last_error().decode()}")
    n = len(files)
    regions = np.zeros(max(n, 1), TRIM_REGION_DTYPE)

    def call(ptrs, lens, n, ff, out, res):
        opts = ResampleOpts(C.sizeof(ResampleOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                            int(max_in_rate), int(lowpass_width))
        return L.afg_batch_decode_trimmed(ptrs, lens, n, C.byref(opts), C.byref(prm), scan, out.data_ptr(), regions.ctypes.data, C.byref(res))

    out, meta = _batch_tensor_call("batch_decode_tensor_trimmed", files, (n, channels, frames), out, first_frame, call)
    for i, m in enumerate(meta):
        m["begin"], m["end"] = int(regions[i]["begin"]), int(regions[i]["end"])
    return out, meta


def biquad(kind, samplerate=1.0, f0=0.0, q=0.7071067811865476, gain_db=0.0):
    """afg_biquad_design: the section (b0, b1, b2, a1, a2), a0 == 1, of one of BIQUAD_KINDS -- the Audio EQ Cookbook's
    kinds at f0 Hz with quality q (and gain_db for "peaking" and the shelves), "preemphasis" with its coefficient in f0, and
    "dc_block" with its corner in f0.  ValueError for what the helper refuses."""
    if kind not in BIQUAD_KINDS:
        raise ValueError(f"biquad: unknown kind {kind!r}: one of {sorted(BIQUAD_KINDS)}")
    out = Biquad()
    L = lib()
    if L.afg_biquad_design(BIQUAD_KINDS[kind], float(samplerate), float(f0), float(q), float(gain_db), C.byref(out)) != 0:
        raise ValueError(f"biquad: {L.afg_last_error().decode()}")
    return (out.b0, out.b1, out.b2, out.a1, out.a2)


def filter_params(sos):
    """afg_filter_params of a cascade: a sequence of 1 .. 8 sections (b0, b1, b2, a1, a2), or scipy's rows of six with
    a0 == 1.  Not checked here beyond its shape: the library refuses what it does not take."""
    if isinstance(sos, FilterParams):
        return sos
    rows = [tuple(float(v) for v in r) for r in np.atleast_2d(np.asarray(sos, dtype=np.float64))]
    if len(rows) > 8 or any(len(r) not in (5, 6) for r in rows):
        raise ValueError("filter_params: 1 .. 8 sections of (b0, b1, b2, a1, a2) or (b0, b1, b2, 1, a1, a2)")
    p = FilterParams()
    p.n_sections = len(rows)
    for k, r in enumerate(rows):
        if len(r) == 6:
            if r[3] != 1.0:
                raise ValueError("filter_params: a section of six numbers must have a0 == 1")
            r = r[:3] + r[4:]
        p.sec[k] = Biquad(*r)
    return p


def filter_bound(sos):
    """afg_filter_bound: E / max|x| of the cascade's interval (include/afg.h).  ValueError for a refused cascade."""
    L = lib()
    e = L.afg_filter_bound(C.byref(filter_params(sos)))
    if not e > 0.0:
        raise ValueError(f"filter_bound: {L.afg_last_error().decode()}")
    return e


def filter_check_rows(rows, sos, in_floats, out_floats, same_plane):
    """afg_filter_check_rows: what afg_filter_hip checks before it launches, on host records.  AfgError when one fails."""
    rows = np.ascontiguousarray(rows, dtype=FILTER_ROW_DTYPE)
    check(lib().afg_filter_check_rows(rows.ctypes.data, len(rows), C.byref(filter_params(sos)), int(in_floats), int(out_floats), 1 if same_plane else 0))


def filter_rows(n_rows, d_rows, sos, d_in, in_floats, d_out, out_floats, d_state=None, stream=None):
    """Enqueue the filter kernel (afg_filter_hip) on device arrays: row k of d_rows (FILTER_ROW_DTYPE records) from d_in to
    d_out -- the same tensor for in place -- through the cascade `sos`; d_state is None or n_rows * n_sections * 4 doubles,
    read as the rows' history and overwritten with the history behind their last frames."""
    check(lib().afg_filter_hip(int(n_rows), _ptr(d_rows), C.byref(filter_params(sos)), _ptr(d_in), int(in_floats), _ptr(d_out), int(out_floats),
                               _ptr(d_state), _stream(stream)))


def filter_tensor(t, sos, valid=None, state=None, out=None):
    """Filter every row of a contiguous float32 device tensor along its last axis through the cascade `sos` (afg_filter_hip,
    one launch on the current stream).  valid: None, or one length per row (the tensor's leading axes flattened): only
    that many frames of the row are read and written.  state: None (zero history), or a float64 device tensor of shape
    t.shape[:-1] + (n_sections, 4) that is read and updated -- a stream filtered in pieces.  out: None (a new tensor), `t`
    itself (in place) or another contiguous tensor of t's shape that does not overlap it; what lies behind `valid` in it is
    left as it is (zero in a new tensor).  Returns out."""
    import torch
    prm = filter_params(sos)
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1:
        raise ValueError("filter_tensor: a contiguous float32 device tensor with at least one axis")
    frames = int(t.shape[-1])
    n = t.numel() // frames if frames else 0
    if out is None:
        out = torch.zeros_like(t) if valid is not None else torch.empty_like(t)
    elif out.shape != t.shape or out.dtype != t.dtype or out.device != t.device or not out.is_contiguous():
        raise ValueError("filter_tensor: out must be a contiguous tensor of t's shape, dtype and device")
    if state is not None and (state.dtype != torch.float64 or state.device != t.device or not state.is_contiguous()
                              or tuple(state.shape) != tuple(t.shape[:-1]) + (prm.n_sections, 4)):
        raise ValueError(f"filter_tensor: state must be a contiguous float64 tensor of shape {tuple(t.shape[:-1]) + (prm.n_sections, 4)} on t's device")
    if frames >= 1 << 32:
        raise ValueError("filter_tensor: rows of 2^32 frames or more")
    rows = np.zeros(n, FILTER_ROW_DTYPE)
    rows["in_off"] = rows["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(frames)
    rows["frames"] = frames
    if valid is not None:
        v = np.asarray(valid.cpu() if hasattr(valid, "cpu") else valid).reshape(-1)
        if v.size != n or (v < 0).any() or (v > frames).any():
            raise ValueError("filter_tensor: valid holds one length per row, 0 .. the last axis")
        rows["frames"] = v
    if n == 0:
        if lib().afg_filter_check_rows(None, 0, C.byref(prm), 0, 0, 0) != 0:
            raise ValueError(f"filter_tensor: {lib().afg_last_error().decode()}")
        return out
    with torch.cuda.device(t.device):
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(t.device)
        filter_rows(n, d_rows, prm, t, t.numel(), out, out.numel(), state, torch.cuda.current_stream().cuda_stream)
    return out


def batch_decode_tensor_filtered(files, frames, channels, samplerate, sos, first_frame=None, mono=False, in_channels=0, max_in_rate=0,
                                 lowpass_width=0, out=None, n_threads=0):
    """afg_batch_decode_filtered: batch_decode_tensor_resampled, then every file's rows filtered in place through the cascade
    `sos` over their own samples -- the rows and lengths of batch_decode_tensor_normalized --, the padding left +0.0.
    Returns (tensor, meta).  The same device and stream rules as batch_decode_tensor."""
    prm = filter_params(sos)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_tensor_filtered: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_tensor_filtered: a mono tensor has one channel")
    L = lib()
    if L.afg_filter_check_rows(None, 0, C.byref(prm), 0, 0, 0) != 0:
        raise ValueError(f"batch_decode_tensor_filtered: {L.afg_last_error().decode()}")

    def call(ptrs, lens, n, ff, out, res):
        opts = ResampleOpts(C.sizeof(ResampleOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                            int(max_in_rate), int(lowpass_width))
        return L.afg_batch_decode_filtered(ptrs, lens, n, C.byref(opts), C.byref(prm), out.data_ptr(), C.byref(res))

    return _batch_tensor_call("batch_decode_tensor_filtered", files, (len(files), channels, frames), out, first_frame, call)


def kweight_design(samplerate):
    """afg_kweight_design: the two sections (b0, b1, b2, a1, a2) of BS.1770's K-weighting at `samplerate` (8000 .. 192000 Hz), the
    shelf and the high-pass -- a cascade filter_tensor takes as it is.  Host only.  ValueError for a rate out of range."""
    out = FilterParams()
    L = lib()
    if L.afg_kweight_design(int(samplerate), C.byref(out)) != 0:
        raise ValueError(f"kweight_design: {L.afg_last_error().decode()}")
    return [(q.b0, q.b1, q.b2, q.a1, q.a2) for q in out.sec[:2]]


def loudness_lufs(energy):
    """afg_loudness_lufs: -0.691 + 10 log10(energy), -inf for 0: the integrated loudness of a record's energy."""
    return float(lib().afg_loudness_lufs(float(energy)))


def loudness_params(samplerate, target_lufs=-23.0, max_peak=0.0, max_gain=0.0, apply=True, weights=None):
    """afg_loudness_params.  weights: None (every row 1) or up to 8 channel weights G_i -- BS.1770's 5.1 order is
    (1, 1, 1, 0, 1.41, 1.41).  A LoudnessParams passes through.  The ranges are the library's to check."""
    if isinstance(samplerate, LoudnessParams):
        return samplerate
    w = [0.0] * 8
    if weights is not None:
        weights = [float(v) for v in weights]
        if len(weights) > 8:
            raise ValueError("loudness_params: at most 8 channel weights")
        w[:len(weights)] = weights
    return LoudnessParams(int(samplerate), 1 if apply else 0, float(target_lufs), float(max_peak), float(max_gain), (C.c_double * 8)(*w),
                          (C.c_uint32 * 2)(0, 0))


def loudness_layout(groups, params):
    """afg_loudness_layout: fills first_sub and first_block of a LOUDNESS_GROUP_DTYPE array in place; returns the
    LoudnessCounts of the launch.  AfgError for parameters out of range."""
    assert groups.dtype == LOUDNESS_GROUP_DTYPE and groups.flags.c_contiguous
    L = lib()
    counts = LoudnessCounts()
    if not L.afg_loudness_layout(groups.ctypes.data, len(groups), C.byref(params), C.byref(counts)):
        raise AfgError(f"afg: {L.afg_last_error().decode()}")
    return counts


def loudness_check_groups(groups, counts, params, in_floats, out_floats, same_plane):
    """afg_loudness_check_groups: what afg_loudness_hip checks before it launches, on host records.  AfgError when one fails."""
    assert groups.dtype == LOUDNESS_GROUP_DTYPE and groups.flags.c_contiguous
    check(lib().afg_loudness_check_groups(groups.ctypes.data, len(groups), C.byref(counts), C.byref(params), int(in_floats), int(out_floats),
                                          1 if same_plane else 0))


def loudness(n_groups, d_groups, counts, params, d_in, in_floats, d_out, out_floats, d_sub, d_blocks, d_stats, stream=None):
    """Enqueue the loudness kernels (afg_loudness_hip) on device arrays: every group's block energies z_j into d_blocks
    (counts.n_blocks doubles), its record into d_stats (LOUDNESS_STATS_DTYPE records) and -- with params.apply -- its valid
    elements times the gain into d_out (d_in itself for in place; None when measuring only).  d_sub: counts.n_sub doubles of
    scratch.  The groups are checked first (the call waits for `stream` to read them): AfgError, and nothing written, when
    one fails."""
    check(lib().afg_loudness_hip(int(n_groups), _ptr(d_groups), C.byref(counts), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_out),
                                 int(out_floats), _ptr(d_sub), _ptr(d_blocks), _ptr(d_stats), _stream(stream)))


def loudness_tensor(t, valid=None, samplerate=16000, target_lufs=-23.0, max_peak=0.0, max_gain=0.0, apply=True, weights=None, out=None,
                    params=None):
    """Measure the integrated loudness (BS.1770-4) of every group of a contiguous float32 device tensor [..., channels, frames]
    -- the channel axis, 8 rows at the most, is one group; the leading axes are flattened -- and, with apply, bring it to
    target_lufs (afg_loudness_hip, on the current stream).  valid: None, or one length per group: only that many frames of
    its rows count and are touched.  out: None (a new tensor, a copy of t behind `valid`), `t` itself (in place) or another
    contiguous tensor of t's shape that does not overlap it.  params: a LoudnessParams instead of the keywords.  Returns
    (out, stats): stats a LOUDNESS_STATS_DTYPE array with one record per group (loudness_lufs(energy) is its loudness); out
    is None when apply is off."""
    import torch
    prm = params if isinstance(params, LoudnessParams) else loudness_params(samplerate, target_lufs, max_peak, max_gain, apply, weights)
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 2:
        raise ValueError("loudness_tensor: a contiguous float32 device tensor [..., channels, frames]")
    rows, frames = int(t.shape[-2]), int(t.shape[-1])
    if rows < 1 or rows > 8 or frames >= 1 << 32:
        raise ValueError("loudness_tensor: 1 .. 8 channels of fewer than 2^32 frames")
    n = t.numel() // (rows * frames) if frames else 0
    L = lib()
    if L.afg_loudness_check_groups(None, 0, None, C.byref(prm), 0, 0, 0) != 0:
        raise ValueError(f"loudness_tensor: {L.afg_last_error().decode()}")
    if not prm.apply:
        if out is not None:
            raise ValueError("loudness_tensor: out without apply")
    elif out is None:
        out = t.clone() if valid is not None else torch.empty_like(t)
    elif out.shape != t.shape or out.dtype != t.dtype or out.device != t.device or not out.is_contiguous():
        raise ValueError("loudness_tensor: out must be a contiguous tensor of t's shape, dtype and device")
    groups = np.zeros(n, LOUDNESS_GROUP_DTYPE)
    groups["in_off"] = groups["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(rows * frames)
    groups["stride"], groups["rows"], groups["valid"] = frames, rows, frames
    if valid is not None:
        v = np.asarray(valid.cpu() if hasattr(valid, "cpu") else valid).reshape(-1)
        if v.size != n or (v < 0).any() or (v > frames).any():
            raise ValueError("loudness_tensor: valid holds one length per group, 0 .. the last axis")
        groups["valid"] = v
    if n == 0:
        return out, np.zeros(0, LOUDNESS_STATS_DTYPE)
    counts = loudness_layout(groups, prm)
    with torch.cuda.device(t.device):
        d_groups = torch.from_numpy(groups.view(np.uint8)).to(t.device)
        d_sub = torch.empty(max(counts.n_sub, 1), dtype=torch.float64, device=t.device)
        d_blocks = torch.empty(max(counts.n_blocks, 1), dtype=torch.float64, device=t.device)
        d_stats = torch.zeros(n * LOUDNESS_STATS_DTYPE.itemsize, dtype=torch.uint8, device=t.device)
        loudness(n, d_groups, counts, prm, t, t.numel(), out, out.numel() if out is not None else 0, d_sub, d_blocks, d_stats,
                 torch.cuda.current_stream().cuda_stream)
        stats = d_stats.cpu().numpy().view(LOUDNESS_STATS_DTYPE).copy()
    return out, stats


def batch_decode_tensor_loudnorm(files, frames, channels, samplerate, target_lufs=-23.0, max_peak=0.0, max_gain=0.0, apply=True, weights=None,
                                 first_frame=None, mono=False, in_channels=0, max_in_rate=0, lowpass_width=0, out=None, n_threads=0):
    """afg_batch_decode_loudnorm: batch_decode_tensor_resampled, then every file measured after BS.1770-4 over its own samples
    -- its channel rows one group, the rows and lengths of batch_decode_tensor_normalized -- and, with apply, brought to
    target_lufs in place; the padding is left as it is.  Returns (tensor, meta, stats): stats a LOUDNESS_STATS_DTYPE array
    with one record per file (zero with gain 1 for a file that failed).  The same device and stream rules as
    batch_decode_tensor; ValueError for arguments out of range, before any call."""
    prm = loudness_params(samplerate, target_lufs, max_peak, max_gain, apply, weights)
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_tensor_loudnorm: frames, channels and samplerate must be at least 1")
    if channels > 8:
        raise ValueError("batch_decode_tensor_loudnorm: at most 8 channels")
    if mono and channels != 1:
        raise ValueError("batch_decode_tensor_loudnorm: a mono tensor has one channel")
    L = lib()
    if L.afg_loudness_check_groups(None, 0, None, C.byref(prm), 0, 0, 0) != 0:
        raise ValueError(f"batch_decode_tensor_loudnorm: {L.afg_last_error().decode()}")
    n = len(files)
    stats = np.zeros(max(n, 1), LOUDNESS_STATS_DTYPE)

    def call(ptrs, lens, n, ff, out, res):
        opts = ResampleOpts(C.sizeof(ResampleOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                            int(max_in_rate), int(lowpass_width))
        return L.afg_batch_decode_loudnorm(ptrs, lens, n, C.byref(opts), C.byref(prm), out.data_ptr(), stats.ctypes.data, C.byref(res))

    out, meta = _batch_tensor_call("batch_decode_tensor_loudnorm", files, (n, channels, frames), out, first_frame, call)
    return out, meta, stats[:n].copy()


def mix_ratio(snr_db):
    """afg_mix_ratio: 10^(-snr_db / 10) in double, as the host computes it for an afg_mix_group in MIX_SNR mode."""
    return float(lib().afg_mix_ratio(float(snr_db)))


def mix_layout(groups):
    """afg_mix_layout: fills first_tile of a MIX_GROUP_DTYPE array in place; returns the launch's tile count."""
    assert groups.dtype == MIX_GROUP_DTYPE and groups.flags.c_contiguous
    return int(lib().afg_mix_layout(groups.ctypes.data, len(groups)))


def mix_check_groups(groups, n_tiles, in_floats, noise_floats, out_floats, plane_at=None):
    """afg_mix_check_groups: what afg_mix_hip checks before it launches, on host records.  plane_at: None (three separate
    planes) or the float indices of the first float of the input, noise and output plane in one address space.  AfgError when
    a check fails."""
    assert groups.dtype == MIX_GROUP_DTYPE and groups.flags.c_contiguous
    at = None if plane_at is None else (C.c_uint64 * 3)(*[int(v) for v in plane_at])
    check(lib().afg_mix_check_groups(groups.ctypes.data, len(groups), int(n_tiles), int(in_floats), int(noise_floats), int(out_floats), at))


def mix(n_groups, d_groups, n_tiles, d_in, in_floats, d_noise, noise_floats, d_out, out_floats, d_partials, d_stats, stream=None):
    """Enqueue the mixing kernels (afg_mix_hip) on device arrays: both energies and the gain of every group into d_stats
    (MIX_STATS_DTYPE records) and every valid element plus the gain times the noise under it into d_out (d_in itself for in
    place).  d_partials: n_tiles * 16 bytes.  The groups are checked first (the call waits for `stream` to read them):
    AfgError, and nothing written, when one fails."""
    check(lib().afg_mix_hip(int(n_groups), _ptr(d_groups), int(n_tiles), _ptr(d_in), int(in_floats), _ptr(d_noise), int(noise_floats),
                            _ptr(d_out), int(out_floats), _ptr(d_partials), _ptr(d_stats), _stream(stream)))


def _per_group(who, name, value, n, dtype, default=None):
    """a scalar or one value per group as an array of n"""
    if value is None:
        value = default
    v = np.asarray(value.cpu() if hasattr(value, "cpu") else value)
    if v.ndim == 0:
        v = np.full(n, v)
    v = v.reshape(-1)
    if v.size != n:
        raise ValueError(f"{who}: {name} is a scalar or holds one value per group ({n})")
    return v.astype(dtype)


def _mix_noise_args(who, noise, channels, n, snr_db, gain, noise_lengths, noise_index, noise_start):
    """What add_noise_tensor and batch_decode_tensor_noisy share: the bank's shape and the per-group clip, start and level,
    checked.  Returns (K, clip rows, N, lengths[K], index[n], start[n] reduced, snr[n] or None, gain[n] or None)."""
    import torch
    if not isinstance(noise, torch.Tensor) or not noise.is_cuda or noise.dtype != torch.float32 or not noise.is_contiguous() or noise.dim() not in (2, 3):
        raise ValueError(f"{who}: noise is a contiguous float32 device tensor [K, N] or [K, channels, N]")
    K, N = int(noise.shape[0]), int(noise.shape[-1])
    clip_rows = 1 if noise.dim() == 2 else int(noise.shape[1])
    if K < 1 or N < 1 or N >= 1 << 32:
        raise ValueError(f"{who}: noise holds at least one clip of 1 .. 2^32 - 1 samples")
    if noise.dim() == 3 and clip_rows != channels:
        raise ValueError(f"{who}: noise [K, channels, N] has {clip_rows} channels, the signal {channels}")
    if (snr_db is None) == (gain is None):
        raise ValueError(f"{who}: exactly one of snr_db and gain")
    lengths = _per_group(who, "noise_lengths", noise_lengths, K, np.int64, N) if noise_lengths is None or np.ndim(noise_lengths) == 0 else None
    if lengths is None:
        lengths = np.asarray(noise_lengths.cpu() if hasattr(noise_lengths, "cpu") else noise_lengths).reshape(-1).astype(np.int64)
        if lengths.size != K:
            raise ValueError(f"{who}: noise_lengths holds one length per clip ({K})")
    if (lengths < 1).any() or (lengths > N).any():
        raise ValueError(f"{who}: noise_lengths: 1 .. {N}")
    index = _per_group(who, "noise_index", noise_index, n, np.int64, 0)
    if (index < 0).any() or (index >= K).any():
        raise ValueError(f"{who}: noise_index: 0 .. {K - 1}")
    start = _per_group(who, "noise_start", noise_start, n, np.int64, 0)
    if (start < 0).any():
        raise ValueError(f"{who}: noise_start: at least 0")
    start = start % lengths[index] if n else start
    snr = g = None
    if snr_db is not None:
        snr = _per_group(who, "snr_db", snr_db, n, np.float64)
        if not np.isfinite(snr).all() or not np.isfinite([mix_ratio(v) for v in snr]).all():
            raise ValueError(f"{who}: snr_db: finite, with a finite ratio 10^(-snr_db / 10)")
    else:
        g = _per_group(who, "gain", gain, n, np.float32)
        if not np.isfinite(g).all() or (g < 0).any():
            raise ValueError(f"{who}: gain: finite and at least 0")
    return K, clip_rows, N, lengths, index, start, snr, g


def add_noise_tensor(t, noise, snr_db=None, gain=None, noise_lengths=None, noise_index=None, noise_start=None, valid=None, out=None):
    """Add noise from a bank of clips to every group of a contiguous float32 device tensor [..., channels, frames] -- the
    channel axis is one group; the leading axes are flattened -- at a signal-to-noise ratio measured over the group's own
    valid samples (afg_mix_hip, on the current stream; include/afg.h has the definition; with the gain it reports, the result
    is torchaudio.functional.add_noise's expression bit for bit).  noise: a contiguous float32 device tensor [K, N] (a clip
    is shared by a group's channels) or [K, channels, N].  noise_lengths: None (N) or one length per clip; a clip shorter
    than the row loops.  noise_index, noise_start, and snr_db or gain (exactly one of the two; gain: y = x + gain * n as it
    is): a scalar or one value per group; noise_start is reduced modulo the clip's length.  valid: None, or one length per
    group: only that many frames of its rows count and are touched.  out: None (a new tensor, a copy of t behind `valid`),
    `t` itself (in place) or another contiguous tensor of t's shape that overlaps neither t nor the bank.  Returns
    (out, stats): stats a MIX_STATS_DTYPE array with one record per group.  ValueError, before any launch, for arguments out
    of range."""
    import torch
    who = "add_noise_tensor"
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 2:
        raise ValueError(f"{who}: a contiguous float32 device tensor [..., channels, frames]")
    rows, frames = int(t.shape[-2]), int(t.shape[-1])
    if rows < 1 or rows > 65535 or frames >= 1 << 32:
        raise ValueError(f"{who}: 1 .. 65535 channels of fewer than 2^32 frames")
    n = t.numel() // (rows * frames) if frames else 0
    K, clip_rows, N, lengths, index, start, snr, g = _mix_noise_args(who, noise, rows, n, snr_db, gain, noise_lengths, noise_index, noise_start)
    if noise.device != t.device:
        raise ValueError(f"{who}: noise must live on t's device")
    if out is None:
        out = t.clone() if valid is not None else torch.empty_like(t)
    elif out.shape != t.shape or out.dtype != t.dtype or out.device != t.device or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous tensor of t's shape, dtype and device")
    groups = np.zeros(n, MIX_GROUP_DTYPE)
    groups["in_off"] = groups["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(rows * frames)
    groups["stride"], groups["rows"], groups["valid"] = frames, rows, frames
    if valid is not None:
        v = np.asarray(valid.cpu() if hasattr(valid, "cpu") else valid).reshape(-1)
        if v.size != n or (v < 0).any() or (v > frames).any():
            raise ValueError(f"{who}: valid holds one length per group, 0 .. the last axis")
        groups["valid"] = v
    if n == 0:
        return out, np.zeros(0, MIX_STATS_DTYPE)
    groups["noise_off"] = index.astype(np.uint64) * np.uint64(clip_rows * N)
    groups["noise_stride"] = 0 if noise.dim() == 2 else N
    groups["noise_len"], groups["noise_start"] = lengths[index], start
    if snr is not None:
        groups["flags"], groups["ratio"] = MIX_SNR, [mix_ratio(v) for v in snr]
    else:
        groups["flags"], groups["gain"] = MIX_GAIN, g
    tiles = mix_layout(groups)
    L = lib()
    at = (C.c_uint64 * 3)(t.data_ptr() // 4, noise.data_ptr() // 4, out.data_ptr() // 4)
    if L.afg_mix_check_groups(groups.ctypes.data, n, tiles, t.numel(), noise.numel(), out.numel(), at) != 0:
        raise ValueError(f"{who}: {L.afg_last_error().decode()}")
    with torch.cuda.device(t.device):
        d_groups = torch.from_numpy(groups.view(np.uint8)).to(t.device)
        d_partials = torch.empty(max(tiles, 1) * 2, dtype=torch.float64, device=t.device)
        d_stats = torch.zeros(n * MIX_STATS_DTYPE.itemsize, dtype=torch.uint8, device=t.device)
        mix(n, d_groups, tiles, t, t.numel(), noise, noise.numel(), out, out.numel(), d_partials, d_stats, torch.cuda.current_stream().cuda_stream)
        stats = d_stats.cpu().numpy().view(MIX_STATS_DTYPE).copy()
    return out, stats


def batch_decode_tensor_noisy(files, frames, channels, samplerate, noise, snr_db, noise_lengths=None, noise_index=None, noise_start=None,
                              first_frame=None, mono=False, in_channels=0, max_in_rate=0, lowpass_width=0, out=None, n_threads=0):
    """afg_batch_decode_mixed: batch_decode_tensor_resampled, then noise from the bank added to every file in place at snr_db
    over the file's own samples -- its channel rows one group, the rows and lengths of batch_decode_tensor_normalized; the
    padding is left as it is.  noise, noise_lengths, noise_index, noise_start and snr_db as add_noise_tensor takes them, one
    value per file where they are no scalars; the bank is at `samplerate` already.  Returns (tensor, meta, stats): stats a
    MIX_STATS_DTYPE array with one record per file (all zero, gain 0, for a file that failed).  The same device and stream
    rules as batch_decode_tensor; ValueError for arguments out of range, before any call."""
    who = "batch_decode_tensor_noisy"
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError(f"{who}: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError(f"{who}: a mono tensor has one channel")
    n = len(files)
    K, clip_rows, N, lengths, index, start, snr, _ = _mix_noise_args(who, noise, channels, n, snr_db, None, noise_lengths, noise_index, noise_start)
    stats = np.zeros(max(n, 1), MIX_STATS_DTYPE)
    c_len, c_idx = (C.c_uint32 * K)(*[int(v) for v in lengths]), (C.c_uint32 * max(n, 1))(*[int(v) for v in index])
    c_start, c_snr = (C.c_uint64 * max(n, 1))(*[int(v) for v in start]), (C.c_double * max(n, 1))(*[float(v) for v in snr])
    bank = MixNoise(noise.data_ptr(), K, N, clip_rows, c_len, c_idx, c_start, c_snr)

    def call(ptrs, lens, n, ff, out, res):
        opts = ResampleOpts(C.sizeof(ResampleOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                            int(max_in_rate), int(lowpass_width))
        return lib().afg_batch_decode_mixed(ptrs, lens, n, C.byref(opts), C.byref(bank), out.data_ptr(), stats.ctypes.data, C.byref(res))

    out, meta = _batch_tensor_call(who, files, (n, channels, frames), out, first_frame, call)
    return out, meta, stats[:n].copy()


def batch_transcode(files, options=None, n_threads=0, devices=None):
    """afg_batch_transcode to WAV: options = encoding_options(...) (None: fp32).  devices as for batch_decode.  Returns a
    list of dicts (status, message, bytes: the complete WAV file, None for a file that did not decode)."""
    bufs = [bytes(f) for f in files]
    n = len(bufs)
    ptrs = (C.c_char_p * max(n, 1))(*bufs)
    lens = (C.c_size_t * max(n, 1))(*[len(b) for b in bufs])
    opts = BatchOpts(C.sizeof(BatchOpts), int(n_threads), 0, None, SAMPLE_F32, DITHER_OFF, 0)
    if devices == "all":
        opts.n_devices = -1
    elif devices is not None:
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        opts.n_devices, opts.devices = len(devices), devs
    res = EncodeResult()
    check(lib().afg_batch_transcode(ptrs, lens, n, FORMAT_WAV, None if options is None else C.byref(options), C.byref(opts),
                                    C.byref(res)))
    try:
        out = []
        for i in range(res.n_files):
            it = res.items[i]
            out.append({"status": it.status, "message": None if it.message is None else it.message.decode(),
                        "bytes": C.string_at(it.bytes, it.size) if it.status == 0 else None})
        return out
    finally:
        lib().afg_encode_free(C.byref(res))


def copy_probe(d_dst, d_src, nbytes, stream=None):
    """Enqueue the streaming copy used to measure the practical HBM copy ceiling (afg_copy_probe_hip)."""
    check(lib().afg_copy_probe_hip(_ptr(d_dst), _ptr(d_src), int(nbytes), _stream(stream)))


def stft_params(n_fft=400, hop=160, win_length=None, center=True, pad_mode=MEL_PAD_REFLECT, out_kind=STFT_POWER, log_floor=0.0):
    """afg_stft_params with Whisper's framing as the default (win_length None: n_fft)."""
    return StftParams(int(n_fft), int(n_fft if win_length is None else win_length), int(hop), 1 if center else 0, int(pad_mode),
                      int(out_kind), float(log_floor), 0)


def stft_tile_frames(params):
    """afg_stft_tile_frames: the frames of one row a workgroup of afg_stft_hip takes for these parameters (it depends on n_fft
    and out_kind).  AfgError for parameters out of range."""
    tile = int(lib().afg_stft_tile_frames(C.byref(params)))
    if tile == 0:
        raise AfgError(lib().afg_last_error().decode())
    return tile


def stft_layout(rows, params):
    """afg_stft_layout: fills first_tile of a MEL_ROW_DTYPE array in place for afg_stft_hip (tiles of stft_tile_frames);
    returns the launch's tile count."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_stft_layout(rows.ctypes.data, len(rows), C.byref(params)))


def stft_check_rows(rows, n_tiles, params, in_floats, table_floats, out_floats):
    """afg_stft_check_rows: what afg_stft_hip checks before it launches, on host records.  AfgError when one fails."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    check(lib().afg_stft_check_rows(rows.ctypes.data, len(rows), int(n_tiles), C.byref(params), int(in_floats), int(table_floats),
                                    int(out_floats)))


def stft(n_rows, d_rows, n_tiles, params, d_in, in_floats, d_table, table_floats, d_out, out_floats, stream=None):
    """Enqueue the linear spectrogram kernel (afg_stft_hip) on device arrays: planar float rows to [rows, n_bins, out_frames]
    (pairs of re, im with STFT_COMPLEX), with mel_fft_tables' table and rows laid out by stft_layout.  The records are checked
    first (the call waits for `stream` to read them): AfgError, and nothing written, when a check fails."""
    check(lib().afg_stft_hip(int(n_rows), _ptr(d_rows), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_table),
                             int(table_floats), _ptr(d_out), int(out_floats), _stream(stream)))


def batch_decode_stft(files, frames, samplerate=16000, n_fft=400, hop=160, win_length=None, center=True, pad_mode=MEL_PAD_REFLECT,
                      out_kind=STFT_POWER, log_floor=0.0, n_out=0, mono=True, out=None, channels=1, first_frame=None, in_channels=0,
                      max_in_rate=0, lowpass_width=0, n_threads=0):
    """afg_batch_decode_stft: (tensor, meta) as batch_decode_mel, with the tensor [len(files), channels, n_fft // 2 + 1, n_out]
    the linear-frequency spectrogram of every row of batch_decode_tensor_resampled's tensor of `frames` samples at
    `samplerate` (include/afg.h has the definition): float32 for STFT_MAGNITUDE, STFT_POWER and STFT_LOG10, complex64 for
    STFT_COMPLEX -- torch.stft's layout (`out`, when given, is the float32 tensor with a last dimension of 2 that
    torch.view_as_real makes of it).  n_out 0: every frame `frames` samples have.  n_fft: prime factors 2, 3 and 5 only.
    The same device and stream rules as batch_decode_tensor."""
    import torch
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_stft: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_stft: a mono tensor has one channel")
    prm = stft_params(n_fft, hop, win_length, center, pad_mode, out_kind, log_floor)
    stft_tile_frames(prm)                                    # (the parameters: AfgError says which)
    most = mel_frames(MelParams(prm.n_fft, prm.win_length, prm.hop, 1, prm.center, prm.pad_mode, MEL_POWER, 0.0), frames)
    if most == 0:
        raise ValueError(f"batch_decode_stft: {frames} samples hold no frame of n_fft {prm.n_fft}")
    n_out = int(n_out)
    if n_out < 0 or n_out > most:
        raise ValueError(f"batch_decode_stft: n_out {n_out}, but {frames} samples have {most} frames")
    shape = (len(files), channels, prm.n_fft // 2 + 1, n_out if n_out else most)
    if prm.out_kind == STFT_COMPLEX:
        shape += (2,)

    def call(ptrs, lens, n, ff, out, res):
        opts = StftOpts(C.sizeof(StftOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                        int(max_in_rate), int(lowpass_width), n_out, prm, 0)
        return lib().afg_batch_decode_stft(ptrs, lens, n, C.byref(opts), out.data_ptr(), C.byref(res))

    out, meta = _batch_tensor_call("batch_decode_stft", files, shape, out, first_frame, call)
    return (torch.view_as_complex(out) if prm.out_kind == STFT_COMPLEX else out), meta


def istft_params(n_fft=400, hop=160, win_length=None, center=True):
    """afg_istft_params with Whisper's framing as the default (win_length None: n_fft)."""
    return IstftParams(int(n_fft), int(n_fft if win_length is None else win_length), int(hop), 1 if center else 0)


def istft_tile_samples(params):
    """afg_istft_tile_samples: the consecutive delivered samples of one row a workgroup of afg_istft_hip owns for these
    parameters (it depends on n_fft and hop).  AfgError for parameters out of range."""
    tile = int(lib().afg_istft_tile_samples(C.byref(params)))
    if tile == 0:
        raise AfgError(lib().afg_last_error().decode())
    return tile


def istft_layout(rows, params):
    """afg_istft_layout: fills first_tile of an ISTFT_ROW_DTYPE array in place (tiles of istft_tile_samples); returns the
    launch's tile count."""
    assert rows.dtype == ISTFT_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_istft_layout(rows.ctypes.data, len(rows), C.byref(params)))


def istft_envelope_min(params, n_frames, out_first, out_frames):
    """afg_istft_envelope_min: the smallest window envelope D[t] over the delivered range of a record, summed in double from
    the table's float32 window.  Host only.  AfgError for parameters or a range out of bounds."""
    d = float(lib().afg_istft_envelope_min(C.byref(params), int(n_frames), int(out_first), int(out_frames)))
    if d < 0.0:
        raise AfgError(lib().afg_last_error().decode())
    return d


def istft_check_rows(rows, n_tiles, params, in_floats, table_floats, out_floats):
    """afg_istft_check_rows: what afg_istft_hip checks before it launches, on host records.  AfgError when one fails."""
    assert rows.dtype == ISTFT_ROW_DTYPE and rows.flags.c_contiguous
    check(lib().afg_istft_check_rows(rows.ctypes.data, len(rows), int(n_tiles), C.byref(params), int(in_floats), int(table_floats),
                                     int(out_floats)))


def istft(n_rows, d_rows, n_tiles, params, d_in, in_floats, d_table, table_floats, d_out, out_floats, stream=None):
    """Enqueue the inverse STFT kernel (afg_istft_hip) on device arrays: slabs of (re, im) pairs in STFT_COMPLEX's layout to
    rows of samples, with mel_fft_tables' table and rows laid out by istft_layout.  The records are checked first (the call
    waits for `stream` to read them): AfgError, and nothing written, when a check fails."""
    check(lib().afg_istft_hip(int(n_rows), _ptr(d_rows), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_table),
                              int(table_floats), _ptr(d_out), int(out_floats), _stream(stream)))


_istft_tables = {}                                           # (device index, n_fft, win_length): the device table, made once and kept


def istft_tensor(spec, n_fft=400, hop=160, win_length=None, center=True, length=None, first=0, valid_frames=None, out=None, _counts=None):
    """The inverse STFT of every slab of a contiguous device tensor (afg_istft_hip, one launch on the current stream;
    include/afg.h has the definition): spec is complex64 [..., n_bins, F] -- torch.stft's and batch_decode_stft(out_kind=
    STFT_COMPLEX)'s layout -- or float32 [..., n_bins, F, 2]; the result is float32 [..., length], samples first .. first +
    length of every line behind the centring pad.  length None: hop * (F - 1) when centred (torch.istft's default), the rest
    of the line otherwise.  valid_frames: None, or one frame count per slab (the leading axes flattened): only that many
    frames are read, and only the samples they make are written -- what lies behind them is left as it is (zero in a new
    tensor).  out: None, or a contiguous float32 tensor [..., length].  Returns out.  AfgError when a record is refused,
    for instance center=False with first=0, where the window envelope is zero."""
    import torch
    prm = istft_params(n_fft, hop, win_length, center)
    istft_tile_samples(prm)                                  # (the parameters: AfgError says which)
    if not spec.is_cuda or not spec.is_contiguous():
        raise ValueError("istft_tensor: a contiguous device tensor")
    if spec.dtype == torch.complex64 and spec.dim() >= 2:
        flat, lead = torch.view_as_real(spec), tuple(spec.shape[:-2])
    elif spec.dtype == torch.float32 and spec.dim() >= 3 and spec.shape[-1] == 2:
        flat, lead = spec, tuple(spec.shape[:-3])
    else:
        raise ValueError("istft_tensor: complex64 [..., n_bins, F] or float32 [..., n_bins, F, 2]")
    n_bins, F = int(flat.shape[-3]), int(flat.shape[-2])
    if n_bins != prm.n_fft // 2 + 1 or F < 1:
        raise ValueError(f"istft_tensor: n_fft {prm.n_fft} has {prm.n_fft // 2 + 1} bins, and at least one frame is needed")
    pad, first = (prm.n_fft // 2 if center else 0), int(first)
    line = lambda frames: prm.n_fft + prm.hop * (frames - 1)
    if length is None:
        length = prm.hop * (F - 1) if center else line(F) - first
    length = int(length)
    if first < 0 or length < 0 or pad + first + length > line(F):
        raise ValueError(f"istft_tensor: samples {first} .. {first + length}, but {F} frames make {line(F) - pad} behind the pad")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if out is None:
        out = (torch.zeros if valid_frames is not None else torch.empty)(lead + (length,), dtype=torch.float32, device=spec.device)
    elif tuple(out.shape) != lead + (length,) or out.dtype != torch.float32 or out.device != spec.device or not out.is_contiguous():
        raise ValueError(f"istft_tensor: out must be a contiguous float32 tensor of shape {lead + (length,)} on spec's device")
    rows = np.zeros(n, ISTFT_ROW_DTYPE)
    rows["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(2 * n_bins * F)
    rows["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(length)
    rows["n_frames"], rows["in_pitch"], rows["out_first"], rows["out_frames"] = F, F, first, length
    if valid_frames is not None:
        v = np.asarray(valid_frames.cpu() if hasattr(valid_frames, "cpu") else valid_frames).reshape(-1).astype(np.int64)
        if v.size != n or (v < 0).any() or (v > F).any():
            raise ValueError("istft_tensor: valid_frames holds one frame count per slab, 0 .. F")
        rows["n_frames"] = v
        reach = np.where(v > 0, (prm.hop * (v - 1) if center else prm.n_fft + prm.hop * (v - 1)) - first, 0)   # as `length`'s default
        rows["out_frames"] = np.clip(reach, 0, length)
        if _counts is not None:                              # (time_stretch_tensor: fewer samples than the frames make)
            rows["out_frames"] = np.minimum(rows["out_frames"], _counts)
    if n == 0 or length == 0:
        return out
    tiles = istft_layout(rows, prm)
    with torch.cuda.device(spec.device):
        key = (torch.cuda.current_device(), prm.n_fft, prm.win_length)
        if key not in _istft_tables:
            _istft_tables[key] = torch.from_numpy(mel_fft_tables(prm.n_fft, prm.win_length)).to(spec.device)
        table = _istft_tables[key]
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(spec.device)
        istft(n, d_rows, tiles, prm, flat, flat.numel(), table, table.numel(), out, out.numel(), torch.cuda.current_stream().cuda_stream)
    return out


def stft_tensor(wave, n_fft=400, hop=160, win_length=None, center=True, pad_mode=MEL_PAD_REFLECT, out_kind=STFT_COMPLEX, valid=None):
    """The linear spectrogram of every row of a contiguous float32 device tensor [..., n] (afg_stft_hip, one launch on the
    current stream; include/afg.h has the definition): the tensor-in counterpart of istft_tensor.  The result is
    [..., n_bins, F] with F the frames n samples have: complex64 for STFT_COMPLEX (torch.stft's layout), float32 otherwise.
    valid: None, or one sample count per row (the leading axes flattened), 0 .. n: row i is then framed as a row of valid[i]
    samples (reflection at its own end), its F_i frames are packed at the front of its slab with a pitch of F_i frames, the
    rest of the slab stays zero, and the call returns (tensor, frame counts).  The table is istft_tensor's, made once per
    device and (n_fft, win_length) and kept.  AfgError when a record is refused."""
    import torch
    prm = stft_params(n_fft, hop, win_length, center, pad_mode, out_kind)
    stft_tile_frames(prm)                                    # (the parameters: AfgError says which)
    if not wave.is_cuda or not wave.is_contiguous() or wave.dtype != torch.float32 or wave.dim() < 1:
        raise ValueError("stft_tensor: a contiguous float32 device tensor [..., n]")
    lead, length = tuple(wave.shape[:-1]), int(wave.shape[-1])
    mel = MelParams(prm.n_fft, prm.win_length, prm.hop, 1, prm.center, prm.pad_mode, MEL_POWER, 0.0)
    F = mel_frames(mel, length)
    if F == 0:
        raise ValueError(f"stft_tensor: {length} samples hold no frame of n_fft {prm.n_fft}")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    n_bins, comps = prm.n_fft // 2 + 1, 2 if prm.out_kind == STFT_COMPLEX else 1
    shape = lead + (n_bins, F) + ((2,) if comps == 2 else ())
    out = (torch.zeros if valid is not None else torch.empty)(shape, dtype=torch.float32, device=wave.device)
    rows = np.zeros(n, MEL_ROW_DTYPE)
    rows["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(length)
    rows["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(comps * n_bins * F)
    rows["in_frames"], rows["out_frames"] = length, F
    if valid is not None:
        v = np.asarray(valid.cpu() if hasattr(valid, "cpu") else valid).reshape(-1).astype(np.int64)
        if v.size != n or (v < 0).any() or (v > length).any():
            raise ValueError("stft_tensor: valid holds one sample count per row, 0 .. n")
        rows["in_frames"] = v
        rows["out_frames"] = [mel_frames(mel, int(c)) if c > 0 else 0 for c in v]
    if n:
        tiles = stft_layout(rows, prm)
        with torch.cuda.device(wave.device):
            key = (torch.cuda.current_device(), prm.n_fft, prm.win_length)
            if key not in _istft_tables:
                _istft_tables[key] = torch.from_numpy(mel_fft_tables(prm.n_fft, prm.win_length)).to(wave.device)
            table = _istft_tables[key]
            d_rows = torch.from_numpy(rows.view(np.uint8)).to(wave.device)
            stft(n, d_rows, tiles, prm, wave, wave.numel(), table, table.numel(), out, out.numel(), torch.cuda.current_stream().cuda_stream)
    res = torch.view_as_complex(out) if comps == 2 else out
    return res if valid is None else (res, rows["out_frames"].astype(np.int64))


def _fbank_window(who, window_type):
    if isinstance(window_type, str):
        if window_type not in FBANK_WINDOW_NAMES:
            raise ValueError(f"{who}: window_type {window_type!r}: one of {sorted(FBANK_WINDOW_NAMES)}")
        return FBANK_WINDOW_NAMES[window_type]
    return int(window_type)


def fbank_n_fft(win_length, round_to_power_of_two=True):
    """afg_fbank_n_fft: Kaldi's transform length for a window -- the next power of two, or the window itself."""
    n = int(lib().afg_fbank_n_fft(int(win_length), 1 if round_to_power_of_two else 0))
    if n == 0:
        raise AfgError(f"afg: {lib().afg_last_error().decode()}")
    return n


def fbank_params(win_length=400, hop=160, n_fft=None, n_mels=23, snip_edges=True, remove_dc=True, preemph=0.97, use_power=True,
                 use_log=True, use_energy=False, raw_energy=True, htk_compat=False, energy_floor=1.0, scale=0.0, layout=FBANK_FRAMES_MAJOR):
    """afg_fbank_params with torchaudio.compliance.kaldi.fbank's defaults at 16 kHz (n_fft None: the next power of two)."""
    n_fft = fbank_n_fft(win_length) if n_fft is None else int(n_fft)
    return FbankParams(int(win_length), int(hop), n_fft, int(n_mels), 1 if snip_edges else 0, 1 if remove_dc else 0, 1 if use_power else 0,
                       1 if use_log else 0, 1 if use_energy else 0, 1 if raw_energy else 0, 1 if htk_compat else 0, int(layout),
                       float(preemph), float(energy_floor), float(scale), 0)


def fbank_frames(params, in_frames):
    """afg_fbank_frames: the frames a row of in_frames samples has (0 also for parameters out of range)."""
    return int(lib().afg_fbank_frames(C.byref(params), int(in_frames)))


def fbank_tables(window_type, win_length, n_fft, blackman_coeff=0.42):
    """afg_fbank_tables: win_length window values (FBANK_WINDOW_* or its name), then n_fft pairs (cos, -sin) of 2 pi j / n_fft,
    as one float32 array.  Host only.  AfgError for arguments out of range or an n_fft the transform does not take."""
    L_ = lib()
    args = (_fbank_window("fbank_tables", window_type), int(win_length), int(n_fft), float(blackman_coeff))
    need = int(L_.afg_fbank_tables(*args, None, 0))
    if need == 0:
        raise AfgError(f"afg: {L_.afg_last_error().decode()}")
    out = np.zeros(need, np.float32)
    L_.afg_fbank_tables(*args, out.ctypes.data, need)
    return out


def fbank_filters(samplerate, n_fft, n_mels, low_freq=20.0, high_freq=0.0):
    """afg_fbank_filters: the float32 bank [n_mels, n_fft // 2 + 1], triangles on the mel axis (high_freq <= 0: an offset from
    Nyquist).  Host only.  AfgError for arguments out of range."""
    L_ = lib()
    args = (int(samplerate), int(n_fft), int(n_mels), float(low_freq), float(high_freq))
    need = int(L_.afg_fbank_filters(*args, None, 0))
    if need == 0:
        raise AfgError(f"afg: {L_.afg_last_error().decode()}")
    out = np.zeros(need, np.float32)
    L_.afg_fbank_filters(*args, out.ctypes.data, need)
    return out.reshape(int(n_mels), need // int(n_mels))


def fbank_layout(rows, params):
    """afg_fbank_layout: fills first_tile of a MEL_ROW_DTYPE array in place (tiles of 16 frames); returns the launch's tile
    count, 0 for parameters out of range."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_fbank_layout(rows.ctypes.data, len(rows), C.byref(params)))


def fbank_check_rows(rows, n_tiles, params, in_floats, table_floats, filters_floats, out_floats):
    """afg_fbank_check_rows: what afg_fbank_hip checks before it launches, on host records.  AfgError when one fails."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    check(lib().afg_fbank_check_rows(rows.ctypes.data, len(rows), int(n_tiles), C.byref(params), int(in_floats), int(table_floats),
                                     int(filters_floats), int(out_floats)))


def fbank(n_rows, d_rows, n_tiles, params, d_in, in_floats, d_table, table_floats, d_filters, filters_floats, d_out, out_floats, stream=None):
    """Enqueue the filter-bank kernel (afg_fbank_hip) on device arrays: planar float rows to [rows, out_frames, cols] (or
    [rows, cols, out_frames] with FBANK_MEL_MAJOR), with fbank_tables' table, a dense bank and rows laid out by fbank_layout.
    The records are checked first (the call waits for `stream` to read them): AfgError, and nothing written, when one fails."""
    check(lib().afg_fbank_hip(int(n_rows), _ptr(d_rows), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_table),
                              int(table_floats), _ptr(d_filters), int(filters_floats), _ptr(d_out), int(out_floats), _stream(stream)))


_fbank_tables = {}                                            # (device, window, win_length, n_fft, blackman, rate, n_mels, low, high) -> tensors


def _fbank_kaldi_params(who, samplerate, num_mel_bins, frame_length, frame_shift, round_to_power_of_two, snip_edges, remove_dc_offset,
                        preemphasis_coefficient, use_power, use_log_fbank, use_energy, raw_energy, htk_compat, energy_floor, scale, layout):
    ws, hop = int(samplerate * frame_length * 0.001), int(samplerate * frame_shift * 0.001)
    if ws < 2 or hop < 1:
        raise ValueError(f"{who}: frame_length {frame_length} ms and frame_shift {frame_shift} ms at {samplerate} Hz")
    return fbank_params(ws, hop, fbank_n_fft(ws, round_to_power_of_two), num_mel_bins, snip_edges, remove_dc_offset, preemphasis_coefficient,
                        use_power, use_log_fbank, use_energy, raw_energy, htk_compat, energy_floor, scale, layout)


def fbank_tensor(wave, samplerate=16000, num_mel_bins=23, frame_length=25.0, frame_shift=10.0, window_type="povey", blackman_coeff=0.42,
                 low_freq=20.0, high_freq=0.0, round_to_power_of_two=True, snip_edges=True, remove_dc_offset=True,
                 preemphasis_coefficient=0.97, use_power=True, use_log_fbank=True, use_energy=False, raw_energy=True, htk_compat=False,
                 energy_floor=1.0, scale=0.0, layout=FBANK_FRAMES_MAJOR, valid=None):
    """Kaldi-compatible filter-bank features of every row of a contiguous float32 device tensor [..., n] (afg_fbank_hip, one
    launch on the current stream; include/afg.h has the definition), with torchaudio.compliance.kaldi.fbank's argument names
    and defaults (no dither, no VTLN, no subtract_mean).  scale 32768 turns a [-1, 1] waveform into what Kaldi reads.  The
    result is [..., F, cols], or [..., cols, F] with FBANK_MEL_MAJOR, F the frames n samples have.  valid: None, or one sample
    count per row (the leading axes flattened), 0 .. n: row i is then framed as a row of valid[i] samples (mirrored at its own
    end), its F_i frames stand at the front of its slab (frames-major; with FBANK_MEL_MAJOR at a pitch of F_i frames), the
    rest stays zero, and the call returns (tensor, frame counts).  The tables are made once per device and parameter set and
    kept.  AfgError when a parameter or a record is refused."""
    import torch
    samplerate = int(samplerate)
    prm = _fbank_kaldi_params("fbank_tensor", samplerate, num_mel_bins, frame_length, frame_shift, round_to_power_of_two, snip_edges,
                              remove_dc_offset, preemphasis_coefficient, use_power, use_log_fbank, use_energy, raw_energy, htk_compat,
                              energy_floor, scale, layout)
    wt = _fbank_window("fbank_tensor", window_type)
    fbank_check_rows(np.zeros(0, MEL_ROW_DTYPE), 0, prm, 0, 0, 0, 0)      # (the parameters: AfgError says which)
    if not wave.is_cuda or not wave.is_contiguous() or wave.dtype != torch.float32 or wave.dim() < 1:
        raise ValueError("fbank_tensor: a contiguous float32 device tensor [..., n]")
    lead, length = tuple(wave.shape[:-1]), int(wave.shape[-1])
    F = fbank_frames(prm, length)
    if F == 0:
        raise ValueError(f"fbank_tensor: {length} samples hold no frame of {prm.win_length} samples")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    cols = prm.n_mels + prm.use_energy
    shape = lead + ((F, cols) if prm.layout == FBANK_FRAMES_MAJOR else (cols, F))
    out = (torch.zeros if valid is not None else torch.empty)(shape, dtype=torch.float32, device=wave.device)
    rows = np.zeros(n, MEL_ROW_DTYPE)
    rows["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(length)
    rows["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(cols * F)
    rows["in_frames"], rows["out_frames"] = length, F
    if valid is not None:
        v = np.asarray(valid.cpu() if hasattr(valid, "cpu") else valid).reshape(-1).astype(np.int64)
        if v.size != n or (v < 0).any() or (v > length).any():
            raise ValueError("fbank_tensor: valid holds one sample count per row, 0 .. n")
        rows["in_frames"] = v
        rows["out_frames"] = [fbank_frames(prm, int(c)) for c in v]
    if n:
        tiles = fbank_layout(rows, prm)
        with torch.cuda.device(wave.device):
            key = (torch.cuda.current_device(), wt, prm.win_length, prm.n_fft, float(blackman_coeff), samplerate, prm.n_mels, float(low_freq),
                   float(high_freq))
            if key not in _fbank_tables:
                _fbank_tables[key] = (torch.from_numpy(fbank_tables(wt, prm.win_length, prm.n_fft, blackman_coeff)).to(wave.device),
                                      torch.from_numpy(fbank_filters(samplerate, prm.n_fft, prm.n_mels, low_freq, high_freq).reshape(-1).copy())
                                      .to(wave.device))
            table, bank = _fbank_tables[key]
            d_rows = torch.from_numpy(rows.view(np.uint8)).to(wave.device)
            fbank(n, d_rows, tiles, prm, wave, wave.numel(), table, table.numel(), bank, bank.numel(), out, out.numel(),
                  torch.cuda.current_stream().cuda_stream)
    return out if valid is None else (out, rows["out_frames"].astype(np.int64))


def batch_decode_fbank(files, frames, samplerate=16000, num_mel_bins=23, frame_length=25.0, frame_shift=10.0, window_type="povey",
                       blackman_coeff=0.42, low_freq=20.0, high_freq=0.0, round_to_power_of_two=True, snip_edges=True, remove_dc_offset=True,
                       preemphasis_coefficient=0.97, use_power=True, use_log_fbank=True, use_energy=False, raw_energy=True, htk_compat=False,
                       energy_floor=1.0, scale=0.0, layout=FBANK_FRAMES_MAJOR, n_out=0, mono=True, out=None, channels=1, first_frame=None,
                       in_channels=0, max_in_rate=0, lowpass_width=0, n_threads=0):
    """afg_batch_decode_fbank: (tensor, meta, lengths).  The tensor [len(files), channels, n_out, cols] (or [..., cols, n_out]
    with FBANK_MEL_MAJOR) holds the Kaldi-compatible filter-bank features of every row of batch_decode_tensor_resampled's
    tensor of `frames` samples at `samplerate` (include/afg.h has the definition; the arguments are fbank_tensor's).  n_out 0:
    every frame `frames` samples have.  lengths: per file, the feature frames its own resampled samples give, capped at n_out
    (0 for a file that failed) -- what a collation masks by.  The same device and stream rules as batch_decode_tensor."""
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_fbank: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_fbank: a mono tensor has one channel")
    prm = _fbank_kaldi_params("batch_decode_fbank", samplerate, num_mel_bins, frame_length, frame_shift, round_to_power_of_two, snip_edges,
                              remove_dc_offset, preemphasis_coefficient, use_power, use_log_fbank, use_energy, raw_energy, htk_compat,
                              energy_floor, scale, layout)
    wt = _fbank_window("batch_decode_fbank", window_type)
    fbank_check_rows(np.zeros(0, MEL_ROW_DTYPE), 0, prm, 0, 0, 0, 0)      # (the parameters: AfgError says which)
    most = fbank_frames(prm, frames)
    if most == 0:
        raise ValueError(f"batch_decode_fbank: {frames} samples hold no frame of {prm.win_length} samples")
    n_out = int(n_out)
    if n_out < 0 or n_out > most:
        raise ValueError(f"batch_decode_fbank: n_out {n_out}, but {frames} samples have {most} frames")
    F, cols = (n_out if n_out else most), prm.n_mels + prm.use_energy
    shape = (len(files), channels) + ((F, cols) if prm.layout == FBANK_FRAMES_MAJOR else (cols, F))
    lengths = np.zeros(max(len(files), 1), np.uint32)

    def call(ptrs, lens, n, ff, out, res):
        opts = FbankOpts(C.sizeof(FbankOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                         int(max_in_rate), int(lowpass_width), n_out, prm, wt, float(low_freq), float(high_freq), float(blackman_coeff), 0)
        return lib().afg_batch_decode_fbank(ptrs, lens, n, C.byref(opts), out.data_ptr(), lengths.ctypes.data, C.byref(res))

    out, meta = _batch_tensor_call("batch_decode_fbank", files, shape, out, first_frame, call)
    return out, meta, lengths[:len(files)].astype(np.int64)


def _cmn_layout_code(who, layout):
    if isinstance(layout, str):
        if layout not in CMN_LAYOUT_NAMES:
            raise ValueError(f"{who}: layout {layout!r}: one of {sorted(CMN_LAYOUT_NAMES)}")
        return CMN_LAYOUT_NAMES[layout]
    return int(layout)


def cmn_params(cols, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False, layout=CMN_FRAMES_MAJOR):
    """afg_cmn_params with Kaldi's (and torchaudio.functional.sliding_window_cmn's) defaults; layout CMN_* or "frames" / "cols"."""
    return CmnParams(int(cmn_window), int(min_cmn_window), 1 if center else 0, 1 if norm_vars else 0, int(cols),
                     _cmn_layout_code("cmn_params", layout), (C.c_uint32 * 2)(0, 0))


def cmn_layout(slabs):
    """afg_cmn_layout: fills first_tile of a CMN_SLAB_DTYPE array in place (tiles of 32 frames); returns the launch's tile count."""
    assert slabs.dtype == CMN_SLAB_DTYPE and slabs.flags.c_contiguous
    return int(lib().afg_cmn_layout(slabs.ctypes.data, len(slabs)))


def cmn_work_bytes(n_tiles, cols):
    """afg_cmn_work_bytes: the workspace afg_slide_cmn_hip needs for n_tiles tiles of `cols` columns."""
    return int(lib().afg_cmn_work_bytes(int(n_tiles), int(cols)))


def cmn_check_slabs(slabs, n_tiles, params, in_floats, out_floats, same_plane):
    """afg_cmn_check_slabs: what afg_slide_cmn_hip checks before it launches, on host records.  AfgError when one fails."""
    assert slabs.dtype == CMN_SLAB_DTYPE and slabs.flags.c_contiguous
    check(lib().afg_cmn_check_slabs(slabs.ctypes.data, len(slabs), int(n_tiles), C.byref(params), int(in_floats), int(out_floats),
                                    1 if same_plane else 0))


def slide_cmn(n_slabs, d_slabs, n_tiles, params, d_in, in_floats, d_out, out_floats, d_work, work_bytes, stream=None):
    """Enqueue the sliding-window normalisation (afg_slide_cmn_hip) on device arrays: slab k of d_slabs (CMN_SLAB_DTYPE records
    laid out by cmn_layout) from d_in to d_out -- the same tensor for in place -- with a workspace of cmn_work_bytes bytes.
    The records are checked first (the call waits for `stream` to read them): AfgError, and nothing written, when one fails."""
    check(lib().afg_slide_cmn_hip(int(n_slabs), _ptr(d_slabs), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_out),
                                  int(out_floats), _ptr(d_work), int(work_bytes), _stream(stream)))


def sliding_cmn_tensor(t, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False, layout="frames", valid_frames=None, out=None):
    """Sliding-window mean (and variance) normalisation of every slab of a contiguous float32 device tensor [..., frames, cols],
    or [..., cols, frames] with layout "cols" (afg_slide_cmn_hip, two launches on the current stream; include/afg.h has the
    definition, Kaldi's window; the arguments are torchaudio.functional.sliding_window_cmn's).  valid_frames: None, or one
    frame count per slab (the leading axes flattened), 0 .. frames: only that many frames of the slab are read and written,
    and the windows end there.  out: None (a new tensor, zero behind valid_frames), `t` itself (in place) or another
    contiguous tensor of t's shape that does not overlap it; what lies behind valid_frames in it is left as it is.  Returns
    out.  AfgError when a parameter is refused."""
    import torch
    code = _cmn_layout_code("sliding_cmn_tensor", layout)
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 2:
        raise ValueError("sliding_cmn_tensor: a contiguous float32 device tensor with at least two axes")
    frames, cols = (int(t.shape[-1]), int(t.shape[-2])) if code == CMN_COL_MAJOR else (int(t.shape[-2]), int(t.shape[-1]))
    prm = cmn_params(max(cols, 1), cmn_window, min_cmn_window, center, norm_vars, code)
    cmn_check_slabs(np.zeros(0, CMN_SLAB_DTYPE), 0, prm, 0, 0, False)      # (the parameters: AfgError says which)
    if out is None:
        out = torch.zeros_like(t) if valid_frames is not None else torch.empty_like(t)
    elif out.shape != t.shape or out.dtype != t.dtype or out.device != t.device or not out.is_contiguous():
        raise ValueError("sliding_cmn_tensor: out must be a contiguous tensor of t's shape, dtype and device")
    if frames >= 1 << 31:
        raise ValueError("sliding_cmn_tensor: slabs of 2^31 frames or more")
    n = t.numel() // (frames * cols) if frames * cols else 0
    slabs = np.zeros(n, CMN_SLAB_DTYPE)
    slabs["in_off"] = slabs["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(frames * cols)
    slabs["pitch"] = frames if code == CMN_COL_MAJOR else cols
    slabs["n_frames"] = frames
    if valid_frames is not None:
        v = np.asarray(valid_frames.cpu() if hasattr(valid_frames, "cpu") else valid_frames).reshape(-1)
        if v.size != n or (v < 0).any() or (v > frames).any():
            raise ValueError("sliding_cmn_tensor: valid_frames holds one frame count per slab, 0 .. frames")
        slabs["n_frames"] = v
    tiles = cmn_layout(slabs) if n else 0
    if tiles == 0:
        return out
    with torch.cuda.device(t.device):
        nbytes = cmn_work_bytes(tiles, cols)
        work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=t.device)
        d_slabs = torch.from_numpy(slabs.view(np.uint8)).to(t.device)
        slide_cmn(n, d_slabs, tiles, prm, t, t.numel(), out, out.numel(), work, nbytes, torch.cuda.current_stream().cuda_stream)
    return out


def batch_decode_fbank_cmn(files, frames, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False, samplerate=16000,
                           num_mel_bins=23, frame_length=25.0, frame_shift=10.0, window_type="povey", blackman_coeff=0.42, low_freq=20.0,
                           high_freq=0.0, round_to_power_of_two=True, snip_edges=True, remove_dc_offset=True, preemphasis_coefficient=0.97,
                           use_power=True, use_log_fbank=True, use_energy=False, raw_energy=True, htk_compat=False, energy_floor=1.0,
                           scale=0.0, layout=FBANK_FRAMES_MAJOR, n_out=0, mono=True, out=None, channels=1, first_frame=None, in_channels=0,
                           max_in_rate=0, lowpass_width=0, n_threads=0):
    """afg_batch_decode_fbank_cmn: batch_decode_fbank, then sliding_cmn_tensor's normalisation in place over every slab's own
    frames (the returned lengths), in one call: (tensor, meta, lengths).  The frames behind a file's length, and the slabs of
    failed files, are batch_decode_fbank's.  The four window arguments are sliding_cmn_tensor's, the rest batch_decode_fbank's."""
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_fbank_cmn: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_fbank_cmn: a mono tensor has one channel")
    prm = _fbank_kaldi_params("batch_decode_fbank_cmn", samplerate, num_mel_bins, frame_length, frame_shift, round_to_power_of_two, snip_edges,
                              remove_dc_offset, preemphasis_coefficient, use_power, use_log_fbank, use_energy, raw_energy, htk_compat,
                              energy_floor, scale, layout)
    wt = _fbank_window("batch_decode_fbank_cmn", window_type)
    fbank_check_rows(np.zeros(0, MEL_ROW_DTYPE), 0, prm, 0, 0, 0, 0)      # (the parameters: AfgError says which)
    cols = prm.n_mels + prm.use_energy
    cmn = cmn_params(cols, cmn_window, min_cmn_window, center, norm_vars, CMN_COL_MAJOR if prm.layout == FBANK_MEL_MAJOR else CMN_FRAMES_MAJOR)
    cmn_check_slabs(np.zeros(0, CMN_SLAB_DTYPE), 0, cmn, 0, 0, False)
    most = fbank_frames(prm, frames)
    if most == 0:
        raise ValueError(f"batch_decode_fbank_cmn: {frames} samples hold no frame of {prm.win_length} samples")
    n_out = int(n_out)
    if n_out < 0 or n_out > most:
        raise ValueError(f"batch_decode_fbank_cmn: n_out {n_out}, but {frames} samples have {most} frames")
    F = n_out if n_out else most
    shape = (len(files), channels) + ((F, cols) if prm.layout == FBANK_FRAMES_MAJOR else (cols, F))
    lengths = np.zeros(max(len(files), 1), np.uint32)

    def call(ptrs, lens, n, ff, out, res):
        opts = FbankOpts(C.sizeof(FbankOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                         int(max_in_rate), int(lowpass_width), n_out, prm, wt, float(low_freq), float(high_freq), float(blackman_coeff), 0)
        return lib().afg_batch_decode_fbank_cmn(ptrs, lens, n, C.byref(opts), C.byref(cmn), out.data_ptr(), lengths.ctypes.data, C.byref(res))

    out, meta = _batch_tensor_call("batch_decode_fbank_cmn", files, shape, out, first_frame, call)
    return out, meta, lengths[:len(files)].astype(np.int64)


def yin_lags(samplerate, fmin, fmax, frame_length, win_length):
    """afg_yin_lags: librosa's lag range (tau_min, tau_max) = (floor(sr / fmax), min(ceil(sr / fmin), frame_length -
    win_length - 1)).  AfgError for an empty range or arguments out of range."""
    lo, hi = C.c_uint32(0), C.c_uint32(0)
    check(lib().afg_yin_lags(float(samplerate), float(fmin), float(fmax), int(frame_length), int(win_length), C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


def yin_params(samplerate, frame_length=2048, win_length=None, hop=None, tau_min=None, tau_max=None, threshold=0.1, center=True,
               pad_mode=MEL_PAD_ZERO, fmin=None, fmax=None):
    """afg_yin_params with librosa.yin's defaults (win_length None: frame_length // 2; hop None: frame_length // 4).  The lag
    range is given as it is (tau_min, tau_max) or drawn from fmin and fmax by yin_lags."""
    frame_length = int(frame_length)
    win_length = frame_length // 2 if win_length is None else int(win_length)
    hop = frame_length // 4 if hop is None else int(hop)
    if tau_min is None or tau_max is None:
        if fmin is None or fmax is None:
            raise ValueError("yin_params: tau_min and tau_max, or fmin and fmax")
        tau_min, tau_max = yin_lags(samplerate, fmin, fmax, frame_length, win_length)
    return YinParams(frame_length, win_length, hop, int(tau_min), int(tau_max), 1 if center else 0, int(pad_mode), float(threshold),
                     float(samplerate), (C.c_uint32 * 2)(0, 0))


def yin_frames(params, in_frames):
    """afg_yin_frames: the frames a row of in_frames samples has (0 also for parameters out of range)."""
    return int(lib().afg_yin_frames(C.byref(params), int(in_frames)))


def yin_layout(rows, params):
    """afg_yin_layout: fills first_tile of a MEL_ROW_DTYPE array in place (tiles of YIN_TILE frames); returns the launch's tile
    count, 0 for parameters out of range."""
    assert rows.dtype == MEL_ROW_DTYPE and rows.flags.c_contiguous
    return int(lib().afg_yin_layout(rows.ctypes.data, len(rows), C.byref(params)))


def yin(n_rows, d_rows, n_tiles, params, d_in, in_floats, d_out, out_floats, stream=None):
    """Enqueue the YIN kernel (afg_yin_hip) on device arrays: planar float rows to slabs [2, out_frames] -- f0 in Hz, then
    d' at the chosen lag (voiced iff below the threshold) -- with rows laid out by yin_layout.  The records are checked first
    (the call waits for `stream` to read them): AfgError, and nothing written, when one fails."""
    check(lib().afg_yin_hip(int(n_rows), _ptr(d_rows), int(n_tiles), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_out), int(out_floats),
                            _stream(stream)))


def _yin_check(params):
    check(lib().afg_yin_hip(0, None, 0, C.byref(params), None, 0, None, 0, None))      # (the parameters: AfgError says which)


def yin_tensor(x, samplerate, fmin, fmax, frame_length=2048, win_length=None, hop=None, threshold=0.1, center=True, pad_mode=MEL_PAD_ZERO,
               valid=None):
    """The YIN pitch of every row of a contiguous float32 device tensor [..., n] (afg_yin_hip, one launch on the current
    stream; include/afg.h has the definition), with librosa.yin's argument names and defaults, except that pad_mode defaults to
    zeros (librosa's np.pad default is "constant").  The result is [..., 2, F], F the frames n samples have: plane 0 the f0 in
    Hz, plane 1 d' at the chosen lag; a frame is voiced iff plane 1 < threshold.  valid: None, or one sample count per row (the
    leading axes flattened), 0 .. n: row i is then framed as a row of valid[i] samples (padded at its own end), its F_i frames
    stand at the front of both planes, the rest is zero, and the call returns (tensor, frame counts).  AfgError when a
    parameter or a record is refused."""
    import torch
    prm = yin_params(samplerate, frame_length, win_length, hop, threshold=threshold, center=center, pad_mode=pad_mode, fmin=fmin, fmax=fmax)
    _yin_check(prm)
    if not x.is_cuda or not x.is_contiguous() or x.dtype != torch.float32 or x.dim() < 1:
        raise ValueError("yin_tensor: a contiguous float32 device tensor [..., n]")
    lead, length = tuple(x.shape[:-1]), int(x.shape[-1])
    F = yin_frames(prm, length)
    if F == 0:
        raise ValueError(f"yin_tensor: {length} samples hold no frame of {prm.frame_length} samples")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    out = torch.empty((n, 2, F), dtype=torch.float32, device=x.device)
    rows = np.zeros(n, MEL_ROW_DTYPE)
    rows["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(length)
    rows["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(2 * F)
    rows["in_frames"], rows["out_frames"] = length, F
    if valid is not None:
        v = np.asarray(valid.cpu() if hasattr(valid, "cpu") else valid).reshape(-1).astype(np.int64)
        if v.size != n or (v < 0).any() or (v > length).any():
            raise ValueError("yin_tensor: valid holds one sample count per row, 0 .. n")
        pad = prm.frame_length // 2 if prm.center else 0
        rows["in_frames"] = v
        rows["out_frames"] = [0 if c == 0 or (prm.pad_mode == MEL_PAD_REFLECT and c <= pad) else yin_frames(prm, int(c)) for c in v]
        out.zero_()                                          # the kernel writes slabs [2, F_i]; they are spread to [2, F] below
    if n:
        tiles = yin_layout(rows, prm)
        with torch.cuda.device(x.device):
            d_rows = torch.from_numpy(rows.view(np.uint8)).to(x.device)
            yin(n, d_rows, tiles, prm, x, x.numel(), out, out.numel(), torch.cuda.current_stream().cuda_stream)
        if valid is not None:
            Fi = torch.from_numpy(rows["out_frames"].astype(np.int64)).to(x.device)
            f = torch.arange(F, device=x.device)
            at = (torch.arange(2, device=x.device)[None, :, None] * Fi[:, None, None] + f[None, None, :]).clamp_(max=2 * F - 1)
            own = (f[None, None, :] < Fi[:, None, None]).expand(n, 2, F)
            out = torch.where(own, out.reshape(n, 2 * F).gather(1, at.reshape(n, 2 * F)).reshape(n, 2, F), torch.zeros((), device=x.device))
    out = out.reshape(lead + (2, F))
    return out if valid is None else (out, rows["out_frames"].astype(np.int64))


def batch_decode_pitch(files, frames, samplerate, fmin, fmax, frame_length=2048, win_length=None, hop=None, threshold=0.1, center=True,
                       pad_mode=MEL_PAD_ZERO, n_out=0, mono=True, out=None, channels=1, first_frame=None, in_channels=0, max_in_rate=0,
                       lowpass_width=0, n_threads=0):
    """afg_batch_decode_pitch: (tensor, meta, lengths).  The tensor [len(files), channels, 2, n_out] holds the YIN pitch (plane
    0: f0 in Hz, plane 1: d' at the chosen lag) of every row of batch_decode_tensor_resampled's tensor of `frames` samples at
    `samplerate` (include/afg.h has the definition; the arguments are yin_tensor's).  n_out 0: every frame `frames` samples
    have.  lengths: per file, the frames its own resampled samples give, capped at n_out (0 for a file that failed); the frames
    past them are zero in both planes.  The same device and stream rules as batch_decode_tensor."""
    frames, channels, samplerate = int(frames), int(channels), int(samplerate)
    if frames < 1 or channels < 1 or samplerate < 1:
        raise ValueError("batch_decode_pitch: frames, channels and samplerate must be at least 1")
    if mono and channels != 1:
        raise ValueError("batch_decode_pitch: a mono tensor has one channel")
    prm = yin_params(samplerate, frame_length, win_length, hop, threshold=threshold, center=center, pad_mode=pad_mode, fmin=fmin, fmax=fmax)
    _yin_check(prm)
    most = yin_frames(prm, frames)
    if most == 0:
        raise ValueError(f"batch_decode_pitch: {frames} samples hold no frame of {prm.frame_length} samples")
    n_out = int(n_out)
    if n_out < 0 or n_out > most:
        raise ValueError(f"batch_decode_pitch: n_out {n_out}, but {frames} samples have {most} frames")
    F = n_out if n_out else most
    lengths = np.zeros(max(len(files), 1), np.uint32)

    def call(ptrs, lens, n, ff, out, res):
        opts = PitchOpts(C.sizeof(PitchOpts), int(n_threads), channels, frames, ff, samplerate, 1 if mono else 0, int(in_channels),
                         int(max_in_rate), int(lowpass_width), n_out, prm, 0)
        return lib().afg_batch_decode_pitch(ptrs, lens, n, C.byref(opts), out.data_ptr(), lengths.ctypes.data, C.byref(res))

    out, meta = _batch_tensor_call("batch_decode_pitch", files, (len(files), channels, 2, F), out, first_frame, call)
    return out, meta, lengths[:len(files)].astype(np.int64)


def pvoc_params(n_fft=400, hop=160):
    """afg_pvoc_params with Whisper's framing as the default."""
    return PvocParams(int(n_fft), int(hop))


def pvoc_out_frames(n_frames, rate):
    """afg_pvoc_out_frames: the steps t >= 0 with fl(t * rate) < n_frames -- the frames a slab of n_frames frames stretches
    to at `rate`.  Host only.  AfgError for arguments out of range."""
    n = int(lib().afg_pvoc_out_frames(int(n_frames), float(rate)))
    if n == 0:
        raise AfgError(lib().afg_last_error().decode())
    return n


def pvoc_bound(params, t):
    """afg_pvoc_bound: K_A * 2^-24 + K_P * 2^-53 * pi * (t + 1), the bracket of the interval E_t = m_t * bracket."""
    b = float(lib().afg_pvoc_bound(C.byref(params), int(t)))
    if b < 0.0:
        raise AfgError(lib().afg_last_error().decode())
    return b


def pvoc_layout(rows, params):
    """Fills out_frames of a PVOC_ROW_DTYPE array in place from n_frames and rate (pvoc_out_frames; 0 for a record without
    frames) and returns their sum.  afg_pvoc_hip needs no tiles, so there is nothing else to lay out."""
    assert rows.dtype == PVOC_ROW_DTYPE and rows.flags.c_contiguous
    for r in rows:
        r["out_frames"] = pvoc_out_frames(r["n_frames"], r["rate"]) if r["n_frames"] else 0
    return int(rows["out_frames"].sum(dtype=np.uint64))


def pvoc_check_rows(rows, params, in_floats, out_floats):
    """afg_pvoc_check_rows: what afg_pvoc_hip checks before it launches, on host records.  AfgError when one fails."""
    assert rows.dtype == PVOC_ROW_DTYPE and rows.flags.c_contiguous
    check(lib().afg_pvoc_check_rows(rows.ctypes.data, len(rows), C.byref(params), int(in_floats), int(out_floats)))


def pvoc(n_rows, d_rows, params, d_in, in_floats, d_out, out_floats, stream=None):
    """Enqueue the phase-vocoder kernel (afg_pvoc_hip) on device arrays: slabs of (re, im) pairs in STFT_COMPLEX's layout to
    slabs of the same layout, stretched by each record's rate.  The records are checked first (the call waits for `stream`
    to read them): AfgError, and nothing written, when a check fails."""
    check(lib().afg_pvoc_hip(int(n_rows), _ptr(d_rows), C.byref(params), _ptr(d_in), int(in_floats), _ptr(d_out), int(out_floats),
                             _stream(stream)))


def _pvoc_slabs(who, flat, lead, n_bins, F, rate, frames, pitch, prm, out):
    """One afg_pvoc_hip launch over the slabs of `flat` (float32 [..., n_bins, F, 2]): slab i holds frames[i] frames at a pitch
    of pitch[i].  Returns (out as float32 [..., n_bins, F_out, 2], the frame counts)."""
    import torch
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    rates = np.broadcast_to(np.asarray(rate.cpu() if hasattr(rate, "cpu") else rate, dtype=np.float64).reshape(-1), (n,)) if n else np.zeros(0)
    rows = np.zeros(n, PVOC_ROW_DTYPE)
    rows["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(2 * n_bins * F)
    rows["rate"], rows["n_frames"], rows["in_pitch"] = rates, frames, pitch
    pvoc_layout(rows, prm)                                   # (AfgError for a rate out of range)
    counts = rows["out_frames"].astype(np.int64)
    most = int(counts.max()) if n else 0
    if out is None:
        out = torch.zeros(lead + (n_bins, most, 2), dtype=torch.float32, device=flat.device)
    else:
        if out.dtype == torch.complex64:
            out = torch.view_as_real(out)
        if out.dtype != torch.float32 or out.device != flat.device or not out.is_contiguous() or tuple(out.shape[:-2]) != lead + (n_bins,) \
                or out.shape[-1] != 2 or out.shape[-2] < most:
            raise ValueError(f"{who}: out must be a contiguous tensor [..., {n_bins}, at least {most}] of complex64 (or float32 pairs) on spec's device")
        if (counts != out.shape[-2]).any():
            out.zero_()                                      # zero behind each slab's own frames
    P = int(out.shape[-2])
    rows["out_off"], rows["out_pitch"] = np.arange(n, dtype=np.uint64) * np.uint64(2 * n_bins * P), P
    if n and most:
        with torch.cuda.device(flat.device):
            d_rows = torch.from_numpy(rows.view(np.uint8)).to(flat.device)
            pvoc(n, d_rows, prm, flat, flat.numel(), out, out.numel(), torch.cuda.current_stream().cuda_stream)
    return out, counts


def phase_vocoder_tensor(spec, rate, n_fft=400, hop=160, valid_frames=None, out=None):
    """The phase-vocoder time stretch of every slab of a contiguous device tensor (afg_pvoc_hip, one launch on the current
    stream; include/afg.h has the definition -- torchaudio's phase_vocoder with the phase summed in float64): spec is
    complex64 [..., n_bins, F] or float32 [..., n_bins, F, 2]; rate is a number or one per slab (the leading axes flattened),
    1/64 .. 64: above 1 is faster and shorter.  valid_frames: None, or one frame count per slab, 0 .. F.  Slab i comes out with
    pvoc_out_frames(its frames, its rate) frames; out (None: a new tensor) is [..., n_bins, the largest of them] or longer,
    of spec's kind, and is zero behind each slab's own frames.  Returns (out, the frame counts)."""
    import torch
    prm = pvoc_params(n_fft, hop)
    pvoc_check_rows(np.zeros(0, PVOC_ROW_DTYPE), prm, 0, 0)  # (the parameters: AfgError says which)
    if not spec.is_cuda or not spec.is_contiguous():
        raise ValueError("phase_vocoder_tensor: a contiguous device tensor")
    if spec.dtype == torch.complex64 and spec.dim() >= 2:
        flat, lead, cplx = torch.view_as_real(spec), tuple(spec.shape[:-2]), True
    elif spec.dtype == torch.float32 and spec.dim() >= 3 and spec.shape[-1] == 2:
        flat, lead, cplx = spec, tuple(spec.shape[:-3]), False
    else:
        raise ValueError("phase_vocoder_tensor: complex64 [..., n_bins, F] or float32 [..., n_bins, F, 2]")
    n_bins, F = int(flat.shape[-3]), int(flat.shape[-2])
    if n_bins != prm.n_fft // 2 + 1 or F < 1:
        raise ValueError(f"phase_vocoder_tensor: n_fft {prm.n_fft} has {prm.n_fft // 2 + 1} bins, and at least one frame is needed")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    frames = np.full(n, F, np.int64)
    if valid_frames is not None:
        frames = np.asarray(valid_frames.cpu() if hasattr(valid_frames, "cpu") else valid_frames).reshape(-1).astype(np.int64)
        if frames.size != n or (frames < 0).any() or (frames > F).any():
            raise ValueError("phase_vocoder_tensor: valid_frames holds one frame count per slab, 0 .. F")
    res, counts = _pvoc_slabs("phase_vocoder_tensor", flat, lead, n_bins, F, rate, frames, F, prm, out)
    return (torch.view_as_complex(res) if cplx else res), counts


def time_stretch_tensor(wave, rate, n_fft=400, hop=160, win_length=None, valid=None):
    """Stretch every row of a contiguous float32 device tensor [..., n] in time without changing its pitch: stft_tensor
    (complex, centred, reflect) -> the phase vocoder -> istft_tensor with valid_frames -- three launches on the current stream
    and no host round trip beyond the record uploads.  rate is a number or one per row, 1/64 .. 64 (above 1: faster, shorter);
    valid: None, or one sample count per row (each above n_fft / 2, for the reflection).  Row i delivers
    min(floor(n_i / rate_i + 0.5), hop * (F_out_i - 1)) samples, zeros behind them.  Returns (the tensor [..., the longest
    of them], the lengths)."""
    import torch
    lead, length = tuple(wave.shape[:-1]), int(wave.shape[-1])
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if valid is None:
        spec = stft_tensor(wave, n_fft, hop, win_length, True, MEL_PAD_REFLECT, STFT_COMPLEX)
        samples, frames = np.full(n, length, np.int64), np.full(n, spec.shape[-1], np.int64)
    else:
        spec, frames = stft_tensor(wave, n_fft, hop, win_length, True, MEL_PAD_REFLECT, STFT_COMPLEX, valid)
        samples = np.asarray(valid.cpu() if hasattr(valid, "cpu") else valid).reshape(-1).astype(np.int64)
    flat = torch.view_as_real(spec)
    n_bins, F = int(flat.shape[-3]), int(flat.shape[-2])
    stretched, counts = _pvoc_slabs("time_stretch_tensor", flat, lead, n_bins, F, rate, frames, np.maximum(frames, 1), pvoc_params(n_fft, hop), None)
    rates = np.broadcast_to(np.asarray(rate.cpu() if hasattr(rate, "cpu") else rate, dtype=np.float64).reshape(-1), (n,))
    lengths = np.minimum(np.floor(samples / rates + 0.5).astype(np.int64), int(hop) * np.maximum(counts - 1, 0))
    most = int(lengths.max()) if n else 0
    y = istft_tensor(torch.view_as_complex(stretched), n_fft, hop, win_length, True, length=most, valid_frames=counts, _counts=lengths)
    return y, lengths.reshape(lead)


def convolve_params(direct_max=CONV_DIRECT_MAX):
    """afg_convolve_params: kernels of at most direct_max taps (0 .. 128) take the direct path, every other the FFT path."""
    return ConvolveParams(int(direct_max))


def convolve_bank_layout(kernels):
    """afg_convolve_bank_layout: fills spec_off of a CONV_KERNEL_DTYPE array in place; returns the spectrum plane's floats
    (the table and one spectrum per partition of 1024 taps).  AfgError for taps out of range."""
    assert kernels.dtype == CONV_KERNEL_DTYPE and kernels.flags.c_contiguous
    need = int(lib().afg_convolve_bank_layout(kernels.ctypes.data, len(kernels)))
    if need == 0:
        raise AfgError(lib().afg_last_error().decode())
    return need


def convolve_bank_check(kernels, bank_floats, spec_floats):
    """afg_convolve_bank_check: what afg_convolve_bank_hip checks before it launches, on host records.  AfgError when one fails."""
    assert kernels.dtype == CONV_KERNEL_DTYPE and kernels.flags.c_contiguous
    check(lib().afg_convolve_bank_check(kernels.ctypes.data, len(kernels), int(bank_floats), int(spec_floats)))


def convolve_bank(n_kernels, d_kernels, d_bank, bank_floats, d_spec, spec_floats, stream=None):
    """Enqueue the bank transform (afg_convolve_bank_hip): the table and every partition's spectrum into d_spec, one launch.
    The records are checked first (the call waits for `stream` to read them): AfgError, and nothing written, when one fails."""
    check(lib().afg_convolve_bank_hip(int(n_kernels), _ptr(d_kernels), _ptr(d_bank), int(bank_floats), _ptr(d_spec), int(spec_floats),
                                      _stream(stream)))


def convolve_layout(rows, kernels, params):
    """afg_convolve_layout: fills first_tile and work_off of a CONV_ROW_DTYPE array in place; returns (tiles, work floats)."""
    assert rows.dtype == CONV_ROW_DTYPE and rows.flags.c_contiguous and kernels.dtype == CONV_KERNEL_DTYPE and kernels.flags.c_contiguous
    work = C.c_uint64(0)
    L = lib()
    tiles = int(L.afg_convolve_layout(rows.ctypes.data, len(rows), kernels.ctypes.data, len(kernels), C.byref(params), C.byref(work)))
    if tiles == 0 and (rows["out_frames"] > 0).any():        # (rows with output have tiles: the parameters or a kernel index were refused)
        raise AfgError(L.afg_last_error().decode())
    return tiles, int(work.value)


def convolve_bound(params, taps):
    """afg_convolve_bound: C of the FFT path's interval E[b] = C * 2^-24 * S[b] for a kernel of `taps`."""
    c = float(lib().afg_convolve_bound(C.byref(params), int(taps)))
    if c < 0.0:
        raise AfgError(lib().afg_last_error().decode())
    return c


def convolve_check_rows(rows, n_tiles, kernels, params, in_floats, bank_floats, spec_floats, work_floats, out_floats, plane_at=None):
    """afg_convolve_check_rows: what afg_convolve_hip checks before it launches, on host records.  plane_at: None, or the float
    index of the first float of the input, bank, spectrum, work and output plane in one address space.  AfgError when a check fails."""
    assert rows.dtype == CONV_ROW_DTYPE and rows.flags.c_contiguous and kernels.dtype == CONV_KERNEL_DTYPE and kernels.flags.c_contiguous
    at = None if plane_at is None else (C.c_uint64 * 5)(*[int(v) for v in plane_at])
    check(lib().afg_convolve_check_rows(rows.ctypes.data, len(rows), int(n_tiles), kernels.ctypes.data, len(kernels), C.byref(params),
                                        int(in_floats), int(bank_floats), int(spec_floats), int(work_floats), int(out_floats), at))


def convolve(n_rows, d_rows, n_tiles, d_kernels, n_kernels, params, d_in, in_floats, d_bank, bank_floats, d_spec, spec_floats, d_work,
             work_floats, d_out, out_floats, stream=None):
    """Enqueue the convolution (afg_convolve_hip) on device arrays: rows laid out by convolve_layout, a bank transformed by
    convolve_bank, a work plane of convolve_layout's size; at most three launches.  The records are checked first (the call
    waits for `stream` to read them): AfgError, and nothing written, when a check fails."""
    check(lib().afg_convolve_hip(int(n_rows), _ptr(d_rows), int(n_tiles), _ptr(d_kernels), int(n_kernels), C.byref(params), _ptr(d_in),
                                 int(in_floats), _ptr(d_bank), int(bank_floats), _ptr(d_spec), int(spec_floats), _ptr(d_work), int(work_floats),
                                 _ptr(d_out), int(out_floats), _stream(stream)))


class ConvolveBank:
    """A bank of convolution kernels on one device, built once: `kernels` is a list of 1-D float32 arrays or tensors (FIR
    taps, impulse responses; 1 .. 65536 values each).  Holds the device bank, the kernel records (host and device) and the
    partition spectra (afg_convolve_bank_hip, run here on the current stream)."""

    def __init__(self, kernels, device=None):
        import torch
        hs = [np.ascontiguousarray(k.detach().cpu().numpy() if hasattr(k, "detach") else k, dtype=np.float32) for k in kernels]
        if not hs or any(h.ndim != 1 for h in hs):
            raise ValueError("ConvolveBank: a list of at least one 1-D array")
        if any(h.size < 1 or h.size > CONV_MAX_TAPS for h in hs):
            raise ValueError(f"ConvolveBank: kernels of 1 .. {CONV_MAX_TAPS} taps")
        self.taps = np.array([h.size for h in hs], np.int64)
        self.records = np.zeros(len(hs), CONV_KERNEL_DTYPE)
        self.records["taps"] = self.taps
        self.records["bank_off"] = np.concatenate([[0], np.cumsum(self.taps)[:-1]])
        self.spec_floats = convolve_bank_layout(self.records)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(self.device):
            self.bank = torch.from_numpy(np.concatenate(hs)).to(self.device)
            self.d_records = torch.from_numpy(self.records.view(np.uint8)).to(self.device)
            self.spec = torch.empty(self.spec_floats, dtype=torch.float32, device=self.device)
            convolve_bank(len(hs), self.d_records, self.bank, self.bank.numel(), self.spec, self.spec_floats, torch.cuda.current_stream().cuda_stream)

    def __len__(self):
        return len(self.records)


def convolve_tensor(t, bank, kernel=0, mode="full", first=None, valid=None, out=None, direct_max=CONV_DIRECT_MAX):
    """Convolve every row of a contiguous float32 device tensor along its last axis with a kernel of a ConvolveBank
    (afg_convolve_hip on the current stream; include/afg.h has the definition).  kernel: one index, or one per row (the
    leading axes flattened).  valid: None, or one length per row, as in filter_tensor.  With n the row's length and T its
    kernel's taps, mode "full" delivers the n + T - 1 samples of the line, "same" n samples from (T - 1) // 2, and "head" n
    samples from `first` (default 0; one value or one per row, at most T - 1) -- a reverb that keeps the length, with
    first = the response's peak.  The work plane is allocated here and freed behind the launch on the current stream.
    Returns a tensor whose last axis is the longest delivered length, with +0.0 behind each row's own; out: None, or a
    contiguous float32 tensor of that shape on t's device that does not overlap t."""
    import torch
    prm = convolve_params(direct_max)
    if prm.direct_max > CONV_DIRECT_MAX:
        raise ValueError(f"convolve_tensor: direct_max 0 .. {CONV_DIRECT_MAX}")
    if not isinstance(bank, ConvolveBank):
        raise ValueError("convolve_tensor: bank is a ConvolveBank")
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1 or t.device != bank.device:
        raise ValueError("convolve_tensor: a contiguous float32 tensor with at least one axis on the bank's device")
    if mode not in ("full", "same", "head"):
        raise ValueError('convolve_tensor: mode is "full", "same" or "head"')
    if first is not None and mode != "head":
        raise ValueError('convolve_tensor: first goes with mode "head"')
    lead, frames = tuple(t.shape[:-1]), int(t.shape[-1])
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if frames >= (1 << 31) - CONV_MAX_TAPS:
        raise ValueError("convolve_tensor: rows of 2^31 - 65536 frames or more")

    def per_row(v, what, hi):
        a = np.asarray(v.cpu() if hasattr(v, "cpu") else v).reshape(-1).astype(np.int64)
        a = np.broadcast_to(a, (n,)) if a.size == 1 else a
        if a.size != n or (a < 0).any() or (a > hi).any():
            raise ValueError(f"convolve_tensor: {what}")
        return a

    named = np.asarray(kernel.cpu() if hasattr(kernel, "cpu") else kernel).reshape(-1)
    if named.size not in (1, n):
        raise ValueError(f"convolve_tensor: kernel is one index or one per row, 0 .. {len(bank) - 1}")
    k = per_row(kernel, f"kernel is one index or one per row, 0 .. {len(bank) - 1}", len(bank) - 1)
    taps = bank.taps[k]
    length = per_row(frames if valid is None else valid, "valid holds one length per row, 0 .. the last axis", frames)
    if mode == "full":
        start, count = np.zeros(n, np.int64), np.where(length > 0, length + taps - 1, 0)
    elif mode == "same":
        start, count = (taps - 1) // 2, length
    else:
        start = per_row(0 if first is None else first, "first is one value or one per row, 0 .. taps - 1", CONV_MAX_TAPS)
        if (start > taps - 1).any():
            raise ValueError("convolve_tensor: first is one value or one per row, 0 .. taps - 1")
        count = length
    # (a row's widest delivery: its whole axis, whatever `valid` says, so that the shape does not depend on the lengths)
    widest = int(frames + bank.taps[named.astype(np.int64)].max() - 1) if mode == "full" and frames and named.size else frames
    shape = lead + (widest,)
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=t.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != t.device or not out.is_contiguous():
        raise ValueError(f"convolve_tensor: out must be a contiguous float32 tensor of shape {shape} on t's device")
    elif n and (count < widest).any():
        out.zero_()
    if n == 0 or frames == 0:
        return out
    rows = np.zeros(n, CONV_ROW_DTYPE)
    rows["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(frames)
    rows["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(widest)
    rows["frames"], rows["kernel"], rows["out_first"], rows["out_frames"] = length, k, start, count
    tiles, work_floats = convolve_layout(rows, bank.records, prm)
    with torch.cuda.device(t.device):
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(t.device)
        work = torch.empty(max(work_floats, 2), dtype=torch.float32, device=t.device)      # (freed behind the launch: the caching allocator's stream order)
        convolve(n, d_rows, tiles, bank.d_records, len(bank), prm, t, t.numel(), bank.bank, bank.bank.numel(), bank.spec, bank.spec_floats,
                 work, work_floats, out, out.numel(), torch.cuda.current_stream().cuda_stream)
    return out


def lds_fill(word=0x7fc00000, stream=None):
    """Test aid (afg_lds_fill_probe_hip): leave `word` (default: NaN) in the LDS of every compute unit."""
    check(lib().afg_lds_fill_probe_hip(int(word), _stream(stream)))


NUMERIC_FROM_ENV, NUMERIC_EXACT, NUMERIC_TOLERANCE = -1, 0, 1


def set_numeric_mode(mode):
    """afg_set_numeric_mode: NUMERIC_EXACT (the reference's expression trees, bit for bit) or NUMERIC_TOLERANCE (default:
    within 1e-5 RMS; the Opus/CELT stage may re-associate); NUMERIC_FROM_ENV hands the choice back to AFG_NUMERIC.
    Returns the mode that was in effect before."""
    prev = lib().afg_set_numeric_mode(int(mode))
    if prev < 0:
        check(prev)
    return prev


def get_numeric_mode():
    return int(lib().afg_get_numeric_mode())


def device_count():
    return int(lib().afg_device_count())


def device_name(device=0):
    buf = C.create_string_buffer(256)
    check(lib().afg_device_name(device, buf, 256))
    return buf.value.decode()
