// afg_wav_front.h -- WAV on the host: WAVDecoder.scan (wav.d:53-217) restated over a memory cursor, and the device side
// of WAV decoding (afg_wav_stage.cpp): a stream's reads and the batch path's WAV stage.  The sample conversion itself
// (readSamples!float, wav.d:242-344) is csrc/wav_pcm.hip; afg_wav.cpp is the writer.
#pragma once
#include "afg_stage.h"

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace afg_wav {

// What scan() leaves in the decoder (wav.d:347-353) plus what the file really holds
struct Info {
    int tag = 0;                    // _audioFormat: 1 PCM, 3 IEEE float (an extensible header has become 3)
    int channels = 0;               // 0 .. 65535
    int bits = 0;                   // 8, 16, 24, 32 or 64
    int sample_rate = 0;            // > 0
    uint32_t frames = 0;            // _lengthInFrames: what the 'data' chunk declares
    uint64_t samples_off = 0;       // _samplesOffsetInFile
    uint64_t present = 0;           // whole samples between samples_off and the end of the file, at most frames * channels
};

// The two refusals that are this library's own: the reference has no defined result there
extern const char *const kReasonSkip;       // a skip amount that is negative as a 32-bit int
extern const char *const kReasonChannels;   // a 'data' chunk behind a 'fmt ' chunk with 0 channels

// scan(): NULL when the file opens as a WAV, else the WAVError reason (the reference's string, or one of the two above).
// Terminates on every input.
const char *scan(const uint8_t *data, size_t size, Info *out);

// The afg_wav_kind readSamples!float uses for the format, or -1 where it refuses (PCM of 64 bits, float of 8 / 16 / 24)
int kind_of(const Info &info);
inline int bytes_per_sample(const Info &info) { return info.bits / 8; }

// A WAV stream: readSamples / seekPosition / tellPosition (wav.d:220-344) with the conversion on the device, a chunk of
// samples at a time through a FIFO.
class StreamConv {
public:
    Info info;
    // readSamples!float behind stream.d:557-570: the frames read; *failed set when the reference's read sets its error
    // (the position has advanced by the clamped request all the same, wav.d:253).  -1: device error.
    // f64: readSamples!double -- `out` takes doubles, made by csrc/pcm_f64.hip from the same bytes.  The FIFO holds one
    // type; a read of the other type drops it (the position is the stream's, not the FIFO's).
    int read(const uint8_t *file, size_t size, void *out, int frames, bool *failed, bool f64 = false);
    bool seek(int frame);                                   // wav.d:220-231
    int tell() const { return (int)position_; }
private:
    int decode(const uint8_t *file, uint64_t frame0, uint64_t frames);
    uint32_t position_ = 0;                                 // _framePosition
    std::vector<uint8_t> fifo_;                             // frames [fifo_frame_, fifo_frame_ + fifo_.size() / (es_ * channels))
    size_t es_ = sizeof(float);                             // bytes per sample of the FIFO: float, or double
    uint64_t fifo_frame_ = 0;
    afg_front::DevBuf in_, out_, spans_;                    // device memory from the library's pool
    afg_front::HandleStream stream_;
};

// The batch path's WAV stage: the files listed in `which` that pass scan() have their sample bytes staged as they are in
// the file, converted on the current device chunk by chunk (upload, one afg_wav_convert_hip launch, download overlapped)
// and their items filled in (float PCM in page-locked memory that `keep` owns).  A file whose samples are not all there,
// or whose format readSamples refuses, becomes an error item with the reference's decoding-error message.  Files that do
// not pass the scan are left alone.
int batch_stage(const uint8_t *const *data, const size_t *length, const std::vector<int> &which,
                int n_threads, afg_batch_item *items, std::shared_ptr<void> &keep, afg_front::SampleOut so = afg_front::SampleOut());   // f64: afg_pcm_to_f64_hip, items point at doubles

extern const char *const kMessageDecodingError;             // internals.d: kErrorDecodingError

}  // namespace afg_wav
