// afg_write_stream.h -- what the write stream (afg_write_stream.cpp), the batch encoder (afg_encode_stage.cpp), the host
// WAV writer (afg_wav.cpp) and the handle (afg_stream.cpp) know of each other.
#pragma once
#include "../../include/afg.h"

#include <cstddef>

namespace afg_write {
struct Writer;                          // the state of a stream opened for writing (afg_write_stream.cpp)
void destroy(Writer *w);

// what every WAV writer puts out: the header's length and a sample's bytes (0: not a sample format)
constexpr size_t kWavHeader = 44;
constexpr int sample_size(int format)
{
    return format == AFG_WAV_S8 ? 1 : format == AFG_WAV_S16LE ? 2 : format == AFG_WAV_S24LE ? 3 : format == AFG_WAV_FP32LE ? 4
           : format == AFG_WAV_FP64LE ? 8 : 0;
}
}  // namespace afg_write

namespace afg_front {
// afg_stream.cpp.  A handle opened for writing: format, channels and rate as the getters report them, `error` its state
// (NULL: valid).  The handle owns the writer.  NULL: out of memory.
afg_stream *stream_for_writing(afg_write::Writer *w, int format, int channels, float samplerate, const char *error);
afg_write::Writer *stream_writer(const afg_stream *s);         // NULL: not opened for writing
void stream_set_error(afg_stream *s, const char *message);
}  // namespace afg_front
