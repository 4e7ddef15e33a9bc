// afg_write_stream.h -- what the write stream (afg_write_stream.cpp), the batch encoder (afg_encode_stage.cpp) and the
// handle (afg_host.cpp) know of each other.
#pragma once
#include "../../include/afg.h"

#include <cstddef>
#include <functional>

namespace afg_write {
struct Writer;                          // the state of a stream opened for writing (afg_write_stream.cpp)
void destroy(Writer *w);
}  // namespace afg_write

namespace afg_front {
// afg_host.cpp.  A handle opened for writing: format, channels and rate as the getters report them, `error` its state
// (NULL: valid).  The handle owns the writer.  NULL: out of memory.
afg_stream *stream_for_writing(afg_write::Writer *w, int format, int channels, float samplerate, const char *error);
afg_write::Writer *stream_writer(const afg_stream *s);         // NULL: not opened for writing
void stream_set_error(afg_stream *s, const char *message);
// fn(0) .. fn(n - 1) on the library's pooled host threads; n_threads 0 = the library's choice (afg_batch_decode)
void parallel_run(size_t n, int n_threads, const std::function<void(size_t)> &fn);
}  // namespace afg_front
