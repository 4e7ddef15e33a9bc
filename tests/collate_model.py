"""numpy model of the collate kernel (include/afg.h: afg_collate_span) and of afg_batch_decode_to_device's slabs.

Words are moved as uint32, so NaN payloads, denormals and -0 are what they were."""
import numpy as np

PREFILL = 0x7fc0dead            # a NaN with a payload: what a test's d_out holds where nothing was stored


def span(in_off=0, count=0, sample0=0, out_off=0, first_frame=0, frames=1, channels=1, out_channels=1):
    """one afg_collate_span as a dict (first_tile is the layout's business)"""
    return dict(in_off=in_off, count=count, sample0=sample0, out_off=out_off, first_frame=first_frame, frames=frames,
                channels=channels, out_channels=out_channels)


def zero_run(at, count):
    """`count` zero floats from d_out[at] on (out_off + sample0 = at: split any way)"""
    return span(count=count, sample0=at % 7, out_off=at - at % 7, channels=0, frames=0, out_channels=0)


def apply_spans(spans, d_in, d_out):
    """What d_out (any 4-byte dtype, flat) holds after the spans have run over d_in: a new uint32 array."""
    src = np.ascontiguousarray(d_in).reshape(-1).view(np.uint32)
    out = np.ascontiguousarray(d_out).reshape(-1).view(np.uint32).copy()
    for sp in spans:
        n = int(sp["count"])
        if n == 0:
            continue
        if sp["channels"] == 0:
            at = int(sp["out_off"]) + int(sp["sample0"])
            out[at:at + n] = 0
            continue
        ch, T = int(sp["channels"]), int(sp["frames"])
        s = int(sp["sample0"]) + np.arange(n, dtype=np.int64)
        f, k = s // ch, s % ch
        t = f - int(sp["first_frame"])
        keep = (k < int(sp["out_channels"])) & (t >= 0) & (t < T)
        out[int(sp["out_off"]) + k[keep] * T + t[keep]] = src[int(sp["in_off"]) + np.arange(n, dtype=np.int64)[keep]]
    return out


def slab(pcm, channels, C, T, first_frame=0):
    """A file's delivered floats (interleaved, frames * channels of them; None: the file failed) as its [C, T] slab:
    frame first_frame lands at t = 0, zeros where the file has no channel or no frame."""
    out = np.zeros((C, T), np.float32)
    if pcm is None or channels <= 0:
        return out
    x = np.ascontiguousarray(pcm, np.float32).reshape(-1, channels)
    part = x[first_frame:first_frame + T, :min(C, channels)]
    out.view(np.uint32)[:part.shape[1], :part.shape[0]] = np.ascontiguousarray(part.T).view(np.uint32)
    return out


def tensor(items, C, T, first_frame=None):
    """batch_decode's items as the [files, C, T] tensor afg_batch_decode_to_device fills"""
    ff = [0] * len(items) if first_frame is None else first_frame
    out = np.zeros((len(items), C, T), np.float32)
    for i, it in enumerate(items):
        ok = it["status"] == 0 and it["pcm"] is not None
        out[i] = slab(it["pcm"] if ok else None, it["channels"] if ok else 0, C, T, int(ff[i]))
    return out
