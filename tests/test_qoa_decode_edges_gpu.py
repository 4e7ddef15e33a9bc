"""QOA frame decode (csrc/qoa_lms.hip) where its two paths differ, through afgpu.qoa_transform.

The dispatch rule, which nothing outside the kernel can observe: one wavefront takes 32 records.  It walks them with
`stereo_walk` -- slices traded between lane pairs, four slices per row staged in LDS and flushed as 16-byte stores -- if
every record of the wavefront with samples != 0 has two channels and an out_off that is a multiple of 4; otherwise the
whole wavefront goes slice by slice through an LDS tile and indexed stores.  Within stereo_walk the products are 24-bit
mads if the wavefront's longest frame has at most 9000 samples and 32-bit multiplies beyond.

So every ragged stereo case runs in two output layouts: aligned (every out_off a multiple of 4: the fast path) and
shifted (the same rows, one of them moved by 2: its wavefront takes the general path), each held to the model and the
oracle, and each row compared between the two.  The cases are built in qoa_cases.py: a byte plane with filler between
the frames and an output plane with at least four values between rows, prefilled with -7 (int16) and a NaN (float).
Every comparison is exact and covers the whole plane: the model's int16 values and float bits inside the rows
(tests/qoa_model.py; tests/test_qoa_model.py holds it and the oracle to each other on these very cases), the prefill
everywhere else.
"""
import numpy as np
import pytest

import afgpu
import oraclelib
import qoa_cases as qc
from test_oracle_qoa import tone

pytestmark = pytest.mark.gpu

BOTH, I16_ONLY, F32_ONLY = (True, True), (True, False), (False, True)


def launch(gpu, case, outputs=BOTH):
    """One afgpu.qoa_transform over prefilled planes; the plane that is not asked for is passed as None.
    Returns (int16 plane or None, float32 plane as uint32 bits or None)."""
    import torch
    d_i = torch.from_numpy(np.full(case.out_total, qc.I16_SENTINEL, np.int16)).to(gpu) if outputs[0] else None
    d_f = torch.from_numpy(np.full(case.out_total, qc.F32_SENTINEL_BITS, np.uint32).view(np.float32)).to(gpu) if outputs[1] else None
    afgpu.qoa_transform(len(case.frames), torch.from_numpy(case.frames.view(np.uint8).copy()).to(gpu),
                        torch.from_numpy(case.data).to(gpu), d_i, d_f)
    torch.cuda.synchronize()
    return (None if d_i is None else d_i.cpu().numpy(), None if d_f is None else d_f.cpu().numpy().view(np.uint32))


def where(case, at):
    """words for output value `at`: the record that owns it, or that no record does"""
    for f, (off, cnt) in enumerate(case.rows()):
        if off <= at < off + cnt:
            ch = int(case.frames["channels"][f])
            return f"record {f} ({int(case.frames['samples'][f])} samples x {ch}), sample {(at - off) // ch} channel {(at - off) % ch}"
    before = [f for f, (off, cnt) in enumerate(case.rows()) if off + cnt <= at]
    return f"outside every row (after record {before[-1] if before else None})"


def check(case, got):
    """the whole plane: the model inside the rows, the prefill outside; then the oracle inside the rows"""
    written, mi, mf = case.model()
    oi, of = case.oracle()
    assert int(written.sum()) == sum(cnt for _, cnt in case.rows())
    for plane, model, oracle, fill, kind in ((got[0], mi, oi, qc.I16_SENTINEL, "int16"),
                                             (got[1], mf.view(np.uint32), of.view(np.uint32), qc.F32_SENTINEL_BITS, "float32 bits")):
        if plane is None:
            continue
        want = np.where(written, model, model.dtype.type(fill))
        assert plane.shape == want.shape
        bad = np.flatnonzero(plane != want)
        assert bad.size == 0, (f"{case.name}: {bad.size} {kind} values differ from the model, first at {bad[0]}: {where(case, int(bad[0]))}: "
                               f"got {plane[bad[0]]}, model {want[bad[0]]}, oracle {oracle[bad[0]]}")
        bad = np.flatnonzero((plane != oracle) & written)
        assert bad.size == 0, f"{case.name}: {bad.size} {kind} values differ from the oracle, first at {bad[0]}: {where(case, int(bad[0]))}"


def same_rows(a, got_a, b, got_b, records_a=None, records_b=None):
    """record by record, the two launches wrote the same values"""
    records_a = range(len(a.frames)) if records_a is None else records_a
    records_b = range(len(b.frames)) if records_b is None else records_b
    assert len(records_a) == len(records_b)
    for fa, fb in zip(records_a, records_b):
        (oa, ca), (ob, cb) = a.rows()[fa], b.rows()[fb]
        assert ca == cb
        for pa, pb in zip(got_a, got_b):
            if pa is not None and pb is not None:
                assert (pa[oa:oa + ca] == pb[ob:ob + cb]).all(), f"{a.name} record {fa} and {b.name} record {fb} differ"


def two_layouts(gpu, case, row, outputs=BOTH):
    """aligned and shifted (record `row` moved by 2), each against the model and the oracle, and against each other"""
    assert not (case.frames["out_off"][case.frames["channels"] == 2] & 3).any()
    moved = case.shifted(row)
    assert int(moved.frames["out_off"][row]) & 3 == 2 and int(moved.frames["samples"][row]) > 0
    got, got_moved = launch(gpu, case, outputs), launch(gpu, moved, outputs)
    check(case, got)
    check(moved, got_moved)
    same_rows(case, got, moved, got_moved)
    return got


# ------------------------------------------------------------------------------------ odd and short tails, outputs ---
@pytest.mark.parametrize("outputs", [BOTH, I16_ONLY, F32_ONLY], ids=["both", "int16", "float32"])
def test_odd_and_short_tails(gpu, outputs):
    """32 stereo frames of 1 .. 5120 samples in one wavefront: the single-pair store (k + 1 == lim) at the first flush
    (1 sample), at later ones (21, 41, 81, 99, 161 ...) and at the last (5119); rows that ended many flushes ago (a negative
    lim) beside rows still running; each output plane alone and both together."""
    case = qc.odd_tails()
    counts = case.frames["samples"]
    assert len(counts) == 32 and set(qc.ODD_TAILS) <= set(int(c) for c in counts) and (case.frames["channels"] == 2).all()
    two_layouts(gpu, case, qc.ODD_SHIFT, outputs)


@pytest.mark.parametrize("cap", qc.SMALL_CAPS)
def test_short_wavefronts(gpu, cap):
    """no frame longer than `cap` samples: max_slices 1, 2, 5, 8 and 9 -- a step with one flush, with a clipped one, and a
    second step of one slice"""
    case = qc.small_tails(cap)
    assert int(case.frames["samples"].max()) == cap and -(-cap // 20) in (1, 2, 5, 8, 9)
    two_layouts(gpu, case, qc.SMALL_SHIFT)


# ------------------------------------------------------------------------------------------ wavefront composition ---
@pytest.mark.parametrize("n_frames", qc.COMPOSITION_COUNTS)
def test_frame_counts(gpu, n_frames):
    """a last wavefront of 1, 31, 32 records; the shifted layout moves the last record"""
    case = qc.composition(n_frames)
    assert len(case.frames) == n_frames
    two_layouts(gpu, case, n_frames - 1)


def test_one_mono_frame_among_stereo(gpu):
    """frame 40 of 65 is mono: wavefront 1 takes the general path between two that take the fast one"""
    case = qc.one_mono()
    assert list(np.flatnonzero(case.frames["channels"] != 2)) == [40]
    two_layouts(gpu, case, qc.MONO_SHIFT)


def test_one_row_off_alignment(gpu):
    """64 stereo frames, only frame 5's out_off is 2 mod 4: its wavefront must leave the 16-byte stores alone"""
    case = qc.composition(64)
    moved = case.shifted(5)
    assert list(np.flatnonzero(moved.frames["out_off"] & 3)) == [5]
    two_layouts(gpu, case, 5)


def test_records_without_samples(gpu):
    """samples == 0 (include/afg.h: skipped) first in a wavefront, in its middle, and a whole wavefront of them"""
    case = qc.zero_records()
    assert list(np.flatnonzero(case.frames["samples"] == 0)) == list(qc.ZERO_RECORDS) and (case.frames["channels"] == 2).all()
    two_layouts(gpu, case, qc.ZERO_SHIFT)


# ------------------------------------------------------------------------------------------------ the general path ---
def test_general_path_shapes(gpu):
    """1 to 8 channels with tails of 1, 19, 21, 161 and a full frame each, shuffled over two wavefronts: odd channel counts
    (an idle slot in the last pair), narrow frames beside wide ones (max_pairs), any out_off"""
    case = qc.general()
    shapes = set(zip((int(s) for s in case.frames["samples"]), (int(c) for c in case.frames["channels"])))
    assert shapes == {(s, c) for s in qc.GENERAL_TAILS for c in range(1, 9)} and len(case.frames) == 40
    assert len(set(int(c) for c in case.frames["channels"][:32])) > 1 and (case.frames["out_off"] & 3).any()
    check(case, launch(gpu, case))


# ------------------------------------------------------------------------------------------------ the 24-bit switch ---
@pytest.mark.parametrize("word", qc.SWITCH_WORDS, ids=qc.word_id)
@pytest.mark.parametrize("kind", qc.SWITCH_KINDS)
def test_24_bit_switch(gpu, kind, word):
    """All-stereo wavefronts at the limit of the 24-bit mads (kI24MaxSamples = 9000) and past it, extreme LMS state.
    The four repeated words are test_qoa_gpu.py's; they do not take the weights far -- once the prediction wraps the
    history's signs turn random and the weights stay below 2^18 (the model's figure; test_qoa_model.py asserts it) -- so
    `driven` slices (qoa_cases.driven_words) follow the history's sign and move one weight by 896 at every sample:
    to 32767 + 9000 * 896 in a 9000-sample frame, just inside 24 bits, and past 2^23 from sample 9326 of a 9400-sample
    frame, which only the 32-bit multiplies get right.
    9020+short: one frame of 9020 samples moves its 31 neighbours of 19 .. 161 samples to the 32-bit multiplies; their
    bits must be those of a launch of the short frames alone."""
    case = qc.switch(kind, word)
    assert (case.frames["channels"] == 2).all() and not (case.frames["out_off"] & 3).any()
    if word == "driven" and kind != "9020+short":
        case.model()
        assert (case.peak > (1 << 23 if kind == "9400" else 32767 + 8900 * 896)).all()
        assert kind == "9400" or (case.peak < 1 << 23).all()
    got = launch(gpu, case)
    check(case, got)
    if kind == "9020+short":
        assert int(case.frames["samples"][qc.SWITCH_LONG_ROW]) == 9020 and int(np.delete(case.frames["samples"], qc.SWITCH_LONG_ROW).max()) <= 161
        alone = case.only(qc.short_rows())
        got_alone = launch(gpu, alone)
        check(alone, got_alone)
        same_rows(case, got, alone, got_alone, qc.short_rows(), range(31))


# ----------------------------------------------------------------------------------- bytes outside the frames ---
@pytest.mark.parametrize("make", [qc.odd_tails, qc.general], ids=["odd_tails", "general"])
def test_bytes_outside_the_frames_do_not_matter(gpu, make):
    """The fast path loads from the frame's first bytes for slice indices past the frame's end and never stores what it
    decodes from them; neither path may look at the filler between frames or at slices a frame carries past its last
    sample.  The same frames with all filler drawn again, then with all such slices drawn again: the same planes."""
    case = make()
    assert case.filler.sum() >= 8 * (len(case.frames) + 1) and case.tail.sum() > 0 and not (case.filler & case.tail).any()
    got = launch(gpu, case)
    check(case, got)
    for which, seed in (("filler", 1), ("tail", 2)):
        other = case.redrawn(which, seed)
        changed = other.data != case.data
        assert changed.any() and not (changed & ~getattr(case, which)).any()
        got_other = launch(gpu, other)
        assert (got_other[0] == got[0]).all() and (got_other[1] == got[1]).all(), f"the output depends on the {which} bytes"


# --------------------------------------------------------------------------------------------------- end to end ---
def test_files_of_odd_lengths_in_one_batch(gpu):
    """afgpu.batch_decode lays the files' rows out itself: a stereo file after one of odd length gets whatever out_off the
    host gives it, and must decode to the oracle's PCM all the same"""
    shapes = [(19, 2), (5121, 2), (41, 1), (81, 2), (5120, 2)]
    files = [oraclelib.qoa_encode(tone(n, ch, seed=n + ch))[0].tobytes() for n, ch in shapes]
    items = afgpu.batch_decode(files)
    assert len(items) == len(files)
    for item, blob, (n, ch) in zip(items, files, shapes):
        want = oraclelib.qoa_decode_file(blob)
        assert item["status"] == 0 and item["format"] == afgpu.FORMAT_QOA, item["message"]
        assert (item["frames"], item["channels"]) == (n, ch) == (want["pcm"].size // ch, want["channels"])
        want_f = want["pcm"].reshape(n, ch).astype(np.float32) * np.float32(1.0 / 32767)
        assert item["pcm"].shape == (n, ch) and (item["pcm"].view(np.uint32) == want_f.view(np.uint32)).all()
