"""The requantiser's tables and test inputs, on the CPU.  afgpu.mp3_qtables() -- what the device holds, and what
requant_numpy reads -- against tables derived from scalefactor-band widths alone (mp3_requant_model.tables_from_bands)
and against the float64 definition of |v|^(4/3); and the hand-made records of tests/mp3_requant_cases.py against the
coverage they are there for.

The 8 rate rows of each of the three kinds (long, short, mixed; table index = kind * 8 + row): row 0 MPEG-2.5 at 11025 and
12000 Hz, row 1 MPEG-2.5 at 8000 Hz, rows 2-4 MPEG-2 at 22050, 24000 and 16000 Hz, rows 5-7 MPEG-1 at 44100, 48000 and
32000 Hz (minimp3.d:134-137)."""
import numpy as np
import pytest

import afgpu
import mp3_requant_cases as cases
import mp3_requant_model as model

# max over a = 1 .. 8206 of |p(a) - a^(4/3)| / a^(4/3), p the model's float32 value (table below 129, L3_pow_43's
# polynomial above), measured from the model on the CPU: 1.3066459759812986e-06, at a = 1055 (just past the switch to the
# unshifted range at 1024, where frac is largest against the 64-step).  Below 129 alone: 7.56e-08.
POW43_MAX_REL = 1.3066459759812986e-06


@pytest.mark.parametrize("table", range(24))
def test_band_and_reorder_tables_follow_from_the_band_widths(table):
    want_bol, want_dst, short_start = model.tables_from_bands()
    bol, dst, _ = afgpu.mp3_qtables()
    assert np.array_equal(bol[table], want_bol[table])                   # every line
    assert np.array_equal(dst[table], want_dst[table])                   # the short part, and the identity before it
    s0 = int(short_start[table])
    assert s0 == (576 if table < 8 else 0 if table < 16 else 48 if table == model.REFUSED else 36)
    assert np.array_equal(dst[table][:s0], np.arange(s0))
    if table >= 8:
        assert sorted(dst[table][s0:]) == list(range(s0, 576))            # a permutation of the short part
        assert (dst[table][s0:] != np.arange(s0, 576)).any()


def test_pow43_table_is_the_float64_power_within_one_ulp():
    """g_pow43[16 + a], a = 0 .. 128 (the table has 145 entries: 128 is the last; 8206 >> 6), the reference's decimal
    literals: within one float32 ulp of a^(4/3) each; the 16 entries in front are their negatives."""
    p43 = afgpu.mp3_qtables()[2]
    a = np.arange(129)
    exact = model.pow43_64(a)
    got = p43[16 + a]
    ulp = np.spacing(np.maximum(np.abs(got), np.float32(1))).astype(np.float64)
    off = np.abs(got.astype(np.float64) - exact) / ulp
    not_nearest = a[got != exact.astype(np.float32)]
    print(f"pow43: {len(not_nearest)} of 129 entries are not the nearest float32 (a = {list(not_nearest)}), worst {off.max():.3f} ulp")
    assert got[0] == 0 and (off <= 1.0).all(), (a[off > 1.0], off.max())
    assert np.array_equal(p43[:16], -p43[16:32].astype(np.float32)) and not np.signbit(p43[16])


def test_model_power_stays_near_the_float64_power():
    a = np.arange(1, model.MAX_ABS + 1)
    exact = model.pow43_64(a)
    rel = np.abs(model.pow43_model(a).astype(np.float64) - exact) / exact
    print(f"pow43 model: max relative error {rel.max()!r} at a = {int(a[rel.argmax()])}")
    assert rel.max() <= 2 * POW43_MAX_REL, (rel.max(), int(a[rel.argmax()]))


@pytest.mark.parametrize("seed", [5, 6])
def test_hand_made_records_reach_every_class(seed):
    """a condition on the inputs: every arithmetic and addressing class of cases.CLASSES at least 16 times, each of the 23
    tables the parser emits in either channel's place, unequal tables with all four reorder-bit pairs"""
    q, gr, sd, coef_floats, mask = cases.hand_made(seed)
    counts = cases.branches(q, gr, sd)
    print(counts)
    assert set(counts) == set(cases.CLASSES)
    assert all(n >= 16 for n in counts.values()), {k: n for k, n in counts.items() if n < 16}
    assert int(np.abs(q.astype(np.int64)).max()) == model.MAX_ABS
    two = gr[gr["nch"] == 2]
    legal = set(range(24)) - {model.REFUSED}
    for c in (0, 1):
        assert set(int(t) & 31 for t in two["table"][:, c]) == legal
    assert (((gr["table"] & 0x80) != 0) == ((gr["table"] & 31) >= 8)).all() and ((gr["table"] & 0x60) == 0).all()
    differ = two[(two["table"][:, 0] & 31) != (two["table"][:, 1] & 31)]
    assert set((int(a) >> 7, int(b) >> 7) for a, b in differ["table"]) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set(int(s) for s in two["stereo"]) == {0, 1, 2} and (gr["stereo"][gr["nch"] != 2] == 0).all()
    assert ((gr["sdesc"] == cases.NO_SDESC) == (gr["stereo"] != 2)).all()
    used = sd[two["sdesc"][two["stereo"] == 2]]
    for kind in (0, 1, 2):
        assert (used["type"] == kind).all(axis=1).any()                  # a descriptor of this type throughout
    assert ((used["type"] != used["type"][:, :1]).any(axis=1)).any()     # and mixed ones
    s = gr["scale"][gr["nch"] > 0]
    assert s.min() == cases.SCALE_MIN and s.max() == cases.SCALE_MAX
    # layout: independent offsets, not in plane order, room between the blocks, unused slots and mono tails unwritten
    live = gr[gr["nch"] > 0]
    assert (np.diff(live["coef_off"].astype(np.int64)) < 0).any() and (np.diff(live["q_off"].astype(np.int64)) < 0).any()
    assert mask.size == coef_floats and not mask[:576].any() and not mask[-576:].any()
    for g in gr:
        end = int(g["coef_off"]) + 576 * int(g["nch"])
        assert not mask[end:end + 576].any() and not mask[int(g["coef_off"]) - 576:int(g["coef_off"])].any()
    want = cases.expected_hand_made(seed)                                # asserts that every product is zero or normal
    assert (want[mask] != cases.SENTINEL).all() and (want[~mask] == cases.SENTINEL).all()


def test_zero_lines_keep_their_sign_through_stereo_processing():
    """what the bit comparison on the device rests on: +0 +- +0 is +0 under mid/side, and a zero line times a negative
    intensity factor is -0"""
    q, gr, sd, coef_floats, mask = cases.hand_made(5)
    words = cases.expected_hand_made(5)[mask]
    assert (words == 0x80000000).any() and (words == 0).any()
